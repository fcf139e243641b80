"""CPU: the C-ABI library loads and exports every symbol include/sd_downscale.h declares (no compute calls)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sd_downscale.h")


def declared_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sd_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_the_boundary():
    names = declared_functions()
    for required in ("sd_bcsd_fit", "sd_bcsd_predict", "sd_bcsd_fit_predict_dev", "sd_analog_fit", "sd_analog_predict",
                     "sd_analogreg_predict", "sd_ctx_create", "sd_last_error"):
        assert required in names


def test_library_exports_every_declared_symbol():
    from skdownscale_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libsd_downscale.so not built yet (python __graft_entry__.py)")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    missing = [n for n in declared_functions() if not hasattr(lib, n)]
    assert not missing, f"symbols declared in the header but not exported: {missing}"
    assert lib.sd_version() >= 100
    # the ctypes signature table covers the whole header (sd_last_error is bound separately)
    assert sorted(set(_lib.SIGNATURES) | {"sd_last_error"}) == declared_functions()


def test_missing_library_fails_loudly(monkeypatch):
    from skdownscale_amd import _lib

    monkeypatch.setattr(_lib, "_libs", {})
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libsd_downscale.so")
    with pytest.raises(_lib.EngineError, match="no CPU fallback"):
        _lib.load()


def test_no_gpu_is_an_error_not_a_fallback():
    from skdownscale_amd import _lib
    from skdownscale_amd.engine import Context

    if not os.path.exists(_lib.LIB_PATH) or os.path.exists("/dev/kfd"):
        pytest.skip("needs the built library and no GPU")
    with pytest.raises((_lib.EngineError, ValueError)):
        Context(0)


def test_cell_status_codes_agree():
    """the per-cell codes of the header, their Python names, and both directions of the fold in csrc/sd_internal.h"""
    from skdownscale_amd import _lib

    codes = dict(re.findall(r"#define SD_CELL_([A-Z_]+) (\d+)", open(HEADER).read()))
    assert {k: int(v) for k, v in codes.items()} == {"OK": 0, "MASKED": 1, "NONFINITE": 2, "BAD_CLIMO": 3, "ONE_CLASS": 4, "EMPTY_RANGE": 5}
    for name, code in codes.items():
        assert getattr(_lib, "CELL_" + name) == int(code)
    internal = open(os.path.join(ROOT, "scikit-downscale_amd", "csrc", "sd_internal.h")).read()
    bits = {k: int(v) for k, v in re.findall(r"#define SDI_([A-Z_]+) (\d+)", internal)}
    assert sorted(bits.values()) == [1, 2, 4, 8, 16] and set(bits) == set(codes) - {"OK"}
    for name in bits:  # bits -> code (sd_public_status) and code -> bits (sd_internal_status)
        assert re.search(rf"if \(bits & SDI_{name}\) return SD_CELL_{name};", internal)
        assert re.search(rf"case SD_CELL_{name}: return SDI_{name};", internal)
    order = re.findall(r"if \(bits & SDI_([A-Z_]+)\) return", internal)
    assert order[:2] == ["MASKED", "NONFINITE"]  # the reference skips a masked cell before it validates it
