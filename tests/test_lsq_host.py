"""The shared least-squares header (scikit-downscale_amd/csrc/sd_lsq.h, compiled with g++ alone through tests/lsq_check.cpp)
against the exact rational reference of tests/_lsq_oracle.py.

minnorm_solve: F = 1..8 x designed rank 0..F x n in {r+1, r+2, F+1, 24} samples, scales 2^[-3,3] for every rank and 2^[-17,17]
for full rank and for rank deficiency through constant columns only (_lsq_oracle.host_cases).  The solver gets the exact centred
cross products rounded to float64; per case, with tol = K eps kappa max|y - mean(y)| (K measured on the LAPACK twin, see
_lsq_oracle.py):
  (a) the prediction at 16 queries outside the row space of the design,
  (b) the prediction at the training rows,
  (c) the component of the coefficients along every exact null vector, relative to |coef| (the Gram-Schmidt part),
  (d) the RMSE,
and a constant feature has coefficient exactly 0.0.  The errors themselves are evaluated in exact arithmetic.

chol_solve: SPD systems of n = 1..9 against the exact solution, and `false` for a zero, a negative and a NaN pivot.
"""
import math
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _lsq_oracle as lo  # noqa: E402


def hexrow(values):
    return " ".join(float(v).hex() for v in values)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("lsq") / "lsq_check"
    src = os.path.join(ROOT, "tests", "lsq_check.cpp")
    inc = os.path.join(ROOT, "scikit-downscale_amd", "csrc")
    res = subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", f"-I{inc}", src, "-o", str(exe)],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]

    def run(requests):
        """requests: lines for lsq_check -> one list of floats (or False) per request"""
        out = subprocess.run([str(exe)], input="\n".join(requests) + "\n", capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.splitlines()
        assert lines[-1] == "end" and len(lines) == len(requests) + 1
        return [False if ln == "false" else [float.fromhex(t) if "0x" in t else float(t) for t in ln.split()[1:]] for ln in lines[:-1]]

    return run


@pytest.fixture(scope="module")
def solved(driver):
    """every host case with the solver's coefficients for its [S | b], computed once"""
    cases = list(lo.host_cases())
    coefs = driver([f"minnorm {fit.F} " + hexrow(fit.system().ravel()) for _, _, _, fit, _, _ in cases])
    return [(name, X, y, fit, Q, wide, np.array(c)) for (name, X, y, fit, Q, wide), c in zip(cases, coefs)]


def test_case_set_is_complete(solved):
    seen = {(fit.F, fit.rank, fit.n, wide) for _, _, _, fit, _, wide, _ in solved}
    for F in range(1, 9):
        for r in range(F + 1):
            for n in {r + 1, r + 2, F + 1, 24}:
                assert (F, r, n, False) in seen
                if r == F:
                    assert (F, r, n, True) in seen
        assert any(fit.F == F and wide and 0 < fit.rank < F for _, _, _, fit, _, wide, _ in solved) or F == 1
    assert all(fit.kappa <= lo.KAPPA_MAX for _, _, _, fit, _, _, _ in solved)


@pytest.mark.parametrize("F", range(1, 9))
def test_minnorm_solve_against_the_exact_pseudo_inverse(solved, F):
    worst = 0.0
    for name, X, y, fit, Q, wide, coef in solved:
        if fit.F != F:
            continue
        const = [f for f in range(F) if fit.S[f][f] == 0]
        assert all(coef[f] == 0.0 for f in const), f"{name}: constant features {const} have coefficients {coef}"
        if fit.rank == 0:
            assert (coef == 0.0).all(), f"{name}: rank 0 but coefficients {coef}"
        ea, eb, ec, ed = fit.errors(coef, Q)
        tol, rel = fit.tol(), lo.K * lo.EPS * fit.kappa
        worst = max(worst, fit.ratio(coef, Q))
        assert ea <= tol, f"{name}: (a) prediction at the queries off by {ea:.3e} > {tol:.3e} (kappa {fit.kappa:.3g})"
        assert eb <= tol, f"{name}: (b) prediction at the training rows off by {eb:.3e} > {tol:.3e} (kappa {fit.kappa:.3g})"
        assert ec <= rel, f"{name}: (c) null-space component of the coefficients {ec:.3e} > {rel:.3e} (kappa {fit.kappa:.3g})"
        assert ed <= tol, f"{name}: (d) RMSE off by {ed:.3e} > {tol:.3e} (kappa {fit.kappa:.3g})"
    print(f"F={F}: largest error / (eps kappa) = {worst:.1f} (K = {lo.K:.0f})")


def test_the_eigenvalue_cut_keeps_a_resolvable_direction(driver):
    """Nearly collinear full-rank designs (_lsq_oracle.close_cases): the smallest eigenvalue of the correlation matrix lies between
    the cut (1e-12) and 2.5e-7 of the largest, so the direction has to be kept.  (b) and (d) only, see make_close_case."""
    cases = list(lo.close_cases())
    assert len(cases) == 14 and all(4e6 <= fit.kappa <= 1e10 and fit.rank == fit.F for _, _, _, fit in cases)
    coefs = driver([f"minnorm {fit.F} " + hexrow(fit.system().ravel()) for _, _, _, fit in cases])
    for (name, X, y, fit), coef in zip(cases, coefs):
        _, eb, _, ed = fit.errors(coef, [])
        sysm = fit.system()
        _, tb, _, td = fit.errors(lo.twin_solve(sysm[:, :-1], sysm[:, -1]), [])
        unit = lo.EPS * fit.kappa * fit.yscale
        print(f"{name}: kappa {fit.kappa:.3g}, error / (eps kappa): solver {max(eb, ed) / unit:.1f}, twin {max(tb, td) / unit:.1f}")
        assert eb <= fit.tol(), f"{name}: (b) prediction at the training rows off by {eb:.3e} > {fit.tol():.3e} (kappa {fit.kappa:.3g})"
        assert ed <= fit.tol(), f"{name}: (d) RMSE off by {ed:.3e} > {fit.tol():.3e} (kappa {fit.kappa:.3g})"


def test_twin_constant_is_the_recorded_one(solved):
    """K comes from the LAPACK twin over this very case set: the recorded constant may not be below what the twin gives now"""
    top = max(v[0] for v in lo.measure_twin(c[:6] for c in solved).values())
    assert top <= lo.TWIN_MAX_RATIO * 1.000001 and lo.K == 8 * lo.TWIN_MAX_RATIO, (top, lo.TWIN_MAX_RATIO)


def shifted_sums(X, y, x0, y0):
    """the one-pass sums of linreg_fit_kernel / grouped_window_kernel in their order: data shifted by (x0, y0), summed in sample
    order, centred as sum - n mean mean -> ([S | b], raw sums of squares), plain float64 arithmetic"""
    n, F = X.shape
    sx, sy, sxx, sxy = [0.0] * F, 0.0, [[0.0] * F for _ in range(F)], [0.0] * F
    for i in range(n):
        d = [float(X[i, f]) - float(x0[f]) for f in range(F)]
        e = float(y[i]) - float(y0)
        sy += e
        for f in range(F):
            sx[f] += d[f]
            sxy[f] += d[f] * e
            for g in range(f, F):
                sxx[f][g] += d[f] * d[g]
    dm, em = [v / n for v in sx], sy / n
    A = np.zeros((F, F + 1))
    for f in range(F):
        A[f, F] = sxy[f] - n * dm[f] * em
        for g in range(f, F):
            A[f, g] = A[g, f] = sxx[f][g] - n * dm[f] * dm[g]
    return A, [sxx[f][f] for f in range(F)]


def test_a_feature_constant_at_a_decimal_value_is_cleared(driver):
    """One-pass shifted sums leave S_ff of a constant feature at rounding level, positive about one time in three when the value is
    no dyadic number; equilibrated, such a row would act as a feature of its own.  clear_unresolved zeroes the row, the column
    and the right-hand side, leaves every other entry alone, and the solve then matches the exact fit (constant feature: 0.0)."""
    rng = np.random.default_rng(11)
    positive = 0
    requests, cases = [], []
    for trial in range(60):
        n, F = int(rng.integers(2, 40)), int(rng.integers(2, 6))
        X = np.round(rng.standard_normal((n, F)), 1)
        y = np.round(rng.standard_normal(n), 1)
        x0 = np.round(rng.standard_normal(F), 1)       # the shift: the first sample of the series, outside this group
        X[:, 1] = np.round(rng.standard_normal(), 1)   # constant over the group, different from the shift
        fit = lo.ExactFit(X, y)
        if not fit.kappa <= lo.KAPPA_MAX or fit.S[0][0] == 0:
            continue
        A, raw = shifted_sums(X, y, x0, 0.0)
        positive += A[1, 1] > 0
        requests.append(f"unresolved {F} {n} " + hexrow(A.ravel()) + " " + hexrow(raw))
        cases.append((fit, A))
    assert positive >= 5, "the case set no longer holds a constant feature with a positive rounded S_ff"
    cleared = driver(requests)
    coefs = driver([f"minnorm {fit.F} " + hexrow(c) for (fit, _), c in zip(cases, cleared)])
    for (fit, A), c, coef in zip(cases, cleared, coefs):
        B = np.array(c).reshape(fit.F, fit.F + 1)
        keep = np.ones_like(A, dtype=bool)
        keep[1, :], keep[:, 1] = False, False
        assert (B[1, :] == 0.0).all() and (B[:, 1] == 0.0).all() and np.array_equal(B[keep], A[keep])
        assert coef[1] == 0.0
        ea, eb, _, ed = fit.errors(coef, [])
        assert max(eb, ed) <= fit.tol(), (fit.n, fit.F, eb, ed, fit.tol(), fit.kappa)
    nan = float("nan")
    kept = driver(["unresolved 2 5 " + hexrow([nan, nan, nan, nan, nan, nan]) + " " + hexrow([nan, nan]),
                   "unresolved 2 5 " + hexrow([1e-9, 0.0, 0.5, 0.0, 2.0, 1.0]) + " " + hexrow([1.0, 2.0])])
    assert all(v != v for v in kept[0]), "a NaN system stays NaN (the caller flags the cell)"
    assert kept[1] == [1e-9, 0.0, 0.5, 0.0, 2.0, 1.0], "a small but resolved variance (1e-9 of the raw sum) is kept"


def spd_system(rng, n):
    """H = M^T M + I from small integers (exact in float64) with cond_2(H) <= 1e4, an integer right-hand side"""
    while True:
        M = rng.integers(-3, 4, (n + 2, n)).astype(float)
        H = M.T @ M + np.eye(n)
        lam = np.linalg.eigvalsh(H)
        if lam[-1] / lam[0] <= 1e4:
            return H, rng.integers(-9, 10, n).astype(float), float(lam[-1] / lam[0])


@pytest.mark.parametrize("n", range(1, 10))
def test_chol_solve_against_the_exact_solution(driver, n):
    """Bound: the computed solution solves (H + dH) d = r with |dH| <= gamma_{3n+1} |L||L^T| (Higham, Accuracy and Stability of
    Numerical Algorithms, theorem 10.4) and || |L||L^T| ||_2 <= n ||H||_2, hence |d - d*|_2 <= n (3n + 1) eps cond_2(H) |d*|_2."""
    rng = np.random.default_rng(100 + n)
    systems = [spd_system(rng, n) for _ in range(8)]
    got = driver([f"chol {n} " + hexrow(H.ravel()) + " " + hexrow(r) for H, r, _ in systems])
    for (H, r, cond), d in zip(systems, got):
        assert d is not False, "chol_solve refused a positive definite system"
        exact = lo._solve([[Fraction(v) for v in row] for row in H], [Fraction(v) for v in r])
        err = math.sqrt(float(sum((Fraction(a) - b) ** 2 for a, b in zip(d, exact))))
        ref = math.sqrt(float(sum(b * b for b in exact)))
        assert err <= n * (3 * n + 1) * lo.EPS * cond * ref, (n, err, cond, ref)


def test_chol_solve_refuses_a_bad_pivot(driver):
    nan = float("nan")
    bad = {
        "zero first pivot": [[0.0]],
        "zero later pivot": [[1.0, 1.0, 0.0], [1.0, 1.0, 0.0], [0.0, 0.0, 1.0]],  # 1 - 1 * 1 == 0 exactly
        "negative first pivot": [[-1.0, 0.0], [0.0, 1.0]],
        "negative later pivot": [[1.0, 2.0], [2.0, 1.0]],                          # 1 - 2 * 2 < 0
        "NaN first pivot": [[nan, 0.0], [0.0, 1.0]],
        "NaN later pivot": [[1.0, 0.0], [0.0, nan]],
        "NaN off the diagonal": [[1.0, nan], [nan, 1.0]],
    }
    got = driver([f"chol {len(H)} " + hexrow(np.array(H).ravel()) + " " + hexrow([1.0] * len(H)) for H in bad.values()])
    for name, d in zip(bad, got):
        assert d is False, f"{name}: chol_solve returned {d}"
    ok = driver(["chol 2 " + hexrow([4.0, 2.0, 2.0, 5.0]) + " " + hexrow([2.0, 5.0])])[0]  # d = (0, 1)
    assert ok == [0.0, 1.0]


def test_softplus_and_sigmoid_do_not_overflow(driver):
    zs = [-800.0, -40.0, -1.5, 0.0, 0.75, 40.0, 800.0]
    got = driver([f"helpers {float(z).hex()}" for z in zs])
    for z, (sp, sg) in zip(zs, got):
        assert math.isfinite(sp) and math.isfinite(sg), (z, sp, sg)
        assert 0.0 <= sg <= 1.0 and sp >= 0.0
        if abs(z) <= 40:
            assert abs(sp - math.log1p(math.exp(z))) <= 4 * lo.EPS * max(1.0, sp)
            assert abs(sg - 1.0 / (1.0 + math.exp(-z))) <= 4 * lo.EPS
    assert got[0] == [0.0, 0.0] and got[-1] == [800.0, 1.0]
