"""Exact reference for the shared least-squares solver (scikit-downscale_amd/csrc/sd_lsq.h).

A float64 design X [n, F] and target y [n] are taken as exact rationals (``fractions.Fraction``): the data are centred, the
centred design is reduced by exact elimination to a rank factorisation Xc = C R (C: the pivot columns [n, r], R: the non-zero
rows of the reduced echelon form [r, F]) and the minimum-norm least-squares coefficients are

    coef = R^T (R R^T)^-1 (C^T C)^-1 C^T yc                   (the Moore-Penrose solution pinv(Xc) yc),

which is what sklearn's LinearRegression (lstsq on the centred data) and sdlsq::minnorm_solve aim at.  The elimination also gives
the exact rank r and an exact basis of the null space of Xc.

The solver works on the equilibrated normal equations, so its error grows with the condition number of the correlation matrix on
its range, kappa = lam_1 / lam_r.  Every comparison against this reference therefore uses the per-case tolerance

    tol = K * 2^-52 * kappa * max|y - mean(y)|

K is not fitted to the code under test: it is measured on ``twin_solve``, the float64 LAPACK restatement of the same method
(equilibrate, numpy.linalg.eigh, eigenvalue cut at 1e-12, projection off the scaled null vectors), over the whole host case set
of tests/test_lsq_host.py, and multiplied by 8 for the difference in constants between cyclic Jacobi and LAPACK.

    python tests/_lsq_oracle.py        # prints the twin's largest error / (eps * kappa) per sweep and the K that follows
"""
from fractions import Fraction
import math

import numpy as np

EPS = 2.0 ** -52
KAPPA_MAX = 1e4
# measured by `python tests/_lsq_oracle.py` (see the module docstring and profiles/lsq/README.md): the twin's largest
# error / (eps * kappa) was 293.0 on the 2^[-3,3] sweep (F7-r2-n4-near-mix) and 39.6 on the 2^[-17,17] sweep
TWIN_MAX_RATIO = 293.0
K = 8 * TWIN_MAX_RATIO


def _fr(v):
    return Fraction(float(v))


def _solve(M, B):
    """exact Gauss-Jordan: M [r][r] non-singular, B [r] -> M^-1 B"""
    r = len(M)
    A = [list(M[i]) + [B[i]] for i in range(r)]
    for c in range(r):
        p = next(i for i in range(c, r) if A[i][c] != 0)
        A[c], A[p] = A[p], A[c]
        inv = 1 / A[c][c]
        A[c] = [v * inv for v in A[c]]
        for i in range(r):
            if i != c and A[i][c] != 0:
                m = A[i][c]
                A[i] = [a - m * b for a, b in zip(A[i], A[c])]
    return [A[i][r] for i in range(r)]


class ExactFit:
    """Exact centred minimum-norm least squares of y on X.  Attributes: n, F, X (the float64 design), rank, xm, ym, coef, intercept (Fractions), null (exact
    basis of the null space of the centred design, F - rank vectors), S, b (exact centred cross products), rmse, yscale =
    max|y - mean(y)|, kappa (floats)."""

    def __init__(self, X, y):
        X = np.asarray(X, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64)
        n, F = X.shape
        self.n, self.F, self.X = n, F, X
        Xe = [[_fr(v) for v in row] for row in X]
        ye = [_fr(v) for v in y]
        self.xm = [sum(Xe[i][f] for i in range(n)) / n for f in range(F)]
        self.ym = sum(ye) / n
        Xc = [[Xe[i][f] - self.xm[f] for f in range(F)] for i in range(n)]
        yc = [v - self.ym for v in ye]
        self.Xc, self.yc = Xc, yc
        # reduced row echelon form of Xc: rank, pivot columns, R
        A = [list(row) for row in Xc]
        piv = []
        row = 0
        for c in range(F):
            p = next((i for i in range(row, n) if A[i][c] != 0), None)
            if p is None:
                continue
            A[row], A[p] = A[p], A[row]
            inv = 1 / A[row][c]
            A[row] = [v * inv for v in A[row]]
            for i in range(n):
                if i != row and A[i][c] != 0:
                    m = A[i][c]
                    A[i] = [a - m * b for a, b in zip(A[i], A[row])]
            piv.append(c)
            row += 1
            if row == n:
                break
        r = len(piv)
        self.rank, self.pivots = r, piv
        R = [A[i] for i in range(r)]
        if r:
            Cm = [[Xc[i][c] for c in piv] for i in range(n)]
            CtC = [[sum(Cm[i][a] * Cm[i][b] for i in range(n)) for b in range(r)] for a in range(r)]
            Cty = [sum(Cm[i][a] * yc[i] for i in range(n)) for a in range(r)]
            w = _solve(CtC, Cty)
            RRt = [[sum(R[a][f] * R[b][f] for f in range(F)) for b in range(r)] for a in range(r)]
            v = _solve(RRt, w)
            self.coef = [sum(R[a][f] * v[a] for a in range(r)) for f in range(F)]
        else:
            self.coef = [Fraction(0)] * F
        self.null = []
        for j in range(F):
            if j in piv:
                continue
            vec = [Fraction(0)] * F
            vec[j] = Fraction(1)
            for a, c in enumerate(piv):
                vec[c] = -R[a][j]
            self.null.append(vec)
        self.intercept = self.ym - sum(m * c for m, c in zip(self.xm, self.coef))
        res = [yc[i] - sum(Xc[i][f] * self.coef[f] for f in range(F)) for i in range(n)]
        self.rmse = math.sqrt(float(sum(v * v for v in res) / n))
        self.yscale = float(max(abs(v) for v in yc))
        cols = [[Xc[i][f] for i in range(n)] for f in range(F)]
        self.S = [[None] * F for _ in range(F)]
        for f in range(F):
            for g in range(f, F):
                self.S[f][g] = self.S[g][f] = sum(a * b for a, b in zip(cols[f], cols[g]))
        self.kappa = self._kappa()

    @property
    def b(self):
        return [sum(self.Xc[i][f] * self.yc[i] for i in range(self.n)) for f in range(self.F)]

    def _kappa(self):
        """lam_1 / lam_r of the exact equilibrated correlation matrix, rounded to float64 (numpy.linalg.eigvalsh)"""
        F, r = self.F, self.rank
        if r == 0:
            return 1.0
        Rm = np.zeros((F, F))
        for f in range(F):
            for g in range(F):
                if self.S[f][f] > 0 and self.S[g][g] > 0:
                    Rm[f, g] = 1.0 if f == g else float(self.S[f][g]) / math.sqrt(float(self.S[f][f] * self.S[g][g]))
        lam = np.sort(np.linalg.eigvalsh(Rm))[::-1][:r]
        return float(lam[0] / lam[-1]) if lam[-1] > 0 else math.inf

    # ---- floats for the comparisons ----
    def coef_f(self):
        return np.array([float(c) for c in self.coef])

    def system(self):
        """[S | b] rounded to float64, as the kernels hand it to the solver"""
        b = self.b
        return np.array([[float(v) for v in self.S[f]] + [float(b[f])] for f in range(self.F)])

    def predict(self, Q):
        """exact predictions at the rows of Q, rounded to float64"""
        return np.array([float(self.intercept + sum(_fr(q[f]) * self.coef[f] for f in range(self.F))) for q in np.atleast_2d(Q)])

    def tol(self, k=None):
        return (K if k is None else k) * EPS * self.kappa * self.yscale

    # ---- exact error measures of a float64 coefficient vector (the four assertions of the host test) ----
    def errors(self, coef, Q):
        """(a) max |(q - xm) . (coef - exact)| over the queries, (b) the same over the training rows, (c) max over the null basis of
        |n . coef| / (|n| |coef|), (d) |rmse(coef) - rmse|; (a), (b), (d) in the units of y, all evaluated in exact arithmetic"""
        dc = [_fr(c) - e for c, e in zip(coef, self.coef)]
        ea = max((abs(sum((_fr(q[f]) - self.xm[f]) * dc[f] for f in range(self.F))) for q in Q), default=Fraction(0))
        eb = max(abs(sum(self.Xc[i][f] * dc[f] for f in range(self.F))) for i in range(self.n))
        cf = [_fr(c) for c in coef]
        cn = math.sqrt(float(sum(c * c for c in cf)))
        ec = 0.0
        for vec in self.null:
            dot = abs(float(sum(a * c for a, c in zip(vec, cf))))
            if dot > 0.0:
                ec = max(ec, dot / (math.sqrt(float(sum(a * a for a in vec))) * cn))
        res = [self.yc[i] - sum(self.Xc[i][f] * cf[f] for f in range(self.F)) for i in range(self.n)]
        ed = abs(math.sqrt(float(sum(v * v for v in res) / self.n)) - self.rmse)
        return float(ea), float(eb), ec, ed

    def ratio(self, coef, Q):
        """the largest of the four errors in units of eps * kappa (* yscale for those in the units of y)"""
        ea, eb, ec, ed = self.errors(coef, Q)
        unit = EPS * self.kappa
        if self.yscale == 0.0:
            return 0.0 if max(ea, eb, ed) == 0.0 and ec == 0.0 else math.inf
        return max(ea / self.yscale, eb / self.yscale, ed / self.yscale, ec) / unit


def twin_solve(S, b):
    """The method of sdlsq::minnorm_solve on LAPACK in float64: the reference K is measured on.  Constant features (zero
    diagonal) are taken out before the decomposition and get coefficient 0: the Jacobi rotations never touch their exactly
    zero rows, LAPACK would smear rounding noise over them."""
    S = np.asarray(S, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    out = np.zeros(len(b))
    live = np.nonzero(np.diag(S) > 0)[0]
    if not len(live):
        return out
    sc = 1.0 / np.sqrt(np.diag(S)[live])
    Rm = S[np.ix_(live, live)] * np.outer(sc, sc)
    np.fill_diagonal(Rm, 1.0)
    lam, V = np.linalg.eigh(Rm)
    keep = lam > 1e-12 * lam.max()
    coef = (V[:, keep] @ ((V[:, keep].T @ (b[live] * sc)) / lam[keep])) * sc
    if not keep.all():  # minimum norm in the original coordinates: project off the scaled null vectors
        Q, _ = np.linalg.qr(V[:, ~keep] * sc[:, None])
        coef = coef - Q @ (Q.T @ coef)
    out[live] = coef
    return out


def make_case(rng, n, F, r, span, n_const=0, dup=False, kmax=KAPPA_MAX, attempts=50, units=None):
    """A design of exact rank r: X = (Z B) diag(s) + o s with small-integer Z [n, r], B [r, F], power-of-two scales s in
    2^[-span, span] and integer offsets o, so every entry is exact in float64 and the centred float64 design has rank r.
    ``n_const`` columns are constant (B column zero), ``dup`` makes the last column a copy of the first in other units.
    ``units`` = (s, o) fixes the scales and offsets (designs that are later stacked share them).  Rejection-samples to
    kappa <= kmax; returns (X, y, ExactFit)."""
    assert 0 <= r <= min(F, n - 1)
    for _ in range(attempts):
        s, o = (2.0 ** rng.integers(-span, span + 1, F), rng.integers(-5, 6, F).astype(float)) if units is None else units
        y = rng.integers(-9, 10, n).astype(float)
        if n > 1 and np.ptp(y) == 0:
            continue
        if r == 0:
            X = np.tile(o * s, (n, 1))
        else:
            Z = rng.integers(-4, 5, (n, r)).astype(float)
            B = rng.integers(-2, 3, (r, F)).astype(float)
            const = rng.choice(F, n_const, replace=False) if n_const else []
            B[:, const] = 0.0
            if dup and F > 1:
                B[:, F - 1] = B[:, 0]
            M = Z @ B
            Mc = n * M - M.sum(axis=0)  # integers: the rank of the centred design, screened in floats before the exact pass
            if np.linalg.matrix_rank(Mc) != r:
                continue
            if n_const and ((np.abs(Mc).sum(axis=0) == 0).sum() != n_const or r != F - n_const):
                continue
            X = M * s + o * s
        fit = ExactFit(X, y)
        if fit.rank != r or not fit.kappa <= kmax:
            continue
        return X, y, fit
    raise RuntimeError(f"no design of rank {r} with kappa <= {kmax:g} in {attempts} attempts (n={n}, F={F})")


def make_close_case(rng, n, F, span=3, attempts=50):
    """A full-rank design whose last column is the first plus 2^-12 times small integers: the smallest eigenvalue of the
    correlation matrix lies between 1e-10 and 2.5e-7 of the largest, well inside what the solver's cut at 1e-12 must keep.  The
    tolerance grows with kappa like everywhere else; a cut that drops the direction is wrong by the order of the target.  Only
    the training rows and the RMSE are compared: along the weak direction v the rows have x . v ~ sqrt(lam_r) while a query off
    the rows has q . v ~ 1, so its prediction carries the error of the coefficients sqrt(kappa) times larger, which is
    extrapolation and not the solver (the twin's error at such queries is ~3e4 eps kappa).  These cases are not part of the set
    K is measured on."""
    for _ in range(attempts):
        s = 2.0 ** rng.integers(-span, span + 1, F)
        o = rng.integers(-5, 6, F).astype(float)
        y = rng.integers(-9, 10, n).astype(float)
        Z = rng.integers(-4, 5, (n, F)).astype(float)
        Z[:, F - 1] = Z[:, 0] + 2.0 ** -12 * rng.integers(-4, 5, n)
        fit = ExactFit(Z * s + o * s, y)
        if np.ptp(y) > 0 and fit.rank == F and 4e6 <= fit.kappa <= 1e10:
            return Z * s + o * s, y, fit
    raise RuntimeError(f"no nearly collinear design in {attempts} attempts (n={n}, F={F})")


def make_queries(rng, X, count=16):
    """queries with |q - mean(x)| <= 2 max|x - mean(x)| per feature; real-valued offsets, so not in the row space of the design"""
    xm = X.mean(axis=0)
    half = 2.0 * np.abs(X - xm).max(axis=0)
    return xm + rng.uniform(-1.0, 1.0, (count, X.shape[1])) * half


def host_cases(seed=0):
    """The host case set: F = 1..8 x rank 0..F x n in {r+1, r+2, F+1, 24} x {scales 2^[-3,3] for every rank; scales 2^[-17,17] for
    full rank and for rank deficiency through constant columns only}, all with kappa <= 1e4.  Yields (name, X, y, fit, Q, wide)."""
    rng = np.random.default_rng(seed)
    for F in range(1, 9):
        for r in range(0, F + 1):
            for n in sorted({r + 1, r + 2, F + 1, 24}):
                if n < r + 1:
                    continue
                for wide in (False, True):
                    for variant in ("mix", "const", "dup"):
                        n_const = 0
                        if r == 0:
                            if variant != "mix":
                                continue
                        elif variant == "const":
                            if r == F:
                                continue
                            n_const = F - r
                        elif variant == "dup":
                            if r == F or wide or F < 2:
                                continue
                        elif wide and r < F:
                            continue  # mixed scales with a null space that is not axis-aligned: a stated limit, not asserted
                        X, y, fit = make_case(rng, n, F, r, 17 if wide else 3, n_const=n_const, dup=variant == "dup")
                        yield f"F{F}-r{r}-n{n}-{'wide' if wide else 'near'}-{variant}", X, y, fit, make_queries(rng, X), wide


def close_cases(seed=1):
    """two nearly collinear full-rank designs per F = 2..8 (n = F + 1 and 24): (name, X, y, fit)"""
    rng = np.random.default_rng(seed)
    for F in range(2, 9):
        for n in (F + 1, 24):
            X, y, fit = make_close_case(rng, n, F)
            yield f"F{F}-r{F}-n{n}-close", X, y, fit


def measure_twin(cases=None):
    worst = {}
    for name, X, y, fit, Q, wide in host_cases() if cases is None else cases:
        sysm = fit.system()
        ratio = fit.ratio(twin_solve(sysm[:, :-1], sysm[:, -1]), Q)
        key = "2^[-17,17]" if wide else "2^[-3,3]"
        if ratio > worst.get(key, (0.0, ""))[0]:
            worst[key] = (ratio, name)
    return worst


if __name__ == "__main__":
    worst = measure_twin()
    for key, (ratio, name) in sorted(worst.items()):
        print(f"twin, scales {key}: largest error / (eps * kappa) = {ratio:.1f} ({name})")
    top = max(v[0] for v in worst.values())
    print(f"TWIN_MAX_RATIO = {top:.1f}, K = 8 * TWIN_MAX_RATIO = {8 * top:.1f}")
