"""Reference and data regimes for the fit error (RMSE of the fit) and the predictions of the one-pass regression kernels where their
sums cancel: linreg_fit_kernel, grouped_window_kernel, analog_regression and the one-feature forms of analog_f1_mean_kernel.

Every one of those kernels takes its centred sums in one pass over data shifted by the first sample of the cell (or window), and
three of them take the residual sum of squares from those sums as well (rss = Syy - coef . Sxy).  Both lose digits when the fit is
nearly exact (rss << Syy) and when the first sample lies far from the rest (the shifted sums grow, the centred ones do not).
``regime`` builds one cell of either kind; ``RefFit`` is the centred least-squares fit in extended precision:

    long double (64-bit significand, eps 1.1e-19) where numpy has one: float64 lstsq on the centred data as the start, three steps
    of refinement on the normal equations with residuals and cross products in long double, residuals summed in long double;
    ``fractions`` (tests/_lsq_oracle.py:ExactFit) elsewhere.

ExactFit takes seconds per cell at the workload's length, so it is the judge of RefFit (tests/test_fit_error_host.py) and not the
reference of a GPU test itself, except for the short windows of the analog and grouped kernels."""
import math

import numpy as np

import _lsq_oracle as lo

EPS = lo.EPS
LONG = np.longdouble
HAVE_LONG = bool(np.finfo(LONG).eps < 2e-19)

RATIOS = (1e-2, 1e-4, 1e-6, 1e-8, 3e-9, 1e-10, 0.0)  # noise variance / signal variance
SHIFTS = (0, 10, 100, 1000)                          # first sample: sigma away in X
OFFSETS = (0.0, 280.0)
RHOS = (0.0, 0.9999)
SIGMA = 10.0


def regime(rng, T, F, ratio, shift, offset, rho, on_line):
    """One cell: features of standard deviation 10 around ``offset`` (feature 1 correlated ``rho`` with feature 0), y = X . 1 + 2 +
    noise of variance ``ratio`` times the variance of the signal; the first sample moved ``shift`` sigma away in every feature,
    with its y (on_line: a leverage point) or without (an outlier).  -> X [T, F], y [T]"""
    Z = rng.standard_normal((T, F))
    if F >= 2:
        Z[:, 1] = rho * Z[:, 0] + math.sqrt(1.0 - rho * rho) * Z[:, 1]
    noise = rng.standard_normal(T)  # (drawn whatever the ratio: the same seed gives the same design at every ratio)
    X = offset + SIGMA * Z
    signal = X.sum(axis=1) + 2.0
    y = signal + math.sqrt(ratio * float(np.var(signal))) * noise
    if shift:
        X[0] += shift * SIGMA
        if on_line:
            y[0] += F * shift * SIGMA
    return X, y


def regimes(F):
    """the product of the ladders above: (ratio, shift, offset, rho); one feature has no correlation to vary"""
    return [(ratio, shift, offset, rho) for ratio in RATIOS for shift in SHIFTS for offset in OFFSETS for rho in (RHOS if F >= 2 else RHOS[:1])]


class RefFit:
    """Centred least squares of y on X (full column rank) in extended precision.  coef [F], intercept, rmse as float64; predict(Q)."""

    def __init__(self, X, y):
        X = np.asarray(X, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64)
        self.n, self.F = X.shape
        self._long = HAVE_LONG
        if self._long:
            Xl, yl = X.astype(LONG), y.astype(LONG)
            xm, ym = Xl.mean(axis=0), yl.mean()
            Xc, yc = Xl - xm, yl - ym
            Xd = Xc.astype(np.float64)
            sc = np.sqrt((Xd * Xd).sum(axis=0))
            sc[sc == 0] = 1.0
            Xs = Xd / sc
            G = Xs.T @ Xs
            coef = (np.linalg.lstsq(Xs, yc.astype(np.float64), rcond=None)[0] / sc).astype(LONG)
            # each step gains ~ -log10(kappa eps64) digits: kappa is 2e4 for rho = 0.9999 and reaches ~1e9 where a far leverage
            # point makes a short series collinear (the host test pins such a cell to ExactFit), so three steps converge
            for _ in range(3):
                r = yc - Xc @ coef
                g = (Xc * r[:, None]).sum(axis=0)
                coef = coef + (np.linalg.solve(G, (g / sc).astype(np.float64)) / sc).astype(LONG)
            res = yc - Xc @ coef
            self._coef, self._icpt = coef, ym - (xm * coef).sum()
            self.rmse = float(np.sqrt((res * res).sum() / self.n))
            self.coef = coef.astype(np.float64)
            self.intercept = float(self._icpt)
        else:
            fit = lo.ExactFit(X, y)
            self._exact = fit
            self.rmse, self.coef, self.intercept = fit.rmse, fit.coef_f(), float(fit.intercept)

    def predict(self, Q):
        Q = np.atleast_2d(np.asarray(Q, dtype=np.float64))
        if self._long:
            return (self._icpt + Q.astype(LONG) @ self._coef).astype(np.float64)
        return self._exact.predict(Q)

    def eval_slack(self, Q):
        """rounding of icpt + q . coef evaluated in float64 with the exact coefficients, per row of Q (tests/test_gpu_lsq.py)"""
        return (self.F + 2) * EPS * (abs(self.intercept) + np.abs(np.atleast_2d(Q)) @ np.abs(self.coef))


def exact_eval_slack(fit, Q):
    """the same for an ExactFit"""
    return (fit.F + 2) * EPS * (abs(float(fit.intercept)) + np.abs(np.atleast_2d(Q)) @ np.abs(fit.coef_f()))


def fit_error_tol(exact, slack):
    """|got - exact| <= 1e-6 exact + slack: the project's contract plus the rounding of one residual evaluated in float64"""
    return 1e-6 * exact + slack


def queries_inside(rng, X, count=16):
    """queries inside the range of the samples after the first (the shifted one)"""
    lo_, hi = X[1:].min(axis=0), X[1:].max(axis=0)
    return lo_ + rng.random((count, X.shape[1])) * (hi - lo_)


class ExactLine:
    """ExactFit for one feature, from integer sums (every float64 is an integer over a power of two): what the one-feature analog
    tests need per query, at a hundredth of the cost.  With one feature rss = Syy - Sxy^2 / Sxx holds exactly in rationals; a window
    of equal x has slope 0 (the minimum-norm solution).  slope, intercept (Fractions), rmse (float); the host test pins it to ExactFit."""

    F = 1

    def __init__(self, x, y):
        from fractions import Fraction

        xf, yf = [Fraction(float(v)) for v in x], [Fraction(float(v)) for v in y]
        D, E = max(v.denominator for v in xf), max(v.denominator for v in yf)
        xi, yi = [v.numerator * (D // v.denominator) for v in xf], [v.numerator * (E // v.denominator) for v in yf]
        n = len(xi)
        sx, sy = sum(xi), sum(yi)
        cxx = n * sum(a * a for a in xi) - sx * sx          # n D^2 Sxx
        cxy = n * sum(a * b for a, b in zip(xi, yi)) - sx * sy  # n D E Sxy
        cyy = n * sum(b * b for b in yi) - sy * sy          # n E^2 Syy
        self.n = n
        self.slope = Fraction(cxy * D, cxx * E) if cxx else Fraction(0)
        self.intercept = Fraction(sy, n * E) - self.slope * Fraction(sx, n * D)
        rss = (Fraction(cyy) - (Fraction(cxy * cxy, cxx) if cxx else 0)) / (n * E * E)
        self.rmse = math.sqrt(float(rss / n))

    def predict(self, q):
        from fractions import Fraction

        return np.array([float(self.intercept + self.slope * Fraction(float(v))) for v in np.ravel(q)])

    def eval_slack(self, q):
        return 3 * EPS * (abs(float(self.intercept)) + np.abs(np.ravel(q)) * abs(float(self.slope)))


# --- data of the analog_regression test (F = 3, k = 40, T = 2000), shared with the host test that asserts its 5 % cap ---------
EPI_T, EPI_F, EPI_K, EPI_TQ, EPI_CAP = 2000, 3, 40, 60, 0.05
EPI_RATIOS = RATIOS


def epilogue_cells(seed=9100):
    """-> X [T, 3, C], y [T, C], Xq [Tq, 3, C]: independent features of sigma 10 around 280, y = X . 1 + 2 + noise along the ratio
    ladder; the last cell (ratio 1e-6) holds a sample 30 sigma out along feature 0 that is the nearest analog of a quarter of its
    queries, which lie beyond it"""
    rng = np.random.default_rng(seed)
    C = len(EPI_RATIOS) + 1
    X, y, Xq = np.empty((EPI_T, EPI_F, C)), np.empty((EPI_T, C)), np.empty((EPI_TQ, EPI_F, C))
    for c in range(C):
        ratio = EPI_RATIOS[c] if c < len(EPI_RATIOS) else 1e-6
        X[:, :, c], y[:, c] = regime(rng, EPI_T, EPI_F, ratio, 0, 280.0, 0.0, True)
        Xq[:, :, c] = 280.0 + 0.5 * SIGMA * rng.standard_normal((EPI_TQ, EPI_F))
    far = np.array([280.0 + 30 * SIGMA, 280.0, 280.0])
    y[7, C - 1] += float((far - X[7, :, C - 1]).sum())  # on the line
    X[7, :, C - 1] = far
    nq = EPI_TQ // 4
    Xq[:nq, :, C - 1] = far + np.column_stack([SIGMA * (1.0 + rng.random(nq)), rng.standard_normal((nq, 2))])
    return X, y, Xq
