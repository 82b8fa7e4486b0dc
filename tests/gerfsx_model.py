"""numpy restatement of the extra-precise refinement (include/mpf_c.h: mpf_residual_x, mpf_gerfsx): the pair accumulation of the
residual (TwoProd by Veltkamp's split, Knuth's TwoSum), the per-column rule XrCol of csrc/solve_rules.h, the loop around them, an
exactly rounded residual (math.fsum over the exact product pairs) and a reference solution kept as an unevaluated pair of doubles."""
import math

import numpy as np

EPS = 2.0 ** -53
HUGE = float(np.finfo(np.float64).max)
RTHRESH, DZ_UB = 0.5, 0.25
RKC = 4096                      # columns of op(A) per partial pair (csrc/solve_xr.hip)
X_WORKING, X_NOPROG, X_CONV, X_NAN = 0, 1, 2, 3
Z_UNSTABLE, Z_WORKING, Z_NOPROG, Z_CONV = -1, 0, 1, 2


def rand(n, seed, dominant=2.0):
    """The suite's diagonally dominant test matrix (tests/test_gpu_gerfs.py: _rand)."""
    A = np.random.default_rng(seed).uniform(-1, 1, (n, n))
    A[np.arange(n), np.arange(n)] += dominant if n > 1 else 0.5
    return np.asfortranarray(A)


def ill(n, kappa, seed):
    """Singular values spread by logspace over kappa (tests/test_gpu_gerfs.py: _ill)."""
    rng = np.random.default_rng(seed)
    U, _ = np.linalg.qr(rng.standard_normal((n, n)))
    V, _ = np.linalg.qr(rng.standard_normal((n, n)))
    s = np.logspace(0, -np.log10(kappa), n)
    return np.asfortranarray((U * s) @ V.T)


def two_sum(a, b):
    """s + t = a + b exactly (Knuth, six operations, no assumption about magnitudes)."""
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = 134217729.0 * a          # 2^27 + 1
    hi = c - (c - a)
    return hi, a - hi


def two_prod(a, b):
    """p + e = a b exactly (Dekker, Veltkamp's split: what fma(a, b, -p) gives without an fma; no over- or underflow here)."""
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _pair_sub_products(hi, lo, Aop, X, k0, k1):
    """(hi, lo) -= sum_{k0 <= k < k1} Aop[:, k] X[k, :], k ascending, as the kernel does it."""
    for k in range(k0, k1):
        p, e = two_prod(Aop[:, k:k + 1], X[k:k + 1, :])
        hi, t = two_sum(hi, -p)
        lo = lo + (t - e)
    return hi, lo


def pair_residual(Aop, X, B, chunk=RKC):
    """R = B - Aop X as mpf_residual_x forms it: every element a pair (hi, lo) from (b, 0), partial pairs per `chunk` columns of
    op(A) added in ascending order by the same pair addition, hi + lo rounded once."""
    n = Aop.shape[0]
    X = X.reshape(n, -1)
    hi, lo = B.reshape(n, -1).astype(np.float64).copy(), np.zeros(X.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        for k0 in range(0, n, chunk):
            ph, pl = _pair_sub_products(np.zeros(X.shape), np.zeros(X.shape), Aop, X, k0, min(n, k0 + chunk))
            hi, t = two_sum(hi, ph)
            lo = lo + (t + pl)
        return hi + lo


def plain_residual(Aop, X, B):
    """The same residual in one fp64 chain, k ascending (what the feature is compared with)."""
    r = B.astype(np.float64).copy()
    for k in range(Aop.shape[0]):
        r = r - Aop[:, k:k + 1] * X[k:k + 1, :]
    return r


def exact_residual(Aop, X, B):
    """B - Aop X with ONE rounding per element: math.fsum over b and the exact product pairs."""
    n, m = X.shape
    R = np.empty((n, m))
    for j in range(m):
        p, e = two_prod(Aop, X[:, j][None, :])
        terms = np.concatenate([B[:, j:j + 1], -p, -e], axis=1).tolist()
        R[:, j] = [math.fsum(row) for row in terms]
    return R


def pair_residual_of_pair(Aop, Xh, Xl, B):
    """B - Aop (Xh + Xl) for a solution kept as a pair of doubles, accumulated in pairs (the reference solution's residual)."""
    hi, lo = B.astype(np.float64).copy(), np.zeros(B.shape)
    for k in range(Aop.shape[0]):
        for Xp in (Xh, Xl):
            p, e = two_prod(Aop[:, k:k + 1], Xp[k:k + 1, :])
            hi, t = two_sum(hi, -p)
            lo = lo + (t - e)
    return hi + lo


def reference_pair(Aop, B, solve, sweeps=8):
    """The solution of Aop X = B as an unevaluated pair (Xh, Xl): refinement with the pair residual of the pair, until the
    correction is below 2^-90 of max |x| or no longer shrinks by four (its error is then far below 2^-53, about kappa n eps^2)."""
    Xh = solve(B)
    Xl = np.zeros(B.shape)
    last = np.inf
    for _ in range(sweeps):
        d = solve(pair_residual_of_pair(Aop, Xh, Xl, B))
        s, t = two_sum(Xh, d)
        Xh, Xl = two_sum(s, t + Xl)
        scale = np.abs(Xh).max(axis=0)
        rel = float((np.abs(d).max(axis=0) / np.where(scale == 0, 1.0, scale)).max())
        if rel <= 2.0 ** -90 or rel > 0.25 * last:
            break
        last = rel
    return Xh, Xl


def errors(X, Xh, Xl):
    """(normwise, componentwise) error of X per column against the pair reference: max |x - xref| / max |xref| and
    max_i |x_i - xref_i| / |xref_i| (0 / 0 reads 0)."""
    diff = np.abs((X - Xh) - Xl)
    nx = np.abs(Xh).max(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        comp = np.where(diff == 0, 0.0, diff / np.abs(Xh))
    return diff.max(axis=0) / np.where(nx == 0, 1.0, nx), comp.max(axis=0)


def _maxn(v):
    """max that keeps a NaN (the kernels' maxn)."""
    return float("nan") if np.isnan(v).any() else float(v.max())


def measures(x, d):
    """(normx, normdx, dz) of a step: max |x_i|, max |d_i|, max |d_i| / |x_i| (HUGE where x_i = 0 != d_i, 0 where both are 0)."""
    ax, ad = np.abs(x), np.abs(d)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(x != 0, ad / ax, np.where(np.isnan(d), d, np.where(d != 0, HUGE, 0.0)))
    return _maxn(ax), _maxn(ad), _maxn(q)


class XrCol:
    """csrc/solve_rules.h: XrCol, statement by statement."""

    def __init__(self):
        self.x_state, self.z_state = X_WORKING, Z_UNSTABLE
        self.corrections = 0
        self.dxratmax = self.dzratmax = 0.0
        self.final_dx_x = self.final_dz_z = self.prev_dx = self.prev_dz = HUGE
        self.last_dx_x = self.last_dz = HUGE

    def step(self, normx, normdx, dz):
        if math.isnan(normx) or math.isnan(normdx) or math.isnan(dz) or math.isinf(normx) or math.isinf(normdx):
            self.x_state = X_NAN
            return False
        f = np.float64
        with np.errstate(all="ignore"):
            dx_x = float(f(normdx) / f(normx)) if normx != 0 else (0.0 if normdx == 0 else HUGE)
            dxrat, dzrat = float(f(normdx) / f(self.prev_dx)), float(f(dz) / f(self.prev_dz))
        self.last_dx_x, self.last_dz = dx_x, dz
        if self.x_state == X_NOPROG and dxrat <= RTHRESH:
            self.x_state = X_WORKING
        if self.x_state == X_WORKING:
            if dx_x <= EPS:
                self.x_state = X_CONV
            elif dxrat > RTHRESH:
                self.x_state = X_NOPROG
            elif self.dxratmax < dxrat:
                self.dxratmax = dxrat
            if self.x_state > X_WORKING:
                self.final_dx_x = dx_x
        if self.z_state == Z_UNSTABLE and dz <= DZ_UB:
            self.z_state = Z_WORKING
        if self.z_state == Z_NOPROG and dzrat <= RTHRESH:
            self.z_state = Z_WORKING
        if self.z_state == Z_WORKING:
            if dz <= EPS:
                self.z_state = Z_CONV
            elif dz > DZ_UB:
                self.z_state, self.dzratmax, self.final_dz_z = Z_UNSTABLE, 0.0, HUGE
            elif dzrat > RTHRESH:
                self.z_state = Z_NOPROG
            elif self.dzratmax < dzrat:
                self.dzratmax = dzrat
            if self.z_state > Z_WORKING:
                self.final_dz_z = dz
        if self.x_state != X_WORKING and self.z_state != Z_WORKING:
            return False
        self.prev_dx, self.prev_dz = normdx, dz
        self.corrections += 1
        return True

    def finish(self, n):
        """(err_norm, err_comp)"""
        if self.x_state == X_NAN:
            return float("inf"), float("inf")
        if self.x_state == X_WORKING:
            self.final_dx_x = self.last_dx_x
        if self.z_state == Z_WORKING:
            self.final_dz_z = self.last_dz
        lbnd = max(10.0, math.sqrt(float(n))) * EPS
        with np.errstate(all="ignore"):
            en = float(np.float64(self.final_dx_x) / np.float64(1 - self.dxratmax))
            ec = float(np.float64(self.final_dz_z) / np.float64(1 - self.dzratmax))
        return max(en, lbnd), max(ec, lbnd)


def run_rule(seq, n, ithresh):
    """XrCol over a scripted sequence of (normx, normdx, dz), as tests/gerfsx_rules_driver.cpp runs it: (trace, col, bounds);
    trace: per step (applied, x_state, z_state, dxratmax, dzratmax)."""
    col, trace = XrCol(), []
    for cnt, (a, b, c) in enumerate(seq):
        if cnt >= ithresh:
            break
        go = col.step(a, b, c)
        trace.append((int(go), col.x_state, col.z_state, col.dxratmax, col.dzratmax))
        if not go:
            break
    return trace, col, col.finish(n)


def clamp_ithresh(ithresh):
    return 10 if ithresh <= 0 else min(ithresh, 31)


def gerfsx_model(Aop, solve, B, X0, ithresh=0, residual=pair_residual):
    """mpf_gerfsx on the host: refines X0 (all columns in lock-step, a stopped column frozen).  solve(V) = op(A)^-1 V on whatever
    factors are modelled.  Returns (X, err_norm, err_comp, cols) -- cols: the XrCol of every column after finish()."""
    n, m = B.shape
    X = X0.astype(np.float64).copy()
    cols = [XrCol() for _ in range(m)]
    active = np.ones(m, dtype=bool)
    for _ in range(clamp_ithresh(ithresh)):
        with np.errstate(all="ignore"):
            D = solve(residual(Aop, X, B))
        for j in range(m):
            if active[j]:
                active[j] = cols[j].step(*measures(X[:, j], D[:, j]))
        if not active.any():
            break
        X[:, active] += D[:, active]
    bounds = [c.finish(n) for c in cols]
    return X, np.array([b[0] for b in bounds]), np.array([b[1] for b in bounds]), cols
