"""numpy restatement of mpf_geequ_batched, mpf_laqge_batched, mpf_lascl2_batched (and their _batched_blocked and _vbatched siblings)
for ONE matrix, and of the Python driver gesvx_batched (include/mpf_c.h) -- test infrastructure.

Nothing is summed: every product is a product with a power of two, every extreme an order-free maximum or minimum, so the same
function restates every layout and kernel form.
  geequ    lacn2_model.geequ's rule (mpf_geequ's definitions) plus the non-finite flag: a NaN or Inf anywhere gives info = 2 n + 1 before
           any scale is formed.  What the contract leaves unwritten is None here.  A zero row gets r_i = 1 (mpf_geequ's kernel).
  laqge    rule 0 never, 1 dlaqge's rule as mpf_gesvx states it, 2 always both; a flagged matrix is never scaled; each element
           (r_i a_ij) c_j, two rounded products in that order, a side that is not scaled contributes none.
  spread   max r / min r and max c / min c of the sides that were scaled, else 1.
  lascl2   V = diag(s) V where the bit is set.
  gesvx    dgesvx's order on top of the LU and refinement models.

family(n) is the input family of the CPU and GPU tests, one slot per kind."""
import numpy as np

import batched_model as BM
import lacn2_model as L2

TINY = np.finfo(np.float64).tiny          # DBL_MIN = smlnum
SMALL = TINY / 2.0 ** -52                 # dlaqge's small = DBL_MIN / DBL_EPSILON
LARGE = 1.0 / SMALL

KINDS = ["well", "rows", "cols", "both", "tiny", "clamp", "zero_row", "zero_col", "nan", "inf"]
FLAGGED = {"zero_row", "zero_col", "nan", "inf"}


def pow2_inv(m):
    """mpf_geequ's factor of a maximum: lacn2_model.pow2_inv, and 1 for m = 0."""
    m = np.asarray(m, dtype=np.float64)
    return np.where(m == 0, 1.0, L2.pow2_inv(np.where(m == 0, 1.0, m)))


def cnd(m):
    big = 1.0 / TINY
    return max(m.min(), TINY) / min(m.max(), big)


def geequ(A):
    """(r, c, rowcnd, colcnd, amax, info); None: not written."""
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[0]
    if n == 0:
        return np.zeros(0), np.zeros(0), 1.0, 1.0, 0.0, 0
    absA = np.abs(A)
    if not np.all(np.isfinite(A)):
        return None, None, None, None, (np.nan if np.any(np.isnan(A)) else np.inf), 2 * n + 1
    rm = absA.max(axis=1)
    amax = rm.max()
    r = pow2_inv(rm)
    if np.any(rm == 0):
        return r, None, 0.0, None, amax, int(np.argmax(rm == 0)) + 1
    rowcnd = cnd(rm)
    with np.errstate(under="ignore"):
        cm = (absA * r[:, None]).max(axis=0)
    if np.any(cm == 0):
        return r, None, rowcnd, None, amax, n + int(np.argmax(cm == 0)) + 1
    return r, pow2_inv(cm), rowcnd, cnd(cm), amax, 0


def decide(rule, rowcnd, colcnd, amax, info, n=1):
    """equed: 0 none, 1 rows, 2 columns, 3 both."""
    assert rule in (0, 1, 2)
    if info != 0 or rule == 0 or n == 0:
        return 0
    if rule == 2:
        return 3
    rows = rowcnd < 0.1 or amax < SMALL or amax > LARGE
    return (1 if rows else 0) | (2 if colcnd < 0.1 else 0)


def laqge(A, eq, rule=1):
    """(As, equed, spread[2]) from geequ's tuple."""
    A = np.asarray(A, dtype=np.float64)
    r, c, rowcnd, colcnd, amax, info = eq
    equed = decide(rule, rowcnd, colcnd, amax, info, A.shape[0])
    As = A.copy()
    spread = np.ones(2)
    with np.errstate(all="ignore"):
        if equed & 1:
            As = r[:, None] * As
            spread[0] = r.max() / r.min()
        if equed & 2:
            As = As * c[None, :]
            spread[1] = c.max() / c.min()
    return As, equed, spread


def lascl2(s, V, equed=None, bit=0):
    V = np.asarray(V, dtype=np.float64)
    if equed is not None and not (equed & bit):
        return V.copy()
    with np.errstate(all="ignore"):
        return (s.reshape((-1,) + (1,) * (V.ndim - 1)) * V)


def gesvx(A, B, trans=False, itmax=0, equilibrate=1, refine=None):
    """(X, rcond, ferr, berr, info, equed, r, c) of one matrix and its right-hand sides B (n, nrhs), in gesvx_batched's order.
    refine: batched_refine_model (n <= 128, the default) or batched_refine_blocked_model."""
    if refine is None:
        import batched_refine_model as refine
    norm = "I" if trans else "1"
    eq = geequ(A)
    As, equed, spread = laqge(A, eq, equilibrate)
    r, c = eq[0], eq[1]
    LU, ipiv, info = BM.getrf_model(As)
    rcond, _ = refine.gecon_model(LU, refine.lange_model(As, norm), norm)
    Bs = lascl2(c if trans else r, B, equed, 2 if trans else 1) if equed else np.array(B, dtype=np.float64)
    X = BM.getrs_model(LU, ipiv, Bs, trans=trans)
    X, ferr, berr, _, _ = refine.gerfs_model(As, LU, ipiv, Bs, X, trans=trans, itmax=itmax)[:5]
    if equed:
        X = lascl2(r if trans else c, X, equed, 1 if trans else 2)
    with np.errstate(all="ignore"):
        ferr = ferr * spread[0 if trans else 1]
    return X, rcond, ferr, berr, info, equed, r, c


# ---- the input family ---------------------------------------------------------------------------------------------------------------------
def well_scaled(n, rng):
    """Entries uniform in [0.5, 1) with random signs: every row maximum in [0.5, 1), so r = 2 and every scaled column maximum in
    [1, 2): rowcnd, colcnd > 0.5 and dlaqge's rule leaves the matrix alone."""
    return rng.uniform(0.5, 1.0, (n, n)) * rng.choice([-1.0, 1.0], (n, n))


def pow2_diag(n, rng, lo=-40, hi=40):
    """2^k, k in [lo, hi], both ends present for n >= 2 (for n = 1 the lower end)."""
    k = rng.integers(lo, hi + 1, n)
    k[0] = lo
    if n > 1:
        k[rng.integers(1, n)] = hi
    return np.ldexp(1.0, k)


def member(kind, n, rng):
    A = well_scaled(n, rng)
    if kind == "well":
        return A
    if kind == "rows":
        return pow2_diag(n, rng)[:, None] * A
    if kind == "cols":
        return A * pow2_diag(n, rng)[None, :]
    if kind == "both":
        return pow2_diag(n, rng)[:, None] * A * pow2_diag(n, rng)[None, :]
    if kind == "tiny":
        return A * 2.0 ** -1000
    if kind == "clamp":
        return A * 2.0 ** -1060                         # subnormal entries: the exponent clamp at -1022
    if kind == "zero_row":
        A[rng.integers(0, n), :] = 0.0
    elif kind == "zero_col":
        A[:, rng.integers(0, n)] = 0.0
    elif kind == "nan":
        A[rng.integers(0, n), rng.integers(0, n)] = np.nan
    else:
        assert kind == "inf"
        A[rng.integers(0, n), rng.integers(0, n)] = -np.inf
    return A


def family(n, seed=0, kinds=KINDS):
    """(batch, n, n) with one slot per kind, in the order of `kinds`."""
    rng = np.random.default_rng(1000 * n + seed)
    return np.stack([member(k, n, rng) for k in kinds])


def expected_equed(kind, n):
    """What rule 1 must decide for a family member, derived (module docstring of tests/test_batched_equil_cpu.py)."""
    if kind in FLAGGED:
        return 0
    if n == 1:                                          # one row, one column: rowcnd = colcnd = 1; only the amax clause can fire
        return 1 if kind in ("tiny", "clamp") else 0
    return {"well": 0, "rows": 1, "cols": 2, "both": 3, "tiny": 1, "clamp": 1}[kind]


# ---- a descriptor: the per-matrix results laid out as mpf_*_vbatched lays them out -----------------------------------------------------------
def descriptor(mats, rule=1, fill=0.0):
    """(r, c, rowcnd, colcnd, amax, info, scaled matrices, equed, spread) of a list of matrices of any orders: r and c are (total_n,)
    with matrix b's at offv[b] = the sum of the orders before it; what is not written holds `fill`."""
    ns = [np.shape(M)[0] for M in mats]
    offv = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
    batch = len(mats)
    r, c = np.full(offv[-1], fill), np.full(offv[-1], fill)
    rowcnd, colcnd, amax = np.full(batch, fill), np.full(batch, fill), np.full(batch, fill)
    info, equed, spread, out = np.zeros(batch, dtype=np.int32), np.zeros(batch, dtype=np.int32), np.ones((batch, 2)), []
    for b, M in enumerate(mats):
        eq = geequ(M)
        sl = slice(offv[b], offv[b + 1])
        for dst, v in ((r, eq[0]), (c, eq[1])):
            if v is not None:
                dst[sl] = v
        for dst, v in ((rowcnd, eq[2]), (colcnd, eq[3]), (amax, eq[4])):
            if v is not None:
                dst[b] = v
        info[b] = eq[5]
        As, equed[b], spread[b] = laqge(M, eq, rule)
        out.append(As)
    return r, c, rowcnd, colcnd, amax, info, out, equed, spread
