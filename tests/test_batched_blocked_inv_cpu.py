"""CPU tests of the blocked batched inverse and determinant as algorithms (tests/batched_blocked_inv_model.py restates
csrc/batched_blocked.hip: bb_getri_kernel and bb_getdet_kernel): the blocked, tiled, skipping form gives the contract's bits -- the
solve's chains on an identity (tests/batched_inv_model.py: getri_model), the signs of zeros included -- for every tile and block
width, and a form that loses one term at a block seam does not.  No GPU."""
import functools
import math

import numpy as np
import pytest

import batched_blocked_inv_model as BI
import batched_inv_model as MI

ORDERS = [1, 2, 31, 32, 33, 64, 65, 97, 161]
PIVOTS = ["random", "identity", "reversal", "last_row", "out_of_range"]
BLOCKS = [32, 24]            # the built width, and one that divides none of ORDERS
TILES = [16, 8]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _pivots(n, kind, rng):
    j = np.arange(n)
    if kind == "random":                                  # as a factorization leaves them: ipiv[j] >= j + 1
        p = j + rng.integers(0, n - j)
    elif kind == "identity":
        p = j
    elif kind == "reversal":
        p = np.where(j < n // 2, n - 1 - j, j)
    elif kind == "last_row":
        p = np.full(n, n - 1)
    else:
        p = j + rng.integers(0, n - j)
        bad = np.array([-6, -1, n, n + 1, 999])           # 0-based; 1-based they are -5, 0, n + 1, n + 2, 1000
        at = rng.integers(0, n, size=min(n, 5))
        p[at] = bad[:len(at)]
    return (p + 1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _factors(n, kind):
    """(LU, ipiv, the contract's inverse): unit-lower L with entries in [-1, 1], some of them -0.0 and +0.0, U well away from zero."""
    rng = np.random.default_rng(1000 * n + PIVOTS.index(kind))
    LU = rng.uniform(-1.0, 1.0, (n, n))
    LU[np.arange(n), np.arange(n)] = rng.uniform(1.0, 2.0, n) * rng.choice([-1.0, 1.0], n)
    low = np.tril_indices(n, -1)
    sel = rng.random(len(low[0]))
    LU[low[0][sel < 0.15], low[1][sel < 0.15]] = 0.0
    LU[low[0][sel > 0.85], low[1][sel > 0.85]] = -0.0
    up = np.triu_indices(n, 1)
    sel = rng.random(len(up[0]))
    LU[up[0][sel < 0.05], up[1][sel < 0.05]] = -0.0
    ipiv = _pivots(n, kind, rng)
    want = MI.getri_model(LU, (BI.clean_pivots(ipiv, n) + 1).astype(np.int32))
    for a in (LU, ipiv, want):
        a.setflags(write=False)
    return LU, ipiv, want


@pytest.mark.parametrize("kind", PIVOTS)
@pytest.mark.parametrize("n", ORDERS)
def test_blocked_inverse_has_the_contracts_bits(n, kind):
    LU, ipiv, want = _factors(n, kind)
    assert np.all(np.isfinite(want))
    for bs in BLOCKS:
        for ct in TILES:
            got = BI.getri_blocked_model(LU, ipiv, ct=ct, bs=bs)
            assert np.array_equal(_bits(got), _bits(want)), (n, kind, bs, ct)


def test_zeros_keep_their_signs():
    """A diagonal U with entries of both signs: the zeros of the inverse are +0 / u_ii, of both signs, and the blocked form has them."""
    n = 70
    LU = np.diag(np.where(np.arange(n) % 3 == 0, -2.0, 4.0))
    ipiv = _pivots(n, "reversal", None)
    want = MI.getri_model(LU, ipiv)
    assert np.any((want == 0.0) & np.signbit(want)) and np.any((want == 0.0) & ~np.signbit(want))
    for ct in TILES:
        assert np.array_equal(_bits(BI.getri_blocked_model(LU, ipiv, ct=ct)), _bits(want))


def test_the_map_is_the_skipping_models():
    for n in (1, 7, 33):
        for kind in PIVOTS[:4]:
            _, ipiv, _ = _factors(n, kind)
            k = BI.column_map(ipiv, n)
            assert np.array_equal(MI.start_rows(ipiv)[k], np.arange(n)) and sorted(k) == list(range(n))


@pytest.mark.parametrize("n,ct", [(65, 16), (97, 8), (161, 16)])
def test_a_dropped_term_changes_the_answer(n, ct):
    """One step's terms left out for the rows beyond its block: at a block seam (the first and last step of a block), and at the
    first block of a tile that does not start at row 0."""
    LU = np.array(_factors(n, "random")[0])
    LU[LU == 0.0] = 0.5                                   # (every term counts)
    ipiv = _factors(n, "random")[1]
    want = BI.getri_blocked_model(LU, ipiv, ct=ct)
    assert np.array_equal(_bits(want), _bits(MI.getri_model(LU, ipiv)))
    k = BI.column_map(ipiv, n)
    for j in (31, 32, 63):
        got = BI.getri_blocked_model(LU, ipiv, ct=ct, drop=("L", j))
        assert not np.array_equal(_bits(got), _bits(want)), ("L", j)
    for j in (32, 63, 64):
        got = BI.getri_blocked_model(LU, ipiv, ct=ct, drop=("U", j))
        assert not np.array_equal(_bits(got), _bits(want)), ("U", j)
    # the tile that starts at q0 = 48 begins its forward sweep in block 1: step 48 is the first that meets its column 48, and the
    # columns that start below row 48 never see it
    got = BI.getri_blocked_model(LU, ipiv, ct=ct, drop=("L", 48))
    diff = _bits(got) != _bits(want)
    assert diff[:, k[48]].any() and not diff[:, k[49:]].any()


DET_ORDERS = [255, 256, 257, 512, 513, 1024]


def _det_diagonals(n):
    rng = np.random.default_rng(n)
    base = rng.uniform(1.0, 2.0, n) * rng.choice([-1.0, 1.0], n)
    yield "up", base * 1e300                              # the running exponent passes +1024 within the first two entries
    yield "down", base * 1e-300                           # ... and -1074
    swing = base.copy()
    swing[: n // 2] *= 1e300
    swing[n // 2:] *= 1e-300                              # leaves the range upwards, comes back, ends near 1
    yield "swing", swing
    yield "subnormal", base * 5e-324 * 2.0 ** 20
    yield "plain", base


@pytest.mark.parametrize("n", DET_ORDERS)
def test_chunked_determinant_has_getdet_models_bits(n):
    rng = np.random.default_rng(7 * n)
    for flips in (0, 1, 2):
        ipiv = np.arange(1, n + 1, dtype=np.int32)
        ipiv[:flips] = n
        if n == 1 and flips:
            continue
        for name, d in _det_diagonals(n):
            want = MI.getdet_model(d, ipiv)
            got = BI.getdet_chunked_model(d, ipiv)
            assert _bits(np.float64(got[0])) == _bits(np.float64(want[0])) and got[1] == want[1], (n, name, flips)
            if name == "up":
                assert want[1] > 1024 * 200
            if name == "down":
                assert want[1] < -1024 * 200
    d = rng.uniform(1.0, 2.0, n)
    ipiv = np.arange(1, n + 1, dtype=np.int32)
    for i in (0, min(255, n - 1), n - 1):
        z = d.copy()
        z[i] = 0.0
        assert BI.getdet_chunked_model(z, ipiv) == (0.0, 0) == MI.getdet_model(z, ipiv)
        z[(i + 1) % n] = np.inf
        got = BI.getdet_chunked_model(z, ipiv)
        assert math.isnan(got[0]) and got[1] == 0 and math.isnan(MI.getdet_model(z, ipiv)[0])
