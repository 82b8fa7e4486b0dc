"""CPU checks of tests/batched_refine_blocked_model.py, the numpy restatement the GPU tests of the blocked batched expert layer compare
with bit for bit (include/mpf_c.h: mpf_lange_batched_blocked, mpf_gecon_batched_blocked, mpf_residual_batched_blocked,
mpf_gerfs_batched_blocked).  No GPU.

Three claims carry the contract "for n <= 128 the blocked entries return the small entries' bits":
  - the tree padded to 1024 is the tree padded to 128 on data of length <= 128 (and to any power of two in between);
  - the model is batched_refine_model on such data, entry by entry;
  - the input family of the GPU tests -- batched_refine_model's stale factors plus one exact column per matrix -- reaches every stop
    reason of the rule at the orders the GPU tests take.  The stale family alone stops reaching "berr <= eps" between n = 161 and 257;
    the exact column (b = column j of op(A), x0 = e_j: r = 0) restores it.  Orders 1023 and 1024 are left to the GPU test's own
    assertion: their factorization in numpy alone takes half a minute.  n = 1 cannot fail to halve and then go on (a scalar's
    correction either converges at once or repeats), so "not halved" is asked from n = 2 on."""
import functools

import numpy as np
import pytest

import batched_model as M
import batched_refine_blocked_model as RB
import batched_refine_model as R

SMALL = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128]
NATURAL = [129, 130, 161, 192, 193, 255, 256, 257]
LARGE = [511, 513]
LARGE_KS = [None, 12, 2]


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 100, 127, 128])
def test_tree_padded_to_1024_is_the_tree_padded_to_128(n):
    rng = np.random.default_rng(n)
    v = np.abs(rng.standard_normal((n, 9))) * 10.0 ** rng.integers(-8, 8, (n, 9))
    want = R.tree_sum(v)
    assert np.array_equal(_bits(RB.tree_sum(v)), _bits(want))
    for pad in (128, 256, 512):
        assert np.array_equal(_bits(RB.tree_sum(v, pad_to=pad)), _bits(want))
    assert np.array_equal(_bits(RB.tree_sum(v.T, axis=1)), _bits(want))


def test_tree_above_128_pairs_i_with_i_plus_512_first():
    # an order where the halving tree and a left-to-right sum differ: 1 + 2^-53 + 2^-53 is 1 from the left, and 1 + 2^-52 in the tree
    v = np.zeros(1024)
    v[0], v[1], v[513] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert RB.tree_sum(v) == 1.0 + 2.0 ** -52 and (v[0] + v[1]) + v[513] == 1.0
    w = np.abs(np.random.default_rng(5).standard_normal(700))
    pad = np.zeros(1024)
    pad[:700] = w
    s = pad[:512] + pad[512:]
    for h in (256, 128, 64, 32, 16, 8, 4, 2, 1):
        s = s[:h] + s[h:2 * h]
    assert RB.tree_sum(w) == s[0]


@functools.lru_cache(maxsize=None)
def _small(n):
    rng = np.random.default_rng(300 + n)
    A = rng.standard_normal((n, n))
    LU, ipiv, info = M.getrf_model(A + 2.0 ** -12 * rng.standard_normal((n, n)))
    assert info == 0
    return A, LU, ipiv, rng.standard_normal((n, 3))


@pytest.mark.parametrize("n", [1, 2, 33, 65, 128])
def test_model_is_the_small_model_up_to_128(n):
    A, LU, ipiv, B = _small(n)
    for norm in ("1", "I", "M"):
        assert np.array_equal(_bits(RB.lange_model(A, norm)), _bits(R.lange_model(A, norm)))
    for norm in ("1", "I"):
        an = R.lange_model(A, norm)
        assert np.array_equal(_bits(RB.gecon_model(LU, an, norm)), _bits(R.gecon_model(LU, an, norm)))
    Z = LU.copy()
    Z[n // 2, n // 2] = 0.0
    assert RB.gecon_model(Z, 1.0, "1") == R.gecon_model(Z, 1.0, "1") == (0.0, np.inf)
    assert RB.gecon_model(LU, 0.0, "I")[0] == 0.0
    for trans in (False, True):
        X0 = M.getrs_model(LU, ipiv, B, trans=trans)
        for itmax in (0, 1):
            got = RB.gerfs_model(A, LU, ipiv, B, X0, trans, itmax)
            want = R.gerfs_model(A, LU, ipiv, B, X0, trans, itmax)
            for g, w in zip(got[:3], want[:3]):
                assert np.array_equal(_bits(g), _bits(w))
            assert np.array_equal(got[3], want[3]) and got[4] == want[4]
    An = A.copy()
    An[n - 1, 0] = np.nan
    got = RB.gerfs_model(An, LU, ipiv, B, M.getrs_model(LU, ipiv, B), False, 0)
    assert got[4] == ["nan"] * 3 and np.isnan(got[2]).all() and not got[3].any()


@pytest.mark.parametrize("n", SMALL + NATURAL + LARGE)
def test_family_with_the_exact_column_reaches_every_stop_reason(n):
    ks = LARGE_KS if n in LARGE else RB.KS
    A, Af, B = RB.family(n, ks)
    stops, exact = set(), set()
    for s in range(len(ks)):
        LU, ipiv, info = M.getrf_model(Af[s])
        assert info == 0
        b = B[s].copy()
        X0 = M.getrs_model(LU, ipiv, b)
        b[:, -1], X0[:, -1] = RB.exact_column(A[s], False)
        r, w = RB.residual_model(A[s], X0[:, -1], b[:, -1])
        assert not r.any() and RB.backward_error(r, w, n) == 0.0          # the exact column: r = 0 exactly
        for itmax in (0, 1):
            X, _, berr, its, st = RB.gerfs_model(A[s], LU, ipiv, b, X0, False, itmax, want_ferr=False)
            stops.update(st)
            exact.add(st[-1])
            assert berr[-1] == 0.0 and its[-1] == 0 and np.array_equal(X[:, -1], X0[:, -1])
    assert exact == {"berr <= eps"}
    assert stops >= ({"berr <= eps", "itmax"} if n == 1 else {"berr <= eps", "not halved", "itmax"}), stops


def test_exact_column_for_the_transposed_system():
    A = np.random.default_rng(11).standard_normal((40, 40))
    b, x0 = RB.exact_column(A, True)
    r, w = RB.residual_model(A, x0, b, trans=True)
    assert not r.any() and w.all()
