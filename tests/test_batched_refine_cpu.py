"""CPU checks of tests/batched_refine_model.py, the numpy restatement the GPU tests of the batched expert layer compare with bit for
bit (include/mpf_c.h: mpf_lange_batched, mpf_gecon_batched, mpf_residual_batched, mpf_gerfs_batched).  No GPU.

Inputs are well conditioned (singular values 1 .. 1e-2: kappa_2 = 100 <= 1e3) with "stale factors": LU of A + 2^-k E, E standard
normal, k in {none, 40, 20, 12, 8, 4, 2}; refinement is against A, X0 = getrs of B.

Where the comparison with tests/gerfs_model.py can hold, and why.  That model forms r = b - op(A) x as a matrix product, this one in
ascending j; the two r differ by about n eps (|b| + |op(A)| |x|), so the two berr differ by about n eps / berr RELATIVE.  A relative
1e-10 is therefore derivable for a column only while berr >= 1e10 n eps (4e-5 at n = 33, 1.4e-4 at n = 128) at every residual the
column sees, and the decisions "berr > eps" and "2 berr <= previous" are the same in both only there; at a converged column berr is
rounding noise of the residual itself and either model may take one correction more.  The decision test takes every column of the
family (itmax 1, 2 and LAPACK's 5) that satisfies this bound at each of its residuals -- and asserts that these columns are many and
reach both "not halved" and "itmax".  The norm comparison with dlacn2 is made twice: against gerfs_model's ferr on those columns, and
for EVERY column against dlacn2 driven by the same solves on the model's own g, where no residual noise enters."""
import functools

import numpy as np
import pytest

import batched_model as M
import batched_refine_model as R
import gerfs_model as G
import lacn2_model as LC

SIZES = [3, 9, 33, 65, 128]
KS = [None, 40, 20, 12, 8, 4, 2]
NRHS = 3


def _inputs(n):
    rng = np.random.default_rng(100 + n)
    Q1, _ = np.linalg.qr(rng.standard_normal((n, n)))
    Q2, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = (Q1 * np.logspace(0, -2, n)) @ Q2.T
    return A, rng.standard_normal((n, n)), rng.standard_normal((n, NRHS))


@functools.lru_cache(maxsize=None)
def _family(n):
    """[(k, A, LU, ipiv, B)] -- computed once, shared, read-only."""
    A, E, B = _inputs(n)
    assert np.linalg.cond(A) <= 1e3
    out = []
    for k in KS:
        LU, ipiv, info = M.getrf_model(A if k is None else A + 2.0 ** -k * E)
        assert info == 0
        for v in (LU, ipiv):
            v.setflags(write=False)
        out.append((k, A, LU, ipiv, B))
    A.setflags(write=False)
    B.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _run(n, trans, itmax):
    """Per member of the family: (model's result, X0)."""
    out = []
    for k, A, LU, ipiv, B in _family(n):
        X0 = M.getrs_model(LU, ipiv, B, trans=trans)
        out.append((R.gerfs_model(A, LU, ipiv, B, X0, trans, itmax), X0))
    return out


def _berr_path(A, LU, ipiv, b, x0, trans, its):
    """berr at every residual a column sees in the model (its + 1 of them)."""
    n, x, path = A.shape[0], np.array(x0, copy=True), []
    for t in range(its + 1):
        r, w = R.residual_model(A, x, b, trans)
        path.append(R.backward_error(r, w, n))
        x = x + M.getrs_model(LU, ipiv, r, trans=trans)
    return path


def _longdouble_solve(A, B):
    """Gaussian elimination with partial pivoting in np.longdouble."""
    n = A.shape[0]
    W = np.concatenate([A.astype(np.longdouble), B.astype(np.longdouble)], axis=1)
    for j in range(n):
        p = j + int(np.argmax(np.abs(W[j:, j])))
        W[[j, p]] = W[[p, j]]
        W[j + 1:] -= np.outer(W[j + 1:, j] / W[j, j], W[j])
    X = np.zeros((n, B.shape[1]), dtype=np.longdouble)
    for j in range(n - 1, -1, -1):
        X[j] = (W[j, n:] - W[j, j + 1:n] @ X[j + 1:]) / W[j, j]
    return X


def test_tree_sum_is_the_stated_tree():
    rng = np.random.default_rng(1)
    for n in (1, 2, 3, 64, 65, 100, 128):
        v = np.abs(rng.standard_normal(n)) * 2.0 ** rng.integers(-30, 30, n)
        p = np.zeros(128)
        p[:n] = v
        h = 64
        while h >= 1:
            p = p[:h] + p[h:2 * h]
            h //= 2
        assert R.tree_sum(v) == p[0]
        assert abs(R.tree_sum(v) - np.sum(v.astype(np.longdouble))) <= 8 * 2.0 ** -53 * np.sum(v)
    assert np.isnan(R.tree_sum([1.0, np.nan, 2.0])) and np.isnan(R.lange_model(np.array([[1.0, np.nan], [0.0, 1.0]]), "M"))
    M2 = np.arange(6.0).reshape(2, 3)[:, :2] - 2.0
    assert R.lange_model(M2, "1") == 3.0 and R.lange_model(M2, "I") == 3.0 and R.lange_model(M2, "M") == 2.0


@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_decisions_and_berr_agree_with_the_dgerfs_model(n, trans):
    thr = 1e10 * n * R.EPS
    compared, stops = 0, set()
    for itmax in (1, 2, 0):
        for (k, A, LU, ipiv, B), ((X, ferr, berr, its, st), X0) in zip(_family(n), _run(n, trans, itmax)):
            def solve(V):
                return M.getrs_model(LU, ipiv, V, trans=trans)

            def solve_t(V):
                return M.getrs_model(LU, ipiv, V, trans=not trans)
            _, ferr_g, berr_g, its_g, _ = G.gerfs_model(A, solve, solve_t, B, X0, trans, itmax)
            for c in range(NRHS):
                if min(_berr_path(A, LU, ipiv, B[:, c], X0[:, c], trans, int(its[c]))) < thr:
                    continue
                print(f"n={n} trans={trans} k={k} itmax={itmax} col={c}: its {its[c]} / {its_g[c]}, berr {berr[c]:.17g} / {berr_g[c]:.17g}, "
                      f"ferr {ferr[c]:.6g} / {ferr_g[c]:.6g}, stop {st[c]}")
                assert its[c] == its_g[c]
                assert abs(berr[c] - berr_g[c]) <= 1e-10 * berr_g[c]
                assert ferr[c] >= ferr_g[c] * (1 - 1e-8)
                compared += 1
                stops.add(st[c])
    assert compared >= 6 * NRHS and stops >= {"not halved", "itmax"}, (compared, stops)


@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_exact_norm_is_at_least_dlacn2s_estimate(n, trans):
    """Every column of the family: the model's ferr numerator against dlacn2 with the same solves on the model's own g."""
    nz = n + 1
    safe1 = nz * R.SAFMIN
    safe2 = safe1 / R.EPS
    for (k, A, LU, ipiv, B), ((X, ferr, berr, its, st), X0) in zip(_family(n), _run(n, trans, 0)):
        for c in range(NRHS):
            r, w = R.residual_model(A, X[:, c], B[:, c], trans)
            g = np.abs(r) + nz * R.EPS * w
            g = np.where(w > safe2, g, g + safe1)
            est, _ = LC.dlacn2(n, lambda v: g * M.getrs_model(LU, ipiv, v, trans=not trans),
                               lambda v: M.getrs_model(LU, ipiv, g * v, trans=trans))
            num = ferr[c] * np.max(np.abs(X[:, c]))
            print(f"n={n} trans={trans} k={k} col={c}: exact {num:.6g}, dlacn2 {est:.6g}")
            assert num >= est * (1 - 1e-8)
            assert num <= est * 3 * n


@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_ferr_bounds_the_forward_error(n, trans):
    """Factors that are accurate (k = none, 40, 20): the rows of the inverse are A's to 2^-20 kappa, far inside the bound's slack."""
    A, _, B = _inputs(n)
    Xt = _longdouble_solve(A.T if trans else A, B)
    for (k, _, LU, ipiv, _), ((X, ferr, berr, its, st), X0) in list(zip(_family(n), _run(n, trans, 0)))[:3]:
        err = np.max(np.abs(X.astype(np.longdouble) - Xt), axis=0) / np.max(np.abs(X), axis=0)
        print(f"n={n} trans={trans} k={k}: forward error {err.astype(float)}, ferr {ferr}")
        assert np.all(ferr >= err.astype(np.float64))
        assert np.all(ferr <= 1e-10)


@pytest.mark.parametrize("norm", ["1", "I"])
@pytest.mark.parametrize("n", SIZES)
def test_rcond_against_dgecon(n, norm):
    for k, A, LU, ipiv, B in _family(n):
        anorm = R.lange_model(A, norm)
        assert abs(anorm - np.linalg.norm(A, 1 if norm == "1" else np.inf)) <= 1e-13 * anorm
        rc, ainvnm = R.gecon_model(LU, anorm, norm)
        ref = LC.gecon(LU, anorm, norm)
        print(f"n={n} norm={norm} k={k}: rcond {rc:.6g}, dgecon {ref:.6g}")
        assert 0 < rc <= ref * (1 + 1e-8)
        assert rc >= ref / (3 * n)
        inv = np.linalg.inv((np.tril(LU, -1) + np.eye(n)) @ np.triu(LU))
        assert abs(ainvnm - np.linalg.norm(inv, 1 if norm == "1" else np.inf)) <= 1e-9 * ainvnm
    Z = np.array(_family(n)[0][2], copy=True)
    Z[n // 2, n // 2] = 0.0
    assert R.gecon_model(Z, 1.0, norm) == (0.0, np.inf)
    assert R.gecon_model(_family(n)[0][2], 0.0, norm)[0] == 0.0
    Z = np.array(_family(n)[0][2], copy=True)
    Z[n - 1, 0] = np.inf
    assert R.gecon_model(Z, 1.0, norm)[0] == 0.0


def test_every_stop_reason_occurs():
    for n in SIZES:
        stops = set()
        for trans in (False, True):
            for itmax in (0, 1, 40):
                for res, _ in _run(n, trans, itmax):
                    stops.update(res[4])
                    assert res[3].max() <= (5 if itmax == 0 else min(itmax, 31))
        assert stops >= {"berr <= eps", "not halved", "itmax"}, (n, stops)


def test_residual_model_is_the_ascending_chain():
    rng = np.random.default_rng(5)
    n = 7
    A, x, b = rng.standard_normal((n, n)), rng.standard_normal(n), rng.standard_normal(n)
    for trans in (False, True):
        Aop = A.T if trans else A
        r, w = R.residual_model(A, x, b, trans)
        for i in range(n):
            ri, wi = b[i], abs(b[i])
            for j in range(n):
                ri = ri - Aop[i, j] * x[j]
                wi = wi + abs(Aop[i, j]) * abs(x[j])
            assert r[i] == ri and w[i] == wi
    bad = A.copy()
    bad[2, 3] = np.nan
    res = R.gerfs_column(bad, *M.getrf_model(A)[:2], b, x)
    assert np.isnan(res[2]) and res[3] == 0 and res[4] == "nan"
