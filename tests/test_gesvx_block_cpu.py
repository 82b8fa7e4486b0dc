"""CPU checks of the many-column expert driver's ground work: mpf_gesvx_block in the header and the ABI list, and the numpy
restatement of its steps 5 .. 7 (tests/gesvx_block_model.py) on matrices whose rows are scaled by 2^[-20, 20]:
    the model's berr with scale vectors == the model's berr on the explicitly equilibrated system, bit for bit (every scale is a
        power of two: the residual and the weights of the two systems differ by an exact factor per row);
    max|x - x_ref| / max|x| <= ferr, x_ref from a refinement with a longdouble residual;
    lo / 3 <= ferr <= 1.01 hi, the bracket of tests/test_gpu_gerfs.py (dlacn2 never overestimates and is within Higham's factor 3;
        the fp64 |r| exceeds the true one by at most nz eps w2), evaluated on the ORIGINAL system."""
import os
import re

import numpy as np
import pytest

import gesvx_block_model as GB
import lacn2_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_in_header_and_abi_list(mpf):
    hdr = open(os.path.join(ROOT, "include", "mpf_c.h")).read()
    assert re.search(r"\bint\s+mpf_gesvx_block\s*\(", hdr)
    assert "mpf_gesvx_block" in mpf.C_ABI_SYMBOLS
    assert hasattr(mpf.MPFContext, "gesvx_block")


def _system(n, trans, seed):
    """(A, B, r, c, S): A = Dr0^-1 A0 with Dr0 = 2^k, k in [-20, 20]; r, c the power-of-two factors of the geequ model; S = Dr A Dc."""
    rng = np.random.default_rng(seed)
    A0 = rng.uniform(-1, 1, (n, n))
    A0[np.arange(n), np.arange(n)] += 2.0 if n > 1 else 0.5
    k = rng.integers(-20, 21, n)
    A = np.ldexp(A0, -k[:, None])
    B = rng.uniform(-1, 1, (n, 3)) * np.logspace(-2, 2, 3)
    if not trans:
        B = np.ldexp(B, -k[:, None])
    r, c, _, _, _, info = M.geequ(A)
    assert info == 0
    S = (A * r[:, None]) * c[None, :]
    assert np.array_equal(S / c[None, :] / r[:, None], A), "the scaling is exact"
    return A, B, r, c, S


@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("n", [1, 7, 40])
def test_model_on_row_scaled_systems(n, trans):
    A, B, r, c, S = _system(n, trans, 10 * n + trans)
    Sop = np.ascontiguousarray(S.T if trans else S)
    Minv = np.linalg.inv(Sop)                                   # the "factors": one explicit inverse of the equilibrated op(S)
    pre, post = (c, r) if trans else (r, c)
    solve, solve_t = GB.scaled_solvers(lambda v: Minv @ v, lambda v: Minv.T @ v, pre, post)
    res = GB.gesvx_block_model(A, B, trans, [(solve, solve_t)])
    assert res["ret"] == 0 and res["attempt"] == 0
    X, ferr, berr = res["X"], res["ferr"], res["berr"]

    # the explicitly equilibrated system op(S) Y = pre .* B, X = post .* Y, from the same start
    Xs, ir = GB.refine_model(A, solve, B, trans)
    Bs, Y0 = pre[:, None] * B, Xs / post[:, None]
    eq = GB.G.gerfs_model(S, lambda v: Minv @ v, lambda v: Minv.T @ v, Bs, Y0, trans)
    print("berr / eps", berr / GB.EPS, "equilibrated", eq[2] / GB.EPS, "iterations", res["iterations"], eq[3])
    assert np.array_equal(berr.view(np.uint64), eq[2].view(np.uint64))
    assert np.array_equal(res["iterations"], eq[3])
    assert np.array_equal(X, post[:, None] * eq[0])

    # bounds on the ORIGINAL system; op(A)^-1 = post .* op(S)^-1 .* pre exactly
    Aop = np.ascontiguousarray(A.T if trans else A)
    inv = post[:, None] * Minv * pre[None, :]
    berr_exact, err, lo, hi = GB.exact_quantities(Aop, inv, B, X, inv @ B)
    print("err / ferr", err / ferr, "ferr / lo", ferr / lo, "ferr / hi", ferr / hi)
    assert np.all(np.abs(berr - berr_exact) <= 2 * (n + 1) * GB.EPS)
    assert np.all(err <= ferr), (err, ferr)
    assert np.all(lo / 3 <= ferr) and np.all(ferr <= 1.01 * hi), (lo, ferr, hi)


def test_model_falls_back_for_all_columns():
    """One column that cannot converge on the first factors sends every column to the second ones, and the result is that of
    a call with the second factors only."""
    n = 12
    rng = np.random.default_rng(3)
    A = rng.uniform(-1, 1, (n, n)) + 3 * np.eye(n)
    inv = np.linalg.inv(A)
    rough = inv * (1 + 0.5 * rng.uniform(-1, 1, (n, n)))         # contracts slowly: trips max_iter = 2
    good = (lambda v: inv @ v, lambda v: inv.T @ v)
    bad = (lambda v: rough @ v, lambda v: rough.T @ v)
    B = rng.uniform(-1, 1, (n, 4))
    res = GB.gesvx_block_model(A, B, False, [bad, good], max_iter=2)
    assert res["attempt"] == 1 and res["ret"] == 0
    direct = GB.gesvx_block_model(A, B, False, [good], max_iter=2)
    assert np.array_equal(direct["X"], res["X"]) and np.array_equal(direct["ferr"], res["ferr"]) and np.array_equal(direct["berr"], res["berr"])
    only = GB.gesvx_block_model(A, B, False, [bad], max_iter=2, bounds=False)
    assert only["ret"] == 1 and only["ferr"] is None
