"""CPU checks of the extra-precise refinement (include/mpf_c.h: mpf_gerfsx): csrc/solve_rules.h's XrCol through a stand-alone driver
(tests/gerfsx_rules_driver.cpp, built here with AddressSanitizer and UBSan and run directly) against tests/gerfsx_model.py, bit for
bit, on scripted sequences that reach every transition; and the model itself -- the pair accumulation against an exactly rounded
residual, the whole refinement against a reference solution kept as a pair of doubles -- which pins what the GPU is compared with."""
import os
import subprocess

import numpy as np
import pytest

import gerfsx_model as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS, HUGE = G.EPS, G.HUGE
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("gerfsx_rules") / "gerfsx_rules_driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                    os.path.join(ROOT, "tests", "gerfsx_rules_driver.cpp")], check=True)

    def run(seq, n, ithresh):
        text = "\n".join(" ".join(float(v).hex() if np.isfinite(v) else repr(float(v)) for v in row) for row in seq) + "\n"
        out = subprocess.run([str(exe), str(n), str(ithresh)], input=text, capture_output=True, text=True, timeout=60)
        assert out.returncode == 0 and not out.stderr, out.stderr
        trace, res = [], {}
        for line in out.stdout.splitlines():
            key, *vals = line.split()
            if key == "step":
                trace.append((int(vals[0]), int(vals[1]), int(vals[2]), float.fromhex(vals[3]), float.fromhex(vals[4])))
            else:
                res[key] = int(vals[0]) if key in ("x_state", "z_state", "corrections") else float.fromhex(vals[0])
        return trace, res
    return run


def _bits(v):
    return np.array([v], dtype=np.float64).view(np.uint64)[0]


def _same(driver, seq, n=100, ithresh=10):
    """Runs the sequence through the driver and the model, asserts they agree bit for bit, returns the driver's (trace, result)."""
    trace, res = driver(seq, n, ithresh)
    mtrace, col, (en, ec) = G.run_rule(seq, n, G.clamp_ithresh(ithresh))
    assert len(trace) == len(mtrace)
    for a, b in zip(trace, mtrace):
        assert a[:3] == b[:3] and _bits(a[3]) == _bits(b[3]) and _bits(a[4]) == _bits(b[4]), (a, b)
    assert (res["x_state"], res["z_state"], res["corrections"]) == (col.x_state, col.z_state, col.corrections)
    for key, val in (("final_dx_x", col.final_dx_x), ("final_dz_z", col.final_dz_z), ("dxratmax", col.dxratmax), ("dzratmax", col.dzratmax),
                     ("err_norm", en), ("err_comp", ec)):
        assert _bits(res[key]) == _bits(val), (key, res[key], val)
    return trace, res


def test_converges_on_both_measures_and_the_floor(driver):
    """Corrections shrinking by 1e-6 per step: two are applied, the third is at eps and is not; both bounds are the floor
    max(10, sqrt(N)) eps, for N = 100 and N = 10000."""
    seq = [(1.0, 1e-3, 1e-3), (1.0, 1e-9, 1e-9), (1.0, 1e-17, 1e-17), (1.0, 1e-30, 1e-30)]
    trace, res = _same(driver, seq)
    assert [t[0] for t in trace] == [1, 1, 0]
    assert (res["x_state"], res["z_state"], res["corrections"]) == (G.X_CONV, G.Z_CONV, 2)
    assert res["final_dx_x"] == 1e-17 and res["final_dz_z"] == 1e-17
    assert res["dxratmax"] == 1e-9 / 1e-3 and res["err_norm"] == 10 * EPS and res["err_comp"] == 10 * EPS
    _, res = _same(driver, seq, n=10000)
    assert res["err_norm"] == 100 * EPS and res["err_comp"] == 100 * EPS


def test_no_progress_by_dxrat(driver):
    """A correction 0.8 x the previous one: both states go to NOPROG, the second correction is not applied, the bounds are the last
    measures over 1 - ratmax."""
    trace, res = _same(driver, [(1.0, 1e-3, 2e-3), (1.0, 0.8e-3, 1.6e-3), (1.0, 1e-20, 1e-20)])
    assert [t[0] for t in trace] == [1, 0]
    assert (res["x_state"], res["z_state"], res["corrections"]) == (G.X_NOPROG, G.Z_NOPROG, 1)
    assert res["final_dx_x"] == 0.8e-3 and res["final_dz_z"] == 1.6e-3
    assert res["err_norm"] == 0.8e-3 / (1 - res["dxratmax"]) and res["err_norm"] >= 0.8e-3


def test_no_progress_then_working_again(driver):
    """x stalls while z still contracts (so the loop goes on), then contracts again: NOPROG -> WORKING -> CONV."""
    seq = [(1.0, 1e-3, 1e-4), (1.0, 0.8e-3, 1e-5), (1.0, 1e-4, 1e-6), (1.0, 1e-18, 1e-18)]
    trace, res = _same(driver, seq)
    assert [t[1] for t in trace] == [G.X_WORKING, G.X_NOPROG, G.X_WORKING, G.X_CONV]
    assert [t[0] for t in trace] == [1, 1, 1, 0] and res["corrections"] == 3
    assert res["dxratmax"] == 1e-4 / 0.8e-3 and res["z_state"] == G.Z_CONV
    # the same for z: stalls while x contracts
    seq = [(1.0, 1e-4, 1e-3), (1.0, 1e-5, 0.8e-3), (1.0, 1e-6, 1e-4), (1.0, 1e-18, 1e-18)]
    trace, res = _same(driver, seq)
    assert [t[2] for t in trace] == [G.Z_WORKING, G.Z_NOPROG, G.Z_WORKING, G.Z_CONV]
    assert res["dzratmax"] == 1e-4 / 0.8e-3


def test_unstable_working_unstable_resets_dzratmax(driver):
    seq = [(1.0, 1e-2, 0.2), (1.0, 1e-3, 0.05), (1.0, 1e-4, 0.3), (1.0, 1e-5, 0.01), (1.0, 1e-18, 1e-18)]
    trace, res = _same(driver, seq)
    assert [t[2] for t in trace] == [G.Z_WORKING, G.Z_WORKING, G.Z_UNSTABLE, G.Z_WORKING, G.Z_CONV]
    assert trace[1][4] == 0.05 / 0.2 and trace[2][4] == 0.0 and trace[3][4] == 0.01 / 0.3
    # z never leaves UNSTABLE: its bound stays HUGE / 1 = DBL_MAX, x converges on its own
    trace, res = _same(driver, [(1.0, 1e-3, 0.9), (1.0, 1e-9, 0.8), (1.0, 1e-17, 0.7)])
    assert (res["x_state"], res["z_state"], res["corrections"]) == (G.X_CONV, G.Z_UNSTABLE, 2)
    assert res["err_comp"] == HUGE and res["err_norm"] == 10 * EPS


def test_zero_entries_give_huge(driver):
    """dz = DBL_MAX (a correction where x_i = 0) keeps z UNSTABLE; normx = 0 with a correction gives dx_x = HUGE; an all-zero
    column converges at once with nothing applied."""
    trace, res = _same(driver, [(1.0, 1e-3, HUGE), (1.0, 1e-9, HUGE), (1.0, 1e-17, 0.0)])
    assert [t[2] for t in trace] == [G.Z_UNSTABLE, G.Z_UNSTABLE, G.Z_CONV] and res["x_state"] == G.X_CONV
    trace, res = _same(driver, [(0.0, 1e-3, HUGE), (1e-3, 1e-9, 1e-6), (1e-3, 1e-20, 1e-17)])
    assert trace[0][:3] == (1, G.X_WORKING, G.Z_UNSTABLE) and res["x_state"] == G.X_CONV and res["corrections"] == 2
    trace, res = _same(driver, [(0.0, 0.0, 0.0), (1.0, 1.0, 1.0)])
    assert trace == [(0, G.X_CONV, G.Z_CONV, 0.0, 0.0)] and res["corrections"] == 0
    assert res["final_dx_x"] == 0.0 and res["final_dz_z"] == 0.0 and res["err_norm"] == 10 * EPS and res["err_comp"] == 10 * EPS


@pytest.mark.parametrize("bad", [(1.0, NAN, 1e-3), (NAN, 1e-3, 1e-3), (1.0, 1e-3, NAN), (INF, 1e-3, 0.0), (1.0, INF, HUGE)])
def test_nan_stops_the_column(driver, bad):
    trace, res = _same(driver, [(1.0, 1e-3, 1e-3), bad, (1.0, 1e-17, 1e-17)])
    assert [t[0] for t in trace] == [1, 0] and res["x_state"] == G.X_NAN and res["corrections"] == 1
    assert res["err_norm"] == INF and res["err_comp"] == INF


def test_ithresh_exhausted_while_working(driver):
    """Three iterations allowed, all contracting by ten: every correction is applied, both states end WORKING and take the last
    measures; ithresh = 0 reads 10 and 99 reads 31."""
    seq = [(1.0, 10.0 ** -(k + 1), 2 * 10.0 ** -(k + 1)) for k in range(40)]
    trace, res = _same(driver, seq, ithresh=3)
    assert len(trace) == 3 and (res["x_state"], res["z_state"], res["corrections"]) == (G.X_WORKING, G.Z_WORKING, 3)
    assert res["final_dx_x"] == seq[2][1] and res["final_dz_z"] == seq[2][2] and res["err_norm"] == seq[2][1] / (1 - res["dxratmax"])
    slow = [(1.0, 0.9 * 0.5 ** k, 0.2 * 0.5 ** k) for k in range(40)]     # contracts by exactly rthresh: never NOPROG, eps after 53 steps
    assert len(_same(driver, slow, ithresh=0)[0]) == 10
    assert len(_same(driver, slow, ithresh=99)[0]) == 31


def test_random_sequences_agree(driver):
    """60 random walks over the magnitudes that decide the branches (ratios around rthresh, dz around dz_ub, values around eps)."""
    rng = np.random.default_rng(12)
    for _ in range(60):
        seq, dx, dz = [], 10.0 ** rng.uniform(-6, 0), 10.0 ** rng.uniform(-3, 0.5)
        for _ in range(12):
            seq.append((float(rng.choice([1.0, 3.0, 0.0], p=[0.8, 0.15, 0.05])), dx, float(rng.choice([dz, HUGE], p=[0.95, 0.05]))))
            dx *= 10.0 ** rng.uniform(-8, 0.2)
            dz *= 10.0 ** rng.uniform(-8, 0.5)
        _same(driver, seq, ithresh=int(rng.integers(0, 14)))


def test_pair_accumulation_against_the_exact_residual():
    """The model's pair accumulation meets the bound the GPU test asserts, with room; one fp64 chain does not.  X is the fp64
    solution (a heavily cancelling residual) and random; one partial and three (chunk = 50)."""
    n, m = 120, 5
    rng = np.random.default_rng(1)
    A = G.rand(n, 3)
    B = rng.uniform(-1, 1, (n, m))
    for X in (np.linalg.solve(A, B), rng.uniform(-1, 1, (n, m))):
        Rx = G.exact_residual(A, X, B)
        S = np.abs(B) + np.abs(A) @ np.abs(X)
        bound = 2.0 ** -52 * np.abs(Rx) + 4 * (n + 1) * 2.0 ** -106 * S
        for chunk in (G.RKC, 50):
            err = np.abs(G.pair_residual(A, X, B, chunk) - Rx)
            assert np.all(err <= bound), (err / bound).max()
    assert not np.all(np.abs(G.plain_residual(A, X, B) - Rx) <= bound)


def test_pair_accumulation_is_exact_on_a_grid():
    """Operands on a 2^-20 and a 2^-30 grid: every product is exact and any correct pair accumulation returns the exact residual
    (an int64 product on the host), across a partial seam; the fp64 chain does not."""
    n, m = 300, 4
    rng = np.random.default_rng(2)
    Ai, Xi = rng.integers(-2 ** 20, 2 ** 20, (n, n)), rng.integers(-2 ** 30, 2 ** 30, (n, m))
    A, X = Ai * 2.0 ** -20, Xi * 2.0 ** -30
    B = np.round((A @ X) * 2.0 ** 40) * 2.0 ** -40          # on the grid too, and off the product by up to 2^-41
    Bi = (B * 2.0 ** 50).astype(np.int64)
    assert np.array_equal(Bi * 2.0 ** -50, B)
    Rx = (Bi - Ai @ Xi) * 2.0 ** -50
    assert np.array_equal(G.pair_residual(A, X, B, chunk=128), Rx) and np.array_equal(G.exact_residual(A, X, B), Rx)
    assert np.count_nonzero(Rx) > 0.5 * Rx.size and not np.array_equal(G.plain_residual(A, X, B), Rx)


@pytest.mark.parametrize("kappa,seed", [(1e2, 1), (1e6, 2), (1e10, 3)])
def test_model_end_to_end(kappa, seed):
    """ill(128, kappa) with numpy's fp64 solve as the preconditioner: the refined x is within 4 x 2^-53 of the pair-of-doubles
    reference, normwise and componentwise (measured: 0.55 .. 0.97), and inside both bounds; the same loop on the plain fp64 residual
    is not."""
    n, m = 128, 3
    A = G.ill(n, kappa, seed)
    B = np.random.default_rng(seed).uniform(-1, 1, (n, m))
    solve = lambda V: np.linalg.solve(A, V)
    Xh, Xl = G.reference_pair(A, B, solve)
    X, en, ec, cols = G.gerfsx_model(A, solve, B, solve(B))
    e_norm, e_comp = G.errors(X, Xh, Xl)
    print("kappa", kappa, "norm/eps", e_norm / EPS, "comp/eps", e_comp / EPS, "corrections", [c.corrections for c in cols])
    assert all(c.x_state == G.X_CONV for c in cols)
    assert np.all(e_norm <= 4 * EPS) and np.all(e_comp <= 4 * EPS)
    assert np.all(e_norm <= en) and np.all(e_comp <= ec)
    Xp = G.gerfsx_model(A, solve, B, solve(B), residual=G.plain_residual)[0]
    assert np.all(G.errors(Xp, Xh, Xl)[0] > 4 * EPS)
