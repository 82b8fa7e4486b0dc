"""CPU checks of GMRES-IR's per-column state machine, GmresCol in csrc/solve_rules.h, which mpf_solve_gmres_ir_block drives: a
stand-alone driver (tests/gmres_rules_driver.cpp, built here with AddressSanitizer and UBSan and run directly) is fed the Hessenberg
columns (h, hn), residuals and betas that the numpy model (tests/gmres_block_model.py) recorded on the fixture cases, and must take
the model's decisions -- where each inner loop stops, the outer count, the converged flag -- and return its vectors y to 1e-13
relative (both sides run the same fp64 formulas; numpy's hypot and the C library's may differ in the last bit)."""
import os
import subprocess

import numpy as np
import pytest

import gmres_block_model as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12
# (n, kappa, restart, max_outer): the fixture cases -- several inner loops of different lengths; one long inner loop; restarts;
# no convergence within 31 outer steps
CASES = [(33, 1e6, 40, 10), (300, 1e5, 40, 10), (300, 1e5, 8, 31), (33, 1e6, 8, 31)]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("gmres_rules") / "gmres_rules_driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                    os.path.join(ROOT, "tests", "gmres_rules_driver.cpp")], check=True)

    def run(restart, max_outer, tol, text):
        out = subprocess.run([str(exe), str(restart), str(max_outer), repr(tol)], input=text, capture_output=True, text=True, timeout=60)
        assert out.returncode == 0 and not out.stderr, out.stdout + out.stderr
        return [line.split() for line in out.stdout.splitlines()]
    return run


_models = {}


def model(n, kappa, restart, max_outer, trans):
    """The model's run on the fixture, computed once per case."""
    key = (n, kappa, restart, max_outer, trans)
    if key not in _models:
        A, A16, B, zero = G.fixture(n, kappa, 5, trans)
        _models[key] = G.gmres_ir_model(A, G.getrf(A16), B, trans, max_outer, restart, TOL)[1] + [zero]
    return _models[key][:-1], _models[key][-1]


def transcript(st):
    """One column's records for the driver, with the answers the model gave: (text, expected lines without the y values, [y])."""
    f = lambda v: float(v).hex() if v == v else "nan"
    text, want, ys = [], [], []
    cycles = list(st["cycles"])
    for outer, rel in enumerate(st["history"]):
        go = outer < len(cycles)
        text.append(f"O {f(rel)}")
        want.append(["O", str(outer), str(int(go))])
        if not go:
            break
        cyc = cycles[outer]
        ok = cyc["beta"] != 0 and cyc["beta"] == cyc["beta"]
        text.append(f"B {f(cyc['beta'])}")
        want.append(["B", str(int(ok))])
        if not ok:
            break
        for k, (h, hn) in enumerate(cyc["steps"]):
            text.append(f"S {k + 1} " + " ".join(f(v) for v in h) + f" {f(hn)}")
            want.append(["S", str(k + 1), str(int(k + 1 < len(cyc["steps"])))])
        text.append("Y")
        want.append(["Y", str(cyc["k"])])
        ys.append(cyc["y"])
    return "\n".join(text) + "\n", want, ys


def check(lines, want, ys, st):
    fin = lines[-1]
    body = lines[:-1]
    assert [l[:2] if l[0] == "Y" else l for l in body] == want, "the state machine decided otherwise than the model"
    got_y = [[float.fromhex(v) for v in l[2:]] for l in body if l[0] == "Y"]
    assert len(got_y) == len(ys)
    for a, b in zip(got_y, ys):
        a, b = np.array(a), np.array(b)
        assert a.shape == b.shape and np.all(np.abs(a - b) <= 1e-13 * np.max(np.abs(b))), "y"
    assert fin[0] == "F" and [int(v) for v in fin[1:4]] == [st["converged"], st["outer_iterations"], st["inner_iterations"]]
    same = lambda tok, v: float.fromhex(tok) == v or (v != v and "nan" in tok)
    assert same(fin[4], st["rel_residual"])
    hist = fin[fin.index("|") + 1:]
    assert len(hist) == len(st["history"]) and all(same(t, v) for t, v in zip(hist, st["history"]))


@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("n,kappa,restart,max_outer", CASES)
def test_state_machine_takes_the_models_decisions(driver, n, kappa, restart, max_outer, trans):
    stats, zero = model(n, kappa, restart, max_outer, trans)
    for st in stats:
        text, want, ys = transcript(st)
        check(driver(restart, max_outer, TOL, text), want, ys, st)


def test_fixture_behaves_as_the_gpu_tests_assume():
    """What tests/test_gpu_gmres_block.py relies on, in the model: at restart 40 every column converges within two outer steps, the
    columns of n = 33 need different inner counts, n = 300 takes one outer step of 32 .. 33 inner steps; at restart 8, n = 300 needs
    restarts and n = 33 does not converge in 31 outer steps (final residual 4e-7 .. 1.2e-4, far from the tolerance); the zero column converges at once."""
    for trans in (0, 1):
        stats, zero = model(33, 1e6, 40, 10, trans)
        nz = [s for j, s in enumerate(stats) if j != zero]
        assert all(s["converged"] and 1 <= s["outer_iterations"] <= 2 for s in nz)
        assert len({s["inner_iterations"] for s in nz}) > 1
        assert (stats[zero]["converged"], stats[zero]["outer_iterations"], stats[zero]["inner_iterations"]) == (1, 0, 0)
        stats, zero = model(300, 1e5, 40, 10, trans)
        nz = [s for j, s in enumerate(stats) if j != zero]
        assert all(s["converged"] and s["outer_iterations"] == 1 and 32 <= s["inner_iterations"] <= 33 for s in nz)
        stats, zero = model(300, 1e5, 8, 31, trans)
        nz = [s for j, s in enumerate(stats) if j != zero]
        assert all(s["converged"] and 7 <= s["outer_iterations"] <= 8 for s in nz)
        stats, zero = model(33, 1e6, 8, 31, trans)
        nz = [s for j, s in enumerate(stats) if j != zero]
        assert all(not s["converged"] and s["outer_iterations"] == 31 and 1e-8 < s["rel_residual"] < 1e-3 for s in nz)
        assert stats[zero]["converged"] == 1
        A, A16, B, zero = G.fixture(33, 1e6, 5, trans)
        cl = G.classical_ir_converges(A, G.getrf(A16), B, trans)
        assert not any(cl[j] for j in range(5) if j != zero), "classical refinement must not converge on the fixture"


def test_happy_breakdown_ends_the_inner_loop(driver):
    """hn == 0: the Krylov space is invariant, the inner loop ends at once and y solves the small system exactly (2 / 1)."""
    lines = driver(5, 10, TOL, f"O {1e-3!r}\nB 2.0\nS 1 1.0 0.0\nY\nO 0.0\n")
    assert lines[:3] == [["O", "0", "1"], ["B", "1"], ["S", "1", "0"]]
    assert lines[3][:2] == ["Y", "1"] and float.fromhex(lines[3][2]) == 2.0
    assert lines[4] == ["O", "1", "0"] and lines[5][:4] == ["F", "1", "1", "1"]


def test_nan_residual_stops_not_converged(driver):
    lines = driver(5, 10, TOL, "O 0.5\nB 1.0\nS 1 0.5 0.5\nS 2 0.25 0.5 0.5\nY\nO nan\n")
    assert lines[-2] == ["O", "1", "0"]
    assert lines[-1][:4] == ["F", "0", "1", "2"] and "nan" in lines[-1][4]


@pytest.mark.parametrize("beta", ["0.0", "nan"])
def test_zero_or_nan_beta_stops_the_column(driver, beta):
    lines = driver(5, 10, TOL, f"O 0.5\nB {beta}\n")
    assert lines[:2] == [["O", "0", "1"], ["B", "0"]]
    assert lines[2][:4] == ["F", "0", "0", "0"] and float.fromhex(lines[2][4]) == 0.5


def test_restart_and_max_outer_bound_the_loops(driver):
    """restart 2: the second step ends the inner loop whatever the residual; max_outer 1: the check before outer step 1 stops.
    The clamps: restart 0 reads 30 (a 30th step is the last), max_outer 0 reads 1."""
    lines = driver(2, 1, TOL, "O 0.5\nB 1.0\nS 1 0.5 0.5\nS 2 0.25 0.5 0.5\nY\nO 0.25\n")
    assert lines[2] == ["S", "1", "1"] and lines[3] == ["S", "2", "0"] and lines[5] == ["O", "1", "0"]
    assert lines[-1][:4] == ["F", "0", "1", "2"]
    steps = "".join(f"S {k + 1} " + " ".join(["0.5"] * (k + 1)) + " 0.5\n" for k in range(30))
    lines = driver(0, 0, TOL, "O 0.5\nB 1.0\n" + steps + "Y\nO 0.25\n")
    assert [l[2] for l in lines if l[0] == "S"] == ["1"] * 29 + ["0"]
    assert lines[-2] == ["O", "1", "0"]
