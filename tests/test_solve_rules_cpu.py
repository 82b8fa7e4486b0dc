"""CPU checks of csrc/solve_rules.h (the refinement stop rule and dlacn2's state machine every solve path drives): a stand-alone
driver (tests/solve_rules_driver.cpp, built here with AddressSanitizer and UBSan and run directly) against the numpy models the
device is compared with, tests/lacn2_model.dlacn2 and the per-column rule of tests/gesvx_block_model.refine_model."""
import os
import subprocess

import numpy as np
import pytest

import gesvx_block_model as M
import lacn2_model as LM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("solve_rules") / "solve_rules_driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                    os.path.join(ROOT, "tests", "solve_rules_driver.cpp")], check=True)

    def run(args, text):
        out = subprocess.run([str(exe), *args], input=text, capture_output=True, text=True, timeout=60)
        assert out.returncode == 0 and not out.stderr, out.stderr
        return dict(line.split(" ", 1) if " " in line else (line, "") for line in out.stdout.splitlines())
    return run


def int_matrix(n, seed):
    """Entries in [-8, 8]: with n a power of two every product and sum of dlacn2 before its final stage is exact in any order.
    seed: of the generator, or the matrix itself as nested lists."""
    if not isinstance(seed, int):
        return np.array(seed, dtype=np.float64).reshape(n, n)
    return np.random.default_rng(seed).integers(-8, 9, (n, n)).astype(np.float64)


def model_lacn2(B):
    """lacn2_model.dlacn2 on x -> B x and x -> B^T x, with what it decided along the way: (est, iter, [j], exit).  j: the rows of
    the unit vectors it multiplied; exit: "n1", or how the loop ended -- "signs" (repeated sign vector), "est" (no growth),
    "itmax" (five iterations) or "jlast" (the argmax came back)."""
    n = B.shape[0]
    xs, ys, zs = [], [], []

    def apply_b(x):
        xs.append(x.copy())
        ys.append(B @ x)
        return ys[-1].copy()

    def apply_bt(x):
        zs.append(B.T @ x)
        return zs[-1].copy()
    est, it = LM.dlacn2(n, apply_b, apply_bt)
    if n == 1:
        return est, it, [], "n1"
    js = [int(np.argmax(x)) for x in xs[1:-1]]
    if len(ys) - 2 == len(zs):   # the last unit vector's product was not followed by a transposed one
        sign = lambda v: np.where(v >= 0, 1.0, -1.0)
        why = "signs" if np.array_equal(sign(ys[-2]), sign(ys[-3])) else "est"
    else:
        why = "itmax" if zs[-1][js[-1]] != np.abs(zs[-1]).max() else "jlast"
    return est, it, js, why


# Five iterations are rare (none in 60 000 seeds at n = 8): this matrix comes from a random search that kept the changes of single
# entries under which model_lacn2 took no fewer iterations.  It walks the unit vectors 0, 7, 4, 1.
FIVE_ITERATIONS = [[-5, 0, -2, 3, 5, 2, -8, 0], [-2, -3, -8, -4, 0, -6, -8, -7], [-4, -6, 7, -6, 0, -3, 0, -6], [0, -2, 7, -4, 8, 2, -4, 0],
                   [-8, 3, -3, 5, -4, -3, 5, -2], [2, -6, 4, -4, 6, 0, 6, 3], [0, -6, -5, -3, 3, -4, 2, 5], [-1, -4, 4, -7, 2, 1, -4, 0]]
# (n, seed, exit): seeds found with model_lacn2 (its iteration count beside them); every exit of the loop is there
LACN2_CASES = [
    (1, 0, "n1"), (1, 3, "n1"),
    (2, 0, "est"), (2, 470, "est"), (2, 1, "signs"), (2, 8, "jlast"), (2, 9, "jlast"),               # 2, 2, 2, 2, 3
    (8, 9, "signs"), (8, 34, "signs"), (8, 20834, "signs"), (8, 0, "jlast"), (8, 28, "jlast"), (8, 2905, "jlast"),   # 2, 3, 4, 2, 3, 4
    (8, FIVE_ITERATIONS, "itmax"),                                                                    # 5
    (64, 0, "jlast"), (64, 1, "jlast"),                                                               # 2, 2
]


@pytest.mark.parametrize("n,seed,why", LACN2_CASES, ids=[f"{c[0]}-{c[1] if isinstance(c[1], int) else 'searched'}-{c[2]}" for c in LACN2_CASES])
def test_lacn2_state_machine_matches_model(driver, n, seed, why):
    """Same iteration count, same unit vectors, same exit as the model; est to 1e-13 relative (exact up to the final stage, whose
    1 + i / (n - 1) vector rounds)."""
    B = int_matrix(n, seed)
    est, it, js, exit_ = model_lacn2(B)
    assert exit_ == why, "the case no longer takes the exit it was chosen for"
    got = driver(["lacn2"], f"{n}\n" + "\n".join(" ".join(repr(float(v)) for v in row) for row in B) + "\n")
    assert int(got["iter"]) == it
    assert [int(v) for v in got["j"].split(",") if v] == js
    assert got["exit"] == why
    assert abs(float.fromhex(got["est"]) - est) <= 1e-13 * est


def test_lacn2_cases_cover_every_exit():
    assert {"signs", "est", "itmax"} <= {c[2] for c in LACN2_CASES}
    assert {1, 2, 8, 64} == {c[0] for c in LACN2_CASES}


H7 = 0.7 * 1.0
# name: (max_iter, tol, scripted relative residuals, expected (iterations, converged, stalled)).  Consecutive values are dyadic or
# within a factor two of each other, so the scripted solve below reproduces them exactly (Sterbenz).
IR_CASES = {
    "converged_at_0": (10, 2.0 ** -40, [2.0 ** -50], (0, 1, 0)),
    "converged_later": (10, 2.0 ** -40, [1.0, 2.0 ** -20, 2.0 ** -45], (2, 1, 0)),
    "max_iter": (3, 2.0 ** -40, [1.0, 0.5, 0.25, 0.125, 0.0625], (3, 0, 0)),
    "max_iter_0": (0, 2.0 ** -40, [0.5, 0.25], (0, 0, 0)),
    "nan": (10, 2.0 ** -40, [1.0, 0.5, float("nan"), 0.25], (2, 0, 0)),
    "stalled": (10, 2.0 ** -40, [1.0, 0.75, 0.5625, 0.5], (2, 0, 1)),
    "stalled_late": (10, 2.0 ** -40, [1.0, 0.25, 0.0625, 0.05, 0.04, 0.03], (4, 0, 1)),
    "one_slow_step_is_no_stall": (10, 2.0 ** -40, [1.0, 0.875, 0.125, 0.109375, 2.0 ** -50], (4, 1, 0)),
    "exactly_0.7_twice_is_no_stall": (10, 2.0 ** -40, [1.0, H7, 0.7 * H7, 2.0 ** -50], (3, 1, 0)),
    "just_above_0.7_twice_stalls": (10, 2.0 ** -40, [1.0, np.nextafter(H7, 1.0), np.nextafter(0.7 * np.nextafter(H7, 1.0), 1.0), 2.0 ** -50],
                                    (2, 0, 1)),
}


def model_ir(script, max_iter, tol):
    """refine_model on the 1 x 1 system 1 * x = 0 with a solve that walks x through -script[k]: ||b|| = 0 reads 1, so the relative
    residual after k corrections is script[k] itself."""
    calls = []

    def solve(V):
        k = len(calls)
        calls.append(k)
        return np.full_like(V, -script[0] if k == 0 else script[k - 1] - script[k])
    _, st = M.refine_model(np.ones((1, 1)), solve, np.zeros((1, 1)), False, max_iter, tol)
    return st[0]


@pytest.mark.parametrize("name", sorted(IR_CASES))
def test_ir_step_matches_refine_model(driver, name):
    """Every field equal, bit for bit: iterations, converged, stalled, rel_residual and the history up to the stop."""
    max_iter, tol, script, (its, conv, stalled) = IR_CASES[name]
    want = model_ir(script, max_iter, tol)
    assert (want["iterations"], want["converged"], want["stalled"]) == (its, conv, stalled)
    hist = [float(v) for v in want["history"]]
    assert [v.hex() for v in hist] == [float(v).hex() for v in script[:its + 1]], "the scripted solve did not reproduce the script"
    got = driver(["ir", str(max_iter), repr(tol)], " ".join(repr(float(v)) for v in script) + "\n")
    assert (int(got["iterations"]), int(got["converged"]), int(got["stalled"])) == (its, conv, stalled)
    same = lambda tok, v: float.fromhex(tok) == v or (v != v and "nan" in tok)
    assert len(got["history"].split()) == len(hist) and all(same(t, v) for t, v in zip(got["history"].split(), hist))
    assert same(got["rel_residual"], hist[-1])
