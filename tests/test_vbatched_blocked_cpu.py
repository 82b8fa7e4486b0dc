"""CPU checks of csrc/vbatch_plan.h with the larger limit (mpf_vbatch_create_blocked: the forwarding rule, the small classes, the large
list and its launch groups, the per-step schedule of the ragged blocked factorization): a stand-alone driver
(tests/vbatch_plan_blocked_driver.cpp, built here with AddressSanitizer and UBSan and run directly) against the numpy restatement
tests/vbatched_blocked_model.py.  Also: the old plan() call returns what it returned."""
import os
import subprocess

import numpy as np
import pytest

import vbatched_blocked_model as BM
import vbatched_model as VM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# both sides of every seam (the small limit, the group tops), and orders that are and are not multiples of 8, 16 and 32
SEAMS = [0, 1, 128, 129, 256, 257, 512, 513, 1024]
MULTIPLES = [8, 12, 16, 24, 31, 32, 33, 40, 48, 63, 64, 65, 96, 100, 130, 136, 144, 160, 161, 200, 255, 264, 272, 288, 300, 511, 520, 528,
             544, 777, 1000, 1016, 1023]
ALL = SEAMS + MULTIPLES
MIN_N = [0, 64, 129, 1025]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("vbatch_plan_blocked") / "vbatch_plan_blocked_driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                    os.path.join(ROOT, "tests", "vbatch_plan_blocked_driver.cpp")], check=True)

    def run(n, ld=None, off=None, batch=None, min_n=129, nb=32, mode=1):
        rows = [[mode, len(n) if batch is None else batch, int(ld is not None), int(off is not None), min_n, nb], n]
        rows += [v for v in (ld, off) if v is not None]
        text = "\n".join(" ".join(str(int(x)) for x in r) for r in rows) + "\n"
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=60)
        assert out.returncode == 0 and not out.stderr, out.stderr
        got = {}
        for ln in out.stdout.splitlines():
            key, _, rest = ln.partition(" ")
            got[key] = rest if key == "error" else [int(x) for x in rest.split()]
        return got
    return run


def check(driver, n, ld=None, off=None, min_n=129, nb=32):
    got, want = driver(n, ld, off, min_n=min_n, nb=nb), BM.plan(n, ld, off, min_n)
    assert "error" not in got, got
    assert got["batch"] == [len(n)] and got["total_n"] == [want["total_n"]] and got["extent"] == [want["extent"]]
    assert got["limits"] == [1024, min_n]
    for key in ("ld", "off", "offv"):
        assert got[key] == want[key].tolist(), key
    assert got["zeros"] == want["zeros"] and got["large"] == want["large"]
    for k, members in enumerate(want["classes"]):
        assert got[f"class{k}"] == members, (k, min_n)
        assert got["nmax"][k] == max((n[b] for b in members), default=0)
    for g, members in enumerate(want["groups"]):
        assert got[f"group{g}"] == members, (g, min_n)
        assert got["gnmax"][g] == max((n[b] for b in members), default=0)
        steps = BM.factor_steps([n[b] for b in members], nb)
        assert got.get(f"steps{g}", []) == [v for s in steps for v in s], (g, min_n, nb)
    # every matrix is in exactly one list
    every = got["zeros"] + sum((got[f"class{k}"] for k in range(7)), []) + got["large"]
    assert sorted(every) == list(range(len(n))) and got["large"] == sum((got[f"group{g}"] for g in range(3)), [])
    return got


def test_forwarding_rule_and_groups_depend_on_n_alone():
    assert [BM.is_small(v, 129) for v in (0, 1, 128, 129, 1024)] == [False, True, True, False, False]
    assert [BM.is_small(v, 64) for v in (1, 63, 64, 128)] == [True, True, False, False]
    assert not any(BM.is_small(v, 0) for v in (1, 64, 128))
    assert [BM.is_small(v, 1025) for v in (128, 129, 1024)] == [True, False, False]       # above 128 nothing is small
    assert [BM.group_of(v) for v in (1, 129, 256, 257, 512, 513, 1024)] == [0, 0, 0, 1, 1, 2, 2]


@pytest.mark.parametrize("min_n", MIN_N)
def test_packed_layout_with_every_seam(driver, min_n):
    rng = np.random.default_rng(1)
    n = [int(v) for v in rng.permutation(ALL * 2)]
    got = check(driver, n, min_n=min_n)
    assert got["offv"] == np.concatenate([[0], np.cumsum(n)[:-1]]).tolist()
    assert got["off"] == np.concatenate([[0], np.cumsum(np.square(n))[:-1]]).tolist()
    keys = [(n[b], b) for b in got["large"]]
    assert keys == sorted(keys)                              # ascending n, equal orders in the batch's order
    if min_n == 0:
        assert all(got[f"class{k}"] == [] for k in range(7)) and len(got["large"]) == sum(v > 0 for v in n)
    if min_n >= 129:
        assert all(n[b] > 128 for b in got["large"])
        assert min(n[b] for b in got["group0"]) * 2 > 256    # a launch's block size: at most twice what its smallest matrix needs
    if min_n == 64:
        assert {n[b] for b in got["large"] if n[b] <= 128} == {64, 65, 96, 100, 128}


@pytest.mark.parametrize("nb", [8, 16, 32])
def test_step_schedule(driver, nb):
    """The active suffix and the row count at every panel step, for groups whose orders straddle multiples of the width."""
    n = [129, 130, 136, 144, 160, 161, 192, 255, 256, 256, 257, 300, 512, 513, 520, 1023, 1024, 1, 7, 8, 9, 33]
    for min_n in (0, 129):
        got = check(driver, n, min_n=min_n, nb=nb)
        for g in range(3):
            orders = [n[b] for b in got[f"group{g}"]]
            steps = got.get(f"steps{g}", [])
            assert len(steps) == 3 * -(-max(orders, default=0) // nb)
            for j0, first, rows in zip(steps[0::3], steps[1::3], steps[2::3]):
                assert all(v <= j0 for v in orders[:first]) and all(v > j0 for v in orders[first:])
                assert rows == orders[-1] - j0 and first < len(orders)
            assert steps[:3] == ([0, 0, orders[-1]] if orders else [])      # every matrix is in its group's first launch
    assert BM.factor_steps([5, 5, 40, 41], 8) == [(0, 0, 41), (8, 2, 33), (16, 2, 25), (24, 2, 17), (32, 2, 9), (40, 3, 1)]


def test_explicit_layout(driver):
    rng = np.random.default_rng(2)
    n = [int(v) for v in rng.permutation(SEAMS + [7, 33, 200, 300])]
    ld = [v + int(rng.integers(0, 4)) for v in n]
    slots = rng.permutation(len(n))                       # the matrices lie in another order than the batch's, with gaps
    size, off = 1027 * 1028 + 7, [0] * len(n)
    for b, s in enumerate(slots):
        off[b] = int(s) * size + int(rng.integers(0, 5))
    got = check(driver, n, ld, off)
    assert got["extent"] == [max(o + (v - 1) * l + v for v, l, o in zip(n, ld, off) if v)]
    check(driver, n, ld, None, min_n=0)
    check(driver, n, None, off, min_n=64)


def test_empty_batch_zeros_and_empty_groups(driver):
    got = check(driver, [])
    assert got["total_n"] == [0] and got["large"] == []
    got = check(driver, [0, 0, 0], min_n=0)
    assert got["zeros"] == [0, 1, 2] and got["large"] == []
    got = check(driver, [5, 600, 0, 128, 129])            # nothing of 257 .. 512
    assert got["class0"] == [0] and got["class6"] == [3] and got["group0"] == [4] and got["group1"] == [] and got["group2"] == [1]
    got = check(driver, [5, 600, 0, 128, 129], min_n=0)   # order 0 stays in the list of its own
    assert got["zeros"] == [2] and got["group0"] == [0, 3, 4] and got["group2"] == [1]


@pytest.mark.parametrize("n, ld, off, batch, text", [
    ([3, 1025], None, None, None, "n > 1024 is not a batch-sized matrix: factor it with mpf_factor_dev"),
    ([3, -1], None, None, None, "n must not be negative"),
    ([3, 400], [3, 399], None, None, "leading dimension < n"),
    ([3, 4], None, [0, -1], None, "offset must not be negative"),
    ([3, 400], None, [0, 8], None, "matrices 0 and 1 overlap"),
    ([400, 2, 2], [1000, 2, 2], [0, 100000, 1400], None, "matrices 0 and 2 overlap"),
    ([], None, None, -1, "batch must not be negative"),
])
def test_refusals(driver, n, ld, off, batch, text):
    got = driver(n, ld, off, batch)
    assert text in got.get("error", "") and got["error"].startswith("vbatch_create_blocked: "), got
    if batch is None:
        assert isinstance(BM.plan(n, ld, off), str)


def test_the_old_call_returns_what_it_returned(driver):
    rng = np.random.default_rng(3)
    n = [int(v) for v in rng.permutation([0, 1, 8, 9, 16, 17, 32, 33, 48, 49, 64, 65, 96, 97, 128] * 2)]
    got, want = driver(n, mode=0), VM.plan(n)
    assert got["limits"] == [128, 129] and got["large"] == [] and all(got[f"group{g}"] == [] for g in range(3))
    assert got["zeros"] == want["zeros"] and got["total_n"] == [want["total_n"]] and got["extent"] == [want["extent"]]
    for k, members in enumerate(want["classes"]):
        assert got[f"class{k}"] == members
        assert got["nmax"][k] == max((n[b] for b in members), default=0)
    err = driver([3, 129], mode=0)["error"]
    assert err == "vbatch_create: n > 128 is not a small matrix: factor it with mpf_factor_dev (and solve with mpf_getrs) (matrix 1)"
