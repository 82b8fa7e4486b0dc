"""CPU checks of csrc/vbatch_plan.h (the host plan of a variable-size batch: validation, prefix sums, overlap test, size classes and their
order): a stand-alone driver (tests/vbatch_plan_driver.cpp, built here with AddressSanitizer and UBSan and run directly) against the
numpy restatement tests/vbatched_model.py."""
import os
import subprocess

import numpy as np
import pytest

import vbatched_model as VM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEAMS = [0, 1, 8, 9, 16, 17, 32, 33, 64, 65, 128]        # both sides of every form's seam
ALL = SEAMS + [48, 49, 96, 97]                           # ... and of the LDS split of the workgroup forms


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("vbatch_plan") / "vbatch_plan_driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                    os.path.join(ROOT, "tests", "vbatch_plan_driver.cpp")], check=True)

    def run(n, ld=None, off=None, batch=None):
        rows = [[len(n) if batch is None else batch, int(ld is not None), int(off is not None)], n] + [v for v in (ld, off) if v is not None]
        text = "\n".join(" ".join(str(int(x)) for x in r) for r in rows) + "\n"
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=60)
        assert out.returncode == 0 and not out.stderr, out.stderr
        got = {}
        for ln in out.stdout.splitlines():
            key, _, rest = ln.partition(" ")
            got[key] = rest if key == "error" else [int(x) for x in rest.split()]
        return got
    return run


def check(driver, n, ld=None, off=None):
    got, want = driver(n, ld, off), VM.plan(n, ld, off)
    assert "error" not in got, got
    assert got["batch"] == [len(n)] and got["total_n"] == [want["total_n"]] and got["extent"] == [want["extent"]]
    for key in ("ld", "off", "offv"):
        assert got[key] == want[key].tolist(), key
    assert got["zeros"] == want["zeros"]
    for k, members in enumerate(want["classes"]):
        assert got[f"class{k}"] == members, k
        assert got["nmax"][k] == max((n[b] for b in members), default=0)
    return got


def test_class_rule_depends_on_n_alone():
    assert [VM.class_of(v) for v in (1, 8, 9, 16, 17, 32, 33, 48, 49, 64, 65, 96, 97, 128)] == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6]


def test_packed_layout_with_every_seam(driver):
    rng = np.random.default_rng(1)
    n = [int(v) for v in rng.permutation(ALL * 3)]
    got = check(driver, n)
    assert got["offv"] == np.concatenate([[0], np.cumsum(n)[:-1]]).tolist()
    assert got["off"] == np.concatenate([[0], np.cumsum(np.square(n))[:-1]]).tolist()
    assert got["extent"] == [int(np.sum(np.square(n)))]
    # inside a class: ascending n, equal orders in the batch's order
    for k in range(len(VM.CLASS_TOP)):
        keys = [(n[b], b) for b in got[f"class{k}"]]
        assert keys == sorted(keys)


def test_explicit_layout(driver):
    rng = np.random.default_rng(2)
    n = [int(v) for v in rng.permutation(ALL * 2)]
    ld = [v + int(rng.integers(0, 4)) for v in n]
    slots = rng.permutation(len(n))                       # the matrices lie in another order than the batch's, with gaps
    size, off = 130 * 131 + 7, [0] * len(n)
    for b, s in enumerate(slots):
        off[b] = int(s) * size + int(rng.integers(0, 5))
    got = check(driver, n, ld, off)
    assert got["extent"] == [max(o + (v - 1) * l + v for v, l, o in zip(n, ld, off) if v)]
    check(driver, n, ld, None)                            # packed with padded leading dimensions
    check(driver, n, None, off)


def test_empty_batch_all_zeros_and_an_empty_class(driver):
    got = check(driver, [])
    assert got["total_n"] == [0] and got["extent"] == [0]
    got = check(driver, [0, 0, 0])
    assert got["zeros"] == [0, 1, 2] and got["extent"] == [0] and all(got[f"class{k}"] == [] for k in range(7))
    got = check(driver, [5, 40, 0, 128, 7])               # nothing of 9 .. 32, 49 .. 96
    assert got["class0"] == [0, 4] and got["class1"] == [] and got["class2"] == [] and got["class3"] == [1] and got["class6"] == [3]
    # a matrix of order 0 has no footprint: its offset may lie inside another matrix
    check(driver, [4, 0], [4, 0], [0, 3])


@pytest.mark.parametrize("n, ld, off, batch, text", [
    ([3, 129], None, None, None, "n > 128 is not a small matrix: factor it with mpf_factor_dev"),
    ([3, -1], None, None, None, "n must not be negative"),
    ([3, 4], [3, 3], None, None, "leading dimension < n"),
    ([3, 4], None, [0, -1], None, "offset must not be negative"),
    ([3, 4], None, [0, 8], None, "matrices 0 and 1 overlap"),
    ([4, 2, 2], [10, 2, 2], [0, 100, 33], None, "matrices 0 and 2 overlap"),   # inside the padded footprint of a matrix that starts earlier
    ([], None, None, -1, "batch must not be negative"),
])
def test_refusals(driver, n, ld, off, batch, text):
    got = driver(n, ld, off, batch)
    assert text in got.get("error", ""), got
    if batch is None:
        assert isinstance(VM.plan(n, ld, off), str)


def test_footprints_that_only_touch_are_accepted(driver):
    got = check(driver, [3, 4, 2], [3, 5, 2], [0, 9, 9 + 3 * 5 + 4])
    assert got["extent"] == [9 + 19 + 4]
    assert "overlap" in driver([3, 4, 2], [3, 5, 2], [0, 9, 9 + 3 * 5 + 3])["error"]
