"""CPU checks for the vbatched expert layer (mpf_lange_vbatched, mpf_gecon_vbatched, mpf_residual_vbatched, mpf_gerfs_vbatched):

  * csrc/vbatch_plan.h's launch groups (refine_chunks: tops, launch limit, workspace cut) and the plan's prefix sums by list position:
    a stand-alone driver (tests/vbatch_plan_refine_driver.cpp, built here with AddressSanitizer and UBSan and run directly) against the
    numpy restatement tests/vbatched_refine_model.py;
  * on tests/batched_refine_blocked_model.py: a halving tree over a block padded to ANY top >= n gives the bits of the tree padded to
    1024 -- the ragged kernels run a matrix in a block sized for a larger neighbour, whose extra rows hold +0 terms."""
import os
import subprocess

import numpy as np
import pytest

import batched_refine_blocked_model as RB
import vbatched_refine_model as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTH_SIDES = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("vbatch_plan_refine") / "vbatch_plan_refine_driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                    os.path.join(ROOT, "tests", "vbatch_plan_refine_driver.cpp")], check=True)

    def run(n, max_launch=VR.MAX_LAUNCH, nrhs=0, limit=0, mode=0):
        text = f"{mode} {len(n)} {max_launch} {nrhs} {limit}\n" + " ".join(str(int(v)) for v in n) + "\n"
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and not out.stderr, out.stderr
        got = {}
        for ln in out.stdout.splitlines():
            key, _, rest = ln.partition(" ")
            got[key] = rest if key == "error" else [int(x) for x in rest.split()]
        got["chunks"] = list(zip(got["chunks"][0::3], got["chunks"][1::3], got["chunks"][2::3]))
        return got
    return run


def check(driver, ns, **kw):
    """The driver's chunks are the model's; consecutive, covering, inside one top, within the limits."""
    ns = sorted(int(v) for v in ns)
    got = driver(ns, **kw)["chunks"]
    assert got == VR.chunks(ns, **kw)
    assert sum((ns[f:f + c] for f, c, _ in got), []) == ns            # concatenating the chunks gives back the list
    at = 0
    for f, c, nmax in got:
        assert f == at and c >= 1 and nmax == ns[f + c - 1]
        assert VR.top_of(ns[f]) == VR.top_of(nmax) and c <= kw.get("max_launch", VR.MAX_LAUNCH)
        assert -(-nmax // 64) * 64 <= max(64, 2 * -(-ns[f] // 64) * 64)   # the block: at most twice the smallest matrix's, at least a wave
        if kw.get("limit", 0) > 0 and c > 1:
            assert sum(VR.cost(v, kw["nrhs"]) for v in ns[f:f + c]) <= kw["limit"]
        at += c
    assert at == len(ns)
    return got


def test_empty_list_and_equal_orders(driver):
    assert check(driver, []) == []
    assert check(driver, [77] * 40) == [(0, 40, 77)]
    assert check(driver, [64] * 3) == [(0, 3, 64)] and check(driver, [65] * 3) == [(0, 3, 65)]


def test_both_sides_of_every_top(driver):
    got = check(driver, BOTH_SIDES * 2)
    assert [(c, nmax) for _, c, nmax in got] == [(8, 64), (6, 128), (6, 256), (6, 512), (6, 1024)]
    assert [VR.top_of(v) for v in (1, 64, 65, 128, 129, 256, 257, 512, 513, 1024)] == [64, 64, 128, 128, 256, 256, 512, 512, 1024, 1024]
    for lo, hi in ((64, 65), (128, 129), (256, 257), (512, 513)):
        assert check(driver, [lo, hi]) == [(0, 1, lo), (1, 1, hi)]
    rng = np.random.default_rng(11)
    check(driver, rng.integers(1, 1025, 500))


def test_a_group_longer_than_one_launch(driver):
    ns = [1] * 40000 + [2] * 30000 + [65] * 5
    got = check(driver, ns)
    assert got == [(0, 1 << 15, 1), (1 << 15, 1 << 15, 2), (1 << 16, 70000 - (1 << 16), 2), (70000, 5, 65)]
    assert [c for _, c, _ in check(driver, [5] * 10 + [100] * 7, max_launch=4)] == [4, 4, 2, 4, 3]


def test_workspace_cut_down_to_one_matrix(driver):
    ns = [60, 61, 62, 63, 64, 64, 64, 100, 100, 100]
    nrhs = 3
    c64, c100 = VR.cost(64, nrhs), VR.cost(100, nrhs)
    assert c64 == 3 * (64 + 1 + 4) and c100 == 3 * (100 + 1 + 7)
    assert check(driver, ns, nrhs=nrhs, limit=VR.LIMIT) == [(0, 7, 64), (7, 3, 100)]                     # the real limit: no cut
    got = check(driver, ns, nrhs=nrhs, limit=2 * c64)                                                   # two of order 64 fit
    assert [c for _, c, _ in got] == [2, 2, 2, 1, 1, 1, 1]
    got = check(driver, ns, nrhs=nrhs, limit=3 * c64)
    assert [c for _, c, _ in got] == [3, 3, 1, 1, 1, 1]
    for limit in (c64, c64 - 1, 1):                                                                     # nothing fits: one matrix each
        assert [c for _, c, _ in check(driver, ns, nrhs=nrhs, limit=limit)] == [1] * len(ns)
    # the launch limit and the workspace limit together, and the limit the entry uses on a shape that needs it
    check(driver, ns * 3, nrhs=nrhs, limit=4 * c64, max_launch=3)
    many = [64] * 1000
    got = check(driver, many, nrhs=512, limit=VR.LIMIT)
    fit = VR.LIMIT // VR.cost(64, 512)
    assert fit == 949 and [c for _, c, _ in got] == [949, 51]


def test_the_plan_lists_every_order_ascending_with_its_prefix_sums(driver):
    """list[zeros .. batch) is in ascending order of n across the classes and the large list, equal orders in the batch's order."""
    rng = np.random.default_rng(5)
    n = [int(v) for v in rng.permutation([0, 0] + BOTH_SIDES * 2 + [8, 9, 16, 17, 32, 33, 48, 49, 96, 97])]
    got = driver(n, mode=1)
    zeros, rest = VR.list_order(n)
    assert got["zeros"] == zeros and got["list"] == rest
    ln = [n[b] for b in zeros + rest]
    assert got["ln"] == ln and ln == sorted(ln)
    assert got["lrow"] == np.concatenate([[0], np.cumsum(ln)]).tolist()
    assert got["ltile"] == np.concatenate([[0], np.cumsum([-(-v // 16) for v in ln])]).tolist()
    assert got["chunks"] == VR.chunks(ln[len(zeros):])
    only_zeros = driver([0, 0, 0], mode=1)
    assert only_zeros["chunks"] == [] and only_zeros["lrow"] == [0, 0, 0, 0]


@pytest.mark.parametrize("n", BOTH_SIDES + [3, 15, 16, 17, 31, 32, 33])
def test_a_tree_padded_to_any_block_is_the_tree_padded_to_1024(n):
    """The terms of a matrix of order n in a block of any whole number of waves >= n, the rest +0: the halving tree over 1024 positions
    (what the kernels run: levels 512 .. 64 over the waves, 32 .. 1 inside a wave) has the bits of the tree over the next power of two
    and of the tree over every top above it -- so no bit moves when the block is sized for a larger matrix of the launch."""
    rng = np.random.default_rng(900 + n)
    v = np.abs(rng.standard_normal((n, 7))) * 2.0 ** rng.integers(-30, 30, (n, 7))
    v[rng.integers(0, n), 3] = 0.0
    want = RB.tree_sum(v)
    p2 = 1 << max(0, (n - 1).bit_length())
    for pad in sorted({p2, *[t for t in VR.TOPS if t >= n], 1024}):
        got = RB.tree_sum(v, pad_to=pad)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), pad
    # a block of `threads` rows: rows n .. threads-1 are explicit +0 terms of the 1024-tree
    for threads in sorted({-(-n // 64) * 64, *[t for t in VR.TOPS if t >= n], 256 if n <= 256 else 1024}):
        blk = np.zeros((threads, 7))
        blk[:n] = v
        assert np.array_equal(RB.tree_sum(blk).view(np.uint64), want.view(np.uint64)), threads
    # and a NaN term stays a NaN in every padding
    v[n // 2, 0] = np.nan
    for pad in {p2, 1024}:
        assert np.isnan(RB.tree_sum(v, pad_to=pad)[0]) and not np.isnan(RB.tree_sum(v, pad_to=pad)[1:]).any()
