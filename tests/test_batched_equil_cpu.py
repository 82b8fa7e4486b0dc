"""CPU checks of the batched equilibration's numpy model (tests/batched_equil_model.py) and of its one piece of host planning
(batch_args::elements_step, through a stand-alone driver built with AddressSanitizer and UBSan and run directly).

The decisions of dlaqge's rule on the input family are derived, not tuned:
  well      entries in [0.5, 1): every row maximum in [0.5, 1), r = 2, every scaled column maximum in [1, 2): rowcnd, colcnd > 0.5 -> 0.
  rows      rows times 2^k, k in [-40, 40] with both ends present: rowcnd <= 2^-79; the scaled matrix is `well` times 2 -> 1.
  cols      every row holds the 2^40 column, so the row maxima lie within a factor 2; the column maxima spread by 2^80 -> 2.
  both      -> 3.      tiny (well times 2^-1000): amax < DBL_MIN / eps -> rows.      clamp (entries near 2^-1060): r = 2^1022 -> rows.
  order 1   rowcnd = colcnd = 1 whatever the scale: only the amax clause can fire."""
import os
import subprocess

import numpy as np
import pytest

import batched_equil_model as EQ
import lacn2_model as L2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDERS = [1, 2, 7, 8, 9, 33, 130]


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("n", ORDERS)
def test_clean_matrices_agree_with_the_large_matrix_restatement(n):
    fam = EQ.family(n)
    for kind, A in zip(EQ.KINDS, fam):
        if kind in EQ.FLAGGED:
            continue
        got, want = EQ.geequ(A), L2.geequ(A)
        assert got[5] == want[5] == 0
        for g, w in zip(got[:5], want[:5]):
            assert same(np.asarray(g, dtype=np.float64), np.asarray(w, dtype=np.float64)), (kind, n)


@pytest.mark.parametrize("n", ORDERS)
def test_rule_one_decides_as_derived(n):
    fam = EQ.family(n)
    for kind, A in zip(EQ.KINDS, fam):
        eq = EQ.geequ(A)
        _, equed, spread = EQ.laqge(A, eq, 1)
        assert equed == EQ.expected_equed(kind, n), (kind, n)
        if kind == "well":
            assert eq[2] >= 0.5 and eq[3] >= 0.5
        if kind == "clamp":
            assert np.all(eq[0] == 2.0 ** 1022)
        assert EQ.laqge(A, eq, 0)[1] == 0
        assert EQ.laqge(A, eq, 2)[1] == (0 if kind in EQ.FLAGGED else 3)
        for s in spread:                                     # exact powers of two
            assert np.frexp(s)[0] == 0.5


def test_flags():
    n = 9
    fam = dict(zip(EQ.KINDS, EQ.family(n)))
    r, c, rowcnd, colcnd, amax, info = EQ.geequ(fam["zero_row"])
    i = int(np.argmax(np.abs(fam["zero_row"]).max(axis=1) == 0))
    assert info == i + 1 and c is None and colcnd is None and rowcnd == 0.0 and r[i] == 1.0
    r, c, rowcnd, colcnd, amax, info = EQ.geequ(fam["zero_col"])
    j = int(np.argmax(np.abs(fam["zero_col"]).max(axis=0) == 0))
    assert info == n + j + 1 and c is None and colcnd is None and rowcnd >= 0.5
    for kind in ("nan", "inf"):
        r, c, rowcnd, colcnd, amax, info = EQ.geequ(fam[kind])
        assert info == 2 * n + 1 and r is None and c is None and rowcnd is None and colcnd is None
        assert np.isnan(amax) if kind == "nan" else amax == np.inf
        for rule in (0, 1, 2):
            As, equed, spread = EQ.laqge(fam[kind], (r, c, rowcnd, colcnd, amax, info), rule)
            assert equed == 0 and same(As, fam[kind]) and same(spread, np.ones(2))
    assert EQ.geequ(np.zeros((0, 0)))[2:] == (1.0, 1.0, 0.0, 0)


@pytest.mark.parametrize("n", ORDERS)
def test_the_scaling_is_exact(n):
    for kind, A in zip(EQ.KINDS, EQ.family(n)):
        if kind in EQ.FLAGGED or kind == "clamp":            # (clamp: the products leave the subnormal range exactly, checked below)
            continue
        eq = EQ.geequ(A)
        As, equed, _ = EQ.laqge(A, eq, 2)
        assert equed == 3 and same(As / eq[1][None, :] / eq[0][:, None], A), (kind, n)
        assert np.abs(As).max() < 2.0 and np.abs(As).max(axis=0).min() >= 1.0
    A = dict(zip(EQ.KINDS, EQ.family(n)))["clamp"]
    eq = EQ.geequ(A)
    As, _, _ = EQ.laqge(A, eq, 2)
    assert same(As / eq[1][None, :] / eq[0][:, None], A)


def test_lascl2_and_bits():
    rng = np.random.default_rng(3)
    s, V = np.ldexp(1.0, rng.integers(-30, 30, 5)), rng.standard_normal((5, 3))
    assert same(EQ.lascl2(s, V), s[:, None] * V)
    assert same(EQ.lascl2(s, V, 1, 2), V) and same(EQ.lascl2(s, V, 3, 2), s[:, None] * V)
    assert same(EQ.lascl2(s, V[:, 0]), s * V[:, 0])


def test_a_descriptor_is_the_per_matrix_model():
    rng = np.random.default_rng(5)
    mats = [EQ.member(k, n, rng) for k, n in zip(EQ.KINDS, [3, 1, 17, 6, 40, 2, 5, 9, 4, 130])]
    mats.insert(3, np.zeros((0, 0)))
    r, c, rowcnd, colcnd, amax, info, out, equed, spread = EQ.descriptor(mats, rule=1, fill=-7.0)
    at = 0
    for b, M in enumerate(mats):
        n = M.shape[0]
        eq = EQ.geequ(M)
        for got, want in ((r[at:at + n], eq[0]), (c[at:at + n], eq[1])):
            assert same(got, want if want is not None else np.full(n, -7.0))
        for got, want in ((rowcnd[b], eq[2]), (colcnd[b], eq[3]), (amax[b], eq[4])):
            assert same(np.float64(got), np.float64(-7.0 if want is None else want))
        As, q, sp = EQ.laqge(M, eq, 1)
        assert info[b] == eq[5] and equed[b] == q and same(out[b], As) and same(spread[b], sp)
        at += n


def test_the_driver_undoes_a_row_scaling_exactly():
    """D A0 and D B against A0 and B for D = diag(2^k): with equilibrate = 2 the row factors absorb D exactly, so the equilibrated
    systems are the same bits and so is everything computed from them."""
    for n in (1, 5, 33):
        rng = np.random.default_rng(n)
        A0, B = EQ.well_scaled(n, rng), rng.standard_normal((n, 2))
        D = EQ.pow2_diag(n, rng)
        for trans in (False, True):
            a = EQ.gesvx(A0, B, trans=trans, equilibrate=2)
            b = EQ.gesvx(D[:, None] * A0, B if trans else D[:, None] * B, trans=trans, equilibrate=2)
            for k in (1, 3, 4, 5):                            # rcond, berr, info, equed
                assert same(np.asarray(a[k]), np.asarray(b[k])), (n, trans, k)
            if not trans:                                     # X and ferr too: the unscaling is on the column side
                assert same(a[0], b[0]) and same(a[2], b[2])


# ---- batch_args::elements_step under the sanitizers --------------------------------------------------------------------------------------
STEP_TABLE = [
    (f"step {1 << 22} 64", str(1 << 22)),                    # n = 8: the launch limit binds
    (f"step {1 << 22} {128 * 128}", str(((1 << 31) - 1) // (128 * 128))),
    (f"step {1 << 22} {(1 << 31) - 1}", "1"),
    (f"step {1 << 22} {1 << 40}", "1"),                      # never zero
    ("step 8 3", "8"),
    (f"cover 300000 {1 << 22} {128 * 128}", "0:131071 131071:131071 262142:37858 ok"),
    ("cover 0 4 4", "ok"),
    ("cover 5 2 1", "0:2 2:2 4:1 ok"),
]


def test_elements_step_under_the_sanitizers(tmp_path):
    exe = tmp_path / "batch_equil_args_driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                    os.path.join(ROOT, "tests", "batch_equil_args_driver.cpp")], check=True)
    out = subprocess.run([str(exe)], input="".join(q + "\n" for q, _ in STEP_TABLE), capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and not out.stderr, out.stderr
    got = [line.strip() for line in out.stdout.splitlines()]
    assert got == [w for _, w in STEP_TABLE]
