"""CPU checks of the fp64 pivot search's ground work: the numpy model (tests/pivot64_model.py) the device's mpf_dgetf2_piv and
pivot_search = 1 are compared with, against LAPACK and against the oracle's no-pivot panel, and the layout of the new fields."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pivot64_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n, nb, seed).  LAPACK's recursive panel rounds differently from the column-by-column model, so near-ties could in principle pick
# another row: these seeds were checked to agree (every case must; none is skipped).
LAPACK_CASES = [(1, 1, 0), (2, 1, 1), (5, 2, 2), (17, 4, 3), (31, 7, 4), (32, 32, 5), (33, 8, 6), (48, 16, 7), (64, 32, 8), (64, 100, 9)]


@pytest.mark.parametrize("n,nb,seed", LAPACK_CASES)
def test_model_agrees_with_lapack(n, nb, seed):
    from scipy.linalg import lu_factor
    A = np.random.default_rng(seed).standard_normal((n, n))
    LU, ipiv = M.factor_piv(A, nb)
    LU_s, piv_s = lu_factor(A)
    want = piv_s.astype(np.int32) + 1
    if n > 1:
        assert np.array_equal(ipiv, want), (ipiv, want)
    assert ipiv[n - 1] == n                                   # the 1 x 1 tail's entry is the identity the caller put there
    scale = np.abs(LU_s).max()
    assert np.abs(LU - LU_s).max() <= 1e-11 * scale
    assert np.abs(np.tril(LU, -1)).max(initial=0.0) <= 1.0
    assert M.plu_residual(A, LU, ipiv) <= 1e-14


@pytest.mark.parametrize("rows,cols,kind", [(1, 1, "normal"), (2, 2, "normal"), (33, 32, "normal"), (70, 40, "ints"), (64, 64, "ints"),
                                            (50, 20, "tiny"), (40, 33, "zero_col")])
def test_model_panel_bits_equal_the_oracle_panel_on_permuted_rows(oracle, rows, cols, kind):
    """Unfused: the pivoting panel == orc_dgetf2_npv on the panel with its rows pre-permuted by the pivots, bit for bit."""
    rng = np.random.default_rng(rows * 131 + cols)
    if kind == "ints":
        P = rng.integers(-3, 4, (rows, cols)).astype(np.float64)      # ties: the first maximum must win
    else:
        P = rng.standard_normal((rows, cols))
    if kind == "tiny":
        P *= 2.0 ** -40
    if kind == "zero_col":
        P[:, cols // 2] = 0.0
    P = np.asfortranarray(P)
    got = P.copy(order="F")
    ipiv, info = M.panel_piv(got, ipiv_offset=7)
    want = M.permute_rows(P, ipiv, ipiv_offset=7)
    with np.errstate(all="ignore"):
        oracle.dgetf2_npv(want)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    if kind == "zero_col":
        assert info == cols // 2 + 1
    elif kind != "ints":
        assert info == 0
    if kind in ("normal", "tiny"):
        assert np.abs(np.tril(got, -1)).max(initial=0.0) <= 1.0


def test_model_first_maximum_and_nan_rule():
    P = np.asfortranarray(np.array([[1.0, 2.0], [-3.0, 1.0], [3.0, 5.0], [np.nan, 1.0]]))
    ipiv, _ = M.panel_piv(P.copy(order="F"))
    assert ipiv[0] == 2                                       # rows 1 and 2 tie at 3: the first wins; the NaN does not
    Z = np.asfortranarray(np.zeros((3, 2)))
    ipiv, info = M.panel_piv(Z)
    assert list(ipiv) == [1, 2] and info == 1


def test_pivot_search_fields_match_header(mpf, tmp_path):
    """mpf_opts.pivot_search / mpf_stats.pivot_search took the reserved words: same offsets, same sizes."""
    src = tmp_path / "lay.c"
    src.write_text("""
#include <stdio.h>
#include <stddef.h>
#include "mpf_c.h"
int main(void) {
    printf("%zu %zu %zu %zu\\n", sizeof(mpf_opts), offsetof(mpf_opts, pivot_search), sizeof(mpf_stats), offsetof(mpf_stats, pivot_search));
    return 0;
}
""")
    exe = tmp_path / "lay"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [C.sizeof(mpf.MpfOpts), mpf.MpfOpts.pivot_search.offset, C.sizeof(mpf.MpfStats), mpf.MpfStats.pivot_search.offset]
    assert out[0] == 32 and out[1] == 28                      # the word after pivot_path, the struct's last
    assert "mpf_dgetf2_piv" in mpf.C_ABI_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "mpf_c.h")).read()
    assert "pivot_fp64" in hdr
