"""CPU checks of the expert driver's ground work: the numpy restatement of dlacn2 / dgecon (tests/lacn2_model.py) that the
GPU tests hold mpf_gecon to agrees with LAPACK's own dgecon, and the new C structs have the layout their ctypes mirrors say."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lacn2_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases():
    rng = np.random.default_rng(11)
    for n in (1, 2, 5, 37, 120, 300):
        A = rng.uniform(-1, 1, (n, n))
        yield f"random{n}", A
        yield f"rowscaled{n}", A * np.logspace(0, 6, n)[:, None]
        yield f"dominant{n}", A + np.diag(np.abs(A).sum(axis=1) + 1)


@pytest.mark.parametrize("norm", ["1", "I"])
def test_restated_dgecon_matches_lapack(norm):
    sl = pytest.importorskip("scipy.linalg")
    from scipy.linalg import lapack
    for name, A in _cases():
        lu, _ = sl.lu_factor(A)
        anorm = np.linalg.norm(A, 1 if norm == "1" else np.inf)
        want, info = lapack.dgecon(lu, anorm, norm=norm)
        assert info == 0
        got = M.gecon(lu, anorm, norm)
        assert abs(got - want) <= 1e-10 * want, (name, got, want)


def test_restated_dgecon_degenerate_cases():
    lu = np.array([[2.0, 1.0], [0.5, 0.0]])
    assert M.gecon(lu, 3.0) == 0.0          # zero diagonal entry of U
    assert M.gecon(np.eye(3), 0.0) == 0.0   # anorm == 0


def test_restated_geequ_powers_of_two():
    rng = np.random.default_rng(5)
    A = rng.uniform(-1, 1, (40, 40)) * np.logspace(-30, 30, 40)[:, None]
    r, c, rowcnd, colcnd, amax, info = M.geequ(A)
    assert info == 0
    for v in (r, c):
        assert np.all(np.frexp(v)[0] == 0.5)
    S = np.abs(A * r[:, None])
    assert np.all((S.max(axis=1) >= 1) & (S.max(axis=1) < 2))
    assert amax == np.abs(A).max() and 0 < rowcnd <= 1 and 0 < colcnd <= 1
    A[7] = 0
    assert M.geequ(A)[5] == 8
    A = rng.uniform(-1, 1, (40, 40)); A[:, 11] = 0
    assert M.geequ(A)[5] == 40 + 12


def test_expert_struct_layouts_match_header(mpf, tmp_path):
    """sizeof / offsetof of mpf_gecon_stats and mpf_gesvx_stats as gcc sees include/mpf_c.h == the ctypes mirrors."""
    src = tmp_path / "lay.c"
    src.write_text("""
#include <stdio.h>
#include <stddef.h>
#include "mpf_c.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(mpf_gecon_stats), offsetof(mpf_gecon_stats, ainvnm), offsetof(mpf_gecon_stats, ms_total),
           sizeof(mpf_gesvx_stats), offsetof(mpf_gesvx_stats, rowcnd), offsetof(mpf_gesvx_stats, rcond), offsetof(mpf_gesvx_stats, ir_lowp),
           offsetof(mpf_gesvx_stats, ir_final));
    return 0;
}
""")
    exe = tmp_path / "lay"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    G, X = mpf.MpfGeconStats, mpf.MpfGesvxStats
    assert out == [C.sizeof(G), G.ainvnm.offset, G.ms_total.offset, C.sizeof(X), X.rowcnd.offset, X.rcond.offset, X.ir_lowp.offset,
                   X.ir_final.offset]
