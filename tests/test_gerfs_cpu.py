"""CPU checks of the error bounds' ground work: the layout of mpf_gerfs_stats against its ctypes mirror, and the numpy restatement
of dgerfs (tests/gerfs_model.py) the device's mpf_gerfs is compared with."""
import ctypes as C
import os
import subprocess

import numpy as np

import gerfs_model as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gerfs_stats_layout_matches_header(mpf, tmp_path):
    """sizeof / offsetof as gcc sees include/mpf_c.h == the ctypes mirror in the Python host."""
    src = tmp_path / "lay.c"
    src.write_text("""
#include <stdio.h>
#include <stddef.h>
#include "mpf_c.h"
int main(void) {
    printf("%zu %zu %zu\\n", sizeof(mpf_gerfs_stats), offsetof(mpf_gerfs_stats, ms_total), offsetof(mpf_gerfs_stats, solves));
    return 0;
}
""")
    exe = tmp_path / "lay"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [C.sizeof(mpf.MpfGerfsStats), mpf.MpfGerfsStats.ms_total.offset, mpf.MpfGerfsStats.solves.offset]
    assert "mpf_gerfs" in mpf.C_ABI_SYMBOLS


def test_model_is_self_consistent():
    """63 x 63, both op(A): refinement with exact (numpy) solves ends at berr <= 4 * 2^-53, and ferr bounds the true error (measured
    against a solution refined once in extended precision)."""
    n, nrhs = 63, 5
    rng = np.random.default_rng(63)
    A = rng.uniform(-1, 1, (n, n))
    A[np.arange(n), np.arange(n)] += 2.0
    B = rng.uniform(-1, 1, (n, nrhs)) * np.logspace(-3, 3, nrhs)
    for trans in (False, True):
        Aop = A.T if trans else A
        X0 = np.linalg.solve(Aop, B) * (1 + 1e-6)           # a start that needs a correction
        X, ferr, berr, its, lits = G.gerfs_model(A, lambda v: np.linalg.solve(Aop, v), lambda v: np.linalg.solve(Aop.T, v), B, X0, trans)
        Al = Aop.astype(np.longdouble)
        X_ref = np.linalg.solve(Aop, B)
        X_ref = X_ref + np.linalg.solve(Aop, (B.astype(np.longdouble) - Al @ X_ref.astype(np.longdouble)).astype(np.float64))
        err = np.abs(X - X_ref).max(axis=0) / np.abs(X).max(axis=0)
        assert np.all(berr <= 4 * G.EPS), berr
        assert np.all(err <= ferr), (err, ferr)
        assert np.all(its >= 1) and np.all((lits >= 2) & (lits <= 5))


def test_model_zero_column_and_single_equation():
    """b = 0, x = 0 gives what dgerfs gives: berr = 1 after one (empty) correction, x = 0.  N = 1: dlacn2 stops after one product."""
    n = 8
    A = np.random.default_rng(1).uniform(-1, 1, (n, n)) + 3 * np.eye(n)
    X, ferr, berr, its, lits = G.gerfs_model(A, lambda v: np.linalg.solve(A, v), lambda v: np.linalg.solve(A.T, v), np.zeros((n, 1)),
                                             np.zeros((n, 1)))
    assert berr[0] == 1.0 and its[0] == 1 and not X.any() and 0 < ferr[0] < 1e-290
    A1 = np.array([[4.0]])
    X, ferr, berr, its, lits = G.gerfs_model(A1, lambda v: v / 4.0, lambda v: v / 4.0, np.array([[2.0]]), np.array([[0.5]]))
    assert X[0, 0] == 0.5 and berr[0] == 0.0 and its[0] == 0 and lits[0] == 1
    assert ferr[0] == (2 * G.EPS * 4.0) / 4.0 / 0.5
