"""CPU checks of csrc/batch_args.h (the argument rules of the strided batched entry points: size check, strided-operand check, getri's
out-of-place test, the forwarding predicate, the chunks of a long batch, the norm letters, the nrhs / trans refusal, the itmax clamp): a stand-alone driver (tests/batch_args_driver.cpp, built here
with AddressSanitizer and UBSan and run directly) against a literal table.  The texts are the ones the entry points have always
returned; the GPU argument tests (test_gpu_batched*.py) see them through the library."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mixed-precision_lu_factorization_amd", "csrc")

# where each family sends a matrix that is too large (the tails the entries of mpf_batched.cpp pass)
THEN_GETRS = "factor it with mpf_factor_dev (and solve with mpf_getrs)"
THEN_GETRI = "factor it with mpf_factor_dev (and invert with mpf_getri)"
THEN_GETDET = "factor it with mpf_factor_dev (and take the determinant with mpf_getdet)"
USE_LANGE = "use mpf_lange (and mpf_gecon / mpf_gerfs) on one matrix at a time"
USE_GECON = "use mpf_gecon (and mpf_gerfs) on one matrix at a time"
USE_GERFS = "use mpf_gerfs (and mpf_gecon) on one matrix at a time"
USE_ONE = "use mpf_lange, mpf_gecon / mpf_gerfs on one matrix at a time"
TAILS = [THEN_GETRS, THEN_GETRI, THEN_GETDET, USE_LANGE, USE_GECON, USE_GERFS, USE_ONE]

BT_MAX_LAUNCH, BB_MAX_LAUNCH, BR_MAX_UNITS = 1 << 22, 1 << 15, 1 << 30

TABLE = [
    # both limits, every tail
    (f"sizes getrf_batched 128 129 1 {THEN_GETRS}",
     "error getrf_batched: n > 128 is not a small matrix: factor it with mpf_factor_dev (and solve with mpf_getrs)"),
    (f"sizes getdet_batched 128 1025 3 {THEN_GETRS}",
     "error getdet_batched: n > 128 is not a small matrix: factor it with mpf_factor_dev (and solve with mpf_getrs)"),
    (f"sizes lange_batched 128 129 1 {USE_LANGE}",
     "error lange_batched: n > 128 is not a small matrix: use mpf_lange (and mpf_gecon / mpf_gerfs) on one matrix at a time"),
    (f"sizes gecon_batched 128 129 1 {USE_GECON}",
     "error gecon_batched: n > 128 is not a small matrix: use mpf_gecon (and mpf_gerfs) on one matrix at a time"),
    (f"sizes residual_batched 128 129 1 {USE_GERFS}",
     "error residual_batched: n > 128 is not a small matrix: use mpf_gerfs (and mpf_gecon) on one matrix at a time"),
    (f"sizes gerfs_batched 128 200 1 {USE_GERFS}",
     "error gerfs_batched: n > 128 is not a small matrix: use mpf_gerfs (and mpf_gecon) on one matrix at a time"),
    (f"sizes getrf_batched_blocked 1024 1025 1 {THEN_GETRS}",
     "error getrf_batched_blocked: n > 1024 is not a batch-sized matrix: factor it with mpf_factor_dev (and solve with mpf_getrs)"),
    (f"sizes getrs_batched_blocked 1024 4096 2 {THEN_GETRS}",
     "error getrs_batched_blocked: n > 1024 is not a batch-sized matrix: factor it with mpf_factor_dev (and solve with mpf_getrs)"),
    (f"sizes getri_batched_blocked 1024 1025 1 {THEN_GETRI}",
     "error getri_batched_blocked: n > 1024 is not a batch-sized matrix: factor it with mpf_factor_dev (and invert with mpf_getri)"),
    (f"sizes getdet_batched_blocked 1024 1025 1 {THEN_GETDET}",
     "error getdet_batched_blocked: n > 1024 is not a batch-sized matrix: factor it with mpf_factor_dev (and take the determinant with mpf_getdet)"),
    (f"sizes lange_batched_blocked 1024 1025 1 {USE_ONE}",
     "error lange_batched_blocked: n > 1024 is not a batch-sized matrix: use mpf_lange, mpf_gecon / mpf_gerfs on one matrix at a time"),
    (f"sizes gerfs_batched_blocked 1024 1025 1 {USE_ONE}",
     "error gerfs_batched_blocked: n > 1024 is not a batch-sized matrix: use mpf_lange, mpf_gecon / mpf_gerfs on one matrix at a time"),
    # the limits themselves and the empty cases are accepted; a negative n or batch is refused before the limit is looked at
    (f"sizes getrf_batched 128 128 7 {THEN_GETRS}", "ok"),
    (f"sizes getrf_batched_blocked 1024 1024 7 {THEN_GETRS}", "ok"),
    (f"sizes getrf_batched_blocked 1024 129 1 {THEN_GETRS}", "ok"),
    (f"sizes getrf_batched 128 0 0 {THEN_GETRS}", "ok"),
    (f"sizes getrf_batched 128 -1 4 {THEN_GETRS}", "error getrf_batched: n and batch must not be negative"),
    (f"sizes gecon_batched_blocked 1024 4 -1 {USE_ONE}", "error gecon_batched_blocked: n and batch must not be negative"),
    (f"sizes getri_batched 128 -2000 -1 {THEN_GETRS}", "error getri_batched: n and batch must not be negative"),
    # a batch of one has no strides
    ("pivots getrs_batched 5 1 4", "ok"),
    ("pivots getrs_batched 5 2 4", "error getrs_batched: stride of ipiv < n"),
    ("pivots gerfs_batched_blocked 300 2 299", "error gerfs_batched_blocked: stride of ipiv < n"),
    ("pivots getrs_batched 5 2 5", "ok"),
    ("strided getrf_batched A 4 100 5 5 1", "error getrf_batched: leading dimension of A < n"),
    ("strided getri_batched_blocked inv 299 90000 300 300 2", "error getri_batched_blocked: leading dimension of inv < n"),
    ("strided getrs_batched B 6 11 5 2 1", "ok"),
    ("strided getrs_batched B 6 11 5 2 2", "error getrs_batched: stride of B is smaller than one matrix"),
    ("strided getrs_batched B 6 12 5 2 2", "ok"),
    ("strided residual_batched_blocked R 5 0 5 1 1", "ok"),
    # two batches of two 3 x 3 matrices, the first at address 1000 with ld 4 and stride 20: 31 doubles, the last one at 1240
    ("overlap 1000 3 2 4 20 1000 4 20", "1"),
    ("overlap 1000 3 2 4 20 1240 3 9", "1"),
    ("overlap 1000 3 2 4 20 1248 3 9", "0"),
    ("overlap 1000 3 2 4 20 864 3 9", "1"),          # the second (18 doubles) ends on the first's first element ...
    ("overlap 1000 3 2 4 20 856 3 9", "0"),          # ... and just before it
    ("overlap 1000 1 1 1 0 1000 1 0", "1"),
    ("overlap 1000 1 1 1 0 1008 1 0", "0"),
    # forwarding: within the small limit AND below the option
    ("forwards 128 129", "1"), ("forwards 128 128", "0"), ("forwards 127 128", "1"), ("forwards 129 1000", "0"), ("forwards 5 0", "0"),
    ("forwards 1 1", "0"),
    # chunks
    (f"chunks 0 {BT_MAX_LAUNCH}", "-"),
    (f"chunks 1 {BT_MAX_LAUNCH}", "0:1"),
    (f"chunks {BT_MAX_LAUNCH} {BT_MAX_LAUNCH}", "0:4194304"),
    (f"chunks {BT_MAX_LAUNCH + 1} {BT_MAX_LAUNCH}", "0:4194304 4194304:1"),
    (f"chunks 0 {BB_MAX_LAUNCH}", "-"),
    (f"chunks 1 {BB_MAX_LAUNCH}", "0:1"),
    (f"chunks {BB_MAX_LAUNCH} {BB_MAX_LAUNCH}", "0:32768"),
    (f"chunks {BB_MAX_LAUNCH + 1} {BB_MAX_LAUNCH}", "0:32768 32768:1"),
    (f"chunks {2 * BB_MAX_LAUNCH + 5} {BB_MAX_LAUNCH}", "0:32768 32768:32768 65536:5"),
    ("chunks_fail 10 3 3", "0:3 3:3 rc 7"),
    ("chunks_fail 10 3 -1", "0:3 3:3 6:3 9:1 rc 0"),
    # the residual: BR_MAX_UNITS (matrix, column) pairs, at most BT_MAX_LAUNCH matrices
    (f"residual_step {BR_MAX_UNITS} {BT_MAX_LAUNCH} 1", "4194304"),
    (f"residual_step {BR_MAX_UNITS} {BT_MAX_LAUNCH} 256", "4194304"),
    (f"residual_step {BR_MAX_UNITS} {BT_MAX_LAUNCH} 257", "4177983"),
    (f"residual_step {BR_MAX_UNITS} {BT_MAX_LAUNCH} 1024", "1048576"),
    # the bound's workspace: 2^25 doubles over nrhs (n + 1 + ceil(n / 16)) per matrix
    (f"ferr_step {BB_MAX_LAUNCH} 1024 1", "30812"),
    (f"ferr_step {BB_MAX_LAUNCH} 1024 64", "481"),
    (f"ferr_step {BB_MAX_LAUNCH} 129 1", "32768"),
    (f"ferr_step {BB_MAX_LAUNCH} 1024 {1 << 25}", "1"),
    ("chunks 30813 30812", "0:30812 30812:1"),
    ("chunks 1000 481", "0:481 481:481 962:38"),
    # the norm letters, either case: lange 0 / 1 / 2, gecon 0 / 1 ('M' is no norm of the inverse)
    ("lange_mode lange_batched 1", "0"), ("lange_mode lange_batched O", "0"), ("lange_mode lange_batched o", "0"),
    ("lange_mode lange_batched_blocked I", "1"), ("lange_mode lange_batched_blocked i", "1"),
    ("lange_mode lange_vbatched M", "2"), ("lange_mode lange_vbatched m", "2"),
    ("lange_mode lange_batched F", "error lange_batched: norm must be '1', 'O', 'I' or 'M'"),
    ("lange_mode lange_batched_blocked 2", "error lange_batched_blocked: norm must be '1', 'O', 'I' or 'M'"),
    ("lange_mode lange_vbatched X", "error lange_vbatched: norm must be '1', 'O', 'I' or 'M'"),
    ("gecon_mode gecon_batched 1", "0"), ("gecon_mode gecon_batched O", "0"), ("gecon_mode gecon_batched o", "0"),
    ("gecon_mode gecon_batched_blocked I", "1"), ("gecon_mode gecon_vbatched i", "1"),
    ("gecon_mode gecon_batched M", "error gecon_batched: norm must be '1', 'O' or 'I'"),
    ("gecon_mode gecon_batched_blocked m", "error gecon_batched_blocked: norm must be '1', 'O' or 'I'"),
    ("gecon_mode gecon_vbatched 0", "error gecon_vbatched: norm must be '1', 'O' or 'I'"),
    # nrhs before trans; nrhs == 0 is no refusal (the entry returns 0 after it)
    ("nrhs_trans getrs_batched 1 0", "ok"), ("nrhs_trans getrs_batched 1 1", "ok"), ("nrhs_trans getrs_batched 0 0", "ok"),
    ("nrhs_trans getrs_batched 0 1", "ok"),
    ("nrhs_trans getrs_batched 1 -1", "error getrs_batched: trans must be 0 or 1"),
    ("nrhs_trans residual_batched_blocked 1 2", "error residual_batched_blocked: trans must be 0 or 1"),
    ("nrhs_trans gerfs_vbatched 0 2", "error gerfs_vbatched: trans must be 0 or 1"),
    ("nrhs_trans gerfs_batched -1 0", "error gerfs_batched: nrhs must not be negative"),
    ("nrhs_trans getrs_vbatched -1 1", "error getrs_vbatched: nrhs must not be negative"),
    ("nrhs_trans getrs_batched_blocked -1 2", "error getrs_batched_blocked: nrhs must not be negative"),
    ("nrhs_trans residual_vbatched -1 -1", "error residual_vbatched: nrhs must not be negative"),
    # the iteration limit: 5 by default, at most 31
    ("itmax -3", "5"), ("itmax 0", "5"), ("itmax 1", "1"), ("itmax 31", "31"), ("itmax 32", "31"),
]


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    exe = tmp_path_factory.mktemp("batch_args") / "batch_args_driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                    os.path.join(ROOT, "tests", "batch_args_driver.cpp")], check=True)
    out = subprocess.run([str(exe)], input="".join(q + "\n" for q, _ in TABLE), capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and not out.stderr, out.stderr
    return out.stdout.splitlines()


def test_every_answer_matches_the_table(answers):
    assert len(answers) == len(TABLE)
    for (question, want), got in zip(TABLE, answers):
        assert got == want, question


def test_the_table_speaks_of_the_librarys_own_tails_and_limits():
    with open(os.path.join(CSRC, "mpf_batched.cpp")) as f:
        host = f.read()
    for tail in TAILS:
        assert '"' + tail + '"' in host, tail
    with open(os.path.join(CSRC, "mpf_internal.h")) as f:
        internal = f.read()
    for name, value in (("BT_MAX_LAUNCH", BT_MAX_LAUNCH), ("BB_MAX_LAUNCH", BB_MAX_LAUNCH), ("BR_MAX_UNITS", BR_MAX_UNITS)):
        m = re.search(r"constexpr int64_t " + name + r" = 1 << (\d+);", internal)
        assert m and 1 << int(m.group(1)) == value, name
