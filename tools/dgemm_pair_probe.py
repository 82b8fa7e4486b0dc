"""fp64 update (dgemm_minus) at K = nb against K = 2 nb on the operands the row-major schedule really runs: the transposed problem
on a row-major N x N matrix R (lda = ldc = N), B' = a row-major L image of width K (ldb = K).  m = columns of R the launch covers,
n = rows.  Random data (an all-zero matrix clocks differently).  Per shape: one K = 2 nb launch, and the same flops as two K = nb
launches (what the one-level schedule issues for two consecutive panels).
usage: dgemm_pair_probe.py [N nb]"""
import importlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
mpf = importlib.import_module("mixed-precision_lu_factorization_amd")
ctx = mpf.MPFContext(0)
dev = ctx.device
N = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
nb = int(sys.argv[2]) if len(sys.argv) > 2 else 256
R = torch.randn(N, N, dtype=torch.float64, device=dev)
REPS = 5


def timed(fn):
    fn(); ctx.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


for m, n in ((14336, 28672), (28672, 28672), (14336, 16384), (28672, 16384), (3584, 28672)):
    c0, r0 = N - m, N - n
    k0 = r0 - 2 * nb
    C = R[r0:, c0:].t()                                  # C'(j, i) = R[r0 + i, c0 + j]
    A1, A2, A12 = R[k0:k0 + nb, c0:].t(), R[k0 + nb:r0, c0:].t(), R[k0:r0, c0:].t()
    L1 = (torch.randn(n, nb, dtype=torch.float64, device=dev) / 16).t()       # B'(kk, i) = LT[i * K + kk]
    L2 = (torch.randn(n, nb, dtype=torch.float64, device=dev) / 16).t()
    L12 = (torch.randn(n, 2 * nb, dtype=torch.float64, device=dev) / 16).t()

    def one():
        ctx.dgemm_minus(C, A1, L1); ctx.dgemm_minus(C, A2, L2)

    def pair():
        ctx.dgemm_minus(C, A12, L12)

    t1 = timed(one); t2 = timed(pair); t1b = timed(one); t2b = timed(pair)
    fl = 2.0 * m * n * 2 * nb
    print(f"cols m={m} rows n={n}: 2 x K={nb}: {t1:.3f} / {t1b:.3f} ms = {fl / min(t1, t1b) / 1e9:.1f} TFLOP/s   "
          f"1 x K={2 * nb}: {t2:.3f} / {t2b:.3f} ms = {fl / min(t2, t2b) / 1e9:.1f} TFLOP/s   "
          f"gain {100 * (1 - min(t2, t2b) / min(t1, t1b)):.1f} %", flush=True)
    R.normal_()
