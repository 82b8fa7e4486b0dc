"""fp64 factorization with the paired bulk phase (option fp64_pair = 1: far columns updated once per panel pair, K = 2 nb) against the
one-level loop (fp64_pair = 0: the launches of the schedule before pairs), interleaved in one process on one matrix; then the hand-over
threshold fp64_pair_min_n.  Device events (mpf_stats.ms_total); LU and IPIV of the two are compared bit for bit.
usage: pair_probe.py [N nb rounds]"""
import importlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
mpf = importlib.import_module("mixed-precision_lu_factorization_amd")
N = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
nb = int(sys.argv[2]) if len(sys.argv) > 2 else 256
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
ctx = mpf.MPFContext(0)
default_min_n = ctx.get_option("fp64_pair_min_n")
A = ctx.matgen(N)
W = torch.empty((N, N), dtype=torch.float64, device=ctx.device).t()


def run(pair, min_n):
    ctx.set_option("fp64_pair", pair)
    ctx.set_option("fp64_pair_min_n", min_n)
    W.copy_(A)
    ipiv, info = ctx.factor(W, nb)
    ctx.synchronize()
    st = ctx.stats()
    return st.ms_total, st.gemm_launches, info, st.hpanel_timeouts, ipiv


run(0, default_min_n); run(1, default_min_n)   # warm-up of both paths
ref = None
for r in range(rounds):
    t0, l0, i0, to0, ip0 = run(0, default_min_n)
    if ref is None:
        ref = (W.clone(), ip0.clone())
    t1, l1, i1, to1, ip1 = run(1, default_min_n)
    same = torch.equal(W, ref[0]) and torch.equal(ip1, ref[1])
    print(f"N={N} nb={nb} round {r}: one-level {t0:.2f} ms ({l0} update launches)  paired {t1:.2f} ms ({l1})  "
          f"{2 / 3 * N ** 3 / t0 / 1e9:.1f} -> {2 / 3 * N ** 3 / t1 / 1e9:.1f} TFLOP/s  info {i0}/{i1} timeouts {to0}/{to1} bits {'identical' if same else 'DIFFER'}", flush=True)
for min_n in (N // 4, 3 * N // 8, N // 2, 5 * N // 8, 3 * N // 4):
    ts = [run(1, min_n)[0] for _ in range(3)]
    print(f"N={N} nb={nb} fp64_pair_min_n={min_n}: {min(ts):.2f} ms (best of 3; {' '.join(f'{t:.2f}' for t in ts)})", flush=True)
