"""Error bounds for solves at scale (default N = 32768, nb = 256, 64 columns) on a diagonally dominant matrix.
For both factor modes (fp64, fp16) and trans 0 / 1: the time of mpf_gerfs (itmax = 10, X from mpf_getrs) next to mpf_getrs and
mpf_solve_ir_block on the same inputs, with gerfs's solve and residual pass counts, and the ratio
    gerfs / (solves x getrs time + residual passes x one solve_ir_block residual)
where one residual = solve_ir_block at max_iter = 0 (x0 + one residual) minus getrs.  Writes profiles/gerfs_probe_n<N>.json.
Usage: python tools/gerfs_probe.py [N] [nrhs] [out.json]"""
import importlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

mpf = importlib.import_module("mixed-precision_lu_factorization_amd")


def ev_ms(fn, reps):
    """Median device time of fn() over reps runs (HIP events on the current stream)."""
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    out.sort()
    return out[len(out) // 2]


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(root, "profiles", f"gerfs_probe_n{n}.json")
    ctx = mpf.MPFContext(0)
    dev = ctx.device
    A = ctx.matgen(n)
    idx = torch.arange(n, device=dev)
    A[idx, idx] += A.sum(dim=1)                               # diagonally dominant
    gen = torch.Generator(device=dev).manual_seed(7)
    B = torch.rand((k, n), dtype=torch.float64, device=dev, generator=gen).t()
    res = {"N": n, "nb": 256, "nrhs": k, "itmax": 10, "rows": []}
    for mode, name in ((0, "fp64"), (1, "fp16")):
        W = A.clone()
        ipiv, info = ctx.factor(W, 256, trailing=mode)
        torch.cuda.synchronize()
        for trans in (0, 1):
            X0 = ctx.getrs(W, ipiv, B, trans=trans)
            X = ctx.colmajor(n, k)
            copy_ms = ev_ms(lambda: X.copy_(B), 3)
            getrs_ms = ev_ms(lambda: (X.copy_(B), ctx.getrs(W, ipiv, X, trans=trans, overwrite=True)), 3) - copy_ms
            ir0_ms = ev_ms(lambda: ctx.solve_ir_block(A, W, ipiv, B, trans=trans, max_iter=0), 3)
            _, ist = ctx.solve_ir_block(A, W, ipiv, B, trans=trans)
            ir_ms = ev_ms(lambda: ctx.solve_ir_block(A, W, ipiv, B, trans=trans), 3)
            _, ferr, berr, st = ctx.gerfs(A, W, ipiv, B, X0, trans=trans, itmax=10)
            gerfs_ms = ev_ms(lambda: (X.copy_(X0), ctx.gerfs(A, W, ipiv, B, X, trans=trans, itmax=10, overwrite=True)), 3) - copy_ms
            solves, passes = st[0].solves, max(s.iterations for s in st) + 1
            res_ms = ir0_ms - getrs_ms
            row = {"factors": name, "trans": trans, "gerfs_ms": round(gerfs_ms, 3), "getrs_ms": round(getrs_ms, 3),
                   "solve_ir_block_ms": round(ir_ms, 3), "solve_ir_block_iterations": max(s.iterations for s in ist),
                   "residual_ms": round(res_ms, 3), "solves": solves, "residual_passes": passes,
                   "lacn2_iterations_max": max(s.lacn2_iterations for s in st),
                   "ratio": round(gerfs_ms / (solves * getrs_ms + passes * res_ms), 3),
                   "berr_max": float(berr.max()), "ferr_max": float(ferr.max())}
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
        del W
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)
    ctx.close()


if __name__ == "__main__":
    main()
