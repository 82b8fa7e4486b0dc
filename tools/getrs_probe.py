"""Blocked multi-right-hand-side solve at scale (default N = 32768, nb = 256) on a diagonally dominant matrix.
For nrhs in {1, 4, 16, 64, 256, 1024}, both factor modes (fp64, fp16) and trans 0 / 1:
  * mpf_getrs against mpf_solve_ir_nrhs / mpf_solve_ir_trans at max_iter = 0 (that baseline also pays one residual per column);
  * mpf_solve_ir_block against the same per-column solves at max_iter = 10, tol = 1e-12 (fp16 factors).
The per-column baselines run up to nrhs = 256 only.  Writes profiles/getrs_probe_n<N>.json.
Usage: python tools/getrs_probe.py [N] [nrhs,nrhs,...] [out.json]"""
import importlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

mpf = importlib.import_module("mixed-precision_lu_factorization_amd")
BASELINE_MAX = 256


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
    nrhs_list = [int(v) for v in sys.argv[2].split(",")] if len(sys.argv) > 2 else [1, 4, 16, 64, 256, 1024]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(root, "profiles", f"getrs_probe_n{n}.json")
    ctx = mpf.MPFContext(0)
    dev = ctx.device
    A = ctx.matgen(n)
    idx = torch.arange(n, device=dev)
    A[idx, idx] += A.sum(dim=1)                               # diagonally dominant
    flop_pass = lambda k: 2.0 * n * n * k                     # one L + U pass (or one residual) over k columns
    res = {"N": n, "nb": 256, "tile_columns": 32,
           "note": "baseline_ms of getrs is mpf_solve_ir_nrhs / mpf_solve_ir_trans at max_iter = 0: one L + U solve AND one "
                   "residual per column; baselines only up to nrhs = 256", "getrs": [], "refine": []}
    gen = torch.Generator(device=dev).manual_seed(7)
    for mode, name in ((0, "fp64"), (1, "fp16")):
        W = A.clone()
        ipiv, info = ctx.factor(W, 256, trailing=mode)
        torch.cuda.synchronize()
        for trans in (0, 1):
            for k in nrhs_list:
                B = torch.rand((k, n), dtype=torch.float64, device=dev, generator=gen).t()
                X = ctx.colmajor(n, k)
                reps = 5 if k <= 64 else 3
                ms = ev_ms(lambda: (X.copy_(B), ctx.getrs(W, ipiv, X, trans=trans, overwrite=True)), reps)
                copy_ms = ev_ms(lambda: X.copy_(B), reps)
                row = {"factors": name, "trans": trans, "nrhs": k, "ms": round(ms - copy_ms, 3),
                       "tflops": round(flop_pass(k) / (ms - copy_ms) / 1e9, 2)}
                if k <= BASELINE_MAX:
                    base = (lambda: ctx.solve_ir_trans(A, W, ipiv, B, max_iter=0)) if trans else \
                        (lambda: ctx.solve_ir_nrhs(A, W, ipiv, B, max_iter=0))
                    row["baseline_ms"] = round(ev_ms(base, 1), 3)
                    row["speedup"] = round(row["baseline_ms"] / row["ms"], 2)
                res["getrs"].append(row)
                print(json.dumps(row), flush=True)
                if mode != 1:
                    continue
                _, st = ctx.solve_ir_block(A, W, ipiv, B, trans=trans)
                ms = ev_ms(lambda: ctx.solve_ir_block(A, W, ipiv, B, trans=trans), 3 if k <= 64 else 1)
                row = {"factors": name, "trans": trans, "nrhs": k, "ms": round(ms, 3),
                       "converged": sum(s.converged for s in st), "max_iterations": max(s.iterations for s in st)}
                if k <= BASELINE_MAX:
                    base = (lambda: ctx.solve_ir_trans(A, W, ipiv, B)) if trans else (lambda: ctx.solve_ir_nrhs(A, W, ipiv, B))
                    row["baseline_ms"] = round(ev_ms(base, 1), 3)
                    row["speedup"] = round(row["baseline_ms"] / row["ms"], 2)
                res["refine"].append(row)
                print(json.dumps(row), flush=True)
        del W
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)
    ctx.close()


if __name__ == "__main__":
    main()
