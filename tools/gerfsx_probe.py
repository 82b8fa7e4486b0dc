"""Extra-precise refinement at scale (N = 8192 and 32768, nb = 256, 32 and 64 columns) on a diagonally dominant matrix.
For both factor modes (fp64, fp16) and trans 0 / 1: the time of one mpf_residual_x next to one pass of the blocked fp64 MFMA residual
(mpf_solve_ir_block at max_iter = 0, which is x0 + one residual, minus mpf_getrs), and the time and the corrections of mpf_gerfsx
(X from mpf_getrs) next to mpf_gerfs (itmax = 10) on the same inputs.  Writes profiles/gerfsx_probe.json.
Usage: python tools/gerfsx_probe.py [out.json] [N ...]"""
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
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "profiles", "gerfsx_probe.json")
    sizes = [int(v) for v in sys.argv[2:]] or [8192, 32768]
    ctx = mpf.MPFContext(0)
    dev = ctx.device
    res = {"nb": 256, "ithresh": 10, "gerfs_itmax": 10, "rows": []}
    for n in sizes:
        A = ctx.matgen(n)
        idx = torch.arange(n, device=dev)
        A[idx, idx] += A.sum(dim=1)                               # diagonally dominant
        gen = torch.Generator(device=dev).manual_seed(7)
        Ball = torch.rand((64, n), dtype=torch.float64, device=dev, generator=gen).t()
        for mode, name in ((0, "fp64"), (1, "fp16")):
            W = A.clone()
            ipiv, info = ctx.factor(W, 256, trailing=mode)
            torch.cuda.synchronize()
            for k in (32, 64):
                B = Ball[:, :k]
                X = ctx.colmajor(n, k)
                for trans in (0, 1):
                    X0 = ctx.getrs(W, ipiv, B, trans=trans)
                    copy_ms = ev_ms(lambda: X.copy_(B), 3)
                    getrs_ms = ev_ms(lambda: (X.copy_(B), ctx.getrs(W, ipiv, X, trans=trans, overwrite=True)), 3) - copy_ms
                    ir0_ms = ev_ms(lambda: ctx.solve_ir_block(A, W, ipiv, B, trans=trans, max_iter=0), 3)
                    resx_ms = ev_ms(lambda: ctx.residual_x(A, X0, B, trans=trans), 3)
                    _, en, ec, st = ctx.gerfsx(A, W, ipiv, B, X0, trans=trans)
                    gerfsx_ms = ev_ms(lambda: (X.copy_(X0), ctx.gerfsx(A, W, ipiv, B, X, trans=trans, overwrite=True)), 3) - copy_ms
                    _, ferr, berr, gst = ctx.gerfs(A, W, ipiv, B, X0, trans=trans, itmax=10)
                    gerfs_ms = ev_ms(lambda: (X.copy_(X0), ctx.gerfs(A, W, ipiv, B, X, trans=trans, itmax=10, overwrite=True)), 3) - copy_ms
                    row = {"N": n, "factors": name, "nrhs": k, "trans": trans, "residual_x_ms": round(resx_ms, 3),
                           "residual_fp64_ms": round(ir0_ms - getrs_ms, 3), "getrs_ms": round(getrs_ms, 3), "gerfsx_ms": round(gerfsx_ms, 3),
                           "gerfsx_corrections_max": max(s.iterations for s in st), "gerfsx_solves_max": max(s.solves for s in st),
                           "gerfsx_converged": sum(s.x_state == 2 for s in st), "err_norm_max": float(en.max()), "err_comp_max": float(ec.max()),
                           "gerfs_ms": round(gerfs_ms, 3), "gerfs_corrections_max": max(s.iterations for s in gst), "gerfs_ferr_max": float(ferr.max())}
                    res["rows"].append(row)
                    print(json.dumps(row), flush=True)
            del W
        del A, Ball
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)
    ctx.close()


if __name__ == "__main__":
    main()
