"""Expert driver at scale (default N = 32768, nb = 256): forward and transposed L + U solve times on fp64 factors, mpf_gecon's
time and solve count, and BASELINE config 5 (the generator + diag(rowsum) with rows scaled by logspace(0, 8)) through mpf_gesv
and through mpf_gesvx.  Also the rcond estimates of the fp16 / fp16x3 factors of a few matrices (the kappa_max calibration).
Usage: python tools/gesvx_probe.py [N] [nb]"""
import importlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

mpf = importlib.import_module("mixed-precision_lu_factorization_amd")


def ev_ms(fn, reps=5):
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
    nb = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    ctx = mpf.MPFContext(0)
    dev = ctx.device
    res = {"N": n, "nb": nb}
    A = ctx.matgen(n)
    idx = torch.arange(n, device=dev)
    A[idx, idx] += A.sum(dim=1)                               # diagonally dominant: kappa ~ 2
    W = A.clone()
    ipiv, _ = ctx.factor(W, nb)
    xs = torch.ones(n, dtype=torch.float64, device=dev)
    b = A @ xs
    # one solve each way (max_iter = 0: set-up + solve + one residual); the solve alone is the difference to the set-up-only call
    f = ev_ms(lambda: ctx.solve_ir(A, W, ipiv, b, max_iter=0))
    t = ev_ms(lambda: ctx.solve_ir_trans(A, W, ipiv, b, max_iter=0))
    f1 = ev_ms(lambda: ctx.solve_ir(A, W, ipiv, b, max_iter=1, tol=0.0))
    t1 = ev_ms(lambda: ctx.solve_ir_trans(A, W, ipiv, b, max_iter=1, tol=0.0))
    # the difference is one refinement sweep: L + U solve (forward or transposed) + axpy + residual + norm
    res["sweep_forward_ms"] = round(f1 - f, 3)
    res["sweep_trans_ms"] = round(t1 - t, 3)
    res["solve_ir0_call_ms"] = {"forward": round(f, 3), "trans": round(t, 3)}
    anorm = ctx.lange(A, "1")
    for rep in range(2):
        t0 = time.perf_counter()
        rcond, st = ctx.gecon(W, anorm, "1")
        wall = (time.perf_counter() - t0) * 1e3
    res["gecon"] = {"ms": round(st.ms_total, 2), "wall_ms": round(wall, 2), "solves": st.solves, "solves_t": st.solves_t,
                    "iterations": st.iterations, "rcond": rcond}
    res["fp64_factor_ms"] = round(ev_ms(lambda: ctx.factor(W.copy_(A), nb), reps=3), 2)
    # BASELINE config 5
    Ak = (A * torch.logspace(0, 8, n, dtype=torch.float64, device=dev)[:, None]).t().contiguous().t()
    del W
    torch.cuda.empty_cache()
    bk = Ak @ xs
    work = ctx.colmajor(n, n)
    for rep in range(2):
        x, gs, _, _ = ctx.gesv(Ak, bk, nb, work=work)
    res["c5_gesv"] = {"path": gs.path, "ms_total": round(gs.ms_total, 1), "fp16_ir_history": [float(v) for v in list(gs.ir_fp16.history)[:3]],
                      "final_rel_residual": gs.ir_final.rel_residual}
    for rep in range(2):
        x, vs, _, _ = ctx.gesvx(Ak, bk, nb, work=work)
    res["c5_gesvx"] = {"path": vs.path, "equed": vs.equed, "ms_total": round(vs.ms_total, 1), "ms_equilibrate": round(vs.ms_equilibrate, 1),
                       "ms_factor": round(vs.ms_factor, 1), "ms_gecon": round(vs.ms_gecon, 1), "ms_ir": round(vs.ms_ir, 1),
                       "rcond_lowp": vs.rcond_lowp, "ir_history": [float(v) for v in list(vs.ir_final.history)[:vs.ir_final.iterations + 1]],
                       "max_abs_err": float((x - xs).abs().max())}
    x, vs, _, _ = ctx.gesvx(Ak, Ak.t() @ xs, nb, trans=True, work=work)
    res["c5_gesvx_trans"] = {"path": vs.path, "ms_total": round(vs.ms_total, 1), "rel_residual": vs.ir_final.rel_residual}
    # kappa_max calibration: 1 / rcond of the low-precision factors next to whether refinement on them converged
    cal = []
    G = ctx.matgen(n)
    for name, M in (("generator", G), ("c5", Ak)):
        for mode in (1, 2):
            x, vs, _, _ = ctx.gesvx(M, M @ xs, nb, try_fp16=mode, kappa_max=1e300, work=work)
            cal.append({"matrix": name, "try_fp16": mode, "equed": vs.equed, "inv_rcond_lowp": (1 / vs.rcond_lowp) if vs.rcond_lowp else None,
                        "lowp_converged": vs.ir_lowp.converged, "lowp_iterations": vs.ir_lowp.iterations,
                        "lowp_history": [float(v) for v in list(vs.ir_lowp.history)[:4]], "path": vs.path, "ms_total": round(vs.ms_total, 1)})
    res["kappa_max_calibration"] = cal
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
