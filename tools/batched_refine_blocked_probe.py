"""mpf_gecon_batched_blocked and mpf_gerfs_batched_blocked on one MI355X: n = 256, 512, 1024 at batch 64 and one large batch at
n = 256, factors from mpf_getrf_batched_blocked on random matrices, as tools/batched_refine_probe.py has it for n <= 128.  Per case,
device time by event pairs around single calls, the median of `reps` after one warm-up call (min and max are kept):
  * gecon_batched_blocked ('1' and 'I') against the only route before it: mpf_getri_batched_blocked into an n^2 workspace per matrix,
    then torch's abs, sum and amax on the inverses.  Hard condition: gecon < that route ("gecon1_over_route_before",
    "geconI_over_route_before" < 1).  Target, reported: gecon '1' at most 1.10 x getri ALONE ("gecon1_over_getri");
  * lange_batched_blocked ('1' and 'I');
  * gerfs_batched_blocked with nrhs 1 and 8, with and without ferr, on solutions that are already converged (a clean refinement),
    beside mpf_getrs_batched_blocked with the same nrhs; the cost of ferr (with - without) beside getri_batched_blocked;
  * a loop over mpf_gerfs on the first matrices of the batch (one context, the factors already on the device), wall time with a
    synchronisation at the end, per matrix, for the ratio "gerfs_loop_over_batched" (hard condition: > 1, with ferr; the loop always
    computes ferr, so "gerfs_loop_over_batched_berr_only" compares it with the cheaper call as well).
Writes profiles/batched_refine_blocked_probe.json.
Usage: python tools/batched_refine_blocked_probe.py [n:batch,n:batch,...] [out.json]"""
import importlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

mpf = importlib.import_module("mixed-precision_lu_factorization_amd")
REPS = 5
LOOP = 16


def event_ms(fn, reps=REPS):
    """(median, min, max) device ms of fn() over reps runs after one warm-up."""
    fn()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def main():
    cases = sys.argv[1] if len(sys.argv) > 1 else "256:64,512:64,1024:64,256:4096"
    cases = [tuple(int(v) for v in c.split(":")) for c in cases.split(",")]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(root, "profiles", "batched_refine_blocked_probe.json")
    ctx = mpf.MPFContext(0)
    res = {"reps": REPS, "timing": "device events around one call; median (min, max)",
           "route_before": "mpf_getri_batched_blocked, then torch abs().sum(dim=1).amax(dim=1) ('I': sum(dim=2))",
           "condition": "gecon1_over_route_before < 1, geconI_over_route_before < 1, gerfs_loop_over_batched > 1",
           "target": "gecon1_over_getri <= 1.10", "rows": []}
    gen = torch.Generator(device=ctx.device)
    gen.manual_seed(1)
    for n, batch in cases:
        A = ctx.colmajor_batch(batch, n, n)
        A.copy_(torch.randn((batch, n, n), dtype=torch.float64, device=ctx.device, generator=gen))
        LU, ipiv, info = ctx.getrf_batched_blocked(A)
        X = ctx.colmajor_batch(batch, n, n)
        info2 = torch.zeros(batch, dtype=torch.int32, device=ctx.device)
        ri = event_ms(lambda: ctx.getri_batched_blocked(LU, ipiv, out=X, info=info2))
        rt1 = event_ms(lambda: (ctx.getri_batched_blocked(LU, ipiv, out=X, info=info2), X.abs().sum(dim=1).amax(dim=1)))
        rtI = event_ms(lambda: (ctx.getri_batched_blocked(LU, ipiv, out=X, info=info2), X.abs().sum(dim=2).amax(dim=1)))
        del X
        torch.cuda.empty_cache()
        l1 = event_ms(lambda: ctx.lange_batched_blocked(A, "1"))
        lI = event_ms(lambda: ctx.lange_batched_blocked(A, "I"))
        an1, anI = ctx.lange_batched_blocked(A, "1"), ctx.lange_batched_blocked(A, "I")
        g1 = event_ms(lambda: ctx.gecon_batched_blocked(LU, an1, "1"))
        gI = event_ms(lambda: ctx.gecon_batched_blocked(LU, anI, "I"))
        rc = ctx.gecon_batched_blocked(LU, an1, "1")
        row = {"n": n, "batch": batch, "singular": int(torch.count_nonzero(info)),
               "getri_ms": round(ri[0], 4), "getri_ms_min_max": [round(ri[1], 4), round(ri[2], 4)],
               "route_before_1_ms": round(rt1[0], 4), "route_before_I_ms": round(rtI[0], 4),
               "lange1_ms": round(l1[0], 4), "langeI_ms": round(lI[0], 4),
               "gecon1_ms": round(g1[0], 4), "gecon1_ms_min_max": [round(g1[1], 4), round(g1[2], 4)],
               "geconI_ms": round(gI[0], 4), "geconI_ms_min_max": [round(gI[1], 4), round(gI[2], 4)],
               "gecon1_over_getri": round(g1[0] / ri[0], 4), "geconI_over_getri": round(gI[0] / ri[0], 4),
               "gecon1_over_route_before": round(g1[0] / rt1[0], 4), "geconI_over_route_before": round(gI[0] / rtI[0], 4),
               "rcond_median": float(rc.median()), "rcond_min": float(rc.min())}
        for nrhs in (1, 8):
            B = ctx.colmajor_batch(batch, n, nrhs)
            B.copy_(torch.randn((batch, n, nrhs), dtype=torch.float64, device=ctx.device, generator=gen))
            Xs = ctx.getrs_batched_blocked(LU, ipiv, B)
            W = Xs.clone(memory_format=torch.preserve_format)
            ts = event_ms(lambda: ctx.getrs_batched_blocked(LU, ipiv, W, overwrite=True))
            del W
            _, ferr, berr, its = ctx.gerfs_batched_blocked(A, LU, ipiv, B, Xs, overwrite=True)   # converge once; later calls are clean
            tb = event_ms(lambda: ctx.gerfs_batched_blocked(A, LU, ipiv, B, Xs, overwrite=True, want_ferr=False))
            tf = event_ms(lambda: ctx.gerfs_batched_blocked(A, LU, ipiv, B, Xs, overwrite=True))
            row.update({f"getrs_nrhs{nrhs}_ms": round(ts[0], 4),
                        f"gerfs_nrhs{nrhs}_berr_only_ms": round(tb[0], 4), f"gerfs_nrhs{nrhs}_with_ferr_ms": round(tf[0], 4),
                        f"gerfs_nrhs{nrhs}_berr_only_over_getrs": round(tb[0] / ts[0], 4),
                        f"ferr_cost_nrhs{nrhs}_ms": round(tf[0] - tb[0], 4),
                        f"ferr_cost_nrhs{nrhs}_over_getri": round((tf[0] - tb[0]) / ri[0], 4),
                        f"first_call_corrections_max_nrhs{nrhs}": int(its.max()), f"berr_max_nrhs{nrhs}": float(berr.max()),
                        f"ferr_median_nrhs{nrhs}": float(ferr.median())})
            try:
                m = min(LOOP, batch)

                def loop():
                    for b in range(m):
                        ctx.gerfs(A[b], LU[b], ipiv[b], B[b], Xs[b], overwrite=True)

                loop()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                loop()
                torch.cuda.synchronize()
                per = (time.perf_counter() - t0) * 1e3 / m
                row.update({f"gerfs_loop_ms_per_matrix_nrhs{nrhs}": round(per, 4),
                            f"gerfs_batched_ms_per_matrix_nrhs{nrhs}": round(tf[0] / batch, 6),
                            f"gerfs_batched_berr_only_ms_per_matrix_nrhs{nrhs}": round(tb[0] / batch, 6),
                            f"gerfs_loop_over_batched_nrhs{nrhs}": round(per / (tf[0] / batch), 1),
                            f"gerfs_loop_over_batched_berr_only_nrhs{nrhs}": round(per / (tb[0] / batch), 1)})
            except mpf.MPFError as e:
                row[f"gerfs_loop_nrhs{nrhs}"] = "mpf_gerfs refused: " + str(e)
            del B, Xs
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
        del A, LU, ipiv, info, info2
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)
    ctx.close()


if __name__ == "__main__":
    main()
