"""mpf_gecon_batched and mpf_gerfs_batched at scale on one MI355X: n = 8, 16, 32, 64, 128 with batch n^2 8 bytes = 512 MB of factors
(mpf_getrf_batched's, of random matrices), as tools/batched_inv_probe.py has it.  Per size, device time by event pairs around single
calls, the median of `reps` after one warm-up call (min and max are kept):
  * gecon_batched ('1' and 'I') against the only route before it: mpf_getri_batched into a second 512 MB buffer, then torch's abs,
    sum and max on the inverses.  The condition stated with the entry: gecon at most 1.10 x getri ALONE on the same batch
    ("gecon1_over_getri", "geconI_over_getri"); a size that misses it is reported as it is;
  * lange_batched ('1');
  * gerfs_batched with nrhs 1 and 8, with and without ferr, on solutions that are already converged (the cost of a clean refinement),
    beside mpf_getrs_batched with the same nrhs;
  * a loop over mpf_gerfs on the first 64 matrices, wall time with a synchronisation at the end, scaled to the batch for the ratio
    "gerfs_loop_over_batched" (per matrix; the condition: > 1).
Writes profiles/batched_refine_probe.json.
Usage: python tools/batched_refine_probe.py [n,n,...] [out.json] [total MB]"""
import importlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

mpf = importlib.import_module("mixed-precision_lu_factorization_amd")
REPS = 5
LOOP = 64


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
    sizes = [int(v) for v in sys.argv[1].split(",")] if len(sys.argv) > 1 else [8, 16, 32, 64, 128]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(root, "profiles", "batched_refine_probe.json")
    total = (int(sys.argv[3]) if len(sys.argv) > 3 else 512) << 20
    ctx = mpf.MPFContext(0)
    res = {"bytes_of_factors": total, "reps": REPS, "timing": "device events around one call; median (min, max)",
           "route_before": "mpf_getri_batched, then torch abs().sum(dim=1).amax(dim=1)",
           "condition": "gecon_ms <= 1.10 getri_ms at every n; gerfs_loop_over_batched > 1", "rows": []}
    gen = torch.Generator(device=ctx.device)
    gen.manual_seed(1)
    for n in sizes:
        batch = total // (8 * n * n)
        A = ctx.colmajor_batch(batch, n, n)
        A.copy_(torch.randn((batch, n, n), dtype=torch.float64, device=ctx.device, generator=gen))
        LU, ipiv, info = ctx.getrf_batched(A)
        X = ctx.colmajor_batch(batch, n, n)
        info2 = torch.zeros(batch, dtype=torch.int32, device=ctx.device)
        ri = event_ms(lambda: ctx.getri_batched(LU, ipiv, out=X, info=info2))
        rt = event_ms(lambda: (ctx.getri_batched(LU, ipiv, out=X, info=info2), X.abs().sum(dim=1).amax(dim=1)))
        del X
        torch.cuda.empty_cache()
        ln = event_ms(lambda: ctx.lange_batched(A, "1"))
        an1, anI = ctx.lange_batched(A, "1"), ctx.lange_batched(A, "I")
        g1 = event_ms(lambda: ctx.gecon_batched(LU, an1, "1"))
        gI = event_ms(lambda: ctx.gecon_batched(LU, anI, "I"))
        rc = ctx.gecon_batched(LU, an1, "1")
        row = {"n": n, "batch": batch, "singular": int(torch.count_nonzero(info)),
               "getri_ms": round(ri[0], 4), "getri_ms_min_max": [round(ri[1], 4), round(ri[2], 4)],
               "route_before_ms": round(rt[0], 4),
               "lange1_ms": round(ln[0], 4),
               "gecon1_ms": round(g1[0], 4), "gecon1_ms_min_max": [round(g1[1], 4), round(g1[2], 4)],
               "geconI_ms": round(gI[0], 4), "geconI_ms_min_max": [round(gI[1], 4), round(gI[2], 4)],
               "gecon1_over_getri": round(g1[0] / ri[0], 4), "geconI_over_getri": round(gI[0] / ri[0], 4),
               "gecon1_over_route_before": round(g1[0] / rt[0], 4),
               "rcond_median": float(rc.median()), "rcond_min": float(rc.min())}
        for nrhs in (1, 8):
            B = ctx.colmajor_batch(batch, n, nrhs)
            B.copy_(torch.randn((batch, n, nrhs), dtype=torch.float64, device=ctx.device, generator=gen))
            Xs = ctx.getrs_batched(LU, ipiv, B)
            W = Xs.clone()
            ts = event_ms(lambda: ctx.getrs_batched(LU, ipiv, W, overwrite=True))
            del W
            _, ferr, berr, its = ctx.gerfs_batched(A, LU, ipiv, B, Xs, overwrite=True)        # converge once; later calls are clean
            tb = event_ms(lambda: ctx.gerfs_batched(A, LU, ipiv, B, Xs, overwrite=True, want_ferr=False))
            tf = event_ms(lambda: ctx.gerfs_batched(A, LU, ipiv, B, Xs, overwrite=True))
            row.update({f"getrs_nrhs{nrhs}_ms": round(ts[0], 4),
                        f"gerfs_nrhs{nrhs}_berr_only_ms": round(tb[0], 4), f"gerfs_nrhs{nrhs}_with_ferr_ms": round(tf[0], 4),
                        f"gerfs_nrhs{nrhs}_berr_only_over_getrs": round(tb[0] / ts[0], 4),
                        f"gerfs_nrhs{nrhs}_with_ferr_over_getrs": round(tf[0] / ts[0], 4),
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
                            f"gerfs_batched_ms_per_matrix_nrhs{nrhs}": round(tf[0] / batch, 7),
                            f"gerfs_loop_over_batched_nrhs{nrhs}": round(per / (tf[0] / batch), 1)})
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
