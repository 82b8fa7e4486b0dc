"""mpf_getrf_batched and mpf_getrs_batched at scale on one MI355X: n = 8, 16, 32, 64, 128 with batch n^2 8 bytes = 512 MB of random
matrices (beyond the 256 MB Infinity Cache).  Per size, device time by event pairs around single calls, the median of `reps` after one
warm-up call of every shape (the spread is kept: min and max):
  * getrf_batched, in place on a fresh copy of the matrices each time (the copy is outside the event pair);
  * getrs_batched with nrhs = 1 and nrhs = 8, in place on fresh right-hand sides;
  * a plain device-to-device copy of the same 512 MB -- the same bytes the factorization has to move (every matrix read once and
    written once), so "share" = factorization rate / copy rate is its share of what the memory system gives a streaming kernel;
  * the yardstick: what a caller had before -- mpf_factor_dev with pivot_search = 1 and nb = n, called once per matrix, wall time of 64
    matrices of the batch (after a warm-up matrix), scaled to the batch.
Rates: matrices/s; GB/s of the factorization counted as 16 n^2 batch / t; of the solve as (8 n^2 + 16 n nrhs) batch / t (the factors
read once, the right-hand sides read and written once).
Writes profiles/batched_probe.json.  No rate is a gate: the numbers are the record.
Usage: python tools/batched_probe.py [n,n,...] [out.json] [total MB]"""
import importlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

mpf = importlib.import_module("mixed-precision_lu_factorization_amd")
REPS = 5


def event_ms(prepare, fn, reps=REPS):
    """(median, min, max) device ms of fn() over reps runs, prepare() before each one outside the timed window; one warm-up."""
    prepare()
    fn()
    out = []
    for _ in range(reps):
        prepare()
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
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(root, "profiles", "batched_probe.json")
    total = (int(sys.argv[3]) if len(sys.argv) > 3 else 512) << 20
    ctx = mpf.MPFContext(0)
    res = {"bytes_of_matrices": total, "reps": REPS, "timing": "device events around one call; median (min, max)",
           "getrf_gbs": "16 n^2 batch / t", "getrs_gbs": "(8 n^2 + 16 n nrhs) batch / t", "copy_gbs": "16 n^2 batch / t of a device-to-device copy",
           "yardstick": "mpf_factor_dev(pivot_search = 1, nb = n) once per matrix, wall time of 64 matrices scaled to the batch", "rows": []}
    gen = torch.Generator(device=ctx.device)
    gen.manual_seed(1)
    for n in sizes:
        batch = total // (8 * n * n)
        src = ctx.colmajor_batch(batch, n, n)
        src.copy_(torch.randn((batch, n, n), dtype=torch.float64, device=ctx.device, generator=gen))
        W = ctx.colmajor_batch(batch, n, n)
        ipiv = torch.zeros((batch, n), dtype=torch.int32, device=ctx.device)
        info = torch.zeros(batch, dtype=torch.int32, device=ctx.device)
        fresh = lambda: W.copy_(src)                                                     # noqa: E731
        cp = event_ms(lambda: None, fresh)
        rf = event_ms(fresh, lambda: ctx.getrf_batched(W, overwrite=True, ipiv=ipiv, info=info))
        singular = int(torch.count_nonzero(info))
        row = {"n": n, "batch": batch, "singular": singular,
               "copy_ms": round(cp[0], 4), "copy_gbs": round(16.0 * n * n * batch / cp[0] / 1e6, 1),
               "getrf_ms": round(rf[0], 4), "getrf_ms_min_max": [round(rf[1], 4), round(rf[2], 4)],
               "getrf_matrices_per_s": round(batch / rf[0] * 1e3), "getrf_gbs": round(16.0 * n * n * batch / rf[0] / 1e6, 1),
               "getrf_share_of_copy": round(cp[0] / rf[0], 4)}
        for nrhs in (1, 8):
            B0 = ctx.colmajor_batch(batch, n, nrhs)
            B0.copy_(torch.randn((batch, n, nrhs), dtype=torch.float64, device=ctx.device, generator=gen))
            X = ctx.colmajor_batch(batch, n, nrhs)
            rs = event_ms(lambda: X.copy_(B0), lambda: ctx.getrs_batched(W, ipiv, X, overwrite=True))
            row[f"getrs{nrhs}_ms"] = round(rs[0], 4)
            row[f"getrs{nrhs}_ms_min_max"] = [round(rs[1], 4), round(rs[2], 4)]
            row[f"getrs{nrhs}_matrices_per_s"] = round(batch / rs[0] * 1e3)
            row[f"getrs{nrhs}_gbs"] = round((8.0 * n * n + 16.0 * n * nrhs) * batch / rs[0] / 1e6, 1)
            del B0, X
        # the yardstick: one mpf_factor_dev per matrix
        fresh()
        m = min(64, batch - 1)
        ctx.factor(W[batch - 1], n, pivot_search=1)                                     # warm-up: allocations, code objects
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for b in range(m):
            ctx.factor(W[b], n, pivot_search=1)
        torch.cuda.synchronize()
        per = (time.perf_counter() - t0) * 1e3 / m
        row["factor_dev_ms_per_matrix"] = round(per, 4)
        row["factor_dev_matrices"] = m
        row["factor_dev_ms_scaled_to_batch"] = round(per * batch, 1)
        row["speedup_over_factor_dev_loop"] = round(per * batch / rf[0], 1)
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
        del src, W, ipiv, info
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)
    ctx.close()


if __name__ == "__main__":
    main()
