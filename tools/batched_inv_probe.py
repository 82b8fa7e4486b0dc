"""mpf_getri_batched and mpf_getdet_batched at scale on one MI355X: n = 8, 16, 32, 64, 128 with batch n^2 8 bytes = 512 MB of factors
(mpf_getrf_batched's, of random matrices; beyond the 256 MB Infinity Cache).  Per size, device time by event pairs around single
calls, the median of `reps` after one warm-up call (min and max are kept):
  * getri_batched into a second 512 MB buffer;
  * getdet_batched;
  * the baseline: what a caller had before these entry points -- fill a batch of identities on the device (zero_ and a fill of the
    diagonals), then mpf_getrs_batched with nrhs = n in place on it.  That code is unchanged, so it is timed in the same run and
    build; the contract guarantees the same bits, which the probe checks on the first and the last 64 matrices of the batch;
  * a plain device-to-device copy of 512 MB: the bytes the inverse has to move (every matrix read once, written once).
Rates: GB/s of the inverse = 16 n^2 batch / t; of the determinant = the bytes a caller would count, 8 n batch / t (what the memory
system moves is a whole sector per diagonal entry).
A form that measures slower than the baseline is not to be shipped for its sizes: "getri_over_baseline" > 1 is the finding to act on.
Writes profiles/batched_inv_probe.json.
Usage: python tools/batched_inv_probe.py [n,n,...] [out.json] [total MB]"""
import importlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

mpf = importlib.import_module("mixed-precision_lu_factorization_amd")
REPS = 5


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
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(root, "profiles", "batched_inv_probe.json")
    total = (int(sys.argv[3]) if len(sys.argv) > 3 else 512) << 20
    ctx = mpf.MPFContext(0)
    res = {"bytes_of_factors": total, "reps": REPS, "timing": "device events around one call; median (min, max)",
           "getri_gbs": "16 n^2 batch / t", "getdet_gbs": "8 n batch / t", "copy_gbs": "16 n^2 batch / t of a device-to-device copy",
           "baseline": "zero_ + fill of the diagonals of a batch of identities, then mpf_getrs_batched(nrhs = n) in place", "rows": []}
    gen = torch.Generator(device=ctx.device)
    gen.manual_seed(1)
    for n in sizes:
        batch = total // (8 * n * n)
        LU = ctx.colmajor_batch(batch, n, n)
        LU.copy_(torch.randn((batch, n, n), dtype=torch.float64, device=ctx.device, generator=gen))
        LU, ipiv, info = ctx.getrf_batched(LU, overwrite=True)
        X = ctx.colmajor_batch(batch, n, n)
        info2 = torch.zeros(batch, dtype=torch.int32, device=ctx.device)
        cp = event_ms(lambda: X.copy_(LU))
        ri = event_ms(lambda: ctx.getri_batched(LU, ipiv, out=X, info=info2))
        keep = torch.cat([X[:64], X[-64:]]).clone()
        dt = event_ms(lambda: ctx.getdet_batched(LU, ipiv))

        def baseline():
            X.zero_()
            X.diagonal(dim1=1, dim2=2).fill_(1.0)
            ctx.getrs_batched(LU, ipiv, X, overwrite=True)

        bl = event_ms(baseline)
        same = bool(torch.equal(torch.cat([X[:64], X[-64:]]).view(torch.int64), keep.view(torch.int64)))
        row = {"n": n, "batch": batch, "singular": int(torch.count_nonzero(info)) + int(torch.count_nonzero(info2)),
               "copy_ms": round(cp[0], 4), "copy_gbs": round(16.0 * n * n * batch / cp[0] / 1e6, 1),
               "getri_ms": round(ri[0], 4), "getri_ms_min_max": [round(ri[1], 4), round(ri[2], 4)],
               "getri_matrices_per_s": round(batch / ri[0] * 1e3), "getri_gbs": round(16.0 * n * n * batch / ri[0] / 1e6, 1),
               "getri_share_of_copy": round(cp[0] / ri[0], 4),
               "baseline_ms": round(bl[0], 4), "baseline_ms_min_max": [round(bl[1], 4), round(bl[2], 4)],
               "getri_over_baseline": round(ri[0] / bl[0], 4), "same_bits_as_baseline": same,
               "getdet_ms": round(dt[0], 4), "getdet_ms_min_max": [round(dt[1], 4), round(dt[2], 4)],
               "getdet_matrices_per_s": round(batch / dt[0] * 1e3), "getdet_gbs": round(8.0 * n * batch / dt[0] / 1e6, 1)}
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
        del LU, X, ipiv, info, info2, keep
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)
    ctx.close()


if __name__ == "__main__":
    main()
