"""mpf_getri_batched_blocked and mpf_getdet_batched_blocked on one MI355X: n = 128, 192, 256, 384, 512, 768, 1024 with batch = 1, 16,
64, 256 (capped so that the factors stay within 512 MB).  Device time by event pairs around ONE call after one warm-up call, the
median of five (min and max are kept), as tools/batched_blocked_probe.py.  Next to each point:
  * "before", the only route to these inverses before this entry point, measured in the same run on code this change does not touch:
    an identity batch filled on the device and mpf_getrs_batched_blocked with nrhs = n in place on it (fill and solve inside one event
    pair; the solve alone is kept too);
  * the inverse at both tile widths (option batched_blocked_inv_ct = 8, 16) and at the automatic one;
  * the share of a device-to-device copy of the same bytes (copy_ms / getri_ms);
  * the share of the unfused fp64 VALU rate: 2/3 n^3 batch multiply-subtract pairs as two fp64 instructions each against HALF of the
    data sheet's 78.6 TFLOP/s vector rate (which counts a fused multiply-add as two) -- a share of a data-sheet figure that nobody has
    measured here;
  * at n = 128 mpf_getri_batched on the same batch (the new path is forced with batched_blocked_min_n = 0);
  * the determinant against a host loop over mpf_getdet (wall time over min(batch, 64) matrices, one synchronise per call as that
    entry point has it, scaled to the batch).
The design has no stages: one kernel forms a tile of columns from the identity to the stored inverse.
The one gate (operation counts: 2/3 n^3 pairs against n^3, and no identity written): at n = 256, 512, 1024 and batch = 64 the new
inverse must take at most 0.75 x "before" -- "gate" in the output, with both times.
Writes profiles/batched_blocked_inv_probe.json.
Usage: python tools/batched_blocked_inv_probe.py [n,n,...] [out.json]"""
import importlib
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

mpf = importlib.import_module("mixed-precision_lu_factorization_amd")
REPS = 5
CAP = 512 << 20
VALU_TFLOPS = 78.6
DET_LOOP = 64


def event_ms(fn, reps=REPS):
    """(median, min, max) device ms of fn() over reps runs after one warm-up."""
    out = []
    for i in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i:
            out.append(e0.elapsed_time(e1))
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def r4(v):
    return round(v, 4)


def parent_commit(root):
    try:
        return subprocess.run(["git", "-C", root, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return "unknown"


def main():
    sizes = [int(v) for v in sys.argv[1].split(",")] if len(sys.argv) > 1 else [128, 192, 256, 384, 512, 768, 1024]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(root, "profiles", "batched_blocked_inv_probe.json")
    ctx = mpf.MPFContext(0, options={"batched_blocked_min_n": 0})
    res = {"reps": REPS, "timing": "device events around one call after one warm-up call; median (min, max)",
           "before": "identity batch filled on the device + mpf_getrs_batched_blocked(nrhs = n) in place, one event pair; "
                     "code of the parent commit, untouched by this change, timed in the same run",
           "parent": os.environ.get("MPF_PROBE_PARENT") or parent_commit(root),
           "valu_tflops_data_sheet": VALU_TFLOPS, "data_cap_bytes": CAP, "rows": [], "gate": []}
    gen = torch.Generator(device=ctx.device)
    gen.manual_seed(1)
    for n in sizes:
        eye1 = torch.eye(n, dtype=torch.float64, device=ctx.device)
        for batch0 in (1, 16, 64, 256):
            batch = max(1, min(batch0, CAP // (8 * n * n)))
            A = ctx.colmajor_batch(batch, n, n)
            A.copy_(torch.randn((batch, n, n), dtype=torch.float64, device=ctx.device, generator=gen))
            LU, ipiv, info = ctx.getrf_batched_blocked(A, overwrite=True)
            X = ctx.colmajor_batch(batch, n, n)
            B = ctx.colmajor_batch(batch, n, n)
            inf2 = torch.zeros(batch, dtype=torch.int32, device=ctx.device)
            cp = event_ms(lambda: X.copy_(LU))

            def before():
                B.copy_(eye1.expand(batch, n, n))
                ctx.getrs_batched_blocked(LU, ipiv, B, overwrite=True)

            tb = event_ms(before)
            ts = event_ms(lambda: ctx.getrs_batched_blocked(LU, ipiv, B, overwrite=True))
            row = {"n": n, "batch": batch, "batch_asked": batch0, "copy_ms": r4(cp[0]), "before_ms": r4(tb[0]),
                   "before_ms_min_max": [r4(tb[1]), r4(tb[2])], "before_solve_alone_ms": r4(ts[0]), "singular": int(torch.count_nonzero(info))}
            for ct in (8, 16, 0):
                ctx.set_option("batched_blocked_inv_ct", ct)
                t = event_ms(lambda: ctx.getri_batched_blocked(LU, ipiv, out=X, info=inf2))
                row["getri_ms" + (f"_ct{ct}" if ct else "")] = r4(t[0])
                if not ct:
                    row["getri_ms_min_max"] = [r4(t[1]), r4(t[2])]
            t0 = row["getri_ms"]
            before()
            row["same_bits_as_before"] = bool(torch.equal(X.view(torch.int64), B.view(torch.int64)))
            row["ratio_to_before"] = r4(t0 / tb[0])
            row["share_of_copy"] = r4(cp[0] / t0)
            row["share_of_unfused_valu_rate"] = r4(2.0 / 3.0 * n ** 3 * batch * 2 / (t0 * 1e-3) / (VALU_TFLOPS / 2 * 1e12))
            if n == 128:
                s = event_ms(lambda: ctx.getri_batched(LU, ipiv, out=X, info=inf2))
                row["getri_batched_ms"] = r4(s[0])
                row["n128_winner"] = "getri_batched" if s[0] <= t0 else "getri_batched_blocked"
            td = event_ms(lambda: ctx.getdet_batched_blocked(LU, ipiv))
            k = min(batch, DET_LOOP)
            one = [(ctx.colmajor(n, n).copy_(LU[b]), ipiv[b].contiguous()) for b in range(k)]
            for rep in range(2):                                   # the first pass warms up
                torch.cuda.synchronize()
                w0 = time.perf_counter()
                for m, p in one:
                    ctx.getdet(m, p)
                torch.cuda.synchronize()
                loop_ms = (time.perf_counter() - w0) * 1e3 * batch / k
            row["getdet_ms"] = r4(td[0])
            row["getdet_loop_over_mpf_getdet_ms"] = r4(loop_ms)
            if batch0 == 64 and n in (256, 512, 1024):
                g = {"n": n, "batch": batch, "new_ms": r4(t0), "before_ms": r4(tb[0]), "ratio": r4(t0 / tb[0])}
                g["passes"] = g["ratio"] <= 0.75
                res["gate"].append(g)
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
            del A, LU, X, B, one
            torch.cuda.empty_cache()
    print(json.dumps(res["gate"]))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)
    ctx.close()


if __name__ == "__main__":
    main()
