"""mpf_getrf_batched_blocked and mpf_getrs_batched_blocked on one MI355X: n = 128, 192, 256, 384, 512, 768, 1024 with batch = 1, 16, 64,
256 (capped so that the matrices stay within 512 MB), fused and unfused; the solve with nrhs = 1 and 8.  Device time by event pairs
around ONE call after one warm-up call, on fresh data each time (the copy that restores the data is outside the pair), the median of
five (min and max are kept).  Next to each point:
  * the only route before these entry points, measured in the same run on entry points this change does not touch: a host loop over 64
    matrices of (a) mpf_factor_dev(pivot_search = 1) at its best nb of 32, 64, 128, 256 and (b) mpf_dgetf2_piv on the whole matrix, WALL
    time with one synchronise at the end, reported per matrix ("old_*_ms_per_matrix") -- the old route's time for a batch is that times
    the batch;
  * at n = 128 mpf_getrf_batched on the same batch (the new path forced with batched_blocked_min_n = 0): decides that option's default;
  * the share of a device-to-device copy of the same bytes (copy_ms / getrf_ms);
  * fused = 1: the share of the fp64 MFMA rate (78.6 TFLOP/s, the data sheet's figure) at 2/3 n^3 flops per matrix;
  * which stage dominates: the probe library runs the panel, row-block and update launches of one call alone (option
    batched_blocked_stages = 1, 2, 4), each between its own event pair (on factored data: the times do not depend on the values).
The one condition (launch counts: >= 64 x 1.125 n launches one after the other against about 3 n / nb for the whole batch): at
n = 256, 512, 1024 and batch = 64 the new call must beat the old loop by at least 2 x -- "gate" in the output.
Writes profiles/batched_blocked_probe.json.
Usage: python tools/batched_blocked_probe.py [n,n,...] [out.json]
       python tools/batched_blocked_probe.py nb-sweep [out.json]   the panel widths 8, 16, 32 at n = 24 .. 1024 and batch 16, 64, 256 (ms,
                                                                   "u" unfused / "f" fused + width) -> profiles/batched_blocked_nb_sweep.json:
                                                                   what the automatic width was chosen from"""
import importlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

mpf = importlib.import_module("mixed-precision_lu_factorization_amd")
REPS = 5
CAP = 512 << 20
MFMA_TFLOPS = 78.6
OLD_LOOP = 64


def event_ms(fn, prep=None, reps=REPS):
    """(median, min, max) device ms of fn() over reps runs after one warm-up; prep() before every run, outside the event pair."""
    out = []
    for i in range(reps + 1):
        if prep:
            prep()
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


def old_route(ctx, n, fused, gen):
    """Wall ms per matrix of the two per-matrix loops over OLD_LOOP fresh matrices, one synchronise at the end."""
    src = torch.randn((OLD_LOOP, n, n), dtype=torch.float64, device=ctx.device, generator=gen)
    best = None
    for nb in (32, 64, 128, 256):
        if nb > n:
            continue
        for rep in range(2):                                   # the first pass warms up
            W = [ctx.colmajor(n, n).copy_(src[i]) for i in range(OLD_LOOP)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for w in W:
                ctx.factor(w, nb, pivot_search=1, fused_panel=fused)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / OLD_LOOP
        if best is None or ms < best[0]:
            best = (ms, nb)
    for rep in range(2):
        W = [ctx.colmajor(n, n).copy_(src[i]) for i in range(OLD_LOOP)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for w in W:
            ctx.dgetf2_piv(w, fused=fused)
        torch.cuda.synchronize()
        ms2 = (time.perf_counter() - t0) * 1e3 / OLD_LOOP
    return best[0], best[1], ms2


def nb_sweep(out_path):
    ctx = mpf.MPFContext(0, options={"batched_blocked_min_n": 0})
    gen = torch.Generator(device=ctx.device)
    gen.manual_seed(3)
    rows = []
    for n in (24, 48, 64, 96, 128, 160, 192, 256, 512, 1024):
        for batch in sorted({min(b, CAP // (8 * n * n)) for b in (16, 64, 256)}):
            src = ctx.colmajor_batch(batch, n, n)
            src.copy_(torch.randn((batch, n, n), dtype=torch.float64, device=ctx.device, generator=gen))
            W = ctx.colmajor_batch(batch, n, n)
            ipiv = torch.zeros((batch, n), dtype=torch.int32, device=ctx.device)
            info = torch.zeros(batch, dtype=torch.int32, device=ctx.device)
            row = {"n": n, "batch": batch}
            for fused in (False, True):
                for nb in (8, 16, 32):
                    ctx.set_option("batched_blocked_nb", nb)
                    t = event_ms(lambda: ctx.getrf_batched_blocked(W, fused=fused, overwrite=True, ipiv=ipiv, info=info), prep=lambda: W.copy_(src))
                    row[f"{'f' if fused else 'u'}{nb}"] = r4(t[0])
            rows.append(row)
            print(json.dumps(row), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump({"reps": REPS, "timing": "as batched_blocked_probe.json; getrf ms by panel width", "rows": rows}, f, indent=1)
    print("wrote", out_path)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "nb-sweep":
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        return nb_sweep(sys.argv[2] if len(sys.argv) > 2 else os.path.join(root, "profiles", "batched_blocked_nb_sweep.json"))
    sizes = [int(v) for v in sys.argv[1].split(",")] if len(sys.argv) > 1 else [128, 192, 256, 384, 512, 768, 1024]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(root, "profiles", "batched_blocked_probe.json")
    ctx = mpf.MPFContext(0, options={"batched_blocked_min_n": 0})
    pctx = mpf.MPFContext(0, probe=True, options={"batched_blocked_min_n": 0})
    res = {"reps": REPS, "timing": "device events around one call on fresh data after one warm-up call; median (min, max)",
           "old_route": f"host loop over {OLD_LOOP} matrices, wall time with one synchronise at the end, per matrix",
           "mfma_tflops_assumed": MFMA_TFLOPS, "data_cap_bytes": CAP, "rows": [], "gate": []}
    gen = torch.Generator(device=ctx.device)
    gen.manual_seed(1)
    for n in sizes:
        old = {fused: old_route(ctx, n, fused, gen) for fused in (False, True)}
        for batch0 in (1, 16, 64, 256):
            batch = max(1, min(batch0, CAP // (8 * n * n)))
            src = ctx.colmajor_batch(batch, n, n)
            src.copy_(torch.randn((batch, n, n), dtype=torch.float64, device=ctx.device, generator=gen))
            W = ctx.colmajor_batch(batch, n, n)
            ipiv = torch.zeros((batch, n), dtype=torch.int32, device=ctx.device)
            info = torch.zeros(batch, dtype=torch.int32, device=ctx.device)
            cp = event_ms(lambda: W.copy_(src))
            row = {"n": n, "batch": batch, "batch_asked": batch0, "copy_ms": r4(cp[0])}
            for fused in (False, True):
                f = "fused" if fused else "unfused"
                t = event_ms(lambda: ctx.getrf_batched_blocked(W, fused=fused, overwrite=True, ipiv=ipiv, info=info), prep=lambda: W.copy_(src))
                o = old[fused]
                row[f] = {"getrf_ms": r4(t[0]), "getrf_ms_min_max": [r4(t[1]), r4(t[2])], "share_of_copy": r4(cp[0] / t[0]),
                          "old_factor_dev_ms_per_matrix": r4(o[0]), "old_factor_dev_best_nb": o[1], "old_dgetf2_piv_ms_per_matrix": r4(o[2]),
                          "speedup_over_old_loop": r4(min(o[0], o[2]) * batch / t[0]), "singular": int(torch.count_nonzero(info))}
                if fused:
                    row[f]["share_of_mfma_rate"] = r4(2.0 / 3.0 * n ** 3 * batch / (t[0] * 1e-3) / (MFMA_TFLOPS * 1e12))
                if n == 128:
                    s = event_ms(lambda: ctx.getrf_batched(W, fused=fused, overwrite=True, ipiv=ipiv, info=info), prep=lambda: W.copy_(src))
                    row[f]["getrf_batched_ms"] = r4(s[0])
                if batch0 == 64 and n in (256, 512, 1024):
                    g = {"n": n, "batch": batch, "fused": fused, "new_ms": r4(t[0]), "old_loop_ms": r4(min(o[0], o[2]) * batch),
                         "ratio": r4(min(o[0], o[2]) * batch / t[0])}
                    g["passes"] = g["ratio"] >= 2.0
                    res["gate"].append(g)
            # W now holds the fused factors: the solve, and the stages alone
            for nrhs in (1, 8):
                B0 = ctx.colmajor_batch(batch, n, nrhs)
                B0.copy_(torch.randn((batch, n, nrhs), dtype=torch.float64, device=ctx.device, generator=gen))
                B = ctx.colmajor_batch(batch, n, nrhs)
                for trans in (False, True):
                    t = event_ms(lambda: ctx.getrs_batched_blocked(W, ipiv, B, trans=trans, overwrite=True), prep=lambda: B.copy_(B0))
                    row[f"getrs_nrhs{nrhs}_trans{int(trans)}_ms"] = r4(t[0])
            LUf = W.clone(memory_format=torch.preserve_format)
            stages = {}
            for name, mask in (("panel", 1), ("row_block", 2), ("update", 4)):
                pctx.set_option("batched_blocked_stages", mask)
                t = event_ms(lambda: pctx.getrf_batched_blocked(W, fused=True, overwrite=True, ipiv=ipiv, info=info), prep=lambda: W.copy_(LUf))
                stages[name + "_ms"] = r4(t[0])
            pctx.set_option("batched_blocked_stages", 7)
            stages["dominant"] = max(("panel", "row_block", "update"), key=lambda k: stages[k + "_ms"])
            row["stages_fused"] = stages
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
            del src, W, ipiv, info, LUf
            torch.cuda.empty_cache()
    print(json.dumps(res["gate"]))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)
    ctx.close()
    pctx.close()


if __name__ == "__main__":
    main()
