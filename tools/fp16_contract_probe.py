"""How far apart are the two rounding contracts of the fp16 pivot panel?  Option fp16_fused = 0 (contract C2: rounded product, rounded
difference) against 1 (C2f: one fused multiply-add) on the generator's own matrix.

1. Pivots: N in {1024, 2048, 4096}, nb = 256, the three trailing modes -- IPIV entries that differ between the settings, the first
   differing column, and the first panel (of nb columns) that holds a difference.  Everything after the first differing pivot is
   another factorization, so the count says how early the two part, not how "wrong" either is; both runs' info and
   hpanel_timeouts are recorded.
2. Time: the pivot kernel alone (the step operator mpf_hgetf2_pivots, as tools/hp_probe.py times it: device events around `reps`
   launches after a warm-up) at 8192 x 256 in both settings, alternating, three rounds; microseconds per column.  Informational:
   the fused step issues one packed instruction where the other issues two; the column step is bound by its latency chain.

Writes profiles/fp16_contract_probe.json.
Usage: python tools/fp16_contract_probe.py [N,N,...] [out.json]"""
import importlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

mpf = importlib.import_module("mixed-precision_lu_factorization_amd")
NB = 256
MODES = (("fp64", mpf.TRAIL_FP64), ("fp16", mpf.TRAIL_FP16), ("fp16x3", mpf.TRAIL_FP16X3))


def factor(ctx, A, mode, fused):
    W = A.clone()
    ip, info = ctx.factor(W, NB, trailing=mode, fp16_fused=fused)
    torch.cuda.synchronize()
    st = ctx.stats()
    assert st.fp16_fused == fused
    return ip.cpu().numpy(), int(info), int(st.hpanel_timeouts)


def timeit(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    sizes = [int(v) for v in sys.argv[1].split(",")] if len(sys.argv) > 1 else [1024, 2048, 4096]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(root, "profiles", "fp16_contract_probe.json")
    ctx = mpf.MPFContext(0)
    res = {"nb": NB, "matrix": "the reference generator's (MPFContext.matgen)",
           "note": "ipiv_differ: IPIV entries that differ between fp16_fused = 0 and 1; first_column: the first of them (0-based, -1: none)",
           "pivots": [], "time": {}}
    for n in sizes:
        A = ctx.matgen(n)
        for name, mode in MODES:
            p0, i0, t0 = factor(ctx, A, mode, 0)
            p1, i1, t1 = factor(ctx, A, mode, 1)
            d = p0 != p1
            first = int(d.argmax()) if d.any() else -1
            row = {"N": n, "trailing": name, "ipiv_differ": int(d.sum()), "of": n, "first_column": first,
                   "first_panel": first // NB if first >= 0 else -1,
                   "differ_in_first_panel": int(d[:NB].sum()), "info": [i0, i1], "hpanel_timeouts": [t0, t1]}
            res["pivots"].append(row)
            print(json.dumps(row), flush=True)
        del A
    rows, cols, reps = 8192, 256, 20
    P = ctx.matgen(rows)[:, :cols]
    per_col = {0: [], 1: []}
    for _ in range(3):
        for fused in (0, 1):
            ctx.set_option("fp16_fused", fused)
            try:
                ms = timeit(lambda: ctx.hgetf2_pivots(P), reps)
            finally:
                ctx.set_option("fp16_fused", 0)
            per_col[fused].append(round(ms * 1e3 / cols, 4))
    res["time"] = {"rows": rows, "cols": cols, "reps_per_round": reps, "what": "mpf_hgetf2_pivots, device events, us per column, three alternating rounds",
                   "us_per_column_fp16_fused_0": per_col[0], "us_per_column_fp16_fused_1": per_col[1],
                   "median_0": sorted(per_col[0])[1], "median_1": sorted(per_col[1])[1]}
    print(json.dumps(res["time"]), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)
    ctx.close()


if __name__ == "__main__":
    main()
