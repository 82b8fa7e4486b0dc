"""fp64 pivot search (mpf_opts.pivot_search = 1) against the existing never-waiting path (pivot_path = 1, what option safe_pivots
selects) on the same matrix and the same tree: N in {4096, 8192, 16384}, nb = 256, fp64 trailing mode.  Both run the generic
schedule; the old one takes its pivots from the fp16 image at two launches per column and then interchanges and factors the panel
in separate passes, the new one does all three in one chain of 1 + 4/32 launches per column on 8-byte elements.
Per size and path: ms_total (median of three runs with the default timers) and the per-phase timers of one more run with
event_timers = 2 (the pivoting panel is booked under ms_dpanel; ms_hpanel is the fp16 pivot kernels).
Writes profiles/pivot64_probe.json.
Usage: python tools/pivot64_probe.py [N,N,...] [out.json]"""
import importlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

mpf = importlib.import_module("mixed-precision_lu_factorization_amd")
NB = 256
PHASES = ("ms_hpanel", "ms_laswp", "ms_dpanel", "ms_trsm", "ms_gemm")


def run(ctx, A, **kw):
    W = A.clone()
    _, info = ctx.factor(W, NB, trailing=mpf.TRAIL_FP64, **kw)
    torch.cuda.synchronize()
    st = ctx.stats()
    return st, info


def main():
    sizes = [int(v) for v in sys.argv[1].split(",")] if len(sys.argv) > 1 else [4096, 8192, 16384]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(root, "profiles", "pivot64_probe.json")
    ctx = mpf.MPFContext(0)
    res = {"nb": NB, "trailing": "fp64", "matrix": "the reference generator's (MPFContext.matgen)",
           "note": "ms_total: median of 3 runs, default timers; phases: one run with event_timers = 2", "rows": []}
    for n in sizes:
        A = ctx.matgen(n)
        row = {"N": n}
        for name, kw in (("pivot_search_1", {"pivot_search": 1}), ("safe_pivots", {"pivot_path": 1})):
            ctx.set_option("event_timers", 1)
            run(ctx, A, **kw)                                       # warm-up: code objects, scratch
            tot = sorted(run(ctx, A, **kw)[0].ms_total for _ in range(3))
            ctx.set_option("event_timers", 2)
            st, info = run(ctx, A, **kw)
            row[name] = {"ms_total": round(tot[1], 3), "ms_total_all": [round(t, 3) for t in tot], "info": info,
                         "pivot_search": int(st.pivot_search), "pivot_path": int(st.pivot_path),
                         "phases": {p: round(getattr(st, p), 3) for p in PHASES}, "ms_total_timed_run": round(st.ms_total, 3)}
        row["ratio"] = round(row["pivot_search_1"]["ms_total"] / row["safe_pivots"]["ms_total"], 3)
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
        del A
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)
    ctx.close()


if __name__ == "__main__":
    main()
