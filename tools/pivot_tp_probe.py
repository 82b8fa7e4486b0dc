"""Tournament pivoting (mpf_opts.pivot_search = 2) against fp64 partial pivoting (pivot_search = 1) and the never-waiting fp16 path
(pivot_path = 1, what option safe_pivots selects) on the same matrix in one session: N in {4096, 8192, 16384}, nb = 256, fp64
trailing mode.  All three run the generic schedule.  Per 32 columns of a panel pivot_search = 1 takes 33 column-step launches,
pivot_search = 2 takes 1 + ceil(log8(groups of 256 rows)) selections, one interchange of the panel's columns and one no-pivot
factorization; the U row-block and the update right of the sub-panel are the same kernels.
Per size and rule: ms_total (median of three runs with the default timers), the per-phase timers of one more run with
event_timers = 2 (the pivoting panel is booked under ms_dpanel), and -- outside the timed runs -- ||PA - LU||_F / ||A||_F and
max |l_ij| of the factors.
Writes profiles/pivot_tp_probe.json.
Usage: python tools/pivot_tp_probe.py [N,N,...] [out.json] [parent commit]"""
import importlib
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

mpf = importlib.import_module("mixed-precision_lu_factorization_amd")
NB = 256
PHASES = ("ms_hpanel", "ms_laswp", "ms_dpanel", "ms_trsm", "ms_gemm")
RULES = (("pivot_search_2", {"pivot_search": 2}), ("pivot_search_1", {"pivot_search": 1}), ("safe_pivots", {"pivot_path": 1}))


def run(ctx, A, **kw):
    W = A.clone()
    ip, info = ctx.factor(W, NB, trailing=mpf.TRAIL_FP64, **kw)
    torch.cuda.synchronize()
    return ctx.stats(), info, W, ip


def parent_commit(root):
    try:
        return subprocess.run(["git", "-C", root, "rev-parse", "--short", "HEAD"], check=True, capture_output=True, text=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return "unknown"


def main():
    sizes = [int(v) for v in sys.argv[1].split(",")] if len(sys.argv) > 1 else [4096, 8192, 16384]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(root, "profiles", "pivot_tp_probe.json")
    parent = sys.argv[3] if len(sys.argv) > 3 else parent_commit(root)
    ctx = mpf.MPFContext(0)
    res = {"nb": NB, "trailing": "fp64", "matrix": "the reference generator's (MPFContext.matgen)", "parent_commit": parent,
           "note": "ms_total: median of 3 runs, default timers; phases: one run with event_timers = 2; fro_rel_err, max_abs_l: that run's factors",
           "rows": []}
    for n in sizes:
        A = ctx.matgen(n)
        row = {"N": n}
        for name, kw in RULES:
            ctx.set_option("event_timers", 1)
            run(ctx, A, **kw)                                       # warm-up: code objects, scratch
            tot = sorted(run(ctx, A, **kw)[0].ms_total for _ in range(3))
            ctx.set_option("event_timers", 2)
            st, info, W, ip = run(ctx, A, **kw)
            _, fro = ctx.check_plu(A, W, ip)
            row[name] = {"ms_total": round(tot[1], 3), "ms_total_all": [round(t, 3) for t in tot], "info": info,
                         "pivot_search": int(st.pivot_search), "pivot_path": int(st.pivot_path),
                         "phases": {p: round(getattr(st, p), 3) for p in PHASES}, "ms_total_timed_run": round(st.ms_total, 3),
                         "fro_rel_err": float(f"{fro:.3e}"), "max_abs_l": round(float(W.tril(-1).abs().max()), 3)}
            del W
        row["dpanel_ratio_2_over_1"] = round(row["pivot_search_2"]["phases"]["ms_dpanel"] / row["pivot_search_1"]["phases"]["ms_dpanel"], 3)
        row["total_ratio_2_over_1"] = round(row["pivot_search_2"]["ms_total"] / row["pivot_search_1"]["ms_total"], 3)
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
