"""A/B of two builds of the library on the blocked batched probes: merges the outputs of tools/batched_blocked_probe.py and
tools/batched_blocked_inv_probe.py, each run four times in the order parent, new, parent, new (MPF_LIB / MPF_PROBE_LIB name the
build), into one file of ratios.  Per point (n, batch, quantity):
  parent_ms   the two parent runs; their relative difference is the point's run-to-run spread
  new_ms      the two runs of the new build
  ratio       mean(new) / mean(parent) -- the reference is the parent's build, never the new one
  box         max(0.02, spread): the project's +-2 % box or the parent's own spread, whichever is wider
  verdict     "within" (|ratio - 1| <= box), "faster" or "slower"; "noise" when the parent runs disagree by more than 5 %
  repeat      for a point that was "noise" or "slower": the same figures from a second session (REPEAT_DIR), when it has the point
Usage: python tools/batched_blocked_ab.py DIR [REPEAT_DIR] [out.json]
       DIR holds blocked_{parent1,new1,parent2,new2}.json and inv_{parent1,new1,parent2,new2}.json"""
import json
import os
import sys

BLOCKED = [("getrf_unfused", lambda r: r["unfused"]["getrf_ms"]), ("getrf_fused", lambda r: r["fused"]["getrf_ms"]),
           ("getrs_nrhs1", lambda r: r["getrs_nrhs1_trans0_ms"]), ("getrs_nrhs1_trans", lambda r: r["getrs_nrhs1_trans1_ms"]),
           ("getrs_nrhs8", lambda r: r["getrs_nrhs8_trans0_ms"]), ("getrs_nrhs8_trans", lambda r: r["getrs_nrhs8_trans1_ms"]),
           ("stage_panel", lambda r: r["stages_fused"]["panel_ms"]), ("stage_row_block", lambda r: r["stages_fused"]["row_block_ms"]),
           ("stage_update", lambda r: r["stages_fused"]["update_ms"])]
INV = [("getri", lambda r: r["getri_ms"]), ("getri_ct8", lambda r: r["getri_ms_ct8"]), ("getri_ct16", lambda r: r["getri_ms_ct16"]),
       ("getdet", lambda r: r["getdet_ms"])]


def points_of(d):
    points = []
    for probe, quantities in (("blocked", BLOCKED), ("inv", INV)):
        runs = {}
        for tag in ("parent1", "new1", "parent2", "new2"):
            with open(os.path.join(d, f"{probe}_{tag}.json")) as f:
                runs[tag] = {(r["n"], r["batch"]): r for r in json.load(f)["rows"]}
        for key in runs["parent1"]:
            for name, get in quantities:
                p = [get(runs["parent1"][key]), get(runs["parent2"][key])]
                w = [get(runs["new1"][key]), get(runs["new2"][key])]
                spread = abs(p[0] - p[1]) / min(p)
                ratio = (w[0] + w[1]) / (p[0] + p[1])
                box = max(0.02, spread)
                verdict = "noise" if spread > 0.05 else ("within" if abs(ratio - 1) <= box else ("faster" if ratio < 1 else "slower"))
                points.append({"n": key[0], "batch": key[1], "quantity": name, "parent_ms": p, "new_ms": w, "parent_spread": round(spread, 4),
                               "ratio": round(ratio, 4), "box": round(box, 4), "verdict": verdict})
    return points


def main():
    args = sys.argv[1:]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_path = args.pop() if args[-1].endswith(".json") else os.path.join(root, "profiles", "batched_blocked_shared_ab.json")
    points = points_of(args[0])
    if len(args) > 1:
        again = {(p["n"], p["batch"], p["quantity"]): p for p in points_of(args[1])}
        for p in points:
            r = again.get((p["n"], p["batch"], p["quantity"]))
            if r and p["verdict"] in ("noise", "slower"):
                p["repeat"] = {k: r[k] for k in ("parent_ms", "new_ms", "parent_spread", "ratio", "box", "verdict")}
    final = [p.get("repeat", p)["verdict"] for p in points]
    res = {"order": "parent, new, parent, new; one process at a time; each probe's own timing (device events, median of five)",
           "rule": "ratio = mean(new) / mean(parent); box = max(0.02, parent spread); noise: parent spread > 0.05, repeated once in a later session",
           "count_first_session": {v: sum(1 for p in points if p["verdict"] == v) for v in ("within", "faster", "slower", "noise")},
           "count_after_repeat": {v: final.count(v) for v in ("within", "faster", "slower", "noise")}, "points": points}
    with open(out_path, "w") as f:   # one point per line
        head = json.dumps({k: v for k, v in res.items() if k != "points"}, indent=1)
        f.write(head[:-2] + ',\n "points": [\n' + ",\n".join("  " + json.dumps(p) for p in points) + "\n ]\n}\n")
    print(json.dumps(res["count_first_session"]), json.dumps(res["count_after_repeat"]))
    for p in points:
        if p.get("repeat", p)["verdict"] in ("slower", "noise"):
            print(json.dumps(p))
    print("wrote", out_path)


if __name__ == "__main__":
    main()
