"""What each factor schedule issues, as mpf_stats counts it: panels, schedule, pivot path, update launches, flops and bytes, the
one-pass blocks of the deferred interchanges, info -- per case, on the generator's matrix.  Bit tests do not see a dropped
count_gemm or a changed number of launches; tests/test_gpu_schedule_counts.py compares a run with the recorded values.
Usage: python tools/schedule_counts.py [out.json]     (default: tests/golden/schedule_counts.json; run it with the library
of the commit whose counts are the reference, and commit the output unchanged)"""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["panels", "superpanel", "lookahead", "pivot_path", "gemm_launches", "gemm_flops", "gemm_bytes", "gemm_big_launches",
          "lazy_onepass_blocks", "info"]
TRAIL_FP64, TRAIL_FP16 = 0, 1


def cases():
    """(name, N, nb, trailing mode, context options): the smallest shapes at which each branch of the schedules is taken."""
    out = []
    for n, nb in ((1536, 256), (2304, 128), (4173, 128)):   # (1536, 256): exactly one pair fits, k5 + 256 = N
        for tag, opts in (("one_lane", {}),
                          ("two_lanes", {"fp64_two_lanes": 256, "chain_pipeline_below": 1024}),   # with a re-split, then the one-lane tail
                          ("pairs", {"fp64_pair": 1, "fp64_pair_min_n": 0}),
                          ("pairs_handover", {"fp64_pair": 1, "fp64_pair_min_n": n // 2})):
            out.append((f"rm_{tag}_{n}_{nb}", n, nb, TRAIL_FP64, dict(opts, fp64_rowmajor_min_n=0)))
    n, nb = 2304, 128                                        # the schedules beside the row-major one
    out.append((f"colmajor_{n}_{nb}", n, nb, TRAIL_FP64, {"fp64_rowmajor": 0}))
    out.append((f"superpanel_fp64_{n}_{nb}", n, nb, TRAIL_FP64, {"superpanel_fp64": 2}))
    out.append((f"safe_pivots_{n}_{nb}", n, nb, TRAIL_FP64, {"safe_pivots": 1}))
    out.append((f"fp16_{n}_{nb}", n, nb, TRAIL_FP16, {}))
    return out


def run_case(mpf, n, nb, trailing, opts):
    c = mpf.MPFContext(0, options=opts)
    try:
        W = c.matgen(n)
        c.factor(W, nb, trailing=trailing)
        c.synchronize()
        s = c.stats()
        return {f: getattr(s, f) for f in FIELDS}
    finally:
        c.close()


def main():
    sys.path.insert(0, ROOT)
    import torch
    mpf = importlib.import_module("mixed-precision_lu_factorization_amd")
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "schedule_counts.json")
    doc = {"num_cus": torch.cuda.get_device_properties(0).multi_processor_count, "cases": {}}
    for name, n, nb, trailing, opts in cases():
        doc["cases"][name] = run_case(mpf, n, nb, trailing, opts)
        print(name, doc["cases"][name], flush=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
