"""mpf_getri at scale on one MI355X: fp64 factors (nb = 256) of the generator's matrix, N = 4096, 8192, 16384, 32768.
Per size:
  * the median of three mpf_getri runs and its rate over 4/3 N^3 flops;
  * the device time of the three stages (inv(U); X L = inv(U); interchanges) from one run under option timeline (the GETRI_TL line);
  * mpf_getrs on an N x N identity with the same factors -- what a caller had before: once at N = 32768, the median of three below;
  * the ratio of the two.  The bar: at N = 32768 mpf_getri takes at most half of the mpf_getrs time.
Writes profiles/getri_probe.json.
Usage: python tools/getri_probe.py [N,N,...] [out.json]"""
import importlib
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

mpf = importlib.import_module("mixed-precision_lu_factorization_amd")


def wall_ms(fn, reps):
    """Median wall time of fn() over reps runs; fn synchronises (every entry point timed here does)."""
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    out.sort()
    return out[len(out) // 2]


def stage_split(ctx, call):
    """One call under option timeline with stderr (the C library's) caught in a file: the GETRI_TL line."""
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+") as f:
        ctx.set_option("timeline", 1)
        os.dup2(f.fileno(), 2)
        try:
            call()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            ctx.set_option("timeline", 0)
        f.seek(0)
        for line in f:
            if line.startswith("GETRI_TL "):
                return [float(v) for v in line.split()[1:4]]
    return None


def main():
    sizes = [int(v) for v in sys.argv[1].split(",")] if len(sys.argv) > 1 else [4096, 8192, 16384, 32768]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(root, "profiles", "getri_probe.json")
    ctx = mpf.MPFContext(0)
    res = {"nb": 256, "factors": "fp64", "matrix": "generator", "flops": "4/3 N^3",
           "bar": "getri_ms <= 0.5 * getrs_identity_ms at N = 32768", "rows": []}
    for n in sizes:
        W = ctx.matgen(n)
        ipiv, info = ctx.factor(W, 256)
        X = ctx.colmajor(n, n)
        ctx.getri(W, ipiv, out=X)                                      # first call: allocations
        ms = wall_ms(lambda: ctx.getri(W, ipiv, out=X), 3)
        split = stage_split(ctx, lambda: ctx.getri(W, ipiv, out=X))
        X.copy_(torch.eye(n, dtype=torch.float64, device=ctx.device))
        reps = 1 if n >= 32768 else 3
        if reps > 1:
            ctx.getrs(W, ipiv, X, overwrite=True)                      # warm-up on whatever X holds
        base = []
        for _ in range(reps):
            X.copy_(torch.eye(n, dtype=torch.float64, device=ctx.device))
            base.append(wall_ms(lambda: ctx.getrs(W, ipiv, X, overwrite=True), 1))
        base.sort()
        getrs_ms = base[len(base) // 2]
        row = {"N": n, "info": info, "getri_ms": round(ms, 3), "getri_tflops": round(4.0 / 3.0 * n ** 3 / ms / 1e9, 2),
               "stage_ms": {"inv_u": split[0], "times_inv_l": split[1], "interchanges": split[2]} if split else None,
               "getrs_identity_ms": round(getrs_ms, 3), "getrs_runs": reps, "ratio": round(ms / getrs_ms, 4)}
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
        del W, X
        torch.cuda.empty_cache()
    last = res["rows"][-1]
    res["bar_met"] = bool(last["N"] == 32768 and last["ratio"] <= 0.5) if last["N"] == 32768 else None
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)
    ctx.close()


if __name__ == "__main__":
    main()
