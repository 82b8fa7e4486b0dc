"""Blocked GMRES-IR at scale: mpf_solve_gmres_ir_block against mpf_solve_gmres_ir column by column, on the reference generator's own
matrix with MPF_TRAIL_FP16 factors (nb = 256) -- the input on which classical refinement does not contract.
For N in {8192, 32768} and nrhs in {1, 32, 64}, both at max_outer = 10, restart = 50, tol = 1e-12 on the same factors in one process:
  * block_ms: wall time of one block call (median, min and max over the repetitions after a warm-up call);
  * percol_ms: the sum of nrhs calls of mpf_solve_gmres_ir (the yardstick; one repetition above nrhs = 1 -- it takes seconds);
  * the inner iterations of both, the block call's inner STEPS (the longest column of every outer step) and, from one more block
    call under option timeline, the device time of those steps split into factor solves, residuals and orthogonalisation, with
    what is left of the inner loops' wall time (the read-back per step, the uploads and launch gaps) as `readback_and_gaps_ms`;
  * the relative residual both paths report, the same recomputed by torch's matrix product, the floor 2^-53 || |A| |x| || / ||b|| of
    an fp64 residual, and the residual history of the block call's worst column;
  * the orthogonalisation's bytes: three sweeps over the k + 1 basis vectors of step k, 3 (k + 1) N cols 8 bytes (the second sweep
    reads its rows twice -- update, then dots -- which this count leaves out), and the rate they were moved at.
Writes profiles/gmres_block_probe.json.  Usage: python tools/gmres_block_probe.py [N,N,...] [nrhs,nrhs,...] [out.json] [label of the measured commit]"""
import importlib
import json
import os
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

mpf = importlib.import_module("mixed-precision_lu_factorization_amd")
MAX_OUTER, RESTART, TOL = 10, 50, 1e-12
HBM_PEAK_GBS = 8000.0   # MI355X


def wall_ms(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    out.sort()
    return {"median": round(out[len(out) // 2], 2), "min": round(out[0], 2), "max": round(out[-1], 2), "reps": reps}


def timeline_split(ctx, call):
    """One call under option timeline with stderr (the C library's) caught in a file: the GMRES_TL line."""
    sys.stderr.flush()
    with tempfile.TemporaryFile(mode="w+b") as f:
        saved = os.dup(2)
        ctx.set_option("timeline", 1)
        os.dup2(f.fileno(), 2)
        try:
            call()
            torch.cuda.synchronize()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            ctx.set_option("timeline", 0)
        f.seek(0)
        for line in f.read().decode().splitlines():
            if line.startswith("GMRES_TL "):
                v = line.split()[1:]
                return {"factor_solve_ms": float(v[0]), "residual_ms": float(v[1]), "orthogonalisation_ms": float(v[2]),
                        "inner_wall_ms": float(v[3]), "inner_steps": int(v[4])}
    return None


def main():
    sizes = [int(v) for v in sys.argv[1].split(",")] if len(sys.argv) > 1 else [8192, 32768]
    nrhs_list = [int(v) for v in sys.argv[2].split(",")] if len(sys.argv) > 2 else [1, 32, 64]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(root, "profiles", "gmres_block_probe.json")
    if len(sys.argv) > 4:
        commit = sys.argv[4]
    else:
        try:
            commit = subprocess.run(["git", "-C", root, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
        except OSError:
            commit = ""
    ctx = mpf.MPFContext(0)
    dev = ctx.device
    res = {"measured_on": commit, "device": torch.cuda.get_device_name(0), "nb": 256, "factors": "TRAIL_FP16", "max_outer": MAX_OUTER,
           "restart": RESTART, "tol": TOL, "hbm_peak_GBs": HBM_PEAK_GBS, "rows": []}
    for n in sizes:
        A = ctx.matgen(n)
        W = A.clone()
        ipiv, info = ctx.factor(W, 256, trailing=mpf.TRAIL_FP16)
        torch.cuda.synchronize()
        gen = torch.Generator(device=dev).manual_seed(7)
        for k in nrhs_list:
            B = torch.rand((k, n), dtype=torch.float64, device=dev, generator=gen).t()
            block = lambda: ctx.solve_gmres_ir_block(A, W, ipiv, B, max_outer=MAX_OUTER, restart=RESTART, tol=TOL)
            Xb, st = block()                                   # warm-up (allocations) and the counts
            Xb = Xb.view(n, k).clone()
            row = {"N": n, "nrhs": k, "block_ms": wall_ms(block, 3), "block_converged": sum(s.converged for s in st),
                   "block_inner_iterations": [min(s.inner_iterations for s in st), max(s.inner_iterations for s in st)],
                   "block_outer_iterations": max(s.outer_iterations for s in st)}
            split = timeline_split(ctx, block)
            if split:
                steps = split["inner_steps"]
                dev_ms = split["factor_solve_ms"] + split["residual_ms"] + split["orthogonalisation_ms"]
                split["readback_and_gaps_ms"] = round(split["inner_wall_ms"] - dev_ms, 3)
                split["per_step_ms"] = {key[:-3]: round(split[key] / steps, 4) for key in
                                        ("factor_solve_ms", "residual_ms", "orthogonalisation_ms", "readback_and_gaps_ms", "inner_wall_ms")}
                # bytes of the orthogonalisation: per outer step the inner steps k = 0 .. K - 1 sweep 3 (k + 1) vectors of N x cols;
                # K per outer step is not reported, so the steps are spread evenly over the outer steps that ran an inner loop
                outers = max(1, row["block_outer_iterations"])
                per, extra = divmod(steps, outers)
                vec = sum((K * (K + 1)) // 2 for K in [per + 1] * extra + [per] * (outers - extra))
                cols = k   # (an upper bound: a frozen column is not swept)
                gbytes = 3.0 * vec * n * cols * 8 / 1e9
                split["orthogonalisation_GB"] = round(gbytes, 3)
                split["orthogonalisation_GBs"] = round(gbytes / (split["orthogonalisation_ms"] / 1e3), 1)
                split["orthogonalisation_share_of_step"] = round(split["orthogonalisation_ms"] / split["inner_wall_ms"], 3)
                split["orthogonalisation_fraction_of_hbm_peak"] = round(split["orthogonalisation_GBs"] / HBM_PEAK_GBS, 3)
                row["split"] = split
            stats = []
            Xp = torch.empty_like(Xb)

            def percol():
                stats.clear()
                for j in range(k):
                    x, s1 = ctx.solve_gmres_ir(A, W, ipiv, B[:, j].contiguous(), max_outer=MAX_OUTER, restart=RESTART, tol=TOL)
                    Xp[:, j] = x
                    stats.append(s1)
            if k == 1:
                percol()
            row["percol_ms"] = wall_ms(percol, 3 if k == 1 else 1)
            row["percol_converged"] = sum(s.converged for s in stats)
            row["percol_inner_iterations"] = [min(s.inner_iterations for s in stats), max(s.inner_iterations for s in stats)]
            # what the two paths reached: the residual each reports (its own kernel's), the same residual recomputed by torch's
            # matrix product for both, and the floor of any fp64 residual, 2^-53 || |A| |x| || / ||b||, per column (min, max)
            rng = lambda v: [float(min(v)), float(max(v))]
            nb = torch.linalg.vector_norm(B, dim=0)
            rel_of = lambda X: (torch.linalg.vector_norm(B - A @ X, dim=0) / nb).tolist()
            row["block_rel_residual"] = rng([s.rel_residual for s in st])
            row["percol_rel_residual"] = rng([s.rel_residual for s in stats])
            row["block_rel_residual_by_torch"] = rng(rel_of(Xb))
            row["percol_rel_residual_by_torch"] = rng(rel_of(Xp))
            Aabs = A.abs()
            row["fp64_residual_floor"] = rng((torch.linalg.vector_norm(Aabs @ Xb.abs(), dim=0) / nb * 2.0 ** -53).tolist())
            del Aabs
            worst = max(st, key=lambda s: (s.rel_residual != s.rel_residual, s.rel_residual))
            row["block_worst_column_history"] = list(worst.history[:worst.outer_iterations + 1])
            row["speedup"] = round(row["percol_ms"]["median"] / row["block_ms"]["median"], 2)
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
            os.makedirs(os.path.dirname(out_path), exist_ok=True)
            with open(out_path, "w") as f:
                json.dump(res, f, indent=1)
        del A, W
    print("wrote", out_path)
    ctx.close()


if __name__ == "__main__":
    main()
