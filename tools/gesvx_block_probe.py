"""The expert driver for many right-hand sides at scale (default N = 32768, nb = 256, 64 columns), on BASELINE config 5 (the generator +
diag(rowsum), rows scaled by logspace(0, 8)) and on the diagonally dominant matrix itself.  Per matrix:
    gesvx_block      wall time of mpf_gesvx_block (itmax = 10, bounds on) and its own stage times
    parts            the same work from the public pieces on the same tree, timed one by one on the equilibrated copy the driver
                     factors (S = Dr A Dc by hand, B scaled to match): factor in the mode of the driver's path, lange + gecon,
                     solve_ir_block, gerfs (itmax = 10); `ratio` = gesvx_block / (equilibrate + the sum of the parts)
    gesvx_x64        64 x the wall time of one mpf_gesvx call on column 0
    getrs pass       with and without scale vectors: the refinement attempt at max_iter = 0 without bounds (load, norms, ONE solve, one
                     residual, store) on fp64 factors, equilibrate = 2 (scaled loads and stores) against equilibrate = 0 (the old
                     kernels); the factors differ by exact powers of two, the launches are the same
Writes profiles/gesvx_block_probe_n<N>.json.   Usage: python tools/gesvx_block_probe.py [N] [nrhs] [out.json]"""
import importlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

mpf = importlib.import_module("mixed-precision_lu_factorization_amd")


def wall_ms(fn, reps=3):
    """Median wall time of fn() (every entry point synchronises)."""
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    out.sort()
    return out[len(out) // 2]


def probe(ctx, name, A, B, nb, work):
    n, k = B.shape
    row = {"matrix": name}
    run = lambda **kw: ctx.gesvx_block(A, B, nb, itmax=10, work=work, **kw)
    res = run(want_scales=True)
    row["gesvx_block_ms"] = round(wall_ms(lambda: run()), 2)
    X, ferr, berr, st, ir, rfs, _, _, r, c = res
    row.update({"path": st.path, "equed": st.equed, "rcond": st.rcond, "ms_equilibrate": round(st.ms_equilibrate, 2),
                "ms_factor": round(st.ms_factor, 2), "ms_gecon": round(st.ms_gecon, 2), "ms_ir": round(st.ms_ir, 2),
                "ms_bounds": round(rfs[0].ms_total, 2), "ir_iterations": max(s.iterations for s in ir),
                "gerfs_iterations": max(s.iterations for s in rfs), "gerfs_solves": rfs[0].solves,
                "berr_max": float(berr.max()), "ferr_max": float(ferr.max())})
    # the parts, on the equilibrated copy
    rs = r if st.equed & 1 else torch.ones_like(r)
    cs = c if st.equed & 2 else torch.ones_like(c)
    S = ((A * rs[:, None]) * cs[None, :]).t().contiguous().t()
    Bs = (B * rs[:, None]).t().contiguous().t()
    mode = mpf.TRAIL_FP16 if st.path == 1 else mpf.TRAIL_FP64
    W = work
    factor_ms = wall_ms(lambda: ctx.factor(W.copy_(S), nb, trailing=mode)) - wall_ms(lambda: W.copy_(S))
    ipiv, _ = ctx.factor(W.copy_(S), nb, trailing=mode)
    gecon_ms = wall_ms(lambda: ctx.gecon(W, ctx.lange(S, "1"), "1"))
    ir_ms = wall_ms(lambda: ctx.solve_ir_block(S, W, ipiv, Bs))
    Y, _ = ctx.solve_ir_block(S, W, ipiv, Bs)
    Yc = ctx.colmajor(n, k)
    gerfs_ms = wall_ms(lambda: ctx.gerfs(S, W, ipiv, Bs, Yc.copy_(Y), itmax=10, overwrite=True)) - wall_ms(lambda: Yc.copy_(Y))
    parts = {"factor_ms": round(factor_ms, 2), "gecon_ms": round(gecon_ms, 2), "solve_ir_block_ms": round(ir_ms, 2), "gerfs_ms": round(gerfs_ms, 2)}
    parts["sum_ms"] = round(sum(parts.values()), 2)
    row["parts"] = parts
    row["ratio"] = round(row["gesvx_block_ms"] / (st.ms_equilibrate + parts["sum_ms"]), 3)
    del S, Bs, Y, Yc
    torch.cuda.empty_cache()
    b0 = B[:, 0].contiguous()
    one = wall_ms(lambda: ctx.gesvx(A, b0, nb, work=work))
    row["gesvx_one_ms"] = round(one, 2)
    row["gesvx_x64_ms"] = round(64 * one, 1)
    # one solve with and without scale vectors
    att = lambda eq: sorted(ctx.gesvx_block(A, B, nb, equilibrate=eq, try_fp16=0, max_iter=0, bounds=False, work=work)[3].ir_final.ms_total
                            for _ in range(3))[1]
    row["attempt0_scaled_ms"] = round(att(2), 3)
    row["attempt0_plain_ms"] = round(att(0), 3)
    print(json.dumps(row), flush=True)
    return row


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(root, "profiles", f"gesvx_block_probe_n{n}.json")
    nb = 256
    ctx = mpf.MPFContext(0)
    dev = ctx.device
    A = ctx.matgen(n)
    idx = torch.arange(n, device=dev)
    A[idx, idx] += A.sum(dim=1)                               # diagonally dominant
    gen = torch.Generator(device=dev).manual_seed(7)
    B = torch.rand((k, n), dtype=torch.float64, device=dev, generator=gen).t()
    work = ctx.colmajor(n, n)
    res = {"N": n, "nb": nb, "nrhs": k, "itmax": 10, "rows": []}
    res["rows"].append(probe(ctx, "diagdom", A, B, nb, work))
    A.mul_(torch.logspace(0, 8, n, dtype=torch.float64, device=dev)[:, None])      # BASELINE config 5
    res["rows"].append(probe(ctx, "config5", A, B, nb, work))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)
    ctx.close()


if __name__ == "__main__":
    main()
