"""The expert layer on a descriptor (mpf_lange_vbatched, mpf_gecon_vbatched, mpf_gerfs_vbatched) at scale on one MI355X, after
tools/vbatched_blocked_probe.py.  Device time by event pairs around one call, the median of `reps` after one warm-up.  Measured: lange
'1'; gecon '1' and 'I'; gerfs with one and with eight right-hand sides, with and without ferr, on solutions that are already converged
(a clean refinement, so every repetition does the same work).
  (a) mixed batches: 191 matrices with n uniform on 1 .. 1024 and 583 with n uniform on 129 .. 512 (that probe's two distributions), and
      2^16 matrices with n uniform on 1 .. 32, against the route a caller has without these entries: group by n, gather every group
      into strided batches on the device, one fixed-size BLOCKED expert call per distinct n, scatter the results back.  The index tensors
      are built outside the timed window; the gathers, the calls and the scatters are inside it.  Hard condition on the first two: every
      operation faster than that route.  The third is reported whatever it is: there the ragged call runs a workgroup per matrix where
      the small fixed-size entries run 8, 16 or 32 lanes per matrix.
  (b) uniform descriptors of n = 256 and n = 512 with batch 64 and 1024, against the fixed-size blocked expert entry on the same
      buffers.  Condition: ragged / fixed at most 1.26.
  (c) both routes must agree bit for bit, in (a) and in (b): asserted.
  (d) with AB_DIR: the A/B of the fixed-size expert entries against the parent commit's library on tools/batched_refine_blocked_probe.py's
      points, from that probe's outputs refine_{parent1,new1,parent2,new2}.json in AB_DIR (run in that order, one process at a time),
      in the manner of tools/batched_blocked_ab.py: ratio = mean(new) / mean(parent), box = max(0.02, the parent's own spread).
Writes profiles/vbatched_refine_probe.json.
Usage: python tools/vbatched_refine_probe.py [out.json] [AB_DIR] [parent commit]"""
import importlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

mpf = importlib.import_module("mixed-precision_lu_factorization_amd")
REPS = 5
OPS = ("lange1", "gecon1", "geconI", "gerfs_nrhs1_berr_only", "gerfs_nrhs1_with_ferr", "gerfs_nrhs8_berr_only", "gerfs_nrhs8_with_ferr")
UNIFORM_LIMIT = 1.26
AB = [("lange1", "lange1_ms"), ("langeI", "langeI_ms"), ("gecon1", "gecon1_ms"), ("geconI", "geconI_ms"),
      ("gerfs_nrhs1_berr_only", "gerfs_nrhs1_berr_only_ms"), ("gerfs_nrhs1_with_ferr", "gerfs_nrhs1_with_ferr_ms"),
      ("gerfs_nrhs8_berr_only", "gerfs_nrhs8_berr_only_ms"), ("gerfs_nrhs8_with_ferr", "gerfs_nrhs8_with_ferr_ms")]


def event_ms(fn, reps=REPS):
    """[median, min, max] device ms of fn() over reps runs after one warm-up."""
    fn()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    out.sort()
    return [round(out[len(out) // 2], 4), round(out[0], 4), round(out[-1], 4)]


def same(a, b):
    return bool(torch.equal(a.contiguous().view(-1).view(torch.int64), b.contiguous().view(-1).view(torch.int64))) if a.dtype == torch.float64 \
        else bool(torch.equal(a, b))


def setup(ctx, vb, gen):
    """Random matrices, their factors, and per nrhs right-hand sides with converged solutions."""
    A = torch.randn(vb.extent, dtype=torch.float64, device=ctx.device, generator=gen)
    LU, ipiv, info = vb.getrf(A)
    rhs = {}
    for nrhs in (1, 8):
        B = ctx.colmajor(vb.total_n, nrhs)
        B.copy_(torch.randn((nrhs, vb.total_n), dtype=torch.float64, device=ctx.device, generator=gen).t())
        X = vb.getrs(LU, ipiv, B)
        vb.gerfs(A, LU, ipiv, B, X, overwrite=True)          # converge once; later calls are clean
        rhs[nrhs] = (B, X)
    return A, LU, ipiv, int(torch.count_nonzero(info)), rhs


def uniform(ctx, n, batch, gen):
    vb = ctx.vbatch_blocked(np.full(batch, n, dtype=np.int32))
    A, LU, ipiv, singular, rhs = setup(ctx, vb, gen)
    as_batch = lambda flat: flat.view(batch, n, n).transpose(1, 2)                     # noqa: E731  (the same memory, (batch, n, n) column-major)
    cols = lambda T: T.t().reshape(-1, batch, n).permute(1, 2, 0)                      # noqa: E731  ((batch, n, nrhs) views of the tall matrix)
    Af, LUf, pf = as_batch(A), as_batch(LU), ipiv.view(batch, n)
    row = {"n": n, "batch": batch, "singular": singular}
    row["lange1_fixed_ms"] = event_ms(lambda: ctx.lange_batched_blocked(Af, "1"))
    row["lange1_vbatched_ms"] = event_ms(lambda: vb.lange(A, "1"))
    an = {nm: vb.lange(A, nm) for nm in ("1", "I")}
    assert same(an["1"], ctx.lange_batched_blocked(Af, "1")) and same(an["I"], ctx.lange_batched_blocked(Af, "I")), ("lange", n, batch)
    for nm in ("1", "I"):
        row[f"gecon{nm}_fixed_ms"] = event_ms(lambda: ctx.gecon_batched_blocked(LUf, an[nm], nm))
        row[f"gecon{nm}_vbatched_ms"] = event_ms(lambda: vb.gecon(LU, an[nm], nm))
        assert same(vb.gecon(LU, an[nm], nm), ctx.gecon_batched_blocked(LUf, an[nm], nm)), ("gecon", nm, n, batch)
    for nrhs in (1, 8):
        B, X = rhs[nrhs]
        Bf, Xf = ctx.colmajor_batch(batch, n, nrhs), ctx.colmajor_batch(batch, n, nrhs)   # packed, so that neither route copies B
        Bf.copy_(cols(B))
        Xf.copy_(cols(X))
        for name, fe in (("berr_only", False), ("with_ferr", True)):
            row[f"gerfs_nrhs{nrhs}_{name}_fixed_ms"] = event_ms(lambda: ctx.gerfs_batched_blocked(Af, LUf, pf, Bf, Xf, want_ferr=fe))
            row[f"gerfs_nrhs{nrhs}_{name}_vbatched_ms"] = event_ms(lambda: vb.gerfs(A, LU, ipiv, B, X, want_ferr=fe))
        got, want = vb.gerfs(A, LU, ipiv, B, X), ctx.gerfs_batched_blocked(Af, LUf, pf, Bf, Xf)
        assert same(cols(got[0]), want[0]) and all(same(g, w) for g, w in zip(got[1:], want[1:])), ("gerfs", nrhs, n, batch)
    for op in OPS:
        row[f"{op}_vbatched_over_fixed"] = round(row[f"{op}_vbatched_ms"][0] / row[f"{op}_fixed_ms"][0], 3)
    vb.close()
    return row


def mixed(ctx, lo, hi, count, gen):
    n = np.random.default_rng(hi).integers(lo, hi + 1, count).astype(np.int32)
    vb = ctx.vbatch_blocked(n)
    A, LU, ipiv, singular, rhs = setup(ctx, vb, gen)
    off, offv = torch.from_numpy(vb.off).to(ctx.device), torch.from_numpy(vb.offv).to(ctx.device)
    groups = []                                              # the old route's index tensors: (n, members, matrix elements, vector elements)
    for v in np.unique(n):
        mem = torch.from_numpy(np.nonzero(n == v)[0]).to(ctx.device)
        groups.append((int(v), mem, (off[mem][:, None] + torch.arange(int(v) * int(v), device=ctx.device)[None, :]).view(-1),
                       (offv[mem][:, None] + torch.arange(int(v), device=ctx.device)[None, :]).view(-1)))
    row = {"n": f"uniform on {lo} .. {hi}", "batch": int(n.size), "total_n": vb.total_n, "bytes_of_matrices": 8 * vb.extent,
           "distinct_n": len(groups), "singular": singular}

    def gather(flat, v, mem, me):                            # (batch_v, n, n) column-major, packed
        return flat[me].view(mem.numel(), v, v).transpose(1, 2)

    out = torch.zeros(vb.batch, dtype=torch.float64, device=ctx.device)

    def old_lange(nm):
        for v, mem, me, ve in groups:
            out[mem] = ctx.lange_batched_blocked(gather(A, v, mem, me), nm)
    row["lange1_grouped_ms"] = event_ms(lambda: old_lange("1"))
    row["lange1_vbatched_ms"] = event_ms(lambda: vb.lange(A, "1"))
    an = {nm: vb.lange(A, nm) for nm in ("1", "I")}
    for nm in ("1", "I"):
        old_lange(nm)
        assert same(out, an[nm]), ("lange", nm, lo, hi)

    def old_gecon(nm):
        for v, mem, me, ve in groups:
            out[mem] = ctx.gecon_batched_blocked(gather(LU, v, mem, me), an[nm][mem], nm)
    for nm in ("1", "I"):
        row[f"gecon{nm}_grouped_ms"] = event_ms(lambda: old_gecon(nm))
        row[f"gecon{nm}_vbatched_ms"] = event_ms(lambda: vb.gecon(LU, an[nm], nm))
        assert same(out, vb.gecon(LU, an[nm], nm)), ("gecon", nm, lo, hi)
    for nrhs in (1, 8):
        B, X = rhs[nrhs]
        Xo = torch.zeros_like(X)
        fo, bo = torch.zeros((vb.batch, nrhs), dtype=torch.float64, device=ctx.device), torch.zeros((vb.batch, nrhs), dtype=torch.float64, device=ctx.device)
        io = torch.zeros((vb.batch, nrhs), dtype=torch.int32, device=ctx.device)

        def old_gerfs(fe):
            for v, mem, me, ve in groups:
                Xg, ferr, berr, its = ctx.gerfs_batched_blocked(gather(A, v, mem, me), gather(LU, v, mem, me), ipiv[ve].view(-1, v),
                                                                B[ve].view(-1, v, nrhs), X[ve].view(-1, v, nrhs), want_ferr=fe)
                Xo[ve] = Xg.reshape(-1, nrhs)
                bo[mem] = berr
                io[mem] = its
                if fe:
                    fo[mem] = ferr
        for name, fe in (("berr_only", False), ("with_ferr", True)):
            row[f"gerfs_nrhs{nrhs}_{name}_grouped_ms"] = event_ms(lambda: old_gerfs(fe))
            row[f"gerfs_nrhs{nrhs}_{name}_vbatched_ms"] = event_ms(lambda: vb.gerfs(A, LU, ipiv, B, X, want_ferr=fe))
        got = vb.gerfs(A, LU, ipiv, B, X)
        assert same(got[0], Xo) and same(got[1], fo) and same(got[2], bo) and same(got[3], io), ("gerfs", nrhs, lo, hi)
        row[f"corrections_max_nrhs{nrhs}"] = int(got[3].max())
    for op in OPS:
        row[f"{op}_speedup_over_grouped"] = round(row[f"{op}_grouped_ms"][0] / row[f"{op}_vbatched_ms"][0], 2)
    vb.close()
    return row


def ab_points(d):
    """The fixed-size expert entries, new build against the parent's, per point of tools/batched_refine_blocked_probe.py."""
    runs = {}
    for tag in ("parent1", "new1", "parent2", "new2"):
        with open(os.path.join(d, f"refine_{tag}.json")) as f:
            runs[tag] = {(r["n"], r["batch"]): r for r in json.load(f)["rows"]}
    points = []
    for key in runs["parent1"]:
        for name, field in AB:
            p = [runs["parent1"][key][field], runs["parent2"][key][field]]
            w = [runs["new1"][key][field], runs["new2"][key][field]]
            spread = abs(p[0] - p[1]) / min(p)
            ratio = (w[0] + w[1]) / (p[0] + p[1])
            box = max(0.02, spread) + 0.02                   # the probe's own repeat-to-repeat spread plus the pool's +- 2 % between boxes
            verdict = "within" if abs(ratio - 1) <= box else ("faster" if ratio < 1 else "slower")
            points.append({"n": key[0], "batch": key[1], "quantity": name, "parent_ms": p, "new_ms": w, "parent_spread": round(spread, 4),
                           "ratio": round(ratio, 4), "box": round(box, 4), "verdict": verdict})
    return points


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "profiles", "vbatched_refine_probe.json")
    ctx = mpf.MPFContext(0)
    gen = torch.Generator(device=ctx.device)
    gen.manual_seed(1)
    res = {"parent_commit": sys.argv[3] if len(sys.argv) > 3 else "449fa1e", "reps": REPS,
           "timing": "device events around one call, ms: [median, min, max]",
           "bit_check": "both routes agree bit for bit in every row (asserted)",
           "grouped": "group by n, gather into strided batches on the device, one fixed-size blocked expert call per distinct n, scatter "
                      "back; the index tensors are built outside the timed window",
           "gerfs": "on converged solutions (a clean refinement): residual, berr and the rule once per column, no correction",
           "mixed": [], "small_orders": [], "uniform": []}
    for lo, hi, count, key in ((1, 1024, 191, "mixed"), (129, 512, 583, "mixed"), (1, 32, 1 << 16, "small_orders")):
        res[key].append(mixed(ctx, lo, hi, count, gen))
        print(json.dumps(res[key][-1]), flush=True)
        torch.cuda.empty_cache()
    for n in (256, 512):
        for batch in (64, 1024):
            res["uniform"].append(uniform(ctx, n, batch, gen))
            print(json.dumps(res["uniform"][-1]), flush=True)
            torch.cuda.empty_cache()
    res["conditions"] = {
        "mixed_every_operation_faster_than_grouped": all(r[f"{op}_speedup_over_grouped"] > 1.0 for r in res["mixed"] for op in OPS),
        "mixed_worst_speedup_over_grouped": min(r[f"{op}_speedup_over_grouped"] for r in res["mixed"] for op in OPS),
        "small_orders_speedup_over_grouped": {op: res["small_orders"][0][f"{op}_speedup_over_grouped"] for op in OPS},
        "uniform_limit": UNIFORM_LIMIT,
        "uniform_worst_vbatched_over_fixed": max(r[f"{op}_vbatched_over_fixed"] for r in res["uniform"] for op in OPS),
    }
    res["conditions"]["uniform_within_limit"] = res["conditions"]["uniform_worst_vbatched_over_fixed"] <= UNIFORM_LIMIT
    if len(sys.argv) > 2 and sys.argv[2]:
        points = ab_points(sys.argv[2])
        res["fixed_size_ab"] = {
            "order": "parent, new, parent, new; one process at a time; tools/batched_refine_blocked_probe.py's own timing",
            "rule": "ratio = mean(new) / mean(parent); box = max(0.02, parent spread) + 0.02 (the pool's +- 2 % between boxes)",
            "count": {v: sum(1 for p in points if p["verdict"] == v) for v in ("within", "faster", "slower")}, "points": points}
        res["conditions"]["fixed_size_no_point_slower_than_parent"] = res["fixed_size_ab"]["count"]["slower"] == 0
    print(json.dumps(res["conditions"]), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)
    ctx.close()


if __name__ == "__main__":
    main()
