"""The variable-size batched entries on a descriptor from mpf_vbatch_create_blocked (orders up to 1024) at scale on one MI355X.
Device time by event pairs around one call, the median of `reps` after one warm-up, fresh data before each call outside the timed
window (as tools/vbatched_probe.py).
  (a) two mixed batches of about 512 MB, n uniform on 1 .. 1024 and on 129 .. 512, all four operations against the route a caller has
      without the descriptor: group by n, gather every group into a strided batch on the device, one fixed-size BLOCKED call per
      distinct n, scatter the results back.  The gather / scatter index tensors are built outside the timed window (the old route is
      not charged for them); the gathers, the calls and the scatters are inside it;
  (b) uniform descriptors of n = 256 and n = 512 with batch 64 and 1024, against the fixed-size blocked entry on the same buffer: what
      the index list and the per-matrix (n, off, ld, offv) loads cost when nothing is ragged;
  (c) both routes must agree bit for bit, in (a) and in (b): asserted.
The fixed-size entries (csrc/batched_blocked.hip) are the baselines: the same bodies (csrc/batched_blocked_body.h) behind a strided fetch.
Writes profiles/vbatched_blocked_probe.json.  Conditions recorded with the numbers: every mixed ratio grouped / vbatched above 1, every
uniform ratio vbatched / fixed at most 1.26.
Usage: python tools/vbatched_blocked_probe.py [out.json] [total MB]"""
import importlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

mpf = importlib.import_module("mixed-precision_lu_factorization_amd")
REPS = 5
OPS = ("getrf", "getrs1", "getri", "getdet")
UNIFORM_LIMIT = 1.26


def event_ms(prepare, fn, reps=REPS):
    """(median, min, max) device ms of fn() over reps runs, prepare() before each one outside the timed window; one warm-up."""
    prepare()
    fn()
    out = []
    for _ in range(reps):
        prepare()
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


def uniform(ctx, n, batch, gen):
    vb = ctx.vbatch_blocked(np.full(batch, n, dtype=np.int32))
    src = torch.randn(vb.extent, dtype=torch.float64, device=ctx.device, generator=gen)
    rhs = torch.randn(vb.total_n, dtype=torch.float64, device=ctx.device, generator=gen)
    as_batch = lambda flat: flat.view(batch, n, n).transpose(1, 2)                     # noqa: E731  (the same memory, (batch, n, n) column-major)
    Wf, Wv = src.clone(), src.clone()
    pf, pv = torch.zeros((batch, n), dtype=torch.int32, device=ctx.device), torch.zeros(vb.total_n, dtype=torch.int32, device=ctx.device)
    inf_f, inf_v = torch.zeros(batch, dtype=torch.int32, device=ctx.device), torch.zeros(batch, dtype=torch.int32, device=ctx.device)
    row = {"n": n, "batch": batch, "bytes_of_matrices": 8 * vb.extent}
    row["getrf_fixed_ms"] = event_ms(lambda: Wf.copy_(src), lambda: ctx.getrf_batched_blocked(as_batch(Wf), overwrite=True, ipiv=pf, info=inf_f))
    row["getrf_vbatched_ms"] = event_ms(lambda: Wv.copy_(src), lambda: vb.getrf(Wv, overwrite=True, ipiv=pv, info=inf_v))
    assert same(Wf, Wv) and same(pf.view(-1), pv) and same(inf_f, inf_v), ("getrf", n)
    Xf, Xv = rhs.clone(), rhs.clone()
    row["getrs1_fixed_ms"] = event_ms(lambda: Xf.copy_(rhs),
                                      lambda: ctx.getrs_batched_blocked(as_batch(Wf), pf, Xf.view(batch, n, 1), overwrite=True))
    row["getrs1_vbatched_ms"] = event_ms(lambda: Xv.copy_(rhs), lambda: vb.getrs(Wv, pv, Xv.view(-1, 1), overwrite=True))
    assert same(Xf, Xv), ("getrs", n)
    If, Iv = torch.zeros_like(src), torch.zeros_like(src)
    row["getri_fixed_ms"] = event_ms(lambda: None, lambda: ctx.getri_batched_blocked(as_batch(Wf), pf, out=as_batch(If), info=inf_f))
    row["getri_vbatched_ms"] = event_ms(lambda: None, lambda: vb.getri(Wv, pv, out=Iv, info=inf_v))
    assert same(If, Iv) and same(inf_f, inf_v), ("getri", n)
    del If, Iv
    row["getdet_fixed_ms"] = event_ms(lambda: None, lambda: ctx.getdet_batched_blocked(as_batch(Wf), pf))
    row["getdet_vbatched_ms"] = event_ms(lambda: None, lambda: vb.getdet(Wv, pv))
    a, b = ctx.getdet_batched_blocked(as_batch(Wf), pf), vb.getdet(Wv, pv)
    assert same(a[0], b[0]) and same(a[1], b[1]), ("getdet", n)
    for op in OPS:
        row[f"{op}_vbatched_over_fixed"] = round(row[f"{op}_vbatched_ms"][0] / row[f"{op}_fixed_ms"][0], 3)
    vb.close()
    return row


def mixed(ctx, lo, hi, total, gen):
    rng = np.random.default_rng(hi)
    mean = sum(v * v for v in range(lo, hi + 1)) / (hi - lo + 1)
    n = rng.integers(lo, hi + 1, int(total / 8 / mean)).astype(np.int32)
    vb = ctx.vbatch_blocked(n)
    src = torch.randn(vb.extent, dtype=torch.float64, device=ctx.device, generator=gen)
    rhs = torch.randn(vb.total_n, dtype=torch.float64, device=ctx.device, generator=gen)
    off, offv = torch.from_numpy(vb.off).to(ctx.device), torch.from_numpy(vb.offv).to(ctx.device)
    groups = []                                              # the old route's index tensors: (n, members, matrix elements, vector elements)
    for v in np.unique(n):
        mem = torch.from_numpy(np.nonzero(n == v)[0]).to(ctx.device)
        groups.append((int(v), mem, (off[mem][:, None] + torch.arange(int(v) * int(v), device=ctx.device)[None, :]).view(-1),
                       (offv[mem][:, None] + torch.arange(int(v), device=ctx.device)[None, :]).view(-1)))
    row = {"n": f"uniform on {lo} .. {hi}", "batch": int(n.size), "total_n": vb.total_n, "bytes_of_matrices": 8 * vb.extent,
           "distinct_n": len(groups)}

    def gather(flat, v, mem, me):                            # (batch_v, n, n) column-major, packed
        return flat[me].view(mem.numel(), v, v).transpose(1, 2)

    Wo, Wv = src.clone(), src.clone()
    po, pv = torch.zeros(vb.total_n, dtype=torch.int32, device=ctx.device), torch.zeros(vb.total_n, dtype=torch.int32, device=ctx.device)
    io, iv = torch.zeros(vb.batch, dtype=torch.int32, device=ctx.device), torch.zeros(vb.batch, dtype=torch.int32, device=ctx.device)

    def old_getrf():
        for v, mem, me, ve in groups:
            LU, ipiv, info = ctx.getrf_batched_blocked(gather(Wo, v, mem, me), overwrite=True)
            Wo[me] = LU.transpose(1, 2).reshape(-1)
            po[ve] = ipiv.view(-1)
            io[mem] = info
    row["getrf_grouped_ms"] = event_ms(lambda: Wo.copy_(src), old_getrf)
    row["getrf_vbatched_ms"] = event_ms(lambda: Wv.copy_(src), lambda: vb.getrf(Wv, overwrite=True, ipiv=pv, info=iv))
    assert same(Wo, Wv) and same(po, pv) and same(io, iv), ("getrf", lo, hi)
    row["singular"] = int(torch.count_nonzero(iv))
    Xo, Xv = rhs.clone(), rhs.clone()

    def old_getrs():
        for v, mem, me, ve in groups:
            X = ctx.getrs_batched_blocked(gather(Wo, v, mem, me), po[ve].view(-1, v), Xo[ve].view(-1, v, 1), overwrite=True)
            Xo[ve] = X.reshape(-1)
    row["getrs1_grouped_ms"] = event_ms(lambda: Xo.copy_(rhs), old_getrs)
    row["getrs1_vbatched_ms"] = event_ms(lambda: Xv.copy_(rhs), lambda: vb.getrs(Wv, pv, Xv.view(-1, 1), overwrite=True))
    assert same(Xo, Xv), ("getrs", lo, hi)
    Io, Iv = torch.zeros_like(src), torch.zeros_like(src)

    def old_getri():
        for v, mem, me, ve in groups:
            X, info = ctx.getri_batched_blocked(gather(Wo, v, mem, me), po[ve].view(-1, v))
            Io[me] = X.transpose(1, 2).reshape(-1)
            io[mem] = info
    row["getri_grouped_ms"] = event_ms(lambda: None, old_getri)
    row["getri_vbatched_ms"] = event_ms(lambda: None, lambda: vb.getri(Wv, pv, out=Iv, info=iv))
    assert same(Io, Iv) and same(io, iv), ("getri", lo, hi)
    del Io, Iv
    mo, eo = torch.zeros(vb.batch, dtype=torch.float64, device=ctx.device), torch.zeros(vb.batch, dtype=torch.int32, device=ctx.device)

    def old_getdet():
        for v, mem, me, ve in groups:
            m, e = ctx.getdet_batched_blocked(gather(Wo, v, mem, me), po[ve].view(-1, v))
            mo[mem] = m
            eo[mem] = e
    row["getdet_grouped_ms"] = event_ms(lambda: None, old_getdet)
    row["getdet_vbatched_ms"] = event_ms(lambda: None, lambda: vb.getdet(Wv, pv))
    m, e = vb.getdet(Wv, pv)
    assert same(mo, m) and same(eo, e), ("getdet", lo, hi)
    for op in OPS:
        row[f"{op}_speedup_over_grouped"] = round(row[f"{op}_grouped_ms"][0] / row[f"{op}_vbatched_ms"][0], 2)
    vb.close()
    return row


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "profiles", "vbatched_blocked_probe.json")
    total = (int(sys.argv[2]) if len(sys.argv) > 2 else 512) << 20
    ctx = mpf.MPFContext(0)
    gen = torch.Generator(device=ctx.device)
    gen.manual_seed(1)
    res = {"bytes_of_matrices_mixed": total, "reps": REPS, "timing": "device events around one call, ms: [median, min, max]",
           "bit_check": "both routes agree bit for bit in every row (asserted)",
           "grouped": "group by n, gather into strided batches on the device, one fixed-size blocked call per distinct n, scatter back; "
                      "the index tensors are built outside the timed window",
           "mixed": [], "uniform": []}
    for lo, hi in ((1, 1024), (129, 512)):
        res["mixed"].append(mixed(ctx, lo, hi, total, gen))
        print(json.dumps(res["mixed"][-1]), flush=True)
        torch.cuda.empty_cache()
    for n in (256, 512):
        for batch in (64, 1024):
            res["uniform"].append(uniform(ctx, n, batch, gen))
            print(json.dumps(res["uniform"][-1]), flush=True)
            torch.cuda.empty_cache()
    res["conditions"] = {
        "mixed_every_operation_faster_than_grouped": all(r[f"{op}_speedup_over_grouped"] > 1.0 for r in res["mixed"] for op in OPS),
        "uniform_limit": UNIFORM_LIMIT,
        "uniform_worst_vbatched_over_fixed": max(r[f"{op}_vbatched_over_fixed"] for r in res["uniform"] for op in OPS),
    }
    res["conditions"]["uniform_within_limit"] = res["conditions"]["uniform_worst_vbatched_over_fixed"] <= UNIFORM_LIMIT
    print(json.dumps(res["conditions"]), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)
    ctx.close()


if __name__ == "__main__":
    main()
