"""The variable-size batched entries (mpf_getrf_vbatched, mpf_getrs_vbatched, mpf_getri_vbatched, mpf_getdet_vbatched) at scale on one
MI355X.  Device time by event pairs around one call, the median of `reps` after one warm-up, fresh data before each call outside the
timed window (as tools/batched_probe.py).
  (a) uniform descriptors of n = 8, 16, 32, 64, 128 with 512 MB of matrices each, against the fixed-size entry on the same buffer:
      what the index lists and per-matrix (n, off, ld, offv) loads cost when nothing is ragged;
  (b) two mixed batches of about 512 MB, n uniform on 1 .. 32 and on 1 .. 128, all four operations against the route a caller has
      without them: group by n, gather every group into a strided batch on the device, one fixed-size call per distinct n, scatter
      the results back.  The gather / scatter index tensors are built outside the timed window (the old route is not charged for
      them); the gathers, the calls and the scatters are inside it;
  (c) both routes must agree bit for bit, in (a) and in (b): asserted.
Writes profiles/vbatched_probe.json.  No rate is a gate: the numbers are the record.
Usage: python tools/vbatched_probe.py [out.json] [total MB]"""
import importlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

mpf = importlib.import_module("mixed-precision_lu_factorization_amd")
REPS = 5


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


def uniform(ctx, n, total, gen):
    batch = total // (8 * n * n)
    vb = ctx.vbatch(np.full(batch, n, dtype=np.int32))
    src = torch.randn(vb.extent, dtype=torch.float64, device=ctx.device, generator=gen)
    rhs = torch.randn(vb.total_n, dtype=torch.float64, device=ctx.device, generator=gen)
    as_batch = lambda flat: flat.view(batch, n, n).transpose(1, 2)                     # noqa: E731  (the same memory, (batch, n, n) column-major)
    Wf, Wv = src.clone(), src.clone()
    pf, pv = torch.zeros((batch, n), dtype=torch.int32, device=ctx.device), torch.zeros(vb.total_n, dtype=torch.int32, device=ctx.device)
    inf_f, inf_v = torch.zeros(batch, dtype=torch.int32, device=ctx.device), torch.zeros(batch, dtype=torch.int32, device=ctx.device)
    row = {"n": n, "batch": batch}
    row["getrf_fixed_ms"] = event_ms(lambda: Wf.copy_(src), lambda: ctx.getrf_batched(as_batch(Wf), overwrite=True, ipiv=pf, info=inf_f))
    row["getrf_vbatched_ms"] = event_ms(lambda: Wv.copy_(src), lambda: vb.getrf(Wv, overwrite=True, ipiv=pv, info=inf_v))
    assert same(Wf, Wv) and same(pf.view(-1), pv) and same(inf_f, inf_v), ("getrf", n)
    Xf, Xv = rhs.clone(), rhs.clone()
    row["getrs1_fixed_ms"] = event_ms(lambda: Xf.copy_(rhs), lambda: ctx.getrs_batched(as_batch(Wf), pf, Xf.view(batch, n, 1), overwrite=True))
    row["getrs1_vbatched_ms"] = event_ms(lambda: Xv.copy_(rhs), lambda: vb.getrs(Wv, pv, Xv.view(-1, 1), overwrite=True))
    assert same(Xf, Xv), ("getrs", n)
    If, Iv = torch.zeros_like(src), torch.zeros_like(src)
    row["getri_fixed_ms"] = event_ms(lambda: None, lambda: ctx.getri_batched(as_batch(Wf), pf, out=as_batch(If), info=inf_f))
    row["getri_vbatched_ms"] = event_ms(lambda: None, lambda: vb.getri(Wv, pv, out=Iv, info=inf_v))
    assert same(If, Iv) and same(inf_f, inf_v), ("getri", n)
    del If, Iv
    row["getdet_fixed_ms"] = event_ms(lambda: None, lambda: ctx.getdet_batched(as_batch(Wf), pf))
    row["getdet_vbatched_ms"] = event_ms(lambda: None, lambda: vb.getdet(Wv, pv))
    a, b = ctx.getdet_batched(as_batch(Wf), pf), vb.getdet(Wv, pv)
    assert same(a[0], b[0]) and same(a[1], b[1]), ("getdet", n)
    for op in ("getrf", "getrs1", "getri", "getdet"):
        row[f"{op}_vbatched_over_fixed"] = round(row[f"{op}_vbatched_ms"][0] / row[f"{op}_fixed_ms"][0], 3)
    vb.close()
    return row


def mixed(ctx, top, total, gen):
    rng = np.random.default_rng(top)
    mean = sum(v * v for v in range(1, top + 1)) / top
    n = rng.integers(1, top + 1, int(total / 8 / mean)).astype(np.int32)
    vb = ctx.vbatch(n)
    src = torch.randn(vb.extent, dtype=torch.float64, device=ctx.device, generator=gen)
    rhs = torch.randn(vb.total_n, dtype=torch.float64, device=ctx.device, generator=gen)
    off, offv = torch.from_numpy(vb.off).to(ctx.device), torch.from_numpy(vb.offv).to(ctx.device)
    groups = []                                              # the old route's index tensors: (n, members, matrix elements, vector elements)
    for v in np.unique(n):
        mem = torch.from_numpy(np.nonzero(n == v)[0]).to(ctx.device)
        groups.append((int(v), mem, (off[mem][:, None] + torch.arange(v * v, device=ctx.device)[None, :]).view(-1),
                       (offv[mem][:, None] + torch.arange(v, device=ctx.device)[None, :]).view(-1)))
    row = {"n": f"uniform on 1 .. {top}", "batch": int(n.size), "total_n": vb.total_n, "bytes_of_matrices": 8 * vb.extent,
           "distinct_n": len(groups)}

    def gather(flat, v, mem, me):                            # (batch_v, n, n) column-major, packed
        return flat[me].view(mem.numel(), v, v).transpose(1, 2)

    Wo, Wv = src.clone(), src.clone()
    po, pv = torch.zeros(vb.total_n, dtype=torch.int32, device=ctx.device), torch.zeros(vb.total_n, dtype=torch.int32, device=ctx.device)
    io, iv = torch.zeros(vb.batch, dtype=torch.int32, device=ctx.device), torch.zeros(vb.batch, dtype=torch.int32, device=ctx.device)

    def old_getrf():
        for v, mem, me, ve in groups:
            LU, ipiv, info = ctx.getrf_batched(gather(Wo, v, mem, me), overwrite=True)
            Wo[me] = LU.transpose(1, 2).reshape(-1)
            po[ve] = ipiv.view(-1)
            io[mem] = info
    row["getrf_grouped_ms"] = event_ms(lambda: Wo.copy_(src), old_getrf)
    row["getrf_vbatched_ms"] = event_ms(lambda: Wv.copy_(src), lambda: vb.getrf(Wv, overwrite=True, ipiv=pv, info=iv))
    assert same(Wo, Wv) and same(po, pv) and same(io, iv), ("getrf", top)
    row["singular"] = int(torch.count_nonzero(iv))
    Xo, Xv = rhs.clone(), rhs.clone()

    def old_getrs():
        for v, mem, me, ve in groups:
            X = ctx.getrs_batched(gather(Wo, v, mem, me), po[ve].view(-1, v), Xo[ve].view(-1, v, 1), overwrite=True)
            Xo[ve] = X.reshape(-1)
    row["getrs1_grouped_ms"] = event_ms(lambda: Xo.copy_(rhs), old_getrs)
    row["getrs1_vbatched_ms"] = event_ms(lambda: Xv.copy_(rhs), lambda: vb.getrs(Wv, pv, Xv.view(-1, 1), overwrite=True))
    assert same(Xo, Xv), ("getrs", top)
    Io, Iv = torch.zeros_like(src), torch.zeros_like(src)

    def old_getri():
        for v, mem, me, ve in groups:
            X, info = ctx.getri_batched(gather(Wo, v, mem, me), po[ve].view(-1, v))
            Io[me] = X.transpose(1, 2).reshape(-1)
            io[mem] = info
    row["getri_grouped_ms"] = event_ms(lambda: None, old_getri)
    row["getri_vbatched_ms"] = event_ms(lambda: None, lambda: vb.getri(Wv, pv, out=Iv, info=iv))
    assert same(Io, Iv) and same(io, iv), ("getri", top)
    del Io, Iv
    mo, eo = torch.zeros(vb.batch, dtype=torch.float64, device=ctx.device), torch.zeros(vb.batch, dtype=torch.int32, device=ctx.device)

    def old_getdet():
        for v, mem, me, ve in groups:
            m, e = ctx.getdet_batched(gather(Wo, v, mem, me), po[ve].view(-1, v))
            mo[mem] = m
            eo[mem] = e
    row["getdet_grouped_ms"] = event_ms(lambda: None, old_getdet)
    row["getdet_vbatched_ms"] = event_ms(lambda: None, lambda: vb.getdet(Wv, pv))
    m, e = vb.getdet(Wv, pv)
    assert same(mo, m) and same(eo, e), ("getdet", top)
    for op in ("getrf", "getrs1", "getri", "getdet"):
        row[f"{op}_speedup_over_grouped"] = round(row[f"{op}_grouped_ms"][0] / row[f"{op}_vbatched_ms"][0], 2)
    vb.close()
    return row


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "profiles", "vbatched_probe.json")
    total = (int(sys.argv[2]) if len(sys.argv) > 2 else 512) << 20
    ctx = mpf.MPFContext(0)
    gen = torch.Generator(device=ctx.device)
    gen.manual_seed(1)
    res = {"bytes_of_matrices": total, "reps": REPS, "timing": "device events around one call, ms: [median, min, max]",
           "bit_check": "both routes agree bit for bit in every row (asserted)",
           "grouped": "group by n, gather into strided batches on the device, one fixed-size call per distinct n, scatter back; the "
                      "index tensors are built outside the timed window",
           "uniform": [], "mixed": []}
    for n in (8, 16, 32, 64, 128):
        res["uniform"].append(uniform(ctx, n, total, gen))
        print(json.dumps(res["uniform"][-1]), flush=True)
        torch.cuda.empty_cache()
    for top in (32, 128):
        res["mixed"].append(mixed(ctx, top, total, gen))
        print(json.dumps(res["mixed"][-1]), flush=True)
        torch.cuda.empty_cache()
    if os.path.exists(out_path):                             # keep what other tools recorded in the same file (the fixed-size probes)
        with open(out_path) as f:
            old = json.load(f)
        res.update({k: v for k, v in old.items() if k not in res})
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)
    ctx.close()


if __name__ == "__main__":
    main()
