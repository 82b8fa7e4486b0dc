"""The batched equilibration on one MI355X: mpf_geequ_* and mpf_laqge_* (rule 2, out of place) through the C entries on preallocated
outputs, at the batched family's usual points of about 512 MB of matrices each -- n = 8 (2^20 matrices), 16, 32, 64, 128 (4096) for the
small entries, n = 256 x 1024, 512 x 256 and 1024 x 64 for the blocked ones, and for descriptors the two mixed distributions (n uniform
on 1 .. 1024 and on 129 .. 512).  Per point, device time by event pairs around single calls, the median of `reps` after one warm-up
call (min and max are kept), and in the same session a device-to-device copy of the same matrix bytes, the reference that is not the
code under test:
  condition   geequ + laqge together at most 3 x the copy for n <= 128 (ideal traffic: one read, then one read and one write = 1.5
              copies), at most 4 x for n > 128 and the descriptors (two reads in geequ: 2 copies);
  reported    geequ alone and laqge alone as fractions of the copy; gesvx_* (equilibrate = 2, one and eight right-hand sides) beside
              solvex_* of the same build.
Writes profiles/batched_equil_probe.json.
Usage: python tools/batched_equil_probe.py [small|blocked|desc|all] [out.json] [nodriver]"""
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

mpf = importlib.import_module("mixed-precision_lu_factorization_amd")
REPS = 5
SMALL = [(8, 1 << 20), (16, 1 << 18), (32, 1 << 16), (64, 1 << 14), (128, 1 << 12)]
BLOCKED = [(256, 1024), (512, 256), (1024, 64)]
DESC = [("uniform 1..1024", 1, 1024), ("uniform 129..512", 129, 512)]
BYTES = 512 << 20


def event_ms(fn, reps=REPS):
    """(median, min, max) device ms of fn() over reps runs after one warm-up."""
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
    return out[len(out) // 2], out[0], out[-1]


def p(t):
    return C.c_void_p(t.data_ptr())


def check(ctx, rc):
    if rc:
        raise mpf.MPFError(ctx.L.mpf_last_error(ctx.h).decode())


def scaled_randn(shape, gen, device):
    """Random matrices with rows and columns scaled by 2^k, k in [-20, 20]: every matrix is scaled on both sides under rule 2."""
    A = torch.randn(shape, dtype=torch.float64, device=device, generator=gen)
    kr = torch.randint(-20, 21, shape[:-1] + (1,), device=device, generator=gen).to(torch.float64)
    kc = torch.randint(-20, 21, shape[:-2] + (1, shape[-1]), device=device, generator=gen).to(torch.float64)
    return A * torch.exp2(kr) * torch.exp2(kc)


def ratios(row, limit, copy, tg, tl):
    row.update({"copy_ms": round(copy[0], 4), "copy_ms_min_max": [round(copy[1], 4), round(copy[2], 4)],
                "geequ_ms": round(tg[0], 4), "geequ_ms_min_max": [round(tg[1], 4), round(tg[2], 4)],
                "laqge_ms": round(tl[0], 4), "laqge_ms_min_max": [round(tl[1], 4), round(tl[2], 4)],
                "geequ_over_copy": round(tg[0] / copy[0], 3), "laqge_over_copy": round(tl[0] / copy[0], 3),
                "both_over_copy": round((tg[0] + tl[0]) / copy[0], 3), "limit": limit,
                "met": bool((tg[0] + tl[0]) / copy[0] <= limit)})


def strided_point(ctx, n, batch, suffix, gen, driver):
    L, h = ctx.L, ctx.h
    A = ctx.colmajor_batch(batch, n, n)
    A.copy_(scaled_randn((batch, n, n), gen, ctx.device))
    out = torch.empty_like(A)
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device=ctx.device)   # noqa: E731
    r, c, rowcnd, colcnd, amax, spread = f64(batch, n), f64(batch, n), f64(batch), f64(batch), f64(batch), f64(batch, 2)
    info, equed = (torch.zeros(batch, dtype=torch.int32, device=ctx.device) for _ in range(2))
    geequ, laqge = getattr(L, "mpf_geequ_batched" + suffix), getattr(L, "mpf_laqge_batched" + suffix)
    tg = event_ms(lambda: check(ctx, geequ(h, p(A), n, n * n, n, batch, p(r), p(c), p(rowcnd), p(colcnd), p(amax), p(info))))
    tl = event_ms(lambda: check(ctx, laqge(h, 2, p(A), n, n * n, n, batch, p(r), p(c), p(rowcnd), p(colcnd), p(amax), p(info), p(out), p(equed),
                                           p(spread))))
    copy = event_ms(lambda: out.copy_(A))
    row = {"entry": "batched" + suffix, "n": n, "batch": batch, "bytes": A.numel() * 8, "flagged": int(torch.count_nonzero(info)),
           "scaled_both": int((equed == 3).sum())}
    ratios(row, 3.0 if n <= 128 else 4.0, copy, tg, tl)
    del out
    if driver:
        for nrhs in (1, 8):
            B = ctx.colmajor_batch(batch, n, nrhs)
            B.copy_(torch.randn((batch, n, nrhs), dtype=torch.float64, device=ctx.device, generator=gen))
            tx = event_ms(lambda: getattr(ctx, "gesvx_batched" + suffix)(A, B, equilibrate=2))
            ts = event_ms(lambda: getattr(ctx, "solvex_batched" + suffix)(A, B))
            row.update({f"gesvx_nrhs{nrhs}_ms": round(tx[0], 4), f"solvex_nrhs{nrhs}_ms": round(ts[0], 4),
                        f"gesvx_over_solvex_nrhs{nrhs}": round(tx[0] / ts[0], 3)})
            del B
    return row


def descriptor_point(ctx, name, lo, hi, gen, driver):
    L, h = ctx.L, ctx.h
    rng = np.random.default_rng(lo)
    ns = []
    while sum(8 * v * v for v in ns) < BYTES:
        ns.append(int(rng.integers(lo, hi + 1)))
    ns = np.array(ns, dtype=np.int32)
    vb = ctx.vbatch_blocked(ns)
    A = torch.zeros(vb.extent, dtype=torch.float64, device=ctx.device)
    for M in vb.unpack(A):
        M.copy_(scaled_randn(tuple(M.shape), gen, ctx.device))
    out = torch.empty_like(A)
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device=ctx.device)   # noqa: E731
    r, c, rowcnd, colcnd, amax, spread = f64(vb.total_n), f64(vb.total_n), f64(vb.batch), f64(vb.batch), f64(vb.batch), f64(vb.batch, 2)
    info, equed = (torch.zeros(vb.batch, dtype=torch.int32, device=ctx.device) for _ in range(2))
    tg = event_ms(lambda: check(ctx, L.mpf_geequ_vbatched(h, vb.h, p(A), p(r), p(c), p(rowcnd), p(colcnd), p(amax), p(info))))
    tl = event_ms(lambda: check(ctx, L.mpf_laqge_vbatched(h, vb.h, 2, p(A), p(r), p(c), p(rowcnd), p(colcnd), p(amax), p(info), p(out), p(equed),
                                                          p(spread))))
    copy = event_ms(lambda: out.copy_(A))
    row = {"entry": "vbatched", "orders": name, "batch": int(vb.batch), "bytes": A.numel() * 8, "flagged": int(torch.count_nonzero(info)),
           "scaled_both": int((equed == 3).sum())}
    ratios(row, 4.0, copy, tg, tl)
    del out
    if driver:
        for nrhs in (1, 8):
            B = ctx.colmajor(vb.total_n, nrhs)
            B.copy_(torch.randn((vb.total_n, nrhs), dtype=torch.float64, device=ctx.device, generator=gen))
            tx = event_ms(lambda: vb.gesvx(A, B, equilibrate=2))
            ts = event_ms(lambda: vb.solvex(A, B))
            row.update({f"gesvx_nrhs{nrhs}_ms": round(tx[0], 4), f"solvex_nrhs{nrhs}_ms": round(ts[0], 4),
                        f"gesvx_over_solvex_nrhs{nrhs}": round(tx[0] / ts[0], 3)})
            del B
    vb.close()
    return row


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(root, "profiles", "batched_equil_probe.json")
    driver = not (len(sys.argv) > 3 and sys.argv[3] == "nodriver")
    ctx = mpf.MPFContext(0)
    res = {"reps": REPS, "timing": "device events around one call; median (min, max)",
           "copy": "torch copy_ of the same matrix bytes, device to device, same session",
           "condition": "both_over_copy = (geequ + laqge rule 2, out of place) / copy <= 3 for n <= 128, <= 4 for n > 128 and descriptors",
           "rows": []}
    gen = torch.Generator(device=ctx.device)
    gen.manual_seed(1)
    points = []
    if which in ("small", "all"):
        points += [lambda n=n, b=b: strided_point(ctx, n, b, "", gen, driver) for n, b in SMALL]
    if which in ("blocked", "all"):
        points += [lambda n=n, b=b: strided_point(ctx, n, b, "_blocked", gen, driver) for n, b in BLOCKED]
    if which in ("desc", "all"):
        points += [lambda a=a: descriptor_point(ctx, *a, gen, driver) for a in DESC]
    for point in points:
        row = point()
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
        torch.cuda.empty_cache()
    res["all_met"] = all(r["met"] for r in res["rows"])
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)
    ctx.close()


if __name__ == "__main__":
    main()
