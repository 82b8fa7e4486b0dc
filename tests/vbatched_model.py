"""numpy restatement of the descriptor of a variable-size batch (csrc/vbatch_plan.h; contract in include/mpf_c.h: mpf_vbatch_create):
prefix sums, extent, the size classes and their order, and the overlap rule.  Only the descriptor: the arithmetic of the vbatched entry
points is that of the fixed-size ones (batched_model.py, batched_inv_model.py, getri_model.py)."""
import numpy as np

MAXN = 128
CLASS_TOP = [8, 16, 32, 48, 64, 96, 128]      # wave forms W = 8 / 16 / 32; workgroup forms H = 1 (48, 64) and H = 2 (96, 128)


def class_of(n):
    """The class of an order 1 <= n <= 128: chosen by n alone."""
    return next(k for k, top in enumerate(CLASS_TOP) if n <= top)


def plan(n, ld=None, off=None):
    """dict(ld, off, offv, total_n, extent, zeros, classes) or the refusal as a string.  classes[k]: the matrices of class k ordered by n,
    equal orders in the batch's order (a stable sort); zeros: the matrices of order 0, which are in no class."""
    n = [int(v) for v in n]
    batch = len(n)
    if batch >= 2 ** 31:
        return "batch >= 2^31"
    ld_, off_, offv, run_m, run_v, extent = [], [], [], 0, 0, 0
    for b, nb in enumerate(n):
        if nb < 0:
            return "n must not be negative"
        if nb > MAXN:
            return "n > 128"
        l = nb if ld is None else int(ld[b])
        if l < nb:
            return "leading dimension < n"
        o = run_m if off is None else int(off[b])
        if o < 0:
            return "offset must not be negative"
        ld_.append(l)
        off_.append(o)
        offv.append(run_v)
        run_m += l * nb
        run_v += nb
        if nb:
            extent = max(extent, o + (nb - 1) * l + nb)
    spans = sorted((off_[b], off_[b] + (n[b] - 1) * ld_[b] + n[b]) for b in range(batch) if n[b])
    end = 0
    for s, e in spans:                          # footprints [s, e) that overlap; touching ones are fine
        if s < end:
            return "overlap"
        end = max(end, e)
    order = sorted(range(batch), key=lambda b: n[b])          # (sorted is stable)
    return dict(ld=np.array(ld_, dtype=np.int64), off=np.array(off_, dtype=np.int64), offv=np.array(offv, dtype=np.int64), total_n=run_v,
                extent=extent, zeros=[b for b in order if n[b] == 0],
                classes=[[b for b in order if n[b] and class_of(n[b]) == k] for k in range(len(CLASS_TOP))])
