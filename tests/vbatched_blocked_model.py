"""numpy restatement of the extended descriptor plan (csrc/vbatch_plan.h with the larger limit; contract in include/mpf_c.h:
mpf_vbatch_create_blocked): the forwarding rule, the small classes and the large list with its launch groups, and the per-step
schedule of the ragged blocked factorization.  Only the plan: the arithmetic is the fixed-size blocked entries'
(batched_blocked_model.py, batched_blocked_inv_model.py)."""
import numpy as np

import vbatched_model as VM

MAXN = 1024
SMALL_MAXN = VM.MAXN                     # 128: above it no matrix is small, whatever min_n says
GROUP_TOP = [256, 512, 1024]


def is_small(n, min_n):
    """The rule by which the fixed-size blocked entries forward to the one-workgroup kernels."""
    return 1 <= n <= SMALL_MAXN and n < min_n


def group_of(n):
    return next(g for g, top in enumerate(GROUP_TOP) if n <= top)


def plan(n, ld=None, off=None, min_n=129):
    """dict(ld, off, offv, total_n, extent, zeros, classes, large, groups) or the refusal as a string.  classes[k]: the small matrices
    of class k; large: the others of order >= 1; groups[g]: the members of `large` whose order is at most GROUP_TOP[g] and above the
    group before -- all ordered by n, equal orders in the batch's order."""
    n = [int(v) for v in n]
    batch = len(n)
    ld_, off_, offv, run_m, run_v, extent = [], [], [], 0, 0, 0
    for b, nb in enumerate(n):
        if nb < 0:
            return "n must not be negative"
        if nb > MAXN:
            return "n > 1024"
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
    for s, e in spans:
        if s < end:
            return "overlap"
        end = max(end, e)
    order = sorted(range(batch), key=lambda b: n[b])          # (sorted is stable)
    small = [b for b in order if is_small(n[b], min_n)]
    large = [b for b in order if n[b] and not is_small(n[b], min_n)]
    return dict(ld=np.array(ld_, dtype=np.int64), off=np.array(off_, dtype=np.int64), offv=np.array(offv, dtype=np.int64), total_n=run_v,
                extent=extent, zeros=[b for b in order if n[b] == 0],
                classes=[[b for b in small if VM.class_of(n[b]) == k] for k in range(len(VM.CLASS_TOP))],
                large=large, groups=[[b for b in large if group_of(n[b]) == g] for g in range(len(GROUP_TOP))])


def factor_steps(orders, nb):
    """[(j0, first, rows)] for the orders of one launch, ascending: at panel step j0 the matrices with n > j0 are the entries from
    `first` on, and `rows` is the largest remaining row count."""
    orders = list(orders)
    assert orders == sorted(orders) and (not orders or orders[0] >= 1)
    nmax = orders[-1] if orders else 0
    return [(j0, next(i for i, v in enumerate(orders) if v > j0), nmax - j0) for j0 in range(0, nmax, nb)]
