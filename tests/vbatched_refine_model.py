"""numpy restatement of the launch groups of the vbatched expert layer (csrc/vbatch_plan.h: refine_chunks) -- test infrastructure.

The entries are every matrix of order >= 1 of a descriptor in ascending order of n.  The list is cut
  * at the tops 64, 128, 256, 512, 1024: a launch's block is sized for its largest matrix, so it is at most twice what the group's
    smallest matrix needs and never below one wave;
  * after max_launch entries (BB_MAX_LAUNCH = 2^15 of csrc/mpf_internal.h);
  * for the refinement with its bound (limit > 0): before the entry that would take the chunk's workspace past `limit` doubles, where
    a matrix of order n costs nrhs (n + 1 + ceil(n / 16)) -- batch_args::ferr_step's count -- but never before the chunk's first entry.
chunks() returns (first, count, nmax) triples."""
import numpy as np

TOPS = [64, 128, 256, 512, 1024]
MAX_LAUNCH = 1 << 15
LIMIT = 1 << 25
CT = 16


def top_of(n):
    return next(t for t in TOPS if n <= t)


def cost(n, nrhs):
    return nrhs * (n + 1 + -(-n // CT))


def chunks(ns, max_launch=MAX_LAUNCH, nrhs=0, limit=0):
    ns = [int(v) for v in ns]
    assert ns == sorted(ns) and all(1 <= v <= 1024 for v in ns)
    out, i = [], 0
    while i < len(ns):
        top, j, work = top_of(ns[i]), i, 0
        while j < len(ns) and j - i < max_launch and ns[j] <= top:
            if limit > 0 and j > i and work + cost(ns[j], nrhs) > limit:
                break
            work += cost(ns[j], nrhs)
            j += 1
        out.append((i, j - i, ns[j - 1]))
        i = j
    return out


def list_order(n):
    """The descriptor's list: the matrices in ascending order of n, equal orders in the batch's order; (zeros, the others)."""
    n = np.asarray(n)
    order = np.argsort(n, kind="stable")
    zeros = int((n == 0).sum())
    return order[:zeros].tolist(), order[zeros:].tolist()
