"""Paired bulk phase of the fp64 row-major schedule (option fp64_pair, factor_rm_pairs): the far columns are updated once per
panel pair with K = 2 nb.  Per element the operations and their order are those of the one-level loop, so LU and IPIV must be
bit-identical with the option on and off, at every hand-over point, and the counted flops must be the same."""
import pytest

pytestmark = pytest.mark.gpu

SIZES = [1536, 2048, 2304, 4096 + 77, 8192]   # even / odd number of panels, N not a multiple of nb


def _factor(c, A, nb, pair, min_n):
    import torch
    c.set_option("fp64_pair", pair)
    c.set_option("fp64_pair_min_n", min_n)
    W = A.clone()
    ipiv, info = c.factor(W, nb)
    c.synchronize()
    torch.cuda.synchronize()
    s = c.stats()
    return W, ipiv.clone(), info, s


@pytest.mark.parametrize("nb", [128, 256])
@pytest.mark.parametrize("n", SIZES)
def test_pairs_bit_identical_to_one_level(mpf, n, nb):
    import torch
    c = mpf.MPFContext(0)
    try:
        c.set_option("fp64_rowmajor_min_n", 0)   # small matrices take the row-major schedule too
        A = c.matgen(n)                          # the generator's matrix: interchanges in every panel
        W0, ip0, info0, s0 = _factor(c, A, nb, 0, 0)
        assert s0.hpanel_timeouts == 0
        # hand-over behind the last possible pair, behind the first pair, and in between
        for min_n in (0, n - 3 * nb, n // 2):
            W1, ip1, info1, s1 = _factor(c, A, nb, 1, min_n)
            assert info1 == info0
            assert s1.hpanel_timeouts == 0
            assert torch.equal(ip1, ip0), f"min_n={min_n}: {int((ip1 != ip0).sum())} pivots differ"
            assert torch.equal(W1, W0), f"min_n={min_n}: {int((W1 != W0).sum())} LU elements differ"
            assert s1.gemm_flops == s0.gemm_flops, (min_n, s1.gemm_flops, s0.gemm_flops)
            assert s1.panels == s0.panels and s1.superpanel == 1
            print(f"N={n} nb={nb} min_n={min_n}: gemm_launches {s1.gemm_launches} (one-level {s0.gemm_launches})")
        W2, ip2, _, s2 = _factor(c, A, nb, 1, 0)   # a second run with the option on: the same bits
        W3, ip3, _, _ = _factor(c, A, nb, 1, 0)
        assert torch.equal(W2, W3) and torch.equal(ip2, ip3)
        # (fewer launches only where the one-level loop runs its two lanes; at these sizes it runs one, and the pairs' thin updates count)
        assert s2.gemm_launches != s0.gemm_launches, "no pair ran: the option did not take the paired phase"
    finally:
        c.close()


def test_pair_off_gives_the_one_level_launches(mpf):
    """fp64_pair = 0 and a threshold above the matrix both leave the one-level loop's launches exactly."""
    c = mpf.MPFContext(0)
    try:
        c.set_option("fp64_rowmajor_min_n", 0)
        A = c.matgen(4096)
        _, _, _, s_off = _factor(c, A, 256, 0, 0)
        _, _, _, s_thr = _factor(c, A, 256, 1, 1 << 30)
        assert s_off.gemm_launches == s_thr.gemm_launches and s_off.gemm_flops == s_thr.gemm_flops
    finally:
        c.close()
