"""One-pass form of the deferred left-hand interchanges (option lazy_gather = 2: one map launch + in-place apply launches,
laswp.hip).  It only changes when and how rows are copied, never what is computed: LU and IPIV must be bit-identical with
the two-pass form (lazy_gather = 1) on the generator's matrix, which pivots in every panel."""
import pytest

pytestmark = pytest.mark.gpu

SIZES = [1536, 2304, 4096 + 77]   # even / odd number of panels, a narrower last panel


def _factor(c, A, nb, trailing=0, **opts):
    import torch
    for k, v in opts.items():
        c.set_option(k, v)
    W = A.clone()
    ipiv, info = c.factor(W, nb, trailing=trailing)
    c.synchronize()
    torch.cuda.synchronize()
    s = c.stats()
    assert s.hpanel_timeouts == 0
    return W, ipiv.clone(), info, s


def _same(a, b, what):
    import torch
    Wa, ipa, infoa, _ = a
    Wb, ipb, infob, _ = b
    assert infoa == infob, what
    assert torch.equal(ipa, ipb), f"{what}: {int((ipa != ipb).sum())} pivots differ"
    assert torch.equal(Wa, Wb), f"{what}: {int((Wa != Wb).sum())} LU elements differ"


@pytest.mark.parametrize("mode", ["fp64", "fp16"])
@pytest.mark.parametrize("nb", [128, 256])
@pytest.mark.parametrize("n", SIZES)
def test_onepass_bit_identical_to_two_pass(mpf, n, nb, mode):
    c = mpf.MPFContext(0)
    try:
        c.set_option("fp64_rowmajor_min_n", 0)   # small matrices take the row-major schedule too
        trailing = mpf.TRAIL_FP64 if mode == "fp64" else mpf.TRAIL_FP16   # (fp16: its default super-panel, snapshots every sb panels)
        A = c.matgen(n)
        old = _factor(c, A, nb, trailing, lazy_gather=1)
        new = _factor(c, A, nb, trailing, lazy_gather=2)
        again = _factor(c, A, nb, trailing, lazy_gather=2)
        _same(new, old, f"N={n} nb={nb} {mode}")
        _same(again, new, f"N={n} nb={nb} {mode}, second call")
        s_old, s_new = old[3], new[3]
        if mode == "fp16":
            assert s_new.superpanel > 1
        npanels, sb = (n + nb - 1) // nb, s_new.superpanel
        assert s_old.lazy_onepass_blocks == 0
        assert s_new.lazy_onepass_blocks == (npanels - 1) // sb * sb   # every block that is owed an interchange
    finally:
        c.close()


@pytest.mark.parametrize("nb", [128, 256])
def test_onepass_mixed_with_the_two_pass_path(mpf, nb):
    """lazy_onepass_max_rows below the first segments' length: those blocks go through the temporary, the later ones do not; at 0
    every block does."""
    n = 4096 + 77
    c = mpf.MPFContext(0)
    try:
        c.set_option("fp64_rowmajor_min_n", 0)
        A = c.matgen(n)
        old = _factor(c, A, nb, lazy_gather=1)
        mixed = _factor(c, A, nb, lazy_gather=2, lazy_onepass_max_rows=2048)
        none = _factor(c, A, nb, lazy_gather=2, lazy_onepass_max_rows=0)
        _same(mixed, old, "max_rows=2048")
        _same(none, old, "max_rows=0")
        # block b's segment has n - (b + 1) nb rows
        want = sum(1 for b in range((n + nb - 1) // nb - 1) if n - (b + 1) * nb <= 2048)
        assert 0 < want < (n + nb - 1) // nb - 1
        assert mixed[3].lazy_onepass_blocks == want
        assert none[3].lazy_onepass_blocks == 0
    finally:
        c.close()


@pytest.mark.parametrize("first_rows", [1023, 1024, 1025, 2 * 1024 + 1])
def test_onepass_segment_lengths_around_the_thread_grid(mpf, first_rows):
    """First segment of 1023 / 1024 / 1025 / 2049 rows: a workgroup whose upper threads hold nothing, a full slice, and a last slice of
    one row."""
    nb = 128
    n = first_rows + nb
    c = mpf.MPFContext(0)
    try:
        A = c.matgen(n)
        for rm_min in (0, 1 << 30):   # row-major and in-place look-ahead schedule
            old = _factor(c, A, nb, fp64_rowmajor_min_n=rm_min, lazy_gather=1)
            new = _factor(c, A, nb, fp64_rowmajor_min_n=rm_min, lazy_gather=2)
            _same(new, old, f"first segment {first_rows} rows, fp64_rowmajor_min_n={rm_min}")
            assert new[3].lazy_onepass_blocks == (n + nb - 1) // nb - 1
    finally:
        c.close()
