"""GPU tests of option fp16_fused (contract C2f, include/mpf_c.h): the fp16 pivot panel's rank-1 step as one fused multiply-add.

Reference: tests/hgetf2_fused_model.py (exact arithmetic, checked on the CPU by tests/test_hgetf2_fused_cpu.py); with the option off,
oracle.hgetf2 as everywhere else.  Pivots and fp16 bit patterns are compared exactly; every test asserts hpanel_timeouts == 0.
Panels whose fp16 factorization meets a zero pivot (inf / NaN) are outside the parity contract and skipped, as in
tests/test_gpu_steps.py -- never a generator-style or a normal one: those assert that they are finite.

Shapes: (2, 2) one workgroup, nothing to hand off; (33, 32); (256, 32) / (257, 32) the first hand-off between two workgroups;
(300, 128), (1000, 256), (2049, 256) partial last slabs; (511, 256) / (512, 256) full width on both sides of a slab boundary.  The
window form's shapes sit on both sides of its layout's seams (window of 136 columns, moved at column 120); (600, 300) is wider than
the LDS kernels take and always generic."""
import functools
import os

import numpy as np
import pytest

import hgetf2_fused_model as M
from conftest import bits16
from test_gpu_steps import _panel_case

pytestmark = pytest.mark.gpu

KINDS = ["gen", "ties", "sparse", "normal"]
STEP_SHAPES = [(2, 2), (33, 32), (256, 32), (257, 32), (300, 128), (511, 256), (512, 256), (1000, 256), (2049, 256)]
WINDOW_SHAPES = [(300, 120), (300, 121), (700, 136), (700, 137), (257, 255), (513, 256), (3000, 256)]
SLAB_SHAPES = [(1000, 256), (2049, 256)]
GENERIC_SHAPES = [(300, 128), (1000, 256), (600, 300)]
INPLACE_SHAPE = (700, 64)
# (kind, rows, cols, seed) of _panel_case: panels of at most 1024 x 128 on which the two contracts pick different pivots (found with the
# model: 43 of 64 pivots differ from column 14 on, 123 of 128 from column 4 on)
DIFFERING_PANELS = [("gen", 300, 64, 0), ("gen", 600, 128, 2)]


def _seed(rows, cols):
    return rows * 131 + cols


def all_panel_cases():
    """(rows, cols, seed) of every panel the tests below run each kind on."""
    shapes = STEP_SHAPES + WINDOW_SHAPES + SLAB_SHAPES + GENERIC_SHAPES + [INPLACE_SHAPE]
    return sorted({(r, c, _seed(r, c)) for r, c in shapes})


def finite16(bits):
    return bool(np.all((np.asarray(bits) & 0x7C00) != 0x7C00))


@functools.lru_cache(maxsize=None)
def _model(oracle, kind, rows, cols, seed, fused):
    """(pivots, factored bits, fp64 panel) of the reference on _panel_case: computed once, shared, read-only."""
    P = _panel_case(oracle, kind, rows, cols, seed)
    if fused:
        piv, bits = M.panel_pivots(P, oracle, True)
    else:
        bits = np.asfortranarray(oracle.double_to_fp16(P))
        piv = oracle.hgetf2(bits)
    for a in (piv, bits, P):
        a.setflags(write=False)
    return piv, bits, P


def _usable(kind, bits):
    """Zero pivot in the fp16 panel: skip -- but the generator-style and normal kinds never are."""
    if kind in ("gen", "normal"):
        assert finite16(bits), "a generator-style / normal panel met a zero pivot"
    elif not finite16(bits):
        pytest.skip("fp16 panel hit a zero pivot (inf/NaN): outside the parity contract")


class _options:
    """Set context options for a block and put the earlier values back."""

    def __init__(self, ctx, **opts):
        self.ctx, self.opts, self.before = ctx, opts, {}

    def __enter__(self):
        for k, v in self.opts.items():
            self.before[k] = self.ctx.get_option(k)
        try:
            for k, v in self.opts.items():
                self.ctx.set_option(k, v)
        except Exception:
            self.__exit__()
            raise
        return self.ctx

    def __exit__(self, *exc):
        for k, v in self.before.items():
            self.ctx.set_option(k, v)
        return False


def _panel_bits(panel, rows, cols):
    return np.asfortranarray(bits16(panel.t().contiguous()).reshape(cols, rows).T)


def _run_pivots(ctx, P, want_panel, off=5):
    ipiv, panel = ctx.hgetf2_pivots(ctx.from_numpy_f(P.copy(order="F")), ipiv_offset=off, want_panel=want_panel)   # (P is the shared, read-only case)
    ctx.synchronize()
    assert ctx.stats().hpanel_timeouts == 0
    return ipiv.cpu().numpy() - off, (_panel_bits(panel, *P.shape) if want_panel else None)


def _first_diff(a, b):
    return f"first diff at column {int(np.argmax(a != b))} of {int((a != b).sum())}"


# ---- the step operator against the model --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rows,cols", STEP_SHAPES)
def test_step_operator_pivots_and_panel_bits(ctx, oracle, kind, rows, cols):
    want_piv, want_bits, P = _model(oracle, kind, rows, cols, _seed(rows, cols), True)
    _usable(kind, want_bits)
    with _options(ctx, fp16_fused=1):
        got_piv, got_bits = _run_pivots(ctx, P, True)
    assert np.array_equal(got_piv, want_piv), _first_diff(got_piv, want_piv)
    assert M.same_bits(got_bits, want_bits)


# ---- every kernel form ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rows,cols", WINDOW_SHAPES)
def test_window_form_and_full_slab_form(ctx, oracle, kind, rows, cols):
    want_piv, want_bits, P = _model(oracle, kind, rows, cols, _seed(rows, cols), True)
    _usable(kind, want_bits)
    for window in (1, 0):
        with _options(ctx, fp16_fused=1, hp_window=window):
            got_piv, _ = _run_pivots(ctx, P, False)
        assert np.array_equal(got_piv, want_piv), f"hp_window={window}: " + _first_diff(got_piv, want_piv)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rows,cols", SLAB_SHAPES)
def test_half_slab_and_single_xcd_forms(ctx, oracle, kind, rows, cols):
    want_piv, want_bits, P = _model(oracle, kind, rows, cols, _seed(rows, cols), True)
    _usable(kind, want_bits)
    for half in (0, 1):
        for local in (0, 1):
            with _options(ctx, fp16_fused=1, hp_half_slabs=half, hp_local_xcd=local):
                got_piv, got_bits = _run_pivots(ctx, P, True)
            tag = f"hp_half_slabs={half} hp_local_xcd={local}: "
            assert np.array_equal(got_piv, want_piv), tag + _first_diff(got_piv, want_piv)
            assert M.same_bits(got_bits, want_bits), tag


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rows,cols", GENERIC_SHAPES)
def test_generic_path_both_forms(ctx, oracle, kind, rows, cols):
    want_piv, want_bits, P = _model(oracle, kind, rows, cols, _seed(rows, cols), True)
    _usable(kind, want_bits)
    for launches in (1, 0):
        with _options(ctx, fp16_fused=1, safe_pivots=1, generic_fused=launches):
            got_piv, got_bits = _run_pivots(ctx, P, True)
        tag = f"generic_fused={launches}: "
        assert np.array_equal(got_piv, want_piv), tag + _first_diff(got_piv, want_piv)
        assert M.same_bits(got_bits, want_bits), tag


@pytest.mark.parametrize("kind", KINDS)
def test_inplace_fp16_entry(ctx, oracle, kind):
    import torch
    rows, cols = INPLACE_SHAPE
    want_piv, want_bits, P = _model(oracle, kind, rows, cols, _seed(rows, cols), True)
    _usable(kind, want_bits)
    bits = oracle.double_to_fp16(P)
    for safe in (0, 1):
        d = torch.from_numpy(np.ascontiguousarray(bits.T).view(np.int16)).to(ctx.device).t()
        with _options(ctx, fp16_fused=1, safe_pivots=safe):
            ipiv = ctx.hgetf2(d)
            ctx.synchronize()
        assert ctx.stats().hpanel_timeouts == 0
        assert np.array_equal(ipiv.cpu().numpy(), want_piv), f"safe_pivots={safe}"
        assert M.same_bits(_panel_bits(d, rows, cols), want_bits), f"safe_pivots={safe}"


# ---- the switch itself ------------------------------------------------------------------------------------------------------------
def test_no_sticky_state(ctx, oracle):
    rows, cols = 1000, 256
    for kind in ("gen", "normal"):
        piv1, bits1, P = _model(oracle, kind, rows, cols, _seed(rows, cols), True)
        piv0, bits0, _ = _model(oracle, kind, rows, cols, _seed(rows, cols), False)
        assert not np.array_equal(piv0, piv1), "the case must tell the settings apart"
        with _options(ctx, fp16_fused=1):
            got_piv, got_bits = _run_pivots(ctx, P, True)
        assert np.array_equal(got_piv, piv1) and M.same_bits(got_bits, bits1)
        assert ctx.get_option("fp16_fused") == 0
        got_piv, got_bits = _run_pivots(ctx, P, True)          # the same context, option off again: the oracle's panel
        assert np.array_equal(got_piv, piv0), _first_diff(got_piv, piv0)
        assert M.same_bits(got_bits, bits0)


@pytest.mark.parametrize("kind,rows,cols,seed", DIFFERING_PANELS)
def test_the_contracts_differ_and_each_side_is_reproduced(ctx, oracle, kind, rows, cols, seed):
    assert rows <= 1024 and cols <= 128
    piv0, bits0, P = _model(oracle, kind, rows, cols, seed, False)
    piv1, bits1, _ = _model(oracle, kind, rows, cols, seed, True)
    assert finite16(bits0) and finite16(bits1)
    assert not np.array_equal(piv0, piv1)
    for fused, piv, bits in ((0, piv0, bits0), (1, piv1, bits1)):
        with _options(ctx, fp16_fused=fused):
            got_piv, got_bits = _run_pivots(ctx, P, True)
            win_piv, _ = _run_pivots(ctx, P, False)
        assert np.array_equal(got_piv, piv), f"fp16_fused={fused}: " + _first_diff(got_piv, piv)
        assert np.array_equal(win_piv, piv), f"fp16_fused={fused}"
        assert M.same_bits(got_bits, bits), f"fp16_fused={fused}"


def test_option_plumbing(ctx, mpf):
    assert "fp16_fused" in mpf.option_names()
    assert ctx.get_option("fp16_fused") == 0
    before = os.environ.get("MPF_FP16_FUSED")
    os.environ["MPF_FP16_FUSED"] = "1"
    try:
        c = mpf.MPFContext(0)
        try:
            assert c.get_option("fp16_fused") == 1
        finally:
            c.close()
    finally:
        if before is None:
            del os.environ["MPF_FP16_FUSED"]
        else:
            os.environ["MPF_FP16_FUSED"] = before
    assert ctx.get_option("fp16_fused") == 0        # a live context never reads the environment again


# ---- whole factorizations -----------------------------------------------------------------------------------------------------
def _bits64(t):
    return np.ascontiguousarray(t.t().contiguous().cpu().numpy()).view(np.uint64)


def _step_loop(ctx, dA, nb):
    """mpf_factor_dev's loop (MPF.cu:100-242) driven from outside through the step operators, under the context's options."""
    import torch
    n = dA.shape[0]
    ipiv = torch.arange(1, n + 1, dtype=torch.int32, device=ctx.device)
    for k in range(0, n, nb):
        pc, pr = min(nb, n - k), n - k
        if pr <= 1:
            break
        pv, _ = ctx.hgetf2_pivots(dA[k:, k:k + pc], ipiv_offset=k)
        ipiv[k:k + pc] = pv
        ctx.laswp(dA, k, pc, pv)
        ctx.dgetf2_npv(dA[k:, k:k + pc])
        if k + pc < n:
            ctx.dtrsm_llnu(dA[k:k + pc, k:k + pc], dA[k:k + pc, k + pc:])
            ctx.dgemm_minus(dA[k + pc:, k + pc:], dA[k + pc:, k:k + pc], dA[k:k + pc, k + pc:])
    ctx.synchronize()
    return ipiv


@pytest.mark.parametrize("n,nb", [(512, 256), (1536, 256), (1024, 128)])
def test_factor_fp64_every_schedule_and_the_step_operators(ctx, oracle, mpf, n, nb):
    A = oracle.matgen_skip(n)
    dA = ctx.from_numpy_f(A)
    runs = {"default": {}, "no_lookahead": {"no_lookahead": True}, "pivot_path": {"pivot_path": 1}, "superpanel_fp64": {}}
    got = {}
    for name, kw in runs.items():
        W = dA.clone()
        opts = {"superpanel_fp64": 2} if name == "superpanel_fp64" else {}
        with _options(ctx, **opts):
            ip, info = ctx.factor(W, nb, fp16_fused=1, **kw)
        ctx.synchronize()
        st = ctx.stats()
        assert info == 0 and st.hpanel_timeouts == 0 and st.fp16_fused == 1, name
        assert ctx.get_option("fp16_fused") == 0, "factor(fp16_fused=...) puts the option back"
        got[name] = (ip.cpu().numpy(), _bits64(W))
        if name == "default":
            lu_default = ctx.to_numpy_f(W)
    W = dA.clone()
    with _options(ctx, fp16_fused=1):
        ip = _step_loop(ctx, W, nb)
        assert ctx.stats().hpanel_timeouts == 0
        Ah = A.copy(order="F")
        iph, info = ctx.factor_host(Ah, nb)
        assert info == 0 and ctx.stats().hpanel_timeouts == 0 and ctx.stats().fp16_fused == 1
    got["step operators"] = (ip.cpu().numpy(), _bits64(W))
    got["factor_host"] = (iph, np.ascontiguousarray(Ah.T).view(np.uint64))
    ip0, lu0 = got["default"]
    for name, (ipx, lux) in got.items():
        assert np.array_equal(ipx, ip0), name
        assert np.array_equal(lux, lu0), name
    mx, _ = oracle.check_plu(A, lu_default, ip0)
    assert mx <= 1e-10, mx                                   # the reference's own criterion (benchmark.cpp:97)
    # option off: the stats say so, and the pivots are the other contract's
    W = dA.clone()
    ipd, _ = ctx.factor(W, nb)
    ctx.synchronize()
    assert ctx.stats().fp16_fused == 0 and ctx.stats().hpanel_timeouts == 0
    LU_o, ip_o = oracle.mpf(A, nb)
    assert np.array_equal(ipd.cpu().numpy(), ip_o) and np.array_equal(_bits64(W), np.ascontiguousarray(LU_o.T).view(np.uint64))


@pytest.mark.parametrize("n,nb", [(2048, 256), (1100, 64)])
def test_factor_fp16_trailing_modes(ctx, oracle, mpf, n, nb):
    """The acceptance check of tests/test_gpu_factor.py::test_fp16_modes_two_level_schedule_on_generator_matrices (its matrix, two of
    its sizes, its bounds: relative Frobenius error of P L U below 2e-2 with fp16 operands, 1e-5 with split ones; look-ahead and
    single stream give the same bits), with the option on.

    Which schedules must agree on IPIV: in these modes the trailing update accumulates in fp32, so a schedule that groups the
    update's K differently (another super-panel width: mpf_opts.superpanel; the generic schedule of pivot_path = 1, which cuts K to
    its operand images) rounds differently, the next panel's fp16 image differs, and so do its pivots -- with the option off as
    with it on (measured on the MI355X, plain fp16 operands, N = 2048, nb = 256: between the default schedule and
    pivot_path = 1 702 of 2048 pivots differ with the option off and 645 with it on, between the default and superpanel = 2
    1205 and 1186; split operands: 668 / 714 and 1225 / 1212; both figures are printed below).  The schedules that run the SAME arithmetic in another order of launches -- look-ahead, single stream, the chain
    not pipelined -- must return the same IPIV and the same bits; the regrouping ones must each pass the acceptance bound and
    repeat themselves."""
    import torch
    A = oracle.matgen_skip(n, skip=3)
    dA = ctx.from_numpy_f(A)

    def run(fused, **kw):
        opts = {k: kw.pop(k) for k in list(kw) if k == "chain_pipeline"}
        W = dA.clone()
        with _options(ctx, **opts):
            p, info = ctx.factor(W, nb, fp16_fused=fused, **kw)
        ctx.synchronize()
        st = ctx.stats()
        assert info == 0 and st.fp16_fused == fused and st.hpanel_timeouts == 0, kw
        return p, W

    for mode, tol in ((mpf.TRAIL_FP16, 2e-2), (mpf.TRAIL_FP16X3, 1e-5)):
        p, W = run(1, trailing=mode)
        for kw in ({"no_lookahead": True}, {"chain_pipeline": 0}):
            p2, W2 = run(1, trailing=mode, **kw)
            assert torch.equal(p, p2) and torch.equal(W, W2), (mode, kw)
        _, fro = oracle.check_plu(A, ctx.to_numpy_f(W), p.cpu().numpy())
        print(f"mode {mode} default schedule: fro = {fro:.3e}")
        assert fro < tol, (mode, fro)
        p_off, _ = run(0, trailing=mode)
        for kw in ({"pivot_path": 1}, {"superpanel": 2}):
            p3, W3 = run(1, trailing=mode, **kw)
            p3b, W3b = run(1, trailing=mode, **kw)
            assert torch.equal(p3, p3b) and torch.equal(W3, W3b), (mode, kw)
            _, fro3 = oracle.check_plu(A, ctx.to_numpy_f(W3), p3.cpu().numpy())
            p3_off, _ = run(0, trailing=mode, **kw)
            print(f"mode {mode} {kw}: fro = {fro3:.3e}; pivots differing from the default schedule's: "
                  f"option on {int((p3 != p).sum())}, option off {int((p3_off != p_off).sum())} of {n}")
            assert fro3 < tol, (mode, kw, fro3)


@pytest.mark.parametrize("search", [1, 2])
def test_no_effect_under_the_fp64_pivot_rules(ctx, mpf, search):
    n, nb = 515, 128
    A = np.asfortranarray(np.random.default_rng(search).standard_normal((n, n)))
    dA = ctx.from_numpy_f(A)
    out = []
    for fused in (0, 1):
        W = dA.clone()
        ip, info = ctx.factor(W, nb, pivot_search=search, fp16_fused=fused)
        ctx.synchronize()
        st = ctx.stats()
        assert info == 0 and st.pivot_search == search and st.fp16_fused == 0 and st.hpanel_timeouts == 0
        out.append((ip.cpu().numpy(), _bits64(W)))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
