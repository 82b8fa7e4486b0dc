"""GPU tests of the argument handling of the batched host entries (csrc/mpf_batched.cpp, rules in csrc/batch_args.h), through the C ABI
(the Python wrappers check first): the sixteen strided entries mpf_{getrf, getrs, getri, getdet, lange, gecon, residual,
gerfs}_batched[_blocked] and the eleven mpf_*_vbatched operator entries.

Every refusal an entry has is provoked with arguments that violate that rule alone, in the entry's own order, and the return code and
the exact text of mpf_last_error are compared with the literal table EXPECTED below.  Cases named "a + b" violate two rules that the
entry checks one after the other, and pin the order: the text is the first rule's.  The empty cases (n, batch or nrhs of 0, a
descriptor without matrices or rows) pass null pointers and impossible leading dimensions and strides and return 0.  The table was
recorded once from the library as it was before the strided entries were put on one host body per operator; where it disagrees with a
reading of the source, the table is right.  No case launches a kernel: every operand buffer is filled with 7 and is still so afterwards
(and each is large enough for n = 1025, the largest order named, should a refusal ever be missing).

The accepted calls: one per body at n = 3, batch = 2 on the default context through the _batched and the _batched_blocked entry -- the
blocked entry takes the small kernels at this order -- with every output compared bit for bit between the two."""
import numpy as np
import pytest

N, BATCH, NRHS = 3, 2, 2
LIMITS = {"_batched": 128, "_batched_blocked": 1024}
OVER = "limit + 1"                      # stands for the first order the family refuses: 129 or 1025
BIG = 1025
OPS = ["getrf", "getrs", "getri", "getdet", "lange", "gecon", "residual", "gerfs"]
VOPS = OPS + ["geequ", "laqge", "lascl2"]
MATS, RHS = ("A", "LU", "inv"), ("B", "X", "R")
F64 = {"A": 2 * BIG * BIG, "LU": 2 * BIG * BIG, "inv": 2 * BIG * BIG, "B": 4 * BIG, "X": 4 * BIG, "R": 4 * BIG, "W": 4 * BIG, "r": 2 * BIG,
       "c": 2 * BIG, "s": 2 * BIG, "mant": 16, "out": 16, "anorm": 16, "rcond": 16, "ainvnm": 16, "ferr": 16, "berr": 16, "rowcnd": 16,
       "colcnd": 16, "amax": 16, "spread": 32}
I32 = {"ipiv": 2 * BIG, "info": 16, "expo": 16, "iters": 16, "equed": 16}
NULLS = {name: None for name in list(F64) + list(I32) + ["V"]}
BAD = {**{"ld" + x: -1 for x in MATS + RHS}, **{"s" + x: -5 for x in MATS + RHS}}


def _ld(x):
    return ("ld" + x + " < n", {"ld" + x: N - 1})


def _st(x):
    return ("stride" + x + " small", {"s" + x: 1})


def _null(x):
    return ("null " + x, {x: None})


SIZES = ("n > limit", {"n": OVER})
PIVOTS = ("strideP < n", {"sP": N - 1})
NRHS_TRANS = [("nrhs < 0", {"nrhs": -1}), ("trans = 2", {"trans": 2})]
NORM = ("norm = X", {"norm": b"X"})
# per strided operator: one violation per check, in the order the entry checks them (pairs of neighbours make the "a + b" cases) ...
CHAIN = {
    "getrf": [SIZES, PIVOTS, _ld("A"), _st("A"), _null("A")],
    "getrs": [SIZES, PIVOTS, *NRHS_TRANS, _ld("LU"), _st("LU"), _ld("B"), _st("B"), _null("LU")],
    "getri": [SIZES, PIVOTS, _ld("LU"), _st("LU"), _ld("inv"), _st("inv"), _null("ipiv"), ("inv = LU", {"inv": "LU"})],
    "getdet": [SIZES, PIVOTS, _ld("LU"), _st("LU"), _null("LU")],
    "lange": [SIZES, NORM, _ld("A"), _st("A"), _null("A")],
    "gecon": [SIZES, ("norm = M", {"norm": b"M"}), _ld("LU"), _st("LU"), _null("LU")],
    "residual": [SIZES, *NRHS_TRANS, _ld("A"), _st("A"), _ld("X"), _st("X"), _ld("B"), _st("B"), _ld("R"), _st("R"), _null("A")],
    "gerfs": [SIZES, PIVOTS, *NRHS_TRANS, _ld("A"), _st("A"), _ld("LU"), _st("LU"), _ld("B"), _st("B"), _ld("X"), _st("X"), _null("A")],
}
# ... and the other ways to violate one of those checks
NEGATIVE = [("n < 0", {"n": -1}), ("batch < 0", {"batch": -1})]
MORE = {
    "getrf": [_null("ipiv")],
    "getrs": [("trans = -1", {"trans": -1}), _null("ipiv"), _null("B")],
    "getri": [_null("LU"), _null("inv"), ("inv inside LU", {"inv": "LU + 8"})],
    "getdet": [_null("ipiv"), _null("mant"), _null("expo")],
    "lange": [_null("out")],
    "gecon": [_null("anorm"), _null("rcond")],
    "residual": [("trans = -1", {"trans": -1}), _null("X"), _null("B"), _null("R")],
    "gerfs": [("trans = -1", {"trans": -1}), _null("LU"), _null("ipiv"), _null("B"), _null("X"), _null("berr")],
}
PAIRED = ("getrs", "getri", "gerfs")
HAS_NRHS = ("getrs", "residual", "gerfs")


def _strided_cases(op):
    """[(case name, overrides)] of one strided operator: refusals first, then the empty cases."""
    chain = CHAIN[op]
    cases = NEGATIVE + chain + MORE[op]
    if op in PAIRED:
        cases += [(a + " + " + b, {**ka, **kb}) for (a, ka), (b, kb) in zip(chain, chain[1:])]
    cases += [("empty: n = 0", {**NULLS, **BAD, "n": 0, "sP": 0}), ("empty: batch = 0", {**NULLS, **BAD, "batch": 0, "sP": -1})]
    if op in HAS_NRHS:
        cases += [("n > limit + trans = 2", {"n": OVER, "trans": 2}), ("trans = 2 + empty: n = 0", {"trans": 2, "n": 0}),
                  ("empty: nrhs = 0", {**NULLS, **BAD, "nrhs": 0})]
    return cases


def _pointer(e, k, name):
    v = k.get(name, name)
    if v is None:
        return None
    base, _, plus = v.partition(" + ")
    return e[base] + int(plus or 0)


def _strided_args(op, e, k, limit):
    """The arguments of mpf_<op>_batched[_blocked] after the context: packed operands of order n unless k says otherwise."""
    k = dict(k)
    if k.get("n") == OVER:
        k["n"] = limit + 1
    n, b, r = k.get("n", N), k.get("batch", BATCH), k.get("nrhs", NRHS)
    p = lambda name: _pointer(e, k, name)                                                  # noqa: E731
    mat = lambda x: (p(x), k.get("ld" + x, n), k.get("s" + x, n * n))                       # noqa: E731
    rhs = lambda x: (p(x), k.get("ld" + x, n), k.get("s" + x, n * r))                       # noqa: E731
    piv, trans = (p("ipiv"), k.get("sP", n)), k.get("trans", 0)
    return {
        "getrf": lambda: (*mat("A"), n, b, *piv, p("info"), 0),
        "getrs": lambda: (trans, *mat("LU"), n, b, *piv, r, *rhs("B")),
        "getri": lambda: (*mat("LU"), n, b, *piv, *mat("inv"), p("info")),
        "getdet": lambda: (*mat("LU"), n, b, *piv, p("mant"), p("expo")),
        "lange": lambda: (k.get("norm", b"1"), *mat("A"), n, b, p("out")),
        "gecon": lambda: (k.get("norm", b"1"), *mat("LU"), n, b, p("anorm"), p("rcond"), p("ainvnm")),
        "residual": lambda: (trans, *mat("A"), n, b, r, *rhs("X"), *rhs("B"), *rhs("R"), p("W")),
        "gerfs": lambda: (trans, *mat("A"), *mat("LU"), n, b, *piv, r, *rhs("B"), *rhs("X"), k.get("itmax", 0), p("ferr"), p("berr"), p("iters")),
    }[op]()


# ---- descriptors ------------------------------------------------------------------------------------------------------------------------
NO_VB, OTHER = ("null descriptor", {"vb": None}), ("another context", {"ctx": "other"})
VLD = lambda x: ("ld" + x + " < total_n", {"ld" + x: 2 * N - 1})                            # noqa: E731
VCHAIN = {
    "getrf": [NO_VB, OTHER, _null("A")],
    "getrs": [NO_VB, OTHER, *NRHS_TRANS, VLD("B"), _null("LU")],
    "getri": [NO_VB, OTHER, _null("ipiv"), ("inv = LU", {"inv": "LU"})],
    "getdet": [NO_VB, OTHER, _null("mant")],
    "lange": [NO_VB, OTHER, NORM, _null("out")],
    "gecon": [NO_VB, OTHER, ("norm = M", {"norm": b"M"}), _null("rcond")],
    "residual": [NO_VB, OTHER, *NRHS_TRANS, VLD("X"), VLD("B"), VLD("R"), _null("A")],
    "gerfs": [NO_VB, OTHER, *NRHS_TRANS, _null("berr"), VLD("B"), VLD("X"), _null("A")],
    "geequ": [NO_VB, OTHER, _null("rowcnd")],
    "laqge": [NO_VB, OTHER, ("rule = 3", {"rule": 3}), _null("rowcnd"), ("out inside A", {"out": "A + 8"})],
    "lascl2": [NO_VB, OTHER, ("nrhs < 0", {"nrhs": -1}), VLD("V"), _null("s")],
}
VMORE = {
    "getrf": [_null("ipiv")],
    "getrs": [("trans = -1", {"trans": -1}), _null("ipiv"), _null("B")],
    "getri": [_null("LU"), _null("inv"), ("inv inside LU", {"inv": "LU + 8"})],
    "getdet": [_null("expo"), _null("LU"), _null("ipiv")],
    "lange": [_null("A")],
    "gecon": [_null("LU"), _null("anorm")],
    "residual": [("trans = -1", {"trans": -1}), _null("X"), _null("B"), _null("R")],
    "gerfs": [("trans = -1", {"trans": -1}), _null("LU"), _null("ipiv"), _null("B"), _null("X")],
    "geequ": [_null("colcnd"), _null("amax"), _null("info"), _null("A"), _null("r"), _null("c")],
    "laqge": [("rule = -1", {"rule": -1}), _null("colcnd"), _null("amax"), _null("info"), _null("equed"), _null("A"), _null("r"), _null("c"),
              _null("out")],
    "lascl2": [_null("V")],
}
VPAIRED = ("getrs", "getri", "residual", "gerfs")
VBAD = {"ld" + x: -1 for x in RHS + ("V",)}
RETURNS_AT_NO_ROWS = ("getrs", "residual", "lascl2")      # total_n == 0: no work; the others write the order-0 outputs


def _vbatched_cases(op):
    chain = VCHAIN[op]
    cases = chain + VMORE[op]
    if op in VPAIRED:
        cases += [(a + " + " + b, {**ka, **kb}) for (a, ka), (b, kb) in zip(chain[1:], chain[2:])]
    cases += [("empty: batch = 0", {**NULLS, **VBAD, "vb": "none"})]
    if op in HAS_NRHS + ("lascl2",):
        cases += [("empty: nrhs = 0", {**NULLS, **VBAD, "nrhs": 0})]
    if op in RETURNS_AT_NO_ROWS:
        cases += [("empty: total_n = 0", {**NULLS, **VBAD, "vb": "zeros"})]
    return cases


def _vbatched_args(op, e, k):
    """The arguments of mpf_<op>_vbatched after the context and the descriptor: tall operands of total_n = 2 N rows unless k says otherwise."""
    p = lambda name: _pointer(e, k, name)                                                  # noqa: E731
    ld = lambda x: k.get("ld" + x, 2 * N)                                                  # noqa: E731
    r, trans, norm = k.get("nrhs", NRHS), k.get("trans", 0), k.get("norm", b"1")
    equil = (p("r"), p("c"), p("rowcnd"), p("colcnd"), p("amax"), p("info"))
    return {
        "getrf": lambda: (p("A"), p("ipiv"), p("info"), 0),
        "getrs": lambda: (trans, p("LU"), p("ipiv"), r, p("B"), ld("B")),
        "getri": lambda: (p("LU"), p("ipiv"), p("inv"), p("info")),
        "getdet": lambda: (p("LU"), p("ipiv"), p("mant"), p("expo")),
        "lange": lambda: (norm, p("A"), p("out")),
        "gecon": lambda: (norm, p("LU"), p("anorm"), p("rcond"), p("ainvnm")),
        "residual": lambda: (trans, p("A"), r, p("X"), ld("X"), p("B"), ld("B"), p("R"), ld("R"), p("W")),
        "gerfs": lambda: (trans, p("A"), p("LU"), p("ipiv"), r, p("B"), ld("B"), p("X"), ld("X"), 0, p("ferr"), p("berr"), p("iters")),
        "geequ": lambda: (p("A"), *equil),
        "laqge": lambda: (k.get("rule", 0), p("A"), *equil, _pointer(e, k, "out") if "out" in k else p("inv"), p("equed"), p("spread")),
        "lascl2": lambda: (p("s"), r, _pointer(e, {"V": k.get("V", "B")}, "V"), ld("V"), p("equed"), 1),
    }[op]()


def collect(ctx, mpf):
    """({"<entry>: <case>": [return code, text of mpf_last_error unless it is 0]} for every case, whether every buffer was left alone)."""
    import torch
    ctx._bind()
    L = ctx.L
    bufs = {name: torch.full((size,), 7.0, dtype=torch.float64, device=ctx.device) for name, size in F64.items()}
    bufs.update({name: torch.full((size,), 7, dtype=torch.int32, device=ctx.device) for name, size in I32.items()})
    e = {name: t.data_ptr() for name, t in bufs.items()}
    got = {}
    for op in OPS:
        for suffix, limit in LIMITS.items():
            fn = getattr(L, "mpf_" + op + suffix)
            for name, k in _strided_cases(op):
                rc = fn(ctx.h, *_strided_args(op, e, k, limit))
                got[f"{op}{suffix}: {name}"] = [rc, L.mpf_last_error(ctx.h).decode() if rc else ""]
    other = mpf.MPFContext(0)
    vbs = {"some": ctx.vbatch_blocked([N] * BATCH), "none": ctx.vbatch_blocked([]), "zeros": ctx.vbatch_blocked([0, 0])}
    try:
        for op in VOPS:
            fn = getattr(L, "mpf_" + op + "_vbatched")
            for name, k in _vbatched_cases(op):
                c = other if k.get("ctx") == "other" else ctx
                which = k.get("vb", "some")
                vb = vbs[which].h if which is not None else None
                rc = fn(c.h, vb, *_vbatched_args(op, e, k))
                got[f"{op}_vbatched: {name}"] = [rc, L.mpf_last_error(c.h).decode() if rc else ""]
    finally:
        for vb in vbs.values():
            vb.close()
        other.close()
    ctx.synchronize()
    untouched = all(bool((t == 7).all()) for t in bufs.values())
    return got, untouched


# {entry: {case: the text of the refusal (return code -1), or None where the call returns 0}}, recorded from the library before the
# change (see the module's text)
EXPECTED = {
    "getrf_batched": {
        "n < 0": "getrf_batched: n and batch must not be negative",
        "batch < 0": "getrf_batched: n and batch must not be negative",
        "n > limit": "getrf_batched: n > 128 is not a small matrix: factor it with mpf_factor_dev (and solve with mpf_getrs)",
        "strideP < n": "getrf_batched: stride of ipiv < n",
        "ldA < n": "getrf_batched: leading dimension of A < n",
        "strideA small": "getrf_batched: stride of A is smaller than one matrix",
        "null A": "getrf_batched: null pointer",
        "null ipiv": "getrf_batched: null pointer",
        "empty: n = 0": None,
        "empty: batch = 0": None,
    },
    "getrf_batched_blocked": {
        "n < 0": "getrf_batched_blocked: n and batch must not be negative",
        "batch < 0": "getrf_batched_blocked: n and batch must not be negative",
        "n > limit": "getrf_batched_blocked: n > 1024 is not a batch-sized matrix: factor it with mpf_factor_dev (and solve with mpf_getrs)",
        "strideP < n": "getrf_batched_blocked: stride of ipiv < n",
        "ldA < n": "getrf_batched_blocked: leading dimension of A < n",
        "strideA small": "getrf_batched_blocked: stride of A is smaller than one matrix",
        "null A": "getrf_batched_blocked: null pointer",
        "null ipiv": "getrf_batched_blocked: null pointer",
        "empty: n = 0": None,
        "empty: batch = 0": None,
    },
    "getrs_batched": {
        "n < 0": "getrs_batched: n and batch must not be negative",
        "batch < 0": "getrs_batched: n and batch must not be negative",
        "n > limit": "getrs_batched: n > 128 is not a small matrix: factor it with mpf_factor_dev (and solve with mpf_getrs)",
        "strideP < n": "getrs_batched: stride of ipiv < n",
        "nrhs < 0": "getrs_batched: nrhs must not be negative",
        "trans = 2": "getrs_batched: trans must be 0 or 1",
        "ldLU < n": "getrs_batched: leading dimension of LU < n",
        "strideLU small": "getrs_batched: stride of LU is smaller than one matrix",
        "ldB < n": "getrs_batched: leading dimension of B < n",
        "strideB small": "getrs_batched: stride of B is smaller than one matrix",
        "null LU": "getrs_batched: null pointer",
        "trans = -1": "getrs_batched: trans must be 0 or 1",
        "null ipiv": "getrs_batched: null pointer",
        "null B": "getrs_batched: null pointer",
        "n > limit + strideP < n": "getrs_batched: n > 128 is not a small matrix: factor it with mpf_factor_dev (and solve with mpf_getrs)",
        "strideP < n + nrhs < 0": "getrs_batched: stride of ipiv < n",
        "nrhs < 0 + trans = 2": "getrs_batched: nrhs must not be negative",
        "trans = 2 + ldLU < n": "getrs_batched: trans must be 0 or 1",
        "ldLU < n + strideLU small": "getrs_batched: leading dimension of LU < n",
        "strideLU small + ldB < n": "getrs_batched: stride of LU is smaller than one matrix",
        "ldB < n + strideB small": "getrs_batched: leading dimension of B < n",
        "strideB small + null LU": "getrs_batched: stride of B is smaller than one matrix",
        "empty: n = 0": None,
        "empty: batch = 0": None,
        "n > limit + trans = 2": "getrs_batched: n > 128 is not a small matrix: factor it with mpf_factor_dev (and solve with mpf_getrs)",
        "trans = 2 + empty: n = 0": "getrs_batched: trans must be 0 or 1",
        "empty: nrhs = 0": None,
    },
    "getrs_batched_blocked": {
        "n < 0": "getrs_batched_blocked: n and batch must not be negative",
        "batch < 0": "getrs_batched_blocked: n and batch must not be negative",
        "n > limit": "getrs_batched_blocked: n > 1024 is not a batch-sized matrix: factor it with mpf_factor_dev (and solve with mpf_getrs)",
        "strideP < n": "getrs_batched_blocked: stride of ipiv < n",
        "nrhs < 0": "getrs_batched_blocked: nrhs must not be negative",
        "trans = 2": "getrs_batched_blocked: trans must be 0 or 1",
        "ldLU < n": "getrs_batched_blocked: leading dimension of LU < n",
        "strideLU small": "getrs_batched_blocked: stride of LU is smaller than one matrix",
        "ldB < n": "getrs_batched_blocked: leading dimension of B < n",
        "strideB small": "getrs_batched_blocked: stride of B is smaller than one matrix",
        "null LU": "getrs_batched_blocked: null pointer",
        "trans = -1": "getrs_batched_blocked: trans must be 0 or 1",
        "null ipiv": "getrs_batched_blocked: null pointer",
        "null B": "getrs_batched_blocked: null pointer",
        "n > limit + strideP < n": "getrs_batched_blocked: n > 1024 is not a batch-sized matrix: factor it with mpf_factor_dev (and solve with mpf_getrs)",
        "strideP < n + nrhs < 0": "getrs_batched_blocked: stride of ipiv < n",
        "nrhs < 0 + trans = 2": "getrs_batched_blocked: nrhs must not be negative",
        "trans = 2 + ldLU < n": "getrs_batched_blocked: trans must be 0 or 1",
        "ldLU < n + strideLU small": "getrs_batched_blocked: leading dimension of LU < n",
        "strideLU small + ldB < n": "getrs_batched_blocked: stride of LU is smaller than one matrix",
        "ldB < n + strideB small": "getrs_batched_blocked: leading dimension of B < n",
        "strideB small + null LU": "getrs_batched_blocked: stride of B is smaller than one matrix",
        "empty: n = 0": None,
        "empty: batch = 0": None,
        "n > limit + trans = 2": "getrs_batched_blocked: n > 1024 is not a batch-sized matrix: factor it with mpf_factor_dev (and solve with mpf_getrs)",
        "trans = 2 + empty: n = 0": "getrs_batched_blocked: trans must be 0 or 1",
        "empty: nrhs = 0": None,
    },
    "getri_batched": {
        "n < 0": "getri_batched: n and batch must not be negative",
        "batch < 0": "getri_batched: n and batch must not be negative",
        "n > limit": "getri_batched: n > 128 is not a small matrix: factor it with mpf_factor_dev (and solve with mpf_getrs)",
        "strideP < n": "getri_batched: stride of ipiv < n",
        "ldLU < n": "getri_batched: leading dimension of LU < n",
        "strideLU small": "getri_batched: stride of LU is smaller than one matrix",
        "ldinv < n": "getri_batched: leading dimension of inv < n",
        "strideinv small": "getri_batched: stride of inv is smaller than one matrix",
        "null ipiv": "getri_batched: null pointer",
        "inv = LU": "getri_batched: d_inv overlaps d_LU (the inverse is formed out of place)",
        "null LU": "getri_batched: null pointer",
        "null inv": "getri_batched: null pointer",
        "inv inside LU": "getri_batched: d_inv overlaps d_LU (the inverse is formed out of place)",
        "n > limit + strideP < n": "getri_batched: n > 128 is not a small matrix: factor it with mpf_factor_dev (and solve with mpf_getrs)",
        "strideP < n + ldLU < n": "getri_batched: stride of ipiv < n",
        "ldLU < n + strideLU small": "getri_batched: leading dimension of LU < n",
        "strideLU small + ldinv < n": "getri_batched: stride of LU is smaller than one matrix",
        "ldinv < n + strideinv small": "getri_batched: leading dimension of inv < n",
        "strideinv small + null ipiv": "getri_batched: stride of inv is smaller than one matrix",
        "null ipiv + inv = LU": "getri_batched: null pointer",
        "empty: n = 0": None,
        "empty: batch = 0": None,
    },
    "getri_batched_blocked": {
        "n < 0": "getri_batched_blocked: n and batch must not be negative",
        "batch < 0": "getri_batched_blocked: n and batch must not be negative",
        "n > limit": "getri_batched_blocked: n > 1024 is not a batch-sized matrix: factor it with mpf_factor_dev (and invert with mpf_getri)",
        "strideP < n": "getri_batched_blocked: stride of ipiv < n",
        "ldLU < n": "getri_batched_blocked: leading dimension of LU < n",
        "strideLU small": "getri_batched_blocked: stride of LU is smaller than one matrix",
        "ldinv < n": "getri_batched_blocked: leading dimension of inv < n",
        "strideinv small": "getri_batched_blocked: stride of inv is smaller than one matrix",
        "null ipiv": "getri_batched_blocked: null pointer",
        "inv = LU": "getri_batched_blocked: d_inv overlaps d_LU (the inverse is formed out of place)",
        "null LU": "getri_batched_blocked: null pointer",
        "null inv": "getri_batched_blocked: null pointer",
        "inv inside LU": "getri_batched_blocked: d_inv overlaps d_LU (the inverse is formed out of place)",
        "n > limit + strideP < n": "getri_batched_blocked: n > 1024 is not a batch-sized matrix: factor it with mpf_factor_dev (and invert with mpf_getri)",
        "strideP < n + ldLU < n": "getri_batched_blocked: stride of ipiv < n",
        "ldLU < n + strideLU small": "getri_batched_blocked: leading dimension of LU < n",
        "strideLU small + ldinv < n": "getri_batched_blocked: stride of LU is smaller than one matrix",
        "ldinv < n + strideinv small": "getri_batched_blocked: leading dimension of inv < n",
        "strideinv small + null ipiv": "getri_batched_blocked: stride of inv is smaller than one matrix",
        "null ipiv + inv = LU": "getri_batched_blocked: null pointer",
        "empty: n = 0": None,
        "empty: batch = 0": None,
    },
    "getdet_batched": {
        "n < 0": "getdet_batched: n and batch must not be negative",
        "batch < 0": "getdet_batched: n and batch must not be negative",
        "n > limit": "getdet_batched: n > 128 is not a small matrix: factor it with mpf_factor_dev (and solve with mpf_getrs)",
        "strideP < n": "getdet_batched: stride of ipiv < n",
        "ldLU < n": "getdet_batched: leading dimension of LU < n",
        "strideLU small": "getdet_batched: stride of LU is smaller than one matrix",
        "null LU": "getdet_batched: null pointer",
        "null ipiv": "getdet_batched: null pointer",
        "null mant": "getdet_batched: null pointer",
        "null expo": "getdet_batched: null pointer",
        "empty: n = 0": None,
        "empty: batch = 0": None,
    },
    "getdet_batched_blocked": {
        "n < 0": "getdet_batched_blocked: n and batch must not be negative",
        "batch < 0": "getdet_batched_blocked: n and batch must not be negative",
        "n > limit": "getdet_batched_blocked: n > 1024 is not a batch-sized matrix: factor it with mpf_factor_dev (and take the determinant with mpf_getdet)",
        "strideP < n": "getdet_batched_blocked: stride of ipiv < n",
        "ldLU < n": "getdet_batched_blocked: leading dimension of LU < n",
        "strideLU small": "getdet_batched_blocked: stride of LU is smaller than one matrix",
        "null LU": "getdet_batched_blocked: null pointer",
        "null ipiv": "getdet_batched_blocked: null pointer",
        "null mant": "getdet_batched_blocked: null pointer",
        "null expo": "getdet_batched_blocked: null pointer",
        "empty: n = 0": None,
        "empty: batch = 0": None,
    },
    "lange_batched": {
        "n < 0": "lange_batched: n and batch must not be negative",
        "batch < 0": "lange_batched: n and batch must not be negative",
        "n > limit": "lange_batched: n > 128 is not a small matrix: use mpf_lange (and mpf_gecon / mpf_gerfs) on one matrix at a time",
        "norm = X": "lange_batched: norm must be '1', 'O', 'I' or 'M'",
        "ldA < n": "lange_batched: leading dimension of A < n",
        "strideA small": "lange_batched: stride of A is smaller than one matrix",
        "null A": "lange_batched: null pointer",
        "null out": "lange_batched: null pointer",
        "empty: n = 0": None,
        "empty: batch = 0": None,
    },
    "lange_batched_blocked": {
        "n < 0": "lange_batched_blocked: n and batch must not be negative",
        "batch < 0": "lange_batched_blocked: n and batch must not be negative",
        "n > limit": "lange_batched_blocked: n > 1024 is not a batch-sized matrix: use mpf_lange, mpf_gecon / mpf_gerfs on one matrix at a time",
        "norm = X": "lange_batched_blocked: norm must be '1', 'O', 'I' or 'M'",
        "ldA < n": "lange_batched_blocked: leading dimension of A < n",
        "strideA small": "lange_batched_blocked: stride of A is smaller than one matrix",
        "null A": "lange_batched_blocked: null pointer",
        "null out": "lange_batched_blocked: null pointer",
        "empty: n = 0": None,
        "empty: batch = 0": None,
    },
    "gecon_batched": {
        "n < 0": "gecon_batched: n and batch must not be negative",
        "batch < 0": "gecon_batched: n and batch must not be negative",
        "n > limit": "gecon_batched: n > 128 is not a small matrix: use mpf_gecon (and mpf_gerfs) on one matrix at a time",
        "norm = M": "gecon_batched: norm must be '1', 'O' or 'I'",
        "ldLU < n": "gecon_batched: leading dimension of LU < n",
        "strideLU small": "gecon_batched: stride of LU is smaller than one matrix",
        "null LU": "gecon_batched: null pointer",
        "null anorm": "gecon_batched: null pointer",
        "null rcond": "gecon_batched: null pointer",
        "empty: n = 0": None,
        "empty: batch = 0": None,
    },
    "gecon_batched_blocked": {
        "n < 0": "gecon_batched_blocked: n and batch must not be negative",
        "batch < 0": "gecon_batched_blocked: n and batch must not be negative",
        "n > limit": "gecon_batched_blocked: n > 1024 is not a batch-sized matrix: use mpf_lange, mpf_gecon / mpf_gerfs on one matrix at a time",
        "norm = M": "gecon_batched_blocked: norm must be '1', 'O' or 'I'",
        "ldLU < n": "gecon_batched_blocked: leading dimension of LU < n",
        "strideLU small": "gecon_batched_blocked: stride of LU is smaller than one matrix",
        "null LU": "gecon_batched_blocked: null pointer",
        "null anorm": "gecon_batched_blocked: null pointer",
        "null rcond": "gecon_batched_blocked: null pointer",
        "empty: n = 0": None,
        "empty: batch = 0": None,
    },
    "residual_batched": {
        "n < 0": "residual_batched: n and batch must not be negative",
        "batch < 0": "residual_batched: n and batch must not be negative",
        "n > limit": "residual_batched: n > 128 is not a small matrix: use mpf_gerfs (and mpf_gecon) on one matrix at a time",
        "nrhs < 0": "residual_batched: nrhs must not be negative",
        "trans = 2": "residual_batched: trans must be 0 or 1",
        "ldA < n": "residual_batched: leading dimension of A < n",
        "strideA small": "residual_batched: stride of A is smaller than one matrix",
        "ldX < n": "residual_batched: leading dimension of X < n",
        "strideX small": "residual_batched: stride of X is smaller than one matrix",
        "ldB < n": "residual_batched: leading dimension of B < n",
        "strideB small": "residual_batched: stride of B is smaller than one matrix",
        "ldR < n": "residual_batched: leading dimension of R < n",
        "strideR small": "residual_batched: stride of R is smaller than one matrix",
        "null A": "residual_batched: null pointer",
        "trans = -1": "residual_batched: trans must be 0 or 1",
        "null X": "residual_batched: null pointer",
        "null B": "residual_batched: null pointer",
        "null R": "residual_batched: null pointer",
        "empty: n = 0": None,
        "empty: batch = 0": None,
        "n > limit + trans = 2": "residual_batched: n > 128 is not a small matrix: use mpf_gerfs (and mpf_gecon) on one matrix at a time",
        "trans = 2 + empty: n = 0": "residual_batched: trans must be 0 or 1",
        "empty: nrhs = 0": None,
    },
    "residual_batched_blocked": {
        "n < 0": "residual_batched_blocked: n and batch must not be negative",
        "batch < 0": "residual_batched_blocked: n and batch must not be negative",
        "n > limit": "residual_batched_blocked: n > 1024 is not a batch-sized matrix: use mpf_lange, mpf_gecon / mpf_gerfs on one matrix at a time",
        "nrhs < 0": "residual_batched_blocked: nrhs must not be negative",
        "trans = 2": "residual_batched_blocked: trans must be 0 or 1",
        "ldA < n": "residual_batched_blocked: leading dimension of A < n",
        "strideA small": "residual_batched_blocked: stride of A is smaller than one matrix",
        "ldX < n": "residual_batched_blocked: leading dimension of X < n",
        "strideX small": "residual_batched_blocked: stride of X is smaller than one matrix",
        "ldB < n": "residual_batched_blocked: leading dimension of B < n",
        "strideB small": "residual_batched_blocked: stride of B is smaller than one matrix",
        "ldR < n": "residual_batched_blocked: leading dimension of R < n",
        "strideR small": "residual_batched_blocked: stride of R is smaller than one matrix",
        "null A": "residual_batched_blocked: null pointer",
        "trans = -1": "residual_batched_blocked: trans must be 0 or 1",
        "null X": "residual_batched_blocked: null pointer",
        "null B": "residual_batched_blocked: null pointer",
        "null R": "residual_batched_blocked: null pointer",
        "empty: n = 0": None,
        "empty: batch = 0": None,
        "n > limit + trans = 2": "residual_batched_blocked: n > 1024 is not a batch-sized matrix: use mpf_lange, mpf_gecon / mpf_gerfs on one matrix at a time",
        "trans = 2 + empty: n = 0": "residual_batched_blocked: trans must be 0 or 1",
        "empty: nrhs = 0": None,
    },
    "gerfs_batched": {
        "n < 0": "gerfs_batched: n and batch must not be negative",
        "batch < 0": "gerfs_batched: n and batch must not be negative",
        "n > limit": "gerfs_batched: n > 128 is not a small matrix: use mpf_gerfs (and mpf_gecon) on one matrix at a time",
        "strideP < n": "gerfs_batched: stride of ipiv < n",
        "nrhs < 0": "gerfs_batched: nrhs must not be negative",
        "trans = 2": "gerfs_batched: trans must be 0 or 1",
        "ldA < n": "gerfs_batched: leading dimension of A < n",
        "strideA small": "gerfs_batched: stride of A is smaller than one matrix",
        "ldLU < n": "gerfs_batched: leading dimension of LU < n",
        "strideLU small": "gerfs_batched: stride of LU is smaller than one matrix",
        "ldB < n": "gerfs_batched: leading dimension of B < n",
        "strideB small": "gerfs_batched: stride of B is smaller than one matrix",
        "ldX < n": "gerfs_batched: leading dimension of X < n",
        "strideX small": "gerfs_batched: stride of X is smaller than one matrix",
        "null A": "gerfs_batched: null pointer",
        "trans = -1": "gerfs_batched: trans must be 0 or 1",
        "null LU": "gerfs_batched: null pointer",
        "null ipiv": "gerfs_batched: null pointer",
        "null B": "gerfs_batched: null pointer",
        "null X": "gerfs_batched: null pointer",
        "null berr": "gerfs_batched: null pointer",
        "n > limit + strideP < n": "gerfs_batched: n > 128 is not a small matrix: use mpf_gerfs (and mpf_gecon) on one matrix at a time",
        "strideP < n + nrhs < 0": "gerfs_batched: stride of ipiv < n",
        "nrhs < 0 + trans = 2": "gerfs_batched: nrhs must not be negative",
        "trans = 2 + ldA < n": "gerfs_batched: trans must be 0 or 1",
        "ldA < n + strideA small": "gerfs_batched: leading dimension of A < n",
        "strideA small + ldLU < n": "gerfs_batched: stride of A is smaller than one matrix",
        "ldLU < n + strideLU small": "gerfs_batched: leading dimension of LU < n",
        "strideLU small + ldB < n": "gerfs_batched: stride of LU is smaller than one matrix",
        "ldB < n + strideB small": "gerfs_batched: leading dimension of B < n",
        "strideB small + ldX < n": "gerfs_batched: stride of B is smaller than one matrix",
        "ldX < n + strideX small": "gerfs_batched: leading dimension of X < n",
        "strideX small + null A": "gerfs_batched: stride of X is smaller than one matrix",
        "empty: n = 0": None,
        "empty: batch = 0": None,
        "n > limit + trans = 2": "gerfs_batched: n > 128 is not a small matrix: use mpf_gerfs (and mpf_gecon) on one matrix at a time",
        "trans = 2 + empty: n = 0": "gerfs_batched: trans must be 0 or 1",
        "empty: nrhs = 0": None,
    },
    "gerfs_batched_blocked": {
        "n < 0": "gerfs_batched_blocked: n and batch must not be negative",
        "batch < 0": "gerfs_batched_blocked: n and batch must not be negative",
        "n > limit": "gerfs_batched_blocked: n > 1024 is not a batch-sized matrix: use mpf_lange, mpf_gecon / mpf_gerfs on one matrix at a time",
        "strideP < n": "gerfs_batched_blocked: stride of ipiv < n",
        "nrhs < 0": "gerfs_batched_blocked: nrhs must not be negative",
        "trans = 2": "gerfs_batched_blocked: trans must be 0 or 1",
        "ldA < n": "gerfs_batched_blocked: leading dimension of A < n",
        "strideA small": "gerfs_batched_blocked: stride of A is smaller than one matrix",
        "ldLU < n": "gerfs_batched_blocked: leading dimension of LU < n",
        "strideLU small": "gerfs_batched_blocked: stride of LU is smaller than one matrix",
        "ldB < n": "gerfs_batched_blocked: leading dimension of B < n",
        "strideB small": "gerfs_batched_blocked: stride of B is smaller than one matrix",
        "ldX < n": "gerfs_batched_blocked: leading dimension of X < n",
        "strideX small": "gerfs_batched_blocked: stride of X is smaller than one matrix",
        "null A": "gerfs_batched_blocked: null pointer",
        "trans = -1": "gerfs_batched_blocked: trans must be 0 or 1",
        "null LU": "gerfs_batched_blocked: null pointer",
        "null ipiv": "gerfs_batched_blocked: null pointer",
        "null B": "gerfs_batched_blocked: null pointer",
        "null X": "gerfs_batched_blocked: null pointer",
        "null berr": "gerfs_batched_blocked: null pointer",
        "n > limit + strideP < n": "gerfs_batched_blocked: n > 1024 is not a batch-sized matrix: use mpf_lange, mpf_gecon / mpf_gerfs on one matrix at a time",
        "strideP < n + nrhs < 0": "gerfs_batched_blocked: stride of ipiv < n",
        "nrhs < 0 + trans = 2": "gerfs_batched_blocked: nrhs must not be negative",
        "trans = 2 + ldA < n": "gerfs_batched_blocked: trans must be 0 or 1",
        "ldA < n + strideA small": "gerfs_batched_blocked: leading dimension of A < n",
        "strideA small + ldLU < n": "gerfs_batched_blocked: stride of A is smaller than one matrix",
        "ldLU < n + strideLU small": "gerfs_batched_blocked: leading dimension of LU < n",
        "strideLU small + ldB < n": "gerfs_batched_blocked: stride of LU is smaller than one matrix",
        "ldB < n + strideB small": "gerfs_batched_blocked: leading dimension of B < n",
        "strideB small + ldX < n": "gerfs_batched_blocked: stride of B is smaller than one matrix",
        "ldX < n + strideX small": "gerfs_batched_blocked: leading dimension of X < n",
        "strideX small + null A": "gerfs_batched_blocked: stride of X is smaller than one matrix",
        "empty: n = 0": None,
        "empty: batch = 0": None,
        "n > limit + trans = 2": "gerfs_batched_blocked: n > 1024 is not a batch-sized matrix: use mpf_lange, mpf_gecon / mpf_gerfs on one matrix at a time",
        "trans = 2 + empty: n = 0": "gerfs_batched_blocked: trans must be 0 or 1",
        "empty: nrhs = 0": None,
    },
    "getrf_vbatched": {
        "null descriptor": "getrf_vbatched: null pointer (descriptor)",
        "another context": "getrf_vbatched: the descriptor belongs to another context",
        "null A": "getrf_vbatched: null pointer",
        "null ipiv": "getrf_vbatched: null pointer",
        "empty: batch = 0": None,
    },
    "getrs_vbatched": {
        "null descriptor": "getrs_vbatched: null pointer (descriptor)",
        "another context": "getrs_vbatched: the descriptor belongs to another context",
        "nrhs < 0": "getrs_vbatched: nrhs must not be negative",
        "trans = 2": "getrs_vbatched: trans must be 0 or 1",
        "ldB < total_n": "getrs_vbatched: leading dimension of B < total_n",
        "null LU": "getrs_vbatched: null pointer",
        "trans = -1": "getrs_vbatched: trans must be 0 or 1",
        "null ipiv": "getrs_vbatched: null pointer",
        "null B": "getrs_vbatched: null pointer",
        "another context + nrhs < 0": "getrs_vbatched: the descriptor belongs to another context",
        "nrhs < 0 + trans = 2": "getrs_vbatched: nrhs must not be negative",
        "trans = 2 + ldB < total_n": "getrs_vbatched: trans must be 0 or 1",
        "ldB < total_n + null LU": "getrs_vbatched: leading dimension of B < total_n",
        "empty: batch = 0": None,
        "empty: nrhs = 0": None,
        "empty: total_n = 0": None,
    },
    "getri_vbatched": {
        "null descriptor": "getri_vbatched: null pointer (descriptor)",
        "another context": "getri_vbatched: the descriptor belongs to another context",
        "null ipiv": "getri_vbatched: null pointer",
        "inv = LU": "getri_vbatched: d_inv overlaps d_LU (the inverse is formed out of place)",
        "null LU": "getri_vbatched: null pointer",
        "null inv": "getri_vbatched: null pointer",
        "inv inside LU": "getri_vbatched: d_inv overlaps d_LU (the inverse is formed out of place)",
        "another context + null ipiv": "getri_vbatched: the descriptor belongs to another context",
        "null ipiv + inv = LU": "getri_vbatched: null pointer",
        "empty: batch = 0": None,
    },
    "getdet_vbatched": {
        "null descriptor": "getdet_vbatched: null pointer (descriptor)",
        "another context": "getdet_vbatched: the descriptor belongs to another context",
        "null mant": "getdet_vbatched: null pointer",
        "null expo": "getdet_vbatched: null pointer",
        "null LU": "getdet_vbatched: null pointer",
        "null ipiv": "getdet_vbatched: null pointer",
        "empty: batch = 0": None,
    },
    "lange_vbatched": {
        "null descriptor": "lange_vbatched: null pointer (descriptor)",
        "another context": "lange_vbatched: the descriptor belongs to another context",
        "norm = X": "lange_vbatched: norm must be '1', 'O', 'I' or 'M'",
        "null out": "lange_vbatched: null pointer",
        "null A": "lange_vbatched: null pointer",
        "empty: batch = 0": None,
    },
    "gecon_vbatched": {
        "null descriptor": "gecon_vbatched: null pointer (descriptor)",
        "another context": "gecon_vbatched: the descriptor belongs to another context",
        "norm = M": "gecon_vbatched: norm must be '1', 'O' or 'I'",
        "null rcond": "gecon_vbatched: null pointer",
        "null LU": "gecon_vbatched: null pointer",
        "null anorm": "gecon_vbatched: null pointer",
        "empty: batch = 0": None,
    },
    "residual_vbatched": {
        "null descriptor": "residual_vbatched: null pointer (descriptor)",
        "another context": "residual_vbatched: the descriptor belongs to another context",
        "nrhs < 0": "residual_vbatched: nrhs must not be negative",
        "trans = 2": "residual_vbatched: trans must be 0 or 1",
        "ldX < total_n": "residual_vbatched: leading dimension of X < total_n",
        "ldB < total_n": "residual_vbatched: leading dimension of B < total_n",
        "ldR < total_n": "residual_vbatched: leading dimension of R < total_n",
        "null A": "residual_vbatched: null pointer",
        "trans = -1": "residual_vbatched: trans must be 0 or 1",
        "null X": "residual_vbatched: null pointer",
        "null B": "residual_vbatched: null pointer",
        "null R": "residual_vbatched: null pointer",
        "another context + nrhs < 0": "residual_vbatched: the descriptor belongs to another context",
        "nrhs < 0 + trans = 2": "residual_vbatched: nrhs must not be negative",
        "trans = 2 + ldX < total_n": "residual_vbatched: trans must be 0 or 1",
        "ldX < total_n + ldB < total_n": "residual_vbatched: leading dimension of X < total_n",
        "ldB < total_n + ldR < total_n": "residual_vbatched: leading dimension of B < total_n",
        "ldR < total_n + null A": "residual_vbatched: leading dimension of R < total_n",
        "empty: batch = 0": None,
        "empty: nrhs = 0": None,
        "empty: total_n = 0": None,
    },
    "gerfs_vbatched": {
        "null descriptor": "gerfs_vbatched: null pointer (descriptor)",
        "another context": "gerfs_vbatched: the descriptor belongs to another context",
        "nrhs < 0": "gerfs_vbatched: nrhs must not be negative",
        "trans = 2": "gerfs_vbatched: trans must be 0 or 1",
        "null berr": "gerfs_vbatched: null pointer",
        "ldB < total_n": "gerfs_vbatched: leading dimension of B < total_n",
        "ldX < total_n": "gerfs_vbatched: leading dimension of X < total_n",
        "null A": "gerfs_vbatched: null pointer",
        "trans = -1": "gerfs_vbatched: trans must be 0 or 1",
        "null LU": "gerfs_vbatched: null pointer",
        "null ipiv": "gerfs_vbatched: null pointer",
        "null B": "gerfs_vbatched: null pointer",
        "null X": "gerfs_vbatched: null pointer",
        "another context + nrhs < 0": "gerfs_vbatched: the descriptor belongs to another context",
        "nrhs < 0 + trans = 2": "gerfs_vbatched: nrhs must not be negative",
        "trans = 2 + null berr": "gerfs_vbatched: trans must be 0 or 1",
        "null berr + ldB < total_n": "gerfs_vbatched: null pointer",
        "ldB < total_n + ldX < total_n": "gerfs_vbatched: leading dimension of B < total_n",
        "ldX < total_n + null A": "gerfs_vbatched: leading dimension of X < total_n",
        "empty: batch = 0": None,
        "empty: nrhs = 0": None,
    },
    "geequ_vbatched": {
        "null descriptor": "geequ_vbatched: null pointer (descriptor)",
        "another context": "geequ_vbatched: the descriptor belongs to another context",
        "null rowcnd": "geequ_vbatched: null pointer",
        "null colcnd": "geequ_vbatched: null pointer",
        "null amax": "geequ_vbatched: null pointer",
        "null info": "geequ_vbatched: null pointer",
        "null A": "geequ_vbatched: null pointer",
        "null r": "geequ_vbatched: null pointer",
        "null c": "geequ_vbatched: null pointer",
        "empty: batch = 0": None,
    },
    "laqge_vbatched": {
        "null descriptor": "laqge_vbatched: null pointer (descriptor)",
        "another context": "laqge_vbatched: the descriptor belongs to another context",
        "rule = 3": "laqge_vbatched: rule must be 0, 1 or 2",
        "null rowcnd": "laqge_vbatched: null pointer",
        "out inside A": "laqge_vbatched: d_out overlaps d_A (in place is d_out == d_A)",
        "rule = -1": "laqge_vbatched: rule must be 0, 1 or 2",
        "null colcnd": "laqge_vbatched: null pointer",
        "null amax": "laqge_vbatched: null pointer",
        "null info": "laqge_vbatched: null pointer",
        "null equed": "laqge_vbatched: null pointer",
        "null A": "laqge_vbatched: null pointer",
        "null r": "laqge_vbatched: null pointer",
        "null c": "laqge_vbatched: null pointer",
        "null out": "laqge_vbatched: null pointer",
        "empty: batch = 0": None,
    },
    "lascl2_vbatched": {
        "null descriptor": "lascl2_vbatched: null pointer (descriptor)",
        "another context": "lascl2_vbatched: the descriptor belongs to another context",
        "nrhs < 0": "lascl2_vbatched: nrhs must not be negative",
        "ldV < total_n": "lascl2_vbatched: leading dimension of V < total_n",
        "null s": "lascl2_vbatched: null pointer",
        "null V": "lascl2_vbatched: null pointer",
        "empty: batch = 0": None,
        "empty: nrhs = 0": None,
        "empty: total_n = 0": None,
    },
}


@pytest.fixture(scope="module")
def recorded(ctx, mpf):
    """collect() once for every test of the table; nothing was written by any of its calls."""
    got, untouched = collect(ctx, mpf)
    assert untouched
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("entry", list(EXPECTED))
def test_refusals_and_empty_cases_of(recorded, entry):
    got = {key.split(": ", 1)[1]: value for key, value in recorded.items() if key.startswith(entry + ": ")}
    want = {case: [0, ""] if text is None else [-1, text] for case, text in EXPECTED[entry].items()}
    assert sorted(got) == sorted(want)
    wrong = {case: (got[case], want[case]) for case in want if got[case] != want[case]}
    assert not wrong, wrong


def test_the_table_names_the_entry_and_a_pair_has_the_text_of_its_first_rule():
    """The table itself (no GPU): 16 strided and 11 vbatched entries, 433 cases; a refusal's text begins with the entry's name, exactly
    the empty cases are accepted, and a case that violates two rules has the text of the one checked first."""
    assert sorted(EXPECTED) == sorted([op + suffix for op in OPS for suffix in LIMITS] + [op + "_vbatched" for op in VOPS])
    assert sum(len(cases) for cases in EXPECTED.values()) == 433
    for entry, cases in EXPECTED.items():
        for case, text in cases.items():
            assert (text is None) == case.startswith("empty"), (entry, case)
            assert text is None or text.startswith(entry + ": "), (entry, case)
            if " + " in case:
                assert text == cases[case.split(" + ")[0]], (entry, case)


def _bits(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint64 if t.element_size() == 8 else np.uint32)


def _accepted(ctx, suffix):
    """Every body once at n = 3, batch = 2 through the entries with this suffix: {output name: tensor}."""
    import torch
    ctx._bind()
    L, h = ctx.L, ctx.h
    rng = np.random.default_rng(2027)
    dev = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(ctx.device)   # noqa: E731
    # column-major matrices as rows of a (batch, cols, rows) array
    A = dev(rng.standard_normal((BATCH, N, N)))
    B = dev(rng.standard_normal((BATCH, NRHS, N)))
    p = lambda t: t.data_ptr()                                                            # noqa: E731
    f64 = lambda *shape: torch.full(shape, 7.0, dtype=torch.float64, device=ctx.device)   # noqa: E731
    i32 = lambda *shape: torch.full(shape, 7, dtype=torch.int32, device=ctx.device)       # noqa: E731
    LU, ipiv, info = A.clone(), i32(BATCH, N), i32(BATCH)
    call = lambda op, *args: getattr(L, "mpf_" + op + suffix)(h, *args)                     # noqa: E731
    ok = lambda rc: rc == 0 or pytest.fail(L.mpf_last_error(h).decode())                   # noqa: E731
    ok(call("getrf", p(LU), N, N * N, N, BATCH, p(ipiv), N, p(info), 0))
    X = B.clone()
    ok(call("getrs", 0, p(LU), N, N * N, N, BATCH, p(ipiv), N, NRHS, p(X), N, N * NRHS))
    inv, info2 = f64(BATCH, N, N), i32(BATCH)
    ok(call("getri", p(LU), N, N * N, N, BATCH, p(ipiv), N, p(inv), N, N * N, p(info2)))
    mant, expo = f64(BATCH), i32(BATCH)
    ok(call("getdet", p(LU), N, N * N, N, BATCH, p(ipiv), N, p(mant), p(expo)))
    anorm, rcond, ainvnm = f64(BATCH), f64(BATCH), f64(BATCH)
    ok(call("lange", b"I", p(A), N, N * N, N, BATCH, p(anorm)))
    ok(call("gecon", b"I", p(LU), N, N * N, N, BATCH, p(anorm), p(rcond), p(ainvnm)))
    R, W = f64(BATCH, NRHS, N), f64(BATCH, NRHS, N)
    ok(call("residual", 1, p(A), N, N * N, N, BATCH, NRHS, p(X), N, N * NRHS, p(B), N, N * NRHS, p(R), N, N * NRHS, p(W)))
    Xr = (X + 1e-9).contiguous()                                                          # something to refine
    ferr, berr, iters = f64(BATCH, NRHS), f64(BATCH, NRHS), i32(BATCH, NRHS)
    ok(call("gerfs", 0, p(A), N, N * N, p(LU), N, N * N, N, BATCH, p(ipiv), N, NRHS, p(B), N, N * NRHS, p(Xr), N, N * NRHS, 0, p(ferr), p(berr),
            p(iters)))
    ctx.synchronize()
    return dict(A=A, B=B, LU=LU, ipiv=ipiv, info=info, X=X, inv=inv, info2=info2, mant=mant, expo=expo, anorm=anorm, rcond=rcond, ainvnm=ainvnm,
                R=R, W=W, Xr=Xr, ferr=ferr, berr=berr, iters=iters)


@pytest.mark.gpu
def test_accepted_calls_give_the_same_bits_through_both_entries(ctx):
    assert ctx.get_option("batched_blocked_min_n") > N                  # the blocked entries take the small kernels at this order
    small, blocked = _accepted(ctx, "_batched"), _accepted(ctx, "_batched_blocked")
    for name in small:
        assert np.array_equal(_bits(small[name]), _bits(blocked[name])), name
    # ... and they are results: nothing is the fill, and the factors solve, invert and refine.  The bounds: a solve with partial
    # pivoting at n = 3 leaves a residual of a few n eps |A| |x| (64 eps allows for pivot growth up to 4); the determinant is that of
    # a matrix this close to A, so off by that times the condition number; the norms are sums of three terms
    s = {name: t.cpu().numpy() for name, t in small.items()}
    assert not any((v == 7).any() for name, v in s.items() if name not in ("A", "B"))
    eps = 2.0 ** -53
    ninf = lambda M: np.abs(M).sum(axis=2).max(axis=1)                                      # noqa: E731
    At, Bt, Xt, It, Xrt = (s[name].transpose(0, 2, 1) for name in ("A", "B", "X", "inv", "Xr"))   # (batch, rows, cols)
    assert not s["info"].any() and not s["info2"].any()
    assert (np.abs(At @ Xt - Bt).max(axis=(1, 2)) <= 64 * eps * ninf(At) * ninf(Xt)).all()
    assert (np.abs(At @ It - np.eye(N)).max(axis=(1, 2)) <= 64 * eps * ninf(At) * ninf(It)).all()
    assert (np.abs(s["mant"] * 2.0 ** s["expo"] / np.linalg.det(At) - 1) <= 64 * eps * ninf(At) * ninf(It)).all()
    assert np.allclose(s["anorm"], ninf(At), rtol=4 * eps, atol=0) and np.allclose(s["ainvnm"], ninf(It), rtol=64 * eps * ninf(At) * ninf(It), atol=0)
    assert np.allclose(s["rcond"] * s["anorm"] * s["ainvnm"], 1.0, rtol=4 * eps, atol=0)
    assert (np.abs(At @ Xrt - Bt).max(axis=(1, 2)) <= 64 * eps * ninf(At) * ninf(Xrt)).all()
    assert (s["berr"] <= 8 * eps).all() and (s["iters"] >= 1).all()         # (dgerfs stops at berr <= eps or when it no longer halves)
