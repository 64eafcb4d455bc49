"""The matrix-core GEMM and 3x3-conv kernels on a real MI355X, in bf16 AND fp16, family by family -- the small-tile kernels with their
split-K reducer, the latency ("ring") kernel, the persistent big-tile kernel -- at the smallest shapes that reach each branch of
csrc/gemm_core.h, csrc/gemm_conv.hip and the shape gate of csrc/gemm_big.hip.

Every result is compared with an fp64 reference of the same operation on the same 16-bit-rounded inputs (tests/gemm_conv_cases.py,
proved on the CPU by tests/test_gemm_conv_refs.py): all outputs finite, NO element outside the per-element bound
``U |want| + K 2^-24 (|A| |W|^T) s + act_abs`` (so a wrong SMALL element shows, which relmax hides), rel-rms below the project's bar where
there are enough elements.  Every output lives in a NaN-filled buffer with guard rows in front and behind and guard columns up to the
leading dimension, all of which must still be NaN afterwards.  Each family is forced with idf_set_tuning and the launch counters
must show that it took the launch -- or, where the code says it declines the shape, that it did not.  The K-slices named in the
[parity] lines come from the Python mirror of the dispatch code (checked on the CPU); the counters cannot show them.
"""
import pytest
import torch

from tests import gemm_conv_cases as K
from tests.gemm_conv_run import DTS, cached, check, exact, gemm_takes, ops_for, run_conv, run_gemm

pytestmark = pytest.mark.gpu

FAMS = list(K.FAMILIES)


# ---- idf_gemm ------------------------------------------------------------------------------------------------------------------
def gemm_test(dt, family, label, build, require_takes=True):
    ops = ops_for(dt)
    case, want, slack = cached((label, dt), build)
    w_key = "wp" if "wp" in case else "w"
    takes = gemm_takes(family, case, w_key)
    if require_takes:
        assert takes, "the case list pairs this shape with a family that the dispatch rules say declines it"
    out, guard, stats = run_gemm(ops, case, family, label, takes, w_key)
    check("idf_gemm", dt, family, label, out, want, slack, guard, case.get("f32out", False))
    return case, out, want, slack, stats


def plain(shape, dt, epi="bias", kind="normal", **kw):
    def build():
        case = K.gemm_case(*shape, dt, epi, kind, **kw)
        return (case,) + tuple(K.gemm_want(case))
    return build


def families_of(shape, **kw):
    return [f for f in FAMS if K.family_takes(f, *shape, **kw)]


DENSE_PARAMS = [(s, f) for s in K.DENSE_SHAPES for f in families_of(s)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape,family", DENSE_PARAMS, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_gemm_dense_shapes(shape, family, dt):
    gemm_test(dt, family, f"bias {shape} slices {K.split_plan(family, *shape)}", plain(shape, dt))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("family", FAMS)
def test_gemm_structured_operands(family, dt):
    """A identity-like, W a ramp: out[m, n] = W[n, m % K] + bias[n], so a swapped row, column or K index cannot pass; exact but for
    the bias add."""
    shape = K.EPI_SHAPE_BIG if family == "big" else K.EPI_SHAPES[0]
    gemm_test(dt, family, f"struct {shape}", plain(shape, dt, kind="struct"))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("family", FAMS)
def test_gemm_exact_integers_through_split_k(family, dt):
    """Integer operands, every partial sum exact in fp32: the split-K result is ``want.to(dtype)`` bit for bit in every family."""
    ops, shape = ops_for(dt), K.DENSE_INT_CASES[family]
    a, w = K.gemm_operands(*shape, dt, kind="ints")
    want = (a.double() @ w.double().t()).to(K.DTYPES[dt])
    assert len(K.split_plan(family, *shape)) > 1
    out, guard, _ = run_gemm(ops, dict(a=a, w=w, kw={}), family, f"ints {shape}", True)
    exact(f"idf_gemm {dt} {family} ints {shape} slices {K.split_plan(family, *shape)}", out, want, guard)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("family", ["small", "ring"])
@pytest.mark.parametrize("Bt,M,N,Kk,shared", K.BATCHED, ids=lambda v: str(v))
def test_gemm_batched(Bt, M, N, Kk, shared, family, dt):
    label = f"batched {(Bt, M, N, Kk)} shared {shared}"
    gemm_test(dt, family, label, plain((M, N, Kk), dt, batch=Bt, shared=shared))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("family", ["small", "ring"])
@pytest.mark.parametrize("Kk", K.ODD_LD_K)
@pytest.mark.parametrize("N,what,pad", K.ODD_LD, ids=lambda v: str(v))
def test_gemm_odd_leading_dimensions(N, what, pad, Kk, family, dt):
    """The scalar fallbacks of epilogue8 (and, at K = 576 in the small family, of the split-K reducer): output, residual, row bias and
    fp32 output in rows whose length is no multiple of the vector width, or ragged inside rows that are."""
    pads = {"ldo": dict(ldo_pad=pad), "ldr": dict(ldr_pad=pad), "ld_rowbias": dict(ldrb_pad=pad), "ldo_f32": dict(ldo_pad=pad)}[what]
    gemm_test(dt, family, f"{what} = N + {pad} {(70, N, Kk)}", plain((70, N, Kk), dt, K.ODD_LD_EPI[what], **pads))


EPI_PARAMS = [(s, f) for s in K.EPI_SHAPES for f in ("small", "ring")] + [(K.EPI_SHAPE_BIG, "big")]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("epi", K.EPILOGUES)
@pytest.mark.parametrize("shape,family", EPI_PARAMS, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_gemm_epilogues(shape, family, epi, dt):
    case, out, want, slack, stats = gemm_test(dt, family, f"{epi} {shape}", plain(shape, dt, epi))
    if stats is not None:                                    # (mu, rstd) of the output rows: the tolerance is K.out_stats_excess's
        e_mu, e_rs = K.out_stats_excess(stats, want, slack, dt)
        print(f"[parity] idf_gemm out_stats {dt} {family} {shape}: mean err/bound {e_mu:.3f} rstd err/bound {e_rs:.3f}")
        assert bool(torch.isfinite(stats).all()) and e_mu <= 1.0 and e_rs <= 1.0


def geglu_build(M, N, Kk, P, dt):
    def build():
        case = K.geglu_case(M, N, Kk, P, dt)
        return (case,) + tuple(K.gemm_ref(case["a"], case["w"], **case["ref_kw"]))
    return build


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("family", FAMS)
@pytest.mark.parametrize("M,N,Kk,P", K.GEGLU_CASES, ids=lambda v: str(v))
def test_gemm_geglu(M, N, Kk, P, family, dt):
    """Both packing periods with a folded LayerNorm.  The persistent kernel takes only (200, 640, 320) at period 32 (whole 320-wide
    tiles; 640 is no multiple of 256, K = 64 is one K-tile): where it declines, the assertion is that it did."""
    gemm_test(dt, family, f"geglu P={P} {(M, N, Kk)}", geglu_build(M, N, Kk, P, dt), require_takes=False)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("family", FAMS)
@pytest.mark.parametrize("act", K.SWEEP_ACTS)
def test_activation_sweep(act, family, dt):
    """Chosen accumulator values through silu_f, gelu_erf_f (a fit that clamps at +-8), quick_gelu_f and the GEGLU gate: from 0 and
    2^-14 to +-1000, where exp overflows the intermediate.  Finite everywhere (check) and inside the bound."""
    Kk = 128 if family == "big" else 64                      # the persistent kernel needs two K-tiles: the second one is zero

    def build():
        case = K.sweep_case(act, dt, Kk)
        return (case,) + tuple(K.gemm_ref(case["a"], case["w"], **case["ref_kw"]))
    gemm_test(dt, family, f"sweep {act} K={Kk}", build)


@pytest.mark.parametrize("f32out", [False, True])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("family", FAMS)
def test_overflow_is_torch_to(family, dt, f32out):
    """Accumulators beyond the fp16 range: the stored value is ``x.to(dtype)`` bit for bit (+-inf, 65504 kept, 65519 -> 65504 by RNE); with
    the fp32 output flag it is the exact value."""
    ops = ops_for(dt)
    c = K.overflow_case(dt, 128 if family == "big" else 64)
    acc = c["a32"].double() @ c["w32"].double().t()
    out, guard, _ = run_gemm(ops, dict(a=c["a"], w=c["w"], kw={}, f32out=f32out), family, "overflow", True)
    torch.cuda.synchronize()
    if dt == "fp16":
        for value, (i, j) in K.OVERFLOW_AT.items():          # the accumulators the case exists for, 65504 itself among them
            assert acc[i, j] == value
    if f32out:
        err = float((out.cpu().double() - acc).abs().max())
        print(f"[parity] idf_gemm {dt} {family} overflow fp32 out: largest difference from the exact accumulator {err:.3g}")
        assert guard() == "" and err == 0.0
        return
    want = acc.to(K.DTYPES[dt])
    if dt == "fp16":
        assert want[0, 0] == float("inf") and want[0, 1] == float("-inf") and want[1, 2] == 65504 and want[1, 5] == 65504
        assert want[2, 3] == float("inf")
    exact(f"idf_gemm {dt} {family} overflow", out, want, guard)


DECLINES = [                                                 # (family, shape, case options): what the code says the family leaves alone
    ("big", (256, 128, 64), {}),                             # one K-tile
    ("big", (130, 136, 128), {}),                            # N no multiple of 128
    ("big", (130, 256, 128), dict(ldo_pad=4)),               # output rows not 16-byte aligned
    ("big", (130, 128, 128), dict(epi="ln_row_self")),       # self-computed LayerNorm statistics on 128-wide tiles
    ("big", (77, 320, 64), dict(batch=3, shared="w")),       # batched
    ("ring", (16640, 64, 512), {}),                          # 130 tiles, 8 K-tiles: left to the small family's split-K
]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("family,shape,opts", DECLINES, ids=lambda v: str(v))
def test_families_decline_what_the_code_says(family, shape, opts, dt):
    opts = dict(opts)
    epi = opts.pop("epi", "bias")
    case = gemm_test(dt, family, f"declined {epi} {shape} {opts}", plain(shape, dt, epi, **opts), require_takes=False)[0]
    assert not gemm_takes(family, case)


# ---- idf_conv3x3, idf_conv3x3_down -----------------------------------------------------------------------------------------------
def conv_test(dt, family, shape, opts, kind="normal", pad_lo=1):
    ops = ops_for(dt)
    label = f"{shape} {opts} {kind}"

    def build():
        case = K.conv_case(shape, opts, dt, kind, pad_lo)
        return (case,) + tuple(K.conv_want(case))
    case, want, slack = cached(("conv", label, pad_lo, dt), build)
    M, N, Kk, dkw = K.conv_dispatch_args(shape, opts, pad_lo)
    assert K.family_takes(family, M, N, Kk, **dkw)
    out, guard = run_conv(ops, case, family, label, True)
    check("idf_conv3x3" if pad_lo else "idf_conv3x3_down", dt, family, f"{label} slices {K.split_plan(family, M, N, Kk, conv=True)}",
          out, want, slack, guard, bool(opts.get("n_valid")))


def conv_families(shape, opts, pad_lo=1):
    M, N, Kk, dkw = K.conv_dispatch_args(shape, opts, pad_lo)
    return [f for f in FAMS if K.family_takes(f, M, N, Kk, **dkw)]


CONV_PARAMS = [(s, o, f) for s, o in K.CONV_CASES for f in conv_families(s, o)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape,opts,family", CONV_PARAMS, ids=lambda v: str(v).replace(" ", ""))
def test_conv3x3(shape, opts, family, dt):
    conv_test(dt, family, shape, opts)


@pytest.mark.parametrize("dt", DTS)
def test_conv3x3_small_family_without_split_k(dt):
    """192 tiles: the one conv of the suite that the small-tile family runs through its own epilogue, not the reducer's."""
    shape, opts = K.CONV_NO_SPLIT
    M, N, Kk, _ = K.conv_dispatch_args(shape, opts)
    assert K.split_plan("small", M, N, Kk, conv=True) == [9]
    conv_test(dt, "small", shape, opts)


STRUCT_PARAMS = [(s, 1, f) for s in K.CONV_STRUCT for f in conv_families(s, {})] + \
                [(K.DOWN_STRUCT + (2, 0), 0, f) for f in conv_families(K.DOWN_STRUCT + (2, 0), {}, 0)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape,pad_lo,family", STRUCT_PARAMS, ids=lambda v: str(v).replace(" ", ""))
def test_conv_structured_operands(shape, pad_lo, family, dt):
    """Pixel p lights channel p % Cin and the weight is a ramp over (Cout, tap, channel): a swapped tap, pixel or channel cannot pass.
    idf_conv3x3 in all three families (the 320-wide shape is the persistent kernel's) and idf_conv3x3_down (pad_lo = 0)."""
    conv_test(dt, family, shape, {}, kind="struct", pad_lo=pad_lo)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("family", FAMS)
def test_conv3x3_exact_integers_through_split_k(family, dt):
    ops, shape = ops_for(dt), K.CONV_INT_CASES[family]
    M, N, Kk, dkw = K.conv_dispatch_args(shape, {})
    assert K.split_plan(family, M, N, Kk, conv=True) == K.CONV_SPLIT_EXPECTED[family] and K.family_takes(family, M, N, Kk, **dkw)
    case = K.conv_case(shape, {}, dt, kind="ints")
    want, _ = K.conv_want(case)
    out, guard = run_conv(ops, case, family, f"ints {shape}", True)
    exact(f"idf_conv3x3 {dt} {family} ints {shape} slices {K.CONV_SPLIT_EXPECTED[family]}", out, want.to(K.DTYPES[dt]), guard)


DOWN_PARAMS = [(s, f) for s in K.DOWN_CASES for f in conv_families(s + (2, 0), {}, 0)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("shape,family", DOWN_PARAMS, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_conv3x3_down(shape, family, res, dt):
    conv_test(dt, family, shape + (2, 0), dict(res=res), pad_lo=0)
