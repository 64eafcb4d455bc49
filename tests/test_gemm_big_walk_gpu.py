"""The persistent big-tile kernel (csrc/gemm_big.hip) where a workgroup runs MORE than one work item, on a real MI355X, in bf16 and fp16,
for each instantiation idf_launch_big / idf_launch_big_fold can choose: 320-, 256- and 128-wide tiles, dense and conv, the in-loop
LayerNorm statistics (LNS), out_stats (STATS), the fused q | k | V^T projection (VT), both GEGLU packings (GLU), GroupNorm partials
from the epilogue (GST), the folded upsample (FOLD), the chunked walk and the hybrid whole-tile-then-K-slice launch.  Every case has
NUM_CU + 2 or a few more work items and a ragged last m-tile, so some workgroups set up the next tile's loader under the draining
epilogue, enter the LDS ring on another stage and reuse their per-wave LDS slot (tests/gemm_conv_cases.py, WALK_*).

The judgement is that of tests/test_gemm_conv_edges_gpu.py: the fp64 reference on the same 16-bit-rounded inputs, all outputs finite, NO
element outside ``U |want| + slack``, rel-rms below the bar, NaN guards around every output intact (a skipped tile leaves NaN inside the
view and fails the bound), exactly one persistent-kernel launch and none of the latency or row-resident kernels.  Integer operands must
give torch's product rounded once, bit for bit, and the small-tile family's bits; identical rows must give identical bits.

The GPU cannot show which walk ran, which workgroup ran which item or how a hybrid launch was cut: that these shapes reach two items
per workgroup, the chunked walk and the slice plans named in the [parity] lines comes from the Python mirror of the kernel's index
arithmetic (``big_walk``, ``hybrid_plan``), proved on the CPU by tests/test_gemm_conv_refs.py -- which also shows that the checks here
reject a stale ring stage, a misplaced block and a skipped wave.  Only GST has a counter of its own; that an out_stats or a
self-normalising launch runs the STATS or LNS instantiation is read from idf_launch_big, whose conditions these cases meet.
"""
import contextlib

import pytest
import torch

from tests import gemm_conv_cases as K
from tests import gemm_conv_run as R
from tests.gemm_conv_run import DTS, check, exact, ops_for, run_conv, run_gemm
from tests.test_conv_up_fold_gpu import TOL_MAX as FOLD_TOL_MAX, TOL_RMS as FOLD_TOL_RMS, rel_rms as fold_rel_rms, relmax as fold_relmax

pytestmark = pytest.mark.gpu

HYBRID = dict(big_mode=3, min_eff=80)                        # IDF_TUNE_GEMM_BIG = 3, IDF_TUNE_BIG_MIN_EFF = 80; restored by R.forced
LN_STATS_TOL = 1e-4                                          # mean (absolute) and rstd (relative), as test_gemm_layernorm_self_stats
GN_PARTIAL_TOL = (2e-5, 2e-4)                                # as test_conv3x3_gn_partial (a)
_LATEST = {}
ids = lambda v: str(v).replace(" ", "")


def latest(key, build):
    """A case and its fp64 reference, built once and shared by the checks that use it; only the latest is kept (a reference of these
    shapes is 2 x 170 MB)."""
    if key not in _LATEST:
        _LATEST.clear()
        _LATEST[key] = build()
    return _LATEST[key]


@contextlib.contextmanager
def no_row_kernel(lib):
    """idf_gemm counts the row-resident and streaming kernels as persistent-kernel launches too: none of them may take a case."""
    before = R.row_kernel_launches(lib)
    yield
    assert R.row_kernel_launches(lib) == before, f"(QKV_ROW, GEGLU_ROW, PROJ_ROW) launches moved: {before} -> {R.row_kernel_launches(lib)}"


def ln_stats_check(what, stats, guard, a):
    assert guard() == "", "ln_stats_out stored outside its [M, 2]"
    st, ref = stats.cpu().double(), K.row_stats32(a).double()
    mu_err, rs_rel = float((st[:, 0] - ref[:, 0]).abs().max()), float((st[:, 1] / ref[:, 1] - 1).abs().max())
    print(f"[parity] {what} ln_stats_out: mu abs err {mu_err:.2e}, rstd rel err {rs_rel:.2e}")
    assert bool(torch.isfinite(st).all()) and mu_err < LN_STATS_TOL and rs_rel < LN_STATS_TOL


# ---- idf_gemm ------------------------------------------------------------------------------------------------------------------
def dense_build(shape, epi, dt):
    def build():
        case = K.walk_dense_case(shape, epi, dt)
        return (case,) + tuple(K.walk_want(case))
    return build


def dense_walk_test(shape, epi, dt, label, **force):
    ops = ops_for(dt)
    case, want, slack = latest(("dense", shape, epi, dt), dense_build(shape, epi, dt))
    w_key = "wp" if "wp" in case else "w"
    assert R.gemm_takes("big", case, w_key), "the dispatch rules say the persistent kernel declines this case"
    extra = {}
    with no_row_kernel(ops.lib):
        out, guard, stats = run_gemm(ops, case, "big", label, True, w_key, extra=extra, **force)
    col0 = case.get("vt_col0")
    if col0:                                                 # q | k row-major, V transposed
        vt, vguard = extra["vt"]
        check("idf_gemm", dt, "big", label + " q|k", out, want[:, :col0], slack[:, :col0], guard)
        check("idf_gemm", dt, "big", label + " V^T", vt.t(), want[:, col0:], slack[:, col0:], vguard)
    else:
        check("idf_gemm", dt, "big", label, out, want, slack, guard, case.get("f32out", False))
    if stats is not None:
        e_mu, e_rs = K.out_stats_excess(stats, want, slack, dt)
        print(f"[parity] idf_gemm out_stats {dt} big {label}: mean err/bound {e_mu:.3f} rstd err/bound {e_rs:.3f}")
        assert bool(torch.isfinite(stats).all()) and e_mu <= 1.0 and e_rs <= 1.0
    if case.get("ln_stats_out"):
        ln_stats_check(f"idf_gemm {dt} big {label}", *extra["ln_stats_out"], case["a"])


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape,epi,items", K.WALK_DENSE, ids=ids)
def test_dense_walk(shape, epi, items, dt):
    width = K.walk_dense_width(shape, epi)
    walk = "chunked" if K.big_walk_chunked(shape[0], shape[1], width) else "strided"
    dense_walk_test(shape, epi, dt, f"{epi} {shape}: {items} tiles of 256 x {width}, {shape[2] // 64} K-tiles, {walk} walk")


@pytest.mark.parametrize("dt", DTS)
def test_dense_hybrid(dt):
    """A whole tile and then a K-slice on one workgroup: 256 whole tiles, the four tiles of the rows from 32768 in two slices of four
    K-tiles each (the mirror's plan), bias and an in-place residual through the reducer."""
    shape, epi = K.WALK_HYBRID_DENSE
    plan = K.hybrid_plan(*shape)
    dense_walk_test(shape, epi, dt, f"hybrid {epi} {shape}: {plan}", **HYBRID)


def ints_gemm(shape, dt):
    a, w = K.gemm_operands(*shape, dt, kind="ints")
    return dict(a=a, w=w, kw={}), (a.double() @ w.double().t()).to(K.DTYPES[dt])


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("hybrid", [False, True], ids=["320-wide", "hybrid"])
def test_dense_exact_integers(hybrid, dt):
    """Integer operands, every fp32 partial sum exact: torch's product rounded once, bit for bit, and the small-tile family's bits."""
    ops = ops_for(dt)
    shape = K.WALK_HYBRID_DENSE[0] if hybrid else K.WALK_EXACT_DENSE
    case, want = ints_gemm(shape, dt)
    assert float((case["a"].double().abs() @ case["w"].double().abs().t()).max()) < 2 ** 24
    what = f"idf_gemm {dt} ints {shape}" + (f" hybrid {K.hybrid_plan(*shape)}" if hybrid else "")
    with no_row_kernel(ops.lib):
        big, guard, _ = run_gemm(ops, case, "big", what, True, **(HYBRID if hybrid else {}))
        exact(what + " big", big, want, guard)
        small, guard, _ = run_gemm(ops, case, "small", what, True)
        exact(what + " small", small, want, guard)
    assert torch.equal(big, small)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", K.WALK_SAME_ROWS, ids=ids)
def test_identical_rows_give_identical_bits(shape, dt):
    """A[m] = A[m % 256]: every m-tile sees the same operand tile, so every 256-row block of the output equals the first bit for bit
    (include/idf.h: identical rows of one launch are bitwise equal under mode 2) -- whatever a tile inherits from the one its
    workgroup ran before shows without a reference.  The ragged last block is compared with the head of the first.  (At two n-tiles
    and 256 workgroups a second-round tile follows a tile of its OWN n-tile, whose operands are the same ones; the 128-wide case's
    tile 256 follows a tile of another n-tile, and that is the case tests/test_gemm_conv_refs.py proves the check on.)"""
    ops = ops_for(dt)
    case = K.same_rows_case(shape, dt)
    what = f"idf_gemm {dt} big identical rows {shape}"
    with no_row_kernel(ops.lib):
        out, guard, _ = run_gemm(ops, case, "big", what, True)
    bad = K.same_rows_mismatch(out)
    print(f"[parity] {what}: {bad} of {out.numel()} elements differ from row m % 256's")
    assert guard() == "" and bool(torch.isfinite(out).all()) and bad == 0


# ---- idf_conv3x3, idf_conv3x3_down, idf_conv_up2x_folded -------------------------------------------------------------------------
def conv_build(shape, opts, pad_lo, dt):
    def build():
        case = K.conv_case(shape, opts, dt, pad_lo=pad_lo)
        return (case,) + tuple(K.conv_want(case))
    return build


def conv_walk_test(shape, opts, pad_lo, dt, label, gn_partial=None, **force):
    ops = ops_for(dt)
    case, want, slack = latest(("conv", shape, str(opts), pad_lo, dt), conv_build(shape, opts, pad_lo, dt))
    M, N, Kk, dkw = K.conv_dispatch_args(shape, opts, pad_lo)
    assert K.family_takes("big", M, N, Kk, **dkw)
    with no_row_kernel(ops.lib):
        out, guard = run_conv(ops, case, "big", label, True, gn_partial=gn_partial, **force)
    check("idf_conv3x3" if pad_lo else "idf_conv3x3_down", dt, "big", label, out, want, slack, guard)
    return out


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape,opts,pad_lo,items", K.WALK_CONV, ids=ids)
def test_conv_walk(shape, opts, pad_lo, items, dt):
    M, N, Kk, _ = K.conv_dispatch_args(shape, opts, pad_lo)
    conv_walk_test(shape, opts, pad_lo, dt, f"{shape} {sorted(opts)}: {M} rows, {items} tiles of 256 x {K.big_tile_width(N)}, {Kk // 64} K-tiles")


@pytest.mark.parametrize("dt", DTS)
def test_conv_walk_gn_partial(dt):
    """GST: the per-wave LDS slot of the statistics epilogue reused by the workgroup's next tile, chunks of two samples in one tile.
    The epilogue must leave the partials (counter), they are the fp64 statistics of the stored output chunk by chunk, and asking for
    them does not change a bit of the output."""
    from instancediffusion_amd import _lib
    ops = ops_for(dt)
    shape, opts, pad_lo, items = K.WALK_GST
    B, H, W_, _, Cout = shape[:5]
    part, pguard = K.guarded(ops.gn_partial_shape(B, H * W_, Cout), torch.float32, "cuda")
    c0 = ops.lib.idf_get_stat(_lib.IDF_STAT_GN_EPI_LAUNCHES)
    label = f"{shape} {sorted(opts)}: {items} tiles of 256 x 320"
    out = conv_walk_test(shape, opts, pad_lo, dt, label + " gn_partial", gn_partial=part)
    assert ops.lib.idf_get_stat(_lib.IDF_STAT_GN_EPI_LAUNCHES) - c0 == 1, "the partials must come out of the conv's epilogue"
    assert pguard() == "", "gn_partial stored outside its buffer"
    mean_err, m2_err = K.gn_partial_errors(part, out)
    print(f"[parity] idf_conv3x3 {dt} big {label} gn_partial: mean err {mean_err:.2e} std, M2 rel err {m2_err:.2e}")
    assert bool(torch.isfinite(part).all()) and mean_err < GN_PARTIAL_TOL[0] and m2_err < GN_PARTIAL_TOL[1]
    plain = conv_walk_test(shape, opts, pad_lo, dt, label)
    assert ops.lib.idf_get_stat(_lib.IDF_STAT_GN_EPI_LAUNCHES) - c0 == 1
    assert torch.equal(out, plain), "asking for the statistics must not change the conv output"


@pytest.mark.parametrize("dt", DTS)
def test_conv_hybrid(dt):
    """18 K-tiles: 256 whole tiles, then the four tail tiles in three slices of six K-tiles (the mirror's plan)."""
    shape, opts = K.WALK_HYBRID_CONV
    M, N, Kk, _ = K.conv_dispatch_args(shape, opts)
    conv_walk_test(shape, opts, 1, dt, f"hybrid {shape} {sorted(opts)}: {K.hybrid_plan(M, N, Kk)}", **HYBRID)


@pytest.mark.parametrize("dt", DTS)
def test_conv_exact_integers(dt):
    ops = ops_for(dt)
    shape = K.WALK_EXACT_CONV
    case = K.conv_case(shape, {}, dt, kind="ints")
    want, slack = K.conv_want(case)
    assert torch.equal(want, want.round()) and float(slack.max()) / (9 * shape[3] * K.EPS32) < 2 ** 24
    want = want.to(K.DTYPES[dt])
    what = f"idf_conv3x3 {dt} ints {shape}"
    with no_row_kernel(ops.lib):
        big, guard = run_conv(ops, case, "big", what, True)
        exact(what + " big", big, want, guard)
        small, guard = run_conv(ops, case, "small", what, True)
        exact(what + " small", small, want, guard)
    assert torch.equal(big, small)


@pytest.mark.parametrize("dt", DTS)
def test_folded_upsample_walk(dt):
    """FOLD: 66 m-tiles x 4 parity phases = 264 items, so eight workgroups run a tile of phase 0 and then one of phase 3, with another
    weight image and window origin.  The weights are folded from the fp32 3x3 image and rounded once; the reference is the 3x3 conv of
    the upsampled image with the 16-bit-rounded UNFOLDED weights, at the bars tests/test_conv_up_fold_gpu.py holds the op to."""
    ops = ops_for(dt)
    shape, items = K.WALK_FOLD
    B, H, W_, Cin, Cout = shape

    def build():
        case = K.fold_case(shape, dt)
        return case, K.conv3x3_ref(case["x"], case["w"], bias=case["bias"], up=1)[0]
    case, want = latest(("fold", shape, dt), build)
    out, guard = K.guarded((B, 2 * H, 2 * W_, Cout), ops.dtype, "cuda")
    what = f"idf_conv_up2x_folded {dt} big {shape}: {items} items of 256 x 320, {4 * Cin // 64} K-tiles"
    with no_row_kernel(ops.lib), R.forced(ops.lib, "big") as launches:
        took = ops.conv_up2x(case["x"].cuda(), case["wf"].cuda(), out, bias=case["bias"].cuda())
        torch.cuda.synchronize()
        assert took is True and launches() == (1, 0), (took, launches())
    emax, erms = fold_relmax(out, want), fold_rel_rms(out, want)
    print(f"[parity] {what}: max {emax:.3e} (bar {FOLD_TOL_MAX:.3e}) rel-rms {erms:.3e} (bar {FOLD_TOL_RMS:.1e})")
    assert guard() == "", f"stored outside the output view: {guard()}"
    assert bool(torch.isfinite(out).all()) and emax < FOLD_TOL_MAX and erms < FOLD_TOL_RMS
