"""idf_conv3x3_skip on a real MI355X: a ResBlock's tail -- conv2(g2) + Wskip . x + both biases -- as ONE contraction over
K = 9 C2 + Cx on the persistent kernel (csrc/gemm_big.hip, SKIPK: the shortcut as K-tiles behind the nine taps), in bf16 and fp16.

Reference: the fp64 3x3 conv + 1x1 on the same 16-bit operands.  Bars: the per-kernel ones of DESIGN §2 (max error <= 2^-7 of the output
max, rel-RMS <= 3e-3), and the rel-RMS may not exceed that of the two launches it replaces (idf_gemm, then idf_conv3x3 with the residual)
on the same inputs times 1.05 -- the new path drops the 16-bit rounding of the shortcut, the 5 % covers the other fp32 summation order.
g2 and x live inside larger NaN-filled allocations with NaN-padded rows, so a read outside either tensor shows in the output; the output
and the GroupNorm partials sit in NaN guards of their own.  The persistent kernel is forced as in tests/test_gemm_big_walk_gpu.py.

Then the engine on the reduced-width mid_box golden: knob on and knob off both within the golden's bar, the counter equal to the number
of shortcut ResBlocks with the knob on and unmoved with it off.
"""
import ctypes as C
import dataclasses

import pytest
import torch

from tests import gemm_conv_cases as K
from tests import gemm_conv_run as R

pytestmark = pytest.mark.gpu

TOL_MAX = 2.0 ** -7
TOL_RMS = 3e-3
GN_PARTIAL_TOL = (2e-5, 2e-4)                                # as test_conv3x3_gn_partial (a)
DTS = ["bf16", "fp16"]
# (B, H, W, C2, Cx, Cout): the conv input width C2 is Cout in a ResBlock; the last case keeps it small
CASES = {
    "one-skip-tile": (2, 16, 16, 320, 64, 320),              # M = 512: two m-tiles, ONE shortcut K-tile behind 45
    "ragged-borders": (3, 10, 10, 320, 640, 320),            # M = 300: ragged last tile, every row on or near a border; unsplit
    "two-n-tiles": (1, 32, 32, 640, 960, 640),               # M = 1024: two n-tiles, 15 shortcut K-tiles behind 90
    "split-k": (2, 8, 8, 1280, 2560, 1280),                  # M = 128: 220 K-tiles in 11 slices of 20, the boundary at 200 inside [180, 220)
    # 137 m-tiles x 2 n-tiles = 274 whole-K items on 256 workgroups: 18 of them run two tiles, the second set up under the first's
    # epilogue; ragged last m-tile; unsplit, so the GroupNorm partials come out of the epilogue (the shape of gemm_conv_cases.WALK_GST)
    "two-items": (3, 104, 112, 64, 64, 640),
}
_REF = {}


def rel_rms(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float(((a - b).pow(2).mean() / b.pow(2).mean().clamp_min(1e-30)).sqrt())


def relmax(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max() / b.double().abs().max().clamp_min(1e-20))


def gen(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def skip_ref64(g2, x, wp, bias, C2):
    """fp64 on the GPU: nine shifted [M, C2] x [C2, Cout] products of the zero-padded g2, the 1x1 on x, the bias.  -> [B, H, W, Cout]"""
    B, H, W_, _ = g2.shape
    gp = torch.nn.functional.pad(g2.double(), (0, 0, 1, 1, 1, 1))
    wd = wp.double()
    y = x.double().reshape(-1, x.shape[-1]) @ wd[:, 9 * C2:].t() + bias.double()
    for t in range(9):
        ky, kx = divmod(t, 3)
        y += gp[:, ky:ky + H, kx:kx + W_].reshape(-1, C2) @ wd[:, t * C2:(t + 1) * C2].t()
    return y.reshape(B, H, W_, -1)


def case_for(name, dt):
    """Operands (16-bit, on the GPU), the packed weight and the fp64 reference of a case: built once, shared, never modified."""
    if (name, dt) not in _REF:
        from instancediffusion_amd.engine import pack_conv3x3_skip
        B, H, W_, C2, Cx, Cout = CASES[name]
        T = K.DTYPES[dt]
        g2 = gen((B, H, W_, C2), 810).to(T).cuda()
        x = gen((B, H, W_, Cx), 811).to(T).cuda()
        w2 = gen((Cout, C2, 3, 3), 812, (9 * C2) ** -0.5)
        ws = gen((Cout, Cx), 813, Cx ** -0.5)
        b2, bs = gen((Cout,), 814) * 2.0 + 0.5, gen((Cout,), 815)       # group means well away from 0
        wp, bp = pack_conv3x3_skip(w2, b2, ws, bs)
        wp = wp.to(T).cuda()
        d = dict(g2=g2, x=x, wp=wp, bias=bp.cuda(), w2=wp[:, :9 * C2].contiguous(), ws=wp[:, 9 * C2:].contiguous(), b2=b2.cuda(), bs=bs.cuda())
        d["want"] = skip_ref64(g2, x, wp, d["bias"], C2).cpu()
        _REF.clear()                                         # keep the latest only (the largest reference is 180 MB)
        _REF[(name, dt)] = d
    return _REF[(name, dt)]


def in_nans(t):
    """``t`` [B, H, W, C] as a view of rows 8 elements longer inside a NaN-filled allocation with spare rows in front and behind."""
    view, _ = K.guarded(tuple(t.shape), t.dtype, "cuda", ld=t.shape[-1] + 8)
    view.copy_(t)
    return view


def run_skip(ops, d, shape, gn=False):
    """One forced launch into guarded buffers -> (out, out guard, partials or None, their guard, (skip, persistent, GN-epilogue) launches)."""
    from instancediffusion_amd import _lib
    B, H, W_, C2, Cx, Cout = shape
    out, guard = K.guarded((B, H, W_, Cout), ops.dtype, "cuda")
    part = pguard = None
    if gn:
        part, pguard = K.guarded(ops.gn_partial_shape(B, H * W_, Cout), torch.float32, "cuda")
    stats = lambda: tuple(ops.lib.idf_get_stat(s) for s in (_lib.IDF_STAT_SKIP_FOLD_LAUNCHES, _lib.IDF_STAT_GEMM_BIG_LAUNCHES,
                                                            _lib.IDF_STAT_GN_EPI_LAUNCHES))
    with R.forced(ops.lib, "big"):
        s0 = stats()
        took = ops.conv3x3_skip(in_nans(d["g2"]), d["wp"], in_nans(d["x"]), out, bias=d["bias"], gn_partial=part)
        torch.cuda.synchronize()
        assert took is True
        return out, guard, part, pguard, tuple(a - b for a, b in zip(stats(), s0))


def two_launches(ops, d, shape):
    """What the call replaces, on the same operands: the shortcut GEMM into a 16-bit tensor, then the conv with it as the residual."""
    B, H, W_, C2, Cx, Cout = shape
    with R.forced(ops.lib, "big"):
        xs = ops.gemm(d["x"].view(-1, Cx), d["ws"], ops.empty((B * H * W_, Cout)), bias=d["bs"]).view(B, H, W_, Cout)
        old = ops.conv3x3(d["g2"], d["w2"], ops.empty((B, H, W_, Cout)), bias=d["b2"], res=xs)
        torch.cuda.synchronize()
    return old


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", list(CASES))
def test_skip_fold_against_fp64_and_the_two_launches(name, dt):
    ops = R.ops_for(dt)
    shape = CASES[name]
    B, H, W_, C2, Cx, Cout = shape
    d = case_for(name, dt)
    gn = (H * W_) % 64 == 0
    out, guard, part, pguard, (n_skip, n_big, n_gst) = run_skip(ops, d, shape, gn=gn)
    old = two_launches(ops, d, shape)
    emax, erms, orms = relmax(out, d["want"]), rel_rms(out, d["want"]), rel_rms(old, d["want"])
    print(f"[skip_fold] {name} {dt} {shape}: K-tiles {9 * C2 // 64} + {Cx // 64}: max {emax:.3e} (bar {TOL_MAX:.3e}) rel-rms {erms:.3e} "
          f"(bar {TOL_RMS:.1e}); two launches rel-rms {orms:.3e}, ratio {erms / orms:.3f} (bar 1.05); GroupNorm partials from the "
          f"epilogue: {n_gst}")
    assert guard() == "", f"stored outside the output view: {guard()}"
    assert (n_skip, n_big) == (1, 1), (n_skip, n_big)
    assert bool(torch.isfinite(out).all()), "non-finite output: a read outside g2 or x, or a tile not written"
    assert emax <= TOL_MAX and erms <= TOL_RMS
    assert erms <= 1.05 * orms
    if gn:
        assert pguard() == "", "gn_partial stored outside its buffer"
        mean_err, m2_err = K.gn_partial_errors(part, out)
        print(f"[skip_fold] {name} {dt} gn_partial: mean err {mean_err:.2e} std, M2 rel err {m2_err:.2e}")
        assert bool(torch.isfinite(part).all()) and mean_err < GN_PARTIAL_TOL[0] and m2_err < GN_PARTIAL_TOL[1]
        plain, pg, _, _, _ = run_skip(ops, d, shape, gn=False)
        assert pg() == "" and torch.equal(plain, out), "asking for the statistics must not change the output"
    if name == "two-items":
        assert n_gst == 1, "an unsplit launch must leave the partials from its epilogue"


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", ["ragged-borders", "split-k"])
def test_graph_replay_equals_eager(name, dt):
    from instancediffusion_amd.engine import capture_graph
    ops = R.ops_for(dt)
    shape = CASES[name]
    B, H, W_, C2, Cx, Cout = shape
    d = case_for(name, dt)
    eager, guard, _, _, _ = run_skip(ops, d, shape)          # also the warm-up outside the capture (split-K workspace, LDS opt-in)
    out, oguard = K.guarded((B, H, W_, Cout), ops.dtype, "cuda")
    g2, x = in_nans(d["g2"]), in_nans(d["x"])
    with R.forced(ops.lib, "big"):
        graph = torch.cuda.CUDAGraph()
        with capture_graph(graph):
            took = ops.conv3x3_skip(g2, d["wp"], x, out, bias=d["bias"])
        assert took is True
        graph.replay()
        torch.cuda.synchronize()
        first = out.clone()
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
    assert guard() == "" and oguard() == ""
    assert torch.equal(first, eager) and torch.equal(out, eager)


def test_argument_errors_before_any_launch():
    """Every pointer, alignment and shape error is reported before anything runs: the counters do not move and the output stays NaN;
    a launch the persistent kernel does not take is IDF_E_UNSUPPORTED the same way."""
    from instancediffusion_amd import _lib
    ops = R.ops_for("bf16")
    lib = ops.lib
    B, H, W_, C2, Cx, Cout = 1, 8, 8, 64, 128, 320
    g2, x, w, bias = ops.empty((B, H, W_, C2)), ops.empty((B, H, W_, Cx)), ops.empty((Cout, 9 * C2 + Cx)), ops.empty((Cout,), torch.float32)
    for t in (g2, x, w, bias):
        t.zero_()
    out = ops.empty((B, H, W_, Cout))
    out.fill_(float("nan"))
    part = ops.empty((B, 1, 32, 2), torch.float32)
    base = dict(g=g2.data_ptr(), x=x.data_ptr(), W=w.data_ptr(), out=out.data_ptr(), bias=bias.data_ptr(), B=B, H=H, Wd=W_, C2=C2, Cx=Cx,
                Cout=Cout, ldg=C2, ldx=Cx, ldo=Cout, dtype=ops.dt, ws=None, ws_bytes=0, gn_partial=None)
    stats = lambda: (lib.idf_get_stat(_lib.IDF_STAT_SKIP_FOLD_LAUNCHES), lib.idf_get_stat(_lib.IDF_STAT_GEMM_BIG_LAUNCHES),
                     lib.idf_get_stat(_lib.IDF_STAT_GEMM_RING_LAUNCHES))
    arg, align, unsupported = -1, -2, -3
    bad = [(dict(g=None), arg), (dict(x=None), arg), (dict(W=None), arg), (dict(out=None), arg), (dict(B=0), arg), (dict(H=0), arg),
           (dict(Wd=-1), arg), (dict(Cout=0), arg), (dict(C2=60), arg), (dict(Cx=0), arg), (dict(Cx=100), arg), (dict(ldg=C2 - 8), arg),
           (dict(ldx=Cx - 8), arg), (dict(ldo=Cout - 8), arg), (dict(gn_partial=part.data_ptr(), ldo=Cout + 8), arg),
           (dict(ldg=C2 + 4), align), (dict(ldx=Cx + 4), align), (dict(ldo=Cout + 4), align), (dict(g=g2.data_ptr() + 2), align),
           (dict(x=x.data_ptr() + 8), align), (dict(W=w.data_ptr() + 2), align), (dict(out=out.data_ptr() + 4), align),
           (dict(bias=bias.data_ptr() + 4), align), (dict(gn_partial=part.data_ptr() + 4), align),
           (dict(dtype=7), unsupported), (dict(Cout=256), unsupported)]
    with R.forced(lib, "big"):
        s0 = stats()
        for change, code in bad:
            assert lib.idf_conv3x3_skip(C.byref(_lib.ConvSkipArgs(**dict(base, **change))), None) == code, change
        assert lib.idf_conv3x3_skip(None, None) == arg
    # unforced, a 64-row launch belongs to the latency kernel: not taken, nothing launched, the caller falls back
    assert ops.conv3x3_skip(g2, w, x, out, bias=bias) is False
    with R.forced(lib, "small"):                             # IDF_TUNE_GEMM_BIG = 0: never a persistent kernel
        assert ops.conv3x3_skip(g2, w, x, out, bias=bias) is False
    torch.cuda.synchronize()
    assert stats() == s0 and bool(torch.isnan(out).all())
    with R.forced(lib, "big"):                               # the same call with nothing wrong goes through
        assert ops.conv3x3_skip(g2, w, x, out, bias=bias) is True
    torch.cuda.synchronize()
    assert bool((out == 0).all())


# ---- the engine ------------------------------------------------------------------------------------------------------------------
def test_engine_knob_on_and_off_hold_the_golden_bar_and_the_counter_counts_shortcut_blocks():
    from grounding_input.text_grounding_tokinzer_input import GroundingNetInput
    from instancediffusion_amd import _lib, engine as E
    from instancediffusion_amd.ops import HipOps
    from tests.test_engine_gpu import _build, _case, _check
    gold, meta, cfg, inp = _case("mid_box")
    model = _build(cfg)
    n_short = sum(1 for m in model.modules() if type(m).__name__ == "ResBlock" and not isinstance(m.skip_connection, torch.nn.Identity))
    assert n_short == 8                                      # mid: 320 -> 640, 640 -> 1280 down; the six concat inputs up
    grounding = {k: v.cuda() for k, v in GroundingNetInput().prepare(inp["gb"]).items()}
    lib = _lib.load()
    count = lambda: lib.idf_get_stat(_lib.IDF_STAT_SKIP_FOLD_LAUNCHES)
    base = E.EngineKnobs.from_env()
    eps = {}
    with R.forced(lib, "big"), torch.no_grad():              # the persistent kernel serves every conv of this 2-row forward
        for on in (True, False):
            eng = E.UNetEngine(model, ops=HipOps(torch.bfloat16), use_graphs=False, knobs=dataclasses.replace(base, skip_fold=on))
            tails = [p["tail"] for blk in eng.in_blocks + [eng.mid_block] + eng.out_blocks for p in blk if p["kind"] == "res"]
            assert sum(t is not None for t in tails) == (n_short if on else 0)
            cond = eng.prepare_cond(inp["context"].cuda(), grounding)
            c0 = count()
            eps[on] = eng.forward_cond(inp["x"].cuda(), inp["t"].cuda(), cond)
            torch.cuda.synchronize()
            assert count() - c0 == (n_short if on else 0)
            _check(eps[on], gold["eps_cond"], f"mid_box cond, persistent kernel forced, skip_fold={int(on)}", "mid_box")
    print(f"[skip_fold] mid_box forward: knob on vs knob off rel-rms {rel_rms(eps[True], eps[False]):.3e}")
