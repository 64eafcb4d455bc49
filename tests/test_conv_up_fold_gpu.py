"""idf_conv_up2x_folded on a real MI355X: nearest-x2 upsample + 3x3 conv as four 2x2 phase convs (the upsample folded into the
weights at pack time) against the fp32 PyTorch expression it replaces,

    F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, b, padding=1),

with the fp32 MASTER weights (the folded image is summed in fp32 and rounded to 16 bit once) at the per-kernel bars of DESIGN §2:
max error <= 2^-7 of the output max, rel-RMS <= 3e-3, in bf16 and fp16.  Every case also prints its rel-RMS against today's
conv3x3(upsample=1) on the same inputs.  Then the engine: IDF_UP_FOLD=0 is bit-identical to the path without the op.
"""
import dataclasses

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL_MAX = 2.0 ** -7
TOL_RMS = 3e-3
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
# the three Upsample layers of the SD-1.5 UNet (bench shapes): (H, W, C)
BENCH_SHAPES = [(32, 32, 640), (16, 16, 1280), (8, 8, 1280)]


def gen(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def rel_rms(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float(((a - b).pow(2).mean() / b.pow(2).mean().clamp_min(1e-30)).sqrt())


def relmax(a, b):
    return float((a.float().cpu() - b.float().cpu()).abs().max() / b.float().abs().max().clamp_min(1e-20))


@pytest.fixture
def lib():
    from instancediffusion_amd import _lib
    return _lib.load()


@pytest.fixture
def forced(lib):
    """The persistent kernel takes every shape that qualifies, whatever its occupancy (as tests/test_kernels_gpu.py `big`)."""
    prev = lib.idf_set_tuning(0, 2)
    yield
    lib.idf_set_tuning(0, prev)


def run_case(lib, dtype_name, B, H, W, Cin, Cout, expect_native):
    """-> None.  expect_native: True = the folded launch must take the shape (one persistent-kernel launch), False = it must decline
    before any launch (the engine then runs conv3x3(upsample=1); checked here the same way)."""
    from instancediffusion_amd.engine import pack_conv3x3, pack_conv_up2x
    from instancediffusion_amd.ops import HipOps
    dt = DTYPES[dtype_name]
    ops = HipOps(dt)
    x = gen((B, H, W, Cin), 20).to(dt)
    w4 = gen((Cout, Cin, 3, 3), 21, (9 * Cin) ** -0.5)
    b = gen((Cout,), 22)
    want = F.conv2d(F.interpolate(x.float().permute(0, 3, 1, 2), scale_factor=2, mode="nearest"), w4, b, padding=1).permute(0, 2, 3, 1)
    wf = pack_conv_up2x(w4).to(dt).cuda()
    w3 = pack_conv3x3(w4).to(dt).cuda()
    xd, bd = x.cuda(), b.cuda()
    old = ops.conv3x3(xd, w3, ops.empty((B, 2 * H, 2 * W, Cout)), bias=bd, upsample=1)
    out = ops.empty((B, 2 * H, 2 * W, Cout))
    out.fill_(float("nan"))                                  # a pixel the launch does not write fails the comparison
    big0 = lib.idf_get_stat(0)
    took = ops.conv_up2x(xd, wf, out, bias=bd)
    torch.cuda.synchronize()
    launches = lib.idf_get_stat(0) - big0
    what = f"conv_up2x [{dtype_name}] ({B},{H},{W},{Cin})->{Cout}"
    if not expect_native:
        assert took is False and launches == 0, (took, launches)
        assert torch.isnan(out.float()).all()                # declined BEFORE any launch: the output is untouched
        print(f"[up_fold] {what}: declined (IDF_E_UNSUPPORTED), the caller runs conv3x3(upsample=1): "
              f"max {relmax(old, want):.3e} rel-rms {rel_rms(old, want):.3e}")
        assert relmax(old, want) < TOL_MAX and rel_rms(old, want) < TOL_RMS
        return
    assert took is True and launches == 1, (took, launches)
    emax, erms = relmax(out, want), rel_rms(out, want)
    print(f"[up_fold] {what}: vs fp32 reference max {emax:.3e} (bar {TOL_MAX:.3e}) rel-rms {erms:.3e} (bar {TOL_RMS:.1e}); "
          f"conv3x3(upsample=1) vs reference rel-rms {rel_rms(old, want):.3e}; folded vs conv3x3(upsample=1) rel-rms {rel_rms(out, old):.3e}")
    assert torch.isfinite(out.float()).all()
    assert emax < TOL_MAX
    assert erms < TOL_RMS


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("H,W,C", BENCH_SHAPES)
def test_bench_shapes_small_batch(lib, forced, dtype_name, H, W, C):
    """Batch 2 (the narrowest forward): a partial tile grid, at 8 x 8 a partial m-tile (128 of 256 rows)."""
    run_case(lib, dtype_name, 2, H, W, C, C, expect_native=True)


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("B,H,W,C", [(16, 32, 32, 640), (16, 16, 16, 1280), (64, 8, 8, 1280)])
def test_bench_shapes_persistent_batch(lib, dtype_name, B, H, W, C):
    """Batches whose 4 x tiles fill whole rounds of the 256 workgroup slots: taken by the automatic rule, nothing forced."""
    run_case(lib, dtype_name, B, H, W, C, C, expect_native=True)


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
def test_small_non_square_forced(lib, forced, dtype_name):
    """Non-square, odd sizes, H = 1 and W = 1 edges: every tap of some rows is padding; 105 / 7 / 5 rows of one 256-row tile."""
    run_case(lib, dtype_name, 3, 5, 7, 64, 320, expect_native=True)
    run_case(lib, dtype_name, 1, 1, 7, 128, 320, expect_native=True)
    run_case(lib, dtype_name, 1, 5, 1, 64, 640, expect_native=True)


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
def test_small_non_square_falls_back(lib, dtype_name):
    """Unforced, a grid far below the occupancy bar, and a Cout without 320-wide tiles: declined, the engine's fallback runs."""
    run_case(lib, dtype_name, 3, 5, 7, 64, 320, expect_native=False)
    run_case(lib, dtype_name, 1, 6, 9, 128, 128, expect_native=False)


def test_rejects_what_it_does_not_implement(lib):
    """Residual / row bias / GroupNorm partials are IDF_E_ARG (-1), not silently dropped."""
    import ctypes as C
    from instancediffusion_amd import _lib
    from instancediffusion_amd.ops import HipOps
    ops = HipOps(torch.bfloat16)
    x, wf, out = ops.empty((1, 8, 8, 64)), ops.empty((4, 320, 256)), ops.empty((1, 16, 16, 320))
    base = dict(x=x.data_ptr(), W=wf.data_ptr(), out=out.data_ptr(), bias=None, rowbias=None, res=None, B=1, Hin=8, Win=8, Cin=64,
                Cout=320, stride=1, upsample=1, ldx=64, ldo=320, ldr=0, ld_rowbias=0, n_valid=0, epi=0, dtype=ops.dt, ws=None,
                ws_bytes=0, gn_partial=None)
    for bad in (dict(res=out.data_ptr()), dict(stride=2), dict(upsample=0), dict(epi=1), dict(n_valid=4), dict(Cin=60)):
        args = _lib.ConvArgs(**dict(base, **bad))
        assert lib.idf_conv_up2x_folded(C.byref(args), None) == -1, bad


def _smoke_model():
    from oracle import ref_cpu
    from tests.test_engine_emulated import build_model
    cfg = dict(ref_cpu.DEFAULT_CFG)
    cfg.update(channel_mult=(1, 2, 4), num_res_blocks=1, mid_dim=512)       # Upsample layers at C = 1280 (4x4) and 640 (8x8)
    return cfg, build_model(cfg)


class _WithoutFold:
    """The ops object as an engine without the new op sees it (the `hasattr` gate of UNetEngine._pack_up)."""

    def __init__(self, ops):
        self._ops = ops

    def __getattr__(self, name):
        if name == "conv_up2x":
            raise AttributeError(name)
        return getattr(self._ops, name)


def _up_layers(eng):
    return [p for blk in eng.out_blocks for p in blk if p["kind"] == "up"]


def test_engine_knob_off_is_the_parent_path_bit_for_bit(lib, forced, monkeypatch):
    """IDF_UP_FOLD=0 packs and runs exactly what an engine without the op does: conv3x3(upsample=1) on the 3x3 image, the same
    bits out.  With the knob on (the persistent kernel forced, so the folded launch takes this reduced-width model's 4x4 and 8x8
    levels) the 3x3 image is NOT kept, the forward holds the smoke() bar against the CPU oracle, and its distance from the
    knob-off forward is printed."""
    from grounding_input.text_grounding_tokinzer_input import GroundingNetInput
    from instancediffusion_amd import engine as E, synth
    from instancediffusion_amd.ops import HipOps
    from oracle import ref_cpu
    cfg, model = _smoke_model()
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(3)
    gb = synth.make_grounding_batch(2, synth.random_boxes(3, g), g)
    x = torch.randn(2, 4, 16, 16, generator=g)
    ctx = torch.randn(2, 77, 768, generator=g)
    t = torch.tensor([801, 33])
    grounding = {k: v.cuda() for k, v in GroundingNetInput().prepare(gb).items()}

    def forward(eng):
        calls = []
        real = eng.ops.conv_up2x if hasattr(eng.ops, "conv_up2x") else None
        if real is not None:
            monkeypatch.setattr(eng.ops, "conv_up2x", lambda *a, **k: calls.append(real(*a, **k)) or calls[-1], raising=False)
        cond = eng.prepare_cond(ctx.cuda(), grounding)
        eps = eng.forward_cond(x.cuda(), t.cuda(), cond).float().cpu()
        return eps, calls

    on = dataclasses.replace(E.EngineKnobs.from_env(), up_fold=True)
    eng_off = E.UNetEngine(model, ops=HipOps(torch.bfloat16), use_graphs=False, knobs=dataclasses.replace(on, up_fold=False))
    eng_parent = E.UNetEngine(model, ops=_WithoutFold(HipOps(torch.bfloat16)), use_graphs=False, knobs=on)
    eng_on = E.UNetEngine(model, ops=HipOps(torch.bfloat16), use_graphs=False, knobs=on)
    ups = [m for m in model.modules() if type(m).__name__ == "Upsample"]
    assert len(_up_layers(eng_off)) == len(ups) == 2
    for eng in (eng_off, eng_parent):
        for p, m in zip(_up_layers(eng), ups):
            assert p["fold"] is None
            assert torch.equal(p["conv"].w.cpu(), E.pack_conv3x3(m.conv.weight.detach().float()).to(torch.bfloat16))
    for p in _up_layers(eng_on):
        assert p["conv"] is None and tuple(p["fold"].shape) == (4, p["fold"].shape[1], 4 * p["fold"].shape[1])
    eps_off, calls_off = forward(eng_off)
    eps_parent, _ = forward(eng_parent)
    assert calls_off == []                                   # the knob-off engine never reaches the new entry point
    assert torch.equal(eps_off, eps_parent)
    eps_on, calls_on = forward(eng_on)
    assert calls_on == [True, True]                          # both Upsample layers ran folded
    assert all(p["conv"] is None for p in _up_layers(eng_on))    # ... and nothing packed the 3x3 image behind its back
    with torch.no_grad():
        objs, _ = ref_cpu.unifusion(sd, cfg, ref_cpu.prepare_grounding(gb))
        want = ref_cpu.unet_forward(sd, cfg, x, t, ctx, objs)
    print(f"[up_fold] reduced-width forward vs CPU oracle: knob on rel-rms {rel_rms(eps_on, want):.3e}, knob off "
          f"{rel_rms(eps_off, want):.3e} (bf16 bar 2e-2, SURVEY §8c); knob on vs knob off rel-rms {rel_rms(eps_on, eps_off):.3e}")
    assert rel_rms(eps_on, want) < 2e-2
    assert rel_rms(eps_off, want) < 2e-2


def test_engine_falls_back_and_packs_the_3x3_image_on_demand(lib):
    """Unforced, a 2-row forward of the reduced-width model is far below the occupancy bar: both Upsample layers decline, the engine
    packs the 3x3 image then and gives the bits of the knob-off engine."""
    from grounding_input.text_grounding_tokinzer_input import GroundingNetInput
    from instancediffusion_amd import engine as E, synth
    from instancediffusion_amd.ops import HipOps
    cfg, model = _smoke_model()
    g = torch.Generator().manual_seed(5)
    gb = synth.make_grounding_batch(2, synth.random_boxes(3, g), g)
    x = torch.randn(2, 4, 16, 16, generator=g).cuda()
    ctx = torch.randn(2, 77, 768, generator=g).cuda()
    t = torch.tensor([500, 500]).cuda()
    grounding = {k: v.cuda() for k, v in GroundingNetInput().prepare(gb).items()}
    eng_on = E.UNetEngine(model, ops=HipOps(torch.bfloat16), use_graphs=False)
    eng_parent = E.UNetEngine(model, ops=_WithoutFold(HipOps(torch.bfloat16)), use_graphs=False)
    assert all(p["conv"] is None for p in _up_layers(eng_on))
    eps_on = eng_on.forward_cond(x, t, eng_on.prepare_cond(ctx, grounding)).float().cpu()
    eps_parent = eng_parent.forward_cond(x, t, eng_parent.prepare_cond(ctx, grounding)).float().cpu()
    assert all(p["conv"] is not None for p in _up_layers(eng_on))
    assert torch.equal(eps_on, eps_parent)
