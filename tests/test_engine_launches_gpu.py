"""Every launch of an engine forward on the MI355X, judged against the fp64 references: ``ShadowOps(HipOps(dtype), dt)`` (tests/shadow_ops.py,
proved on the CPU by tests/test_shadow_ops_refs.py) is handed to the full-width UNet, VAE and CLIP engines as ``ops=``, so each of the
launches a forward issues -- with the views, strides, aliasing and keyword combinations the ENGINE builds, which no kernel case table
builds together -- is held to its own per-element bound, 0 elements outside, nothing written beside a view, no input modified.
The end-to-end goldens (tests/test_engine_gpu.py, 2e-2 rel-RMS) say THAT something is off; a failure here names the launch, its
arguments and the engine buffers they live in.

Synthetic weights, the smallest shapes that still reach the code, bf16 and fp16.  Each test prints a ``[launches]`` summary per op
(launches judged, worst error / bound, rows judged / rows total) and what passed through unjudged, which must equal its allow-list.

To point the judge at a new kernel path: give ``ShadowOps`` a ``_plan_<op>`` (tensors, the views the op may write, a judge that calls
the op's fp64 reference), prove it in tests/test_shadow_ops_refs.py with a mutation, and run a forward here that reaches the path.

Kernels these tests cannot reach: the row-resident q | k | v and GEGLU projections and the C = 320 streaming projection take a launch
only from two tiles per CU (M >= 65536 .. 131072 rows), which no knob lowers; the largest forward here has M = 8192.  Their own
modules (tests/test_row_kernels_gpu.py, tests/test_proj320_stream_gpu.py) judge them per element at those sizes.
"""
import dataclasses
import time

import pytest
import torch

from tests import cases
from tests import gemm_conv_run as R
from tests.shadow_ops import HELPERS, ShadowOps

pytestmark = pytest.mark.gpu

DTS = ["bf16", "fp16"]
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
UNET_ALLOW = {"empty", "zeros", "gn_partial_shape", "mlp_supported", "mlp_pack", "proj_row_takes"}
assert UNET_ALLOW <= HELPERS
_MODEL = {}


def unet():
    """The full 1.228 B-parameter model of configs/test_mask.yaml on synthetic weights (built once per session)."""
    if "unet" not in _MODEL:
        from tests.test_engine_emulated import build_model
        _MODEL["unet"] = build_model(cases.cfg_for("test_mask.yaml", "full"))
    return _MODEL["unet"]


def unet_inputs(B, latent, seed, att_masks=False):
    """Boxes, polygons and segs live (the ConvNeXt mask tokens run); ``att_masks``: instance masks at the 64 x 64 resolution."""
    from instancediffusion_amd import synth
    g = torch.Generator().manual_seed(seed)
    boxes = synth.random_boxes(3, g)
    gb = synth.make_grounding_batch(B, boxes, g, with_polygons=True, with_segs=True)
    if att_masks:
        att = torch.zeros(B, 30, 64, 64)
        for i in range(3):
            x1, y1, x2, y2 = (int(round(float(v) * 64)) for v in boxes[i])
            att[:, i, x1:x2, y1:y2] = 1
        gb["att_masks"] = att
    return dict(gb=gb, x=torch.randn(B, 4, latent, latent, generator=g), ctx=torch.randn(B, 77, 768, generator=g),
                uc=torch.randn(B, 77, 768, generator=g), t=torch.tensor([981.0, 400.0][:B]))


def shadow_unet(dt, knobs=None, **kw):
    from instancediffusion_amd.engine import EngineKnobs, UNetEngine
    from instancediffusion_amd.ops import HipOps
    sh = ShadowOps(HipOps(DTYPES[dt]), dt, **kw)
    eng = UNetEngine(unet(), ops=sh, dtype=DTYPES[dt], use_graphs=False,
                     knobs=dataclasses.replace(EngineKnobs.from_env(), **(knobs or {})))
    sh.engine = eng
    return sh, eng


def finish(sh, what, allow, t0):
    """The summary, then the verdict: the first offending launch by its recorded line; the pass-through set against its allow-list."""
    torch.cuda.synchronize()
    sh.print_summary(what)
    print(f"[launches] {what}: {len(sh.records)} launches judged in {time.time() - t0:.1f} s")
    bad = sh.failures()
    assert not bad, f"{len(bad)} launches failed; the first: {sh.line(bad[0])}"
    assert sh.passed == allow, f"passed through unjudged: {sorted(sh.passed)}, allow-list {sorted(allow)}"
    return sh.summary()


def paired_forward(eng, inp):
    """prepare_cond for 2 conditional and 2 null-grounding rows, then ONE paired forward of the 4 rows."""
    from grounding_input.text_grounding_tokinzer_input import GroundingNetInput
    from instancediffusion_amd.engine import Cond
    gi = GroundingNetInput()
    g = {k: v.cuda() for k, v in gi.prepare(inp["gb"]).items()}
    pair = Cond.cat([eng.prepare_cond(inp["ctx"].cuda(), g), eng.prepare_cond(inp["uc"].cuda(), gi.get_null_input(batch=2))])
    eps = eng.forward_cond(inp["x"].cuda(), inp["t"].cuda(), pair, paired=True)
    assert tuple(eps.shape) == (4, 4) + tuple(inp["x"].shape[2:]) and bool(torch.isfinite(eps).all())
    return pair


@pytest.mark.parametrize("dt", DTS)
def test_unet_default_dispatch(dt):
    """16 x 16 latent, 4 rows (levels 16^2 / 8^2 / 4^2 / 2^2: N = 256 takes the fused q | k | v launch with V^T stored into the [C][B][N]
    image, the lower levels the two-GEMM form with the padded V^T leading dimension), then 1 row at 24 x 24 (levels 24 / 12 / 6 / 3: odd
    planes, no ``gn_partial`` below the first level)."""
    t0 = time.time()
    sh, eng = shadow_unet(dt, strict=False)
    with torch.no_grad():
        pair = paired_forward(eng, unet_inputs(2, 16, 50))
        n16 = len(sh.records)
        one = unet_inputs(1, 24, 51)
        eng.forward_cond(one["x"].cuda(), one["t"].cuda(), pair.select(torch.tensor([0], device="cuda")))
    s = finish(sh, f"unet default {dt}", UNET_ALLOW, t0)
    flags = {r["flags"] for r in sh.records if r["op"] == "gemm"}
    assert any("gate" in f and "res" in f for f in flags) and any("geglu32" in f for f in flags), flags
    assert any("vt_out" in f for f in flags) and any("ln_col" in f for f in flags) and any("rowbias" in r["flags"] for r in sh.records)
    assert any("gn_partial" in r["flags"] for r in sh.records[:n16])
    odd = [r for r in sh.records[n16:] if r["op"] == "conv3x3" and tuple(r["args"]["out"][0][1:3]) in ((12, 12), (6, 6), (3, 3))]
    assert odd and not any("gn_partial" in r["flags"] for r in odd), "12^2 / 6^2 / 3^2 planes are no whole 64-row chunks: no partials"
    assert {"gemm", "conv3x3", "attention", "groupnorm", "layernorm", "scaleu_concat", "conv_in", "cast16", "timestep_embedding",
            "unifusion_embed", "seg_in_conv", "dwconv7x7", "layernorm_patch2"} <= set(s)


@pytest.mark.parametrize("dt", DTS)
def test_unet_bench_kernels_at_small_m(dt):
    """The same 16 x 16, 4-row forward with the fused MLP from 128 rows (``mlp_min_m``) and the persistent GEMM / conv kernel wherever
    the shape qualifies (IDF_TUNE_GEMM_BIG = 2, restored): the counters must show the persistent kernel, the conv-epilogue GroupNorm
    partials and the shortcut-as-K-tiles conv serving launches, and ``conv_up2x`` / ``conv3x3_skip`` / ``mlp_geglu`` must have run."""
    from instancediffusion_amd import _lib
    t0 = time.time()
    sh, eng = shadow_unet(dt, knobs=dict(mlp_min_m=128), strict=False)
    lib = sh.lib
    names = ("GEMM_BIG", "GN_EPI", "SKIP_FOLD", "ATTN2", "ATTN8", "ATTN_RES", "QKV_ROW", "GEGLU_ROW", "PROJ_ROW")
    stat = lambda: {n: int(lib.idf_get_stat(getattr(_lib, f"IDF_STAT_{n}_LAUNCHES"))) for n in names}
    with R.forced(lib, "big"), torch.no_grad():
        before = stat()
        paired_forward(eng, unet_inputs(2, 16, 50))
        served = {n: v - before[n] for n, v in stat().items()}
    print(f"[launches] unet bench kernels {dt}: launch counters {served}")
    s = finish(sh, f"unet bench kernels {dt}", UNET_ALLOW, t0)
    assert served["GEMM_BIG"] > 0 and served["GN_EPI"] > 0 and served["SKIP_FOLD"] > 0, served
    assert served["ATTN2"] + served["ATTN8"] + served["ATTN_RES"] > 0, served
    assert s.get("mlp_geglu", {}).get("launches", 0) > 0, "the fused MLP took no launch"
    assert any(sh.returned.get("conv_up2x", [])) and any(sh.returned.get("conv3x3_skip", [])), sh.returned


@pytest.mark.parametrize("dt", DTS)
def test_unet_masked_gated_self_attention(dt):
    """The visibility words apply only at N = 64^2: one 2-row forward at a 64 x 64 latent with instance masks live, judged on sampled rows;
    it also reaches the default-dispatch kernels of the real size."""
    from grounding_input.text_grounding_tokinzer_input import GroundingNetInput
    t0 = time.time()
    model = unet()
    model.efficient_attention = False
    try:
        sh, eng = shadow_unet(dt, strict=False)
    finally:
        model.efficient_attention = True
    assert eng.masked_fuser
    inp = unet_inputs(2, 64, 52, att_masks=True)
    with torch.no_grad():
        g = {k: v.cuda() for k, v in GroundingNetInput().prepare(inp["gb"], return_att_masks=True).items()}
        cond = eng.prepare_cond(inp["ctx"].cuda(), g)
        assert cond.vis, "the instance masks did not reach the conditioning"
        eps = eng.forward_cond(inp["x"].cuda(), inp["t"].cuda(), cond)
    assert bool(torch.isfinite(eps).all())
    finish(sh, f"unet masked 64x64 {dt}", UNET_ALLOW, t0)
    masked = [r for r in sh.records if r["op"] == "attention" and "mask" in r["flags"]]
    assert masked and all(r["args"]["q"][0][1] == 4096 for r in masked)
    assert any(r["parts"][0]["rows"] < r["parts"][0]["total"] for r in sh.records), "nothing was sampled at the real size"


@pytest.mark.parametrize("dt", DTS)
def test_vae(dt):
    """Full decoder on a 2 x 4 x 8 x 8 latent (the head-dim-512 attention chain: batched strided fp32-out GEMM, softmax_rows, batched GEMM with
    bias) and full encoder on a 2 x 3 x 64 x 64 image (conv3x3_down, vae_posterior with noise and moments)."""
    from instancediffusion_amd.ops import HipOps
    from instancediffusion_amd.vae_engine import VAEDecoderEngine, VAEEncoderEngine
    if "vae" not in _MODEL:
        _MODEL["vae"] = cases.build_vae(cases.vae_cfg_for("full"))
    g = torch.Generator().manual_seed(53)
    t0 = time.time()
    sh = ShadowOps(HipOps(DTYPES[dt]), dt, strict=False)
    dec = VAEDecoderEngine(_MODEL["vae"], ops=sh, dtype=DTYPES[dt], use_graphs=False)
    sh.engine = dec
    with torch.no_grad():
        img = dec.decode((torch.randn(2, 4, 8, 8, generator=g) * 0.7).cuda())
    assert tuple(img.shape) == (2, 3, 64, 64) and bool(torch.isfinite(img).all())
    s = finish(sh, f"vae decode {dt}", {"empty"}, t0)
    assert {"pointwise_nchw", "conv_in", "softmax_rows", "gemm", "conv3x3", "groupnorm"} <= set(s)
    assert any("f32out" in r["flags"] and "batched" in r["flags"] for r in sh.records if r["op"] == "gemm")
    t0 = time.time()
    sh = ShadowOps(HipOps(DTYPES[dt]), dt, strict=False)
    enc = VAEEncoderEngine(_MODEL["vae"], ops=sh, dtype=DTYPES[dt], use_graphs=False)
    sh.engine = enc
    from tests import vae_encode_cases as vc
    with torch.no_grad():
        z, moments = enc.encode(vc.encode_image(2, 64, 54).cuda(), torch.randn(2, 4, 8, 8, generator=g).cuda())
    assert bool(torch.isfinite(z).all()) and bool(torch.isfinite(moments).all())
    s = finish(sh, f"vae encode {dt}", {"empty"}, t0)
    assert {"conv3x3_down", "vae_posterior", "softmax_rows"} <= set(s)
    assert any("noise" in r["flags"] and "moments" in r["flags"] for r in sh.records if r["op"] == "vae_posterior")


@pytest.mark.parametrize("dt", DTS)
def test_clip(dt):
    """The full text tower on 3 x 77 ids and the image tower at its real width (2 images)."""
    pytest.importorskip("transformers")
    from instancediffusion_amd.clip_engine import CLIPTextEngine, CLIPVisionEngine
    from instancediffusion_amd.ops import HipOps
    from tests import clip_cases
    from tests import clip_vision_cases as cv
    t0 = time.time()
    sh = ShadowOps(HipOps(DTYPES[dt]), dt, strict=False)
    eng = CLIPTextEngine(clip_cases.full_transformer(), ops=sh, dtype=DTYPES[dt])
    sh.engine = eng
    ids = clip_cases.load_golden("clip_text")["input_ids"]
    third = ids[1].clone()
    third[1:5] = ids[0][1:5]                                 # a third sequence of its own: the golden keeps two
    z, _ = eng.encode_ids(torch.cat([ids[:2], third[None]]))
    assert tuple(z.shape)[:2] == (3, 77) and bool(torch.isfinite(z).all())
    s = finish(sh, f"clip text {dt}", {"empty"}, t0)
    assert {"clip_embed", "attention_causal", "gemm", "layernorm"} <= set(s)
    t0 = time.time()
    sh = ShadowOps(HipOps(DTYPES[dt]), dt, strict=False)
    ve = CLIPVisionEngine(cv.full_vision(), ops=sh, dtype=DTYPES[dt])
    sh.engine = ve
    out = ve.encode_pixels(cv.pixel_values(2, cv.FULL_VISION["image_size"]))
    assert bool(torch.isfinite(out[0]).all())
    s = finish(sh, f"clip vision {dt}", {"empty"}, t0)
    assert {"clip_patchify", "attention_qkv", "gemm", "layernorm"} <= set(s)
