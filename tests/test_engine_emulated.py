"""Host-logic tests of the engine (no GPU): the op sequence, weight packing, in-place residual aliasing, Cond
caches and two-segment attention bookkeeping are exercised against the CPU oracle / reference goldens through the
CPU op emulation in tests/emul_ops.py.  With fp32 storage the engine must agree with the reference to fp32 round-off;
with bf16 storage the error shows what to expect from the MI355X kernels.
"""
import dataclasses
import os

import pytest
import torch

from instancediffusion_amd import synth
from instancediffusion_amd.engine import EngineKnobs, UNetEngine, pack_geglu
from instancediffusion_amd.host.config import unet_kwargs_from_cfg
from ldm.modules.diffusionmodules.openaimodel import UNetModel
from grounding_input.text_grounding_tokinzer_input import GroundingNetInput
from tests import cases
from tests.emul_ops import EmulOps


_SYNTH_CACHE = {}                            # one entry: (schema key) -> key-seeded state dict


def _synth_sd(schema):
    """synth.synth_state_dict(schema), kept for the next model of the same schema: the 1.228 B-parameter model's weights are 7 s of
    CPU randn, and two dozen GPU tests build that model one after the other (load_state_dict COPIES: a test that edits its model
    -- the first-conv swap, the fuser scale -- never touches the cached tensors)."""
    key = hash(tuple(sorted(schema.items())))
    if key not in _SYNTH_CACHE:
        _SYNTH_CACHE.clear()
        _SYNTH_CACHE[key] = synth.synth_state_dict(schema)
    return _SYNTH_CACHE[key]


def build_model(cfg, efficient_attention=True):
    with torch.device("meta"):
        m = UNetModel(**dict(unet_kwargs_from_cfg(cfg), efficient_attention=efficient_attention))
    m = m.to_empty(device="cpu")
    m.load_state_dict(_synth_sd({k: tuple(v.shape) for k, v in m.state_dict().items()}))
    return m.eval()


# The default CPU suite keeps the fp32 runs of the four reduced-width configurations (every host-logic branch: packing,
# LayerNorm folding, Cond caches, batching) within a few minutes; the real-width "mid" model and the bf16 STORAGE emulations
# (CPU bf16 matmuls: 1.5 - 3 min each) only predict what the GPU parity tests measure directly and run with IDF_FULL_CPU_SUITE=1.
FULL = os.environ.get("IDF_FULL_CPU_SUITE") == "1"
heavy = pytest.mark.skipif(not FULL, reason="heavy CPU emulation: set IDF_FULL_CPU_SUITE=1 (the GPU parity tests cover it)")


@pytest.mark.parametrize("tag,dtype,tol", [
    ("tiny_box", torch.float32, 3e-4), ("tiny_point", torch.float32, 3e-4),
    pytest.param("mid_box", torch.float32, 3e-4, marks=heavy),
    ("tiny_mask", torch.float32, 3e-4), ("tiny_scribble", torch.float32, 3e-4),
    pytest.param("tiny_mask", torch.bfloat16, 4e-2, marks=heavy), pytest.param("tiny_box", torch.bfloat16, 4e-2, marks=heavy),
    pytest.param("mid_box", torch.bfloat16, 4e-2, marks=heavy),
])
def test_engine_forward_vs_reference(tag, dtype, tol):
    gold = cases.load_golden(tag)
    meta = gold["meta"]
    cfg = cases.cfg_for(meta["cfg"], meta["variant"])
    inp = cases.build_inputs(meta)
    model = build_model(cfg)
    eng = UNetEngine(model, ops=EmulOps(dtype), use_graphs=False)
    gi = GroundingNetInput()
    g = gi.prepare(inp["gb"])
    with torch.no_grad():
        cond = eng.prepare_cond(inp["context"], g)
        eps = eng.forward_cond(inp["x"], inp["t"], cond)
        err = cases.rel_rms(eps, gold["eps_cond"])
        assert err < tol, f"cond rel-rms {err}"
        cond0 = eng.prepare_cond(inp["uc"], gi.get_null_input())
        err = cases.rel_rms(eng.forward_cond(inp["x"], inp["t"], cond0), gold["eps_uncond"])
        assert err < tol, f"uncond rel-rms {err}"
        eng.set_fuser_scale(0.3)
        err = cases.rel_rms(eng.forward_cond(inp["x"], inp["t"], cond), gold["eps_scale03"])
        assert err < tol, f"scale 0.3 rel-rms {err}"
        # batched cond+uncond in one forward == the two separate forwards
        eng.set_fuser_scale(1.0)
        both = eng.forward_cond(torch.cat([inp["x"], inp["x"]]), torch.cat([inp["t"], inp["t"]]),
                                type(cond).cat([cond, cond0]))
        B = inp["x"].shape[0]
        assert cases.rel_rms(both[:B], gold["eps_cond"]) < tol and cases.rel_rms(both[B:], gold["eps_uncond"]) < tol


@pytest.mark.parametrize("mode", [0, 2])
def test_layernorm_statistics_sources_agree(mode):
    """The three ways the LN-folded GEMMs get (mu, rstd) -- from the producer's out_stats pass (mode 0), summed by the
    consumer itself (mode 2), the default mix (mode 1) -- are the same arithmetic on the same rows: the emulated forward
    must agree to fp32 round-off whichever buffers carry them (catches a stale or clobbered `st.stats`)."""
    gold = cases.load_golden("tiny_mask")
    meta = gold["meta"]
    cfg = cases.cfg_for(meta["cfg"], meta["variant"])
    inp = cases.build_inputs(meta)
    model = build_model(cfg)
    g = GroundingNetInput().prepare(inp["gb"])
    outs = {}
    for m in (1, mode):
        eng = UNetEngine(model, ops=EmulOps(torch.float32), use_graphs=False, knobs=dataclasses.replace(EngineKnobs.from_env(), ln_self=m))
        with torch.no_grad():
            cond = eng.prepare_cond(inp["context"], g)
            outs[m] = eng.forward_cond(inp["x"], inp["t"], cond).clone()
    assert cases.rel_rms(outs[mode], outs[1]) < 1e-5
    assert cases.rel_rms(outs[mode], gold["eps_cond"]) < 3e-4


def test_fuser_skipped_at_scale_zero_is_exact():
    gold = cases.load_golden("tiny_box")
    meta = gold["meta"]
    cfg = cases.cfg_for(meta["cfg"], meta["variant"])
    inp = cases.build_inputs(meta)
    model = build_model(cfg)
    eng = UNetEngine(model, ops=EmulOps(torch.float32), use_graphs=False)
    g = GroundingNetInput().prepare(inp["gb"])
    from oracle import ref_cpu
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    with torch.no_grad():
        cond = eng.prepare_cond(inp["context"], g)
        eng.set_fuser_scale(0.0)
        n_att = eng.ops.calls.get("attention", 0)
        eps = eng.forward_cond(inp["x"], inp["t"], cond)
        n_st = eng.n_st
        assert eng.ops.calls["attention"] - n_att == 2 * n_st          # self + cross only: fuser launches skipped
        objs, _ = ref_cpu.unifusion(sd, cfg, ref_cpu.prepare_grounding(inp["gb"]))
        ref = ref_cpu.unet_forward(sd, cfg, inp["x"], inp["t"], inp["context"], objs, fuser_scale=0.0)
    assert cases.rel_rms(eps, ref) < 3e-4


def test_pack_geglu_layout():
    w = torch.arange(128 * 4, dtype=torch.float32).reshape(128, 4)
    b = torch.arange(128, dtype=torch.float32)
    wp, bp = pack_geglu(w, b)
    # packed rows [0:32] = value rows 0..31, [32:64] = gate rows 64..95, [64:96] = value 32..63, [96:128] = gate 96..127
    assert torch.equal(bp[:32], b[:32]) and torch.equal(bp[32:64], b[64:96])
    assert torch.equal(bp[64:96], b[32:64]) and torch.equal(bp[96:], b[96:])
    assert torch.equal(wp[40], w[72])


def test_model_forward_refuses_without_hip(monkeypatch):
    """The product path must fail loudly (no silent CPU fallback) when there is no GPU."""
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    cfg = cases.cfg_for("test_box.yaml", "tiny")
    model = build_model(cfg)
    with pytest.raises(RuntimeError):
        model.engine


def test_broadcast_mask_stack_is_tokenized_once():
    """utils/input.py mirror hands ``segs`` over as a stride-0 batch broadcast; the tokenizer must give the same tokens
    as for the reference's ``.repeat`` copies while running the ConvNeXt backbone on ONE sample."""
    gold = cases.load_golden("tiny_mask")
    meta = gold["meta"]
    cfg = cases.cfg_for(meta["cfg"], meta["variant"])
    inp = cases.build_inputs(dict(meta, batch=1))
    model = build_model(cfg)
    gi = GroundingNetInput()
    gb1 = inp["gb"]
    rep = {k: v.repeat(3, *([1] * (v.dim() - 1))) for k, v in gb1.items()}
    bc = dict(rep, segs=gb1["segs"][0].unsqueeze(0).expand(3, *gb1["segs"].shape[1:]))
    assert bc["segs"].stride(0) == 0
    with torch.no_grad():
        e1 = UNetEngine(model, ops=EmulOps(torch.float32), use_graphs=False)
        t_rep = e1.tokens(gi.prepare(rep))
        e2 = UNetEngine(model, ops=EmulOps(torch.float32), use_graphs=False)
        t_bc = e2.tokens(gi.prepare(bc))
    assert torch.allclose(t_rep, t_bc, atol=1e-6) and t_bc.shape[0] == 3
    assert e1.ops.calls["seg_in_conv"] == 1 and e2.ops.calls["seg_in_conv"] == 1
    assert e2.ops.calls["dwconv7x7"] == e1.ops.calls["dwconv7x7"]        # same launches, one third of the rows


def test_fused_qkv_projection_equals_the_two_gemm_form():
    """From ``knobs.vt_min_n`` tokens per sample (round 5: 256; rounds 3-4: 1024) the engine issues ONE q | k | v GEMM whose last C
    columns land transposed in the batch-interleaved V^T image (``vt_out``, include/idf.h); below, and with IDF_VT_GLOBAL=0, the
    q | k GEMM plus the transposed-V GEMM it replaced.  Same forward every way (32x32 latent on the 3-level model: the 320-channel
    level has 1024 tokens, the 640-channel level 256, the last one 64), also against the CPU oracle; the fused call count is checked."""
    from oracle import ref_cpu
    cfg = cases.cfg_for("test_box.yaml", "mid")
    model = build_model(cfg)
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(21)
    from instancediffusion_amd import synth
    gb = synth.make_grounding_batch(2, synth.random_boxes(3, g), g)
    x = torch.randn(2, 4, 32, 32, generator=g)
    ctx = torch.randn(2, 77, 768, generator=g)
    t = torch.tensor([700.0, 300.0])
    grounding = GroundingNetInput().prepare(gb)
    outs = []
    with torch.no_grad():
        for vt_global, min_n in ((True, 256), (True, 1024), (False, 256)):
            ops = EmulOps(torch.float32)
            fused_calls = [0]
            real = ops.gemm

            def counting(*a, _real=real, **k):
                fused_calls[0] += k.get("vt_out") is not None
                return _real(*a, **k)
            ops.gemm = counting
            eng = UNetEngine(model, ops=ops, use_graphs=False)
            assert eng.knobs.vt_min_n == 256                # the shipped default
            eng.knobs = dataclasses.replace(eng.knobs, vt_global=vt_global, vt_min_n=min_n)
            cond = eng.prepare_cond(ctx, grounding)
            outs.append(eng.forward_cond(x, t, cond))
            n_fused = sum(1 for p in eng._st_layers() if p["c"] == 320 or (p["c"] == 640 and min_n <= 256))
            assert fused_calls[0] == (2 * n_fused if vt_global else 0)          # self + gated self-attention per layer
        objs, _ = ref_cpu.unifusion(sd, cfg, ref_cpu.prepare_grounding(gb))
        want = ref_cpu.unet_forward(sd, cfg, x, t.long(), ctx, objs)
    assert cases.rel_rms(outs[0], outs[2]) < 1e-5 and cases.rel_rms(outs[1], outs[2]) < 1e-5
    assert cases.rel_rms(outs[0], want) < 3e-4


def test_fused_mlp_is_used_from_its_row_threshold_and_equals_the_two_gemm_form():
    """engine._ff sends the GEGLU feed-forward of a C = 320 block to the fused kernel (ops.mlp_geglu) only from
    ``knobs.mlp_min_m`` token rows up -- below, the kernel's 128-row tiles no longer fill the chip and the two GEMMs are faster
    (profiles/r04_mlp_small_m.log).  Same forward either way; call counts checked (3-level model, 32x32 latent: the 320-channel
    level has 2 x 1024 rows)."""
    cfg = cases.cfg_for("test_box.yaml", "mid")
    model = build_model(cfg)
    g = torch.Generator().manual_seed(22)
    gb = synth.make_grounding_batch(2, synth.random_boxes(3, g), g)
    x = torch.randn(2, 4, 32, 32, generator=g)
    ctx = torch.randn(2, 77, 768, generator=g)
    t = torch.tensor([700.0, 300.0])
    grounding = GroundingNetInput().prepare(gb)
    outs, calls = [], []
    with torch.no_grad():
        for min_m in (2048, 2049):                               # M = 2 x 1024 rows at the 320-channel level
            ops = EmulOps(torch.float32)
            eng = UNetEngine(model, ops=ops, use_graphs=False, knobs=dataclasses.replace(EngineKnobs.from_env(), mlp_min_m=min_m))
            cond = eng.prepare_cond(ctx, grounding)
            before = ops.calls.get("mlp_geglu", 0)
            outs.append(eng.forward_cond(x, t, cond))
            calls.append(ops.calls.get("mlp_geglu", 0) - before)
            n_top = sum(1 for p in eng._st_layers() if p["c"] == 320)
    assert eng.knobs.mlp_fused and calls == [2 * n_top, 0] and n_top > 0          # the fuser's feed-forward and the block's own, per layer
    assert cases.rel_rms(outs[0], outs[1]) < 1e-5


@pytest.mark.parametrize("fuser", [True, False])
def test_paired_forward_hoists_the_conditioning_free_prefix_exactly(fuser):
    """A guidance batch [cond | uncond] carries the same latent and timestep in both halves: with ``paired=True`` the engine
    runs the first conv, the first ResBlock and the first block's self-attention ONCE for the n distinct rows and duplicates
    them behind the last layer that does not read the conditioning (``knobs.pair_hoist``).  Exact: the same bits as the forward
    over all 2n rows (batch-invariant emulator), with half the attention rows in that first self-attention; also with the
    fuser switched off (alpha = 0 stage), and equal to the CPU oracle."""
    from oracle import ref_cpu
    from instancediffusion_amd.engine import Cond
    cfg = cases.cfg_for("test_box.yaml", "mid")
    model = build_model(cfg)
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(33)
    gb = synth.make_grounding_batch(2, synth.random_boxes(3, g), g)
    x = torch.randn(2, 4, 16, 16, generator=g)
    ctx, uc = torch.randn(2, 77, 768, generator=g), torch.randn(2, 77, 768, generator=g)
    t = torch.tensor([700.0, 300.0])
    gi = GroundingNetInput()
    grounding = gi.prepare(gb)
    outs, rows = [], []
    with torch.no_grad():
        for hoist in (True, False):
            eng = UNetEngine(model, ops=EmulOps(torch.float32, batch_invariant=True), use_graphs=False,
                             knobs=dataclasses.replace(EngineKnobs.from_env(), pair_hoist=hoist))
            if not fuser:
                eng.set_fuser_scale(0.0)
            pair = Cond.cat([eng.prepare_cond(ctx, grounding), eng.prepare_cond(uc, gi.get_null_input(batch=2))])
            r0 = eng.ops.rows.get("attention", 0)
            outs.append(eng.forward_cond(torch.cat([x, x]), torch.cat([t, t]), pair, paired=True))
            rows.append(eng.ops.rows["attention"] - r0)
        objs, _ = ref_cpu.unifusion(sd, cfg, ref_cpu.prepare_grounding(gb))
        want = ref_cpu.unet_forward(sd, cfg, x, t.long(), ctx, objs, fuser_scale=1.0 if fuser else 0.0)
    assert torch.equal(outs[0], outs[1]), "the hoisted prefix must give the bits of the full-width forward"
    assert rows[0] == rows[1] - 2, (rows, "one self-attention launch over n = 2 instead of 2n = 4 rows")
    assert cases.rel_rms(outs[0][:2], want) < 3e-4


def test_paired_flag_on_a_batch_that_is_not_a_guidance_pair_is_rejected():
    """VERDICT r4 / ADVICE r4: ``forward_cond(paired=True)`` trusts the caller that rows [n, 2n) repeat (x, t) of rows [0, n).
    The guarantee is verified when a launch configuration is first used (and on every call with IDF_DEBUG_PAIRED=1): a batch
    with different latents OR different timesteps in its halves raises instead of returning the hoisted (wrong) eps."""
    from instancediffusion_amd.engine import Cond
    cfg = cases.cfg_for("test_box.yaml", "tiny")
    model = build_model(cfg)
    g = torch.Generator().manual_seed(34)
    gb = synth.make_grounding_batch(2, synth.random_boxes(3, g), g)
    x = torch.randn(2, 4, 16, 16, generator=g)
    ctx, uc = torch.randn(2, 77, 768, generator=g), torch.randn(2, 77, 768, generator=g)
    t = torch.tensor([700.0, 300.0])
    gi = GroundingNetInput()
    with torch.no_grad():
        eng = UNetEngine(model, ops=EmulOps(torch.float32), use_graphs=False)
        pair = Cond.cat([eng.prepare_cond(ctx, gi.prepare(gb)), eng.prepare_cond(uc, gi.get_null_input(batch=2))])
        x2 = torch.cat([x, x + 1e-3])
        with pytest.raises(ValueError, match="paired=True"):
            eng.forward_cond(x2, torch.cat([t, t]), pair, paired=True)
        with pytest.raises(ValueError, match="paired=True"):
            eng.forward_cond(torch.cat([x, x]), torch.cat([t, t + 1]), pair, paired=True)
        ok = eng.forward_cond(torch.cat([x, x]), torch.cat([t, t]), pair, paired=True)      # a real pair passes (and marks the key)
        assert torch.isfinite(ok).all()
        # the same key again: not re-checked by default (no host sync per step) ...
        eng.forward_cond(x2, torch.cat([t, t]), pair, paired=True)
        # ... but on every call in debug mode
        eng.knobs = dataclasses.replace(eng.knobs, debug_paired=True)
        with pytest.raises(ValueError, match="paired=True"):
            eng.forward_cond(x2, torch.cat([t, t]), pair, paired=True)
        # without the flag the same batch is an ordinary 4-row forward
        assert torch.isfinite(eng.forward_cond(x2, torch.cat([t, t]), pair)).all()
        # the structural form -- the caller hands over the n DISTINCT rows and the engine writes both halves of its
        # input itself; nothing to verify, and the result is the full pair's, bit for bit (this is what the samplers do)
        eng.knobs = dataclasses.replace(eng.knobs, debug_paired=False)
        half = eng.forward_cond(x, t, pair, paired=True)
        assert tuple(half.shape) == (4, 4, 16, 16) and torch.equal(half, ok)


def test_groupnorm_partials_travel_from_the_producing_conv_to_the_next_groupnorm():
    """Round 5: a 3x3 conv whose output feeds a GroupNorm leaves that GroupNorm's partial statistics (idf_conv3x3 gn_partial) and the
    GroupNorm only normalises.  The engine hands the partials from a producing conv to the layer that follows IMMEDIATELY -- ResBlock
    conv1 -> its second GroupNorm, ResBlock conv2 -> the SpatialTransformer's norm / the next ResBlock's first GroupNorm, Downsample ->
    the next ResBlock -- and drops them behind anything else: a SpatialTransformer rewrites its input buffer in place, and the decoder's
    first GroupNorm reads the ScaleU concat.  Checked: every partial a conv leaves is consumed by exactly one GroupNorm, the GroupNorms
    behind a SpatialTransformer / a concat run their own statistics pass, and the forward equals the IDF_GN_EPI=0 one to fp32 rounding."""
    cfg = cases.cfg_for("test_box.yaml", "mid")
    model = build_model(cfg)
    g = torch.Generator().manual_seed(35)
    gb = synth.make_grounding_batch(2, synth.random_boxes(3, g), g)
    x = torch.randn(2, 4, 32, 32, generator=g)
    ctx = torch.randn(2, 77, 768, generator=g)
    t = torch.tensor([700.0, 300.0])
    grounding = GroundingNetInput().prepare(gb)
    outs, counts = [], []
    with torch.no_grad():
        for epi in (True, False):
            ops = EmulOps(torch.float32)
            eng = UNetEngine(model, ops=ops, use_graphs=False, knobs=dataclasses.replace(EngineKnobs.from_env(), gn_epi=epi))
            cond = eng.prepare_cond(ctx, grounding)
            c0 = dict(ops.calls)
            outs.append(eng.forward_cond(x, t, cond))
            counts.append({k: ops.calls.get(k, 0) - c0.get(k, 0) for k in ("conv3x3_gn_partial", "groupnorm_from_partial", "groupnorm")})
    on, off = counts
    assert off["conv3x3_gn_partial"] == 0 and off["groupnorm_from_partial"] == 0
    assert on["groupnorm"] == off["groupnorm"]                                     # the same GroupNorms run either way
    assert on["conv3x3_gn_partial"] == on["groupnorm_from_partial"] > 0            # produced exactly where consumed
    # GroupNorms that keep their own pass: the first ResBlock's (behind conv_in), the ones behind a SpatialTransformer, the decoder's
    # first (ScaleU concat) and the output GroupNorm
    n_res = sum(1 for blk in list(eng.in_blocks) + [eng.mid_block] + list(eng.out_blocks) for p in blk if p["kind"] == "res")
    n_st_after_res = sum(1 for blk in list(eng.in_blocks) + [eng.mid_block] + list(eng.out_blocks)
                         for a, b in zip(blk, blk[1:]) if a["kind"] == "res" and b["kind"] == "st")
    assert on["groupnorm_from_partial"] >= n_res + n_st_after_res                  # every gn2 + every norm right behind a ResBlock
    assert on["groupnorm_from_partial"] < on["groupnorm"]
    assert cases.rel_rms(outs[0], outs[1]) < 2e-5        # fp32 summation order of the statistics only (64-row chunk partials vs F.group_norm)
