"""The engine's wiring around proj320s_kernel on the CPU op emulation: an ops object that claims the kernel takes the C = 320
projections (``proj_row_takes``) makes the engine hand the cross-attention query its statistics from the producer in front of it.
Every combination of fuser on / off, paired forward or not, q | k | v row kernel on / off and fused / two-GEMM feed-forward must
equal the forward of an engine whose ops object has no such kernel -- in particular the paired forward with the q | k | v row kernel
off and the fuser's feed-forward unfused, where the statistics buffer is allocated BEHIND the duplication of the first layer."""
import dataclasses

import pytest
import torch

from grounding_input.text_grounding_tokinzer_input import GroundingNetInput
from instancediffusion_amd.engine import Cond, EngineKnobs, UNetEngine
from tests import cases
from tests.emul_ops import EmulOps
from tests.test_engine_emulated import build_model


class _Takes(EmulOps):
    """The emulated ops with the query of every C = 320 layer claimed by the streaming kernel; counts the queries handed statistics."""
    handed = 0

    def proj_row_takes(self, M, C):
        return C == 320

    def gemm(self, a, w, out, **kw):
        ln = kw.get("ln_row")
        if ln is not None and ln[0] is not None and w.shape[-2] == 320 and w.shape[-1] == 320 and kw.get("vt_out") is None:
            assert ln[0].shape[-2] == a.shape[-2]
            self.handed += 1
        return super().gemm(a, w, out, **kw)


@pytest.mark.parametrize("ff_fused", [True, False])
@pytest.mark.parametrize("qkv_row", [True, False])
@pytest.mark.parametrize("paired", [True, False])
@pytest.mark.parametrize("fuser", [True, False])
def test_handing_the_query_its_statistics_changes_nothing(fuser, paired, qkv_row, ff_fused):
    from instancediffusion_amd import synth
    knobs = dataclasses.replace(EngineKnobs.from_env(), qkv_row=qkv_row, mlp_min_m=0 if ff_fused else 1 << 30)
    cfg = cases.cfg_for("test_box.yaml", "mid")
    model = build_model(cfg)
    g = torch.Generator().manual_seed(41)
    gb = synth.make_grounding_batch(2, synth.random_boxes(3, g), g)
    x = torch.randn(2, 4, 16, 16, generator=g)
    ctx, uc = torch.randn(2, 77, 768, generator=g), torch.randn(2, 77, 768, generator=g)
    t = torch.tensor([700.0, 300.0])
    gi = GroundingNetInput()
    grounding = gi.prepare(gb)
    outs = []
    with torch.no_grad():
        for ops in (_Takes(torch.float32, batch_invariant=True), EmulOps(torch.float32, batch_invariant=True)):
            eng = UNetEngine(model, ops=ops, use_graphs=False, knobs=knobs)
            if not fuser:
                eng.set_fuser_scale(0.0)
            pair = Cond.cat([eng.prepare_cond(ctx, grounding), eng.prepare_cond(uc, gi.get_null_input(batch=2))])
            outs.append(eng.forward_cond(torch.cat([x, x]), torch.cat([t, t]), pair, paired=paired))
            if isinstance(ops, _Takes):
                sts = [p for blk in eng.in_blocks + [eng.mid_block] + eng.out_blocks for p in blk if p["kind"] == "st" and p["c"] == 320]
                n320 = len(sts)
                fused_ff = ff_fused and all("w2p" in p["f_ff"] for p in sts) and ops.mlp_supported(4 * 256, 320)
                want = 0 if (eng.knobs.ln_self != 1 or (fuser and fused_ff)) else n320
                assert n320 > 0 and ops.handed == want, (ops.handed, want)
    assert torch.isfinite(outs[0]).all()
    assert cases.rel_rms(outs[0], outs[1]) < 1e-5
