"""A reader of LN(y) that is HANDED its statistics must get what the GEMM that last wrote y emitted (engine._ln_routing).  If a reader
and the writer in front of it ever disagree, a GEMM normalises with the statistics of rows that have changed since, and nothing
raises.  The ops double here makes that visible: after every ``gemm`` / ``mlp_geglu`` call that writes the residual stream (the
``st.x`` / ``st.x2`` buffers) while emitting neither ``out_stats`` nor ``ln_stats_out``, it fills every live ``st.stats`` /
``st.stats2`` buffer with NaN.  The forward must stay finite and equal, bit for bit, the forward of the plain double.

Cases: every value of every switch that the routing reads, each against otherwise-default knobs (paired forward, fuser on, no
``proj_row_takes``), plus the corner where the statistics buffer is allocated BEHIND the duplication of the paired forward (fuser
on: the query's statistics come from the fuser's two-GEMM feed-forward) and the same corner with the fuser off.  Inputs: those of
tests/test_proj320_engine_emulated.py (the 320-channel level has 256 tokens: fused q | k | v; the deeper levels are unfused)."""
import dataclasses

import pytest
import torch

from grounding_input.text_grounding_tokinzer_input import GroundingNetInput
from instancediffusion_amd import synth
from instancediffusion_amd.engine import Cond, EngineKnobs, UNetEngine
from tests import cases
from tests.emul_ops import EmulOps
from tests.test_engine_emulated import build_model


def _poisoning(base):
    class Poisoning(base):
        eng = None

        def _wrote(self, out, emitted):
            bufs = self.eng._bufs if self.eng is not None else {}
            ptr = out.untyped_storage().data_ptr()
            if not emitted and any(role in ("st.x", "st.x2") and t.untyped_storage().data_ptr() == ptr for (role, _, _), t in bufs.items()):
                for (role, _, _), t in bufs.items():
                    if role in ("st.stats", "st.stats2"):
                        t.fill_(float("nan"))
                self.poisoned += 1

        def gemm(self, a, w, out, **kw):
            r = super().gemm(a, w, out, **kw)
            self._wrote(out, kw.get("out_stats") is not None or kw.get("ln_stats_out") is not None)
            return r

        def mlp_geglu(self, x, stats, w1, cd, w2p, b2, out, **kw):
            r = super().mlp_geglu(x, stats, w1, cd, w2p, b2, out, **kw)
            self._wrote(out, False)
            return r
    ops = Poisoning(torch.float32, batch_invariant=True)
    ops.poisoned = 0
    return ops


class _Takes(EmulOps):
    def proj_row_takes(self, M, C):
        return C == 320


@pytest.fixture(scope="module")
def inputs():
    model = build_model(cases.cfg_for("test_box.yaml", "mid"))
    g = torch.Generator().manual_seed(41)
    gb = synth.make_grounding_batch(2, synth.random_boxes(3, g), g)
    x = torch.randn(2, 4, 16, 16, generator=g)
    ctx, uc = torch.randn(2, 77, 768, generator=g), torch.randn(2, 77, 768, generator=g)
    gi = GroundingNetInput()
    return model, x, torch.tensor([700.0, 300.0]), ctx, uc, gi.prepare(gb), gi.get_null_input(batch=2)


_CORNER = dict(qkv_row=False, mlp_min_m=1 << 30, takes=True)
CASES = {
    "defaults": {}, "ln_self_0": dict(ln_self=0), "ln_self_2": dict(ln_self=2), "qkv_row_off": dict(qkv_row=False),
    "mlp_min_m_0": dict(mlp_min_m=0), "mlp_min_m_huge": dict(mlp_min_m=1 << 30), "fuser_off": dict(fuser=False),
    "unpaired": dict(paired=False), "takes": dict(takes=True), "vt_min_n_1024": dict(vt_min_n=1024), "vt_global_off": dict(vt_global=False),
    "stats_buffer_behind_the_duplication": _CORNER, "stats_buffer_behind_the_duplication_fuser_off": dict(_CORNER, fuser=False),
}


@pytest.mark.parametrize("case", list(CASES))
def test_no_handed_reader_gets_statistics_nobody_wrote(case, inputs):
    model, x, t, ctx, uc, grounding, null = inputs
    kn = dict(CASES[case])
    fuser, paired, base = kn.pop("fuser", True), kn.pop("paired", True), (_Takes if kn.pop("takes", False) else EmulOps)
    knobs = dataclasses.replace(EngineKnobs.from_env(), **kn)
    eps = []
    with torch.no_grad():
        for ops in (_poisoning(base), base(torch.float32, batch_invariant=True)):
            eng = UNetEngine(model, ops=ops, use_graphs=False, knobs=knobs)
            if not fuser:
                eng.set_fuser_scale(0.0)
            pair = Cond.cat([eng.prepare_cond(ctx, grounding), eng.prepare_cond(uc, null)])
            ops.eng = eng
            eps.append(eng.forward_cond(torch.cat([x, x]), torch.cat([t, t]), pair, paired=paired))
            ops.eng = None
            if len(eps) == 1:
                assert ops.poisoned >= eng.n_st           # at least the last feed-forward of every block emits nothing
    assert torch.isfinite(eps[0]).all()
    assert torch.equal(eps[0], eps[1])
