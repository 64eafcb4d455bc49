"""DDIMSampler parity on a real MI355X: the HIP engine (hipGraph replay, one batched [cond | uncond] forward per step, the fused
``idf_ddim_update`` / ``idf_q_sample_blend`` launches) against the unmodified reference's DDIM trajectories
(``tests/golden/{tiny,mid}_box_ddim.pt``), the reference's noise draws replayed through ``noise_fn``.

Bar: the trajectory bar of tests/test_samplers_gpu.py (rel-RMS 5e-2 in bf16, 1e-2 in fp16) with the rule for reduced-width goldens:
never below 1.25 x the reference's OWN autocast error on the same trajectory, which the golden stores (``floor``).  Every case prints
a "[parity]" line.
"""
from functools import partial

import pytest
import torch

from tests import ddim_cases

pytestmark = pytest.mark.gpu
TRAJ_TOL = {torch.bfloat16: 5e-2, torch.float16: 1e-2}
FLOOR_KEY = {torch.bfloat16: "bf16", torch.float16: "fp16"}


def _cuda(d):
    return {k: v.cuda() for k, v in d.items()}


def _sampler(tag, dtype):
    from instancediffusion_amd import synth
    from instancediffusion_amd.host.alpha import alpha_generator, set_alpha_scale
    from instancediffusion_amd.host.diffusion import LatentDiffusion
    from instancediffusion_amd.host.samplers import DDIMSampler
    from grounding_input.text_grounding_tokinzer_input import GroundingNetInput
    from tests import cases
    from tests.test_engine_emulated import build_model
    meta = ddim_cases.load(tag)["meta"]
    inp = cases.build_inputs(meta)
    model = build_model(cases.cfg_for(meta["cfg"], meta["variant"]))
    model.compute_dtype = dtype
    model.first_conv_sd_override = synth.synth_first_conv_sd()
    gi = GroundingNetInput()
    model.grounding_tokenizer_input = gi
    diffusion = LatentDiffusion(linear_start=0.00085, linear_end=0.012, timesteps=1000).cuda()
    sampler = DDIMSampler(diffusion, model, alpha_generator_func=partial(alpha_generator, type=meta["alpha_type"]),
                          set_alpha_scale=set_alpha_scale)
    i0 = dict(x=inp["x"].cuda(), timesteps=None, context=inp["context"].cuda(), grounding_input=gi.prepare(_cuda(inp["gb"])))
    return meta, inp, sampler, i0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("tag,name", ddim_cases.ALL_CASES)
def test_ddim_matches_reference(tag, name, dtype):
    from tests import cases
    gold, case, eta, mask, x0, _ = ddim_cases.case_inputs(tag, name)
    meta, inp, sampler, i0 = _sampler(tag, dtype)
    it = iter(ddim_cases.used_noises(case, mask is not None))
    sampler.noise_fn = lambda shape: next(it).cuda()
    out = sampler.sample(meta["S"], tuple(inp["x"].shape), i0, uc=inp["uc"].cuda(), guidance_scale=ddim_cases.GUIDANCE,
                         mask=None if mask is None else mask.cuda(), x0=None if x0 is None else x0.cuda(), eta=eta)
    assert next(it, None) is None, "every recorded draw is used"
    floor = float(case["floor"][FLOOR_KEY[dtype]])
    tol = max(TRAJ_TOL[dtype], 1.25 * floor)
    err = cases.rel_rms(out.cpu(), case["final"])
    print(f"[parity] {tag} DDIM {name} S={meta['S']} CFG7.5 {dtype}: latent rel-rms {err:.3e} (tol {tol:.2e}; the reference's own "
          f"autocast error {floor:.2e})")
    assert torch.isfinite(out).all() and err < tol


def test_default_noise_fn_gives_a_finite_stochastic_trajectory():
    from tests import cases
    outs = {}
    for eta in (0.0, 0.5):
        meta, inp, sampler, i0 = _sampler("tiny_box_ddim", torch.bfloat16)
        torch.manual_seed(11)
        outs[eta] = sampler.sample(meta["S"], tuple(inp["x"].shape), i0, uc=inp["uc"].cuda(), guidance_scale=ddim_cases.GUIDANCE, eta=eta)
        assert torch.isfinite(outs[eta]).all()
    diff = cases.rel_rms(outs[0.5].cpu(), outs[0.0].cpu())
    print(f"[ddim] tiny_box eta 0.5 (default noise_fn) vs eta 0: rel-rms {diff:.3f}")
    assert diff > 1e-2
