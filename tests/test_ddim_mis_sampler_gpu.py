"""``DDIMSamplerInst`` on a real MI355X: the HIP engine (hipGraph replay, wide phase-1 forwards, ``idf_ddim_update_units`` /
``idf_q_sample_blend_units`` through the unit -> image table, ``idf_mis_merge``) on the tiny_box inputs against the composed CPU oracle
``ddim_mis_reference`` (tests/ddim_mis_cases.py), and ``sample_layouts`` on a uniform layout list against ``sample()``, bit for bit.

Bar: exactly the one tests/test_ddim_sampler_gpu.py holds ``DDIMSampler`` to on the same model -- rel-RMS 5e-2 in bf16, 1e-2 in fp16,
never below 1.25 x the reference's own autocast error on the DDIM trajectory of the same name, which ``tiny_box_ddim.pt`` stores.  The
forwards and the step arithmetic are the same, so no new bar is needed.  Every case prints a "[parity]" line.
"""
import functools
from functools import partial

import pytest
import torch

from tests import ddim_cases
from tests import ddim_mis_cases as mc
from tests.test_ddim_sampler_gpu import FLOOR_KEY, TRAJ_TOL

pytestmark = pytest.mark.gpu


def _cuda(d):
    return {k: v.cuda() for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def _case():
    from tests import cases
    meta = cases.load_golden(mc.TAG)["meta"]
    assert (meta["S"], meta["mis"], meta["n_inst"], meta["batch"]) == (mc.S, mc.MIS, 2, 2)
    return meta, cases.build_inputs(meta)


def _sampler(dtype):
    from instancediffusion_amd import synth
    from instancediffusion_amd.host.alpha import alpha_generator, set_alpha_scale
    from instancediffusion_amd.host.diffusion import LatentDiffusion
    from instancediffusion_amd.host.samplers import DDIMSamplerInst
    from grounding_input.text_grounding_tokinzer_input import GroundingNetInput
    from tests import cases
    from tests.test_engine_emulated import build_model
    meta, inp = _case()
    model = build_model(cases.cfg_for(meta["cfg"], meta["variant"]))
    model.compute_dtype = dtype
    model.first_conv_sd_override = synth.synth_first_conv_sd()
    gi = GroundingNetInput()
    model.grounding_tokenizer_input = gi
    diffusion = LatentDiffusion(linear_start=0.00085, linear_end=0.012, timesteps=1000).cuda()
    sampler = DDIMSamplerInst(diffusion, model, alpha_generator_func=partial(alpha_generator, type=meta["alpha_type"]),
                              set_alpha_scale=set_alpha_scale, mis=mc.MIS)
    return sampler, gi


def _inputs(gi, rows=slice(None)):
    from instancediffusion_amd import synth
    meta, inp = _case()
    gb = {k: v[rows] for k, v in inp["gb"].items()}
    out = [dict(x=inp["x"][rows].cuda(), timesteps=None, context=inp["context"][rows].cuda(), grounding_input=gi.prepare(_cuda(gb)))]
    for i in range(meta["n_inst"]):
        out.append(dict(x=inp["x"][rows].cuda(), timesteps=None, context=inp["inst_ctx"][i][rows].cuda(),
                        grounding_input=gi.prepare(_cuda(synth.instance_batch(gb, i)))))
    return out


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(oracle result, mask, x0, noises) of one case: computed once on the CPU, shared by the dtypes, left unchanged."""
    from instancediffusion_amd import synth
    from oracle import ref_cpu
    from tests import cases
    meta, inp = _case()
    eta, masked = mc.CASES[name]
    shape = tuple(inp["x"].shape)
    mask, x0 = mc.make_inpaint(shape) if masked else (None, None)
    noises = mc.make_noises(shape, mc.S, eta, masked)
    cfg = cases.cfg_for(meta["cfg"], meta["variant"])
    with torch.no_grad():
        model = ref_cpu.OracleModel(synth.synth_state_dict(cases.unet_schema(cfg)), cfg, synth.synth_first_conv_sd())
        inputs = [dict(x=inp["x"].clone(), timesteps=None, context=inp["context"], grounding_input=ref_cpu.prepare_grounding(inp["gb"]))]
        for i in range(meta["n_inst"]):
            inputs.append(dict(x=inp["x"].clone(), timesteps=None, context=inp["inst_ctx"][i],
                               grounding_input=ref_cpu.prepare_grounding(synth.instance_batch(inp["gb"], i))))
        want = mc.ddim_mis_reference(model, mc.S, inputs, inp["uc"], mc.GUIDANCE, mc.MIS, eta=eta, alpha_type=meta["alpha_type"],
                                     mask=mask, x0=x0, noises=noises)
    return want, mask, x0, noises


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", list(mc.CASES))
def test_ddim_mis_matches_the_composed_reference(name, dtype):
    from tests import cases
    meta, inp = _case()
    want, mask, x0, noises = _reference(name)
    sampler, gi = _sampler(dtype)
    it = iter(noises)
    sampler.noise_fn = lambda shape: next(it).cuda()
    out = sampler.sample(mc.S, tuple(inp["x"].shape), _inputs(gi), uc=inp["uc"].cuda(), guidance_scale=mc.GUIDANCE,
                         mask=None if mask is None else mask.cuda(), x0=None if x0 is None else x0.cuda(), eta=mc.CASES[name][0])
    assert next(it, None) is None, "every draw is used"
    floor = float(ddim_cases.load("tiny_box_ddim")["cases"][name]["floor"][FLOOR_KEY[dtype]])
    tol = max(TRAJ_TOL[dtype], 1.25 * floor)
    err = cases.rel_rms(out.cpu(), want)
    print(f"[parity] tiny_box DDIM-MIS {name} S={mc.S} mis={mc.MIS} CFG7.5 {dtype}: latent rel-rms {err:.3e} (tol {tol:.2e}; the "
          f"reference's own autocast error on the DDIM trajectory {floor:.2e})")
    assert torch.isfinite(out).all() and err < tol


def test_a_uniform_layout_list_equals_sample():
    """The two rows of tiny_box as one batch-2 ``sample()`` and as two one-image layouts of ``sample_layouts``: the same units in the
    same forwards, eta 0.5 with a mask -- bit for bit (``idf_mis_merge_ragged`` with equal counts is ``idf_mis_merge``)."""
    meta, inp = _case()
    _, mask, x0, noises = _reference("eta0.5_mask")
    outs = []
    for layouts in (False, True):
        sampler, gi = _sampler(torch.bfloat16)
        it = iter(noises)
        sampler.noise_fn = lambda shape: next(it).cuda()
        if layouts:
            outs.append(sampler.sample_layouts(mc.S, [_inputs(gi, slice(0, 1)), _inputs(gi, slice(1, 2))], uc=inp["uc"].cuda(),
                                               guidance_scale=mc.GUIDANCE, eta=0.5, masks=[mask[0:1].cuda(), mask[1:2].cuda()],
                                               x0s=[x0[0:1].cuda(), x0[1:2].cuda()]))
        else:
            outs.append(sampler.sample(mc.S, tuple(inp["x"].shape), _inputs(gi), uc=inp["uc"].cuda(), guidance_scale=mc.GUIDANCE,
                                       mask=mask.cuda(), x0=x0.cuda(), eta=0.5))
        assert next(it, None) is None
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
