"""``DPMSolverSampler`` and ``DPMSolverSamplerInst`` on a real MI355X: the HIP engine (hipGraph replay, one batched [cond | uncond]
forward per step, one ``idf_dpmpp_update`` launch behind it; under the Multi-instance Sampler the wide phase-1 forwards and
``idf_mis_merge``) on the tiny_box inputs at S = 5, CFG 7.5, against the composed CPU oracles of tests/dpmpp_cases.py; and
``sample_layouts`` on a uniform layout list against ``sample()``, bit for bit.

Bar: the rule of tests/test_ddim_sampler_gpu.py, ``max(TRAJ_TOL[dtype], 1.25 x floor)``.  The second-order step weights two x0
predictions by |c_0| + |c_1| > Bc, so the forward's rounding error is amplified beyond DDIM's and DDIM's stored floor does not apply:
``floor`` is the oracle's OWN autocast error on the SAME trajectory (``dpmpp_reference`` / ``dpmpp_mis_reference`` under bf16 / fp16
autocast against fp32), stored in tests/golden/dpmpp_floor.pt by tests/make_dpmpp_golden.py.  Every case prints a "[parity]" line.
"""
import functools
import os
from functools import partial

import pytest
import torch

from tests import dpmpp_cases as dc
from tests.test_ddim_sampler_gpu import FLOOR_KEY, TRAJ_TOL

pytestmark = pytest.mark.gpu


def _cuda(d):
    return {k: v.cuda() for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def _case():
    from tests import cases
    meta = cases.load_golden(dc.TAG)["meta"]
    assert (meta["S"], meta["mis"], meta["n_inst"], meta["batch"]) == (dc.S, dc.MIS, 2, 2)
    return meta, cases.build_inputs(meta)


@functools.lru_cache(maxsize=None)
def _floors():
    gold = torch.load(os.path.join(dc.GOLD, dc.FLOOR_GOLDEN), weights_only=False)
    assert (gold["meta"]["tag"], gold["meta"]["S"], gold["meta"]["mis"], gold["meta"]["guidance"]) == (dc.TAG, dc.S, dc.MIS, dc.GUIDANCE)
    return gold["floors"]


def _sampler(kind, dtype):
    from instancediffusion_amd import synth
    from instancediffusion_amd.host.alpha import alpha_generator, set_alpha_scale
    from instancediffusion_amd.host.diffusion import LatentDiffusion
    from instancediffusion_amd.host.samplers import DPMSolverSampler, DPMSolverSamplerInst
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
    kw = dict(alpha_generator_func=partial(alpha_generator, type=meta["alpha_type"]), set_alpha_scale=set_alpha_scale)
    sampler = DPMSolverSamplerInst(diffusion, model, mis=dc.MIS, **kw) if kind == "mis" else DPMSolverSampler(diffusion, model, **kw)
    return sampler, gi


def _inputs(gi, rows=slice(None), instances=True):
    from instancediffusion_amd import synth
    meta, inp = _case()
    gb = {k: v[rows] for k, v in inp["gb"].items()}
    out = [dict(x=inp["x"][rows].cuda(), timesteps=None, context=inp["context"][rows].cuda(), grounding_input=gi.prepare(_cuda(gb)))]
    for i in range(meta["n_inst"] if instances else 0):
        out.append(dict(x=inp["x"][rows].cuda(), timesteps=None, context=inp["inst_ctx"][i][rows].cuda(),
                        grounding_input=gi.prepare(_cuda(synth.instance_batch(gb, i)))))
    return out


@functools.lru_cache(maxsize=None)
def _reference(kind, order):
    """The oracle's result: computed once on the CPU, shared by the dtypes, left unchanged."""
    from instancediffusion_amd import synth
    from oracle import ref_cpu
    from tests import cases
    meta, inp = _case()
    cfg = cases.cfg_for(meta["cfg"], meta["variant"])
    with torch.no_grad():
        model = ref_cpu.OracleModel(synth.synth_state_dict(cases.unet_schema(cfg)), cfg, synth.synth_first_conv_sd())
        inputs = [dict(x=inp["x"].clone(), timesteps=None, context=inp["context"], grounding_input=ref_cpu.prepare_grounding(inp["gb"]))]
        if kind == "plain":
            return dc.dpmpp_reference(model, dc.S, inputs[0], inp["uc"], dc.GUIDANCE, order=order, alpha_type=meta["alpha_type"])
        for i in range(meta["n_inst"]):
            inputs.append(dict(x=inp["x"].clone(), timesteps=None, context=inp["inst_ctx"][i],
                               grounding_input=ref_cpu.prepare_grounding(synth.instance_batch(inp["gb"], i))))
        return dc.dpmpp_mis_reference(model, dc.S, inputs, inp["uc"], dc.GUIDANCE, dc.MIS, order=order, alpha_type=meta["alpha_type"])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("order", [1, 2], ids=["order1", "order2"])
@pytest.mark.parametrize("kind", ["plain", "mis"])
def test_dpmpp_matches_the_composed_reference(kind, order, dtype):
    from tests import cases
    meta, inp = _case()
    want = _reference(kind, order)
    sampler, gi = _sampler(kind, dtype)

    def no_noise(shape):
        raise AssertionError("a DPM-Solver++ run without a mask draws no noise")
    sampler.noise_fn = no_noise
    inputs = _inputs(gi, instances=kind == "mis")
    out = sampler.sample(dc.S, tuple(inp["x"].shape), inputs if kind == "mis" else inputs[0], uc=inp["uc"].cuda(),
                         guidance_scale=dc.GUIDANCE, order=order)
    floor = float(_floors()[kind][order][FLOOR_KEY[dtype]])
    tol = max(TRAJ_TOL[dtype], 1.25 * floor)
    err = cases.rel_rms(out.cpu(), want)
    print(f"[parity] tiny_box DPM-Solver++ {kind} order {order} S={dc.S} CFG7.5 {dtype}: latent rel-rms {err:.3e} (tol {tol:.2e}; the "
          f"oracle's own autocast error on this trajectory {floor:.2e})")
    assert torch.isfinite(out).all() and err < tol


def test_a_uniform_layout_list_equals_sample():
    """The two rows of tiny_box as one batch-2 ``sample()`` and as two one-image layouts of ``sample_layouts``: the same units in the
    same forwards, order 2 -- bit for bit (``idf_mis_merge_ragged`` with equal counts is ``idf_mis_merge``)."""
    meta, inp = _case()
    outs = []
    for layouts in (False, True):
        sampler, gi = _sampler("mis", torch.bfloat16)
        if layouts:
            outs.append(sampler.sample_layouts(dc.S, [_inputs(gi, slice(0, 1)), _inputs(gi, slice(1, 2))], uc=inp["uc"].cuda(),
                                               guidance_scale=dc.GUIDANCE, order=2))
        else:
            outs.append(sampler.sample(dc.S, tuple(inp["x"].shape), _inputs(gi), uc=inp["uc"].cuda(), guidance_scale=dc.GUIDANCE, order=2))
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
