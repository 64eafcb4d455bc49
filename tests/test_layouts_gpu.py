"""``PLMSSamplerInst.sample_layouts`` on a real MI355X: four different layouts (N = 0, 1, 3, 2 instances, one with two images) in ONE
call of the HIP engine against the unmodified reference run layout by layout (tests/golden/tiny_box_layouts.pt).

Bar: the rule of tests/test_ddim_sampler_gpu.py -- rel-RMS 5e-2 in bf16, 1e-2 in fp16, never below 1.25 x the reference's OWN autocast
error on the same trajectory, which the golden stores per image.  Every image prints a "[parity]" line.  Also: the batching is real
(the forwards of a heterogeneous batch are the forwards ``sample()`` forms from the same number of units), and the merge is one
``idf_mis_merge_ragged`` call."""
from functools import partial

import pytest
import torch

from tests import layouts_cases as lc

pytestmark = pytest.mark.gpu
TRAJ_TOL = {torch.bfloat16: 5e-2, torch.float16: 1e-2}
FLOOR_KEY = {torch.bfloat16: "bf16", torch.float16: "fp16"}


def _cuda(v):
    if torch.is_tensor(v):
        return v.cuda()
    if isinstance(v, dict):
        return {k: _cuda(x) for k, x in v.items()}
    if isinstance(v, list):
        return [_cuda(x) for x in v]
    return v


def _sampler(dtype):
    from instancediffusion_amd import synth
    from instancediffusion_amd.host.alpha import alpha_generator, set_alpha_scale
    from instancediffusion_amd.host.diffusion import LatentDiffusion
    from instancediffusion_amd.host.samplers import PLMSSamplerInst
    from grounding_input.text_grounding_tokinzer_input import GroundingNetInput
    from tests import cases
    from tests.test_engine_emulated import build_model
    model = build_model(cases.cfg_for(lc.CFG, lc.VARIANT))
    model.compute_dtype = dtype
    model.first_conv_sd_override = synth.synth_first_conv_sd()
    gi = GroundingNetInput()
    model.grounding_tokenizer_input = gi
    diffusion = LatentDiffusion(linear_start=0.00085, linear_end=0.012, timesteps=1000).cuda()
    sampler = PLMSSamplerInst(diffusion, model, alpha_generator_func=partial(alpha_generator, type=list(lc.ALPHA_TYPE)),
                              set_alpha_scale=set_alpha_scale, mis=lc.MIS)
    return sampler, gi, synth


def _layouts(gi, synth, which, images=None):
    """(layouts, uc [L,77,768]) of the case's layouts ``which`` on the device; ``images``: cut every layout to its first images."""
    layouts, ucs = [], []
    for l in which:
        d = _cuda(lc.build_layout(lc.LAYOUTS[l], synth))
        x = d["x"] if images is None else d["x"][:images]
        layouts.append(lc.input_all(d, x, gi.prepare, synth))
        ucs.append(d["uc"])
    return layouts, torch.cat(ucs, 0)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_every_image_of_the_four_layout_batch_matches_its_golden(dtype):
    from tests import cases
    gold = cases.load_golden(lc.TAG)
    sampler, gi, synth = _sampler(dtype)
    layouts, uc = _layouts(gi, synth, range(4))
    out = sampler.sample_layouts(S=lc.S, layouts=layouts, uc=uc, guidance_scale=lc.GUIDANCE).cpu()
    assert torch.isfinite(out).all() and out.shape[0] == sum(s["images"] for s in lc.LAYOUTS)
    g, failed = 0, []
    for l, spec in enumerate(lc.LAYOUTS):
        for k in range(spec["images"]):
            floor = float(gold["floors"][l][k][FLOOR_KEY[dtype]])
            tol = max(TRAJ_TOL[dtype], 1.25 * floor)
            err = cases.rel_rms(out[g], gold["finals"][l][k])
            print(f"[parity] {lc.TAG} layout {l} (N = {spec['n_inst']}) image {k} S={lc.S} CFG7.5 {dtype}: latent rel-rms {err:.3e} "
                  f"(tol {tol:.2e}; the reference's own autocast error {floor:.2e})")
            if not err < tol:
                failed.append((l, k, err, tol))
            g += 1
    assert not failed, failed


def test_a_uniform_layout_list_equals_sample_bit_for_bit():
    """tiny_box (N = 2, two images with their own conditioning) through sample(), and its two rows as two layouts of one image each
    through sample_layouts: the same units in the same forwards, the same kernels, so the same bits."""
    from tests import cases
    sampler, gi, synth = _sampler(torch.bfloat16)
    meta = cases.load_golden("tiny_box")["meta"]
    inp = _cuda(cases.build_inputs(meta))

    def inputs(rows):
        gb = {k: v[rows] for k, v in inp["gb"].items()}
        out = [dict(x=inp["x"][rows].clone(), timesteps=None, context=inp["context"][rows], grounding_input=gi.prepare(gb))]
        for i in range(meta["n_inst"]):
            out.append(dict(x=inp["x"][rows].clone(), timesteps=None, context=inp["inst_ctx"][i][rows],
                            grounding_input=gi.prepare(synth.instance_batch(gb, i))))
        return out
    want = sampler.sample(S=meta["S"], shape=tuple(inp["x"].shape), input=inputs(slice(0, 2)), uc=inp["uc"], guidance_scale=7.5)
    got = sampler.sample_layouts(S=meta["S"], layouts=[inputs(slice(0, 1)), inputs(slice(1, 2))], uc=inp["uc"], guidance_scale=7.5)
    assert torch.isfinite(got).all() and torch.equal(got, want)


def test_the_batching_is_real_and_the_merge_is_one_launch():
    """Layouts with N = (1, 3), one image each: 6 units, 2 images.  They must go through the same number of forwards, with the same
    row widths, as the existing sample() on tiny_box (N = 2, B = 2: also 6 units) -- and not through what two separate calls issue."""
    from tests import cases
    sampler, gi, synth = _sampler(torch.bfloat16)
    eng = sampler.engine
    widths, merges = [], {"ragged": 0, "dense": 0}
    real_fwd, real_ragged, real_dense = eng.forward_cond, eng.ops.mis_merge_ragged, eng.ops.mis_merge

    def fwd(x, t, cond, *a, **k):
        widths.append(int(cond.B))
        return real_fwd(x, t, cond, *a, **k)

    def ragged(*a, **k):
        merges["ragged"] += 1
        return real_ragged(*a, **k)

    def dense(*a, **k):
        merges["dense"] += 1
        return real_dense(*a, **k)
    eng.forward_cond, eng.ops.mis_merge_ragged, eng.ops.mis_merge = fwd, ragged, dense
    try:
        layouts, uc = _layouts(gi, synth, [1, 2], images=1)
        out = sampler.sample_layouts(S=lc.S, layouts=layouts, uc=uc, guidance_scale=lc.GUIDANCE)
        batched, widths[:] = list(widths), []
        assert merges == {"ragged": 1, "dense": 0} and out.shape[0] == 2 and torch.isfinite(out).all()
        # the existing entry point on tiny_box: N = 2, B = 2
        meta = cases.load_golden("tiny_box")["meta"]
        inp = _cuda(cases.build_inputs(meta))
        assert (meta["n_inst"] + 1) * meta["batch"] == 6 and meta["S"] == lc.S and meta["mis"] == lc.MIS
        inputs = [dict(x=inp["x"].clone(), timesteps=None, context=inp["context"], grounding_input=gi.prepare(inp["gb"]))]
        for i in range(meta["n_inst"]):
            inputs.append(dict(x=inp["x"].clone(), timesteps=None, context=inp["inst_ctx"][i],
                               grounding_input=gi.prepare(synth.instance_batch(inp["gb"], i))))
        sampler.sample(S=meta["S"], shape=tuple(inp["x"].shape), input=inputs, uc=inp["uc"], guidance_scale=7.5)
        dense_run, widths[:] = list(widths), []
        # ... and what two separate calls issue for the same two layouts
        for l in (1, 2):
            one, uc1 = _layouts(gi, synth, [l], images=1)
            sampler.sample(S=lc.S, shape=(1, 4, lc.LATENT, lc.LATENT), input=one[0], uc=uc1, guidance_scale=lc.GUIDANCE)
        separate = list(widths)
    finally:
        eng.forward_cond, eng.ops.mis_merge_ragged, eng.ops.mis_merge = real_fwd, real_ragged, real_dense
    print(f"[layouts] forward widths: sample_layouts N=(1,3) {batched}; sample() N=2 B=2 {dense_run}; two separate calls {separate}")
    assert batched == dense_run, "a heterogeneous batch of 6 units forms the forwards of a dense batch of 6 units"
    assert len(separate) > len(batched) and sorted(separate) != sorted(batched)
