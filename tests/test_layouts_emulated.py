"""``PLMSSamplerInst.sample_layouts`` host logic (no GPU), over the CPU op emulation: four different layouts (N = 0, 1, 3, 2 instances,
one with two images) in ONE call against the unmodified reference run layout by layout (tests/golden/tiny_box_layouts.pt), against
the existing ``sample()`` on every layout alone, under a permutation of the list, and on a uniform list against ``sample()`` itself;
the refusals, the input builder and the CLI's argument errors."""
import json
import os
import sys
from functools import partial

import pytest
import torch

from instancediffusion_amd import synth
from instancediffusion_amd.engine import UNetEngine
from instancediffusion_amd.host.alpha import alpha_generator, set_alpha_scale
from instancediffusion_amd.host.diffusion import LatentDiffusion
from instancediffusion_amd.host.samplers import PLMSSamplerInst
from grounding_input.text_grounding_tokinzer_input import GroundingNetInput
from tests import cases
from tests import layouts_cases as lc
from tests.emul_ops_layouts import EmulOpsLayouts
from tests.test_engine_emulated import build_model

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL_TRAJ_TOL = 5e-3                      # the bar of tests/test_samplers_emulated.py
_ENV = {}


def env(batch_invariant):
    """(model with an emulated engine, GroundingNetInput, diffusion), built once per flavour of the op emulation."""
    if batch_invariant not in _ENV:
        model = build_model(cases.cfg_for(lc.CFG, lc.VARIANT))
        model._engine = UNetEngine(model, ops=EmulOpsLayouts(torch.float32, batch_invariant=batch_invariant), use_graphs=False)
        model.first_conv_sd_override = synth.synth_first_conv_sd()
        gi = GroundingNetInput()
        model.grounding_tokenizer_input = gi
        _ENV[batch_invariant] = (model, gi, LatentDiffusion(linear_start=0.00085, linear_end=0.012, timesteps=1000))
    return _ENV[batch_invariant]


def sampler_for(batch_invariant, alpha_type=lc.ALPHA_TYPE, **kw):
    model, gi, diffusion = env(batch_invariant)
    return PLMSSamplerInst(diffusion, model, alpha_generator_func=partial(alpha_generator, type=list(alpha_type)),
                           set_alpha_scale=set_alpha_scale, mis=lc.MIS, **kw), gi


@pytest.fixture(scope="module")
def datas():
    return [lc.build_layout(spec, synth) for spec in lc.LAYOUTS]


def layouts_of(datas, gi, order=None):
    order = range(len(datas)) if order is None else order
    return [lc.input_all(datas[l], datas[l]["x"], gi.prepare, synth) for l in order], torch.cat([datas[l]["uc"] for l in order], 0)


def blocks(out, datas, order=None):
    """sample_layouts' output split into one [K_l, 4, H, W] block per layout of the list."""
    order = range(len(datas)) if order is None else order
    res, k = [], 0
    for l in order:
        n = datas[l]["x"].shape[0]
        res.append(out[k:k + n])
        k += n
    assert k == out.shape[0]
    return res


@pytest.fixture(scope="module")
def batched(datas):
    """The four-layout batch through sample_layouts, once (plain op emulation); shared, left unchanged."""
    sampler, gi = sampler_for(False)
    layouts, uc = layouts_of(datas, gi)
    calls = dict(sampler.engine.ops.calls)
    out = sampler.sample_layouts(S=lc.S, layouts=layouts, uc=uc, guidance_scale=lc.GUIDANCE)
    assert sampler.engine.ops.calls.get("mis_merge_ragged", 0) - calls.get("mis_merge_ragged", 0) == 1
    return blocks(out, datas)


def alone(sampler, gi, data, k):
    """Image k of one layout through the EXISTING entry point, at batch 1."""
    x = data["x"][k:k + 1]
    return sampler.sample(S=lc.S, shape=tuple(x.shape), input=lc.input_all(data, x, gi.prepare, synth), uc=data["uc"],
                          guidance_scale=lc.GUIDANCE)


def test_every_image_matches_its_reference_golden(batched, datas):
    gold = cases.load_golden(lc.TAG)
    assert [s["n_inst"] for s in gold["meta"]["layouts"]] == [0, 1, 3, 2] and [s["images"] for s in gold["meta"]["layouts"]] == [1, 1, 2, 1]
    for l, got in enumerate(batched):
        for k in range(got.shape[0]):
            err = cases.rel_rms(got[k], gold["finals"][l][k])
            print(f"[parity] layout {l} (N = {lc.LAYOUTS[l]['n_inst']}) image {k}: rel-RMS {err:.3e} against the reference, bar {EMUL_TRAJ_TOL:.0e}")
            assert err < EMUL_TRAJ_TOL, (l, k, err)


@pytest.fixture(scope="module")
def shape_bar(datas):
    """The only difference between the batched call and a layout alone is the batch-shape dependence of the CPU's fp32 GEMMs.  Its
    size is measured on existing code -- one layout at batch 1 against the same layout as two identical rows of a batch-2 ``sample()``
    -- and the batched call gets 4 x that figure, never less than 1e-6 rel-RMS.  -> (bar, the batch-1 result of layout 3)."""
    sampler, gi = sampler_for(False)
    d = datas[3]

    def rep(v):
        return v.repeat(2, *([1] * (v.dim() - 1)))
    one = alone(sampler, gi, d, 0)
    d2 = dict(x=rep(d["x"][:1]), context=rep(d["context"]), uc=rep(d["uc"]), gb={k: rep(v) for k, v in d["gb"].items()},
              inst_ctx=[rep(c) for c in d["inst_ctx"]])
    two = sampler.sample(S=lc.S, shape=tuple(d2["x"].shape), input=lc.input_all(d2, d2["x"], gi.prepare, synth), uc=d2["uc"],
                         guidance_scale=lc.GUIDANCE)
    shape_dep = cases.rel_rms(two[:1], one)
    bar = max(4 * shape_dep, 1e-6)
    print(f"[layouts] batch-shape dependence of the emulation (batch 1 against two rows of batch 2): {shape_dep:.3e} -> bar {bar:.3e}")
    return bar, one


def test_every_image_matches_the_layout_run_alone_through_sample(batched, datas, shape_bar):
    sampler, gi = sampler_for(False)
    bar, one = shape_bar
    worst = 0.0
    for l, got in enumerate(batched):
        for k in range(got.shape[0]):
            err = cases.rel_rms(got[k:k + 1], one if (l, k) == (3, 0) else alone(sampler, gi, datas[l], k))
            worst = max(worst, err)
            print(f"[layouts] layout {l} image {k}: rel-RMS {err:.3e} against sample() on the layout alone")
            assert err <= bar, (l, k, err, bar)
    print(f"[layouts] worst {worst:.3e}, bar {bar:.3e}")


def test_crop_and_paste_matches_the_layout_run_alone(datas, shape_bar):
    """Merge mode 1 through the ragged path (per-unit boxes, global entries ignored) against sample() with crop_and_paste_latents,
    at the same bar."""
    sampler, gi = sampler_for(False, crop_and_paste_latents=True)
    order = [1, 3]
    layouts, uc = layouts_of(datas, gi, order)
    out = blocks(sampler.sample_layouts(S=lc.S, layouts=layouts, uc=uc, guidance_scale=lc.GUIDANCE), datas, order)
    for got, l in zip(out, order):
        err = cases.rel_rms(got, alone(sampler, gi, datas[l], 0))
        print(f"[layouts] crop-and-paste, layout {l}: rel-RMS {err:.3e} against sample() on the layout alone, bar {shape_bar[0]:.3e}")
        assert err <= shape_bar[0], (l, err)


WORKER_THREADS = 2           # torch's CPU kernels reduce in a thread-count-dependent order: compare like with like, as
                             # tests/test_samplers_emulated.py does for its bit-for-bit world-size comparisons


@pytest.fixture
def two_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(WORKER_THREADS)
    yield
    torch.set_num_threads(n)


def test_permuting_the_layouts_permutes_the_outputs(datas, two_threads):
    sampler, gi = sampler_for(True)
    outs = {}
    for order in ([0, 1, 2, 3], [2, 0, 3, 1]):
        layouts, uc = layouts_of(datas, gi, order)
        out = sampler.sample_layouts(S=lc.S, layouts=layouts, uc=uc, guidance_scale=lc.GUIDANCE)
        outs[tuple(order)] = dict(zip(order, blocks(out, datas, order)))
    a, b = outs[(0, 1, 2, 3)], outs[(2, 0, 3, 1)]
    for l in range(4):
        assert torch.equal(a[l], b[l]), l


def test_a_uniform_layout_list_equals_sample(two_threads):
    """tiny_box (N = 2, two images with their own conditioning): sample() on the batch-2 inputs against sample_layouts on the two
    rows as two layouts of one image each -- the same units in the same forwards, bit for bit (batch-invariant emulation)."""
    sampler, gi = sampler_for(True)
    meta = cases.load_golden("tiny_box")["meta"]
    inp = cases.build_inputs(meta)
    assert meta["mis"] == lc.MIS and meta["S"] == lc.S and meta["alpha_type"] == lc.ALPHA_TYPE

    def inputs(rows):
        def cut(v):
            return v[rows]
        gb = {k: cut(v) for k, v in inp["gb"].items()}
        out = [dict(x=cut(inp["x"]).clone(), timesteps=None, context=cut(inp["context"]), grounding_input=gi.prepare(gb))]
        for i in range(meta["n_inst"]):
            out.append(dict(x=cut(inp["x"]).clone(), timesteps=None, context=cut(inp["inst_ctx"][i]),
                            grounding_input=gi.prepare(synth.instance_batch(gb, i))))
        return out
    want = sampler.sample(S=meta["S"], shape=tuple(inp["x"].shape), input=inputs(slice(0, 2)), uc=inp["uc"], guidance_scale=7.5)
    got = sampler.sample_layouts(S=meta["S"], layouts=[inputs(slice(0, 1)), inputs(slice(1, 2))], uc=inp["uc"], guidance_scale=7.5)
    assert torch.equal(got, want)
    assert cases.rel_rms(got, cases.load_golden("tiny_box")["mis"]) < EMUL_TRAJ_TOL


def test_refusals(datas, monkeypatch):
    sampler, gi = sampler_for(True)
    layouts, uc = layouts_of(datas, gi)
    with monkeypatch.context() as m:                                      # a model built for masked gated self-attention
        m.setattr(sampler.engine, "masked_fuser", True)
        with pytest.raises(ValueError, match="masked gated self-attention"):
            sampler.sample_layouts(S=lc.S, layouts=layouts, uc=uc, guidance_scale=lc.GUIDANCE)
    early, _ = sampler_for(True, alpha_type=[0.2, 0.0, 0.8])              # S = 5: alphas [1, 0, 0, 0, 0], phase 1 = steps 0, 1
    with pytest.raises(ValueError, match="reaches 0 inside phase 1"):
        early.sample_layouts(S=lc.S, layouts=layouts, uc=uc, guidance_scale=lc.GUIDANCE)
    paste, _ = sampler_for(True, crop_and_paste_latents=True)             # layout 0 has no instance
    with pytest.raises(ValueError, match="crop_and_paste_latents"):
        paste.sample_layouts(S=lc.S, layouts=layouts, uc=uc, guidance_scale=lc.GUIDANCE)
    with pytest.raises(ValueError, match="uc has 3 rows"):
        sampler.sample_layouts(S=lc.S, layouts=layouts, uc=uc[:3], guidance_scale=lc.GUIDANCE)
    with pytest.raises(ValueError):
        sampler.sample_layouts(S=lc.S, layouts=[], uc=uc, guidance_scale=lc.GUIDANCE)


def test_the_shim_mirrors_the_entry_point():
    from ldm.models.diffusion.plms_instance import PLMSSamplerInst as Shim
    assert Shim.sample_layouts is PLMSSamplerInst.sample_layouts


# ---- input builder and CLI -------------------------------------------------------------------------------------------
DEMOS = [os.path.join(REPO, "demos", n) for n in ("demo_four_boxes.json", "demo_points.json", "demo_scribbles.json")]


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_input_builder_rows_equal_prepare_batch_on_the_layout_alone():
    import inference
    from instancediffusion_amd.host.input import meta_from_demo_json, prepare_batch, prepare_instance_meta, prepare_layout_inputs
    enc, gi = inference.SyntheticTextEncoder(), GroundingNetInput()
    metas = [meta_from_demo_json(json.load(open(p)), 0.75) for p in DEMOS]
    K = [1, 2, 1]
    noises = [torch.randn(k, 4, 64, 64, generator=torch.Generator().manual_seed(5 + k)) for k in K]

    def batch(meta, b):
        return gi.prepare(prepare_batch(meta, batch=b, max_objs=30, model=enc, processor=None, image_size=64, device="cpu"))
    # Multi-instance Sampler form: per layout [global, instance 1, ..], conditioning at batch 1, x shared
    layouts = prepare_layout_inputs(metas, noises, gi, enc, enc, instances=True, device="cpu")
    assert [len(lay) for lay in layouts] == [1 + len(m["phrases"]) for m in metas]
    planes = set()
    for meta, x, lay in zip(metas, noises, layouts):
        for j, inp in enumerate(lay):
            m = meta if j == 0 else prepare_instance_meta(meta, j - 1)
            _same(inp["grounding_input"], batch(m, 1))
            assert inp["x"] is x and torch.equal(inp["context"], enc.encode([m["prompt"]]))
            planes.add(inp["grounding_input"]["segs"].data_ptr())
    assert len(planes) == 1, "every all-zero mask stack of the call is the same zero plane set"
    # mis == 0 form: one row-stacked input
    inp = prepare_layout_inputs(metas, noises, gi, enc, enc, instances=False, device="cpu")
    assert torch.equal(inp["x"], torch.cat(noises, 0)) and inp["context"].shape == (4, 77, 768)
    g, k0 = inp["grounding_input"], 0
    assert g["segs"].shape == (4, 30, 512, 512) and g["segs"].stride(0) == 0, "zero segs stay a stride-0 view"
    for meta, k in zip(metas, K):
        want = batch(meta, k)
        for key in want:
            assert torch.equal(g[key][k0:k0 + k], want[key]), key
        assert torch.equal(inp["context"][k0:k0 + k], enc.encode([meta["prompt"]] * k))
        k0 += k
    # a real mask stack is kept, and then the rows are stacked for real
    metas[1]["segs"][0, 10:20, 10:20] = 1.0
    g = prepare_layout_inputs(metas, noises, gi, enc, enc, instances=False, device="cpu")["grounding_input"]
    assert g["segs"].stride(0) != 0 and float(g["segs"][1].sum()) == 100.0 and float(g["segs"][0].sum()) == 0.0 == float(g["segs"][3].sum())


def test_cli_argument_errors(monkeypatch):
    import inference
    assert inference.layout_folders(["a/x.json", "b/y.json", "c/x.json", "x.json"]) == ["x", "y", "x_2", "x_3"]

    def run(*argv):
        monkeypatch.setattr(sys, "argv", ["inference.py", "--synthetic_weights", "--input_json", DEMOS[0], DEMOS[1], *argv])
        with pytest.raises(SystemExit) as e:
            inference.main()
        return str(e.value)
    assert "takes one --input_json" in run("--use_masked_att")
    assert "takes one --input_json" in run("--init_image", "a.png", "--inpaint_mask", "m.png", "--mis", "0")
    assert "--keep_best K needs --clip_score" in run("--keep_best", "1")
