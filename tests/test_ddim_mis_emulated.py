"""``DDIMSamplerInst`` (the Multi-instance Sampler on DDIM steps) host logic without a GPU, over the CPU op emulation
(tests/emul_ops_ddim_mis.py): exact degenerate cases against ``DDIMSampler``, the tiny_box case against the composed oracle
(tests/ddim_mis_cases.py), independence of chunking and of the world size, the noise rule, masks, ``sample_layouts``, the CLI and the
C ABI of the two unit kernels.

Bit-for-bit comparisons between runs that form different forwards use the batch-invariant emulation at a fixed thread count, as
tests/test_samplers_emulated.py and tests/test_layouts_emulated.py do.
"""
import os
import sys
from functools import partial

import numpy as np
import pytest
import torch

from instancediffusion_amd import synth
from instancediffusion_amd.engine import UNetEngine
from instancediffusion_amd.host.alpha import alpha_generator, set_alpha_scale
from instancediffusion_amd.host.diffusion import LatentDiffusion
from instancediffusion_amd.host.samplers import DDIMSampler, DDIMSamplerInst, PLMSSamplerInst
from grounding_input.text_grounding_tokinzer_input import GroundingNetInput
from oracle import ref_cpu
from tests import cases, ddim_cases
from tests import ddim_mis_cases as mc
from tests import layouts_cases as lc
from tests.emul_ops_ddim_mis import EmulOpsDDIMMis
from tests.test_engine_emulated import build_model

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL_TRAJ_TOL = 5e-3            # the bar of tests/test_samplers_emulated.py
WORKER_THREADS = 2              # torch's CPU kernels reduce in a thread-count-dependent order: compare like with like
_ENV = {}
_GI = GroundingNetInput()       # one for both emulation flavours: inputs prepared through it serve either model


class CountingOps(EmulOpsDDIMMis):
    def mis_merge(self, lat, boxes_i32, out, mode):
        self._count("mis_merge")
        return super().mis_merge(lat, boxes_i32, out, mode)


def env(batch_invariant=True):
    """(meta, inputs of tiny_box, model over the emulated engine, GroundingNetInput, diffusion), once per emulation flavour."""
    if batch_invariant not in _ENV:
        meta = cases.load_golden(mc.TAG)["meta"]
        assert (meta["S"], meta["mis"], meta["n_inst"], meta["batch"]) == (mc.S, mc.MIS, 2, 2)
        model = build_model(cases.cfg_for(meta["cfg"], meta["variant"]))
        model._engine = UNetEngine(model, ops=CountingOps(torch.float32, batch_invariant=batch_invariant), use_graphs=False)
        model.first_conv_sd_override = synth.synth_first_conv_sd()
        model.grounding_tokenizer_input = _GI
        _ENV[batch_invariant] = (meta, cases.build_inputs(meta), model, _GI,
                                 LatentDiffusion(linear_start=0.00085, linear_end=0.012, timesteps=1000))
    return _ENV[batch_invariant]


def sampler_for(cls=DDIMSamplerInst, batch_invariant=True, mis=mc.MIS, alpha_type=None, **kw):
    meta, inp, model, gi, diffusion = env(batch_invariant)
    extra = dict(mis=mis, **kw) if cls is not DDIMSampler else {}
    return cls(diffusion, model, alpha_generator_func=partial(alpha_generator, type=list(alpha_type or meta["alpha_type"])),
               set_alpha_scale=set_alpha_scale, **extra)


def mis_inputs(rows=slice(None), instances=True):
    meta, inp, model, gi, _ = env()
    gb = {k: v[rows] for k, v in inp["gb"].items()}
    out = [dict(x=inp["x"][rows].clone(), timesteps=None, context=inp["context"][rows], grounding_input=gi.prepare(gb))]
    for i in range(meta["n_inst"] if instances else 0):
        out.append(dict(x=inp["x"][rows].clone(), timesteps=None, context=inp["inst_ctx"][i][rows],
                        grounding_input=gi.prepare(synth.instance_batch(gb, i))))
    return out


def run(sampler, eta, masked, noises=None, inputs=None, mask=None, x0=None, counts=None):
    """One ``sample()`` on tiny_box with the draws replayed; -> (result, number of draws made)."""
    meta, inp, _, _, _ = env()
    shape = tuple(inp["x"].shape)
    if masked and mask is None:
        mask, x0 = mc.make_inpaint(shape)
    drawn = mc.replay(sampler, noises if noises is not None else mc.make_noises(shape, mc.S, eta, masked))
    calls = sampler.engine.ops.calls
    before = dict(calls)
    kw = dict(mask=mask, x0=x0) if masked else {}
    out = sampler.sample(mc.S, shape, inputs if inputs is not None else mis_inputs(), uc=inp["uc"], guidance_scale=mc.GUIDANCE, eta=eta, **kw)
    if counts is not None:
        counts.update({k: v - before.get(k, 0) for k, v in calls.items() if v != before.get(k, 0)})
    return out, len(drawn)


@pytest.fixture
def two_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(WORKER_THREADS)
    yield
    torch.set_num_threads(n)


ETA_MASK = [(0.0, False), (0.5, False), (0.5, True)]
IDS = ["eta0", "eta0.5", "eta0.5_mask"]


# ---- 1, 2: the exact degenerate cases -------------------------------------------------------------------------------------
@pytest.mark.parametrize("eta,masked", ETA_MASK, ids=IDS)
@pytest.mark.parametrize("mis", [0.0, 0.19], ids=["mis0", "int(S*mis)==0"])
def test_without_a_phase_one_step_it_is_ddim_on_the_global_input(mis, eta, masked, two_threads):
    assert int(mc.S * mis) == 0
    want, n_want = run(sampler_for(DDIMSampler), eta, masked, inputs=mis_inputs(instances=False)[0])
    got, n_got = run(sampler_for(mis=mis), eta, masked)
    assert n_got == n_want == mc.n_draws(mc.S, eta, masked)
    assert torch.equal(got, want)


@pytest.mark.parametrize("eta,masked", ETA_MASK, ids=IDS)
def test_a_layout_without_instances_is_ddim(eta, masked, two_threads):
    want, n_want = run(sampler_for(DDIMSampler), eta, masked, inputs=mis_inputs(instances=False)[0])
    counts = {}
    got, n_got = run(sampler_for(), eta, masked, inputs=mis_inputs(instances=False), counts=counts)
    assert n_got == n_want and torch.equal(got, want)                          # the mean of one unit
    assert counts.get("mis_merge") == 1


# ---- 3: against the composed oracle -----------------------------------------------------------------------------------------
@pytest.fixture
def oracle():
    """A fresh ``OracleModel`` per test: it caches the UniFusion tokens under ``id(grounding dict)`` without holding the dict, so a
    model that outlives the input dicts of one run can hand a later run's dict (at a reused address) another input's tokens."""
    meta, inp, _, _, _ = env()
    cfg = cases.cfg_for(meta["cfg"], meta["variant"])
    model = ref_cpu.OracleModel(synth.synth_state_dict(cases.unet_schema(cfg)), cfg, synth.synth_first_conv_sd())

    def inputs():
        out = [dict(x=inp["x"].clone(), timesteps=None, context=inp["context"], grounding_input=ref_cpu.prepare_grounding(inp["gb"]))]
        for i in range(meta["n_inst"]):
            out.append(dict(x=inp["x"].clone(), timesteps=None, context=inp["inst_ctx"][i],
                            grounding_input=ref_cpu.prepare_grounding(synth.instance_batch(inp["gb"], i))))
        return out
    return model, inputs


@pytest.mark.parametrize("eta,masked", ETA_MASK, ids=IDS)
def test_tiny_box_matches_the_composed_reference(oracle, eta, masked):
    meta, inp, _, _, _ = env(False)
    shape = tuple(inp["x"].shape)
    mask, x0 = mc.make_inpaint(shape) if masked else (None, None)
    noises = mc.make_noises(shape, mc.S, eta, masked)
    model, inputs = oracle
    with torch.no_grad():
        want = mc.ddim_mis_reference(model, mc.S, inputs(), inp["uc"], mc.GUIDANCE, mc.MIS, eta=eta, alpha_type=meta["alpha_type"],
                                     mask=mask, x0=x0, noises=noises)
    counts = {}
    got, n = run(sampler_for(batch_invariant=False), eta, masked, noises=noises, counts=counts)
    err = cases.rel_rms(got, want)
    print(f"[emulated] tiny_box DDIM-MIS eta {eta} mask {masked}: rel-rms {err:.3e} against ddim_mis_reference (bar {EMUL_TRAJ_TOL:.0e})")
    assert n == len(noises) and torch.isfinite(got).all() and err < EMUL_TRAJ_TOL
    mis_step = int(mc.S * mc.MIS)                                               # 6 units = one forward per phase-1 step
    assert counts.get("ddim_update_units", 0) == mis_step and counts.get("ddim_update", 0) == mc.S - mis_step
    assert counts.get("ddim_update_units", 0) + counts.get("ddim_update", 0) == mc.S
    assert counts.get("q_sample_blend_units", 0) == (mis_step if masked else 0)
    assert counts.get("q_sample_blend", 0) == ((mc.S - mis_step) + 1 if masked else 0)   # phase 2, + the hoisted evaluation's input
    assert counts.get("mis_merge") == 1 and "mis_merge_ragged" not in counts and "cfg_combine" not in counts


def test_crop_and_paste_merge_matches_the_composed_reference(oracle):
    meta, inp, _, _, _ = env(False)
    noises = mc.make_noises(tuple(inp["x"].shape), mc.S, 0.5, False)
    model, inputs = oracle
    with torch.no_grad():
        want = mc.ddim_mis_reference(model, mc.S, inputs(), inp["uc"], mc.GUIDANCE, mc.MIS, eta=0.5, alpha_type=meta["alpha_type"],
                                     noises=noises, crop_and_paste=True)
    got, _ = run(sampler_for(batch_invariant=False, crop_and_paste_latents=True), 0.5, False, noises=noises)
    err = cases.rel_rms(got, want)
    print(f"[emulated] tiny_box DDIM-MIS eta 0.5, crop-and-paste merge: rel-rms {err:.3e} against ddim_mis_reference")
    assert err < EMUL_TRAJ_TOL


# ---- 4: chunking -------------------------------------------------------------------------------------------------------------
def test_result_does_not_depend_on_chunking(two_threads):
    """One unit per forward against all six in one: fails if noise is drawn per chunk (or per unit)."""
    counts = {}
    one, n_one = run(sampler_for(max_units=1), 0.5, True, counts=counts)
    assert counts["ddim_update_units"] == 6 * int(mc.S * mc.MIS)
    full, n_full = run(sampler_for(), 0.5, True)
    assert n_one == n_full == mc.n_draws(mc.S, 0.5, True)
    assert torch.equal(one, full)


def test_alpha_zero_inside_phase_one_takes_the_serial_order(two_threads, monkeypatch):
    """alpha_type [0.2, 0, 0.8] at S = 5: alphas [1, 0, 0, 0, 0], so phase 1 (steps 0, 1) swaps the first conv: one instance at a
    time, as ``PLMSSamplerInst.sample`` -- and still the same draws.  (The swap itself is stubbed: it hard-codes 320 channels, the
    reduced-width model has 64.)"""
    counts, swaps = {}, []
    monkeypatch.setattr(env()[2], "restore_first_conv_from_SD", lambda: swaps.append(1))
    out, n = run(sampler_for(alpha_type=[0.2, 0.0, 0.8]), 0.5, False, counts=counts)
    assert swaps
    assert torch.isfinite(out).all() and n == mc.S
    # three chunks (global, instance 1, instance 2) of one unit per image, in image order: no table needed
    mis_step = int(mc.S * mc.MIS)
    assert counts["ddim_update"] == 3 * mis_step + (mc.S - mis_step) and "ddim_update_units" not in counts


# ---- 5: masks ------------------------------------------------------------------------------------------------------------------
def test_an_all_zero_mask_changes_nothing(two_threads):
    meta, inp, _, _, _ = env()
    shape = tuple(inp["x"].shape)
    noises = mc.make_noises(shape, mc.S, 0.5, True)                             # q_sample draw, step draw, q_sample draw, ..
    _, x0 = mc.make_inpaint(shape)
    masked, _ = run(sampler_for(), 0.5, True, noises=noises, mask=torch.zeros(shape[0], 1, *shape[2:]), x0=x0)
    plain, _ = run(sampler_for(), 0.5, False, noises=noises[1::2])
    assert torch.equal(masked, plain)


def test_kept_region_is_shared_by_every_trajectory_of_an_image(two_threads):
    """In front of every phase-1 step the trajectories of an image are equal inside the kept region (they hold q_sample(x0, t) with
    the image's one draw there), whatever their conditioning did in the step before; with a mask of all ones nothing of phase 1
    survives the first blend of phase 2, so the result is ``DDIMSampler``'s with the draws of phase 2."""
    meta, inp, _, _, _ = env()
    shape = tuple(inp["x"].shape)
    mask, x0 = mc.make_inpaint(shape)
    sampler = sampler_for()
    ops, seen = sampler.engine.ops, []
    real = ops.q_sample_blend_units
    ops.q_sample_blend_units = lambda *a: seen.append((real(*a).clone(), a[4].clone())) or seen[-1][0]
    try:
        run(sampler, 0.5, True, mask=mask, x0=x0)
    finally:
        del ops.q_sample_blend_units
    assert len(seen) == int(mc.S * mc.MIS)
    for blended, img_of in seen:
        assert img_of.tolist() == [0, 1, 0, 1, 0, 1]                           # instance-major units of two images
        for b in range(shape[0]):
            keep = mask[b].expand(shape[1:]) > 0
            rows = [blended[u][keep] for u in range(6) if img_of[u] == b]
            assert all(torch.equal(r, rows[0]) for r in rows[1:])
    assert not torch.equal(seen[1][0][0], seen[1][0][2])                      # outside it they differ after one step
    ones = torch.ones(shape[0], 1, *shape[2:])
    noises = mc.make_noises(shape, mc.S, 0.5, True)
    got, _ = run(sampler_for(), 0.5, True, noises=noises, mask=ones, x0=x0)
    want, _ = run(sampler_for(DDIMSampler), 0.5, True, noises=noises, mask=ones, x0=x0, inputs=mis_inputs(instances=False)[0])
    assert torch.equal(got, want)


# ---- 6: sample_layouts -------------------------------------------------------------------------------------------------------
def test_a_uniform_layout_list_equals_sample(two_threads):
    meta, inp, _, _, _ = env()
    shape = tuple(inp["x"].shape)
    mask, x0 = mc.make_inpaint(shape)
    noises = mc.make_noises(shape, mc.S, 0.5, True)
    want, _ = run(sampler_for(), 0.5, True, noises=noises, mask=mask, x0=x0)
    sampler = sampler_for()
    drawn = mc.replay(sampler, noises)
    counts = dict(sampler.engine.ops.calls)
    got = sampler.sample_layouts(mc.S, [mis_inputs(slice(0, 1)), mis_inputs(slice(1, 2))], uc=inp["uc"], guidance_scale=mc.GUIDANCE,
                                 eta=0.5, masks=[mask[0:1], mask[1:2]], x0s=[x0[0:1], x0[1:2]])
    assert len(drawn) == len(noises) and torch.equal(got, want)
    assert sampler.engine.ops.calls.get("mis_merge_ragged", 0) - counts.get("mis_merge_ragged", 0) == 1


RAGGED = [dict(seed=3101, n_inst=0, n_boxes=1, images=1), dict(seed=3102, n_inst=2, n_boxes=2, images=2),
          dict(seed=3103, n_inst=1, n_boxes=1, images=1)]


def test_a_ragged_layout_list_equals_sample_on_every_layout_alone(two_threads):
    """N = 0, 2, 1 instances, K = 1, 2, 1 images; layout 1 is inpainted, layout 2 has a mask too, layout 0 has none."""
    _, _, model, gi, diffusion = env()
    datas = [lc.build_layout(spec, synth) for spec in RAGGED]
    K = [d["x"].shape[0] for d in datas]
    shape = (sum(K),) + tuple(datas[0]["x"].shape[1:])
    mask, x0 = mc.make_inpaint(shape)
    noises = mc.make_noises(shape, lc.S, 0.5, True)
    base = [sum(K[:l]) for l in range(len(K))]
    masks = [None] + [mask[base[l]:base[l] + K[l]] for l in (1, 2)]
    x0s = [None] + [x0[base[l]:base[l] + K[l]] for l in (1, 2)]
    sampler = sampler_for(mis=lc.MIS, alpha_type=lc.ALPHA_TYPE)
    mc.replay(sampler, noises)
    got = sampler.sample_layouts(lc.S, [lc.input_all(d, d["x"], gi.prepare, synth) for d in datas], uc=torch.cat([d["uc"] for d in datas], 0),
                                 guidance_scale=lc.GUIDANCE, eta=0.5, masks=masks, x0s=x0s)
    assert tuple(got.shape) == shape
    for l, d in enumerate(datas):
        for k in range(K[l]):
            row = base[l] + k
            alone = sampler_for(mis=lc.MIS, alpha_type=lc.ALPHA_TYPE)
            mc.replay(alone, [n[row:row + 1] for n in noises])
            x = d["x"][k:k + 1]
            kw = dict(mask=torch.zeros(1, 1, *shape[2:]), x0=torch.zeros(1, *shape[1:])) if masks[l] is None else \
                dict(mask=masks[l][k:k + 1], x0=x0s[l][k:k + 1])
            want = alone.sample(lc.S, tuple(x.shape), lc.input_all(d, x, gi.prepare, synth), uc=d["uc"], guidance_scale=lc.GUIDANCE, eta=0.5, **kw)
            assert torch.equal(got[row:row + 1], want), (l, k)


def test_sample_layouts_refusals(monkeypatch):
    _, _, model, gi, _ = env()
    datas = [lc.build_layout(spec, synth) for spec in RAGGED]
    layouts = [lc.input_all(d, d["x"], gi.prepare, synth) for d in datas]
    uc = torch.cat([d["uc"] for d in datas], 0)
    sampler = sampler_for(mis=lc.MIS)
    with monkeypatch.context() as m:
        m.setattr(sampler.engine, "masked_fuser", True)
        with pytest.raises(ValueError, match="masked gated self-attention"):
            sampler.sample_layouts(lc.S, layouts, uc=uc, guidance_scale=lc.GUIDANCE)
    with pytest.raises(ValueError, match="reaches 0 inside phase 1"):
        sampler_for(mis=lc.MIS, alpha_type=[0.2, 0.0, 0.8]).sample_layouts(lc.S, layouts, uc=uc, guidance_scale=lc.GUIDANCE)
    with pytest.raises(ValueError, match="crop_and_paste_latents"):
        sampler_for(mis=lc.MIS, crop_and_paste_latents=True).sample_layouts(lc.S, layouts, uc=uc, guidance_scale=lc.GUIDANCE)
    with pytest.raises(ValueError, match="one entry per layout"):
        sampler.sample_layouts(lc.S, layouts, uc=uc, guidance_scale=lc.GUIDANCE, masks=[torch.zeros(1, 1, 16, 16)] * 3, x0s=None)
    with pytest.raises(ValueError, match="x0s without masks"):
        sampler.sample_layouts(lc.S, layouts, uc=uc, guidance_scale=lc.GUIDANCE, masks=None, x0s=[torch.zeros(1, 4, 16, 16)] * 3)


def test_the_shim_and_the_signatures():
    import inspect
    from ldm.models.diffusion.ddim_instance import DDIMSamplerInst as Shim
    assert Shim is DDIMSamplerInst and issubclass(Shim, PLMSSamplerInst)
    assert inspect.signature(Shim.__init__) == inspect.signature(PLMSSamplerInst.__init__)
    p = inspect.signature(Shim.sample).parameters
    assert list(p) == ["self", "S", "shape", "input", "uc", "guidance_scale", "mask", "x0", "eta"] and p["eta"].default == 0.
    p = inspect.signature(Shim.sample_layouts).parameters
    assert list(p) == ["self", "S", "layouts", "uc", "guidance_scale", "eta", "masks", "x0s"]
    assert (p["eta"].default, p["masks"].default, p["x0s"].default) == (0., None, None)
    with pytest.raises(NotImplementedError):                                   # the inherited PLMS entry point would run DDIM steps
        sampler_for().plms_sampling((2, 4, 16, 16), mis_inputs())


def test_per_call_state_is_dropped_when_the_call_returns(two_threads):
    sampler = sampler_for()
    out, _ = run(sampler, 0.5, True)
    assert torch.isfinite(out).all() and sampler._run is None and sampler._inpaint is None


# ---- 7: world sizes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_ranks_are_bit_identical_to_one_process(world):
    """eta 0.5 with a mask over gloo: 2 ranks (``image`` ownership: a rank's phase 2 covers a subset of the images, through the
    table) and 3 ranks (more ranks than images, ``instance`` ownership).  Every rank draws; rank 0's draws are what all use."""
    import torch.multiprocessing as mp
    from tests import ddim_mis_worker
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 500) + 31 + world
    procs = [ctx.Process(target=ddim_mis_worker.run, args=(r, world, port, q, WORKER_THREADS)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=600) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
    n = torch.get_num_threads()
    torch.set_num_threads(WORKER_THREADS)
    try:
        one, n_one = run(sampler_for(), 0.5, True)
    finally:
        torch.set_num_threads(n)
    for rank, out, drawn in res:
        assert drawn == n_one, rank
        assert torch.equal(torch.from_numpy(out), one), f"rank {rank} of world {world} must be bit-identical to one process"


# ---- 8: CLI ------------------------------------------------------------------------------------------------------------------------
def test_cli_refuses_ddim_inst_without_mis_before_any_model_is_built(monkeypatch):
    import inference
    built = []
    monkeypatch.setattr(inference, "instantiate_from_config", lambda *a, **k: built.append(a) or (_ for _ in ()).throw(AssertionError("built")))
    monkeypatch.setattr(inference, "load_yaml", lambda *a, **k: built.append(a) or {})
    monkeypatch.setattr(sys, "argv", ["inference.py", "--synthetic_weights", "--sampler", "ddim_inst", "--mis", "0"])
    with pytest.raises(SystemExit) as e:
        inference.main()
    assert isinstance(e.value.code, str) and "--mis > 0" in e.value.code and not built


class _StubAutoencoder(torch.nn.Module):
    """8 x nearest-neighbour up / 8 x mean-pool down between a 4-channel latent and an RGB image: the CLI's plumbing, not a VAE."""

    def decode(self, z):
        return z[:, :3].repeat_interleave(8, 2).repeat_interleave(8, 3)

    def encode(self, img):
        p = torch.nn.functional.avg_pool2d(img, 8)
        return torch.cat([p, p[:, :1]], 1)


DEMOS = [os.path.join(REPO, "demos", n) for n in ("demo_four_boxes.json", "demo_points.json")]


@pytest.mark.parametrize("n_json", [1, 2])
def test_cli_runs_ddim_inst_end_to_end_on_the_emulation(monkeypatch, tmp_path, n_json):
    """``inference.py --sampler ddim_inst`` with eta and inpainting, one JSON (``sample``) and two (``sample_layouts``, the one
    image / mask pair for both layouts), on a reduced-width UNet over the emulated engine and a stub autoencoder.  ``--alpha 1``: the
    gate never reaches 0 (the first-conv swap hard-codes the full model's 320 channels)."""
    import inference
    import instancediffusion_amd.engine as engine_mod
    from PIL import Image
    meta = cases.load_golden(mc.TAG)["meta"]
    made = []

    def instantiate(cfg, *a, **k):
        if cfg["target"].endswith("UNetModel"):
            return build_model(dict(cases.cfg_for(meta["cfg"], meta["variant"]), image_size=meta["latent"]))
        if cfg["target"].endswith("AutoencoderKL"):
            return _StubAutoencoder()
        return real_instantiate(cfg, *a, **k)

    def emulated_engine(model, dtype=None, **k):
        made.append(RealEngine(model, ops=CountingOps(torch.float32), use_graphs=False))
        return made[-1]
    real_instantiate, RealEngine = inference.instantiate_from_config, engine_mod.UNetEngine
    monkeypatch.setattr(inference, "instantiate_from_config", instantiate)
    monkeypatch.setattr(engine_mod, "UNetEngine", emulated_engine)
    size = 8 * meta["latent"]
    g = np.random.default_rng(5)
    blocks = g.integers(0, 256, (size // 8, size // 8, 3), dtype=np.uint8)        # constant 8 x 8 blocks: a latent of full contrast
    Image.fromarray(np.kron(blocks, np.ones((8, 8, 1), dtype=np.uint8))).save(tmp_path / "img.png")
    keep = np.zeros((size, size), dtype=np.uint8)
    keep[:, : size // 2] = 255
    Image.fromarray(keep, mode="L").save(tmp_path / "mask.png")
    monkeypatch.setattr(sys, "argv", ["inference.py", "--synthetic_weights", "--device", "cpu", "--test_config", "configs/test_box.yaml",
                                      "--sampler", "ddim_inst", "--mis", "0.4", "--alpha", "1.0", "--steps", "5", "--ddim_eta", "0.5", "--num_images", "1",
                                      "--init_image", str(tmp_path / "img.png"), "--inpaint_mask", str(tmp_path / "mask.png"),
                                      "--output", str(tmp_path / "out"), "--save_latents", "--input_json", *DEMOS[:n_json]])
    monkeypatch.chdir(REPO)
    inference.main()
    calls = made[-1].ops.calls
    assert calls.get("ddim_update_units", 0) > 0 and calls.get("q_sample_blend_units", 0) > 0 and "plms_update" not in calls
    assert calls.get("mis_merge_ragged" if n_json == 2 else "mis_merge", 0) == 1
    found = [os.path.join(d, f) for d, _, fs in os.walk(tmp_path / "out") for f in fs]
    assert sum(f.endswith(".png") for f in found) == n_json
    lats = [torch.load(f)["latents"] for f in found if f.endswith("latents.pt")]
    assert len(lats) == n_json and all(tuple(v.shape) == (1, 4, meta["latent"], meta["latent"]) and torch.isfinite(v).all() for v in lats)
    # the kept half is held to the encoded image up to the last step's noise; the repainted half is not
    x0 = _StubAutoencoder().encode(inference.load_init_image(str(tmp_path / "img.png"), size))
    half = meta["latent"] // 2
    for v in lats:
        assert cases.rel_rms(v[..., :half], x0[..., :half]) < 0.2 < cases.rel_rms(v[..., half:], x0[..., half:])


# ---- 9: C ABI ------------------------------------------------------------------------------------------------------------------------
def test_unit_kernels_argument_validation_without_gpu():
    """Both symbols are exported with prototypes, and every argument error is reported before anything touches a device (fake, never
    dereferenced pointers, as tests/test_capi.py does)."""
    from instancediffusion_amd import _lib
    lib = _lib.load()
    assert "idf_ddim_update_units" in _lib.SYMBOLS and "idf_q_sample_blend_units" in _lib.SYMBOLS and lib.idf_abi_version() == 5
    assert lib.idf_ddim_update_units.argtypes is not None and len(lib.idf_ddim_update_units.argtypes) == 16
    assert lib.idf_q_sample_blend_units.argtypes is not None and len(lib.idf_q_sample_blend_units.argtypes) == 14
    a_t, a_prev, sigma = ddim_cases.TRIPLES[1]

    def upd(x=0x10000, ec=0x20000, eu=0x30000, a_t=a_t, a_prev=a_prev, sigma=sigma, nz=0x40000, tab=0x60000, out=0x50000, U=3, B=2, chw=64):
        return lib.idf_ddim_update_units(x, ec, eu, 7.5, a_t, a_prev, sigma, 0.76, nz, tab, out, None, U, B, chw, None)
    bad = [upd(x=None), upd(ec=None), upd(out=None), upd(a_t=0.0), upd(a_t=-1.0), upd(a_prev=-0.5), upd(sigma=-0.5),
           upd(a_prev=0.9, sigma=0.5), upd(nz=None), upd(a_t=float("nan")),                    # idf_ddim_update's cases
           upd(U=0), upd(U=-1), upd(B=0), upd(chw=0), upd(tab=None),                           # the new ones: U != B needs the table
           upd(x=None, tab=None, U=2), upd(x=None, nz=None, sigma=0.0)]                        # table-free forms check the rest too
    assert bad == [-1] * len(bad), bad

    def blend(x0=0x10000, nz=0x20000, mask=0x30000, img=0x40000, tab=0x60000, out=0x50000, U=3, B=2, Cc=4, HW=32, mc_=1):
        return lib.idf_q_sample_blend_units(x0, nz, mask, img, tab, 0.6, 0.8, out, U, B, Cc, HW, mc_, None)
    bad = [blend(x0=None), blend(nz=None), blend(mask=None), blend(img=None), blend(out=None), blend(B=0), blend(Cc=0), blend(HW=0),
           blend(mc_=0), blend(mc_=2), blend(mc_=5), blend(U=0), blend(tab=None), blend(tab=None, U=2)]
    assert bad == [-1] * len(bad), bad
