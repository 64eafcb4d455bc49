"""``DPMSolverSamplerInst`` (the Multi-instance Sampler on DPM-Solver++(2M) steps) host logic without a GPU, over the CPU op emulation
(tests/emul_ops_dpmpp.py): exact degenerate cases against ``DPMSolverSampler``, the tiny_box case against the composed oracle
(tests/dpmpp_cases.py), independence of chunking and of the world size, ``sample_layouts`` and the CLI.

Bit-for-bit comparisons between runs that form different forwards use the batch-invariant emulation at a fixed thread count, as
tests/test_ddim_mis_emulated.py does.
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
from instancediffusion_amd.host.samplers import DPMSolverSampler, DPMSolverSamplerInst
from grounding_input.text_grounding_tokinzer_input import GroundingNetInput
from oracle import ref_cpu
from tests import cases
from tests import ddim_mis_cases as mc
from tests import dpmpp_cases as dc
from tests import layouts_cases as lc
from tests.emul_ops_dpmpp import EmulOpsDPMppMis
from tests.test_engine_emulated import build_model

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL_TRAJ_TOL = 5e-3            # the bar of tests/test_samplers_emulated.py
WORKER_THREADS = 2              # torch's CPU kernels reduce in a thread-count-dependent order: compare like with like
_ENV = {}
_GI = GroundingNetInput()


class CountingOps(EmulOpsDPMppMis):
    def mis_merge(self, lat, boxes_i32, out, mode):
        self._count("mis_merge")
        return super().mis_merge(lat, boxes_i32, out, mode)


def env(batch_invariant=True):
    """(meta, inputs of tiny_box, model over the emulated engine, GroundingNetInput, diffusion), once per emulation flavour."""
    if batch_invariant not in _ENV:
        meta = cases.load_golden(dc.TAG)["meta"]
        assert (meta["S"], meta["mis"], meta["n_inst"], meta["batch"]) == (dc.S, dc.MIS, 2, 2)
        model = build_model(cases.cfg_for(meta["cfg"], meta["variant"]))
        model._engine = UNetEngine(model, ops=CountingOps(torch.float32, batch_invariant=batch_invariant), use_graphs=False)
        model.first_conv_sd_override = synth.synth_first_conv_sd()
        model.grounding_tokenizer_input = _GI
        _ENV[batch_invariant] = (meta, cases.build_inputs(meta), model, _GI,
                                 LatentDiffusion(linear_start=0.00085, linear_end=0.012, timesteps=1000))
    return _ENV[batch_invariant]


def sampler_for(cls=DPMSolverSamplerInst, batch_invariant=True, mis=dc.MIS, alpha_type=None, **kw):
    meta, inp, model, gi, diffusion = env(batch_invariant)
    extra = dict(mis=mis, **kw) if cls is not DPMSolverSampler else {}
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


def run(sampler, order, masked, noises=None, inputs=None, mask=None, x0=None, counts=None, discretize="uniform"):
    """One ``sample()`` on tiny_box with the q_sample draws replayed; -> (result, number of draws made)."""
    meta, inp, _, _, _ = env()
    shape = tuple(inp["x"].shape)
    if masked and mask is None:
        mask, x0 = mc.make_inpaint(shape)
    drawn = mc.replay(sampler, noises if noises is not None else dc.make_noises(shape, dc.S, masked))
    calls = sampler.engine.ops.calls
    before = dict(calls)
    kw = dict(mask=mask, x0=x0) if masked else {}
    out = sampler.sample(dc.S, shape, inputs if inputs is not None else mis_inputs(), uc=inp["uc"], guidance_scale=dc.GUIDANCE, order=order,
                         discretize=discretize, **kw)
    if counts is not None:
        counts.update({k: v - before.get(k, 0) for k, v in calls.items() if v != before.get(k, 0)})
    return out, len(drawn)


@pytest.fixture
def two_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(WORKER_THREADS)
    yield
    torch.set_num_threads(n)


ORDER_MASK = [(1, False), (2, False), (2, True)]
IDS = ["order1", "order2", "order2_mask"]


# ---- the exact degenerate cases -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order,masked", ORDER_MASK, ids=IDS)
@pytest.mark.parametrize("mis", [0.0, 0.19], ids=["mis0", "int(S*mis)==0"])
def test_without_a_phase_one_step_it_is_the_plain_sampler_on_the_global_input(mis, order, masked, two_threads):
    assert int(dc.S * mis) == 0
    want, n_want = run(sampler_for(DPMSolverSampler), order, masked, inputs=mis_inputs(instances=False)[0])
    got, n_got = run(sampler_for(mis=mis), order, masked)
    assert n_got == n_want == (dc.S if masked else 0)
    assert torch.equal(got, want)


@pytest.mark.parametrize("order,masked", ORDER_MASK, ids=IDS)
def test_a_layout_without_instances_is_the_plain_sampler(order, masked, two_threads):
    """Phase 1 advances the global unit alone, the mean of one unit is exact, and phase 2 continues with that unit's history."""
    want, n_want = run(sampler_for(DPMSolverSampler), order, masked, inputs=mis_inputs(instances=False)[0])
    counts = {}
    got, n_got = run(sampler_for(), order, masked, inputs=mis_inputs(instances=False), counts=counts)
    assert n_got == n_want and torch.equal(got, want)
    assert counts.get("mis_merge") == 1 and counts.get("dpmpp_update") == dc.S
    assert counts.get("dpmpp_update_order2", 0) == (dc.S - 1 if order == 2 else 0)       # the first phase-2 step is second order


# ---- against the composed oracle ----------------------------------------------------------------------------------------------
@pytest.fixture
def oracle():
    """A fresh ``OracleModel`` per test (see tests/test_ddim_mis_emulated.py)."""
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


@pytest.mark.parametrize("order,masked", ORDER_MASK, ids=IDS)
def test_tiny_box_matches_the_composed_reference(oracle, order, masked):
    meta, inp, _, _, _ = env(False)
    shape = tuple(inp["x"].shape)
    mask, x0 = mc.make_inpaint(shape) if masked else (None, None)
    noises = dc.make_noises(shape, dc.S, masked)
    model, inputs = oracle
    with torch.no_grad():
        want = dc.dpmpp_mis_reference(model, dc.S, inputs(), inp["uc"], dc.GUIDANCE, dc.MIS, order=order, alpha_type=meta["alpha_type"],
                                      mask=mask, x0=x0, noises=noises)
    counts = {}
    got, n = run(sampler_for(batch_invariant=False), order, masked, noises=noises, counts=counts)
    err = cases.rel_rms(got, want)
    print(f"[emulated] tiny_box DPM-Solver++ MIS order {order} mask {masked}: rel-rms {err:.3e} against dpmpp_mis_reference "
          f"(bar {EMUL_TRAJ_TOL:.0e})")
    assert n == len(noises) and torch.isfinite(got).all() and err < EMUL_TRAJ_TOL
    mis_step = int(dc.S * dc.MIS)                                               # 6 units = one forward per phase-1 step
    assert counts.get("dpmpp_update") == dc.S                                   # one launch per step, in either phase
    # order 2: every step but the first of phase 1 -- the first step of phase 2 included (the global unit's history)
    assert counts.get("dpmpp_update_order2", 0) == (dc.S - 1 if order == 2 else 0)
    assert counts.get("q_sample_blend_units", 0) == (mis_step if masked else 0)
    assert counts.get("q_sample_blend", 0) == ((dc.S - mis_step) + 1 if masked else 0)   # phase 2, + the hoisted evaluation's input
    assert counts.get("mis_merge") == 1 and "mis_merge_ragged" not in counts and "cfg_combine" not in counts
    assert "ddim_update" not in counts and "ddim_update_units" not in counts and "plms_update" not in counts
    # forwards: the hoisted evaluation (6 cond + 2 uncond rows: one), one per remaining phase-1 step, one per phase-2 step
    assert counts.get("conv_in") == dc.S


def test_phase_two_depends_on_the_history_of_the_global_unit(two_threads):
    """Dropping the history at the merge (a first-order first step of phase 2) gives another result: the hand-over is observable."""
    full, _ = run(sampler_for(), 2, False)
    sampler = sampler_for()
    sampler._history_stack = staticmethod(lambda rows: [])
    cut, _ = run(sampler, 2, False)
    assert not torch.equal(full, cut)


def test_crop_and_paste_merge_matches_the_composed_reference(oracle):
    meta, inp, _, _, _ = env(False)
    model, inputs = oracle
    with torch.no_grad():
        want = dc.dpmpp_mis_reference(model, dc.S, inputs(), inp["uc"], dc.GUIDANCE, dc.MIS, order=2, alpha_type=meta["alpha_type"],
                                      crop_and_paste=True)
    got, _ = run(sampler_for(batch_invariant=False, crop_and_paste_latents=True), 2, False)
    err = cases.rel_rms(got, want)
    print(f"[emulated] tiny_box DPM-Solver++ MIS order 2, crop-and-paste merge: rel-rms {err:.3e} against dpmpp_mis_reference")
    assert err < EMUL_TRAJ_TOL


# ---- chunking -----------------------------------------------------------------------------------------------------------------
def test_result_does_not_depend_on_chunking(two_threads):
    """One unit per forward against all six in one."""
    counts = {}
    one, n_one = run(sampler_for(max_units=1), 2, True, counts=counts)
    mis_step = int(dc.S * dc.MIS)
    assert counts["dpmpp_update"] == 6 * mis_step + (dc.S - mis_step)
    full, n_full = run(sampler_for(), 2, True)
    assert n_one == n_full == dc.S
    assert torch.equal(one, full)


def test_an_all_zero_mask_changes_nothing(two_threads):
    meta, inp, _, _, _ = env()
    shape = tuple(inp["x"].shape)
    _, x0 = mc.make_inpaint(shape)
    masked, _ = run(sampler_for(), 2, True, mask=torch.zeros(shape[0], 1, *shape[2:]), x0=x0)
    plain, _ = run(sampler_for(), 2, False)
    assert torch.equal(masked, plain)


# ---- sample_layouts -----------------------------------------------------------------------------------------------------------
def test_a_uniform_layout_list_equals_sample(two_threads):
    meta, inp, _, _, _ = env()
    shape = tuple(inp["x"].shape)
    mask, x0 = mc.make_inpaint(shape)
    noises = dc.make_noises(shape, dc.S, True)
    want, _ = run(sampler_for(), 2, True, noises=noises, mask=mask, x0=x0)
    sampler = sampler_for()
    drawn = mc.replay(sampler, noises)
    counts = dict(sampler.engine.ops.calls)
    got = sampler.sample_layouts(dc.S, [mis_inputs(slice(0, 1)), mis_inputs(slice(1, 2))], uc=inp["uc"], guidance_scale=dc.GUIDANCE,
                                 order=2, masks=[mask[0:1], mask[1:2]], x0s=[x0[0:1], x0[1:2]])
    assert len(drawn) == len(noises) and torch.equal(got, want)
    assert sampler.engine.ops.calls.get("mis_merge_ragged", 0) - counts.get("mis_merge_ragged", 0) == 1


RAGGED = [dict(seed=3101, n_inst=0, n_boxes=1, images=1), dict(seed=3102, n_inst=2, n_boxes=2, images=2),
          dict(seed=3103, n_inst=1, n_boxes=1, images=1)]


@pytest.mark.parametrize("discretize", ["uniform", "logsnr"])
def test_a_ragged_layout_list_equals_sample_on_every_layout_alone(two_threads, discretize):
    """N = 0, 2, 1 instances, K = 1, 2, 1 images; layout 1 is inpainted, layout 2 has a mask too, layout 0 has none."""
    _, _, model, gi, diffusion = env()
    datas = [lc.build_layout(spec, synth) for spec in RAGGED]
    K = [d["x"].shape[0] for d in datas]
    shape = (sum(K),) + tuple(datas[0]["x"].shape[1:])
    mask, x0 = mc.make_inpaint(shape)
    noises = dc.make_noises(shape, lc.S, True)
    base = [sum(K[:l]) for l in range(len(K))]
    masks = [None] + [mask[base[l]:base[l] + K[l]] for l in (1, 2)]
    x0s = [None] + [x0[base[l]:base[l] + K[l]] for l in (1, 2)]
    sampler = sampler_for(mis=lc.MIS, alpha_type=lc.ALPHA_TYPE)
    mc.replay(sampler, noises)
    got = sampler.sample_layouts(lc.S, [lc.input_all(d, d["x"], gi.prepare, synth) for d in datas], uc=torch.cat([d["uc"] for d in datas], 0),
                                 guidance_scale=lc.GUIDANCE, order=2, discretize=discretize, masks=masks, x0s=x0s)
    assert tuple(got.shape) == shape
    for l, d in enumerate(datas):
        for k in range(K[l]):
            row = base[l] + k
            alone = sampler_for(mis=lc.MIS, alpha_type=lc.ALPHA_TYPE)
            mc.replay(alone, [n[row:row + 1] for n in noises])
            x = d["x"][k:k + 1]
            kw = dict(mask=torch.zeros(1, 1, *shape[2:]), x0=torch.zeros(1, *shape[1:])) if masks[l] is None else \
                dict(mask=masks[l][k:k + 1], x0=x0s[l][k:k + 1])
            want = alone.sample(lc.S, tuple(x.shape), lc.input_all(d, x, gi.prepare, synth), uc=d["uc"], guidance_scale=lc.GUIDANCE,
                                order=2, discretize=discretize, **kw)
            assert torch.equal(got[row:row + 1], want), (l, k)


def test_refusals_and_per_call_state(two_threads):
    sampler = sampler_for()
    with pytest.raises(ValueError, match="order must be 1 or 2"):
        sampler.sample(dc.S, (2, 4, 16, 16), mis_inputs(), order=3)
    with pytest.raises(ValueError, match="order must be 1 or 2"):
        sampler.sample_layouts(dc.S, [mis_inputs(slice(0, 1))], order=0)
    with pytest.raises(TypeError):                                              # eta does not exist
        sampler.sample(dc.S, (2, 4, 16, 16), mis_inputs(), eta=0.5)
    with pytest.raises(NotImplementedError):                                    # the inherited PLMS entry point
        sampler.plms_sampling((2, 4, 16, 16), mis_inputs())
    out, _ = run(sampler, 2, True)
    assert torch.isfinite(out).all() and sampler._run is None and sampler._inpaint is None


# ---- world sizes ------------------------------------------------------------------------------------------------------------------
def test_two_ranks_are_bit_identical_to_one_process():
    """Order 2 with a mask over gloo, 2 ranks (``image`` ownership: a rank's phase 2 covers a subset of the images and continues from
    the history of ITS global units)."""
    import torch.multiprocessing as mp
    from tests import dpmpp_mis_worker
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 500) + 57
    procs = [ctx.Process(target=dpmpp_mis_worker.run, args=(r, world, port, q, WORKER_THREADS)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=600) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
    n = torch.get_num_threads()
    torch.set_num_threads(WORKER_THREADS)
    try:
        one, n_one = run(sampler_for(), 2, True)
    finally:
        torch.set_num_threads(n)
    for rank, out, drawn in res:
        assert drawn == n_one, rank
        assert torch.equal(torch.from_numpy(out), one), f"rank {rank} of world {world} must be bit-identical to one process"


# ---- CLI ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv,needle", [
    (["--sampler", "dpmpp_inst", "--mis", "0"], "--mis > 0"),
    (["--sampler", "dpmpp"], "--mis 0"),                                        # the default --mis is > 0
    (["--sampler", "dpmpp", "--mis", "0.36"], "--mis 0"),
    (["--sampler", "dpmpp", "--mis", "0", "--ddim_eta", "0.5"], "--ddim_eta"),
    (["--sampler", "dpmpp_inst", "--mis", "0.36", "--ddim_eta", "0"], "--ddim_eta"),
    (["--sampler", "ddim", "--mis", "0", "--dpm_order", "1"], "--dpm_order"),
    (["--mis", "0", "--dpm_spacing", "logsnr"], "--dpm_spacing"),
    (["--sampler", "dpmpp", "--mis", "0", "--init_image", "a.png"], "both --init_image and --inpaint_mask"),
])
def test_cli_refusals_come_before_any_model_is_built(monkeypatch, argv, needle):
    import inference
    built = []
    monkeypatch.setattr(inference, "instantiate_from_config", lambda *a, **k: built.append(a) or (_ for _ in ()).throw(AssertionError("built")))
    monkeypatch.setattr(inference, "load_yaml", lambda *a, **k: built.append(a) or {})
    monkeypatch.setattr(sys, "argv", ["inference.py", "--synthetic_weights"] + argv)
    with pytest.raises(SystemExit) as e:
        inference.main()
    assert isinstance(e.value.code, str) and needle in e.value.code and not built


@pytest.mark.parametrize("bad", [["--dpm_order", "3"], ["--dpm_spacing", "quad"], ["--sampler", "dpm"]])
def test_cli_argparse_refuses_unknown_choices(monkeypatch, bad):
    import inference
    monkeypatch.setattr(sys, "argv", ["inference.py", "--synthetic_weights", "--sampler", "dpmpp", "--mis", "0"] + bad)
    with pytest.raises(SystemExit) as e:
        inference.main()
    assert e.value.code == 2


class _StubAutoencoder(torch.nn.Module):
    """8 x nearest-neighbour up / 8 x mean-pool down between a 4-channel latent and an RGB image: the CLI's plumbing, not a VAE."""

    def decode(self, z):
        return z[:, :3].repeat_interleave(8, 2).repeat_interleave(8, 3)

    def encode(self, img):
        p = torch.nn.functional.avg_pool2d(img, 8)
        return torch.cat([p, p[:, :1]], 1)


DEMOS = [os.path.join(REPO, "demos", n) for n in ("demo_four_boxes.json", "demo_points.json")]


@pytest.mark.parametrize("sampler,mis", [("dpmpp_inst", "0.4"), ("dpmpp", "0")])
@pytest.mark.parametrize("n_json", [1, 2])
def test_cli_runs_end_to_end_on_the_emulation(monkeypatch, tmp_path, n_json, sampler, mis):
    """``inference.py --sampler dpmpp_inst | dpmpp`` with inpainting, one JSON (``sample``) and two (``sample_layouts`` / one row-stacked
    call; the one image / mask pair for both layouts), on a reduced-width UNet over the emulated engine and a stub autoencoder.
    ``--alpha 1``: the gate never reaches 0 (the first-conv swap hard-codes the full model's 320 channels)."""
    import inference
    import instancediffusion_amd.engine as engine_mod
    from PIL import Image
    meta = cases.load_golden(dc.TAG)["meta"]
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
                                      "--sampler", sampler, "--mis", mis, "--alpha", "1.0", "--steps", "5", "--dpm_spacing", "logsnr",
                                      "--num_images", "1", "--init_image", str(tmp_path / "img.png"), "--inpaint_mask", str(tmp_path / "mask.png"),
                                      "--output", str(tmp_path / "out"), "--save_latents", "--input_json", *DEMOS[:n_json]])
    monkeypatch.chdir(REPO)
    inference.main()
    calls = made[-1].ops.calls
    inst = sampler == "dpmpp_inst"
    assert calls.get("dpmpp_update", 0) > 0 and calls.get("dpmpp_update_order2", 0) > 0
    assert "plms_update" not in calls and "ddim_update" not in calls and "ddim_update_units" not in calls
    if inst:
        assert calls.get("q_sample_blend_units", 0) > 0 and calls.get("mis_merge_ragged" if n_json == 2 else "mis_merge", 0) == 1
    else:
        assert calls.get("q_sample_blend", 0) == 5 and calls["dpmpp_update"] == 5 and "mis_merge" not in calls
    found = [os.path.join(d, f) for d, _, fs in os.walk(tmp_path / "out") for f in fs]
    assert sum(f.endswith(".png") for f in found) == n_json
    lats = [torch.load(f)["latents"] for f in found if f.endswith("latents.pt")]
    assert len(lats) == n_json and all(tuple(v.shape) == (1, 4, meta["latent"], meta["latent"]) and torch.isfinite(v).all() for v in lats)
    # the kept half is held to the encoded image up to the last step's noise; the repainted half is not
    x0 = _StubAutoencoder().encode(inference.load_init_image(str(tmp_path / "img.png"), size))
    half = meta["latent"] // 2
    for v in lats:
        assert cases.rel_rms(v[..., :half], x0[..., :half]) < 0.2 < cases.rel_rms(v[..., half:], x0[..., half:])
