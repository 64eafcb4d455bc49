"""``sample_from`` (entering the schedule at step ``start``) of the three single-trajectory samplers, ``noised_start`` and ``hires_pass``
over the CPU op emulation (tests/emul_ops_hires.py), tiny_box inputs at S = 5, CFG 7.5: exact continuation of a full run, the restated
samplers of tests/hires_cases.py, exact launch counts, the alpha schedule at its absolute indices."""
from functools import partial

import numpy as np
import pytest
import torch

from instancediffusion_amd import synth
from instancediffusion_amd.engine import UNetEngine
from instancediffusion_amd.host import hires
from instancediffusion_amd.host.alpha import alpha_generator, set_alpha_scale
from instancediffusion_amd.host.diffusion import LatentDiffusion
from instancediffusion_amd.host.samplers import DDIMSampler, DPMSolverSampler, PLMSSampler
from grounding_input.text_grounding_tokinzer_input import GroundingNetInput
from oracle import ref_cpu
from tests import cases, ddim_mis_cases
from tests import hires_cases as hc
from tests.emul_ops_hires import EmulOpsHires
from tests.test_engine_emulated import build_model

EMUL_TRAJ_TOL = 5e-3            # the bar of the emulated trajectory tests (tests/test_ddim_host.py, tests/test_dpmpp_host.py)
CLASSES = {"plms": PLMSSampler, "ddim": DDIMSampler, "dpmpp": DPMSolverSampler}
KW = {"plms": {}, "ddim": dict(eta=0.0), "dpmpp": dict(order=2)}
UPDATE = {"plms": "plms_update", "ddim": "ddim_update", "dpmpp": "dpmpp_update"}


def _setup(kind, alphas_fn=None, recorder=None):
    meta = cases.load_golden(hc.TAG)["meta"]
    assert meta["S"] == hc.S
    inp = cases.build_inputs(meta)
    model = build_model(cases.cfg_for(meta["cfg"], meta["variant"]))
    model._engine = UNetEngine(model, ops=EmulOpsHires(torch.float32), use_graphs=False)
    model.first_conv_sd_override = synth.synth_first_conv_sd()
    gi = GroundingNetInput()
    model.grounding_tokenizer_input = gi

    def set_alpha(m, a):
        if recorder is not None:
            recorder.append(a)
        return set_alpha_scale(m, a)
    sampler = CLASSES[kind](LatentDiffusion(linear_start=0.00085, linear_end=0.012, timesteps=1000), model,
                            alpha_generator_func=alphas_fn or partial(alpha_generator, type=meta["alpha_type"]), set_alpha_scale=set_alpha)
    return meta, inp, gi, sampler


def _oracle(meta):
    cfg = cases.cfg_for(meta["cfg"], meta["variant"])
    return ref_cpu.OracleModel(synth.synth_state_dict(cases.unet_schema(cfg)), cfg, synth.synth_first_conv_sd())


def _oracle_input(inp, x):
    return dict(x=x.clone(), timesteps=None, context=inp["context"], grounding_input=ref_cpu.prepare_grounding(inp["gb"]))


def _sampler_input(inp, gi, x):
    return dict(x=x.clone(), timesteps=None, context=inp["context"], grounding_input=gi.prepare(inp["gb"]))


def _counted(sampler, fn):
    calls = sampler.engine.ops.calls
    before = dict(calls)
    out = fn()
    return out, {k: v - before.get(k, 0) for k, v in calls.items() if v != before.get(k, 0)}


def _forwards(counts):
    """UNet forwards of a run: the emulation counts the first conv once per forward."""
    return counts.get("conv_in", 0)


def _check_counts(kind, counts, start, masked=False):
    """S - start forwards (+ 1 for PLMS's predictor step), one update per step (PLMS: two at the predictor step, each behind a
    guidance combine), a blend only with a mask, and never a q_sample or a resize inside a sampler."""
    n = hc.S - start
    assert _forwards(counts) == n + (1 if kind == "plms" else 0), counts
    assert counts.get(UPDATE[kind]) == n + (1 if kind == "plms" else 0), counts
    assert counts.get("cfg_combine", 0) == (n + 1 if kind == "plms" else 0), counts
    if kind == "dpmpp":
        assert counts.get("dpmpp_update_order2", 0) == n - 1, counts
    assert counts.get("q_sample_blend", 0) == (n if masked else 0), counts
    assert "q_sample" not in counts and "resize_planes" not in counts
    assert not [k for k in UPDATE.values() if k != UPDATE[kind] and k in counts], counts


# ---- start = 0 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", hc.SAMPLERS)
def test_start_zero_is_sample_bit_for_bit(kind):
    meta, inp, gi, sampler = _setup(kind)
    shape = tuple(inp["x"].shape)
    a, ca = _counted(sampler, lambda: sampler.sample(hc.S, shape, _sampler_input(inp, gi, inp["x"]), uc=inp["uc"], guidance_scale=hc.GUIDANCE,
                                                     **KW[kind]))
    b, cb = _counted(sampler, lambda: sampler.sample_from(hc.S, shape, _sampler_input(inp, gi, inp["x"]), 0, uc=inp["uc"],
                                                          guidance_scale=hc.GUIDANCE, **KW[kind]))
    assert torch.isfinite(a).all() and torch.equal(a, b) and ca == cb
    _check_counts(kind, cb, 0)


# ---- continuation -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, kw", [("ddim", dict(eta=0.0)), ("dpmpp", dict(order=1))], ids=["ddim-eta0", "dpmpp-order1"])
def test_a_start_continues_a_full_run_bit_for_bit(kind, kw):
    """Steps without history: the latent entering step 2 of a full run, fed to ``sample_from(start=2)``, ends where the full run ends."""
    meta, inp, gi, sampler = _setup(kind)
    shape = tuple(inp["x"].shape)
    seen = []
    real = sampler._step_update

    def spy(img, *a):
        out = real(img, *a)
        seen.append(out.clone())
        return out
    sampler._step_update = spy
    full = sampler.sample(hc.S, shape, _sampler_input(inp, gi, inp["x"]), uc=inp["uc"], guidance_scale=hc.GUIDANCE, **kw)
    del sampler._step_update
    assert len(seen) == hc.S and torch.equal(seen[-1], full)
    i2 = _sampler_input(inp, gi, seen[hc.START - 1])
    got, counts = _counted(sampler, lambda: sampler.sample_from(hc.S, shape, i2, hc.START, uc=inp["uc"], guidance_scale=hc.GUIDANCE, **kw))
    assert torch.equal(got, full) and i2["x"] is got and int(i2["timesteps"][0]) == int(sampler.ddim_timesteps[0])
    assert _forwards(counts) == hc.S - hc.START and counts[UPDATE[kind]] == hc.S - hc.START and "dpmpp_update_order2" not in counts


@pytest.mark.parametrize("start", [1, 2, 4])
@pytest.mark.parametrize("kind", hc.SAMPLERS)
def test_a_start_matches_the_restated_sampler(kind, start):
    """PLMS (a predictor step at ``start``), DDIM and DPM-Solver++ order 2 (a first-order step at ``start``) from a seeded latent."""
    meta, inp, gi, sampler = _setup(kind)
    shape = tuple(inp["x"].shape)
    x = hc.seeded(shape)
    with torch.no_grad():
        want = hc.reference(kind, _oracle(meta), hc.S, _oracle_input(inp, x), inp["uc"], hc.GUIDANCE, start, alpha_type=meta["alpha_type"])
    got, counts = _counted(sampler, lambda: sampler.sample_from(hc.S, shape, _sampler_input(inp, gi, x), start, uc=inp["uc"],
                                                                guidance_scale=hc.GUIDANCE, **KW[kind]))
    err = cases.rel_rms(got, want)
    print(f"[emulated] tiny_box {kind} start {start} of {hc.S}: rel-rms {err:.3e} against the restated sampler (bar {EMUL_TRAJ_TOL:.0e})")
    assert torch.isfinite(got).all() and err < EMUL_TRAJ_TOL
    _check_counts(kind, counts, start)


@pytest.mark.parametrize("kind", ["ddim", "dpmpp"])
def test_the_blend_applies_from_start_on(kind):
    meta, inp, gi, sampler = _setup(kind)
    shape = tuple(inp["x"].shape)
    mask, x0 = ddim_mis_cases.make_inpaint(shape)
    x = hc.seeded(shape)
    noises = hc.seeded(shape, seed=hc.SEED + 1, n=hc.S - hc.START)
    with torch.no_grad():
        want = hc.reference(kind, _oracle(meta), hc.S, _oracle_input(inp, x), inp["uc"], hc.GUIDANCE, hc.START, alpha_type=meta["alpha_type"],
                            mask=mask, x0=x0, noises=noises)
    drawn = ddim_mis_cases.replay(sampler, list(noises))
    got, counts = _counted(sampler, lambda: sampler.sample_from(hc.S, shape, _sampler_input(inp, gi, x), hc.START, uc=inp["uc"],
                                                                guidance_scale=hc.GUIDANCE, mask=mask, x0=x0, **KW[kind]))
    err = cases.rel_rms(got, want)
    print(f"[emulated] tiny_box {kind} start {hc.START} with a mask: rel-rms {err:.3e} (bar {EMUL_TRAJ_TOL:.0e})")
    assert len(drawn) == hc.S - hc.START and err < EMUL_TRAJ_TOL
    _check_counts(kind, counts, hc.START, masked=True)


# ---- the alpha schedule -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", [0, 2, 4])
@pytest.mark.parametrize("kind", hc.SAMPLERS)
def test_alphas_are_the_absolute_ones(kind, start):
    """A decaying gate (1, 0.8, .., 0.2: it never reaches 0, the tiny model cannot swap its first conv): the run entered at ``start``
    sets alphas[start:], one value per step."""
    seen = []

    def decaying(n):
        return [float(v) for v in np.linspace(1.0, 0.2, n)]
    meta, inp, gi, sampler = _setup(kind, alphas_fn=decaying, recorder=seen)
    shape = tuple(inp["x"].shape)
    x = hc.seeded(shape)
    got = sampler.sample_from(hc.S, shape, _sampler_input(inp, gi, x), start, uc=inp["uc"], guidance_scale=hc.GUIDANCE, **KW[kind])
    assert seen == decaying(hc.S)[start:] and len(seen) == hc.S - start
    with torch.no_grad():
        want = hc.reference(kind, _oracle(meta), hc.S, _oracle_input(inp, x), inp["uc"], hc.GUIDANCE, start, alphas=decaying(hc.S))
    assert cases.rel_rms(got, want) < EMUL_TRAJ_TOL


# ---- refusals ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", [-1, hc.S])
@pytest.mark.parametrize("kind", hc.SAMPLERS)
def test_a_start_outside_the_schedule_runs_nothing(kind, start):
    meta, inp, gi, sampler = _setup(kind)
    shape = tuple(inp["x"].shape)
    before = dict(sampler.engine.ops.calls)
    with pytest.raises(ValueError):
        sampler.sample_from(hc.S, shape, _sampler_input(inp, gi, inp["x"]), start, uc=inp["uc"], guidance_scale=hc.GUIDANCE, **KW[kind])
    assert sampler.engine.ops.calls == before


# ---- noised_start, upscale_latents, hires_pass --------------------------------------------------------------------------
def test_noised_start_is_one_q_sample_at_the_first_timestep():
    meta, inp, gi, sampler = _setup("ddim")
    shape = tuple(inp["x"].shape)
    x0, noise = hc.seeded(shape), hc.seeded(shape, seed=hc.SEED + 2)
    (x, start), counts = _counted(sampler, lambda: hires.noised_start(sampler, x0, hc.S, hc.STRENGTH, noise, eta=0.0))
    assert start == hc.START and counts == {"q_sample": 1}
    # the coefficients are the diffusion's own float32 buffers at t = 401 (sqrt taken in float64, then rounded: ddpm.py:33-36) ...
    d = sampler.diffusion
    assert hc.timestep_of(hc.S, start) == 401
    assert torch.equal(x, hc.q_sample_expr(x0, noise, float(d.sqrt_alphas_cumprod[401]), float(d.sqrt_one_minus_alphas_cumprod[401])))
    assert torch.equal(x, d.q_sample(x0, torch.full((shape[0],), 401, dtype=torch.long), noise))
    # ... which the oracle's q_sample (float32 sqrt of the float32 table) meets within an ulp of each coefficient
    assert float((x - hc.q_sample_at(x0, hc.S, start, noise)).abs().max()) <= 4 * hc.U * float(max(x0.abs().max(), noise.abs().max()))
    with pytest.raises(ValueError):
        hires.noised_start(sampler, x0, hc.S, 0.0, noise)
    with pytest.raises(ValueError):
        hires.noised_start(sampler, x0, hc.S, hc.STRENGTH, noise[:1])


@pytest.mark.parametrize("mode", ["bicubic", "bilinear"])
def test_upscale_latents_is_one_launch_over_cached_tables(mode):
    meta, inp, gi, sampler = _setup("plms")
    ops = sampler.engine.ops
    z = hc.seeded((2, 4, 16, 16))
    hires._TABLES.clear()
    out, counts = _counted(sampler, lambda: hires.upscale_latents(ops, z, hc.HIRES_SIZE, mode))
    assert counts == {"resize_planes": 1} and tuple(out.shape) == (2, 4, 24, 24) and len(hires._TABLES) == 1
    tables = next(iter(hires._TABLES.values()))
    again = hires.upscale_latents(ops, z, hc.HIRES_SIZE, mode)
    assert len(hires._TABLES) == 1 and all(a is b for a, b in zip(tables, next(iter(hires._TABLES.values())))) and torch.equal(out, again)
    assert torch.equal(out, hc.resize_expr(z, hc.HIRES_SIZE, mode))
    err = float((out.double() - hc.interpolate64(z, hc.HIRES_SIZE, mode)).abs().max()) / (hc.U * float(z.abs().max()))
    assert err <= 20.0
    hires.upscale_latents(ops, z, (32, 24), mode)
    assert len(hires._TABLES) == 2


@pytest.mark.parametrize("kind", hc.SAMPLERS)
def test_hires_pass_matches_the_composed_reference(kind):
    """16^2 -> 24^2 at strength 0.6 behind a first pass: against ``F.interpolate`` on float64 input rounded to fp32, torch's q_sample
    with the same noise, and the restated sampler from ``start`` at 24^2."""
    meta, inp, gi, sampler = _setup(kind)
    shape = tuple(inp["x"].shape)
    noise = hc.seeded((shape[0], shape[1]) + hc.HIRES_SIZE, seed=hc.SEED + 3)
    i1 = _sampler_input(inp, gi, inp["x"])
    first = sampler.sample(hc.S, shape, i1, uc=inp["uc"], guidance_scale=hc.GUIDANCE, **KW[kind]).clone()
    got, counts = _counted(sampler, lambda: hires.hires_pass(sampler, first, i1, inp["uc"], hc.GUIDANCE, hc.S, hc.STRENGTH, hc.HIRES_SIZE,
                                                             "bicubic", noise, **KW[kind]))
    assert tuple(got.shape) == (shape[0], shape[1]) + hc.HIRES_SIZE and torch.equal(i1["x"], first), "the first pass's input is left as it is"
    assert counts.pop("resize_planes") == 1 and counts.pop("q_sample") == 1
    _check_counts(kind, counts, hc.START)
    with torch.no_grad():
        # the second pass alone, from the emulation's own first pass: what hires_pass adds
        _, want = hc.hires_reference(kind, _oracle(meta), _oracle_input(inp, inp["x"]), inp["uc"], noise, first=first, alpha_type=meta["alpha_type"])
        # and the whole composed run, first pass included
        first_ref, want_all = hc.hires_reference(kind, _oracle(meta), _oracle_input(inp, inp["x"]), inp["uc"], noise, alpha_type=meta["alpha_type"])
    err, err_all = cases.rel_rms(got, want), cases.rel_rms(got, want_all)
    print(f"[emulated] tiny_box {kind} hires 16^2 -> 24^2 strength {hc.STRENGTH}: rel-rms {err:.3e} second pass alone, {err_all:.3e} with the "
          f"first pass (first pass itself {cases.rel_rms(first, first_ref):.3e}; bar {EMUL_TRAJ_TOL:.0e})")
    assert torch.isfinite(got).all() and err < EMUL_TRAJ_TOL and err_all < EMUL_TRAJ_TOL


def test_hires_pass_undoes_a_first_conv_swap():
    """A first pass whose gate reached 0 leaves the first conv swapped; the second pass re-enters in front of those steps and must see
    the model's own first conv there, as a full run would (``UNetModel.reinstate_first_conv``, and the engine's packed image with it)."""
    meta, inp, gi, sampler = _setup("ddim")
    model = sampler.model
    conv = model.input_blocks[0][0]
    own_w, own_b = conv.weight.detach().clone(), conv.bias.detach().clone()
    g = torch.Generator().manual_seed(5)
    model.first_conv_sd_override = dict(weight=torch.randn(own_w.shape, generator=g), bias=torch.randn(own_b.shape, generator=g))
    packed = model.engine.in_blocks[0][0]
    model.reinstate_first_conv()                                             # nothing swapped: a no-op
    assert model.input_blocks[0][0] is conv
    model.restore_first_conv_from_SD()
    assert torch.equal(packed["w"], model.first_conv_sd_override["weight"]) and not torch.equal(packed["w"], own_w)
    shape = tuple(inp["x"].shape)
    hires.hires_pass(sampler, hc.seeded(shape), _sampler_input(inp, gi, inp["x"]), inp["uc"], hc.GUIDANCE, hc.S, 0.2, hc.HIRES_SIZE,
                     "bilinear", hc.seeded((shape[0], shape[1]) + hc.HIRES_SIZE), eta=0.0)
    now = model.input_blocks[0][0]
    assert torch.equal(now.weight, own_w) and torch.equal(now.bias, own_b) and not model._first_conv_swapped
    assert torch.equal(packed["w"], own_w.float()) and torch.equal(packed["b"], own_b.float())
    model.restore_first_conv_from_SD()                                       # and the swap can happen again
    assert torch.equal(packed["w"], model.first_conv_sd_override["weight"])
