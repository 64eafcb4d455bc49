"""DDIMSampler host logic without a GPU: schedule, loop, noise order, the ``ldm`` shim and ``inference.py``'s new flags.

Goldens (``tests/golden/{tiny,mid}_box_ddim.pt``, tests/make_ddim_golden.py) are the UNMODIFIED reference's ``DDIMSampler``
trajectories, schedules and noise draws.  The sampler runs over the CPU op emulation (tests/emul_ops_ddim.py), whose two DDIM ops are
the fp32 torch expressions the HIP kernels reproduce bit for bit (tests/test_ddim_kernels_gpu.py).
"""
import inspect
import sys
from functools import partial

import numpy as np
import pytest
import torch

from instancediffusion_amd import synth
from instancediffusion_amd.engine import UNetEngine
from instancediffusion_amd.host.alpha import alpha_generator, set_alpha_scale
from instancediffusion_amd.host.diffusion import LatentDiffusion
from instancediffusion_amd.host.samplers import DDIMSampler, PLMSSampler
from grounding_input.text_grounding_tokinzer_input import GroundingNetInput
from oracle import ref_cpu
from tests import cases, ddim_cases
from tests.emul_ops_ddim import EmulOpsDDIM
from tests.test_engine_emulated import build_model

ORACLE_TRAJ_TOL = 5e-3          # tests/test_oracle_golden.py: TRAJ_TOL and its max-abs companion
EMUL_TRAJ_TOL = 5e-3            # tests/test_samplers_emulated.py


def _diffusion():
    return LatentDiffusion(linear_start=0.00085, linear_end=0.012, timesteps=1000)


def _setup(tag):
    gold = ddim_cases.load(tag)
    meta = gold["meta"]
    cfg = cases.cfg_for(meta["cfg"], meta["variant"])
    inp = cases.build_inputs(meta)
    assert torch.equal(inp["x"].flatten()[:32], meta["x_fp"]["head"])
    model = build_model(cfg)
    model._engine = UNetEngine(model, ops=EmulOpsDDIM(torch.float32), use_graphs=False)
    model.first_conv_sd_override = synth.synth_first_conv_sd()
    gi = GroundingNetInput()
    model.grounding_tokenizer_input = gi
    sampler = DDIMSampler(_diffusion(), model, alpha_generator_func=partial(alpha_generator, type=meta["alpha_type"]),
                          set_alpha_scale=set_alpha_scale)
    return gold, meta, inp, model, gi, sampler


def _sampler_input(inp, gi):
    return dict(x=inp["x"].clone(), timesteps=None, context=inp["context"], grounding_input=gi.prepare(inp["gb"]))


def _replay(sampler, noises):
    drawn = []
    it = iter(noises)

    def noise_fn(shape):
        n = next(it)
        assert tuple(n.shape) == tuple(shape)
        drawn.append(n)
        return n.clone()
    sampler.noise_fn = noise_fn
    return drawn


# ---- schedule -----------------------------------------------------------------------------------------------------
def _schedules():
    out = []
    for tag, g in ddim_cases.GOLDENS.items():
        gold = ddim_cases.load(tag)
        out += [(f"{tag}:{name}", gold["meta"]["S"], c) for name, c in gold["cases"].items()]
        if tag == "tiny_box_ddim":
            out += [(key, int(key[1:].split("_")[0]), c) for key, c in gold["schedules"].items()]
    return out


@pytest.mark.parametrize("what,S,ref", _schedules(), ids=[s[0] for s in _schedules()])
def test_schedule_is_the_references(what, S, ref):
    """Timesteps and the fp32 scalars a step hands the kernel (a_t, a_prev, sigma_t, sqrt(1 - a_t)) equal the reference's
    make_schedule buffers after the fp32 cast ``torch.full`` applies (ddim.py:118-121) -- S = 5 and S = 50, eta 0 / 0.5 / 1."""
    sampler = DDIMSampler(_diffusion(), model=None)
    sampler.make_schedule(ddim_num_steps=S, ddim_eta=float(ref["eta"]))
    assert torch.equal(torch.as_tensor(sampler.ddim_timesteps.copy()), ref["ddim_timesteps"]) and len(sampler.ddim_timesteps) == S

    def f32(v):
        return torch.as_tensor(np.asarray(v)).to(torch.float32)
    for name in ("ddim_alphas", "ddim_alphas_prev", "ddim_sigmas", "ddim_sqrt_one_minus_alphas"):
        assert torch.equal(f32(getattr(sampler, name)), ref[name].to(torch.float32)), name
    assert (float(ref["eta"]) == 0) == bool((f32(sampler.ddim_sigmas) == 0).all())
    # the test-side restatement agrees too
    steps, a, a_prev, sigmas, s1m = ddim_cases.ddim_schedule(S, float(ref["eta"]))
    assert torch.equal(f32(sigmas), ref["ddim_sigmas"].to(torch.float32)) and torch.equal(f32(s1m), ref["ddim_sqrt_one_minus_alphas"].float())
    assert torch.equal(f32(a), ref["ddim_alphas"].float()) and torch.equal(f32(a_prev), ref["ddim_alphas_prev"].to(torch.float32))


def test_kernel_test_triples_come_from_the_schedule():
    c = ddim_cases.load("tiny_box_ddim")["cases"]["eta0.5"]
    for (a_t, a_prev, sigma), index in zip(ddim_cases.TRIPLES, (4, 2, 0)):
        got = (float(c["ddim_alphas"][index].float()), float(c["ddim_alphas_prev"][index].to(torch.float32)),
               float(c["ddim_sigmas"][index].to(torch.float32)))
        assert got == (float(np.float32(a_t)), float(np.float32(a_prev)), float(np.float32(sigma))), (index, got)


def test_plms_schedule_still_refuses_eta():
    with pytest.raises(ValueError):
        PLMSSampler(_diffusion(), model=None).make_schedule(5, ddim_eta=0.5)


# ---- trajectories -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,name", ddim_cases.ALL_CASES)
def test_ddim_reference_matches_golden(tag, name):
    """The test-side restatement of ddim.py over the CPU oracle model, held to the bar tests/test_oracle_golden.py holds the
    oracle's PLMS trajectories to."""
    gold, case, eta, mask, x0, noises = ddim_cases.case_inputs(tag, name)
    meta = gold["meta"]
    cfg = cases.cfg_for(meta["cfg"], meta["variant"])
    inp = cases.build_inputs(meta)
    with torch.no_grad():
        model = ref_cpu.OracleModel(synth.synth_state_dict(cases.unet_schema(cfg)), cfg, synth.synth_first_conv_sd())
        i0 = dict(x=inp["x"].clone(), timesteps=None, context=inp["context"], grounding_input=ref_cpu.prepare_grounding(inp["gb"]))
        out = ddim_cases.ddim_reference(model, meta["S"], i0, inp["uc"], ddim_cases.GUIDANCE, eta=eta, alpha_type=meta["alpha_type"],
                                        mask=mask, x0=x0, noises=noises)
    err = cases.rel_rms(out, case["final"])
    print(f"[oracle] {tag} {name}: ddim_reference vs the reference golden: rel-rms {err:.3e}")
    assert err < ORACLE_TRAJ_TOL
    assert float((out - case["final"]).abs().max()) < 10 * ORACLE_TRAJ_TOL * float(case["final"].abs().max()) + 1e-6


@pytest.mark.parametrize("tag,name", ddim_cases.ALL_CASES)
def test_ddim_sampler_matches_reference(tag, name):
    """DDIMSampler over the emulated engine in fp32 against the unmodified reference, the reference's noise draws replayed."""
    gold, case, eta, mask, x0, _ = ddim_cases.case_inputs(tag, name)
    _, meta, inp, model, gi, sampler = _setup(tag)
    noises = ddim_cases.used_noises(case, mask is not None)
    drawn = _replay(sampler, noises)
    i0 = _sampler_input(inp, gi)
    # the reference's eta route: make_schedule + ddim_sampling (its sample() always schedules eta 0)
    sampler.make_schedule(ddim_num_steps=meta["S"], ddim_eta=eta)
    out = sampler.ddim_sampling(tuple(inp["x"].shape), i0, inp["uc"], ddim_cases.GUIDANCE, mask=mask, x0=x0)
    assert len(drawn) == len(noises)
    assert [int(v) for v in sampler.ddim_timesteps] == case["ddim_timesteps"].tolist()
    err = cases.rel_rms(out, case["final"])
    print(f"[emulated] {tag} {name}: DDIMSampler fp32 vs the reference golden: rel-rms {err:.3e}")
    assert err < EMUL_TRAJ_TOL
    assert i0["x"] is out and int(i0["timesteps"][0]) == int(sampler.ddim_timesteps[0]) and i0["timesteps"].dtype == torch.long
    calls = model.engine.ops.calls
    assert calls["ddim_update"] == meta["S"] and calls.get("q_sample_blend", 0) == (meta["S"] if mask is not None else 0)


def test_sample_eta_extension_equals_the_make_schedule_route():
    gold, case, eta, mask, x0, noises = ddim_cases.case_inputs("tiny_box_ddim", "eta0.5")
    outs = []
    for route in ("sample", "make_schedule"):
        _, meta, inp, model, gi, sampler = _setup("tiny_box_ddim")
        _replay(sampler, noises)
        if route == "sample":
            outs.append(sampler.sample(meta["S"], tuple(inp["x"].shape), _sampler_input(inp, gi), uc=inp["uc"],
                                       guidance_scale=ddim_cases.GUIDANCE, eta=eta))
        else:
            sampler.make_schedule(meta["S"], ddim_eta=eta)
            outs.append(sampler.ddim_sampling(tuple(inp["x"].shape), _sampler_input(inp, gi), inp["uc"], ddim_cases.GUIDANCE))
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("eta,masked,per_step", [(0.0, False, []), (0.5, False, ["step"]), (0.5, True, ["q_sample", "step"]),
                                                 (0.0, True, ["q_sample"])])
def test_noise_draws_and_their_order(eta, masked, per_step):
    """0 draws at eta 0 without a mask, S at eta > 0, 2 S with a mask in q-sample-then-step order (and, the documented deviation,
    only the S q_sample draws at eta 0 with a mask): recorded through ``noise_fn`` against the ops that consumed them."""
    gold, meta, inp, model, gi, sampler = _setup("tiny_box_ddim")
    ops, log, g = model.engine.ops, [], torch.Generator().manual_seed(7)

    def noise_fn(shape):
        n = torch.randn(tuple(shape), generator=g)
        log.append(("draw", n))
        return n
    sampler.noise_fn = noise_fn
    real_blend, real_update = ops.q_sample_blend, ops.ddim_update

    def blend(x0, noise, *a, **k):
        log.append(("q_sample", noise))
        return real_blend(x0, noise, *a, **k)

    def update(x, e_c, e_u, g_, a_t, a_prev, sigma_t, s1m, noise, out, **k):
        if noise is not None:
            log.append(("step", noise))
        return real_update(x, e_c, e_u, g_, a_t, a_prev, sigma_t, s1m, noise, out, **k)
    ops.q_sample_blend, ops.ddim_update = blend, update
    kw = dict(mask=gold["mask"], x0=gold["x0"]) if masked else {}
    out = sampler.sample(meta["S"], tuple(inp["x"].shape), _sampler_input(inp, gi), uc=inp["uc"], guidance_scale=ddim_cases.GUIDANCE,
                         eta=eta, **kw)
    assert torch.isfinite(out).all()
    draws = [n for kind, n in log if kind == "draw"]
    assert len(draws) == meta["S"] * len(per_step)
    # every draw is consumed by the next op, and the ops of a step come in the reference's order
    assert [kind for kind, _ in log] == [k for _ in range(meta["S"]) for use in per_step for k in ("draw", use)]
    for (k0, n0), (k1, n1) in zip(log[0::2], log[1::2]):
        assert k0 == "draw" and n0 is n1


def test_default_noise_fn_draws_fp32_on_the_engine_device():
    gold, meta, inp, model, gi, sampler = _setup("tiny_box_ddim")
    n = sampler.noise_fn((2, 4, 3, 3))
    assert n.dtype == torch.float32 and tuple(n.shape) == (2, 4, 3, 3) and n.device == model.engine.device


# ---- the shim -----------------------------------------------------------------------------------------------------
def test_ldm_shim_resolves_to_the_host_class_with_the_reference_signatures():
    from ldm.models.diffusion.ddim import DDIMSampler as Shim
    assert Shim is DDIMSampler
    assert list(inspect.signature(Shim.__init__).parameters) == ["self", "diffusion", "model", "schedule", "alpha_generator_func",
                                                                 "set_alpha_scale"]
    p = inspect.signature(Shim.sample).parameters
    assert list(p)[:8] == ["self", "S", "shape", "input", "uc", "guidance_scale", "mask", "x0"]          # ddim.py:58
    assert (p["uc"].default, p["guidance_scale"].default, p["mask"].default, p["x0"].default) == (None, 1, None, None)
    assert list(p)[8:] == ["eta"] and p["eta"].default == 0.
    assert list(inspect.signature(Shim.ddim_sampling).parameters) == ["self", "shape", "input", "uc", "guidance_scale", "mask", "x0"]
    ms = inspect.signature(Shim.make_schedule).parameters
    assert list(ms) == ["self", "ddim_num_steps", "ddim_discretize", "ddim_eta"] and ms["ddim_eta"].default == 0.


# ---- inference.py -------------------------------------------------------------------------------------------------
def test_load_init_image_and_latent_mask(tmp_path):
    import inference
    from PIL import Image
    g = np.random.default_rng(3)
    rgb = g.integers(0, 256, (32, 32, 3), dtype=np.uint8)
    Image.fromarray(rgb).save(tmp_path / "img.png")
    x = inference.load_init_image(str(tmp_path / "img.png"), 32)
    assert x.dtype == torch.float32 and tuple(x.shape) == (1, 3, 32, 32)
    assert torch.equal(x[0], torch.from_numpy(rgb.astype(np.float32)).permute(2, 0, 1) / 127.5 - 1.0)
    assert float(x.min()) >= -1.0 and float(x.max()) <= 1.0
    keep = np.full((32, 32), 255, dtype=np.uint8)
    keep[9, 20] = 0                                   # one black pixel clears its whole 8 x 8 block: latent (1, 2)
    keep[24:, :8] = 127                               # just below the threshold: repaint; 128 keeps
    keep[24:, 8:16] = 128
    Image.fromarray(keep, mode="L").save(tmp_path / "mask.png")
    m = inference.latent_mask(str(tmp_path / "mask.png"), 32)
    want = torch.ones(1, 1, 4, 4)
    want[0, 0, 1, 2] = 0
    want[0, 0, 3, 0] = 0
    assert m.dtype == torch.float32 and torch.equal(m, want)
    for fn, path in ((inference.load_init_image, "img.png"), (inference.latent_mask, "mask.png")):
        with pytest.raises(SystemExit):
            fn(str(tmp_path / path), 64)


@pytest.mark.parametrize("argv", [
    ["--sampler", "ddim"],                                                     # the default --mis is > 0
    ["--sampler", "ddim", "--mis", "0.36"],
    ["--ddim_eta", "0.5", "--mis", "0"],
    ["--sampler", "plms", "--ddim_eta", "0", "--mis", "0"],
    ["--sampler", "ddim", "--mis", "0", "--ddim_eta", "-0.1"],
    ["--mis", "0", "--init_image", "a.png"],
    ["--mis", "0", "--inpaint_mask", "m.png"],
    ["--init_image", "a.png", "--inpaint_mask", "m.png"],                      # inpainting under the default --mis
    ["--init_image", "a.png", "--inpaint_mask", "m.png", "--mis", "0.36"],
])
def test_cli_rejections_come_before_any_model_is_built(monkeypatch, argv):
    import inference
    built = []
    monkeypatch.setattr(inference, "instantiate_from_config", lambda *a, **k: built.append(a) or (_ for _ in ()).throw(AssertionError("built")))
    monkeypatch.setattr(inference, "load_yaml", lambda *a, **k: built.append(a) or {})
    monkeypatch.setattr(sys, "argv", ["inference.py", "--synthetic_weights"] + argv)
    with pytest.raises(SystemExit) as e:
        inference.main()
    assert isinstance(e.value.code, str) and e.value.code, "a message, not an exit status"
    assert not built


# ---- C ABI --------------------------------------------------------------------------------------------------------
def test_argument_validation_without_gpu():
    """Both entry points are exported with a prototype, and every argument error is reported before anything touches a device
    (fake, never dereferenced pointers -- as tests/test_capi.py does for the other entry points)."""
    from instancediffusion_amd import _lib
    lib = _lib.load()
    assert "idf_ddim_update" in _lib.SYMBOLS and "idf_q_sample_blend" in _lib.SYMBOLS and lib.idf_abi_version() == 5
    a_t, a_prev, sigma = ddim_cases.TRIPLES[1]

    def upd(x=0x10000, ec=0x20000, eu=0x30000, a_t=a_t, a_prev=a_prev, sigma=sigma, nz=0x40000, out=0x50000, n=256):
        return lib.idf_ddim_update(x, ec, eu, 7.5, a_t, a_prev, sigma, 0.76, nz, out, None, n, None)
    assert [upd(x=None), upd(ec=None), upd(out=None), upd(n=0), upd(a_t=0.0), upd(a_t=-1.0), upd(a_prev=-0.5), upd(sigma=-0.5),
            upd(a_prev=0.9, sigma=0.5), upd(nz=None), upd(a_t=float("nan"))] == [-1] * 11

    def blend(x0=0x10000, nz=0x20000, mask=0x30000, img=0x40000, out=0x50000, B=2, Cc=4, HW=32, mc=1):
        return lib.idf_q_sample_blend(x0, nz, mask, img, 0.6, 0.8, out, B, Cc, HW, mc, None)
    assert [blend(x0=None), blend(nz=None), blend(mask=None), blend(img=None), blend(out=None), blend(B=0), blend(Cc=0), blend(HW=0),
            blend(mc=0), blend(mc=2), blend(mc=5)] == [-1] * 11
