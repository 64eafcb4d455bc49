"""img2img starts and the hi-res second pass on a real MI355X: the HIP engine (hipGraph replay keyed by shape, ``idf_q_sample``,
``idf_resize_planes``, the samplers' ``sample_from``) on the reduced model and the tiny_box inputs at S = 5, CFG 7.5, against the composed
CPU oracles of tests/hires_cases.py; one engine at two resolutions, interleaved; ``inference.py --strength`` / ``--hires_scale`` end to end.

Bar: the rule of tests/test_ddim_sampler_gpu.py, ``max(TRAJ_TOL[dtype], 1.25 x floor)``, ``floor`` = the oracle's OWN autocast error on the
SAME trajectory (tests/golden/hires_floor.pt, tests/make_hires_golden.py).  Every case prints a "[parity]" line.
"""
import functools
import os
import sys
from functools import partial

import pytest
import torch

from tests import hires_cases as hc
from tests.test_ddim_sampler_gpu import FLOOR_KEY, TRAJ_TOL

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = {"plms": {}, "ddim": dict(eta=0.0), "dpmpp": dict(order=2)}


def _cuda(d):
    return {k: v.cuda() for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def _case():
    from tests import cases
    meta = cases.load_golden(hc.TAG)["meta"]
    assert (meta["S"], meta["batch"], meta["latent"]) == (hc.S, 2, 16)
    return meta, cases.build_inputs(meta)


@functools.lru_cache(maxsize=None)
def _floors():
    gold = torch.load(os.path.join(hc.GOLD, hc.FLOOR_GOLDEN), weights_only=False)
    m = gold["meta"]
    assert (m["tag"], m["S"], m["guidance"], m["strength"], m["start"], tuple(m["size"]), m["seed"]) == \
        (hc.TAG, hc.S, hc.GUIDANCE, hc.STRENGTH, hc.START, hc.HIRES_SIZE, hc.SEED), "hires_floor.pt was made for other settings"
    return gold["floors"]


def _sampler(kind, dtype):
    from instancediffusion_amd import synth
    from instancediffusion_amd.host.alpha import alpha_generator, set_alpha_scale
    from instancediffusion_amd.host.diffusion import LatentDiffusion
    from instancediffusion_amd.host.samplers import DDIMSampler, DPMSolverSampler, PLMSSampler
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
    cls = {"plms": PLMSSampler, "ddim": DDIMSampler, "dpmpp": DPMSolverSampler}[kind]
    return cls(diffusion, model, alpha_generator_func=partial(alpha_generator, type=meta["alpha_type"]), set_alpha_scale=set_alpha_scale), gi


def _input(gi, x=None):
    meta, inp = _case()
    return dict(x=(inp["x"] if x is None else x).cuda(), timesteps=None, context=inp["context"].cuda(), grounding_input=gi.prepare(_cuda(inp["gb"])))


@functools.lru_cache(maxsize=None)
def _reference(case, kind):
    """The composed oracle's result: computed once on the CPU in fp32, shared by the dtypes, left unchanged."""
    from instancediffusion_amd import synth
    from oracle import ref_cpu
    from tests import cases
    meta, inp = _case()
    cfg = cases.cfg_for(meta["cfg"], meta["variant"])
    shape = tuple(inp["x"].shape)
    with torch.no_grad():
        model = ref_cpu.OracleModel(synth.synth_state_dict(cases.unet_schema(cfg)), cfg, synth.synth_first_conv_sd())
        base = dict(x=inp["x"].clone(), timesteps=None, context=inp["context"], grounding_input=ref_cpu.prepare_grounding(inp["gb"]))
        if case == "img2img":
            x0, noise = hc.case_tensors("img2img", shape)
            return hc.img2img_reference(kind, model, base, inp["uc"], x0, noise, alpha_type=meta["alpha_type"])
        return hc.hires_reference(kind, model, base, inp["uc"], hc.case_tensors("hires", shape), alpha_type=meta["alpha_type"])[1]


def _run(case, kind, sampler, gi):
    from instancediffusion_amd.host import hires
    meta, inp = _case()
    shape = tuple(inp["x"].shape)
    uc = inp["uc"].cuda()
    if case == "img2img":
        x0, noise = hc.case_tensors("img2img", shape)
        x, start = hires.noised_start(sampler, x0.cuda(), hc.S, hc.STRENGTH, noise.cuda(), **KW[kind])
        assert start == hc.START
        return sampler.sample_from(hc.S, shape, _input(gi, x), start, uc=uc, guidance_scale=hc.GUIDANCE, **KW[kind])
    i1 = _input(gi)
    first = sampler.sample(hc.S, shape, i1, uc=uc, guidance_scale=hc.GUIDANCE, **KW[kind])
    return hires.hires_pass(sampler, first, i1, uc, hc.GUIDANCE, hc.S, hc.STRENGTH, hc.HIRES_SIZE, "bicubic",
                            hc.case_tensors("hires", shape).cuda(), **KW[kind])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("kind", hc.SAMPLERS)
@pytest.mark.parametrize("case", hc.CASES)
def test_matches_the_composed_reference(case, kind, dtype):
    """img2img from a seeded x0 at strength 0.6 (start 2), and a first pass + ``hires_pass`` 16^2 -> 24^2 at strength 0.6, for PLMS, DDIM
    eta 0 and DPM-Solver++ order 2."""
    from tests import cases
    want = _reference(case, kind)
    sampler, gi = _sampler(kind, dtype)
    out = _run(case, kind, sampler, gi)
    floor = float(_floors()[case][kind][FLOOR_KEY[dtype]])
    tol = max(TRAJ_TOL[dtype], 1.25 * floor)
    err = cases.rel_rms(out.cpu(), want)
    print(f"[parity] tiny_box {case} {kind} S={hc.S} strength {hc.STRENGTH} CFG7.5 {dtype}: latent rel-rms {err:.3e} (tol {tol:.2e}; the "
          f"oracle's own autocast error on this trajectory {floor:.2e})")
    assert tuple(out.shape) == tuple(want.shape) and torch.isfinite(out).all() and err < tol


def test_one_engine_at_two_resolutions_interleaved():
    """16^2, then 24^2, then 16^2 again on ONE engine (its buffers are keyed by shape, its graphs by (B, H, W, fuser, paired)): the two
    16^2 results equal each other and a fresh engine's, the 24^2 result equals a fresh engine's -- bit for bit."""
    meta, inp = _case()
    uc = inp["uc"].cuda()
    x24 = hc.seeded((2, 4) + hc.HIRES_SIZE).cuda()

    def at16(sampler, gi):
        return sampler.sample(hc.S, tuple(inp["x"].shape), _input(gi), uc=uc, guidance_scale=hc.GUIDANCE, eta=0.0).clone()

    def at24(sampler, gi):
        return sampler.sample_from(hc.S, tuple(x24.shape), _input(gi, x24), hc.START, uc=uc, guidance_scale=hc.GUIDANCE, eta=0.0).clone()
    sampler, gi = _sampler("ddim", torch.bfloat16)
    a16, a24, b16 = at16(sampler, gi), at24(sampler, gi), at16(sampler, gi)
    fresh16 = at16(*_sampler("ddim", torch.bfloat16))
    fresh24 = at24(*_sampler("ddim", torch.bfloat16))
    assert torch.isfinite(a16).all() and torch.isfinite(a24).all()
    assert torch.equal(a16, b16) and torch.equal(a16, fresh16) and torch.equal(a24, fresh24)


# ---- inference.py -------------------------------------------------------------------------------------------------------
def _reduced_config(tmp_path):
    """configs/test_box.yaml with the reduced UNet of the tiny goldens at 16 x 16 latents (128-pixel images); the VAE stays as it is.
    The runs use --alpha 1.0: the gate never reaches 0, the reduced model (64 channels) cannot take Stable Diffusion's first conv."""
    import yaml
    cfg = yaml.safe_load(open(os.path.join(REPO, "configs", "test_box.yaml")))
    p = cfg["model"]["params"]
    p["image_size"], p["model_channels"] = 16, 64
    p["grounding_tokenizer"]["params"]["mid_dim"] = 256
    path = tmp_path / "reduced_box.yaml"
    path.write_text(yaml.safe_dump(cfg))
    return str(path)


def _run_cli(monkeypatch, tmp_path, extra):
    import inference
    out_dir = tmp_path / "OUT"
    argv = ["inference.py", "--synthetic_weights", "--num_images", "2", "--steps", "5", "--seed", "3", "--alpha", "1.0",
            "--input_json", os.path.join(REPO, "demos", "demo_four_boxes.json"), "--test_config", _reduced_config(tmp_path),
            "--output", str(out_dir), "--save_latents", "--dtype", "bf16"] + extra
    monkeypatch.setattr(sys, "argv", argv)
    monkeypatch.chdir(REPO)
    inference.main()
    folder = out_dir / "gc7.5-seed3-alpha1.0"
    pngs = sorted(p for p in os.listdir(folder) if p.endswith(".png"))
    return folder, pngs, torch.load(folder / "latents.pt")


def test_cli_hires_scale_writes_larger_images(tmp_path, monkeypatch):
    """The default sampler (PLMS under the Multi-instance Sampler, --mis 0.36) at 16^2, then the second pass at 24^2: 192-pixel PNGs."""
    from PIL import Image
    folder, pngs, saved = _run_cli(monkeypatch, tmp_path, ["--hires_scale", "1.5"])
    assert len(pngs) == 2 and all(Image.open(folder / p).size == (192, 192) for p in pngs)
    lat, lat1 = saved["latents"].float(), saved["latents_pass1"].float()
    assert tuple(lat.shape) == (2, 4, 24, 24) and tuple(lat1.shape) == (2, 4, 16, 16)
    assert torch.isfinite(lat).all() and torch.isfinite(lat1).all() and float(lat.std()) > 0


def test_cli_img2img_writes_its_images(tmp_path, monkeypatch):
    import numpy as np
    from PIL import Image
    g = np.random.default_rng(5)
    ramp = np.linspace(0, 255, 128, dtype=np.float32)
    rgb = np.stack([ramp[None, :].repeat(128, 0), ramp[:, None].repeat(128, 1), g.uniform(0, 255, (128, 128)).astype(np.float32)], -1)
    Image.fromarray(rgb.astype(np.uint8)).save(tmp_path / "init.png")
    folder, pngs, saved = _run_cli(monkeypatch, tmp_path, ["--init_image", str(tmp_path / "init.png"), "--strength", "0.5"])
    assert len(pngs) == 2 and all(Image.open(folder / p).size == (128, 128) for p in pngs)
    lat = saved["latents"].float()
    assert tuple(lat.shape) == (2, 4, 16, 16) and torch.isfinite(lat).all() and float(lat.std()) > 0 and "latents_pass1" not in saved
