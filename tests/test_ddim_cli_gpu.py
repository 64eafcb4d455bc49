"""``inference.py --sampler ddim`` and the inpainting flags end to end on a real MI355X, in process, as tests/test_inference_cli_gpu.py
runs the PLMS entry point.

The deterministic run (eta 0) is compared with ``tests/ddim_cases.ddim_reference`` over the CPU oracle model (``oracle/ref_cpu.py``,
pinned to the reference's goldens; ``ddim_reference`` itself is pinned to the reference's DDIM goldens by tests/test_ddim_host.py)
on the same meta, starting noise and weights.  That side is a committed fixture, ``tests/golden/cli_ddim_latents.pt``
(``python tests/make_cli_ddim_latents.py``: eight full-size CPU forwards); ``IDF_CLI_LIVE_ORACLE=1`` runs it live instead.
"""
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG, INPUT_JSON = "test_box.yaml", "demos/demo_four_boxes.json"
# 4 steps: the smallest count near 3 the uniform discretisation takes -- at S = 3 make_ddim_timesteps (util.py:55-69) yields
# range(0, 1000, 333) + 1 = [1, 334, 667, 1000], four steps whose last indexes alphas_cumprod[1000] out of bounds, in the reference too
STEPS, ALPHA, SEED, ETA = 4, 0.8, 3, 0.0
DEFAULT_NEG = ("longbody, lowres, bad anatomy, bad hands, missing fingers, extra digit, fewer digits, cropped, worst quality, "
               "low quality")                      # inference.py's --negative_prompt default (reference inference.py:171)
FIXTURE = os.path.join(REPO, "tests", "golden", "cli_ddim_latents.pt")


def _oracle_latent():
    """The pipeline of ``inference.main() --sampler ddim --mis 0 --num_images 1`` on the CPU oracle: (latent, n_forward)."""
    import inference
    from instancediffusion_amd import synth
    from instancediffusion_amd.host.input import meta_from_demo_json, prepare_batch
    from oracle import ref_cpu
    from tests import cases, ddim_cases
    cfg = cases.cfg_for(CFG, "full")
    om = ref_cpu.OracleModel(synth.synth_state_dict(cases.unet_schema(cfg)), cfg, synth.synth_first_conv_sd())
    meta = meta_from_demo_json(json.load(open(os.path.join(REPO, INPUT_JSON))), ALPHA)
    enc = inference.SyntheticTextEncoder()
    torch.manual_seed(SEED)
    x = torch.randn(1, 4, 64, 64)
    batch = prepare_batch(meta, batch=1, max_objs=inference.MAX_OBJS, model=enc, processor=None, image_size=64, device="cpu")
    inp = dict(x=x.clone(), timesteps=None, context=enc.encode([meta["prompt"]]), grounding_input=ref_cpu.prepare_grounding(batch))
    with torch.no_grad():
        # eta 0: every sigma is zero, the draws (zeros here) are multiplied away as in the reference
        lat = ddim_cases.ddim_reference(om, STEPS, inp, enc.encode([DEFAULT_NEG]), 7.5, eta=ETA, alpha_type=meta["alpha_type"],
                                        noises=[torch.zeros_like(x)] * STEPS)
    return lat, om.n_forward


def _want():
    if os.environ.get("IDF_CLI_LIVE_ORACLE") == "1":
        return _oracle_latent() + ("run live",)
    fx = torch.load(FIXTURE)
    assert (fx["steps"], fx["alpha"], fx["seed"], fx["eta"], fx["negative_prompt"], fx["cfg"], fx["input_json"]) == \
        (STEPS, ALPHA, SEED, ETA, DEFAULT_NEG, CFG, INPUT_JSON), "cli_ddim_latents.pt was made for other settings: re-run tests/make_cli_ddim_latents.py"
    return fx["latent"], fx["n_forward"], "fixture"


def _run_cli(monkeypatch, out_dir, extra):
    import inference
    argv = ["inference.py", "--synthetic_weights", "--num_images", "1", "--steps", str(STEPS), "--mis", "0", "--alpha", str(ALPHA),
            "--seed", str(SEED), "--input_json", os.path.join(REPO, INPUT_JSON), "--test_config", os.path.join(REPO, "configs", CFG),
            "--output", str(out_dir), "--save_latents", "--dtype", "bf16", "--sampler", "ddim"] + extra
    monkeypatch.setattr(sys, "argv", argv)
    monkeypatch.chdir(REPO)
    inference.main()
    folder = out_dir / f"gc7.5-seed{SEED}-alpha{ALPHA}"
    pngs = sorted(p for p in os.listdir(folder) if p.endswith(".png"))
    lat = torch.load(folder / "latents.pt")["latents"].float()
    assert tuple(lat.shape) == (1, 4, 64, 64) and torch.isfinite(lat).all()
    return folder, pngs, lat


def test_ddim_cli_end_to_end_matches_oracle(tmp_path, monkeypatch):
    import numpy as np
    from PIL import Image
    from tests import cases
    folder, pngs, lat = _run_cli(monkeypatch, tmp_path / "OUT", [])
    assert len(pngs) == 1
    img = Image.open(folder / pngs[0])
    assert img.size == (512, 512) and img.mode == "RGB"
    assert float(np.asarray(img, dtype=np.float32).std()) > 1.0, "a constant image means the decode path did nothing"
    want, n_fwd, src = _want()
    err = cases.rel_rms(lat, want)
    print(f"[parity] inference.py --sampler ddim end to end ({CFG}, S={STEPS}, eta 0, mis 0): latent rel-rms {err:.3e} vs ddim_reference "
          f"over the CPU oracle ({n_fwd} oracle forwards, {src}; tol 5e-2)")
    assert err < 5e-2


def test_ddim_cli_inpainting_runs(tmp_path, monkeypatch):
    """--ddim_eta 0.5 --init_image --inpaint_mask: ``AutoencoderKL.encode`` feeds x0, the left half of the image is kept."""
    import numpy as np
    from PIL import Image
    g = np.random.default_rng(5)
    ramp = np.linspace(0, 255, 512, dtype=np.float32)
    rgb = np.stack([ramp[None, :].repeat(512, 0), ramp[:, None].repeat(512, 1), g.uniform(0, 255, (512, 512)).astype(np.float32)], -1)
    Image.fromarray(rgb.astype(np.uint8)).save(tmp_path / "init.png")
    keep = np.zeros((512, 512), dtype=np.uint8)
    keep[:, :256] = 255
    Image.fromarray(keep, mode="L").save(tmp_path / "mask.png")
    folder, pngs, lat = _run_cli(monkeypatch, tmp_path / "OUT", ["--ddim_eta", "0.5", "--init_image", str(tmp_path / "init.png"),
                                                                  "--inpaint_mask", str(tmp_path / "mask.png")])
    assert len(pngs) == 1 and Image.open(folder / pngs[0]).size == (512, 512)
    assert float(lat.std()) > 0
