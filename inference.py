#!/usr/bin/env python
"""Entry-point mirror of the reference ``inference.py`` (demo CLI) on the MI355X path.

Same flags, same demo-JSON format (``demos/*.json``: caption, width/height, annos[{bbox, mask, point, scribble,
caption}]) and the same call sequence as the reference (inference.py:165-309): demo JSON -> ``meta`` ->
``utils.input.prepare_batch`` (+ ``prepare_instance_meta`` per instance when MIS is on) -> ``PLMSSampler`` /
``PLMSSamplerInst`` -> ``autoencoder.decode`` -> PNGs.  UNet, samplers and VAE decoder run on the HIP engine.

Beyond the reference's flags: ``--sampler ddim`` (+ ``--ddim_eta``) runs ``DDIMSampler`` (ldm/models/diffusion/ddim.py) instead of
``PLMSSampler``, and ``--init_image`` / ``--inpaint_mask`` reach the samplers' ``mask`` / ``x0`` arguments (plms.py:99-104,
ddim.py:94-98): the image is encoded by ``AutoencoderKL.encode``, the mask is pooled to the latent grid.  ``--sampler ddim_inst`` runs
``DDIMSamplerInst``, the Multi-instance Sampler (``--mis`` > 0) on DDIM steps: ``--ddim_eta`` and inpainting work under it, with one or
several ``--input_json`` (the one image / mask pair then applies to every layout).  ``--sampler dpmpp`` (``--mis 0``) and ``dpmpp_inst``
(``--mis`` > 0) run DPM-Solver++(2M) -- ``DPMSolverSampler`` / ``DPMSolverSamplerInst``, ``--dpm_order``, ``--dpm_spacing`` -- meant for
20-25 ``--steps``; inpainting and several ``--input_json`` work under both, ``--ddim_eta`` under neither.

Two neighbours of the path need assets that do not exist offline; both are handled explicitly, never silently:
  * text encoding (CLIP-L/14: ``ldm/modules/encoders``, ``utils/model.py:12-18``): with ``--ckpt`` the checkpoint's
    text encoder is used (needs the BPE vocabulary locally, see host/text_encoder.py); ``--text_encoder synthetic``
    (default without a checkpoint) draws a deterministic embedding per string -- layout-faithful, not meaningful;
  * weights: ``--ckpt instancediffusion_sd15.pth`` goes through ``utils.checkpoint.load_model_ckpt`` (ema -> model
    fallback, autoencoder / text_encoder / diffusion sub-dicts); without it ``--synthetic_weights`` must be given.
The SDXL-refiner cascade (``--cascade_strength``, diffusers + downloads) is outside the path.

``--init_image`` with ``--strength F`` and no mask is img2img: the picture is encoded, noised to the timestep of step
``S - floor(S F)`` and denoised from there (``host/hires.noised_start`` + ``sample_from``).  ``--hires_scale F`` adds a latent hi-res second
pass behind any first pass: the finished latents are enlarged on the device (``idf_resize_planes``), noised ``--hires_strength`` of
the way back and the tail of the schedule is denoised at the larger size with the same conditioning (``host/hires.hires_pass``); the
decoder then writes ``8 round(image_size F)``-pixel PNGs.  Both run the single-trajectory sampler that matches ``--sampler`` on the global
input; with ``--mis`` > 0 they must enter the schedule behind the Multi-instance phase (strength <= 1 - mis).  Image quality of either
cannot be judged on ``--synthetic_weights``.

``--instance_masks json`` makes the JSON's ``mask`` entries (COCO run-length masks) condition generation, as the reference's
``eval_local.py`` route does (utils/input.py:161-186); the reference's ``inference.py`` decodes them and throws them away (:249), which
stays the default (``ignore``).  The masks are decoded and resized on the device (``idf_rle_decode_planes``): only run lengths are uploaded.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
from functools import partial

import torch

from instancediffusion_amd.host.alpha import alpha_generator, set_alpha_scale
from instancediffusion_amd.host.config import instantiate_from_config, load_yaml
from instancediffusion_amd.host.input import meta_from_demo_json, prepare_batch, prepare_instance_meta, prepare_layout_inputs
from instancediffusion_amd.host.samplers import (DDIMSampler, DDIMSamplerInst, DPMSolverSampler, DPMSolverSamplerInst, PLMSSampler,
                                                  PLMSSamplerInst)

MAX_OBJS = 30


def text_embedding(s: str, dim: int = 768, rows: int = 1) -> torch.Tensor:
    g = torch.Generator().manual_seed(int.from_bytes(hashlib.sha256(s.encode()).digest()[:7], "little"))
    return torch.randn(rows, dim, generator=g)


class SyntheticTextEncoder:
    """Stand-in for FrozenCLIPEmbedder.encode (encoders/modules.py:144-172) and for the pooled CLIP phrase feature
    (utils/model.py:130-152): deterministic per string."""

    def encode(self, prompts):
        return torch.stack([text_embedding("ctx:" + p, 768, 77) for p in prompts])

    def pooled(self, phrase):
        return text_embedding("pooled:" + phrase, 768, 1)[0]


class ClipPhraseEncoder:
    """Pooled phrase features from the checkpoint's own CLIP text transformer (the reference loads a second copy of
    the same CLIP-L/14 text model through ``CLIPModel``; its pooler output is the same tensor)."""

    def __init__(self, text_encoder):
        self.text_encoder = text_encoder

    def pooled(self, phrase):
        return self.text_encoder.encode([phrase], return_pooler_output=True)[1][0]


def get_model_inputs(meta, gi, text_encoder, phrase_encoder, num_images, device, starting_noise, negative_prompt=None,
                     instance_input=False, use_masked_att=False, batch=None):
    """inference.py:39-78.  ``use_masked_att``: also build the box-shaped visibility planes and hand them to the model
    (``eval_local.py --use_masked_att``; the reference's inference.py builds them but never passes them on).  ``batch``: the
    ``prepare_batch`` result when the caller already has it (``--instance_masks json`` prepares all rows in one call)."""
    if batch is None:
        batch = prepare_batch(meta, batch=num_images, max_objs=MAX_OBJS, model=phrase_encoder, processor=None,
                              image_size=starting_noise.shape[-1], use_masked_att=use_masked_att, device=device)
    context = text_encoder.encode([meta["prompt"]] * num_images).to(device)
    uc = None
    if not instance_input:
        uc = text_encoder.encode(num_images * [negative_prompt if negative_prompt is not None else ""]).to(device)
    grounding_input = gi.prepare(batch, return_att_masks=use_masked_att)
    return dict(x=starting_noise, timesteps=None, context=context, grounding_input=grounding_input), uc


def save_images(images: torch.Tensor, folder: str) -> list:
    """inference.py:120-130: clamp to [-1, 1], map to uint8 RGB, one PNG per sample (numbered after existing files)."""
    import numpy as np
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    start = len(os.listdir(folder))
    names = []
    for i, sample in enumerate(images):
        sample = torch.clamp(sample, min=-1, max=1) * 0.5 + 0.5
        arr = (sample.float().cpu().numpy().transpose(1, 2, 0) * 255).astype(np.uint8)
        name = os.path.join(folder, f"{start + i}.png")
        Image.fromarray(arr).save(name)
        names.append(name)
    return names


def _open_sized(path: str, size: int, mode: str):
    from PIL import Image
    img = Image.open(path).convert(mode)
    if img.size != (size, size):
        raise SystemExit(f"{path} is {img.size[0]} x {img.size[1]}: the model samples {size} x {size} images (8 x its latent size)")
    return img


def load_init_image(path: str, size: int) -> torch.Tensor:
    """``--init_image``: an RGB image of size x size -> fp32 [1, 3, size, size] in [-1, 1] (v / 127.5 - 1), the encoder's input."""
    import numpy as np
    arr = np.asarray(_open_sized(path, size, "RGB"), dtype=np.float32)
    return (torch.from_numpy(arr.copy()).permute(2, 0, 1) / 127.5 - 1.0).unsqueeze(0).contiguous()


def latent_mask(path: str, size: int) -> torch.Tensor:
    """``--inpaint_mask``: a grey-scale image of size x size, a pixel >= 128 means "keep the original" -> fp32 [1, 1, size / 8,
    size / 8] of {0, 1}: a latent pixel keeps the original only if all of its 8 x 8 pixels do (min-pool), so that nothing the user
    asked to repaint is held to the original."""
    import numpy as np
    keep = torch.from_numpy((np.asarray(_open_sized(path, size, "L")) >= 128).astype(np.float32))
    return -torch.nn.functional.max_pool2d(-keep[None, None], 8)


def clip_scores(args, images: torch.Tensor, data: dict, dtype, input_json=None, loaded=None) -> dict:
    """``--clip_score``: the local CLIP score (host/clip_score.py) of every instance of every decoded image, straight from the fp32
    decoder output -- on backend ``hip`` the pixels never leave the device (``idf_clip_crop_resize`` quantises them as
    ``save_images`` does).  -> the content of ``clip_scores.json``."""
    from instancediffusion_amd.host import clip_score as cs
    boxes, phrases = cs.instances_from_demo_json(data)
    if loaded is None or "scorer" not in loaded:                  # ``loaded``: a dict that keeps the model over several layouts
        model, tokenize, tokenizer = cs.load_clip(args.clip_path)
        scorer = cs.InstanceClipScorer(model.to(images.device), tokenize, backend=args.clip_score, dtype=dtype)
        if loaded is not None:
            loaded.update(scorer=scorer, tokenizer=tokenizer)
    else:
        scorer, tokenizer = loaded["scorer"], loaded["tokenizer"]
    scores = scorer.score_batch(images.float(), boxes, phrases)
    means, ranking = cs.rank_by_mean(scores)
    return dict(metric="local CLIP score (eval_attribute_binding.py, HF branch)", input_json=input_json or args.input_json, backend=args.clip_score,
                dtype=args.dtype if args.clip_score == "hip" else "fp32", tokenizer=tokenizer,
                weights=args.clip_path or "synthetic", phrases=phrases,
                images={str(i): [round(v, 6) for v in s] for i, s in enumerate(scores)},
                means={str(i): round(m, 6) for i, m in enumerate(means)}, ranking=ranking,
                mean=round(sum(means) / len(means), 6))


def report_masks(path: str, areas) -> None:
    """``--instance_masks json``: one line per layout -- how many instances carried a mask, and which masks are empty."""
    have = [i for i, a in enumerate(areas) if a >= 0]
    empty = [i for i in have if areas[i] == 0]
    print(f"masks {path}: {len(have)} of {len(areas)} instances carry a mask"
          + (f"; area 0 (no conditioning): instances {empty}" if empty else "; none is empty"))


def refuse_dropped_masks(args, model) -> None:
    if args.instance_masks == "json" and model.position_net.eval_drops()[4]:
        raise SystemExit(f"--instance_masks json: the model config ({args.test_config}) drops masks (test_drop_masks), so the JSON's "
                         "masks would do nothing; use a config that keeps them (configs/test_mask.yaml)")


def layout_folders(paths) -> list:
    """Output folder name per input JSON: its stem; a stem seen before gets a numeric suffix (a.json, x/a.json -> a, a_2)."""
    seen, out = {}, []
    for p in paths:
        stem = os.path.splitext(os.path.basename(p))[0]
        seen[stem] = seen.get(stem, 0) + 1
        out.append(stem if seen[stem] == 1 else f"{stem}_{seen[stem]}")
    return out


def load_inpaint(args, model, autoencoder, dev):
    """``--init_image`` / ``--inpaint_mask`` -> (keep mask [1, 1, h, w], x0 [1, 4, h, w]) on the device, or None."""
    if args.init_image is None:
        return None
    size = 8 * model.image_size
    image, keep = load_init_image(args.init_image, size), latent_mask(args.inpaint_mask, size)
    # the posterior sample times scale_factor (autoencoder.py:27-31), its noise the next draw of the CPU default generator
    return keep.to(dev), autoencoder.encode(image.to(dev))


def hires_side(image_size: int, scale: float) -> int:
    """``--hires_scale``: the second pass's latent side, ``round(image_size * scale)``; it must be a multiple of 8 (three stride-2
    levels in the UNet, 8 x 8 pixels per latent in the decoder) and larger than ``image_size``."""
    side = int(round(image_size * scale))
    if not scale > 1 or side <= image_size:
        raise SystemExit(f"--hires_scale must be > 1 (and enlarge the {image_size} x {image_size} latents), got {scale}")
    if side % 8:
        lo, hi = side // 8 * 8, side // 8 * 8 + 8
        near = [f"{v / image_size:g} ({v} x {v} latents)" for v in (lo, hi) if v > image_size]
        raise SystemExit(f"--hires_scale {scale}: the second pass would run {side} x {side} latents, not a multiple of 8; the nearest valid "
                         f"scales are {' and '.join(near)}")
    return side


def single_sampler(args, diffusion, model, ag):
    """The single-trajectory sampler that matches ``--sampler`` and the keywords of its ``sample`` / ``sample_from``: what an img2img
    start and the hi-res second pass run, on the global input."""
    kw = dict(alpha_generator_func=ag, set_alpha_scale=set_alpha_scale)
    if args.sampler in ("ddim", "ddim_inst"):
        return DDIMSampler(diffusion, model, **kw), dict(eta=args.ddim_eta or 0.)
    if args.sampler in ("dpmpp", "dpmpp_inst"):
        return DPMSolverSampler(diffusion, model, **kw), dict(order=args.dpm_order, discretize=args.dpm_spacing)
    return PLMSSampler(diffusion, model, **kw), {}


def refuse_start_inside_mis(flag: str, S: int, strength: float, mis: float) -> None:
    """A run that enters the S-step schedule behind the Multi-instance phase IS the single-trajectory sampler on the global input; one
    that would enter inside it is refused (not built)."""
    from instancediffusion_amd.host.hires import steps_for_strength
    start, _ = steps_for_strength(S, strength)
    if mis > 0 and start < int(S * mis):
        raise SystemExit(f"{flag} {strength} with --mis {mis}: the run would enter the {S}-step schedule at step {start}, inside the "
                         f"Multi-instance phase (steps 0 .. {int(S * mis) - 1}); the limit is strength <= 1 - mis = {1 - mis:g} "
                         "(or give --mis 0)")


def run_layouts(args, paths, model, autoencoder, diffusion, gi, text_encoder, phrase_encoder, dev, dtype):
    """Several ``--input_json``: different layouts, ``--num_images`` images each, sampled in ONE batch (``sample_layouts``; with
    ``--mis 0`` one row-stacked ``PLMSSampler`` / ``DDIMSampler`` call).  Every layout gets the starting noise a single-JSON run
    with the same ``--seed`` draws, the negative prompt is shared, and layout l is written to
    OUTPUT/<save_folder_name>/<json stem>/ with its own ``latents.pt`` / ``clip_scores.json``; ``--keep_best`` applies per layout."""
    datas = [json.load(open(p)) for p in paths]
    save_folder_name = f"gc{args.guidance_scale}-seed{args.seed}-alpha{args.alpha}"
    metas = [meta_from_demo_json(d, args.alpha, ckpt=args.ckpt, save_folder_name=save_folder_name, instance_masks=args.instance_masks)
             for d in datas]
    ops = model.engine.ops if args.instance_masks == "json" else None      # the masks are decoded on the device
    torch.manual_seed(args.seed)
    starting_noise = torch.randn(args.num_images, 4, model.image_size, model.image_size).to(dev)
    noises = [starting_noise] * len(paths)
    uc = text_encoder.encode([args.negative_prompt if args.negative_prompt is not None else ""]).to(dev)
    ag = partial(alpha_generator, type=metas[0]["alpha_type"])
    K = args.num_images
    if args.mis > 0:
        extra = {}
        if args.sampler == "ddim_inst":
            sampler = DDIMSamplerInst(diffusion, model, alpha_generator_func=ag, set_alpha_scale=set_alpha_scale, mis=args.mis)
            extra["eta"] = args.ddim_eta or 0.
            inpaint = load_inpaint(args, model, autoencoder, dev)
            if inpaint is not None:                                        # the one image / mask pair applies to every layout
                extra.update(masks=[inpaint[0]] * len(paths), x0s=[inpaint[1]] * len(paths))
        elif args.sampler == "dpmpp_inst":
            sampler = DPMSolverSamplerInst(diffusion, model, alpha_generator_func=ag, set_alpha_scale=set_alpha_scale, mis=args.mis)
            extra.update(order=args.dpm_order, discretize=args.dpm_spacing)
            inpaint = load_inpaint(args, model, autoencoder, dev)
            if inpaint is not None:
                extra.update(masks=[inpaint[0]] * len(paths), x0s=[inpaint[1]] * len(paths))
        else:
            sampler = PLMSSamplerInst(diffusion, model, alpha_generator_func=ag, set_alpha_scale=set_alpha_scale, mis=args.mis)
        layouts = prepare_layout_inputs(metas, noises, gi, text_encoder, phrase_encoder, instances=True, max_objs=MAX_OBJS, device=dev,
                                        ops=ops)
        areas = [lay[0].get("mask_areas") for lay in layouts]
        try:
            samples = sampler.sample_layouts(S=args.steps, layouts=layouts, uc=uc, guidance_scale=args.guidance_scale, **extra)
        except ValueError as e:
            raise SystemExit(str(e))
    else:
        inp = prepare_layout_inputs(metas, noises, gi, text_encoder, phrase_encoder, instances=False, max_objs=MAX_OBJS, device=dev,
                                    ops=ops)
        areas = inp.get("mask_areas", [None] * len(paths))
        n = K * len(paths)
        extra = {}
        if args.sampler == "ddim":
            sampler = DDIMSampler(diffusion, model, alpha_generator_func=ag, set_alpha_scale=set_alpha_scale)
            extra["eta"] = args.ddim_eta or 0.
        elif args.sampler == "dpmpp":
            sampler = DPMSolverSampler(diffusion, model, alpha_generator_func=ag, set_alpha_scale=set_alpha_scale)
            extra.update(order=args.dpm_order, discretize=args.dpm_spacing)
            inpaint = load_inpaint(args, model, autoencoder, dev)
            if inpaint is not None:                                        # the one image / mask pair applies to every row
                extra.update(mask=inpaint[0].expand(n, -1, -1, -1), x0=inpaint[1].expand(n, -1, -1, -1))
        else:
            sampler = PLMSSampler(diffusion, model, alpha_generator_func=ag, set_alpha_scale=set_alpha_scale)
        samples = sampler.sample(S=args.steps, shape=(n, model.in_channels, model.image_size, model.image_size), input=inp,
                                 uc=uc.expand(n, -1, -1), guidance_scale=args.guidance_scale, **extra)
    if args.instance_masks == "json":
        for path, meta, a in zip(paths, metas, areas):
            report_masks(path, a if a is not None else [-1] * len(meta["phrases"]))
    loaded = {}
    for l, (path, stem) in enumerate(zip(paths, layout_folders(paths))):
        lat = samples[l * K:(l + 1) * K]
        images = autoencoder.decode(lat)
        folder = os.path.join(args.output, save_folder_name, stem)
        report = None
        if args.clip_score:
            report = clip_scores(args, images, datas[l], dtype, input_json=path, loaded=loaded)
            if args.keep_best is not None:
                images = images[report["ranking"][:args.keep_best]]
        names = save_images(images, folder)
        if report is not None:
            kept = report["ranking"][:args.keep_best] if args.keep_best is not None else list(range(len(names)))
            report["saved"] = {os.path.basename(n): i for n, i in zip(names, kept)}
            with open(os.path.join(folder, "clip_scores.json"), "w") as f:
                f.write(json.dumps(report, indent=1) + "\n")
        if args.save_latents:
            torch.save(dict(latents=lat.cpu(), caption=datas[l]["caption"], phrases=metas[l]["phrases"]),
                       os.path.join(folder, "latents.pt"))
        print(f"saved {len(names)} images {tuple(images.shape[1:])} to {folder}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--output", type=str, default="OUTPUT")
    ap.add_argument("--num_images", type=int, default=8)
    ap.add_argument("--guidance_scale", type=float, default=7.5)
    ap.add_argument("--negative_prompt", type=str, default="longbody, lowres, bad anatomy, bad hands, missing fingers, "
                    "extra digit, fewer digits, cropped, worst quality, low quality")
    ap.add_argument("--input_json", type=str, nargs="+", default=["demos/demo_four_boxes.json"],
                    help="one demo JSON, or several: different layouts sampled in ONE batch (--num_images each), written to "
                         "OUTPUT/<save_folder_name>/<json stem>/")
    ap.add_argument("--ckpt", type=str, default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--alpha", type=float, default=0.75)
    ap.add_argument("--mis", type=float, default=0.36)
    ap.add_argument("--cascade_strength", type=float, default=0.0)
    ap.add_argument("--test_config", type=str, default="configs/test_mask.yaml")
    ap.add_argument("--device", type=str, default="cuda")
    ap.add_argument("--text_encoder", choices=["synthetic", "clip"], default=None)
    ap.add_argument("--clip_backend", choices=["hf", "hip"], default="hf",
                    help="CLIP text transformer on Hugging Face transformers (fp32 eager) or on the HIP kernels (--dtype storage)")
    ap.add_argument("--synthetic_weights", action="store_true")
    ap.add_argument("--dtype", choices=["bf16", "fp16"], default="bf16")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--save_latents", action="store_true")
    ap.add_argument("--use_masked_att", action="store_true",
                    help="masked gated self-attention (attention.py:187-255): instance patches only see their own box")
    ap.add_argument("--instance_masks", choices=["ignore", "json"], default="ignore",
                    help="json: condition on the COCO run-length masks of the JSON's annos (decoded on the device); ignore: as the "
                         "reference script, which decodes them and throws them away")
    ap.add_argument("--clip_score", choices=["hf", "hip"], default=None,
                    help="score every instance crop of every image against its phrase (local CLIP score) and write clip_scores.json "
                         "next to the PNGs; hip: crop, resize and both CLIP towers on the HIP kernels, from the decoder output on the device")
    ap.add_argument("--clip_path", type=str, default=None,
                    help="--clip_score: local directory of openai/clip-vit-large-patch14 (local files only); with --synthetic_weights "
                         "and no path, a key-seeded synthetic CLIP model")
    ap.add_argument("--keep_best", type=int, default=None,
                    help="write only the K images with the best mean CLIP score (needs --clip_score; the JSON still lists all)")
    ap.add_argument("--sampler", choices=["plms", "ddim", "ddim_inst", "dpmpp", "dpmpp_inst"], default="plms",
                    help="ddim: DDIMSampler (ldm/models/diffusion/ddim.py) instead of PLMSSampler; without the Multi-instance Sampler.  "
                         "ddim_inst: DDIMSamplerInst, the Multi-instance Sampler (--mis > 0) on DDIM steps.  dpmpp: DPMSolverSampler, "
                         "DPM-Solver++(2M), usable at 20-25 --steps (--mis 0); dpmpp_inst: DPMSolverSamplerInst, the same under the "
                         "Multi-instance Sampler (--mis > 0)")
    ap.add_argument("--dpm_order", type=int, choices=[1, 2], default=2,
                    help="--sampler dpmpp / dpmpp_inst: 2 = DPM-Solver++(2M), 1 = its first-order step (DDIM with eta 0)")
    ap.add_argument("--dpm_spacing", choices=["uniform", "logsnr"], default="uniform",
                    help="--sampler dpmpp / dpmpp_inst: uniform = the timesteps of PLMS and DDIM; logsnr = evenly spaced in log(alpha / sigma)")
    ap.add_argument("--ddim_eta", type=float, default=None,
                    help="--sampler ddim / ddim_inst: eta of the DDIM variance schedule (default 0: deterministic; 1: DDPM-like)")
    ap.add_argument("--init_image", type=str, default=None,
                    help="inpainting: PNG of the sampled size whose kept region is held to the original (needs --inpaint_mask)")
    ap.add_argument("--inpaint_mask", type=str, default=None,
                    help="inpainting: grey-scale PNG of the sampled size, >= 128 keeps the original, < 128 is repainted")
    ap.add_argument("--strength", type=float, default=None,
                    help="img2img (--init_image without --inpaint_mask): how far the picture is noised back, in (0, 1]; the last "
                         "floor(steps * strength) steps run.  With --mis > 0: strength <= 1 - mis")
    ap.add_argument("--hires_scale", type=float, default=None,
                    help="latent hi-res second pass: enlarge the finished latents by this factor (> 1; round(image_size * F) must be a "
                         "multiple of 8, e.g. 1.5 -> 96 x 96 latents, 768-pixel images) and denoise the tail of the schedule there")
    ap.add_argument("--hires_strength", type=float, default=0.5, help="--hires_scale: how far the enlarged latents are noised back, in (0, 1]")
    ap.add_argument("--hires_steps", type=int, default=None, help="--hires_scale: steps of the second pass's schedule (default: --steps)")
    ap.add_argument("--hires_mode", choices=["bicubic", "bilinear"], default="bicubic", help="--hires_scale: how the latents are enlarged")
    args = ap.parse_args()
    paths = list(args.input_json)
    img2img = args.strength is not None
    hires = args.hires_scale is not None
    if args.strength is not None and args.inpaint_mask is not None:
        raise SystemExit("--strength is img2img (--init_image without a mask); with --inpaint_mask the kept region is held at every step "
                         "and there is no strength")
    if img2img and args.init_image is None:
        raise SystemExit("--strength needs --init_image (img2img)")
    if img2img and not 0.0 < args.strength <= 1.0:
        raise SystemExit(f"--strength must be in (0, 1], got {args.strength}")
    if hires and not args.hires_scale > 1:
        raise SystemExit(f"--hires_scale must be > 1, got {args.hires_scale}")
    if hires and not 0.0 < args.hires_strength <= 1.0:
        raise SystemExit(f"--hires_strength must be in (0, 1], got {args.hires_strength}")
    if hires and args.hires_steps is not None and args.hires_steps < 1:
        raise SystemExit("--hires_steps must be >= 1")
    if (img2img or hires) and len(paths) > 1:
        raise SystemExit("--strength (img2img) and --hires_scale take one --input_json")
    if (img2img or hires) and args.use_masked_att:
        raise SystemExit("--strength (img2img) and --hires_scale do not run with --use_masked_att: its mask planes are built for the "
                         "model's own latent size and a full run")
    if hires and args.inpaint_mask is not None:
        raise SystemExit("--hires_scale does not run with inpainting (--inpaint_mask): the mask and x0 exist at the first size only")
    if img2img:
        refuse_start_inside_mis("--strength", args.steps, args.strength, args.mis)
    if hires:
        refuse_start_inside_mis("--hires_strength", args.hires_steps or args.steps, args.hires_strength, args.mis)
    ddim_inst = args.sampler == "ddim_inst"
    dpm = args.sampler in ("dpmpp", "dpmpp_inst")
    inst_inpaints = args.sampler in ("ddim_inst", "dpmpp_inst")            # the Multi-instance Samplers that take mask / x0
    if ddim_inst and not args.mis > 0:
        raise SystemExit("--sampler ddim_inst is the Multi-instance Sampler on DDIM steps: give --mis > 0 (or --sampler ddim)")
    if args.sampler == "dpmpp_inst" and not args.mis > 0:
        raise SystemExit("--sampler dpmpp_inst is the Multi-instance Sampler on DPM-Solver++ steps: give --mis > 0 (or --sampler dpmpp)")
    if args.sampler == "dpmpp" and args.mis > 0:
        raise SystemExit("--sampler dpmpp runs without the Multi-instance Sampler: give --mis 0 (or --sampler dpmpp_inst)")
    if dpm and args.ddim_eta is not None:
        raise SystemExit("--ddim_eta: DPM-Solver++ steps are deterministic, --sampler dpmpp / dpmpp_inst take no eta")
    if not dpm and (args.dpm_order != 2 or args.dpm_spacing != "uniform"):
        raise SystemExit("--dpm_order / --dpm_spacing need --sampler dpmpp or dpmpp_inst")
    if len(paths) > 1:
        if (args.init_image is not None or args.inpaint_mask is not None) and not (inst_inpaints or args.sampler == "dpmpp"):
            raise SystemExit("inpainting (--init_image / --inpaint_mask) takes one --input_json")
        if args.use_masked_att:
            raise SystemExit("--use_masked_att takes one --input_json: the mask / no-mask decision is per layout call")
    else:
        args.input_json = paths[0]                                         # one path: exactly the single-layout run
    if args.sampler == "ddim" and args.mis > 0:
        raise SystemExit("--sampler ddim has no Multi-instance Sampler (the reference has none): give --mis 0")
    if args.ddim_eta is not None and args.sampler not in ("ddim", "ddim_inst"):
        raise SystemExit("--ddim_eta needs --sampler ddim")
    if args.ddim_eta is not None and args.ddim_eta < 0:
        raise SystemExit("--ddim_eta must be >= 0")
    if (args.init_image is None) != (args.inpaint_mask is None) and not img2img:
        raise SystemExit("inpainting needs both --init_image and --inpaint_mask")
    if args.init_image is not None and args.mis > 0 and not inst_inpaints and not img2img:
        raise SystemExit("inpainting (--init_image / --inpaint_mask) runs without the Multi-instance Sampler: give --mis 0")
    if args.keep_best is not None and (args.clip_score is None or args.keep_best < 1):
        raise SystemExit("--keep_best K needs --clip_score and K >= 1")
    if args.clip_score and not (args.clip_path or args.synthetic_weights):
        raise SystemExit("--clip_score needs --clip_path DIR (or --synthetic_weights for the synthetic CLIP model)")
    if args.cascade_strength > 0:
        raise SystemExit("the SDXL refiner cascade is outside the sampling path (needs diffusers + downloads)")
    dev = torch.device(args.device)
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16

    if args.ckpt:
        from utils.checkpoint import load_model_ckpt
        model, autoencoder, clip_text, diffusion, cfg = load_model_ckpt(args.ckpt, args, args.device)
        use_clip = (args.text_encoder or "clip") == "clip"
        refuse_dropped_masks(args, model)
    elif args.synthetic_weights:
        from instancediffusion_amd import synth
        cfg = load_yaml(args.test_config)
        with torch.device("meta"):
            model = instantiate_from_config(cfg["model"])
            autoencoder = instantiate_from_config(cfg["autoencoder"])
        refuse_dropped_masks(args, model)
        model.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}),
                              assign=True)
        model.first_conv_sd_override = synth.synth_first_conv_sd()
        autoencoder.load_state_dict(
            synth.synth_state_dict({k: tuple(v.shape) for k, v in autoencoder.state_dict().items()}, 7), assign=True)
        model.eval(), autoencoder.eval()
        diffusion = instantiate_from_config(cfg["diffusion"]).to(args.device)
        clip_text, use_clip = None, False
        if args.text_encoder == "clip":
            raise SystemExit("--text_encoder clip needs --ckpt (the CLIP weights live in the checkpoint)")
    else:
        raise SystemExit("give --ckpt instancediffusion_sd15.pth, or --synthetic_weights for a dry run")
    model.compute_dtype = dtype
    autoencoder.compute_dtype = dtype
    if clip_text is not None:                  # prompt, negative prompt and phrase encodes all go through this one object
        clip_text.backend = args.clip_backend
        clip_text.compute_dtype = dtype
    if args.use_masked_att:
        model.efficient_attention = False      # the reference builds the mask only on its non-efficient path (:189)
        model.invalidate_engine()
    gi = instantiate_from_config(cfg["grounding_tokenizer_input"])
    model.grounding_tokenizer_input = gi
    text_encoder = clip_text if use_clip else SyntheticTextEncoder()
    phrase_encoder = ClipPhraseEncoder(clip_text) if use_clip else text_encoder

    if len(paths) > 1:
        return run_layouts(args, paths, model, autoencoder, diffusion, gi, text_encoder, phrase_encoder, dev, dtype)
    data = json.load(open(args.input_json))
    save_folder_name = f"gc{args.guidance_scale}-seed{args.seed}-alpha{args.alpha}"
    meta = meta_from_demo_json(data, args.alpha, ckpt=args.ckpt, save_folder_name=save_folder_name, instance_masks=args.instance_masks)
    torch.manual_seed(args.seed)
    starting_noise = torch.randn(args.num_images, 4, model.image_size, model.image_size).to(dev)
    side2 = hires_side(model.image_size, args.hires_scale) if hires else None
    inpaint = {}
    loaded = None if img2img else load_inpaint(args, model, autoencoder, dev)
    if loaded is not None:
        inpaint = dict(mask=loaded[0].expand(args.num_images, -1, -1, -1), x0=loaded[1].expand(args.num_images, -1, -1, -1))

    rows = None
    if args.instance_masks == "json":
        # every row of the call -- the global input and, under the Multi-instance Sampler, one per instance -- in ONE prepare_batch:
        # their mask stacks come from one idf_rle_decode_planes launch
        if args.mis > 0:
            meta["instance_meta"] = [prepare_instance_meta(meta, i) for i in range(len(meta["phrases"]))]
        rows = prepare_batch(meta, batch=args.num_images, max_objs=MAX_OBJS, model=phrase_encoder, processor=None,
                             image_size=starting_noise.shape[-1], use_masked_att=args.use_masked_att, device=dev, ops=model.engine.ops)
        report_masks(args.input_json, rows.get("mask_areas", [-1] * len(meta["phrases"])))
    inp, uc = get_model_inputs(meta, gi, text_encoder, phrase_encoder, args.num_images, dev, starting_noise,
                               args.negative_prompt, use_masked_att=args.use_masked_att, batch=rows)
    ag = partial(alpha_generator, type=meta["alpha_type"])
    shape = (args.num_images, model.in_channels, model.image_size, model.image_size)
    single, single_kw = single_sampler(args, diffusion, model, ag)         # img2img and the hi-res second pass run this one
    if img2img:
        # a start behind the Multi-instance phase is the single-trajectory sampler on the global input (refuse_start_inside_mis)
        from instancediffusion_amd.host.hires import noised_start
        x0 = autoencoder.encode(load_init_image(args.init_image, 8 * model.image_size).to(dev)).expand(args.num_images, -1, -1, -1)
        inp["x"], start = noised_start(single, x0, args.steps, args.strength, starting_noise, **single_kw)   # the seeded noise is the draw
        samples = single.sample_from(args.steps, shape, inp, start, uc=uc, guidance_scale=args.guidance_scale, **single_kw)
    elif args.mis > 0:
        extra = {}
        if ddim_inst:
            sampler = DDIMSamplerInst(diffusion, model, alpha_generator_func=ag, set_alpha_scale=set_alpha_scale, mis=args.mis)
            extra = dict(inpaint, eta=args.ddim_eta or 0.)
        elif args.sampler == "dpmpp_inst":
            sampler = DPMSolverSamplerInst(diffusion, model, alpha_generator_func=ag, set_alpha_scale=set_alpha_scale, mis=args.mis)
            extra = dict(inpaint, order=args.dpm_order, discretize=args.dpm_spacing)
        else:
            sampler = PLMSSamplerInst(diffusion, model, alpha_generator_func=ag, set_alpha_scale=set_alpha_scale, mis=args.mis)
        inputs = [inp]
        for i in range(len(meta["phrases"])):
            inst, _ = get_model_inputs(prepare_instance_meta(meta, i), gi, text_encoder, phrase_encoder, args.num_images,
                                       dev, starting_noise, instance_input=True, use_masked_att=args.use_masked_att,
                                       batch=None if rows is None else rows["instance_meta"][i])
            inputs.append(inst)
        samples = sampler.sample(S=args.steps, shape=shape, input=inputs, uc=uc, guidance_scale=args.guidance_scale, **extra)
    else:
        if args.sampler == "ddim":
            sampler = DDIMSampler(diffusion, model, alpha_generator_func=ag, set_alpha_scale=set_alpha_scale)
            inpaint["eta"] = args.ddim_eta or 0.
        elif args.sampler == "dpmpp":
            sampler = DPMSolverSampler(diffusion, model, alpha_generator_func=ag, set_alpha_scale=set_alpha_scale)
            inpaint.update(order=args.dpm_order, discretize=args.dpm_spacing)
        else:
            sampler = PLMSSampler(diffusion, model, alpha_generator_func=ag, set_alpha_scale=set_alpha_scale)
        samples = sampler.sample(S=args.steps, shape=shape, input=inp, uc=uc, guidance_scale=args.guidance_scale, **inpaint)
    pass1 = None
    if hires:
        from instancediffusion_amd.host.hires import hires_pass
        pass1 = samples
        noise2 = torch.randn(args.num_images, model.in_channels, side2, side2).to(dev)     # the next draw behind --seed
        samples = hires_pass(single, pass1, inp, uc, args.guidance_scale, args.hires_steps or args.steps, args.hires_strength,
                             (side2, side2), args.hires_mode, noise2, **single_kw)
    images = autoencoder.decode(samples)                                   # inference.py:95
    folder = os.path.join(args.output, save_folder_name)
    report = None
    if args.clip_score:
        report = clip_scores(args, images, data, dtype)
        if args.keep_best is not None:                                     # best first; the JSON still lists every image
            images = images[report["ranking"][:args.keep_best]]
    names = save_images(images, folder)
    if report is not None:
        kept = report["ranking"][:args.keep_best] if args.keep_best is not None else list(range(len(names)))
        report["saved"] = {os.path.basename(n): i for n, i in zip(names, kept)}
        with open(os.path.join(folder, "clip_scores.json"), "w") as f:
            f.write(json.dumps(report, indent=1) + "\n")
    if args.save_latents:
        saved = dict(latents=samples.cpu(), caption=data["caption"], phrases=meta["phrases"])
        if pass1 is not None:
            saved["latents_pass1"] = pass1.cpu()
        torch.save(saved, os.path.join(folder, "latents.pt"))
    print(f"saved {len(names)} images {tuple(images.shape[1:])} to {folder}")


if __name__ == "__main__":
    main()
