"""Writes tests/golden/tiny_box_ddim.pt and mid_box_ddim.pt: ``DDIMSampler`` of the UNMODIFIED reference.

    IDF_REFERENCE=/path/to/InstanceDiffusion python tests/make_ddim_golden.py [--only TAG]

Generation time only: the reference tree is imported as it is, through the shims and builders of oracle/make_golden.py
(``install_shims``, ``load_cfg``, ``build``, ``patch_first_conv``, ``ref_alpha_generator``, ``ref_set_alpha_scale``).  Inputs are
those of ``tiny_box`` / ``mid_box`` (their ``meta`` is copied, so ``cases.build_inputs`` re-creates them: generator 1234, S = 5,
16x16 latents, batch 2, CFG 7.5); mask, x0 and every noise draw come from generator 4321, as in ``gen_plms_mask_case``.  A fixture
holds tensors, floats and strings only:

  meta        the case, in the form ``tests/cases.build_inputs`` understands
  mask, x0    [B,1,L,L] {0,1} and [B,4,L,L] of the inpainting cases
  cases[name] eta; final (the latent ``make_schedule(S, ddim_eta=eta)`` + ``ddim_sampling`` returns); the reference's own
              ddim_timesteps / ddim_alphas / ddim_alphas_prev / ddim_sigmas / ddim_sqrt_one_minus_alphas; noises: every draw in call
              order (q_sample's through its ``noise`` argument, p_sample_ddim's by wrapping ``torch.randn_like`` during the call);
              floor: rel-RMS of the same call under torch.autocast("cpu", dtype) against its fp32 result, same noises replayed
  schedules   the five schedule arrays for S = 50 at eta 0 / 0.5 / 1 (no forward)
"""
import argparse
import importlib.util
import os
import sys
import time
from copy import deepcopy
from functools import partial

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _f32(v):
    return torch.as_tensor(v).detach().clone()


def schedule_of(sampler):
    return dict(ddim_timesteps=torch.as_tensor(sampler.ddim_timesteps.copy()), ddim_alphas=_f32(sampler.ddim_alphas),
                ddim_alphas_prev=_f32(sampler.ddim_alphas_prev), ddim_sigmas=_f32(sampler.ddim_sigmas),
                ddim_sqrt_one_minus_alphas=_f32(sampler.ddim_sqrt_one_minus_alphas))


def rel_rms(a, b):
    a, b = a.double(), b.double()
    return float(((a - b).pow(2).mean() / b.pow(2).mean().clamp_min(1e-30)).sqrt())


@torch.no_grad()
def gen(tag, dc, mg):
    from ldm.models.diffusion.ddim import DDIMSampler
    spec = dc.GOLDENS[tag]
    meta = dict(torch.load(os.path.join(dc.GOLD, spec["inputs_of"] + ".pt"), weights_only=False)["meta"])
    meta.update(tag=tag, alpha_type=list(spec["alpha_type"]), mis=0.0, n_inst=0)
    cfg = mg.load_cfg(meta["cfg"], meta["variant"])
    model, gi, diffusion, schema, synth = mg.build(cfg)
    B, L, S = meta["batch"], meta["latent"], meta["S"]
    g = torch.Generator().manual_seed(1234)                       # the order of oracle/make_golden.gen_case
    bx = synth.random_boxes(meta["n_boxes"], g)
    gb = synth.make_grounding_batch(B, bx, g, with_scribbles=False, with_polygons=False, with_segs=False, seg_size=meta["seg_size"])
    x = torch.randn(B, 4, L, L, generator=g)
    context = torch.randn(B, 77, 768, generator=g)
    uc = torch.randn(B, 77, 768, generator=g)
    assert torch.equal(x.flatten()[:32], meta["x_fp"]["head"]) and torch.equal(context.flatten()[:32], meta["ctx_fp"]["head"])
    g2 = torch.Generator().manual_seed(dc.MASK_SEED)
    mask = (torch.rand(B, 1, L, L, generator=g2) > 0.5).float()
    x0 = torch.randn(B, 4, L, L, generator=g2)
    grounding = gi.prepare(gb)
    real_q, real_randn_like = diffusion.q_sample, torch.randn_like

    def run(eta, masked, source, autocast=None):
        """One reference trajectory; ``source(shape)`` supplies every noise draw."""
        m2 = deepcopy(model)
        m2.grounding_tokenizer_input = gi
        mg.patch_first_conv(m2, synth.synth_first_conv_sd())
        diffusion.q_sample = lambda x_start, t, noise=None: real_q(x_start, t, noise=source(x_start.shape))
        torch.randn_like = lambda t, **kw: source(t.shape)
        try:
            sampler = DDIMSampler(diffusion, m2, alpha_generator_func=partial(mg.ref_alpha_generator, type=list(spec["alpha_type"])),
                                  set_alpha_scale=mg.ref_set_alpha_scale)
            sampler.make_schedule(ddim_num_steps=S, ddim_eta=eta)
            inp = dict(x=x.clone(), timesteps=None, context=context, grounding_input=grounding)
            kw = dict(mask=mask, x0=x0) if masked else {}
            if autocast is None:
                out = sampler.ddim_sampling(tuple(x.shape), inp, uc, dc.GUIDANCE, **kw)
            else:
                with torch.autocast("cpu", dtype=autocast):
                    out = sampler.ddim_sampling(tuple(x.shape), inp, uc, dc.GUIDANCE, **kw)
        finally:
            diffusion.q_sample, torch.randn_like = real_q, real_randn_like
            os.chdir(mg.REF)
        return out.detach().float().clone(), sampler

    out = dict(meta=meta, mask=mask, x0=x0, cases={}, schedules={}, torch=str(torch.__version__))
    for name, (eta, masked) in spec["cases"].items():
        t0 = time.time()
        gn = torch.Generator().manual_seed(dc.MASK_SEED + 1)
        noises = []

        def record(shape):
            n = torch.randn(tuple(shape), generator=gn)
            noises.append(n.clone())
            return n
        final, sampler = run(eta, masked, record)
        assert len(noises) == (2 * S if masked else S)
        floor = {}
        for key, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
            it = iter(noises)
            low, _ = run(eta, masked, lambda shape: next(it).clone(), autocast=dt)
            floor[key] = rel_rms(low, final)
        out["cases"][name] = dict(eta=float(eta), final=final, noises=torch.stack(noises), floor=floor, **schedule_of(sampler))
        print(f"[golden] {tag} {name}: eta {eta}, mask {masked}, {len(noises)} draws, latent rms {float(final.pow(2).mean().sqrt()):.4f}, "
              f"autocast floor {floor}, {time.time() - t0:.0f} s", flush=True)
    sampler = DDIMSampler(diffusion, model)
    for S50, eta in dc.SCHEDULE_ONLY:
        sampler.make_schedule(ddim_num_steps=S50, ddim_eta=eta)
        out["schedules"][dc.schedule_key(S50, eta)] = dict(eta=float(eta), **schedule_of(sampler))
    path = os.path.join(dc.GOLD, f"{tag}.pt")
    torch.save(out, path)
    print(f"[golden] wrote {path}, {os.path.getsize(path) / 1024:.0f} KB", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="all")
    args = ap.parse_args()
    dc = _load("idf_ddim_cases", os.path.join(REPO, "tests", "ddim_cases.py"))       # torch / numpy only at module level
    mg = _load("idf_make_golden", os.path.join(REPO, "oracle", "make_golden.py"))
    mg.REF = os.environ.get("IDF_REFERENCE", mg.REF)
    mg.install_shims()                                            # the reference tree wins over this repository's ``ldm`` mirror
    for tag in dc.GOLDENS:
        if args.only in ("all", tag):
            gen(tag, dc, mg)


if __name__ == "__main__":
    main()
