"""Writes tests/golden/tiny_box_layouts.pt: the Multi-instance Sampler of the UNMODIFIED reference on four different layouts.

    IDF_REFERENCE=/path/to/InstanceDiffusion python tests/make_layouts_golden.py

Generation time only: the reference tree is imported as it is, through the shims and builders of oracle/make_golden.py
(``install_shims``, ``load_cfg``, ``build``, ``patch_first_conv``, ``ref_alpha_generator``, ``ref_set_alpha_scale``).  The case is
tests/layouts_cases.py: ``test_box.yaml`` "tiny", 16x16 latents, S = 5, mis 0.4, alpha_type [1, 0, 0], CFG 7.5, layouts with
N = 0, 1, 3, 2 instances and their own seeded boxes, contexts and noise, one of them with two images.  Every image is run
SEPARATELY through the reference's ``PLMSSamplerInst`` at batch 1, on a fresh copy of the model.  The fixture holds tensors, floats
and strings only:

  meta      cfg, variant, latent, S, mis, alpha_type, guidance, seg_size and the layout specs (seed, n_inst, n_boxes, images)
  finals    per layout [images, 4, L, L]: the latents the reference returns
  floors    per layout, per image {"bf16", "fp16"}: rel-RMS of the same call under torch.autocast("cpu", dtype) against its fp32 result
"""
import importlib.util
import os
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


def rel_rms(a, b):
    a, b = a.double(), b.double()
    return float(((a - b).pow(2).mean() / b.pow(2).mean().clamp_min(1e-30)).sqrt())


@torch.no_grad()
def main():
    lc = _load("idf_layouts_cases", os.path.join(REPO, "tests", "layouts_cases.py"))
    mg = _load("idf_make_golden", os.path.join(REPO, "oracle", "make_golden.py"))
    mg.REF = os.environ.get("IDF_REFERENCE", mg.REF)
    mg.install_shims()                                            # the reference tree wins over this repository's ``ldm`` mirror
    from ldm.models.diffusion.plms_instance import PLMSSamplerInst
    cfg = mg.load_cfg(lc.CFG, lc.VARIANT)
    model, gi, diffusion, schema, synth = mg.build(cfg)

    def run(data, k, autocast=None):
        """Image k of one layout: one reference call at batch 1 on a freshly built model."""
        m2 = deepcopy(model)
        m2.grounding_tokenizer_input = gi
        mg.patch_first_conv(m2, synth.synth_first_conv_sd())
        try:
            sampler = PLMSSamplerInst(diffusion, m2, alpha_generator_func=partial(mg.ref_alpha_generator, type=list(lc.ALPHA_TYPE)),
                                      set_alpha_scale=mg.ref_set_alpha_scale, mis=lc.MIS)
            inputs = lc.input_all(data, data["x"][k:k + 1], gi.prepare, synth)
            kw = dict(S=lc.S, shape=(1, 4, lc.LATENT, lc.LATENT), input=inputs, uc=data["uc"], guidance_scale=lc.GUIDANCE)
            if autocast is None:
                out = sampler.sample(**kw)
            else:
                with torch.autocast("cpu", dtype=autocast):
                    out = sampler.sample(**kw)
        finally:
            os.chdir(mg.REF)
        return out.detach().float().clone()

    out = dict(meta=dict(tag=lc.TAG, cfg=lc.CFG, variant=lc.VARIANT, latent=lc.LATENT, S=lc.S, mis=lc.MIS, alpha_type=list(lc.ALPHA_TYPE),
                         guidance=lc.GUIDANCE, seg_size=lc.SEG_SIZE, layouts=[dict(s) for s in lc.LAYOUTS]),
               finals=[], floors=[], torch=str(torch.__version__))
    for spec in lc.LAYOUTS:
        t0 = time.time()
        data = lc.build_layout(spec, synth)
        finals, floors = [], []
        for k in range(spec["images"]):
            final = run(data, k)
            floors.append({key: rel_rms(run(data, k, autocast=dt), final) for key, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16))})
            finals.append(final)
        out["finals"].append(torch.cat(finals, 0))
        out["floors"].append(floors)
        print(f"[golden] {lc.TAG} seed {spec['seed']}: N = {spec['n_inst']}, {spec['images']} image(s), latent rms "
              f"{float(out['finals'][-1].pow(2).mean().sqrt()):.4f}, autocast floors {floors}, {time.time() - t0:.0f} s", flush=True)
    path = os.path.join(mg.GOLD, f"{lc.TAG}.pt")
    torch.save(out, path)
    print(f"[golden] wrote {path}, {os.path.getsize(path) / 1024:.0f} KB", flush=True)


if __name__ == "__main__":
    main()
