#!/usr/bin/env python
"""Generate tests/golden/hires_floor.pt: the FLOORS of tests/test_hires_sampler_gpu.py.  Reads only this repository's CPU oracle.

The reference has neither an img2img start nor a second pass, so there is no reference trajectory to store; the GPU test compares
against the composed oracles of tests/hires_cases.py, computed when it runs.  What cannot be computed there in a few seconds is the
oracle's OWN 16-bit error: the same ``img2img_reference`` / ``hires_reference`` call under ``torch.autocast("cpu", dtype)`` against its fp32
result -- rel-RMS of the final latents, tiny_box inputs, S = 5, CFG 7.5, strength 0.6 (start 2), 16^2 -> 24^2 bicubic, for PLMS, DDIM eta 0
and DPM-Solver++ order 2.  Floats and strings only:

  meta     tag, S, guidance, strength, start, size, seed, torch version
  floors   {"img2img" | "hires": {"plms" | "ddim" | "dpmpp": {"bf16" | "fp16": rel-RMS}}}

Usage:  python tests/make_hires_golden.py
"""
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    from instancediffusion_amd import synth
    from oracle import ref_cpu
    from tests import cases
    from tests import hires_cases as hc
    meta = cases.load_golden(hc.TAG)["meta"]
    inp = cases.build_inputs(meta)
    cfg = cases.cfg_for(meta["cfg"], meta["variant"])
    shape = tuple(inp["x"].shape)

    def run(case, kind, autocast=None):
        model = ref_cpu.OracleModel(synth.synth_state_dict(cases.unet_schema(cfg)), cfg, synth.synth_first_conv_sd())
        base = dict(x=inp["x"].clone(), timesteps=None, context=inp["context"], grounding_input=ref_cpu.prepare_grounding(inp["gb"]))

        def call():
            if case == "img2img":
                x0, noise = hc.case_tensors("img2img", shape)
                return hc.img2img_reference(kind, model, base, inp["uc"], x0, noise, alpha_type=meta["alpha_type"])
            return hc.hires_reference(kind, model, base, inp["uc"], hc.case_tensors("hires", shape), alpha_type=meta["alpha_type"])[1]
        with torch.no_grad():
            if autocast is None:
                return call().float().clone()
            with torch.autocast("cpu", dtype=autocast):
                return call().float().clone()

    floors = {}
    for case in hc.CASES:
        floors[case] = {}
        for kind in hc.SAMPLERS:
            t0 = time.time()
            final = run(case, kind)
            floors[case][kind] = {key: float(cases.rel_rms(run(case, kind, dt), final))
                                  for key, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16))}
            assert all(0.0 < v < 0.5 for v in floors[case][kind].values()), floors
            print(f"[golden] {hc.TAG} {case} {kind}: latent rms {float(final.pow(2).mean().sqrt()):.4f}, autocast floors "
                  f"{floors[case][kind]}, {time.time() - t0:.0f} s", flush=True)
    out = dict(meta=dict(tag=hc.TAG, S=hc.S, guidance=hc.GUIDANCE, strength=hc.STRENGTH, start=hc.START, size=list(hc.HIRES_SIZE),
                         seed=hc.SEED, torch=str(torch.__version__)), floors=floors)
    path = os.path.join(hc.GOLD, hc.FLOOR_GOLDEN)
    torch.save(out, path)
    print(f"[golden] wrote {path}, {os.path.getsize(path)} bytes", flush=True)


if __name__ == "__main__":
    main()
