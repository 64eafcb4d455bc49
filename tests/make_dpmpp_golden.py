#!/usr/bin/env python
"""Generate tests/golden/dpmpp_floor.pt: the FLOORS of tests/test_dpmpp_sampler_gpu.py.  Reads only this repository's CPU oracle.

The reference has no DPM solver, so there is no reference trajectory to store; the GPU test compares against the composed oracle
(tests/dpmpp_cases.py), computed when it runs.  What cannot be computed there in a few seconds is the oracle's OWN 16-bit error: the
same ``dpmpp_reference`` / ``dpmpp_mis_reference`` call under ``torch.autocast("cpu", dtype)`` against its fp32 result -- rel-RMS of the
final latents, tiny_box inputs, S = 5, CFG 7.5, uniform spacing, orders 1 and 2.  Floats and strings only:

  meta     tag, S, mis, guidance, torch version
  floors   {"plain" | "mis": {order: {"bf16" | "fp16": rel-RMS}}}

Usage:  python tests/make_dpmpp_golden.py
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
    from tests import dpmpp_cases as dc
    meta = cases.load_golden(dc.TAG)["meta"]
    inp = cases.build_inputs(meta)
    cfg = cases.cfg_for(meta["cfg"], meta["variant"])

    def run(kind, order, autocast=None):
        model = ref_cpu.OracleModel(synth.synth_state_dict(cases.unet_schema(cfg)), cfg, synth.synth_first_conv_sd())
        inputs = [dict(x=inp["x"].clone(), timesteps=None, context=inp["context"], grounding_input=ref_cpu.prepare_grounding(inp["gb"]))]
        if kind == "mis":
            for i in range(meta["n_inst"]):
                inputs.append(dict(x=inp["x"].clone(), timesteps=None, context=inp["inst_ctx"][i],
                                   grounding_input=ref_cpu.prepare_grounding(synth.instance_batch(inp["gb"], i))))

        def call():
            if kind == "mis":
                return dc.dpmpp_mis_reference(model, dc.S, inputs, inp["uc"], dc.GUIDANCE, dc.MIS, order=order, alpha_type=meta["alpha_type"])
            return dc.dpmpp_reference(model, dc.S, inputs[0], inp["uc"], dc.GUIDANCE, order=order, alpha_type=meta["alpha_type"])
        with torch.no_grad():
            if autocast is None:
                return call().float().clone()
            with torch.autocast("cpu", dtype=autocast):
                return call().float().clone()

    floors = {}
    for kind in ("plain", "mis"):
        floors[kind] = {}
        for order in (1, 2):
            t0 = time.time()
            final = run(kind, order)
            floors[kind][order] = {key: float(cases.rel_rms(run(kind, order, dt), final))
                                   for key, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16))}
            assert all(0.0 < v < 0.5 for v in floors[kind][order].values()), floors
            print(f"[golden] {dc.TAG} DPM-Solver++ {kind} order {order}: latent rms {float(final.pow(2).mean().sqrt()):.4f}, autocast floors "
                  f"{floors[kind][order]}, {time.time() - t0:.0f} s", flush=True)
    out = dict(meta=dict(tag=dc.TAG, S=dc.S, mis=dc.MIS, guidance=dc.GUIDANCE, torch=str(torch.__version__)), floors=floors)
    path = os.path.join(dc.GOLD, dc.FLOOR_GOLDEN)
    torch.save(out, path)
    print(f"[golden] wrote {path}, {os.path.getsize(path)} bytes", flush=True)


if __name__ == "__main__":
    main()
