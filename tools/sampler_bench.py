#!/usr/bin/env python
"""Wall time of ``sample()``: DDIMSampler (eta 0) against PLMSSampler on the full model, alternated runs, median.

    python tools/sampler_bench.py [--steps 50] [--batch 8] [--runs 5] [--dtype bf16]

Informational (no bar): DDIM runs S batched [cond | uncond] forwards and one fused update launch per step, PLMS S + 1 forwards
(its first step evaluates twice), a guidance launch per forward and an update launch per step.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time
from functools import partial

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--dtype", choices=["bf16", "fp16"], default="bf16")
    args = ap.parse_args()
    import inference
    from instancediffusion_amd import synth
    from instancediffusion_amd.host.alpha import alpha_generator, set_alpha_scale
    from instancediffusion_amd.host.config import instantiate_from_config, load_yaml
    from instancediffusion_amd.host.input import meta_from_demo_json
    from instancediffusion_amd.host.samplers import DDIMSampler, PLMSSampler
    dev = torch.device("cuda")
    cfg = load_yaml(os.path.join(REPO, "configs", "test_box.yaml"))
    with torch.device("meta"):
        model = instantiate_from_config(cfg["model"])
    model.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}), assign=True)
    model.first_conv_sd_override = synth.synth_first_conv_sd()
    model.eval()
    model.compute_dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    diffusion = instantiate_from_config(cfg["diffusion"]).to(dev)
    gi = instantiate_from_config(cfg["grounding_tokenizer_input"])
    model.grounding_tokenizer_input = gi
    meta = meta_from_demo_json(json.load(open(os.path.join(REPO, "demos", "demo_four_boxes.json"))), 0.75)
    enc = inference.SyntheticTextEncoder()
    torch.manual_seed(0)
    noise = torch.randn(args.batch, 4, model.image_size, model.image_size).to(dev)
    inp, uc = inference.get_model_inputs(meta, gi, enc, enc, args.batch, dev, noise, "low quality")
    ag = partial(alpha_generator, type=meta["alpha_type"])
    shape = tuple(noise.shape)
    samplers = {"plms": PLMSSampler(diffusion, model, alpha_generator_func=ag, set_alpha_scale=set_alpha_scale),
                "ddim": DDIMSampler(diffusion, model, alpha_generator_func=ag, set_alpha_scale=set_alpha_scale)}

    def run(name):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = samplers[name].sample(S=args.steps, shape=shape, input=dict(inp, x=noise), uc=uc, guidance_scale=7.5)
        torch.cuda.synchronize()
        assert torch.isfinite(out).all()
        return (time.perf_counter() - t0) * 1e3
    for name in samplers:                                       # warm-up: graph capture, conditioning caches
        run(name)
    times = {name: [] for name in samplers}
    for _ in range(args.runs):
        for name in samplers:
            times[name].append(run(name))
    med = {k: statistics.median(v) for k, v in times.items()}
    print(json.dumps(dict(what="sample() wall time, full model, CFG 7.5", steps=args.steps, batch=args.batch, dtype=args.dtype,
                          runs=args.runs, forwards=dict(plms=2 * (args.steps + 1), ddim=2 * args.steps),
                          ms_median={k: round(v, 1) for k, v in med.items()},
                          ms_all={k: [round(t, 1) for t in v] for k, v in times.items()},
                          ddim_over_plms=round(med["ddim"] / med["plms"], 4))))


if __name__ == "__main__":
    main()
