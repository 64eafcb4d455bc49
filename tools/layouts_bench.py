#!/usr/bin/env python
"""Heterogeneous-layout throughput: ``PLMSSamplerInst.sample_layouts`` on L distinct layouts in ONE call against a loop of L
``sample()`` calls at batch 1 (one call per layout, the only way before ``sample_layouts``).

    python tools/layouts_bench.py [--layouts 32] [--runs 5] [--steps 50] [--dtype bf16] [--out profiles/layouts_bench.json]

L synthetic layouts (seeded boxes / contexts / noise, instance counts cycling through 2 .. 8), one image each, the full
SD-1.5-sized UNet with key-seeded weights, CFG 7.5, mis 0.36, alpha [0.8, 0, 0.2].  Both ways run in ONE process, alternated
(batched, loop, batched, loop, ..) after one untimed round of each (graph capture, first-conv swap); every timed round includes
the conditioning set-up of its calls.  Reported: median seconds of each way over the runs, the spread (max - min) / median of each,
and the ratio loop / batched.  Prints one JSON line and writes it to ``--out``."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from functools import partial

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

GUIDANCE, MIS, ALPHA_TYPE, LATENT = 7.5, 0.36, [0.8, 0.0, 0.2], 64


def make_layouts(n_layouts, gi, device):
    """[input_all of layout l] with conditioning at batch 1 and x [1, 4, 64, 64]; ONE zero mask-plane set on the device for all."""
    from instancediffusion_amd import synth
    zero = torch.zeros(1, 30, 512, 512, device=device)
    layouts, counts = [], []

    def dev(d):
        return {k: (zero if k == "segs" else v.to(device)) for k, v in d.items()}
    for l in range(n_layouts):
        n = 2 + l % 7                                                     # 2 .. 8 instances
        g = torch.Generator().manual_seed(9000 + l)
        gb = synth.make_grounding_batch(1, synth.random_boxes(n, g), g, seg_size=8)
        x = torch.randn(1, 4, LATENT, LATENT, generator=g).to(device)
        lay = [dict(x=x, timesteps=None, context=torch.randn(1, 77, 768, generator=g).to(device), grounding_input=gi.prepare(dev(gb)))]
        for i in range(n):
            lay.append(dict(x=x, timesteps=None, context=torch.randn(1, 77, 768, generator=g).to(device),
                            grounding_input=gi.prepare(dev(synth.instance_batch(gb, i)))))
        layouts.append(lay)
        counts.append(n)
    return layouts, counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layouts", type=int, default=32)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--dtype", choices=["bf16", "fp16"], default="bf16")
    ap.add_argument("--out", type=str, default=os.path.join(REPO, "profiles", "layouts_bench.json"))
    args = ap.parse_args()
    assert args.runs >= 5, "median of at least 5 runs"
    import bench
    from instancediffusion_amd.host.alpha import alpha_generator, set_alpha_scale
    from instancediffusion_amd.host.config import SD15_BOX_CFG
    from instancediffusion_amd.host.diffusion import LatentDiffusion
    from instancediffusion_amd.host.samplers import PLMSSamplerInst
    from grounding_input.text_grounding_tokinzer_input import GroundingNetInput
    dev = torch.device("cuda")
    model, _ = bench.build_model(dict(SD15_BOX_CFG))
    model.compute_dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    gi = GroundingNetInput()
    model.grounding_tokenizer_input = gi
    diffusion = LatentDiffusion(linear_start=0.00085, linear_end=0.012, timesteps=1000).to(dev)
    sampler = PLMSSamplerInst(diffusion, model, alpha_generator_func=partial(alpha_generator, type=ALPHA_TYPE),
                              set_alpha_scale=set_alpha_scale, mis=MIS)
    layouts, counts = make_layouts(args.layouts, gi, dev)
    uc = torch.randn(1, 77, 768, generator=torch.Generator().manual_seed(77)).to(dev)
    shape = (1, 4, LATENT, LATENT)

    def batched():
        return sampler.sample_layouts(S=args.steps, layouts=[[dict(d) for d in lay] for lay in layouts], uc=uc, guidance_scale=GUIDANCE)

    def loop():
        return torch.cat([sampler.sample(S=args.steps, shape=shape, input=[dict(d) for d in lay], uc=uc, guidance_scale=GUIDANCE)
                          for lay in layouts], 0)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        assert torch.isfinite(out).all() and out.shape[0] == args.layouts
        return time.perf_counter() - t0, out
    t, a = timed(batched)                                                 # untimed round: graph capture, first-conv swap
    print(f"[layouts_bench] warm-up: batched {t:.3f} s", file=sys.stderr, flush=True)
    t, b = timed(loop)
    print(f"[layouts_bench] warm-up: loop {t:.3f} s", file=sys.stderr, flush=True)
    _, a = timed(batched)                                                 # same model state (swapped first conv) for the comparison
    rel = float(((a - b).double().pow(2).mean() / b.double().pow(2).mean()).sqrt())
    tb, tl = [], []
    for _ in range(args.runs):
        tb.append(timed(batched)[0])
        tl.append(timed(loop)[0])
        print(f"[layouts_bench] batched {tb[-1]:.3f} s, loop {tl[-1]:.3f} s", file=sys.stderr, flush=True)
    mb, ml = statistics.median(tb), statistics.median(tl)
    res = dict(metric="heterogeneous layouts: one sample_layouts call against a loop of sample() calls at batch 1",
               layouts=args.layouts, instance_counts=counts, units=sum(c + 1 for c in counts), steps=args.steps, dtype=args.dtype,
               guidance=GUIDANCE, mis=MIS, alpha_type=ALPHA_TYPE, runs=args.runs,
               batched_s=round(mb, 4), loop_s=round(ml, 4), batched_all_s=[round(t, 4) for t in tb], loop_all_s=[round(t, 4) for t in tl],
               batched_spread=round((max(tb) - min(tb)) / mb, 4), loop_spread=round((max(tl) - min(tl)) / ml, 4),
               speedup_loop_over_batched=round(ml / mb, 4), batched_img_per_s=round(args.layouts / mb, 4),
               loop_img_per_s=round(args.layouts / ml, 4), batched_vs_loop_latent_rel_rms=rel,
               device=torch.cuda.get_device_name(0))
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    # the acceptance condition: the batched call is not slower than the loop beyond the measured run-to-run spread
    if mb > ml * (1 + max(res["batched_spread"], res["loop_spread"])):
        raise SystemExit(f"sample_layouts ({mb:.3f} s) is slower than the loop ({ml:.3f} s) beyond the run-to-run spread")


if __name__ == "__main__":
    main()
