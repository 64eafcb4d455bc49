#!/usr/bin/env python
"""Wall time of ``sample()``: DDIMSampler (eta 0) against PLMSSampler on the full model, alternated runs, median.

    python tools/sampler_bench.py [--steps 50] [--batch 8] [--runs 5] [--dtype bf16]

Informational (no bar): DDIM runs S batched [cond | uncond] forwards and one fused update launch per step, PLMS S + 1 forwards
(its first step evaluates twice), a guidance launch per forward and an update launch per step.  Prints one JSON line.

    python tools/sampler_bench.py --mis 0.36 [--instances 8]

the same for the Multi-instance Samplers: ``DDIMSamplerInst`` (eta 0) against ``PLMSSamplerInst`` with N instance inputs (the demo's
instances, repeated when N is larger), and -- a second JSON line -- the step launches with and without the unit -> image table:
HIP events around 20 launches of ``idf_ddim_update`` / ``idf_ddim_update_units`` and ``idf_q_sample_blend`` / ``_units`` at the width of
one phase-1 forward, against an ESTIMATE of a phase-1 step: ``sample()``'s median wall time times that step's share of the forward
rows of the call (``phase1_step_us_estimate``); no forward is timed on its own.

    python tools/sampler_bench.py --sampler dpmpp [--mis 0.36] [--out profiles/dpmpp_bench.json]

DPM-Solver++(2M): ``DPMSolverSampler`` (with ``--mis``: ``DPMSolverSamplerInst``) against DDIM eta 0 at EQUAL S, then at S = 20 against
PLMS at S = 50 -- a statement about forwards, not about image quality: the weights are synthetic -- both pairs alternated in one
process, median of ``--runs``, all runs listed; and HIP events around 20 launches of ``idf_dpmpp_update`` against ``idf_ddim_update``
at batch 8 and at 72 rows.  Prints one JSON line and writes it to ``--out``.
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
    ap.add_argument("--mis", type=float, default=0.0, help="> 0: DDIMSamplerInst against PLMSSamplerInst at this phase-1 share")
    ap.add_argument("--instances", type=int, default=8, help="--mis: instance inputs per image")
    ap.add_argument("--sampler", choices=["ddim", "dpmpp"], default="ddim", help="dpmpp: the DPM-Solver++(2M) pairs (see above)")
    ap.add_argument("--out", type=str, default=os.path.join(REPO, "profiles", "dpmpp_bench.json"), help="--sampler dpmpp: result file")
    args = ap.parse_args()
    import inference
    from instancediffusion_amd import synth
    from instancediffusion_amd.host.alpha import alpha_generator, set_alpha_scale
    from instancediffusion_amd.host.config import instantiate_from_config, load_yaml
    from instancediffusion_amd.host.input import meta_from_demo_json, prepare_instance_meta
    from instancediffusion_amd.host.samplers import (DDIMSampler, DDIMSamplerInst, DPMSolverSampler, DPMSolverSamplerInst, PLMSSampler,
                                                      PLMSSamplerInst)
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
    if args.mis > 0:
        kw = dict(alpha_generator_func=ag, set_alpha_scale=set_alpha_scale, mis=args.mis)
        samplers = {"plms": PLMSSamplerInst(diffusion, model, **kw), "ddim": DDIMSamplerInst(diffusion, model, **kw),
                    "dpmpp": DPMSolverSamplerInst(diffusion, model, **kw)}
        n_demo = len(meta["phrases"])
        insts = [inference.get_model_inputs(prepare_instance_meta(meta, i % n_demo), gi, enc, enc, args.batch, dev, noise,
                                            instance_input=True)[0] for i in range(args.instances)]
    else:
        samplers = {"plms": PLMSSampler(diffusion, model, alpha_generator_func=ag, set_alpha_scale=set_alpha_scale),
                    "ddim": DDIMSampler(diffusion, model, alpha_generator_func=ag, set_alpha_scale=set_alpha_scale),
                    "dpmpp": DPMSolverSampler(diffusion, model, alpha_generator_func=ag, set_alpha_scale=set_alpha_scale)}
    if args.sampler != "dpmpp":
        del samplers["dpmpp"]

    def inputs():
        if args.mis > 0:
            return [dict(inp, x=noise)] + [dict(i, x=noise) for i in insts]
        return dict(inp, x=noise)

    def run(name, steps=None):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = samplers[name].sample(S=steps or args.steps, shape=shape, input=inputs(), uc=uc, guidance_scale=7.5)
        torch.cuda.synchronize()
        assert torch.isfinite(out).all()
        return (time.perf_counter() - t0) * 1e3
    if args.sampler == "dpmpp":
        return dpmpp_pairs(args, run, model.engine.ops, shape)
    for name in samplers:                                       # warm-up: graph capture, conditioning caches
        run(name)
    times = {name: [] for name in samplers}
    for _ in range(args.runs):
        for name in samplers:
            times[name].append(run(name))
    med = {k: statistics.median(v) for k, v in times.items()}
    if args.mis > 0:
        print(json.dumps(dict(what="sample() wall time of the Multi-instance Samplers, full model, CFG 7.5, eta 0", steps=args.steps,
                              batch=args.batch, instances=args.instances, mis=args.mis, dtype=args.dtype, runs=args.runs,
                              ms_median={k: round(v, 1) for k, v in med.items()},
                              ms_all={k: [round(t, 1) for t in v] for k, v in times.items()},
                              ddim_over_plms=round(med["ddim"] / med["plms"], 4))))
        return unit_kernels(model.engine.ops, args.batch, args.instances + 1, shape[1:], med["ddim"], args.steps, args.mis)
    print(json.dumps(dict(what="sample() wall time, full model, CFG 7.5", steps=args.steps, batch=args.batch, dtype=args.dtype,
                          runs=args.runs, forwards=dict(plms=2 * (args.steps + 1), ddim=2 * args.steps),
                          ms_median={k: round(v, 1) for k, v in med.items()},
                          ms_all={k: [round(t, 1) for t in v] for k, v in times.items()},
                          ddim_over_plms=round(med["ddim"] / med["plms"], 4))))


def dpmpp_pairs(args, run, ops, shape, launches=20):
    """Two alternated pairs of ``sample()`` calls and the two update launches on their own; one JSON line, also written to --out."""
    def pair(a, b):
        """a, b: (name, steps).  Warm-up of both, then ``--runs`` alternated runs; medians, every run, the spread of each."""
        for name, steps in (a, b):
            run(name, steps)
        times = {a: [], b: []}
        for _ in range(args.runs):
            for name, steps in (a, b):
                times[(name, steps)].append(run(name, steps))
        med = {k: statistics.median(v) for k, v in times.items()}
        key = lambda k: f"{k[0]}_S{k[1]}"
        return dict(ms_median={key(k): round(v, 1) for k, v in med.items()}, ms_all={key(k): [round(t, 1) for t in v] for k, v in times.items()},
                    spread_pct={key(k): round(100 * (max(v) - min(v)) / med[k], 2) for k, v in times.items()},
                    ratio=round(med[a] / med[b], 4))
    equal = pair(("dpmpp", args.steps), ("ddim", args.steps))
    fewer = pair(("dpmpp", 20), ("plms", 50))
    dev = ops.device
    a_t, a_prev, s1m = 0.42288151383399963, 0.752143383026123, 0.7596831917762756
    kern = {}
    for rows in (8, 72):
        g = torch.Generator(device="cpu").manual_seed(1)
        x, ec, eu, last = (torch.randn((rows,) + tuple(shape[1:]), generator=g).to(dev) for _ in range(4))
        out, p0 = torch.empty_like(x), torch.empty_like(x)
        cases = {"dpmpp_update": lambda: ops.dpmpp_update(x, ec, eu, 7.5, a_t ** 0.5, s1m, 0.9, 0.3, -0.1, last, out, p0),
                 "ddim_update": lambda: ops.ddim_update(x, ec, eu, 7.5, a_t, a_prev, 0.0, s1m, None, out)}
        us = {}
        for name, fn in cases.items():
            fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us[name] = round(e0.elapsed_time(e1) * 1e3 / launches, 2)
        kern[f"rows{rows}"] = dict(us_per_launch=us, bytes_per_element=dict(dpmpp_update=6 * 4, ddim_update=4 * 4))
    res = dict(what="DPM-Solver++(2M) sample() wall time, full model, synthetic weights, CFG 7.5; the S = 20 against S = 50 pair counts "
                    "forwards and says nothing about image quality", batch=args.batch, dtype=args.dtype, runs=args.runs, mis=args.mis,
               instances=args.instances if args.mis > 0 else 0,
               equal_steps=dict(pair=f"dpmpp against ddim eta 0, S = {args.steps}", **equal),
               fewer_steps=dict(pair="dpmpp S = 20 against plms S = 50", **fewer),
               update_launch=dict(what=f"HIP events around {launches} launches, order 2 against DDIM eta 0, fp32 [rows, {shape[1]}, {shape[2]}, "
                                       f"{shape[3]}]", **kern))
    line = json.dumps(res)
    print(line)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


def unit_kernels(ops, B, per_img, chw_shape, sample_ms, steps, mis, launches=20):
    """The blend and the update at the width of one phase-1 forward (U = B x per_img units), with the table and -- on operands
    gathered to U rows, which is what the table saves -- without it: HIP events around ``launches`` launches, microseconds each."""
    dev = ops.device
    U = B * per_img
    g = torch.Generator(device="cpu").manual_seed(1)
    x, ec, eu = (torch.randn((U,) + tuple(chw_shape), generator=g).to(dev) for _ in range(3))
    nz, x0, qn = (torch.randn((B,) + tuple(chw_shape), generator=g).to(dev) for _ in range(3))
    mask = (torch.rand((B, 1) + tuple(chw_shape[1:]), generator=g) > 0.5).float().to(dev)
    tab = torch.tensor([u % B for u in range(U)], dtype=torch.int32).to(dev)
    idx = tab.long()
    nzU, x0U, qnU, maskU = (t[idx].contiguous() for t in (nz, x0, qn, mask))
    out = torch.empty_like(x)
    a_t, a_prev, sigma, s1m = 0.42288151383399963, 0.752143383026123, 0.21679943799972534, 0.7596831917762756
    cases = {
        "ddim_update_units": lambda: ops.ddim_update_units(x, ec, eu, 7.5, a_t, a_prev, sigma, s1m, nz, tab, out),
        "ddim_update": lambda: ops.ddim_update(x, ec, eu, 7.5, a_t, a_prev, sigma, s1m, nzU, out),
        "q_sample_blend_units": lambda: ops.q_sample_blend_units(x0, qn, mask, x, tab, 0.65, 0.76, out),
        "q_sample_blend": lambda: ops.q_sample_blend(x0U, qnU, maskU, x, 0.65, 0.76, out),
        "gather_4_operands": lambda: [t[idx].contiguous() for t in (nz, x0, qn, mask)],
    }
    us = {}
    for name, fn in cases.items():
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us[name] = round(e0.elapsed_time(e1) * 1e3 / launches, 2)
    # a phase-1 step of the run above: its share of sample() by forward rows (U of U + B (steps - mis_step) ... per step)
    mis_step = int(steps * mis)
    rows = mis_step * U + (steps - mis_step) * B
    step_us = sample_ms * 1e3 * U / rows
    print(json.dumps(dict(what="step launches at the width of one phase-1 forward, HIP events", units=U, images=B, launches=launches,
                          us_per_launch=us, phase1_step_us_estimate=round(step_us, 1),
                          share_of_step={k: round(v / step_us, 5) for k, v in us.items()})))


if __name__ == "__main__":
    main()
