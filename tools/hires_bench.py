#!/usr/bin/env python
"""The latent hi-res second pass against sampling the large canvas from step 0, the resize launch on its own, and the two kernels'
register use.  Full model, SYNTHETIC weights: the numbers are times, image quality cannot be judged on synthetic weights.

    python tools/hires_bench.py [--batch 8] [--steps 50] [--mis 0.36] [--runs 5] [--dtype bf16] [--out profiles/hires_bench.json]

(a) ``two_pass``: ``PLMSSamplerInst`` (the Multi-instance Sampler, the demo's instances) at the model's 64^2 latents, S steps, then
    ``hires_pass`` to 96^2 at strength 0.5 (``PLMSSampler`` from step S / 2) -- against ``direct``: the same ``PLMSSamplerInst`` call at 96^2
    from step 0.  Alternated in one process, median of ``--runs``, every run listed.
(b) ``resize_launch``: HIP events around 20 ``idf_resize_planes`` launches for 8 x 4 x 64^2 -> 96^2 and 32 x 4 x 64^2 -> 128^2, bicubic and
    bilinear, against a device-to-device copy of the output bytes.

    python tools/hires_bench.py --resources          (no GPU needed)

(c) ``resources``: VGPRs, SGPRs, scratch and LDS of ``resize_planes_kernel`` and ``q_sample_kernel`` from the compiler's
    ``-Rpass-analysis=kernel-resource-usage`` remarks (gfx950).

Each mode rewrites its own sections of ``--out`` and keeps the others.
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time
from functools import partial

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def merge_out(path, sections):
    res = {}
    if os.path.exists(path):
        with open(path) as f:
            res = json.load(f)
    res.update(sections)
    with open(path, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(sections))


def resources():
    """{kernel: {VGPRs, SGPRs, ScratchSize, LDS}} of the two kernels, from the compiler's remarks."""
    csrc = os.path.join(REPO, "instancediffusion_amd", "csrc")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-mllvm", "-amdgpu-mfma-vgpr-form",
             "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull]
    out = {}
    for src, want in (("hires.hip", "resize_planes_kernel"), ("misc.hip", "q_sample_kernel")):
        text = subprocess.run(["/opt/rocm/bin/hipcc"] + flags + [os.path.join(csrc, src)], capture_output=True, text=True, check=True).stderr
        name = None
        for line in text.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                # the mangled name of kernel<int[, bool]>: ..20resize_planes_kernelILi4ELb1EE.. -> resize_planes_kernel<4, true>
                t = re.search(r"\d([a-z][a-z_]*_kernel)I((?:L[ib]\d+E)+)E", m.group(1))
                name = m.group(1) if t is None else t.group(1) + "<" + ", ".join(
                    v if k == "i" else ("true" if v == "1" else "false") for k, v in re.findall(r"L([ib])(\d+)E", t.group(2))) + ">"
                continue
            m = re.search(r"remark:\s+(VGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]): (\d+)", line)
            if m and name and want in name:
                out.setdefault(name, {})[m.group(1)] = int(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--mis", type=float, default=0.36)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--dtype", choices=["bf16", "fp16"], default="bf16")
    ap.add_argument("--strength", type=float, default=0.5)
    ap.add_argument("--resources", action="store_true", help="only section (c): compile the two files and record the kernels' resources")
    ap.add_argument("--out", type=str, default=os.path.join(REPO, "profiles", "hires_bench.json"))
    args = ap.parse_args()
    if args.resources:
        return merge_out(args.out, dict(resources=dict(what="-Rpass-analysis=kernel-resource-usage, gfx950; resize_planes_kernel<taps, 16-B "
                                                            "stores>, q_sample_kernel<elements per thread>", kernels=resources())))
    import torch
    import inference
    from instancediffusion_amd import synth
    from instancediffusion_amd.host import hires
    from instancediffusion_amd.host.alpha import alpha_generator, set_alpha_scale
    from instancediffusion_amd.host.config import instantiate_from_config, load_yaml
    from instancediffusion_amd.host.input import meta_from_demo_json, prepare_instance_meta
    from instancediffusion_amd.host.samplers import PLMSSampler, PLMSSamplerInst
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
    B, side, side2 = args.batch, model.image_size, inference.hires_side(model.image_size, 1.5)
    torch.manual_seed(0)
    noise = torch.randn(B, 4, side, side).to(dev)
    noise2 = torch.randn(B, 4, side2, side2).to(dev)
    inp, uc = inference.get_model_inputs(meta, gi, enc, enc, B, dev, noise, "low quality")
    insts = [inference.get_model_inputs(prepare_instance_meta(meta, i), gi, enc, enc, B, dev, noise, instance_input=True)[0]
             for i in range(len(meta["phrases"]))]
    kw = dict(alpha_generator_func=partial(alpha_generator, type=meta["alpha_type"]), set_alpha_scale=set_alpha_scale)
    mis, single = PLMSSamplerInst(diffusion, model, mis=args.mis, **kw), PLMSSampler(diffusion, model, **kw)
    start, _ = hires.steps_for_strength(args.steps, args.strength)
    assert start >= int(args.steps * args.mis), "the second pass must enter behind the Multi-instance phase"

    def first_pass(x):
        model.reinstate_first_conv()                     # every run starts as a freshly loaded model does
        inputs = [dict(inp, x=x)] + [dict(i, x=x) for i in insts]
        return mis.sample(S=args.steps, shape=tuple(x.shape), input=inputs, uc=uc, guidance_scale=7.5), inputs[0]

    def two_pass():
        lat, i0 = first_pass(noise)
        return hires.hires_pass(single, lat, i0, uc, 7.5, args.steps, args.strength, (side2, side2), "bicubic", noise2)

    def direct():
        return first_pass(noise2)[0]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        assert tuple(out.shape) == (B, 4, side2, side2) and torch.isfinite(out).all()
        return (time.perf_counter() - t0) * 1e3
    legs = {"two_pass": two_pass, "direct": direct}
    for fn in legs.values():                             # warm-up: graph capture at both sizes, conditioning caches
        timed(fn)
    times = {k: [] for k in legs}
    for _ in range(args.runs):
        for k, fn in legs.items():
            times[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in times.items()}
    n_inst = len(insts)
    sampling = dict(
        what=f"PLMS + Multi-instance Sampler (mis {args.mis}, {n_inst} instances), S = {args.steps}, {B} images, full model, synthetic weights, "
             f"CFG 7.5: {side}^2 first pass + hires_pass to {side2}^2 at strength {args.strength} (PLMSSampler from step {start}) against the same "
             f"Multi-instance call at {side2}^2 from step 0; wall time of the sampling calls, no VAE; says nothing about image quality",
        dtype=args.dtype, runs=args.runs, ms_median={k: round(v, 1) for k, v in med.items()},
        ms_all={k: [round(t, 1) for t in v] for k, v in times.items()},
        spread_pct={k: round(100 * (max(v) - min(v)) / med[k], 2) for k, v in times.items()},
        two_pass_over_direct=round(med["two_pass"] / med["direct"], 4))

    ops = model.engine.ops
    launches = 20
    resize = {}
    for rows, s_in, s_out in ((8, 64, 96), (32, 64, 128)):
        g = torch.Generator(device="cpu").manual_seed(1)
        z = torch.randn(rows, 4, s_in, s_in, generator=g).to(dev)
        out = torch.empty(rows, 4, s_out, s_out, device=dev)
        twin = torch.randn(rows, 4, s_out, s_out, generator=g).to(dev)
        cases = {}
        for mode in ("bicubic", "bilinear"):
            hires.upscale_latents(ops, z, (s_out, s_out), mode)                                      # builds and uploads the tables
            tabs = hires._TABLES[(str(z.device), s_in, s_in, s_out, s_out, mode)]
            cases[mode] = partial(ops.resize_planes, z, out, *tabs)
        cases["copy_of_output_bytes"] = partial(out.copy_, twin)
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
        resize[f"{rows}x4x{s_in}^2->{s_out}^2"] = dict(us_per_launch=us, output_bytes=out.numel() * 4, input_bytes=z.numel() * 4)
    merge_out(args.out, dict(sampling=sampling,
                             resize_launch=dict(what=f"HIP events around {launches} launches, fp32 planes; the copy moves the output's bytes "
                                                     "device to device", **resize)))


if __name__ == "__main__":
    main()
