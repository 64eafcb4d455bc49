#!/usr/bin/env python
"""Time the CLIP ViT-L/14 text transformer on one MI355X: ``CLIPTextEngine`` (HIP kernels, 16-bit storage)
against the Hugging Face ``CLIPTextModel`` it replaces (PyTorch eager) in the same 16-bit dtype and in fp32.

    python tools/clip_bench.py [--iters 7] [--dtype bf16|fp16] [--out profiles/clip_encode_bench.json]
    python tools/clip_bench.py --vision [--iters 7] [--dtype bf16|fp16] [--sizes 8 256] [--out profiles/clip_vision_bench.json]

``--vision`` times the ViT-L/14 image tower instead (``CLIPVisionEngine`` against ``CLIPVisionModelWithProjection``) at B = 8 and
B = 256 crops (8 instances x 32 images) of 224 x 224, T = 257, with the same method, and adds the GEMM / attention / rest split of
one engine pass.  Run it under ``timeout`` as every GPU step.

Sizes: B = 2 sequences (prompt + negative prompt) and B = 288 (the per-instance prompts of the Multi-instance Sampler at N = 8 and
32 images), T = 77.  The three paths alternate inside one process, each timed ``iters`` (>= 5) times after a warm-up; the figure
is the median, the spread (min, max) is kept beside it.  Key-seeded synthetic weights (no checkpoints offline): timing does not
depend on the values.  Prints ONE JSON line and writes the same object to ``--out``.  Per-family HIP-event times of one engine pass
show where its time goes.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def family_ms(eng, ids):
    """Per-op-family HIP-event times of one engine pass (events on the launch stream)."""
    real, rec = eng.ops, []

    class Timer:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if name in ("empty", "zeros", "device", "dtype") or not callable(fn):
                return fn

            def timed(*a, **k):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                r = fn(*a, **k)
                e.record()
                rec.append((name + (".quick_gelu" if k.get("act") else ".ln" if k.get("ln_row") else ""), s, e))
                return r
            return timed
    eng.ops = Timer()
    try:
        (eng.encode_pixels if hasattr(eng, "encode_pixels") else eng.encode_ids)(ids)
    finally:
        eng.ops = real
    torch.cuda.synchronize()
    fam = {}
    for name, s, e in rec:
        fam[name] = fam.get(name, 0.0) + s.elapsed_time(e)
    return {k: round(v, 3) for k, v in sorted(fam.items(), key=lambda kv: -kv[1])}


def timed_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


VIT_L14 = dict(hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16, image_size=224, patch_size=14,
               projection_dim=768, hidden_act="quick_gelu", layer_norm_eps=1e-5)


def main_vision(args, iters, dtype):
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    from instancediffusion_amd import synth
    from instancediffusion_amd.clip_engine import CLIPVisionEngine
    hf32 = CLIPVisionModelWithProjection(CLIPVisionConfig(**VIT_L14)).eval()
    hf32.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in hf32.state_dict().items() if v.is_floating_point()}, 22),
                         strict=False)
    hf32 = hf32.cuda()
    eng = CLIPVisionEngine(hf32, dtype=dtype)
    hf16 = CLIPVisionModelWithProjection(CLIPVisionConfig(**VIT_L14)).eval()
    hf16.load_state_dict(hf32.state_dict())
    hf16 = hf16.cuda().to(dtype)
    res = dict(what="CLIP ViT-L/14 image tower, 224 px, T = 257: CLIPVisionEngine vs transformers eager, ms per call (median of "
                    "alternated runs)", dtype=args.dtype, iters=iters, device=torch.cuda.get_device_name(0), sizes={})
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for B in args.sizes or [8, 256]:
            px = torch.randn((B, 3, 224, 224), generator=g).cuda()
            px16 = px.to(dtype)
            paths = {"engine_" + args.dtype: lambda: eng.encode_pixels(px),
                     "hf_" + args.dtype: lambda: hf16(pixel_values=px16).image_embeds,
                     "hf_fp32": lambda: hf32(pixel_values=px).image_embeds}
            for fn in paths.values():                        # warm-up: buffers, kernel selection, caches
                fn()
                fn()
            times = {k: [] for k in paths}
            for _ in range(iters):                           # alternately, so that all see the same clocks
                for k, fn in paths.items():
                    times[k].append(timed_ms(fn))
            assert bool(torch.isfinite(eng.encode_pixels(px)[2]).all())
            entry = {k: dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3)) for k, v in times.items()}
            e, h = entry["engine_" + args.dtype], entry["hf_" + args.dtype]
            entry["speedup_vs_hf_" + args.dtype] = round(h["median_ms"] / e["median_ms"], 2)
            entry["speedup_vs_hf_fp32"] = round(entry["hf_fp32"]["median_ms"] / e["median_ms"], 2)
            fam = family_ms(eng, px)
            entry["engine_family_ms"] = fam
            gemm = sum(v for k, v in fam.items() if k.startswith("gemm"))
            attn = sum(v for k, v in fam.items() if k.startswith("attention"))
            entry["engine_split_ms"] = dict(gemm=round(gemm, 3), attention=round(attn, 3), rest=round(sum(fam.values()) - gemm - attn, 3))
            res["sizes"][f"B{B}"] = entry
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--dtype", choices=["bf16", "fp16"], default="bf16")
    ap.add_argument("--sizes", type=int, nargs="+", default=None)
    ap.add_argument("--vision", action="store_true", help="time the image tower (CLIPVisionEngine) instead of the text transformer")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    iters = max(args.iters, 5)
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    if args.out is None:
        args.out = os.path.join(REPO, "profiles", "clip_vision_bench.json" if args.vision else "clip_encode_bench.json")
    if args.vision:
        res = main_vision(args, iters, dtype)
        print(json.dumps(res))
        if args.out:
            with open(args.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
        return
    args.sizes = args.sizes or [2, 288]
    from transformers import CLIPTextConfig, CLIPTextModel
    from instancediffusion_amd import synth
    from instancediffusion_amd.clip_engine import CLIPTextEngine
    from instancediffusion_amd.host.text_encoder import CLIP_L14_TEXT
    hf32 = CLIPTextModel(CLIPTextConfig(**CLIP_L14_TEXT)).eval()
    hf32.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in hf32.state_dict().items() if v.is_floating_point()}, 21),
                         strict=False)
    hf32 = hf32.cuda()
    eng = CLIPTextEngine(hf32, dtype=dtype)
    hf16 = CLIPTextModel(CLIPTextConfig(**CLIP_L14_TEXT)).eval()
    hf16.load_state_dict(hf32.state_dict())
    hf16 = hf16.cuda().to(dtype)
    res = dict(what="CLIP ViT-L/14 text transformer, T = 77: CLIPTextEngine vs transformers eager, ms per call (median of alternated runs)",
               dtype=args.dtype, iters=iters, device=torch.cuda.get_device_name(0), sizes={})
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for B in args.sizes:
            ids = torch.randint(320, 49000, (B, 77), generator=g)
            ids[:, 0], ids[:, 40:] = 49406, 49407
            ids = ids.cuda()
            paths = {"engine_" + args.dtype: lambda: eng.encode_ids(ids),
                     "hf_" + args.dtype: lambda: hf16(input_ids=ids).last_hidden_state,
                     "hf_fp32": lambda: hf32(input_ids=ids).last_hidden_state}
            for fn in paths.values():                        # warm-up: buffers, kernel selection, caches
                fn()
                fn()
            times = {k: [] for k in paths}
            for _ in range(iters):                           # alternately, so that all see the same clocks
                for k, fn in paths.items():
                    times[k].append(timed_ms(fn))
            z = eng.encode_ids(ids)[0]
            assert bool(torch.isfinite(z).all())
            entry = {k: dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3)) for k, v in times.items()}
            e, h = entry["engine_" + args.dtype], entry["hf_" + args.dtype]
            entry["speedup_vs_hf_" + args.dtype] = round(h["median_ms"] / e["median_ms"], 2)
            entry["speedup_vs_hf_fp32"] = round(entry["hf_fp32"]["median_ms"] / e["median_ms"], 2)
            entry["engine_not_slower_beyond_spread"] = bool(e["median_ms"] <= h["max_ms"])
            entry["engine_family_ms"] = family_ms(eng, ids)
            res["sizes"][f"B{B}"] = entry
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
