#!/usr/bin/env python
"""Time the CLIP ViT-L/14 text transformer on one MI355X: ``CLIPTextEngine`` (HIP kernels, 16-bit storage)
against the Hugging Face ``CLIPTextModel`` it replaces (PyTorch eager) in the same 16-bit dtype and in fp32.

    python tools/clip_bench.py [--iters 7] [--dtype bf16|fp16] [--out profiles/clip_encode_bench.json]
    python tools/clip_bench.py --vision [--iters 7] [--dtype bf16|fp16] [--sizes 8 256] [--out profiles/clip_vision_bench.json]
    python tools/clip_bench.py --score [--iters 7] [--dtype bf16|fp16] [--out profiles/clip_score_batched.json]

``--vision`` times the ViT-L/14 image tower instead (``CLIPVisionEngine`` against ``CLIPVisionModelWithProjection``) at B = 8 and
B = 256 crops (8 instances x 32 images) of 224 x 224, T = 257, with the same method, and adds the GEMM / attention / rest split of
one engine pass.  ``--score`` times the local CLIP score of 32 images x 8 instances: the per-image ``score()`` loop against
``score_batch`` from a device-resident fp32 batch, the crop kernel alone (bytes, GB/s) and the PIL preprocessing alone.  Run it under
``timeout`` as every GPU step.

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


def main_score(args, iters, dtype):
    """``--score``: 32 images of 512 x 512, 8 instances (the four boxes of demos/demo_four_boxes.json and their mirror images),
    synthetic ViT-L/14 weights: the per-image ``InstanceClipScorer.score`` loop (PIL crop + resize on the host, the tower on 8 crops
    at a time, one text call per phrase per image) against ``score_batch`` on the fp32 batch as it lies on the device after
    ``AutoencoderKL.decode``; beside them the crop kernel alone and the PIL preprocessing of the same crops alone."""
    import numpy as np
    from PIL import Image
    from instancediffusion_amd.host import clip_score as cs
    B, HW = 32, 512
    data = json.load(open(os.path.join(REPO, "demos", "demo_four_boxes.json")))
    boxes, phrases = cs.instances_from_demo_json(data)
    boxes = boxes + [[1.0 - b[2], b[1], 1.0 - b[0], b[3]] for b in boxes]
    phrases = phrases + ["the mirror image of " + p for p in phrases]
    model, tokenize, tokenizer = cs.load_clip(None)
    scorer = cs.InstanceClipScorer(model.cuda(), tokenize, backend="hip", dtype=dtype)
    g = torch.Generator().manual_seed(0)
    batch = (torch.rand((B, 3, HW, HW), generator=g) * 2.4 - 1.2).cuda()                 # decoder output, some of it beyond [-1, 1]
    pil = [Image.fromarray(a) for a in cs.quantise_images(batch)]
    S = scorer.size
    rects = cs.crop_rects(boxes, HW, HW)
    crops, blob, ntab, K = cs.pack_crop_tables(rects * B, [b for b in range(B) for _ in rects], S)
    tables, lut = torch.from_numpy(blob).cuda(), cs.pixel_lut().cuda()
    out = torch.empty((B * len(rects), 3, S, S), dtype=torch.float32, device="cuda")
    ops = scorer._vision.ops
    bytes_read = sum(3 * 4 * (x1 - x0) * (y1 - y0) for x0, y0, x1, y1 in rects) * B + blob.nbytes
    bytes_written = out.numel() * 4
    paths = {"score_loop": lambda: [scorer.score(im, boxes, phrases) for im in pil],
             "score_batch": lambda: scorer.score_batch(batch, boxes, phrases),
             "crop_kernel": lambda: ops.clip_crop_resize(batch, crops, tables, ntab, lut, out, K),
             "pil_preprocess": lambda: [cs.preprocess(c, S) for im in pil for c in cs.crop_instances(im, boxes)]}
    with torch.no_grad():
        loop, batched = paths["score_loop"](), paths["score_batch"]()                    # warm-up: buffers, kernel selection, caches
        for fn in paths.values():
            fn()
        times = {k: [] for k in paths}
        for _ in range(iters):                               # alternately, so that all see the same clocks
            for k, fn in paths.items():
                times[k].append(timed_ms(fn))
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        dev_ms = []
        for _ in range(iters):                               # the kernel on the device alone: HIP events around 20 launches
            s.record()
            for _ in range(20):
                paths["crop_kernel"]()
            e.record()
            torch.cuda.synchronize()
            dev_ms.append(s.elapsed_time(e) / 20)
    entry = {k: dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3)) for k, v in times.items()}
    kern_ms = statistics.median(dev_ms)
    diff = max(abs(a - b) for x, y in zip(loop, batched) for a, b in zip(x, y))
    return dict(what="local CLIP score of 32 images of 512 x 512, 8 instances each, ViT-L/14 synthetic weights: per-image score() loop "
                     "vs score_batch from the device-resident fp32 batch, ms per call (median of alternated runs)",
                dtype=args.dtype, iters=iters, device=torch.cuda.get_device_name(0), images=B, instances=len(rects), taps=K,
                table_sets=ntab, **entry,
                speedup_batch_vs_loop=round(entry["score_loop"]["median_ms"] / entry["score_batch"]["median_ms"], 2),
                batch_faster_beyond_spread=bool(entry["score_batch"]["max_ms"] < entry["score_loop"]["min_ms"]),
                crop_kernel_device=dict(median_ms=round(kern_ms, 4), min_ms=round(min(dev_ms), 4), max_ms=round(max(dev_ms), 4),
                                        bytes_read=int(bytes_read), bytes_written=int(bytes_written),
                                        gb_per_s=round((bytes_read + bytes_written) / kern_ms / 1e6, 1)),
                max_abs_score_difference_loop_vs_batch=diff)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--dtype", choices=["bf16", "fp16"], default="bf16")
    ap.add_argument("--sizes", type=int, nargs="+", default=None)
    ap.add_argument("--vision", action="store_true", help="time the image tower (CLIPVisionEngine) instead of the text transformer")
    ap.add_argument("--score", action="store_true", help="time the local CLIP score: the per-image score() loop against score_batch")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    iters = max(args.iters, 5)
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    if args.out is None:
        args.out = os.path.join(REPO, "profiles", "clip_score_batched.json" if args.score else
                                "clip_vision_bench.json" if args.vision else "clip_encode_bench.json")
    if args.vision or args.score:
        res = (main_score if args.score else main_vision)(args, iters, dtype)
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
