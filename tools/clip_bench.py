#!/usr/bin/env python
"""Time the CLIP ViT-L/14 text transformer on one MI355X: ``CLIPTextEngine`` (HIP kernels, 16-bit storage)
against the Hugging Face ``CLIPTextModel`` it replaces (PyTorch eager) in the same 16-bit dtype and in fp32.

    python tools/clip_bench.py [--iters 7] [--dtype bf16|fp16] [--out profiles/clip_encode_bench.json]

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
        eng.encode_ids(ids)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--dtype", choices=["bf16", "fp16"], default="bf16")
    ap.add_argument("--sizes", type=int, nargs="+", default=[2, 288])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "clip_encode_bench.json"))
    args = ap.parse_args()
    iters = max(args.iters, 5)
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
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
