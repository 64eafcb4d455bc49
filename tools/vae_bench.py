#!/usr/bin/env python
"""Time AutoencoderKL.decode on one MI355X: full SD-1.5 KL-f8 decoder, 64x64 latents -> 512x512.

    python tools/vae_bench.py [batch] [iters]
    python tools/vae_bench.py [batch] [iters] --encode

Prints ONE JSON line: ms per image, images/s and achieved TFLOP/s against the 2514.5 GFLOP/image of the reference
decoder, plus per-op-family HIP-event times of one eager decode.

``--encode``: the same line for ``AutoencoderKL.encode`` on 512x512 images (graph replay after a warm-up, at least 20 timed
iterations), the GFLOP per image computed here from the encoder engine's packed layer shapes, the decode figures measured in the
same process alternately with encode, the eager per-family times, and the share / achieved TFLOP/s of ``conv3x3_down``.
"""
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
GFLOP_PER_IMAGE = 2514.5


def encoder_gflop(eng, H, W):
    """(multiply-add FLOP of one image through the packed encoder, the part of it in conv3x3_down), in GFLOP: every conv and GEMM
    from the shapes of the packed weights; norms, softmax and the posterior tail are not counted."""
    total = 2 * eng.conv_in[0].numel() * H * W
    down = 0
    for layers in eng.levels + [eng.mid]:
        for kind, p in layers:
            if kind == "res":
                total += 2 * (p["conv1"].w.numel() + p["conv2"].w.numel() + (p["skip"].w.numel() if p["skip"] is not None else 0)) * H * W
            elif kind == "attn":
                N, C = H * W, p["c"]
                total += 2 * (p["wqk"].numel() + p["wv"].numel() + p["proj"].w.numel()) * N + 2 * 2 * N * N * C
            elif kind == "down":
                H, W = (H - 2) // 2 + 1, (W - 2) // 2 + 1
                down += 2 * p.w.numel() * H * W
    total += down + 2 * (eng.n_out * eng.conv_out.w.shape[1] + eng.q_w.numel()) * H * W       # conv_out: the real rows only
    return total / 1e9, down / 1e9


def eager_family_ms(eng, enqueue):
    """Per-op-family HIP-event times of one eager pass (events on the launch stream)."""
    real = eng.ops
    rec = []

    class Timer:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if name in ("empty", "zeros", "device", "dtype"):
                return fn

            def timed(*a, **k):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                r = fn(*a, **k)
                e.record()
                rec.append((name, s, e))
                return r
            return timed if callable(fn) else fn
    eng.ops = Timer()
    try:
        enqueue()
    finally:
        eng.ops = real
    torch.cuda.synchronize()
    fam = {}
    for name, s, e in rec:
        fam[name] = fam.get(name, 0.0) + s.elapsed_time(e)
    return fam


def bench_encode(ae, B, iters):
    iters = max(iters, 20)
    ae.max_encode_batch = B
    g = torch.Generator().manual_seed(0)
    x = (torch.rand(B, 3, 512, 512, generator=g) * 2 - 1).cuda()
    noise = torch.randn(B, 4, 64, 64, generator=g).cuda()
    z = ae.encode(x, noise=noise)                # warm-up + graph capture, both directions
    ae.decode(z)
    torch.cuda.synchronize()
    t_enc = t_dec = 0.0
    for _ in range(iters):                       # alternately, so that both see the same clocks
        t0 = time.perf_counter()
        z = ae.encode(x, noise=noise)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        img = ae.decode(z)
        torch.cuda.synchronize()
        t_enc += t1 - t0
        t_dec += time.perf_counter() - t1
    t_enc /= iters
    t_dec /= iters
    assert torch.isfinite(z).all() and torch.isfinite(img).all()
    eng = ae.encoder_engine
    gflop, gflop_down = encoder_gflop(eng, 512, 512)
    fam = eager_family_ms(eng, lambda: eng._encode_ops(
        eng.buf("io.x", x.shape, torch.float32), eng.buf("io.noise", noise.shape, torch.float32),
        eng.buf("io.z", z.shape, torch.float32), eng.buf("io.moments", (B, 8, 64, 64), torch.float32)))
    down_ms = fam.get("conv3x3_down", 0.0)
    print(json.dumps(dict(what="AutoencoderKL.encode, SD-1.5 KL-f8, 512x512 -> 64x64 latent, bf16", batch=B, iters=iters,
                          ms_per_image=round(t_enc / B * 1e3, 3), images_per_s=round(B / t_enc, 2),
                          gflop_per_image=round(gflop, 1), tflops=round(B * gflop / t_enc / 1e3, 1),
                          decode=dict(ms_per_image=round(t_dec / B * 1e3, 3), tflops=round(B * GFLOP_PER_IMAGE / t_dec / 1e3, 1)),
                          conv3x3_down=dict(gflop_per_image=round(gflop_down, 1), eager_ms=round(down_ms, 3),
                                            share_of_eager=round(down_ms / max(sum(fam.values()), 1e-9), 3),
                                            tflops=round(B * gflop_down / max(down_ms, 1e-9), 1)),
                          eager_family_ms={k: round(v, 3) for k, v in sorted(fam.items(), key=lambda kv: -kv[1])})))


def main():
    argv = [a for a in sys.argv[1:] if a != "--encode"]
    encode = "--encode" in sys.argv[1:]
    B = int(argv[0]) if len(argv) > 0 else 4
    iters = int(argv[1]) if len(argv) > 1 else 5
    from instancediffusion_amd import synth     # seeded synthetic weights (no checkpoints offline)
    from instancediffusion_amd.host.config import instantiate_from_config, load_yaml
    cfg = load_yaml(os.path.join(REPO, "configs", "test_box.yaml"))
    with torch.device("meta"):
        ae = instantiate_from_config(cfg["autoencoder"])
    ae.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in ae.state_dict().items()}, 7), assign=True)
    ae.eval()
    ae.max_decode_batch = B
    if encode:
        return bench_encode(ae, B, iters)
    z = torch.randn(B, 4, 64, 64, device="cuda") * 0.18215 * 4
    ae.decode(z)                                 # warm-up + graph capture
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        img = ae.decode(z)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / iters
    assert torch.isfinite(img).all()
    # per-family times of one eager decode (HIP events on the launch stream)
    eng = ae.engine
    fam = eager_family_ms(eng, lambda: eng._decode_ops(eng.buf("io.z", z.shape, torch.float32),
                                                       eng.buf("io.img", (B, 3, 512, 512), torch.float32)))
    print(json.dumps(dict(what="AutoencoderKL.decode, SD-1.5 KL-f8, 64x64 latent -> 512x512, bf16", batch=B,
                          ms_per_image=round(dt / B * 1e3, 3), images_per_s=round(B / dt, 2),
                          tflops=round(B * GFLOP_PER_IMAGE / dt / 1e3, 1),
                          eager_family_ms={k: round(v, 3) for k, v in sorted(fam.items(), key=lambda kv: -kv[1])})))


if __name__ == "__main__":
    main()
