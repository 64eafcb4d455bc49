#!/usr/bin/env python
"""Headline benchmark: InstanceDiffusion Multi-instance Sampler throughput on MI355X.

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

Workload (BASELINE.json metric): SD-1.5 InstanceDiffusion UNet (1.228 B parameters, seeded
synthetic weights -- no checkpoints exist offline), 512x512 images = 64x64 latents, 50 PLMS steps, classifier-free
guidance 7.5, N=8 box instances, Multi-instance Sampler mis=0.36 (=> 406 UNet forwards per image), alpha schedule
[0.8, 0, 0.2].  One "step" = one full sampling of the global image batch.  Default: weak scaling, images_per_gpu x n_gpus
images per step; ``--images-total K`` fixes the global batch instead (strong scaling, e.g. 8 images on 1 / 2 / 4 / 8 GPUs).
At n_gpus > 1 the (instance, image) work units of MIS phase 1 are sharded over the ranks by ``--sharding``: "instance"
(default; owner = (image + instance) mod N: the N+1 trajectories of every image are spread over the GPUs and ONE RCCL
all-gather of the unit latents each rank owns recombines them, in the fixed [instance][image] order, before the same idf_mis_merge
call as on one GPU: north_star's split) or "image" (owner = image mod N: replicas, nothing to exchange at the merge).  Inputs are resident in HBM before the timed region.  VAE decode is outside the path.

Prints ONE JSON line on rank 0 with the driver contract fields (metric, value, unit, higher_is_better, dtype, ms_per_step,
...).  A plain run does only the headline: set-up, ``--warmup`` untimed + ``--steps`` timed samplings, the line.
``--full`` adds the measurements that take runs of their own:
  "roofline"     -- dominant kernel's achieved TFLOP/s (algorithmic flops / HIP-event duration) vs 2.5 PF bf16 MFMA
  "executed"     -- the flops the engine really ran in the timed region
  "cpu_baseline" -- the CPU oracle (port of the reference algorithm, fp32) timed on this host on a bounded sample
  and the short legs "reference_batch_leg" (8 images, 1 GPU), "strong_scaling_leg" (8 images in total, N > 1 GPUs) and
  "alt_dtype_leg" (the other 16-bit type); each ``--no-*`` option below drops one of them.
``--dump-outputs DIR`` writes the latents the last timed sampling returned as DIR/latents.npy (float32; the inputs are
seeded, so two builds run with the same arguments can be compared output for output).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from functools import partial

import torch

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

PEAK_MFMA_TF = 2500.0          # dense bf16 MFMA, MI355X_MICROARCH.md
ALT_STEPS = 3                  # timed samplings of the other-dtype leg (one step after one warm-up was within clock-ramp noise)
N_INST, S_STEPS, MIS, GUIDANCE, ALPHA_TYPE, LATENT = 8, 50, 0.36, 7.5, [0.8, 0.0, 0.2], 64
GFLOP_PER_FWD = 1227.3         # reference-algorithmic work per UNet forward per sample at 64x64


def n_forwards(n_inst, S, mis):
    ms = int(S * mis)
    return 2 * ((n_inst + 1) * (ms + 1) + (S - ms))


def build_model(cfg):
    from instancediffusion_amd import synth
    from instancediffusion_amd.host.config import unet_kwargs_from_cfg
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    with torch.device("meta"):
        model = UNetModel(**unet_kwargs_from_cfg(cfg))
    sd = synth.synth_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict(sd, assign=True)
    model.first_conv_sd_override = synth.synth_first_conv_sd()
    return model.eval(), sd


def make_inputs(cfg, n_images, device):
    """Seeded synthetic C3 inputs: N random boxes, random text embeddings / contexts, shared noise.

    Every image of the batch carries the same grounding (as ``utils/input.py:prepare_batch`` produces: one meta
    repeated ``batch`` times), so the grounding tensors are built for ONE sample: the small ones are repeated on the
    device, the 30 x 512 x 512 mask stack (31 MB per sample) is a stride-0 batch broadcast -- the reference's
    ``.repeat`` layout would cost 9 inputs x 31 MB x images of host AND device memory per rank (72 GB at 256 images)."""
    from instancediffusion_amd import synth
    from grounding_input.text_grounding_tokinzer_input import GroundingNetInput
    g = torch.Generator().manual_seed(1234)
    boxes = synth.random_boxes(N_INST, g)
    gb1 = synth.make_grounding_batch(1, boxes, g)
    x = torch.randn(n_images, 4, LATENT, LATENT, generator=g)
    ctx = torch.randn(n_images, 77, 768, generator=g)
    # ONE negative-prompt context for the whole batch, as inference.py builds it (text_encoder.encode(batch * [negative_prompt])):
    # a stride-0 broadcast, so the samplers build that conditioning once (per-rank setup independent of the world size)
    uc = torch.randn(1, 77, 768, generator=g)
    inst_ctx = [torch.randn(n_images, 77, 768, generator=g) for _ in range(N_INST)]
    gi = GroundingNetInput()

    def dev(d1):
        out = {}
        for k, v in d1.items():
            v = v.to(device)
            out[k] = v.expand(n_images, *v.shape[1:]) if k == "segs" else v.repeat(n_images, *([1] * (v.dim() - 1)))
        return out
    inputs = [dict(x=x.to(device), timesteps=None, context=ctx.to(device), grounding_input=gi.prepare(dev(gb1)))]
    for i in range(N_INST):
        inputs.append(dict(x=x.to(device), timesteps=None, context=inst_ctx[i].to(device),
                           grounding_input=gi.prepare(dev(synth.instance_batch(gb1, i)))))
    gi.prepare(dev(gb1))
    return inputs, uc.to(device).expand(n_images, 77, 768), gi, dict(gb=gb1, x=x, ctx=ctx)


class OpTimer:
    """Wraps the ops object for ONE eager forward: HIP events (on the launch stream) around every C-ABI call."""

    def __init__(self, ops):
        self.ops, self.records = ops, []

    def __getattr__(self, name):
        fn = getattr(self.ops, name)
        if name not in ("gemm", "conv3x3", "attention", "groupnorm", "layernorm", "scaleu_concat", "conv_in",
                        "timestep_embedding", "mlp_geglu"):
            return fn
        # the fused GEGLU feed-forward is the two dense products of an MLP in one launch: it is booked under the dense-GEMM
        # family with the flops of both (the intermediate it no longer writes / reads is not part of its algorithmic bytes)
        fam = "gemm" if name == "mlp_geglu" else name

        def timed(*a, **k):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            r = fn(*a, **k)
            e.record()
            self.records.append((fam, self._work(name, a, k), s, e, self._bytes(name, a, k)))
            return r
        return timed

    @staticmethod
    def _work(name, a, k):
        if name == "gemm":
            A, W, out = a[0], a[1], a[2]
            batch = out.shape[0] if out.dim() == 3 else 1
            return 2.0 * batch * A.shape[-2] * W.shape[-2] * A.shape[-1]
        if name == "mlp_geglu":                                  # (x, stats, w1, cd, w2p, b2, out)
            x, w1, w2p = a[0], a[2], a[4]
            return 2.0 * x.shape[0] * (w1.shape[0] * w1.shape[1] + w2p.shape[0] * w2p.shape[1])
        if name == "conv3x3":
            x, w, out = a[0], a[1], a[2]
            npix = out.numel() // out.shape[1] if k.get("n_valid") else out.numel() // out.shape[-1]
            return 2.0 * npix * w.shape[0] * w.shape[1]
        if name == "attention":
            q, n0 = a[0], a[3]
            return 4.0 * q.shape[0] * q.shape[1] * (n0 + k.get("n1", 0)) * q.shape[2]
        return 0.0

    @staticmethod
    def _bytes(name, a, k):
        """Algorithmic (compulsory) HBM bytes of one launch: every operand read once, the result written once."""
        def nb(t):
            return 0 if t is None else t.numel() * t.element_size()
        if name == "gemm":
            return nb(a[0]) + nb(a[1]) + nb(a[2]) + nb(k.get("res")) + nb(k.get("bias")) + nb(k.get("vt_out")) + nb(k.get("out_stats"))
        if name == "mlp_geglu":
            return 2 * nb(a[0]) + nb(a[1]) + nb(a[2]) + nb(a[3]) + nb(a[4]) + nb(a[5]) + nb(a[6])   # x (LN input and residual), stats, weights, out
        if name == "conv3x3":
            return nb(a[0]) + nb(a[1]) + nb(a[2]) + nb(k.get("res")) + nb(k.get("bias"))
        if name == "attention":
            q, k0, vt0, n0, out = a[0], a[1], a[2], a[3], a[4]
            extra = nb(k.get("k1")) + nb(k.get("vt1"))
            return 2 * (q.shape[0] * q.shape[1] * q.shape[2]) * 2 + 2 * q.shape[0] * n0 * q.shape[2] * 2 + extra
        return 0

    def summary(self):
        torch.cuda.synchronize()
        agg = {}
        for name, work, s, e, nbytes in self.records:
            d = agg.setdefault(name, dict(calls=0, ms=0.0, flops=0.0, bytes=0.0))
            d["calls"] += 1
            d["ms"] += s.elapsed_time(e)
            d["flops"] += work
            d["bytes"] += nbytes
        return agg


def pmc_traffic(op_name, batch):
    """HBM bytes per launch of the dominant kernel family from the committed rocprofv3 PMC passes (FETCH_SIZE x2 per
    the gfx950 correction + WRITE_SIZE, separate runs; profiles/README.md).  None when no pass exists for this batch."""
    path = os.path.join(REPO, "profiles", "pmc_traffic.json")
    if not os.path.exists(path):
        return None
    try:
        tab = json.load(open(path))
        return tab.get(str(batch), {}).get(op_name)
    except Exception:
        return None


def measure_roofline(engine, batch, fuser_on=True):
    """One instrumented eager forward at the phase-1 batch: per-kernel-family durations from HIP events.  The forward is a
    PAIRED one ([cond | uncond] rows sharing latent and timestep), as every sampler forward of the timed region is: its
    conditioning-free prefix runs on batch / 2 rows (engine.PAIR_HOIST), and the flops per row counted here are the executed ones."""
    dev = engine.device
    cond = engine._slots[batch]
    x = torch.randn(batch, 4, LATENT, LATENT, device=dev)
    t = torch.full((batch,), 500.0, device=dev)
    eps = torch.empty(batch, 4, LATENT, LATENT, device=dev)
    real = engine.ops
    for _ in range(2):                                   # 1 warm + 1 measured
        timer = OpTimer(real)
        engine.ops = timer
        try:
            engine._forward_ops(x, t, cond, eps, fuser_on, paired=True)
        finally:
            engine.ops = real
    agg = timer.summary()
    total_ms = sum(d["ms"] for d in agg.values())
    dom = max(agg.items(), key=lambda kv: kv[1]["ms"])
    name, d = dom
    kern = {"conv3x3": "gemm_kernel_big<.., CONV=true> (persistent 256x320 implicit-GEMM 3x3 conv, LDS-DMA gather; "
                       "gemm_kernel_ring<..,true> + split-K for small grids)",
            "gemm": "gemm_kernel_big<.., CONV=false> (persistent 256x{320,256}-tile dense GEMM, LDS-DMA staging, in-register "
                    "epilogue; gemm_kernel_ring / gemm_kernel_dma 128x128 for small grids and batched launches) + mlp320w_kernel (the C = 320 GEGLU "
                    "feed-forwards, both products in one launch, one generated instruction stream per SIMD) + qkv320w_kernel / qkv640w_kernel / "
                    "geglu640w_kernel (the fused q | k | v projections of the C = 320 / 640 levels and the GEGLU projection of the C = 640 "
                    "level, activation rows resident in registers)",
            "attention": "attn4w_kernel<DT,2> for d=40 (64 queries/wave, asm-scheduled stream, LDS-DMA K / V^T rings, max-free softmax, XCD-aware "
                         "grid) / attn8_kernel for d=80,160 (32 queries/wave, LDS-DMA rings, deferred-rescale running max) / "
                         "attn_kernel for the 77-key cross-attention"
            }.get(name, name)
    achieved = d["flops"] / (d["ms"] * 1e-3) / 1e12 if d["ms"] > 0 else 0.0
    pmc = pmc_traffic(name, batch)
    # `traffic` = HBM bytes per launch from the committed rocprofv3 PMC passes (FETCH_SIZE x2 gfx950 correction +
    # WRITE_SIZE, separate runs), averaged over the family's launches of one forward at this batch; null without a pass
    return dict(_flops_per_row=sum(v["flops"] for v in agg.values()) / batch,
                bound="mfma", kernel=kern, achieved=round(achieved, 2), peak=PEAK_MFMA_TF, unit="TFLOP/s",
                frac=round(achieved / PEAK_MFMA_TF, 4),
                traffic=None if pmc is None else float(pmc["hbm_bytes_per_launch"]), traffic_unit="bytes/launch",
                traffic_source=None if pmc is None else pmc.get("source"),
                traffic_measured_in_this_run=False,      # a table lookup of the committed rocprofv3 --pmc passes (counters cannot be read from inside the process)
                launches_per_forward=d["calls"], avg_launch_us=round(d["ms"] * 1e3 / d["calls"], 2),
                algorithmic_gflop_per_launch=round(d["flops"] / d["calls"] / 1e9, 3),
                algorithmic_mbytes_per_launch=round(d["bytes"] / d["calls"] / 1e6, 2), measured_at_batch=batch,
                forward_breakdown_ms={k: round(v["ms"], 3) for k, v in sorted(agg.items(), key=lambda kv: -kv[1]["ms"])},
                forward_total_ms=round(total_ms, 3),
                # context for `frac`, NOT measured in this run: what the chip sustains under its power limit, from the torch-free
                # micro-benchmarks of round 3 (a kernel issuing nothing but bf16 MFMAs; the same stream plus this kernel family's
                # LDS fragment reads and LDS-DMA pieces per MFMA, without any synchronisation)
                peak_context=dict(spec_peak=PEAK_MFMA_TF, sustained_mfma_only=1876.0, sustained_mfma_plus_kloop_operand_traffic=1115.0,
                                  unit="TFLOP/s", source="profiles/r03_ubench_mfma_sustain.log, profiles/r03_ubench_mfma_power.log "
                                                          "(tools/ubench/mfma_sustain.hip, mfma_power.hip)"))


def cpu_baseline(cfg, sd, host_inputs, budget_s=25.0):
    """The CPU oracle (fp32 port of the reference algorithm) on this host's cores, bounded sample."""
    from oracle import ref_cpu
    # MKL-DNN oversubscribes badly on many-core hosts (256 threads: 235 s per forward measured); 32 threads is
    # the fastest setting we found -- `cores` below reports the threads actually used.
    torch.set_num_threads(min(os.cpu_count() or 1, 32))
    gb, x, ctx = host_inputs["gb"], host_inputs["x"][:1], host_inputs["ctx"][:1]
    g = ref_cpu.prepare_grounding({k: v[:1] for k, v in gb.items()})
    t = torch.full((1,), 981, dtype=torch.long)
    with torch.no_grad():
        objs, _ = ref_cpu.unifusion(sd, cfg, g)
        t_begin = time.time()
        ref_cpu.unet_forward(sd, cfg, x, t, ctx, objs)              # warm-up (counts against the budget)
        times = []
        if time.time() - t_begin > budget_s / 2:
            times.append(time.time() - t_begin)                     # slow host: the warm-up IS the sample
        while len(times) < 5 and (time.time() - t_begin) < budget_s:
            t0 = time.time()
            ref_cpu.unet_forward(sd, cfg, x, t, ctx, objs)
            times.append(time.time() - t0)
    t_fwd = sorted(times)[len(times) // 2]
    nf = n_forwards(N_INST, S_STEPS, MIS)
    # the extrapolation factor, checked: the port's own Multi-instance Sampler (S = 50, N = 8, mis 0.36, CFG) driven with
    # a forward that only counts its calls (each call = one B = 1 UNet forward of the reference's serial loop)
    class _Counting(ref_cpu.OracleModel):
        def __call__(self, inp):
            self.n_forward += 1
            return torch.zeros_like(inp["x"])
    cm = _Counting(sd, cfg, None)
    x1 = x.clone()
    ins = [dict(x=x1, timesteps=None, context=ctx, grounding_input=g) for _ in range(N_INST + 1)]
    with torch.no_grad():
        ref_cpu.plms_sample_mis(cm, S_STEPS, ins, ctx, GUIDANCE, MIS, alpha_type=None)
    assert cm.n_forward == nf, (cm.n_forward, nf)
    return dict(value=1.0 / (nf * t_fwd), unit="img/s", cores=torch.get_num_threads(), kind="port",
                sample=f"{len(times)} timed full-size UNet forwards (B=1, 64x64 latent, fp32, median {t_fwd:.3f} s) "
                       f"x {nf} forwards/image (extrapolated; {nf} = UNet calls counted in a full S=50 N=8 mis=0.36 run of the "
                       f"port's sampler with a call-counting forward)")


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(out_dir, latents):
    """The sampler's result of the last timed step (latents [images, 4, 64, 64]) -> out_dir/latents.npy, float32.  Beyond
    DUMP_MAX_BYTES a fixed, seeded sample of whole images is written, in image order."""
    import numpy as np
    lat = latents.detach().float()
    per_image = lat[0].numel() * 4
    if lat.shape[0] * per_image > DUMP_MAX_BYTES:
        keep = torch.randperm(lat.shape[0], generator=torch.Generator().manual_seed(0))[:DUMP_MAX_BYTES // per_image]
        lat = lat[keep.sort().values.to(lat.device)]
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "latents.npy"), lat.cpu().numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--images-per-gpu", type=int, default=32)  # 32 images x (8+1) trajectories = 288 units per MIS step
    ap.add_argument("--max-units", type=int, default=128,
                    help="MIS phase-1 (instance, image) units per batched forward (PLMSSamplerInst's default): 128 units x cond/uncond = "
                         "256-row forwards (2 of them + one 64-row forward per MIS step at 32 images; 1.230 ms per row against 1.250 at 128 "
                         "rows, profiles/r06_replay_256.log; 2.037 against 2.013 img/s same-box, profiles/r06_maxunits_ab.log); phase 2 runs "
                         "64-row forwards (one row pair per image)")
    ap.add_argument("--images-total", type=int, default=0,
                    help="strong scaling: fix the GLOBAL images per step (split over the ranks) instead of images per GPU")
    ap.add_argument("--sharding", choices=["auto", "image", "instance"], default="instance",
                    help="MIS phase-1 unit ownership at n_gpus > 1 (host/samplers.py); no effect at 1 GPU")
    ap.add_argument("--dtype", choices=["bf16", "fp16"], default="bf16", help="storage / MFMA input type of the headline run")
    ap.add_argument("--full", action="store_true",
                    help="also measure roofline / executed flops, the CPU baseline and the short extra legs (off: headline only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the latents of the last timed step as DIR/latents.npy (float32)")
    ap.add_argument("--no-alt-dtype", action="store_true", help="skip the short leg in the other 16-bit type")
    ap.add_argument("--no-strong-leg", action="store_true", help="at n_gpus > 1: skip the short strong-scaling leg (8 images total)")
    ap.add_argument("--no-ref-batch-leg", action="store_true", help="at 1 GPU: skip the short leg at the reference's own batch (8 images)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    args = ap.parse_args()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    assert world == args.gpus, f"launch with torch.distributed.run --nproc-per-node {args.gpus} (WORLD_SIZE={world})"
    # test hooks (1-GPU boxes): IDF_BENCH_SINGLE_DEVICE=1 maps every rank to cuda:0 and IDF_DIST_BACKEND=gloo replaces
    # RCCL, so the rank-sharded sampler + collectives can be exercised end-to-end without a multi-GPU node.
    if os.environ.get("IDF_BENCH_SINGLE_DEVICE") == "1":
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    import torch.distributed as dist
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        backend = os.environ.get("IDF_DIST_BACKEND", "nccl")     # "nccl" == RCCL on ROCm
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)

    from instancediffusion_amd.host.alpha import alpha_generator, set_alpha_scale
    from instancediffusion_amd.host.config import SD15_BOX_CFG
    from instancediffusion_amd.host.diffusion import LatentDiffusion
    from instancediffusion_amd.host.samplers import PLMSSamplerInst
    cfg = dict(SD15_BOX_CFG)
    model, sd = build_model(cfg)
    diffusion = LatentDiffusion(linear_start=0.00085, linear_end=0.012, timesteps=1000).to(dev)
    torch_dtype = {"bf16": torch.bfloat16, "fp16": torch.float16}
    nf = n_forwards(N_INST, S_STEPS, MIS)
    if args.images_total:
        assert args.images_total >= 1
    n_images = args.images_total if args.images_total else args.images_per_gpu * world

    def sync():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def run_leg(dtype_name, n_img, steps, warmup, sharding):
        """One measurement: `warmup` untimed + `steps` timed samplings of n_img images; returns (img/s, ms/step, rows)."""
        model.compute_dtype = torch_dtype[dtype_name]
        model.invalidate_engine()
        eng = model.engine                                        # packs the weights into HBM in this storage type
        inputs, uc, gi, host_inputs = make_inputs(cfg, n_img, dev)
        model.grounding_tokenizer_input = gi
        sampler = PLMSSamplerInst(diffusion, model, alpha_generator_func=partial(alpha_generator, type=ALPHA_TYPE),
                                  set_alpha_scale=set_alpha_scale, mis=MIS, max_units=args.max_units, unit_sharding=sharding)
        shape = (n_img, 4, LATENT, LATENT)
        rows = {True: 0, False: 0}                                # forward rows executed on this rank, fuser on / off
        real_forward = eng.forward_cond

        def counting_forward(x, t, cond, out=None, **kw):
            rows[eng.fuser_scale != 0.0] += int(cond.B)               # (a paired forward is handed its n distinct rows; it runs cond.B = 2n)
            return real_forward(x, t, cond, out=out, **kw)
        eng.forward_cond = counting_forward

        def one_step():
            # NOTE (reference quirk kept): the first-conv swap at alpha == 0 is never undone (openaimodel.py:469-480),
            # so every image batch after the first starts with the SD first conv -- same arithmetic cost either way.
            ins = [dict(d) for d in inputs]
            return sampler.sample(S=S_STEPS, shape=shape, input=ins, uc=uc, guidance_scale=GUIDANCE)

        for _ in range(warmup):
            out = one_step()
        sync()
        rows[True] = rows[False] = 0
        t0 = time.perf_counter()
        for _ in range(steps):
            out = one_step()
        sync()
        elapsed = time.perf_counter() - t0
        if world > 1:
            tt = torch.tensor([elapsed, float(rows[True]), float(rows[False])], device=dev, dtype=torch.float64)
            dist.all_reduce(tt[:1], op=dist.ReduceOp.MAX)
            dist.all_reduce(tt[1:], op=dist.ReduceOp.SUM)
            elapsed, rows[True], rows[False] = float(tt[0]), int(tt[1]), int(tt[2])
        assert torch.isfinite(out).all()
        eng.forward_cond = real_forward
        return dict(value=n_img * steps / elapsed, ms_per_step=elapsed / max(steps, 1) * 1e3, images=n_img, steps=steps,
                    rows_on=rows[True], rows_off=rows[False], host_inputs=host_inputs, out=out)

    main_leg = run_leg(args.dtype, n_images, args.steps, args.warmup, args.sharding)
    value = main_leg["value"]
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, main_leg["out"])
    line = None
    if rank == 0:
        line = {
            "metric": "images/sec at 512x512, 50 PLMS steps, N=8 instances (Multi-instance Sampler)",
            "value": round(value, 4), "unit": "img/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(main_leg["ms_per_step"], 2), "higher_is_better": True,
            "scaling": "strong" if args.images_total else "weak", "vs_baseline": None,
            "dtype": args.dtype, "data": "synthetic",
            # what torch.distributed itself reports (the driver's SCALE record can check that RCCL saw N ranks)
            "dist_backend": dist.get_backend() if world > 1 else None,
            "dist_world_size": dist.get_world_size() if world > 1 else 1,
            "config": {"workload": "C3: SD-1.5 InstanceDiffusion UNet (1.228B params, seeded random weights), 64x64 latent "
                                   "(512x512), 50 PLMS steps, CFG 7.5, N=8 boxes, MIS 0.36, alpha [0.8,0,0.2]",
                       "images_per_gpu": None if args.images_total else args.images_per_gpu,
                       "global_images_per_step": n_images, "unet_forwards_per_image": nf,
                       "sharding": args.sharding if world > 1 else "none (1 GPU)",
                       "parallelism": f"MIS (instance, image) units sharded x{world} [{args.sharding}], one RCCL all-gather of the "
                                      f"owned instance latents at the merge; phase 2 sharded over images x{world}"},
            # reference-algorithmic work: every forward the reference runs (406 per image) at its own 1227.3 GFLOP
            "whole_step_algorithmic_tflops_per_gpu": round(value * nf * GFLOP_PER_FWD / 1e3 / world, 1),
            "whole_step_frac_of_mfma_peak": round(value * nf * GFLOP_PER_FWD / 1e3 / world / PEAK_MFMA_TF, 4),
        }
    # ---- --full: measurements with runs of their own (outside the headline's timed region)
    if args.full:
        eng = model.engine
        if rank == 0 and not args.no_roofline:
            phase1_batch = max(eng._slots.keys())
            line["roofline"] = measure_roofline(eng, phase1_batch, True)
            # executed work: what the engine really ran after the exact hoists -- forward ROWS counted in the timed
            # region (first-evaluation de-duplication included) x the GEMM / conv / attention flops of one instrumented row,
            # with the fuser on and off (alpha == 0 steps); UniFusion and the grounding-token K/V run once per conditioning,
            # outside the forwards, and are not counted
            off = measure_roofline(eng, phase1_batch, False)
            f_on = line["roofline"].pop("_flops_per_row")
            f_off = off["_flops_per_row"]
            ex_tf = (main_leg["rows_on"] * f_on + main_leg["rows_off"] * f_off) / 1e12          # all ranks, timed region
            secs = main_leg["ms_per_step"] * 1e-3 * args.steps
            line["executed"] = dict(
                tflop_per_image=round(ex_tf / (n_images * args.steps), 1), reference_tflop_per_image=round(nf * GFLOP_PER_FWD / 1e3, 1),
                forward_rows_per_image=round((main_leg["rows_on"] + main_leg["rows_off"]) / (n_images * args.steps), 1),
                gflop_per_row_fuser_on=round(f_on / 1e9, 1), gflop_per_row_fuser_off=round(f_off / 1e9, 1),
                tflops_per_gpu=round(ex_tf / secs / world, 1), frac_of_mfma_peak=round(ex_tf / secs / world / PEAK_MFMA_TF, 4))
        if rank == 0 and not args.no_cpu_baseline and world == 1:    # reported at N=1 only (the host cores are shared at N>1)
            line["cpu_baseline"] = cpu_baseline(cfg, sd, main_leg["host_inputs"])
        # ---- short extra legs (outside the headline's timed region; each its own warm-up + timed samplings)
        if world > 1 and not args.no_strong_leg and not args.images_total:
            # strong scaling at the reference's own batch: 8 images in total (inference.py num_images), split over the ranks
            k = 8
            leg = run_leg(args.dtype, k, 1, 1, args.sharding)
            if rank == 0:
                ms = int(S_STEPS * MIS)
                p1, p2 = (N_INST + 1) * (ms + 1), S_STEPS - ms                   # forward pairs per image: shardable / per-image serial
                line["strong_scaling_leg"] = dict(global_images=k, value=round(leg["value"], 4), unit="img/s", steps=1, warmup=1,
                                                  ms_per_step=round(leg["ms_per_step"], 2), sharding=args.sharding,
                                                  forward_rows_per_image=round((leg["rows_on"] + leg["rows_off"]) / k, 1),
                                                  # phase 1 spreads over all ranks, phase 2 runs one trajectory per image: with fewer
                                                  # images than ranks only `k` ranks work in phase 2 (and on 2-row forwards)
                                                  amdahl_cap_vs_1gpu=round((p1 + p2) / (p1 / world + p2 / min(world, k)), 2),
                                                  ranks_idle_in_phase2=max(0, world - k))
        if world == 1 and not args.no_ref_batch_leg and not args.images_total and args.images_per_gpu != 8:
            # the reference's own batch: num_images = 8 per prompt (inference.py) on one GPU -- phase 1 runs
            # 72 units as 2 x 64-row + 1 x 16-row forwards per step, phase 2 16-row forwards
            leg = run_leg(args.dtype, 8, 1, 1, args.sharding)
            line["reference_batch_leg"] = dict(global_images=8, value=round(leg["value"], 4), unit="img/s", steps=1, warmup=1,
                                               ms_per_step=round(leg["ms_per_step"], 2),
                                               forward_rows_per_image=round((leg["rows_on"] + leg["rows_off"]) / 8, 1))
        if not args.no_alt_dtype:
            alt = "fp16" if args.dtype == "bf16" else "bf16"
            leg = run_leg(alt, n_images, ALT_STEPS, 1, args.sharding)
            if rank == 0:
                line["alt_dtype_leg"] = dict(dtype=alt, value=round(leg["value"], 4), unit="img/s", steps=ALT_STEPS, warmup=1,
                                             ms_per_step=round(leg["ms_per_step"], 2),
                                             note="same workload in the other 16-bit storage type (the reference's GPU path is fp16 "
                                                  "autocast, inference.py:94); fp16 parity is 10x tighter and the MFMA rate is the "
                                                  "same.  Rounds 2-4 ran this leg 5-6 % behind bf16: the d = 40 attention kept the largest "
                                                  "P of a query at 2^-1 in fp16 (2^-7 in bf16), so any score 2 log2-units above the reference "
                                                  "sent the wave through the exact re-base path; round 5 gives fp16 the same 2^-7 headroom "
                                                  "(attention4.hip RefShift; small P become fp16 denormals, which the conversion produces and "
                                                  "the MFMA consumes exactly)")
    if rank == 0:
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
