#!/usr/bin/env python
"""Conditioning set-up with instance masks: ``prepare_layout_inputs`` with the masks decoded on the host (numpy decode + Pillow NEAREST,
one 30 x 512 x 512 fp32 stack assembled and uploaded per conditioning row) against the device route (run lengths uploaded, ONE
``idf_rle_decode_planes`` launch for all rows of the call).

    python tools/mask_input_bench.py [--layouts 32] [--runs 5] [--out profiles/mask_input_bench.json]

The workload is the layout mix of tools/layouts_bench.py (L layouts, instance counts cycling through 2 .. 8, seeded boxes), every
instance carrying one of the eight demo masks of tests/golden/rle_masks.json, round-robin; both routes build the input of
``PLMSSamplerInst.sample_layouts`` (a global row and one row per instance for every layout).  Both run in ONE process, alternated
(host, device, host, device, ..) after one untimed round of each; reported: the median seconds of each over the runs, their spread, and
the bytes of mask data each puts on the bus, and how many real device allocations each timed round made (0 when the caching allocator
serves the round from what the untimed rounds left; anything else is allocation time, not set-up work, and says so).  The kernel alone is timed with events around 20 launches over tables that are already
on the device, next to a fill of the same output bytes (the HBM write rate this process reaches).  Prints one JSON line and writes it
to ``--out``.  Nothing here is a pass / fail bar."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

MAX_OBJS, SIZE, LATENT = 30, 512, 64


class Text:
    """Seeded stand-ins for the text encoders: their cost is the same on both routes and not what is measured."""

    def encode(self, prompts):
        return torch.zeros(len(prompts), 77, 768)

    def pooled(self, phrase):
        return torch.ones(768)


def make_metas(n_layouts):
    from instancediffusion_amd import synth
    from instancediffusion_amd.host.input import meta_from_demo_json
    masks = json.load(open(os.path.join(REPO, "tests", "golden", "rle_masks.json")))["masks"]
    metas, counts, k = [], [], 0
    for l in range(n_layouts):
        n = 2 + l % 7                                                     # 2 .. 8 instances, as tools/layouts_bench.py
        g = torch.Generator().manual_seed(9000 + l)
        annos = []
        for x0, y0, x1, y1 in synth.random_boxes(n, g).tolist():
            m = masks[k % len(masks)]
            k += 1
            annos.append(dict(bbox=[x0 * SIZE, y0 * SIZE, (x1 - x0) * SIZE, (y1 - y0) * SIZE], caption=f"instance {k}",
                              mask=dict(size=m["size"], counts=m["counts"])))
        metas.append(meta_from_demo_json(dict(caption=f"layout {l}", width=SIZE, height=SIZE, annos=annos), 0.75, instance_masks="json"))
        counts.append(n)
    return metas, counts


def kernel_alone(ops, metas, launches=20):
    """Events around ``launches`` launches of the call's one kernel (tables resident), and around as many fills of its output."""
    from instancediffusion_amd.host.masks import pack_masks
    parsed, dst, row = [], [], 0
    for meta in metas:                                                    # the rows prepare_layout_inputs(instances=True) forms
        for k, r in enumerate(meta["rle"]):
            parsed.append(r)
            dst.append(row * MAX_OBJS + k)
        row += 1
        for r in meta["rle"]:
            parsed.append(r)
            dst.append(row * MAX_OBJS)
            row += 1
    row = min(row, 256)                                                   # one launch addresses < 2^31 elements
    keep = [j for j, d in enumerate(dst) if d < row * MAX_OBJS]
    t = pack_masks([parsed[j] for j in keep], SIZE)
    M = len(keep)
    ints = torch.from_numpy(np.concatenate([t["run_begin"], t["run_end"], t["src_hw"].reshape(-1), np.asarray([dst[j] for j in keep], np.int32),
                                            t["ends"].view(np.int32)])).cuda()
    out = torch.zeros(row, MAX_OBJS, SIZE, SIZE, device="cuda")
    area = torch.zeros(M, dtype=torch.int32, device="cuda")
    at = lambda k: C.c_void_p(ints.data_ptr() + 4 * k * M)                # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def launch():
        rc = ops.lib.idf_rle_decode_planes(C.c_void_p(ints.data_ptr() + 20 * M), int(t["ends"].size), at(0), at(1), at(2), at(4), M,
                                           C.c_void_p(out.data_ptr()), row * MAX_OBJS, SIZE, C.c_void_p(area.data_ptr()), st)
        assert rc == 0, rc

    def events(fn):
        fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e-3 / launches
    written = M * SIZE * SIZE * 4                                         # the planes the jobs name
    t_kernel = events(launch)
    planes = torch.empty(M, SIZE, SIZE, device="cuda")
    t_fill = events(lambda: planes.fill_(1.0))
    t_zero = events(lambda: out.zero_())
    return dict(jobs=M, rows=row, runs=int(t["ends"].size), launches=launches, kernel_s=t_kernel, kernel_bytes_written=written,
                kernel_write_GBps=round(written / t_kernel / 1e9, 1), fill_same_bytes_s=t_fill,
                fill_write_GBps=round(written / t_fill / 1e9, 1), kernel_over_fill=round(t_kernel / t_fill, 3),
                zero_fill_of_all_rows_s=t_zero, zero_fill_bytes=out.numel() * 4, zero_fill_GBps=round(out.numel() * 4 / t_zero / 1e9, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layouts", type=int, default=32)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(REPO, "profiles", "mask_input_bench.json"))
    args = ap.parse_args()
    assert args.runs >= 5, "median of at least 5 runs"
    from grounding_input.text_grounding_tokinzer_input import GroundingNetInput
    from instancediffusion_amd.host.input import prepare_layout_inputs
    from instancediffusion_amd.host.masks import table_bytes
    from instancediffusion_amd.ops import HipOps
    ops = HipOps()
    metas, counts = make_metas(args.layouts)
    noises = [torch.zeros(1, 4, LATENT, LATENT, device="cuda") for _ in metas]
    text = Text()
    rows = sum(c + 1 for c in counts)
    uploaded = []
    real = ops.rle_decode_planes
    ops.rle_decode_planes = lambda table, *a, **k: (uploaded.append(table_bytes(table)), real(table, *a, **k))[1]

    mallocs = {None: [], ops: []}

    def run(route_ops):
        torch.cuda.synchronize()
        before = torch.cuda.memory_stats().get("num_device_alloc", 0)
        t0 = time.perf_counter()
        lay = prepare_layout_inputs(metas, noises, GroundingNetInput(), text, text, instances=True, max_objs=MAX_OBJS, device="cuda",
                                    ops=route_ops)
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        mallocs[route_ops].append(torch.cuda.memory_stats().get("num_device_alloc", 0) - before)   # allocator misses: real device allocations
        return t, lay
    t, host = run(None)                                                   # untimed round of each
    print(f"[mask_input_bench] warm-up: host {t:.3f} s", file=sys.stderr, flush=True)
    t, dev = run(ops)
    print(f"[mask_input_bench] warm-up: device {t:.3f} s", file=sys.stderr, flush=True)
    same = all(torch.equal(a["grounding_input"]["segs"], b["grounding_input"]["segs"]) for la, lb in zip(host, dev) for a, b in zip(la, lb))
    launches_per_call, table = len(uploaded), uploaded[-1]
    del host, dev
    th, td = [], []
    mallocs[None].clear(), mallocs[ops].clear()
    for _ in range(args.runs):
        th.append(run(None)[0])
        td.append(run(ops)[0])
        print(f"[mask_input_bench] host {th[-1]:.3f} s, device {td[-1]:.3f} s", file=sys.stderr, flush=True)
    torch.cuda.empty_cache()
    mh, md = statistics.median(th), statistics.median(td)
    stack = MAX_OBJS * SIZE * SIZE * 4
    res = dict(metric="conditioning set-up with instance masks: prepare_layout_inputs(instances=True), masks decoded on the host vs on the device",
               layouts=args.layouts, instance_counts=counts, rows=rows, masks=sum(counts), runs=args.runs,
               host_s=round(mh, 4), device_s=round(md, 4), host_all_s=[round(t, 4) for t in th], device_all_s=[round(t, 4) for t in td],
               host_spread=round((max(th) - min(th)) / mh, 4), device_spread=round((max(td) - min(td)) / md, 4),
               speedup_host_over_device=round(mh / md, 3), host_min_s=round(min(th), 4), device_min_s=round(min(td), 4),
               host_device_allocations_per_round=list(mallocs[None]), device_device_allocations_per_round=list(mallocs[ops]),
               host_mask_bytes_uploaded=rows * stack, device_mask_bytes_uploaded=table,
               upload_ratio=round(rows * stack / table, 1), device_launches_per_call=launches_per_call, routes_bit_identical=bool(same),
               kernel=kernel_alone(ops, metas), device=torch.cuda.get_device_name(0))
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
