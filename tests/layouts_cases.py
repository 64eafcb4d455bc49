"""The heterogeneous-layout sampler case shared by tests/make_layouts_golden.py (which feeds it to the unmodified reference) and the
``sample_layouts`` tests: four layouts with N = 0, 1, 3, 2 instances, each with its own seeded boxes, contexts and start noise; one
layout has two images.  torch only at module level; ``synth`` (instancediffusion_amd/synth.py) is handed in, because the generator
imports it by path while the reference tree owns the ``ldm`` package name."""
from __future__ import annotations

import torch

TAG = "tiny_box_layouts"
CFG, VARIANT, LATENT, S, MIS, ALPHA_TYPE, GUIDANCE = "test_box.yaml", "tiny", 16, 5, 0.4, [1, 0, 0], 7.5
SEG_SIZE = 512
LAYOUTS = [                       # seed, instances (MIS trajectories beside the global one), boxes in the global grounding, images
    dict(seed=2101, n_inst=0, n_boxes=2, images=1),
    dict(seed=2102, n_inst=1, n_boxes=1, images=1),
    dict(seed=2103, n_inst=3, n_boxes=3, images=2),
    dict(seed=2104, n_inst=2, n_boxes=2, images=1),
]


def build_layout(spec: dict, synth) -> dict:
    """x [images,4,L,L], context / uc [1,77,768], the global grounding batch (batch 1) and one context per instance."""
    g = torch.Generator().manual_seed(spec["seed"])
    bx = synth.random_boxes(spec["n_boxes"], g)
    gb = synth.make_grounding_batch(1, bx, g, with_scribbles=False, with_polygons=False, with_segs=False, seg_size=SEG_SIZE)
    x = torch.randn(spec["images"], 4, LATENT, LATENT, generator=g)
    context = torch.randn(1, 77, 768, generator=g)
    uc = torch.randn(1, 77, 768, generator=g)
    inst_ctx = [torch.randn(1, 77, 768, generator=g) for _ in range(spec["n_inst"])]
    return dict(x=x, context=context, uc=uc, gb=gb, inst_ctx=inst_ctx)


def input_all(data: dict, x: torch.Tensor, prepare, synth) -> list:
    """The MIS ``input_all`` list of one layout with start latents ``x``; ``prepare`` = GroundingNetInput.prepare."""
    out = [dict(x=x.clone(), timesteps=None, context=data["context"], grounding_input=prepare(data["gb"]))]
    for i, ctx in enumerate(data["inst_ctx"]):
        out.append(dict(x=x.clone(), timesteps=None, context=ctx, grounding_input=prepare(synth.instance_batch(data["gb"], i))))
    prepare(data["gb"])
    return out
