"""Test support of ``DDIMSamplerInst`` (the Multi-instance Sampler on DDIM steps).  The reference has no such sampler, so the oracle is a
composition of reference parts: the loop structure of plms_instance.py:86-156 (every input runs the first ``int(S * mis)`` steps on its
own conditioning, serially; merge; the global input runs the rest), with ddim.py:94-131 as the step -- ``ddim_cases.ddim_update_expr``
behind the two model calls, ``ddim_cases.q_sample_blend_expr`` in front of them -- and ``ref_cpu.plms_sample_mis``'s merge.

The noise rule: one draw per IMAGE per step, shared by the image's trajectories; within a step the q_sample draw (when
inpainting), then the step's draw (when sigma != 0); ``noises`` lists the draws in step order.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from tests import ddim_cases

TAG = "tiny_box"                 # inputs of tests/golden/tiny_box.pt: batch 2, N = 2 instances, S = 5, alpha_type [1, 0, 0]
S, MIS, GUIDANCE = 5, 0.4, 7.5   # phase 1 = steps 0, 1
CASES = {"eta0": (0.0, False), "eta0.5": (0.5, False), "eta0.5_mask": (0.5, True)}
NOISE_SEED = 2468


def n_draws(S: int, eta: float, masked: bool) -> int:
    """Draws of one call: S q_sample draws with a mask, S step draws at eta > 0 (every sigma of a schedule with eta > 0 is > 0)."""
    return S * (int(masked) + int(eta != 0))


def make_noises(shape, S: int, eta: float, masked: bool, seed: int = NOISE_SEED) -> List[torch.Tensor]:
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(tuple(shape), generator=g) for _ in range(n_draws(S, eta, masked))]


def make_inpaint(shape, seed: int = ddim_cases.MASK_SEED):
    """(mask [B, 1, H, W] of zeros and ones with both present in every image, x0 [B, 4, H, W])."""
    g = torch.Generator().manual_seed(seed)
    mask = (torch.rand(shape[0], 1, *shape[2:], generator=g) > 0.5).float()
    mask[:, :, 0, 0], mask[:, :, -1, -1] = 1.0, 0.0
    return mask, torch.randn(tuple(shape), generator=g)


def replay(sampler, noises):
    """Feed ``noises`` through ``noise_fn``; -> the list the draws are recorded in."""
    drawn, it = [], iter(noises)

    def noise_fn(shape):
        n = next(it)
        assert tuple(n.shape) == tuple(shape), (tuple(n.shape), tuple(shape))
        drawn.append(n)
        return n.clone()
    sampler.noise_fn = noise_fn
    return drawn


def ddim_mis_reference(model, S: int, inputs: List[dict], uc, guidance_scale: float, mis: float, eta: float = 0.0,
                       alpha_type: Optional[Sequence[float]] = None, mask=None, x0=None, noises=None,
                       crop_and_paste: bool = False) -> torch.Tensor:
    """``model``: oracle.ref_cpu.OracleModel, a fresh one per call (it caches tokens under the ``id`` of the grounding dicts, which
    must not outlive them); ``inputs``: [global, instance 1, ..] as ``ref_cpu.plms_sample_mis`` takes them."""
    from oracle import ref_cpu
    steps, a, a_prev, sigmas, s1m = ddim_cases.ddim_schedule(S, eta)
    time_range = np.flip(steps)
    total = steps.shape[0]
    b = inputs[0]["x"].shape[0]
    latent_size = inputs[0]["x"].shape[2]
    alphas = ref_cpu.alpha_generator(len(time_range), alpha_type) if alpha_type is not None else None
    mis_step = int(total * mis)
    # the draws, in step order: per step the q_sample draw, then the step's
    it = iter(noises if noises is not None else [])
    q_noise, step_noise = {}, {}
    for i in range(total):
        if mask is not None:
            q_noise[i] = next(it)
        if float(np.float32(sigmas[total - i - 1])) != 0:
            step_noise[i] = next(it)
    assert next(it, None) is None, "every draw has its step"

    def step_of(inp, i):
        step = int(time_range[i])
        index = total - i - 1
        inp["timesteps"] = torch.full((b,), step, dtype=torch.long)
        if mask is not None:                                                      # ddim.py:94-98
            ac = torch.tensor(ref_cpu.alphas_cumprod(), dtype=torch.float32)      # ref_cpu.q_sample's coefficients (ldm.py:17-20)
            inp["x"] = ddim_cases.q_sample_blend_expr(x0, q_noise[i], mask, inp["x"], float(ac.sqrt()[step]), float((1.0 - ac).sqrt()[step]))
        e_t = model(inp)                                                          # ddim.py:110-114
        e_uc = None
        if uc is not None and guidance_scale != 1:
            e_uc = model(dict(x=inp["x"], timesteps=inp["timesteps"], context=uc))
        inp["x"], _ = ddim_cases.ddim_update_expr(inp["x"], e_t, e_uc, guidance_scale, a[index], a_prev[index], sigmas[index], s1m[index],
                                                  step_noise.get(i))

    for inp in inputs:                                                            # plms_instance.py:86-104
        for i in range(mis_step):
            ref_cpu._step_common(model, alphas, i)
            step_of(inp, i)
    base = inputs[0]
    if crop_and_paste:                                                            # :128-135
        for src in inputs[1:]:
            base["x"] = ref_cpu.crop_paste(base["x"], src["x"], src["grounding_input"]["boxes"][0][0].tolist(), latent_size)
    else:
        base["x"] = torch.mean(torch.stack([i["x"] for i in inputs]), dim=0)
    for i in range(mis_step, total):                                              # :138-156
        ref_cpu._step_common(model, alphas, i)
        step_of(base, i)
    return base["x"]
