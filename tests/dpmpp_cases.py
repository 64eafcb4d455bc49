"""DPM-Solver++(2M) test support: the fp32 torch expression ``idf_dpmpp_update`` must reproduce bit for bit, and composed CPU fp32
oracles of ``DPMSolverSampler`` / ``DPMSolverSamplerInst`` over ``oracle/ref_cpu.OracleModel``.  The reference has no DPM solver, so
the oracles are compositions: ``ddim_cases.ddim_reference`` / ``ddim_mis_cases.ddim_mis_reference``'s loops (the reference's ddim.py
and plms_instance.py structure) with the step of Lu et al. 2022, "DPM-Solver++", Algorithm 2 (data-prediction form) -- its
coefficients restated here in float64, independently of ``host/samplers.dpmpp_coeffs``.

Only torch / numpy are imported at module level (tests/make_dpmpp_golden.py loads this file); the repository's modules are imported
inside the functions that need them.
"""
from __future__ import annotations

import os
from typing import List, Optional, Sequence

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")

TAG = "tiny_box"                 # inputs of tests/golden/tiny_box.pt: batch 2, N = 2 instances, S = 5, alpha_type [1, 0, 0]
S, MIS, GUIDANCE = 5, 0.4, 7.5   # phase 1 = steps 0, 1
NOISE_SEED = 1357
FLOOR_GOLDEN = "dpmpp_floor.pt"  # tests/make_dpmpp_golden.py


# ---- the kernel's reference expression ------------------------------------------------------------------------------
def dpmpp_update_expr(x, e_cond, e_uncond, guidance, sqrt_at, sqrt_1m_at, c_x, c_0, c_1, x0_last):
    """-> (x_prev, x0_t): every operation torch's fp32 one, in the kernel's order; the coefficients are one-element fp32 tensors."""
    def full(v):
        return torch.full((1,) * x.dim(), float(v), dtype=torch.float32)
    e = e_cond
    if e_uncond is not None:
        e = e_uncond + guidance * (e_cond - e_uncond)
    p = (x - full(sqrt_1m_at) * e) / full(sqrt_at)
    r = full(c_x) * x + full(c_0) * p
    if x0_last is not None:
        r = r + full(c_1) * x0_last
    return r, p


# ---- the schedule and the coefficients, restated --------------------------------------------------------------------
def _lambda(a):
    a = np.float64(a)
    return 0.5 * (np.log(a) - np.log1p(-a))


def timesteps(S: int, discretize: str) -> np.ndarray:
    from oracle import ref_cpu
    if discretize == "uniform":
        return ref_cpu._schedule(S)[0]
    assert discretize == "logsnr"
    ac = torch.tensor(ref_cpu.alphas_cumprod(), dtype=torch.float32).numpy().astype(np.float64)
    T = ac.shape[0]
    if S == 1:
        return np.asarray([T - 1])
    lam = _lambda(ac)
    t = []
    for target in np.linspace(lam[1], lam[T - 1], S):
        d = np.abs(lam[1:] - target)
        t.append(1 + int(np.flatnonzero(d == d.min())[0]))
    for k in range(1, S):
        t[k] = max(t[k], t[k - 1] + 1)
    t[-1] = min(t[-1], T - 1)
    for k in range(S - 2, -1, -1):
        t[k] = min(t[k], t[k + 1] - 1)
    return np.asarray(t)


def schedule(S: int, discretize: str = "uniform"):
    """-> timesteps (ascending), a, a_prev (float32, as the reference's buffers), sqrt(a), sqrt(1 - a) (float32)."""
    from oracle import ref_cpu
    steps = timesteps(S, discretize)
    ac32 = torch.tensor(ref_cpu.alphas_cumprod(), dtype=torch.float32)
    a = ac32[steps].numpy()
    a_prev = np.asarray([ac32[0].item()] + ac32[steps[:-1]].tolist(), dtype=np.float32)
    return steps, a, a_prev, np.sqrt(a), np.sqrt(np.float32(1.0) - a)


def coeffs(a_t, a_prev, a_last=None):
    """Algorithm 2 of the paper in float64, written with expm1 / log1p (another route than the code under test), rounded once."""
    a_t, a_prev = np.float64(np.float32(a_t)), np.float64(np.float32(a_prev))
    h = _lambda(a_prev) - _lambda(a_t)
    bc = -np.sqrt(a_prev) * np.expm1(-h)
    c_x = np.sqrt((1.0 - a_prev) / (1.0 - a_t))
    if a_last is None:
        return np.float32(c_x), np.float32(bc), np.float32(0.0)
    r = (_lambda(a_t) - _lambda(np.float64(np.float32(a_last)))) / h
    return np.float32(c_x), np.float32(bc * (1.0 + 0.5 / r)), np.float32(-bc * 0.5 / r)


# ---- noise and inpainting inputs ------------------------------------------------------------------------------------
def make_noises(shape, S: int, masked: bool, seed: int = NOISE_SEED) -> List[torch.Tensor]:
    """The draws of one call: S q_sample draws with a mask, none without."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(tuple(shape), generator=g) for _ in range(S if masked else 0)]


def _step(model, inp, uc, guidance_scale, sched, i, hist, order, mask, x0, q_noise):
    """One step on ``inp`` in place: the blend, the two model calls, the update; ``hist``: [] or [the last x0 prediction]."""
    from oracle import ref_cpu
    from tests import ddim_cases
    steps, a, a_prev, sqrt_a, s1m = sched
    total = steps.shape[0]
    index = total - i - 1
    step = int(steps[index])
    b = inp["x"].shape[0]
    inp["timesteps"] = torch.full((b,), step, dtype=torch.long)
    if mask is not None:
        ac = torch.tensor(ref_cpu.alphas_cumprod(), dtype=torch.float32)
        inp["x"] = ddim_cases.q_sample_blend_expr(x0, q_noise, mask, inp["x"], float(ac.sqrt()[step]), float((1.0 - ac).sqrt()[step]))
    e_t = model(inp)
    e_uc = None
    if uc is not None and guidance_scale != 1:
        e_uc = model(dict(x=inp["x"], timesteps=inp["timesteps"], context=uc))
    last = hist[0] if (order == 2 and hist) else None
    c = coeffs(a[index], a_prev[index], a[index + 1] if last is not None else None)
    inp["x"], p = dpmpp_update_expr(inp["x"], e_t, e_uc, guidance_scale, sqrt_a[index], s1m[index], *c, last)
    hist[:] = [p]


def dpmpp_reference(model, S: int, input: dict, uc, guidance_scale: float, order: int = 2, discretize: str = "uniform",
                    alpha_type: Optional[Sequence[float]] = None, mask=None, x0=None, noises=None) -> torch.Tensor:
    """``DPMSolverSampler.sample`` on the CPU in fp32.  ``noises``: the q_sample draws in step order (with a mask)."""
    from oracle import ref_cpu
    sched = schedule(S, discretize)
    total = sched[0].shape[0]
    alphas = ref_cpu.alpha_generator(total, alpha_type) if alpha_type is not None else None
    hist: list = []
    for i in range(total):
        ref_cpu._step_common(model, alphas, i)
        _step(model, input, uc, guidance_scale, sched, i, hist, order, mask, x0, noises[i] if mask is not None else None)
    return input["x"]


def dpmpp_mis_reference(model, S: int, inputs: List[dict], uc, guidance_scale: float, mis: float, order: int = 2,
                        discretize: str = "uniform", alpha_type: Optional[Sequence[float]] = None, mask=None, x0=None, noises=None,
                        crop_and_paste: bool = False) -> torch.Tensor:
    """``DPMSolverSamplerInst.sample``: the loop structure of plms_instance.py:86-156 (every input runs the first ``int(S * mis)``
    steps on its own conditioning, serially; ``ref_cpu``'s merge; the global input runs the rest WITH ITS OWN history, as PLMS's eps
    history continues there).  ``model``: a fresh ``OracleModel`` per call (see ``ddim_mis_cases.ddim_mis_reference``)."""
    from oracle import ref_cpu
    sched = schedule(S, discretize)
    total = sched[0].shape[0]
    latent_size = inputs[0]["x"].shape[2]
    alphas = ref_cpu.alpha_generator(total, alpha_type) if alpha_type is not None else None
    mis_step = int(total * mis)
    hists = [[] for _ in inputs]
    for inp, hist in zip(inputs, hists):
        for i in range(mis_step):
            ref_cpu._step_common(model, alphas, i)
            _step(model, inp, uc, guidance_scale, sched, i, hist, order, mask, x0, noises[i] if mask is not None else None)
    base = inputs[0]
    if crop_and_paste:
        for src in inputs[1:]:
            base["x"] = ref_cpu.crop_paste(base["x"], src["x"], src["grounding_input"]["boxes"][0][0].tolist(), latent_size)
    else:
        base["x"] = torch.mean(torch.stack([i["x"] for i in inputs]), dim=0)
    for i in range(mis_step, total):
        ref_cpu._step_common(model, alphas, i)
        _step(model, base, uc, guidance_scale, sched, i, hists[0], order, mask, x0, noises[i] if mask is not None else None)
    return base["x"]
