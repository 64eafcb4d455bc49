"""img2img / hi-res test support: the fixed resize expression ``idf_resize_planes`` must reproduce bit for bit, the torch expression of
``idf_q_sample``, CPU fp32 restatements of the three single-trajectory samplers that ENTER the schedule at step ``start``
(``ref_cpu.plms_sample`` / ``ddim_cases.ddim_reference`` / ``dpmpp_cases.dpmpp_reference`` with the loop begun at ``start`` and an
empty history), and the composed oracles of an img2img run and of a first pass + hi-res second pass.  TEST INFRASTRUCTURE.

Only torch / numpy are imported at module level (tests/make_hires_golden.py loads this file); the repository's modules are imported
inside the functions that need them.
"""
from __future__ import annotations

import os
from typing import Optional, Sequence

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")

TAG = "tiny_box"                  # inputs of tests/golden/tiny_box.pt: batch 2, 16 x 16 latents, S = 5, alpha_type [1, 0, 0]
S, GUIDANCE = 5, 7.5
STRENGTH, START = 0.6, 2          # floor(5 * 0.6 + 1e-6) = 3 steps run: the schedule is entered at step 2
HIRES_SIZE = (24, 24)             # 16^2 -> 24^2: scale 1.5, as 64^2 -> 96^2
SEED = 2468                       # the img2img x0 and every q_sample draw of these cases
FLOOR_GOLDEN = "hires_floor.pt"   # tests/make_hires_golden.py
SAMPLERS = ("plms", "ddim", "dpmpp")   # PLMS, DDIM eta 0, DPM-Solver++ order 2
U = 2.0 ** -24                    # unit roundoff of fp32

# (Hi, Wi, Ho, Wo): the sizes the table formula was checked on against F.interpolate on float64 input
TABLE_SIZES = [(16, 16, 24, 24), (8, 12, 20, 17), (64, 64, 96, 96), (64, 64, 128, 128), (3, 3, 64, 64), (7, 9, 3, 31), (16, 16, 8, 8),
               (1, 1, 4, 4), (16, 16, 16, 16)]


# ---- the kernels' reference expressions -----------------------------------------------------------------------------
def q_sample_expr(x0, noise, sqrt_ac, sqrt_1m_ac):
    """ldm.py:17-20 as torch evaluates it in fp32 (the coefficient gathered per sample: one value for the whole batch here)."""
    shape = (x0.shape[0],) + (1,) * (x0.dim() - 1) if x0.dim() > 1 else (1,)
    a = torch.full(shape, float(sqrt_ac), dtype=torch.float32)
    b = torch.full(shape, float(sqrt_1m_ac), dtype=torch.float32)
    return a * x0 + b * noise


def apply_tables(src, xi, xw, yi, yw, dtype=torch.float32):
    """The fixed expression of ``idf_resize_planes`` (include/idf.h) over given tables, every operation a separate torch operation in
    ``dtype``; every tap index clamped to [0, n - 1]:
      row_j = ((s[r_j][c_0] xw_0 + s[r_j][c_1] xw_1) + s[r_j][c_2] xw_2) + s[r_j][c_3] xw_3
      out   = ((row_0 yw_0 + row_1 yw_1) + row_2 yw_2) + row_3 yw_3
    src [.., Hi, Wi]; xi int [Wo], xw [Wo, taps], yi int [Ho], yw [Ho, taps] (numpy or torch)."""
    xi, yi = torch.as_tensor(np.asarray(xi)).to(torch.int64), torch.as_tensor(np.asarray(yi)).to(torch.int64)
    xw, yw = torch.as_tensor(np.asarray(xw)).to(dtype), torch.as_tensor(np.asarray(yw)).to(dtype)
    Hi, Wi = src.shape[-2], src.shape[-1]
    taps = xw.shape[1]
    s = src.to(dtype)
    out = None
    for j in range(taps):
        r = (yi + j).clamp(0, Hi - 1)
        row = None
        for k in range(taps):
            c = (xi + k).clamp(0, Wi - 1)
            term = s[..., r[:, None], c[None, :]] * xw[None, :, k]
            row = term if row is None else row + term
        v = row * yw[:, j, None]
        out = v if out is None else out + v
    return out


def resize_expr(src, size, mode, dtype=torch.float32):
    """``apply_tables`` over ``host.hires.resize_tables``: float32 = what the kernel must give bit for bit; float64 = the fp32-rounded
    weights with (nearly) exact sums, to be held against ``F.interpolate`` on float64 input."""
    from instancediffusion_amd.host.hires import resize_tables
    xi, xw = resize_tables(src.shape[-1], size[1], mode)
    yi, yw = resize_tables(src.shape[-2], size[0], mode)
    return apply_tables(src, xi, xw, yi, yw, dtype)


def interpolate64(src, size, mode):
    """torch's own resize on float64 input (its fp32 path computes the source coordinate in fp32: not a reference)."""
    x = src.double()
    lead = x.shape[:-2]
    y = torch.nn.functional.interpolate(x.reshape(1, -1, *x.shape[-2:]), size=tuple(size), mode=mode, align_corners=False)
    return y.reshape(*lead, *size)


# ---- the samplers, restated with a start ----------------------------------------------------------------------------
def _alphas(total, alpha_type, alphas):
    from oracle import ref_cpu
    if alphas is not None:
        assert len(alphas) == total
        return list(alphas)
    return ref_cpu.alpha_generator(total, alpha_type) if alpha_type is not None else None


def plms_reference(model, S: int, inp: dict, uc, guidance_scale: float, start: int = 0,
                   alpha_type: Optional[Sequence[float]] = None, alphas=None) -> torch.Tensor:
    """``ref_cpu.plms_sample`` (plms.py:66-113) entered at step ``start``: absolute index, timestep and alpha, an empty eps history."""
    from oracle import ref_cpu
    steps, a, a_prev = ref_cpu._schedule(S)
    time_range = np.flip(steps)
    total = steps.shape[0]
    b = inp["x"].shape[0]
    al = _alphas(total, alpha_type, alphas)
    old_eps: list = []
    img = inp["x"]
    for i in range(start, total):
        ref_cpu._step_common(model, al, i)
        ts = torch.full((b,), int(time_range[i]), dtype=torch.long)
        ts_next = torch.full((b,), int(time_range[min(i + 1, total - 1)]), dtype=torch.long)
        img, e_t = ref_cpu._p_sample_plms(model, inp, ts, total - i - 1, a, a_prev, uc, guidance_scale, old_eps, ts_next)
        inp["x"] = img
        old_eps.append(e_t)
        if len(old_eps) >= 4:
            old_eps.pop(0)
    return img


def ddim_reference(model, S: int, inp: dict, uc, guidance_scale: float, start: int = 0, eta: float = 0.0,
                   alpha_type: Optional[Sequence[float]] = None, alphas=None, mask=None, x0=None, noises=None) -> torch.Tensor:
    """``ddim_cases.ddim_reference`` (ddim.py:25-131) entered at step ``start``.  ``noises``: the draws of steps start .. S-1 in
    ``DDIMSampler``'s order (per step the q_sample draw with a mask, then the step's draw where sigma != 0)."""
    from oracle import ref_cpu
    from tests import ddim_cases
    steps, a, a_prev, sigmas, s1m = ddim_cases.ddim_schedule(S, eta)
    it = iter(noises or [])
    time_range = np.flip(steps)
    total = steps.shape[0]
    b = inp["x"].shape[0]
    al = _alphas(total, alpha_type, alphas)
    ac = torch.tensor(ref_cpu.alphas_cumprod(), dtype=torch.float32)
    img = inp["x"]
    for i in range(start, total):
        ref_cpu._step_common(model, al, i)
        index, step = total - i - 1, int(time_range[i])
        inp["timesteps"] = torch.full((b,), step, dtype=torch.long)
        if mask is not None:
            img = ddim_cases.q_sample_blend_expr(x0, next(it), mask, img, float(ac.sqrt()[step]), float((1.0 - ac).sqrt()[step]))
            inp["x"] = img
        e_t = model(inp)
        e_uc = None
        if uc is not None and guidance_scale != 1:
            e_uc = model(dict(x=inp["x"], timesteps=inp["timesteps"], context=uc))
        sigma = float(np.float32(sigmas[index]))
        img, _ = ddim_cases.ddim_update_expr(inp["x"], e_t, e_uc, guidance_scale, a[index], a_prev[index], sigma, s1m[index],
                                             next(it) if sigma != 0 else None)
        inp["x"] = img
    return img


def dpmpp_reference(model, S: int, inp: dict, uc, guidance_scale: float, start: int = 0, order: int = 2,
                    alpha_type: Optional[Sequence[float]] = None, alphas=None, mask=None, x0=None, noises=None) -> torch.Tensor:
    """``dpmpp_cases.dpmpp_reference`` entered at step ``start``: the step at ``start`` is first order.  ``noises``: the q_sample draws
    of steps start .. S-1 (with a mask)."""
    from oracle import ref_cpu
    from tests import dpmpp_cases
    sched = dpmpp_cases.schedule(S, "uniform")
    total = sched[0].shape[0]
    al = _alphas(total, alpha_type, alphas)
    hist: list = []
    for i in range(start, total):
        ref_cpu._step_common(model, al, i)
        dpmpp_cases._step(model, inp, uc, guidance_scale, sched, i, hist, order, mask, x0, noises[i - start] if mask is not None else None)
    return inp["x"]


def reference(kind: str, model, S, inp, uc, guidance_scale, start=0, **kw):
    """The restated sampler ``kind`` of SAMPLERS: PLMS, DDIM eta 0, DPM-Solver++ order 2."""
    if kind == "plms":
        return plms_reference(model, S, inp, uc, guidance_scale, start, **kw)
    if kind == "ddim":
        return ddim_reference(model, S, inp, uc, guidance_scale, start, eta=0.0, **kw)
    assert kind == "dpmpp"
    return dpmpp_reference(model, S, inp, uc, guidance_scale, start, order=2, **kw)


# ---- composed oracles -----------------------------------------------------------------------------------------------
def timestep_of(S: int, start: int) -> int:
    from oracle import ref_cpu
    return int(np.flip(ref_cpu._schedule(S)[0])[start])


def seeded(shape, seed=SEED, n=1):
    g = torch.Generator().manual_seed(seed)
    out = [torch.randn(tuple(shape), generator=g) for _ in range(n)]
    return out[0] if n == 1 else out


def q_sample_at(x0, S, start, noise):
    """x0 noised to the timestep of step ``start``: ``ref_cpu.q_sample`` (the float32 full-table coefficients)."""
    from oracle import ref_cpu
    t = torch.full((x0.shape[0],), timestep_of(S, start), dtype=torch.long)
    return ref_cpu.q_sample(x0, t, noise)


CASES = ("img2img", "hires")      # the two parity cases of tests/test_hires_sampler_gpu.py (floors: tests/make_hires_golden.py)


def case_tensors(case: str, shape):
    """The seeded tensors of a parity case at latent ``shape``: img2img -> (x0, q_sample noise); hires -> the q_sample noise at
    HIRES_SIZE."""
    if case == "img2img":
        return seeded(shape, SEED), seeded(shape, SEED + 1)
    assert case == "hires"
    return seeded((shape[0], shape[1]) + HIRES_SIZE, SEED + 2)


def img2img_reference(kind, model, inp: dict, uc, x0, noise, S=S, start=START, guidance_scale=GUIDANCE, **kw):
    """img2img: q_sample of ``x0`` with ``noise`` at step ``start``'s timestep, then the restated sampler from ``start``."""
    inp = dict(inp, x=q_sample_at(x0, S, start, noise), timesteps=None)
    return reference(kind, model, S, inp, uc, guidance_scale, start, **kw)


def hires_reference(kind, model, inp: dict, uc, noise, size=HIRES_SIZE, mode="bicubic", S=S, start=START, guidance_scale=GUIDANCE,
                    first=None, **kw):
    """First pass (the restated sampler from step 0 on ``inp``; ``first``: its result when the caller has it) + the second pass:
    ``F.interpolate`` on float64 input rounded to fp32, q_sample with ``noise``, the restated sampler from ``start`` at the new size.
    -> (first pass latents, final latents)."""
    if first is None:
        first = reference(kind, model, S, dict(inp, x=inp["x"].clone(), timesteps=None), uc, guidance_scale, 0, **kw).clone()
    z = interpolate64(first, size, mode).to(torch.float32)
    inp2 = dict(inp, x=q_sample_at(z, S, start, noise), timesteps=None)
    return first, reference(kind, model, S, inp2, uc, guidance_scale, start, **kw)
