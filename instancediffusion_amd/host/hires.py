"""img2img starts and the latent hi-res second pass: the host pieces around ``sample_from`` of the three single-trajectory samplers.

Both features are one mechanism -- enter the S-step schedule at step ``start`` with a given latent:

  * img2img: encode the picture (``AutoencoderKL.encode``), noise it to the timestep of step ``start`` (``noised_start``: one
    ``idf_q_sample`` launch), run steps start .. S-1;
  * hi-res second pass: sample at the model's latent size, enlarge the LATENT (``upscale_latents``: one ``idf_resize_planes`` launch
    over tables built here), noise it part of the way back and denoise the tail of the schedule at the larger size with the same
    conditioning (``hires_pass``).  Boxes, points, scribbles and the 512^2 ``segs`` planes are resolution-free, so the first pass's
    input dict is reused as it is.

The resize tables follow ``F.interpolate(align_corners=False)``'s geometry but come from EXACT integer arithmetic: the source
coordinate of output o is ((2 o + 1) n_in - n_out) / (2 n_out); its floor is an integer division and the fraction t a remainder over
2 n_out, so no coordinate is ever rounded (torch's own fp32 path computes it in fp32 and is up to ~80 ulp off at 64 -> 96).  The weights
are evaluated in float64 and rounded to fp32 once.  The kernel, ``resize_reference`` and the tests' restatement evaluate the same fixed
expression over these tables (include/idf.h), each operation rounded on its own, so all three agree bit for bit in fp32.
"""
from __future__ import annotations

import math
from typing import Dict, Tuple

import numpy as np
import torch

from .diffusion import make_ddim_timesteps

MODES = {"bilinear": 2, "bicubic": 4}            # mode -> taps
CUBIC_A = -0.75                                   # torch's (and OpenCV's) cubic convolution coefficient


def _cubic1(x):
    """|x| <= 1."""
    return ((CUBIC_A + 2.0) * x - (CUBIC_A + 3.0)) * x * x + 1.0


def _cubic2(x):
    """1 < |x| < 2."""
    return ((CUBIC_A * x - 5.0 * CUBIC_A) * x + 8.0 * CUBIC_A) * x - 4.0 * CUBIC_A


def resize_tables(n_in: int, n_out: int, mode: str = "bicubic") -> Tuple[np.ndarray, np.ndarray]:
    """The table of one axis: (first tap int32 [n_out], weights fp32 [n_out, taps]); output o reads the source entries
    first[o] + k, k < taps, each CLAMPED to [0, n_in - 1] by whoever applies the table (torch's border rule).

    bicubic: f = floor(src), t = src - f (no clamp of src); first tap f - 1 (>= -2: src > -1/2 only when upscaling, f = -1 there);
    weights [c2(t + 1), c1(t), c1(1 - t), c2(2 - t)] of the A = -0.75 cubic.  bilinear: the numerator of src clamped to >= 0; first
    tap f; weights [1 - t, t]."""
    if mode not in MODES:
        raise ValueError(f"resize mode must be one of {sorted(MODES)}, got {mode!r}")
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f"resize: sizes must be >= 1, got {n_in} -> {n_out}")
    taps = MODES[mode]
    first = np.empty(n_out, dtype=np.int32)
    w = np.empty((n_out, taps), dtype=np.float64)
    den = 2 * n_out
    for o in range(n_out):
        num = (2 * o + 1) * n_in - n_out                                   # src = num / den, exactly
        if taps == 2:
            num = max(num, 0)
        f, rem = divmod(num, den)                                          # Python's floor division: right for num < 0 too
        t = rem / den                                                      # one correctly rounded float64 division
        if taps == 2:
            first[o] = f
            w[o] = (1.0 - t, t)
        else:
            first[o] = f - 1
            w[o] = (_cubic2(t + 1.0), _cubic1(t), _cubic1(1.0 - t), _cubic2(2.0 - t))
    return first, w.astype(np.float32)


def resize_reference(src: torch.Tensor, size, mode: str = "bicubic", dtype=torch.float32) -> torch.Tensor:
    """CPU twin of ``idf_resize_planes`` over ``resize_tables``: the kernel's fixed expression (include/idf.h), every operation a
    separate torch operation in ``dtype`` -- float32: the kernel's result bit for bit; float64: the same fp32-rounded weights with
    exact-enough sums.  src [.., Hi, Wi] -> [.., Ho, Wo]."""
    Hi, Wi = int(src.shape[-2]), int(src.shape[-1])
    Ho, Wo = int(size[0]), int(size[1])
    xi, xw = resize_tables(Wi, Wo, mode)
    yi, yw = resize_tables(Hi, Ho, mode)
    taps = xw.shape[1]
    s = src.detach().cpu().to(dtype)
    xw_t, yw_t = torch.from_numpy(xw).to(dtype), torch.from_numpy(yw).to(dtype)
    cols = [torch.from_numpy(np.clip(xi.astype(np.int64) + k, 0, Wi - 1)) for k in range(taps)]
    rows = [torch.from_numpy(np.clip(yi.astype(np.int64) + k, 0, Hi - 1)) for k in range(taps)]
    out = None
    for j in range(taps):
        sr = s.index_select(-2, rows[j])                                   # [.., Ho, Wi]
        h = sr.index_select(-1, cols[0]) * xw_t[:, 0]
        for k in range(1, taps):
            h = h + sr.index_select(-1, cols[k]) * xw_t[:, k]
        v = h * yw_t[:, j].unsqueeze(-1)
        out = v if out is None else out + v
    return out


def q_sample_reference(x0: torch.Tensor, noise: torch.Tensor, sqrt_ac: float, sqrt_1m_ac: float) -> torch.Tensor:
    """CPU twin of ``idf_q_sample``: ldm.py:19-20 with the two coefficients as fp32 scalars."""
    a = torch.full((1,) * x0.dim(), float(sqrt_ac), dtype=torch.float32)
    b = torch.full((1,) * x0.dim(), float(sqrt_1m_ac), dtype=torch.float32)
    return a * x0 + b * noise


def steps_for_strength(S: int, strength: float, timesteps=None) -> Tuple[int, int]:
    """-> (start, t): a run of strength ``strength`` re-does the last ``n_run = min(S, max(1, floor(S strength + 1e-6)))`` steps of the
    S-step schedule: it enters at step ``start = S - n_run``, whose timestep is ``t = timesteps[n_run - 1]`` -- the level the start
    latent must be noised to.  ``timesteps``: the run's ascending ``ddim_timesteps`` (default: the uniform spacing at T = 1000).
    strength 1 is a full run from (what should then be) pure noise.  ValueError outside (0, 1]."""
    S = int(S)
    if S < 1:
        raise ValueError(f"steps_for_strength: S must be >= 1, got {S}")
    if not (isinstance(strength, (int, float, np.floating)) and 0.0 < float(strength) <= 1.0):
        raise ValueError(f"strength must be in (0, 1], got {strength!r}")
    if timesteps is None:
        timesteps = make_ddim_timesteps("uniform", S, 1000)
    if len(timesteps) != S:
        raise ValueError(f"steps_for_strength: {len(timesteps)} timesteps for S = {S}")
    n_run = min(S, max(1, int(math.floor(S * float(strength) + 1e-6))))
    return S - n_run, int(timesteps[n_run - 1])


def _schedule_kw(sampler_kw: Dict) -> Dict:
    """What of ``sample_from``'s keywords ``make_schedule`` takes (the others are the step rule's)."""
    kw = {}
    if "eta" in sampler_kw:
        kw["ddim_eta"] = sampler_kw["eta"]
    if "discretize" in sampler_kw:
        kw["ddim_discretize"] = sampler_kw["discretize"]
    return kw


def noised_start(sampler, x0: torch.Tensor, S: int, strength: float, noise: torch.Tensor, **sampler_kw):
    """-> (x, start): ``x0`` noised to the timestep of step ``start`` of ``sampler``'s S-step schedule (``steps_for_strength``), by ONE
    ``idf_q_sample`` launch with the full-table ``sqrt_alphas_cumprod[t]`` / ``sqrt_one_minus_alphas_cumprod[t]`` the inpainting blend
    uses.  ``sampler_kw``: the keywords the run's ``sample_from`` will get (``eta``, ``order``, ``discretize``): they decide the timesteps."""
    sampler.make_schedule(S, **_schedule_kw(sampler_kw))
    start, t = steps_for_strength(S, strength, sampler.ddim_timesteps)
    assert t == int(np.flip(sampler.ddim_timesteps)[start])
    ops = sampler.engine.ops
    dev = sampler.engine.device
    x0 = x0.to(dev, torch.float32).contiguous()
    noise = noise.to(dev, torch.float32).contiguous()
    if noise.shape != x0.shape:
        raise ValueError(f"noised_start: noise {tuple(noise.shape)} for latents {tuple(x0.shape)}")
    sa = float(sampler.diffusion.sqrt_alphas_cumprod.detach().to(torch.float32).cpu()[t])
    s1 = float(sampler.diffusion.sqrt_one_minus_alphas_cumprod.detach().to(torch.float32).cpu()[t])
    return ops.q_sample(x0, noise, sa, s1, ops.empty(x0.shape, torch.float32)), start


_TABLES: Dict[tuple, tuple] = {}                  # (device, h, w, h2, w2, mode) -> the four device tables


def upscale_latents(ops, z: torch.Tensor, size, mode: str = "bicubic") -> torch.Tensor:
    """z [B, C, h, w] fp32 on the device -> [B, C, h2, w2]: the tables built and uploaded once per (h, w, h2, w2, mode) and device,
    then one ``idf_resize_planes`` launch."""
    h, w = int(z.shape[-2]), int(z.shape[-1])
    h2, w2 = int(size[0]), int(size[1])
    z = z.to(torch.float32).contiguous()
    key = (str(z.device), h, w, h2, w2, mode)
    if key not in _TABLES:
        xi, xw = resize_tables(w, w2, mode)
        yi, yw = resize_tables(h, h2, mode)
        _TABLES[key] = tuple(torch.from_numpy(a).to(z.device) for a in (xi, xw, yi, yw))
    out = ops.empty(tuple(z.shape[:-2]) + (h2, w2), torch.float32)
    return ops.resize_planes(z, out, *_TABLES[key])


def hires_pass(sampler, latents: torch.Tensor, input: dict, uc, guidance_scale: float, S: int, strength: float, size,
               mode: str = "bicubic", noise: torch.Tensor = None, **sampler_kw) -> torch.Tensor:
    """The second pass of a hi-res run: ``latents`` (the first pass's result) enlarged to ``size`` = (h2, w2), noised to the timestep
    of step ``start`` and denoised through steps start .. S-1 by ``sampler.sample_from`` (a ``PLMSSampler``, ``DDIMSampler`` or
    ``DPMSolverSampler``) at the new shape, with ``input``'s context and grounding input.  ``noise`` [B, 4, h2, w2]: the q_sample draw
    (default: ``torch.randn`` on the device).  ``input`` is left as it is."""
    eng = sampler.engine
    if hasattr(sampler.model, "reinstate_first_conv"):
        # the first pass may have swapped the first conv at its alpha == 0 steps; this pass re-enters in front of them
        sampler.model.reinstate_first_conv()
    z = upscale_latents(eng.ops, latents.to(eng.device), size, mode)
    if noise is None:
        noise = torch.randn(tuple(z.shape), device=eng.device, dtype=torch.float32)
    x, start = noised_start(sampler, z, S, strength, noise, **sampler_kw)
    inp = {k: v for k, v in input.items() if k not in ("x", "timesteps")}
    inp.update(x=x, timesteps=None)
    return sampler.sample_from(S, tuple(x.shape), inp, start, uc=uc, guidance_scale=guidance_scale, **sampler_kw)
