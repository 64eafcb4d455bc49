"""DDIM test support: the case tables of the ``*_ddim.pt`` goldens, a CPU fp32 restatement of the reference's ``DDIMSampler``
(ldm/models/diffusion/ddim.py) over any callable model, and the fp32 torch expressions the two step kernels
(``idf_ddim_update``, ``idf_q_sample_blend``) must reproduce bit for bit.

Only torch / numpy are imported at module level, so that tests/make_ddim_golden.py can load this file by path next to the
reference tree; everything of this repository is imported inside the functions that need it.
"""
from __future__ import annotations

import os
from typing import Callable, Optional, Sequence

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")

# golden file -> (golden whose inputs it shares, alpha_type, {case: (eta, with mask / x0)}).  tiny never reaches alpha 0 (its first
# conv has 64 channels, the swap hard-codes 320); mid runs the first-conv swap in its last two steps.
GOLDENS = {
    "tiny_box_ddim": dict(inputs_of="tiny_box", alpha_type=[1, 0, 0],
                          cases={"eta0": (0.0, False), "eta0.5": (0.5, False), "eta0.5_mask": (0.5, True)}),
    "mid_box_ddim": dict(inputs_of="mid_box", alpha_type=[0.6, 0, 0.4], cases={"eta0": (0.0, False), "eta0.5": (0.5, False)}),
}
ALL_CASES = [(tag, name) for tag, g in GOLDENS.items() for name in g["cases"]]
SCHEDULE_ONLY = [(50, 0.0), (50, 0.5), (50, 1.0)]                 # (S, eta): schedule entries without a forward
GUIDANCE = 7.5
MASK_SEED = 4321                                                 # mask, x0 and every noise draw, as gen_plms_mask_case

# (a_t, a_prev, sigma_t) of S = 5, eta 0.5 at index 4, 2 and 0 (first step, middle, last step) in float32 -- the kernel tests' triples
# (tests/test_ddim_host.py checks them against the golden schedule)
TRIPLES = [(0.03654652461409569, 0.1598164439201355, 0.410071462392807), (0.42288151383399963, 0.752143383026123, 0.21679943799972534),
           (0.9982960224151611, 0.9991499781608582, 0.010324177332222462)]


def schedule_key(S: int, eta: float) -> str:
    return f"S{S}_eta{eta:g}"


def load(tag: str) -> dict:
    return torch.load(os.path.join(GOLD, f"{tag}.pt"), weights_only=False)


# ---- the kernels' reference expressions ---------------------------------------------------------------------------
def ddim_update_expr(x, e_cond, e_uncond, guidance, a_t, a_prev, sigma_t, sqrt_1m_at, noise):
    """ddim.py:110-129 behind the model calls, as torch evaluates it in fp32: -> (x_prev, pred_x0).

    Every per-element operation is torch's, in torch's order.  The three SCALAR square roots (``a_t.sqrt()``, ``a_prev.sqrt()``,
    ``(1 - a_prev - sigma_t**2).sqrt()`` of :124-129, one-element tensors in the reference) are taken with the correctly rounded
    fp32 square root (numpy's = C's ``sqrtf``, which the launcher uses) and NOT with ``Tensor.sqrt``: torch's CPU sqrt is not
    correctly rounded (this build: 387 of 65536 random fp32 inputs are one ulp off numpy / ``sqrtf`` / the rounded float64 root,
    which numpy equals on all of them), so a kernel with IEEE arithmetic cannot equal ``Tensor.sqrt`` bit for bit on every input.
    The radicand is still built from separately rounded fp32 operations in the reference's order."""
    def full(v):
        return torch.full((1,) * x.dim(), float(v), dtype=torch.float32)          # :118-121
    f32 = np.float32
    e_t = e_cond
    if e_uncond is not None:
        e_t = e_uncond + guidance * (e_cond - e_uncond)                           # :114
    sqrt_at, sqrt_aprev = full(np.sqrt(f32(a_t))), full(np.sqrt(f32(a_prev)))
    dc = full(np.sqrt((f32(1.0) - f32(a_prev)) - f32(sigma_t) * f32(sigma_t)))
    sigma_t, s1m = full(sigma_t), full(sqrt_1m_at)
    pred_x0 = (x - s1m * e_t) / sqrt_at                                           # :124
    dir_xt = dc * e_t                                                             # :127
    x_prev = sqrt_aprev * pred_x0 + dir_xt                                        # :129
    if noise is not None:
        x_prev = x_prev + sigma_t * noise                                         # :128-129
    return x_prev, pred_x0


def q_sample_blend_expr(x0, noise, mask, img, sqrt_ac, sqrt_1m_ac):
    """ldm.py:17-20 (coefficients gathered per sample: the same value for the whole batch here) + ddim.py:97."""
    shape = (x0.shape[0],) + (1,) * (x0.dim() - 1)
    a = torch.full(shape, float(sqrt_ac), dtype=torch.float32)
    b = torch.full(shape, float(sqrt_1m_ac), dtype=torch.float32)
    img_orig = a * x0 + b * noise
    return img_orig * mask + (1. - mask) * img


# ---- the sampler, restated ----------------------------------------------------------------------------------------
def ddim_schedule(S: int, eta: float):
    """make_ddim_timesteps('uniform') + make_ddim_sampling_parameters (util.py:55-83) + ddim.py:50 on the float32 alphas_cumprod
    buffer.  util.py:78 mixes a float32 torch tensor (alphas) with a float64 numpy array (alphas_prev): its one division runs as
    reciprocal(1 - alphas) in float32 times the float64 numerator, the rest in float64.  -> timesteps, a, a_prev (float32),
    sigmas (float64), sqrt(1 - a) (float32)."""
    from oracle import ref_cpu
    steps, a, a_prev = ref_cpu._schedule(S)
    recip = (np.float32(1.0) / (np.float32(1.0) - a)).astype(np.float64)
    a64, p64 = a.astype(np.float64), a_prev.astype(np.float64)
    sigmas = eta * np.sqrt(recip * (1 - p64) * (1 - a64 / p64))
    return steps, a, a_prev, sigmas, np.sqrt(np.float32(1.0) - a)


def ddim_reference(model: Callable, S: int, input: dict, uc, guidance_scale: float, eta: float = 0.0,
                   alpha_type: Optional[Sequence[float]] = None, mask=None, x0=None, noises=None) -> torch.Tensor:
    """DDIMSampler.make_schedule(S, ddim_eta=eta) + ddim_sampling (ddim.py:25-131) on the CPU in fp32.  ``model``: a callable on
    the reference's input dict with ``set_alpha_scale`` / ``restore_first_conv_from_SD`` (oracle/ref_cpu.OracleModel).  ``noises``:
    the draws in the reference's call order -- per step the q_sample draw (with a mask), then the step's draw, which the reference
    makes at every sigma (:128); None draws from the global generator."""
    from oracle import ref_cpu
    steps, a, a_prev, sigmas, s1m = ddim_schedule(S, eta)
    it = iter(noises) if noises is not None else None

    def draw(like):
        return next(it) if it is not None else torch.randn_like(like)
    time_range = np.flip(steps)
    total = steps.shape[0]
    b = input["x"].shape[0]
    alphas = ref_cpu.alpha_generator(len(time_range), alpha_type) if alpha_type is not None else None
    img = input["x"]
    for i, step in enumerate(time_range):
        ref_cpu._step_common(model, alphas, i)                                    # :85-88
        index = total - i - 1
        input["timesteps"] = torch.full((b,), int(step), dtype=torch.long)
        if mask is not None:                                                      # :94-98
            assert x0 is not None
            img = ref_cpu.q_sample(x0, input["timesteps"], draw(x0)) * mask + (1. - mask) * img
            input["x"] = img
        e_t = model(input)                                                        # :110-114
        e_uc = None
        if uc is not None and guidance_scale != 1:
            e_uc = model(dict(x=input["x"], timesteps=input["timesteps"], context=uc))
        img, _ = ddim_update_expr(input["x"], e_t, e_uc, guidance_scale, a[index], a_prev[index], sigmas[index], s1m[index],
                                  draw(input["x"]))
        input["x"] = img
    return img


# ---- shared by the trajectory tests -------------------------------------------------------------------------------
def case_inputs(tag: str, name: str):
    """(golden file, case entry, eta, mask, x0, noises as a list) of one golden case."""
    gold = load(tag)
    case = gold["cases"][name]
    eta, masked = GOLDENS[tag]["cases"][name]
    assert float(case["eta"]) == eta
    return gold, case, eta, (gold["mask"] if masked else None), (gold["x0"] if masked else None), list(case["noises"])


def used_noises(case, masked: bool):
    """The draws ``DDIMSampler`` makes, in its order: the reference's, without the step draws of sigma == 0 steps."""
    n = list(case["noises"])
    if float(case["eta"]) == 0.0:
        return n[0::2] if masked else []
    return n
