"""PLMS sampler, the Multi-instance Sampler (MIS, on PLMS and on DDIM steps) and the DDIM sampler for the MI355X engine.

Host mirror of ``ldm/models/diffusion/plms.py`` (PLMSSampler), ``plms_instance.py`` (PLMSSamplerInst) and ``ddim.py``
(DDIMSampler): same constructor / ``sample()`` API, same schedule, same update rule and quirks, different execution plan:

  * the conditional and unconditional (classifier-free guidance) evaluations of a step run as ONE batched UNet
    forward; in MIS phase 1 all N+1 instance trajectories (x images) advance together in one batch -- the reference
    runs those 2(N+1) forwards per step serially (plms_instance.py:86-104);
  * everything step-invariant lives in ``engine.Cond`` objects built once per ``sample()`` call;
  * latents, eps history and the PLMS/CFG arithmetic stay on the GPU in fp32 (fused kernels);
  * with ``torch.distributed`` initialised (one process per GPU, RCCL), MIS phase 1 is sharded over
    (instance, image) work units, the instance latents are recombined by ONE all-gather of the unit latents each rank owns
    (scattered by index into the fixed [instance][image] stack: pure data movement) and merged by the
    same ``idf_mis_merge`` call as on one rank -- outputs are bit-identical at every world size -- and phase 2 is
    sharded over images;
  * DDIM: the raw [cond | uncond] eps halves of the step's one forward go straight into ``idf_ddim_update`` (guidance, pred_x0,
    direction and noise term in one launch), the inpainting blend in front of a step is one ``idf_q_sample_blend`` launch;
  * ``DDIMSamplerInst``: the Multi-instance Sampler on DDIM steps (the reference has none).  The two Inst classes share units, bank,
    chunking, hoist, merge and sharding and differ in one hook, ``_advance`` ("advance these n rows one step"), and in the history
    that travels from phase 1 to phase 2 (DDIM: none);
  * ``DPMSolverSampler`` / ``DPMSolverSamplerInst``: DPM-Solver++(2M) (the reference has none) on DDIM's loop and on the Multi-instance
    Sampler: one forward and one ``idf_dpmpp_update`` launch per step, coefficients from ``dpmpp_coeffs``, history = the last x0;
  * ``sample_from(S, shape, input, start, ..)`` on the three single-trajectory samplers (``PLMSSampler``, ``DDIMSampler``,
    ``DPMSolverSampler``; the reference has none): enter the schedule at step ``start`` with a given latent -- img2img starts and the
    hi-res second pass of ``host/hires.py``.  The ``*Inst`` samplers take no start.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from .diffusion import make_ddim_timesteps


def guided_uc_shared(uc: torch.Tensor) -> bool:
    """Are all rows of the unconditional context the same (stride-0 broadcast, or equal values)?  The stride test costs
    nothing; the value test is one full-tensor compare and a host sync, run ONCE per ``sample()`` call on the live tensor.
    (Round 4 memoised it under (address, shape, strides, version) -- a key that does not identify the tensor's CONTENT: a fresh
    ``uc`` of another call can reuse the address at version 0 and hit a stale True, which silently broadcast row 0's negative
    prompt to every image; ``_version`` also raises under inference_mode.  ADVICE r4.)"""
    if uc.shape[0] <= 1:
        return False
    if uc.stride(0) == 0:
        return True
    return bool((uc[1:] == uc[:1]).all())


def ddim_sigmas(a32: np.ndarray, a_prev32: np.ndarray, eta: float) -> np.ndarray:
    """util.py:78 as the reference's operand types evaluate it: ``alphas`` is a float32 torch tensor and ``alphas_prev`` a float64
    numpy array, so ``(1 - alphas_prev) / (1 - alphas)`` runs as Tensor.__rtruediv__ = reciprocal(1 - alphas) in float32, times the
    float64 numerator; every other operation is float64.  A step rounds its sigma to float32."""
    a, ap = a32.astype(np.float64), a_prev32.astype(np.float64)
    recip = (np.float32(1.0) / (np.float32(1.0) - a32)).astype(np.float64)
    return eta * np.sqrt(recip * (1 - ap) * (1 - a / ap))


def dpmpp_coeffs64(a_t, a_prev, a_last=None):
    """``dpmpp_coeffs`` in front of its one rounding: three float64 values (the inputs are taken as they come)."""
    def parts(a):
        a = np.float64(a)
        al, sg = np.sqrt(a), np.sqrt(1.0 - a)
        return al, sg, np.log(al / sg)
    _, s_t, l_t = parts(a_t)
    al_p, s_p, l_p = parts(a_prev)
    h = l_p - l_t
    bc = al_p * (1.0 - np.exp(-h))
    c_x, c_0, c_1 = s_p / s_t, bc, np.float64(0.0)
    if a_last is not None:
        r = (l_t - parts(a_last)[2]) / h
        c_0, c_1 = bc * (1.0 + 1.0 / (2.0 * r)), -bc / (2.0 * r)
    return c_x, c_0, c_1


def dpmpp_coeffs(a_t, a_prev, a_last=None):
    """The coefficients of one DPM-Solver++(2M) step in data-prediction form (Lu et al. 2022, "DPM-Solver++", Algorithm 2):
    ``x_prev = c_x x + c_0 x0_t + c_1 x0_last`` with ``x0_t = (x - sigma_t e) / alpha_t`` -> (c_x, c_0, c_1) as float32.

    alpha = sqrt(a), sigma = sqrt(1 - a), lambda = log(alpha / sigma), h = lambda_prev - lambda_t, Bc = alpha_prev (1 - exp(-h)).
    ``a_last`` None (the first step of a run): order 1, (sigma_prev / sigma_t, Bc, 0) -- DDIM with eta 0.  ``a_last`` = a of the
    previous step: order 2 with r = (lambda_t - lambda_last) / h, (sigma_prev / sigma_t, Bc (1 + 1 / (2 r)), -Bc / (2 r)).
    The inputs are the float32 schedule values the samplers hold; everything is float64, the results are rounded once."""
    f = [np.float32(a) for a in (a_t, a_prev)] + [None if a_last is None else np.float32(a_last)]
    return tuple(np.float32(c) for c in dpmpp_coeffs64(*f))


def logsnr_timesteps(S: int, alphas_cumprod) -> np.ndarray:
    """S ascending timesteps in [1, T-1], as evenly spaced in lambda = log(alpha / sigma) as distinct integers allow: the integer
    whose lambda is nearest each of linspace(lambda(1), lambda(T-1), S) (the lower t on a tie), then made strictly increasing
    from below, capped at T-1, and made strictly increasing from above.  S = 1: [T-1].  lambda in float64 from ``alphas_cumprod``."""
    ac = np.asarray(alphas_cumprod).astype(np.float64)
    T = int(ac.shape[0])
    if S < 1 or S > T - 1:
        raise ValueError(f"logsnr spacing: S must be in [1, {T - 1}], got {S}")
    if S == 1:
        return np.asarray([T - 1])
    lam = np.log(np.sqrt(ac) / np.sqrt(1.0 - ac))
    t = [1 + int(np.argmin(np.abs(lam[1:] - target))) for target in np.linspace(lam[1], lam[T - 1], S)]   # argmin: the first = lower t
    for k in range(1, S):
        t[k] = max(t[k], t[k - 1] + 1)
    t[S - 1] = min(t[S - 1], T - 1)
    for k in range(S - 2, -1, -1):
        t[k] = min(t[k], t[k + 1] - 1)
    return np.asarray(t)


class _PLMSBase(object):
    def __init__(self, diffusion, model, schedule="linear", alpha_generator_func=None, set_alpha_scale=None):
        super().__init__()
        self.diffusion = diffusion
        self.model = model
        self.device = diffusion.betas.device
        self.ddpm_num_timesteps = diffusion.num_timesteps
        self.schedule = schedule
        self.alpha_generator_func = alpha_generator_func
        self.set_alpha_scale = set_alpha_scale

    # ---- schedule (plms.py:25-62; util.py:55-83) ------------------------------------------------------
    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0., verbose=False):
        if ddim_eta != 0:
            raise ValueError('ddim_eta must be 0 for PLMS')
        ac = self.diffusion.alphas_cumprod.detach().to(torch.float32).cpu()
        self.ddim_timesteps = self._timesteps(ddim_discretize, ddim_num_steps, ac.numpy(), verbose)
        assert ac.shape[0] == self.ddpm_num_timesteps, 'alphas have to be defined for each timestep'
        # float32 values, exactly as the reference's float32 buffers (make_ddim_sampling_parameters, eta = 0)
        self.ddim_alphas = ac[self.ddim_timesteps].numpy()
        self.ddim_alphas_prev = np.asarray([ac[0].item()] + ac[self.ddim_timesteps[:-1]].tolist(), dtype=np.float32)
        self.ddim_sigmas = np.zeros_like(self.ddim_alphas)
        self.ddim_sqrt_one_minus_alphas = torch.sqrt(1.0 - ac[self.ddim_timesteps]).numpy()

    def _timesteps(self, discretize, S, ac, verbose=False):
        """The S timesteps of a run, ascending (``ac``: the float32 alphas_cumprod); the DPM-Solver++ samplers add a spacing."""
        return make_ddim_timesteps(discretize, S, self.ddpm_num_timesteps, verbose)

    # ---- engine plumbing --------------------------------------------------------------------------------
    @property
    def engine(self):
        return self.model.engine

    def _cond(self, inp: Dict) -> "object":
        g = inp["grounding_input"] if "grounding_input" in inp else self.model.grounding_tokenizer_input.get_null_input()
        return self.engine.prepare_cond(inp["context"], g)

    def _uncond(self, uc: torch.Tensor):
        return self.engine.prepare_cond(uc, self.model.grounding_tokenizer_input.get_null_input(batch=uc.shape[0]))

    def _check_first_conv(self, alphas):
        """The alpha schedule reaches 0 (default alpha_type [0.8, 0, 0.2]: at step 40 of 50) -> the model will swap its first
        conv for Stable Diffusion's (openaimodel.py:469-480) and needs that 48-KB file: find out NOW, not 40 steps in."""
        if alphas is not None and any(a == 0 for a in alphas) and hasattr(self.model, "check_first_conv_available"):
            self.model.check_first_conv_available()

    def _apply_alpha(self, alphas, i):
        """plms.py:90-94: per-step gate + first-conv swap."""
        if alphas is not None:
            self.set_alpha_scale(self.model, alphas[i])
            if alphas[i] == 0:
                self.model.restore_first_conv_from_SD()
            self.engine.sync_fuser_scale_from_modules()

    def _eps(self, x, step: int, cond_pair, n: int, guided: bool, guidance_scale: float):
        """Guided eps for n trajectories: one batched forward of [cond | uncond] (plms.py:121-127)."""
        eng = self.engine
        if guided:
            # the n distinct rows only: the engine writes both halves of its static [cond | uncond] input itself (the
            # paired invariant is structural, not a promise checked once per launch configuration)
            t = torch.full((n,), float(step), device=x.device, dtype=torch.float32)
            e2 = eng.forward_cond(x, t, cond_pair, out=eng.buf("smp.eps2", (2 * n,) + tuple(x.shape[1:]), torch.float32), paired=True)
            return eng.ops.cfg_combine(e2[:n], e2[n:], guidance_scale, eng.ops.empty(x.shape, torch.float32))
        t = torch.full((n,), float(step), device=x.device, dtype=torch.float32)
        return eng.forward_cond(x, t, cond_pair)

    def _plms_step(self, x, old_eps: list, index: int, step: int, step_next: int, cond_pair, n, guided, gs,
                   e_t_first=None):
        """p_sample_plms (plms.py:117-167).  Returns (x_prev, e_t).  ``e_t_first``: guided eps of the first
        evaluation when the caller already computed it (MIS start-of-trajectory de-duplication)."""
        ops = self.engine.ops
        a_t, a_prev = float(self.ddim_alphas[index]), float(self.ddim_alphas_prev[index])
        s1m = float(self.ddim_sqrt_one_minus_alphas[index])
        e_t = e_t_first if e_t_first is not None else self._eps(x, step, cond_pair, n, guided, gs)
        new = ops.empty(x.shape, torch.float32)
        if len(old_eps) == 0:
            x_pred = ops.plms_update(x, e_t, [], None, 0, a_t, a_prev, s1m, ops.empty(x.shape, torch.float32))
            e_next = self._eps(x_pred, step_next, cond_pair, n, guided, gs)
            ops.plms_update(x, e_t, [], e_next, 1, a_t, a_prev, s1m, new)
        else:
            ops.plms_update(x, e_t, old_eps, None, min(len(old_eps), 3) + 1, a_t, a_prev, s1m, new)
        return new, e_t

    def _check_start(self, start):
        """``start``: the step at which a single-trajectory run enters the S-step schedule made by ``make_schedule`` (``input["x"]`` is
        the latent ENTERING that step; 0 = a full run).  ValueError outside [0, S-1], before any forward."""
        total = int(self.ddim_timesteps.shape[0])
        if isinstance(start, bool) or not isinstance(start, (int, np.integer)) or not 0 <= start < total:
            raise ValueError(f"start must be an integer in [0, {total - 1}] (the run has {total} steps), got {start!r}")
        return int(start)

    @staticmethod
    def _push(old_eps: list, e_t):
        old_eps.append(e_t)
        if len(old_eps) >= 4:
            old_eps.pop(0)


class PLMSSampler(_PLMSBase):
    """plms.py:9-167."""

    @torch.no_grad()
    def sample(self, S, shape, input, uc=None, guidance_scale=1, mask=None, x0=None, start=0):
        """``start``: see ``sample_from``."""
        self.make_schedule(ddim_num_steps=S)
        return self.plms_sampling(shape, input, uc, guidance_scale, mask=mask, x0=x0, start=start)

    @torch.no_grad()
    def sample_from(self, S, shape, input, start, uc=None, guidance_scale=1, mask=None, x0=None):
        """Enter the S-step schedule at step ``start`` (an extension, ``host/hires.py``: img2img starts and the hi-res second pass; the
        one spelling the three single-trajectory samplers share): ``input["x"]`` is the latent ENTERING step ``start``; steps
        start .. S-1 run with their ABSOLUTE index, timestep and ``alphas[i]``, so the grounding gate and the first-conv swap fall where
        they would in a full run.  The history begins empty at ``start`` (here: a predictor step, two forwards); the inpainting blend,
        with a mask, applies from ``start`` on.  ``start`` 0 is ``sample``, bit for bit; outside [0, S-1]: ValueError before any forward."""
        return self.sample(S, shape, input, uc, guidance_scale, mask=mask, x0=x0, start=start)

    @torch.no_grad()
    def plms_sampling(self, shape, input, uc=None, guidance_scale=1, mask=None, x0=None, start=0):
        start = self._check_start(start)
        eng = self.engine
        dev = eng.device
        b = shape[0]
        img = input["x"]
        if img is None:
            img = torch.randn(shape, device=dev)
            input["x"] = img
        img = img.to(dev, torch.float32)
        guided = uc is not None and guidance_scale != 1
        cond = self._cond(input)
        if guided:
            bank = type(cond).cat([cond, self._uncond(uc)])
            pair = eng.gather_cond(bank, torch.arange(2 * b, device=dev))
        else:
            pair = cond
        time_range = np.flip(self.ddim_timesteps)
        total = self.ddim_timesteps.shape[0]
        alphas = self.alpha_generator_func(len(time_range)) if self.alpha_generator_func is not None else None
        self._check_first_conv(alphas)
        old_eps: list = []
        for i in range(start, total):
            step = time_range[i]
            self._apply_alpha(alphas, i)
            index = total - i - 1
            step_next = int(time_range[min(i + 1, len(time_range) - 1)])
            if mask is not None:
                assert x0 is not None
                ts = torch.full((b,), int(step), device=dev, dtype=torch.long)
                img_orig = self.diffusion.q_sample(x0.to(dev), ts)
                img = img_orig * mask + (1. - mask) * img
            img, e_t = self._plms_step(img, old_eps, index, int(step), step_next, pair, b, guided, guidance_scale)
            input["x"] = img
            input["timesteps"] = torch.full((b,), int(step), device=dev, dtype=torch.long)
            self._push(old_eps, e_t)
        return img


class PLMSSamplerInst(_PLMSBase):
    """Multi-instance Sampler, plms_instance.py:7-212."""

    def __init__(self, diffusion, model, schedule="linear", alpha_generator_func=None, set_alpha_scale=None, mis=0.0,
                 crop_and_paste_latents=False, shard_across_ranks: Optional[bool] = None, max_units: int = 128,
                 unit_sharding: str = "auto"):
        super().__init__(diffusion, model, schedule, alpha_generator_func, set_alpha_scale)
        self.mis = mis
        self.crop_and_paste_latents = crop_and_paste_latents      # hard-coded False in the reference (:128)
        self.shard_across_ranks = shard_across_ranks
        assert unit_sharding in ("auto", "image", "instance")
        self.unit_sharding = unit_sharding
        # phase-1 (instance, image) units per batched forward: 128 units x [cond | uncond] = 256-row forwards (1.230 ms per row
        # against 1.250 at 128 rows and 1.27 at 64, graph-replayed: profiles/r06_replay_256.log; bench + 1.2 %, r06_maxunits_ab.log)
        self.max_units = max_units

    @torch.no_grad()
    def sample(self, S, shape, input, uc=None, guidance_scale=1, mask=None, x0=None):
        self.make_schedule(ddim_num_steps=S)
        return self.plms_sampling(shape, input, uc, guidance_scale, mask=mask, x0=x0)

    @staticmethod
    def units_per_forward(max_units: int, h: int, w: int) -> int:
        """(instance, image) units per phase-1 forward: ``max_units`` at latents up to 64 x 64; beyond (C4: 96 x 96) the same TOKEN
        budget per forward (2 max_units x 4096 rows of the 64^2 level: 2^20 at the default, the width every kernel's index ranges
        are tested at), but never fewer than the 64 units the default of rounds 3-6 formed at every size."""
        return min(max_units, max(64, max_units * 4096 // (h * w)))

    @staticmethod
    def chunk_sizes(n_units: int, per_fwd: int):
        """Phase-1 forwards of a rank's n_units: full ones of per_fwd units, then the remainder -- cut at a multiple of 64 units when
        it is larger than that: 128-row multiples fill the persistent kernels' tile grids (2 / 4 full rounds of the 32^2 level's
        256-row tiles on 256 CUs), widths in between do not (72 units as ONE 144-row forward ran the 8-image bench leg 3 % slower
        than 64 + 8: profiles/r06_bench_final.json against r06_bench_final_maxunits64_*.json)."""
        out, left = [], n_units
        while left > 0:
            n = per_fwd if left >= per_fwd else (left if left <= 64 or left % 64 == 0 else left // 64 * 64)
            out.append(n)
            left -= n
        return out

    # ---- distributed helpers ----------------------------------------------------------------------------
    def _dist(self):
        import torch.distributed as dist
        on = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        if self.shard_across_ranks is False:
            on = False
        return (dist, dist.get_rank(), dist.get_world_size()) if on else (None, 0, 1)

    # ---- the step rule: all a Multi-instance Sampler on another step (``DDIMSamplerInst``) overrides -----------------------------
    def _begin_run(self, shape, dist=None):
        """Called once per sampling call, after the checks and before any forward; ``shape``: the stacked latents of ALL images."""

    def _hoist_input(self, x_start):
        """What the hoisted first evaluation sees of the start latents: step 0's input, the same for every unit of an image."""
        return x_start

    def _advance(self, x, hist, i, time_range, total, pair, n, guided, guidance_scale, first=None, rows_img=None):
        """Advance the n rows of x one step (step i of the schedule): -> the new x; ``hist`` is updated in place.  ``first``: the raw
        (cond, uncond) eps halves of this evaluation when the caller already has them (the hoist); ``rows_img[k]``: the image row k
        belongs to.  Here: p_sample_plms, ``hist`` = the eps history."""
        e_first = None
        if first is not None:
            ops = self.engine.ops
            e_first = ops.cfg_combine(first[0], first[1], guidance_scale, ops.empty(x.shape, torch.float32))
        step_next = int(time_range[min(i + 1, len(time_range) - 1)])
        x, e_t = self._plms_step(x, hist, total - i - 1, int(time_range[i]), step_next, pair, n, guided, guidance_scale, e_t_first=e_first)
        self._push(hist, e_t)
        return x

    def _new_history(self):
        """The history a run of rows starts with; what travels from phase 1 to phase 2 is row k's part of it, ``_history_row``,
        re-stacked over the rows of phase 2 by ``_history_stack``."""
        return []

    @staticmethod
    def _history_row(hist, k):
        return [e[k] for e in hist]

    @staticmethod
    def _history_stack(rows):
        return [torch.stack([h[i] for h in rows]) for i in range(len(rows[0]))]

    # ---- the two phases over a list of work units (shared by ``plms_sampling`` and ``sample_layouts``) ----------------
    # A unit is any hashable key; the caller says where its conditioning lives (``row_of[u]``: bank row), which image it
    # belongs to (``img_of(u)``: index into the stacked start latents, key of ``row_unc``) and where its start latent is (``x_of(u)``).
    def _rows(self, units, row_of, row_unc, img_of, guided):
        """Bank rows of a [cond | uncond] forward over ``units``."""
        r = [row_of[u] for u in units]
        if guided:
            r += [row_unc[img_of(u)] for u in units]
        return torch.tensor(r, device=self.engine.device, dtype=torch.long)

    def _phase1(self, bank, chunks, units, row_of, row_unc, img_of, x_of, x_start, alphas, time_range, total, mis_step, guided,
                guidance_scale, per_fwd):
        """Advance every unit of ``chunks`` through the first ``mis_step`` steps, one batched forward per chunk and evaluation.
        ``x_start`` (the start latents of all images, [n_img, 4, H, W] on the device) asks for the hoisted first evaluation, None
        for none.  Returns ({unit: latent}, {unit: its history, ``_history_row``})."""
        eng = self.engine
        dev = eng.device
        x_units: Dict[tuple, torch.Tensor] = {}
        eps_units: Dict[tuple, list] = {}
        # Exact hoist of the very first evaluation: every instance trajectory of image b still holds the SAME latent (the
        # shared starting noise, inference.py:300-301) and the unconditional branch sees only (x, t, uc, null grounding),
        # so it is identical for the N+1 instances of an image.  Evaluate all conditional rows of this rank's units plus
        # ONE unconditional row per image up front, in full-width forwards, instead of one unconditional row per unit.
        first_idx: Dict[tuple, int] = {}
        first_unc: Dict[int, int] = {}
        E_first = None
        if x_start is not None:
            self._apply_alpha(alphas, 0)
            x_start = self._hoist_input(x_start)
            imgs = sorted({img_of(u) for u in units})
            row_ids = [row_of[u] for u in units] + [row_unc[b] for b in imgs]
            row_img = [img_of(u) for u in units] + imgs
            first_idx = {u: k for k, u in enumerate(units)}
            first_unc = {b: len(units) + k for k, b in enumerate(imgs)}
            width = 2 * per_fwd
            parts = []
            for k in range(0, len(row_ids), width):
                r = torch.tensor(row_ids[k:k + width], device=dev, dtype=torch.long)
                xx = x_start[torch.tensor(row_img[k:k + width], device=dev, dtype=torch.long)]
                tt = torch.full((xx.shape[0],), float(time_range[0]), device=dev, dtype=torch.float32)
                slot = eng.gather_cond(bank, r)
                parts.append(eng.forward_cond(xx, tt, slot, out=eng.buf("smp.eps_first", xx.shape, torch.float32)).clone())
            E_first = torch.cat(parts, 0)
        for chunk in chunks:
            if not chunk:
                continue
            n = len(chunk)
            pair = None
            x = torch.stack([x_of(u) for u in chunk]).to(dev, torch.float32)
            old = self._new_history()
            rows_img = [img_of(u) for u in chunk]
            for i in range(mis_step):
                self._apply_alpha(alphas, i)
                first = None
                if i == 0 and E_first is not None:
                    ic = torch.tensor([first_idx[u] for u in chunk], device=dev, dtype=torch.long)
                    iu = torch.tensor([first_unc[img_of(u)] for u in chunk], device=dev, dtype=torch.long)
                    first = (E_first[ic].contiguous(), E_first[iu].contiguous())
                if i == 0 or pair is None:
                    pair = eng.gather_cond(bank, self._rows(chunk, row_of, row_unc, img_of, guided))
                x = self._advance(x, old, i, time_range, total, pair, n, guided, guidance_scale, first=first, rows_img=rows_img)
            for k, u in enumerate(chunk):
                x_units[u] = x[k]
                eps_units[u] = self._history_row(old, k)
        return x_units, eps_units

    def _phase2(self, x, old, pair, n, alphas, time_range, total, mis_step, guided, guidance_scale, rows_img):
        """The shared trajectory from step ``mis_step`` on (plms_instance.py:138-156): n rows, ``old`` = their history."""
        for i in range(mis_step, len(time_range)):
            self._apply_alpha(alphas, i)
            x = self._advance(x, old, i, time_range, total, pair, n, guided, guidance_scale, rows_img=rows_img)
        return x

    @torch.no_grad()
    def plms_sampling(self, shape, input_all, uc=None, guidance_scale=1, mask=None, x0=None):
        """``mask`` / ``x0`` are accepted and ignored, as in the reference (plms_instance.py never reads them)."""
        return self._mis_sampling(shape, input_all, uc, guidance_scale)

    def _mis_sampling(self, shape, input_all, uc, guidance_scale):
        eng = self.engine
        ops = eng.ops
        dev = eng.device
        dist, rank, world = self._dist()
        B = shape[0]
        latent_size = shape[2]
        img = input_all[0]["x"]
        if img is None:
            img = torch.randn(shape, device=dev)
            if dist is not None:
                dist.broadcast(img, 0)
            for inp in input_all:
                inp["x"] = img
        n_all = len(input_all)
        guided = uc is not None and guidance_scale != 1
        time_range = np.flip(self.ddim_timesteps)
        total = self.ddim_timesteps.shape[0]
        alphas = self.alpha_generator_func(len(time_range)) if self.alpha_generator_func is not None else None
        self._check_first_conv(alphas)
        mis_step = int(total * self.mis)
        self._begin_run(tuple(shape), dist)

        # ---------------- work split (decided BEFORE any conditioning is built) ---------------------------------
        # Phase 1 = N+1 independent trajectories per image (plms_instance.py:86-104); work unit = (instance j, image b).  "image" sharding: owner = b % world -- every trajectory of an image lives on
        # the rank that also runs its phase 2, the first-evaluation hoist touches only this rank's images and per-rank work
        # is independent of the world size (weak scaling); used when the images divide evenly over the ranks.
        # "instance" sharding: owner = (b + j) % world -- spreads the N+1 trajectories of FEW images (B < world, e.g. one
        # image on 8 GPUs) over the ranks; the owner of image b (rank b % world) still runs (0, b), whose eps history
        # continues into phase 2.  Either way the merge is at most one small all-gather.
        mode = self.unit_sharding
        if mode == "auto":
            mode = "image" if (B % world == 0) else "instance"
        if mode == "image":
            units = [(j, b) for j in range(n_all) for b in range(B) if b % world == rank]
        else:
            units = [(j, b) for j in range(n_all) for b in range(B) if (b + j) % world == rank]
        mine = [b for b in range(B) if b % world == rank]                     # images this rank owns in phase 2

        # Conditioning (UniFusion tokens + per-layer K/V caches) only for the (input, image) pairs THIS rank touches: input j
        # is prepared on the images of this rank's units (j, b) -- with either ownership rule that is B / world images per
        # input, so per-rank setup work and HBM stay constant as ranks are added (weak scaling); the unconditional branch
        # is prepared on the union.  One bank of all conditionings; batches are assembled by a single row gather straight
        # into the engine's static slot.
        need_j = [sorted({b for (jj, b) in units if jj == j} | (set(mine) if j == 0 else set())) for j in range(n_all)]
        need_u = sorted({b for (_, b) in units} | set(mine))
        # identical unconditional rows (one negative prompt broadcast over the batch, inference.py:303): build that
        # conditioning ONCE and let every image gather the same bank row -- with `instance` ownership need_u is all B
        # images of the global batch, and per-rank setup work must not grow with the world size
        uc_shared = bool(guided_uc_shared(uc)) if (uc is not None and len(need_u) > 1) else False
        row_of: Dict[tuple, int] = {}
        off = 0
        for j in range(n_all):
            for k, b in enumerate(need_j[j]):
                row_of[(j, b)] = off + k
            off += len(need_j[j])
        row_unc = {b: off + (0 if uc_shared else k) for k, b in enumerate(need_u)}

        def take(v, imgs):
            if not torch.is_tensor(v) or v.dim() == 0 or v.shape[0] != B or len(imgs) == B:
                return v
            if v.stride(0) == 0:                                               # batch-broadcast view stays a view
                return v[:1].expand(len(imgs), *v.shape[1:])
            return v.index_select(0, torch.tensor(imgs, device=v.device, dtype=torch.long))

        def local(inp, imgs):
            d = dict(inp)
            d["context"] = take(inp["context"], imgs)
            if "grounding_input" in inp:
                gin = inp["grounding_input"]
                d["grounding_input"] = {k: take(v, imgs) for k, v in gin.items()}
                if torch.is_tensor(gin.get("att_masks")) and len(imgs) != B:
                    # attention.py:200 decides mask / no mask on the WHOLE per-call tensor: take that decision here, on
                    # the un-sharded batch, so that a rank's row subset cannot flip it (results independent of world)
                    d["grounding_input"]["att_masks_any"] = bool((gin["att_masks"] > 0).any())
            else:
                d["grounding_input"] = self.model.grounding_tokenizer_input.get_null_input(batch=len(imgs))
            return d

        conds = [self._cond(local(input_all[j], need_j[j])) for j in range(n_all) if need_j[j]]
        cond_u = self._uncond(take(uc, need_u[:1] if uc_shared else need_u)) if (guided and need_u) else None
        parts = conds + ([cond_u] if cond_u is not None else [])
        bank = type(parts[0]).cat(parts) if parts else None

        def img_of(u):
            return u[1]

        def rows(units):
            return self._rows(units, row_of, row_unc, img_of, guided)

        # Reference quirk: restore_first_conv_from_SD is never undone, so if alpha hits 0 inside phase 1 the LATER
        # instances would run their EARLY steps with the swapped conv.  Only then is the serial order observable;
        # reproduce it by advancing one instance at a time.
        serial = alphas is not None and any(alphas[i] == 0 for i in range(mis_step))
        per_fwd = self.units_per_forward(self.max_units, int(shape[2]), int(shape[3]))
        if serial:
            chunks = [[u for u in units if u[0] == j] for j in range(n_all)]
        else:
            chunks, k = [], 0
            for n in self.chunk_sizes(len(units), per_fwd):
                chunks.append(units[k:k + n])
                k += n
        same_start = all(inp["x"] is input_all[0]["x"] or torch.equal(inp["x"], input_all[0]["x"]) for inp in input_all[1:])
        hoist = bool(guided and same_start and units and mis_step > 0 and not serial)
        x_units, eps_units = self._phase1(bank, chunks, units, row_of, row_unc, img_of, lambda u: input_all[u[0]]["x"][u[1]],
                                          input_all[0]["x"].to(dev, torch.float32) if hoist else None, alphas, time_range, total,
                                          mis_step, guided, guidance_scale, per_fwd)

        # ---------------- merge (plms_instance.py:128-135) ------------------------------------------------------
        # The SAME arithmetic at every world size: the N+1 unit latents of every image are laid out in the fixed order
        # [instance][image] and idf_mis_merge reduces them (mean, or crop-and-paste) -- a rank fills in the units it ran and
        # ONE all-gather (RCCL) brings in the others' (below): the merged latent is bit-identical to the 1-rank result.
        # With `image` ownership a rank holds every unit of the images it continues in phase 2: nothing to exchange.
        lat = torch.zeros((n_all, B) + tuple(shape[1:]), device=dev, dtype=torch.float32)
        for (j, b), xv in x_units.items():
            lat[j, b] = xv
        if dist is not None and mode != "image":
            # the ONE hot-path collective: an all-gather of the unit latents each rank OWNS (round 4; rounds 2-3 all-reduced the
            # whole zero-padded stack, (N+1) B latents per rank).  Every rank can enumerate every rank's unit list, so the
            # gathered blocks are scattered into the fixed [instance][image] layout by index -- pure data movement, the stack
            # (and with it the merged latent) is bit-identical to the single-rank one.  Payload per rank: ceil((N+1) B / W)
            # latents of 64 KiB.
            owned = [[(j, b) for j in range(n_all) for b in range(B) if (b + j) % world == r] for r in range(world)]
            cap = max(len(o) for o in owned)
            send = torch.zeros((cap,) + tuple(shape[1:]), device=dev, dtype=torch.float32)
            for k, u in enumerate(owned[rank]):
                send[k] = x_units[u]
            recv = [torch.empty_like(send) for _ in range(world)]
            dist.all_gather(recv, send)
            flat = lat.view((n_all * B,) + tuple(shape[1:]))
            for r in range(world):
                if r != rank and owned[r]:
                    idx_r = torch.tensor([j * B + b for (j, b) in owned[r]], device=dev, dtype=torch.long)
                    flat[idx_r] = recv[r][:len(owned[r])]
        if self.crop_and_paste_latents:
            boxes = torch.tensor([[int(v * latent_size) for v in inp["grounding_input"]["boxes"][0][0].tolist()]
                                  for inp in input_all[1:]], dtype=torch.int32, device=dev).reshape(-1, 4)
            merged = ops.mis_merge(lat, boxes, ops.empty(tuple(shape), torch.float32), 1)
        else:
            merged = ops.mis_merge(lat, None, ops.empty(tuple(shape), torch.float32), 0)

        # ---------------- phase 2: shared trajectory, one per image, sharded over images (:138-156) -------------
        out = torch.zeros(tuple(shape), device=dev, dtype=torch.float32)
        if mine:
            idx = torch.tensor(mine, device=dev)
            n = len(mine)
            x = merged[idx].contiguous()
            old = self._history_stack([eps_units[(0, b)] for b in mine]) if mis_step > 0 else self._new_history()
            pair = eng.gather_cond(bank, rows([(0, b) for b in mine]))
            out[idx] = self._phase2(x, old, pair, n, alphas, time_range, total, mis_step, guided, guidance_scale, mine)
        if dist is not None:
            # finished images of every rank, again as an all-gather of what each rank owns (images b = r, r + W, ...)
            cap = (B + world - 1) // world
            send = torch.zeros((cap,) + tuple(shape[1:]), device=dev, dtype=torch.float32)
            if mine:
                send[:len(mine)] = out[torch.tensor(mine, device=dev)]
            recv = [torch.empty_like(send) for _ in range(world)]
            dist.all_gather(recv, send)
            for r in range(world):
                theirs = [b for b in range(B) if b % world == r]
                if r != rank and theirs:
                    out[torch.tensor(theirs, device=dev)] = recv[r][:len(theirs)]
        input_all[0]["x"] = out
        return out

    # ---- a batch of DIFFERENT layouts in one call -------------------------------------------------------------------
    SEG_ROWS_PER_PREPARE = 8            # rows with a real mask stack (31 MB each at 30 x 512^2) per prepare_cond call

    def _stack_conds(self, inputs):
        """One conditioning row per batch-1 input dict, in the order given, built with FEW ``prepare_cond`` calls over stacked
        rows: every row whose ``segs`` are all zero goes into one call, with one zero plane set broadcast over the rows (a
        stride-0 view, as ``host/input.py`` and ``get_null_input`` hand it out); rows with a real mask stack follow
        SEG_ROWS_PER_PREPARE at a time.  Returns (Cond, bank row of every input)."""
        eng = self.engine
        dev = eng.device
        gi = self.model.grounding_tokenizer_input
        rows, zero_of = [], {}
        for inp in inputs:
            g = inp["grounding_input"] if "grounding_input" in inp else gi.get_null_input(batch=1)
            if inp["context"].shape[0] != 1 or g["boxes"].shape[0] != 1:
                raise ValueError("sample_layouts: every input dict holds its conditioning at batch 1")
            segs = g["segs"]
            if id(segs) not in zero_of:
                zero_of[id(segs)] = not bool(segs[:1].any())
            rows.append((inp["context"], g, zero_of[id(segs)]))

        def points(g):
            p = g.get("points")
            return ((g["boxes"][..., :2] + g["boxes"][..., 2:]) / 2.0) if p is None else p

        def prepare(sel, segs):
            ctx = torch.cat([rows[r][0].to(dev) for r in sel], 0)
            g = {k: torch.cat([rows[r][1][k].to(dev) for r in sel], 0)
                 for k in ("boxes", "masks", "positive_embeddings", "scribbles", "polygons")}
            g["points"] = torch.cat([points(rows[r][1]).to(dev) for r in sel], 0)
            g["segs"] = segs
            return eng.prepare_cond(ctx, g)

        seg_shape = rows[0][1]["segs"].shape[1:]
        zero = [r for r, (_, g, z) in enumerate(rows) if z and g["segs"].shape[1:] == seg_shape]
        real = [r for r in range(len(rows)) if r not in set(zero)]
        parts, order = [], []
        if zero:
            plane = rows[zero[0]][1]["segs"][:1].to(dev)
            parts.append(prepare(zero, plane.expand(len(zero), *seg_shape)))
            order += zero
        for k in range(0, len(real), self.SEG_ROWS_PER_PREPARE):
            sel = real[k:k + self.SEG_ROWS_PER_PREPARE]
            parts.append(prepare(sel, torch.cat([rows[r][1]["segs"][:1].to(dev) for r in sel], 0)))
            order += sel
        bank = type(parts[0]).cat(parts) if len(parts) > 1 else parts[0]
        where = {r: k for k, r in enumerate(order)}
        return bank, [where[r] for r in range(len(rows))]

    @torch.no_grad()
    def sample_layouts(self, S, layouts, uc=None, guidance_scale=1):
        """One call for L DIFFERENT layouts with different instance counts, their work units packed into the same wide forwards
        ``sample()`` forms from copies of one layout.

        ``layouts[l]`` is the ``input_all`` list of layout l, ``[global, instance 1, .., instance N_l]`` with N_l >= 0: every dict
        holds its conditioning (``context``, ``grounding_input``) at batch 1 and ``x`` [K_l, 4, H, W], the start latents of that
        layout's K_l images, shared by the layout's dicts.  ``uc``: one row for all, or one row per layout.  Returns
        [sum K_l, 4, H, W], layout after layout; image k of layout l is what ``sample(S, (1, 4, H, W), layouts[l] with x[k:k+1],
        uc_l, guidance_scale)`` returns as the first call on a freshly loaded model (the first-conv swap happens at the same
        step for every row, so this holds for all layouts at once).  The input dicts are left as they are.

        Execution: the two phases of ``plms_sampling`` over the ragged unit list (layout, instance, image), chunked by
        ``units_per_forward`` / ``chunk_sizes``; the hoisted first evaluation keeps one unconditional row per image; conditioning is
        prepared once per LAYOUT and shared by its images through bank row indices; the merge is ONE ``idf_mis_merge_ragged`` call.
        Runs on this process's GPU only: layout batches are NOT sharded over ranks, whatever ``shard_across_ranks`` says.

        ValueError: a model built for masked gated self-attention (the mask / no-mask decision is per reference call), an alpha
        schedule that reaches 0 inside phase 1 (the reference's serial-order quirk cannot be reproduced for independent layouts),
        ``crop_and_paste_latents`` with a layout without instances."""
        self.make_schedule(ddim_num_steps=S)
        return self._mis_layouts(layouts, uc, guidance_scale)

    def _mis_layouts(self, layouts, uc, guidance_scale):
        eng = self.engine
        ops = eng.ops
        dev = eng.device
        if len(layouts) == 0 or any(len(lay) == 0 for lay in layouts):
            raise ValueError("sample_layouts: needs at least one layout, and every layout at least its global input")
        if eng.masked_fuser:
            raise ValueError("sample_layouts: a model built for masked gated self-attention takes its mask / no-mask decision per "
                             "reference call; use sample() per layout")
        time_range = np.flip(self.ddim_timesteps)
        total = self.ddim_timesteps.shape[0]
        alphas = self.alpha_generator_func(len(time_range)) if self.alpha_generator_func is not None else None
        mis_step = int(total * self.mis)
        if alphas is not None and any(alphas[i] == 0 for i in range(mis_step)):
            raise ValueError("sample_layouts: the alpha schedule reaches 0 inside phase 1; the reference then runs the instances "
                             "in serial order with a swapped first conv, which independent layouts cannot reproduce")
        n_inst = [len(lay) - 1 for lay in layouts]
        if self.crop_and_paste_latents and min(n_inst) == 0:
            raise ValueError("sample_layouts: crop_and_paste_latents needs at least one instance in every layout")
        L = len(layouts)
        xs = [lay[0]["x"] for lay in layouts]
        if any(not torch.is_tensor(x) or x.dim() != 4 or x.shape[0] < 1 or x.shape[1:] != xs[0].shape[1:] for x in xs):
            raise ValueError("sample_layouts: every layout carries its start latents x [K_l, 4, H, W], all of one size")
        guided = uc is not None and guidance_scale != 1
        if guided and uc.shape[0] not in (1, L):
            raise ValueError(f"sample_layouts: uc has {uc.shape[0]} rows, expected 1 or one per layout ({L})")
        self._check_first_conv(alphas)
        K = [int(x.shape[0]) for x in xs]
        base = [sum(K[:l]) for l in range(L)]
        n_img = sum(K)
        shape = (n_img,) + tuple(xs[0].shape[1:])
        H, W = int(shape[2]), int(shape[3])
        self._begin_run(shape, None)

        # ---------------- units, instance-major as in plms_sampling (a uniform layout list forms sample()'s forwards) -------
        units = [(l, j, k) for j in range(max(n_inst) + 1) for l in range(L) if j <= n_inst[l] for k in range(K[l])]

        def img_of(u):
            return base[u[0]] + u[2]

        # ---------------- conditioning bank: one row per (layout, input), one unconditional row per layout (or one for all) --
        flat = [(l, j) for l in range(L) for j in range(n_inst[l] + 1)]
        bank, where = self._stack_conds([layouts[l][j] for (l, j) in flat])
        row_lj = {lj: where[k] for k, lj in enumerate(flat)}
        row_of = {u: row_lj[(u[0], u[1])] for u in units}
        row_unc: Dict[int, int] = {}
        if guided:
            uc_shared = uc.shape[0] == 1 or guided_uc_shared(uc)
            off = bank.B
            bank = type(bank).cat([bank, self._uncond(uc[:1] if uc_shared else uc)])
            row_unc = {base[l] + k: off + (0 if uc_shared else l) for l in range(L) for k in range(K[l])}

        # ---------------- phase 1 ---------------------------------------------------------------------------------------------
        per_fwd = self.units_per_forward(self.max_units, H, W)
        chunks, k0 = [], 0
        for n in self.chunk_sizes(len(units), per_fwd):
            chunks.append(units[k0:k0 + n])
            k0 += n
        same_start = all(inp["x"] is lay[0]["x"] or torch.equal(inp["x"], lay[0]["x"]) for lay in layouts for inp in lay[1:])
        hoist = bool(guided and same_start and mis_step > 0)
        x_start = torch.cat([x.to(dev, torch.float32) for x in xs], 0)
        x_units, eps_units = self._phase1(bank, chunks, units, row_of, row_unc, img_of, lambda u: layouts[u[0]][u[1]]["x"][u[2]],
                                          x_start if hoist else None, alphas, time_range, total, mis_step, guided, guidance_scale,
                                          per_fwd)

        # ---------------- merge: the unit latents image after image, an image's global unit first; ONE ragged launch ---------
        by_img = [(l, j, k) for l in range(L) for k in range(K[l]) for j in range(n_inst[l] + 1)]
        unit_off = [0]
        for l in range(L):
            for k in range(K[l]):
                unit_off.append(unit_off[-1] + n_inst[l] + 1)
        lat = torch.zeros((len(by_img),) + tuple(shape[1:]), device=dev, dtype=torch.float32)
        for pos, u in enumerate(by_img):
            if u in x_units:
                lat[pos] = x_units[u]
        if self.crop_and_paste_latents:
            zero4 = [0, 0, 0, 0]
            boxes = torch.tensor([zero4 if j == 0 else [int(v * H) for v in layouts[l][j]["grounding_input"]["boxes"][0][0].tolist()]
                                  for (l, j, k) in by_img], dtype=torch.int32, device=dev).reshape(-1, 4)
            merged = ops.mis_merge_ragged(lat, unit_off, boxes, ops.empty(shape, torch.float32), 1)
        else:
            merged = ops.mis_merge_ragged(lat, unit_off, None, ops.empty(shape, torch.float32), 0)

        # ---------------- phase 2: one row per image, with the eps history of that image's global unit ------------------------
        glob = [(l, 0, k) for l in range(L) for k in range(K[l])]
        old = self._history_stack([eps_units[u] for u in glob]) if mis_step > 0 else self._new_history()
        pair = eng.gather_cond(bank, self._rows(glob, row_of, row_unc, img_of, guided))
        return self._phase2(merged.contiguous(), old, pair, n_img, alphas, time_range, total, mis_step, guided, guidance_scale,
                            list(range(n_img)))


class _OneForwardSampler(_PLMSBase):
    """The loop of the samplers whose step is ONE forward and one fused update launch (``DDIMSampler``, ``DPMSolverSampler``):
    ddim.py:79-105 with the step rule left to ``_step_update``.  Noise comes from ONE overridable attribute,
    ``noise_fn(shape) -> fp32 tensor on the engine's device`` (default ``torch.randn``)."""

    def __init__(self, diffusion, model, schedule="linear", alpha_generator_func=None, set_alpha_scale=None):
        super().__init__(diffusion, model, schedule, alpha_generator_func, set_alpha_scale)
        self.noise_fn = lambda shape: torch.randn(tuple(shape), device=self.engine.device, dtype=torch.float32)

    def _step_update(self, img, e_c, e_u, guidance_scale, i, index, hist):
        """The update behind step i's forward (``index`` = its place in the schedule arrays): the raw eps halves -> the new latents.
        ``hist``: a list the rule may keep its history in, empty at the first step."""
        raise NotImplementedError

    def _sampling(self, shape, input, uc, guidance_scale=1, mask=None, x0=None, start=0):
        """``start``: see ``PLMSSampler.sample``; the step rule's history begins empty at ``start``."""
        start = self._check_start(start)
        eng = self.engine
        ops = eng.ops
        dev = eng.device
        b = shape[0]
        img = input["x"]
        if img is None:
            img = torch.randn(shape, device=dev)
            input["x"] = img
        img = img.to(dev, torch.float32).contiguous()
        guided = uc is not None and guidance_scale != 1
        cond = self._cond(input)
        if guided:
            bank = type(cond).cat([cond, self._uncond(uc)])
            pair = eng.gather_cond(bank, torch.arange(2 * b, device=dev))
        else:
            pair = cond
        if mask is not None:
            assert x0 is not None
            x0 = x0.to(dev, torch.float32).expand(img.shape).contiguous()
            mask = mask.to(dev, torch.float32)
            mask = mask.expand(b, mask.shape[1] if mask.shape[1] == img.shape[1] else 1, *img.shape[2:]).contiguous()
            sqrt_ac = self.diffusion.sqrt_alphas_cumprod.detach().to(torch.float32).cpu()
            sqrt_1m_ac = self.diffusion.sqrt_one_minus_alphas_cumprod.detach().to(torch.float32).cpu()
        time_range = np.flip(self.ddim_timesteps)
        total = self.ddim_timesteps.shape[0]
        alphas = self.alpha_generator_func(len(time_range)) if self.alpha_generator_func is not None else None
        self._check_first_conv(alphas)
        hist: list = []
        for i in range(start, total):
            step = time_range[i]
            self._apply_alpha(alphas, i)                                      # ddim.py:85-88
            index = total - i - 1
            input["timesteps"] = torch.full((b,), int(step), device=dev, dtype=torch.long)
            if mask is not None:                                              # ddim.py:94-98
                img = ops.q_sample_blend(x0, self.noise_fn(img.shape), mask, img, float(sqrt_ac[int(step)]),
                                         float(sqrt_1m_ac[int(step)]), ops.empty(img.shape, torch.float32))
                input["x"] = img
            # p_sample_ddim (ddim.py:107-131): one batched [cond | uncond] forward, its raw halves into the fused update
            t = torch.full((b,), float(step), device=dev, dtype=torch.float32)
            if guided:
                e2 = eng.forward_cond(img, t, pair, out=eng.buf("smp.eps2", (2 * b,) + tuple(img.shape[1:]), torch.float32), paired=True)
                e_c, e_u = e2[:b], e2[b:]
            else:
                e_c, e_u = eng.forward_cond(img, t, pair), None
            img = self._step_update(img, e_c, e_u, guidance_scale, i, index, hist)
            input["x"] = img
        return img


class DDIMSampler(_OneForwardSampler):
    """ddim.py:7-131.  ``eta`` > 0 (stochastic sampling) and the ``mask`` / ``x0`` inpainting blend included.

    Noise comes from ``noise_fn`` in the reference's order within a step: the q_sample draw (ldm.py:18), then the step's (ddim.py:128).
    Deliberate deviation: at ``sigma_t == 0`` no step noise is drawn -- the reference draws one and multiplies it by zero; the
    values are the same, the consumption of the random stream is not."""

    # ---- schedule (ddim.py:25-54; util.py:55-83) ------------------------------------------------------------
    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0.):
        super().make_schedule(ddim_num_steps, ddim_discretize, 0.)             # timesteps, a_t, a_prev, sqrt(1 - a_t): float32
        self.ddim_sigmas = ddim_sigmas(self.ddim_alphas, self.ddim_alphas_prev, ddim_eta)

    @torch.no_grad()
    def sample(self, S, shape, input, uc=None, guidance_scale=1, mask=None, x0=None, eta=0.):
        """``eta`` is an extension: the reference's ``sample`` always schedules eta 0 (ddim.py:59); its eta is reachable through
        ``make_schedule(S, ddim_eta=eta)`` + ``ddim_sampling``, which works here too."""
        self.make_schedule(ddim_num_steps=S, ddim_eta=eta)
        return self.ddim_sampling(shape, input, uc, guidance_scale, mask=mask, x0=x0)

    @torch.no_grad()
    def sample_from(self, S, shape, input, start, uc=None, guidance_scale=1, mask=None, x0=None, eta=0.):
        """``sample`` entered at step ``start`` (see ``PLMSSampler.sample_from``).  ``sample`` and ``ddim_sampling`` keep the reference's
        argument lists."""
        self.make_schedule(ddim_num_steps=S, ddim_eta=eta)
        return self._sampling(shape, input, uc, guidance_scale, mask=mask, x0=x0, start=start)

    @torch.no_grad()
    def ddim_sampling(self, shape, input, uc, guidance_scale=1, mask=None, x0=None):
        return self._sampling(shape, input, uc, guidance_scale, mask=mask, x0=x0)

    def _step_update(self, img, e_c, e_u, guidance_scale, i, index, hist):
        ops = self.engine.ops
        sigma = float(np.float32(self.ddim_sigmas[index]))
        noise = self.noise_fn(img.shape) if sigma != 0 else None
        return ops.ddim_update(img, e_c, e_u, guidance_scale, float(self.ddim_alphas[index]), float(self.ddim_alphas_prev[index]),
                               sigma, float(self.ddim_sqrt_one_minus_alphas[index]), noise, ops.empty(img.shape, torch.float32))


class DDIMSamplerInst(PLMSSamplerInst):
    """The Multi-instance Sampler on DDIM steps: ``PLMSSamplerInst``'s units, conditioning bank, chunking, hoisted first evaluation,
    merge and sharding, with ``DDIMSampler``'s step -- eta > 0 and the ``mask`` / ``x0`` inpainting blend included -- in both phases.
    The reference has no such sampler; phase 1 follows plms_instance.py:86-104 with ddim.py:94-131 as the step, phase 2 is ddim.py.

    A DDIM step carries no history: nothing but the latents travels from phase 1 to phase 2, and a step is ONE forward.

    Noise: every draw comes from ``noise_fn`` (as in ``DDIMSampler``) and is one draw per IMAGE per step, [n_img, 4, H, W], shared by
    the image's N+1 trajectories (they start from the same latent; independent noise would decorrelate what the merge averages).
    Order within a step: the q_sample draw when inpainting, then the step's draw when sigma != 0.  Phase 1 runs chunk-major, so all
    draws of a call are made up front, in step order: the result does not depend on ``max_units`` / chunking, nor on the world size
    (every rank draws, rank 0's draws are broadcast, as the start noise is).  Per-image operands are never gathered per unit: the
    unit kernels (``idf_ddim_update_units``, ``idf_q_sample_blend_units``) read them through a device table unit -> image."""

    def __init__(self, diffusion, model, schedule="linear", alpha_generator_func=None, set_alpha_scale=None, mis=0.0,
                 crop_and_paste_latents=False, shard_across_ranks: Optional[bool] = None, max_units: int = 128,
                 unit_sharding: str = "auto"):
        super().__init__(diffusion, model, schedule, alpha_generator_func, set_alpha_scale, mis, crop_and_paste_latents,
                         shard_across_ranks, max_units, unit_sharding)
        self.noise_fn = lambda shape: torch.randn(tuple(shape), device=self.engine.device, dtype=torch.float32)
        self._inpaint = None            # (x0, mask) of the call being set up, one row per image
        self._run = None                # per-call state of the step hook, see _begin_run

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0.):
        super().make_schedule(ddim_num_steps, ddim_discretize, 0.)
        self.ddim_sigmas = ddim_sigmas(self.ddim_alphas, self.ddim_alphas_prev, ddim_eta)

    @torch.no_grad()
    def sample(self, S, shape, input, uc=None, guidance_scale=1, mask=None, x0=None, eta=0.):
        self.make_schedule(ddim_num_steps=S, ddim_eta=eta)
        return self._sample_call(shape, input, uc, guidance_scale, mask, x0)

    def _sample_call(self, shape, input, uc, guidance_scale, mask, x0):
        """``sample`` behind ``make_schedule``."""
        self._inpaint = None
        if mask is not None:
            assert x0 is not None
            self._inpaint = (x0, mask)
        try:
            return self._mis_sampling(shape, self._without_idle_instances(input), uc, guidance_scale)
        finally:
            self._inpaint = self._run = None        # the draws, x0 / mask and the tables live for the call only

    def plms_sampling(self, *args, **kwargs):
        raise NotImplementedError("DDIMSamplerInst runs DDIM steps: use sample() or sample_layouts()")

    @torch.no_grad()
    def sample_layouts(self, S, layouts, uc=None, guidance_scale=1, eta=0., masks=None, x0s=None):
        """``PLMSSamplerInst.sample_layouts`` on DDIM steps.  ``masks`` / ``x0s``: None, or one entry per layout -- a mask [1 or K_l, 1 or
        4, H, W] and an x0 [1 or K_l, 4, H, W], or None for a layout that is not inpainted (it gets an all-zero mask, which leaves its
        latents bit for bit as they are; the q_sample draw still covers its images)."""
        self.make_schedule(ddim_num_steps=S, ddim_eta=eta)
        return self._layouts_call(layouts, uc, guidance_scale, masks, x0s)

    def _layouts_call(self, layouts, uc, guidance_scale, masks, x0s):
        """``sample_layouts`` behind ``make_schedule``: the per-layout masks / x0s stacked one row per image, then the two phases."""
        self._inpaint = None
        if masks is None and x0s is not None and any(x is not None for x in x0s):
            raise ValueError("sample_layouts: x0s without masks; masks and x0s hold one entry per layout, both given or both None")
        if masks is not None and any(m is not None for m in masks):
            if x0s is None or len(masks) != len(layouts) or len(x0s) != len(layouts) or \
                    any((m is None) != (x is None) for m, x in zip(masks, x0s)):
                raise ValueError("sample_layouts: masks and x0s hold one entry per layout, both given or both None")
            ms, xs = [], []
            per_channel = any(m is not None and m.shape[1] != 1 for m in masks)
            for lay, m, x in zip(layouts, masks, x0s):
                lat = lay[0]["x"]
                K, Cc = int(lat.shape[0]), int(lat.shape[1])
                if m is None:
                    m, x = lat.new_zeros((1, 1) + tuple(lat.shape[2:])), torch.zeros_like(lat[:1])
                ms.append(m.expand(K, Cc if per_channel else 1, *lat.shape[2:]))
                xs.append(x.expand(K, *lat.shape[1:]))
            self._inpaint = (torch.cat([x.to(self.engine.device) for x in xs], 0), torch.cat([m.to(self.engine.device) for m in ms], 0))
        try:
            return self._mis_layouts([self._without_idle_instances(lay) for lay in layouts], uc, guidance_scale)
        finally:
            self._inpaint = self._run = None

    def _without_idle_instances(self, input_all):
        """With no phase-1 step (``int(S * mis) == 0``) the instance trajectories are never advanced and the mean merges N+1 copies
        of the start latent -- (x + x + x) / 3 is not x in fp32.  Only the global input is kept then: the mean of one unit is exact,
        so the call IS ``DDIMSampler`` on the global input, bit for bit.  (Crop-and-paste copies values; it keeps its boxes.)"""
        if int(self.ddim_timesteps.shape[0] * self.mis) == 0 and not self.crop_and_paste_latents:
            return input_all[:1]
        return input_all

    # ---- the step rule ------------------------------------------------------------------------------------------------------
    def _begin_run(self, shape, dist=None):
        """All noise of the call, in step order, and the inpainting operands, one row per image."""
        dev = self.engine.device
        n_img = shape[0]
        total = self.ddim_timesteps.shape[0]
        run = dict(n_img=n_img, tables={}, q_noise=[None] * total, step_noise=[None] * total, x0=None)
        if self._inpaint is not None:
            x0, mask = self._inpaint
            run["x0"] = x0.to(dev, torch.float32).expand(shape).contiguous()
            mask = mask.to(dev, torch.float32)
            run["mask"] = mask.expand(n_img, mask.shape[1] if mask.shape[1] == shape[1] else 1, *shape[2:]).contiguous()
            run["sqrt_ac"] = self.diffusion.sqrt_alphas_cumprod.detach().to(torch.float32).cpu()
            run["sqrt_1m_ac"] = self.diffusion.sqrt_one_minus_alphas_cumprod.detach().to(torch.float32).cpu()

        def draw():
            n = self.noise_fn(shape).to(dev, torch.float32).contiguous()
            if dist is not None:
                dist.broadcast(n, 0)
            return n
        for i in range(total):
            if run["x0"] is not None:
                run["q_noise"][i] = draw()
            if float(np.float32(self.ddim_sigmas[total - i - 1])) != 0:
                run["step_noise"][i] = draw()
        self._run = run
        self._inpaint = None

    def _table(self, rows_img):
        """Device int32 table row -> image of the unit kernels; None when the rows ARE the images, in order."""
        run = self._run
        if list(rows_img) == list(range(run["n_img"])):
            return None
        key = tuple(rows_img)
        if key not in run["tables"]:
            run["tables"][key] = torch.tensor(key, dtype=torch.int32).to(self.engine.device)
        return run["tables"][key]

    def _blend(self, x, i, step, tab):
        """ddim.py:94-98 in front of step i: one launch for all rows."""
        run, ops = self._run, self.engine.ops
        sa, s1 = float(run["sqrt_ac"][step]), float(run["sqrt_1m_ac"][step])
        out = ops.empty(x.shape, torch.float32)
        if tab is None:
            return ops.q_sample_blend(run["x0"], run["q_noise"][i], run["mask"], x, sa, s1, out)
        return ops.q_sample_blend_units(run["x0"], run["q_noise"][i], run["mask"], x, tab, sa, s1, out)

    def _hoist_input(self, x_start):
        # the blend is per image, so an image's trajectories still share step 0's input; every chunk blends its own rows again, to
        # the same values
        if self._run["x0"] is None:
            return x_start
        return self._blend(x_start.contiguous(), 0, int(np.flip(self.ddim_timesteps)[0]), None)

    def _advance(self, x, hist, i, time_range, total, pair, n, guided, guidance_scale, first=None, rows_img=None):
        """The blend (when inpainting) and p_sample_ddim (ddim.py:107-131): one batched [cond | uncond] forward, its raw halves into
        the fused update (``_step_update``)."""
        eng = self.engine
        run = self._run
        step, index = int(time_range[i]), total - i - 1
        tab = self._table(rows_img)
        x = x.contiguous()
        if run["x0"] is not None:
            x = self._blend(x, i, step, tab)
        if first is not None:
            e_c, e_u = first
        else:
            t = torch.full((n,), float(step), device=x.device, dtype=torch.float32)
            if guided:
                e2 = eng.forward_cond(x, t, pair, out=eng.buf("smp.eps2", (2 * n,) + tuple(x.shape[1:]), torch.float32), paired=True)
                e_c, e_u = e2[:n], e2[n:]
            else:
                e_c, e_u = eng.forward_cond(x, t, pair), None
        return self._step_update(x, e_c, e_u, guidance_scale, i, index, hist, tab)

    def _step_update(self, x, e_c, e_u, guidance_scale, i, index, hist, tab):
        """The update behind step i's forward: the raw eps halves -> the new rows; ``tab``: ``_table`` of the rows."""
        ops = self.engine.ops
        sigma = float(np.float32(self.ddim_sigmas[index]))
        noise = self._run["step_noise"][i] if sigma != 0 else None
        args = (guidance_scale, float(self.ddim_alphas[index]), float(self.ddim_alphas_prev[index]), sigma,
                float(self.ddim_sqrt_one_minus_alphas[index]), noise)
        out = ops.empty(x.shape, torch.float32)
        if tab is None:
            return ops.ddim_update(x, e_c, e_u, *args, out)
        return ops.ddim_update_units(x, e_c, e_u, *args, tab, out)

    def _new_history(self):
        return None

    @staticmethod
    def _history_row(hist, k):
        return None

    @staticmethod
    def _history_stack(rows):
        return None


class _DPMSolverRule(object):
    """DPM-Solver++(2M), data-prediction form (Lu et al. 2022, "DPM-Solver++", Algorithm 2; the reference has no DPM solver): what
    ``DPMSolverSampler`` and ``DPMSolverSamplerInst`` share.  A step is one forward and ONE ``idf_dpmpp_update`` launch on the raw
    [cond | uncond] eps halves; its history is the previous step's x0 prediction.  Steps are deterministic."""

    order = 2

    def _timesteps(self, discretize, S, ac, verbose=False):
        if discretize == "logsnr":
            return logsnr_timesteps(S, ac)
        return super()._timesteps(discretize, S, ac, verbose)

    def _set_order(self, order):
        if order not in (1, 2):
            raise ValueError(f"DPM-Solver++: order must be 1 or 2, got {order!r}")
        self.order = int(order)

    def _dpmpp(self, x, e_c, e_u, guidance_scale, index, hist):
        """``hist``: [] at the first step of a trajectory, else [the previous step's x0 prediction] (order 2 only: order 1 keeps none,
        so it never passes an x0_last)."""
        ops = self.engine.ops
        last = hist[0] if hist else None
        a_t = self.ddim_alphas[index]
        c_x, c_0, c_1 = dpmpp_coeffs(a_t, self.ddim_alphas_prev[index], self.ddim_alphas[index + 1] if last is not None else None)
        x0_t = ops.empty(x.shape, torch.float32)
        out = ops.dpmpp_update(x, e_c, e_u, guidance_scale, float(np.sqrt(np.float32(a_t))), float(self.ddim_sqrt_one_minus_alphas[index]),
                               float(c_x), float(c_0), float(c_1), last, ops.empty(x.shape, torch.float32), x0_t)
        if self.order == 2:
            hist[:] = [x0_t]
        return out


class DPMSolverSampler(_DPMSolverRule, _OneForwardSampler):
    """DPM-Solver++(2M) on ``DDIMSampler``'s loop: the alpha gate, the first-conv check and the optional ``mask`` / ``x0`` inpainting
    blend in front of each step (its q_sample draw, from ``noise_fn``, is the only noise).  ``order`` 1 is DDIM with eta 0 up to the
    rounding of the coefficients; ``discretize``: "uniform" (PLMS's and DDIM's timesteps) or "logsnr" (``logsnr_timesteps``)."""

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform"):
        super().make_schedule(ddim_num_steps, ddim_discretize, 0.)

    @torch.no_grad()
    def sample(self, S, shape, input, uc=None, guidance_scale=1, mask=None, x0=None, order=2, discretize="uniform"):
        self._set_order(order)
        self.make_schedule(S, discretize)
        return self._sampling(shape, input, uc, guidance_scale, mask=mask, x0=x0)

    @torch.no_grad()
    def sample_from(self, S, shape, input, start, uc=None, guidance_scale=1, mask=None, x0=None, order=2, discretize="uniform"):
        """``sample`` entered at step ``start`` (see ``PLMSSampler.sample_from``): the step at ``start`` is first order."""
        self._set_order(order)
        self.make_schedule(S, discretize)
        return self._sampling(shape, input, uc, guidance_scale, mask=mask, x0=x0, start=start)

    def _step_update(self, img, e_c, e_u, guidance_scale, i, index, hist):
        return self._dpmpp(img, e_c, e_u, guidance_scale, index, hist)


class DPMSolverSamplerInst(_DPMSolverRule, DDIMSamplerInst):
    """The Multi-instance Sampler on DPM-Solver++(2M) steps: ``DDIMSamplerInst`` (units, bank, chunking, hoist, merge, sharding, the
    inpainting blend through the unit table) with the step's update and the history swapped.  There is no eta: the schedule's sigmas
    are zero, so the q_sample draw is the only noise.  As with PLMS, phase 2 continues from the history of the image's GLOBAL unit:
    its first step is second order when there was a phase 1.  The hoisted first evaluation feeds the first-order first step."""

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform"):
        super().make_schedule(ddim_num_steps, ddim_discretize, 0.)

    @torch.no_grad()
    def sample(self, S, shape, input, uc=None, guidance_scale=1, mask=None, x0=None, order=2, discretize="uniform"):
        self._set_order(order)
        self.make_schedule(S, discretize)
        return self._sample_call(shape, input, uc, guidance_scale, mask, x0)

    @torch.no_grad()
    def sample_layouts(self, S, layouts, uc=None, guidance_scale=1, order=2, discretize="uniform", masks=None, x0s=None):
        """``DDIMSamplerInst.sample_layouts`` with ``order`` / ``discretize`` in place of ``eta``."""
        self._set_order(order)
        self.make_schedule(S, discretize)
        return self._layouts_call(layouts, uc, guidance_scale, masks, x0s)

    def _step_update(self, x, e_c, e_u, guidance_scale, i, index, hist, tab):
        return self._dpmpp(x, e_c, e_u, guidance_scale, index, hist)

    # the history travels as PLMS's eps history does: a list of [rows, ...] tensors, here at most one
    _new_history = PLMSSamplerInst._new_history
    _history_row = staticmethod(PLMSSamplerInst._history_row)
    _history_stack = staticmethod(PLMSSamplerInst._history_stack)
