"""CPU emulation of the two DDIM step ops -- TEST DOUBLE ONLY, like tests/emul_ops.py (which stays as it is): the fp32 torch
expressions the HIP kernels reproduce bit for bit (tests/ddim_cases.py), so that ``DDIMSampler``'s host logic runs without a GPU."""
from __future__ import annotations

from tests import ddim_cases
from tests.emul_ops import EmulOps


class EmulOpsDDIM(EmulOps):
    def ddim_update(self, x, e_cond, e_uncond, guidance, a_t, a_prev, sigma_t, sqrt_1m_at, noise, out, pred_x0=None):
        self._count("ddim_update")
        assert (noise is None) == (sigma_t == 0), "a step draws noise exactly when its sigma is not zero"
        x_prev, p0 = ddim_cases.ddim_update_expr(x, e_cond, e_uncond, guidance, a_t, a_prev, sigma_t, sqrt_1m_at, noise)
        out.copy_(x_prev)
        if pred_x0 is not None:
            pred_x0.copy_(p0)
        return out

    def q_sample_blend(self, x0, noise, mask, img, sqrt_ac, sqrt_1m_ac, out):
        self._count("q_sample_blend")
        assert mask.shape[1] in (1, out.shape[1]) and mask.shape[0] == out.shape[0]
        out.copy_(ddim_cases.q_sample_blend_expr(x0, noise, mask, img, sqrt_ac, sqrt_1m_ac))
        return out
