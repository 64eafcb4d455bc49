"""CPU emulation of the two DDIM step ops over work units -- TEST DOUBLE ONLY, like tests/emul_ops_ddim.py (which stays as it is): a
row gather through the unit -> image table (entries clamped, as the kernels clamp them) in front of the fp32 torch expressions of
tests/ddim_cases.py, so that ``DDIMSamplerInst``'s host logic runs without a GPU.  The ragged merge comes from tests/emul_ops_layouts.py."""
from __future__ import annotations

import torch

from tests import ddim_cases
from tests.emul_ops_ddim import EmulOpsDDIM
from tests.emul_ops_layouts import EmulOpsLayouts


def gather_rows(t, img_of, U):
    """Row img_of[u] of the per-image tensor t for every unit u (clamped to t's rows); img_of None: the rows themselves (U == B)."""
    if img_of is None:
        assert t.shape[0] == U, "without a table unit u is image u"
        return t
    idx = torch.as_tensor(img_of).to(torch.long).clamp(0, t.shape[0] - 1)
    assert idx.numel() == U
    return t[idx]


def ddim_update_units_expr(x, e_cond, e_uncond, guidance, a_t, a_prev, sigma_t, sqrt_1m_at, noise, img_of):
    nz = None if noise is None else gather_rows(noise, img_of, x.shape[0])
    return ddim_cases.ddim_update_expr(x, e_cond, e_uncond, guidance, a_t, a_prev, sigma_t, sqrt_1m_at, nz)


def q_sample_blend_units_expr(x0, noise, mask, img, img_of, sqrt_ac, sqrt_1m_ac):
    U = img.shape[0]
    return ddim_cases.q_sample_blend_expr(gather_rows(x0, img_of, U), gather_rows(noise, img_of, U), gather_rows(mask, img_of, U), img,
                                          sqrt_ac, sqrt_1m_ac)


class EmulOpsDDIMMis(EmulOpsDDIM, EmulOpsLayouts):
    def ddim_update_units(self, x, e_cond, e_uncond, guidance, a_t, a_prev, sigma_t, sqrt_1m_at, noise, img_of, out, pred_x0=None):
        self._count("ddim_update_units")
        assert (noise is None) == (sigma_t == 0), "a step draws noise exactly when its sigma is not zero"
        assert img_of is None or (img_of.dtype == torch.int32 and img_of.numel() == out.shape[0])
        x_prev, p0 = ddim_update_units_expr(x, e_cond, e_uncond, guidance, a_t, a_prev, sigma_t, sqrt_1m_at, noise, img_of)
        out.copy_(x_prev)
        if pred_x0 is not None:
            pred_x0.copy_(p0)
        return out

    def q_sample_blend_units(self, x0, noise, mask, img, img_of, sqrt_ac, sqrt_1m_ac, out):
        self._count("q_sample_blend_units")
        assert img_of.dtype == torch.int32 and img_of.numel() == out.shape[0]
        assert mask.shape[1] in (1, out.shape[1]) and mask.shape[0] == x0.shape[0] == noise.shape[0]
        out.copy_(q_sample_blend_units_expr(x0, noise, mask, img, img_of, sqrt_ac, sqrt_1m_ac))
        return out
