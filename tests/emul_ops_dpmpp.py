"""CPU emulation of the DPM-Solver++ step op -- TEST DOUBLE ONLY, like tests/emul_ops_ddim.py (which stays as it is): the fp32 torch
expression ``idf_dpmpp_update`` reproduces bit for bit (tests/dpmpp_cases.py), so that ``DPMSolverSampler``'s and
``DPMSolverSamplerInst``'s host logic runs without a GPU."""
from __future__ import annotations

import math

import torch

from tests import dpmpp_cases
from tests.emul_ops_ddim import EmulOpsDDIM
from tests.emul_ops_ddim_mis import EmulOpsDDIMMis


class _DpmppUpdate(object):
    def dpmpp_update(self, x, e_cond, e_uncond, guidance, sqrt_at, sqrt_1m_at, c_x, c_0, c_1, x0_last, out, x0_out):
        self._count("dpmpp_update")
        if x0_last is not None:
            self._count("dpmpp_update_order2")
        assert sqrt_at > 0 and all(math.isfinite(v) for v in (sqrt_at, sqrt_1m_at, c_x, c_0, c_1))
        assert x0_out is not None and x0_out.shape == out.shape and out.dtype == x0_out.dtype == torch.float32
        r, p = dpmpp_cases.dpmpp_update_expr(x, e_cond, e_uncond, guidance, sqrt_at, sqrt_1m_at, c_x, c_0, c_1, x0_last)
        out.copy_(r)
        x0_out.copy_(p)
        return out


class EmulOpsDPMpp(_DpmppUpdate, EmulOpsDDIM):
    pass


class EmulOpsDPMppMis(_DpmppUpdate, EmulOpsDDIMMis):
    pass
