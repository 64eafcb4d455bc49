"""CPU emulation of the two ops of the img2img / hi-res path -- TEST DOUBLE ONLY, like tests/emul_ops_ddim.py (which stays as it is):
the fp32 torch expressions ``idf_q_sample`` and ``idf_resize_planes`` reproduce bit for bit (tests/hires_cases.py), so that
``host/hires.py`` and the samplers' ``start`` run without a GPU."""
from __future__ import annotations

import torch

from tests import hires_cases
from tests.emul_ops_dpmpp import EmulOpsDPMpp


class EmulOpsHires(EmulOpsDPMpp):
    """PLMS's, DDIM's and DPM-Solver++'s step ops plus ``q_sample`` and ``resize_planes``."""

    def plms_update(self, *args):                      # tests/emul_ops.py does not count PLMS's two ops
        self._count("plms_update")
        return super().plms_update(*args)

    def cfg_combine(self, *args):
        self._count("cfg_combine")
        return super().cfg_combine(*args)

    def q_sample(self, x0, noise, sqrt_ac, sqrt_1m_ac, out):
        self._count("q_sample")
        assert x0.shape == noise.shape == out.shape and out.dtype == torch.float32
        out.copy_(hires_cases.q_sample_expr(x0, noise, sqrt_ac, sqrt_1m_ac))
        return out

    def resize_planes(self, src, dst, xi, xw, yi, yw):
        self._count("resize_planes")
        assert src.shape[:-2] == dst.shape[:-2] and src.dtype == dst.dtype == torch.float32
        assert xi.dtype == yi.dtype == torch.int32 and xw.dtype == yw.dtype == torch.float32 and xw.shape[1] in (2, 4)
        assert tuple(xi.shape) == (dst.shape[-1],) and tuple(yi.shape) == (dst.shape[-2],)
        dst.copy_(hires_cases.apply_tables(src, xi, xw, yi, yw, torch.float32))
        return dst
