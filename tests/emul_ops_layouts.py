"""CPU emulation of ``idf_mis_merge_ragged`` -- TEST DOUBLE ONLY, like tests/emul_ops.py (which stays as it is): the sequential fp32
torch loops the HIP kernel reproduces bit for bit, so that ``PLMSSamplerInst.sample_layouts``'s host logic runs without a GPU."""
from __future__ import annotations

import torch

from instancediffusion_amd.ops import HipOps
from tests.emul_ops import EmulOps


def merge_ragged_expr(lat, unit_off, boxes_i32, mode):
    """lat [U,C,H,W] fp32, unit_off: B + 1 ints, boxes_i32 [U,4] or None -> [B,C,H,W].  Mode 0: s = 0; s = s + lat[k] in unit
    order; s / count.  Mode 1: the image's first unit, then every later unit's box pasted in order (dim 2 <- box[0]:box[2],
    dim 3 <- box[1]:box[3])."""
    out = []
    for b in range(len(unit_off) - 1):
        k0, k1 = unit_off[b], unit_off[b + 1]
        if mode == 0:
            s = torch.zeros_like(lat[0])
            for k in range(k0, k1):
                s = s + lat[k]
            out.append(s / float(k1 - k0))
        else:
            v = lat[k0].clone()
            for k in range(k0 + 1, k1):
                bb = boxes_i32[k].tolist()
                v[:, bb[0]:bb[2], bb[1]:bb[3]] = lat[k][:, bb[0]:bb[2], bb[1]:bb[3]]
            out.append(v)
    return torch.stack(out)


class EmulOpsLayouts(EmulOps):
    def mis_merge_ragged(self, lat, unit_off, boxes_i32, out, mode):
        self._count("mis_merge_ragged")
        off = HipOps.check_unit_offsets(unit_off, out.shape[0], lat.shape[0])
        assert lat.dtype == torch.float32 and (mode == 0 or tuple(boxes_i32.shape) == (lat.shape[0], 4))
        out.copy_(merge_ragged_expr(lat, off, boxes_i32, mode))
        return out
