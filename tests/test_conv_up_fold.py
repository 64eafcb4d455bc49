"""Pack-time fold of the nearest-x2 upsample into the 3x3 conv weights (engine.pack_conv_up2x): four 2x2 phase convs on the
low-resolution image equal conv3x3(pad 1) of the upsampled image.  CPU, fp32: pins the identity and the packing order
[phase = py*2+px][Cout][(ty*2+tx)*Cin + ci] that idf_conv_up2x_folded reads."""
import pytest
import torch
import torch.nn.functional as F

from instancediffusion_amd.engine import pack_conv_up2x


def apply_folded(x, wf, b):
    """x [B, Cin, H, W] fp32, wf [4, Cout, 4*Cin] as packed, b [Cout] -> [B, Cout, 2H, 2W]: phase (py, px) is a 2x2 conv whose
    window starts at (y - 1 + py, x - 1 + px), written to the output pixels (2y + py, 2x + px)."""
    B, Cin, H, W = x.shape
    Cout = wf.shape[1]
    out = x.new_empty(B, Cout, 2 * H, 2 * W)
    for py in range(2):
        for px in range(2):
            w = wf[py * 2 + px].reshape(Cout, 2, 2, Cin).permute(0, 3, 1, 2)            # [Cout, Cin, ty, tx]
            xp = F.pad(x, (1 - px, px, 1 - py, py))                                     # zeros: left / right / top / bottom
            out[:, :, py::2, px::2] = F.conv2d(xp, w, b)
    return out


@pytest.mark.parametrize("B,Cin,Cout,H,W", [(2, 8, 6, 5, 7), (1, 4, 4, 1, 1), (1, 3, 5, 1, 6), (2, 5, 3, 4, 1), (1, 16, 16, 8, 8),
                                            (3, 2, 7, 2, 3)])
def test_fold_equals_upsample_conv(B, Cin, Cout, H, W):
    g = torch.Generator().manual_seed(1000 * H + W)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g)
    b = torch.randn(Cout, generator=g)
    want = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, b, padding=1)
    wf = pack_conv_up2x(w)
    assert wf.shape == (4, Cout, 4 * Cin) and wf.dtype == torch.float32
    got = apply_folded(x, wf, b)
    # fp32 round-off only: each output sums 9 Cin products either way, in a different association
    tol = 32 * torch.finfo(torch.float32).eps * float(want.abs().max()) * (9 * Cin) ** 0.5
    assert float((got - want).abs().max()) <= tol


def test_fold_packing_order():
    """w[co, ci, ky, kx] = distinct powers: every packed entry is the sum the docstring of pack_conv_up2x names."""
    Cout, Cin = 2, 3
    w = torch.zeros(Cout, Cin, 3, 3)
    for ky in range(3):
        for kx in range(3):
            w[:, :, ky, kx] = float(2 ** (ky * 3 + kx))
    w = w * (1 + torch.arange(Cin, dtype=torch.float32))[None, :, None, None] + 1000.0 * torch.arange(Cout, dtype=torch.float32)[:, None, None, None]
    wf = pack_conv_up2x(w)
    rows = {0: ([0], [1, 2]), 1: ([0, 1], [2])}                  # [py][ty] -> 3x3 rows summed
    for py in range(2):
        for px in range(2):
            for ty in range(2):
                for tx in range(2):
                    want = sum(w[:, :, ky, kx] for ky in rows[py][ty] for kx in rows[px][tx])
                    got = wf[py * 2 + px][:, (ty * 2 + tx) * Cin:(ty * 2 + tx + 1) * Cin]
                    assert torch.equal(got, want), (py, px, ty, tx)
