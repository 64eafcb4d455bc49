"""Pack-time fold of a ResBlock's 1x1 shortcut behind the nine taps of its second 3x3 conv (engine.pack_conv3x3_skip): in fp64 the
packed weight times the row [nine taps of g2 | x] of every output pixel is conv2(g2) + skip(x), the summed bias included -- the layout
[Cout][(ky*3+kx)*C2 + ci | 9*C2 + cx] that idf_conv3x3_skip reads.  The tap sibling the kernel's loader walks that K axis with
(conv_tap_at_skip / conv_tap_step_skip, csrc/gemm_core.h) is mirrored here and checked against the layout for every K-tile."""
import pytest
import torch
import torch.nn.functional as F

from instancediffusion_amd.engine import pack_conv3x3_skip


def im2col_skip(g2, x):
    """[B, C2, H, W], [B, Cx, H, W] -> [B*H*W, 9*C2 + Cx]: the nine pad-1 taps of g2 in the order (ky*3+kx)*C2 + ci, then x's channels."""
    B, C2, H, W = g2.shape
    gp = F.pad(g2, (1, 1, 1, 1))
    taps = [gp[:, :, ky:ky + H, kx:kx + W].permute(0, 2, 3, 1) for ky in range(3) for kx in range(3)]
    return torch.cat(taps + [x.permute(0, 2, 3, 1)], dim=-1).reshape(B * H * W, 9 * C2 + x.shape[1])


@pytest.mark.parametrize("C2,Cx,Cout,H,W", [(4, 6, 5, 3, 4), (8, 2, 8, 1, 1), (6, 16, 6, 5, 2)])
def test_packed_weight_times_im2col_is_conv_plus_shortcut(C2, Cx, Cout, H, W):
    g = torch.Generator().manual_seed(C2 * 100 + Cx)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    w2, b2, ws, bs = rnd(Cout, C2, 3, 3), rnd(Cout), rnd(Cout, Cx, 1, 1), rnd(Cout)
    g2, x = rnd(2, C2, H, W), rnd(2, Cx, H, W)
    wp, bp = pack_conv3x3_skip(w2, b2, ws, bs)
    assert tuple(wp.shape) == (Cout, 9 * C2 + Cx) and wp.is_contiguous() and tuple(bp.shape) == (Cout,)
    got = im2col_skip(g2, x) @ wp.t() + bp
    want = (F.conv2d(g2, w2, b2, padding=1) + F.conv2d(x, ws, bs)).permute(0, 2, 3, 1).reshape(-1, Cout)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_layout_and_fp32_bias_sum():
    """Distinct powers of two: every packed entry is the one tap or shortcut weight the docstring names; the bias is summed in fp32
    (a 16-bit sum of these two would lose the small one)."""
    Cout, C2, Cx = 2, 3, 5
    w2 = torch.arange(Cout * C2 * 9, dtype=torch.float32).reshape(Cout, C2, 3, 3) + 1.0
    ws = -(torch.arange(Cout * Cx, dtype=torch.float32).reshape(Cout, Cx) + 1.0)
    b2, bs = torch.full((Cout,), 1.0), torch.full((Cout,), 2.0 ** -20)
    wp, bp = pack_conv3x3_skip(w2, b2, ws, bs)
    for co in range(Cout):
        for ky in range(3):
            for kx in range(3):
                for ci in range(C2):
                    assert wp[co, (ky * 3 + kx) * C2 + ci] == w2[co, ci, ky, kx]
        assert torch.equal(wp[co, 9 * C2:], ws[co])
    assert bp.dtype == torch.float32 and torch.equal(bp, torch.full((Cout,), 1.0 + 2.0 ** -20))


def tap_at_skip(k, cin):
    tap = min(k // cin, 9)
    return tap, k - tap * cin


def tap_step_skip(tap, ci0, bk, cin):
    ci0 += bk
    if tap < 9 and ci0 >= cin:
        ci0, tap = 0, tap + 1
    return tap, ci0


@pytest.mark.parametrize("C2,Cx", [(320, 64), (320, 640), (640, 960), (1280, 2560), (640, 320), (1280, 640)])
def test_tap_walk_mirror(C2, Cx):
    """The loader's K walk: from any K-tile (a split-K slice may start anywhere, inside the shortcut range too) stepping tile by tile
    names the same (tap, channel) as the direct decode, taps 0..8 cover 9*C2 and tap 9 runs over exactly [0, Cx)."""
    nkt = (9 * C2 + Cx) // 64
    for start in range(nkt):
        tap, ci0 = tap_at_skip(start * 64, C2)
        for kt in range(start, min(start + 3, nkt)):
            assert (tap, ci0) == tap_at_skip(kt * 64, C2)
            assert (tap < 9 and ci0 + 64 <= C2 and tap * C2 + ci0 == kt * 64) or (tap == 9 and 9 * C2 + ci0 == kt * 64 and ci0 + 64 <= Cx)
            tap, ci0 = tap_step_skip(tap, ci0, 64, C2)
