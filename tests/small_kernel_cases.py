"""Cases, fp64 references and the per-element bound for the bandwidth-bound kernels (GroupNorm, LayerNorm, row statistics, the 2x2
patch gather, depthwise 7x7, seg_in_conv, ScaleU, the timestep and UniFusion embeddings, conv_in).  No GPU and no HIP library:
tests/test_small_kernel_refs.py proves this module on the CPU, tests/test_small_kernels_gpu.py applies it to the kernels.

The references are written directly in torch on fp64 and share no code with tests/emul_ops.py.  Each takes the kernel's own inputs
(the 16-bit tensors already rounded, the fp32 ones as they are) and upcasts them.

``within_one_rounding`` is the project's ULP table (tests/test_clip_engine_gpu.py) applied to every element's OWN magnitude:

    |got - want| <= U[dt] * |want| + 1e-5 * max|want|,      U = {bf16: 2^-7, fp16: 2^-10}

One correct rounding of the result costs at most U/2 relative, which leaves a factor of two for the fp32 arithmetic in front of it;
the absolute term is the project's fp32 bar (1e-5 of the output max) and covers cancellation near zero and fp16 subnormals.
"""
import math

import torch
import torch.nn.functional as F

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
U = {"bf16": 2.0 ** -7, "fp16": 2.0 ** -10}
RMS_BAR = {"bf16": 3e-3, "fp16": 3e-3 / 8}            # tests/test_kernels_gpu.py's rel-rms bar, scaled by the mantissa width
RMS_MIN_ELEMS = 4096


def within_one_rounding(got, want64, dt):
    """Share of elements outside the bound above (a NaN in ``got`` counts as outside).  Tests require exactly 0."""
    want = want64.detach().double().cpu()
    got = got.detach().double().cpu().reshape(want.shape)
    bound = U[dt] * want.abs() + 1e-5 * want.abs().max()
    return float((~((got - want).abs() <= bound)).double().mean())


def relmax(got, want64):
    want = want64.detach().double().cpu()
    return float((got.detach().double().cpu().reshape(want.shape) - want).abs().max() / want.abs().max().clamp_min(1e-30))


def rel_rms(got, want64):
    want = want64.detach().double().cpu()
    got = got.detach().double().cpu().reshape(want.shape)
    return float(((got - want).pow(2).mean() / want.pow(2).mean().clamp_min(1e-60)).sqrt())


def gen(shape, seed, scale=1.0, shift=0.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale + shift


# ---- fp64 references ---------------------------------------------------------------------------------------------------------
def groupnorm_ref(x, gamma, beta, eps, silu, stats=None):
    """x [B, HW, C]: 32 groups of C/32 adjacent channels, statistics over (HW, C/32).  ``stats`` = (mean, variance) [B, 32] fp64: the
    statistics the kernel is HANDED (``groupnorm(.., partial=)``) in place of x's own."""
    B, HW, C = x.shape
    xd = x.double().reshape(B, HW, 32, C // 32)
    if stats is None:
        mu = xd.mean(dim=(1, 3), keepdim=True)
        var = (xd - mu).pow(2).mean(dim=(1, 3), keepdim=True)
    else:
        mu, var = (s.double().reshape(B, 1, 32, 1) for s in stats)
    y = ((xd - mu) / (var + eps).sqrt()).view(B, HW, C) * gamma.double() + beta.double()
    return y * torch.sigmoid(y) if silu else y


def row_stats_ref(x, eps):
    xd = x.double()
    mu = xd.mean(-1)
    var = (xd - mu[..., None]).pow(2).mean(-1)
    return mu, 1.0 / (var + eps).sqrt()


def layernorm_ref(x, gamma, beta, eps):
    mu, rstd = row_stats_ref(x, eps)
    return (x.double() - mu[..., None]) * rstd[..., None] * gamma.double() + beta.double()


def layernorm_patch2_ref(x, gamma, beta, eps):
    """x [B, H, W, C] -> [B (H/2) (W/2), 4C]: pixel (b, y, x) to row (b, y/2, x/2), column block ((y&1)*2 + (x&1)) * C."""
    B, H, W, C = x.shape
    y = layernorm_ref(x, gamma, beta, eps)
    out = torch.zeros(B * (H // 2) * (W // 2), 4 * C, dtype=torch.float64)
    for b in range(B):
        for yy in range(H):
            for xx in range(W):
                row = (b * (H // 2) + yy // 2) * (W // 2) + xx // 2
                blk = (yy & 1) * 2 + (xx & 1)
                out[row, blk * C:(blk + 1) * C] = y[b, yy, xx]
    return out


def dwconv7x7_ref(x, w_tap_major, bias):
    """x [B, H, W, C], w [49, C] (tap ky*7 + kx major), pad 3."""
    C = x.shape[-1]
    w = w_tap_major.double().t().reshape(C, 1, 7, 7)
    y = F.conv2d(x.double().permute(0, 3, 1, 2), w, bias.double(), padding=3, groups=C)
    return y.permute(0, 2, 3, 1)


def seg_in_conv_ref(segs, w, bias):
    """3x3 conv, pad 1, Cin -> 3, as the 4x4 patch matrix: row b*(S/4)^2 + py*(S/4) + px, column c*16 + ky*4 + kx."""
    B, _, S, _ = segs.shape
    y = F.conv2d(segs.double(), w.double(), bias.double(), padding=1)
    P = S // 4
    out = torch.zeros(B * P * P, 48, dtype=torch.float64)
    for b in range(B):
        for c in range(3):
            for yy in range(S):
                for xx in range(S):
                    out[b * P * P + (yy // 4) * P + xx // 4, c * 16 + (yy & 3) * 4 + (xx & 3)] = y[b, c, yy, xx]
    return out


def scaleu_ref(h, skip, hscale, s):
    """h [B,H,W,Ch] * hscale | Fourier filter of skip [B,H,W,Cs]: fft2, the centred 2x2 low-frequency window times s, ifft2."""
    _, H, W, _ = skip.shape
    xf = torch.fft.fftshift(torch.fft.fft2(skip.double().permute(0, 3, 1, 2)), dim=(-2, -1))
    mask = torch.ones(H, W, dtype=torch.float64)
    mask[H // 2 - 1:H // 2 + 1, W // 2 - 1:W // 2 + 1] = float(s)
    y = torch.fft.ifft2(torch.fft.ifftshift(xf * mask, dim=(-2, -1))).real.permute(0, 2, 3, 1)
    return torch.cat([h.double() * hscale.double(), y], -1)


def timestep_embedding_ref(t, dim):
    """[cos(t f_k) | sin(t f_k)]: the angle in fp32 as the module computes it, cos / sin of that angle in fp64."""
    half = dim // 2
    freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32) / half)
    a = (t.float()[:, None] * freqs[None]).double()
    return torch.cat([torch.cos(a), torch.sin(a)], -1)


def unifusion_embed_ref(text, loc, tmask, lmask, null_text, null_loc, freqs):
    """[text or null_text | Fourier features of loc or null_loc]; feature block 2j is sin(f_j loc), 2j + 1 is cos(f_j loc).  The
    angle is the module's fp32 product, its sin / cos fp64."""
    parts = []
    for f in freqs:
        a = (f * loc).double()
        parts += [torch.sin(a), torch.cos(a)]
    fe = torch.cat(parts, -1)
    tm, lm = tmask.double()[:, None], lmask.double()[:, None]
    return torch.cat([text.double() * tm + (1 - tm) * null_text.double(), fe * lm + (1 - lm) * null_loc.double()], -1)


def conv_in_ref(x_nchw, w, bias):
    return F.conv2d(x_nchw.double(), w.double(), bias.double(), padding=1).permute(0, 2, 3, 1)


# ---- case lists (the smallest shapes that reach each branch of the kernels) and their inputs ------------------------------
GN_CASES = [(1, 1, 32), (2, 4, 32), (1, 31, 64), (1, 33, 320), (2, 1089, 64), (1, 2049, 32), (1, 100, 2560)]
GN_LARGE_MEAN = (2, 1089, 64)
GN_SPLIT = (1, 49, 64)
LN_CASES = [(M, C) for M in (1, 5, 9) for C in (8, 504, 520, 1032, 1528, 1536)]
LN_LARGE_MEAN = (9, 520)
LNP_CASES = [(2, 2, 2, 8), (1, 4, 6, 96), (1, 6, 2, 520)]
DW_CASES = [(1, 1, 1, 8), (2, 3, 5, 8), (1, 7, 4, 24), (1, 9, 16, 136)]
SEG_CASES = [(1, 1, 4, 48), (2, 32, 8, 64), (1, 30, 12, 72)]
SCALEU_CASES = [(1, 2, 2, 8, 8), (2, 5, 7, 8, 24), (1, 23, 23, 72, 40), (1, 32, 33, 16, 8), (1, 128, 128, 8, 8)]
TEMB_T = (0.0, 1.0, 981.5, 999.0)
TEMB_CASES = [(B, dim, k) for (B, dim) in ((1, 2), (3, 320), (2, 1280)) for k in range(len(TEMB_T))]
UNI_CASES = [(1, 8, 4), (5, 768, 40)]
CONV_IN_CASES = [(1, 4, 5, 7, 320), (2, 4, 8, 8, 64), (1, 3, 6, 6, 32)]
GN_EPS, LN_EPS = 1e-5, 1e-6


def affine(C, seed):
    return 1 + 0.1 * gen((C,), seed), 0.1 * gen((C,), seed + 1)


def large_mean(shape, seed):
    """256 + 2k, k in {-1, 0, 1}: exact in bf16 and fp16, |mean| / std = 157."""
    k = torch.randint(-1, 2, shape, generator=torch.Generator().manual_seed(seed)).float()
    return 256.0 + 2.0 * k


def gn_inputs(case, dt, large=False):
    B, HW, C = case
    x = large_mean(case, 59) if large else gen(case, 500 + HW + C, 1.5, 0.7)
    gm, bt = affine(C, 510 + C)
    return dict(x=x.to(DTYPES[dt]), gamma=gm, beta=bt)


def gn_want(inp, silu):
    return groupnorm_ref(inp["x"], inp["gamma"], inp["beta"], GN_EPS, silu)


def ln_inputs(case, dt, large=False):
    M, C = case
    x = large_mean(case, 61) if large else gen(case, 530 + M + C, 2.0, 0.3)
    gm, bt = affine(C, 540 + C)
    return dict(x=x.to(DTYPES[dt]), gamma=gm, beta=bt)


def ln_want(inp):
    return layernorm_ref(inp["x"], inp["gamma"], inp["beta"], LN_EPS)


def lnp_inputs(case, dt):
    C = case[-1]
    gm, bt = affine(C, 560 + C)
    return dict(x=gen(case, 550 + C, 2.0, 0.5).to(DTYPES[dt]), gamma=gm, beta=bt)


def lnp_want(inp):
    return layernorm_patch2_ref(inp["x"], inp["gamma"], inp["beta"], LN_EPS)


def dw_inputs(case, dt):
    C = case[-1]
    return dict(x=gen(case, 570 + case[1] + C).to(DTYPES[dt]), w=gen((49, C), 571, 1 / 7), bias=gen((C,), 572))


def dw_want(inp):
    return dwconv7x7_ref(inp["x"], inp["w"], inp["bias"])


def seg_inputs(case):
    B, Cin, S, _ = case
    segs = torch.rand(B, Cin, S, S, generator=torch.Generator().manual_seed(580 + Cin))      # real-valued masks, not 0/1
    return dict(segs=segs, w=gen((3, Cin, 3, 3), 581, 0.1), bias=gen((3,), 582))


def seg_want(inp):
    return seg_in_conv_ref(inp["segs"], inp["w"], inp["bias"])


def scaleu_inputs(case, dt):
    B, H, W, Ch, Cs = case
    h, skip = gen((B, H, W, Ch), 590 + H), gen((B, H, W, Cs), 591 + W, 1.0, 0.5)
    hs = torch.tanh(0.3 * gen((Ch,), 592)) + 1
    sm1 = torch.tanh(torch.tensor([-0.4]))                                                   # the kernel takes s - 1
    return dict(h=h.to(DTYPES[dt]), skip=skip.to(DTYPES[dt]), hscale=hs, sm1=sm1)


def scaleu_want(inp):
    return scaleu_ref(inp["h"], inp["skip"], inp["hscale"], float(inp["sm1"][0].double() + 1.0))


def temb_inputs(case):
    B, _, k = case
    return dict(t=torch.tensor([TEMB_T[(k + i) % len(TEMB_T)] for i in range(B)]))


def temb_want(case, inp):
    return timestep_embedding_ref(inp["t"], case[1])


def uni_inputs(case):
    rows, text_dim, D = case
    return dict(text=gen((rows, text_dim), 600), loc=torch.rand(rows, D, generator=torch.Generator().manual_seed(601)),
                tmask=(torch.arange(rows) % 3 != 1).float(), lmask=(torch.arange(rows) % 2 == 0).float(),
                null_text=gen((text_dim,), 602), null_loc=gen((32 * D,), 603), freqs=100.0 ** (torch.arange(16) / 16))


def uni_want(inp):
    return unifusion_embed_ref(**inp)


def conv_in_inputs(case):
    B, Cin, H, W, Cout = case
    return dict(x=gen((B, Cin, H, W), 610 + H), w=gen((Cout, Cin, 3, 3), 611, 1 / 6), bias=gen((Cout,), 612))


def conv_in_want(inp):
    return conv_in_ref(inp["x"], inp["w"], inp["bias"])


def all_wants(dt):
    """(label, fp64 expected output) of every case above: what the CPU tests check the bound on."""
    for case in GN_CASES:
        inp = gn_inputs(case, dt)
        for silu in (False, True):
            yield f"groupnorm{'_silu' if silu else ''} {case}", gn_want(inp, silu)
    yield f"groupnorm large mean {GN_LARGE_MEAN}", gn_want(gn_inputs(GN_LARGE_MEAN, dt, large=True), False)
    yield f"groupnorm split {GN_SPLIT}", gn_want(gn_inputs(GN_SPLIT, dt), True)
    for case in LN_CASES:
        yield f"layernorm {case}", ln_want(ln_inputs(case, dt))
    yield f"layernorm large mean {LN_LARGE_MEAN}", ln_want(ln_inputs(LN_LARGE_MEAN, dt, large=True))
    for case in LNP_CASES:
        yield f"layernorm_patch2 {case}", lnp_want(lnp_inputs(case, dt))
    for case in DW_CASES:
        yield f"dwconv7x7 {case}", dw_want(dw_inputs(case, dt))
    for case in SEG_CASES:
        yield f"seg_in_conv {case}", seg_want(seg_inputs(case))
    for case in SCALEU_CASES:
        yield f"scaleu_concat {case}", scaleu_want(scaleu_inputs(case, dt))
    for case in TEMB_CASES:
        yield f"timestep_embedding {case}", temb_want(case, temb_inputs(case))
    for case in UNI_CASES:
        yield f"unifusion_embed {case}", uni_want(uni_inputs(case))
    for case in CONV_IN_CASES:
        yield f"conv_in {case}", conv_in_want(conv_in_inputs(case))


# ---- cast16: values at which a conversion goes wrong -----------------------------------------------------------------------
def cast16_values(dt):
    """fp32 inputs of the cast kernel: ties to even, +-0, the largest finite value and the first that rounds to inf, nan; for fp16
    also +-1e5, subnormals and the smallest normal.  The contract is ``x.to(dtype)``."""
    if dt == "fp16":
        v = [1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -20, -(1.0 + 2.0 ** -11), 2048.0 + 1.0, 2048.0 + 3.0,
             65504.0, 65519.996, 65520.0, -65504.0, -65520.0, 1e5, -1e5,
             2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, 3 * 2.0 ** -25, -(2.0 ** -24), 2.0 ** -26,
             1e-5, 6e-8]
    else:
        big = torch.tensor([0x7f7f0000, 0x7f7f7fff, 0x7f7f8000, 0x7f7fffff], dtype=torch.int32).view(torch.float32).tolist()
        v = [1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -(1.0 + 2.0 ** -8), 256.0 + 1.0, 256.0 + 3.0,
             big[0], big[1], big[2], big[3], -big[0], -big[2], 2.0 ** -126, 1e-30]
    return torch.tensor([0.0, -0.0, float("nan"), float("inf"), float("-inf")] + v, dtype=torch.float32)


def cast16_input(n, dt):
    """n values: the special ones first (as many as fit), seeded normal data behind them."""
    sp = cast16_values(dt)
    x = gen((n,), 620 + n, 3.0)
    k = min(n, sp.numel())
    x[:k] = sp[:k]
    if n > sp.numel():                                        # the specials again at the very end: last thread, last block
        m = min(n - sp.numel(), sp.numel())
        x[n - m:] = sp[:m]
    return x
