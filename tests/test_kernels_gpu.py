"""Per-kernel parity on a real MI355X: every C-ABI entry point vs a plain PyTorch fp32 reference of the same op
(tests/emul_ops.EmulOps in fp32) on the same seeded inputs.  Tolerances are relative to the output max:
bf16 storage, fp32 accumulation -> 2^-7 (one bf16 ulp of the largest element) unless stated; fp32 outputs 1e-5.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16_TOL = 2.0 ** -7


@pytest.fixture(scope="module")
def ops():
    from instancediffusion_amd.ops import HipOps
    return HipOps(torch.bfloat16)


@pytest.fixture(scope="module")
def ref():
    from tests.emul_ops import EmulOps
    return EmulOps(torch.float32)


def gen(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def to16(t):
    return t.to(torch.bfloat16)


def relmax(a, b):
    return float((a.float().cpu() - b.float().cpu()).abs().max() / b.float().abs().max().clamp_min(1e-20))


def dev(t):
    return t.cuda()


def rel_rms(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float(((a - b).pow(2).mean() / b.pow(2).mean().clamp_min(1e-30)).sqrt())


# Second per-kernel metric next to `relmax` (which is relative to the LARGEST output and would hide errors on the small
# ones): relative RMS error over all elements.  One 16-bit rounding of every output gives 2^-9 / sqrt(3) = 1.1e-3 in bf16;
# bar = 3e-3 (attention, whose probabilities are rounded to 16 bits before P.V: 6e-3).
BF16_RMS_TOL = 3e-3


# ---------------------------------------------------------------------------------------------------
# GEMM
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (4096, 320, 320), (300, 640, 1280), (77, 64, 768),
                                   (184, 1280, 768), (64, 1280, 5120), (2, 20160, 1280), (1000, 960, 192)])
def test_gemm_bias(ops, ref, M, N, K):
    a, w, b = to16(gen((M, K), 1)), to16(gen((N, K), 2, K ** -0.5)), gen((N,), 3)
    want = a.float() @ w.float().t() + b
    out = ops.gemm(dev(a), dev(w), ops.empty((M, N)), bias=dev(b))
    torch.cuda.synchronize()
    assert relmax(out, want) < BF16_TOL
    assert rel_rms(out, want) < BF16_RMS_TOL


def test_gemm_is_transpose_detecting(ops):
    """A = I-like structure with asymmetric B (guide rule: symmetric inputs hide row/col swaps)."""
    M = N = K = 128
    a = torch.eye(M, K)
    w = (torch.arange(N)[:, None] * 3 + torch.arange(K)[None, :] * 0.25) / 64.0
    out = ops.gemm(dev(to16(a)), dev(to16(w)), ops.empty((M, N)))
    torch.cuda.synchronize()
    want = to16(a).float() @ to16(w).float().t()
    assert relmax(out, want) < BF16_TOL


@pytest.mark.parametrize("act", [None, "silu", "gelu"])
def test_gemm_epilogues(ops, act):
    M, N, K = 520, 320, 640
    a, w, b = to16(gen((M, K), 4)), to16(gen((N, K), 5, K ** -0.5)), gen((N,), 6)
    res = to16(gen((M, N), 7))
    rowb = to16(gen((4, N), 8))
    gate = torch.tensor([0.37])
    acc = a.float() @ w.float().t() + b + rowb.float()[torch.arange(M) // 130]
    if act == "silu":
        acc = torch.nn.functional.silu(acc)
    elif act == "gelu":
        acc = torch.nn.functional.gelu(acc)
    want = res.float() + 0.37 * acc
    out = ops.gemm(dev(a), dev(w), ops.empty((M, N)), bias=dev(b), rowbias=dev(rowb), rows_per_batch=130,
                   res=dev(res), gate=dev(gate), act=act)
    torch.cuda.synchronize()
    assert relmax(out, want) < BF16_TOL
    # in-place residual (out aliases res), as the engine uses it
    buf = dev(res.clone())
    ops.gemm(dev(a), dev(w), buf, bias=dev(b), res=buf)
    torch.cuda.synchronize()
    assert relmax(buf, res.float() + a.float() @ w.float().t() + b) < BF16_TOL


def test_gemm_geglu(ops, ref):
    from instancediffusion_amd.engine import pack_geglu
    M, C = 333, 320
    a = to16(gen((M, C), 9))
    w, b = gen((8 * C, C), 10, C ** -0.5), gen((8 * C,), 11)
    w16 = to16(w)
    h = a.float() @ w16.float().t() + b
    x, g = h.chunk(2, -1)
    want = x * torch.nn.functional.gelu(g)
    wp, bp = pack_geglu(w16.float(), b)
    out = ops.gemm(dev(a), dev(to16(wp)), ops.empty((M, 4 * C)), bias=dev(bp), geglu=True)
    torch.cuda.synchronize()
    assert relmax(out, want) < BF16_TOL


def test_gemm_batched_transposed_v(ops):
    """V^T[b] = Wv . X_b^T with a zero-padded leading dimension (what the attention kernel consumes)."""
    B, N, C = 3, 77, 320
    x, wv = to16(gen((B, N, C), 12)), to16(gen((C, C), 13, C ** -0.5))
    vt = ops.zeros((B, C, 128))
    ops.gemm(dev(wv), dev(x), vt[:, :, :N])
    torch.cuda.synchronize()
    want = torch.einsum("ck,bnk->bcn", wv.float(), x.float())
    assert relmax(vt[:, :, :N], want) < BF16_TOL
    assert float(vt[:, :, N:].float().abs().max()) == 0.0


def test_gemm_f32_out_and_strided_out(ops):
    M, N, K = 60, 768, 256
    a, w = to16(gen((2, 30, K), 14)), to16(gen((N, K), 15, K ** -0.5))
    objs = ops.zeros((2, 184, N))
    ops.gemm(dev(a), dev(w), objs[:, 30:60, :])
    out32 = ops.gemm(dev(a.view(M, K)), dev(w), ops.empty((M, N), torch.float32))
    torch.cuda.synchronize()
    want = a.float() @ w.float().t()
    assert relmax(objs[:, 30:60], want) < BF16_TOL
    assert float(objs[:, :30].float().abs().max()) == 0.0 and float(objs[:, 60:].float().abs().max()) == 0.0
    assert relmax(out32, want.view(M, N)) < 1e-5


# ---------------------------------------------------------------------------------------------------
# conv
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,Cin,Cout,stride,up", [
    (1, 16, 16, 64, 64, 1, 0), (2, 8, 8, 320, 640, 1, 0), (2, 16, 16, 128, 128, 2, 0), (1, 8, 8, 128, 128, 1, 1),
    (1, 12, 12, 192, 320, 1, 0), (1, 7, 9, 64, 64, 2, 0), (1, 64, 64, 320, 320, 1, 0)])
def test_conv3x3(ops, ref, B, H, W, Cin, Cout, stride, up):
    from instancediffusion_amd.engine import pack_conv3x3
    x = to16(gen((B, H, W, Cin), 20))
    w4 = gen((Cout, Cin, 3, 3), 21, (9 * Cin) ** -0.5)
    b = gen((Cout,), 22)
    wp = to16(pack_conv3x3(w4))
    Ho = ((H << up) - 1) // stride + 1
    Wo = ((W << up) - 1) // stride + 1
    rowb = to16(gen((B, Cout), 23))
    res = to16(gen((B, Ho, Wo, Cout), 24))
    want = ref.conv3x3(x.float(), wp.float(), torch.empty(B, Ho, Wo, Cout), bias=b, rowbias=rowb.float(),
                       res=res.float(), stride=stride, upsample=up)
    out = ops.conv3x3(dev(x), dev(wp), ops.empty((B, Ho, Wo, Cout)), bias=dev(b), rowbias=dev(rowb), res=dev(res),
                      stride=stride, upsample=up)
    torch.cuda.synchronize()
    assert relmax(out, want) < BF16_TOL
    assert rel_rms(out, want) < BF16_RMS_TOL


def test_conv3x3_out_nchw(ops, ref):
    from instancediffusion_amd.engine import pack_conv3x3
    B, H, W, Cin = 2, 16, 16, 64
    x = to16(gen((B, H, W, Cin), 25))
    w4 = torch.zeros(64, Cin, 3, 3)
    w4[:4] = gen((4, Cin, 3, 3), 26, (9 * Cin) ** -0.5)
    b = torch.zeros(64)
    b[:4] = gen((4,), 27)
    wp = to16(pack_conv3x3(w4))
    want = ref.conv3x3(x.float(), wp.float(), torch.empty(B, 4, H, W), bias=b, n_valid=4)
    out = ops.conv3x3(dev(x), dev(wp), ops.empty((B, 4, H, W), torch.float32), bias=dev(b), n_valid=4)
    torch.cuda.synchronize()
    assert relmax(out, want) < 1e-4          # fp32 output of bf16 operands: accumulation-order differences only


@pytest.mark.parametrize("B,Cin,H,W,Cout", [(2, 4, 16, 16, 64), (3, 4, 10, 13, 320), (64, 4, 64, 64, 320), (1, 4, 96, 96, 320),
                                            (2, 4, 8, 6, 512)])
def test_conv_in(ops, ref, B, Cin, H, W, Cout):
    """First conv from the fp32 NCHW latent.  The UNet's 4 -> 320 case runs on the matrix cores (round 4, conv_in_mfma_kernel:
    both operands split into bf16 head + tail, K = 108, fp32-class accuracy); every other channel count -- incl. the VAE's
    4 -> 512 -- on the persistent quad kernel (weights staged once per workgroup; 4 horizontally adjacent pixels per thread).
    Widths that are not a multiple of 4 and the bench shape included."""
    x, w, b = gen((B, Cin, H, W), 28), gen((Cout, Cin, 3, 3), 29, 1 / 6), gen((Cout,), 30)
    want = ref.conv_in(x, w, b, torch.empty(B, H, W, Cout))
    out = ops.conv_in(dev(x), dev(w), dev(b), ops.empty((B, H, W, Cout)))
    torch.cuda.synchronize()
    assert relmax(out, want) < BF16_TOL and rel_rms(out, want) < BF16_RMS_TOL


# ---------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,d,Nq,n0,n1", [
    (1, 8, 40, 256, 256, 0), (2, 8, 40, 256, 256, 184), (1, 8, 80, 64, 64, 184), (2, 8, 160, 100, 100, 184),
    (1, 8, 40, 4096, 4096, 184), (2, 8, 40, 200, 77, 0), (1, 8, 8, 256, 256, 184), (1, 8, 16, 64, 64, 0),
    (1, 8, 32, 16, 16, 184), (1, 2, 160, 130, 77, 0)])
def test_attention(ops, ref, B, H, d, Nq, n0, n1):
    C = H * d
    q, k0, v0 = to16(gen((B, Nq, C), 40)), to16(gen((B, n0, C), 41)), to16(gen((B, n0, C), 42))
    ld0 = (n0 + 63) // 64 * 64
    vt0 = torch.zeros(B, C, ld0, dtype=torch.bfloat16)
    vt0[:, :, :n0] = v0.transpose(1, 2)
    kw = {}
    rkw = {}
    if n1:
        k1, v1 = to16(gen((B, n1, C), 43)), to16(gen((B, n1, C), 44))
        vt1 = torch.full((B, C, 192), float("nan"), dtype=torch.bfloat16)    # pad must be masked by the kernel
        vt1[:, :, :n1] = v1.transpose(1, 2)
        kw = dict(k1=dev(k1), vt1=dev(vt1), n1=n1)
        rkw = dict(k1=k1.float(), vt1=torch.nan_to_num(vt1.float()), n1=n1)
    want = ref.attention(q.float(), k0.float(), vt0.float(), n0, torch.empty(B, Nq, C), H, **rkw)
    out = ops.attention(dev(q), dev(k0), dev(vt0), n0, ops.empty((B, Nq, C)), H, **kw)
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    assert relmax(out, want) < 2 * BF16_TOL          # P is rounded to bf16 inside the kernel
    assert rel_rms(out, want) < 2 * BF16_RMS_TOL


@pytest.mark.parametrize("B,H,d,Nq,n0", [(8, 8, 40, 4096 + 40, 77), (32, 8, 80, 1024, 77), (8, 8, 160, 4096, 77),
                                         (16, 8, 40, 2048, 128), (20, 8, 40, 1024, 40)])
def test_attention_resident_keys(ops, ref, B, H, d, Nq, n0):
    """Cross-attention shapes large enough for the resident-key path (<= 2 key tiles staged once per workgroup, which then
    walks several 128-query blocks; launch_attn picks it from B * H * query blocks >= 2048): ragged last block, one- and
    two-tile key sets, all three head dims of the UNet."""
    C = H * d
    q, k0, v0 = to16(gen((B, Nq, C), 70)), to16(gen((B, n0, C), 71)), to16(gen((B, n0, C), 72))
    ld0 = (n0 + 63) // 64 * 64
    vt0 = torch.full((B, C, ld0), float("nan"), dtype=torch.bfloat16)        # pad must be masked by the kernel
    vt0[:, :, :n0] = v0.transpose(1, 2)
    want = ref.attention(q.float(), k0.float(), torch.nan_to_num(vt0.float()), n0, torch.empty(B, Nq, C), H)
    out = ops.attention(dev(q), dev(k0), dev(vt0), n0, ops.empty((B, Nq, C)), H)
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    assert relmax(out, want) < 2 * BF16_TOL
    assert rel_rms(out, want) < 2 * BF16_RMS_TOL


def test_attention_forced_rescale(ops, ref):
    """Online-softmax rescale branch: a spiked key in a LATE tile must rescale earlier accumulations."""
    B, H, d, N = 1, 8, 40, 512
    C = H * d
    q, k, v = gen((B, N, C), 45), gen((B, N, C), 46), gen((B, N, C), 47)
    k[:, 400] = q[:, 7] * 4.0                       # row 7 gets a huge score at kv=400 (7th tile)
    q, k, v = to16(q), to16(k), to16(v)
    vt = v.transpose(1, 2).contiguous()
    want = ref.attention(q.float(), k.float(), vt.float(), N, torch.empty(B, N, C), H)
    out = ops.attention(dev(q), dev(k), dev(vt), N, ops.empty((B, N, C)), H)
    torch.cuda.synchronize()
    assert relmax(out, want) < 2 * BF16_TOL


def test_attention_strided_qk_views(ops, ref):
    """q/k as column slices of a fused [B, N, 2C] projection buffer (how the engine calls it)."""
    B, H, d, N = 2, 8, 40, 320
    C = H * d
    qk = to16(gen((B, N, 2 * C), 48))
    v = to16(gen((B, N, C), 49))
    vt = v.transpose(1, 2).contiguous()
    want = ref.attention(qk[:, :, :C].float(), qk[:, :, C:].float(), vt.float(), N, torch.empty(B, N, C), H)
    dqk = dev(qk)
    out = ops.attention(dqk[:, :, :C], dqk[:, :, C:], dev(vt), N, ops.empty((B, N, C)), H)
    torch.cuda.synchronize()
    assert relmax(out, want) < 2 * BF16_TOL


# ---------------------------------------------------------------------------------------------------
# norms / scaleu / misc
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,HW,C,silu", [(2, 256, 64, True), (1, 4096, 320, True), (2, 64, 2560, True),
                                         (3, 1024, 960, False), (1, 144, 1920, True), (2, 16, 128, False)])
def test_groupnorm(ops, ref, B, HW, C, silu):
    x = to16(gen((B, HW, C), 50) * 1.5 + 0.7)
    gm, bt = 1 + 0.1 * gen((C,), 51), 0.1 * gen((C,), 52)
    want = ref.groupnorm(x.float(), torch.empty(B, HW, C), gm, bt, 1e-5, silu)
    out = ops.groupnorm(dev(x), ops.empty((B, HW, C)), dev(gm), dev(bt), 1e-5, silu)
    torch.cuda.synchronize()
    assert relmax(out, want) < BF16_TOL
    assert rel_rms(out, want) < BF16_RMS_TOL
    out2 = ops.groupnorm(dev(x), ops.empty((B, HW, C)), dev(gm), dev(bt), 1e-5, silu)
    torch.cuda.synchronize()
    assert torch.equal(out, out2), "GroupNorm must be bitwise run-to-run deterministic"


@pytest.mark.parametrize("B,HW,C", [(1, 4096, 320), (2, 1000, 640), (1, 144, 1920)])
def test_groupnorm_large_mean_over_std(ops, B, HW, C):
    """Variance is accumulated SHIFTED (per-thread pivot) and merged with Chan's formula, not as E[x^2] - mu^2: a group
    whose |mean| is ~160x its std (about the most 8 mantissa bits can express) must still normalise to output rounding.
    The inputs (256 + 2k, k in {-1, 0, 1}) are exact in bf16 and fp16, so the fp64 reference sees the kernel's values."""
    g = torch.Generator().manual_seed(59)
    k = torch.randint(-1, 2, (B, HW, C), generator=g).float()
    x = 256.0 + 2.0 * k                                         # std 1.63, mean 256: E[x^2] - mu^2 in fp32 loses ~5 digits
    assert torch.equal(to16(x).float(), x)
    gm, bt = torch.ones(C), torch.zeros(C)
    xd = x.double().view(B, HW, 32, C // 32)
    mu = xd.mean(dim=(1, 3), keepdim=True)
    var = xd.var(dim=(1, 3), unbiased=False, keepdim=True)
    want = ((xd - mu) / (var + 1e-5).sqrt()).view(B, HW, C).float()
    out = ops.groupnorm(dev(to16(x)), ops.empty((B, HW, C)), dev(gm), dev(bt), 1e-5, False)
    torch.cuda.synchronize()
    err = float((out.float().cpu() - want).abs().max())
    print(f"[parity] groupnorm mean/std=157 B{B} HW{HW} C{C}: max abs err {err:.3e} (values up to {float(want.abs().max()):.2f})")
    assert err < 6e-3                                           # one bf16 rounding of outputs up to ~1.23 is 3.9e-3


@pytest.mark.parametrize("M,C", [(4096, 320), (1000, 640), (77, 1280), (5, 64), (184, 128)])
def test_layernorm(ops, ref, M, C):
    x = to16(gen((M, C), 53) * 2 + 0.3)
    gm, bt = 1 + 0.1 * gen((C,), 54), 0.1 * gen((C,), 55)
    want = ref.layernorm(x.float(), torch.empty(M, C), gm, bt)
    out = ops.layernorm(dev(x), ops.empty((M, C)), dev(gm), dev(bt))
    torch.cuda.synchronize()
    assert relmax(out, want) < BF16_TOL


@pytest.mark.parametrize("B,H,W,Ch,Cs", [(2, 8, 8, 1280, 1280), (1, 64, 64, 320, 320), (1, 16, 16, 1280, 640),
                                         (2, 12, 12, 128, 64), (1, 24, 48, 64, 64), (3, 96, 96, 72, 40), (2, 32, 32, 640, 640)])
def test_scaleu_concat(ops, B, H, W, Ch, Cs):
    from oracle import ref_cpu
    h, skip = to16(gen((B, H, W, Ch), 56)), to16(gen((B, H, W, Cs), 57) + 0.5)
    hs, s = torch.tanh(0.3 * gen((Ch,), 58)) + 1, torch.tanh(torch.tensor([-0.4])) + 1
    # reference algorithm (FFT) in NCHW fp32 on the bf16-rounded inputs
    want_h = h.float() * hs
    want_s = ref_cpu.fourier_filter(skip.float().permute(0, 3, 1, 2), 1, s).permute(0, 2, 3, 1)
    out = ops.scaleu_concat(dev(h), dev(skip), ops.empty((B, H, W, Ch + Cs)), dev(hs), dev(s - 1))
    torch.cuda.synchronize()
    assert relmax(out[..., :Ch], want_h) < BF16_TOL
    assert relmax(out[..., Ch:], want_s) < BF16_TOL


def test_small_kernels(ops, ref):
    from oracle import ref_cpu
    t = torch.tensor([981.0, 1.0, 500.0])
    out = ops.timestep_embedding(dev(t), ops.empty((3, 320)))
    want = ref_cpu.timestep_embedding(t, 320)
    torch.cuda.synchronize()
    assert float((out.float().cpu() - want).abs().max()) < 2.0 ** -7
    # unifusion embed
    rows, D = 60, 40
    text, loc = gen((rows, 768), 60), torch.rand(rows, D, generator=torch.Generator().manual_seed(61))
    tm = (torch.arange(rows) % 3 != 0).float()
    lm = (torch.arange(rows) % 2 == 0).float()
    nt, nl = gen((768,), 62), gen((32 * D,), 63)
    freqs = 100.0 ** (torch.arange(16) / 16)
    want = ref.unifusion_embed(text, loc, tm, lm, nt, nl, freqs, torch.empty(rows, 768 + 32 * D))
    out = ops.unifusion_embed(dev(text), dev(loc), dev(tm), dev(lm), dev(nt), dev(nl), dev(freqs),
                              ops.empty((rows, 768 + 32 * D)))
    torch.cuda.synchronize()
    assert relmax(out, want) < BF16_TOL
    # cfg + plms + merge (fp32 kernels: 1e-5)
    ec, eu, x = gen((2, 4, 16, 16), 64), gen((2, 4, 16, 16), 65), gen((2, 4, 16, 16), 66)
    old = [gen((2, 4, 16, 16), 67 + i) for i in range(3)]
    et = ops.cfg_combine(dev(ec), dev(eu), 7.5, ops.empty(ec.shape, torch.float32))
    torch.cuda.synchronize()
    assert relmax(et, eu + 7.5 * (ec - eu)) < 1e-6
    a_t, a_prev = 0.0047, 0.0313
    s1m = float(torch.sqrt(1.0 - torch.tensor(a_t)))
    for mode in range(5):
        want = ref.plms_update(x, ec, old, eu, mode, a_t, a_prev, s1m, torch.empty_like(x))
        got = ops.plms_update(dev(x), dev(ec), [dev(o) for o in old], dev(eu), mode, a_t, a_prev, s1m,
                              ops.empty(x.shape, torch.float32))
        torch.cuda.synchronize()
        assert relmax(got, want) < 1e-5, mode
    lat = gen((4, 2, 4, 16, 16), 70)
    boxes = torch.tensor([[1, 2, 9, 12], [4, 0, 16, 5], [0, 0, 3, 3]], dtype=torch.int32)
    for mode in (0, 1):
        want = ref.mis_merge(lat, boxes, torch.empty(2, 4, 16, 16), mode)
        got = ops.mis_merge(dev(lat), dev(boxes), ops.empty((2, 4, 16, 16), torch.float32), mode)
        torch.cuda.synchronize()
        assert relmax(got, want) < 1e-6


# ---------------------------------------------------------------------------------------------------
# UniFusion mask-tokenizer pieces (ConvNeXt)
# ---------------------------------------------------------------------------------------------------
def test_convnext_pieces(ops, ref):
    # seg_in_conv: 30 -> 3 conv written as the stem patch matrix
    segs = (torch.rand(2, 30, 64, 64, generator=torch.Generator().manual_seed(80)) > 0.6).float()
    w, b = gen((3, 30, 3, 3), 81, 0.1), gen((3,), 82)
    want = ref.seg_in_conv(segs, w, b, torch.zeros(2 * 16 * 16, 64))
    out = ops.seg_in_conv(dev(segs), dev(w), dev(b), ops.zeros((2 * 16 * 16, 64)))
    torch.cuda.synchronize()
    assert relmax(out, want) < BF16_TOL
    # depthwise 7x7
    for (B, H, C) in [(2, 16, 96), (1, 8, 768), (1, 32, 192)]:
        x = to16(gen((B, H, H, C), 83))
        wt, bb = gen((49, C), 84, 1 / 7), gen((C,), 85)
        want = ref.dwconv7x7(x.float(), wt, bb, torch.empty(B, H, H, C))
        out = ops.dwconv7x7(dev(x), dev(wt), dev(bb), ops.empty((B, H, H, C)))
        torch.cuda.synchronize()
        assert relmax(out, want) < BF16_TOL
    # LayerNorm + 2x2 patch gather
    x = to16(gen((2, 8, 8, 96), 86) * 2 + 0.5)
    gm, bt = 1 + 0.1 * gen((96,), 87), 0.1 * gen((96,), 88)
    want = ref.layernorm_patch2(x.float(), torch.zeros(2 * 16, 384), gm, bt, 1e-6)
    out = ops.layernorm_patch2(dev(x), ops.zeros((2 * 16, 384)), dev(gm), dev(bt), 1e-6)
    torch.cuda.synchronize()
    assert relmax(out, want) < BF16_TOL
    # LayerNorm into a K-padded buffer (C = 96 -> ld 128), pad stays zero
    x2 = to16(gen((100, 96), 89))
    buf = ops.zeros((100, 128))
    ops.layernorm(dev(x2), buf[:, :96], dev(gm), dev(bt), 1e-6)
    torch.cuda.synchronize()
    assert relmax(buf[:, :96], ref.layernorm(x2.float(), torch.empty(100, 96), gm, bt, 1e-6)) < BF16_TOL
    assert float(buf[:, 96:].float().abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------
# persistent big-tile GEMM / conv kernel (gemm_big.hip), forced through idf_set_tuning
# ---------------------------------------------------------------------------------------------------
@pytest.fixture
def big():
    """Force the persistent big-tile kernel for every qualifying shape; yields a callable returning how many launches it
    served since the fixture started (so a test cannot pass on the 128x128 kernels by accident)."""
    from instancediffusion_amd import _lib
    lib = _lib.load()
    prev = lib.idf_set_tuning(0, 2)
    start = lib.idf_get_stat(0)
    yield lambda: lib.idf_get_stat(0) - start
    lib.idf_set_tuning(0, prev)


@pytest.mark.parametrize("M,N,K", [(1000, 320, 320), (4113, 640, 1280), (300, 512, 256), (256, 1280, 128),
                                   (33280, 640, 320), (66560 + 5, 320, 192)])
def test_gemm_big_bias(ops, big, M, N, K):
    a, w, b = to16(gen((M, K), 1)), to16(gen((N, K), 2, K ** -0.5)), gen((N,), 3)
    want = a.float() @ w.float().t() + b
    out = ops.gemm(dev(a), dev(w), ops.empty((M, N)), bias=dev(b))
    torch.cuda.synchronize()
    assert big() == 1
    assert relmax(out, want) < BF16_TOL
    assert rel_rms(out, want) < BF16_RMS_TOL


def test_gemm_big_matches_small_kernel_bitwise_on_exact_data(ops, big):
    """Integer-valued operands: every partial sum is exact in fp32, so both kernels must agree bit for bit."""
    from instancediffusion_amd import _lib
    M, N, K = 70000, 960, 320
    g = torch.Generator().manual_seed(5)
    a = torch.randint(-4, 5, (M, K), generator=g).to(torch.bfloat16)
    w = torch.randint(-4, 5, (N, K), generator=g).to(torch.bfloat16)
    o_big = ops.gemm(dev(a), dev(w), ops.empty((M, N)))
    torch.cuda.synchronize()
    assert big() == 1
    _lib.load().idf_set_tuning(0, 0)
    o_small = ops.gemm(dev(a), dev(w), ops.empty((M, N)))
    torch.cuda.synchronize()
    _lib.load().idf_set_tuning(0, 2)
    assert big() == 1
    assert torch.equal(o_big, o_small)
    assert torch.equal(o_big.float().cpu(), (a.float() @ w.float().t()).to(torch.bfloat16).float())


@pytest.mark.parametrize("act", [None, "silu", "gelu"])
def test_gemm_big_epilogues(ops, big, act):
    M, N, K = 1300, 640, 320
    a, w, b = to16(gen((M, K), 4)), to16(gen((N, K), 5, K ** -0.5)), gen((N,), 6)
    res = to16(gen((M, N), 7))
    rowb = to16(gen((4, N), 8))
    gate = torch.tensor([0.37])
    acc = a.float() @ w.float().t() + b + rowb.float()[torch.arange(M) // 325]
    if act == "silu":
        acc = torch.nn.functional.silu(acc)
    elif act == "gelu":
        acc = torch.nn.functional.gelu(acc)
    want = res.float() + 0.37 * acc
    out = ops.gemm(dev(a), dev(w), ops.empty((M, N)), bias=dev(b), rowbias=dev(rowb), rows_per_batch=325,
                   res=dev(res), gate=dev(gate), act=act)
    torch.cuda.synchronize()
    assert relmax(out, want) < BF16_TOL
    buf = dev(res.clone())                                   # in-place residual
    ops.gemm(dev(a), dev(w), buf, bias=dev(b), res=buf)
    out32 = ops.gemm(dev(a), dev(w), ops.empty((M, N), torch.float32))
    torch.cuda.synchronize()
    assert big() == 3
    assert relmax(buf, res.float() + a.float() @ w.float().t() + b) < BF16_TOL
    assert relmax(out32, a.float() @ w.float().t()) < 1e-5


@pytest.mark.parametrize("M,C", [(700, 320), (2100, 640)])
def test_gemm_big_geglu(ops, big, M, C):
    from instancediffusion_amd.engine import pack_geglu
    a = to16(gen((M, C), 9))
    w, b = gen((8 * C, C), 10, C ** -0.5), gen((8 * C,), 11)
    w16 = to16(w)
    h = a.float() @ w16.float().t() + b
    x, g = h.chunk(2, -1)
    want = x * torch.nn.functional.gelu(g)
    wp, bp = pack_geglu(w16.float(), b)
    out = ops.gemm(dev(a), dev(to16(wp)), ops.empty((M, 4 * C)), bias=dev(bp), geglu=True)
    torch.cuda.synchronize()
    assert big() == 1
    assert relmax(out, want) < BF16_TOL


def test_gemm_big_f16(big):
    from instancediffusion_amd.ops import HipOps
    o16 = HipOps(torch.float16)
    M, N, K = 777, 320, 640
    a, w = gen((M, K), 31).half(), gen((N, K), 32, K ** -0.5).half()
    out = o16.gemm(dev(a), dev(w), o16.empty((M, N)))
    torch.cuda.synchronize()
    assert big() == 1
    assert relmax(out, a.float() @ w.float().t()) < 2.0 ** -10


@pytest.mark.parametrize("B,H,W,Cin,Cout,stride,up", [
    (2, 16, 16, 128, 320, 1, 0), (3, 16, 16, 64, 640, 2, 0), (1, 8, 8, 128, 320, 1, 1), (1, 12, 20, 192, 256, 1, 0),
    (1, 7, 9, 64, 320, 2, 0), (5, 64, 64, 320, 320, 1, 0)])
def test_conv3x3_big(ops, ref, big, B, H, W, Cin, Cout, stride, up):
    from instancediffusion_amd.engine import pack_conv3x3
    x = to16(gen((B, H, W, Cin), 20))
    w4 = gen((Cout, Cin, 3, 3), 21, (9 * Cin) ** -0.5)
    b = gen((Cout,), 22)
    wp = to16(pack_conv3x3(w4))
    Ho = ((H << up) - 1) // stride + 1
    Wo = ((W << up) - 1) // stride + 1
    rowb = to16(gen((B, Cout), 23))
    res = to16(gen((B, Ho, Wo, Cout), 24))
    want = ref.conv3x3(x.float(), wp.float(), torch.empty(B, Ho, Wo, Cout), bias=b, rowbias=rowb.float(),
                       res=res.float(), stride=stride, upsample=up)
    out = ops.conv3x3(dev(x), dev(wp), ops.empty((B, Ho, Wo, Cout)), bias=dev(b), rowbias=dev(rowb), res=dev(res),
                      stride=stride, upsample=up)
    torch.cuda.synchronize()
    assert big() == 1
    assert relmax(out, want) < BF16_TOL


def test_big_kernel_split_k(ops, ref):
    """Few tiles, long K (the 8x8-level convs and ff-out GEMMs at batch 64: 64 tiles on 256 CUs): the persistent kernel
    splits K over 4 work items per tile, fp32 partials in the workspace, epilogue in the reducer.  Default tuning (auto)."""
    from instancediffusion_amd import _lib
    from instancediffusion_amd.engine import pack_conv3x3
    lib = _lib.load()
    start = lib.idf_get_stat(0)
    # conv 8x8, batch 64, 1280 -> 1280 (K = 11520 = 180 K-tiles -> 4 slices of 45 on 64 tiles) with every epilogue term
    B, H, W, Cin, Cout = 64, 8, 8, 1280, 1280
    x = to16(gen((B, H, W, Cin), 60))
    w4 = gen((Cout, Cin, 3, 3), 61, (9 * Cin) ** -0.5)
    b = gen((Cout,), 62)
    wp = to16(pack_conv3x3(w4))
    rowb, res = to16(gen((B, Cout), 63)), to16(gen((B, H, W, Cout), 64))
    want = ref.conv3x3(x.float(), wp.float(), torch.empty(B, H, W, Cout), bias=b, rowbias=rowb.float(), res=res.float())
    out = ops.conv3x3(dev(x), dev(wp), ops.empty((B, H, W, Cout)), bias=dev(b), rowbias=dev(rowb), res=dev(res))
    torch.cuda.synchronize()
    assert lib.idf_get_stat(0) - start == 1, "the 8x8-level conv must run on the persistent kernel (split-K)"
    assert relmax(out, want) < BF16_TOL
    # dense ff-out GEMM at the 8x8 level: M = 4096, N = 1280, K = 5120 (80 K-tiles -> 4 slices of 20), in-place residual
    M, N, K = 4096, 1280, 5120
    a, w, bias = to16(gen((M, K), 65)), to16(gen((N, K), 66, K ** -0.5)), gen((N,), 67)
    buf = dev(to16(gen((M, N), 68)))
    want = buf.float().cpu() + a.float() @ w.float().t() + bias
    ops.gemm(dev(a), dev(w), buf, bias=dev(bias), res=buf)
    torch.cuda.synchronize()
    assert lib.idf_get_stat(0) - start == 2
    assert relmax(buf, want) < BF16_TOL
    # exact data: split-K partial sums are exact in fp32 -> bitwise equal to the unsplit small-tile kernel
    g = torch.Generator().manual_seed(69)
    ai = torch.randint(-3, 4, (M, K), generator=g).to(torch.bfloat16)
    wi = torch.randint(-3, 4, (N, K), generator=g).to(torch.bfloat16)
    o1 = ops.gemm(dev(ai), dev(wi), ops.empty((M, N)))
    lib.idf_set_tuning(0, 0)
    o2 = ops.gemm(dev(ai), dev(wi), ops.empty((M, N)))
    torch.cuda.synchronize()
    lib.idf_set_tuning(0, 1)
    assert torch.equal(o1, o2)


def test_big_kernel_hybrid_tail_split(ops, ref):
    """Tile counts just above a whole number of 256-CU rounds (the 18-row forwards of a sharded / small batch: 288 tiles =
    1.125 rounds) used to fall back to the 128^2 kernels.  Now the leading full rounds run whole tiles and the tail rows are
    cut into K-slices (fp32 partials + reducer over the tail rows only).  Dense GEMM with every epilogue term, a 3x3 conv, and
    bit-for-bit equality with the small-tile kernel on exact data; the launch counter shows the persistent kernel took them."""
    from instancediffusion_amd import _lib
    from instancediffusion_amd.engine import pack_conv3x3
    lib = _lib.load()
    prev_mode = lib.idf_set_tuning(0, 3)                                 # automatic dispatch + hybrid tail split (opt-in)
    # (the hybrid form serves grids BELOW the automatic rule's occupancy bar; the shapes here sit at 56 %, between the
    # round-3 bar the mechanism was built under and the round-4 default of 50 %)
    prev_bar = lib.idf_set_tuning(_lib.IDF_TUNE_BIG_MIN_EFF, 80)
    start = lib.idf_get_stat(0)
    # 18 rows of the 64^2 level: M = 73728 -> 288 tiles of 256 x 320; K = 1280 (20 K-tiles -> 5 slices of 4)
    M, N, K = 18 * 4096, 320, 1280
    a, w, bias = to16(gen((M, K), 165)), to16(gen((N, K), 166, K ** -0.5)), gen((N,), 167)
    buf = dev(to16(gen((M, N), 168)))
    want = buf.float().cpu() + a.float() @ w.float().t() + bias
    ops.gemm(dev(a), dev(w), buf, bias=dev(bias), res=buf)
    torch.cuda.synchronize()
    assert lib.idf_get_stat(0) - start == 1, "288 tiles: persistent kernel with a split tail"
    assert relmax(buf, want) < BF16_TOL and rel_rms(buf, want) < BF16_RMS_TOL
    # ff-out shape (K = 1280: 20 K-tiles) with a partial last m-tile, exact data: equal to the small-tile kernel bit for bit
    M2, N2, K2 = 18 * 4096 - 100, 320, 1280
    g = torch.Generator().manual_seed(169)
    ai = torch.randint(-3, 4, (M2, K2), generator=g).to(torch.bfloat16)
    wi = torch.randint(-3, 4, (N2, K2), generator=g).to(torch.bfloat16)
    o1 = ops.gemm(dev(ai), dev(wi), ops.empty((M2, N2)))
    torch.cuda.synchronize()
    assert lib.idf_get_stat(0) - start == 2
    lib.idf_set_tuning(0, 0)
    o2 = ops.gemm(dev(ai), dev(wi), ops.empty((M2, N2)))
    torch.cuda.synchronize()
    lib.idf_set_tuning(0, 3)
    assert torch.equal(o1, o2)
    assert torch.equal(o1.float().cpu(), (ai.float() @ wi.float().t()).to(torch.bfloat16).float())
    # conv 320 -> 320 at 64^2, batch 18 (288 tiles, 45 K-tiles), bias + time-embedding row bias + residual
    B, H, W, Cin, Cout = 18, 64, 64, 320, 320
    x = to16(gen((B, H, W, Cin), 170))
    wp = to16(pack_conv3x3(gen((Cout, Cin, 3, 3), 171, (9 * Cin) ** -0.5)))
    b = gen((Cout,), 172)
    rowb, res = to16(gen((B, Cout), 173)), to16(gen((B, H, W, Cout), 174))
    want = ref.conv3x3(x.float(), wp.float(), torch.empty(B, H, W, Cout), bias=b, rowbias=rowb.float(), res=res.float())
    out = ops.conv3x3(dev(x), dev(wp), ops.empty((B, H, W, Cout)), bias=dev(b), rowbias=dev(rowb), res=dev(res))
    torch.cuda.synchronize()
    assert lib.idf_get_stat(0) - start == 3
    assert relmax(out, want) < BF16_TOL and rel_rms(out, want) < BF16_RMS_TOL
    # two n-tiles per row block (N = 640: 576 tiles = 2.25 rounds -> the tail starts on an m-tile boundary; 10 K-tiles, 2 slices)
    M3, N3, K3 = 18 * 4096, 640, 640
    ai = torch.randint(-3, 4, (M3, K3), generator=g).to(torch.bfloat16)
    wi = torch.randint(-3, 4, (N3, K3), generator=g).to(torch.bfloat16)
    o3 = ops.gemm(dev(ai), dev(wi), ops.empty((M3, N3)))
    torch.cuda.synchronize()
    assert lib.idf_get_stat(0) - start == 4
    assert torch.equal(o3.float().cpu(), (ai.float() @ wi.float().t()).to(torch.bfloat16).float())
    # K = 320 (5 K-tiles): no slice count leaves >= 4 K-tiles per slice -> the launch goes to the small-tile kernels
    ai = torch.randint(-3, 4, (18 * 4096, 320), generator=g).to(torch.bfloat16)
    wi = torch.randint(-3, 4, (320, 320), generator=g).to(torch.bfloat16)
    o4 = ops.gemm(dev(ai), dev(wi), ops.empty((18 * 4096, 320)))
    torch.cuda.synchronize()
    assert lib.idf_get_stat(0) - start == 4
    assert torch.equal(o4.float().cpu(), (ai.float() @ wi.float().t()).to(torch.bfloat16).float())
    # default mode (1): no tail split -- 288 tiles go to the small-tile kernels, identical rows stay bitwise equal
    lib.idf_set_tuning(0, 1)
    same = to16(gen((1, K), 175)).expand(M, K).contiguous()
    o5 = ops.gemm(dev(same), dev(w), ops.empty((M, N)))
    torch.cuda.synchronize()
    assert lib.idf_get_stat(0) - start == 4 and bool((o5 == o5[:1]).all())
    lib.idf_set_tuning(0, prev_mode)
    lib.idf_set_tuning(_lib.IDF_TUNE_BIG_MIN_EFF, prev_bar)


# ---------------------------------------------------------------------------------------------------
# the latency kernel of the small-batch launches (gemm_kernel_ring, gemm_conv.hip), forced through idf_set_tuning
# ---------------------------------------------------------------------------------------------------
@pytest.fixture
def ring():
    """Keep the persistent kernel out and send EVERY GEMM / conv launch to the latency kernel (threshold = any tile count);
    yields a callable returning how many launches it served since the fixture started."""
    from instancediffusion_amd import _lib
    lib = _lib.load()
    prev_big = lib.idf_set_tuning(_lib.IDF_TUNE_GEMM_BIG, 0)
    prev = lib.idf_set_tuning(_lib.IDF_TUNE_GEMM_RING, 1 << 30)
    start = lib.idf_get_stat(_lib.IDF_STAT_GEMM_RING_LAUNCHES)
    yield lambda: lib.idf_get_stat(_lib.IDF_STAT_GEMM_RING_LAUNCHES) - start
    lib.idf_set_tuning(_lib.IDF_TUNE_GEMM_RING, prev)
    lib.idf_set_tuning(_lib.IDF_TUNE_GEMM_BIG, prev_big)


# shapes of a 2-row forward (K = 320: the whole K range in flight; split-K at the 16x16 / 8x8 levels), fewer K-tiles than ring
# stages (K = 64 / 128 / 192), ragged M and N, a 2-row time-embedding GEMM
@pytest.mark.parametrize("M,N,K", [(8192, 320, 320), (2048, 640, 640), (512, 1280, 1280), (128, 1280, 5120), (1000, 960, 192),
                                   (128, 128, 64), (77, 64, 768), (300, 72, 128), (2, 10240, 1280), (4096, 1280, 2560)])
def test_gemm_ring_bias(ops, ref, ring, M, N, K):
    test_gemm_bias(ops, ref, M, N, K)
    assert ring() == 1


def test_gemm_ring_declines_what_only_split_k_fills(ops, ref, ring):
    """129 ... 191 tiles with a long K (the 2-row time-embedding GEMM: 158 tiles, 20 K-tiles): variants 1 / 2 split K for their
    two workgroups per CU, the one-per-CU latency kernel cannot and leaves the launch to them."""
    test_gemm_bias(ops, ref, 2, 20160, 1280)
    assert ring() == 0


@pytest.mark.parametrize("act", [None, "gelu"])
def test_gemm_ring_epilogues(ops, ref, ring, act):
    test_gemm_epilogues(ops, act)
    test_gemm_geglu(ops, ref)
    test_gemm_batched_transposed_v(ops)
    test_gemm_f32_out_and_strided_out(ops)
    assert ring() >= 6


@pytest.mark.parametrize("M,N,K,mode", [(300, 640, 320, "row"), (4096, 1280, 640, "row"), (200, 2560, 320, "geglu"),
                                        (320, 200, 320, "col"), (640, 2048, 640, "col")])
def test_gemm_ring_layernorm_folded(ops, ring, M, N, K, mode):
    test_gemm_layernorm_folded(ops, M, N, K, mode)
    assert ring() >= 1


@pytest.mark.parametrize("M,C,stats", [(4096, 1280, "none"), (200, 320, "given"), (1000, 320, "self")])
def test_gemm_ring_geglu_period32(ops, ring, M, C, stats):
    test_gemm_geglu_period32(ops, M, C, stats)
    assert ring() >= 2


@pytest.mark.parametrize("M,C,own", [(8192 + 16, 320, True), (2048, 640, False), (1000, 320, True)])
def test_gemm_ring_fused_qkv_fallback(ops, ring, M, C, own):
    test_gemm_fused_qkv_transposed_v(ops, M, C, own)
    assert ring() >= 2


@pytest.mark.parametrize("B,H,W,Cin,Cout,stride,up", [
    (1, 16, 16, 64, 64, 1, 0), (2, 8, 8, 320, 640, 1, 0), (2, 16, 16, 128, 128, 2, 0), (1, 8, 8, 128, 128, 1, 1),
    (1, 12, 12, 192, 320, 1, 0), (1, 7, 9, 64, 64, 2, 0), (2, 8, 8, 1280, 1280, 1, 0), (2, 8, 8, 1280, 1280, 1, 1)])
def test_conv3x3_ring(ops, ref, ring, B, H, W, Cin, Cout, stride, up):
    test_conv3x3(ops, ref, B, H, W, Cin, Cout, stride, up)
    assert ring() == 1


def test_gemm_ring_matches_small_kernels_bitwise_on_exact_data(ops, ring):
    """Integer-valued operands: every partial sum is exact in fp32, so the latency kernel (its own split-K rule included) and the
    K-loop variants 1 / 2 it replaces must agree bit for bit -- dense with a residual, split-K dense, and a split-K conv."""
    from instancediffusion_amd import _lib
    from instancediffusion_amd.engine import pack_conv3x3
    lib = _lib.load()
    g = torch.Generator().manual_seed(71)

    def both(fn):
        o1 = fn()
        torch.cuda.synchronize()
        n1 = ring()
        lib.idf_set_tuning(_lib.IDF_TUNE_GEMM_RING, 0)
        o2 = fn()
        torch.cuda.synchronize()
        lib.idf_set_tuning(_lib.IDF_TUNE_GEMM_RING, 1 << 30)
        assert ring() == n1, "the second run must not touch the latency kernel"
        return o1, o2

    for M, N, K in [(8192, 320, 320), (512, 1280, 1280), (130, 1280, 5120)]:
        a = torch.randint(-3, 4, (M, K), generator=g).to(torch.bfloat16)
        w = torch.randint(-3, 4, (N, K), generator=g).to(torch.bfloat16)
        r = torch.randint(-8, 9, (M, N), generator=g).to(torch.bfloat16)
        o1, o2 = both(lambda: ops.gemm(dev(a), dev(w), ops.empty((M, N)), res=dev(r)))
        assert torch.equal(o1, o2)
        assert torch.equal(o1.float().cpu(), (a.float() @ w.float().t() + r.float()).to(torch.bfloat16).float())
    B, H, Cin, Cout = 2, 8, 1280, 1280
    x = torch.randint(-2, 3, (B, H, H, Cin), generator=g).to(torch.bfloat16)
    wp = pack_conv3x3(torch.randint(-2, 3, (Cout, Cin, 3, 3), generator=g).float()).to(torch.bfloat16)
    o1, o2 = both(lambda: ops.conv3x3(dev(x), dev(wp), ops.empty((B, H, H, Cout))))
    assert torch.equal(o1, o2)


# ---------------------------------------------------------------------------------------------------
# the 64-queries-per-wave attention kernel (attention4.hip), forced through idf_set_tuning
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(params=[1, 2, 3, 4, 5], ids=["v4-4waves", "v4-8waves", "v4-4waves-plain-grid", "v4w-1wave-per-simd", "v4w-2waves-per-simd"])
def attn2(request):
    """The 64-queries-per-wave LDS-DMA kernel (attention4.hip) in its two block orders and the asm-scheduled stream of
    attention4w.hip (round 6; d = 40 only -- other head dims fall through to attention4.hip) with 128 / 64 queries per wave;
    yields the launch counter."""
    from instancediffusion_amd import _lib
    lib = _lib.load()
    prev = lib.idf_set_tuning(1, request.param)
    start = lib.idf_get_stat(1)
    yield lambda: lib.idf_get_stat(1) - start
    lib.idf_set_tuning(1, prev)


@pytest.mark.parametrize("B,H,d,Nq,n0,n1", [
    (1, 8, 40, 256, 256, 0), (2, 8, 40, 256, 256, 184), (1, 8, 40, 4096, 4096, 184), (2, 8, 40, 200, 72, 0),
    (1, 8, 40, 300, 304, 184), (1, 3, 24, 100, 128, 8), (2, 4, 56, 513, 520, 0), (1, 8, 40, 1000, 1000, 40)])
def test_attention_v2(ops, ref, attn2, B, H, d, Nq, n0, n1):
    C = H * d
    q, k0, v0 = to16(gen((B, Nq, C), 40)), to16(gen((B, n0, C), 41)), to16(gen((B, n0, C), 42))
    ld0 = (n0 + 63) // 64 * 64
    vt0 = torch.full((B, C, ld0), float("nan"), dtype=torch.bfloat16)        # pad must never reach the output
    vt0[:, :, :n0] = v0.transpose(1, 2)
    kw = {}
    rkw = {}
    if n1:
        k1, v1 = to16(gen((B, n1, C), 43)), to16(gen((B, n1, C), 44))
        vt1 = torch.full((B, C, 192), float("nan"), dtype=torch.bfloat16)
        vt1[:, :, :n1] = v1.transpose(1, 2)
        kw = dict(k1=dev(k1), vt1=dev(vt1), n1=n1)
        rkw = dict(k1=k1.float(), vt1=torch.nan_to_num(vt1.float()), n1=n1)
    want = ref.attention(q.float(), k0.float(), torch.nan_to_num(vt0.float()), n0, torch.empty(B, Nq, C), H, **rkw)
    out = ops.attention(dev(q), dev(k0), dev(vt0), n0, ops.empty((B, Nq, C)), H, **kw)
    torch.cuda.synchronize()
    assert attn2() == 1
    assert torch.isfinite(out.float()).all()
    assert relmax(out, want) < 2 * BF16_TOL


def test_attention_v2_declines_an_output_it_cannot_store_with_16_byte_vectors(ops, ref, attn2):
    """the 64-query kernel's epilogue writes O as 16-B vectors; an output whose row stride is only 8-B aligned
    (ldo % 8 == 4, legal for idf_attention) must go to the 32-query kernel instead of being written misaligned."""
    B, H, d, N = 1, 8, 40, 256
    C = H * d
    q, k0, v0 = to16(gen((B, N, C), 140)), to16(gen((B, N, C), 141)), to16(gen((B, N, C), 142))
    vt0 = v0.transpose(1, 2).contiguous()
    want = ref.attention(q.float(), k0.float(), vt0.float(), N, torch.empty(B, N, C), H)
    wide = ops.zeros((B, N, C + 4))                              # ldo = 324: rows 8-B aligned only
    out = ops.attention(dev(q), dev(k0), dev(vt0), N, wide[:, :, :C], H)
    torch.cuda.synchronize()
    assert attn2() == 0, "the launch must have gone to the 32-query kernel"
    assert relmax(out, want) < 2 * BF16_TOL
    assert float(wide[:, :, C:].float().abs().max()) == 0.0
    out2 = ops.attention(dev(q), dev(k0), dev(vt0), N, ops.empty((B, N, C)), H)
    torch.cuda.synchronize()
    assert attn2() == 1 and relmax(out2, want) < 2 * BF16_TOL


def test_attention_v2_forced_rescale_and_strided_views(ops, ref, attn2):
    """Late spike (rescale branch after many alpha == 1 tiles) on q/k column slices of a fused projection buffer."""
    B, H, d, N = 2, 8, 40, 640
    C = H * d
    qk = gen((B, N, 2 * C), 45)
    v = to16(gen((B, N, C), 47))
    qk[:, 500, C:] = qk[:, 7, :C] * 4.0             # key 500 (8th tile) gets a huge score for query 7
    qk[:, 3, C:] = qk[:, 300, :C] * 4.0             # and query 300 peaks in the FIRST tile (alpha stays 1 afterwards)
    qk = to16(qk)
    vt = v.transpose(1, 2).contiguous()
    want = ref.attention(qk[:, :, :C].float(), qk[:, :, C:].float(), vt.float(), N, torch.empty(B, N, C), H)
    dqk = dev(qk)
    out = ops.attention(dqk[:, :, :C], dqk[:, :, C:], dev(vt), N, ops.empty((B, N, C)), H)
    torch.cuda.synchronize()
    assert attn2() == 1
    assert relmax(out, want) < 2 * BF16_TOL


def test_attention_v2_matches_v1(ops, attn2):
    """Same inputs through both kernels: identical algorithm, only the fp32 summation order of P.V differs."""
    from instancediffusion_amd import _lib
    B, H, d, N = 1, 8, 40, 1024
    C = H * d
    q, k, v = to16(gen((B, N, C), 50)), to16(gen((B, N, C), 51)), to16(gen((B, N, C), 52))
    vt = v.transpose(1, 2).contiguous()
    o2 = ops.attention(dev(q), dev(k), dev(vt), N, ops.empty((B, N, C)), H)
    torch.cuda.synchronize()
    assert attn2() == 1
    mode = _lib.load().idf_set_tuning(1, 0)
    o1 = ops.attention(dev(q), dev(k), dev(vt), N, ops.empty((B, N, C)), H)
    torch.cuda.synchronize()
    _lib.load().idf_set_tuning(1, mode)
    assert attn2() == 1
    assert relmax(o2, o1) < BF16_TOL


# ---------------------------------------------------------------------------------------------------
# LayerNorm folded into the GEMM epilogue (IDF_EPI_LN_ROW / IDF_EPI_LN_COL) + row statistics
# ---------------------------------------------------------------------------------------------------
def _fold(w, gamma, beta, bias=None):
    """engine._fold_ln: (16-bit gamma-folded weight, its row sums c, d = W beta + bias)."""
    w16 = to16(w * gamma[None, :])
    return w16, w16.float().sum(1), w @ beta + (bias if bias is not None else 0.0)


@pytest.mark.parametrize("M,C", [(4096, 320), (1000, 640), (77, 1280), (5, 64)])
def test_row_stats(ops, M, C):
    x = to16(gen((M, C), 80) * 2 + 0.7)
    st = ops.row_stats(dev(x), ops.empty((M, 2), torch.float32), 1e-5)
    torch.cuda.synchronize()
    xf = x.float()
    assert torch.allclose(st[:, 0].cpu(), xf.mean(-1), rtol=1e-5, atol=1e-5)
    assert torch.allclose(st[:, 1].cpu(), torch.rsqrt(xf.var(-1, unbiased=False) + 1e-5), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("M,N,K,mode", [
    (65536, 640, 320, "row"), (65536, 320, 320, "row"), (300, 640, 320, "row"), (4096, 1280, 640, "row"),      # big / fallback
    (65536, 2560, 320, "geglu"), (200, 2560, 320, "geglu"),
    (320, 65536, 320, "col"), (320, 200, 320, "col"), (640, 4096, 640, "col")])
def test_gemm_layernorm_folded(ops, M, N, K, mode):
    """out = LN(x) W^T computed as rstd * (x (gamma W)^T - mu c) + d in the GEMM epilogue (attention.py:294-295,320-322),
    against the fp32 reference LayerNorm -> Linear on the same 16-bit x; the explicit LN -> 16-bit -> GEMM path the engine
    used before is one 16-bit rounding WORSE than this, so the old kernel tolerance applies unchanged."""
    import torch.nn.functional as F
    from instancediffusion_amd.engine import pack_geglu
    gamma, beta = 1 + 0.2 * gen((K,), 81), 0.3 * gen((K,), 82)
    if mode == "col":                                   # the normalised operand is the N-side one (tokens), A = weight
        xw = to16(gen((N, K), 83) * 1.5 + 0.4)
        wa = gen((M, K), 84, K ** -0.5)
        w16, c, d = _fold(wa, gamma, beta)
        st = ops.row_stats(dev(xw), ops.empty((N, 2), torch.float32), 1e-5)
        out = ops.gemm(dev(w16), dev(xw), ops.empty((M, N)), ln_col=(st, dev(c), dev(d)))
        want = (F.layer_norm(xw.float(), (K,), gamma, beta, 1e-5) @ wa.t()).t()
    else:
        x = to16(gen((M, K), 83) * 1.5 + 0.4)
        w, b = gen((N, K), 84, K ** -0.5), 0.2 * gen((N,), 85)
        st = ops.row_stats(dev(x), ops.empty((M, 2), torch.float32), 1e-5)
        ln = F.layer_norm(x.float(), (K,), gamma, beta, 1e-5)
        if mode == "geglu":
            wp, dp = pack_geglu(w * gamma[None, :], b + w @ beta)
            w16 = to16(wp)
            out = ops.gemm(dev(x), dev(w16), ops.empty((M, N // 2)), bias=dev(dp), geglu=True, ln_row=(st, dev(w16.float().sum(1))))
            h = ln @ w.t() + b
            want = h[:, :N // 2] * F.gelu(h[:, N // 2:])
        else:
            w16, c, d = _fold(w, gamma, beta, b)
            out = ops.gemm(dev(x), dev(w16), ops.empty((M, N)), bias=dev(d), ln_row=(st, dev(c)))
            want = ln @ w.t() + b
    torch.cuda.synchronize()
    err, mx = rel_rms(out, want), relmax(out, want)
    print(f"[parity] gemm LN-folded {mode} M{M} N{N} K{K}: rel-rms {err:.3e} max-rel {mx:.3e}")
    assert mx < BF16_TOL and err < BF16_TOL / 2


@pytest.mark.parametrize("M,N,K,geglu", [(65536, 640, 320, False), (65536 + 77, 320, 320, False), (16384, 1280, 640, False),
                                         (4096, 1280, 1280, False), (65536, 2560, 320, True), (16384, 5120, 640, True),
                                         (300, 640, 320, False), (200, 2560, 320, True), (1000, 192, 64, False)])
def test_gemm_layernorm_self_stats(ops, M, N, K, geglu):
    """LN_ROW without statistics: the persistent kernel sums its A rows in the K loop (v_dot2c on the fragments it
    multiplies), the small-tile path runs the statistics pass first.  Against the fp32 LayerNorm -> Linear reference, with a
    row offset (|mean| ~ 2 x std) so that E[x^2] - mu^2 is exercised; the emitted statistics are checked too."""
    import torch.nn.functional as F
    from instancediffusion_amd.engine import pack_geglu
    gamma, beta = 1 + 0.2 * gen((K,), 91), 0.3 * gen((K,), 92)
    x = to16(gen((M, K), 93) * 1.5 + 3.0 * gen((M, 1), 94))
    w, b = gen((N, K), 95, K ** -0.5), 0.2 * gen((N,), 96)
    ln = F.layer_norm(x.float(), (K,), gamma, beta, 1e-5)
    st = ops.empty((M, 2), torch.float32)
    if geglu:
        wp, dp = pack_geglu(w * gamma[None, :], b + w @ beta)
        w16 = to16(wp)
        out = ops.gemm(dev(x), dev(w16), ops.empty((M, N // 2)), bias=dev(dp), geglu=True, ln_row=(None, dev(w16.float().sum(1))),
                       ln_stats_out=st)
        h = ln @ w.t() + b
        want = h[:, :N // 2] * F.gelu(h[:, N // 2:])
    else:
        w16, c, d = _fold(w, gamma, beta, b)
        out = ops.gemm(dev(x), dev(w16), ops.empty((M, N)), bias=dev(d), ln_row=(None, dev(c)), ln_stats_out=st)
        want = ln @ w.t() + b
    torch.cuda.synchronize()
    err, mx = rel_rms(out, want), relmax(out, want)
    xf = x.float()
    mu_err = float((st[:, 0].cpu() - xf.mean(-1)).abs().max())
    rs_rel = float((st[:, 1].cpu() / torch.rsqrt(xf.var(-1, unbiased=False) + 1e-5) - 1).abs().max())
    print(f"[parity] gemm LN self-stats M{M} N{N} K{K} geglu={geglu}: rel-rms {err:.3e} max-rel {mx:.3e}; "
          f"mu abs err {mu_err:.2e}, rstd rel err {rs_rel:.2e}")
    assert mx < BF16_TOL and err < BF16_TOL / 2
    assert mu_err < 1e-4 and rs_rel < 1e-4


@pytest.mark.parametrize("M,C,stats", [(65536, 320, "given"), (65536, 320, "self"), (16384, 640, "given"), (4096, 1280, "none"),
                                       (200, 320, "given"), (1000, 320, "self")])
def test_gemm_geglu_period32(ops, M, C, stats):
    """IDF_EPI_GEGLU_P32: weight rows interleaved [16 value | 16 gate] per 32, value and gate of an output in ONE MFMA fragment,
    so the GEGLU GEMMs (N = 8C: 2560 / 5120 / 10240, all multiples of 320) run on the 320-wide persistent tiles.  Against the
    fp32 reference, and BIT FOR BIT against the period-64 packing of the same weights (same K order per output element, same
    epilogue arithmetic); small M exercises the 128x128 kernels' form of the same epilogue."""
    import torch.nn.functional as F
    from instancediffusion_amd.engine import pack_geglu
    K, N = C, 8 * C
    gamma, beta = 1 + 0.2 * gen((K,), 181), 0.3 * gen((K,), 182)
    x = to16(gen((M, K), 183) * 1.5 + 0.5 * gen((M, 1), 184))
    w, b = gen((N, K), 185, K ** -0.5), 0.2 * gen((N,), 186)
    outs = {}
    for period in (32, 64):
        if stats == "none":
            wp, bp = pack_geglu(to16(w).float(), b, period)
            outs[period] = ops.gemm(dev(x), dev(to16(wp)), ops.empty((M, N // 2)), bias=dev(bp), geglu=True, geglu_period=period)
            want_h = x.float() @ to16(w).float().t() + b
        else:
            wp, dp = pack_geglu(w * gamma[None, :], b + w @ beta, period)
            w16 = to16(wp)
            st = ops.empty((M, 2), torch.float32)
            if stats == "given":
                ops.row_stats(dev(x), st, 1e-5)
            outs[period] = ops.gemm(dev(x), dev(w16), ops.empty((M, N // 2)), bias=dev(dp), geglu=True, geglu_period=period,
                                    ln_row=(st if stats == "given" else None, dev(w16.float().sum(1))),
                                    ln_stats_out=st if stats == "self" else None)
            want_h = F.layer_norm(x.float(), (K,), gamma, beta, 1e-5) @ w.t() + b
    torch.cuda.synchronize()
    want = want_h[:, :N // 2] * F.gelu(want_h[:, N // 2:])
    err, mx = rel_rms(outs[32], want), relmax(outs[32], want)
    print(f"[parity] GEGLU period 32 M{M} C{C} stats={stats}: rel-rms {err:.3e} max-rel {mx:.3e}; equal to period 64: "
          f"{torch.equal(outs[32], outs[64])}")
    assert mx < BF16_TOL and err < BF16_TOL / 2
    assert torch.equal(outs[32], outs[64])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M,gated,inplace", [(128, False, False), (4096, True, True), (65536 + 128, True, False), (524288, False, True)])
def test_gemm_fused_mlp(M, gated, inplace, dtype):
    """idf_mlp_geglu (mlp_fused.hip): LayerNorm -> GEGLU projection -> Linear -> [gated] residual of a C = 320 transformer block
    in ONE launch (attention.py:36-63, call sites :309 / :337), against the fp32 chain LN -> Linear -> value * gelu(gate) ->
    Linear -> x + gate * (...), and against the two idf_gemm calls it replaces (same operands, same rounding of the
    intermediate to the 16-bit type: equal up to the fp32 summation order of the second product).  M = 128: one tile, 127
    workgroups idle; 65664: a tile count that is not a multiple of the CU count; 524288: the 128-row forward, in place
    (out aliases x, as the engine calls it).  The error is measured on the MLP's contribution out - x as well: next to the
    residual it is small, and a relative error of the sum would hide it."""
    import torch.nn.functional as F
    from instancediffusion_amd.engine import pack_geglu
    from instancediffusion_amd.ops import HipOps
    ops = HipOps(dtype)
    C, Hd = 320, 1280
    gamma, beta = 1 + 0.2 * gen((C,), 301), 0.3 * gen((C,), 302)
    w1, b1 = gen((2 * Hd, C), 303, C ** -0.5), 0.2 * gen((2 * Hd,), 304)
    w2, b2 = gen((C, Hd), 305, Hd ** -0.5), 0.2 * gen((C,), 306)
    rows = min(M, 8192)                                           # distinct rows; tiled over M (the reference is per row)
    x = (gen((rows, C), 307) * 1.5 + 0.5 * gen((rows, 1), 308)).to(dtype)
    x = x.repeat(M // rows + 1, 1)[:M].contiguous()
    gate = torch.tensor([0.6], dtype=torch.float32) if gated else None
    wp, dp = pack_geglu(w1 * gamma[None, :], b1 + w1 @ beta, 32)
    w1_16, w2_16 = wp.to(dtype).cuda(), w2.to(dtype).cuda()
    c1 = w1_16.float().sum(1).contiguous()
    cd, w2p = ops.mlp_pack(w1_16, c1, dp.cuda(), w2_16)
    xd = x.cuda()
    st = ops.empty((M, 2), torch.float32)
    ops.row_stats(xd, st, 1e-5)
    # the two-GEMM path
    mid = ops.gemm(xd, w1_16, ops.empty((M, Hd)), bias=dp.cuda(), geglu=True, geglu_period=32, ln_row=(st, c1))
    two = ops.gemm(mid, w2_16, ops.empty((M, C)), bias=b2.cuda(), res=xd, gate=None if gate is None else gate.cuda())
    del mid
    # fused (in place: on a copy of x, so that `xd` stays the reference input)
    xin = xd.clone() if inplace else xd
    out = xin if inplace else ops.empty((M, C))
    ops.mlp_geglu(xin, st, w1_16, cd, w2p, b2.cuda(), out, gate=None if gate is None else gate.cuda())
    torch.cuda.synchronize()
    # fp32 reference on the GPU (plain torch), distinct rows only
    xr = xd[:rows].float()
    h = F.layer_norm(xr, (C,), gamma.cuda(), beta.cuda(), 1e-5) @ w1.cuda().t() + b1.cuda()
    mlp = (h[:, :Hd] * F.gelu(h[:, Hd:])) @ w2.cuda().t() + b2.cuda()
    want = xr + (0.6 if gated else 1.0) * mlp
    tol = {torch.bfloat16: (BF16_TOL, BF16_RMS_TOL, 1.5e-2), torch.float16: (2.0 ** -10, 4e-4, 2e-3)}[dtype]
    err, mx = rel_rms(out[:rows], want), relmax(out[:rows], want)
    err_mlp = rel_rms(out[:rows].float() - xr, want - xr)
    err_two = rel_rms(two[:rows].float() - xr, want - xr)
    same = rel_rms(out, two)
    print(f"[parity] fused MLP M{M} {dtype} gate={gated} inplace={inplace}: out rel-rms {err:.3e} max-rel {mx:.3e}; MLP term alone "
          f"{err_mlp:.3e} (two-GEMM path {err_two:.3e}); fused vs two-GEMM output {same:.3e}")
    assert mx < tol[0] and err < tol[1]
    assert err_mlp < tol[2] and err_mlp < 1.25 * err_two + 1e-4
    assert same < tol[1] / 4
    if M > rows:                                                  # every copy of a row gives the same bits, whatever tile / CU ran it
        assert torch.equal(out[:rows], out[rows:2 * rows]) and torch.equal(out[:128], out[M - (M % rows or rows):][:128])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M,gated", [(128, True), (65536 + 128, False), (524288, True)])
def test_gemm_fused_mlp_stream_kernel_is_bit_identical(M, gated, dtype):
    """mlp320w_kernel (one generated instruction stream per SIMD, the default of idf_mlp_geglu since round 6) computes the same sums in
    the same order as mlp320_kernel (IDF_TUNE_MLP = 0): the two outputs must agree BIT FOR BIT, in place as the engine calls it --
    which also keeps the rounds 4-5 kernel under test."""
    from instancediffusion_amd import _lib
    from instancediffusion_amd.engine import pack_geglu
    from instancediffusion_amd.ops import HipOps
    ops = HipOps(dtype)
    lib = _lib.load()
    C, Hd = 320, 1280
    gamma, beta = 1 + 0.2 * gen((C,), 601), 0.3 * gen((C,), 602)
    w1, b1 = gen((2 * Hd, C), 603, C ** -0.5), 0.2 * gen((2 * Hd,), 604)
    w2, b2 = gen((C, Hd), 605, Hd ** -0.5), 0.2 * gen((C,), 606)
    rows = min(M, 8192)
    x = (gen((rows, C), 607) * 1.5 + 0.5 * gen((rows, 1), 608)).to(dtype)
    x = x.repeat(M // rows + 1, 1)[:M].contiguous().cuda()
    gate = torch.tensor([0.6], dtype=torch.float32).cuda() if gated else None
    wp, dp = pack_geglu(w1 * gamma[None, :], b1 + w1 @ beta, 32)
    w1_16, w2_16 = wp.to(dtype).cuda(), w2.to(dtype).cuda()
    c1 = w1_16.float().sum(1).contiguous()
    cd, w2p = ops.mlp_pack(w1_16, c1, dp.cuda(), w2_16)
    st = ops.empty((M, 2), torch.float32)
    ops.row_stats(x, st, 1e-5)
    outs = {}
    for mode in (0, 1):
        prev = lib.idf_set_tuning(_lib.IDF_TUNE_MLP, mode)
        xin = x.clone()
        ops.mlp_geglu(xin, st, w1_16, cd, w2p, b2.cuda(), xin, gate=gate)
        torch.cuda.synchronize()
        lib.idf_set_tuning(_lib.IDF_TUNE_MLP, prev)
        outs[mode] = xin
    assert torch.isfinite(outs[1].float()).all() and not torch.equal(outs[1], x)
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("ratio", [10.0, 100.0])
def test_gemm_layernorm_self_stats_large_mean_bound(ops, ratio):
    """the in-loop row sums of the persistent kernel are single-pass (sum x, sum x^2 by v_dot2c, fp32), so a row
    with |mean| / std = r loses about r^2 * 2^-24 * sqrt(K) of its variance to cancellation -- gfx950 has no packed bf16
    subtract to shift the operands first.  Stated bound, checked here against the exact two-pass idf_row_stats: rstd relative
    error <= 2e-6 * r^2 (r = 10: 2e-4, r = 100: 2e-2; LayerNorm inputs of this model have r < 10).  The engine only uses the
    in-loop sums at C = 320 (LN_SELF mode 1); idf_row_stats / the epilogue partials (shifted, Chan-merged) have no such term."""
    M, N, K = 65536, 640, 320
    x = to16(gen((M, K), 93) + ratio)
    w16 = to16(gen((N, K), 95, K ** -0.5))
    st_self, st_exact = ops.empty((M, 2), torch.float32), ops.empty((M, 2), torch.float32)
    ops.gemm(dev(x), dev(w16), ops.empty((M, N)), bias=dev(gen((N,), 96)), ln_row=(None, dev(w16.float().sum(1))), ln_stats_out=st_self)
    ops.row_stats(dev(x), st_exact, 1e-5)
    torch.cuda.synchronize()
    rs = float((st_self[:, 1] / st_exact[:, 1] - 1).abs().max())
    mu = float((st_self[:, 0] - st_exact[:, 0]).abs().max())
    print(f"[bound] in-loop LayerNorm sums at |mean|/std = {ratio:g}: rstd rel err {rs:.2e} (bound {2e-6 * ratio ** 2:.1e}), mu abs err {mu:.2e}")
    assert rs <= 2e-6 * ratio ** 2 and mu < 1e-4 * ratio


def test_gemm_layernorm_self_stats_f16():
    """The fp16 instantiation of the in-loop row sums (v_dot2c_f32_f16) on the persistent kernel."""
    import torch.nn.functional as F
    from instancediffusion_amd.ops import HipOps
    o16 = HipOps(torch.float16)
    M, N, K = 65536, 640, 320
    gamma, beta = 1 + 0.2 * gen((K,), 91), 0.3 * gen((K,), 92)
    x = (gen((M, K), 93) * 1.5 + 3.0 * gen((M, 1), 94)).half()
    w, b = gen((N, K), 95, K ** -0.5), 0.2 * gen((N,), 96)
    w16 = (w * gamma[None, :]).half()
    c, d = w16.float().sum(1), w @ beta + b
    st = o16.empty((M, 2), torch.float32)
    out = o16.gemm(dev(x), dev(w16), o16.empty((M, N)), bias=dev(d), ln_row=(None, dev(c)), ln_stats_out=st)
    torch.cuda.synchronize()
    want = F.layer_norm(x.float(), (K,), gamma, beta, 1e-5) @ w.t() + b
    xf = x.float()
    mu_err = float((st[:, 0].cpu() - xf.mean(-1)).abs().max())
    rs_rel = float((st[:, 1].cpu() / torch.rsqrt(xf.var(-1, unbiased=False) + 1e-5) - 1).abs().max())
    err, mx = rel_rms(out, want), relmax(out, want)
    print(f"[parity] gemm LN self-stats fp16 M{M} N{N} K{K}: rel-rms {err:.3e} max-rel {mx:.3e}; mu abs err {mu_err:.2e}, "
          f"rstd rel err {rs_rel:.2e}")
    assert mx < 2.0 ** -9 and err < 2.0 ** -10
    assert mu_err < 1e-4 and rs_rel < 1e-4


@pytest.mark.parametrize("M,C,own", [(65536, 320, True), (65536, 320, False), (16384, 640, False), (8192, 320, True),
                                     (8192 + 16, 320, True), (2048, 640, False), (1000, 320, True)])
def test_gemm_fused_qkv_transposed_v(ops, M, C, own):
    """Fused q | k | v projection (engine._self_attn): out = LN(x) [Wq; Wk]^T row-major, vt_out = (LN(x) Wv^T)^T -- one
    launch of the persistent kernel whose V tiles run with swapped MFMA operands (big shapes; counted), the two GEMMs it
    replaces otherwise (small M, M % 16 != 0).  LayerNorm folded in, statistics from the K loop (own) or handed in.
    Against fp32 LayerNorm -> Linear, and bit-for-bit against the two-GEMM form on exact (integer) data."""
    import torch.nn.functional as F
    from instancediffusion_amd import _lib
    lib = _lib.load()
    K = C
    gamma, beta = 1 + 0.2 * gen((K,), 101), 0.3 * gen((K,), 102)
    x = to16(gen((M, K), 103) * 1.5 + 0.8 * gen((M, 1), 104))
    w = gen((3 * C, K), 105, K ** -0.5)
    w16, c, d = _fold(w, gamma, beta)
    ln = F.layer_norm(x.float(), (K,), gamma, beta, 1e-5)
    want = ln @ w.t()
    st = ops.empty((M, 2), torch.float32)
    if not own:
        ops.row_stats(dev(x), st, 1e-5)
    qk, vt = ops.empty((M, 2 * C)), ops.empty((C, M))
    start = lib.idf_get_stat(0)
    ops.gemm(dev(x), dev(w16), qk, bias=dev(d), ln_row=(None if own else st, dev(c)), ln_stats_out=st if own else None, vt_out=vt)
    torch.cuda.synchronize()
    served = lib.idf_get_stat(0) - start
    e_qk, e_v = rel_rms(qk, want[:, :2 * C]), rel_rms(vt.t(), want[:, 2 * C:])
    print(f"[parity] fused q|k|v M{M} C{C} own-stats={own}: q|k rel-rms {e_qk:.3e}, V^T rel-rms {e_v:.3e}; "
          f"{served} persistent-kernel launch(es)")
    assert relmax(qk, want[:, :2 * C]) < BF16_TOL and e_qk < BF16_TOL / 2
    assert relmax(vt.t(), want[:, 2 * C:]) < BF16_TOL and e_v < BF16_TOL / 2
    if M >= 16384 and M % 16 == 0:
        assert served == 1, "the bench-sized fused projection must be ONE launch of the persistent kernel"
    if own:
        xf = x.float()
        assert float((st[:, 0].cpu() - xf.mean(-1)).abs().max()) < 1e-4
    # exact data, identity LayerNorm fold ((mu, rstd) = (0, 1), c = d = 0: the epilogue the fused form requires, arithmetic-free):
    # the transposed tiles must equal the plain product bit for bit
    g = torch.Generator().manual_seed(106)
    ai = torch.randint(-3, 4, (M, K), generator=g).to(torch.bfloat16)
    wi = torch.randint(-3, 4, (3 * C, K), generator=g).to(torch.bfloat16)
    qk2, vt2 = ops.empty((M, 2 * C)), ops.empty((C, M))
    st0 = torch.tensor([0.0, 1.0]).repeat(M, 1).cuda()
    zero = torch.zeros(3 * C, device="cuda")
    ops.gemm(dev(ai), dev(wi), qk2, bias=zero, ln_row=(st0, zero), vt_out=vt2)
    torch.cuda.synchronize()
    exact = (ai.float() @ wi.float().t()).to(torch.bfloat16)
    assert torch.equal(qk2.cpu(), exact[:, :2 * C]) and torch.equal(vt2.cpu(), exact[:, 2 * C:].t())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M", [65536, 131072 + 128 * 5])
def test_gemm_geglu_row_kernel(M, dtype):
    """geglu_fused.hip: the GEGLU projection of the C = 640 level (K = 640, N = 5120, period-32 packing, LayerNorm folded, statistics
    handed in) on the row-resident kernel (idf_gemm takes it from two 128-row tiles per CU up).  Against fp32 LN -> Linear ->
    value * gelu(gate), against the persistent kernel on the same operands (the K sum runs as two partial sums and the fold is
    fma-contracted: a small fraction of the outputs may differ by an ulp), every copy of a row bitwise equal whatever tile / wave
    computed it, launch counted."""
    import torch.nn.functional as F
    from instancediffusion_amd import _lib
    from instancediffusion_amd.engine import pack_geglu
    from instancediffusion_amd.ops import HipOps
    ops = HipOps(dtype)
    lib = _lib.load()
    C, N = 640, 5120
    gamma, beta = 1 + 0.2 * gen((C,), 501), 0.3 * gen((C,), 502)
    rows = 2048
    x = (gen((rows, C), 503) * 1.5 + 0.8 * gen((rows, 1), 504)).to(dtype)
    x = x.repeat(M // rows + 1, 1)[:M].contiguous().cuda()
    w, b = gen((N, C), 505, C ** -0.5), 0.2 * gen((N,), 506)
    wp, dp = pack_geglu(w * gamma[None, :], b + w @ beta, 32)
    w16 = wp.to(dtype).cuda()
    c, d = w16.float().sum(1).contiguous(), dp.cuda()
    st = ops.empty((M, 2), torch.float32)
    ops.row_stats(x, st, 1e-5)
    h = F.layer_norm(x[:rows].float(), (C,), gamma.cuda(), beta.cuda(), 1e-5) @ w.cuda().t() + b.cuda()
    want = h[:, :N // 2] * F.gelu(h[:, N // 2:])
    outs = {}
    for mode in (1, 0):
        prev = lib.idf_set_tuning(_lib.IDF_TUNE_GEGLU_ROW, mode)
        out = ops.empty((M, N // 2))
        n0 = lib.idf_get_stat(_lib.IDF_STAT_GEGLU_ROW_LAUNCHES)
        ops.gemm(x, w16, out, bias=d, geglu=True, geglu_period=32, ln_row=(st, c))
        torch.cuda.synchronize()
        served = lib.idf_get_stat(_lib.IDF_STAT_GEGLU_ROW_LAUNCHES) - n0
        lib.idf_set_tuning(_lib.IDF_TUNE_GEGLU_ROW, prev)
        assert served == mode
        outs[mode] = out
    out = outs[1]
    tol = {torch.bfloat16: (BF16_TOL, BF16_TOL / 2), torch.float16: (2.0 ** -9, 2.0 ** -10)}[dtype]
    err, mx = rel_rms(out[:rows], want), relmax(out[:rows], want)
    err0 = rel_rms(outs[0][:rows], want)
    both = rel_rms(out, outs[0])
    nd = float((out != outs[0]).float().mean())
    print(f"[parity] GEGLU row kernel M{M} {dtype}: rel-rms {err:.3e} (persistent kernel {err0:.3e}) max-rel {mx:.3e}; vs persistent kernel "
          f"rel-rms {both:.2e}, differing elements {nd:.2e}")
    assert mx < tol[0] and err < tol[1] and err < 1.05 * err0 + 1e-5
    assert both < 2e-4 and nd < 2e-2
    assert torch.equal(out[:rows], out[rows:2 * rows]) and torch.equal(out[:rows], out[M - (M % rows or rows) - rows:][:rows])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M,C", [(131072, 320), (262144 + 256 * 7, 320), (65536, 640), (131072 + 128 * 3, 640)])
def test_gemm_fused_qkv_row_kernel(M, C, dtype):
    """qkv_fused.hip / qkv640_fused.hip: the fused q | k | v projection of the C = 320 / C = 640 level on the row-resident kernels
    (idf_gemm with vt_out takes them from two 256- / 128-row tiles per CU up when the statistics are handed in).  Against fp32 LayerNorm -> Linear, against the persistent
    kernel on the same operands (the mean term of the fold rides the MFMAs as 16-bit hi + lo products: a fraction of the outputs may
    differ by one ulp, no more), every copy of a row bitwise equal whatever tile / wave / row group computed it, launch counted; and
    exact data with the identity fold ((mu, rstd) = (0, 1), c = d = 0) must equal the plain product bit for bit."""
    import torch.nn.functional as F
    from instancediffusion_amd import _lib
    from instancediffusion_amd.ops import HipOps
    ops = HipOps(dtype)
    lib = _lib.load()
    gamma, beta = 1 + 0.2 * gen((C,), 401), 0.3 * gen((C,), 402)
    rows = 4096
    x = (gen((rows, C), 403) * 1.5 + 0.8 * gen((rows, 1), 404)).to(dtype)
    x = x.repeat(M // rows + 1, 1)[:M].contiguous().cuda()
    w = gen((3 * C, C), 405, C ** -0.5)
    w16 = (w * gamma[None, :]).to(dtype)
    c, d = w16.float().sum(1).cuda(), (w @ beta).cuda()
    w16 = w16.cuda()
    st = ops.empty((M, 2), torch.float32)
    ops.row_stats(x, st, 1e-5)
    want = F.layer_norm(x[:rows].float(), (C,), gamma.cuda(), beta.cuda(), 1e-5) @ w.cuda().t()
    outs = {}
    for mode in (1, 0):
        prev = lib.idf_set_tuning(_lib.IDF_TUNE_QKV_ROW, mode)
        qk, vt = ops.empty((M, 2 * C)), ops.empty((C, M))
        n0 = lib.idf_get_stat(_lib.IDF_STAT_QKV_ROW_LAUNCHES)
        ops.gemm(x, w16, qk, bias=d, ln_row=(st, c), vt_out=vt)
        torch.cuda.synchronize()
        served = lib.idf_get_stat(_lib.IDF_STAT_QKV_ROW_LAUNCHES) - n0
        lib.idf_set_tuning(_lib.IDF_TUNE_QKV_ROW, prev)
        assert served == mode
        outs[mode] = (qk, vt)
    qk, vt = outs[1]
    tol = {torch.bfloat16: (BF16_TOL, BF16_TOL / 2), torch.float16: (2.0 ** -10, 2.0 ** -11)}[dtype]
    e_qk, e_v = rel_rms(qk[:rows], want[:, :2 * C]), rel_rms(vt[:, :rows].t(), want[:, 2 * C:])
    ulp = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}[dtype]
    scale = float(want.abs().max())
    dq = float((qk.float() - outs[0][0].float()).abs().max()) / scale
    dv = float((vt.float() - outs[0][1].float()).abs().max()) / scale
    nq = float((qk != outs[0][0]).float().mean())
    print(f"[parity] q|k|v row kernel M{M} {dtype}: q|k rel-rms {e_qk:.3e}, V^T rel-rms {e_v:.3e}; vs persistent kernel max diff / max "
          f"{dq:.2e} / {dv:.2e}, differing q|k elements {nq:.2e}")
    assert relmax(qk[:rows], want[:, :2 * C]) < tol[0] and e_qk < tol[1]
    assert relmax(vt[:, :rows].t(), want[:, 2 * C:]) < tol[0] and e_v < tol[1]
    assert dq <= ulp and dv <= ulp and nq < 1e-2
    assert torch.equal(qk[:rows], qk[rows:2 * rows]) and torch.equal(qk[:rows], qk[M - (M % rows or rows) - rows:][:rows])
    assert torch.equal(vt[:, :rows], vt[:, rows:2 * rows])
    # exact data
    g = torch.Generator().manual_seed(406)
    ai = torch.randint(-3, 4, (M, C), generator=g).to(dtype).cuda()
    wi = torch.randint(-3, 4, (3 * C, C), generator=g).to(dtype).cuda()
    st0 = torch.tensor([0.0, 1.0]).repeat(M, 1).cuda()
    zero = torch.zeros(3 * C, device="cuda")
    qk2, vt2 = ops.empty((M, 2 * C)), ops.empty((C, M))
    n0 = lib.idf_get_stat(_lib.IDF_STAT_QKV_ROW_LAUNCHES)
    ops.gemm(ai, wi, qk2, bias=zero, ln_row=(st0, zero), vt_out=vt2)
    torch.cuda.synchronize()
    assert lib.idf_get_stat(_lib.IDF_STAT_QKV_ROW_LAUNCHES) - n0 == 1
    exact = (ai.float() @ wi.float().t()).to(dtype)
    assert torch.equal(qk2, exact[:, :2 * C]) and torch.equal(vt2, exact[:, 2 * C:].t())


def test_gemm_fused_qkv_f16_and_argument_checks():
    from instancediffusion_amd import _lib
    from instancediffusion_amd.ops import HipOps
    o16 = HipOps(torch.float16)
    M, C = 32768, 320
    g = torch.Generator().manual_seed(107)
    ai = torch.randint(-3, 4, (M, C), generator=g).half()
    wi = torch.randint(-3, 4, (3 * C, C), generator=g).half()
    qk, vt = o16.empty((M, 2 * C)), o16.empty((C, M))
    st0 = torch.tensor([0.0, 1.0]).repeat(M, 1).cuda()           # identity LayerNorm fold: (mu, rstd) = (0, 1), c = d = 0
    zero = torch.zeros(3 * C, device="cuda")
    o16.gemm(dev(ai), dev(wi), qk, bias=zero, ln_row=(st0, zero), vt_out=vt)
    torch.cuda.synchronize()
    exact = (ai.float() @ wi.float().t()).half()
    assert torch.equal(qk.cpu(), exact[:, :2 * C]) and torch.equal(vt.cpu(), exact[:, 2 * C:].t())
    # epilogues the transposed tiles do not implement are refused, not silently dropped -- and so is a call without the
    # LayerNorm fold (its two-GEMM form could not carry the transposed columns' bias; include/idf.h)
    with pytest.raises(_lib.IdfError):
        o16.gemm(dev(ai), dev(wi), qk, bias=zero, ln_row=(st0, zero), vt_out=vt, act="silu")
    with pytest.raises(_lib.IdfError):
        o16.gemm(dev(ai), dev(wi), qk, bias=zero, ln_row=(st0, zero), vt_out=vt, res=qk)
    with pytest.raises(_lib.IdfError):
        o16.gemm(dev(ai), dev(wi), qk, vt_out=vt)
    with pytest.raises(_lib.IdfError):
        o16.gemm(dev(ai), dev(wi), qk, bias=zero, vt_out=vt)


@pytest.mark.parametrize("M,N,K,offset", [(65536, 320, 320, 0.0), (65536 + 48, 320, 320, 40.0), (32768, 640, 640, 0.0),
                                          (16384, 1280, 1280, 5.0), (65536, 512, 128, 0.0)])
def test_gemm_out_stats_from_the_epilogue(ops, M, N, K, offset):
    """Bench-sized producers: the persistent kernel leaves per-wave (mean, M2) partials of the rows it stores and a 16-B-per-row
    finalize pass merges them (2, 4, 8 slots per row at N = 320 / 640 / 1280; 256-wide tiles at N = 512) -- no pass re-reads
    the output.  The result must equal the exact two-pass statistics of the 16-bit output actually written, also for rows
    whose |mean| is hundreds of standard deviations (shifted accumulation + Chan merge: no E[x^2] - mu^2)."""
    from instancediffusion_amd import _lib
    lib = _lib.load()
    a, w, b = to16(gen((M, K), 86)), to16(gen((N, K), 87, K ** -0.5)), gen((N,), 88) + offset
    r = to16(gen((M, N), 89) * 0.1 + offset)
    st = ops.empty((M, 2), torch.float32)
    y = dev(r).clone()
    prev = lib.idf_set_tuning(0, 2)            # whenever the shape qualifies (M = 65584 is 257 tiles: the auto rule would decline)
    start = lib.idf_get_stat(0)
    ops.gemm(dev(a), dev(w), y, bias=dev(b), res=y, out_stats=st, out_stats_eps=1e-5)
    torch.cuda.synchronize()
    lib.idf_set_tuning(0, prev)
    assert lib.idf_get_stat(0) - start == 1, "bench-sized producer must run on the persistent kernel"
    yf = y.float().cpu()
    mu, rs = yf.double().mean(-1), torch.rsqrt(yf.double().var(-1, unbiased=False) + 1e-5)
    mu_err = float((st[:, 0].cpu().double() - mu).abs().max() / (mu.abs().max() + 1e-6))
    rs_err = float((st[:, 1].cpu().double() / rs - 1).abs().max())
    print(f"[parity] out_stats from the epilogue M{M} N{N} K{K} offset {offset}: mu rel err {mu_err:.2e}, rstd rel err {rs_err:.2e}")
    assert mu_err < 2e-6 and rs_err < 2e-4


def test_gemm_out_stats(ops):
    """The by-product (mu, rstd) of the OUTPUT rows equals the statistics of the 16-bit output actually written."""
    M, N, K = 4096, 320, 320
    a, w, b, r = to16(gen((M, K), 86)), to16(gen((N, K), 87, K ** -0.5)), gen((N,), 88), to16(gen((M, N), 89))
    st = ops.empty((M, 2), torch.float32)
    y = dev(r).clone()
    ops.gemm(dev(a), dev(w), y, bias=dev(b), res=y, out_stats=st, out_stats_eps=1e-5)
    torch.cuda.synchronize()
    yf = y.float().cpu()
    assert torch.allclose(st[:, 0].cpu(), yf.mean(-1), rtol=1e-5, atol=1e-5)
    assert torch.allclose(st[:, 1].cpu(), torch.rsqrt(yf.var(-1, unbiased=False) + 1e-5), rtol=1e-5, atol=1e-6)



@pytest.fixture(params=[(torch.bfloat16, 1), (torch.float16, 1), (torch.bfloat16, 4), (torch.float16, 4), (torch.bfloat16, 5), (torch.float16, 5)],
                ids=["bf16", "fp16", "bf16-v4w", "fp16-v4w", "bf16-v4w-2waves", "fp16-v4w-2waves"])
def attn4(request):
    """attention4.hip (mode 1) / attention4w.hip (modes 4, 5) forced through idf_set_tuning, in both storage types."""
    from instancediffusion_amd import _lib
    from instancediffusion_amd.ops import HipOps
    lib = _lib.load()
    dt, mode = request.param
    prev = lib.idf_set_tuning(1, mode)
    start = lib.idf_get_stat(1)
    yield HipOps(dt), dt, (lambda: lib.idf_get_stat(1) - start)
    lib.idf_set_tuning(1, prev)


@pytest.mark.parametrize("case", ["plain", "late-spike", "first-tile-spike", "overflow", "tail-only", "seg1-spike"])
def test_attention_v4_reference_value_paths(ref, attn4, case):
    """The max-free softmax of variant 4: the reference value m is fixed on the first tile and only raised when a packed P
    reaches 2.  Exercise (a) the common path, (b) a finite late spike (m raised from the packed P, O rescaled), (c) a spike
    in the first tile (later P underflow, never raised), (d) a spike that overflows P to inf (the workgroup redoes the
    block with the exact per-tile max), (e) n0 < 64 (the first tile is a tail tile) and (f) a spike inside the tail tile
    of segment 1.  Checked against the fp32 reference in rel-RMS AND relative to the output max."""
    ops, dt, count = attn4
    B, H, d, N, n1 = 2, 8, 40, 640, 184
    if case == "tail-only":
        N = 40
    C = H * d
    q, k, v = gen((B, N, C), 60), gen((B, N, C), 61), gen((B, N, C), 62)
    k1, v1 = gen((B, n1, C), 63), gen((B, n1, C), 64)
    if case == "late-spike":
        k[:, 500] = q[:, 7] * 4.0                       # ~ +36 in log2 units for query 7 at key 500 (8th tile)
    if case == "first-tile-spike":
        k[:, 3] = q[:, 300] * 6.0
    if case == "overflow":
        # ~ +360 in log2 units for query 9 (P = inf in bf16 and fp16) and, q.q' being ~N(0, 40), tens to hundreds for many other
        # queries: finite-but-huge P (2^20 .. 2^127 in bf16) next to inf in the same waves
        k[:, 450] = q[:, 9] * 40.0
    if case == "seg1-spike":
        k1[:, 180] = q[:, 11] * 5.0                     # inside the 56-key tail tile of the grounding segment
    q, k, v, k1, v1 = (t.to(dt) for t in (q, k, v, k1, v1))
    ld0 = (N + 63) // 64 * 64
    vt = torch.full((B, C, ld0), float("nan"), dtype=dt)
    vt[:, :, :N] = v.transpose(1, 2)
    vt1 = torch.full((B, C, 192), float("nan"), dtype=dt)
    vt1[:, :, :n1] = v1.transpose(1, 2)
    want = ref.attention(q.float(), k.float(), torch.nan_to_num(vt.float()), N, torch.empty(B, N, C), H,
                         k1=k1.float(), vt1=torch.nan_to_num(vt1.float()), n1=n1)
    out = ops.attention(dev(q), dev(k), dev(vt), N, ops.empty((B, N, C)), H, k1=dev(k1), vt1=dev(vt1), n1=n1)
    torch.cuda.synchronize()
    assert count() == 1
    assert torch.isfinite(out.float()).all()
    tol = BF16_TOL if dt == torch.bfloat16 else 2.0 ** -10
    err, mx = rel_rms(out, want), relmax(out, want)
    print(f"[parity] attention v4 {case} {dt}: rel-rms {err:.3e} max-rel {mx:.3e}")
    # "overflow": scores of +-100 .. 360 log2 units.  Q enters the MFMA pre-multiplied by scale*log2(e) and rounded to the
    # 16-bit type once (as in variant 2's lazy mode and in torch's math SDPA), i.e. a score carries a relative error of up to
    # 2^-9 (bf16) / 2^-12 (fp16): +-0.5 / +-0.06 log2 units at |score| = 300.  For the handful of queries whose spike key
    # competes with another key within that margin the softmax weights shift by a few percent -- the worst element is
    # allowed 4x the usual bound there, the rel-RMS bound (which is what the UNet sees) stays.
    mx_tol = 8 * tol if case == "overflow" else 2 * tol
    assert mx < mx_tol and err < tol


# ---------------------------------------------------------------------------------------------------
# GroupNorm partial statistics out of the conv epilogue (round 5: idf_conv3x3 gn_partial + idf_groupnorm_apply)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("B,H,Cin,Cout,stride,extra,epi_path", [
    (8, 64, 320, 320, 1, "rowbias", True),        # ResBlock conv1 at 64^2: 128 tiles, 16 groups per wave column half
    (8, 64, 320, 320, 1, "rowbias_big", True),    # a time-embedding row bias ~100 x the conv output's std (the pivot of
                                                  # the epilogue's shifted sums must include it, or M2 cancels)
    (32, 32, 640, 640, 1, "res", True),           # conv2 + skip at 32^2: two n-tiles of 8 groups per wave column half
    (64, 16, 1280, 1280, 1, "rowbias", True),     # 16^2: one 256-row tile per sample, four n-tiles of 8 groups
    (64, 64, 320, 320, 2, None, True),            # Downsample (stride 2): 32^2 outputs
    (16, 32, 640, 640, 1, "res", False),          # 128 tiles of a long K: split-K launch -> the statistics pass fills the buffer
    (128, 8, 1280, 1280, 1, "res", False),        # 8^2: split-K launch -> the statistics pass fills the buffer
    (2, 16, 320, 320, 1, "rowbias", False)])      # small grid (latency kernel) -> statistics pass
def test_conv3x3_gn_partial(ref, dt, B, H, Cin, Cout, stride, extra, epi_path):
    """The conv leaves (mean, M2) per (sample, 64-row chunk, group) of the 16-bit output it stores.  Checked (a) against fp64
    statistics of that output, chunk by chunk, (b) GroupNorm from the partials == GroupNorm with its own statistics pass to
    fp32 summation order, (c) which path filled the buffer (launch counter), (d) the conv output itself is bit-identical to the
    call without gn_partial, (e) run-to-run bitwise determinism."""
    from instancediffusion_amd import _lib
    from instancediffusion_amd.engine import pack_conv3x3
    from instancediffusion_amd.ops import HipOps
    from tests.gemm_conv_cases import gn_partial_errors
    ops = HipOps(dt)
    lib = _lib.load()
    x = (gen((B, H, H, Cin), 120) * 0.5).to(dt)
    w = gen((Cout, Cin, 3, 3), 121, (9 * Cin) ** -0.5)
    wp = pack_conv3x3(w).to(dt)
    bias = gen((Cout,), 122) * 2.0 + 0.5                       # group means well away from 0
    Ho = (H - 1) // stride + 1
    kw = {}
    if extra == "rowbias":
        kw["rowbias"] = dev(gen((B, Cout), 123).to(dt))
    if extra == "rowbias_big":
        kw["rowbias"] = dev((gen((B, Cout), 123) * 50.0).to(dt))
    if extra == "res":
        kw["res"] = dev(gen((B, Ho, Ho, Cout), 124).to(dt))
    shape = ops.gn_partial_shape(B, Ho * Ho, Cout)
    assert shape == (B, Ho * Ho // 64, 32, 2)
    part = ops.empty(shape, torch.float32)
    part.fill_(float("nan"))
    c0 = lib.idf_get_stat(_lib.IDF_STAT_GN_EPI_LAUNCHES)
    out = ops.conv3x3(dev(x), dev(wp), ops.empty((B, Ho, Ho, Cout)), bias=dev(bias), stride=stride, gn_partial=part, **kw)
    torch.cuda.synchronize()
    assert (lib.idf_get_stat(_lib.IDF_STAT_GN_EPI_LAUNCHES) - c0 == 1) == epi_path
    plain = ops.conv3x3(dev(x), dev(wp), ops.empty((B, Ho, Ho, Cout)), bias=dev(bias), stride=stride, **kw)
    torch.cuda.synchronize()
    assert torch.equal(out, plain), "asking for the statistics must not change the conv output"
    assert torch.isfinite(part).all()
    # (a) fp64 statistics of the stored output
    mean_err, m2_err = gn_partial_errors(part, out)
    print(f"[parity] conv gn_partial B{B} {H}^2 {Cin}->{Cout} s{stride} {dt} epilogue={epi_path}: mean err {mean_err:.2e} std, M2 rel err {m2_err:.2e}")
    assert mean_err < 2e-5 and m2_err < 2e-4
    # (b) GroupNorm from the partials vs its own statistics pass
    gm, bt = dev(1 + 0.1 * gen((Cout,), 125)), dev(0.1 * gen((Cout,), 126))
    g1 = ops.groupnorm(out, ops.empty(tuple(out.shape)), gm, bt, 1e-5, True, partial=part)
    g2 = ops.groupnorm(out, ops.empty(tuple(out.shape)), gm, bt, 1e-5, True)
    torch.cuda.synchronize()
    assert relmax(g1, g2.float().cpu()) < 2.0 ** -7 and rel_rms(g1, g2.float().cpu()) < 5e-4
    # (e) determinism
    part2 = ops.empty(shape, torch.float32)
    ops.conv3x3(dev(x), dev(wp), ops.empty((B, Ho, Ho, Cout)), bias=dev(bias), stride=stride, gn_partial=part2, **kw)
    torch.cuda.synchronize()
    assert torch.equal(part, part2)


# ---------------------------------------------------------------------------------------------------
# the d = 80 / 160 LDS-DMA attention kernel (attention8.hip, round 5), forced through idf_set_tuning(IDF_TUNE_ATTN8)
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(params=[(1, torch.bfloat16), (1, torch.float16), (2, torch.bfloat16), (3, torch.bfloat16), (4, torch.bfloat16),
                        (5, torch.bfloat16), (6, torch.float16)],
                ids=["default-bf16", "default-fp16", "8waves", "plain-grid", "d160-4waves", "d80-4waves-pipelined",
                     "d80-8waves-pipelined-fp16"])
def attn8(request):
    """attention8.hip in its launch variants and both storage types; yields (ops, dtype, launch counter)."""
    from instancediffusion_amd import _lib
    from instancediffusion_amd.ops import HipOps
    lib = _lib.load()
    mode, dt = request.param
    prev = lib.idf_set_tuning(_lib.IDF_TUNE_ATTN8, mode)
    start = lib.idf_get_stat(_lib.IDF_STAT_ATTN8_LAUNCHES)
    yield HipOps(dt), dt, (lambda: lib.idf_get_stat(_lib.IDF_STAT_ATTN8_LAUNCHES) - start)
    lib.idf_set_tuning(_lib.IDF_TUNE_ATTN8, prev)


@pytest.mark.parametrize("B,H,d,Nq,n0,n1", [
    (2, 8, 80, 1024, 1024, 184), (1, 8, 80, 300, 304, 184), (2, 8, 160, 256, 256, 184), (1, 8, 160, 64, 64, 184),
    (1, 8, 160, 100, 104, 0), (2, 8, 80, 200, 72, 0), (1, 4, 80, 513, 520, 40), (3, 8, 160, 256, 256, 0), (1, 8, 80, 64, 8, 8)])
def test_attention_v8(ref, attn8, B, H, d, Nq, n0, n1):
    """Shapes of the 32^2 / 16^2 / 8^2 levels plus ragged query counts, key tails in either segment, a one-tile key set and
    an 8-key one; the V^T pads are NaN (they must never reach the output) and q / k are column slices of one buffer, as the
    engine passes them."""
    ops, dt, count = attn8
    C = H * d
    nk = max(Nq, n0)
    qk = gen((B, nk, 2 * C), 40).to(dt)
    v0 = gen((B, n0, C), 42).to(dt)
    ld0 = (n0 + 63) // 64 * 64
    vt0 = torch.full((B, C, ld0), float("nan"), dtype=dt)
    vt0[:, :, :n0] = v0.transpose(1, 2)
    q, k0 = qk[:, :Nq, :C], qk[:, :n0, C:]
    kw, rkw = {}, {}
    if n1:
        k1, v1 = gen((B, n1, C), 43).to(dt), gen((B, n1, C), 44).to(dt)
        vt1 = torch.full((B, C, 192), float("nan"), dtype=dt)
        vt1[:, :, :n1] = v1.transpose(1, 2)
        kw = dict(k1=dev(k1), vt1=dev(vt1), n1=n1)
        rkw = dict(k1=k1.float(), vt1=torch.nan_to_num(vt1.float()), n1=n1)
    want = ref.attention(q.float(), k0.float(), torch.nan_to_num(vt0.float()), n0, torch.empty(B, Nq, C), H, **rkw)
    dqk = dev(qk)
    out = ops.attention(dqk[:, :Nq, :C], dqk[:, :n0, C:], dev(vt0), n0, ops.empty((B, Nq, C)), H, **kw)
    torch.cuda.synchronize()
    assert count() == 1, "the launch must have gone to attention8.hip"
    assert torch.isfinite(out.float()).all()
    tol, rms_tol = (2 * BF16_TOL, 2 * BF16_RMS_TOL) if dt == torch.bfloat16 else (2.0 ** -9, 1e-3)
    err, mx = rel_rms(out, want), relmax(out, want)
    print(f"[parity] attention v8 d{d} Nq{Nq} keys {n0}+{n1} {dt}: rel-rms {err:.3e} max-rel {mx:.3e}")
    assert mx < tol and err < rms_tol


@pytest.mark.parametrize("case", ["late-spike", "first-tile-spike", "huge-spike", "seg1-spike", "creeping-max"])
@pytest.mark.parametrize("d", [80, 160])
def test_attention_v8_rescale_paths(ref, attn8, case, d):
    """The deferred rescale: O is rescaled (and the reference m raised) only when a tile maximum exceeds m by more than 2^6.
    (a) a late spike (many tiles at alpha == 1, then one big raise), (b) a spike in the first tile (every later P underflows),
    (c) a spike of hundreds of log2 units (no overflow with a running max: P <= 2^6 always), (d) a spike inside the tail tile of
    segment 1, (e) a maximum that creeps up by ~3 log2 units per tile (below the threshold most tiles: P grows up to 2^6 before
    a rescale -- the deferred path proper).  Against the fp32 reference, rel-RMS and relative to the output max."""
    ops, dt, count = attn8
    B, H, N, n1 = 2, 8, 640, 184
    C = H * d
    q, k, v = gen((B, N, C), 60), gen((B, N, C), 61), gen((B, N, C), 62)
    k1, v1 = gen((B, n1, C), 63), gen((B, n1, C), 64)
    if case == "late-spike":
        k[:, 500] = q[:, 7] * 4.0
    if case == "first-tile-spike":
        k[:, 3] = q[:, 300] * 6.0
    if case == "huge-spike":
        k[:, 450] = q[:, 9] * 40.0
    if case == "seg1-spike":
        k1[:, 180] = q[:, 11] * 5.0
    if case == "creeping-max":
        for t in range(10):                              # key 64 t + 5 scores ~ 3 (t + 1) log2 units for query 21
            k[:, 64 * t + 5] = q[:, 21] * (0.33 * (t + 1) * (80.0 / d) ** 0.5)
    q, k, v, k1, v1 = (t.to(dt) for t in (q, k, v, k1, v1))
    vt = torch.full((B, C, N), float("nan"), dtype=dt)
    vt[:, :, :N] = v.transpose(1, 2)
    vt1 = torch.full((B, C, 192), float("nan"), dtype=dt)
    vt1[:, :, :n1] = v1.transpose(1, 2)
    want = ref.attention(q.float(), k.float(), torch.nan_to_num(vt.float()), N, torch.empty(B, N, C), H,
                         k1=k1.float(), vt1=torch.nan_to_num(vt1.float()), n1=n1)
    out = ops.attention(dev(q), dev(k), dev(vt), N, ops.empty((B, N, C)), H, k1=dev(k1), vt1=dev(vt1), n1=n1)
    torch.cuda.synchronize()
    assert count() == 1
    assert torch.isfinite(out.float()).all()
    tol = BF16_TOL if dt == torch.bfloat16 else 2.0 ** -10
    err, mx = rel_rms(out, want), relmax(out, want)
    print(f"[parity] attention v8 d{d} {case} {dt}: rel-rms {err:.3e} max-rel {mx:.3e}")
    # "huge-spike": scores of hundreds of log2 units.  Q enters the MFMA pre-multiplied by scale*log2(e) and rounded to the 16-bit
    # type once (as in attention4.hip and in torch's math SDPA; the fma-scaled build variant, -DIDF_ATTN8_FMA_SCALE, passes the plain
    # bound here): a score carries a relative error of up to 2^-9 (bf16) / 2^-12 (fp16), i.e. +-0.7 / +-0.09 log2 units at
    # |score| = 360.  For the handful of queries whose spike key competes with another key within that margin the softmax weights
    # shift by a few per cent -- the worst element is allowed 4x the usual bound there (as in test_attention_v4_reference_value_paths'
    # "overflow" case), the rel-RMS bound (which is what the UNet sees) stays.
    mx_tol = 8 * tol if case == "huge-spike" else 2 * tol
    assert mx < mx_tol and err < tol


def test_attention_v8_matches_v1(attn8):
    """Same inputs through attention8.hip and the register-staged kernel of attention.hip: same algorithm, different summation
    order and rescale schedule."""
    from instancediffusion_amd import _lib
    ops, dt, count = attn8
    B, H, d, N = 2, 8, 80, 1024
    C = H * d
    q, k, v = gen((B, N, C), 50).to(dt), gen((B, N, C), 51).to(dt), gen((B, N, C), 52).to(dt)
    vt = v.transpose(1, 2).contiguous()
    o8 = ops.attention(dev(q), dev(k), dev(vt), N, ops.empty((B, N, C)), H)
    torch.cuda.synchronize()
    assert count() == 1
    mode = _lib.load().idf_set_tuning(_lib.IDF_TUNE_ATTN8, 0)
    o1 = ops.attention(dev(q), dev(k), dev(vt), N, ops.empty((B, N, C)), H)
    torch.cuda.synchronize()
    _lib.load().idf_set_tuning(_lib.IDF_TUNE_ATTN8, mode)
    assert count() == 1
    assert relmax(o8, o1) < (BF16_TOL if dt == torch.bfloat16 else 2.0 ** -10)


# ---------------------------------------------------------------------------------------------------
# full-size properties (BASELINE shapes: 64-row forward batch at the 64x64 latent): no oracle needed
# ---------------------------------------------------------------------------------------------------
FULL_B = 16          # rows of the property checks (the kernels see M = FULL_B * 4096 = 65536 token rows)


def test_full_size_gemm_identity_and_linearity(ops):
    """W = I reproduces A exactly (every output is ONE product), and GEMM(a1 + a2) == GEMM(a1) + GEMM(a2) on integer data."""
    M, C = FULL_B * 4096, 320
    g = torch.Generator().manual_seed(70)
    a = torch.randint(-8, 9, (M, C), generator=g).to(torch.bfloat16)
    eye = torch.eye(C).to(torch.bfloat16)
    out = ops.gemm(dev(a), dev(eye), ops.empty((M, C)))
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), a)
    w = torch.randint(-2, 3, (640, C), generator=g).to(torch.bfloat16)
    a2 = torch.randint(-8, 9, (M, C), generator=g).to(torch.bfloat16)
    o1 = ops.gemm(dev(a), dev(w), ops.empty((M, 640), torch.float32))
    o2 = ops.gemm(dev(a2), dev(w), ops.empty((M, 640), torch.float32))
    o12 = ops.gemm(dev(a + a2), dev(w), ops.empty((M, 640), torch.float32))
    torch.cuda.synchronize()
    assert torch.equal(o12, o1 + o2)


def test_full_size_conv3x3_taps_are_shifts(ops):
    """A 3x3 kernel that is 1 on one tap (identity over channels) shifts the image by that tap with zero padding -- exact."""
    from instancediffusion_amd.engine import pack_conv3x3
    B, H, C = FULL_B, 64, 320
    g = torch.Generator().manual_seed(71)
    x = torch.randint(-8, 9, (B, H, H, C), generator=g).to(torch.bfloat16)
    dx = dev(x)
    for (ky, kx) in [(1, 1), (0, 0), (2, 1), (1, 2)]:
        w4 = torch.zeros(C, C, 3, 3)
        w4[torch.arange(C), torch.arange(C), ky, kx] = 1.0
        out = ops.conv3x3(dx, dev(to16(pack_conv3x3(w4))), ops.empty((B, H, H, C)))
        torch.cuda.synchronize()
        want = torch.zeros_like(x)
        dy, dxx = ky - 1, kx - 1                           # out[y][x] = in[y + dy][x + dxx]
        ys, xs = slice(max(0, -dy), H - max(0, dy)), slice(max(0, -dxx), H - max(0, dxx))
        yd, xd = slice(max(0, dy), H - max(0, -dy)), slice(max(0, dxx), H - max(0, -dxx))
        want[:, ys, xs] = x[:, yd, xd]
        assert torch.equal(out.cpu(), want), (ky, kx)


def test_full_size_attention_rows_sum_to_one(ops):
    """V = 1 everywhere: every output element is sum_j softmax_j = 1, for the self- and the two-segment (gated) form."""
    B, H, d, N = 2, 8, 40, 4096
    C = H * d
    q, k = to16(gen((B, N, C), 72)), to16(gen((B, N, C), 73))
    vt = torch.ones(B, C, N, dtype=torch.bfloat16)
    out = ops.attention(dev(q), dev(k), dev(vt), N, ops.empty((B, N, C)), H)
    k1, vt1 = to16(gen((B, 184, C), 74)), torch.zeros(B, C, 192, dtype=torch.bfloat16)
    vt1[:, :, :184] = 1.0
    out2 = ops.attention(dev(q), dev(k), dev(vt), N, ops.empty((B, N, C)), H, k1=dev(k1), vt1=dev(vt1), n1=184)
    torch.cuda.synchronize()
    for o in (out, out2):
        assert float((o.float() - 1.0).abs().max()) <= 2.0 ** -7


def test_full_size_scaleu_identity_settings(ops):
    """hscale = 1 and sm1 = 0 make ScaleU a pure concat: bit-exact copy of both inputs."""
    B, H, C = FULL_B, 64, 320
    h, skip = to16(gen((B, H, H, C), 75)), to16(gen((B, H, H, C), 76))
    out = ops.scaleu_concat(dev(h), dev(skip), ops.empty((B, H, H, 2 * C)), dev(torch.ones(C)), dev(torch.zeros(1)))
    torch.cuda.synchronize()
    assert torch.equal(out[..., :C].cpu(), h) and torch.equal(out[..., C:].cpu(), skip)


def test_full_size_groupnorm_moments(ops):
    """gamma = 1, beta = 0, no SiLU: every (sample, group) of the output has mean 0 and variance 1."""
    B, HW, C = FULL_B, 4096, 320
    x = to16(gen((B, HW, C), 77) * 3.0 + 1.5)
    out = ops.groupnorm(dev(x), ops.empty((B, HW, C)), dev(torch.ones(C)), dev(torch.zeros(C)), 1e-5, False)
    torch.cuda.synchronize()
    o = out.float().view(B, HW, 32, C // 32).permute(0, 2, 1, 3).reshape(B, 32, -1)
    assert float(o.mean(-1).abs().max()) < 2e-3
    assert float((o.var(-1, unbiased=False) - 1.0).abs().max()) < 5e-3
