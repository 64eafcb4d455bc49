"""VAE encoder (``AutoencoderKL.encode``) on a real MI355X: the asymmetric-pad stride-2 conv on every kernel family that can
serve it and the posterior tail vs fp32 PyTorch, then ``encode`` end to end against goldens of the unmodified reference
(tests/make_vae_encode_golden.py).

Stated tolerance, the one of the decoder (tests/test_vae_gpu.py): bf16 storage / fp32 accumulate -> moments rel-RMS <= 3e-2,
fp16 <= 5e-3; kernels 2^-7 (bf16) / 2^-10 (fp16) of the output max.  The reference's own bf16-autocast error on these cases
(each fixture's ``floor``) is 1.3e-2 .. 1.8e-2 rel-RMS, so the bf16 bar leaves about 40 % of margin.  Second gate: the
logvar max-abs error stays within 2 x the fixture's floor (a maximum over up to 32K values under another rounding pattern is a
noisy statistic, hence the factor).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}
E2E_TOL = {torch.bfloat16: 3e-2, torch.float16: 5e-3}


def gen(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def relmax(a, b):
    return float((a.float().cpu() - b.float().cpu()).abs().max() / b.float().abs().max().clamp_min(1e-20))


# ---- idf_conv3x3_down, once per kernel family ----------------------------------------------------------------------
DOWN_SHAPES = [(1, 512, 512, 128), (1, 256, 256, 256), (1, 128, 128, 512), (2, 64, 64, 256), (1, 30, 46, 128), (2, 31, 17, 256)]
FAMILIES = {                      # name -> (IDF_TUNE_GEMM_BIG, IDF_TUNE_GEMM_RING, launch counter that must move, ... stay)
    "persistent": (2, 0, "big", "ring"),
    "small_tile": (0, 0, None, "big+ring"),
    "latency": (0, 1 << 30, "ring", "big"),
}


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_conv3x3_down_every_kernel_family(family, dtype):
    from instancediffusion_amd import _lib
    from instancediffusion_amd.engine import pack_conv3x3
    from instancediffusion_amd.ops import HipOps
    from tests import vae_encode_cases as vc
    ops = HipOps(dtype)
    ref = vc.EncEmulOps(torch.float32)
    lib = ops.lib
    big, ring, moves, _ = FAMILIES[family]

    def stats():
        return lib.idf_get_stat(_lib.IDF_STAT_GEMM_BIG_LAUNCHES), lib.idf_get_stat(_lib.IDF_STAT_GEMM_RING_LAUNCHES)
    prev_big = lib.idf_set_tuning(_lib.IDF_TUNE_GEMM_BIG, big)
    prev_ring = lib.idf_set_tuning(_lib.IDF_TUNE_GEMM_RING, ring)
    try:
        shapes = DOWN_SHAPES if dtype == torch.bfloat16 else DOWN_SHAPES[3:]
        for B, H, W, C in shapes:
            Ho, Wo = (H - 2) // 2 + 1, (W - 2) // 2 + 1
            x = gen((B, H, W, C), 1).to(dtype)
            w = pack_conv3x3(gen((C, C, 3, 3), 2, (9 * C) ** -0.5)).to(dtype)
            b = gen((C,), 3, 0.1)
            want = ref.conv3x3_down(x.float(), w.float(), torch.empty(B, Ho, Wo, C), bias=b)
            b0, r0 = stats()
            out = ops.conv3x3_down(x.cuda(), w.cuda(), ops.empty((B, Ho, Wo, C)), bias=b.cuda())
            torch.cuda.synchronize()
            b1, r1 = stats()
            err = relmax(out, want)
            print(f"[kernel] conv3x3_down {family} {dtype} B{B} {H}x{W} C{C}: max err {err:.3e} of max, "
                  f"persistent launches +{b1 - b0}, latency launches +{r1 - r0}")
            assert (b1 - b0, r1 - r0) == {"big": (1, 0), "ring": (0, 1), None: (0, 0)}[moves], (family, B, H, W, C)
            assert out.shape == want.shape and err < TOL[dtype]
        # with a residual, as every other conv epilogue
        B, H, W, C = 1, 64, 64, 256
        x = gen((B, H, W, C), 4).to(dtype)
        w = pack_conv3x3(gen((C, C, 3, 3), 5, (9 * C) ** -0.5)).to(dtype)
        res = gen((B, 32, 32, C), 6).to(dtype)
        want = ref.conv3x3_down(x.float(), w.float(), torch.empty(B, 32, 32, C), res=res.float())
        out = ops.conv3x3_down(x.cuda(), w.cuda(), ops.empty((B, 32, 32, C)), res=res.cuda())
        torch.cuda.synchronize()
        assert relmax(out, want) < TOL[dtype]
    finally:
        lib.idf_set_tuning(_lib.IDF_TUNE_GEMM_BIG, prev_big)
        lib.idf_set_tuning(_lib.IDF_TUNE_GEMM_RING, prev_ring)


def test_conv3x3_down_gn_partial_contract():
    """gn_partial is idf_conv3x3's contract: the partial statistics of the output, whichever kernel took the launch."""
    from instancediffusion_amd.engine import pack_conv3x3
    from instancediffusion_amd.ops import HipOps
    from tests import vae_encode_cases as vc
    ops = HipOps(torch.bfloat16)
    B, H, W, C = 2, 32, 32, 320
    x = gen((B, H, W, C), 1).to(torch.bfloat16)
    w = pack_conv3x3(gen((C, C, 3, 3), 2, (9 * C) ** -0.5)).to(torch.bfloat16)
    out = ops.empty((B, 16, 16, C))
    part = ops.empty(ops.gn_partial_shape(B, 256, C), torch.float32)
    ops.conv3x3_down(x.cuda(), w.cuda(), out, gn_partial=part)
    torch.cuda.synchronize()
    v = out.float().cpu().reshape(B, -1, 64, 32, C // 32).permute(0, 1, 3, 2, 4).reshape(B, 4, 32, -1)
    assert float((part.cpu()[..., 0] - v.mean(-1)).abs().max()) < 1e-4
    m2 = ((v - v.mean(-1, keepdim=True)) ** 2).sum(-1)
    assert float(((part.cpu()[..., 1] - m2).abs() / m2).max()) < 1e-3
    want = vc.EncEmulOps(torch.float32).conv3x3_down(x.float(), w.float(), torch.empty(B, 16, 16, C))
    assert relmax(out, want) < TOL[torch.bfloat16]


# ---- idf_vae_posterior ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C2,E,H,W", [(2, 8, 4, 64, 64), (1, 8, 4, 7, 9), (3, 16, 8, 16, 12), (1, 6, 3, 5, 4)])
@pytest.mark.parametrize("with_noise", [True, False])
@pytest.mark.parametrize("with_moments", [True, False])
def test_vae_posterior(B, C2, E, H, W, with_noise, with_moments):
    from instancediffusion_amd.ops import HipOps
    ops = HipOps(torch.bfloat16)
    assert C2 == 2 * E
    h = gen((B, C2, H, W), 1)
    # synthetic moments with logvar = -50, 0 and +40 at known pixels (clamp on both sides, exp stays finite).  The mean rows read
    # the first half of the input channels only and the logvar rows read the second half through an orthogonal block, so moving
    # one logvar output to its target moves nothing else and no large terms cancel in the fp32 dot products
    w = torch.zeros(2 * E, C2)
    w[:E, :E] = gen((E, E), 2, E ** -0.5)
    w[E:, :E] = gen((E, E), 5, 0.3 * E ** -0.5)
    q = torch.linalg.qr(gen((E, E), 6))[0]
    w[E:, E:] = q
    bias = gen((2 * E,), 3, 0.1)
    m0 = torch.einsum("oc,bchw->bohw", w, h) + bias.view(1, -1, 1, 1)
    for k, target in enumerate((-50.0, 0.0, 40.0)):
        y, xq, j = k % H, (k * 2 + 1) % W, k % E
        d = torch.zeros(E)
        d[j] = target - m0[0, E + j, y, xq]
        h[0, E:, y, xq] += q.t() @ d
    noise = gen((B, E, H, W), 4) if with_noise else None
    m = torch.einsum("oc,bchw->bohw", w.double(), h.double()) + bias.double().view(1, -1, 1, 1)
    mean, logvar = m[:, :E], m[:, E:].clamp(-30.0, 20.0)
    assert float(m[:, E:].min()) < -49 and float(m[:, E:].max()) > 39 and float(logvar.max()) == 20.0 and float(logvar.min()) == -30.0
    scale = 0.18215
    want = (mean + (torch.exp(0.5 * logvar) * noise.double() if with_noise else 0)) * scale
    z = ops.empty((B, E, H, W), torch.float32)
    mo = ops.empty((B, 2 * E, H, W), torch.float32) if with_moments else None
    ops.vae_posterior(h.cuda(), w.cuda(), bias.cuda(), None if noise is None else noise.cuda(), scale, z, mo)
    torch.cuda.synchronize()
    assert torch.isfinite(z).all()
    assert relmax(z, want) < 1e-5
    if with_moments:
        assert torch.isfinite(mo).all() and relmax(mo, torch.cat([mean, logvar], 1)) < 1e-5
        assert float(mo[:, E:].max()) <= 20.0 and float(mo[:, E:].min()) >= -30.0
    # a dense quant_conv matrix, no bias
    h2, w2 = gen((B, C2, H, W), 7), gen((2 * E, C2), 8, C2 ** -0.5)
    z2 = ops.vae_posterior(h2.cuda(), w2.cuda(), None, None, 1.0, ops.empty((B, E, H, W), torch.float32))
    assert relmax(z2, torch.einsum("oc,bchw->bohw", w2.double(), h2.double())[:, :E]) < 1e-5


# ---- end to end -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["vae_enc_tiny", "vae_enc_full_128", "vae_enc_full_512"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_vae_encode_matches_reference_golden(tag, dtype):
    from tests import cases
    from tests import vae_encode_cases as vc
    ae, x, gold = vc.build(tag)
    ae.compute_dtype = dtype
    torch.manual_seed(vc.NOISE_SEED)
    z, mean, logvar = ae.encode(x, return_moments=True)
    torch.manual_seed(vc.NOISE_SEED)
    z2 = ae.encode(x.cuda())
    assert z.is_cuda and z.dtype == torch.float32
    assert torch.equal(z, z2), "hipGraph replay must be bitwise identical to the eager warm-up"
    moments = torch.cat([mean, logvar], 1).cpu()
    e = vc.moment_errors(moments, gold["moments"])
    zerr = cases.rel_rms(z.cpu(), gold["z"])
    name = "bf16" if dtype == torch.bfloat16 else "fp16"
    print(f"[parity] VAE encode {tag} {name}: moments rel-rms {e['moments_rel_rms']:.3e}, logvar max-abs {e['logvar_max_abs']:.3e} "
          f"rms {e['logvar_rms']:.3e}, z rel-rms {zerr:.3e}; reference bf16-autocast floor: moments {gold['floor']['moments_rel_rms']:.3e}, "
          f"logvar max-abs {gold['floor']['logvar_max_abs']:.3e} rms {gold['floor']['logvar_rms']:.3e}")
    assert torch.isfinite(z).all() and moments.shape == gold["moments"].shape
    assert e["moments_rel_rms"] < E2E_TOL[dtype]
    assert e["logvar_max_abs"] <= 2 * gold["floor"]["logvar_max_abs"]
    assert zerr < E2E_TOL[dtype]
    zm = ae.encode(x, noise=False)
    assert torch.equal(zm, mean * gold["scale_factor"])


def test_vae_encode_full_size_properties():
    """512x512 images: batch entries independent, chunking over max_encode_batch transparent, a non-square size works and a
    size the mid attention cannot take is a ValueError."""
    from tests import cases
    from tests import vae_encode_cases as vc
    ae = cases.build_vae(cases.vae_cfg_for("full"))
    x = vc.encode_image(3, 512, 31)
    x[2] = x[0]
    noise = gen((3, 4, 64, 64), 32)
    noise[2] = noise[0]
    z = ae.encode(x, noise=noise)
    assert z.shape == (3, 4, 64, 64) and torch.isfinite(z).all()
    same = cases.rel_rms(z[2].cpu(), z[0].cpu())
    print(f"[property] latents 0 and 2 (same image): bitwise equal = {torch.equal(z[0], z[2])}, rel-rms {same:.1e}")
    assert (torch.equal(z[0], z[2]) or same < 1e-3) and not torch.equal(z[0], z[1])
    ae.max_encode_batch = 2
    z2 = ae.encode(x, noise=noise)
    # another batch size takes other tile schedules, i.e. another fp32 summation order -> 16-bit-level agreement
    assert cases.rel_rms(z2.cpu(), z.cpu()) < 1e-2
    zr = ae.encode(vc.encode_image(1, 512, 33, width=384))
    assert zr.shape == (1, 4, 64, 48) and torch.isfinite(zr).all()
    with pytest.raises(ValueError, match="multiple"):
        ae.encode(torch.zeros(1, 3, 100, 100))


def test_vae_round_trip_plumbing():
    """decode(encode(x, noise=False)) at full size: finite, the input's shape, and scale_factor applied once in each direction
    (the latent from ``encode`` and ``mean * scale_factor`` from ``return_moments`` decode to the same bits).  A plumbing check,
    not a quality claim: the weights are synthetic."""
    from tests import cases
    from tests import vae_encode_cases as vc
    ae = cases.build_vae(cases.vae_cfg_for("full"))
    x = vc.encode_image(1, 512, 41)
    z, mean, _ = ae.encode(x, noise=False, return_moments=True)
    img = ae.decode(z)
    assert img.shape == x.shape and torch.isfinite(img).all()
    assert torch.equal(img, ae.decode(mean * ae.scale_factor))
