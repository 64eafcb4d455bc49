"""VAE encoder (``AutoencoderKL.encode``), no GPU: the engine's host logic (weight packing, op order, Downsample, the posterior
tail, RNG-stream parity with the reference) through the CPU op emulation against goldens of the unmodified reference's
``encode`` (tests/make_vae_encode_golden.py), the emulation of the asymmetric-pad stride-2 conv, the argument validation of the
two new C-ABI entry points, and the decoder's op sequence after the engines came to share a base class."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests import cases
from tests import vae_encode_cases as vc


def _encode(tag, dtype, noise):
    from instancediffusion_amd.vae_engine import VAEEncoderEngine
    ae, x, gold = vc.build(tag)
    eng = VAEEncoderEngine(ae, ops=vc.EncEmulOps(dtype), use_graphs=False)
    with torch.no_grad():
        z, moments = eng.encode(x, noise(gold) if noise else None)
    return eng, z, moments, gold


def _reference_noise(gold):
    torch.manual_seed(vc.NOISE_SEED)
    E = gold["moments"].shape[1] // 2
    return torch.randn(gold["moments"][:, :E].shape)      # the reference's call (distributions.py:36): CPU default generator


@pytest.mark.parametrize("tag,dtype,tol", [("vae_enc_tiny", torch.float32, 3e-4), ("vae_enc_tiny", torch.bfloat16, 4e-2),
                                           ("vae_enc_full_128", torch.float32, 3e-4), ("vae_enc_full_128", torch.bfloat16, 4e-2),
                                           ("vae_enc_full_512", torch.float32, 3e-4), ("vae_enc_full_512", torch.bfloat16, 4e-2)])
def test_vae_encoder_engine_vs_reference(tag, dtype, tol):
    eng, z, moments, gold = _encode(tag, dtype, _reference_noise)
    e = vc.moment_errors(moments, gold["moments"])
    zerr = cases.rel_rms(z, gold["z"])
    print(f"[parity] emulated VAE encoder {tag} {dtype}: moments rel-rms {e['moments_rel_rms']:.3e}, logvar max-abs "
          f"{e['logvar_max_abs']:.3e} rms {e['logvar_rms']:.3e}, z rel-rms {zerr:.3e}; reference bf16-autocast floor {gold['floor']}")
    assert moments.shape == gold["moments"].shape and z.shape == gold["z"].shape
    assert e["moments_rel_rms"] < tol
    calls = eng.ops.calls
    assert calls["vae_posterior"] == 1 and calls["softmax_rows"] == 1 and calls["conv_in"] == 1
    if vc.CASES[tag]["variant"] == "full":
        assert calls["conv3x3_down"] == 3
        assert (calls["conv3x3"], calls["groupnorm"], calls["gemm"]) == (21, 22, 7)
        # 10 res blocks x 2 convs + conv_out; 10 x 2 norms + the attention's + norm_out; 2 shortcuts + the attention's 5 GEMMs
    else:
        assert calls["conv3x3_down"] == 2
    if dtype == torch.float32:
        # RNG-stream parity: torch.manual_seed + CPU randn gives the reference's sample to fp32 round-off
        assert zerr < 3e-4 and float((z - gold["z"]).abs().max()) < 2e-3 * float(gold["z"].abs().max())


def test_vae_encoder_mode_is_scaled_mean():
    eng, z, moments, gold = _encode("vae_enc_tiny", torch.float32, None)
    E = moments.shape[1] // 2
    assert torch.equal(z, moments[:, :E] * gold["scale_factor"])
    assert cases.rel_rms(z, gold["moments"][:, :E] * gold["scale_factor"]) < 3e-4


def test_fixture_logvar_never_reaches_the_clamp():
    """The goldens cannot show the clamp (the kernel test on synthetic moments does): say so where a reader looks for it."""
    for tag in vc.CASES:
        lo, hi = vc.load(tag)["logvar_range"]
        assert -30.0 < lo and hi < 20.0


def test_host_encode_draws_the_reference_noise_and_chunks():
    """``AutoencoderKL.encode`` itself (noise handling, chunking over max_encode_batch, return_moments) with an emulated engine."""
    from instancediffusion_amd.vae_engine import VAEEncoderEngine
    ae, x, gold = vc.build("vae_enc_tiny")
    ae._enc_engine = VAEEncoderEngine(ae, ops=vc.EncEmulOps(torch.float32), use_graphs=False)
    torch.manual_seed(vc.NOISE_SEED)
    z = ae.encode(x)
    assert cases.rel_rms(z, gold["z"]) < 3e-4
    ae.max_encode_batch = 1
    torch.manual_seed(vc.NOISE_SEED)
    z1, mean, logvar = ae.encode(x, return_moments=True)
    assert cases.rel_rms(z1, z) < 1e-5 and ae._enc_engine.ops.calls["vae_posterior"] == 3
    assert cases.rel_rms(torch.cat([mean, logvar], 1), gold["moments"]) < 3e-4
    zm = ae.encode(x, noise=False)
    assert cases.rel_rms(zm, mean * gold["scale_factor"]) < 1e-6
    with pytest.raises(ValueError, match="multiple of"):
        ae.encode(torch.zeros(1, 3, 100, 100))
    with pytest.raises(ValueError):
        ae.encode(x, noise=torch.zeros(1, 4, 8, 8))
    ae.load_state_dict(ae.state_dict())
    assert ae._enc_engine is None and ae._engine is None


def test_full_config_rejects_sizes_the_mid_attention_cannot_take():
    from instancediffusion_amd.vae_engine import VAEEncoderEngine
    ae = cases.build_vae(cases.vae_cfg_for("full"))
    eng = VAEEncoderEngine(ae, ops=vc.EncEmulOps(torch.float32), use_graphs=False)
    eng.check_size(512, 384)
    eng.check_size(64, 64)
    for hw in ((100, 100), (96, 96), (512, 100)):
        with pytest.raises(ValueError, match="multiple"):
            eng.check_size(*hw)


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(1, 16, 16, 64, 64), (2, 15, 23, 64, 128), (1, 30, 46, 128, 64), (1, 7, 8, 64, 64)])
def test_emulated_conv3x3_down(B, H, W, Cin, Cout):
    from instancediffusion_amd.engine import pack_conv3x3
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, Cin, H, W, generator=g)
    w4 = torch.randn(Cout, Cin, 3, 3, generator=g) * (9 * Cin) ** -0.5
    b = torch.randn(Cout, generator=g)
    want = F.conv2d(F.pad(x, (0, 1, 0, 1)), w4, b, stride=2)
    Ho, Wo = (H - 2) // 2 + 1, (W - 2) // 2 + 1
    assert want.shape == (B, Cout, Ho, Wo)
    ops = vc.EncEmulOps(torch.float32)
    out = ops.conv3x3_down(x.permute(0, 2, 3, 1).contiguous(), pack_conv3x3(w4), torch.empty(B, Ho, Wo, Cout), bias=b)
    assert float((out.permute(0, 3, 1, 2) - want).abs().max()) < 1e-5
    # and it is NOT the symmetric pad-1 stride-2 conv idf_conv3x3 computes
    sym = ops.conv3x3(x.permute(0, 2, 3, 1).contiguous(), pack_conv3x3(w4), torch.empty(B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cout),
                      bias=b, stride=2)
    assert sym.shape != out.shape or float((sym - out).abs().max()) > 1e-2


def test_new_entry_points_validate_without_gpu():
    """Both symbols are exported and prototyped, and argument errors come back as IDF_E_* before any launch (fake pointers)."""
    from instancediffusion_amd import _lib
    lib = _lib.load()
    for name in ("idf_conv3x3_down", "idf_vae_posterior"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    assert lib.idf_abi_version() == 5

    def conv_args(**kw):
        c = _lib.ConvArgs(x=0x10000, W=0x20000, out=0x30000, bias=0x40000, B=1, Hin=16, Win=16, Cin=128, Cout=128, stride=2,
                          upsample=0, ldx=128, ldo=128, epi=_lib.EPI_BIAS, dtype=0)
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    assert lib.idf_conv3x3_down(None, None) == -1
    assert lib.idf_conv3x3_down(ctypes.byref(_lib.ConvArgs()), None) == -1
    assert lib.idf_conv3x3_down(ctypes.byref(conv_args(stride=1)), None) == -1
    assert lib.idf_conv3x3_down(ctypes.byref(conv_args(upsample=1)), None) == -1
    assert lib.idf_conv3x3_down(ctypes.byref(conv_args(Hin=1)), None) == -1
    assert lib.idf_conv3x3_down(ctypes.byref(conv_args(Win=1)), None) == -1
    assert lib.idf_conv3x3_down(ctypes.byref(conv_args(x=None)), None) == -1
    assert lib.idf_conv3x3_down(ctypes.byref(conv_args(W=None)), None) == -1
    assert lib.idf_conv3x3_down(ctypes.byref(conv_args(out=None)), None) == -1
    assert lib.idf_conv3x3_down(ctypes.byref(conv_args(bias=None)), None) == -1           # BIAS without a bias
    assert lib.idf_conv3x3_down(ctypes.byref(conv_args(Cin=96, ldx=96)), None) == -1      # Cin % 64
    assert lib.idf_conv3x3_down(ctypes.byref(conv_args(ldx=132)), None) == -2             # 16-B rows
    # the gn_partial contract is idf_conv3x3's: 15 x 15 = 225 output rows are not whole 64-row chunks
    assert lib.idf_conv3x3_down(ctypes.byref(conv_args(Hin=30, Win=30, gn_partial=0x50000)), None) == -1

    def post(h=0x10000, w=0x20000, bias=0x30000, noise=0x40000, z=0x50000, moments=None, B=1, C2=8, E=4, HW=4096):
        return lib.idf_vae_posterior(h, w, bias, noise, 0.18215, z, moments, B, C2, E, HW, None)
    assert post(h=None) == -1 and post(w=None) == -1 and post(z=None) == -1
    assert post(C2=17) == -1 and post(E=9) == -1 and post(C2=0) == -1 and post(E=0) == -1
    assert post(HW=0) == -1 and post(HW=-4) == -1 and post(B=0) == -1


def test_decoder_engine_issues_the_same_ops_as_before_the_shared_base_class():
    """Counters of the decoder engine on vae_tiny / vae_full_16 as the commit before the refactor issued them."""
    from instancediffusion_amd.vae_engine import VAEDecoderEngine, VAEEncoderEngine, _VAEEngine
    assert issubclass(VAEDecoderEngine, _VAEEngine) and issubclass(VAEEncoderEngine, _VAEEngine)
    before = {"vae_tiny": {"pointwise_nchw": 1, "conv_in": 1, "groupnorm": 18, "conv3x3": 19, "gemm": 6, "softmax_rows": 1},
              "vae_full_16": {"pointwise_nchw": 1, "conv_in": 1, "groupnorm": 30, "conv3x3": 32, "gemm": 7, "softmax_rows": 1}}
    for tag, want in before.items():
        gold = cases.load_golden(tag)
        meta = gold["meta"]
        ae = cases.build_vae(cases.vae_cfg_for(meta["variant"]), meta["salt"])
        eng = VAEDecoderEngine(ae, ops=vc.EncEmulOps(torch.float32), use_graphs=False)
        with torch.no_grad():
            img = eng.decode(cases.vae_latent(meta))
        assert eng.ops.calls == want
        assert cases.rel_rms(img, gold["img"]) < 3e-4
