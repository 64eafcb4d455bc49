"""The CLIP text path on a real MI355X: ``idf_attention_causal``, ``idf_clip_embed`` and ``IDF_EPI_QUICKGELU`` against fp32 PyTorch
on the same 16-bit-rounded inputs, and ``CLIPTextEngine`` / ``FrozenCLIPEmbedder(backend="hip")`` end to end against the outputs of
the unmodified reference class (tests/golden/clip_engine_tiny.pt, tests/golden/clip_text.pt).

Kernel tolerances are those of tests/test_kernels_gpu.py (relative to the output max: one 16-bit ulp of the largest element, twice
that for attention, whose probabilities are rounded to 16 bits before P.V).  The end-to-end bar is 1.5 x the FLOOR stored with the
golden: the rel-RMS error of the same reference module cast to the 16-bit type against its own fp32 output.  The engine rounds at
the same places as that cast or at fewer (fp32 accumulation, softmax and LayerNorm statistics); the factor covers a different
rounding pattern (tests/test_engine_gpu.py uses 1.25 x floor for the same purpose on larger tensors).
"""
import ctypes as C

import pytest
import torch

from tests import clip_cases
from tests.clip_cases import rel_rms

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
ULP = {"bf16": 2.0 ** -7, "fp16": 2.0 ** -10}              # relmax of one rounding of the largest element
ATTN_RMS = {"bf16": 6e-3, "fp16": 6e-3 / 8}                # test_kernels_gpu.py's attention bar, scaled by the mantissa width
_OPS = {}


def ops_for(dt):
    if dt not in _OPS:
        from instancediffusion_amd.ops import HipOps
        _OPS[dt] = HipOps(DTYPES[dt])
    return _OPS[dt]


def gen(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def relmax(a, b):
    return float((a.float().cpu() - b.float().cpu()).abs().max() / b.float().abs().max().clamp_min(1e-20))


# ---- idf_attention_causal ------------------------------------------------------------------------------------------------
def run_attention(ops, qkv16, B, H, T, ld=None):
    """qkv16 [B*T, 3*H*64] 16-bit on the CPU -> output [B*T, H*64] 16-bit on the GPU; ``ld``: row stride of the device copy."""
    C3 = 3 * H * 64
    buf = torch.full((B * T, ld or C3), float("nan"), dtype=qkv16.dtype, device="cuda")
    buf[:, :C3] = qkv16.cuda()
    out = torch.full((B * T + 1, H * 64), float("nan"), dtype=qkv16.dtype, device="cuda")    # one guard row behind the output
    ops.attention_causal(buf[:, :C3], out[:B * T], H, T)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[B * T]).all()), "stored behind the last row"
    return out[:B * T]


@pytest.mark.parametrize("padded_ld", [False, True])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("B,H,T", [(1, 1, 1), (1, 1, 16), (1, 2, 17), (2, 3, 32), (1, 2, 33), (3, 12, 77), (1, 2, 128)])
def test_attention_causal(B, H, T, dt, padded_ld):
    ops = ops_for(dt)
    qkv = gen((B * T, 3 * H * 64), 100 + T).to(DTYPES[dt])
    out = run_attention(ops, qkv, B, H, T, ld=3 * H * 64 + 72 if padded_ld else None)
    want = clip_cases.causal_attention_ref(qkv, B, T, H)
    em, er = relmax(out, want), rel_rms(out, want)
    print(f"[parity] idf_attention_causal {dt} B={B} H={H} T={T}: relmax {em:.2e} rel-rms {er:.2e}")
    assert bool(torch.isfinite(out).all())
    assert em < 2 * ULP[dt] and er < ATTN_RMS[dt]


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_attention_causal_rows_do_not_see_later_positions(dt):
    """Changing q, k and v at positions > p leaves the output rows <= p bit-identical."""
    ops, B, H, T = ops_for(dt), 2, 2, 77
    qkv = gen((B * T, 3 * H * 64), 7).to(DTYPES[dt])
    base = run_attention(ops, qkv, B, H, T).cpu()
    for p in (0, 31, 32, 76):
        other = qkv.clone().view(B, T, -1)
        other[:, p + 1:] = (gen((B, T - p - 1, 3 * H * 64), 8 + p) * 3.0).to(DTYPES[dt])
        got = run_attention(ops, other.view(B * T, -1), B, H, T).cpu().view(B, T, -1)
        assert torch.equal(got[:, :p + 1], base.view(B, T, -1)[:, :p + 1]), p
        if p < T - 1:
            assert not torch.equal(got[:, p + 1:], base.view(B, T, -1)[:, p + 1:])


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_attention_causal_one_dominant_early_key_stays_finite(dt):
    """Key 3 leads every later query's score row by a logit gap of 60: the running maximum is set early and every later chunk
    underflows against it."""
    ops, H, T = ops_for(dt), 1, 77
    qkv = torch.zeros((T, 192))
    qkv[:, 0] = 1.0                                          # q . k_j = k_j[0]
    qkv[3, 64] = 60.0 * 8.0                                  # scale = 1/8: logit 60 at key 3, 0 elsewhere
    qkv[:, 128:] = gen((T, 64), 11)
    qkv = qkv.to(DTYPES[dt])
    out = run_attention(ops, qkv, 1, H, T)
    want = clip_cases.causal_attention_ref(qkv, 1, T, H)
    assert bool(torch.isfinite(out).all())
    assert relmax(out, want) < 2 * ULP[dt]
    assert torch.equal(out[40].cpu(), qkv[3, 128:])          # softmax is one-hot on key 3 to fp32 precision


def test_attention_causal_rejects_before_any_launch():
    ops = ops_for("bf16")
    lib, s = ops.lib, ops._stream()
    qkv, out = ops.zeros((130, 3 * 64 + 8)), ops.zeros((130, 64))
    call = lambda ld, T, H, d, qp=None: lib.idf_attention_causal(C.c_void_p(qp or qkv.data_ptr()), ld, C.c_void_p(out.data_ptr()),
                                                                 H * d, 1, T, H, d, 0.125, ops.dt, s)
    assert call(192, 77, 1, 64) == 0
    assert call(192, 129, 1, 64) == -3                        # IDF_E_UNSUPPORTED: T > 128
    assert call(120, 77, 1, 40) == -3                         # head dim 40
    assert call(196, 77, 1, 64) == -2                         # IDF_E_ALIGN: rows not 16-B aligned
    assert call(192, 77, 1, 64, qkv.data_ptr() + 2) == -2
    assert call(128, 77, 1, 64) == -1                         # IDF_E_ARG: ld < 3*H*d
    assert call(192, 0, 1, 64) == -1
    torch.cuda.synchronize()


# ---- idf_clip_embed --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_clip_embed(dt):
    ops, vocab, T, Cc = ops_for(dt), 300, 77, 136
    tok, pos = gen((vocab, Cc), 1).to(DTYPES[dt]), gen((T, Cc), 2).to(DTYPES[dt])
    ids = torch.randint(0, vocab, (3, T), generator=torch.Generator().manual_seed(3), dtype=torch.int32)
    ids[0, 0], ids[0, 1] = 0, vocab - 1
    ids[1, 5], ids[1, 6], ids[2, 76] = vocab, -4, 2 ** 31 - 1                      # out of range: clamped, never read outside
    out = torch.full((3 * T, Cc + 8), float("nan"), dtype=DTYPES[dt], device="cuda")
    ops.clip_embed(ids.cuda(), tok.cuda(), pos.cuda(), out[:, :Cc])
    torch.cuda.synchronize()
    want = (tok.float()[ids.long().clamp(0, vocab - 1)] + pos.float()[None]).to(DTYPES[dt]).view(3 * T, Cc)
    assert torch.equal(out[:, :Cc].cpu(), want)                                   # fp32 add, one rounding: exact
    assert bool(torch.isnan(out[:, Cc:]).all())


# ---- IDF_EPI_QUICKGELU -------------------------------------------------------------------------------------------------------
def _force_family(lib, family):
    """-> (previous knob values, counter to watch or None).  ``small``: the 128-wide-tile kernels (and their split-K reducer)."""
    from instancediffusion_amd import _lib
    big, ring = {"big": (2, 0), "ring": (0, 1 << 20), "small": (0, 0)}[family]
    prev = (lib.idf_set_tuning(_lib.IDF_TUNE_GEMM_BIG, big), lib.idf_set_tuning(_lib.IDF_TUNE_GEMM_RING, ring))
    return prev, {"big": _lib.IDF_STAT_GEMM_BIG_LAUNCHES, "ring": _lib.IDF_STAT_GEMM_RING_LAUNCHES}.get(family)


@pytest.mark.parametrize("family", ["big", "ring", "small"])
@pytest.mark.parametrize("ln", [False, True])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("M,N,K", [(77, 512, 128), (231, 3072, 768), (1000, 256, 64)])
def test_gemm_quick_gelu(M, N, K, dt, ln, family):
    from instancediffusion_amd import _lib
    ops = ops_for(dt)
    lib = ops.lib
    a, w, b = (gen((M, K), 1) + (0.5 if ln else 0.0)).to(DTYPES[dt]), gen((N, K), 2, K ** -0.5).to(DTYPES[dt]), gen((N,), 3)
    af = a.float()
    if ln:
        af = (af - af.mean(-1, keepdim=True)) * torch.rsqrt(af.var(-1, unbiased=False, keepdim=True) + 1e-5)
    y = af @ w.float().t() + b
    want = y * torch.sigmoid(1.702 * y)
    takes = family != "big" or K >= 128                      # the persistent kernel's K loop needs two K-tiles
    prev, stat = _force_family(lib, family)
    try:
        before = [lib.idf_get_stat(s) for s in (_lib.IDF_STAT_GEMM_BIG_LAUNCHES, _lib.IDF_STAT_GEMM_RING_LAUNCHES)]
        out = ops.gemm(a.cuda(), w.cuda(), ops.empty((M, N)), bias=b.cuda(), act="quick_gelu",
                       ln_row=(None, w.float().sum(1).cuda()) if ln else None)
        torch.cuda.synchronize()
        after = [lib.idf_get_stat(s) for s in (_lib.IDF_STAT_GEMM_BIG_LAUNCHES, _lib.IDF_STAT_GEMM_RING_LAUNCHES)]
    finally:
        lib.idf_set_tuning(_lib.IDF_TUNE_GEMM_BIG, prev[0])
        lib.idf_set_tuning(_lib.IDF_TUNE_GEMM_RING, prev[1])
    if family == "small":
        assert after == before
    elif takes:
        assert lib.idf_get_stat(stat) > before[0 if family == "big" else 1], f"{family} kernel did not take the launch"
    em = relmax(out, want)
    print(f"[parity] idf_gemm QUICKGELU {dt} {family} ln={ln} ({M}, {N}, {K}): relmax {em:.2e}")
    assert em < ULP[dt]


def test_quick_gelu_excludes_the_other_activations():
    from instancediffusion_amd import _lib
    ops = ops_for("bf16")
    a, w, out, b = ops.zeros((128, 64)), ops.zeros((128, 64)), ops.zeros((128, 128)), ops.zeros((128,), torch.float32)
    for other, want in ((_lib.EPI_SILU, -1), (_lib.EPI_GELU, -1), (_lib.EPI_GEGLU, -1), (0, 0)):
        args = _lib.GemmArgs(A=a.data_ptr(), W=w.data_ptr(), out=out.data_ptr(), bias=b.data_ptr(), M=128, N=128, K=64, lda=64, ldw=64,
                             ldo=128, batch=1, epi=_lib.EPI_BIAS | _lib.EPI_QUICKGELU | other, dtype=ops.dt)
        assert ops.lib.idf_gemm(C.byref(args), ops._stream()) == want, other
    x, wc, o4 = ops.zeros((1, 8, 8, 64)), ops.zeros((64, 576)), ops.zeros((1, 8, 8, 64))
    cargs = _lib.ConvArgs(x=x.data_ptr(), W=wc.data_ptr(), out=o4.data_ptr(), B=1, Hin=8, Win=8, Cin=64, Cout=64, stride=1, upsample=0,
                          ldx=64, ldo=64, epi=_lib.EPI_QUICKGELU, dtype=ops.dt)
    assert ops.lib.idf_conv3x3(C.byref(cargs), ops._stream()) == -1               # an idf_gemm flag
    torch.cuda.synchronize()


# ---- engine end to end ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def transformers_modules():
    pytest.importorskip("transformers")
    return {"tiny": clip_cases.tiny_transformer(), "clip_text": clip_cases.full_transformer()}


def _case(name):
    gold = clip_cases.load_golden("clip_engine_tiny" if name == "tiny" else "clip_text")
    return gold, clip_cases.load_golden("clip_engine_tiny")["floors"][name]


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("name", ["tiny", "clip_text"])
def test_engine_matches_reference_within_the_16_bit_floor(transformers_modules, name, dt):
    """Measured on an MI355X, last_hidden_state / pooler_output as multiples of the floor: tiny bf16 0.80 / 0.79, fp16 0.20 / 0.22;
    full size bf16 0.85 / 0.80, fp16 0.21 / 0.21 (absolute values in the README row of the CLIP text transformer)."""
    from instancediffusion_amd.clip_engine import CLIPTextEngine
    gold, floors = _case(name)
    eng = CLIPTextEngine(transformers_modules[name], ops=ops_for(dt))
    z, pooled = eng.encode_ids(gold["input_ids"])
    torch.cuda.synchronize()
    assert z.dtype == torch.float32 and pooled.dtype == torch.float32 and z.is_cuda
    assert tuple(z.shape) == tuple(gold["last_hidden_state"].shape) and tuple(pooled.shape) == tuple(gold["pooler_output"].shape)
    ez, ep = rel_rms(z, gold["last_hidden_state"]), rel_rms(pooled, gold["pooler_output"])
    fz, fp = floors[dt]["last_hidden_state"], floors[dt]["pooler_output"]
    print(f"[parity] CLIPTextEngine {name} {dt}: last_hidden_state rel-rms {ez:.3e} = {ez / fz:.2f} x floor {fz:.3e}; "
          f"pooler_output {ep:.3e} = {ep / fp:.2f} x floor {fp:.3e}")
    assert ez <= 1.5 * fz and ep <= 1.5 * fp


def test_engine_chunking_and_static_buffers(transformers_modules):
    from instancediffusion_amd.clip_engine import CLIPTextEngine
    gold, _ = _case("tiny")
    eng = CLIPTextEngine(transformers_modules["tiny"], ops=ops_for("bf16"))
    z64, p64 = eng.encode_ids(gold["input_ids"])
    ptrs = {k: v.data_ptr() for k, v in eng._bufs.items()}
    z64b, _ = eng.encode_ids(gold["input_ids"])
    assert {k: v.data_ptr() for k, v in eng._bufs.items()} == ptrs and torch.equal(z64, z64b)      # same B: same buffers
    eng.max_batch = 2                                        # B = 3 as chunks of 2 and 1 sequences
    z2, p2 = eng.encode_ids(gold["input_ids"])
    assert torch.equal(z2, z64) and torch.equal(p2, p64)
    for r, p in enumerate(clip_cases.TINY_EOS_POSITIONS):
        assert torch.equal(p64[r], z64[r, p])


def test_frozen_clip_embedder_hip_backend(transformers_modules):
    """The public switch: backend="hip" meets the engine's bar through ``encode``; backend="hf" on the same object is still the
    fp32 transformers path (1e-5 against the reference class)."""
    from instancediffusion_amd import synth
    from ldm.modules.encoders.modules import FrozenCLIPEmbedder
    gold, floors = _case("clip_text")
    enc = FrozenCLIPEmbedder(device="cuda", backend="hip")
    res = enc.load_state_dict(synth.synth_state_dict({k: tuple(v) for k, v in gold["schema"].items()}, gold["meta"]["salt"]), strict=False)
    assert not res.unexpected_keys
    enc = enc.to("cuda")
    ids = gold["input_ids"]

    class FixedTokenizer:
        def __call__(self, text, **kw):
            return {"input_ids": ids[:len(text)]}
    enc._tokenizer = FixedTokenizer()
    assert enc._engine is None                               # lazily created
    z, pooled = enc.encode(["a", "b"], return_pooler_output=True)
    assert enc._engine is not None and enc._engine.dtype == torch.bfloat16
    assert z.dtype == torch.float32 and z.is_cuda and tuple(z.shape) == (2, 77, 768) and tuple(pooled.shape) == (2, 768)
    assert torch.equal(enc(["a", "b"]), z)
    ez, ep = rel_rms(z, gold["last_hidden_state"]), rel_rms(pooled, gold["pooler_output"])
    print(f"[parity] FrozenCLIPEmbedder(backend='hip') bf16: last_hidden_state {ez:.3e}, pooler_output {ep:.3e}")
    assert ez <= 1.5 * floors["bf16"]["last_hidden_state"] and ep <= 1.5 * floors["bf16"]["pooler_output"]
    enc.backend = "hf"
    z, pooled = enc.encode(["a", "b"], return_pooler_output=True)
    assert rel_rms(z, gold["last_hidden_state"]) < 1e-5 and rel_rms(pooled, gold["pooler_output"]) < 1e-5
