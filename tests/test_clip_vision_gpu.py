"""The CLIP image tower and the local CLIP score on a real MI355X: ``idf_attention_qkv`` against fp32 PyTorch on the same
16-bit-rounded inputs, ``idf_clip_patchify`` against ``unfold``, ``CLIPVisionEngine`` / ``CLIPTextEngine.text_features`` against
``transformers`` in fp32, and ``InstanceClipScorer(backend="hip")`` against ``backend="hf"``.

Kernel bars are those of tests/test_clip_engine_gpu.py's causal attention test (relmax < 2 ulp of the type: the probabilities are
rounded to 16 bits before P.V; rel-RMS < 6e-3 scaled by the mantissa width).  The end-to-end bar is 1.5 x the FLOOR: the rel-RMS
of the same ``transformers`` module cast to the 16-bit type against its own fp32 output (computed live for the tiny config, stored
in tests/golden/clip_vision_full.pt for ViT-L/14), the factor tests/test_clip_engine_gpu.py uses, for the reason given there.
"""
import ctypes as C

import pytest
import torch

from tests import clip_cases
from tests import clip_vision_cases as vc
from tests.clip_cases import rel_rms

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
ULP = {"bf16": 2.0 ** -7, "fp16": 2.0 ** -10}
ATTN_RMS = {"bf16": 6e-3, "fp16": 6e-3 / 8}
TMAX = 288                                                   # IDF_ATTENTION_QKV_TMAX (include/idf.h)
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


# ---- idf_attention_qkv ---------------------------------------------------------------------------------------------------
def run_attention(ops, qkv16, B, H, T, ld=None):
    """qkv16 [B*T, 3*H*64] 16-bit on the CPU -> output [B*T, H*64] 16-bit on the GPU.  NaN behind everything the kernel may touch:
    the pad columns of a padded ``ld``, 32 rows behind ``qkv`` (a pad key read from memory instead of the zero fill poisons the
    softmax), one guard row behind the output."""
    C3 = 3 * H * 64
    buf = torch.full((B * T + 32, ld or C3), float("nan"), dtype=qkv16.dtype, device="cuda")
    buf[:B * T, :C3] = qkv16.cuda()
    out = torch.full((B * T + 1, H * 64), float("nan"), dtype=qkv16.dtype, device="cuda")
    ops.attention_qkv(buf[:B * T, :C3], out[:B * T], H, T)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[B * T]).all()), "stored behind the last row"
    return out[:B * T]


def test_tmax_is_the_header_value():
    assert ops_for("bf16").ATTENTION_QKV_TMAX == TMAX >= 257


@pytest.mark.parametrize("padded_ld", [False, True])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("B,H,T", [(1, 1, 1), (1, 2, 16), (1, 2, 17), (2, 3, 50), (1, 2, 128), (1, 2, 129), (2, 2, 197), (2, 16, 257),
                                   (1, 1, TMAX)])
def test_attention_qkv(B, H, T, dt, padded_ld):
    ops = ops_for(dt)
    qkv = gen((B * T, 3 * H * 64), 100 + T).to(DTYPES[dt])
    out = run_attention(ops, qkv, B, H, T, ld=3 * H * 64 + 72 if padded_ld else None)
    want = vc.full_attention_ref(qkv, B, T, H)
    em, er = relmax(out, want), rel_rms(out, want)
    print(f"[parity] idf_attention_qkv {dt} B={B} H={H} T={T}: relmax {em:.2e} rel-rms {er:.2e}")
    assert bool(torch.isfinite(out).all())
    assert em < 2 * ULP[dt] and er < ATTN_RMS[dt]


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_attention_qkv_is_bidirectional(dt):
    """Changing k and v at the LAST position changes output row 0 (a causal kernel would not), and the result still meets the bar."""
    ops, B, H, T = ops_for(dt), 1, 2, 257
    qkv = gen((B * T, 3 * H * 64), 21).to(DTYPES[dt])
    base = run_attention(ops, qkv, B, H, T).cpu()
    other = qkv.clone()
    other[T - 1, H * 64:] = (gen((2 * H * 64,), 22) * 2.0).to(DTYPES[dt])
    got = run_attention(ops, other, B, H, T)
    assert not torch.equal(got[0].cpu(), base[0])
    want = vc.full_attention_ref(other, B, T, H)
    assert relmax(got, want) < 2 * ULP[dt] and rel_rms(got, want) < ATTN_RMS[dt]


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_attention_qkv_sequences_do_not_interact(dt):
    ops, B, H, T = ops_for(dt), 2, 2, 50
    qkv = gen((B * T, 3 * H * 64), 23).to(DTYPES[dt])
    base = run_attention(ops, qkv, B, H, T).cpu()
    other = qkv.clone()
    other[T:] = (gen((T, 3 * H * 64), 24) * 3.0).to(DTYPES[dt])
    got = run_attention(ops, other, B, H, T).cpu()
    assert torch.equal(got[:T], base[:T]) and not torch.equal(got[T:], base[T:])


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_attention_qkv_late_dominant_key(dt):
    """The key at T - 1 = 256 -- alone in the last 32-key chunk -- leads every score row by a logit gap of 60: the running maximum
    is set by the last chunk and everything accumulated before is rescaled by exp(-60)."""
    ops, H, T = ops_for(dt), 1, 257
    qkv = torch.zeros((T, 192))
    qkv[:, 0] = 1.0                                          # q . k_j = k_j[0]
    qkv[T - 1, 64] = 60.0 * 8.0                              # scale = 1/8: logit 60 at the last key, 0 elsewhere
    qkv[:, 128:] = gen((T, 64), 11)
    qkv = qkv.to(DTYPES[dt])
    out = run_attention(ops, qkv, 1, H, T)
    want = vc.full_attention_ref(qkv, 1, T, H)
    assert bool(torch.isfinite(out).all())
    assert relmax(out, want) < 2 * ULP[dt]
    assert torch.equal(out[40].cpu(), qkv[T - 1, 128:])      # softmax is one-hot on the last key to fp32 precision


def test_attention_qkv_rejects_before_any_launch():
    ops = ops_for("bf16")
    lib, s = ops.lib, ops._stream()
    qkv, out = ops.zeros((TMAX + 2, 3 * 64 + 8)), ops.zeros((TMAX + 2, 64))
    call = lambda ld, T, H, d, qp=None: lib.idf_attention_qkv(C.c_void_p(qp or qkv.data_ptr()), ld, C.c_void_p(out.data_ptr()),
                                                              H * d, 1, T, H, d, 0.125, ops.dt, s)
    assert call(192, 257, 1, 64) == 0
    assert call(192, TMAX + 1, 1, 64) == -3                   # IDF_E_UNSUPPORTED: T > TMAX
    assert call(120, 77, 1, 40) == -3                         # head dim 40
    assert call(196, 77, 1, 64) == -2                         # IDF_E_ALIGN: rows not 16-B aligned
    assert call(192, 77, 1, 64, qkv.data_ptr() + 2) == -2
    assert call(128, 77, 1, 64) == -1                         # IDF_E_ARG: ld < 3*H*d
    assert call(192, 0, 1, 64) == -1
    torch.cuda.synchronize()


# ---- idf_clip_patchify -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("B,S,P", [(1, 28, 14), (2, 32, 16), (1, 64, 32), (2, 224, 14)])
def test_clip_patchify(B, S, P, dt):
    ops, Cc = ops_for(dt), 136
    G, k = S // P, 3 * P * P
    Kp, T = (k + 63) // 64 * 64, G * G + 1
    px = gen((B, 3, S, S), 30 + S)
    cls = gen((Cc,), 31).to(DTYPES[dt])
    patch = torch.full((B * G * G + 1, Kp), float("nan"), dtype=DTYPES[dt], device="cuda")       # one guard row
    x = torch.full((B * T + 1, Cc), float("nan"), dtype=DTYPES[dt], device="cuda")
    ops.clip_patchify(px.cuda(), patch[:B * G * G], cls.cuda(), x[:B * T], P)
    torch.cuda.synchronize()
    got = patch.cpu()
    assert torch.equal(got[:B * G * G, :k], vc.patchify_ref(px, P).to(DTYPES[dt]))               # one rounding, no arithmetic
    assert bool((got[:B * G * G, k:] == 0).all()) and bool(torch.isnan(got[B * G * G]).all())
    xc = x.cpu().view(-1, Cc)
    for b in range(B):
        assert torch.equal(xc[b * T], cls)
    rest = torch.ones(B * T + 1, dtype=torch.bool)
    rest[0:B * T:T] = False
    assert bool(torch.isnan(xc[rest]).all())                                                     # nothing but the class rows


def test_clip_patchify_rejects():
    ops = ops_for("bf16")
    px, patch, cls, x = ops.zeros((1, 3, 30, 30), torch.float32), ops.zeros((4, 640)), ops.zeros((128,)), ops.zeros((5, 128))
    call = lambda S, P: ops.lib.idf_clip_patchify(C.c_void_p(px.data_ptr()), C.c_void_p(patch.data_ptr()), 640, C.c_void_p(cls.data_ptr()),
                                                  C.c_void_p(x.data_ptr()), 128, 1, S, P, 128, ops.dt, ops._stream())
    assert call(28, 14) == 0
    assert call(30, 14) == -1                                 # IDF_E_ARG: S % P
    torch.cuda.synchronize()


# ---- engines end to end ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_case():
    pytest.importorskip("transformers")
    model, px = vc.tiny_vision(), vc.pixel_values(3, vc.TINY_VISION["image_size"])
    ref, floors = vc.with_floors(model, lambda m: vc.vision_reference(m, px))
    return model, px, ref, floors


def _check(tag, got, ref, floors):
    ok = True
    for name, g in zip(vc.OUTPUTS, got):
        e, f = rel_rms(g, ref[name]), floors[name]
        print(f"[parity] {tag}: {name} rel-rms {e:.3e} = {e / f:.2f} x floor {f:.3e}")
        ok = ok and e <= 1.5 * f
    return ok


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_vision_engine_tiny_within_the_16_bit_floor(tiny_case, dt):
    from instancediffusion_amd.clip_engine import CLIPVisionEngine
    model, px, ref, floors = tiny_case
    eng = CLIPVisionEngine(model, ops=ops_for(dt))
    got = eng.encode_pixels(px)
    torch.cuda.synchronize()
    assert all(g.dtype == torch.float32 and g.is_cuda for g in got)
    assert tuple(got[0].shape) == (3, 17, 128) and tuple(got[1].shape) == (3, 128) and tuple(got[2].shape) == (3, 64)
    assert _check(f"CLIPVisionEngine tiny {dt}", got, ref, floors[dt])


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_vision_engine_full_size_within_the_16_bit_floor(dt):
    pytest.importorskip("transformers")
    from instancediffusion_amd.clip_engine import CLIPVisionEngine
    gold = vc.load_golden("clip_vision_full")
    assert gold["meta"]["config"] == vc.FULL_VISION and gold["meta"]["salt"] == vc.FULL_SALT
    eng = CLIPVisionEngine(vc.full_vision(), ops=ops_for(dt))
    z, pooled, embeds = eng.encode_pixels(vc.pixel_values(gold["meta"]["batch"], vc.FULL_VISION["image_size"]))
    torch.cuda.synchronize()
    assert tuple(z.shape) == (2, 257, 1024) and bool(torch.isfinite(z).all())
    ref = dict(last_hidden_state=gold["last_hidden_state_rows"], pooler_output=gold["pooler_output"], image_embeds=gold["image_embeds"])
    assert _check(f"CLIPVisionEngine ViT-L/14 {dt}", (z[:, gold["meta"]["rows"]], pooled, embeds), ref, gold["floors"][dt])


def test_vision_engine_chunking(tiny_case):
    """B = max_batch + 1: the second chunk holds one image.  Its rows equal the unchunked ones to the engine's own bar (another
    row count may select another GEMM kernel: same values up to fp32 summation order), and the buffers are static."""
    from instancediffusion_amd.clip_engine import CLIPVisionEngine
    model, px, ref, floors = tiny_case
    eng = CLIPVisionEngine(model, ops=ops_for("bf16"))
    whole = eng.encode_pixels(px)
    eng.max_batch = 2                                        # B = 3 = max_batch + 1
    parts = eng.encode_pixels(px)
    ptrs = {k: v.data_ptr() for k, v in eng._bufs.items()}
    again = eng.encode_pixels(px)
    assert {k: v.data_ptr() for k, v in eng._bufs.items()} == ptrs and all(torch.equal(a, b) for a, b in zip(parts, again))
    assert _check("CLIPVisionEngine tiny bf16, chunks of 2 + 1", parts, ref, floors["bf16"])
    for name, a, b in zip(vc.OUTPUTS, parts, whole):
        assert rel_rms(a, b) <= 1.5 * floors["bf16"][name], name


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("name", ["tiny", "clip_text"])
def test_text_features_within_the_16_bit_floor(name, dt):
    pytest.importorskip("transformers")
    from instancediffusion_amd.clip_engine import CLIPTextEngine
    if name == "tiny":
        model, ids = vc.tiny_clip_model(), clip_cases.tiny_input_ids()
        ref, floors = vc.with_floors(model, lambda m: dict(t=vc.features(m.get_text_features(input_ids=ids)).float()))
        want, floor = ref["t"], floors[dt]["t"]
    else:
        gold = vc.load_golden("clip_vision_full")
        model, ids = vc.full_text_clip_model(), clip_cases.load_golden("clip_text")["input_ids"]
        want, floor = gold["text_features"], gold["text_floors"][dt]
    eng = CLIPTextEngine(model.text_model, ops=ops_for(dt), text_projection=model.text_projection)
    got = eng.text_features(ids)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape)
    e = rel_rms(got, want)
    print(f"[parity] CLIPTextEngine.text_features {name} {dt}: rel-rms {e:.3e} = {e / floor:.2f} x floor {floor:.3e}")
    assert e <= 1.5 * floor


# ---- scorer --------------------------------------------------------------------------------------------------------------------
def test_scorer_hip_backend_against_hf():
    """Crop, preprocess, normalise and dot, not the kernels again: with e = the relative L2 error of the un-normalised hip features
    against hf, |cos(a', b') - cos(a, b)| <= |a'/|a'| - a/|a|| + |b'/|b'| - b/|b|| <= 2 (e_img + e_txt) (normalising a vector
    perturbed by e |a| moves it by at most 2 e)."""
    pytest.importorskip("transformers")
    from PIL import Image
    from instancediffusion_amd.host.clip_score import InstanceClipScorer, crop_instances, hash_tokenize, preprocess
    model = vc.tiny_clip_model()
    arr = torch.randint(0, 256, (120, 160, 3), generator=torch.Generator().manual_seed(9), dtype=torch.uint8).numpy()
    image = Image.fromarray(arr)                             # 160 x 120 RGB
    boxes = [[0.0, 0.1, 0.5, 0.9], [0.25, 0.0, 1.0, 0.6], [0.4, 0.45, 0.95, 1.0]]
    phrases = ["a grey tabby cat", "a brown dog", "a robin with a red breast"]
    tokenize = lambda p: hash_tokenize(p, clip_cases.TINY_CONFIG["vocab_size"])
    hf = InstanceClipScorer(model, tokenize, backend="hf")
    hip = InstanceClipScorer(model, tokenize, backend="hip", ops=ops_for("bf16"))
    crops = crop_instances(image, boxes)
    fi, ft = hf.image_features(crops), hf.text_features(phrases)
    gi, gt = hip.image_features(crops), hip.text_features(phrases)
    rel = lambda a, b: (a - b).norm(dim=-1) / b.norm(dim=-1)
    e_img, e_txt = rel(gi, fi), rel(gt, ft)
    s_hf, s_hip = hf.score(image, boxes, phrases), hip.score(image, boxes, phrases)
    # floors: the same CLIPModel cast to bf16 against itself in fp32, on the same crops and ids
    px = torch.stack([preprocess(c, 56) for c in crops])
    _, fl_i = vc.with_floors(model, lambda m: dict(f=vc.features(m.get_image_features(pixel_values=px.to(next(m.parameters()).dtype))).float()))
    _, fl_t = vc.with_floors(model, lambda m: dict(f=torch.cat([vc.features(m.get_text_features(input_ids=tokenize(p))).float() for p in phrases])))
    ei, et = rel_rms(gi, fi), rel_rms(gt, ft)
    print(f"[parity] InstanceClipScorer hip vs hf: scores {s_hip} vs {s_hf}; per-instance e_img {e_img.tolist()} e_txt {e_txt.tolist()}; "
          f"features rel-rms image {ei:.3e} (floor {fl_i['bf16']['f']:.3e}), text {et:.3e} (floor {fl_t['bf16']['f']:.3e})")
    for i in range(3):
        assert abs(s_hip[i] - s_hf[i]) <= 2.0 * float(e_img[i] + e_txt[i])
    assert ei <= 1.5 * fl_i["bf16"]["f"] and et <= 1.5 * fl_t["bf16"]["f"]
