"""``idf_clip_crop_resize`` and the batched CLIP scorer on a real MI355X.

1. The kernel against PIL: for every case of tests/clip_preproc_cases.py and both source kinds the output is ``torch.equal`` to
   ``preprocess(image.crop(...))`` -- every element, nothing excluded; NaN guard rows behind the output and the tables stay NaN.  The
   fp32 kind is held to ``inference.save_images``' conversion done in numpy, then PIL, on a source full of the values that decide a
   quantiser (``clip_preproc_cases.quantiser_probes``).
2. Bad arguments return an error before any launch (IDF_STAT_CLIP_PREPROC_LAUNCHES unchanged).
3. ``score_batch`` on ``hip`` against the per-image ``score`` on ``hip``: the pixels are identical by 1., so the two can differ only by
   the GEMM kernel a chunk's row count selects; the bar for exactly that is ``test_vision_engine_chunking``'s, image features within
   1.5 x the bf16 floor of ``with_floors``; the scores within 2 (e_img + e_txt) as ``test_scorer_hip_backend_against_hf`` derives, and
   ``score_batch`` ``hip`` against ``hf`` under that test's own conditions.
4. A device-resident fp32 batch against its own PNG round trip: equal pixels, hence equal scores.
5. ``inference.py --clip_score hip --keep_best 1`` against ``tools/clip_score.py --batched --backend hip`` on the PNGs of the same run.
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

from tests import clip_cases
from tests import clip_preproc_cases as pc
from tests import clip_vision_cases as vc
from tests.clip_cases import rel_rms

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 224
NAN_BITS = 0x7fc00000
STAT = 12                                                    # IDF_STAT_CLIP_PREPROC_LAUNCHES (include/idf.h)
_OPS = {}


def ops():
    if "o" not in _OPS:
        from instancediffusion_amd.ops import HipOps
        _OPS["o"] = HipOps(torch.bfloat16)
    return _OPS["o"]


def run_kernel(src, crops, size):
    """src: uint8 [B, H, W, 3] or fp32 [B, 3, H, W] on the CPU; crops [(image, x0, y0, x1, y1)] -> fp32 [N, 3, size, size] on the CPU.
    One NaN guard row behind the output, 64 NaN words behind the tables: both must still be NaN afterwards."""
    from instancediffusion_amd.host.clip_score import pack_crop_tables, pixel_lut
    o = ops()
    rec, blob, ntab, K = pack_crop_tables([c[1:] for c in crops], [c[0] for c in crops], size)
    tables = torch.from_numpy(np.concatenate([blob, np.full(64, NAN_BITS, np.int32)])).cuda()
    out = torch.full((len(crops) + 1, 3, size, size), float("nan"), dtype=torch.float32, device="cuda")
    n0 = o.lib.idf_get_stat(STAT)
    o.clip_crop_resize(src.cuda(), rec, tables, ntab, pixel_lut().cuda(), out[:len(crops)], K)
    torch.cuda.synchronize()
    assert o.lib.idf_get_stat(STAT) == n0 + 1                # one launch
    assert bool(torch.isnan(out[len(crops)]).all()), "stored behind the last crop"
    assert bool(torch.isnan(tables[blob.size:].view(torch.float32)).all()) and torch.equal(tables[:blob.size].cpu(), torch.from_numpy(blob))
    return out[:len(crops)].cpu()


CASES = pc.cases(S)


# ---- 1. the kernel against PIL ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("idx", range(len(CASES)), ids=[c[0] for c in CASES])
def test_crop_resize_is_the_pil_path(idx, kind):
    name, shape, crops = CASES[idx]
    if kind == "u8":
        u8 = pc.source_u8(shape)
        src = torch.from_numpy(u8)
    else:
        src = pc.source_f32(shape)
        u8 = pc.save_images_u8(src)                          # inference.save_images' conversion in numpy, then PIL
    got = run_kernel(src, crops, S)
    want = pc.pil_reference(u8, crops, S)
    bad = int((got != want).sum())
    print(f"[parity] idf_clip_crop_resize {kind} '{name}': {bad} of {got.numel()} elements differ from PIL")
    assert torch.equal(got, want)


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_crop_resize_small_target_and_one_crop(kind):
    """S = 56 (the tiny tower's size: other band counts, 56 / 4 = 14 dwords per row) on the cases that fit 32 taps there; the first
    is a launch of ONE crop."""
    from instancediffusion_amd.host.clip_score import MAX_TAPS, resample_tables
    ran = 0
    for name, shape, crops in pc.cases(56):
        if resample_tables([c[1:] for c in crops], 56)["K"] > MAX_TAPS:
            continue
        src = torch.from_numpy(pc.source_u8(shape)) if kind == "u8" else pc.source_f32(shape)
        u8 = src.numpy() if kind == "u8" else pc.save_images_u8(src)
        assert torch.equal(run_kernel(src, crops, 56), pc.pil_reference(u8, crops, 56)), name
        ran += 1
    assert ran >= 8


def test_fp32_source_holds_every_quantiser_probe():
    """The fp32 case sources really contain, inside a crop, every probe value: the whole-image case lists them at the start of
    every channel plane."""
    probes = pc.quantiser_probes()
    src = pc.source_f32((1, 512, 512))
    assert torch.equal(src[0, 1].reshape(-1)[:probes.numel()], probes)
    assert bool((probes[:256] == ((torch.arange(256, dtype=torch.float32) / 255 - 0.5) * 2)).all())
    assert bool(torch.signbit(probes[probes == 0]).any())    # -0.0


# ---- 2. rejection before any launch ----------------------------------------------------------------------------------------------
def test_crop_resize_rejects_before_any_launch():
    from instancediffusion_amd.host.clip_score import pack_crop_tables, pixel_lut
    o = ops()
    lib, st = o.lib, o._stream()
    H, W = 64, 96
    src8 = torch.zeros((1, H, W, 3), dtype=torch.uint8, device="cuda")
    rec, blob, ntab, K = pack_crop_tables([(4, 4, 60, 40)], [0], S)
    tables = torch.zeros(8 + 4 * S + 2 * 33 * S, dtype=torch.int32, device="cuda")       # room for K = 33
    tables[:blob.size] = torch.from_numpy(blob).cuda()
    lut, out = pixel_lut().cuda(), torch.zeros((1, 3, S, S), dtype=torch.float32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(src=p(src8), kind=0, crops=rec, tab=p(tables), lutp=p(lut), outp=p(out), size=S, taps=K, ncrop=1):
        crops = np.ascontiguousarray(crops, dtype=np.int32)
        return lib.idf_clip_crop_resize(src, kind, 1, H, W, C.c_void_p(crops.ctypes.data), ncrop, tab, ntab, lutp, outp, size, taps, st)

    def rect(*v):
        r = rec.copy()
        r[0, :len(v)] = v
        return r
    assert call() == 0
    torch.cuda.synchronize()
    n0 = lib.idf_get_stat(STAT)
    assert n0 >= 1
    assert call(taps=33) == -3                               # IDF_E_UNSUPPORTED: K > 32
    assert call(crops=rect(0, 40, 4, 57, 36)) == -1          # x0 + width = 97 > W
    assert call(crops=rect(0, 4, 30, 56, 35)) == -1          # y0 + height = 65 > H
    assert call(crops=rect(0, -1, 4, 56, 36)) == -1 and call(crops=rect(1, 4, 4, 56, 36)) == -1    # x0 < 0; image 1 of 1
    assert call(crops=rect(0, 4, 4, 0, 36)) == -1 and call(crops=rect(0, 4, 4, 56, 36, 1)) == -1   # empty; table set 1 of 1
    assert call(src=None) == -1 and call(tab=None) == -1 and call(lutp=None) == -1 and call(outp=None) == -1
    assert lib.idf_clip_crop_resize(p(src8), 0, 1, H, W, None, 1, p(tables), ntab, p(lut), p(out), S, K, st) == -1
    assert call(size=0) == -1 and call(size=222) == -1       # S = 0; S % 4
    assert call(kind=2) == -1 and call(kind=-1) == -1        # unknown source kind
    assert call(taps=0) == -1 and call(ncrop=0) == -1
    assert call(outp=C.c_void_p(out.data_ptr() + 4)) == -2   # IDF_E_ALIGN
    assert lib.idf_get_stat(STAT) == n0                      # nothing was launched
    torch.cuda.synchronize()
    # the host refuses an empty box before it builds anything
    from instancediffusion_amd.host.clip_score import crop_rects
    with pytest.raises(ValueError):
        crop_rects([[0.5, 0.1, 0.5, 0.9]], W, H)


# ---- 3. batched scorer against the per-image scorer --------------------------------------------------------------------------------
BOXES = [[0.0, 0.1, 0.5, 0.9], [0.25, 0.0, 1.0, 0.6], [0.4, 0.45, 0.95, 1.0]]
PHRASES = ["a grey tabby cat", "a brown dog", "a robin with a red breast"]


@pytest.fixture(scope="module")
def scorers():
    pytest.importorskip("transformers")
    from instancediffusion_amd.host.clip_score import InstanceClipScorer, hash_tokenize
    model = vc.tiny_clip_model()
    tokenize = lambda p: hash_tokenize(p, clip_cases.TINY_CONFIG["vocab_size"])
    return (model, tokenize, InstanceClipScorer(model, tokenize, backend="hf"),
            InstanceClipScorer(model, tokenize, backend="hip", ops=ops()))


def test_score_batch_hip_against_score_hip_and_hf(scorers):
    from PIL import Image
    from instancediffusion_amd.host.clip_score import crop_instances, preprocess
    model, tokenize, hf, hip = scorers
    u8 = torch.from_numpy(pc.source_u8((3, 120, 160)))       # 160 x 120 RGB, three images, three instances each
    pil = [Image.fromarray(a.numpy()) for a in u8]
    crops = [c for im in pil for c in crop_instances(im, BOXES)]
    n0 = ops().lib.idf_get_stat(STAT)
    px = hip.pixels_batch(u8.cuda(), BOXES)
    assert ops().lib.idf_get_stat(STAT) == n0 + 1 and px.is_cuda
    want_px = torch.stack([preprocess(c, 56) for c in crops])
    assert torch.equal(px.cpu(), want_px)                    # the pixels of the two paths are the same bits
    rel = lambda a, b: (a - b).norm(dim=-1) / b.norm(dim=-1)
    # hip batched vs hip per image
    f_loop = torch.cat([hip.image_features(crop_instances(im, BOXES)) for im in pil])
    f_batch = hip.image_features_batch(u8.cuda(), BOXES)
    _, fl_i = vc.with_floors(model, lambda m: dict(f=vc.features(m.get_image_features(pixel_values=want_px.to(next(m.parameters()).dtype))).float()))
    _, fl_t = vc.with_floors(model, lambda m: dict(f=torch.cat([vc.features(m.get_text_features(input_ids=tokenize(p))).float() for p in PHRASES])))
    e_paths = rel_rms(f_batch, f_loop)
    print(f"[parity] score_batch hip vs score hip: image features rel-rms {e_paths:.3e} (bar 1.5 x floor {fl_i['bf16']['f']:.3e})")
    assert e_paths <= 1.5 * fl_i["bf16"]["f"]
    s_loop = [hip.score(im, BOXES, PHRASES) for im in pil]
    s_batch = hip.score_batch(u8.cuda(), BOXES, PHRASES)
    t_loop, t_batch = hip.text_features(PHRASES), hip.text_features_cached(PHRASES)
    e_img, e_txt = rel(f_batch, f_loop).view(3, 3), rel(t_batch, t_loop)
    print(f"[parity] score_batch hip {s_batch} vs score hip {s_loop}; e_img {e_img.tolist()} e_txt {e_txt.tolist()}")
    for b in range(3):
        for i in range(3):
            assert abs(s_batch[b][i] - s_loop[b][i]) <= 2.0 * float(e_img[b][i] + e_txt[i])
    # hip batched vs hf batched: the conditions of test_scorer_hip_backend_against_hf
    f_hf, t_hf = hf.image_features_batch(u8, BOXES), hf.text_features(PHRASES)
    s_hf = hf.score_batch(u8, BOXES, PHRASES)
    e_img, e_txt = rel(f_batch, f_hf).view(3, 3), rel(t_batch, t_hf)
    ei, et = rel_rms(f_batch, f_hf), rel_rms(t_batch, t_hf)
    print(f"[parity] score_batch hip vs hf: features rel-rms image {ei:.3e} (floor {fl_i['bf16']['f']:.3e}), text {et:.3e} "
          f"(floor {fl_t['bf16']['f']:.3e}); scores {s_batch} vs {s_hf}")
    for b in range(3):
        for i in range(3):
            assert abs(s_batch[b][i] - s_hf[b][i]) <= 2.0 * float(e_img[b][i] + e_txt[i])
    assert ei <= 1.5 * fl_i["bf16"]["f"] and et <= 1.5 * fl_t["bf16"]["f"]
    assert hip.attribute_accuracy_batch(u8.cuda(), BOXES, ["red car", "blue bird", "green apple"]) is not None


# ---- 4. device batch against the PNG round trip ----------------------------------------------------------------------------------
def test_device_batch_equals_its_png_round_trip(scorers, tmp_path):
    import inference
    from PIL import Image
    _, _, _, hip = scorers
    batch = pc.source_f32((3, 120, 160)).cuda()              # fp32 [3, 3, 120, 160] on the device, as AutoencoderKL.decode leaves it
    names = inference.save_images(batch, str(tmp_path / "png"))
    back = torch.from_numpy(np.stack([np.asarray(Image.open(n).convert("RGB"), dtype=np.uint8) for n in names]))
    px_dev, px_png = hip.pixels_batch(batch, BOXES), hip.pixels_batch(back.cuda(), BOXES)
    assert tuple(px_dev.shape) == (9, 3, 56, 56) and torch.equal(px_dev, px_png)
    assert hip.score_batch(batch, BOXES, PHRASES) == hip.score_batch(back.cuda(), BOXES, PHRASES)
    assert hip.score_batch([Image.open(n) for n in names], BOXES, PHRASES) == hip.score_batch(batch, BOXES, PHRASES)


# ---- 5. inference.py --clip_score hip ----------------------------------------------------------------------------------------------
def test_inference_cli_clip_score_and_keep_best(tmp_path, monkeypatch, capsys):
    pytest.importorskip("transformers")
    import inference
    from tests.test_inference_cli_gpu import ALPHA, SEED, STEPS
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import clip_score as tool
    finally:
        sys.path.remove(os.path.join(REPO, "tools"))
    demo = os.path.join(REPO, "demos", "demo_four_boxes.json")
    monkeypatch.chdir(REPO)
    monkeypatch.delenv("IDF_CLIP_PATH", raising=False)
    folder = f"gc7.5-seed{SEED}-alpha{ALPHA}"

    def run(out, extra):
        monkeypatch.setattr(sys, "argv", ["inference.py", "--synthetic_weights", "--num_images", "2", "--steps", str(STEPS), "--alpha", str(ALPHA),
                                          "--seed", str(SEED), "--input_json", demo, "--test_config", os.path.join(REPO, "configs", "test_box.yaml"),
                                          "--output", str(out), "--dtype", "bf16", "--clip_score", "hip"] + extra)
        inference.main()
        return out / folder
    best = run(tmp_path / "A", ["--keep_best", "1"])
    assert sorted(n for n in os.listdir(best) if n.endswith(".png")) == ["0.png"]
    rep = json.load(open(best / "clip_scores.json"))
    assert sorted(rep["images"]) == ["0", "1"] and all(len(v) == 4 for v in rep["images"].values()) and len(rep["phrases"]) == 4
    assert sorted(rep["ranking"]) == [0, 1] and rep["means"][str(rep["ranking"][0])] >= rep["means"][str(rep["ranking"][1])]
    assert rep["saved"] == {"0.png": rep["ranking"][0]} and rep["backend"] == "hip" and rep["dtype"] == "bf16" and rep["weights"] == "synthetic"
    for i in ("0", "1"):
        assert rep["means"][i] == pytest.approx(sum(rep["images"][i]) / 4, abs=1e-6)
    both = run(tmp_path / "B", [])                           # the same run without --keep_best: both PNGs
    assert sorted(n for n in os.listdir(both) if n.endswith(".png")) == ["0.png", "1.png"]
    assert json.load(open(both / "clip_scores.json"))["images"] == rep["images"]
    capsys.readouterr()
    monkeypatch.setattr(sys, "argv", ["clip_score.py", "--input_json", demo, "--images", str(both), "--synthetic_weights", "--backend", "hip",
                                      "--batched"])
    tool.main()
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    print(f"[parity] inference.py --clip_score hip {rep['images']} vs tools/clip_score.py --batched {line['images']}")
    assert line["images"] == {"0.png": rep["images"]["0"], "1.png": rep["images"]["1"]}
    assert line["phrases"] == rep["phrases"] and line["mean"] == rep["mean"]
    # the saved PNG of the first run is the best-ranked image of the second
    from PIL import Image
    assert np.array_equal(np.asarray(Image.open(best / "0.png")), np.asarray(Image.open(both / f"{rep['ranking'][0]}.png")))
