"""The host side of the device crop + resize (host/clip_score.py), without a GPU: ``resample_reference`` -- the tables of
``resample_tables`` applied with numpy integers, the CPU twin of ``idf_clip_crop_resize`` -- is ``torch.equal`` to the PIL path
``preprocess(image.crop(...))`` on every case of tests/clip_preproc_cases.py at S = 56 and 224; the crop rounding, the table shapes and
the batched scorer on backend ``hf``; the new flags of the entry points."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import clip_preproc_cases as pc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("S", pc.SIZES)
@pytest.mark.parametrize("idx", range(len(pc.cases(224))), ids=[c[0] for c in pc.cases(224)])
def test_resample_reference_is_the_pil_path(idx, S):
    from instancediffusion_amd.host.clip_score import resample_reference
    name, shape, crops = pc.cases(S)[idx]
    src = pc.source_u8(shape)
    got = resample_reference(src, [c[1:] for c in crops], S, image_index=[c[0] for c in crops])
    want = pc.pil_reference(src, crops, S)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(crops), 3, S, S)
    assert torch.equal(got, want), f"{name}: {int((got != want).sum())} of {got.numel()} elements differ"


def test_quantise_images_is_the_save_images_conversion():
    from instancediffusion_amd.host.clip_score import quantise_images
    x = pc.source_f32((2, 24, 40))
    assert np.array_equal(quantise_images(x), pc.save_images_u8(x))
    probes = pc.quantiser_probes()
    assert probes.numel() >= 3 * 256 + 8 and bool((probes == 0).any()) and float(probes.max()) > 1 and float(probes.min()) < -1


def test_crop_rects_round_ties_to_even_as_image_crop():
    from PIL import Image
    from instancediffusion_amd.host.clip_score import crop_instances, crop_rects
    W, H = 10, 20
    image = Image.new("RGB", (W, H))
    boxes = [[0.25, 0.125, 0.35, 0.175],      # x W = 2.5, 3.5 -> 2, 4; y H = 2.5, 3.5 -> 2, 4
             [0.05, 0.025, 0.45, 0.475],      # 0.5, 4.5 -> 0, 4; 0.5, 9.5 -> 0, 10
             [0.0, 0.0, 1.0, 1.0], [0.31, 0.52, 0.77, 0.93]]
    rects = crop_rects(boxes, W, H)
    assert rects[0] == (2, 2, 4, 4) and rects[1] == (0, 0, 4, 10) and rects[2] == (0, 0, W, H)
    for r, c in zip(rects, crop_instances(image, boxes)):
        assert (r[2] - r[0], r[3] - r[1]) == c.size


def test_empty_or_outside_box_raises():
    from instancediffusion_amd.host.clip_score import crop_rects, resample_tables
    with pytest.raises(ValueError):
        crop_rects([[0.2, 0.2, 0.2, 0.9]], 100, 100)          # zero width
    with pytest.raises(ValueError):
        crop_rects([[0.2, 0.504, 0.9, 0.496]], 100, 100)      # y rounds to 50, 50
    with pytest.raises(ValueError):
        crop_rects([[0.2, 0.2, 1.2, 0.9]], 100, 100)
    with pytest.raises(ValueError):
        resample_tables([(3, 3, 3, 9)], 56)


def test_table_shapes_and_tap_counts_follow_the_rule():
    """K = Pillow's ksize = 2 ceil(2 max(in / out, 1)) + 1 of the worst axis: 11 for 512 -> 224, 15 for 768, 21 for 1024, 5 when
    nothing shrinks; the two axes of 448 x 449 differ."""
    from instancediffusion_amd.host.clip_score import MAX_TAPS, pack_crop_tables, resample_tables
    S = 224
    for side, K in ((512, 11), (768, 15), (1024, 21), (224, 5), (5, 5)):
        t = resample_tables([(0, 0, side, side)], S)
        assert t["K"] == K and t["first"].shape == (1, 2, S) and t["count"].shape == (1, 2, S) and t["coef"].shape == (1, 2, S, K)
        assert t["first"].dtype == t["count"].dtype == t["coef"].dtype == np.int32
        assert int(t["count"].max()) <= K and int(t["first"].min()) >= 0 and int((t["first"] + t["count"]).max()) <= side
        live = np.arange(K)[None, None, None, :] < t["count"][..., None]
        assert not t["coef"][~live].any()                                                  # zero behind the count
        assert np.abs(t["coef"].sum(-1) - (1 << 22)).max() <= K                           # normalised weights, each rounded once
    t = resample_tables([(1, 2, 449, 451), (0, 0, 37, 211)], S)
    # 448 -> 224: support exactly 4, a window of 8 source pixels; 449 -> 224: support 4.009, 9 pixels at some indices, ksize 11
    assert t["K"] == 11 and int(t["count"][0, 0].max()) == 8 and int(t["count"][0, 1].max()) == 9
    assert int(t["count"][1, 0].max()) <= 5                                                # 37 -> 224 upscales: support 2
    # the packed blob: crop records, then one table set per distinct crop size
    rects = [(0, 0, 100, 50), (7, 9, 107, 59), (0, 0, 50, 100)]
    crops, blob, ntab, K = pack_crop_tables(rects, [0, 1, 1], S)
    assert ntab == 2 and crops.shape == (3, 8) and crops[:, 5].tolist() == [0, 0, 1] and crops[1, :5].tolist() == [1, 7, 9, 100, 50]
    assert blob.dtype == np.int32 and blob.size == 3 * 8 + ntab * (4 * S + 2 * K * S)
    with pytest.raises(ValueError):
        pack_crop_tables([(0, 0, 2048, 2048)], [0], S)                                     # 39 taps > MAX_TAPS
    assert MAX_TAPS == 32


def test_pixel_lut_is_the_preprocess_expression():
    from PIL import Image
    from instancediffusion_amd.host.clip_score import pixel_lut, preprocess
    lut = pixel_lut()
    assert lut.dtype == torch.float32 and tuple(lut.shape) == (3, 256)
    for v in (0, 1, 127, 128, 254, 255):
        assert torch.equal(preprocess(Image.new("RGB", (8, 8), (v, v, v)), 8)[:, 0, 0], lut[:, v])


@pytest.fixture(scope="module")
def tiny_scorer():
    pytest.importorskip("transformers")
    from tests import clip_cases
    from tests import clip_vision_cases as vc
    from instancediffusion_amd.host.clip_score import InstanceClipScorer, hash_tokenize
    return InstanceClipScorer(vc.tiny_clip_model(), lambda p: hash_tokenize(p, clip_cases.TINY_CONFIG["vocab_size"]), backend="hf")


BOXES = [[0.0, 0.1, 0.5, 0.9], [0.25, 0.0, 1.0, 0.6], [0.4, 0.45, 0.95, 1.0]]
PHRASES = ["a grey tabby cat", "a brown dog", "a robin with a red breast"]


def test_score_batch_hf_is_a_loop_of_score(tiny_scorer):
    from PIL import Image
    u8 = torch.from_numpy(pc.source_u8((3, 120, 160)))
    pil = [Image.fromarray(a.numpy()) for a in u8]
    want = [tiny_scorer.score(im, BOXES, PHRASES) for im in pil]
    assert tiny_scorer.score_batch(u8, BOXES, PHRASES) == want
    assert tiny_scorer.score_batch(pil, BOXES, PHRASES) == want
    assert tiny_scorer.score_batch(u8, [BOXES] * 3, [PHRASES] * 3) == want               # one set per image
    assert set(tiny_scorer._phrase_cache) == set(PHRASES)                                  # each phrase encoded once, kept
    # fp32 decoder output: scored as the PNGs save_images would write
    f32 = pc.source_f32((2, 120, 160))
    want = [tiny_scorer.score(Image.fromarray(a), BOXES, PHRASES) for a in pc.save_images_u8(f32)]
    assert tiny_scorer.score_batch(f32, BOXES, PHRASES) == want
    with pytest.raises(ValueError):
        tiny_scorer.score_batch(u8, BOXES, PHRASES[:2])
    with pytest.raises(ValueError):
        tiny_scorer.score_batch(u8, [BOXES] * 2, PHRASES)


def test_attribute_accuracy_batch_hf_is_a_loop_of_attribute_accuracy(tiny_scorer):
    from PIL import Image
    u8 = torch.from_numpy(pc.source_u8((2, 120, 160)))
    phrases = ["red car", "blue bird", "green apple"]
    want = [tiny_scorer.attribute_accuracy(Image.fromarray(a.numpy()), BOXES, phrases) for a in u8]
    assert tiny_scorer.attribute_accuracy_batch(u8, BOXES, phrases) == want


def test_rank_by_mean():
    from instancediffusion_amd.host.clip_score import rank_by_mean
    means, ranking = rank_by_mean([[0.1, 0.3], [0.4, 0.2], [0.0, 0.4], [-0.5, 0.1]])
    assert ranking == [1, 0, 2, 3] and means[1] == pytest.approx(0.3)


def test_synthetic_clip_model_lives_in_the_package():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import clip_score as tool
    finally:
        sys.path.remove(os.path.join(REPO, "tools"))
    from instancediffusion_amd.host import clip_score as cs
    assert tool.synthetic_clip_model is cs.synthetic_clip_model and cs.SYNTH_SALT == 31 and cs.CLIP_L14_VISION["hidden_size"] == 1024


@pytest.mark.parametrize("script,flags", [("inference.py", ["--clip_score", "--clip_path", "--keep_best"]),
                                          (os.path.join("tools", "clip_score.py"), ["--batched"]),
                                          (os.path.join("tools", "clip_bench.py"), ["--score"])])
def test_entry_points_show_the_new_flags(script, flags):
    r = subprocess.run([sys.executable, os.path.join(REPO, script), "--help"], capture_output=True, text=True, cwd=REPO, timeout=300)
    assert r.returncode == 0, r.stderr[-500:]
    for f in flags:
        assert f in r.stdout
