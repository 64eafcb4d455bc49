"""CPU tests of the CLIP image tower's host logic (weight packing, the patch GEMM's views, op sequencing, chunking, the class row)
and of ``CLIPTextEngine.text_features`` over an fp32 emulation of the op set (tests/clip_vision_cases.ClipVisionEmulOps) against
``transformers`` in fp32, and of the host side of the local CLIP score (preprocess, crop rule, demo JSON, argmax rule, the tool's
command line).  The kernels themselves are tested on the GPU (tests/test_clip_vision_gpu.py).
"""
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import clip_cases
from tests import clip_vision_cases as vc

pytest.importorskip("transformers")

REPO = clip_cases.REPO


def _ops(**kw):
    return vc.ClipVisionEmulOps(torch.float32, **kw)


# ---- engines on the emulated ops ------------------------------------------------------------------------------------------
def test_vision_engine_fp32_emulation_matches_transformers():
    from instancediffusion_amd.clip_engine import CLIPVisionEngine
    model, px = vc.tiny_vision(), vc.pixel_values(3, 56)
    ref = vc.vision_reference(model, px)
    eng = CLIPVisionEngine(model, ops=_ops())
    got = eng.encode_pixels(px)
    assert tuple(got[0].shape) == (3, 17, 128) and tuple(got[1].shape) == (3, 128) and tuple(got[2].shape) == (3, 64)
    for name, g in zip(vc.OUTPUTS, got):
        e = vc.rel_rms(g, ref[name])
        print(f"[parity] CLIPVisionEngine, fp32 emulation vs transformers (tiny): {name} {e:.2e}")
        assert g.dtype == torch.float32 and e <= 1e-4        # the bar of tests/test_clip_engine_emulated.py
    calls = eng.ops.calls
    assert calls["clip_patchify"] == 1 and calls["attention_qkv"] == 2 and "attention_causal" not in calls
    assert calls["gemm"] == 1 + 4 * 2 + 1 and calls["layernorm"] == 2          # patch GEMM, 4 per layer, projection; pre / post LN


def test_vision_engine_chunks_and_poisoned_buffers():
    """Static buffers are handed out poisoned (NaN) by the emulation: everything an output reads must have been written; chunks
    of max_batch images (B = max_batch + 1) give the rows of one call."""
    from instancediffusion_amd.clip_engine import CLIPVisionEngine
    model, px = vc.tiny_vision(), vc.pixel_values(3, 56)
    eng = CLIPVisionEngine(model, ops=_ops(batch_invariant=True))
    whole = eng.encode_pixels(px)
    assert all(bool(torch.isfinite(t).all()) for t in whole)
    eng.max_batch = 2
    parts = eng.encode_pixels(px)
    assert all(torch.equal(a, b) for a, b in zip(whole, parts))


def test_vision_engine_without_projection_and_through_a_clip_model():
    from instancediffusion_amd.clip_engine import CLIPVisionEngine
    cm, px = vc.tiny_clip_model(), vc.pixel_values(2, 56)
    eng = CLIPVisionEngine(cm.vision_model, ops=_ops())
    assert eng.encode_pixels(px)[2] is None
    with pytest.raises(RuntimeError):
        eng.image_features(px)
    eng = CLIPVisionEngine(cm.vision_model, ops=_ops(), visual_projection=cm.visual_projection)
    want = vc.features(cm.get_image_features(pixel_values=px))
    assert vc.rel_rms(eng.image_features(px), want) <= 1e-4


def test_vision_engine_rejects_what_it_cannot_run():
    from instancediffusion_amd.clip_engine import CLIPVisionEngine
    for change, what in ((dict(hidden_act="gelu"), "quick_gelu"), (dict(num_attention_heads=4), "head dim"),
                         (dict(image_size=252), "exceed"),                       # 18 x 18 + 1 = 325 > TMAX
                         (dict(hidden_size=1600, num_attention_heads=25, num_hidden_layers=1), "1536")):
        cfg = dict(vc.TINY_VISION, num_hidden_layers=1)
        cfg.update(change)
        with pytest.raises(RuntimeError, match=what):
            CLIPVisionEngine(vc.build_vision(cfg, 1), ops=_ops())
    eng = CLIPVisionEngine(vc.tiny_vision(), ops=_ops())
    with pytest.raises(ValueError):
        eng.encode_pixels(torch.zeros((1, 3, 64, 64)))


def test_text_features_fp32_emulation_matches_get_text_features():
    from instancediffusion_amd.clip_engine import CLIPTextEngine
    cm, ids = vc.tiny_clip_model(), clip_cases.tiny_input_ids()
    want = vc.features(cm.get_text_features(input_ids=ids))
    eng = CLIPTextEngine(cm.text_model, ops=_ops(), text_projection=cm.text_projection)
    got = eng.text_features(ids)
    e = vc.rel_rms(got, want)
    print(f"[parity] CLIPTextEngine.text_features, fp32 emulation vs CLIPModel.get_text_features (tiny): {e:.2e}")
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 64) and e <= 1e-4
    with pytest.raises(RuntimeError, match="text_projection"):
        CLIPTextEngine(cm.text_model, ops=_ops()).text_features(ids)


def test_full_size_golden_is_the_committed_case():
    gold = vc.load_golden("clip_vision_full")
    assert gold["meta"]["config"] == vc.FULL_VISION and gold["meta"]["salt"] == vc.FULL_SALT and gold["meta"]["proj_salt"] == vc.PROJ_SALT
    assert gold["meta"]["rows"] == [0] + list(vc.FULL_ROWS)
    assert tuple(gold["last_hidden_state_rows"].shape) == (2, 9, 1024) and tuple(gold["image_embeds"].shape) == (2, 768)
    assert float(gold["image_embeds"].std()) > 1e-3, "degenerate golden"
    for dt in ("bf16", "fp16"):
        for out in vc.OUTPUTS:
            assert 1e-4 < gold["floors"][dt][out] < 2e-2
        assert 1e-4 < gold["text_floors"][dt] < 2e-2


# ---- host side of the score ---------------------------------------------------------------------------------------------------
def test_preprocess_shape_and_constant_image():
    from PIL import Image
    from instancediffusion_amd.host import clip_score as cs
    x = cs.preprocess(Image.new("RGB", (300, 200), (10, 128, 250)))
    assert x.dtype == torch.float32 and tuple(x.shape) == (3, 224, 224)
    for c, v in enumerate((10, 128, 250)):
        want = (v / 255.0 - cs.CLIP_MEAN[c]) / cs.CLIP_STD[c]
        assert torch.allclose(x[c], torch.full((224, 224), want), atol=1e-6, rtol=0)
    assert tuple(cs.preprocess(Image.new("L", (31, 90), 7), size=56).shape) == (3, 56, 56)        # converted to RGB


def test_preprocess_crop_window():
    """A 300 x 200 image: the shorter side 200 -> 224, the longer 300 -> 336; the window is columns 56..279 of that resize."""
    import numpy as np
    from PIL import Image
    from instancediffusion_amd.host import clip_score as cs
    assert cs.resize_and_crop_window(300, 200) == (336, 224, 56, 0)
    assert cs.resize_and_crop_window(200, 300) == (224, 336, 0, 56)
    arr = torch.randint(0, 256, (200, 300, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8).numpy()
    img = Image.fromarray(arr)
    want = np.asarray(img.resize((336, 224), Image.BICUBIC).crop((56, 0, 280, 224)))
    want = torch.from_numpy(want.copy()).permute(2, 0, 1).float() / 255.0
    want = (want - torch.tensor(cs.CLIP_MEAN).view(3, 1, 1)) / torch.tensor(cs.CLIP_STD).view(3, 1, 1)
    assert torch.allclose(cs.preprocess(img), want, atol=1e-6, rtol=0)


def test_crop_rule_and_demo_json_boxes():
    from PIL import Image
    from instancediffusion_amd.host import clip_score as cs
    data = json.load(open(os.path.join(REPO, "demos", "demo_four_boxes.json")))
    boxes, phrases = cs.instances_from_demo_json(data)
    assert phrases == ["a grey tabby cat", "a brown dog", "a robin with a red breast", "a green lawn"]
    assert boxes[1] == [179 / 512, 102 / 512, (179 + 153) / 512, (102 + 153) / 512] and boxes[3][2] == 1.0
    img = Image.new("RGB", (256, 128))
    crops = cs.crop_instances(img, boxes)                    # image.crop((x0 W, y0 H, x1 W, y1 H)): PIL rounds the corners
    assert [c.size for c in crops] == [img.crop((b[0] * 256, b[1] * 128, b[2] * 256, b[3] * 128)).size for b in boxes]
    assert crops[3].size == (256, 38) and crops[0].size == (90, 57)


def test_attribute_accuracy_on_hand_made_features():
    from instancediffusion_amd.host import clip_score as cs
    assert len(cs.COLOR_LIST) == len(cs.TEXTURE_LIST) == 8 and cs.COLOR_LIST[2] == "red" and cs.TEXTURE_LIST[7] == "glass"
    labels = cs.normalise(torch.eye(8)[:, :8] + 0.01)
    img = cs.normalise(torch.stack([labels[2] * 3 + 0.1 * labels[5], labels[7], -labels[0]]))
    assert cs.predict_attribute(img, labels).tolist()[:2] == [2, 7]

    class Fixed(cs.InstanceClipScorer):                      # features by hand: crop i looks like label (2, 5, 0)[i]
        def __init__(self):
            pass

        def image_features(self, crops):
            return torch.stack([labels[2], labels[5] * 4, labels[0]])

        def text_features(self, phrases):
            assert list(phrases) == [cs.LABEL_PROMPT.format(w) for w in cs.COLOR_LIST]
            return labels * 2.0
    from PIL import Image
    acc = Fixed().attribute_accuracy(Image.new("RGB", (8, 8)), [[0, 0, 1, 1]] * 3, ["red car", "blue bird", "white dog"], cs.COLOR_LIST)
    assert acc == [1, 1, 0]                                  # "white" is label 1, the crop looks like label 0


def test_hash_tokenize_is_documented_and_in_range():
    from instancediffusion_amd.host import clip_score as cs
    ids = cs.hash_tokenize("A brown  dog", 512)
    assert tuple(ids.shape) == (1, 5) and ids[0, 0] == 510 and ids[0, -1] == 511 and bool((ids[0, 1:-1] < 510).all())
    assert torch.equal(ids, cs.hash_tokenize("a BROWN dog", 512)) and cs.hash_tokenize(" ".join(["w"] * 100), 512).shape[1] == 77


def test_scorer_hf_backend_is_the_transformers_call():
    from PIL import Image
    from instancediffusion_amd.host import clip_score as cs
    cm = vc.tiny_clip_model()
    tokenize = lambda p: cs.hash_tokenize(p, 512)
    with pytest.raises(ValueError):
        cs.InstanceClipScorer(cm, tokenize, backend="bogus")
    sc = cs.InstanceClipScorer(cm, tokenize)
    assert sc.backend == "hf" and sc.size == 56
    arr = torch.randint(0, 256, (120, 160, 3), generator=torch.Generator().manual_seed(9), dtype=torch.uint8).numpy()
    img = Image.fromarray(arr)
    boxes, phrases = [[0.0, 0.1, 0.5, 0.9], [0.25, 0.0, 1.0, 0.6]], ["a grey tabby cat", "a brown dog"]
    got = sc.score(img, boxes, phrases)
    for i, (b, p) in enumerate(zip(boxes, phrases)):
        px = cs.preprocess(img.crop((b[0] * 160, b[1] * 120, b[2] * 160, b[3] * 120)), 56)[None]
        fi = vc.features(cm.get_image_features(pixel_values=px))
        ft = vc.features(cm.get_text_features(input_ids=tokenize(p)))
        want = float((fi / fi.norm(dim=-1, keepdim=True) * (ft / ft.norm(dim=-1, keepdim=True))).sum())
        assert abs(got[i] - want) < 1e-6 and -1.0 <= got[i] <= 1.0


def test_clip_score_tool_help_runs_without_a_gpu():
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "clip_score.py"), "--help"], capture_output=True, text=True,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 0 and "--input_json" in r.stdout and "--synthetic_weights" in r.stdout and "--backend" in r.stdout
