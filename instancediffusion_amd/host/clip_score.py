"""Local CLIP score of a generated image against its instance prompts: the HF branch of the reference's
``eval/eval_attribute_binding.py:19-60,180-208``.  Every instance box is cropped out of the image, the crop's CLIP image features
and the phrase's CLIP text features are L2-normalised, and their dot product is the score; the attribute accuracy is the argmax of
the crop's features over eight "a {word} object" prompts (:54-59, :162-169).

``backend="hf"`` (the default) calls ``get_image_features`` / ``get_text_features`` of the ``transformers`` ``CLIPModel`` handed in,
unchanged.  ``backend="hip"`` runs both towers on the HIP kernels (``clip_engine.CLIPVisionEngine`` / ``CLIPTextEngine``, 16-bit
storage in ``dtype``); there is no fallback from it.  Not ported: the ``open_clip`` branch and the COCO loop around the metric.

The batched path (``score_batch`` / ``attribute_accuracy_batch``) scores B images at once.  On ``hip`` the crop and the bicubic
resize run on the device (``idf_clip_crop_resize``) and give the very pixels ``preprocess`` gives: Pillow's 8-bit resample is integer
arithmetic over coefficient tables, ``resample_tables`` builds those tables in float64 exactly as Pillow does, and
``resample_reference`` applies them with numpy integers (the kernel's CPU twin).
"""
from __future__ import annotations

import functools
import hashlib
from typing import Callable, List, Optional, Sequence

import torch

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
# eval_attribute_binding.py:81-85: the eight colours and the eight textures of the attribute-binding evaluation
COLOR_LIST = ("black", "white", "red", "green", "yellow", "blue", "pink", "purple")
TEXTURE_LIST = ("rubber", "fluffy", "metallic", "wooden", "plastic", "fabric", "leather", "glass")
LABEL_PROMPT = "a {} object"
BACKENDS = ("hf", "hip")
PRECISION_BITS = 22          # Pillow's 8-bit resample: coefficients in 22-bit fixed point (32 - 8 - 2)
MAX_TAPS = 32                # the largest tap count idf_clip_crop_resize accepts (a 1024-px short side resized to 224 needs 21)
# openai/clip-vit-large-patch14, the model of the reference's metric
CLIP_L14_VISION = dict(hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16, image_size=224,
                       patch_size=14, projection_dim=768, hidden_act="quick_gelu", layer_norm_eps=1e-5)
SYNTH_SALT = 31


def resize_and_crop_window(width: int, height: int, size: int = 224):
    """The ``CLIPFeatureExtractor`` geometry: -> (new_w, new_h, left, top): the shorter side becomes ``size`` (the longer one
    ``int(size * long / short)``), then the centred ``size`` x ``size`` window."""
    if width <= height:
        nw, nh = size, int(size * height / width)
    else:
        nw, nh = int(size * width / height), size
    return nw, nh, (nw - size) // 2, (nh - size) // 2


def preprocess(pil_image, size: int = 224) -> torch.Tensor:
    """PIL image -> fp32 [3, size, size]: RGB, bicubic resize of the shorter side to ``size``, centre crop, / 255, CLIP mean / std."""
    import numpy as np
    from PIL import Image
    img = pil_image.convert("RGB")
    nw, nh, left, top = resize_and_crop_window(img.width, img.height, size)
    img = img.resize((nw, nh), Image.BICUBIC).crop((left, top, left + size, top + size))
    x = torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).permute(2, 0, 1).float() * (1.0 / 255.0)
    return (x - torch.tensor(CLIP_MEAN).view(3, 1, 1)) / torch.tensor(CLIP_STD).view(3, 1, 1)


def crop_instances(image, boxes_xyxy_norm: Sequence[Sequence[float]]) -> list:
    """eval_attribute_binding.py:186-190: ``image.crop((x0 W, y0 H, x1 W, y1 H))`` per normalised box."""
    W, H = image.width, image.height
    return [image.crop((b[0] * W, b[1] * H, b[2] * W, b[3] * H)) for b in boxes_xyxy_norm]


def crop_rects(boxes_xyxy_norm: Sequence[Sequence[float]], W: int, H: int) -> list:
    """``Image.crop``'s rounding of ``crop_instances``' float boxes: -> [(x0, y0, x1, y1)] ints, each coordinate through Python
    ``round`` (ties to even).  A crop of zero width or height, or one that leaves the image, is a ValueError: PIL fails on the first
    and pads the second with black, which no instance box of the metric asks for."""
    rects = []
    for b in boxes_xyxy_norm:
        x0, y0, x1, y1 = (int(round(v)) for v in (b[0] * W, b[1] * H, b[2] * W, b[3] * H))
        if x1 <= x0 or y1 <= y0:
            raise ValueError(f"box {tuple(b)} is an empty crop ({x0}, {y0}, {x1}, {y1}) of a {W} x {H} image")
        if x0 < 0 or y0 < 0 or x1 > W or y1 > H:
            raise ValueError(f"box {tuple(b)} leaves the {W} x {H} image: ({x0}, {y0}, {x1}, {y1})")
        rects.append((x0, y0, x1, y1))
    return rects


def _cubic(x):
    """Pillow's ``bicubic_filter`` (a = -0.5), operation for operation, on a float64 array."""
    import numpy as np
    a = -0.5
    x = np.abs(x)
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def _axis_tables(in_size: int, out_size: int, first_out: int, S: int):
    """Pillow's ``precompute_coeffs`` + ``normalize_coeffs_8bpc`` for the output indices [first_out, first_out + S) of an axis
    resized from ``in_size`` to ``out_size``: -> (first [S], count [S], coef [S, k] int32), k = Pillow's ``ksize`` = 2 ceil(support) + 1 (no count is larger).
    Vectorised over the output indices; the taps are walked in a Python loop so that the sum runs left to right as Pillow's."""
    import numpy as np
    scale = np.float64(in_size) / np.float64(out_size)
    filterscale = max(scale, np.float64(1.0))
    support = 2.0 * filterscale
    ss = 1.0 / filterscale
    center = (np.arange(first_out, first_out + S, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size)
    count = xmax - xmin
    k = int(np.ceil(support)) * 2 + 1
    w = np.zeros((S, k), dtype=np.float64)
    ww = np.zeros(S, dtype=np.float64)
    for x in range(k):
        live = x < count
        w[:, x] = np.where(live, _cubic((x + xmin - center + 0.5) * ss), 0.0)
        ww = ww + w[:, x]                                      # a tap that is not live adds +0.0: the sum is Pillow's
    w = np.where((ww != 0.0)[:, None], w / np.where(ww != 0.0, ww, 1.0)[:, None], w)
    coef = np.trunc(np.where(w < 0, -0.5, 0.5) + w * np.float64(1 << PRECISION_BITS)).astype(np.int32)
    return xmin.astype(np.int32), count.astype(np.int32), coef


def resample_tables(rects: Sequence[Sequence[int]], S: int) -> dict:
    """The coefficient tables of ``preprocess`` for every crop rectangle (x0, y0, x1, y1): the crop is resized so that its short
    side becomes S (``resize_and_crop_window``) and only the centred S x S window is kept, so each axis needs S output indices.
    -> dict(K, first [N, 2, S] int32, count [N, 2, S] int32, coef [N, 2, S, K] int32); axis 0 is horizontal, axis 1 vertical;
    ``first`` counts from the crop's own corner; K is the largest ``ksize`` of the call (11 for 512 -> 224, 21 for 1024 -> 224),
    coefficients behind an index' count are 0."""
    import numpy as np
    per = []
    for x0, y0, x1, y1 in rects:
        cw, ch = int(x1 - x0), int(y1 - y0)
        if cw <= 0 or ch <= 0:
            raise ValueError(f"empty crop rectangle {(x0, y0, x1, y1)}")
        nw, nh, left, top = resize_and_crop_window(cw, ch, S)
        per.append((_axis_tables(cw, nw, left, S), _axis_tables(ch, nh, top, S)))
    K = max(t[2].shape[1] for pair in per for t in pair)
    N = len(per)
    first, count = np.zeros((N, 2, S), np.int32), np.zeros((N, 2, S), np.int32)
    coef = np.zeros((N, 2, S, K), np.int32)
    for n, pair in enumerate(per):
        for ax, (f, c, k) in enumerate(pair):
            first[n, ax], count[n, ax], coef[n, ax, :, :k.shape[1]] = f, c, k
    return dict(K=K, first=first, count=count, coef=coef)


def pack_crop_tables(rects: Sequence[Sequence[int]], image_index: Sequence[int], S: int):
    """What one ``idf_clip_crop_resize`` launch reads: -> (crops int32 [N, 8] = (image, x0, y0, width, height, table set, 0, 0),
    blob int32 = those records | per table set the (first, count) pairs [2, S, 2] | per table set the coefficients [2, K, S]
    (tap-major), number of table sets, K).  The tables depend on a crop's size alone, so crops of one size share a set: the B
    images of a batch with one list of boxes upload N sets, not B N."""
    import numpy as np
    sizes, tset = {}, []
    for x0, y0, x1, y1 in rects:
        tset.append(sizes.setdefault((x1 - x0, y1 - y0), len(sizes)))
    t = resample_tables([(0, 0, w, h) for w, h in sizes], S)
    if t["K"] > MAX_TAPS:
        raise ValueError(f"a crop of this call needs {t['K']} taps to reach {S} px; idf_clip_crop_resize takes at most {MAX_TAPS}")
    crops = np.zeros((len(rects), 8), np.int32)
    for n, (x0, y0, x1, y1) in enumerate(rects):
        crops[n, :6] = (image_index[n], x0, y0, x1 - x0, y1 - y0, tset[n])
    bounds = np.stack([t["first"], t["count"]], axis=-1)                                   # [T, 2, S, 2]
    blob = np.concatenate([crops.ravel(), bounds.ravel(), t["coef"].transpose(0, 1, 3, 2).ravel()]).astype(np.int32)
    return crops, blob, len(sizes), t["K"]


def _resample_axis(rows, first, count, coef):
    """One 8-bit pass of Pillow's ``ImagingResample`` along axis 1 of ``rows`` [R, in, 3] uint8 -> [R, S, 3] uint8:
    clip8((2^21 + sum pixel * k) >> 22) in int32."""
    import numpy as np
    S, K = coef.shape
    idx = np.minimum(first[:, None] + np.arange(K)[None, :], rows.shape[1] - 1)          # taps behind the count carry k = 0
    acc = np.full((rows.shape[0], S, 3), 1 << (PRECISION_BITS - 1), dtype=np.int32)
    for k in range(K):
        acc += rows[:, idx[:, k], :].astype(np.int32) * coef[None, :, k, None]
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def pixel_lut() -> torch.Tensor:
    """fp32 [3, 256]: what ``preprocess`` makes of byte v in channel c, by its own torch expression."""
    x = torch.arange(256, dtype=torch.uint8).view(1, 256, 1).expand(3, 256, 1).float() * (1.0 / 255.0)
    return ((x - torch.tensor(CLIP_MEAN).view(3, 1, 1)) / torch.tensor(CLIP_STD).view(3, 1, 1)).view(3, 256).contiguous()


def quantise_images(images: torch.Tensor):
    """``inference.save_images``' conversion of decoder output fp32 [B, 3, H, W] -> numpy uint8 [B, H, W, 3]: clamp to [-1, 1],
    * 0.5 + 0.5, * 255 in fp32, truncate."""
    import numpy as np
    x = torch.clamp(images.float(), min=-1, max=1) * 0.5 + 0.5
    return (x.cpu().numpy().transpose(0, 2, 3, 1) * 255).astype(np.uint8)


def resample_reference(src, rects: Sequence[Sequence[int]], S: int, image_index: Optional[Sequence[int]] = None,
                       tables: Optional[dict] = None) -> torch.Tensor:
    """The CPU twin of ``idf_clip_crop_resize``: src uint8 [B, H, W, 3] (numpy or tensor) or [H, W, 3], crop n = ``rects[n]`` of
    image ``image_index[n]`` (default 0) -> fp32 [N, 3, S, S], ``torch.equal`` to ``preprocess`` of the PIL crops.  Horizontal pass
    over the intermediate rows the vertical window needs, then the vertical pass on its uint8 result, then ``pixel_lut``."""
    import numpy as np
    src = np.asarray(src.cpu() if isinstance(src, torch.Tensor) else src)
    if src.ndim == 3:
        src = src[None]
    if src.dtype != np.uint8 or src.ndim != 4 or src.shape[-1] != 3:
        raise ValueError("resample_reference expects uint8 [B, H, W, 3]")
    t = tables or resample_tables(rects, S)
    lut = pixel_lut().numpy()
    out = np.empty((len(rects), 3, S, S), np.float32)
    for n, (x0, y0, x1, y1) in enumerate(rects):
        crop = src[image_index[n] if image_index is not None else 0, y0:y1, x0:x1]
        vf, vc = t["first"][n, 1], t["count"][n, 1]
        lo, hi = int(vf.min()), int((vf + vc).max())
        mid = _resample_axis(crop[lo:hi], t["first"][n, 0], t["count"][n, 0], t["coef"][n, 0])            # [rows, S, 3]
        res = _resample_axis(mid.transpose(1, 0, 2), vf - lo, vc, t["coef"][n, 1]).transpose(1, 0, 2)   # [S(y), S(x), 3]
        for c in range(3):
            out[n, c] = lut[c][res[:, :, c]]
    return torch.from_numpy(out)


@functools.lru_cache(maxsize=1)
def synthetic_clip_model():
    """A key-seeded ViT-L/14 ``CLIPModel``: a dry run of the whole path without a checkpoint (the scores mean nothing).  Built once
    per process."""
    from transformers import CLIPConfig, CLIPModel
    from .. import synth
    from .text_encoder import CLIP_L14_TEXT
    model = CLIPModel(CLIPConfig(text_config=dict(CLIP_L14_TEXT), vision_config=dict(CLIP_L14_VISION), projection_dim=768)).eval()
    model.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items() if v.is_floating_point()},
                                                 SYNTH_SALT), strict=False)
    return model


def instances_from_demo_json(data: dict):
    """The demo JSON ``inference.py`` reads -> (normalised xyxy boxes, phrases) of its instances."""
    from .input import rescale_box
    W, H = data["width"], data["height"]
    annos = data["annos"]
    return [rescale_box(a["bbox"], W, H) for a in annos], [a["caption"] for a in annos]


def hash_tokenize(phrase: str, vocab_size: int, max_length: int = 77) -> torch.Tensor:
    """Stand-in tokenizer for synthetic weights without a BPE vocabulary: -> ids [1, L].  The phrase is lower-cased and split at
    white space; word w becomes ``int.from_bytes(sha256(w)[:8], "little") % (vocab_size - 2)``; <|startoftext|> = vocab_size - 2
    goes in front and <|endoftext|> = vocab_size - 1 (the largest id, as in CLIP's vocabulary) behind, after truncation to
    ``max_length - 2`` words.  No padding, as ``tokenizer(text, return_tensors="pt")`` of the reference."""
    words = phrase.lower().split()[:max_length - 2]
    ids = [int.from_bytes(hashlib.sha256(w.encode()).digest()[:8], "little") % (vocab_size - 2) for w in words]
    return torch.tensor([[vocab_size - 2] + ids + [vocab_size - 1]], dtype=torch.long)


def normalise(x: torch.Tensor) -> torch.Tensor:
    return x / torch.linalg.norm(x, dim=-1, keepdim=True)


def predict_attribute(img_features: torch.Tensor, label_features: torch.Tensor) -> torch.Tensor:
    """eval_attribute_binding.py:54-59: normalised image features [N, P] x normalised label features [L, P] -> argmax label [N]."""
    return (img_features[:, None, :] * label_features[None, :, :]).sum(-1).argmax(-1)


def _features(out) -> torch.Tensor:
    return out if isinstance(out, torch.Tensor) else out.pooler_output      # transformers >= 5 wraps the features in an output


def local_tokenizer(path):
    """The BPE tokenizer ``host/text_encoder.py`` uses, from local files only; None when the vocabulary is not there."""
    from transformers import CLIPTokenizer
    from .text_encoder import CLIP_L14_TEXT
    try:
        tok = CLIPTokenizer.from_pretrained(path, local_files_only=True)
    except Exception:
        return None
    return tok if len(tok) >= CLIP_L14_TEXT["vocab_size"] else None     # transformers >= 5 builds an EMPTY tokenizer without files


def load_clip(clip_path: Optional[str]):
    """The CLIP model and tokenizer of the command-line entry points: -> (CLIPModel, tokenize, "bpe" | "hash").  ``clip_path``: a
    local directory of openai/clip-vit-large-patch14 (``local_files_only``: nothing is ever fetched); None: the key-seeded synthetic
    model, with the BPE vocabulary under ``$IDF_CLIP_PATH`` when there is one, else ``hash_tokenize``."""
    import os
    if clip_path is None:
        model = synthetic_clip_model()
        tok = local_tokenizer(os.environ.get("IDF_CLIP_PATH", "openai/clip-vit-large-patch14"))
    else:
        from transformers import CLIPModel
        model = CLIPModel.from_pretrained(clip_path, local_files_only=True).eval()
        tok = local_tokenizer(clip_path)
        if tok is None:
            raise SystemExit(f"no CLIP BPE vocabulary (vocab.json, merges.txt) in {clip_path}")
    vocab = int(model.config.text_config.vocab_size)
    tokenize = (lambda p: tok(p, truncation=True, max_length=77, return_tensors="pt")) if tok is not None \
        else (lambda p: hash_tokenize(p, vocab))
    return model, tokenize, "bpe" if tok is not None else "hash"


def rank_by_mean(scores: Sequence[Sequence[float]]):
    """-> (per-image means, image ids from the best mean to the worst; ties keep the id order)."""
    means = [sum(v) / len(v) if len(v) else float("-inf") for v in scores]
    return means, sorted(range(len(means)), key=lambda i: -means[i])


class InstanceClipScorer:
    """``tokenize``: phrase -> ids [1, L] (a tensor, or what ``CLIPTokenizer(text, return_tensors="pt")`` returns)."""

    def __init__(self, clip_model, tokenize: Callable, backend: str = "hf", dtype: torch.dtype = torch.bfloat16, ops=None):
        if backend not in BACKENDS:
            raise ValueError(f"InstanceClipScorer backend must be one of {BACKENDS}, got '{backend}'")
        self.model, self.tokenize, self.backend = clip_model, tokenize, backend
        self.size = int(clip_model.config.vision_config.image_size)
        self._vision = self._text = None
        self._phrase_cache = {}                                # phrase -> un-normalised fp32 text features [P] (the batched path)
        self._lut = None
        if backend == "hip":
            from ..clip_engine import CLIPTextEngine, CLIPVisionEngine      # raise without libidf_gfx950.so / a GPU: no fallback
            self._vision = CLIPVisionEngine(clip_model.vision_model, ops=ops, dtype=dtype, visual_projection=clip_model.visual_projection)
            self._text = CLIPTextEngine(clip_model.text_model, ops=self._vision.ops, text_projection=clip_model.text_projection)

    def _ids(self, phrase: str) -> torch.Tensor:
        ids = self.tokenize(phrase)
        if not isinstance(ids, torch.Tensor):
            ids = ids["input_ids"]
        return torch.as_tensor(ids).view(1, -1).long()

    @torch.no_grad()
    def image_features(self, crops: list) -> torch.Tensor:
        """PIL crops -> un-normalised fp32 features [N, P] on the CPU."""
        px = torch.stack([preprocess(c, self.size) for c in crops])
        if self.backend == "hip":
            return self._vision.image_features(px).float().cpu()
        dev = next(self.model.parameters()).device
        return _features(self.model.get_image_features(pixel_values=px.to(dev))).float().cpu()

    @torch.no_grad()
    def text_features(self, phrases: Sequence[str]) -> torch.Tensor:
        """Phrases -> un-normalised fp32 features [N, P] on the CPU (one call per phrase: the ids are not padded)."""
        out = []
        for ph in phrases:
            ids = self._ids(ph)
            if self.backend == "hip":
                out.append(self._text.text_features(ids).float().cpu())
            else:
                dev = next(self.model.parameters()).device
                out.append(_features(self.model.get_text_features(input_ids=ids.to(dev))).float().cpu())
        return torch.cat(out, 0)

    def score(self, image, boxes_xyxy_norm, phrases: Sequence[str]) -> List[float]:
        """The local CLIP score of every instance: cos(image features of its crop, text features of its phrase)."""
        if len(boxes_xyxy_norm) != len(phrases):
            raise ValueError("one phrase per box")
        img = normalise(self.image_features(crop_instances(image.convert("RGB"), boxes_xyxy_norm)))
        txt = normalise(self.text_features(phrases))
        return [float(v) for v in (img * txt).sum(-1)]

    def attribute_accuracy(self, image, boxes_xyxy_norm, phrases: Sequence[str], label_prompts: Sequence[str] = COLOR_LIST,
                           label_features: Optional[torch.Tensor] = None) -> List[int]:
        """1 per instance whose crop is closest to the "a {word} object" prompt of its phrase's first word, else 0;
        ``label_prompts``: the words (``COLOR_LIST`` / ``TEXTURE_LIST``)."""
        labels = list(label_prompts)
        gt = torch.tensor([labels.index(ph.split(" ")[0]) for ph in phrases])
        if label_features is None:
            label_features = normalise(self.text_features([LABEL_PROMPT.format(w) for w in labels]))
        img = normalise(self.image_features(crop_instances(image.convert("RGB"), boxes_xyxy_norm)))
        return [int(v) for v in (predict_attribute(img, label_features) == gt)]

    # ---- the batched path ------------------------------------------------------------------------------------------------------
    @staticmethod
    def _per_image(sets, B: int, what: str) -> list:
        """One set for the whole batch (a list of boxes / phrases) or a list of B sets -> a list of B sets."""
        sets = list(sets)
        shared = len(sets) == 0 or isinstance(sets[0], str) or not hasattr(sets[0][0], "__len__")
        if shared:
            return [sets] * B
        if len(sets) != B:
            raise ValueError(f"{what}: one set for the batch or one per image ({B}), got {len(sets)} sets")
        return [list(x) for x in sets]

    def _as_pil(self, images) -> list:
        from PIL import Image
        if not isinstance(images, torch.Tensor):
            return [im.convert("RGB") for im in images]
        arr = images.cpu().numpy() if images.dtype == torch.uint8 else quantise_images(images)
        return [Image.fromarray(a) for a in arr]

    def _as_device_batch(self, images) -> torch.Tensor:
        """-> uint8 [B, H, W, 3] or fp32 [B, 3, H, W], contiguous on the engine's device."""
        import numpy as np
        if not isinstance(images, torch.Tensor):
            arrs = [np.asarray(im.convert("RGB"), dtype=np.uint8) for im in images]
            if len({a.shape for a in arrs}) != 1:
                raise ValueError("score_batch on backend 'hip' needs images of one size")
            images = torch.from_numpy(np.stack(arrs))
        ok = (images.dtype == torch.uint8 and images.dim() == 4 and images.shape[-1] == 3) or \
             (images.dtype == torch.float32 and images.dim() == 4 and images.shape[1] == 3)
        if not ok:
            raise ValueError(f"images: uint8 [B, H, W, 3] or fp32 [B, 3, H, W], got {images.dtype} {tuple(images.shape)}")
        return images.to(self._vision.device).contiguous()

    @torch.no_grad()
    def pixels_batch(self, images, boxes) -> torch.Tensor:
        """The image tower's input for every crop of every image, fp32 [sum N_b, 3, S, S], image-major.  ``hip``: one table build, one
        upload and one ``idf_clip_crop_resize`` launch, on the device; ``hf``: ``crop_instances`` + ``preprocess`` per crop, on the CPU."""
        S = self.size
        if self.backend != "hip":
            pil = self._as_pil(images)
            per = self._per_image(boxes, len(pil), "boxes")
            return torch.stack([preprocess(c, S) for im, bx in zip(pil, per) for c in crop_instances(im, bx)])
        src = self._as_device_batch(images)
        B = src.shape[0]
        H, W = (src.shape[1], src.shape[2]) if src.dtype == torch.uint8 else (src.shape[2], src.shape[3])
        per = self._per_image(boxes, B, "boxes")
        shared = crop_rects(per[0], W, H) if all(p is per[0] for p in per) else None
        rects, index = [], []
        for b in range(B):
            r = shared if shared is not None else crop_rects(per[b], W, H)
            rects += r
            index += [b] * len(r)
        crops, blob, ntab, K = pack_crop_tables(rects, index, S)
        ops = self._vision.ops
        if self._lut is None:
            self._lut = pixel_lut().to(ops.device)
        tables = torch.from_numpy(blob).to(ops.device)
        out = torch.empty((len(rects), 3, S, S), dtype=torch.float32, device=ops.device)
        return ops.clip_crop_resize(src, crops, tables, ntab, self._lut, out, K)

    @torch.no_grad()
    def image_features_batch(self, images, boxes) -> torch.Tensor:
        """-> un-normalised fp32 features [sum N_b, P] on the CPU.  ``hip``: one tower call over all crops (the engine cuts it into
        its ``max_batch`` chunks).  ``hf``: one ``get_image_features`` per image, the very call ``score`` makes -- ``transformers``
        eager is not batch-invariant (the fp32 GEMMs pick their blocking by the row count: 1.5e-7 between 3 and 9 crops of the tiny
        model on a CPU), and this backend is the reference the batched scores are held to exactly."""
        px = self.pixels_batch(images, boxes)
        if self.backend == "hip":
            return self._vision.image_features(px).float().cpu()
        dev = next(self.model.parameters()).device
        counts = [len(p) for p in self._per_image(boxes, self._batch_size(images), "boxes")]
        return torch.cat([_features(self.model.get_image_features(pixel_values=part.to(dev))).float().cpu() for part in px.split(counts)])

    def text_features_cached(self, phrases: Sequence[str]) -> torch.Tensor:
        """``text_features``, each distinct phrase computed once per scorer."""
        for ph in phrases:
            if ph not in self._phrase_cache:
                self._phrase_cache[ph] = self.text_features([ph])[0]
        return torch.stack([self._phrase_cache[ph] for ph in phrases])

    def _batch_size(self, images) -> int:
        return int(images.shape[0]) if isinstance(images, torch.Tensor) else len(images)

    def score_batch(self, images, boxes, phrases) -> List[List[float]]:
        """``score`` for a batch: images uint8 [B, H, W, 3] / fp32 [B, 3, H, W] (decoder output in [-1, 1], quantised as
        ``inference.save_images`` does) / a list of PIL images; boxes and phrases: one set for the whole batch, or B sets.
        -> [B][N] scores."""
        B = self._batch_size(images)
        pb, pp = self._per_image(boxes, B, "boxes"), self._per_image(phrases, B, "phrases")
        if any(len(a) != len(b) for a, b in zip(pb, pp)):
            raise ValueError("one phrase per box")
        img = normalise(self.image_features_batch(images, boxes))
        txt = normalise(self.text_features_cached([ph for p in pp for ph in p]))
        flat = [float(v) for v in (img * txt).sum(-1)]
        out, i = [], 0
        for p in pp:
            out.append(flat[i:i + len(p)])
            i += len(p)
        return out

    def attribute_accuracy_batch(self, images, boxes, phrases, label_prompts: Sequence[str] = COLOR_LIST,
                                 label_features: Optional[torch.Tensor] = None) -> List[List[int]]:
        """``attribute_accuracy`` for a batch (the arguments of ``score_batch``): -> [B][N] of 0 / 1."""
        B = self._batch_size(images)
        pb, pp = self._per_image(boxes, B, "boxes"), self._per_image(phrases, B, "phrases")
        if any(len(a) != len(b) for a, b in zip(pb, pp)):
            raise ValueError("one phrase per box")
        labels = list(label_prompts)
        gt = torch.tensor([labels.index(ph.split(" ")[0]) for p in pp for ph in p])
        if label_features is None:
            label_features = normalise(self.text_features_cached([LABEL_PROMPT.format(w) for w in labels]))
        img = normalise(self.image_features_batch(images, boxes))
        flat = [int(v) for v in (predict_attribute(img, label_features) == gt)]
        out, i = [], 0
        for p in pp:
            out.append(flat[i:i + len(p)])
            i += len(p)
        return out
