"""Local CLIP score of a generated image against its instance prompts: the HF branch of the reference's
``eval/eval_attribute_binding.py:19-60,180-208``.  Every instance box is cropped out of the image, the crop's CLIP image features
and the phrase's CLIP text features are L2-normalised, and their dot product is the score; the attribute accuracy is the argmax of
the crop's features over eight "a {word} object" prompts (:54-59, :162-169).

``backend="hf"`` (the default) calls ``get_image_features`` / ``get_text_features`` of the ``transformers`` ``CLIPModel`` handed in,
unchanged.  ``backend="hip"`` runs both towers on the HIP kernels (``clip_engine.CLIPVisionEngine`` / ``CLIPTextEngine``, 16-bit
storage in ``dtype``); there is no fallback from it.  Not ported: the ``open_clip`` branch and the COCO loop around the metric.
"""
from __future__ import annotations

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


class InstanceClipScorer:
    """``tokenize``: phrase -> ids [1, L] (a tensor, or what ``CLIPTokenizer(text, return_tensors="pt")`` returns)."""

    def __init__(self, clip_model, tokenize: Callable, backend: str = "hf", dtype: torch.dtype = torch.bfloat16, ops=None):
        if backend not in BACKENDS:
            raise ValueError(f"InstanceClipScorer backend must be one of {BACKENDS}, got '{backend}'")
        self.model, self.tokenize, self.backend = clip_model, tokenize, backend
        self.size = int(clip_model.config.vision_config.image_size)
        self._vision = self._text = None
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
