"""Shared pieces of the CLIP image-tower tests (tests/test_clip_vision_emulated.py, tests/test_clip_vision_gpu.py) and of the golden
generator (tests/make_clip_vision_golden.py): the two configs, seeded inputs, the fp32 emulation of the two ops the tower adds to
the op set, the fp32 attention reference and the builders of the ``transformers`` modules on key-seeded weights.
TEST INFRASTRUCTURE.
"""
from __future__ import annotations

import copy
import functools

import torch

from tests import clip_cases
from tests.clip_cases import ClipEmulOps, load_golden, rel_rms  # noqa: F401  (re-exported)

# hidden 128 = 2 heads of 64, 2 layers, 56 / 14 -> 4 x 4 patches + class token: T = 17 (one 16-query tile and one query more)
TINY_VISION = dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, image_size=56, patch_size=14,
                   projection_dim=64, hidden_act="quick_gelu", layer_norm_eps=1e-5)
# ViT-L/14 at 224 px (openai/clip-vit-large-patch14): T = 257
FULL_VISION = dict(hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16, image_size=224,
                   patch_size=14, projection_dim=768, hidden_act="quick_gelu", layer_norm_eps=1e-5)
TINY_SALT, FULL_SALT, PROJ_SALT = 41, 42, 43
FULL_ROWS = (1, 2, 16, 17, 128, 129, 255, 256)              # the rows of last_hidden_state the golden keeps beside the class row
OUTPUTS = ("last_hidden_state", "pooler_output", "image_embeds")


def pixel_values(B: int, size: int, seed: int = 5) -> torch.Tensor:
    """Seeded inputs with the statistics of CLIP-normalised images (about unit variance, a per-channel offset)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn((B, 3, size, size), generator=g) + torch.tensor([0.3, -0.2, 0.1]).view(1, 3, 1, 1)


def _seed(module, salt):
    from instancediffusion_amd import synth
    sd = module.state_dict()
    module.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in sd.items() if v.is_floating_point()}, salt),
                           strict=False)
    for p in module.parameters():
        p.requires_grad = False
    return module.eval()


def build_vision(config: dict, salt: int):
    """``transformers.CLIPVisionModelWithProjection(config)`` in eval mode on key-seeded weights."""
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    return _seed(CLIPVisionModelWithProjection(CLIPVisionConfig(**config)), salt)


@functools.lru_cache(maxsize=None)
def tiny_vision():
    return build_vision(TINY_VISION, TINY_SALT)


@functools.lru_cache(maxsize=None)
def full_vision():
    return build_vision(FULL_VISION, FULL_SALT)


def build_clip_model(text_transformer=None, vision_config: dict = TINY_VISION, salt: int = PROJ_SALT, projection_dim=None):
    """``transformers.CLIPModel`` on key-seeded weights; with ``text_transformer`` (a ``CLIPTextModel`` of tests/clip_cases) its text
    tower is that module's config and weights, so only the projections and the image tower are new."""
    from transformers import CLIPConfig, CLIPModel
    text_config = dict(clip_cases.TINY_CONFIG) if text_transformer is None else text_transformer.config.to_dict()
    proj = int(projection_dim or vision_config["projection_dim"])
    model = _seed(CLIPModel(CLIPConfig(text_config=text_config, vision_config=dict(vision_config), projection_dim=proj)), salt)
    if text_transformer is not None:
        src = getattr(text_transformer, "text_model", text_transformer).state_dict()
        dst = getattr(model.text_model, "text_model", model.text_model)
        res = dst.load_state_dict(src, strict=False)
        assert not res.unexpected_keys and all("position_ids" in k for k in res.missing_keys), res
    return model


@functools.lru_cache(maxsize=None)
def tiny_clip_model():
    return build_clip_model(clip_cases.tiny_transformer())


@functools.lru_cache(maxsize=None)
def full_text_clip_model():
    """The full-size text transformer of tests/golden/clip_text.pt under key-seeded projections (and the tiny image tower)."""
    return build_clip_model(clip_cases.full_transformer())


def features(out) -> torch.Tensor:
    """``get_image_features`` / ``get_text_features`` return the tensor (transformers 4.x) or an output whose ``pooler_output`` is it."""
    return out if isinstance(out, torch.Tensor) else out.pooler_output


@torch.no_grad()
def vision_reference(model, px: torch.Tensor) -> dict:
    """The three outputs of a ``CLIPVisionModelWithProjection`` in the module's own dtype, as fp32."""
    vm = model.vision_model
    px = px.to(next(model.parameters()).dtype)
    out = vm(pixel_values=px)
    return dict(last_hidden_state=out.last_hidden_state.float(), pooler_output=out.pooler_output.float(),
                image_embeds=model.visual_projection(out.pooler_output).float())


@torch.no_grad()
def with_floors(model, fn):
    """-> (fn(model) in fp32, {dt: {name: rel-RMS of fn(a copy of the model cast to dt) against it}}); the model is not touched."""
    ref = fn(model)
    floors = {}
    for name, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        got = fn(copy.deepcopy(model).to(dt))
        floors[name] = {k: rel_rms(got[k].float(), ref[k]) for k in ref}
    return ref, floors


def full_attention_ref(qkv: torch.Tensor, B: int, T: int, H: int) -> torch.Tensor:
    """fp32 reference of idf_attention_qkv on (already rounded) qkv [>= B*T, 3*H*64]: -> [B*T, H*64]."""
    C = H * 64
    out = torch.empty((B * T, C), dtype=torch.float32)
    for b in range(B):
        x = qkv[b * T:(b + 1) * T].float()
        q, k, v = (x[:, i * C:(i + 1) * C].reshape(T, H, 64).transpose(0, 1) for i in range(3))
        p = torch.softmax((q @ k.transpose(1, 2)) * 64 ** -0.5, -1)
        out[b * T:(b + 1) * T] = (p @ v).transpose(0, 1).reshape(T, C)
    return out


def patchify_ref(px: torch.Tensor, P: int) -> torch.Tensor:
    """fp32 [B, 3, S, S] -> [B*G*G, 3*P*P] by ``unfold``: column c*P*P + ky*P + kx, row (b, gy, gx)."""
    return torch.nn.functional.unfold(px, kernel_size=P, stride=P).transpose(1, 2).reshape(-1, 3 * P * P)


class ClipVisionEmulOps(ClipEmulOps):
    """ClipEmulOps plus the two ops the image tower adds: ``attention_qkv`` and ``clip_patchify``."""

    ATTENTION_QKV_TMAX = 288

    def attention_qkv(self, qkv, out, heads, T):
        self._count("attention_qkv")
        B = out.shape[0] // T
        assert out.shape[-1] == heads * 64 and qkv.shape[-1] == 3 * heads * 64 and T <= self.ATTENTION_QKV_TMAX
        out[:B * T].copy_(full_attention_ref(qkv, B, T, heads))
        return out

    def clip_patchify(self, pixels, patch, cls_row, x, patch_size):
        self._count("clip_patchify")
        B, _, S, _ = pixels.shape
        G, k = S // patch_size, 3 * patch_size * patch_size
        assert pixels.dtype == torch.float32 and S % patch_size == 0 and patch.shape[1] == (k + 63) // 64 * 64
        patch[:B * G * G] = 0
        patch[:B * G * G, :k] = patchify_ref(pixels, patch_size).to(patch.dtype)
        x.view(-1, x.shape[-1])[0:B * (G * G + 1):G * G + 1] = cls_row
        return patch
