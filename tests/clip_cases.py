"""Shared pieces of the CLIP text-engine tests (tests/test_clip_engine_emulated.py, tests/test_clip_engine_gpu.py) and of the golden
generator (tests/make_clip_engine_golden.py): the reduced config, its fixed ids, the fp32 emulation of the three ops the engine
adds to the op set, and the builders of the ``transformers`` module on key-seeded weights.  TEST INFRASTRUCTURE.
"""
from __future__ import annotations

import functools
import os

import torch

from tests.emul_ops import EmulOps

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# hidden 128 = 2 heads of 64, 2 layers; <|startoftext|> = 510, <|endoftext|> = 511 = the largest id.  eos_token_id = 2 is the value
# the hub's config.json of openai/clip-vit-large-patch14 carries (the pooled row is then the LARGEST id's; oracle/make_golden.py)
TINY_CONFIG = dict(vocab_size=512, hidden_size=128, intermediate_size=512, projection_dim=128, num_hidden_layers=2,
                   num_attention_heads=2, max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5,
                   pad_token_id=1, bos_token_id=0, eos_token_id=2)
TINY_SALT = 33
TINY_EOS_POSITIONS = (1, 10, 76)


def tiny_input_ids() -> torch.Tensor:
    """Three id rows shaped like the CLIP tokenizer's: 510, word ids, 511 at TINY_EOS_POSITIONS, padded with 511."""
    g = torch.Generator().manual_seed(78)
    ids = torch.full((3, 77), 511, dtype=torch.long)
    for r, p in enumerate(TINY_EOS_POSITIONS):
        ids[r, 0] = 510
        ids[r, 1:p] = torch.randint(3, 500, (p - 1,), generator=g)
    return ids


def rel_rms(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double().cpu(), b.double().cpu()
    return float(((a - b).pow(2).mean() / b.pow(2).mean().clamp_min(1e-30)).sqrt())


@functools.lru_cache(maxsize=None)
def load_golden(tag: str) -> dict:
    return torch.load(os.path.join(REPO, "tests", "golden", f"{tag}.pt"), weights_only=False)


def build_transformer(config: dict, schema: dict, salt: int):
    """``transformers.CLIPTextModel(config)`` in eval mode with the key-seeded weights of ``schema`` (the keys of the reference
    FrozenCLIPEmbedder's state dict, either ``transformers`` key layout)."""
    from transformers import CLIPTextConfig, CLIPTextModel
    from instancediffusion_amd import synth
    tr = CLIPTextModel(CLIPTextConfig(**config)).eval()
    nested_here = any(k.startswith("text_model.") for k in tr.state_dict())
    sd = {}
    for k, v in synth.synth_state_dict({k: tuple(v) for k, v in schema.items()}, salt).items():
        k = k[len("transformer."):]
        if k.startswith("text_model.") and not nested_here:
            k = k[len("text_model."):]
        elif not k.startswith("text_model.") and nested_here:
            k = "text_model." + k
        sd[k] = v
    res = tr.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys and all("position_ids" in k for k in res.missing_keys), res
    for p in tr.parameters():
        p.requires_grad = False
    return tr


def tiny_transformer():
    gold = load_golden("clip_engine_tiny")
    return build_transformer(gold["meta"]["config"], gold["schema"], gold["meta"]["salt"])


def full_transformer():
    """The full-size CLIP-L/14 text transformer on the weights of tests/golden/clip_text.pt (123 M parameters)."""
    gold = load_golden("clip_text")
    return build_transformer(gold["meta"]["hub_config"], gold["schema"], gold["meta"]["salt"])


def causal_attention_ref(qkv: torch.Tensor, B: int, T: int, H: int) -> torch.Tensor:
    """fp32 reference of idf_attention_causal on (already rounded) qkv [>= B*T, 3*H*64]: -> [B*T, H*64]."""
    C = H * 64
    out = torch.empty((B * T, C), dtype=torch.float32)
    mask = torch.ones(T, T, dtype=torch.bool).tril()
    for b in range(B):                                           # sequence by sequence: independent of what else is in the call
        x = qkv[b * T:(b + 1) * T].float()
        q, k, v = (x[:, i * C:(i + 1) * C].reshape(T, H, 64).transpose(0, 1) for i in range(3))
        s = (q @ k.transpose(1, 2)) * 64 ** -0.5
        p = torch.softmax(s.masked_fill(~mask, float("-inf")), -1)
        out[b * T:(b + 1) * T] = (p @ v).transpose(0, 1).reshape(T, C)
    return out


class ClipEmulOps(EmulOps):
    """EmulOps plus the three ops the CLIP text engine adds: ``gemm(act="quick_gelu")``, ``attention_causal``, ``clip_embed``."""

    def gemm(self, a, w, out, *, act=None, **kw):
        if act != "quick_gelu":
            return super().gemm(a, w, out, act=act, **kw)
        assert kw.get("res") is None and not kw.get("geglu") and kw.get("out_stats") is None      # IDF_EPI_QUICKGELU's combinations
        y = super().gemm(a, w, torch.empty(out.shape, dtype=torch.float32), **kw)
        out.copy_(y * torch.sigmoid(1.702 * y))
        return out

    def attention_causal(self, qkv, out, heads, T):
        self._count("attention_causal")
        B = out.shape[0] // T
        assert out.shape[-1] == heads * 64 and qkv.shape[-1] == 3 * heads * 64
        out[:B * T].copy_(causal_attention_ref(qkv, B, T, heads))
        return out

    def clip_embed(self, ids_i32, tok_emb, pos_emb, out):
        self._count("clip_embed")
        B, T = ids_i32.shape
        assert ids_i32.dtype == torch.int32
        ids = ids_i32.long().clamp(0, tok_emb.shape[0] - 1)
        out[:B * T].copy_((tok_emb.float()[ids] + pos_emb.float()[:T][None]).reshape(B * T, -1))
        return out
