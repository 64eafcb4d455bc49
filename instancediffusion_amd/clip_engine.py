"""CLIP text-transformer executor for MI355X: ``FrozenCLIPEmbedder.forward``
(``ldm/modules/encoders/modules.py:144-172`` -> Hugging Face ``CLIPTextModel``) over the C-ABI kernels.

Design, following ``vae_engine.py``:
  * the hidden state is a 16-bit token-major matrix [B*T, C] for the whole network; ``idf_clip_embed`` writes it from the ids;
  * per layer five launches: the stacked q | k | v projection with LayerNorm 1 folded in (``IDF_EPI_LN_ROW``, the GEMM computes the
    row statistics itself) -> ``idf_attention_causal`` -> out-projection + residual -> fc1 with LayerNorm 2 folded in and the
    QuickGELU epilogue -> fc2 + residual.  Neither normalised activation ever exists in memory;
  * ``idf_layernorm`` applies ``final_layer_norm``; the pooled row is picked on the host from the ids, by the rule of the
    ``transformers`` module that was handed in (the first ``eos_token_id``, or the largest id for the legacy ``eos_token_id == 2``);
  * weights are packed once at construction, activations live in static buffers keyed by the chunk's sequence count, and a call
    is cut into chunks of at most ``max_batch`` sequences.  Sequences never interact, so chunking changes a result only through
    the GEMM kernel a row count selects (same values up to fp32 summation order; bit-equal where the chunks select the same
    kernels, which whole ``max_batch`` chunks do among themselves).

Nothing depends on the width or the depth beyond head dim 64 and C % 64 == 0.
"""
from __future__ import annotations

from typing import Dict

import torch

from .engine import _Lin


class CLIPTextEngine:
    def __init__(self, transformer_module, ops=None, dtype: torch.dtype = torch.bfloat16):
        if ops is None:
            from .ops import HipOps          # raises when libidf_gfx950.so / the GPU is missing: no fallback
            ops = HipOps(dtype)
        self.ops = ops
        self.dtype = ops.dtype
        self.device = ops.device
        self.max_batch = 64
        self._bufs: Dict[tuple, torch.Tensor] = {}
        self._pack(transformer_module)

    # ---- weight packing ---------------------------------------------------------------------------------------
    def _w16(self, t):
        return t.detach().to(device=self.device, dtype=torch.float32).to(self.dtype).contiguous()

    def _f32(self, t):
        return t.detach().to(device=self.device, dtype=torch.float32).contiguous()

    def _fold_ln(self, w, bias, norm):
        """``engine.UNetEngine._fold_ln``: -> (16-bit gamma-folded weight, c = its row sums as the MFMA sees them,
        d = W beta + bias)."""
        w = w.detach().float()
        g, b = norm.weight.detach().float(), norm.bias.detach().float()
        w16 = self._w16(w * g[None, :])
        return w16, w16.float().sum(1).contiguous(), self._f32(w @ b + bias.detach().float())

    def _lin(self, m) -> _Lin:
        return _Lin(self._w16(m.weight), self._f32(m.bias))

    def _pack(self, tr):
        tm = getattr(tr, "text_model", tr)               # transformers 4.x nests the transformer, >= 5 does not
        cfg = tr.config
        if cfg.hidden_act != "quick_gelu":
            raise RuntimeError(f"CLIPTextEngine: hidden_act '{cfg.hidden_act}' has no epilogue (quick_gelu only)")
        self.C, self.heads = int(cfg.hidden_size), int(cfg.num_attention_heads)
        if self.C != 64 * self.heads:
            raise RuntimeError(f"CLIPTextEngine: head dim {self.C // self.heads} is not 64")
        self.eps = float(cfg.layer_norm_eps)
        self.eos_token_id = int(getattr(tm, "eos_token_id", cfg.eos_token_id))
        emb = tm.embeddings
        self.tok, self.pos = self._w16(emb.token_embedding.weight), self._w16(emb.position_embedding.weight)
        self.layers = []
        for ly in tm.encoder.layers:
            a = ly.self_attn
            wqkv = torch.cat([a.q_proj.weight.detach(), a.k_proj.weight.detach(), a.v_proj.weight.detach()], 0)
            bqkv = torch.cat([a.q_proj.bias.detach(), a.k_proj.bias.detach(), a.v_proj.bias.detach()], 0)
            self.layers.append(dict(qkv=self._fold_ln(wqkv, bqkv, ly.layer_norm1), out=self._lin(a.out_proj),
                                    fc1=self._fold_ln(ly.mlp.fc1.weight, ly.mlp.fc1.bias, ly.layer_norm2), fc2=self._lin(ly.mlp.fc2)))
        self.inter = int(tm.encoder.layers[0].mlp.fc1.weight.shape[0])
        self.final = (self._f32(tm.final_layer_norm.weight), self._f32(tm.final_layer_norm.bias))

    # ---- buffers ----------------------------------------------------------------------------------------------
    def buf(self, role: str, shape, dtype=None) -> torch.Tensor:
        dtype = dtype or self.dtype
        key = (role, tuple(int(s) for s in shape), dtype)
        t = self._bufs.get(key)
        if t is None:
            t = self.ops.empty(key[1], dtype)
            self._bufs[key] = t
        return t

    # ---- forward ----------------------------------------------------------------------------------------------
    def _chunk(self, ids: torch.Tensor) -> torch.Tensor:
        """ids int32 [b, T] on the engine's device -> final-LayerNorm output, 16-bit [b*T, C] (a static buffer)."""
        ops = self.ops
        b, T = ids.shape
        M, C = b * T, self.C
        ids_s = self.buf(f"ids.{b}", (b, T), torch.int32)
        ids_s.copy_(ids)
        x, y = self.buf(f"x.{b}", (M, C)), self.buf(f"y.{b}", (M, C))
        qkv, att, h = self.buf(f"qkv.{b}", (M, 3 * C)), self.buf(f"att.{b}", (M, C)), self.buf(f"h.{b}", (M, self.inter))
        ops.clip_embed(ids_s, self.tok, self.pos, x)
        for p in self.layers:
            w, c, d = p["qkv"]
            ops.gemm(x, w, qkv, bias=d, ln_row=(None, c), ln_eps=self.eps)
            ops.attention_causal(qkv, att, self.heads, T)
            ops.gemm(att, p["out"].w, y, bias=p["out"].b, res=x)
            w, c, d = p["fc1"]
            ops.gemm(y, w, h, bias=d, ln_row=(None, c), ln_eps=self.eps, act="quick_gelu")
            ops.gemm(h, p["fc2"].w, x, bias=p["fc2"].b, res=y)
        return ops.layernorm(x, self.buf(f"z.{b}", (M, C)), self.final[0], self.final[1], self.eps)

    def pooled_index(self, ids: torch.Tensor) -> torch.Tensor:
        """The row ``CLIPTextModel`` pools: the first ``eos_token_id`` (the largest id with the legacy ``eos_token_id == 2``)."""
        ids = ids.to(torch.int)
        return (ids if self.eos_token_id == 2 else (ids == self.eos_token_id).int()).argmax(dim=-1)

    @torch.no_grad()
    def encode_ids(self, ids: torch.Tensor):
        """ids [B, T] integer -> (last_hidden_state fp32 [B, T, C], pooler_output fp32 [B, C]) on the engine's device."""
        if ids.dim() != 2 or ids.shape[0] < 1 or not 1 <= ids.shape[1] <= min(128, self.pos.shape[0]):
            raise ValueError(f"CLIPTextEngine.encode_ids expects ids [B, T <= {min(128, self.pos.shape[0])}], got {tuple(ids.shape)}")
        B, T = ids.shape
        idx = self.pooled_index(ids.cpu()).to(self.device)
        ids32 = ids.to(device=self.device, dtype=torch.int32)
        z = torch.empty((B, T, self.C), dtype=torch.float32, device=self.device)
        for i in range(0, B, self.max_batch):
            part = ids32[i:i + self.max_batch]
            z[i:i + part.shape[0]] = self._chunk(part).view(part.shape[0], T, self.C)
        return z, z[torch.arange(B, device=self.device), idx]
