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

``CLIPVisionEngine`` is the image tower (``CLIPModel.get_image_features`` of ``eval/eval_attribute_binding.py:19-60``) on the same
code: the per-layer weights and the layer loop live in ``_CLIPEngine``, packing primitives and buffers in ``EngineBase``; the tower swaps ``idf_attention_causal`` for
``idf_attention_qkv`` and the embedding gather for ``idf_clip_patchify`` + one batched GEMM.
"""
from __future__ import annotations

import torch

from .engine_base import EngineBase


class _CLIPEngine(EngineBase):
    """What the two towers share on top of ``EngineBase`` (packing primitives with the LayerNorm fold, static buffers): the
    per-layer weights and the encoder-layer loop.  The towers run eagerly: they capture no graph."""

    NAME = "CLIP engine"

    def __init__(self, ops=None, dtype: torch.dtype = torch.bfloat16):
        super().__init__(ops, dtype, use_graphs=False)
        self.max_batch = 64

    # ---- weight packing ---------------------------------------------------------------------------------------
    def _pack_encoder(self, cfg, encoder):
        """The checks and the per-layer weights both towers need; sets C, heads, eps, layers, inter."""
        if cfg.hidden_act != "quick_gelu":
            raise RuntimeError(f"{self.NAME}: hidden_act '{cfg.hidden_act}' has no epilogue (quick_gelu only)")
        self.C, self.heads = int(cfg.hidden_size), int(cfg.num_attention_heads)
        if self.C != 64 * self.heads:
            raise RuntimeError(f"{self.NAME}: head dim {self.C // self.heads} is not 64")
        self.eps = float(cfg.layer_norm_eps)
        self.layers = []
        for ly in encoder.layers:
            a = ly.self_attn
            wqkv = torch.cat([a.q_proj.weight.detach(), a.k_proj.weight.detach(), a.v_proj.weight.detach()], 0)
            bqkv = torch.cat([a.q_proj.bias.detach(), a.k_proj.bias.detach(), a.v_proj.bias.detach()], 0)
            self.layers.append(dict(qkv=self._fold_ln(wqkv, bqkv, ly.layer_norm1), out=self._lin(a.out_proj),
                                    fc1=self._fold_ln(ly.mlp.fc1.weight, ly.mlp.fc1.bias, ly.layer_norm2), fc2=self._lin(ly.mlp.fc2)))
        self.inter = int(encoder.layers[0].mlp.fc1.weight.shape[0])

    # ---- the encoder layers -------------------------------------------------------------------------------------
    def _run_layers(self, x, y, b, T, attention):
        """x 16-bit [b*T, C] -> the last layer's output, in x again (y is scratch of the same shape); five launches per layer."""
        ops = self.ops
        M, C = b * T, self.C
        qkv, att, h = self.buf(f"qkv.{b}", (M, 3 * C)), self.buf(f"att.{b}", (M, C)), self.buf(f"h.{b}", (M, self.inter))
        for p in self.layers:
            w, c, d = p["qkv"]
            ops.gemm(x, w, qkv, bias=d, ln_row=(None, c), ln_eps=self.eps)
            attention(qkv, att, self.heads, T)
            ops.gemm(att, p["out"].w, y, bias=p["out"].b, res=x)
            w, c, d = p["fc1"]
            ops.gemm(y, w, h, bias=d, ln_row=(None, c), ln_eps=self.eps, act="quick_gelu")
            ops.gemm(h, p["fc2"].w, x, bias=p["fc2"].b, res=y)
        return x

    def _project(self, rows16, w, role):
        """rows16 16-bit [B, C] -> fp32 [B, P] = rows . w^T (``visual_projection`` / ``text_projection``: no bias), a fresh tensor."""
        B = rows16.shape[0]
        out = torch.empty((B, w.shape[0]), dtype=torch.float32, device=self.device)
        for i in range(0, B, self.max_batch):
            n = min(self.max_batch, B - i)
            a = self.buf(f"{role}.in.{n}", (n, self.C))
            a.copy_(rows16[i:i + n])
            out[i:i + n] = self.ops.gemm(a, w, self.buf(f"{role}.out.{n}", (n, w.shape[0]), torch.float32))
        return out


class CLIPTextEngine(_CLIPEngine):
    NAME = "CLIPTextEngine"

    def __init__(self, transformer_module, ops=None, dtype: torch.dtype = torch.bfloat16, text_projection=None):
        """``text_projection``: the weight [P, C] (or the bias-free ``nn.Linear``) of ``CLIPModel.text_projection``, for
        ``text_features``; without it nothing changes."""
        super().__init__(ops, dtype)
        self._pack(transformer_module)
        self.text_proj = None if text_projection is None else self._w16(getattr(text_projection, "weight", text_projection))

    def _pack(self, tr):
        tm = getattr(tr, "text_model", tr)               # transformers 4.x nests the transformer, >= 5 does not
        cfg = tr.config
        self._pack_encoder(cfg, tm.encoder)
        self.eos_token_id = int(getattr(tm, "eos_token_id", cfg.eos_token_id))
        emb = tm.embeddings
        self.tok, self.pos = self._w16(emb.token_embedding.weight), self._w16(emb.position_embedding.weight)
        self.final = (self._f32(tm.final_layer_norm.weight), self._f32(tm.final_layer_norm.bias))

    # ---- forward ----------------------------------------------------------------------------------------------
    def _chunk(self, ids: torch.Tensor) -> torch.Tensor:
        """ids int32 [b, T] on the engine's device -> final-LayerNorm output, 16-bit [b*T, C] (a static buffer)."""
        ops = self.ops
        b, T = ids.shape
        M, C = b * T, self.C
        ids_s = self.buf(f"ids.{b}", (b, T), torch.int32)
        ids_s.copy_(ids)
        x, y = self.buf(f"x.{b}", (M, C)), self.buf(f"y.{b}", (M, C))
        ops.clip_embed(ids_s, self.tok, self.pos, x)
        self._run_layers(x, y, b, T, ops.attention_causal)
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

    @torch.no_grad()
    def text_features(self, ids: torch.Tensor) -> torch.Tensor:
        """``CLIPModel.get_text_features``: ids [B, T] -> fp32 [B, P], the pooled row through ``text_projection`` (one idf_gemm)."""
        if self.text_proj is None:
            raise RuntimeError("CLIPTextEngine.text_features needs the text_projection weight (pass text_projection= at construction)")
        _, pooled = self.encode_ids(ids)
        return self._project(pooled.to(self.dtype), self.text_proj, "tproj")      # exact: pooled holds 16-bit values


class CLIPVisionEngine(_CLIPEngine):
    """``CLIPVisionModel`` (+ ``visual_projection``) on the HIP kernels: patchify + one batched GEMM (class row and position
    embedding included) -> ``pre_layrnorm`` -> the shared layers with ``idf_attention_qkv`` -> ``post_layernorm`` of the B class
    rows -> the projection GEMM with fp32 output."""

    NAME = "CLIPVisionEngine"

    def __init__(self, vision_module, ops=None, dtype: torch.dtype = torch.bfloat16, visual_projection=None):
        """``vision_module``: a ``transformers`` ``CLIPVisionModel`` / ``CLIPVisionModelWithProjection`` (its own
        ``visual_projection`` is used unless one is passed) or the bare ``CLIPVisionTransformer`` of a ``CLIPModel``."""
        super().__init__(ops, dtype)
        if visual_projection is None:
            visual_projection = getattr(vision_module, "visual_projection", None)
        self._pack(vision_module, visual_projection)

    def _pack(self, vm, proj):
        vt = getattr(vm, "vision_model", vm)
        cfg = vt.config if hasattr(vt, "config") else vm.config
        cfg = getattr(cfg, "vision_config", cfg)
        self._pack_encoder(cfg, vt.encoder)
        tmax = getattr(self.ops, "ATTENTION_QKV_TMAX", 288)
        self.S, self.P = int(cfg.image_size), int(cfg.patch_size)
        if self.S % self.P or self.P > 32:
            raise RuntimeError(f"CLIPVisionEngine: image size {self.S} / patch size {self.P} (needs S % P == 0, P <= 32)")
        self.G = self.S // self.P
        self.T = self.G * self.G + 1
        if self.T > tmax:
            raise RuntimeError(f"CLIPVisionEngine: T = {self.T} positions exceed idf_attention_qkv's {tmax}")
        if self.C > 1536:
            raise RuntimeError(f"CLIPVisionEngine: hidden size {self.C} exceeds the self-normalising LayerNorm fold's 1536")
        emb = vt.embeddings
        if getattr(emb.patch_embedding, "bias", None) is not None:
            raise RuntimeError("CLIPVisionEngine: a patch embedding with a bias is not CLIP's")
        k = 3 * self.P * self.P
        self.Kp = (k + 63) // 64 * 64
        w = torch.zeros((self.C, self.Kp), dtype=torch.float32)
        w[:, :k] = emb.patch_embedding.weight.detach().float().reshape(self.C, k).cpu()
        self.wpatch = self._w16(w)                                           # [C, Kp]: flattened c*P*P + ky*P + kx, zero-padded
        pos = emb.position_embedding.weight.detach().float()
        self.cls_row = self._w16(emb.class_embedding.detach().float().reshape(-1) + pos[0])
        self.pos_patch = self._w16(pos[1:])                                  # [G*G, C]: the residual of the patch GEMM
        pre = vt.pre_layrnorm if hasattr(vt, "pre_layrnorm") else vt.pre_layernorm      # (sic) the attribute name in transformers
        self.pre = (self._f32(pre.weight), self._f32(pre.bias))
        self.post = (self._f32(vt.post_layernorm.weight), self._f32(vt.post_layernorm.bias))
        self.vis_proj = None if proj is None else self._w16(getattr(proj, "weight", proj))

    def _chunk(self, pixels: torch.Tensor):
        """pixels fp32 [b, 3, S, S] on the device -> (last hidden state 16-bit [b*T, C], post-LayerNorm class rows 16-bit [b, C]),
        both static buffers."""
        ops = self.ops
        b, T, C, GG = pixels.shape[0], self.T, self.C, self.G * self.G
        px = self.buf(f"px.{b}", (b, 3, self.S, self.S), torch.float32)
        px.copy_(pixels)
        x, y = self.buf(f"x.{b}", (b * T, C)), self.buf(f"y.{b}", (b * T, C))
        patch = self.buf(f"patch.{b}", (b * GG, self.Kp))
        ops.clip_patchify(px, patch, self.cls_row, y, self.P)
        ops.gemm(patch.view(b, GG, self.Kp), self.wpatch, y.view(b, T, C)[:, 1:], res=self.pos_patch)
        ops.layernorm(y, x, self.pre[0], self.pre[1], self.eps)
        self._run_layers(x, y, b, T, ops.attention_qkv)
        pooled = ops.layernorm(x.view(b, T, C)[:, 0], self.buf(f"pool.{b}", (b, C)), self.post[0], self.post[1], self.eps)
        return x, pooled

    @torch.no_grad()
    def encode_pixels(self, pixel_values: torch.Tensor):
        """pixel_values [B, 3, S, S] -> (last_hidden_state fp32 [B, T, C], pooler_output fp32 [B, C], image_embeds fp32 [B, P] or
        None without a projection) on the engine's device."""
        if pixel_values.dim() != 4 or pixel_values.shape[0] < 1 or tuple(pixel_values.shape[1:]) != (3, self.S, self.S):
            raise ValueError(f"CLIPVisionEngine.encode_pixels expects pixel_values [B, 3, {self.S}, {self.S}], got {tuple(pixel_values.shape)}")
        B = pixel_values.shape[0]
        px = pixel_values.to(device=self.device, dtype=torch.float32)
        z = torch.empty((B, self.T, self.C), dtype=torch.float32, device=self.device)
        pooled = torch.empty((B, self.C), dtype=torch.float32, device=self.device)
        embeds = None if self.vis_proj is None else torch.empty((B, self.vis_proj.shape[0]), dtype=torch.float32, device=self.device)
        for i in range(0, B, self.max_batch):
            part = px[i:i + self.max_batch]
            n = part.shape[0]
            x, p16 = self._chunk(part)
            z[i:i + n] = x.view(n, self.T, self.C)
            pooled[i:i + n] = p16
            if embeds is not None:
                embeds[i:i + n] = self.ops.gemm(p16, self.vis_proj, self.buf(f"emb.{n}", (n, self.vis_proj.shape[0]), torch.float32))
        return z, pooled, embeds

    def image_features(self, pixel_values: torch.Tensor) -> torch.Tensor:
        """``CLIPModel.get_image_features``: -> fp32 [B, P]."""
        if self.vis_proj is None:
            raise RuntimeError("CLIPVisionEngine.image_features needs the visual_projection weight")
        return self.encode_pixels(pixel_values)[2]
