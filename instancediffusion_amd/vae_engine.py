"""VAE executors for MI355X: ``AutoencoderKL.decode`` and ``AutoencoderKL.encode`` over the same C-ABI kernels.

``VAEDecoderEngine`` replaces ``ldm/models/autoencoder.py:32-36`` + ``Decoder.forward`` (``ldm/modules/diffusionmodules/model.py:534-568``),
``VAEEncoderEngine`` replaces ``autoencoder.py:27-31`` + ``Encoder.forward`` (``model.py:434-459``) + ``DiagonalGaussianDistribution``
(``ldm/modules/distributions/distributions.py:24-37``).  Design, following the UNet engine:
  * activations NHWC 16-bit for the whole network.  Decoder: the latent enters as fp32 NCHW (``idf_pointwise_nchw`` applies
    ``1/scale_factor`` and ``post_quant_conv``, ``idf_conv_in`` reads it), the image leaves as fp32 NCHW straight from the last conv's
    epilogue (``IDF_EPI_OUT_NCHW``).  Encoder: the image enters as fp32 NCHW through ``idf_conv_in``, conv_out leaves fp32 NCHW the same
    way and ``idf_vae_posterior`` does everything behind it (``quant_conv``, clamp, sample, ``scale_factor``) -- no layout permutes anywhere;
  * every 3x3 conv / 1x1 shortcut / projection is the MFMA GEMM / implicit-GEMM conv kernel, ``nearest x2`` is folded into the
    following conv's gather, the encoder's ``Downsample`` (pad right and bottom only, stride 2) is ``idf_conv3x3_down``,
    GroupNorm(eps 1e-6)+SiLU is the streaming two-launch kernel;
  * the mid-block attention is single-head with head dim = 512 (model.py:178-196), beyond the register budget of the
    flash kernels: scores = ONE batched MFMA GEMM with fp32 output, ``idf_softmax_rows`` normalises them into 16-bit
    probabilities, a second batched GEMM applies V^T.  The bias of the ``v`` 1x1 conv is added in that GEMM's epilogue
    (softmax rows sum to 1, so P.(V + 1 b^T) = P.V + 1 b^T exactly);
  * one decode / encode = a fixed launch sequence over static buffers, captured into a hipGraph per (batch, H, W).

Work (SD-1.5 KL-f8, 512x512 image <-> 64x64 latent): decoder 2514.5 GFLOP per image; the encoder about half of
that (tools/vae_bench.py --encode computes it from the packed layer shapes).
"""
from __future__ import annotations

import torch

from .engine_base import EngineBase


class _VAEEngine(EngineBase):
    """What the decoder and the encoder share on top of ``EngineBase`` (packing primitives, static buffers, graph replay): the
    packing of the res / attention blocks and the blocks themselves."""

    def __init__(self, vae, ops=None, dtype: torch.dtype = torch.bfloat16, use_graphs: bool = True):
        super().__init__(ops, dtype, use_graphs)
        self._pack(vae)

    # ---- weight packing ---------------------------------------------------------------------------------------
    def _pack_res(self, rb):
        return dict(cin=rb.in_channels, cout=rb.out_channels,
                    n1=(self._f32(rb.norm1.weight), self._f32(rb.norm1.bias)), conv1=self._conv(rb.conv1),
                    n2=(self._f32(rb.norm2.weight), self._f32(rb.norm2.bias)), conv2=self._conv(rb.conv2),
                    skip=self._lin(rb.nin_shortcut) if rb.in_channels != rb.out_channels else None)

    def _pack_attn(self, ab):
        C = ab.in_channels
        wq, wk = ab.q.weight.detach().reshape(C, C), ab.k.weight.detach().reshape(C, C)
        return dict(c=C, norm=(self._f32(ab.norm.weight), self._f32(ab.norm.bias)),
                    wqk=self._w16(torch.cat([wq, wk], 0)),
                    bqk=self._f32(torch.cat([ab.q.bias.detach(), ab.k.bias.detach()], 0)),
                    wv=self._w16(ab.v.weight.detach().reshape(C, C)), bv=self._f32(ab.v.bias),
                    proj=self._lin(ab.proj_out))

    def _pack(self, vae):
        raise NotImplementedError

    # ---- blocks -----------------------------------------------------------------------------------------------
    def _res(self, p, x, out_role):
        """ResnetBlock.forward (model.py:121-143), temb None."""
        ops = self.ops
        B, H, W, Cin = x.shape
        Cout = p["cout"]
        g = ops.groupnorm(x, self.buf("gn", x.shape), p["n1"][0], p["n1"][1], 1e-6, True)
        h1 = ops.conv3x3(g, p["conv1"].w, self.buf("h1", (B, H, W, Cout)), bias=p["conv1"].b)
        g2 = ops.groupnorm(h1, self.buf("gn", h1.shape), p["n2"][0], p["n2"][1], 1e-6, True)
        if p["skip"] is not None:
            xs = ops.gemm(x.view(B * H * W, Cin), p["skip"].w, self.buf("skip", (B * H * W, Cout)),
                          bias=p["skip"].b).view(B, H, W, Cout)
        else:
            xs = x
        return ops.conv3x3(g2, p["conv2"].w, self.buf(out_role, (B, H, W, Cout)), bias=p["conv2"].b, res=xs)

    def _attn(self, p, x, out_role):
        """AttnBlock.forward (model.py:178-202): softmax(q k^T / sqrt(C)) v over the H*W positions, one head."""
        ops = self.ops
        B, H, W, C = x.shape
        N, M = H * W, B * H * W
        assert N % 64 == 0, "the V^T GEMM needs H*W to be a multiple of 64"
        g = ops.groupnorm(x, self.buf("gn", x.shape), p["norm"][0], p["norm"][1], 1e-6, False)
        qk = ops.gemm(g.view(M, C), p["wqk"], self.buf("at.qk", (M, 2 * C)), bias=p["bqk"]).view(B, N, 2 * C)
        vt = ops.gemm(p["wv"], g.view(B, N, C), self.buf("at.vt", (B, C, N)))             # V^T[b] = Wv . X_b^T
        s = ops.gemm(qk[:, :, :C], qk[:, :, C:], self.buf("at.s", (B, N, N), torch.float32))
        pr = ops.softmax_rows(s, self.buf("at.p", (B, N, N)), float(C) ** -0.5)
        o = ops.gemm(pr, vt, self.buf("at.o", (B, N, C)), bias=p["bv"])                    # + b_v: rows of P sum to 1
        out = ops.gemm(o.view(M, C), p["proj"].w, self.buf(out_role, (M, C)), bias=p["proj"].b, res=x.view(M, C))
        return out.view(B, H, W, C)

    def _layers(self, h, cur, groups):
        """Run ("res" | "attn" | "up" | "down", packed) layers, ping-ponging between the activation roles "a" and "b"."""
        ops = self.ops
        for layers in groups:
            for kind, p in layers:
                nxt = "b" if cur == "a" else "a"
                if kind == "res":
                    h = self._res(p, h, nxt)
                elif kind == "attn":
                    h = self._attn(p, h, nxt)
                elif kind == "up":
                    Bq, Hq, Wq, C = h.shape
                    h = ops.conv3x3(h, p.w, self.buf(nxt, (Bq, 2 * Hq, 2 * Wq, C)), bias=p.b, upsample=1)
                else:
                    Bq, Hq, Wq, C = h.shape
                    h = ops.conv3x3_down(h, p.w, self.buf(nxt, (Bq, (Hq - 2) // 2 + 1, (Wq - 2) // 2 + 1, C)), bias=p.b)
                cur = nxt
        return h


class VAEDecoderEngine(_VAEEngine):
    def _pack(self, vae):
        dec = vae.decoder
        assert not dec.tanh_out, "tanh_out decoders are not used by any reference config"
        self.inv_scale = 1.0 / float(vae.scale_factor)
        pq = vae.post_quant_conv
        self.pq_w = self._f32(pq.weight.detach().reshape(pq.weight.shape[0], pq.weight.shape[1]))
        self.pq_b = self._f32(pq.bias)
        self.conv_in = (self._f32(dec.conv_in.weight), self._f32(dec.conv_in.bias))
        self.mid = [("res", self._pack_res(dec.mid.block_1)), ("attn", self._pack_attn(dec.mid.attn_1)),
                    ("res", self._pack_res(dec.mid.block_2))]
        self.levels = []
        for i_level in reversed(range(dec.num_resolutions)):
            up = dec.up[i_level]
            layers = []
            for i_block in range(dec.num_res_blocks + 1):
                layers.append(("res", self._pack_res(up.block[i_block])))
                if len(up.attn) > 0:
                    layers.append(("attn", self._pack_attn(up.attn[i_block])))
            if i_level != 0:
                layers.append(("up", self._conv(up.upsample.conv)))
            self.levels.append(layers)
        self.norm_out = (self._f32(dec.norm_out.weight), self._f32(dec.norm_out.bias))
        self.conv_out = self._conv_out_padded(dec.conv_out)
        self.n_out = dec.conv_out.weight.shape[0]
        self.up_factor = 2 ** (dec.num_resolutions - 1)

    def _decode_ops(self, z: torch.Tensor, img: torch.Tensor):
        """Enqueue one decode.  z [B, zc, H, W] fp32, img [B, 3, f*H, f*W] fp32."""
        ops = self.ops
        B, zc, H, W = z.shape
        z2 = ops.pointwise_nchw(z, self.pq_w, self.pq_b, self.buf("z.pq", (B, self.pq_w.shape[0], H, W), torch.float32),
                                self.inv_scale)
        h = ops.conv_in(z2, self.conv_in[0], self.conv_in[1], self.buf("a", (B, H, W, self.conv_in[0].shape[0])))
        h = self._layers(h, "a", [self.mid] + self.levels)
        g = ops.groupnorm(h, self.buf("gn", h.shape), self.norm_out[0], self.norm_out[1], 1e-6, True)
        ops.conv3x3(g, self.conv_out.w, img, bias=self.conv_out.b, n_valid=self.n_out)
        return img

    def decode(self, z: torch.Tensor) -> torch.Tensor:
        B, zc, H, W = z.shape
        f = self.up_factor
        z_s = self.buf("io.z", z.shape, torch.float32)
        img_s = self.buf("io.img", (B, self.n_out, f * H, f * W), torch.float32)
        z_s.copy_(z)
        self._replay((B, H, W), lambda: self._decode_ops(z_s, img_s))
        return img_s.clone()


class VAEEncoderEngine(_VAEEngine):
    """``AutoencoderKL.encode``: image [B, 3, H, W] fp32 -> (z, moments), the mirror of ``VAEDecoderEngine``."""

    def _pack(self, vae):
        enc = vae.encoder
        self.scale = float(vae.scale_factor)
        q = vae.quant_conv
        self.q_w = self._f32(q.weight.detach().reshape(q.weight.shape[0], q.weight.shape[1]))
        self.q_b = self._f32(q.bias)
        self.embed_dim = q.weight.shape[0] // 2
        self.conv_in = (self._f32(enc.conv_in.weight), self._f32(enc.conv_in.bias))
        self.levels = []
        for i_level in range(enc.num_resolutions):
            down = enc.down[i_level]
            layers = []
            for i_block in range(enc.num_res_blocks):
                layers.append(("res", self._pack_res(down.block[i_block])))
                if len(down.attn) > 0:
                    layers.append(("attn", self._pack_attn(down.attn[i_block])))
            if i_level != enc.num_resolutions - 1:
                layers.append(("down", self._conv(down.downsample.conv)))
            self.levels.append(layers)
        self.mid = [("res", self._pack_res(enc.mid.block_1)), ("attn", self._pack_attn(enc.mid.attn_1)),
                    ("res", self._pack_res(enc.mid.block_2))]
        self.norm_out = (self._f32(enc.norm_out.weight), self._f32(enc.norm_out.bias))
        self.conv_out = self._conv_out_padded(enc.conv_out)
        self.n_out = enc.conv_out.weight.shape[0]                       # 2 * z_channels
        self.down_factor = 2 ** (enc.num_resolutions - 1)

    def check_size(self, H: int, W: int):
        """Every Downsample halves an even size, and every attention (the mid block's, at H*W / factor^2 positions) needs a
        multiple of 64 positions for its V^T GEMM."""
        f = self.down_factor
        if H <= 0 or W <= 0 or H % f or W % f:
            raise ValueError(f"AutoencoderKL.encode: image size {H}x{W} must be a multiple of {f} in both directions")
        h, w = H, W
        for layers in self.levels + [self.mid]:
            for kind, _ in layers:
                if kind == "attn" and (h * w) % 64:
                    raise ValueError(
                        f"AutoencoderKL.encode: image size {H}x{W} gives an attention over {h}x{w} = {h * w} positions; the V^T GEMM "
                        f"needs a multiple of 64 (for the 4-level config: H and W multiples of 64)")
                if kind == "down":
                    h, w = h // 2, w // 2

    def _encode_ops(self, x: torch.Tensor, noise, z: torch.Tensor, moments: torch.Tensor):
        """Enqueue one encode.  x [B, 3, H, W] fp32, noise [B, E, H/f, W/f] fp32 or None, z likewise, moments [B, 2E, H/f, W/f]."""
        ops = self.ops
        B, _, H, W = x.shape
        h = ops.conv_in(x, self.conv_in[0], self.conv_in[1], self.buf("a", (B, H, W, self.conv_in[0].shape[0])))
        h = self._layers(h, "a", self.levels + [self.mid])
        g = ops.groupnorm(h, self.buf("gn", h.shape), self.norm_out[0], self.norm_out[1], 1e-6, True)
        ho = ops.conv3x3(g, self.conv_out.w, self.buf("enc.out", (B, self.n_out, h.shape[1], h.shape[2]), torch.float32),
                         bias=self.conv_out.b, n_valid=self.n_out)
        ops.vae_posterior(ho, self.q_w, self.q_b, noise, self.scale, z, moments)
        return z

    def encode(self, x: torch.Tensor, noise=None):
        """x [B, 3, H, W] fp32; noise [B, E, H/f, W/f] or None (the mode).  Returns (z, moments) -- z already times scale_factor,
        moments = mean | logvar clamped to [-30, 20], both fp32 on the engine's device."""
        B, _, H, W = x.shape
        self.check_size(H, W)
        f, E = self.down_factor, self.embed_dim
        x_s = self.buf("io.x", x.shape, torch.float32)
        z_s = self.buf("io.z", (B, E, H // f, W // f), torch.float32)
        m_s = self.buf("io.moments", (B, 2 * E, H // f, W // f), torch.float32)
        x_s.copy_(x)
        n_s = None
        if noise is not None:
            n_s = self.buf("io.noise", z_s.shape, torch.float32)
            n_s.copy_(noise)
        self._replay((B, H, W, noise is not None), lambda: self._encode_ops(x_s, n_s, z_s, m_s))
        return z_s.clone(), m_s.clone()
