"""Tensor-level wrappers over the C ABI (``include/idf.h``): derive pointers / leading dimensions / strides from
(possibly strided) torch views and enqueue the HIP kernel on torch's current stream.

PyTorch here is plumbing only (device memory + stream); every numeric op is a hand-written gfx950 kernel.
``HipOps()`` raises if the shared library is missing or no GPU is visible -- there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib
from ._lib import (EPI_BIAS, EPI_GATE, EPI_GEGLU, EPI_GEGLU_P32, EPI_GELU, EPI_LN_COL, EPI_LN_ROW, EPI_OUT_F32, EPI_OUT_NCHW,
                   EPI_QUICKGELU, EPI_RES, EPI_ROWBIAS, EPI_SILU)

_DT = {torch.bfloat16: _lib.IDF_BF16, torch.float16: _lib.IDF_F16}


def _p(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _rows2d(t: torch.Tensor):
    """(ld, batch_stride) of a [.., R, Ccols] view whose last dim is contiguous."""
    assert t.stride(-1) == 1 or t.shape[-1] == 1, "last dim must be contiguous"
    return t.stride(-2), (t.stride(0) if t.dim() == 3 else 0)


class HipOps:
    """The product backend.  One instance per compute dtype (bf16 default, fp16 supported by every kernel)."""

    def __init__(self, dtype: torch.dtype = torch.bfloat16, device: Optional[torch.device] = None):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("no MI355X visible: the InstanceDiffusion HIP path needs a GPU (no CPU fallback)")
        self.dtype = dtype
        self.dt = _DT[dtype]
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        self._ws = {}

    # ------------------------------------------------------------------------------------------------
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def _workspace(self, key, nfloats: int) -> torch.Tensor:
        """fp32 scratch keyed by (role, size): a buffer is NEVER reallocated or freed once handed out, because
        captured hipGraphs keep its raw device pointer."""
        k = (key, int(nfloats))
        w = self._ws.get(k)
        if w is None:
            w = torch.empty(int(nfloats), dtype=torch.float32, device=self.device)
            self._ws[k] = w
        return w

    SPLITK_WS_BYTES = 256 << 20

    def _splitk_ws(self) -> torch.Tensor:
        return self._workspace("splitk", self.SPLITK_WS_BYTES // 4)

    def empty(self, shape, dtype=None):
        return torch.empty(shape, dtype=dtype or self.dtype, device=self.device)

    def zeros(self, shape, dtype=None):
        return torch.zeros(shape, dtype=dtype or self.dtype, device=self.device)

    # ------------------------------------------------------------------------------------------------
    def gemm(self, a, w, out, *, bias=None, rowbias=None, rows_per_batch=0, res=None, gate=None,
             act: Optional[str] = None, geglu: bool = False, geglu_period: int = 64, ln_row=None, ln_col=None, out_stats=None, out_stats_eps=1e-5,
             ln_eps=1e-5, ln_stats_out=None, vt_out=None):
        """out[..,M,N] = epi(a[..,M,K] @ w[..,N,K]^T).  2-D or batched 3-D views; a/w may be shared (2-D) in a
        batched call.  geglu: ``w``/``bias`` are in the packed [P/2 value | P/2 gate] row order (``geglu_period`` P = 64 or 32,
        engine.pack_geglu), out has N/2 cols.
        ln_row = (stats [.., M, 2], c [N]): ``a`` is the RAW input of a LayerNorm whose gamma is folded into ``w`` and whose
        beta term travels in ``bias`` (include/idf.h IDF_EPI_LN_ROW).  ln_col = (stats [.., N, 2], c [M], d [M]): the same
        with the normalised operand on the ``w`` side (transposed-V projection).  out_stats [.., M, 2]: also emit (mu, rstd)
        of every output row for a LayerNorm that follows.  vt_out [N - out.shape[-1], >= M]: fused q | k | v projection --
        the product's columns beyond out's width are stored transposed there (include/idf.h)."""
        batched = out.dim() == 3
        M, K = a.shape[-2], a.shape[-1]
        N = w.shape[-2]
        assert w.shape[-1] == K
        lda, sA = _rows2d(a)
        ldw, sW = _rows2d(w)
        ldo, sO = _rows2d(out)
        epi = 0
        if bias is not None:
            epi |= EPI_BIAS
        if rowbias is not None:
            epi |= EPI_ROWBIAS
        ldr = sR = 0
        if res is not None:
            epi |= EPI_RES
            ldr, sR = _rows2d(res)
        if gate is not None:
            epi |= EPI_GATE
        if act == "silu":
            epi |= EPI_SILU
        elif act == "gelu":
            epi |= EPI_GELU
        elif act == "quick_gelu":
            epi |= EPI_QUICKGELU
        elif act is not None:
            raise ValueError(act)
        if geglu:
            epi |= EPI_GEGLU
            assert geglu_period in (32, 64)
            if geglu_period == 32:
                epi |= EPI_GEGLU_P32
            assert out.shape[-1] == N // 2
        elif vt_out is not None:
            assert not batched and out.shape[-2] == M and vt_out.shape[0] == N - out.shape[-1] and vt_out.shape[1] >= M
            assert vt_out.stride(1) == 1 and vt_out.dtype == self.dtype
        else:
            assert out.shape[-1] == N and out.shape[-2] == M
        if out.dtype == torch.float32:
            epi |= EPI_OUT_F32
        ln_stats = ln_c = ln_d = None
        s_ln = 0
        if ln_row is not None:
            ln_stats, ln_c = ln_row                     # ln_stats None: the GEMM computes the row statistics itself
            assert bias is not None and ln_c.numel() == N
            assert ln_stats is None or (ln_stats.shape[-2] == M and ln_stats.dtype == torch.float32)
            if ln_stats is None:
                assert not batched
                if ln_stats_out is not None:
                    assert ln_stats_out.is_contiguous() and ln_stats_out.dtype == torch.float32 and ln_stats_out.numel() == 2 * M
            epi |= EPI_LN_ROW
        elif ln_col is not None:
            ln_stats, ln_c, ln_d = ln_col
            assert ln_stats.shape[-2] == N and ln_c.numel() == M and ln_d.numel() == M and ln_stats.dtype == torch.float32
            epi |= EPI_LN_COL
        if ln_stats is not None:
            assert ln_stats.is_contiguous() and ln_stats.shape[-1] == 2
            s_ln = ln_stats.stride(0) if (batched and ln_stats.dim() == 3) else 0
        if out_stats is not None:
            assert out_stats.is_contiguous() and out_stats.dtype == torch.float32 and out_stats.numel() == 2 * out.numel() // N
        args = _lib.GemmArgs(
            A=a.data_ptr(), W=w.data_ptr(), out=out.data_ptr(),
            bias=None if bias is None else bias.data_ptr(),
            rowbias=None if rowbias is None else rowbias.data_ptr(),
            res=None if res is None else res.data_ptr(),
            gate=None if gate is None else gate.data_ptr(),
            M=M, N=N, K=K, lda=lda, ldw=ldw, ldo=ldo, ldr=ldr,
            ld_rowbias=0 if rowbias is None else rowbias.stride(-2), rows_per_batch=rows_per_batch,
            batch=out.shape[0] if batched else 1, strideA=sA, strideW=sW, strideO=sO, strideR=sR,
            epi=epi, dtype=self.dt, ws=self._splitk_ws().data_ptr(), ws_bytes=self.SPLITK_WS_BYTES,
            ln_stats=None if ln_stats is None else ln_stats.data_ptr(), stride_ln_stats=s_ln,
            ln_c=None if ln_c is None else ln_c.data_ptr(), ln_d=None if ln_d is None else ln_d.data_ptr(),
            out_stats=None if out_stats is None else out_stats.data_ptr(), out_stats_eps=float(out_stats_eps),
            ln_eps=float(ln_eps), ln_stats_out=None if ln_stats_out is None else ln_stats_out.data_ptr(),
            vt_out=None if vt_out is None else vt_out.data_ptr(), ld_vt=0 if vt_out is None else vt_out.stride(0),
            vt_col0=0 if vt_out is None else out.shape[-1])
        _lib.check(self.lib.idf_gemm(C.byref(args), self._stream()), "idf_gemm")
        return out

    # permutation of the k index inside every 16-group of the fused MLP's second weight (include/idf.h idf_mlp_geglu): an
    # involution (it swaps positions 4..7 and 8..11)
    MLP_W2_PERM = (0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15)

    def proj_row_takes(self, M: int, C: int) -> bool:
        """Does idf_gemm run an N = K = C projection of M rows on proj320s_kernel (weights resident, rows streaming)?  Asks the
        library: its knobs (IDF_TUNE_PROJ_ROW, IDF_TUNE_GEMM_BIG) and its threshold for the current device."""
        if C != 320 or M % 32:
            return False
        min_m = self.lib.idf_get_stat(_lib.IDF_STAT_PROJ_ROW_MIN_M)
        return 0 < min_m <= M

    @staticmethod
    def mlp_supported(M: int, C: int) -> bool:
        """Shapes idf_mlp_geglu takes (the 64 x 64-latent blocks: C = 320, whole 128-row tiles)."""
        return C == 320 and M % 128 == 0

    @classmethod
    def mlp_pack(cls, w1p16, c1, d1, w2_16):
        """Operand images of idf_mlp_geglu from the period-32-packed first projection (16-bit weight, fp32 row sums c1 and
        bias / beta term d1) and the 16-bit second weight [C, 4C]: (cd [8C/64][128] fp32, w2p)."""
        n2 = c1.numel()
        cd = torch.cat([c1.float().view(n2 // 64, 64), d1.float().view(n2 // 64, 64)], dim=1).contiguous()
        perm = torch.tensor(cls.MLP_W2_PERM, device=w2_16.device)
        n, k = w2_16.shape
        w2p = w2_16.view(n, k // 16, 16).index_select(2, perm).reshape(n, k).contiguous()
        return cd, w2p

    def mlp_geglu(self, x, stats, w1, cd, w2p, b2, out, *, gate=None):
        """out = x + [gate *] FF(LN(x)) in one launch (idf_mlp_geglu); x / out [M, 320] views (may alias), stats [M, 2]."""
        M, Cc = x.shape
        assert self.mlp_supported(M, Cc) and out.shape == x.shape and x.stride(-1) == 1 and out.stride(-1) == 1
        assert stats.is_contiguous() and stats.dtype == torch.float32 and stats.numel() == 2 * M
        assert w1.shape == (8 * Cc, Cc) and w2p.shape == (Cc, 4 * Cc) and cd.is_contiguous() and cd.numel() == 16 * Cc
        assert w1.stride(-1) == 1 and w2p.stride(-1) == 1 and b2.dtype == torch.float32 and cd.dtype == torch.float32
        args = _lib.MlpArgs(x=x.data_ptr(), ldx=x.stride(0), ln_stats=stats.data_ptr(), w1=w1.data_ptr(), ldw1=w1.stride(0),
                            cd=cd.data_ptr(), w2p=w2p.data_ptr(), ldw2=w2p.stride(0), b2=b2.data_ptr(),
                            gate=None if gate is None else gate.data_ptr(), out=out.data_ptr(), ldo=out.stride(0), M=M, C=Cc,
                            dtype=self.dt)
        _lib.check(self.lib.idf_mlp_geglu(C.byref(args), self._stream()), "idf_mlp_geglu")
        return out

    @staticmethod
    def gn_partial_shape(B, HW, C):
        """Shape of the GroupNorm partial-statistics buffer a conv3x3 can fill for its output ([B, HW/64, 32, 2] fp32), or
        None when the output does not qualify (whole 64-row chunks per sample, 32 groups)."""
        return (B, HW // 64, 32, 2) if (HW % 64 == 0 and C % 32 == 0) else None

    def conv3x3(self, x, w, out, *, bias=None, rowbias=None, res=None, stride=1, upsample=0, n_valid=0, gn_partial=None):
        """x [B,H,W,Cin] view (channel-contiguous), w [Cout, 9*Cin]; out [B,Ho,Wo,Cout] 16-bit, or fp32 NCHW
        [B,n_valid,Ho,Wo] when ``n_valid`` > 0 (final conv).  ``gn_partial`` (fp32 [B, Ho*Wo/64, 32, 2], see
        ``gn_partial_shape``): filled with the GroupNorm partial statistics of the output, for ``groupnorm(.., partial=)``."""
        B, H, W_, Cin = x.shape
        assert x.stride(-1) == 1 and x.stride(1) == W_ * x.stride(2) and x.stride(0) == H * x.stride(1)
        Cout = w.shape[0]
        epi = 0
        if bias is not None:
            epi |= EPI_BIAS
        if rowbias is not None:
            epi |= EPI_ROWBIAS
        if res is not None:
            epi |= EPI_RES
        if n_valid:
            epi |= EPI_OUT_NCHW
            assert out.dtype == torch.float32 and out.is_contiguous()
            ldo = 0
        else:
            ldo = out.stride(2)
        args = _lib.ConvArgs(
            x=x.data_ptr(), W=w.data_ptr(), out=out.data_ptr(),
            bias=None if bias is None else bias.data_ptr(),
            rowbias=None if rowbias is None else rowbias.data_ptr(),
            res=None if res is None else res.data_ptr(),
            B=B, Hin=H, Win=W_, Cin=Cin, Cout=Cout, stride=stride, upsample=upsample,
            ldx=x.stride(2), ldo=ldo, ldr=0 if res is None else res.stride(2),
            ld_rowbias=0 if rowbias is None else rowbias.stride(-2), n_valid=n_valid, epi=epi, dtype=self.dt,
            ws=self._splitk_ws().data_ptr(), ws_bytes=self.SPLITK_WS_BYTES,
            gn_partial=None if gn_partial is None else gn_partial.data_ptr())
        if gn_partial is not None:
            assert gn_partial.dtype == torch.float32 and gn_partial.is_contiguous() and out.is_contiguous()
            assert tuple(gn_partial.shape) == self.gn_partial_shape(out.shape[0], out.shape[1] * out.shape[2], Cout)
        _lib.check(self.lib.idf_conv3x3(C.byref(args), self._stream()), "idf_conv3x3")
        return out

    def conv3x3_down(self, x, w, out, *, bias=None, res=None, gn_partial=None):
        """The VAE encoder's Downsample (``idf_conv3x3_down``): zero-pad right and bottom only, 3x3 stride 2.
        x [B,H,W,Cin] view (channel-contiguous), w [Cout, 9*Cin]; out [B,(H-2)//2+1,(W-2)//2+1,Cout] 16-bit."""
        B, H, W_, Cin = x.shape
        assert x.stride(-1) == 1 and x.stride(1) == W_ * x.stride(2) and x.stride(0) == H * x.stride(1)
        Cout = w.shape[0]
        assert tuple(out.shape) == (B, (H - 2) // 2 + 1, (W_ - 2) // 2 + 1, Cout) and out.stride(-1) == 1
        assert out.stride(1) == out.shape[2] * out.stride(2) and out.stride(0) == out.shape[1] * out.stride(1)
        epi = 0
        if bias is not None:
            epi |= EPI_BIAS
        if res is not None:
            epi |= EPI_RES
        args = _lib.ConvArgs(
            x=x.data_ptr(), W=w.data_ptr(), out=out.data_ptr(),
            bias=None if bias is None else bias.data_ptr(), rowbias=None,
            res=None if res is None else res.data_ptr(),
            B=B, Hin=H, Win=W_, Cin=Cin, Cout=Cout, stride=2, upsample=0,
            ldx=x.stride(2), ldo=out.stride(2), ldr=0 if res is None else res.stride(2),
            ld_rowbias=0, n_valid=0, epi=epi, dtype=self.dt,
            ws=self._splitk_ws().data_ptr(), ws_bytes=self.SPLITK_WS_BYTES,
            gn_partial=None if gn_partial is None else gn_partial.data_ptr())
        if gn_partial is not None:
            assert gn_partial.dtype == torch.float32 and gn_partial.is_contiguous() and out.is_contiguous()
            assert tuple(gn_partial.shape) == self.gn_partial_shape(out.shape[0], out.shape[1] * out.shape[2], Cout)
        _lib.check(self.lib.idf_conv3x3_down(C.byref(args), self._stream()), "idf_conv3x3_down")
        return out

    def conv_up2x(self, x, wf, out, *, bias=None) -> bool:
        """Nearest-x2 upsample + 3x3 conv with the upsample folded into the weights (``idf_conv_up2x_folded``): x [B,H,W,Cin] view
        (channel-contiguous), wf [4, Cout, 4*Cin] from ``engine.pack_conv_up2x``; out [B,2H,2W,Cout] 16-bit.  Returns False --
        nothing launched, ``out`` untouched -- when the native path does not take the shape; the caller then runs
        ``conv3x3(.., upsample=1)`` with the 3x3 image."""
        B, H, W_, Cin = x.shape
        assert x.stride(-1) == 1 and x.stride(1) == W_ * x.stride(2) and x.stride(0) == H * x.stride(1)
        Cout = wf.shape[1]
        assert tuple(wf.shape) == (4, Cout, 4 * Cin) and wf.is_contiguous() and wf.dtype == self.dtype
        assert tuple(out.shape) == (B, 2 * H, 2 * W_, Cout) and out.stride(-1) == 1 and out.dtype == self.dtype
        assert out.stride(1) == out.shape[2] * out.stride(2) and out.stride(0) == out.shape[1] * out.stride(1)
        args = _lib.ConvArgs(
            x=x.data_ptr(), W=wf.data_ptr(), out=out.data_ptr(), bias=None if bias is None else bias.data_ptr(),
            rowbias=None, res=None, B=B, Hin=H, Win=W_, Cin=Cin, Cout=Cout, stride=1, upsample=1,
            ldx=x.stride(2), ldo=out.stride(2), ldr=0, ld_rowbias=0, n_valid=0, epi=0 if bias is None else EPI_BIAS,
            dtype=self.dt, ws=None, ws_bytes=0, gn_partial=None)
        rc = self.lib.idf_conv_up2x_folded(C.byref(args), self._stream())
        if rc == _lib.E_UNSUPPORTED:
            return False
        _lib.check(rc, "idf_conv_up2x_folded")
        return True

    def conv3x3_skip(self, g2, w_packed, x, out, *, bias=None, gn_partial=None) -> bool:
        """ResBlock tail in one launch (``idf_conv3x3_skip``): out = conv3x3(g2) + Wskip . x + bias, the 1x1 shortcut as extra K-tiles
        of the conv.  g2 [B,H,W,C2] and x [B,H,W,Cx] views (channel-contiguous), w_packed [Cout, 9*C2 + Cx] from
        ``engine.pack_conv3x3_skip`` (conv taps, then the shortcut columns), bias fp32 [Cout] = the two biases summed; out
        [B,H,W,Cout] 16-bit; ``gn_partial`` as in ``conv3x3``.  Returns False -- nothing launched, ``out`` untouched -- when the
        persistent kernel does not take the launch; the caller then runs ``gemm`` + ``conv3x3(.., res=)``."""
        B, H, W_, C2 = g2.shape
        Cx, Cout = x.shape[-1], w_packed.shape[0]
        for t in (g2, x, out):
            assert t.shape[:3] == (B, H, W_) and t.dtype == self.dtype
            assert t.stride(-1) == 1 and t.stride(1) == W_ * t.stride(2) and t.stride(0) == H * t.stride(1)
        assert tuple(w_packed.shape) == (Cout, 9 * C2 + Cx) and w_packed.is_contiguous() and w_packed.dtype == self.dtype
        assert out.shape[-1] == Cout
        if bias is not None:
            assert bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == Cout
        if gn_partial is not None:
            assert gn_partial.dtype == torch.float32 and gn_partial.is_contiguous() and out.is_contiguous()
            assert tuple(gn_partial.shape) == self.gn_partial_shape(B, H * W_, Cout)
        args = _lib.ConvSkipArgs(
            g=g2.data_ptr(), x=x.data_ptr(), W=w_packed.data_ptr(), out=out.data_ptr(),
            bias=None if bias is None else bias.data_ptr(), B=B, H=H, Wd=W_, C2=C2, Cx=Cx, Cout=Cout,
            ldg=g2.stride(2), ldx=x.stride(2), ldo=out.stride(2), dtype=self.dt,
            ws=self._splitk_ws().data_ptr(), ws_bytes=self.SPLITK_WS_BYTES,
            gn_partial=None if gn_partial is None else gn_partial.data_ptr())
        rc = self.lib.idf_conv3x3_skip(C.byref(args), self._stream())
        if rc == _lib.E_UNSUPPORTED:
            return False
        _lib.check(rc, "idf_conv3x3_skip")
        return True

    def conv_in(self, x_nchw, w, bias, out):
        B, Cin, H, W_ = x_nchw.shape
        assert x_nchw.dtype == torch.float32 and x_nchw.is_contiguous() and out.is_contiguous()
        _lib.check(self.lib.idf_conv_in(_p(x_nchw), _p(w), _p(bias), _p(out), B, Cin, H, W_, out.shape[-1], self.dt,
                                        self._stream()), "idf_conv_in")
        return out

    def attention(self, q, k0, vt0, n0, out, heads, *, k1=None, vt1=None, n1=0, qbits=None, kbits0=None, kbits1=None):
        """q [B,Nq,C] view, k [B,n,C] view, vt [B,C,ld>=ceil64(n)], out [B,Nq,C] view.  Optional visibility mask:
        int32 words qbits [B,Nq], kbits0 [B,>=n0], kbits1 [B,>=n1] (see include/idf.h)."""
        if qbits is not None:
            for t in (qbits, kbits0) + ((kbits1,) if n1 else ()):
                assert t.dtype == torch.int32 and t.stride(-1) == 1 and t.dim() == 2
        B, Nq, Cc = q.shape
        d = Cc // heads
        a = _lib.AttnArgs(
            q=q.data_ptr(), ldq=q.stride(1), strideQ=q.stride(0), nq=Nq,
            k0=k0.data_ptr(), ldk0=k0.stride(1), strideK0=k0.stride(0),
            vt0=vt0.data_ptr(), ldv0=vt0.stride(1), strideV0=vt0.stride(0), n0=n0,
            k1=None if k1 is None else k1.data_ptr(), ldk1=0 if k1 is None else k1.stride(1),
            strideK1=0 if k1 is None else k1.stride(0),
            vt1=None if vt1 is None else vt1.data_ptr(), ldv1=0 if vt1 is None else vt1.stride(1),
            strideV1=0 if vt1 is None else vt1.stride(0), n1=n1,
            out=out.data_ptr(), ldo=out.stride(1), strideO=out.stride(0),
            B=B, H=heads, d=d, scale=float(d) ** -0.5, dtype=self.dt,
            qbits=None if qbits is None else qbits.data_ptr(), strideQb=0 if qbits is None else qbits.stride(0),
            kbits0=None if qbits is None else kbits0.data_ptr(), strideKb0=0 if qbits is None else kbits0.stride(0),
            kbits1=None if (qbits is None or not n1) else kbits1.data_ptr(),
            strideKb1=0 if (qbits is None or not n1) else kbits1.stride(0))
        _lib.check(self.lib.idf_attention(C.byref(a), self._stream()), "idf_attention")
        return out

    def attention_causal(self, qkv, out, heads, T):
        """Causal self-attention of the CLIP text transformer (``idf_attention_causal``): qkv [>= B*T, 3*C] view, columns q | k | v
        as the fused projection leaves them, rows b*T + t; out [>= B*T, C] view.  B = out.shape[0] // T; head dim C / heads."""
        Cc = out.shape[-1]
        B = out.shape[0] // T
        assert qkv.dim() == 2 and out.dim() == 2 and qkv.shape[-1] == 3 * Cc and qkv.shape[0] >= B * T and Cc % heads == 0
        assert qkv.stride(-1) == 1 and out.stride(-1) == 1 and qkv.dtype == self.dtype and out.dtype == self.dtype
        d = Cc // heads
        _lib.check(self.lib.idf_attention_causal(_p(qkv), qkv.stride(0), _p(out), out.stride(0), B, T, heads, d, float(d) ** -0.5,
                                                 self.dt, self._stream()), "idf_attention_causal")
        return out

    def clip_embed(self, ids_i32, tok_emb, pos_emb, out):
        """out[b*T + t] = tok_emb[ids[b, t]] + pos_emb[t] (``idf_clip_embed``): ids int32 [B, T] contiguous, 16-bit tables
        [vocab, C] / [>= T, C] contiguous, out [>= B*T, C] view.  Ids outside the table are clamped."""
        B, T = ids_i32.shape
        vocab, Cc = tok_emb.shape
        assert ids_i32.dtype == torch.int32 and ids_i32.is_contiguous() and tok_emb.is_contiguous() and pos_emb.is_contiguous()
        assert tok_emb.dtype == self.dtype and pos_emb.dtype == self.dtype and out.dtype == self.dtype
        assert pos_emb.shape[0] >= T and pos_emb.shape[1] == Cc and out.shape[0] >= B * T and out.shape[1] == Cc and out.stride(-1) == 1
        _lib.check(self.lib.idf_clip_embed(_p(ids_i32), _p(tok_emb), _p(pos_emb), _p(out), out.stride(0), B, T, Cc, vocab, self.dt,
                                           self._stream()), "idf_clip_embed")
        return out

    ATTENTION_QKV_TMAX = _lib.ATTENTION_QKV_TMAX

    def attention_qkv(self, qkv, out, heads, T):
        """Bidirectional self-attention of the CLIP image tower (``idf_attention_qkv``): the layout of ``attention_causal``, every
        query sees every key.  Head dim 64, T <= ``ATTENTION_QKV_TMAX``."""
        Cc = out.shape[-1]
        B = out.shape[0] // T
        assert qkv.dim() == 2 and out.dim() == 2 and qkv.shape[-1] == 3 * Cc and qkv.shape[0] >= B * T and Cc % heads == 0
        assert qkv.stride(-1) == 1 and out.stride(-1) == 1 and qkv.dtype == self.dtype and out.dtype == self.dtype
        d = Cc // heads
        _lib.check(self.lib.idf_attention_qkv(_p(qkv), qkv.stride(0), _p(out), out.stride(0), B, T, heads, d, float(d) ** -0.5,
                                              self.dt, self._stream()), "idf_attention_qkv")
        return out

    def clip_patchify(self, pixels, patch, cls_row, x, patch_size):
        """``idf_clip_patchify``: pixels fp32 [B, 3, S, S] contiguous -> patch [B*G*G, Kp] 16-bit view (G = S / patch_size, Kp = 3 P P
        rounded up to 64, column order c*P*P + ky*P + kx, pad columns zero), and the class rows x[b*(G*G + 1)] = cls_row [C]."""
        B, ch, S, S2 = pixels.shape
        G = S // patch_size
        Cc = cls_row.numel()
        assert ch == 3 and S == S2 and pixels.dtype == torch.float32 and pixels.is_contiguous()
        assert patch.dim() == 2 and patch.shape[0] >= B * G * G and patch.shape[1] == (3 * patch_size * patch_size + 63) // 64 * 64
        assert x.dim() == 2 and x.shape[0] >= B * (G * G + 1) and x.shape[1] == Cc and x.stride(-1) == 1 and patch.stride(-1) == 1
        assert patch.dtype == self.dtype and x.dtype == self.dtype and cls_row.dtype == self.dtype and cls_row.is_contiguous()
        _lib.check(self.lib.idf_clip_patchify(_p(pixels), _p(patch), patch.stride(0), _p(cls_row), _p(x), x.stride(0), B, S, patch_size,
                                              Cc, self.dt, self._stream()), "idf_clip_patchify")
        return patch

    CLIP_RESIZE_KMAX = _lib.CLIP_RESIZE_KMAX

    def clip_crop_resize(self, src, crops, tables, ntab, lut, out, K):
        """``idf_clip_crop_resize``: src uint8 [B, H, W, 3] or fp32 [B, 3, H, W] contiguous on the device; crops int32 numpy
        [Ncrop, 8] on the HOST (image, x0, y0, width, height, table set, 0, 0); tables int32 on the device (the packed blob of
        ``host.clip_score.pack_crop_tables``: crop records, bounds, tap-major coefficients of ``ntab`` table sets at K taps);
        lut fp32 [3, 256]; out fp32 [Ncrop, 3, S, S] contiguous.  Bit-identical to Pillow's crop + bicubic resize + CLIP normalisation."""
        import numpy as np
        if src.dtype == torch.uint8:
            kind, (B, H, W, ch) = _lib.IDF_CLIP_SRC_U8, src.shape
        else:
            kind, (B, ch, H, W) = _lib.IDF_CLIP_SRC_F32, src.shape
            assert src.dtype == torch.float32
        Ncrop, S = out.shape[0], out.shape[-1]
        assert ch == 3 and src.is_contiguous() and src.is_cuda and out.is_contiguous() and out.dtype == torch.float32
        assert tuple(out.shape) == (Ncrop, 3, S, S) and lut.dtype == torch.float32 and tuple(lut.shape) == (3, 256) and lut.is_contiguous()
        assert isinstance(crops, np.ndarray) and crops.dtype == np.int32 and crops.shape == (Ncrop, 8) and crops.flags.c_contiguous
        assert tables.dtype == torch.int32 and tables.is_contiguous() and tables.numel() >= Ncrop * 8 + ntab * (4 * S + 2 * K * S)
        _lib.check(self.lib.idf_clip_crop_resize(_p(src), kind, B, H, W, C.c_void_p(crops.ctypes.data), Ncrop, _p(tables), int(ntab),
                                                 _p(lut), _p(out), S, int(K), self._stream()), "idf_clip_crop_resize")
        return out

    def rle_decode_planes(self, table, dst_plane, out, area=None, zero=True):
        """``idf_rle_decode_planes``: ``table`` = ``host.masks.pack_masks(..)`` of the call's M jobs (host numpy arrays, validated
        there and checked against ``out`` here, then uploaded: a few hundred run ends per mask), ``dst_plane``: M ints, the plane of
        ``out`` fp32 [.., S, S] (contiguous, its leading dims flattened to P planes) that job m fills with its mask, decoded and
        nearest-resized to S x S, bit for bit ``host.masks.decode_rle_reference``.  ``zero``: clear ``out`` first, so that planes no
        job names are zero.  -> (out, area int32 [M] on the device: the ones each job wrote)."""
        import numpy as np
        ends, rb, re, hw = (np.ascontiguousarray(table[k]) for k in ("ends", "run_begin", "run_end", "src_hw"))
        dst = np.ascontiguousarray(np.asarray(dst_plane, dtype=np.int64))
        M, S = int(rb.shape[0]), int(out.shape[-1])
        P = out.numel() // (S * S) if S else 0
        if not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.dim() >= 2 and out.shape[-2] == S):
            raise ValueError("rle_decode_planes: out must be a contiguous fp32 [.., S, S] tensor on the device")
        if S < 1 or S % 4 or P * S * S >= 2 ** 31:
            raise ValueError(f"rle_decode_planes: S = {S} must be a positive multiple of 4 and out smaller than 2^31 elements")
        if not (ends.dtype == np.uint32 and rb.dtype == np.int32 and re.dtype == np.int32 and hw.dtype == np.int32):
            raise ValueError("rle_decode_planes: not a pack_masks table")
        if re.shape != (M,) or hw.shape != (M, 2) or dst.shape != (M,):
            raise ValueError(f"rle_decode_planes: {M} jobs need {M} run ranges, source sizes and destination planes")
        if M and (rb.min() < 0 or (rb > re).any() or re.max() > ends.size or dst.min() < 0 or dst.max() >= P or hw.min() < 1
                  or int(hw.max()) * S >= 2 ** 31 or len(set(dst.tolist())) != M):
            raise ValueError("rle_decode_planes: a run range, source size or destination plane is out of range, or a plane is named twice")
        if area is None:
            area = torch.zeros(M, dtype=torch.int32, device=out.device)
        else:
            assert area.is_cuda and area.dtype == torch.int32 and area.is_contiguous() and area.numel() == M
            area.zero_()
        if zero:
            out.zero_()
        if M == 0:
            return out, area
        ints = np.concatenate([rb, re, hw.reshape(-1), dst.astype(np.int32), ends.view(np.int32)])      # one upload
        dev = torch.from_numpy(ints).to(out.device)
        base, n_ends = dev.data_ptr(), int(ends.size)
        at = lambda k: C.c_void_p(base + 4 * k * M)                                                      # noqa: E731
        _lib.check(self.lib.idf_rle_decode_planes(C.c_void_p(base + 20 * M), n_ends, at(0), at(1), at(2), at(4), M, _p(out), P, S,
                                                  _p(area), self._stream()), "idf_rle_decode_planes")
        return out, area

    def groupnorm(self, x, out, gamma, beta, eps, silu, partial=None):
        """x/out [B, HW, C] (or [B,H,W,C]) contiguous.  ``partial``: the statistics of x are already there ([B, nchunks, 32, 2]
        fp32 (mean, M2) per row chunk, as a conv3x3 leaves them): only the normalise pass runs."""
        assert x.is_contiguous() and out.is_contiguous()
        B, Cc = x.shape[0], x.shape[-1]
        HW = x.numel() // (B * Cc)
        if partial is not None:
            assert partial.dtype == torch.float32 and partial.is_contiguous() and partial.shape[0] == B and partial.shape[2:] == (32, 2)
            _lib.check(self.lib.idf_groupnorm_apply(_p(x), _p(out), _p(gamma), _p(beta), _p(partial), B, HW, Cc,
                                                    int(partial.shape[1]), float(eps), int(bool(silu)), self.dt,
                                                    self._stream()), "idf_groupnorm_apply")
            return out
        ws = self._workspace("gn", self.lib.idf_groupnorm_ws_floats(B, HW))
        _lib.check(self.lib.idf_groupnorm(_p(x), _p(out), _p(gamma), _p(beta), _p(ws), B, HW, Cc, float(eps),
                                          int(bool(silu)), self.dt, self._stream()), "idf_groupnorm")
        return out

    def layernorm(self, x, out, gamma, beta, eps=1e-5):
        """x/out [M, C] views (last dim contiguous)."""
        M, Cc = x.shape
        _lib.check(self.lib.idf_layernorm(_p(x), x.stride(0), _p(out), out.stride(0), _p(gamma), _p(beta), M, Cc,
                                          float(eps), self.dt, self._stream()), "idf_layernorm")
        return out

    def row_stats(self, x, stats, eps=1e-5):
        """stats[m] = (mean, rstd) of row m of x [M, C] (fp32 [M, 2]): the LayerNorm statistics a following gemm(ln_row /
        ln_col) applies in its epilogue."""
        M, Cc = x.shape
        assert stats.is_contiguous() and stats.dtype == torch.float32 and stats.numel() == 2 * M
        _lib.check(self.lib.idf_row_stats(_p(x), x.stride(0), _p(stats), M, Cc, float(eps), self.dt, self._stream()),
                   "idf_row_stats")
        return stats

    def layernorm_patch2(self, x, out, gamma, beta, eps):
        """x [B,H,W,C] contiguous; out [B*(H/2)*(W/2), >=4C] rows in 2x2 patch order."""
        B, H, W_, Cc = x.shape
        assert x.is_contiguous() and out.stride(-1) == 1
        _lib.check(self.lib.idf_layernorm_patch2(_p(x), _p(out), out.stride(0), _p(gamma), _p(beta), B, H, W_, Cc,
                                                 float(eps), self.dt, self._stream()), "idf_layernorm_patch2")
        return out

    def seg_in_conv(self, segs, w, bias, out):
        """segs fp32 [B,Cin,S,S]; out [B*(S/4)^2, ld>=48] 16-bit stem patch matrix."""
        B, Cin, S, _ = segs.shape
        assert segs.is_contiguous() and segs.dtype == torch.float32
        _lib.check(self.lib.idf_seg_in_conv(_p(segs), _p(w), _p(bias), _p(out), B, Cin, S, out.stride(0), self.dt,
                                            self._stream()), "idf_seg_in_conv")
        return out

    def dwconv7x7(self, x, w_tap_major, bias, out):
        B, H, W_, Cc = x.shape
        assert x.is_contiguous() and out.is_contiguous()
        _lib.check(self.lib.idf_dwconv7x7(_p(x), _p(w_tap_major), _p(bias), _p(out), B, H, W_, Cc, self.dt,
                                          self._stream()), "idf_dwconv7x7")
        return out

    def scaleu_concat(self, h, skip, out, hscale, sm1):
        B, H, W_, Ch = h.shape
        Cs = skip.shape[-1]
        assert h.is_contiguous() and skip.is_contiguous() and out.is_contiguous() and out.shape[-1] == Ch + Cs
        ws = self._workspace("scaleu", B * Cs * 64)
        _lib.check(self.lib.idf_scaleu_concat(_p(h), _p(skip), _p(out), _p(hscale), _p(sm1), _p(ws), B, H, W_, Ch, Cs,
                                              self.dt, self._stream()), "idf_scaleu_concat")
        return out

    def timestep_embedding(self, t_f32, out):
        B, dim = out.shape
        _lib.check(self.lib.idf_timestep_embedding(_p(t_f32), _p(out), B, dim, self.dt, self._stream()),
                   "idf_timestep_embedding")
        return out

    def unifusion_embed(self, text, loc, tmask, lmask, null_text, null_loc, freqs, out):
        rows, text_dim = text.shape
        D = loc.shape[-1]
        assert out.is_contiguous() and out.shape == (rows, text_dim + 32 * D)
        for t in (text, loc, tmask, lmask, null_text, null_loc, freqs):
            assert t.dtype == torch.float32 and t.is_contiguous()
        _lib.check(self.lib.idf_unifusion_embed(_p(text), _p(loc), _p(tmask), _p(lmask), _p(null_text), _p(null_loc),
                                                _p(freqs), _p(out), rows, text_dim, D, self.dt, self._stream()),
                   "idf_unifusion_embed")
        return out

    def cfg_combine(self, e_cond, e_uncond, guidance, out):
        _lib.check(self.lib.idf_cfg_combine(_p(e_cond), _p(e_uncond), float(guidance), _p(out), out.numel(),
                                            self._stream()), "idf_cfg_combine")
        return out

    def plms_update(self, x, e_t, old, e_next, mode, a_t, a_prev, sqrt_1m_at, out):
        e1 = old[-1] if len(old) >= 1 else None
        e2 = old[-2] if len(old) >= 2 else None
        e3 = old[-3] if len(old) >= 3 else None
        _lib.check(self.lib.idf_plms_update(_p(x), _p(e_t), _p(e1), _p(e2), _p(e3), _p(e_next), int(mode), float(a_t),
                                            float(a_prev), float(sqrt_1m_at), _p(out), out.numel(), self._stream()),
                   "idf_plms_update")
        return out

    def ddim_update(self, x, e_cond, e_uncond, guidance, a_t, a_prev, sigma_t, sqrt_1m_at, noise, out, pred_x0=None):
        """One DDIM step behind the forward (ddim.py:110-131): guidance (``e_uncond`` None: unguided), pred_x0, dir_xt and the
        noise term (``noise`` None: none, needs sigma_t == 0).  fp32, contiguous, all of ``out``'s size; ``out`` may be ``x``."""
        for t in (x, e_cond, out) + tuple(t for t in (e_uncond, noise, pred_x0) if t is not None):
            assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == out.numel()
        _lib.check(self.lib.idf_ddim_update(_p(x), _p(e_cond), _p(e_uncond), float(guidance), float(a_t), float(a_prev),
                                            float(sigma_t), float(sqrt_1m_at), _p(noise), _p(out), _p(pred_x0), out.numel(),
                                            self._stream()), "idf_ddim_update")
        return out

    def dpmpp_update(self, x, e_cond, e_uncond, guidance, sqrt_at, sqrt_1m_at, c_x, c_0, c_1, x0_last, out, x0_out):
        """One DPM-Solver++(2M) step behind the forward: guidance (``e_uncond`` None: unguided), x0_out = (x - sqrt_1m_at e) / sqrt_at,
        out = c_x x + c_0 x0_out (+ c_1 x0_last; ``x0_last`` None: order 1).  fp32, contiguous, all of ``out``'s size; ``out`` may be
        ``x``, ``x0_out`` may be ``x0_last``.  -> out."""
        for t in (x, e_cond, out, x0_out) + tuple(t for t in (e_uncond, x0_last) if t is not None):
            assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == out.numel()
        _lib.check(self.lib.idf_dpmpp_update(_p(x), _p(e_cond), _p(e_uncond), float(guidance), float(sqrt_at), float(sqrt_1m_at),
                                             float(c_x), float(c_0), float(c_1), _p(x0_last), _p(out), _p(x0_out), out.numel(),
                                             self._stream()), "idf_dpmpp_update")
        return out

    def q_sample_blend(self, x0, noise, mask, img, sqrt_ac, sqrt_1m_ac, out):
        """q_sample + the inpainting blend (ldm.py:17-20, ddim.py:94-98): out = (sqrt_ac x0 + sqrt_1m_ac noise) mask + (1 - mask) img.
        x0 / noise / img / out [B,C,H,W] fp32, mask [B,1,H,W] or [B,C,H,W]; ``out`` may be ``img``."""
        B, Cc = out.shape[0], out.shape[1]
        HW = out.numel() // (B * Cc)
        assert mask.dim() == out.dim() and mask.shape[0] == B and mask.shape[1] in (1, Cc) and mask.shape[2:] == out.shape[2:]
        for t in (x0, noise, img):
            assert t.shape == out.shape
        for t in (x0, noise, mask, img, out):
            assert t.dtype == torch.float32 and t.is_contiguous()
        _lib.check(self.lib.idf_q_sample_blend(_p(x0), _p(noise), _p(mask), _p(img), float(sqrt_ac), float(sqrt_1m_ac), _p(out),
                                               B, Cc, HW, int(mask.shape[1]), self._stream()), "idf_q_sample_blend")
        return out

    def q_sample(self, x0, noise, sqrt_ac, sqrt_1m_ac, out):
        """q_sample alone (ldm.py:17-20): out = sqrt_ac x0 + sqrt_1m_ac noise.  fp32, contiguous, all of ``out``'s size; ``out`` may be
        ``x0``."""
        for t in (x0, noise, out):
            assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == out.numel()
        _lib.check(self.lib.idf_q_sample(_p(x0), _p(noise), float(sqrt_ac), float(sqrt_1m_ac), _p(out), out.numel(), self._stream()),
                   "idf_q_sample")
        return out

    def resize_planes(self, src, dst, xi, xw, yi, yw):
        """``idf_resize_planes``: src [.., Hi, Wi] -> dst [.., Ho, Wo], fp32 contiguous with the same leading dimensions (the planes),
        no overlap.  Device tables of ``host.hires.resize_tables``: xi int32 [Wo], xw fp32 [Wo, taps], yi int32 [Ho], yw fp32 [Ho, taps],
        taps 2 or 4 (the kernel clamps every tap index)."""
        assert src.dim() >= 2 and dst.dim() == src.dim() and tuple(src.shape[:-2]) == tuple(dst.shape[:-2])
        Hi, Wi, Ho, Wo = int(src.shape[-2]), int(src.shape[-1]), int(dst.shape[-2]), int(dst.shape[-1])
        planes = src.numel() // max(Hi * Wi, 1)
        taps = int(xw.shape[-1])
        for t in (src, dst, xw, yw):
            assert t.dtype == torch.float32 and t.is_contiguous() and t.device == dst.device
        for t in (xi, yi):
            assert t.dtype == torch.int32 and t.is_contiguous() and t.device == dst.device
        assert tuple(xi.shape) == (Wo,) and tuple(xw.shape) == (Wo, taps) and tuple(yi.shape) == (Ho,) and tuple(yw.shape) == (Ho, taps)
        _lib.check(self.lib.idf_resize_planes(_p(src), _p(dst), _p(xi), _p(xw), _p(yi), _p(yw), taps, planes, Hi, Wi, Ho, Wo,
                                              self._stream()), "idf_resize_planes")
        return dst

    def ddim_update_units(self, x, e_cond, e_uncond, guidance, a_t, a_prev, sigma_t, sqrt_1m_at, noise, img_of, out, pred_x0=None):
        """``ddim_update`` over U work units whose step noise is one row per IMAGE: x / e_cond / e_uncond / out [U,C,H,W], noise
        [B,C,H,W] or None (needs sigma_t == 0), img_of: int32 [U] on the device (unit u reads noise[img_of[u]]; the kernel clamps the
        entries) or None when there is no noise or U == B.  ``out`` may be ``x``."""
        U = out.shape[0]
        chw = out.numel() // U
        for t in (x, e_cond, out) + tuple(t for t in (e_uncond, pred_x0) if t is not None):
            assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == out.numel()
        B = U
        if noise is not None:
            B = noise.shape[0]
            assert noise.dtype == torch.float32 and noise.is_contiguous() and noise.numel() == B * chw
        if img_of is not None:
            assert img_of.dtype == torch.int32 and img_of.is_contiguous() and img_of.numel() == U and img_of.device == out.device
        _lib.check(self.lib.idf_ddim_update_units(_p(x), _p(e_cond), _p(e_uncond), float(guidance), float(a_t), float(a_prev),
                                                  float(sigma_t), float(sqrt_1m_at), _p(noise), _p(img_of), _p(out), _p(pred_x0), U, B,
                                                  chw, self._stream()), "idf_ddim_update_units")
        return out

    def q_sample_blend_units(self, x0, noise, mask, img, img_of, sqrt_ac, sqrt_1m_ac, out):
        """``q_sample_blend`` over U work units: img / out [U,C,H,W]; x0 / noise [B,C,H,W] and mask [B,1,H,W] or [B,C,H,W] one row per
        IMAGE, unit u reads row img_of[u] (int32 [U] on the device; the kernel clamps the entries).  ``out`` may be ``img``."""
        U, Cc = out.shape[0], out.shape[1]
        B = x0.shape[0]
        HW = out.numel() // (U * Cc)
        assert img.shape == out.shape and noise.shape == x0.shape and tuple(x0.shape[1:]) == tuple(out.shape[1:])
        assert mask.dim() == out.dim() and mask.shape[0] == B and mask.shape[1] in (1, Cc) and mask.shape[2:] == out.shape[2:]
        for t in (x0, noise, mask, img, out):
            assert t.dtype == torch.float32 and t.is_contiguous()
        assert img_of.dtype == torch.int32 and img_of.is_contiguous() and img_of.numel() == U and img_of.device == out.device
        _lib.check(self.lib.idf_q_sample_blend_units(_p(x0), _p(noise), _p(mask), _p(img), _p(img_of), float(sqrt_ac), float(sqrt_1m_ac),
                                                     _p(out), U, B, Cc, HW, int(mask.shape[1]), self._stream()),
                   "idf_q_sample_blend_units")
        return out

    def mis_merge(self, lat, boxes_i32, out, mode):
        n1, B, Cc, H, W_ = lat.shape
        assert lat.is_contiguous() and out.is_contiguous()
        _lib.check(self.lib.idf_mis_merge(_p(lat), _p(boxes_i32), _p(out), n1 - 1, B, Cc, H, W_, int(mode),
                                          self._stream()), "idf_mis_merge")
        return out

    @staticmethod
    def check_unit_offsets(unit_off, B, U):
        """The offset table of ``mis_merge_ragged`` as a list of ints: B + 1 entries, starts at 0, strictly increasing (every image
        owns at least its global unit), ends at U.  ValueError otherwise -- the kernel only clamps what it loads."""
        off = [int(v) for v in (unit_off.tolist() if torch.is_tensor(unit_off) else unit_off)]
        if len(off) != B + 1 or off[0] != 0 or off[-1] != U or any(b <= a for a, b in zip(off, off[1:])):
            raise ValueError(f"mis_merge_ragged: unit offsets must be {B + 1} strictly increasing entries from 0 to {U}, got {off}")
        return off

    def mis_merge_ragged(self, lat, unit_off, boxes_i32, out, mode):
        """``idf_mis_merge`` over a ragged unit list.  lat [U,C,H,W] fp32 (unit latents, image after image, an image's global unit
        first), unit_off: B + 1 host ints (validated here, then uploaded), boxes_i32 [U,4] int32 on the device (mode 1) or None,
        out [B,C,H,W]."""
        U, Cc, H, W_ = lat.shape
        B = out.shape[0]
        assert lat.dtype == torch.float32 and out.dtype == torch.float32 and lat.is_contiguous() and out.is_contiguous()
        assert tuple(out.shape[1:]) == (Cc, H, W_)
        off = torch.tensor(self.check_unit_offsets(unit_off, B, U), dtype=torch.int32).to(self.device)
        if boxes_i32 is not None:
            assert boxes_i32.dtype == torch.int32 and boxes_i32.is_contiguous() and tuple(boxes_i32.shape) == (U, 4)
        _lib.check(self.lib.idf_mis_merge_ragged(_p(lat), _p(off), _p(boxes_i32), _p(out), B, U, Cc, H, W_, int(mode),
                                                 self._stream()), "idf_mis_merge_ragged")
        return out

    def cast16(self, x_f32, out):
        assert x_f32.is_contiguous() and out.is_contiguous()
        _lib.check(self.lib.idf_cast_f32_to_16(_p(x_f32), _p(out), out.numel(), self.dt, self._stream()),
                   "idf_cast_f32_to_16")
        return out

    def softmax_rows(self, s_f32, out, scale):
        """s_f32 [.., R, n] fp32 (rows stacked contiguously), out same shape 16-bit: out = softmax(scale * s, -1)."""
        assert s_f32.dtype == torch.float32 and s_f32.is_contiguous() and out.is_contiguous() and out.shape == s_f32.shape
        n = s_f32.shape[-1]
        rows = s_f32.numel() // n
        _lib.check(self.lib.idf_softmax_rows(_p(s_f32), _p(out), rows, n, n, n, float(scale), self.dt, self._stream()),
                   "idf_softmax_rows")
        return out

    def pointwise_nchw(self, x, w, bias, out, in_scale=1.0):
        """fp32 NCHW 1x1 conv between small channel counts: out = w @ (in_scale * x) + bias."""
        B, Cin = x.shape[0], x.shape[1]
        Cout = w.shape[0]
        HW = x.numel() // (B * Cin)
        for t in (x, w, out) + ((bias,) if bias is not None else ()):
            assert t.dtype == torch.float32 and t.is_contiguous()
        _lib.check(self.lib.idf_pointwise_nchw(_p(x), _p(w), _p(bias), _p(out), B, Cin, Cout, HW, float(in_scale),
                                               self._stream()), "idf_pointwise_nchw")
        return out

    def vae_posterior(self, h, w, bias, noise, scale, z, moments=None):
        """Everything of ``AutoencoderKL.encode`` behind the encoder's conv_out, fp32 NCHW: h [B,C2,H,W], w [2E,C2], bias [2E] or
        None, noise [B,E,H,W] or None (the mode); z [B,E,H,W] = (mean + exp(0.5 clamp(logvar)) * noise) * scale; ``moments``
        [B,2E,H,W] (optional) receives mean | clamped logvar."""
        B, C2 = h.shape[0], h.shape[1]
        E2 = w.shape[0]
        HW = h.numel() // (B * C2)
        assert E2 % 2 == 0 and tuple(w.shape) == (E2, C2) and tuple(z.shape) == (B, E2 // 2) + tuple(h.shape[2:])
        assert noise is None or noise.shape == z.shape
        assert moments is None or tuple(moments.shape) == (B, E2) + tuple(h.shape[2:])
        assert bias is None or tuple(bias.shape) == (E2,)
        for t in (h, w, z) + tuple(t for t in (bias, noise, moments) if t is not None):
            assert t.dtype == torch.float32 and t.is_contiguous()
        _lib.check(self.lib.idf_vae_posterior(_p(h), _p(w), _p(bias), _p(noise), float(scale), _p(z), _p(moments), B, C2, E2 // 2,
                                              HW, self._stream()), "idf_vae_posterior")
        return z
