"""What the UNet, VAE and CLIP executors share: the contract between packed weights, static buffers and hipGraph replay.

  * weights are packed ONCE at construction into HBM-resident 16-bit GEMM images and fp32 vectors (``_w16``, ``_f32``, ``_lin``,
    ``_conv``, ``_fold_ln``, ``_conv_out_padded``);
  * every activation lives in a static buffer keyed by ``(role, shape, dtype)`` (``buf``) that is never reallocated or freed;
  * a forward is a fixed launch sequence over those buffers: run eagerly once (which sizes every buffer), synchronize, capture
    once into a hipGraph per key, then replay (``_replay``).  An engine whose graphs read per-batch-size state drops them with
    ``_drop_graphs`` when that state is replaced.

This module imports nothing from ``engine.py``, ``host/`` or ``ldm/``: loading the CLIP or VAE engine does not load the UNet's.
"""
import contextlib
import gc

import torch


@contextlib.contextmanager
def capture_graph(graph):
    """``torch.cuda.graph(graph)`` with the cyclic garbage collector held off.  torch.cuda.graph no longer collects on entry, so a
    dead cycle from earlier work (a dropped model with its engine, graphs and events) could be finalised between two captured
    launches, and a finaliser that calls the runtime inside a capture aborts the process (seen in the GPU suite: ``Fatal Python
    error: Aborted`` while garbage-collecting inside the capture of a sampler test).  Collect before, keep the collector out."""
    gc.collect()
    was_on = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(graph):
            yield
    finally:
        if was_on:
            gc.enable()


def pack_conv3x3(w: torch.Tensor) -> torch.Tensor:
    """[Cout, Cin, 3, 3] -> [Cout, (ky*3+kx)*Cin + ci]  (K order of the implicit-GEMM gather)."""
    co, ci = w.shape[0], w.shape[1]
    return w.permute(0, 2, 3, 1).reshape(co, 9 * ci).contiguous()


class _Lin:
    __slots__ = ("w", "b")

    def __init__(self, w, b):
        self.w, self.b = w, b


class EngineBase:
    def __init__(self, ops=None, dtype: torch.dtype = torch.bfloat16, use_graphs: bool = False):
        if ops is None:
            from .ops import HipOps          # raises when libidf_gfx950.so / the GPU is missing: no fallback
            ops = HipOps(dtype)
        self.ops = ops
        self.dtype = ops.dtype
        self.device = ops.device
        self.use_graphs = use_graphs and self.device.type == "cuda"
        self._bufs = {}                      # (role, shape, dtype) -> static tensor
        self._graphs = {}                    # launch key -> captured graph

    # ---- weight packing (once; HBM-resident 16-bit GEMM images + fp32 vectors) ---------------------------------
    def _w16(self, t: torch.Tensor) -> torch.Tensor:
        return t.detach().to(device=self.device, dtype=torch.float32).to(self.dtype).contiguous()

    def _f32(self, t: torch.Tensor) -> torch.Tensor:
        return t.detach().to(device=self.device, dtype=torch.float32).contiguous()

    def _lin(self, m, with_bias=True) -> _Lin:
        w = m.weight
        if w.dim() == 4:
            w = w.reshape(w.shape[0], w.shape[1])            # 1x1 conv
        return _Lin(self._w16(w), self._f32(m.bias) if (with_bias and m.bias is not None) else None)

    def _conv(self, m) -> _Lin:
        return _Lin(self._w16(pack_conv3x3(m.weight.detach().float())), self._f32(m.bias))

    # LayerNorm -> Linear pairs are stored FOLDED (include/idf.h IDF_EPI_LN_ROW / LN_COL): the weight carries gamma,
    #   LN(x) W^T = rstd * (x (gamma*W)^T - mu * c) + d,   c = row sums of the 16-bit (gamma*W),   d = W beta (+ bias),
    # so the forward never materialises LN(x): a GEMM reads the raw residual stream and its epilogue applies (mu, rstd).
    def _fold_ln(self, w: torch.Tensor, bias, norm):
        """-> (16-bit gamma-folded weight, c [N] fp32 = its row sums as the MFMA sees them, d [N] fp32 = W beta + bias)."""
        w = w.detach().float()
        g, b = norm.weight.detach().float(), norm.bias.detach().float()
        w16 = self._w16(w * g[None, :])
        d = w @ b + (bias.detach().float() if bias is not None else 0.0)
        return w16, w16.float().sum(1).contiguous(), self._f32(d)

    def _conv_out_padded(self, oc) -> _Lin:
        """conv_out with few output channels: weights zero-padded to 64 rows (one N tile), the epilogue stores ``n_valid`` of them."""
        wpad = torch.zeros(64, oc.weight.shape[1], 3, 3)
        wpad[: oc.weight.shape[0]] = oc.weight.detach().float().cpu()
        bpad = torch.zeros(64)
        bpad[: oc.bias.shape[0]] = oc.bias.detach().float().cpu()
        return _Lin(self._w16(pack_conv3x3(wpad)), self._f32(bpad))

    # ---- buffers ----------------------------------------------------------------------------------------------
    def buf(self, role: str, shape, dtype=None, zero=False) -> torch.Tensor:
        """The static buffer of ``(role, shape, dtype)``, allocated (``zero``: zero-filled) the first time it is asked for.
        Invariant: a buffer handed out is never reallocated or freed while the engine lives -- captured graphs hold its raw
        pointer, so a replay would read and write memory the allocator may have given to someone else."""
        dtype = dtype or self.dtype
        key = (role, tuple(int(s) for s in shape), dtype)
        t = self._bufs.get(key)
        if t is None:
            t = (self.ops.zeros if zero else self.ops.empty)(key[1], dtype)
            self._bufs[key] = t
        return t

    # ---- graph replay -----------------------------------------------------------------------------------------
    def _replay(self, key, enqueue):
        """Run ``enqueue()`` -- a fixed launch sequence over static buffers -- eagerly, or as the hipGraph captured for ``key``."""
        if not self.use_graphs:
            enqueue()
            return
        graph = self._graphs.get(key)
        if graph is None:
            enqueue()                                  # eager warm-up sizes every buffer
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with capture_graph(graph):
                enqueue()
            self._graphs[key] = graph
        graph.replay()

    def _drop_graphs(self, B: int):
        """Forget every graph captured for batch size ``B`` (their keys start with it): what they read has been replaced."""
        for k in [k for k in self._graphs if k[0] == B]:
            del self._graphs[k]
