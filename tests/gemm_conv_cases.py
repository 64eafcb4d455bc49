"""Cases, input builders, fp64 references and the per-element bound for the matrix-core kernels behind ``idf_gemm``, ``idf_conv3x3`` and
``idf_conv3x3_down``: the small-tile kernels (with their split-K reducer), the latency ("ring") kernel and the persistent big-tile
kernel.  No GPU and no HIP library: tests/test_gemm_conv_refs.py proves this module on the CPU, tests/test_gemm_conv_edges_gpu.py
applies it to the kernels, tests/test_gemm_big_walk_gpu.py to the persistent kernel where a workgroup walks several work items (the
WALK_* cases and the mirror of the tile walk, at the end of this file).

The references are written directly in torch on fp64 and share no code with tests/emul_ops.py.  Each takes the kernel's own inputs
(the 16-bit tensors already rounded, the fp32 ones as they are) and upcasts them; each returns ``(want, slack)``.

The bound, per element, for a K-term dot product followed by one 16-bit rounding:

    |got - want| <= U[dt] * |want| + slack,      slack = K * 2^-24 * (|A| |W|^T)[m, n] * s + act_abs

U is the project's table (bf16 2^-7, fp16 2^-10; 2^-22 for an fp32 output).  K * 2^-24 * |A| |W|^T is the standard forward error bound of
an fp32 dot product: it holds for ANY summation order, so it covers split-K and the MFMA's internal order; it is computed in fp64 from
the actual operands (for the conv, over the gathered taps).  ``s`` is the factor the epilogue applies behind the accumulator: rstd of a
folded LayerNorm, the gate, and 1.13 >= |act'| for SiLU, erf-GELU and QuickGELU.  ``act_abs`` is the 2.6e-5 that csrc/common.h documents
for gelu_erf_f (times |value| for GEGLU), 0 otherwise.  A NaN is outside.  Tests require exactly 0 elements outside.
"""
import math

import torch
import torch.nn.functional as F

from tests.small_kernel_cases import DTYPES, RMS_BAR, RMS_MIN_ELEMS, U, gen, rel_rms, relmax   # noqa: F401  (re-exported)

EPS32 = 2.0 ** -24
U_F32 = 2.0 ** -22
ACT_SLOPE = 1.13
GELU_ABS = 2.6e-5
NUM_CU = 256                                             # MI355X: the dispatch rules below count workgroup slots
BK = 64
FAMILIES = {                                             # name -> (IDF_TUNE_GEMM_BIG, IDF_TUNE_GEMM_RING)
    "small": (0, 0),
    "ring": (0, 1 << 30),
    "big": (2, 0),
}


# ---- the bound -----------------------------------------------------------------------------------------------------------------
def outside(got, want64, slack, dt, f32out=False):
    """(number of elements outside the bound, largest error / bound).  A NaN in ``got`` is outside."""
    want = want64.detach().double().cpu()
    got = got.detach().double().cpu().reshape(want.shape)
    bound = (U_F32 if f32out else U[dt]) * want.abs() + slack.double().reshape(want.shape)
    err = (got - want).abs()
    bad = ~(err <= bound)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    return int(bad.sum()), float(ratio.max())


# ---- guarded output buffers ----------------------------------------------------------------------------------------------------
def guarded(shape, dtype, device="cpu", ld=None):
    """An output view of ``shape`` (rows of shape[-1] elements, leading dimension ``ld``) inside a NaN-filled buffer with spare rows
    in front and behind and the spare columns up to ``ld``: (view, check).  ``check()`` names where a guard element is no longer
    NaN ("front", "behind", "beside"), or returns "" when every one still is."""
    cols = shape[-1]
    ld = cols if ld is None else ld
    rows = 1
    for s in shape[:-1]:
        rows *= s
    spare = max(1, -(-256 // ld))                        # at least one row and at least 256 elements on either side
    buf = torch.full((rows + 2 * spare, ld), float("nan"), dtype=dtype, device=device)
    view = buf[spare:spare + rows, :cols]
    if len(shape) != 2:
        view = view.unflatten(0, tuple(shape[:-1]))

    def check():
        where = []
        if not bool(torch.isnan(buf[:spare]).all()):
            where.append("front")
        if not bool(torch.isnan(buf[spare + rows:]).all()):
            where.append("behind")
        if ld > cols and not bool(torch.isnan(buf[spare:spare + rows, cols:]).all()):
            where.append("beside")
        return " ".join(where)
    return view, check


# ---- fp64 references -----------------------------------------------------------------------------------------------------------
def _act(y, act):
    if act == "silu":
        return y * torch.sigmoid(y)
    if act == "gelu":
        return y * 0.5 * (1.0 + torch.erf(y / math.sqrt(2.0)))
    if act == "quick_gelu":
        return y * torch.sigmoid(1.702 * y)
    assert act is None, act
    return y


def gemm_ref(a, w, *, bias=None, rowbias=None, rows_per_batch=0, ln_row=None, ln_col=None, ln_eps=1e-5, act=None, geglu=False,
             res=None, gate=None, cd=torch.float64):
    """epi(a[.., M, K] @ w[.., N, K]^T) as include/idf.h defines it, computed in ``cd``; -> (want, slack).  ``geglu``: w / bias are the
    UNPACKED projection ([value rows | gate rows]); want = value * gelu(gate), N/2 columns.  ln_row = (stats [.., M, 2] or None, c [N]),
    ln_col = (stats [.., N, 2], c [M], d [M]) with the statistics as given (None: of a's rows, computed here)."""
    K = a.shape[-1]
    A, Wm = a.to(cd), w.to(cd)
    acc = A @ Wm.transpose(-1, -2)
    mag = a.double().abs() @ w.double().abs().transpose(-1, -2)
    s = torch.ones_like(mag)
    if ln_row is not None:
        st, c = ln_row
        if st is None:
            mu = A.mean(-1)
            rstd = 1.0 / ((A - mu[..., None]).pow(2).mean(-1) + ln_eps).sqrt()
        else:
            mu, rstd = st[..., 0].to(cd), st[..., 1].to(cd)
        acc = rstd[..., None] * (acc - mu[..., None] * c.to(cd))
        s = s * rstd.double().abs()[..., None]
    if ln_col is not None:
        st, c, d = ln_col
        mu, rstd = st[..., 0].to(cd).unsqueeze(-2), st[..., 1].to(cd).unsqueeze(-2)
        acc = rstd * (acc - c.to(cd)[:, None] * mu) + d.to(cd)[:, None]
        s = s * rstd.double().abs()
    if bias is not None:
        acc = acc + bias.to(cd)
    if geglu:
        n = acc.shape[-1] // 2
        v, g = acc[..., :n], acc[..., n:]
        want = v * _act(g, "gelu")
        slack = K * EPS32 * s[..., :n] * (mag[..., :n] * _act(g, "gelu").double().abs() + ACT_SLOPE * v.double().abs() * mag[..., n:]) \
            + GELU_ABS * v.double().abs()
        return want, slack
    if rowbias is not None:
        idx = torch.arange(acc.shape[-2], device=acc.device) // rows_per_batch
        acc = acc + rowbias.to(cd)[idx]
    slack = K * EPS32 * mag * s
    if act is not None:
        acc = _act(acc, act)
        slack = slack * ACT_SLOPE + (GELU_ABS if act == "gelu" else 0.0)
    if res is not None:
        g = 1.0 if gate is None else gate.to(cd)
        acc = res.to(cd) + g * acc
        slack = slack * (1.0 if gate is None else float(gate.double().abs()))
    return acc, slack


def conv_out_hw(H, W, stride, up, pad_lo):
    return ((H << up) + pad_lo - 2) // stride + 1, ((W << up) + pad_lo - 2) // stride + 1


def conv3x3_ref(x, w, *, bias=None, rowbias=None, res=None, stride=1, up=0, pad_lo=1, n_valid=0, cd=torch.float64, front=None,
                pad_mode="constant"):
    """3x3 conv of x [B, H, W, Cin] with the [Cout, 9*Cin] weight image (column (ky*3 + kx)*Cin + ci), optional nearest-x2 in front;
    ``pad_lo`` zero rows / columns in front of the image (1: idf_conv3x3; 0: idf_conv3x3_down, which pads right and bottom only).
    -> (want, slack): [B, Ho, Wo, Cout], or NCHW [B, n_valid, Ho, Wo].  ``front`` / ``pad_mode`` exist for the CPU tests that show the
    bound rejects a wrong window origin and a clamped read in place of the zero padding."""
    B, H, W_, Cin = x.shape
    Cout = w.shape[0]
    Ho, Wo = conv_out_hw(H, W_, stride, up, pad_lo)
    fr = pad_lo if front is None else front

    def core(xi, wt):
        if up:
            xi = F.interpolate(xi, scale_factor=2, mode="nearest")
        Hup, Wup = xi.shape[-2:]
        xp = F.pad(xi, (fr, (Wo - 1) * stride + 3 - fr - Wup, fr, (Ho - 1) * stride + 3 - fr - Hup), mode=pad_mode)
        return F.conv2d(xp, wt, stride=stride)
    wt = w.reshape(Cout, 3, 3, Cin).permute(0, 3, 1, 2)
    y = core(x.to(cd).permute(0, 3, 1, 2), wt.to(cd))
    mag = core(x.double().abs().permute(0, 3, 1, 2), wt.double().abs())
    if bias is not None:
        y = y + bias.to(cd).view(1, -1, 1, 1)
    if rowbias is not None:
        y = y + rowbias.to(cd)[:, :, None, None]
    if res is not None:
        y = y + res.to(cd).permute(0, 3, 1, 2)
    slack = 9 * Cin * EPS32 * mag
    if n_valid:
        return y[:, :n_valid].contiguous(), slack[:, :n_valid].contiguous()
    return y.permute(0, 2, 3, 1).contiguous(), slack.permute(0, 2, 3, 1).contiguous()


# ---- the dispatch rules of csrc/gemm_conv.hip launch() and csrc/gemm_big.hip idf_launch_big(), for the forced families ------------
def tile_grid(M, N, conv=False, geglu=False):
    """Tiles of the small-tile / latency kernels: 128 x 128 when N fills it (or the conv's N > 128), else 128 x 64."""
    t128 = geglu or N % 128 == 0 or N > 1024 or (conv and N > 128)
    bn = 128 if t128 else 64
    return -(-N // bn) * -(-M // 128), bn


def split_plan(family, M, N, K, *, conv=False, geglu=False, batch=1, ws=True):
    """K-tiles per slice of the split-K launch the forced family makes of the shape, e.g. [5, 4]; [nk] when it does not split.
    A mirror of the host code for the shapes listed here, not a measurement: it assumes NUM_CU workgroup slots and a workspace that
    holds every slab (it leaves out the loops that lower the slice count until ``ws_bytes`` suffices), and the launch counters cannot
    show the slice count.  ``ws=False``: the launch has no workspace (self-computed ln_row statistics occupy it) and never splits."""
    nk = K // BK
    tiles, _ = tile_grid(M, N, conv, geglu)
    want = 1
    if family == "small" and batch == 1 and ws and not geglu and tiles < 192 and nk >= 8:
        want = min(-(-512 // tiles), nk // 4, 64)
    elif family == "ring" and batch == 1 and ws and not geglu and tiles * 2 <= NUM_CU and nk >= 16:
        want = min(NUM_CU // tiles, nk // 8, 64)
    elif family == "big":
        bn = 320 if N % 320 == 0 else 256 if N % 256 == 0 else 128
        big_tiles = (N // bn) * -(-M // 256)
        if bn != 128 and not geglu and ws and big_tiles * 2 <= NUM_CU:
            for cand in range(NUM_CU // big_tiles, 1, -1):
                if nk % cand == 0 and nk // cand >= 16:
                    return [nk // cand] * cand
        return [nk]
    if want <= 1:
        return [nk]
    per = -(-nk // want)
    return [min(per, nk - b) for b in range(0, nk, per)]


def family_takes(family, M, N, K, *, conv=False, geglu=False, geglu_period=64, batch=1, self_ln=False, nchw=False, ldo=None, ldr=None,
                 ld_rowbias=None, ws=True):
    """Does the forced family take the launch (``ldo`` etc. None: not used / dense)?  What it declines runs on the small-tile kernels.
    The same assumptions as ``split_plan`` (NUM_CU slots, a workspace that always fits)."""
    if family == "small":
        return True
    nk = K // BK
    tiles, _ = tile_grid(M, N, conv, geglu)
    if family == "ring":                                 # launch_ring_cfg: 129 .. 191 tiles with a long K are left to split-K
        return not (batch == 1 and ws and not geglu and tiles * 2 > NUM_CU and tiles < 192 and nk >= 8)
    if batch != 1 or K < 2 * BK or nchw:
        return False
    if any(ld is not None and ld % 8 for ld in (ldo, ldr, ld_rowbias)):
        return False
    if geglu:
        return N % 256 == 0 or (geglu_period == 32 and N % 320 == 0)
    return N % 320 == 0 or N % 256 == 0 or (N % 128 == 0 and not self_ln)


# ---- dense GEMM cases ----------------------------------------------------------------------------------------------------------
DENSE_SHAPES = [
    (1, 8, 64), (5, 9, 64),                              # one K-tile; one row, one 8-column chunk / a ragged second chunk
    (127, 72, 128), (129, 77, 192),                      # fewer K-tiles than ring stages (2 and 3); M either side of one tile
    (130, 320, 320), (130, 256, 128),                    # 128 x 64 tiles (N = 64 mod 128) versus 128 x 128 tiles
    (256, 128, 128), (300, 320, 128),                    # smallest persistent shapes: 128- and 320-wide tiles, two K-tiles
    (8, 8, 512),                                         # small family: split-K, 2 slices of 4 K-tiles
    (70, 77, 576),                                       # small family: 5 + 4 K-tiles, N % 4 != 0: scalar slab stores and reducer
    (33, 100, 832),                                      # small family: 5 + 5 + 3 K-tiles, N % 8 == 4: vector slabs, ragged last chunk
    (130, 136, 1024),                                    # latency kernel: split-K, 2 slices of 8
    (64, 9, 1088),                                       # latency kernel: 9 + 8 K-tiles
    (256, 256, 2048),                                    # persistent kernel: two slices of 16 K-tiles
]
SPLIT_EXPECTED = {                                       # (family, shape) -> K-tiles per slice, as the comments above claim
    ("small", (8, 8, 512)): [4, 4], ("small", (70, 77, 576)): [5, 4], ("small", (33, 100, 832)): [5, 5, 3],
    ("ring", (130, 136, 1024)): [8, 8], ("ring", (64, 9, 1088)): [9, 8], ("big", (256, 256, 2048)): [16, 16],
}
BATCHED = [(3, 77, 320, 64, "w"), (3, 77, 320, 64, "a")]  # batched launches never split; shared W (2-D) / shared A: the transposed-V call
# odd leading dimensions: (N, what, pad) at M = 70 and K in ODD_LD_K (unsplit, and the small family's split-K + reducer)
ODD_LD = [(77, "ldo", 3), (80, "ldo", 3), (80, "ldr", 1), (77, "ldr", 1), (80, "ld_rowbias", 4), (80, "ldo_f32", 2), (77, "ldo_f32", 2)]
ODD_LD_K = (128, 576)
ODD_LD_EPI = {"ldo": "bias", "ldr": "res", "ld_rowbias": "bias_rowbias", "ldo_f32": "f32out"}
# every epilogue; the second shape is split-K + reducer in the small family -- but for ln_row_self, whose statistics take the workspace
# (csrc/gemm_conv.hip launch()): that one runs unsplit there, through the kernel's own epilogue at nine K-tiles
EPI_SHAPES = [(130, 136, 128), (70, 136, 576)]
EPI_SHAPE_BIG = (130, 256, 128)                          # N = 136 is not the persistent kernel's: its epilogues run here
EPILOGUES = ["bias", "bias_rowbias", "res", "res_gate", "res_alias", "silu_res_gate", "gelu_res_gate", "quick_gelu_res_gate", "f32out",
             "ln_row", "ln_row_self", "ln_col", "out_stats"]
GEGLU_CASES = [(130, 128, 64, 64), (130, 128, 64, 32), (200, 640, 320, 64), (200, 640, 320, 32)]   # (M, N packed, K, period)
SWEEP = [0.0, 2.0 ** -14, 1e-3, 0.1, 0.5, 1, 1.5, 2, 3, 4, 5, 6, 7, 7.5, 8, 8.5, 10, 12, 20, 60, 100, 1000]
SWEEP_ACTS = ["silu", "gelu", "quick_gelu", "geglu64", "geglu32"]


def _ramp(n, k, a=3, b=1, mod=17):
    """[n, k] of (a i + b j) % mod - mod // 2 over 8: exact in both types, no two rows or columns alike."""
    i, j = torch.arange(n)[:, None], torch.arange(k)[None]
    return ((a * i + b * j) % mod - mod // 2).float() / 8.0


def _ints(shape, seed):
    return torch.randint(-2, 3, shape, generator=torch.Generator().manual_seed(seed)).float()


def gemm_operands(M, N, K, dt, kind="normal", batch=0, shared=None, shift=0.0):
    """a [.., M, K] and w [.., N, K] in the 16-bit type.  kind: seeded normal (weights scaled by K^-0.5); "struct": a identity-like,
    w a ramp, so out[m, n] = w[n, m % K] and a row / column swap cannot pass; "ints": small integers, every partial sum exact."""
    sa = (M, K) if (not batch or shared == "a") else (batch, M, K)
    sw = (N, K) if (not batch or shared == "w") else (batch, N, K)
    if kind == "struct":
        a = torch.zeros(M, K)
        a[torch.arange(M), torch.arange(M) % K] = 1.0
        w = _ramp(N, K)
    elif kind == "ints":
        a, w = _ints(sa, 700 + M), _ints(sw, 701 + N)
    else:
        a, w = gen(sa, 702 + M + K) + shift, gen(sw, 703 + N + K, K ** -0.5)
    return a.to(DTYPES[dt]), w.to(DTYPES[dt])


def row_stats32(x, eps=1e-5):
    xd = x.double()
    mu = xd.mean(-1)
    return torch.stack([mu, 1.0 / ((xd - mu[..., None]).pow(2).mean(-1) + eps).sqrt()], -1).float()


def gemm_case(M, N, K, dt, epi="bias", kind="normal", batch=0, shared=None, ldo_pad=0, ldr_pad=0, ldrb_pad=0):
    """-> dict(a, w, kw): ``kw`` are the keyword arguments both of ``HipOps.gemm`` and (minus the leading dimensions) of ``gemm_ref``;
    kw["f32out"] / kw["out_stats"] / kw["res_alias"] are flags for the runner."""
    ln = epi in ("ln_row", "ln_row_self", "ln_col")
    a, w = gemm_operands(M, N, K, dt, kind, batch, shared, shift=0.5 if ln else 0.0)
    T = DTYPES[dt]
    lead = (batch,) if batch else ()
    kw = {}
    if epi not in ("res", "res_gate", "res_alias", "ln_col", "out_stats"):
        kw["bias"] = gen((N,), 710 + N)
    if epi.endswith("out_stats"):                        # four rows of variance ~4e-6, below OUT_STATS_EPS: a missing eps shows there
        a[..., :4, :] = (a[..., :4, :].float() * 2.0 ** -9).to(T)
    if epi == "bias_rowbias":
        kw["rowbias"], kw["rows_per_batch"] = gen((-(-M // 50), N), 711).to(T), 50
    if "res" in epi:
        kw["res"] = gen(lead + (M, N), 712 + M).to(T)
    if epi.endswith("res_gate"):
        kw["gate"] = torch.tensor([math.tanh(0.7)])
    for act in ("silu", "gelu", "quick_gelu"):
        if epi.startswith(act + "_"):
            kw["act"] = act
    if epi == "ln_row":
        kw["ln_row"] = (row_stats32(a), w.float().sum(-1))
    if epi == "ln_row_self":
        kw["ln_row"] = (None, w.float().sum(-1))
    if epi == "ln_col":
        kw["ln_col"] = (row_stats32(w), a.float().sum(-1), gen((M,), 713))
    return dict(a=a, w=w, kw=kw, f32out=epi == "f32out", out_stats=epi.endswith("out_stats"), res_alias=epi.endswith("res_alias"),
                ldo_pad=ldo_pad, ldr_pad=ldr_pad, ldrb_pad=ldrb_pad)


OUT_STATS_EPS = 1e-5


def out_stats_excess(stats, want64, slack, dt, eps=OUT_STATS_EPS):
    """(mean error / its bound, rstd error / its bound), the largest over the rows, of the ``out_stats`` by-product: (mu, rstd) of
    every output row, rstd = (var + eps)^-1/2.  With e the per-element error of the values the kernel takes them of (the stored ones
    or the fp32 ones in front of the rounding, |e| <= b = U |want| + slack either way):
      |mu' - mu| <= mean|e| <= mean(b);
      |std' - std| <= rms(e - mean e) <= rms(b) by the triangle inequality on the centred row, and with r = rstd
      |r' / r - 1| = |std' - std| (std' + std) r r' / (1 + r' / r) <= rms(b) r to first order, as std r <= 1: 1.5 rms(b) r covers the
      higher orders for rms(b) r <= 1/2.
    Both get the project's fp32 bar on top, 1e-5 (of max|want| for the mean), for the statistics arithmetic itself."""
    want = want64.double().cpu()
    st = stats.detach().double().cpu().reshape(-1, 2)
    want = want.reshape(st.shape[0], -1)
    bound = U[dt] * want.abs() + slack.double().reshape(want.shape)
    mu = want.mean(-1)
    rstd = 1.0 / ((want - mu[:, None]).pow(2).mean(-1) + eps).sqrt()
    e_mu = (st[:, 0] - mu).abs() / (bound.mean(-1) + 1e-5 * want.abs().max())
    e_rs = (st[:, 1] / rstd - 1).abs() / (1.5 * bound.pow(2).mean(-1).sqrt() * rstd + 1e-5)
    nan = lambda t: torch.where(torch.isnan(t), torch.full_like(t, float("inf")), t)
    return float(nan(e_mu).max()), float(nan(e_rs).max())


def gemm_want(case, cd=torch.float64):
    return gemm_ref(case["a"], case["w"], cd=cd, **case["kw"])


def geglu_case(M, N, K, period, dt, kind="normal"):
    """The UNPACKED projection w [N, K] / b [N] ([value | gate] halves) for the reference, its ``engine.pack_geglu`` image for the
    kernel, and a folded LayerNorm with given statistics."""
    from instancediffusion_amd.engine import pack_geglu
    a, w = gemm_operands(M, N, K, dt, kind, shift=0.5)
    b = gen((N,), 720 + N)
    wp, bp = pack_geglu(w, b, period)
    ln = (row_stats32(a), w.float().sum(-1))
    lnp = (ln[0], pack_geglu(w, ln[1], period)[1])
    return dict(a=a, w=w, wp=wp, ref_kw=dict(bias=b, ln_row=ln, geglu=True), kw=dict(bias=bp, ln_row=lnp, geglu=True, geglu_period=period))


def sweep_values(dt):
    """+-SWEEP, each value rounded to the 16-bit type first, repeated up to 128 columns."""
    v = torch.tensor(SWEEP + [-x for x in SWEEP]).to(DTYPES[dt])
    return v.repeat(-(-128 // v.numel()))[:128]


def sweep_case(act, dt, K=64):
    """Accumulators that are exactly the sweep values: A[m, 0] = 1, W[n, 0] = x_n, every other product zero.  For GEGLU the sweep is
    the gate and the value alternates between 1 and -3.  M = 5 rows, 128 output columns."""
    from instancediffusion_amd.engine import pack_geglu
    x = sweep_values(dt)
    a = torch.zeros(5, K, dtype=DTYPES[dt])
    a[:, 0] = 1.0
    if not act.startswith("geglu"):
        w = torch.zeros(128, K, dtype=DTYPES[dt])
        w[:, 0] = x
        return dict(a=a, w=w, kw=dict(act=act), ref_kw=dict(act=act))
    period = int(act[5:])
    w = torch.zeros(256, K, dtype=DTYPES[dt])
    w[:128, 0] = torch.where(torch.arange(128) % 2 == 0, 1.0, -3.0).to(DTYPES[dt])
    w[128:, 0] = x
    b = torch.zeros(256)
    wp, bp = pack_geglu(w, b, period)
    return dict(a=a, w=w, wp=wp, kw=dict(bias=bp, geglu=True, geglu_period=period), ref_kw=dict(bias=b, geglu=True))


# rows of A / W, columns k = 0, 1 (every other k is zero); acc[i, j] = A[i, 0] W[j, 0] + A[i, 1] W[j, 1]
OVERFLOW_AT = {70000: (0, 0), -70000: (0, 1), 65519: (1, 2), 65527: (2, 3), 65504: (1, 5)}      # fp16: accumulator -> (row, column)
OVERFLOW_A = {"fp16": ((250.0, 0.0), (2047.0, 15.0), (1771.0, 0.0), (0.0, 0.0), (1.0, 0.0)), "bf16": ((250.0, 0.0), (0.0, 0.0), (1.0, 0.0))}
OVERFLOW_W = {"fp16": ((280.0, 0.0), (-280.0, 0.0), (32.0, 1.0), (37.0, 0.0), (1.0, 0.0), (32.0, 0.0)), "bf16": ((280.0, 0.0), (-280.0, 0.0), (1.0, 0.0))}


def overflow_case(dt, K=64):
    """fp16: accumulators of exactly +-70000 (250 x 280), 65504 (2047 x 32 + 15 x 0: the largest finite value, which must stay),
    65519 (2047 x 32 + 15 x 1: below the tie at 65520, RNE to 65504) and 65527 (1771 x 37: above the tie, inf), with their cross products; bf16: +-70000, which stays finite.  The contract
    is ``want.to(dtype)`` bit for bit: +-inf above the fp16 range."""
    a = torch.zeros(len(OVERFLOW_A[dt]), K)
    a[:, :2] = torch.tensor(OVERFLOW_A[dt])
    w = torch.zeros(128, K)
    w[:len(OVERFLOW_W[dt]), :2] = torch.tensor(OVERFLOW_W[dt])
    return dict(a32=a, w32=w, a=a.to(DTYPES[dt]), w=w.to(DTYPES[dt]))


# ---- conv cases ----------------------------------------------------------------------------------------------------------------
# (B, H, W, Cin, Cout, stride, up), options
CONV_CASES = [
    ((1, 1, 1, 64, 64, 1, 0), {}),                       # one pixel: eight of nine taps are padding
    ((1, 1, 3, 64, 72, 1, 0), {}),                       # one image row; a second 64-wide column tile that holds one 8-column chunk
    ((2, 2, 2, 64, 64, 2, 0), {}),                       # stride 2 down to 1 x 1 per sample
    ((1, 3, 3, 64, 64, 2, 0), {}),                       # stride 2, odd size: 2 x 2 out
    ((1, 1, 1, 64, 64, 1, 1), {}),                       # nearest-x2 of one pixel
    ((1, 2, 3, 128, 64, 1, 1), {}),                      # nearest-x2, two K-tiles per tap
    ((3, 5, 7, 64, 64, 1, 0), dict(rowbias=True, res=True)),    # 105 rows: one tile holds three samples, per-sample row bias
    ((3, 5, 7, 64, 320, 2, 0), dict(rowbias=True, res=True)),   # 36 rows, stride 2, 320 wide (the persistent kernel's too)
    ((1, 4, 4, 128, 136, 1, 0), {}),                     # two weight K-tiles per tap; 128-wide tiles with a ragged second one
    ((2, 8, 8, 128, 320, 1, 0), {}),                     # persistent kernel, 320-wide tile
    ((2, 8, 8, 128, 320, 2, 0), {}),                     # ... stride 2
    ((2, 4, 4, 128, 320, 1, 1), {}),                     # ... nearest-x2
    ((2, 3, 5, 64, 64, 1, 0), dict(n_valid=3)),          # NCHW fp32 output, n_valid < 8
    ((2, 3, 5, 64, 64, 1, 0), dict(n_valid=4)),
    ((2, 3, 5, 64, 64, 1, 0), dict(xslice=True)),        # input a channel slice buf[..., 64:128] of 192 channels: ldx = 192
    ((2, 3, 5, 64, 64, 1, 0), dict(res=True, ldo_pad=8)),        # output rows padded: ldo = Cout + 8
    ((2, 3, 5, 64, 64, 1, 0), dict(res=True, ldr_pad=8)),        # residual rows padded: ldr = Cout + 8
]
CONV_NO_SPLIT = ((6, 64, 64, 64, 64, 1, 0), {})          # 192 tiles: the small-tile family WITHOUT split-K (small family only)
DOWN_CASES = [(1, 2, 2, 64, 64), (2, 3, 3, 64, 64), (1, 5, 4, 128, 72)]       # idf_conv3x3_down (B, H, W, Cin, Cout), +- residual
CONV_STRUCT = [(3, 5, 7, 64, 64, 1, 0), (2, 8, 8, 128, 320, 1, 0)]          # structured operands; the second is the persistent kernel's too
DOWN_STRUCT = (1, 5, 4, 128, 72)
CONV_INT_CASES = {                                       # a split-K conv per family, exact-integer inputs
    "small": (3, 5, 7, 64, 64, 1, 0),                    # 9 K-tiles: 5 + 4
    "ring": (1, 4, 4, 128, 136, 1, 0),                   # 18 K-tiles: 9 + 9
    "big": (2, 8, 8, 256, 320, 1, 0),                    # 36 K-tiles: two slices of 18
}
CONV_SPLIT_EXPECTED = {"small": [5, 4], "ring": [9, 9], "big": [18, 18]}
DENSE_INT_CASES = {"small": (70, 77, 576), "ring": (64, 9, 1088), "big": (256, 256, 2048)}


def conv_case(shape, opts, dt, kind="normal", pad_lo=1):
    """-> dict(x, w, kw, ...): x [B, H, W, Cin] (a channel slice of a wider buffer with opts["xslice"]), w [Cout, 9*Cin]."""
    B, H, W_, Cin, Cout, stride, up = shape
    T = DTYPES[dt]
    Ho, Wo = conv_out_hw(H, W_, stride, up, pad_lo)
    if kind == "struct":                                 # pixel p lights channel p % Cin; the weight is a ramp over (Cout, tap, ci)
        x = torch.zeros(B * H * W_, Cin)
        x[torch.arange(B * H * W_), torch.arange(B * H * W_) % Cin] = 1.0
        x, w = x.view(B, H, W_, Cin), _ramp(Cout, 9 * Cin, 5, 3, 31) / 2.0
    elif kind == "ints":
        x, w = _ints((B, H, W_, Cin), 730 + H), _ints((Cout, 9 * Cin), 731 + Cout)
    else:
        x, w = gen((B, H, W_, Cin), 732 + H * W_ + Cin), gen((Cout, 9 * Cin), 733 + Cout, (9 * Cin) ** -0.5)
    x = x.to(T)
    if opts.get("xslice"):
        buf = gen((B, H, W_, 192), 734).to(T)
        buf[..., 64:64 + Cin] = x
        x = buf[..., 64:64 + Cin]
    kw = dict(stride=stride, up=up, pad_lo=pad_lo)
    if kind != "ints":
        kw["bias"] = gen((Cout,), 735 + Cout)
    if opts.get("rowbias"):
        kw["rowbias"] = gen((B, Cout), 736).to(T)
    if opts.get("res"):
        kw["res"] = gen((B, Ho, Wo, Cout), 737 + Ho).to(T)
    if opts.get("n_valid"):
        kw["n_valid"] = opts["n_valid"]
    return dict(x=x, w=w.to(T), kw=kw, out_shape=(B, Ho, Wo, Cout), ldo_pad=opts.get("ldo_pad", 0), ldr_pad=opts.get("ldr_pad", 0))


def conv_want(case, cd=torch.float64, **mut):
    return conv3x3_ref(case["x"], case["w"], cd=cd, **case["kw"], **mut)


def conv_dispatch_args(shape, opts, pad_lo=1):
    """(M, N, K, keyword arguments of family_takes) of a conv case."""
    B, H, W_, Cin, Cout, stride, up = shape
    Ho, Wo = conv_out_hw(H, W_, stride, up, pad_lo)
    return B * Ho * Wo, Cout, 9 * Cin, dict(conv=True, nchw=bool(opts.get("n_valid")), ldo=Cout + opts.get("ldo_pad", 0),
                                           ldr=Cout + opts.get("ldr_pad", 0) if opts.get("res") else None)


# ---- every case, for the CPU proofs ------------------------------------------------------------------------------------------------
def want_of(kind, case, cd=torch.float64, **mut):
    """(want, slack) of a case of ``all_cases`` in compute type ``cd``."""
    if kind == "conv":
        return conv_want(case, cd, **mut)
    if kind == "geglu":
        return gemm_ref(case["a"], case["w"], cd=cd, **case["ref_kw"])
    return gemm_want(case, cd)


def all_cases(dt):
    """(label, kind, case, f32out) of every case the GPU tests run on random or structured inputs (the bit-for-bit cases -- integers,
    overflow -- have no bound to prove)."""
    for shape in DENSE_SHAPES:
        yield f"gemm {shape}", "gemm", gemm_case(*shape, dt), False
    yield "gemm struct (130, 136, 128)", "gemm", gemm_case(130, 136, 128, dt, kind="struct"), False
    for (Bt, M, N, K, sh) in BATCHED:
        yield f"gemm batched shared {sh}", "gemm", gemm_case(M, N, K, dt, batch=Bt, shared=sh), False
    for (N, what, pad) in ODD_LD:
        for K in ODD_LD_K:
            yield f"gemm odd {what} N={N} K={K}", "gemm", gemm_case(70, N, K, dt, ODD_LD_EPI[what]), what == "ldo_f32"
    for shape in EPI_SHAPES + [EPI_SHAPE_BIG]:
        for epi in EPILOGUES:
            yield f"gemm {epi} {shape}", "gemm", gemm_case(*shape, dt, epi), epi == "f32out"
    for (M, N, K, P) in GEGLU_CASES:
        yield f"geglu P={P} {(M, N, K)}", "geglu", geglu_case(M, N, K, P, dt), False
    for act in SWEEP_ACTS:
        for K in (64, 128):
            case = sweep_case(act, dt, K)
            yield f"sweep {act} K={K}", "geglu" if "wp" in case else "sweep", case, False
    for shape, opts in CONV_CASES + [CONV_NO_SPLIT]:
        yield f"conv {shape} {opts}", "conv", conv_case(shape, opts, dt), bool(opts.get("n_valid"))
    for shape in CONV_STRUCT:
        yield f"conv struct {shape}", "conv", conv_case(shape, {}, dt, kind="struct"), False
    yield f"conv_down struct {DOWN_STRUCT}", "conv", conv_case(DOWN_STRUCT + (2, 0), {}, dt, kind="struct", pad_lo=0), False
    for (B, H, W_, Cin, Cout) in DOWN_CASES:
        for res in (False, True):
            yield f"conv_down {(B, H, W_, Cin, Cout)} res={res}", "conv", conv_case((B, H, W_, Cin, Cout, 2, 0), dict(res=res), dt, pad_lo=0), False


# ---- the persistent kernel's tile walk (csrc/gemm_big.hip) ---------------------------------------------------------------------------
# A mirror of gemm_kernel_big's work-item arithmetic and of the hybrid plan of idf_launch_big, like ``split_plan`` not a measurement:
# NUM_CU workgroup slots, a workspace that always fits.  The GPU cannot show which walk ran or which workgroup ran which item -- both
# walks compute the same bits -- so what the walk cases below reach is proved here, on the CPU (tests/test_gemm_conv_refs.py), and
# tests/test_gemm_big_walk_gpu.py judges only the results.
BM_BIG = 256


def big_tile_width(N, geglu=False, geglu_period=64):
    """The BN idf_launch_big picks for N weight rows (packed rows for GEGLU); 0: the persistent kernel does not take it."""
    if geglu:
        return 320 if geglu_period == 32 and N % 320 == 0 else 256 if N % 256 == 0 else 0
    return 320 if N % 320 == 0 else 256 if N % 256 == 0 else 128 if N % 128 == 0 else 0


def big_tiles(M, N, bn):
    return (N // bn) * -(-M // BM_BIG)


def hybrid_plan(M, N, K, min_eff=80, num_cu=NUM_CU):
    """The hybrid launch idf_launch_big makes of a plain GEMM / conv under IDF_TUNE_GEMM_BIG = 3 when its tile grid fills less than
    ``min_eff`` % of the slots of its rounds: dict(whole, rem, S, tail_m0, items) -- ``whole`` leading whole-tile items, the remaining
    ``rem`` tiles (rows from ``tail_m0``) cut into ``S`` K-slices each -- or None when it launches unsplit or declines."""
    bn = big_tile_width(N)
    tiles_n, tiles, nk = N // bn, big_tiles(M, N, bn), K // BK
    rounds = -(-tiles // num_cu)
    if tiles * 100 >= min_eff * rounds * num_cu or tiles * 2 <= num_cu or bn == 128:
        return None                                      # at the bar: unsplit; half-empty grids are uniform split-K's (split_plan)
    whole = ((tiles // num_cu) * num_cu // tiles_n) * tiles_n
    rem = tiles - whole
    if whole <= 0 or rem <= 0:
        return None
    for S in range(num_cu // rem, 1, -1):
        if nk % S == 0 and nk // S >= 4:                 # slices of at least four K-tiles
            return dict(whole=whole, rem=rem, S=S, tail_m0=whole // tiles_n * BM_BIG, items=whole + rem * S)
    return None


def big_walk_chunked(M, N, bn, hybrid=None, fold=False, num_cu=NUM_CU):
    """Does the launch take the chunked walk (tile_walk == 1 and more items than workgroups)?"""
    items = 4 * big_tiles(M, N, bn) if fold else big_tiles(M, N, bn)
    return hybrid is None and N // bn >= 32 and items > min(items, num_cu)


def big_walk(M, N, bn, hybrid=None, fold=False, num_cu=NUM_CU):
    """For every workgroup (by blockIdx.x) the ordered work items (tile, slice) it runs.  ``hybrid`` = (full items, S) of a split
    launch (its item_map: items below ``full`` are whole tiles, the rest S slices per tile); ``fold``: the four parity phases of
    idf_conv_up2x_folded, phase-major -- "tile" is then phase * tiles + tile.  G = min(items, num_cu) workgroups; workgroup L takes
    slot (L & 7) * (G >> 3) + (L >> 3) when G % 8 == 0, else L; slot s walks s, s + G, ... or, chunked, [s q + min(s, r), ...).
    A mirror of the kernel's index arithmetic, not a measurement: no counter or output shows which walk a launch took."""
    tiles = big_tiles(M, N, bn)
    full, S = hybrid if hybrid is not None else (tiles, 1)
    items = 4 * tiles if fold else full + (tiles - full) * S
    G = min(items, num_cu)
    chunked = big_walk_chunked(M, N, bn, hybrid, fold, num_cu)

    def item_map(i):
        return (i, 0) if i < full or fold else (full + (i - full) // S, (i - full) % S)
    walk = []
    for bid in range(G):
        slot = (bid & 7) * (G >> 3) + (bid >> 3) if G % 8 == 0 else bid
        if chunked:
            q, r = divmod(items, G)
            seq0 = slot * q + min(slot, r)
            seq = range(seq0, seq0 + q + (1 if slot < r else 0))
        else:
            seq = range(slot, items, G)
        walk.append([item_map(i) for i in seq])
    return walk


# Walk cases: the smallest M that gives at least NUM_CU + 2 work items and ends in a ragged last m-tile; K-tile counts that make
# consecutive tiles enter the LDS ring on different stages (2 stages: an odd count; the 128-wide tiles' 3 stages: 2, 3 and 4).
# (shape (M, N, K) with N the weight rows -- packed for GEGLU, q | k | v for the fused projection --, epilogue, work items)
WALK_VT_COL0 = 640
WALK_DENSE = [
    ((32924, 640, 128), "bias_res_gate", 258),           # 320-wide plain, 2 K-tiles
    ((32924, 640, 192), "bias_res_gate", 258),           # ... 3 K-tiles
    ((32924, 640, 192), "f32out", 258),
    ((32924, 512, 192), "bias", 258),                    # 256-wide plain
    ((32924, 512, 192), "gelu_res_gate", 258),
    ((22172, 384, 128), "bias_rowbias", 261),            # 128-wide, 3 stages: a tile enters the ring 2 ...
    ((22172, 384, 192), "bias_rowbias", 261),            # ... 0 ...
    ((22172, 384, 256), "bias_rowbias", 261),            # ... 1 stages (mod 3) behind its predecessor
    ((32924, 640, 192), "ln_row_self", 258),             # LNS: statistics summed in the K loop, ln_stats_out checked
    ((32924, 512, 192), "ln_row_self", 258),
    ((32924, 640, 192), "bias_res_out_stats", 258),      # STATS: out_stats from the epilogue registers
    ((32924, 512, 192), "bias_res_out_stats", 258),
    ((22096, 960, 192), "vt", 261),                      # VT: fused q | k | V^T, statistics given; M % 16 == 0, M % 256 == 80
    ((22096, 960, 192), "vt_self", 261),                 # VT + LNS
    ((32924, 640, 192), "geglu32", 258),                 # GLU: period 32 on 320-wide tiles, statistics given
    ((32924, 640, 192), "geglu32_self", 258),            # GLU + LNS
    ((32924, 512, 192), "geglu64", 258),                 # period 64 on 256-wide tiles
    ((2204, 10240, 128), "bias", 288),                   # chunked walk: 32 n-tiles of 320 per m-tile, 9 m-tiles ...
    ((2204, 8192, 128), "bias", 288),                    # ... of 256 ...
    ((2204, 10240, 128), "geglu32", 288),                # ... and the GLU kernel; 32 workgroups take two consecutive n-tiles
]
WALK_CHUNKED = [c for c in WALK_DENSE if c[0][0] == 2204]
RB_RES = dict(rowbias=True, res=True)
# ((B, H, W, Cin, Cout, stride, up), options, pad_lo, work items); Cin = 64: nine K-tiles
WALK_CONV = [
    ((3, 104, 106, 64, 640, 1, 0), RB_RES, 1, 260),      # 320-wide; 33072 rows, tiles straddle the samples
    ((3, 208, 211, 64, 640, 2, 0), RB_RES, 1, 260),      # the same output through stride 2
    ((3, 52, 53, 64, 640, 1, 1), RB_RES, 1, 260),        # ... through nearest-x2
    ((3, 208, 212, 64, 640, 2, 0), dict(res=True), 0, 260),     # ... through idf_conv3x3_down (which has no row bias)
    ((3, 104, 106, 64, 512, 1, 0), RB_RES, 1, 260),      # 256-wide
    ((3, 148, 149, 64, 128, 1, 0), RB_RES, 1, 259),      # 128-wide, 3 stages; 66156 rows
]
# GST: gn_partial out of the epilogue.  Ho * Wo = 182 x 64, 34944 rows: 137 m-tiles x 2; a sample boundary falls on a 64-row chunk
# inside a tile
WALK_GST = ((3, 104, 112, 64, 640, 1, 0), dict(rowbias=True), 1, 274)
WALK_FOLD = ((1, 129, 129, 64, 320), 264)                # idf_conv_up2x_folded: 66 m-tiles x 4 phases
WALK_HYBRID_DENSE = ((33180, 640, 512), "bias_res_alias")      # 260 tiles, 256 whole + 4 x 2 slices of 4 K-tiles
WALK_HYBRID_CONV = ((3, 104, 106, 128, 640, 1, 0), RB_RES)     # 18 K-tiles: 256 whole + 4 x 3 slices of 6
WALK_HYBRID_EXPECTED = {
    "dense": dict(whole=256, rem=4, S=2, tail_m0=32768, items=264),
    "conv": dict(whole=256, rem=4, S=3, tail_m0=32768, items=268),
}
WALK_EXACT_DENSE = (32924, 640, 192)                     # integer operands, bit for bit: 320-wide dense, 320-wide conv, hybrid dense
WALK_EXACT_CONV = (3, 104, 106, 64, 640, 1, 0)
WALK_SAME_ROWS = [(32924, 640, 192), (32924, 512, 192), (22172, 384, 192)]    # A[m] = A[m % 256]: 320-, 256- and 128-wide


def walk_dense_width(shape, epi):
    return big_tile_width(shape[1], epi.startswith("geglu"), int(epi[5:7]) if epi.startswith("geglu") else 64)


def walk_dense_case(shape, epi, dt, kind="normal"):
    """The case dict of a WALK_DENSE entry (as ``gemm_case`` / ``geglu_case``); ``ln_stats_out`` / ``vt_col0`` name its by-products."""
    M, N, Kk = shape
    if epi.startswith("geglu"):
        case = geglu_case(M, N, Kk, int(epi[5:7]), dt, kind)
        if epi.endswith("_self"):
            case["kw"]["ln_row"] = (None, case["kw"]["ln_row"][1])
            case["ref_kw"]["ln_row"] = (None, case["ref_kw"]["ln_row"][1])
            case["ln_stats_out"] = True
        return case
    if epi.startswith("vt"):
        a, w = gemm_operands(M, N, Kk, dt, shift=0.5)
        self_ln = epi == "vt_self"
        kw = dict(bias=gen((N,), 710 + N), ln_row=(None if self_ln else row_stats32(a), w.float().sum(-1)))
        return dict(a=a, w=w, kw=kw, vt_col0=WALK_VT_COL0, ln_stats_out=self_ln)
    case = gemm_case(M, N, Kk, dt, epi, kind)
    case["ln_stats_out"] = epi == "ln_row_self"
    return case


def walk_want(case, cd=torch.float64):
    return want_of("geglu" if "ref_kw" in case else "gemm", case, cd)


def same_rows_case(shape, dt):
    """A[m] = A[m % 256]: every m-tile sees the same operand tile.  Bias only -- a per-row residual or row bias would tell the
    rows apart."""
    case = gemm_case(*shape, dt, "bias")
    case["a"] = case["a"][torch.arange(shape[0]) % BM_BIG].contiguous()
    return case


def fold_case(shape, dt):
    """idf_conv_up2x_folded: the fp32 3x3 image, folded in fp32 and rounded once (wf), and rounded unfolded (w) for the reference."""
    from instancediffusion_amd.engine import pack_conv_up2x
    B, H, W_, Cin, Cout = shape
    w4 = gen((Cout, Cin, 3, 3), 741, (9 * Cin) ** -0.5)
    T = DTYPES[dt]
    return dict(x=gen((B, H, W_, Cin), 740).to(T), wf=pack_conv_up2x(w4).to(T), bias=gen((Cout,), 742),
                w=w4.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin).to(T))


def walk_launches():
    """(label, M, N, tile width, hybrid (full, S) or None, fold, work items the tables claim, chunked?) of every walk case."""
    for shape, epi, items in WALK_DENSE:
        yield f"dense {shape} {epi}", shape[0], shape[1], walk_dense_width(shape, epi), None, False, items, shape[0] == 2204
    for shape, opts, pad_lo, items in WALK_CONV + [WALK_GST]:
        M, N, _, _ = conv_dispatch_args(shape, opts, pad_lo)
        yield f"conv {shape} pad_lo={pad_lo}", M, N, big_tile_width(N), None, False, items, False
    (B, H, W_, _, Cout), items = WALK_FOLD
    yield "fold", B * H * W_, Cout, 320, None, True, items, False
    (M, N, Kk), _ = WALK_HYBRID_DENSE
    plan = hybrid_plan(M, N, Kk)
    yield "hybrid dense", M, N, 320, (plan["whole"], plan["S"]), False, plan["items"], False
    M, N, Kk, _ = conv_dispatch_args(*WALK_HYBRID_CONV)
    plan = hybrid_plan(M, N, Kk)
    yield "hybrid conv", M, N, 320, (plan["whole"], plan["S"]), False, plan["items"], False


# ---- GroupNorm partials of a conv output ---------------------------------------------------------------------------------------------
def gn_partial_errors(part, out):
    """(mean, M2) per (sample, 64-row chunk, group) that a conv left in ``part`` [B, HW / 64, 32, 2] against fp64 statistics of the
    16-bit output ``out`` [B, Ho, Wo, C] it stored, chunk by chunk: (largest mean error in units of the chunk's standard deviation,
    largest relative M2 error)."""
    B, C = out.shape[0], out.shape[-1]
    v = out.double().cpu().reshape(B, -1, 64, 32, C // 32).permute(0, 1, 3, 2, 4).reshape(B, part.shape[1], 32, -1)
    mean = v.mean(-1)
    m2 = ((v - mean[..., None]) ** 2).sum(-1)
    pc = part.double().cpu()
    scale = (m2 / v.shape[-1]).sqrt().clamp_min(1e-3)           # per-chunk std
    nan = lambda t: torch.where(torch.isnan(t), torch.full_like(t, float("inf")), t)
    return float(nan((pc[..., 0] - mean).abs() / scale).max()), float(nan((pc[..., 1] - m2).abs() / m2.clamp_min(1e-6)).max())


def same_rows_mismatch(out):
    """Elements of a 16-bit ``out`` [M, N] whose bits differ from row m % 256's -- 0 when rows m and m % 256 were computed from the
    same operands by the same arithmetic (every complete 256-row block, and the ragged last one against the head of the first)."""
    bits = out.view(torch.int16)
    M, full = out.shape[0], out.shape[0] // BM_BIG
    first = bits[:BM_BIG]
    bad = int((bits[:full * BM_BIG].reshape(full, BM_BIG, -1) != first).sum())
    return bad + int((bits[full * BM_BIG:] != first[:M - full * BM_BIG]).sum())
