"""Cases, input builders, fp64 references, the per-element bound, an fp32 replay and a mirror of the dispatch rules for the attention
kernels: the 32-queries-per-wave kernel of csrc/attention.hip (plain, MASK, resident keys), the LDS-DMA kernels of csrc/attention4.hip,
csrc/attention4w.hip and csrc/attention8.hip behind ``idf_attention``, the two fused-qkv kernels of csrc/clip.hip
(``idf_attention_causal``, ``idf_attention_qkv``) and ``idf_softmax_rows``.  No GPU and no HIP library: tests/test_attention_refs.py
proves this module on the CPU, tests/test_attention_edges_gpu.py applies it to the kernels.

The references are plain torch in fp64 on the kernel's own 16-bit inputs (upcast, never re-rounded) and share no code with
tests/emul_ops.py.  They run on whatever device the inputs are on and walk the queries in chunks.

THE BOUND.  ``u`` is the unit roundoff of the storage type (2^-8 bf16, 2^-11 fp16), eps = 2^-24 that of fp32.  For one query q, with
s_j = scale q.k_j, p the fp64 softmax of s over the visible keys, out = sum_j p_j v_j and A_j = scale sum_e |q_e| |k_je|:

 1. Scores.  attention4.hip, attention4w.hip and attention8.hip feed the MFMA a Q that was multiplied by scale*log2(e) and rounded to
    the 16-bit type once: every product q_e k_je carries a relative error <= u, so |ds_j| <= u A_j.  (The 32-query kernel and the CLIP
    kernels scale the fp32 accumulator instead and need less; one bound serves all.)  The fp32 dot product of d terms in any order
    adds d eps A_j; SCORE_C = 3 more eps A_j (|s_j| <= A_j) stand for the rounding of the constant scale*log2(e) on the host, of the
    multiplication / fma that applies it (or of the Q pre-scaling product before its 16-bit rounding) and of the subtraction of the
    reference value m.  v_exp_f32 is good to one ulp and its argument s_j - m is rounded once more: EXP_C = 4 units of
    2^-23 (|s_j| + |max s|), plus 2^-22 absolute for the result's own ulp, written as a score perturbation.  Together
        Delta_j = (u + (d + 3) eps) A_j + 2^-21 (|s_j| + |max_i s_i|) + 2^-22.
 2. What a score perturbation delta (|delta_j| <= Delta_j) does to the output, exactly: with Z' = sum_j p_j e^delta_j,
        out' - out = (1 / Z') sum_j p_j (e^delta_j - 1) (v_j - out),
    because sum_j p_j (v_j - out) = 0.  Hence |out'_e - out_e| <= sum_j p_j (e^Delta_j - 1) |v_je - out_e| / sum_j p_j e^-Delta_j.
 3. P is rounded to the 16-bit type before P.V: u sum_j p_j |v_je| in the numerator; the denominator is either summed from the same
    rounded P (MFMA ones-row, CLIP kernels: u |out_e| at most) or in fp32 from the unrounded P (nothing): u (sum_j p_j |v_je| + |out_e|).
 4. fp16 only: a P below 2^-14 is subnormal (v_cvt_pk_f16_f32 produces it, the MFMA consumes it), spacing 2^-24, error <= 2^-25
    ABSOLUTE on the scale where the row's largest exp(s_j - m) is >= 1, i.e. relative to Z~ = sum_j exp(s_j - max s):
        2^-25 / Z~ * sum_{j: exp(s_j - max s) < 2^-14} |v_je - out_e|.
    This needs every kernel's reference value m to be at most the row's true maximum.  attention4.hip and attention4w.hip used to
    put m 7 log2 units ABOVE the maximum of the tile it was taken from, in fp16 as in bf16, so that every P below 2^-7 of the largest
    was a denormal: ``rebase_replay`` is that arithmetic, tests/test_attention_refs.py shows it outside this bound with shift 7 and
    inside with the shift 0 the kernels now use in fp16.
 5. fp32 accumulation of P.V and of the denominator l over n = n0 + n1 keys in any order, the per-tile rescales and the final
    reciprocal and product (ACC_C = 4: alpha's exp2, alpha * o, 1 / l, o * inv): (n + d + 4) eps sum_j p_j |v_je|.
 6. The final rounding: u |out_e|.
``attention_bound`` returns the sum of 2..6.  A NaN or an element outside counts; tests require exactly 0 outside.

``idf_softmax_rows`` (fp32 scores x in, 16-bit probabilities out; x_j = scale s_j): the fma and the max put
Delta_j = 2^-22 (|x_j| + |max x|) + 2^-22 on each exponent (three fp32 roundings of numbers that size -- the constant scale*log2(e), the
fma, the product m * scale_log2e -- and v_exp's ulp), p'_j / p_j = e^delta_j Z / Z' lies within e^(+-(Delta_j + max Delta)), the fp32
sum of n terms and the reciprocal and product add (n + 2) eps, the store rounds once (u), and an fp16 result below 2^-14 is subnormal
(2^-25 absolute):  |p'_j - p_j| <= p_j (expm1(Delta_j + max Delta) + (n + 2) eps + u) [+ 2^-25].

THE SECOND MEASURE.  The bound is a worst case and sits far above the error of a correct kernel, so an excess rounding can hide
under it.  ``attention_replay`` is the kernels' arithmetic in fp32 on the CPU -- Q pre-scaled and rounded once, P rounded to the
16-bit type, l summed from the rounded P, one output rounding -- and a case passes when the kernel's rel-RMS error against the fp64
reference is at most RMS_FACTOR = 2 x the replay's on the same inputs.  The factor covers what differs between the kernels (summation
order, the reference value they subtract, whether Q is pre-rounded); the bar never comes from a kernel's own figures.

EXACT-DATA CASES.  "census": q = 0, so every visible P is exactly 1, V[j][e] = 1 iff (global key index j) % d == e: out[q][e] =
count_e / n_visible from integer fp32 sums, one reciprocal and one rounding: ``census_bound`` = (u + 2^-21) |want| (2^-21: the
reciprocal, the product, and 1 / l against a correctly rounded quotient).  "negative": q = +1, k = -4 + 0.25 randn: every real score
is far below 0 and a pad key read as zeros would take the whole softmax; v = 1 + 0.25 randn, so that doing so moves every output by about 1.
"""
import math

import torch

from tests.small_kernel_cases import DTYPES, gen, relmax   # noqa: F401  (re-exported)

UR = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}              # unit roundoff of the storage types
EPS32 = 2.0 ** -24
SCORE_C, ACC_C = 3, 4
RMS_FACTOR = 2.0
LOG2E32 = 1.4426950408889634
CHUNK_ELEMS = 1 << 24                                      # fp64 elements of the [queries, keys, d] intermediate per chunk


# ---- the core: fp64 softmax attention of per-head operands, with its bound ------------------------------------------------------
def _core(qh, kh, vh, vis, scale, dt):
    """qh [G, c, d], kh / vh [G, n, d] fp64, vis None or bool broadcastable to [G, c, n] -> (out, bound) [G, c, d]."""
    u, d, n = UR[dt], qh.shape[-1], kh.shape[-2]
    s = scale * (qh @ kh.transpose(-1, -2))
    a = scale * (qh.abs() @ kh.abs().transpose(-1, -2))
    if vis is not None:
        s = s.masked_fill(~vis, float("-inf"))
    mx = s.max(-1, keepdim=True).values
    pt = torch.exp(s - mx)
    z = pt.sum(-1, keepdim=True)
    p = pt / z
    out = p @ vh
    delta = (u + (d + SCORE_C) * EPS32) * a + 2.0 ** -21 * (s.abs() + mx.abs()) + 2.0 ** -22
    if vis is not None:
        delta = torch.where(vis, delta, torch.zeros_like(delta))
    diff = (vh.unsqueeze(-3) - out.unsqueeze(-2)).abs()                        # [G, c, n, d]
    t1 = ((p * torch.expm1(delta)).unsqueeze(-1) * diff).sum(-2) / (p * torch.exp(-delta)).sum(-1, keepdim=True)
    pv = p @ vh.abs()
    bound = t1 + u * (pv + out.abs()) + (n + d + ACC_C) * EPS32 * pv + u * out.abs()
    if dt == "fp16":
        sub = (pt < 2.0 ** -14)
        if vis is not None:
            sub = sub & vis
        bound = bound + 2.0 ** -25 / z * (sub.to(diff.dtype).unsqueeze(-1) * diff).sum(-2)
    return out, bound


def _chunked(qh, kh, vh, vis_fn, scale, dt):
    """``_core`` over query chunks; ``vis_fn(lo, hi)`` -> the visibility of queries [lo, hi) or None."""
    G, nq, d = qh.shape
    step = max(1, CHUNK_ELEMS // max(1, G * kh.shape[-2] * d))
    outs, bounds = [], []
    for lo in range(0, nq, step):
        o, b = _core(qh[:, lo:lo + step], kh, vh, None if vis_fn is None else vis_fn(lo, min(nq, lo + step)), scale, dt)
        outs.append(o)
        bounds.append(b)
    return torch.cat(outs, 1), torch.cat(bounds, 1)


def _heads(x, H):
    """[B, n, H*d] -> [B*H, n, d] fp64."""
    B, n, C = x.shape
    return x.double().reshape(B, n, H, C // H).permute(0, 2, 1, 3).reshape(B * H, n, C // H)


def _unheads(x, B):
    G, n, d = x.shape
    return x.reshape(B, G // B, n, d).permute(0, 2, 1, 3).reshape(B, n, (G // B) * d)


def visibility(qbits, kbits0, n0, kbits1, n1, qidx):
    """include/idf.h: query q sees key j iff their words intersect, or j is q's own token in segment 0.  -> bool [B, len(qidx), n0 + n1]."""
    vis = (qbits[:, qidx, None] & kbits0[:, None, :n0]) != 0
    own = qidx[:, None] == torch.arange(n0, device=qidx.device)[None]
    vis = vis | own[None]
    if n1:
        vis = torch.cat([vis, (qbits[:, qidx, None] & kbits1[:, None, :n1]) != 0], -1)
    return vis


def attention_ref(c, qsel=None, device=None):
    """fp64 reference and bound of an ``idf_attention`` case (``attn_case``): -> (want, bound) [B, nq or len(qsel), C].  Keys and values
    are read from the K views and the V^T images exactly as the kernel is handed them, [:n] of each segment."""
    dev = device or "cpu"
    H, n0, n1, dt = c["H"], c["n0"], c["n1"], c["dt"]
    q = c["q"].to(dev)
    qidx = torch.arange(c["nq"], device=dev) if qsel is None else qsel.to(dev)
    k = c["k0"].to(dev)[:, :n0]
    v = c["vt0"].to(dev)[:, :, :n0].transpose(1, 2)
    if n1:
        k = torch.cat([k, c["k1"].to(dev)[:, :n1]], 1)
        v = torch.cat([v, c["vt1"].to(dev)[:, :, :n1].transpose(1, 2)], 1)
    B = q.shape[0]
    qh, kh, vh = _heads(q[:, qidx], H), _heads(k, H), _heads(v, H)
    vis_fn = None
    if c.get("qbits") is not None:
        qb, kb0 = c["qbits"].to(dev), c["kbits0"].to(dev)
        kb1 = c["kbits1"].to(dev) if n1 else None

        def vis_fn(lo, hi):
            vis = visibility(qb, kb0, n0, kb1, n1, qidx[lo:hi])
            return vis[:, None].expand(B, H, hi - lo, n0 + n1).reshape(B * H, hi - lo, n0 + n1)
    want, bound = _chunked(qh, kh, vh, vis_fn, c["d"] ** -0.5, dt)
    return _unheads(want, B), _unheads(bound, B)


def _qkv_heads(qkv, B, T, H, d=64):
    C = H * d
    x = qkv[:B * T, :3 * C].double().reshape(B, T, 3, H, d).permute(2, 0, 3, 1, 4).reshape(3, B * H, T, d)
    return x[0], x[1], x[2]


def qkv_attention_ref(c, device=None):
    """fp64 reference and bound of ``idf_attention_causal`` (c["causal"]) / ``idf_attention_qkv`` on the fused rows [q | k | v]:
    -> (want, bound) [B*T, H*64]."""
    dev = device or "cpu"
    B, T, H = c["B"], c["T"], c["H"]
    qh, kh, vh = _qkv_heads(c["qkv"].to(dev), B, T, H)
    tri = torch.ones(T, T, dtype=torch.bool, device=dev).tril()
    vis_fn = (lambda lo, hi: tri[lo:hi][None]) if c["causal"] else None
    want, bound = _chunked(qh, kh, vh, vis_fn, 64 ** -0.5, c["dt"])
    return _unheads(want, B).reshape(B * T, H * 64), _unheads(bound, B).reshape(B * T, H * 64)


def softmax_rows_ref(s32, scale, dt):
    """fp64 softmax(scale * s) of fp32 rows [R, n] and its bound (module docstring)."""
    x = scale * s32.double()
    mx = x.max(-1, keepdim=True).values
    p = torch.softmax(x, -1)
    delta = 2.0 ** -22 * (x.abs() + mx.abs()) + 2.0 ** -22
    bound = p * (torch.expm1(delta + delta.max(-1, keepdim=True).values) + (x.shape[-1] + 2) * EPS32 + UR[dt])
    if dt == "fp16":
        bound = bound + 2.0 ** -25
    return p, bound


# ---- the bound applied -----------------------------------------------------------------------------------------------------------
def rel_rms(got, want64):
    """rel-RMS error, computed where the reference lives."""
    want = want64.detach().double()
    got = got.detach().to(want.device).double().reshape(want.shape)
    return float(((got - want).pow(2).mean() / want.pow(2).mean().clamp_min(1e-60)).sqrt())


def outside(got, want64, bound):
    """(number of elements outside the bound, largest error / bound), computed where the reference lives.  A NaN in ``got`` is outside."""
    want = want64.detach().double()
    got = got.detach().to(want.device).double().reshape(want.shape)
    bound = bound.detach().to(want.device).double().reshape(want.shape)
    err = (got - want).abs()
    bad = ~(err <= bound)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    return int(bad.sum()), float(ratio.max())


def census_bound(want64, dt):
    return (UR[dt] + 2.0 ** -21) * want64.abs()


# ---- the fp32 replay of the kernels' arithmetic ---------------------------------------------------------------------------------------
def _replay_core(qh, kh, vh, vis, scale, T, p_type=None, prescale=True):
    """fp32: qh [G, c, d], kh / vh [G, n, d] (16-bit values in fp32) -> the 16-bit result as fp32."""
    c = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E32, dtype=torch.float32)
    if prescale:
        s = (qh * c).to(T).float() @ kh.transpose(-1, -2)
    else:
        s = (qh @ kh.transpose(-1, -2)) * c
    if vis is not None:
        s = s.masked_fill(~vis, float("-inf"))
    p = torch.exp2(s - s.max(-1, keepdim=True).values)
    p16 = p.to(p_type or T).float()
    return ((p16 @ vh) / p16.sum(-1, keepdim=True)).to(T).float()


def attention_replay(c, qsel=None, p_type=None, **mut):
    """The fp32 replay of an ``attn_case`` -> [B, nq or len(qsel), C] fp32 holding 16-bit values.  ``mut`` are the wrong kernels of
    tests/test_attention_refs.py: drop_keys (global key indices left out), dup_key, zero_pad_key, scale, head_shift, vt1_ld0,
    nan_pad, diag_seg1, word0_sees_all."""
    H, n0, n1, d = c["H"], c["n0"], c["n1"], c["d"]
    T = DTYPES[c["dt"]]
    qidx = torch.arange(c["nq"]) if qsel is None else qsel
    q = c["q"][:, qidx]
    B = q.shape[0]
    n0r = (n0 + 63) // 64 * 64 if mut.get("nan_pad") else n0     # the wrong kernel multiplies the pad columns by a zero weight
    k = c["k0"][:, :n0]
    vt0 = c["vt0"]
    v = vt0[:, :, :n0r].transpose(1, 2)
    if n1:
        vt1 = c["vt1"]
        if mut.get("vt1_ld0"):                               # segment 1's V^T rows addressed with segment 0's leading dimension
            flat = vt1.reshape(B, -1)
            idx = (torch.arange(vt1.shape[1])[:, None] * vt0.shape[2] + torch.arange(n1)[None]) % flat.shape[1]
            vt1 = flat[:, idx]
        k = torch.cat([k, c["k1"][:, :n1]], 1)
        v = torch.cat([v, vt1[:, :, :n1].transpose(1, 2)], 1)
    qh, kh, vh = _heads(q, H).float(), _heads(k, H).float(), _heads(v, H).float()
    if mut.get("head_shift"):                                # V of head h + 1
        vh = vh.reshape(B, H, -1, d).roll(-1, 1).reshape(B * H, -1, d)
    vis = None
    if c.get("qbits") is not None:
        vis = visibility(c["qbits"], c["kbits0"], n0, c["kbits1"] if n1 else None, n1, qidx)
        if mut.get("diag_seg1") and n1:
            vis[:, :, n0:] |= (qidx[:, None] == torch.arange(n1)[None])[None]
        if mut.get("word0_sees_all"):                        # an all-ones key word treated as "everybody sees it"
            kb = torch.cat([c["kbits0"][:, :n0]] + ([c["kbits1"][:, :n1]] if n1 else []), 1)
            vis |= (kb == -1)[:, None, :]
        vis = vis[:, None].expand(B, H, len(qidx), n0 + n1).reshape(B * H, len(qidx), n0 + n1)
    if mut.get("nan_pad"):                                   # pad keys: clamped duplicates of the last key, weight exactly 0, V = NaN
        assert not n1 and vis is None, "the nan_pad mutant is written for one unmasked segment"
        kh = torch.cat([kh, kh[:, -1:].expand(-1, n0r - n0, -1)], 1)
        vis = (torch.arange(n0r) < n0)[None, None].expand(B * H, len(qidx), n0r)
    if mut.get("drop_keys") is not None:
        keep = torch.ones(n0 + n1, dtype=torch.bool)
        keep[mut["drop_keys"]] = False
        kh, vh = kh[:, keep], vh[:, keep]
        vis = None if vis is None else vis[..., keep]
    if mut.get("dup_key") is not None:
        j = mut["dup_key"]
        kh, vh = torch.cat([kh, kh[:, j:j + 1]], 1), torch.cat([vh, vh[:, j:j + 1]], 1)
        if vis is not None:
            vis = torch.cat([vis, vis[..., j:j + 1]], -1)
    if mut.get("zero_pad_key"):
        kh, vh = torch.cat([kh, torch.zeros_like(kh[:, :1])], 1), torch.cat([vh, torch.zeros_like(vh[:, :1])], 1)
    out = _replay_core(qh, kh, vh, vis, mut.get("scale", d ** -0.5), T, p_type, mut.get("prescale", True))
    return _unheads(out, B)


def rebase_replay(c, shift):
    """The max-free softmax of attention4.hip in fp32: the reference value m of a query is the maximum of its first 64-key tile plus
    ``shift`` log2 units, rounded to the storage type, and is raised (O and l rescaled) to a later tile's maximum plus ``shift`` when
    that tile holds a P >= 2.  -> [B, nq, C] fp32 holding 16-bit values."""
    H, n0, n1, d = c["H"], c["n0"], c["n1"], c["d"]
    T = DTYPES[c["dt"]]
    k, v = c["k0"][:, :n0], c["vt0"][:, :, :n0].transpose(1, 2)
    if n1:
        k, v = torch.cat([k, c["k1"][:, :n1]], 1), torch.cat([v, c["vt1"][:, :, :n1].transpose(1, 2)], 1)
    qh, kh, vh = _heads(c["q"], H).float(), _heads(k, H).float(), _heads(v, H).float()
    cs = torch.tensor(d ** -0.5, dtype=torch.float32) * torch.tensor(LOG2E32, dtype=torch.float32)
    s = (qh * cs).to(T).float() @ kh.transpose(-1, -2)
    m = (s[..., :64].max(-1, keepdim=True).values + shift).to(T).float()
    num, den = torch.zeros_like(qh), torch.zeros_like(qh[..., :1])
    for t0 in list(range(0, n0, 64)) + [n0 + t for t in range(0, n1, 64)]:
        st = s[..., t0:min(t0 + 64, n0 if t0 < n0 else n0 + n1)]
        grew = torch.exp2(st - m).to(T).float().max(-1, keepdim=True).values >= 2.0
        m_new = torch.where(grew, (st.max(-1, keepdim=True).values + shift).to(T).float(), m)
        alpha = torch.exp2(m - m_new)
        num, den, m = num * alpha, den * alpha, m_new
        p16 = torch.exp2(st - m).to(T).float()
        num, den = num + p16 @ vh[:, t0:t0 + st.shape[-1]], den + p16.sum(-1, keepdim=True)
    return _unheads((num / den).to(T).float(), c["B"])


def qkv_replay(c, p_type=None, off_by_one=False):
    B, T, H = c["B"], c["T"], c["H"]
    Td = DTYPES[c["dt"]]
    qh, kh, vh = (t.float() for t in _qkv_heads(c["qkv"], B, T, H))
    vis = torch.ones(T, T, dtype=torch.bool).tril(-1 if off_by_one else 0)[None] if c["causal"] else None
    out = _replay_core(qh, kh, vh, vis, 64 ** -0.5, Td, p_type, prescale=False)
    return _unheads(out, B).reshape(B * T, H * 64)


def softmax_rows_replay(s32, scale, dt):
    sl2 = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E32, dtype=torch.float32)
    m = s32.max(-1, keepdim=True).values * sl2
    e = torch.exp2(s32 * sl2 - m)
    return (e * (1.0 / e.sum(-1, keepdim=True))).to(DTYPES[dt]).float()


# ---- input builders --------------------------------------------------------------------------------------------------------------------
def _nan(shape, T):
    return torch.full(shape, float("nan"), dtype=T)


def attn_case(B, H, d, nq, n0, n1, dt, kind="normal", mask=False, seed=0):
    """An ``idf_attention`` case on the CPU.  q and k0 are column slices of ONE fused buffer [B, rows, 2C] whose rows behind nq (q half)
    and behind n0 (k half) are NaN; k1 is a view of a buffer with two NaN rows behind n1; the V^T images have their pad columns (up to
    the multiple of 64) NaN.  kind: "normal" | "flat" | "census" | "negative" | a spike case of ``SPIKES``."""
    T = DTYPES[dt]
    C = H * d
    sd = 900 + 7 * seed + d + nq + 3 * n0 + 5 * n1
    if nq > 4096:                                           # the resident-key shapes: 1021 seeded rows, walked with a stride (cheap to build)
        q = gen((B, 1021, C), sd)[:, (torch.arange(nq) * 389) % 1021]
    else:
        q = gen((B, nq, C), sd)
    k, v = gen((B, n0, C), sd + 1), gen((B, n0, C), sd + 2)
    k1, v1 = gen((B, n1, C), sd + 3), gen((B, n1, C), sd + 4)
    if kind == "census":
        q = torch.zeros(B, nq, C)
        j = torch.arange(n0 + n1)
        hot = torch.zeros(n0 + n1, d)
        hot[j, j % d] = 1.0
        hot = hot.repeat(1, H)[None].expand(B, -1, -1)
        v, v1 = hot[:, :n0].clone(), hot[:, n0:].clone()
    elif kind == "negative":
        q = torch.ones(B, nq, C)
        k, k1 = -4.0 + 0.25 * k, -4.0 + 0.25 * k1
        v, v1 = 1.0 + 0.25 * v, 1.0 + 0.25 * v1              # outputs near 1: a pad key (V = 0) that takes the softmax moves them by 1
    elif kind == "flat":                                      # no score a whole log2 unit above another: no kernel re-bases
        q = q * 2.0 ** -4
    elif kind != "normal":
        assert nq == n0 == 640 and n1 == 184, "the spike cases are written for 640 + 184 keys"
        if kind == "late":
            k[:, 500] = q[:, 7] * 4.0                       # a finite spike in the 8th tile
        elif kind == "first":
            k[:, 3] = q[:, 300] * 6.0                       # a spike in the first tile: every later P underflows
        elif kind == "overflow":
            k[:, 450] = q[:, 9] * 40.0                      # hundreds of log2 units: P = inf without a running max ("huge-spike")
        elif kind == "seg1":
            k1[:, 180] = q[:, 11] * 5.0                     # inside the 56-key tail tile of segment 1
        elif kind == "creep":
            for t in range(10):                             # a maximum that creeps up by ~3 log2 units per tile
                k[:, 64 * t + 5] = q[:, 21] * (0.33 * (t + 1) * (80.0 / d) ** 0.5)
        else:
            raise ValueError(kind)
    rows = max(nq, n0) + 2
    qk = _nan((B, rows, 2 * C), T)
    qk[:, :nq, :C] = q.to(T)
    qk[:, :n0, C:] = k.to(T)
    vt0 = _nan((B, C, (n0 + 63) // 64 * 64), T)
    vt0[:, :, :n0] = v.to(T).transpose(1, 2)
    c = dict(B=B, H=H, d=d, nq=nq, n0=n0, n1=n1, dt=dt, kind=kind, qk=qk, q=qk[:, :nq, :C], k0=qk[:, :n0, C:], vt0=vt0, k1=None, vt1=None)
    if n1:
        k1b = _nan((B, n1 + 2, C), T)
        k1b[:, :n1] = k1.to(T)
        vt1 = _nan((B, C, (n1 + 63) // 64 * 64), T)
        vt1[:, :, :n1] = v1.to(T).transpose(1, 2)
        c.update(k1b=k1b, k1=k1b[:, :n1], vt1=vt1)
    if mask:
        # five instances; ~40 % of the tokens in none.  Queries carry bit 31, which the unconditional keys of segment 1 (word -1) share;
        # every 7th query (inside segment 0) has word 0 and sees only itself; segment-1 keys 0..4 are the instances' own, key 7 of
        # the last batch element is seen by nobody, and key 9 has a word that query 9 (word 0 or not) does not share unless it is in
        # instance 0: the own-token rule must not reach into segment 1
        g = torch.Generator().manual_seed(sd + 9)
        words = ((torch.rand(B, max(nq, n0), 5, generator=g) < 0.2).int() * (1 << torch.arange(5))).sum(-1).int()
        qb = (words[:, :nq] | torch.tensor(-2 ** 31, dtype=torch.int32)).contiguous()
        qb[:, 0:min(nq, n0):7] = 0
        kb0 = torch.zeros(B, n0 + 3, dtype=torch.int32)
        kb0[:, :n0] = words[:, :n0]
        kb0[:, 5:n0:11] = -1                                   # a few unconditional keys in segment 0 as well
        c.update(qbits=qb, kbits0=kb0, kbits1=None)
        if n1:
            kb1 = torch.full((B, n1 + 3), -1, dtype=torch.int32)
            kb1[:, :min(5, n1)] = (1 << torch.arange(5)).int()[:min(5, n1)]
            if n1 > 9:
                kb1[B - 1, 7] = 0
                kb1[:, 9] = 1
            c["kbits1"] = kb1
    return c


def qkv_case(B, T, H, dt, causal, kind="normal", pad=8):
    """A fused-qkv case: rows b*T + t of [q | k | v], each H*64 wide, leading dimension 3*H*64 + pad with NaN pad columns and two NaN
    rows behind row B*T."""
    Td = DTYPES[dt]
    C = H * 64
    x = gen((B * T, 3 * C), 950 + T + 3 * H + int(causal))
    if kind == "census":
        x[:, :C] = 0.0
        hot = torch.zeros(T, 64)
        hot[torch.arange(T), torch.arange(T) % 64] = 1.0
        x[:, 2 * C:] = hot.repeat(B, H)
    buf = _nan((B * T + 2, 3 * C + pad), Td)
    buf[:B * T, :3 * C] = x.to(Td)
    return dict(B=B, T=T, H=H, dt=dt, causal=causal, kind=kind, buf=buf, qkv=buf[:, :3 * C])


def softmax_case(rows, n, dt, pad=4):
    """fp32 scores [rows, n] in rows of n + pad (NaN pad); row 0 has one dominant entry (every other probability underflows)."""
    s = gen((rows, n), 970 + n + rows, 3.0)
    s[0, n // 2] = 400.0
    buf = torch.full((rows, n + pad), float("nan"))
    buf[:, :n] = s
    return dict(rows=rows, n=n, dt=dt, buf=buf, s=buf[:, :n], scale=0.125)


def guarded_out(shape, T, device="cpu", col_pad=8, batch_gap=0):
    """An output view [B, nq, C] inside a NaN-filled buffer with ``col_pad`` guard columns, one guard row per batch element and
    ``batch_gap`` extra elements between the batch elements (an unaligned batch stride): (view, check); ``check()`` -> "" or what was
    overwritten."""
    B, nq, C = shape
    ld = C + col_pad
    sb = (nq + 1) * ld + batch_gap
    buf = torch.full((B * sb + 8,), float("nan"), dtype=T, device=device)
    view = buf.as_strided((B, nq, C), (sb, ld, 1))
    mask = torch.ones(buf.numel(), dtype=torch.bool, device=device)
    mask.as_strided((B, nq, C), (sb, ld, 1)).fill_(False)

    def check():
        return "" if bool(torch.isnan(buf[mask]).all()) else "a guard element was overwritten"
    return view, check


# ---- the dispatch rules of idf_attention (csrc/attention.hip) and of the three LDS-DMA launchers ----------------------------------------
SUPPORTED_D = (8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 88, 96, 120, 128, 152, 160)
UNSUPPORTED_D = (104, 112, 136, 144)                       # 7 or 9 K-steps of 16: launch_attn has no instantiation


def dispatch(d, nq, n0, n1, B, H, *, attn2, attn8, mask=False, ldo=None, so=None, lds_ok=True):
    """Which kernel takes an ``idf_attention`` launch under the knob values IDF_TUNE_ATTN2 / IDF_TUNE_ATTN8: -> dict(kernel, qb, counter).
    kernel: "attn4w" | "attn4" | "attn8" | "attn32" | "attn32_res" | "attn32_mask" | "unsupported"; qb = queries per workgroup;
    counter = the launch counter that moves ("attn2", "attn8", "res" or None).  ``ldo`` / ``so``: leading dimension and batch stride of
    the output in elements (None: aligned); ``lds_ok``: every other row start and batch stride is 16-byte aligned.  The gates of
    idf_launch_attn4w, idf_launch_attn4 and idf_launch_attn8 are one rule: n0 % 8 == n1 % 8 == 0 and everything 16-byte aligned (the
    32-bit offset gates are out of reach of any test size)."""
    ldo = d * H if ldo is None else ldo
    so = 0 if so is None else so
    dma = (not mask) and n0 % 8 == 0 and n1 % 8 == 0 and ldo % 8 == 0 and so % 8 == 0 and lds_ok
    if dma and attn2 >= 4 and attn2 != 6 and d == 40:
        return dict(kernel="attn4w", qb=512 if attn2 == 4 else 256, counter="attn2")
    if dma and attn2 > 0 and d in (24, 40, 56):
        return dict(kernel="attn4", qb=512 if attn2 == 2 else 256, counter="attn2")
    if dma and attn8 > 0 and d in (80, 160):
        if d == 80:
            qb = 256 if attn8 in (2, 6) else 128
        else:
            qb = 128 if (attn8 == 4 or (attn8 != 2 and nq < 256)) else 256
        return dict(kernel="attn8", qb=qb, counter="attn8")
    if d % 8 or d > 160 or (d + 15) // 16 in (7, 9):
        return dict(kernel="unsupported", qb=0, counter=None)
    if mask:
        return dict(kernel="attn32_mask", qb=128, counter=None)
    nqb = -(-nq // 128)
    tiles = -(-n0 // 64) + -(-n1 // 64)
    qpw = min(8, max(1, (nqb * H * B) // 1024))
    if tiles <= 2 and nqb >= 2 and qpw > 1:
        return dict(kernel="attn32_res", qb=128 * qpw, counter="res")
    return dict(kernel="attn32", qb=128, counter=None)


def blocks(case_dims, qb):
    B, H, d, nq, n0, n1 = case_dims
    return -(-nq // qb) * H * B


# ---- the case lists: the SMALLEST shapes that reach each path -------------------------------------------------------------------------
FAMILIES = {                                               # name -> (IDF_TUNE_ATTN2, IDF_TUNE_ATTN8, kernel, head dims)
    "a32": (0, 0, "attn32", SUPPORTED_D),
    "a4-m1": (1, 0, "attn4", (24, 40, 56)), "a4-m2": (2, 0, "attn4", (24, 40, 56)), "a4-m3": (3, 0, "attn4", (24, 40, 56)),
    "a4w-m4": (4, 0, "attn4w", (40,)), "a4w-m5": (5, 0, "attn4w", (40,)),
    "a8-m1": (0, 1, "attn8", (80, 160)), "a8-m2": (0, 2, "attn8", (80, 160)), "a8-m3": (0, 3, "attn8", (80, 160)),
    "a8-m4": (0, 4, "attn8", (80, 160)), "a8-m5": (0, 5, "attn8", (80, 160)), "a8-m6": (0, 6, "attn8", (80, 160)),
}
STAR_N0 = (8, 56, 64, 72, 128, 136)
STAR_N1 = (0, 8, 64, 184)
A32_N0 = (1, 7, 63, 65, 77)
A32_N1 = (1, 5)
BASE_N0, BASE_N1 = 72, 8                                   # both segments present, a tail tile in each


def family_qb(fam, d, nq=1 << 20):
    a2, a8, _, _ = FAMILIES[fam]
    if fam == "a32":
        return 128
    return dispatch(d, nq, 8, 8, 1, 1, attn2=a2, attn8=a8)["qb"]


def star(fam, d):
    """The one-factor-at-a-time star of a family at head dim d: (B, H, d, nq, n0, n1) around (1, 3, d, QB + 1, 72, 8); H = 3 makes the
    head strides odd multiples of d; the (B, H) points make the block total divisible by 8 (2 x 4 x 1, 2 x 4 x 3) and not (3, 6, 9)."""
    qb = family_qb(fam, d)
    base = (1, 3, d, qb + 1, BASE_N0, BASE_N1)
    pts = [base]
    nqs = [1, qb - 1, qb, qb + 1, 2 * qb + 1] + ([31, 32, 33] if fam == "a32" else [])
    if fam.startswith("a8") and d == 160 and FAMILIES[fam][1] in (1, 3, 5, 6):
        nqs += [255, 256, 257]                               # d = 160: 4-wave workgroups below 256 queries, 8-wave from there
    for nq in nqs:
        pts.append((1, 3, d, nq, BASE_N0, BASE_N1))
    for n0 in STAR_N0 + (A32_N0 if fam == "a32" else ()):
        pts.append((1, 3, d, qb + 1, n0, BASE_N1))
    for n1 in STAR_N1 + (A32_N1 if fam == "a32" else ()):
        pts.append((1, 3, d, qb + 1, BASE_N0, n1))
    pts += [(2, 4, d, qb, BASE_N0, BASE_N1), (2, 4, d, 2 * qb + 1, BASE_N0, BASE_N1), (3, 1, d, qb + 1, BASE_N0, BASE_N1), (4, 2, d, 7, BASE_N0, BASE_N1)]
    return list(dict.fromkeys(pts))


STAR_D = {"a32": (40, 64)}                                 # the 32-query kernel: the full star at an MFMASUM d and at a VALU-sum d


def family_cases(fam):
    """(B, H, d, nq, n0, n1, kind, mask) of a family: the star at every head dim (the 32-query kernel: at STAR_D, and the base point and a
    ragged one at every other supported d), the exact-data cases and, for the DMA kernels, the spike cases."""
    out = []
    for d in FAMILIES[fam][3]:
        if fam != "a32" or d in STAR_D["a32"]:
            out += [p + ("normal", False) for p in star(fam, d)]
        else:
            out += [(1, 3, d, 129, BASE_N0, BASE_N1, "normal", False), (2, 2, d, 33, 77, 5, "normal", False)]
        qb = family_qb(fam, d)
        for n0, n1 in ((72, 0), (264, 0), (136, 184), (1208, 0)):
            out.append((1, 2, d, min(qb + 1, 65), n0, n1, "census", False))
        out.append((1, 2, d, 33, 72, 8, "negative", False))
        out.append((1, 2, d, 33, 1208, 0, "negative", False))
        if fam == "a32":
            out.append((1, 2, d, 33, 77, 5, "census", False))
            out.append((1, 2, d, 33, 77, 0, "negative", False))
    if fam != "a32":
        d0 = FAMILIES[fam][3]
        for d in (d0 if fam.startswith("a8") else (40,)):
            for kind in SPIKES:
                out.append((1, 2, d, 640, 640, 184, kind, False))
    return list(dict.fromkeys(out))


SPIKES = ("late", "first", "overflow", "seg1", "creep")


def mask_cases():
    """The MASK instantiations of the 32-query kernel: every supported d at a ragged two-block shape with both segments, a star of
    nq / n0 / n1 at d = 40, and the census of the visible set."""
    out = [(2, 2, d, 130, 136, 184, "normal", True) for d in SUPPORTED_D]
    out += [(1, 3, 40, nq, 264, 8, "normal", True) for nq in (1, 31, 32, 33, 127, 128, 129, 257)]
    out += [(1, 3, 40, 65, n0, 8, "normal", True) for n0 in (65, 72, 77, 128, 136)]
    out += [(1, 3, 40, 65, 72, n1, "normal", True) for n1 in (0, 1, 5, 64, 184)]
    out += [(1, 2, d, 65, 136, 184, "census", True) for d in (8, 40, 64, 160)]
    return out


# resident keys: B * H * ceil(nq / 128) = 4 * 4 * 129 = 2064 in [2048, 3072): two query blocks per workgroup, an odd block count per
# (b, h) so the last workgroup of a head walks ONE block, and that block holds 5 queries.  Its 16 * 65 = 1040 workgroups are a
# multiple of 8 (the XCD remap is on); RES_PLAIN's 3 * 3 * 115 = 1035 are not (plain block order)
RES_NQ = 128 * 128 + 5
RES_CASES = [(4, 4, d, RES_NQ, 77, n1, "normal", False) for d, n1 in ((8, 0), (40, 0), (80, 0), (160, 0))] + \
            [(4, 4, 40, RES_NQ, 56, 5, "normal", False), (4, 4, 40, RES_NQ, 77, 0, "census", False)]
RES_PLAIN = (3, 3, 40, 128 * 228 + 5, 77, 0, "normal", False)  # 9 * 229 = 2061 blocks
RES_BELOW = (4, 4, 40, 128 * 126 + 5, 77, 0, "normal", False)  # 16 * 127 = 2032 < 2048: must NOT take the resident-key path

CAUSAL_T = (1, 15, 16, 17, 31, 32, 33, 64, 65, 128)
QKV_T = CAUSAL_T + (129, 257, 288)
SOFTMAX_N = (4, 60, 64, 68, 256, 4096)
SOFTMAX_ROWS = (1, 3, 300)


def qkv_cases():
    """(B, T, H, causal, kind)"""
    out = []
    for causal, Ts in ((True, CAUSAL_T), (False, QKV_T)):
        for T in Ts:
            out.append((2 if T < 200 else 1, T, 3 if T % 2 else 1, causal, "normal"))
        for T in (17, 65, 128) + (() if causal else (257,)):
            out.append((1, T, 1, causal, "census"))
    return out


def subset(nq, keep=48):
    """Query indices for the CPU proofs of a large case: the first and last 8 and a stride in between (every query is independent)."""
    if nq <= keep:
        return None
    mid = torch.linspace(8, nq - 9, keep - 16).long()
    return torch.unique(torch.cat([torch.arange(8), mid, torch.arange(nq - 8, nq)]))
