"""Cases, fp64 references, the per-element bound, the row sampler and the dispatch mirror for the row-resident fused kernels: the fused
q | k | v projections (csrc/qkv_fused.hip qkv320w_kernel, csrc/qkv640_fused.hip qkv640w_kernel), the GEGLU projection of the C = 640
level (csrc/geglu_fused.hip geglu640w_kernel) and the fused MLP (csrc/mlp_fused.hip mlp320_kernel / mlp320w_kernel).  No GPU and no HIP
library: tests/test_row_kernel_refs.py proves this module on the CPU, tests/test_row_kernels_gpu.py applies it to the kernels.

Every one of the M rows is distinct (seeded generator, on the device the case is built on), and the (mu, rstd) handed in are NOT the
rows' own in the default case: include/idf.h defines the fold as rstd[m] * (acc - mu[m] * c[n]) + d[n] with the statistics as given,
so every output is tied to its own row's pair and a kernel that indexed them wrongly, or recomputed them, is outside the bound.

Bounds (tests/gemm_conv_cases.py: |got - want| <= U |want| + slack, 0 elements outside):
  q | k | v   gemm_ref's slack + 2^-16 rstd[m] |mu[m]| |c[n]|: the kernels carry -mu c[n] as a k-step of 16-bit hi + lo products, two
              factors each good to 2^-17 (csrc/qkv_fused.hip header);
  GEGLU       gemm_ref(geglu=True) as it stands;
  fused MLP   ``mlp_ref``: H in fp64, rounded to the 16-bit type as the kernel does, the second product in fp64; the intermediate's
              allowance is e = slack1 + flip (one ulp where the fp64 H lies within slack1 of a rounding midpoint), the output's
              |gate| (e |W2|^T + 1280 2^-24 |H16| |W2|^T).
"""
import torch

from tests.gemm_conv_cases import EPS32, family_takes, gemm_ref, guarded, outside   # noqa: F401  (re-exported)
from tests.small_kernel_cases import DTYPES, RMS_BAR, U, gen, rel_rms               # noqa: F401  (re-exported)

LN_EPS = 1e-5
SPLIT16 = 2.0 ** -16                                     # the hi + lo mean term of the q | k | v kernels
# kernel -> K, N (weight rows), BM (tile rows), columns of `out`
KERNELS = {
    "qkv320": dict(K=320, N=960, BM=256, cols=640),
    "qkv640": dict(K=640, N=1920, BM=128, cols=1280),
    "geglu640": dict(K=640, N=5120, BM=128, cols=2560),
    "mlp": dict(K=320, N=2560, BM=128, cols=320),
}
MLP_C, MLP_H = 320, 1280
KINDS = ["normal", "large_mean10", "large_mean100", "tiny_mean", "zero_row"]
E_UNSUPPORTED = -3


def m0(kernel, cus):
    """The least M idf_gemm hands to the row kernel: two tiles per CU (csrc/mw_row.h mw_row_eligible); the MLP takes one tile."""
    return KERNELS[kernel]["BM"] * (1 if kernel == "mlp" else 2 * cus)


# A zero row's q | k | v output is d[n] itself and its slack is 0: the bound is U |d[n]|, which the correctly rounded fp16 value of a
# SUBNORMAL d[n] need not meet (half a subnormal step is 2^-25, more than 2^-10 |d| below 2^-15).  The d tables stay at or above the
# smallest normal fp16 number.  (A zero row's GEGLU output d_v gelu(d_g) can still be subnormal; its bound carries 2.6e-5 |d_v| for the
# gelu fit, and tests/test_row_kernel_refs.py checks on these very tables that this covers half a subnormal step wherever it has to.)
D_FLOOR = 2.0 ** -14
HALF_SUBNORMAL_STEP = {"bf16": 2.0 ** -134, "fp16": 2.0 ** -25}


def zero_rows(M, BM):
    """The all-zero rows of the "zero_row" kind: in the first tile, in the second, and the very last row (all in ``sample_rows``)."""
    return [5, min(M - 1, BM + 37), M - 1]


# ---- case builders -------------------------------------------------------------------------------------------------------------
def row_inputs(M, K, dt, kind="normal", device="cpu", seed=0, BM=128):
    """x [M, K] in the 16-bit type, M distinct rows, and the handed-in statistics [M, 2] fp32, both on ``device``."""
    g = torch.Generator(device=device).manual_seed(900 + seed)
    rn = lambda *s: torch.randn(s, generator=g, device=device, dtype=torch.float32)
    ru = lambda *s: torch.rand(s, generator=g, device=device, dtype=torch.float32)
    base = rn(M, K)
    sign = torch.where(ru(M) < 0.5, -1.0, 1.0)
    if kind.startswith("large_mean"):
        x = base + float(kind[len("large_mean"):]) * sign[:, None]
    elif kind == "tiny_mean":
        x = 1.5 * (base - base.mean(-1, keepdim=True))
    else:
        x = 1.5 * base + 0.8 * rn(M, 1)
    x = x.to(DTYPES[dt])
    del base
    xd = x.double()
    mu = xd.mean(-1)
    rstd = 1.0 / ((xd - mu[:, None]).pow(2).mean(-1) + LN_EPS).sqrt()
    del xd
    mu, rstd = mu.float(), rstd.float()
    if kind in ("normal", "zero_row"):                   # not the rows' own: every output is tied to its row's pair
        mu = mu + 0.3 * rn(M)
        rstd = rstd * (0.5 + ru(M))
    elif kind == "tiny_mean":                            # in fp16 the lo half of the split of mu is subnormal
        mu = sign * 1e-4 * (0.5 + ru(M))
    stats = torch.stack([mu, rstd], -1).contiguous()
    if kind == "zero_row":
        for r in zero_rows(M, BM):
            x[r] = 0
            stats[r, 0], stats[r, 1] = 0.0, LN_EPS ** -0.5
    return x, stats


def weights(kernel, dt):
    """The kernel's constant operands (CPU): w [N, K] 16-bit (UNPACKED for the GEGLU kernels: [value rows | gate rows]), c its fp32 row
    sums, d fp32; for the GEGLU kernels also the period-32 images wp / cp / dp; for the MLP w2 [320, 1280], b2 and the packed images."""
    from instancediffusion_amd.engine import pack_geglu
    k = KERNELS[kernel]
    seed = 910 + 10 * list(KERNELS).index(kernel)
    w = (gen((k["N"], k["K"]), seed, k["K"] ** -0.5) * (1 + 0.2 * gen((k["K"],), seed + 1))).to(DTYPES[dt])
    c = w.float().sum(-1)
    d = 0.3 * gen((k["N"],), seed + 2)
    d = torch.where(d.abs() < D_FLOOR, torch.where(d < 0, -D_FLOOR, D_FLOOR), d)
    out = dict(w=w, c=c, d=d)
    if kernel in ("geglu640", "mlp"):
        out["wp"], out["dp"] = pack_geglu(w, d, 32)
        out["cp"] = pack_geglu(w, c, 32)[1]
    if kernel == "mlp":
        out["w2"] = gen((MLP_C, MLP_H), seed + 3, MLP_H ** -0.5).to(DTYPES[dt])
        out["b2"] = 0.2 * gen((MLP_C,), seed + 4)
    return out


def row_case(kernel, M, dt, kind="normal", device="cpu", seed=0):
    k = KERNELS[kernel]
    x, stats = row_inputs(M, k["K"], dt, kind, device, seed + list(KERNELS).index(kernel), k["BM"])
    return dict(kernel=kernel, dt=dt, kind=kind, M=M, x=x, stats=stats, **weights(kernel, dt))


# ---- the row sampler -----------------------------------------------------------------------------------------------------------
def sample_tiles(M, BM, G):
    """Tiles 0, 1, G - 1, G, G + 1 and one in the middle of the wider gap between them and the last two."""
    tiles = M // BM
    gaps = [(2, G - 2), (G + 2, tiles - 3)]
    lo, hi = max(gaps, key=lambda g: g[1] - g[0])
    return sorted({t for t in (0, 1, G - 1, G, G + 1, (lo + hi) // 2 if lo <= hi else tiles // 2) if 0 <= t < tiles})


def sample_rows(M, BM, G, total=2048, seed=0):
    """Sorted row indices: every row of tiles 0, 1, G - 1, G, G + 1 (G = the grid: where a persistent workgroup wraps round to its second
    tile) and of one tile in the middle, the last two tiles with whatever rows follow them, and a seeded scatter of single rows up
    to about ``total`` (256 at least)."""
    rows = set(range(max(0, (M // BM - 2) * BM), M))
    for t in sample_tiles(M, BM, G):
        rows.update(range(t * BM, (t + 1) * BM))
    n = max(256, total - len(rows))
    rows.update(torch.randint(0, M, (n,), generator=torch.Generator().manual_seed(930 + seed)).tolist())
    return torch.tensor(sorted(rows))


# ---- fp64 references -----------------------------------------------------------------------------------------------------------
def _take(t, rows):
    return (t if rows is None else t[rows.to(t.device)]).cpu()


def round_flip(h, slack1, dt):
    """One ulp of h's 16-bit neighbourhood where h lies within slack1 of a rounding midpoint (a value inside the allowance rounds to
    the other neighbour), 0 elsewhere.  The neighbours come from the bit pattern: right in every binade and among the subnormals."""
    T = DTYPES[dt]
    h16 = h.to(T)
    bits = h16.view(torch.int16).to(torch.int32)
    mag, sgn = bits & 0x7fff, torch.where(bits < 0, -1.0, 1.0).double()
    val = lambda m: m.to(torch.int16).view(T).double()
    one = val(torch.ones_like(mag))
    away = sgn * val(mag + 1)
    toward = torch.where(mag == 0, -sgn * one, sgn * val((mag - 1).clamp_min(0)))
    c = h16.double()
    dist = torch.minimum((h.double() - (c + away) / 2).abs(), (h.double() - (c + toward) / 2).abs())
    ulp = torch.maximum((away - c).abs(), (toward - c).abs())
    return torch.where(dist <= slack1, ulp, torch.zeros_like(ulp))


def mlp_core(x, stats, w1, c1, d1, w2, b2, dt, cd=torch.float64, round_h=True):
    """(y, S): y = W2 . H16 + b2 with H = value * gelu(gate half) of LN(x) W1^T + d1 rounded to the 16-bit type before the second product
    (include/idf.h idf_mlp_geglu; w1 / c1 / d1 UNPACKED), and its allowance S = e |W2|^T + 1280 2^-24 |H16| |W2|^T, e = slack1 + flip."""
    h, slack1 = gemm_ref(x, w1, bias=d1, ln_row=(stats, c1), geglu=True, cd=cd)
    h16 = h.to(DTYPES[dt]) if round_h else h
    y = h16.to(cd) @ w2.to(cd).t() + b2.to(cd)
    e = slack1 + round_flip(h, slack1, dt)
    w2a = w2.double().abs().t()
    return y, e @ w2a + MLP_H * EPS32 * (h16.double().abs() @ w2a)


def mlp_gated(x, y, S, gate):
    """(want, slack) of out = x + [gate *] y from ``mlp_core``'s (y, S); ``gate`` a float as the kernel reads it (fp32), or None."""
    g = 1.0 if gate is None else float(torch.tensor(gate, dtype=torch.float32))
    return x.to(y.dtype) + torch.tensor(g, dtype=y.dtype) * y, abs(g) * S


def mlp_ref(x, stats, w1, c1, d1, w2, b2, gate, dt, cd=torch.float64, round_h=True):
    """x + [gate *] (W2 . H16 + b2) -> (want, slack)."""
    return mlp_gated(x, *mlp_core(x, stats, w1, c1, d1, w2, b2, dt, cd, round_h), gate)


def row_ref(case, rows=None, cd=torch.float64, stats="given", **kw):
    """(want, slack) of the case on ``rows`` (all when None): [n, N] for q | k | v (the V columns behind the q | k ones, NOT
    transposed), [n, N / 2] for GEGLU, [n, 320] for the MLP (``gate=``).  stats="self": of the rows themselves (ln_stats = NULL)."""
    x = _take(case["x"], rows)
    st = None if stats == "self" else _take(case["stats"], rows)
    kernel = case["kernel"]
    if kernel == "mlp":
        return mlp_ref(x, st, case["w"], case["c"], case["d"], case["w2"], case["b2"], kw.get("gate"), case["dt"], cd,
                       kw.get("round_h", True))
    if kernel == "geglu640":
        if kw.get("act"):                                # the GEGLU shape as a plain projection with an activation
            return gemm_ref(x, case["wp"], bias=case["dp"], ln_row=(st, case["cp"]), act=kw["act"], cd=cd)
        return gemm_ref(x, case["w"], bias=case["d"], ln_row=(st, case["c"]), geglu=True, cd=cd)
    want, slack = gemm_ref(x, case["w"], bias=case["d"], ln_row=(st, case["c"]), cd=cd)
    if st is not None and kw.get("split", True):        # split=False: the persistent kernel's bound (an fp32 fma per element)
        slack = slack + SPLIT16 * mean_term(st, case["c"])
    return want, slack


def mean_term(st, c):
    """rstd[m] |mu[m]| |c[n]|: the size of the mean term of the fold."""
    return (st[:, 1].double() * st[:, 0].double().abs())[:, None] * c.double().abs()[None]


def spacing(want, dt):
    """The step of the 16-bit type at each |want| (the subnormal step below the smallest normal number)."""
    tiny = {"bf16": 2.0 ** -126, "fp16": 2.0 ** -14}[dt]
    return U[dt] * torch.exp2(torch.floor(torch.log2(want.double().abs().clamp_min(tiny))))


def pair_fraction_bar(case, rows, want):
    """An upper estimate, from the fp64 reference alone, of the share of outputs on which the row kernel and the persistent kernel round
    apart.  Both add the same K products in fp32 and fold the same mean term, but at different places of the chain: the row kernels
    as one more k-step of the accumulator (q | k | v: 16-bit hi + lo factors, each good to U / 2, so (U / 2)^2 of the term together), the
    persistent kernel as one fma behind it.  The partial sums of the two chains differ by the term itself, so each of the K / 16 + 1
    accumulator updates may round differently by 2^-24 of it on either side:
        delta[m, n] = ((U / 2)^2 + 2 (K / 16 + 1) 2^-24) rstd[m] |mu[m]| |c[n]|      (through v gelu(g) for GEGLU, slope <= 1.13)
    Two values delta apart round to different 16-bit numbers with probability delta / spacing: the bar is the mean of
    min(1, delta / spacing(want)) over the sampled elements.  It grows in proportion to |mean| / std; the GPU tests use it at the
    ratios 10 and 100, where the fractions stated for the default cases (1e-2, 2e-2) are out of two correct kernels' reach."""
    kernel, dt = case["kernel"], case["dt"]
    K = KERNELS[kernel]["K"]
    st = _take(case["stats"], rows)
    coef = 2 * (K // 16 + 1) * EPS32 + (0.0 if kernel == "geglu640" else (U[dt] / 2) ** 2)
    delta = coef * mean_term(st, case["c"])
    if kernel == "geglu640":
        acc, _ = gemm_ref(_take(case["x"], rows), case["w"], bias=case["d"], ln_row=(st, case["c"]))
        n = acc.shape[-1] // 2
        v, g = acc[:, :n], acc[:, n:]
        gelu = g * 0.5 * (1.0 + torch.erf(g / 2.0 ** 0.5))
        delta = delta[:, :n] * gelu.abs() + 1.13 * v.abs() * delta[:, n:]
    return float((delta / spacing(want, dt)).clamp_max(1.0).mean())


# ---- the dispatch rules of csrc/mw_row.h (mw_row_eligible, mw_row_vt_eligible), the idf_launch_* guards and idf_mlp_geglu ------------
def row_takes(kernel, M, cus, *, K=None, N=None, lda=None, ldw=None, ldo=None, ld_vt=None, stats=True, act=None, res=False,
              geglu=None, period=32, vt=None, vt_col0=None, batch=1, out_stats=False, knob=1, big_mode=1, C=MLP_C, ldw2=None):
    """Does the launch run on the row kernel ``kernel``?  Leading dimensions None: dense.  For "mlp": does idf_mlp_geglu accept the
    shape (it has no other kernel: what it declines is IDF_E_UNSUPPORTED / IDF_E_ARG / IDF_E_ALIGN).  The 16-byte alignment of the
    base pointers, the 16-bit type and the presence of `bias`, which the C++ conditions also ask for, are taken for granted: every
    launch of the tests has them.  The GPU tests pass M, the leading dimensions, ``stats`` and ``act``; the other options (K, N, res,
    period, vt, vt_col0, batch, out_stats, knob, big_mode) exist for the hand-written table of tests/test_row_kernel_refs.py, which
    walks the remaining C++ conditions."""
    k = KERNELS[kernel]
    if kernel == "mlp":
        ldx, ldw1 = (C if lda is None else lda), (C if ldw is None else ldw)
        ldo = C if ldo is None else ldo
        ldw2 = MLP_H if ldw2 is None else ldw2
        if C != MLP_C or M <= 0 or M % k["BM"]:
            return False
        if ldx < C or ldo < C or ldw1 < C or ldw2 < MLP_H or any(ld % 8 for ld in (ldx, ldo, ldw1, ldw2)):
            return False
        return 64 * ldw1 * 2 < 2 ** 31 and 320 * ldw2 * 2 < 2 ** 31 and stats
    Kk, Nn, BM, cols = (k["K"] if K is None else K), (k["N"] if N is None else N), k["BM"], k["cols"]
    is_geglu = kernel == "geglu640"
    geglu = is_geglu if geglu is None else geglu
    vt = (not is_geglu) if vt is None else vt
    lda, ldw = (Kk if lda is None else lda), (Kk if ldw is None else ldw)
    ldo = (Nn // 2 if geglu else (cols if vt else Nn)) if ldo is None else ldo
    if knob == 0 or big_mode == 0 or batch != 1:
        return False
    # mw_row_eligible
    if Kk != k["K"] or Nn != k["N"]:
        return False
    if M % BM or M < BM * 2 * cus:
        return False
    if not stats:
        return False
    if lda < Kk or ldw < Kk or ldo < cols or lda % 8 or ldw % 8 or ldo % 8:
        return False
    if Nn * ldw * 2 >= 2 ** 31 or BM * ldo * 2 >= 2 ** 31:
        return False
    extra = act is not None or res
    if is_geglu:                                         # idf_launch_geglu640w: exactly BIAS | GEGLU | GEGLU_P32 | LN_ROW, no by-product
        return not vt and geglu and period == 32 and not extra and not out_stats
    # idf_launch_qkv320w / idf_launch_qkv640w: mw_row_vt_eligible, vt_col0 = 2 C, exactly BIAS | LN_ROW
    ld_vt = M if ld_vt is None else ld_vt
    if not vt or ld_vt < M or ld_vt % 8 or 32 * ld_vt * 2 >= 2 ** 31:
        return False
    return (cols if vt_col0 is None else vt_col0) == cols and not geglu and not extra and not out_stats
