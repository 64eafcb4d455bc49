"""tests/row_kernel_cases.py proved on the CPU at a few hundred rows, before a GPU is involved: fp32 arithmetic of the same operation
rounded once to the type is inside the bound for every row kind and both types, the bound rejects the wrong results the GPU tests
exist to catch (each applied to that fp32 evaluation), the dispatch mirror agrees with a table written out by hand from the C++
conditions, and the row sampler holds the tiles it names."""
import pytest
import torch

from tests import row_kernel_cases as R

DTS = ["bf16", "fp16"]
M_CPU = {"qkv320": 512, "qkv640": 384, "geglu640": 384, "mlp": 384}
_CASES = {}


def case_of(kernel, dt, kind="normal"):
    """A case, its fp64 reference and its fp32 evaluation, built once (never modified)."""
    key = (kernel, dt, kind)
    if key not in _CASES:
        case = R.row_case(kernel, M_CPU[kernel], dt, kind)
        kw = dict(gate=0.6) if kernel == "mlp" else {}
        _CASES[key] = (case, kw) + tuple(R.row_ref(case, **kw)) + (R.row_ref(case, cd=torch.float32, **kw)[0],)
    return _CASES[key]


def rejects(got32, want, slack, dt):
    return R.outside(got32.to(R.DTYPES[dt]), want, slack, dt)[0]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("kernel", list(R.KERNELS))
def test_fp32_arithmetic_rounded_once_is_inside_the_bound(kernel, kind, dt):
    case, kw, want, slack, got32 = case_of(kernel, dt, kind)
    assert bool(torch.isfinite(want).all()) and bool(torch.isfinite(slack).all()) and bool((slack >= 0).all())
    bad, ratio = R.outside(got32.to(R.DTYPES[dt]), want, slack, dt)
    print(f"[bound] {kernel} {dt} {kind}: fp32 rounded once, err/bound {ratio:.3f}, outside {bad}")
    assert bad == 0, (bad, ratio)
    assert R.rel_rms(got32.to(R.DTYPES[dt]), want) < R.RMS_BAR[dt]
    if kind == "zero_row":                               # the zero rows' outputs are d[n] (q | k | v), x + g (W2 H(d1) + b2) (MLP)
        r = R.zero_rows(case["M"], R.KERNELS[kernel]["BM"])[0]
        assert not bool(case["x"][r].any()) and float(case["stats"][r, 1]) == pytest.approx(1e-5 ** -0.5)
        if kernel.startswith("qkv"):
            assert torch.allclose(want[r], case["d"].double(), atol=1e-12) and float(slack[r].max()) == 0.0
            assert float(case["d"].abs().min()) >= R.D_FLOOR == 2.0 ** -14         # U |d| is a bound for normal numbers only
        # wherever a zero row's output is an fp16 subnormal, the bound holds the half step a correct rounding may cost
        for r in R.zero_rows(case["M"], R.KERNELS[kernel]["BM"]):
            bound = R.U[dt] * want[r].abs() + slack[r]
            assert bool(((want[r].abs() >= 2.0 ** -14) | (bound >= R.HALF_SUBNORMAL_STEP[dt])).all()), (kernel, r)
    if kind == "tiny_mean" and dt == "fp16":             # the lo half of the hi + lo split of mu is subnormal in fp16
        mu = case["stats"][:, 0]
        lo = (mu - mu.half().float()).abs()
        assert float(mu.abs().max()) < 2e-4 and float(lo.max()) < 2.0 ** -14
    if kind.startswith("large_mean"):
        r = float(kind[len("large_mean"):])
        got = (case["stats"][:, 0].abs() * case["stats"][:, 1])
        assert float((got / r - 1).abs().max()) < 0.2


def test_the_handed_in_statistics_are_not_the_rows_own():
    case = case_of("qkv320", "bf16")[0]
    x = case["x"].double()
    mu = x.mean(-1)
    rstd = 1 / (x.var(-1, unbiased=False) + 1e-5).sqrt()
    assert float((case["stats"][:, 0].double() - mu).abs().median()) > 0.1
    assert float((case["stats"][:, 1].double() / rstd - 1).abs().median()) > 0.1
    assert len({tuple(r) for r in case["x"][:, :8].float().tolist()}) == case["M"]          # all rows distinct


# ---- the bound rejects what the GPU tests exist to catch -------------------------------------------------------------------------
def _eval32(case, kw=None, **changes):
    return R.row_ref(dict(case, **changes), cd=torch.float32, **(kw or {}))[0]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kernel", list(R.KERNELS))
def test_statistics_of_the_row_128_below_are_outside(kernel, dt):
    case, kw, want, slack, got32 = case_of(kernel, dt)
    got = _eval32(case, kw, stats=case["stats"].roll(-128, 0))
    assert rejects(got, want, slack, dt) > 0.5 * want.numel()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kernel", list(R.KERNELS))
def test_a_dropped_mean_term_of_one_row_group_is_outside(kernel, dt):
    case, kw, want, slack, got32 = case_of(kernel, dt)
    st = case["stats"].clone()
    rstd_mu = st[32:64, 1] * st[32:64, 0]
    st[32:64, 0] = 0
    got = _eval32(case, kw, stats=st)
    assert torch.equal(got[:32], got32[:32]) and torch.equal(got[64:], got32[64:])
    assert rejects(got, want, slack, dt) > 0
    assert float(rstd_mu.abs().max()) > 0.1


@pytest.mark.parametrize("kernel", ["qkv320", "qkv640"])
def test_a_hi_only_c_is_outside_at_large_mean_100_in_bf16(kernel):
    """The lo half of the 16-bit split of c dropped: invisible at |mean| / std < 1, 0.2 |c| at a ratio of 100."""
    case, kw, want, slack, got32 = case_of(kernel, "bf16", "large_mean100")
    got = _eval32(case, c=case["c"].bfloat16().float())
    bad = rejects(got, want, slack, "bf16")
    print(f"[bound] {kernel} hi-only c at large_mean 100 bf16: {bad} of {want.numel()} outside")
    assert bad > 0.25 * want.numel()
    # ... while the split the kernel documents (both halves, each factor good to 2^-17) is inside the term the bound carries for it
    c, mu = case["c"].double(), case["stats"][:, 0].double()
    split = lambda t: t.float().bfloat16().double() + (t.float() - t.float().bfloat16().float()).bfloat16().double()
    err = (case["stats"][:, 1].double()[:, None] * (mu[:, None] * c[None] - split(mu)[:, None] * split(c)[None])).abs()
    allow = R.SPLIT16 * (case["stats"][:, 1].double() * mu.abs())[:, None] * c.abs()[None]
    assert bool((err <= allow).all())


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kernel", ["qkv320", "qkv640"])
def test_an_untransposed_block_of_v_is_outside(kernel, dt):
    case, kw, want, slack, got32 = case_of(kernel, dt)
    cols = R.KERNELS[kernel]["cols"]
    vt_want, vt_slack = want[:, cols:].t(), slack[:, cols:].t()
    vt = got32[:, cols:].t().clone()
    assert rejects(vt, vt_want, vt_slack, dt) == 0
    vt[32:64, 64:96] = vt[32:64, 64:96].t().clone()
    bad = rejects(vt, vt_want, vt_slack, dt)
    assert 0.9 * 32 * 31 < bad <= 32 * 32


@pytest.mark.parametrize("dt", DTS)
def test_a_16_group_of_w2_without_its_permutation_is_outside(dt):
    from instancediffusion_amd.ops import HipOps
    case, kw, want, slack, got32 = case_of("mlp", dt)
    perm = torch.tensor(HipOps.MLP_W2_PERM)
    assert sorted(perm.tolist()) == list(range(16)) and torch.equal(perm[perm], torch.arange(16))     # an involution
    # the packing is the caller's: mlp_pack's image of W2 un-permutes to W2
    cd, w2p = HipOps.mlp_pack(case["wp"], case["cp"], case["dp"], case["w2"])
    assert torch.equal(w2p.view(320, 80, 16)[:, :, perm].reshape(320, 1280), case["w2"])
    assert torch.equal(cd.view(40, 2, 64)[:, 0].reshape(-1), case["cp"]) and torch.equal(cd.view(40, 2, 64)[:, 1].reshape(-1), case["dp"])
    w2 = case["w2"].clone()
    w2[:, 16 * 37:16 * 38] = w2[:, 16 * 37:16 * 38][:, perm]
    got = _eval32(case, kw, w2=w2)
    assert rejects(got, want, slack, dt) > 0


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kernel", ["geglu640", "mlp"])
def test_swapped_halves_of_one_period_32_group_are_outside(kernel, dt):
    """Packed rows 32 j .. + 31 are [16 value | 16 gate]: swapped, the unpacked value rows 16 j .. + 15 and their gate rows trade places."""
    case, kw, want, slack, got32 = case_of(kernel, dt)
    n = R.KERNELS[kernel]["N"] // 2
    j = 21
    w, c, d = case["w"].clone(), case["c"].clone(), case["d"].clone()
    v, g = slice(16 * j, 16 * j + 16), slice(n + 16 * j, n + 16 * j + 16)
    for t in (w, c, d):
        t[v], t[g] = t[g].clone(), t[v].clone()
    got = _eval32(case, kw, w=w, c=c, d=d)
    bad = rejects(got, want, slack, dt)
    assert bad > 0
    if kernel == "geglu640":                             # exactly those 16 columns
        assert torch.equal(torch.cat([got[:, :16 * j], got[:, 16 * j + 16:]], 1), torch.cat([got32[:, :16 * j], got32[:, 16 * j + 16:]], 1))
        assert bad > 0.9 * 16 * want.shape[0]
    # and the packing itself: the kernel's image un-packs to the reference's halves
    wp = case["wp"].view(-1, 2, 16, case["w"].shape[-1])
    assert torch.equal(wp[:, 0].reshape(n, -1), case["w"][:n]) and torch.equal(wp[:, 1].reshape(n, -1), case["w"][n:])


@pytest.mark.parametrize("dt", DTS)
def test_h_kept_in_fp32_moves_some_elements(dt):
    """Not required to be rejected (an intermediate that is MORE precise than stated): only counted."""
    case, kw, want, slack, got32 = case_of("mlp", dt)
    got = R.row_ref(case, cd=torch.float32, round_h=False, **kw)[0]
    moved = int((got.to(R.DTYPES[dt]) != got32.to(R.DTYPES[dt])).sum())
    print(f"[bound] mlp {dt}: H kept in fp32 moves {moved} of {want.numel()} outputs, {rejects(got, want, slack, dt)} of them outside the bound")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kernel", list(R.KERNELS))
def test_a_tile_stored_one_tile_later_is_outside(kernel, dt):
    case, kw, want, slack, got32 = case_of(kernel, dt)
    BM = R.KERNELS[kernel]["BM"]
    got = got32.clone()
    got[BM:] = got32[:-BM]
    assert rejects(got, want, slack, dt) > 0.5 * (want.numel() - BM * want.shape[1])


@pytest.mark.parametrize("dt", DTS)
def test_round_flip_marks_the_midpoints(dt):
    T = R.DTYPES[dt]
    u = R.U[dt]                                          # the spacing of the type in [1, 2)
    h = torch.tensor([1.0 + u / 2 + 1e-6, 1.0 + u / 2 - 1e-6, 1.0 + u / 4, 1.0 - u / 4 + 1e-6, 0.5 + u / 8, 2.0 - u / 2 - 1e-6], dtype=torch.float64)
    s = torch.full_like(h, 1e-5)
    f = R.round_flip(h, s, dt)
    assert f[0] == u and f[1] == u and f[2] == 0 and f[3] == u and f[4] == 0 and f[5] == u
    tiny = float(torch.tensor([1], dtype=torch.int16).view(T))
    assert R.round_flip(torch.tensor([tiny / 2], dtype=torch.float64), torch.tensor([1e-30], dtype=torch.float64), dt)[0] == tiny


# ---- the dispatch mirror ---------------------------------------------------------------------------------------------------------
# (kernel, M, options) -> takes, written out from csrc/mw_row.h, the idf_launch_* guards and idf_mlp_geglu; at 256 CUs and at 64
DISPATCH_256 = [
    ("qkv320", 131072, {}, True), ("qkv320", 131072 - 256, {}, False), ("qkv320", 131072 + 32, {}, False),
    ("qkv320", 131072 + 7 * 256, {}, True), ("qkv320", 131072, dict(stats=False), False), ("qkv320", 131072, dict(act="silu"), False),
    ("qkv320", 131072, dict(res=True), False), ("qkv320", 131072, dict(ldo=644), False), ("qkv320", 131072, dict(ldo=648), True),
    ("qkv320", 131072, dict(ldo=632), False), ("qkv320", 131072, dict(lda=328, ldw=328, ldo=648, ld_vt=131080), True),
    ("qkv320", 131072, dict(ld_vt=131076), False), ("qkv320", 131072, dict(ld_vt=131064), False), ("qkv320", 131072, dict(lda=324), False),
    ("qkv320", 131072, dict(vt_col0=320), False), ("qkv320", 131072, dict(vt=False), False), ("qkv320", 131072, dict(knob=0), False),
    ("qkv320", 131072, dict(big_mode=0), False), ("qkv320", 131072, dict(K=640), False), ("qkv320", 131072, dict(N=1920), False),
    ("qkv320", 131072, dict(ld_vt=2 ** 25), False), ("qkv320", 131072, dict(ldw=1118488), False), ("qkv320", 131072, dict(ldw=1118480), True),
    ("qkv640", 65536, {}, True), ("qkv640", 65536 - 128, {}, False), ("qkv640", 65536 + 32, {}, False), ("qkv640", 65536 + 3 * 128, {}, True),
    ("qkv640", 65536, dict(stats=False), False), ("qkv640", 65536, dict(ldo=1284), False), ("qkv640", 65536, dict(ldo=1288), True),
    ("qkv640", 65536, dict(lda=648, ldw=648, ldo=1288, ld_vt=65544), True), ("qkv640", 65536, dict(vt_col0=640), False),
    ("geglu640", 65536, {}, True), ("geglu640", 65536 - 128, {}, False), ("geglu640", 65536 + 32, {}, False),
    ("geglu640", 65536 + 7 * 128, {}, True), ("geglu640", 65536, dict(stats=False), False),
    ("geglu640", 65536, dict(geglu=False, act="silu"), False), ("geglu640", 65536, dict(act="silu"), False),
    ("geglu640", 65536, dict(period=64), False), ("geglu640", 65536, dict(ldo=2564), False), ("geglu640", 65536, dict(ldo=2568), True),
    ("geglu640", 65536, dict(lda=648, ldw=648, ldo=2568), True), ("geglu640", 65536, dict(out_stats=True), False),
    ("geglu640", 65536, dict(knob=0), False), ("geglu640", 65536, dict(batch=2), False), ("geglu640", 65536, dict(vt=True), False),
    ("mlp", 128, {}, True), ("mlp", 192, {}, False), ("mlp", 128 * 13, {}, True), ("mlp", 128 * 520, {}, True), ("mlp", 128, dict(C=640), False),
    ("mlp", 128, dict(lda=328, ldo=328, ldw=328, ldw2=1288), True), ("mlp", 128, dict(ldo=324), False), ("mlp", 128, dict(ldw2=1272), False),
]
DISPATCH_64 = [
    ("qkv320", 32768, {}, True), ("qkv320", 32768 - 256, {}, False), ("qkv640", 16384, {}, True), ("qkv640", 16384 - 128, {}, False),
    ("geglu640", 16384, {}, True), ("geglu640", 16384 - 128, {}, False), ("geglu640", 16384 + 32, {}, False), ("mlp", 192, {}, False),
]


@pytest.mark.parametrize("cus,table", [(256, DISPATCH_256), (64, DISPATCH_64)])
def test_the_dispatch_mirror_agrees_with_the_table(cus, table):
    for kernel, M, opts, takes in table:
        assert R.row_takes(kernel, M, cus, **opts) == takes, (kernel, M, opts)
    for kernel in ("qkv320", "qkv640", "geglu640"):
        BM = R.KERNELS[kernel]["BM"]
        assert R.m0(kernel, cus) == 2 * BM * cus
        assert R.row_takes(kernel, R.m0(kernel, cus), cus) and not R.row_takes(kernel, R.m0(kernel, cus) - BM, cus)
    assert R.m0("mlp", cus) == 128


# ---- the row sampler -------------------------------------------------------------------------------------------------------------
def gpu_shapes(cus):
    """(M, BM, G) of every launch of tests/test_row_kernels_gpu.py that is checked on a sample."""
    for kernel in ("qkv320", "qkv640", "geglu640"):
        BM = R.KERNELS[kernel]["BM"]
        for extra in (0, 3 * BM, 7 * BM, -BM, 32):
            M = R.m0(kernel, cus) + extra
            yield M, BM, min(M // BM, cus)
    for tiles in (cus + 1, 2 * cus + 8):
        yield 128 * tiles, 128, cus


@pytest.mark.parametrize("cus", [256, 64, 304])
def test_the_row_sampler_holds_the_tiles_it_names(cus):
    for M, BM, G in gpu_shapes(cus):
        rows = R.sample_rows(M, BM, G)
        assert rows.dtype == torch.int64 and bool((rows[1:] > rows[:-1]).all()) and 0 <= int(rows[0]) and int(rows[-1]) == M - 1
        assert 1800 <= rows.numel() < 4096, (M, BM, G, rows.numel())
        have = set(rows.tolist())
        tiles = M // BM
        for t in (0, 1, G - 1, G, min(G + 1, tiles - 1), tiles - 2, tiles - 1):
            assert all(r in have for r in range(t * BM, (t + 1) * BM)), (M, BM, G, t)
        named = {0, 1, G - 1, G, G + 1, tiles - 2, tiles - 1}
        mid = [t for t in range(tiles) if t not in named and all(r in have for r in range(t * BM, (t + 1) * BM))]
        assert mid, "one whole tile in the middle"
        assert all(r in have for r in range(tiles * BM, M))                                  # rows behind the last whole tile
        singles = [r for r in have if not all(q in have for q in range(r // BM * BM, min(M, r // BM * BM + BM)))]
        assert len(singles) >= 200 and len({r // BM for r in singles}) > min(100, tiles // 2)                 # the scatter reaches many other tiles
    assert torch.equal(R.sample_rows(65536, 128, 256), R.sample_rows(65536, 128, 256))       # seeded
    assert R.sample_rows(128, 128, 1).tolist() == list(range(128))


@pytest.mark.parametrize("dt", DTS)
def test_the_pair_fraction_bar(dt):
    """spacing() is the step of the type; the bar is 0 without a mean term and grows with |mean| / std."""
    T = R.DTYPES[dt]
    v = torch.tensor([1.0, 1.5, 1.75, 0.75, 3.0, 2.0 ** -20], dtype=torch.float64)
    nxt = lambda t: (t.to(T).view(torch.int16) + 1).view(T).double() - t.to(T).double()
    assert torch.equal(R.spacing(v, dt), nxt(v))
    bars = {}
    for kernel in ("qkv320", "qkv640", "geglu640"):
        for kind in ("normal", "large_mean10", "large_mean100"):
            case, kw, want, slack, got32 = case_of(kernel, dt, kind)
            bars[kind] = R.pair_fraction_bar(case, None, want)
        print(f"[bound] {kernel} {dt}: pair fraction bar {bars}")
        assert 0.0 < bars["normal"] < bars["large_mean10"] < bars["large_mean100"] <= 1.0
        zero = dict(case_of(kernel, dt)[0])
        zero["stats"] = zero["stats"].clone()
        zero["stats"][:, 0] = 0
        assert R.pair_fraction_bar(zero, None, want) == 0.0
