"""The attention kernels on a real MI355X, in bf16 AND fp16, family by family and mode by mode -- the 32-queries-per-wave kernel of
csrc/attention.hip (every head dim it is instantiated for, plain, MASK and resident keys), attention4.hip (modes 1, 2, 3),
attention4w.hip (modes 4, 5), attention8.hip (modes 1..6), the two fused-qkv kernels of csrc/clip.hip and idf_softmax_rows -- at the
smallest shapes that walk each one across its own edges: queries per workgroup, the 64-key tile and its 8-key chunks, one-key tails,
an empty second segment, block totals that switch the XCD remap on and off.

Every result is compared with the fp64 reference of tests/attention_cases.py on the same 16-bit inputs (proved on the CPU by
tests/test_attention_refs.py): all outputs finite, NO element outside the per-element bound derived there (so a wrong SMALL element
shows, which an error relative to the largest output hides), and a rel-RMS error of at most 2 x that of the fp32 replay of the kernels'
arithmetic on the same inputs.  The exact-data cases (the key census) are judged by (u + 2^-21) |want| alone: every P is exactly 1 there
and the replay's own error can be 0.  V^T pad columns, the K / Q rows behind n / nq and the output's guard columns and rows are NaN;
the guards must still be NaN afterwards.  Each family is forced with idf_set_tuning (restored by a fixture) and the launch counters must
show that it took the launch -- or, where the code says it declines the shape, that it did not.  The references run in fp64 on the
device: they are plain torch and the largest case has 262 000 queries.
"""
import pytest
import torch

from tests import attention_cases as A

pytestmark = pytest.mark.gpu

DTS = ["bf16", "fp16"]
_OPS, _REFS = {}, {}
CACHE_MAX = 1 << 22                                          # references above this many elements are not kept


def ops_for(dt):
    if dt not in _OPS:
        from instancediffusion_amd.ops import HipOps
        _OPS[dt] = HipOps(A.DTYPES[dt])
    return _OPS[dt]


@pytest.fixture(autouse=True)
def knobs():
    """Restores IDF_TUNE_ATTN2 / IDF_TUNE_ATTN8 behind every test, whatever it forced."""
    from instancediffusion_amd import _lib
    lib = _lib.load()
    prev2 = lib.idf_set_tuning(_lib.IDF_TUNE_ATTN2, 0)
    prev8 = lib.idf_set_tuning(_lib.IDF_TUNE_ATTN8, 0)
    lib.idf_set_tuning(_lib.IDF_TUNE_ATTN2, prev2)
    lib.idf_set_tuning(_lib.IDF_TUNE_ATTN8, prev8)
    yield
    lib.idf_set_tuning(_lib.IDF_TUNE_ATTN2, prev2)
    lib.idf_set_tuning(_lib.IDF_TUNE_ATTN8, prev8)


def counters(lib):
    from instancediffusion_amd import _lib
    return tuple(lib.idf_get_stat(s) for s in (_lib.IDF_STAT_ATTN2_LAUNCHES, _lib.IDF_STAT_ATTN8_LAUNCHES, _lib.IDF_STAT_ATTN_RES_LAUNCHES))


def case_and_ref(dims, dt):
    """The case (CPU), its fp64 reference and bound (device) and the rel-RMS error of the fp32 replay (None for the exact-data cases and
    for cases too large to replay on the CPU in a test's time: those are judged by the bound alone and say so in their [parity] line)."""
    key = (dims, dt)
    if key in _REFS:
        return _REFS[key]
    c = A.attn_case(*dims[:6], dt, kind=dims[6], mask=dims[7])
    want, bound = A.attention_ref(c, device="cuda")
    if dims[6] == "census":
        bound = torch.minimum(bound, A.census_bound(want, dt))
        rms = None
    else:
        rms = A.rel_rms(A.attention_replay(c), want)
    val = (c, want, bound, rms)
    if want.numel() <= CACHE_MAX:
        _REFS[key] = val
    return val


def launch(ops, c, a2, a8, col_pad=8, batch_gap=0):
    """Run the case under the forced knobs: -> (out view, guard check, counter deltas (attn2, attn8, resident keys))."""
    from instancediffusion_amd import _lib
    B, H, d, nq, n0, n1 = (c[k] for k in ("B", "H", "d", "nq", "n0", "n1"))
    C = H * d
    qk = c["qk"].cuda()
    kw = {}
    if n1:
        kw.update(k1=c["k1b"].cuda()[:, :n1], vt1=c["vt1"].cuda(), n1=n1)
    if c.get("qbits") is not None:
        kw.update(qbits=c["qbits"].cuda(), kbits0=c["kbits0"].cuda(), kbits1=c["kbits1"].cuda() if n1 else None)
    out, guard = A.guarded_out((B, nq, C), ops.dtype, "cuda", col_pad, batch_gap)
    ops.lib.idf_set_tuning(_lib.IDF_TUNE_ATTN2, a2)
    ops.lib.idf_set_tuning(_lib.IDF_TUNE_ATTN8, a8)
    start = counters(ops.lib)
    ops.attention(qk[:, :nq, :C], qk[:, :n0, C:], c["vt0"].cuda(), n0, out, H, **kw)
    torch.cuda.synchronize()
    return out, guard, tuple(a - b for a, b in zip(counters(ops.lib), start))


def expect_counters(disp):
    return {"attn2": (1, 0, 0), "attn8": (0, 1, 0), "res": (0, 0, 1), None: (0, 0, 0)}[disp["counter"]]


def judge(what, out, want, bound, rms_replay, guard):
    bad, ratio = A.outside(out, want, bound)
    rms = A.rel_rms(out, want)
    vs = "exact data" if rms_replay is None else f"{rms / max(rms_replay, 1e-300):.2f} x replay {rms_replay:.2e}"
    print(f"[parity] {what}: err/bound {ratio:.3f} outside {bad} rel-rms {rms:.2e} ({vs})")
    assert guard() == "", f"stored outside the output view: {guard()}"
    assert bool(torch.isfinite(out).all()), "non-finite output"
    assert bad == 0, f"{bad} of {want.numel()} elements outside the bound (worst error / bound {ratio:.3f})"
    if rms_replay is not None:
        assert rms <= A.RMS_FACTOR * rms_replay, f"rel-rms {rms:.3e} above {A.RMS_FACTOR} x the fp32 replay's {rms_replay:.3e}"
    return ratio, rms


def attention_test(fam, dims, dt, a2, a8, kernel, **launch_kw):
    ops = ops_for(dt)
    c, want, bound, rms_replay = case_and_ref(dims, dt)
    B, H, d, nq, n0, n1 = dims[:6]
    C = H * d
    ldo = C + launch_kw.get("col_pad", 8)
    so = (nq + 1) * ldo + launch_kw.get("batch_gap", 0)
    disp = A.dispatch(d, nq, n0, n1, B, H, attn2=a2, attn8=a8, mask=dims[7], ldo=ldo, so=so)
    assert disp["kernel"] == kernel, f"the case list pairs this shape with {kernel}; the dispatch rules say {disp['kernel']}"
    out, guard, moved = launch(ops, c, a2, a8, **launch_kw)
    assert moved == expect_counters(disp), f"{kernel} expected; (attn2, attn8, resident-key) launches {moved}"
    judge(f"idf_attention {fam} {dt} {kernel} qb {disp['qb']} blocks {A.blocks(dims[:6], disp['qb'])} {dims[6]} {dims[:6]}", out, want,
          bound, rms_replay, guard)
    return out


def ids(v):
    return str(v).replace(" ", "")


FAMILY_PARAMS = [(fam, dims) for fam in A.FAMILIES for dims in A.family_cases(fam)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("fam,dims", FAMILY_PARAMS, ids=ids)
def test_attention_family(fam, dims, dt):
    """Every kernel family and mode over its star of nq / n0 / n1 / (B, H), the key census, the negative-score case and (the LDS-DMA
    kernels) the spike cases of the v4 / v8 tests, judged by the bound."""
    a2, a8, kernel, _ = A.FAMILIES[fam]
    attention_test(fam, dims, dt, a2, a8, kernel)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("dims", A.mask_cases(), ids=ids)
def test_attention_masked(dims, dt):
    """The MASK instantiations at every supported head dim, with the knobs at their defaults' values (a mask goes to the 32-query
    kernel whatever they say); queries with word 0, unconditional keys, a key nobody sees."""
    attention_test("mask", dims, dt, 5, 1, "attn32_mask")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("dims", A.RES_CASES + [A.RES_PLAIN], ids=ids)
def test_attention_resident_keys(dims, dt):
    """The resident-key instantiations: the new launch counter shows that they ran; two query blocks per workgroup, the last workgroup
    of every head walks one ragged block; with and without the XCD remap."""
    attention_test("res", dims, dt, 0, 0, "attn32_res")


@pytest.mark.parametrize("dt", DTS)
def test_attention_just_below_the_resident_key_threshold(dt):
    attention_test("res-below", A.RES_BELOW, dt, 0, 0, "attn32")


DECLINES = [                                                 # (family, dims, launch options): what the forced family must leave alone
    ("a4-m1", (1, 3, 40, 257, 77, 8, "normal", False), {}),              # n0 % 8 != 0
    ("a4w-m5", (1, 3, 40, 257, 72, 5, "normal", False), {}),             # n1 % 8 != 0
    ("a8-m1", (1, 3, 80, 129, 77, 8, "normal", False), {}),
    ("a8-m1", (1, 3, 160, 129, 72, 5, "normal", False), {}),
    ("a4-m1", (2, 3, 40, 257, 72, 8, "normal", False), dict(col_pad=4)),   # ldo % 8 == 4: the 32-query kernel's 8-byte stores
    ("a4w-m4", (2, 3, 40, 257, 72, 8, "normal", False), dict(col_pad=4)),
    ("a4w-m5", (2, 3, 40, 257, 72, 8, "normal", False), dict(col_pad=4)),
    ("a8-m1", (2, 3, 80, 129, 72, 8, "normal", False), dict(col_pad=4)),
    ("a8-m2", (2, 3, 160, 257, 72, 8, "normal", False), dict(col_pad=4)),
    ("a4-m2", (2, 3, 40, 257, 72, 8, "normal", False), dict(batch_gap=4)),  # an unaligned batch stride under aligned rows
    ("a4w-m5", (2, 3, 40, 257, 72, 8, "normal", False), dict(batch_gap=4)),
    ("a8-m1", (2, 3, 80, 129, 72, 8, "normal", False), dict(batch_gap=4)),
    ("a4-m1", (1, 2, 40, 33, 72, 8, "census", False), dict(col_pad=4)),
]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("fam,dims,opts", DECLINES, ids=ids)
def test_families_decline_what_the_code_says(fam, dims, opts, dt):
    a2, a8, _, _ = A.FAMILIES[fam]
    attention_test(fam + "-declined", dims, dt, a2, a8, "attn32", **opts)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind", ["normal", "flat", "census"])
def test_attn2_modes_1_4_5_are_bit_identical(kind, dt):
    """include/idf.h: the results of modes 1, 4 and 5 are bit-identical unless a re-base / rerun path is taken.  None is on the census
    (every score 0) or on "flat" random data (no score a log2 unit above another).  On plain random data bf16 takes none either (its
    reference value sits 7 log2 units above the first tile's maximum); fp16, whose reference value IS that maximum, re-bases in
    mode 1 whenever a later score is a log2 unit higher -- there modes 4 and 5 (no per-tile re-base) are bit-identical to each other
    and mode 1 is held to the bound like them."""
    dims = (2, 3, 40, 513, 264, 184, kind, False)
    outs = [attention_test(f"mode-{m}", dims, dt, m, 0, "attn4" if m == 1 else "attn4w") for m in (1, 4, 5)]
    pairs = [(4, 5)] if (kind == "normal" and dt == "fp16") else [(1, 4), (1, 5)]
    for a, b in pairs:
        oa, ob = outs[(1, 4, 5).index(a)], outs[(1, 4, 5).index(b)]
        differ = int((oa.view(torch.int16) != ob.view(torch.int16)).sum())
        print(f"[parity] idf_attention {dt} {kind}: mode {b} against mode {a}, {differ} of {oa.numel()} elements differ in bits")
        assert differ == 0


@pytest.mark.parametrize("dt", DTS)
def test_d40_through_both_kernels_against_one_reference(dt):
    dims = (2, 3, 40, 257, 136, 184, "normal", False)
    attention_test("a32", dims, dt, 0, 0, "attn32")
    attention_test("a4-m1", dims, dt, 1, 0, "attn4")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("mask", [False, True])
@pytest.mark.parametrize("d", A.UNSUPPORTED_D)
def test_unsupported_head_dims_return_before_any_launch(d, mask, dt):
    """d = 104, 112, 136, 144: IDF_E_UNSUPPORTED, no counter moves, the NaN-filled output stays NaN."""
    from instancediffusion_amd import _lib
    ops = ops_for(dt)
    c = A.attn_case(1, 2, d, 33, 72, 8, dt, mask=mask)
    out, guard = A.guarded_out((1, 33, 2 * d), ops.dtype, "cuda")
    start = counters(ops.lib)
    kw = dict(k1=c["k1b"].cuda()[:, :8], vt1=c["vt1"].cuda(), n1=8)
    if mask:
        kw.update(qbits=c["qbits"].cuda(), kbits0=c["kbits0"].cuda(), kbits1=c["kbits1"].cuda())
    qk = c["qk"].cuda()
    with pytest.raises(_lib.IdfError, match="unsupported"):
        ops.attention(qk[:, :33, :2 * d], qk[:, :72, 2 * d:], c["vt0"].cuda(), 72, out, 2, **kw)
    torch.cuda.synchronize()
    assert counters(ops.lib) == start and bool(torch.isnan(out).all()) and guard() == ""


# ---- idf_attention_causal / idf_attention_qkv -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B,T,H,causal,kind", A.qkv_cases(), ids=ids)
def test_fused_qkv_attention(B, T, H, causal, kind, dt):
    ops = ops_for(dt)
    c = A.qkv_case(B, T, H, dt, causal, kind)
    want, bound = A.qkv_attention_ref(c, device="cuda")
    rms_replay = None
    if kind == "census":
        bound = torch.minimum(bound, A.census_bound(want, dt))
    else:
        rms_replay = A.rel_rms(A.qkv_replay(c), want)
    C = H * 64
    buf = torch.full((B * T + 1, C + 8), float("nan"), dtype=ops.dtype, device="cuda")
    out = buf[:B * T, :C]
    (ops.attention_causal if causal else ops.attention_qkv)(c["buf"].cuda()[:, :3 * C], out, H, T)
    torch.cuda.synchronize()
    guard = lambda: "" if bool(torch.isnan(buf[B * T:]).all() and torch.isnan(buf[:, C:]).all()) else "a guard element was overwritten"
    judge(f"idf_attention_{'causal' if causal else 'qkv'} {dt} {kind} B{B} T{T} H{H}", out, want, bound, rms_replay, guard)


# ---- idf_softmax_rows --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("rows", A.SOFTMAX_ROWS)
@pytest.mark.parametrize("n", A.SOFTMAX_N)
def test_softmax_rows(n, rows, dt):
    """lds and ldp larger than n (NaN between the rows), a dominant entry in row 0."""
    from instancediffusion_amd import _lib
    ops = ops_for(dt)
    c = A.softmax_case(rows, n, dt)
    want, bound = A.softmax_rows_ref(c["s"], c["scale"], dt)
    rms_replay = A.rel_rms(A.softmax_rows_replay(c["s"], c["scale"], dt), want)
    s = c["buf"].cuda()
    ldp = n + 8
    buf = torch.full((rows + 1, ldp), float("nan"), dtype=ops.dtype, device="cuda")
    _lib.check(ops.lib.idf_softmax_rows(s.data_ptr(), buf.data_ptr(), rows, n, s.stride(0), ldp, c["scale"], ops.dt, ops._stream()),
               "idf_softmax_rows")
    torch.cuda.synchronize()
    guard = lambda: "" if bool(torch.isnan(buf[rows:]).all() and torch.isnan(buf[:, n:]).all()) else "a guard element was overwritten"
    judge(f"idf_softmax_rows {dt} rows {rows} n {n}", buf[:rows, :n], want, bound, rms_replay, guard)
