"""The row-resident fused kernels on a real MI355X, in bf16 AND fp16: qkv320w_kernel, qkv640w_kernel and geglu640w_kernel behind
idf_gemm, mlp320_kernel and mlp320w_kernel behind idf_mlp_geglu -- per element, on distinct rows, at the edges of their dispatch.

Every row of every case is distinct and the (mu, rstd) handed in are not the rows' own (tests/row_kernel_cases.py, proved on the CPU by
tests/test_row_kernel_refs.py).  About 2048 sampled rows -- whole tiles where a persistent workgroup starts, wraps round and ends, and a
scatter -- are compared with an fp64 reference of the same operation: NO element outside the per-element bound.  The whole output is
compared with the persistent kernel's on the same operands (tests/test_gemm_conv_edges_gpu.py proves that one per element), which
means something now that no two rows are alike.  Every output lives in a NaN-filled buffer whose guard rows and columns must still be
NaN afterwards; the launch counters must show that the row kernel took the launch, or, where the code says it declines, that it did
not.  The smallest M that reaches a kernel is two tiles per CU, so the shapes are derived from the CU count.
"""
import contextlib
import ctypes

import pytest
import torch

from tests import row_kernel_cases as R
from tests.gemm_conv_run import exact, padded

pytestmark = pytest.mark.gpu

DTS = ["bf16", "fp16"]
GEMM_KERNELS = ["qkv320", "qkv640", "geglu640"]
_OPS, _CACHE = {}, {}


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def ops_for(dt):
    if dt not in _OPS:
        from instancediffusion_amd.ops import HipOps
        _OPS[dt] = HipOps(R.DTYPES[dt])
    return _OPS[dt]


def ids():
    from instancediffusion_amd import _lib
    return {"qkv320": (_lib.IDF_TUNE_QKV_ROW, _lib.IDF_STAT_QKV_ROW_LAUNCHES), "qkv640": (_lib.IDF_TUNE_QKV_ROW, _lib.IDF_STAT_QKV_ROW_LAUNCHES),
            "geglu640": (_lib.IDF_TUNE_GEGLU_ROW, _lib.IDF_STAT_GEGLU_ROW_LAUNCHES), "mlp": (_lib.IDF_TUNE_MLP, None)}


@contextlib.contextmanager
def knob(lib, which, value):
    prev = lib.idf_set_tuning(which, value)
    try:
        yield
    finally:
        lib.idf_set_tuning(which, prev)


def grid(kernel, M):
    return min(M // R.KERNELS[kernel]["BM"], cus())


def built(kernel, M, dt, kind="normal", **ref_kw):
    """(case on the GPU, sampled rows, want, slack).  The M0 cases of the default kind serve several tests: built once, never modified."""
    def build():
        case = R.row_case(kernel, M, dt, kind, device="cuda")
        rows = R.sample_rows(M, R.KERNELS[kernel]["BM"], grid(kernel, M))
        return (case, rows) + tuple(R.row_ref(case, rows, **ref_kw))
    if kind != "normal" or M != R.m0(kernel, cus()) or ref_kw:
        return build()
    key = (kernel, M, dt)
    if key not in _CACHE:
        _CACHE[key] = build()
    return _CACHE[key]


# ---- idf_gemm: qkv320w_kernel, qkv640w_kernel, geglu640w_kernel ----------------------------------------------------------------------
def launch(ops, case, *, row=1, pads=(), ldo_pad=None, stats="given", act=None, x=None, st=None):
    """One idf_gemm call of the case with the row knob at ``row``: -> (out, vt or None, guard checks, launches the row kernel's counter
    shows, launches IDF_STAT_GEMM_BIG_LAUNCHES shows: the persistent kernel's, and the row kernels' too)."""
    kernel, M = case["kernel"], case["M"]
    k = R.KERNELS[kernel]
    geglu = kernel == "geglu640"
    pad = lambda name: 8 if name in pads or "all" in pads else 0
    xd = padded(case["x"] if x is None else x, pad("lda"))
    w = padded(case["wp" if geglu else "w"], pad("ldw"))
    c, d = (case["cp" if geglu else "c"]).cuda(), (case["dp" if geglu else "d"]).cuda()
    cols = k["N"] if act else k["cols"]
    out, g_out = R.guarded((M, cols), ops.dtype, "cuda", ld=cols + (pad("ldo") if ldo_pad is None else ldo_pad))
    guards, vt = [g_out], None
    kw = dict(bias=d)
    if stats == "given":
        kw["ln_row"] = (case["stats"] if st is None else st, c)
    else:
        kw["ln_row"], kw["ln_stats_out"] = (None, c), ops.empty((M, 2), torch.float32)
    if act:
        kw["act"] = act
    elif geglu:
        kw.update(geglu=True, geglu_period=32)
    else:
        vt, g_vt = R.guarded((k["N"] - cols, M), ops.dtype, "cuda", ld=M + pad("ld_vt"))
        guards.append(g_vt)
        kw["vt_out"] = vt
    from instancediffusion_amd import _lib
    which, stat = ids()[kernel]
    with knob(ops.lib, which, row):
        n0, b0 = ops.lib.idf_get_stat(stat), ops.lib.idf_get_stat(_lib.IDF_STAT_GEMM_BIG_LAUNCHES)
        ops.gemm(xd, w, out, **kw)
        torch.cuda.synchronize()
        served, big = ops.lib.idf_get_stat(stat) - n0, ops.lib.idf_get_stat(_lib.IDF_STAT_GEMM_BIG_LAUNCHES) - b0
    return out, vt, guards, served, big


def mirror_opts(kernel, M, pads=(), ldo_pad=None, stats="given", act=None):
    """The launch options of ``launch`` as R.row_takes names them."""
    k = R.KERNELS[kernel]
    pad = lambda name: 8 if name in pads or "all" in pads else 0
    opts = dict(lda=k["K"] + pad("lda"), ldw=k["K"] + pad("ldw"), stats=stats == "given")
    if kernel != "geglu640":
        opts["ld_vt"] = M + pad("ld_vt")
    opts["ldo"] = (k["N"] if act else k["cols"]) + (pad("ldo") if ldo_pad is None else ldo_pad)
    if act:
        opts.update(act=act, geglu=False)
    return opts


def gathered(out, vt, rows):
    r = rows.cuda()
    return out[r] if vt is None else torch.cat([out[r], vt[:, r].t()], 1)


def check_sample(label, dt, out, vt, rows, want, slack, guards):
    """The four assertions of every launch: guards intact, outputs finite, 0 sampled elements outside the bound, rel-rms below the bar."""
    got = gathered(out, vt, rows)
    bad, ratio = R.outside(got, want, slack, dt)
    er = R.rel_rms(got, want)
    print(f"[parity] {label}: {rows.numel()} rows, err/bound {ratio:.3f} rel-rms {er:.2e} outside {bad}")
    for g in guards:
        assert g() == "", f"stored outside the output view: {g()}"
    assert bool(torch.isfinite(out).all()) and (vt is None or bool(torch.isfinite(vt).all())), "non-finite output"
    assert bad == 0, f"{bad} of {want.numel()} sampled elements outside the bound (worst error / bound {ratio:.3f})"
    assert er < R.RMS_BAR[dt]
    return ratio


def whole_vs_persistent(label, kernel, dt, got, ref, scale, frac_bar=None):
    """The whole outputs against the persistent kernel's on the same operands.  Every pair: no element differs by more than one ulp
    of the type at the output's scale (the two kernels' values are far less than a step apart before the rounding, so they differ by
    one step at most; an element, row or tile in the wrong place differs by the output's own size).  Then the bars
    tests/test_kernels_gpu.py states for the pair: q | k | v fewer than 1e-2 of the elements differ, GEGLU rel-rms < 2e-4 and fewer than
    2e-2 differ.  ``frac_bar`` (|mean| / std of 10 and 100): two correct kernels cannot meet those fractions there -- the mean term
    is 10 and 100 times the output, and where in the fp32 chain it is folded decides the rounding of 2 to 12 % of the outputs, as
    R.pair_fraction_bar derives from the fp64 reference; that figure takes the place of the stated fraction, and the rel-rms bar is
    what the two sides' own bars imply, 2 RMS_BAR."""
    num = den = 0.0
    differ = total = 0
    worst = 0.0
    for a, b in zip(got, ref):
        if a is None:
            continue
        dlt = a.float() - b.float()
        num += float(dlt.pow(2).sum(dtype=torch.float64))
        den += float(b.float().pow(2).sum(dtype=torch.float64))
        worst = max(worst, float(dlt.abs().max()))
        differ += int((a != b).sum())
        total += a.numel()
    rms, frac = (num / den) ** 0.5, differ / total
    bar = {"geglu640": 2e-2}.get(kernel, 1e-2) if frac_bar is None else frac_bar
    print(f"[parity] {label} vs persistent kernel: {total} elements, rel-rms {rms:.2e}, max diff / max {worst / scale:.2e}, differing {frac:.2e} "
          f"(bar {bar:.2e})")
    assert worst / scale <= R.U[dt]
    assert frac < bar
    if frac_bar is not None:
        assert rms < 2 * R.RMS_BAR[dt]
    elif kernel == "geglu640":
        assert rms < 2e-4
    return frac


def row_and_persistent(label, kernel, dt, case, rows, want, slack, large_mean=False, **lk):
    """Tests 1-3: the row kernel takes the launch and meets the bound on the sample; with the row knob at 0 the persistent kernel takes
    the same operands (its counter rises, the row kernel's does not), meets ITS bound on the sample -- the same one without the
    hi + lo term -- and agrees with the row kernel on the whole output."""
    ops = ops_for(dt)
    assert R.row_takes(kernel, case["M"], cus(), **mirror_opts(kernel, case["M"], **lk))
    out, vt, guards, served, big = launch(ops, case, row=1, **lk)
    assert (served, big) == (1, 1), "the row kernel must take this launch"
    check_sample(label, dt, out, vt, rows, want, slack, guards)
    out0, vt0, guards0, served0, big0 = launch(ops, case, row=0, **lk)
    assert (served0, big0) == (0, 1), "with the row knob at 0 the persistent kernel must take this launch"
    slack0 = slack if kernel == "geglu640" else slack - R.SPLIT16 * R.mean_term(case["stats"][rows.cuda()].cpu(), case["c"])
    check_sample(label + " persistent kernel", dt, out0, vt0, rows, want, slack0, guards0)
    bar = R.pair_fraction_bar(case, rows, want) if large_mean else None
    whole_vs_persistent(label, kernel, dt, (out, vt), (out0, vt0), float(want.abs().max()), bar)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("extra", [0, 3, 7])
@pytest.mark.parametrize("kernel", GEMM_KERNELS)
def test_sampled_rows_against_fp64_and_the_whole_output_against_the_persistent_kernel(kernel, extra, dt):
    """M0 (two tiles per CU) and M0 + 3, + 7 tiles: tile counts that are uneven across the workgroups."""
    M = R.m0(kernel, cus()) + extra * R.KERNELS[kernel]["BM"]
    case, rows, want, slack = built(kernel, M, dt)
    row_and_persistent(f"{kernel} {dt} M{M}", kernel, dt, case, rows, want, slack)


PADS = [(k, p) for k in GEMM_KERNELS for p in ("lda", "ldw", "ldo", "ld_vt", "all") if not (k == "geglu640" and p == "ld_vt")]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kernel,pad", PADS)
def test_padded_leading_dimensions(kernel, pad, dt):
    """lda = K + 8, ldw = K + 8, ldo = cols + 8, ld_vt = M + 8, each alone and all together: the spare columns are NaN on the inputs and
    guarded on the outputs."""
    M = R.m0(kernel, cus())
    case, rows, want, slack = built(kernel, M, dt)
    row_and_persistent(f"{kernel} {dt} M{M} padded {pad}", kernel, dt, case, rows, want, slack, pads=(pad,))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind", R.KINDS[1:])
@pytest.mark.parametrize("kernel", GEMM_KERNELS)
def test_row_kinds(kernel, kind, dt):
    """|mean| / std of 10 and 100 with the rows' own statistics (the hi + lo mean term of the q | k | v kernels, 2^-16 rstd |mu| |c| in
    the bound, exists for these), |mu| ~ 1e-4 (the lo half subnormal in fp16), and all-zero rows with (0, 1 / sqrt(1e-5))."""
    M = R.m0(kernel, cus())
    case, rows, want, slack = built(kernel, M, dt, kind)
    row_and_persistent(f"{kernel} {dt} M{M} {kind}", kernel, dt, case, rows, want, slack, large_mean=kind.startswith("large_mean"))
    if kernel != "geglu640":                             # the share of the bound that the documented split takes, measured against fp64
        split = R.SPLIT16 * R.mean_term(case["stats"][rows.cuda()].cpu(), case["c"])
        print(f"[parity] {kernel} {dt} {kind}: hi + lo term / bound, largest {float((split / (R.U[dt] * want.abs() + slack)).max()):.3f}")


# ---- a row's result does not depend on where it runs ---------------------------------------------------------------------------------
def copy_sites(kernel, M):
    """Source rows (row group 1 of tile 0) and where their copies go: another wave's row group of the same tile, another row group of
    the workgroup's NEXT tile (tile G), a tile of another workgroup."""
    BM, G = R.KERNELS[kernel]["BM"], grid(kernel, M)
    return 32, [32 + BM // 2, G * BM + 64, 3 * BM]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kernel", GEMM_KERNELS)
def test_a_rows_result_does_not_depend_on_where_it_runs(kernel, dt):
    ops = ops_for(dt)
    M = R.m0(kernel, cus())
    case = built(kernel, M, dt)[0]
    x, st = case["x"].clone(), case["stats"].clone()
    src, dsts = copy_sites(kernel, M)
    for d in dsts:
        x[d:d + 32], st[d:d + 32] = x[src:src + 32], st[src:src + 32]
    out, vt, guards, served, _ = launch(ops, case, x=x, st=st)
    assert served == 1 and all(g() == "" for g in guards)
    assert not torch.equal(out[src:src + 32], out[src + 32:src + 64])
    for d in dsts:
        assert torch.equal(out[d:d + 32], out[src:src + 32]), f"rows {d} .. differ from their originals"
        if vt is not None:
            assert torch.equal(vt[:, d:d + 32], vt[:, src:src + 32]), f"V^T columns {d} .. differ from their originals"


# ---- declines --------------------------------------------------------------------------------------------------------------------
DECLINES = [(k, c) for k in GEMM_KERNELS for c in ("M0-BM", "M0+32", "self_stats", "ldo+4")] + [("geglu640", "silu")]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kernel,what", DECLINES)
def test_row_kernels_decline_what_the_code_says(kernel, what, dt):
    """One tile below two per CU, M % BM != 0, statistics not handed in, an activation on the GEGLU shape, output rows that are not
    16-byte aligned: the mirror says the row kernel declines, its counter does not move, and whoever runs the launch instead is
    inside the same per-element bound."""
    ops = ops_for(dt)
    k = R.KERNELS[kernel]
    M = R.m0(kernel, cus()) + {"M0-BM": -k["BM"], "M0+32": 32}.get(what, 0)
    lk, ref_kw = {}, {}
    if what == "self_stats":
        lk, ref_kw = dict(stats="self"), dict(stats="self")
    elif what == "silu":
        lk, ref_kw = dict(act="silu"), dict(act="silu")
    elif what == "ldo+4":
        lk = dict(ldo_pad=4)
    # who serves it instead: the persistent kernel, but for the output rows that are not 16-byte aligned -- those it declines too,
    # and the small-tile kernels run the launch.  (q | k | v: as the two GEMMs of idf_gemm's fallback, out = A Wqk^T on the small-tile
    # kernels and V^T = Wv A^T, whose rows of ld_vt elements ARE aligned, on the persistent kernel: one launch counted.)
    geglu = kernel == "geglu640" and what != "silu"
    big_takes = R.family_takes("big", M, k["N"], k["K"], geglu=geglu, geglu_period=32, self_ln=what == "self_stats",
                               ldo=(k["cols"] if what != "silu" else k["N"]) + lk.get("ldo_pad", 0))
    assert big_takes == (what != "ldo+4")
    case, rows, want, slack = built(kernel, M, dt, **ref_kw)
    assert not R.row_takes(kernel, M, cus(), **mirror_opts(kernel, M, **lk))
    out, vt, guards, served, big = launch(ops, case, row=1, **lk)
    assert served == 0, "the row kernel must decline this launch"
    if what == "ldo+4" and vt is not None:
        big_takes = R.family_takes("big", k["N"] - k["cols"], M, k["K"], ldo=M)
    assert big == int(big_takes), "the persistent kernel takes what the row kernel declines, except unaligned output rows"
    check_sample(f"{kernel} {dt} M{M} declined {what}", dt, out, vt, rows, want, slack, guards)


@pytest.mark.parametrize("dt", DTS)
def test_mlp_refuses_other_shapes_before_any_launch(dt):
    """M = 192 and C != 320: IDF_E_UNSUPPORTED, nothing written."""
    from instancediffusion_amd import _lib
    ops = ops_for(dt)
    for M, C in ((192, 320), (128, 640)):
        assert not R.row_takes("mlp", M, cus(), C=C)
        x = torch.ones((M, C), dtype=ops.dtype, device="cuda")
        out, guard = R.guarded((M, C), ops.dtype, "cuda")
        st, cd = ops.zeros((M, 2), torch.float32), ops.zeros((16 * C,), torch.float32)
        w1, w2, b2 = ops.zeros((8 * C, C)), ops.zeros((C, 4 * C)), ops.zeros((C,), torch.float32)
        args = _lib.MlpArgs(x=x.data_ptr(), ldx=C, ln_stats=st.data_ptr(), w1=w1.data_ptr(), ldw1=C, cd=cd.data_ptr(), w2p=w2.data_ptr(),
                            ldw2=4 * C, b2=b2.data_ptr(), gate=None, out=out.data_ptr(), ldo=C, M=M, C=C, dtype=ops.dt)
        rc = ops.lib.idf_mlp_geglu(ctypes.byref(args), None)
        torch.cuda.synchronize()
        assert rc == _lib.E_UNSUPPORTED == R.E_UNSUPPORTED
        with pytest.raises(_lib.IdfError, match="unsupported"):
            _lib.check(rc, "idf_mlp_geglu")
        assert guard() == "" and bool(torch.isnan(out).all()), "a refused call must not write"


# ---- overflow is torch.to --------------------------------------------------------------------------------------------------------
TARGETS = [70000.0, -70000.0, 65504.0, 65519.0]           # fp16: +inf, -inf, the largest finite value kept, below the tie at 65520 -> 65504


@pytest.mark.parametrize("kernel", GEMM_KERNELS)
def test_overflow_is_torch_to(kernel):
    """fp16 results beyond the type's range are ``want.to(fp16)`` bit for bit where the 16-bit conversion lives in a generated stream:
    integer data and the identity fold ((mu, rstd) = (0, 1), c = 0), every sum exact in fp32; d[n] puts chosen columns -- of a q | k
    chunk and of a V chunk -- on +-7e4, 65504 and 65519, and two columns with live weights straddle the tie at 65520.  For GEGLU the
    gate half is exactly 16 (gelu(16) = 16 to the last bit) and the value half is the target / 16."""
    from instancediffusion_amd.engine import pack_geglu
    ops = ops_for("fp16")
    k = R.KERNELS[kernel]
    M, N, Kk, cols = R.m0(kernel, cus()), k["N"], k["K"], k["cols"]
    g = torch.Generator(device="cuda").manual_seed(940)
    x = torch.randint(-3, 4, (M, Kk), generator=g, device="cuda").half()
    w = torch.randint(-3, 4, (N, Kk), generator=g, device="cuda").half()
    d = torch.zeros(N, device="cuda")
    st = torch.tensor([0.0, 1.0], device="cuda").repeat(M, 1)
    wantt = torch.tensor(TARGETS).half()
    assert wantt.tolist() == [float("inf"), float("-inf"), 65504.0, 65504.0]
    if kernel == "geglu640":
        tcols = torch.tensor([7, 70, 1333, cols - 1])
        w[tcols], w[cols + tcols] = 0, 0
        d[tcols], d[cols + tcols] = torch.tensor(TARGETS, device="cuda") / 16, 16.0
        wp, dp = pack_geglu(w, d, 32)
        case = dict(kernel=kernel, M=M, x=x, stats=st, wp=wp, cp=torch.zeros(N), dp=dp)
    else:
        nv = N - cols
        tcols = torch.tensor([7, 70, cols // 2 + 13, cols - 1, cols, cols + 33, cols + nv // 2 + 4, N - 1])
        live = torch.tensor([9, cols + 9])
        w[tcols] = 0
        d[tcols], d[live] = torch.tensor(TARGETS + TARGETS, device="cuda"), 65512.0
        case = dict(kernel=kernel, M=M, x=x, stats=st, w=w, c=torch.zeros(N), d=d)
    out, vt, guards, served, _ = launch(ops, case)
    assert served == 1
    if kernel == "geglu640":
        exact(f"{kernel} fp16 overflow", out[:, tcols.cuda()], wantt.repeat(M, 1), guards[0])
        return
    want = (x.float() @ w.float().t() + d).half()         # exact: integers below 2^24
    lv = want[:, live.cuda()].float()
    assert bool(torch.isinf(lv).any()) and bool((lv == 65504).any()), "the live columns straddle the tie"
    got = torch.cat([out, vt.t()], 1)
    assert bool((got == want).all()), f"{int((got != want).sum())} elements are not want.to(fp16)"
    exact(f"{kernel} fp16 overflow q | k", out[:, tcols[:4].cuda()], wantt.repeat(M, 1), guards[0])
    exact(f"{kernel} fp16 overflow V^T", vt[(tcols[4:] - cols).cuda()], wantt[:, None].repeat(1, M), guards[1])


# ---- idf_mlp_geglu: mlp320_kernel (IDF_TUNE_MLP 0) and mlp320w_kernel (1) ----------------------------------------------------------
def mlp_built(M, dt):
    """(case on the GPU, rows checked, x of those rows, y, S): the gate-independent part of the reference, once per (M, dt)."""
    key = ("mlp", M, dt)
    if key not in _CACHE:
        case = R.row_case("mlp", M, dt, device="cuda")
        rows = torch.arange(M) if M <= 4096 else R.sample_rows(M, 128, grid("mlp", M))
        x = case["x"][rows.cuda()].cpu()
        y, S = R.mlp_core(x, case["stats"][rows.cuda()].cpu(), case["w"], case["c"], case["d"], case["w2"], case["b2"], dt)
        from instancediffusion_amd.ops import HipOps
        case["cd"], case["w2p"] = HipOps.mlp_pack(case["wp"].cuda(), case["cp"].cuda(), case["dp"].cuda(), case["w2"].cuda())
        _CACHE[key] = (case, rows, x, y, S)
    return _CACHE[key]


def mlp_launch(ops, case, mode, *, inplace=False, gate=None, pad=0, x=None, st=None):
    """-> (out, guard check).  ``pad``: ldx, ldo, ldw1, ldw2 longer by that much (spare columns NaN); in place, x and out are one buffer."""
    M = case["M"]
    xs = case["x"] if x is None else x
    out, guard = R.guarded((M, R.MLP_C), ops.dtype, "cuda", ld=R.MLP_C + pad)
    if inplace:
        out.copy_(xs)
        xin = out
    else:
        xin = padded(xs, pad)
    gt = None if gate is None else torch.tensor([gate], dtype=torch.float32, device="cuda")
    with knob(ops.lib, ids()["mlp"][0], mode):
        ops.mlp_geglu(xin, case["stats"] if st is None else st, padded(case["wp"], pad), case["cd"], padded(case["w2p"], pad),
                      case["b2"].cuda(), out, gate=gt)
        torch.cuda.synchronize()
    return out, guard


def mlp_sizes():
    return [128, 128 * 13, 128 * 24, 128 * (cus() + 1), 128 * (2 * cus() + 8)]


MLP_VARIANTS = [(False, None, 0), (True, 0.6, 0), (False, -1.25, 8), (True, None, 8), (True, -1.25, 0), (False, 0.6, 8)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("inplace,gate,pad", MLP_VARIANTS)
@pytest.mark.parametrize("size", range(5))
def test_fused_mlp(size, inplace, gate, pad, dt):
    """One tile; 13 workgroups (the G % 8 != 0 branch of mw_first_tile with more than one); 24 (G % 8 == 0 below the CU count); one and
    eight tiles more than one / two per CU.  Out of place and in place, gate None / 0.6 / -1.25, contiguous and with ldx, ldo, ldw1,
    ldw2 padded by 8: both kernels inside the per-element MLP bound (all rows up to M = 4096, the sample beyond) and bit-identical."""
    ops = ops_for(dt)
    M = mlp_sizes()[size]
    assert R.row_takes("mlp", M, cus(), **(dict(lda=328, ldo=328, ldw=328, ldw2=1288) if pad else {}))
    case, rows, x, y, S = mlp_built(M, dt)
    want, slack = R.mlp_gated(x, y, S, gate)
    outs = {}
    for mode in (1, 0):
        out, guard = mlp_launch(ops, case, mode, inplace=inplace, gate=gate, pad=pad)
        check_sample(f"fused MLP {dt} M{M} grid {grid('mlp', M)} kernel {mode} inplace={inplace} gate={gate} pad={pad}", dt, out, None, rows,
                     want, slack, [guard])
        outs[mode] = out
    assert torch.equal(outs[0], outs[1]), "mlp320w_kernel and mlp320_kernel must agree bit for bit"


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("mode", [0, 1])
def test_fused_mlp_gate_zero_returns_x(mode, dt):
    """x + 0 * finite is x, bit for bit."""
    ops = ops_for(dt)
    case = mlp_built(128 * 13, dt)[0]
    for inplace in (False, True):
        out, guard = mlp_launch(ops, case, mode, inplace=inplace, gate=0.0)
        exact(f"fused MLP {dt} kernel {mode} gate 0.0 inplace={inplace}", out, case["x"].cpu(), guard)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("mode", [0, 1])
def test_a_rows_mlp_result_does_not_depend_on_where_it_runs(mode, dt):
    ops = ops_for(dt)
    M = mlp_sizes()[-1]
    case = mlp_built(M, dt)[0]
    x, st = case["x"].clone(), case["stats"].clone()
    src, dsts = copy_sites("mlp", M)
    for d in dsts:
        x[d:d + 32], st[d:d + 32] = x[src:src + 32], st[src:src + 32]
    out, guard = mlp_launch(ops, case, mode, gate=0.6, x=x, st=st)
    assert guard() == "" and not torch.equal(out[src:src + 32], out[src + 32:src + 64])
    for d in dsts:
        assert torch.equal(out[d:d + 32], out[src:src + 32]), f"rows {d} .. differ from their originals"
