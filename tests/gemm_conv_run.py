"""What the GPU modules of the matrix-core kernels share (tests/test_gemm_conv_edges_gpu.py, tests/test_gemm_big_walk_gpu.py): forcing a
kernel family and counting its launches, launching a case of tests/gemm_conv_cases.py into NaN-guarded buffers, and the two judgements,
``check`` (finite, per-element bound, rel-rms, guards) and ``exact`` (bit for bit).  Importing it needs neither a GPU nor the HIP library."""
import contextlib

import torch

from tests import gemm_conv_cases as K

DTS = ["bf16", "fp16"]
_OPS, _REFS = {}, {}
ROW_KERNEL_STATS = ("IDF_STAT_QKV_ROW_LAUNCHES", "IDF_STAT_GEGLU_ROW_LAUNCHES", "IDF_STAT_PROJ_ROW_LAUNCHES")


def ops_for(dt):
    if dt not in _OPS:
        from instancediffusion_amd.ops import HipOps
        _OPS[dt] = HipOps(K.DTYPES[dt])
    return _OPS[dt]


def cached(key, build):
    """A case and its fp64 reference, computed once and shared by the families that run it (never modified)."""
    if key not in _REFS:
        _REFS[key] = build()
    return _REFS[key]


@contextlib.contextmanager
def forced(lib, family, big_mode=None, min_eff=None):
    """Force a kernel family; yields a function that returns the (persistent, latency) launches since.  ``big_mode`` replaces the
    family's IDF_TUNE_GEMM_BIG value (3: automatic dispatch with the hybrid tail split), ``min_eff`` sets IDF_TUNE_BIG_MIN_EFF."""
    from instancediffusion_amd import _lib
    big, ring = K.FAMILIES[family]
    prev_big = lib.idf_set_tuning(_lib.IDF_TUNE_GEMM_BIG, big if big_mode is None else big_mode)
    prev_ring = lib.idf_set_tuning(_lib.IDF_TUNE_GEMM_RING, ring)
    prev_eff = None if min_eff is None else lib.idf_set_tuning(_lib.IDF_TUNE_BIG_MIN_EFF, min_eff)
    stats = lambda: (lib.idf_get_stat(_lib.IDF_STAT_GEMM_BIG_LAUNCHES), lib.idf_get_stat(_lib.IDF_STAT_GEMM_RING_LAUNCHES))
    start = stats()
    try:
        yield lambda: tuple(a - b for a, b in zip(stats(), start))
    finally:
        if prev_eff is not None:
            lib.idf_set_tuning(_lib.IDF_TUNE_BIG_MIN_EFF, prev_eff)
        lib.idf_set_tuning(_lib.IDF_TUNE_GEMM_RING, prev_ring)
        lib.idf_set_tuning(_lib.IDF_TUNE_GEMM_BIG, prev_big)


def row_kernel_launches(lib):
    """The launch counters of the row-resident and streaming kernels (QKV_ROW, GEGLU_ROW, PROJ_ROW), which idf_gemm also counts as
    persistent-kernel launches."""
    from instancediffusion_amd import _lib
    return tuple(lib.idf_get_stat(getattr(_lib, name)) for name in ROW_KERNEL_STATS)


def assert_family(family, takes, launches, what):
    want = {"small": (0, 0), "ring": (0, 1), "big": (1, 0)}[family] if takes else (0, 0)
    assert launches == want, f"{what}: {family} family {'must take' if takes else 'must decline'} the launch; (persistent, latency) " \
                             f"launches {launches}"


def padded(t, pad):
    """``t`` on the GPU as a view of rows ``pad`` elements longer, the spare columns NaN."""
    if not pad:
        return t.cuda()
    buf = torch.full(tuple(t.shape[:-1]) + (t.shape[-1] + pad,), float("nan"), dtype=t.dtype, device="cuda")
    buf[..., :t.shape[-1]] = t.cuda()
    return buf[..., :t.shape[-1]]


def check(entry, dt, family, label, got, want, slack, guard, f32out=False):
    torch.cuda.synchronize()
    bad, ratio = K.outside(got, want, slack, dt, f32out)
    em, er = K.relmax(got, want), K.rel_rms(got, want)
    print(f"[parity] {entry} {dt} {family} {label}: err/bound {ratio:.3f} relmax {em:.2e} rel-rms {er:.2e} outside {bad}")
    assert guard() == "", f"stored outside the output view: {guard()}"
    assert bool(torch.isfinite(got).all()), "non-finite output"
    assert bad == 0, f"{bad} of {want.numel()} elements outside the bound (worst error / bound {ratio:.3f})"
    if want.numel() >= K.RMS_MIN_ELEMS:
        assert er < K.RMS_BAR[dt]


def exact(what, got, want, guard):
    """Bit for bit, with its [parity] line: the number of elements whose bits differ and the largest difference among them."""
    torch.cuda.synchronize()
    got = got.cpu()
    bad = got.view(torch.int16) != want.view(torch.int16)
    bad &= ~((got == 0) & (want == 0))                       # +0 and -0 are the same result
    worst = float((got.double() - want.double())[bad].abs().nan_to_num(nan=float("inf")).max()) if bool(bad.any()) else 0.0
    print(f"[parity] {what}: bit for bit, {int(bad.sum())} of {want.numel()} differ, largest difference {worst:.3g}")
    assert guard() == "", f"stored outside the output view: {guard()}"
    assert not bool(bad.any()), [(i, float(got[tuple(i)]), float(want[tuple(i)])) for i in bad.nonzero().tolist()[:8]]


# ---- idf_gemm ------------------------------------------------------------------------------------------------------------------
def run_gemm(ops, case, family, what, takes, w_key="w", extra=None, **force):
    """Launch the case under the forced family (``force``: further arguments of ``forced``): -> (out view, guard check, out_stats or
    None).  A case with ``ln_stats_out`` / ``vt_col0`` also gets those by-products, in guarded buffers of their own, returned in the
    ``extra`` dict: extra["ln_stats_out"] = (stats, guard check), extra["vt"] = (V^T view, guard check)."""
    a, w = case["a"].cuda(), case[w_key].cuda()
    kw = dict(case["kw"])
    geglu = kw.get("geglu", False)
    M, N = a.shape[-2], w.shape[-2] // (2 if geglu else 1)
    if case.get("vt_col0"):
        N = case["vt_col0"]
    lead = tuple(max(a.shape[:-2], w.shape[:-2]))
    out, guard = K.guarded(lead + (M, N), torch.float32 if case.get("f32out") else ops.dtype, "cuda", ld=N + case.get("ldo_pad", 0))
    for k in ("bias", "gate"):
        if k in kw:
            kw[k] = kw[k].cuda()
    if "rowbias" in kw:
        kw["rowbias"] = padded(kw["rowbias"], case.get("ldrb_pad", 0))
    if "res" in kw:
        if case.get("res_alias"):
            out.copy_(kw["res"].cuda())
            kw["res"] = out
        else:
            kw["res"] = padded(kw["res"], case.get("ldr_pad", 0))
    for k in ("ln_row", "ln_col"):
        if k in kw:
            kw[k] = tuple(None if t is None else t.cuda().contiguous() for t in kw[k])
    stats = sguard = None
    if case.get("out_stats"):
        stats, sguard = K.guarded((M, 2), torch.float32, "cuda")
        kw["out_stats"] = stats
    byproducts = {}
    if case.get("ln_stats_out"):
        byproducts["ln_stats_out"] = K.guarded((M, 2), torch.float32, "cuda")
        kw["ln_stats_out"] = byproducts["ln_stats_out"][0]
    if case.get("vt_col0"):
        byproducts["vt"] = K.guarded((w.shape[-2] - N, M), ops.dtype, "cuda")
        kw["vt_out"] = byproducts["vt"][0]
    with forced(ops.lib, family, **force) as launches:
        ops.gemm(a, w, out, **kw)
        torch.cuda.synchronize()
        assert_family(family, takes, launches(), what)
    if sguard is not None:
        assert sguard() == "", "out_stats stored outside its [M, 2]"
    if extra is not None:
        extra.update(byproducts)
    return out, guard, stats


def gemm_takes(family, case, w_key="w"):
    kw = case["kw"]
    M, Kk = case["a"].shape[-2:]
    N = case[w_key].shape[-2]
    batch = max(case["a"].dim(), case[w_key].dim()) == 3
    cols = N // 2 if kw.get("geglu") else N
    return K.family_takes(family, M, N, Kk, geglu=kw.get("geglu", False), geglu_period=kw.get("geglu_period", 64),
                          batch=3 if batch else 1, self_ln="ln_row" in kw and kw["ln_row"][0] is None,
                          ldo=cols + case.get("ldo_pad", 0), ldr=cols + case.get("ldr_pad", 0) if "res" in kw else None,
                          ld_rowbias=N + case.get("ldrb_pad", 0) if "rowbias" in kw else None)


# ---- idf_conv3x3, idf_conv3x3_down -----------------------------------------------------------------------------------------------
def run_conv(ops, case, family, what, takes, gn_partial=None, **force):
    x = case["x"]
    if x.is_contiguous():
        xd = x.cuda()
    else:                                                    # a channel slice: keep the wide rows
        base = x._base.cuda()
        xd = base[..., x.storage_offset():x.storage_offset() + x.shape[-1]]
        assert xd.stride() == x.stride()
    kw = dict(case["kw"])
    pad_lo, up = kw.pop("pad_lo"), kw.pop("up")
    B, Ho, Wo, Cout = case["out_shape"]
    nv = kw.get("n_valid", 0)
    if nv:
        out, guard = K.guarded((B, nv, Ho, Wo), torch.float32, "cuda")
    else:
        out, guard = K.guarded((B, Ho, Wo, Cout), ops.dtype, "cuda", ld=Cout + case["ldo_pad"])
    for k in ("bias", "rowbias"):
        if k in kw:
            kw[k] = kw[k].cuda()
    if "res" in kw:
        kw["res"] = padded(kw["res"], case["ldr_pad"])
    if gn_partial is not None:
        kw["gn_partial"] = gn_partial
    with forced(ops.lib, family, **force) as launches:
        if pad_lo == 0:
            kw.pop("stride")
            ops.conv3x3_down(xd, case["w"].cuda(), out, **kw)
        else:
            ops.conv3x3(xd, case["w"].cuda(), out, upsample=up, **kw)
        torch.cuda.synchronize()
        assert_family(family, takes, launches(), what)
    return out, guard
