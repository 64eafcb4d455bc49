"""The bandwidth-bound kernels on a real MI355X, per kernel, in bf16 AND fp16, at the shapes where they change path: gn_stats_kernel /
gn_apply_kernel, ln_kernel (LayerNorm and the 2x2 patch gather), row_stats_kernel, dwconv7_kernel, seg_in_conv_kernel, the ScaleU
pair, temb_kernel, unifusion_embed_kernel, both conv_in kernels and cast_kernel.

Every result is compared with an fp64 reference of the same operation on the same 16-bit-rounded inputs
(tests/small_kernel_cases.py, proved on the CPU by tests/test_small_kernel_refs.py): all outputs finite, NO element outside
``within_one_rounding`` (the ULP of the element's own magnitude, so an error on the small outputs shows), relmax below one ULP of the
largest, and rel-rms below the project's bar where there are enough elements for an rms.  Outputs live in NaN-filled buffers with a
guard row (and pad columns, where the entry point takes a leading dimension) that must still be NaN afterwards.
"""
import ctypes as C

import pytest
import torch

from tests import small_kernel_cases as K

pytestmark = pytest.mark.gpu

DTS = ["bf16", "fp16"]


def cid(case):
    return "x".join(str(v) for v in case)
_OPS = {}
NAN = float("nan")


def ops_for(dt):
    if dt not in _OPS:
        from instancediffusion_amd.ops import HipOps
        _OPS[dt] = HipOps(K.DTYPES[dt])
    return _OPS[dt]


def dev(inp):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in inp.items()}


def guarded(shape, dtype):
    """A contiguous NaN-filled output of ``shape`` with one guard row (of the last dimension) behind it: (view, guard)."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + shape[-1],), NAN, dtype=dtype, device="cuda")
    return buf[:n].view(shape), buf[n:]


def untouched(t):
    return bool(torch.isnan(t).all())


def check(entry, dt, shape, got, want):
    torch.cuda.synchronize()
    em, er = K.relmax(got, want), K.rel_rms(got, want)
    share = K.within_one_rounding(got, want, dt)
    print(f"[parity] {entry} {dt} {shape}: relmax {em:.2e} rel-rms {er:.2e} outside-one-rounding {share:.2e}")
    assert bool(torch.isfinite(got).all()), "non-finite output"
    assert share == 0.0, f"{share:.3e} of the elements are further than one {dt} rounding from the fp64 reference"
    assert em < K.U[dt]
    if want.numel() >= K.RMS_MIN_ELEMS:
        assert er < K.RMS_BAR[dt]


def raises(kind):
    from instancediffusion_amd._lib import IdfError
    return pytest.raises(IdfError, match=kind)


# ---- GroupNorm ---------------------------------------------------------------------------------------------------------------
def run_groupnorm(ops, inp, silu, **kw):
    d = dev(inp)
    out, guard = guarded(tuple(inp["x"].shape), ops.dtype)
    ops.groupnorm(d["x"], out, d["gamma"], d["beta"], K.GN_EPS, silu, **kw)
    torch.cuda.synchronize()
    assert untouched(guard), "stored behind the last row"
    return out


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", K.GN_CASES, ids=cid)
def test_groupnorm(case, dt, silu):
    ops, inp = ops_for(dt), K.gn_inputs(case, dt)
    want = K.gn_want(inp, silu)
    out = run_groupnorm(ops, inp, silu)
    check("idf_groupnorm" + ("+silu" if silu else ""), dt, case, out, want)
    assert torch.equal(out, run_groupnorm(ops, inp, silu)), "GroupNorm must be bitwise run-to-run deterministic"
    if case == (1, 1, 32):                                    # one value per group: no variance, the output is beta itself
        assert torch.equal(out.cpu(), want.to(K.DTYPES[dt]).view(out.shape))


@pytest.mark.parametrize("dt", DTS)
def test_groupnorm_large_mean(dt):
    """|mean| / std = 157 on a shape with an empty trailing row chunk; the inputs are exact in both types."""
    ops, inp = ops_for(dt), K.gn_inputs(K.GN_LARGE_MEAN, dt, large=True)
    assert torch.equal(inp["x"].float(), K.large_mean(K.GN_LARGE_MEAN, 59))
    out = run_groupnorm(ops, inp, False)
    check("idf_groupnorm mean/std=157", dt, K.GN_LARGE_MEAN, out, K.gn_want(inp, False))
    assert torch.equal(out, run_groupnorm(ops, inp, False))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("nchunks", [1, 7, 49])
def test_groupnorm_split_entry_points(nchunks, dt):
    """idf_groupnorm_stats, then idf_groupnorm_apply on its partials: any chunk count meets the bound, the combined entry point's own
    count reproduces it bit for bit."""
    ops, inp = ops_for(dt), K.gn_inputs(K.GN_SPLIT, dt)
    B, HW, Cc = K.GN_SPLIT
    d = dev(inp)
    partial, guard = guarded((B, nchunks, 32, 2), torch.float32)
    rc = ops.lib.idf_groupnorm_stats(C.c_void_p(d["x"].data_ptr()), C.c_void_p(partial.data_ptr()), B, HW, Cc, nchunks, ops.dt,
                                     ops._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert untouched(guard) and bool(torch.isfinite(partial).all())
    out = run_groupnorm(ops, inp, True, partial=partial)
    check(f"idf_groupnorm_stats+apply nchunks={nchunks}", dt, K.GN_SPLIT, out, K.gn_want(inp, True))
    if nchunks == max(1, min(64, HW // 32)):                  # gn_nchunks(HW)
        assert torch.equal(out, run_groupnorm(ops, inp, True))


def test_groupnorm_rejects_before_any_launch():
    """C = 8192 passes the statistics pass's LDS limit and not the apply pass's: nothing may run, the workspace stays as it was."""
    ops = ops_for("bf16")
    B, HW, Cc = 1, 4, 8192
    x, out = ops.zeros((B, HW, Cc)), ops.zeros((B, HW, Cc))
    gm, bt = torch.ones(Cc, device="cuda"), torch.zeros(Cc, device="cuda")
    ws = torch.full((int(ops.lib.idf_groupnorm_ws_floats(B, HW)) + 64,), NAN, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = ops.lib.idf_groupnorm(p(x), p(out), p(gm), p(bt), p(ws), B, HW, Cc, 1e-5, 0, ops.dt, ops._stream())
    torch.cuda.synchronize()
    assert rc == -3 and untouched(ws)                         # IDF_E_UNSUPPORTED
    rc = ops.lib.idf_groupnorm(p(x), p(out), p(gm), p(bt), p(ws), B, HW, 4096, 1e-5, 0, ops.dt, ops._stream())
    torch.cuda.synchronize()
    assert rc == 0 and not untouched(ws[:64])                 # the same call at a supported width does run


# ---- LayerNorm, row statistics, patch gather ---------------------------------------------------------------------------------
def run_layernorm(ops, inp, pad=8):
    M, Cc = inp["x"].shape
    d = dev(inp)
    xb = torch.full((M, Cc + pad), NAN, dtype=ops.dtype, device="cuda")
    xb[:, :Cc] = d["x"]
    ob = torch.full((M + 1, Cc + pad), NAN, dtype=ops.dtype, device="cuda")
    ops.layernorm(xb[:, :Cc], ob[:M, :Cc], d["gamma"], d["beta"], K.LN_EPS)
    torch.cuda.synchronize()
    assert untouched(ob[M]) and untouched(ob[:M, Cc:]), "stored outside the view"
    return ob[:M, :Cc], xb


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", K.LN_CASES, ids=cid)
def test_layernorm_and_row_stats(case, dt):
    ops, inp = ops_for(dt), K.ln_inputs(case, dt)
    M, Cc = case
    out, xb = run_layernorm(ops, inp)
    check("idf_layernorm", dt, case, out, K.ln_want(inp))
    stats, guard = guarded((M, 2), torch.float32)
    ops.row_stats(xb[:, :Cc], stats, K.LN_EPS)
    torch.cuda.synchronize()
    mu, rstd = K.row_stats_ref(inp["x"], K.LN_EPS)
    e_mu, e_rs = K.relmax(stats[:, 0], mu), K.relmax(stats[:, 1], rstd)
    print(f"[parity] idf_row_stats {dt} {case}: mean relmax {e_mu:.2e} rstd relmax {e_rs:.2e}")
    assert untouched(guard) and bool(torch.isfinite(stats).all())
    assert e_mu < 1e-5 and e_rs < 1e-5


@pytest.mark.parametrize("dt", DTS)
def test_layernorm_large_mean_rows(dt):
    ops, inp = ops_for(dt), K.ln_inputs(K.LN_LARGE_MEAN, dt, large=True)
    assert torch.equal(inp["x"].float(), K.large_mean(K.LN_LARGE_MEAN, 61))
    out, xb = run_layernorm(ops, inp)
    check("idf_layernorm mean/std=157", dt, K.LN_LARGE_MEAN, out, K.ln_want(inp))
    stats, _ = guarded((K.LN_LARGE_MEAN[0], 2), torch.float32)
    ops.row_stats(xb[:, :K.LN_LARGE_MEAN[1]], stats, K.LN_EPS)
    torch.cuda.synchronize()
    mu, rstd = K.row_stats_ref(inp["x"], K.LN_EPS)
    assert K.relmax(stats[:, 0], mu) < 1e-5 and K.relmax(stats[:, 1], rstd) < 1e-5


def test_layernorm_rejects():
    ops = ops_for("bf16")
    inp = K.ln_inputs((5, 1544), "bf16")
    with raises("invalid argument"):                          # C > 1536: more than three register chunks per lane
        run_layernorm(ops, inp)
    inp = K.ln_inputs((5, 520), "bf16")
    with raises("misaligned"):                                # rows not 16-byte aligned
        run_layernorm(ops, inp, pad=4)
    st = torch.zeros(5, 2, device="cuda")
    with raises("invalid argument"):
        ops.row_stats(ops.zeros((5, 1544)), st)
    with raises("misaligned"):
        ops.row_stats(ops.zeros((5, 524))[:, :520], st)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", K.LNP_CASES, ids=cid)
def test_layernorm_patch2(case, dt):
    ops, inp = ops_for(dt), K.lnp_inputs(case, dt)
    B, H, W, Cc = case
    R = B * (H // 2) * (W // 2)
    d = dev(inp)
    ob = torch.full((R + 1, 4 * Cc + 8), NAN, dtype=ops.dtype, device="cuda")
    ops.layernorm_patch2(d["x"], ob[:R], d["gamma"], d["beta"], K.LN_EPS)
    torch.cuda.synchronize()
    assert untouched(ob[R]) and untouched(ob[:R, 4 * Cc:]), "the pad columns and the guard row must stay untouched"
    check("idf_layernorm_patch2", dt, case, ob[:R, :4 * Cc], K.lnp_want(inp))


def test_layernorm_patch2_rejects_odd_height():
    ops = ops_for("bf16")
    d = dev(K.lnp_inputs((1, 3, 2, 8), "bf16"))
    with raises("invalid argument"):
        ops.layernorm_patch2(d["x"], ops.zeros((2, 40)), d["gamma"], d["beta"], K.LN_EPS)


# ---- ConvNeXt pieces ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", K.DW_CASES, ids=cid)
def test_dwconv7x7(case, dt):
    ops, inp = ops_for(dt), K.dw_inputs(case, dt)
    d = dev(inp)
    out, guard = guarded(case, ops.dtype)
    ops.dwconv7x7(d["x"], d["w"], d["bias"], out)
    torch.cuda.synchronize()
    assert untouched(guard)
    check("idf_dwconv7x7", dt, case, out, K.dw_want(inp))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", K.SEG_CASES, ids=cid)
def test_seg_in_conv(case, dt):
    ops, inp = ops_for(dt), K.seg_inputs(case)
    B, _, S, ldo = case
    R = B * (S // 4) ** 2
    d = dev(inp)
    ob = torch.full((R + 1, ldo), NAN, dtype=ops.dtype, device="cuda")
    ops.seg_in_conv(d["segs"], d["w"], d["bias"], ob[:R])
    torch.cuda.synchronize()
    assert untouched(ob[R]) and (ldo == 48 or untouched(ob[:R, 48:])), "columns >= 48 and the guard row must stay untouched"
    check("idf_seg_in_conv", dt, case, ob[:R, :48], K.seg_want(inp))


def test_seg_in_conv_rejects():
    ops = ops_for("bf16")
    for case in ((1, 33, 8, 48), (1, 4, 6, 48)):              # Cin beyond the LDS image; S not a multiple of the 4x4 patch
        d = dev(K.seg_inputs(case))
        with raises("invalid argument"):
            ops.seg_in_conv(d["segs"], d["w"], d["bias"], ops.zeros((4, 48)))


# ---- ScaleU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", K.SCALEU_CASES, ids=cid)
def test_scaleu_concat(case, dt):
    ops, inp = ops_for(dt), K.scaleu_inputs(case, dt)
    B, H, W, Ch, Cs = case
    d = dev(inp)
    out, guard = guarded((B, H, W, Ch + Cs), ops.dtype)
    ops.scaleu_concat(d["h"], d["skip"], out, d["hscale"], d["sm1"])
    torch.cuda.synchronize()
    assert untouched(guard)
    want = K.scaleu_want(inp)
    check("idf_scaleu_concat h", dt, case, out[..., :Ch], want[..., :Ch])
    check("idf_scaleu_concat skip", dt, case, out[..., Ch:], want[..., Ch:])


def test_scaleu_rejects_a_plane_beyond_the_twiddle_table():
    ops = ops_for("bf16")
    d = dev(K.scaleu_inputs((1, 129, 2, 8, 8), "bf16"))
    with raises("invalid argument"):
        ops.scaleu_concat(d["h"], d["skip"], ops.zeros((1, 129, 2, 16)), d["hscale"], d["sm1"])


# ---- embeddings, conv_in, cast -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", K.TEMB_CASES, ids=cid)
def test_timestep_embedding(case, dt):
    """Values in [-1, 1] of angles up to 999: an fp32 ulp of the angle is 6e-5, so the bound is absolute, one ULP of 1."""
    ops, inp = ops_for(dt), K.temb_inputs(case)
    B, dim, _ = case
    out, guard = guarded((B, dim), ops.dtype)
    ops.timestep_embedding(inp["t"].cuda(), out)
    torch.cuda.synchronize()
    want = K.temb_want(case, inp)
    err = float((out.double().cpu() - want).abs().max())
    print(f"[parity] idf_timestep_embedding {dt} {(B, dim)} t={inp['t'].tolist()}: max abs err {err:.2e} rel-rms {K.rel_rms(out, want):.2e}")
    assert untouched(guard) and bool(torch.isfinite(out).all())
    assert err < K.U[dt]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", K.UNI_CASES, ids=cid)
def test_unifusion_embed(case, dt):
    ops, inp = ops_for(dt), K.uni_inputs(case)
    rows, text_dim, D = case
    d = dev(inp)
    out, guard = guarded((rows, text_dim + 32 * D), ops.dtype)
    ops.unifusion_embed(d["text"], d["loc"], d["tmask"], d["lmask"], d["null_text"], d["null_loc"], d["freqs"], out)
    torch.cuda.synchronize()
    assert untouched(guard)
    check("idf_unifusion_embed", dt, case, out, K.uni_want(inp))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", K.CONV_IN_CASES, ids=cid)
def test_conv_in(case, dt):
    ops, inp = ops_for(dt), K.conv_in_inputs(case)
    B, _, H, W, Cout = case
    d = dev(inp)
    out, guard = guarded((B, H, W, Cout), ops.dtype)
    ops.conv_in(d["x"], d["w"], d["bias"], out)
    torch.cuda.synchronize()
    assert untouched(guard)
    check("idf_conv_in", dt, case, out, K.conv_in_want(inp))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n", [1, 7, 257, 4099])
def test_cast16_is_torch_to(n, dt):
    """Bit for bit ``x.to(dtype)``: round to nearest even, overflow to inf, fp16 subnormals kept, the sign of zero kept."""
    ops, x = ops_for(dt), K.cast16_input(n, dt)
    out, guard = guarded((n,), ops.dtype)
    ops.cast16(x.cuda(), out)
    torch.cuda.synchronize()
    assert untouched(guard)
    got, want = out.cpu(), x.to(K.DTYPES[dt])
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan)
    bad = (got.view(torch.int16) != want.view(torch.int16)) & ~nan
    assert not bool(bad.any()), [(float(x[i]), float(got[i]), float(want[i])) for i in bad.nonzero().flatten().tolist()[:8]]
