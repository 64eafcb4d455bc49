"""proj320s_kernel (csrc/proj320_stream.hip) on a real MI355X: the N = K = 320 projections behind idf_gemm with the weights resident
in registers and the rows streaming through LDS, against fp64 torch on the same 16-bit operands and against the launches it
replaces (the same idf_gemm call with IDF_TUNE_PROJ_ROW = 0).

Error bar.  The two paths differ in fp32 summation order only, so nobody can derive the figure ahead of time; the bar is relative:
the new kernel's rel-RMS error against fp64 may exceed the replaced path's on the same operands by at most 10 %.  Both are printed.

out_stats are held to torch.var_mean (fp64) of the STORED 16-bit output.  The kernel sums a row's 320 fp32 values as 8 chains of
40 plus three pairwise steps, twice (mean, then squared deviations): |mu - mu64| <= 43 * 2^-24 * mean|v| = 2.6e-6 mean|v|, held at
1e-5 (mean|v| + |mu|); rstd inherits twice the relative error of the variance plus one rsqrt ulp, held at 2e-5 relative.

Shapes: M = the least the kernel takes on the box (two 256-row tiles per CU, the rule of qkv320w_kernel: 84 MB per matrix at 256 CUs),
that + one 32-row block (an uneven tail across CUs), and 3.5 tiles per CU.
"""
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

C = 320
BASE_ROWS = 1024                     # the operands repeat with this period: the same row lands in different blocks / workgroups
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


def gen(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def rel_rms(a, b):
    a, b = a.double(), b.double()
    return float(((a - b).pow(2).mean() / b.pow(2).mean().clamp_min(1e-300)).sqrt())


@pytest.fixture(scope="module")
def lib():
    from instancediffusion_amd import _lib
    return _lib.load()


def stat(lib, which):
    return int(lib.idf_get_stat(which))


def min_m(lib):
    from instancediffusion_amd import _lib
    m = stat(lib, _lib.IDF_STAT_PROJ_ROW_MIN_M)
    assert m > 0 and m % 1024 == 0
    return m


def sizes(lib):
    m = min_m(lib)
    return {"min": m, "min+1": m + 32, "3.5": m // 2 * 3 + m // 4}


_OPERANDS = {}


def operands(dtype_name, M):
    """(A, W, bias, res, gate, ln stats, c) for one dtype and M, built once; the row period is BASE_ROWS."""
    key = (dtype_name, M)
    if key not in _OPERANDS:
        _OPERANDS.clear()                                    # one set resident at a time
        dt = DTYPES[dtype_name]
        rep = lambda t: t.repeat(M // BASE_ROWS + 1, 1)[:M].contiguous().cuda()
        a = rep((gen((BASE_ROWS, C), 11) * 1.3 + 0.5 * gen((BASE_ROWS, 1), 12)).to(dt))
        # LN_ROW operand: rows whose mean is ~100 x their std (the (acc - mu c) cancellation at its worst)
        s = 0.02 * (1 + gen((BASE_ROWS, 1), 13).abs())
        a_ln = rep((100 * s + s * gen((BASE_ROWS, C), 14)).to(dt))
        w = gen((C, C), 15, C ** -0.5).to(dt).cuda()
        bias = gen((C,), 16).cuda()
        res = rep(gen((BASE_ROWS, C), 17, 2.0).to(dt))
        gate = torch.tensor([0.37], device="cuda")
        _OPERANDS[key] = dict(a=a, a_ln=a_ln, w=w, bias=bias, res=res, gate=gate, c=w.float().sum(1).contiguous())
    return _OPERANDS[key]


def reference(op, epi, st):
    """fp64 torch on the same 16-bit operands (and the same fp32 statistics / constants), one period of rows."""
    a = (op["a_ln"] if epi == "ln" else op["res"] if epi == "allsame" else op["a"])[:BASE_ROWS].double()
    y = a @ op["w"].double().t()
    if epi == "ln":
        y = st[:BASE_ROWS, 1:2].double() * (y - st[:BASE_ROWS, 0:1].double() * op["c"].double()[None, :])
    y = y + op["bias"].double()[None, :]
    if epi in ("res", "inplace", "allsame"):
        y = op["res"][:BASE_ROWS].double() + y
    if epi == "gate":
        y = op["res"][:BASE_ROWS].double() + op["gate"].double() * y
    return y


def call(ops, op, epi, st, stats, alias=True):
    """One idf_gemm call -> (out, out_stats or None).  alias=False: the cases whose output overwrites A run with a separate output
    (the same arithmetic; the replaced path tiles N and promises nothing for out == A)."""
    M = op["a"].shape[0]
    kw = dict(bias=op["bias"])
    a = op["a"]
    out = ops.empty((M, C))
    out.fill_(float("nan"))
    if epi == "ln":
        a, kw["ln_row"] = op["a_ln"], (st, op["c"])
    if epi in ("res", "gate"):
        kw["res"] = op["res"]
    if epi == "inplace":                                     # out is res (the attention out-projections on y, proj_out on x), A differs
        out = op["res"].clone()
        kw["res"] = out
    if epi == "aout":                                        # out is A (the kernel holds a block's rows in LDS before its first store)
        a = op["a"].clone()
        out = a if alias else out
    if epi == "allsame":                                     # out is res is A
        a = op["res"].clone()
        kw["res"] = a if alias else op["res"]
        out = a if alias else out
    if epi == "gate":
        kw["gate"] = op["gate"]                              # read from device memory by the kernel
    ost = None
    if stats:
        ost = ops.empty((M, 2), torch.float32)
        ost.fill_(float("nan"))
        kw["out_stats"] = ost
    ops.gemm(a, op["w"], out, **kw)
    torch.cuda.synchronize()
    return out, ost


@pytest.mark.parametrize("stats", [False, True], ids=["", "out_stats"])
@pytest.mark.parametrize("epi", ["bias", "res", "inplace", "gate", "ln", "aout", "allsame"])
@pytest.mark.parametrize("size", ["min", "min+1", "3.5"])
@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
def test_against_fp64_and_the_replaced_path(lib, dtype_name, size, epi, stats):
    from instancediffusion_amd import _lib
    from instancediffusion_amd.ops import HipOps
    ops = HipOps(DTYPES[dtype_name])
    M = sizes(lib)[size]
    op = operands(dtype_name, M)
    st = None
    if epi == "ln":
        st = ops.empty((M, 2), torch.float32)
        ops.row_stats(op["a_ln"], st, 1e-5)
    want = reference(op, epi, st)
    got = {}
    for knob in (1, 0):
        prev = lib.idf_set_tuning(_lib.IDF_TUNE_PROJ_ROW, knob)
        try:
            n0, b0 = stat(lib, _lib.IDF_STAT_PROJ_ROW_LAUNCHES), stat(lib, _lib.IDF_STAT_GEMM_BIG_LAUNCHES)
            got[knob] = call(ops, op, epi, st, stats, alias=bool(knob))
            served = stat(lib, _lib.IDF_STAT_PROJ_ROW_LAUNCHES) - n0
            big = stat(lib, _lib.IDF_STAT_GEMM_BIG_LAUNCHES) - b0
        finally:
            lib.idf_set_tuning(_lib.IDF_TUNE_PROJ_ROW, prev)
        assert served == knob, (knob, served)
        if knob:
            assert big == 1                                  # a served call is also counted with the persistent-kernel launches
    out, ost = got[1]
    old, _ = got[0]
    assert torch.isfinite(out.float()).all()
    e_new, e_old = rel_rms(out[:BASE_ROWS], want), rel_rms(old[:BASE_ROWS], want)
    print(f"[proj320s] {dtype_name} M{M} {epi}{' +out_stats' if stats else ''}: rel-rms vs fp64 {e_new:.4e}, replaced path {e_old:.4e} "
          f"(ratio {e_new / e_old:.4f}); differing elements {float((out != old).float().mean()):.2e}")
    assert e_new <= 1.10 * e_old
    # the same row in different blocks / workgroups: the same bits
    per = [out[i:i + BASE_ROWS] for i in range(0, M - BASE_ROWS + 1, BASE_ROWS)]
    assert all(torch.equal(per[0], p) for p in per[1:])
    tail = M % BASE_ROWS
    if tail:
        assert torch.equal(out[M - tail:], out[:tail])
    if stats:
        var, mean = torch.var_mean(out.double(), dim=1, unbiased=False)
        mabs = out.double().abs().mean(1)
        e_mu = float(((ost[:, 0].double() - mean).abs() / (mabs + mean.abs())).max())
        e_rs = float((ost[:, 1].double() * (var + 1e-5).sqrt() - 1).abs().max())
        print(f"[proj320s] {dtype_name} M{M} {epi} out_stats vs var_mean of the stored output: mu {e_mu:.2e} (bar 1e-5), rstd {e_rs:.2e} (bar 2e-5)")
        assert e_mu <= 1e-5 and e_rs <= 2e-5


def test_exact_data_is_exact(lib):
    """Small integers: every product and sum is exact, so out == A . W^T + b bit for bit (a swapped row / column or k map cannot hide:
    W is not symmetric)."""
    from instancediffusion_amd import _lib
    from instancediffusion_amd.ops import HipOps
    for dt in (torch.bfloat16, torch.float16):
        ops = HipOps(dt)
        M = min_m(lib) + 32
        g = torch.Generator().manual_seed(5)
        a = torch.randint(-3, 4, (M, C), generator=g).to(dt).cuda()
        w = torch.randint(-3, 4, (C, C), generator=g).to(dt).cuda()
        b = torch.randint(-8, 9, (C,), generator=g).float().cuda()
        n0 = stat(lib, _lib.IDF_STAT_PROJ_ROW_LAUNCHES)
        out = ops.gemm(a, w, ops.empty((M, C)), bias=b)
        torch.cuda.synchronize()
        assert stat(lib, _lib.IDF_STAT_PROJ_ROW_LAUNCHES) - n0 == 1
        assert torch.equal(out, (a.float() @ w.float().t() + b[None, :]).to(dt))


def _both_knobs(lib, fn):
    """fn() under knob 1 and 0 -> the two results; stat 8 must not move under either."""
    from instancediffusion_amd import _lib
    res = []
    for knob in (1, 0):
        prev = lib.idf_set_tuning(_lib.IDF_TUNE_PROJ_ROW, knob)
        try:
            n0 = stat(lib, _lib.IDF_STAT_PROJ_ROW_LAUNCHES)
            res.append(fn())
            torch.cuda.synchronize()
            assert stat(lib, _lib.IDF_STAT_PROJ_ROW_LAUNCHES) == n0
        finally:
            lib.idf_set_tuning(_lib.IDF_TUNE_PROJ_ROW, prev)
    return res


def test_what_it_does_not_take_is_the_parent_launch(lib):
    """A non-qualifying M (below two tiles per CU; not a whole number of 32-row blocks), N = 320 with K = 640, a batched call and vt_out set:
    stat 8 does not move and the result is that of the knob-off library bit for bit."""
    from instancediffusion_amd.ops import HipOps
    ops = HipOps(torch.bfloat16)
    m = min_m(lib)
    w, b = gen((C, C), 21, C ** -0.5).bfloat16().cuda(), gen((C,), 22).cuda()
    for M in (m - 32, m + 16):
        a = gen((M, C), 23).bfloat16().cuda()
        r = _both_knobs(lib, lambda: ops.gemm(a, w, ops.empty((M, C)), bias=b))
        assert torch.equal(r[0], r[1])
    a6, w6 = gen((m, 2 * C), 24).bfloat16().cuda(), gen((C, 2 * C), 25, (2 * C) ** -0.5).bfloat16().cuda()
    r = _both_knobs(lib, lambda: ops.gemm(a6, w6, ops.empty((m, C)), bias=b))
    assert torch.equal(r[0], r[1])
    ab = gen((2, m, C), 26).bfloat16().cuda()
    r = _both_knobs(lib, lambda: ops.gemm(ab, w, ops.empty((2, m, C)), bias=b))
    assert torch.equal(r[0], r[1])
    a = gen((m, C), 27).bfloat16().cuda()
    st = ops.empty((m, 2), torch.float32)
    ops.row_stats(a, st, 1e-5)
    c = w.float().sum(1).contiguous()

    def vt():
        out, v = ops.empty((m, C // 2)), ops.empty((C // 2, m))
        ops.gemm(a, w, out, bias=b, ln_row=(st, c), vt_out=v)
        return torch.cat([out, v.t()], 1)
    r = _both_knobs(lib, vt)
    assert torch.equal(r[0], r[1])


def test_mode_0_of_the_persistent_kernel_bypasses_every_row_kernel(lib):
    """IDF_TUNE_GEMM_BIG = 0 is the independent small-tile reference: stats 6, 7 and 8 stay put on shapes their kernels take."""
    from instancediffusion_amd import _lib
    from instancediffusion_amd.ops import HipOps
    ops = HipOps(torch.bfloat16)
    cus = min_m(lib) // 512
    which = (_lib.IDF_STAT_QKV_ROW_LAUNCHES, _lib.IDF_STAT_GEGLU_ROW_LAUNCHES, _lib.IDF_STAT_PROJ_ROW_LAUNCHES)

    def run():
        n0 = [stat(lib, s) for s in which]
        M = 512 * cus                                        # the new kernel's shape
        a, w, b = gen((M, C), 31).bfloat16().cuda(), gen((C, C), 32, C ** -0.5).bfloat16().cuda(), gen((C,), 33).cuda()
        ops.gemm(a, w, ops.empty((M, C)), bias=b)
        M = 512 * cus                                        # qkv320w_kernel's: K = 320, N = 960, two 256-row tiles per CU
        a, w3, b3 = gen((M, C), 34).bfloat16().cuda(), gen((3 * C, C), 35, C ** -0.5).bfloat16().cuda(), gen((3 * C,), 36).cuda()
        st = ops.empty((M, 2), torch.float32)
        ops.row_stats(a, st, 1e-5)
        ops.gemm(a, w3, ops.empty((M, 2 * C)), bias=b3, ln_row=(st, w3.float().sum(1).contiguous()), vt_out=ops.empty((C, M)))
        M = 256 * cus                                        # geglu640w_kernel's: K = 640, N = 5120, two 128-row tiles per CU
        a, w8, b8 = gen((M, 2 * C), 37).bfloat16().cuda(), gen((16 * C, 2 * C), 38, (2 * C) ** -0.5).bfloat16().cuda(), gen((16 * C,), 39).cuda()
        st = ops.empty((M, 2), torch.float32)
        ops.row_stats(a, st, 1e-5)
        ops.gemm(a, w8, ops.empty((M, 8 * C)), bias=b8, geglu=True, geglu_period=32, ln_row=(st, w8.float().sum(1).contiguous()))
        torch.cuda.synchronize()
        return [stat(lib, s) - n for s, n in zip(which, n0)]

    assert run() == [1, 1, 1]                                # (the shapes do reach the three kernels under the default mode)
    prev = lib.idf_set_tuning(_lib.IDF_TUNE_GEMM_BIG, 0)
    try:
        assert stat(lib, _lib.IDF_STAT_PROJ_ROW_MIN_M) == 0
        assert run() == [0, 0, 0]
    finally:
        lib.idf_set_tuning(_lib.IDF_TUNE_GEMM_BIG, prev)


def _query_handed(knobs, p, M, fuser, takes):
    """The test's own rule for the cross-attention query of an M-row C = 320 layer: its statistics are handed in (so the kernel can
    take it) where the kernel takes M rows, the engine runs LN-self mode 1, and the producer in front of it is an idf_gemm epilogue:
    always with the fuser off (attn1's out-projection); with it on only where the fuser's feed-forward is NOT the fused MLP launch."""
    ff_fused = "w2p" in p["f_ff"] and knobs.ln_self != 2 and M >= knobs.mlp_min_m and M % 128 == 0
    return knobs.ln_self == 1 and takes(M) and not (fuser and ff_fused)


@pytest.mark.parametrize("case", ["fuser_on", "fuser_off", "paired_fuser_on_qkv_row_off_ff_unfused"])
def test_engine_forward_knob_on_and_off(lib, case):
    """A reduced-width model (one ResBlock per level, three levels; C = 320 at the first) at a row count whose C = 320 level
    qualifies, knob on and off: both within the forward bar of the reference golden, and stat 8 = the number of qualifying sites
    counted from the layer list (per C = 320 SpatialTransformer: proj_in, attn1.out, attn2.out, proj_out; f_attn.out with the fuser on;
    the cross-attention query where its statistics are handed in -- `_query_handed`, the test's own rule).  The third case is a
    PAIRED forward (the first transformer layer runs its head on half the rows and duplicates), with the q | k | v row kernel off (the
    q | k | v projection then sums its own statistics: no producer in front of the duplication) and the fuser's feed-forward as two
    GEMMs: the query's statistics come from that feed-forward, into the buffer allocated BEHIND the duplication."""
    from grounding_input.text_grounding_tokinzer_input import GroundingNetInput
    from instancediffusion_amd import _lib
    from instancediffusion_amd.engine import Cond
    from tests.test_engine_gpu import _build, _case, _check
    fuser = case != "fuser_off"
    paired = case.startswith("paired")
    gold, meta, cfg, inp = _case("mid_box")
    model = _build(cfg)
    gi = GroundingNetInput()
    model.grounding_tokenizer_input = gi
    g = {k: v.cuda() for k, v in gi.prepare(inp["gb"]).items()}
    eng = model.engine
    if paired:
        eng.knobs = dataclasses.replace(eng.knobs, qkv_row=False, mlp_min_m=1 << 30)
    L = meta["latent"]
    rows = -(-min_m(lib) // (L * L))
    rows += rows % 2
    n = rows // 2
    M = rows * L * L
    eps = {}
    with torch.no_grad():
        c = eng.prepare_cond(inp["context"].cuda(), g)
        u = eng.prepare_cond(inp["uc"][:1].cuda(), gi.get_null_input(batch=1))
        nc = inp["context"].shape[0]                         # the golden's batch: its first sample is replicated
        slot = eng.gather_cond(Cond.cat([c, u]), torch.tensor([0] * n + [nc] * n, device="cuda"))
        x = inp["x"].cuda().float()[:1].repeat(rows, 1, 1, 1)
        t = inp["t"].cuda().float()[:1].repeat(rows)
        eng.use_graphs = False
        if not fuser:
            eng.fuser_scale = 0.0
        blocks = eng.in_blocks + [eng.mid_block] + eng.out_blocks
        sts = [p for blk in blocks for p in blk if p["kind"] == "st" and p["c"] == C]
        hoisted = eng.in_blocks[1][1] if paired else None     # its proj_in and attn1.out run on the n distinct rows
        assert len(sts) > 0 and (not paired or (hoisted["kind"] == "st" and hoisted["c"] == C))
        for knob in (1, 0):
            prev = lib.idf_set_tuning(_lib.IDF_TUNE_PROJ_ROW, knob)
            try:
                takes = lambda m: eng.ops.proj_row_takes(m, C)   # the library's knob and threshold
                sites = 0
                for p in sts:
                    head = M // 2 if p is hoisted else M
                    sites += 2 * int(takes(head)) + (2 + int(fuser)) * int(takes(M)) + int(_query_handed(eng.knobs, p, M, fuser, takes))
                n0 = stat(lib, _lib.IDF_STAT_PROJ_ROW_LAUNCHES)
                eps[knob] = eng.forward_cond(x, t, slot, paired=paired).float().cpu()
                served = stat(lib, _lib.IDF_STAT_PROJ_ROW_LAUNCHES) - n0
            finally:
                lib.idf_set_tuning(_lib.IDF_TUNE_PROJ_ROW, prev)
            print(f"[proj320s] mid_box {rows}-row forward (M = {M}), {case}, knob {knob}: {served} launches on proj320s_kernel, "
                  f"{sites} qualifying sites in {len(sts)} C = 320 transformer layers")
            assert served == sites and (sites > 0) == bool(knob)
    if fuser:
        for knob in (1, 0):
            _check(eps[knob][:1], gold["eps_cond"][:1], f"mid_box {rows}-row forward, {case}, knob {knob}, cond rows", "mid_box")
            _check(eps[knob][n:n + 1], gold["eps_uncond"][:1], f"mid_box {rows}-row forward, {case}, knob {knob}, uncond rows", "mid_box")
    else:
        # the golden holds no fuser-off output: the knob-on forward is held to the knob-off one at the same bar
        err = rel_rms(eps[1], eps[0])
        print(f"[proj320s] fuser off: knob on vs knob off rel-rms {err:.3e}")
        assert err < 2e-2
    assert all(torch.equal(eps[1][i], eps[1][0]) for i in range(1, n))
