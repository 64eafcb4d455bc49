"""tests/gemm_conv_cases.py proved on the CPU, before a GPU is involved: its fp64 references agree with the project's fp32 ones, fp32
arithmetic rounded once to the type is inside the bound on every case the GPU tests run, the bound rejects the wrong results those tests
exist to catch, the case lists reach the branches their comments name, and the guard helper sees a single stray store."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import gemm_conv_cases as K
from tests.emul_ops import EmulOps
from tests.vae_encode_cases import EncEmulOps

DTS = ["bf16", "fp16"]


def _f(t):
    return t.float() if torch.is_tensor(t) and t.dtype in (torch.bfloat16, torch.float16) else t


def _emul(kind, case):
    """The same case through the project's fp32 emulation (tests/emul_ops.py)."""
    assert issubclass(EncEmulOps, EmulOps)                   # the project's emulation, plus conv3x3_down
    ref = EncEmulOps(torch.float32)
    if kind == "conv":
        kw = dict(case["kw"])
        pad_lo, up = kw.pop("pad_lo"), kw.pop("up")
        kw = {k: _f(v) for k, v in kw.items()}
        B, Ho, Wo, Cout = case["out_shape"]
        nv = kw.get("n_valid", 0)
        out = torch.empty((B, nv, Ho, Wo) if nv else (B, Ho, Wo, Cout))
        if pad_lo == 0:
            kw.pop("stride")
            return ref.conv3x3_down(case["x"].float(), case["w"].float(), out, **kw)
        return ref.conv3x3(case["x"].float(), case["w"].float(), out, upsample=up, **kw)
    kw = {k: _f(v) for k, v in case["kw"].items()}
    quick = kw.get("act") == "quick_gelu"
    if quick:                                                # the emulation has no QuickGELU: its linear part, then the activation in fp32
        res, gate = kw.pop("res", None), kw.pop("gate", None)
        kw.pop("act")
    w = case["wp"] if kind == "geglu" else case["w"]
    if "bias" not in kw and kw.get("geglu"):
        kw["bias"] = torch.zeros(w.shape[-2])
    M, N = case["a"].shape[-2], w.shape[-2] // (2 if kw.get("geglu") else 1)
    lead = tuple(max(case["a"].shape[:-2], w.shape[:-2]))
    y = ref.gemm(case["a"].float(), w.float(), torch.empty(lead + (M, N)), **kw)
    if quick:
        y = y * torch.sigmoid(1.702 * y)
        if res is not None:
            y = res + (gate if gate is not None else 1.0) * y
    return y


@pytest.mark.parametrize("dt", DTS)
def test_references_agree_with_the_fp32_ones(dt):
    n = 0
    for label, kind, case, _ in K.all_cases(dt):
        want, slack = K.want_of(kind, case)
        assert bool(torch.isfinite(want).all()) and bool(torch.isfinite(slack).all()) and bool((slack >= 0).all()), label
        err = K.relmax(_emul(kind, case), want)
        assert err < 1e-5, (label, err)
        n += 1
    assert n > 100


@pytest.mark.parametrize("dt", DTS)
def test_fp32_arithmetic_rounded_once_is_inside_the_bound(dt):
    """What a correct kernel computes -- fp32 arithmetic of the same operation, one rounding to the output type -- has 0 elements
    outside the bound on every case, meets the rel-rms bar, and is not trivially far inside (the bound is not slack everywhere)."""
    worst = 0.0
    for label, kind, case, f32out in K.all_cases(dt):
        want, slack = K.want_of(kind, case)
        got32, _ = K.want_of(kind, case, torch.float32)
        got = got32 if f32out else got32.to(K.DTYPES[dt])
        bad, ratio = K.outside(got, want, slack, dt, f32out)
        assert bad == 0, (label, bad, ratio)
        worst = max(worst, ratio)
        if want.numel() >= K.RMS_MIN_ELEMS and not f32out:
            assert K.rel_rms(got, want) < K.RMS_BAR[dt], label
    assert 0.25 < worst <= 1.0, worst


def test_case_lists_reach_the_branches_they_name():
    for (family, shape), slices in K.SPLIT_EXPECTED.items():
        assert K.split_plan(family, *shape) == slices, (family, shape)
        assert K.family_takes(family, *shape)
    for family, shape in K.CONV_INT_CASES.items():
        M, N, Kk, kw = K.conv_dispatch_args(shape, {})
        assert K.family_takes(family, M, N, Kk, **kw)
        assert K.split_plan(family, M, N, Kk, conv=True) == K.CONV_SPLIT_EXPECTED[family], (family, shape)
    for family, shape in K.DENSE_INT_CASES.items():
        assert len(K.split_plan(family, *shape)) > 1
    # the conv that does not split K: 192 tiles of 128 x 64 in the small family
    M, N, Kk, kw = K.conv_dispatch_args(*K.CONV_NO_SPLIT)
    assert K.tile_grid(M, N, conv=True) == (192, 64) and K.split_plan("small", M, N, Kk, conv=True) == [9]
    # every other conv case has nk >= 9 and fewer than 192 tiles: the small family splits it
    for shape, opts in K.CONV_CASES:
        M, N, Kk, kw = K.conv_dispatch_args(shape, opts)
        assert len(K.split_plan("small", M, N, Kk, conv=True)) > 1, shape
    # batched launches never split, and the persistent kernel does not take them
    for (Bt, M, N, Kk, _) in K.BATCHED:
        assert K.split_plan("small", M, N, Kk, batch=Bt) == [Kk // 64] and not K.family_takes("big", M, N, Kk, batch=Bt)
    # the persistent kernel: K >= 128, whole 128- / 256- / 320-wide tiles, 16-byte rows everywhere
    assert not K.family_takes("big", 256, 128, 64) and K.family_takes("big", 256, 128, 128) and K.family_takes("big", 300, 320, 128)
    assert not K.family_takes("big", *K.EPI_SHAPES[0]) and K.family_takes("big", *K.EPI_SHAPE_BIG)
    assert not K.family_takes("big", 130, 128, 128, self_ln=True) and K.family_takes("big", 130, 256, 128, self_ln=True)
    assert not K.family_takes("big", 130, 256, 128, ldo=259) and not K.family_takes("big", 200, 640, 320, geglu=True)
    assert K.family_takes("big", 200, 640, 320, geglu=True, geglu_period=32)
    # odd leading dimensions: each misses the vector path it is there to miss, or (N = 77 in rows of 80) has a ragged last chunk
    # with spare columns behind it that a full-width store would overwrite
    for (N, what, pad) in K.ODD_LD:
        assert (N + pad) % (4 if what == "ldo_f32" else 8) != 0 or (N % 8 != 0 and what == "ldo")


def test_sweep_and_overflow_inputs_are_exact():
    for dt in DTS:
        x = K.sweep_values(dt)
        assert x.dtype == K.DTYPES[dt] and x.numel() == 128 and float(x.float().abs().max()) == 1000.0
        assert set(x[:44].float().abs().tolist()) == set(torch.tensor(K.SWEEP).to(K.DTYPES[dt]).float().tolist())
        for act in K.SWEEP_ACTS:                             # the accumulator IS the sweep value: one non-zero product per output
            case = K.sweep_case(act, dt)
            acc = case["a"].double() @ case["w"].double().t()
            assert torch.equal(acc[0, -128:], x.double()) and int((case["a"] != 0).sum()) == 5
        c = K.overflow_case(dt)
        assert torch.equal(c["a"].float(), c["a32"]) and torch.equal(c["w"].float(), c["w32"]), "every overflow input is exact in its type"
    c = K.overflow_case("fp16")
    acc = c["a32"].double() @ c["w32"].double().t()
    for value, (i, j) in K.OVERFLOW_AT.items():
        assert acc[i, j] == value, (value, float(acc[i, j]))
    r = acc.to(torch.float16)
    stored = {70000: float("inf"), -70000: float("-inf"), 65519: 65504.0, 65527: float("inf"), 65504: 65504.0}
    for value, (i, j) in K.OVERFLOW_AT.items():
        assert float(r[i, j]) == stored[value], value
    assert float(acc.abs().max()) < 2 ** 24                  # exact in the fp32 accumulator, whatever the order


def test_integer_cases_are_exact_in_fp32():
    for family, shape in K.DENSE_INT_CASES.items():
        a, w = K.gemm_operands(*shape, "bf16", kind="ints")
        assert torch.equal(a.float(), a.float().round()) and float((a.double().abs() @ w.double().abs().t()).max()) < 2 ** 24
    for family, shape in K.CONV_INT_CASES.items():
        case = K.conv_case(shape, {}, "fp16", kind="ints")
        want, slack = K.conv_want(case)
        assert torch.equal(want, want.round()) and float(slack.max()) / (9 * shape[3] * K.EPS32) < 2 ** 24


# ---- the bound rejects what the GPU tests exist to catch -------------------------------------------------------------------------
def _rejects(got32, want, slack, dt, f32out=False):
    return K.outside(got32 if f32out else got32.to(K.DTYPES[dt]), want, slack, dt, f32out)[0] > 0


@pytest.mark.parametrize("dt", DTS)
def test_a_dropped_k_tile_of_one_slice_is_outside(dt):
    """Split-K (70, 77, 576), slices of 5 + 4 K-tiles: the first slice loses its last K-tile."""
    case = K.gemm_case(70, 77, 576, dt)
    want, slack = K.gemm_want(case)
    a = case["a"].float().clone()
    a[:, 4 * 64:5 * 64] = 0
    got = a @ case["w"].float().t() + case["kw"]["bias"]
    bad, _ = K.outside(got.to(K.DTYPES[dt]), want, slack, dt)
    assert bad > 0.9 * want.numel()
    assert K.relmax(got, want) > 0.05                        # (relmax sees this one too; it would not on outputs small next to the max)


@pytest.mark.parametrize("dt", DTS)
def test_a_ragged_last_chunk_without_bias_is_outside(dt):
    """N = 77: columns 72 .. 76 are the ragged final 8-column chunk.  Shrink those columns' weights so that relmax cannot see it."""
    case = K.gemm_case(70, 77, 576, dt)
    want, slack = K.gemm_want(case)
    got = case["a"].float() @ case["w"].float().t() + case["kw"]["bias"]
    assert not _rejects(got, want, slack, dt)
    got[:, 72:] -= case["kw"]["bias"][72:]
    assert _rejects(got, want, slack, dt)
    small = dict(case, kw=dict(bias=case["kw"]["bias"].clone()))
    small["w"] = case["w"].clone()
    small["w"][72:] = (small["w"][72:].float() / 1024).to(K.DTYPES[dt])
    small["kw"]["bias"][72:] /= 1024
    want, slack = K.gemm_want(small)
    got = small["a"].float() @ small["w"].float().t() + small["kw"]["bias"]
    got[:, 72:] -= small["kw"]["bias"][72:]
    assert K.relmax(got.to(K.DTYPES[dt]), want) < K.U[dt], "the old metric passes this"
    assert _rejects(got, want, slack, dt), "the bound does not"


@pytest.mark.parametrize("period", [64, 32])
@pytest.mark.parametrize("dt", DTS)
def test_swapped_geglu_halves_are_outside(dt, period):
    case = K.geglu_case(130, 128, 64, period, dt)
    want, slack = K.gemm_ref(case["a"], case["w"], **case["ref_kw"])
    n = want.shape[-1]
    sw = torch.cat([case["w"][n:], case["w"][:n]])
    kw = dict(case["ref_kw"], bias=torch.cat([case["ref_kw"]["bias"][n:], case["ref_kw"]["bias"][:n]]),
              ln_row=(case["ref_kw"]["ln_row"][0], torch.cat([case["ref_kw"]["ln_row"][1][n:], case["ref_kw"]["ln_row"][1][:n]])))
    got, _ = K.gemm_ref(case["a"], sw, cd=torch.float32, **kw)
    assert K.outside(got.to(K.DTYPES[dt]), want, slack, dt)[0] > 0.9 * want.numel()
    # and the packing itself: the kernel's image un-packs to the reference's halves
    h = period // 2
    wp = case["wp"].view(-1, 2, h, case["w"].shape[-1])
    assert torch.equal(wp[:, 0].reshape(n, -1), case["w"][:n]) and torch.equal(wp[:, 1].reshape(n, -1), case["w"][n:])


def test_an_accumulator_rounded_to_bf16_in_an_fp16_kernel_is_outside():
    n = 0
    for label, kind, case, f32out in K.all_cases("fp16"):
        if kind != "gemm" or f32out or "act" in case["kw"] or "ln_row" in case["kw"] or "ln_col" in case["kw"]:
            continue
        want, slack = K.want_of(kind, case)
        kw = {k: v for k, v in case["kw"].items() if k in ("bias", "rowbias", "rows_per_batch", "res", "gate")}
        acc = (case["a"].float() @ case["w"].float().transpose(-1, -2)).to(torch.bfloat16).float()
        rest, _ = K.gemm_ref(torch.zeros_like(case["a"]), case["w"], cd=torch.float32, **kw)       # the epilogue's addends
        g = float(kw["gate"]) if "gate" in kw else 1.0
        got = g * acc + rest
        if want.numel() > 64 and "struct" not in label:
            assert _rejects(got, want, slack, "fp16"), label
            n += 1
    assert n >= 30


@pytest.mark.parametrize("dt", DTS)
def test_a_wrong_conv_window_is_outside(dt):
    """pad_lo off by one (the window starts at yo * stride instead of yo * stride - 1, and the reverse for conv3x3_down), and the
    clamped pixel read in place of the zero padding."""
    n = 0
    for label, kind, case, f32out in K.all_cases(dt):
        if kind != "conv" or "struct" in label:
            continue
        want, slack = K.want_of(kind, case)
        pad_lo = case["kw"]["pad_lo"]
        for mut in (dict(front=1 - pad_lo), dict(pad_mode="replicate")):
            got, _ = K.want_of(kind, case, torch.float32, **mut)
            assert got.shape == want.shape
            if torch.equal(got, K.want_of(kind, case, torch.float32)[0]):
                continue                                     # (2, 3, 3) down to 1 x 1: the one window reads no padding at all
            got = got if f32out else got.to(K.DTYPES[dt])
            assert K.outside(got, want, slack, dt, f32out)[0] > 0, (label, mut)
            n += 1
    assert n >= 2 * (len(K.CONV_CASES) + 2 * len(K.DOWN_CASES)) - 4


@pytest.mark.parametrize("dt", DTS)
def test_tanh_gelu_on_the_sweep_is_outside(dt):
    for act, kind in (("gelu", "sweep"), ("geglu64", "geglu")):
        case = K.sweep_case(act, dt)
        want, slack = K.want_of(kind, case)
        acc = (case["a"].float() @ case["w"].float().t())
        if kind == "geglu":
            v, g = acc[:, :128], acc[:, 128:]
            good, bad = v * F.gelu(g), v * F.gelu(g, approximate="tanh")
        else:
            good, bad = F.gelu(acc), F.gelu(acc, approximate="tanh")
        assert not _rejects(good, want, slack, dt)
        assert _rejects(bad, want, slack, dt)
    # the kernel's own fit (csrc/common.h gelu_erf_f, x * sigmoid(p(x)), argument clamped to +-8) is inside, as documented
    x = K.sweep_values(dt).double()
    xc = x.clamp(-8, 8)
    p = xc * (1.59501576 + xc * xc * (7.40113019e-2 + xc * xc * -7.03035068e-4))
    want = x * 0.5 * (1 + torch.erf(x / math.sqrt(2)))
    assert float(((x * torch.sigmoid(p)) - want).abs().max()) <= K.GELU_ABS


def test_a_nan_is_outside():
    case = K.gemm_case(5, 9, 64, "bf16")
    want, slack = K.gemm_want(case)
    got = want.clone()
    assert K.outside(got, want, slack, "bf16") == (0, 0.0)
    got[3, 8] = float("nan")
    bad, ratio = K.outside(got, want, slack, "bf16")
    assert bad == 1 and ratio == float("inf")
    got[3, 8] = float("inf")
    assert K.outside(got, want, slack, "bf16")[0] == 1


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_the_guard_reports_a_single_stray_store(dtype):
    for shape, ld in (((7, 9), 12), ((3, 5, 8), 8), ((2, 3, 5, 64), 72), ((1, 1), 1)):
        view, check = K.guarded(shape, dtype, ld=ld)
        assert tuple(view.shape) == shape and view.stride(-1) == 1 and view.stride(-2) == ld
        assert bool(torch.isnan(view).all()) and check() == ""
        view.fill_(1.0)
        assert check() == ""                                 # the view itself is free to write
        base = view.untyped_storage()
        flat = torch.empty(0, dtype=dtype).set_(base)        # the whole buffer
        rows = view.numel() // shape[-1]
        first = view.storage_offset()
        last = first + (rows - 1) * ld + shape[-1] - 1
        probes = [(first - 1, "front"), (0, "front"), (last + (ld - shape[-1]) + 1, "behind"), (flat.numel() - 1, "behind")]
        if ld > shape[-1]:
            probes += [(first + shape[-1], "beside"), (last + 1, "beside")]
        for pos, where in probes:
            flat[pos] = 0.0                                  # a stray store of a zero: what a zero-filled pad would not show
            assert check() == where, (shape, pos, where, check())
            flat[pos] = float("nan")
        assert check() == ""


@pytest.mark.parametrize("dt", DTS)
def test_the_out_stats_tolerance_rejects_wrong_statistics(dt):
    """Statistics of the rounded output and of the fp32 values are both inside; statistics over N - 1 columns, with eps left out
    (the case has rows whose variance is below eps), with the variance in place of rstd, and a NaN are outside."""
    for shape in K.EPI_SHAPES + [K.EPI_SHAPE_BIG]:
        case = K.gemm_case(*shape, dt, "out_stats")
        want, slack = K.gemm_want(case)
        got32, _ = K.gemm_want(case, torch.float32)
        assert float(want[:4].var(-1, unbiased=False).max()) < K.OUT_STATS_EPS < float(want[4:].var(-1, unbiased=False).min())

        def stats(x, eps=K.OUT_STATS_EPS, power=-0.5):
            x = x.float()
            mu = x.mean(-1)
            return torch.stack([mu, ((x - mu[:, None]).pow(2).mean(-1) + eps).pow(power)], -1)
        for good in (stats(got32.to(K.DTYPES[dt])), stats(got32)):
            e_mu, e_rs = K.out_stats_excess(good, want, slack, dt)
            assert e_mu <= 1.0 and e_rs <= 1.0, (shape, e_mu, e_rs)
        assert max(K.out_stats_excess(stats(got32[:, :-1]), want, slack, dt)) > 1.0
        assert K.out_stats_excess(stats(got32, eps=0.0), want, slack, dt)[1] > 1.0
        assert K.out_stats_excess(stats(got32, power=1.0), want, slack, dt)[1] > 1.0
        bad = stats(got32)
        bad[7, 0] = float("nan")
        assert K.out_stats_excess(bad, want, slack, dt)[0] == float("inf")


# ---- the persistent kernel's tile walk -----------------------------------------------------------------------------------------------
def _is_partition(walk, items):
    flat = [it for wg in walk for it in wg]
    return len(flat) == len(items) and set(flat) == set(items) and len(set(flat)) == len(flat)


def _items(M, N, bn, hybrid=None, fold=False):
    tiles = K.big_tiles(M, N, bn)
    if fold:
        return [(t, 0) for t in range(4 * tiles)]
    if hybrid is None:
        return [(t, 0) for t in range(tiles)]
    full, S = hybrid
    return [(t, 0) for t in range(full)] + [(t, s) for t in range(full, tiles) for s in range(S)]


def test_the_walk_mirror_partitions_the_work_items():
    """Every work item of every walk case runs on exactly one workgroup, under both walks, with and without the XCD permutation
    (G = 250 is no multiple of 8), whole launches, hybrid ones and the folded launch's four phases."""
    n = 0
    for label, M, N, bn, hybrid, fold, items, _ in K.walk_launches():
        walk = K.big_walk(M, N, bn, hybrid, fold)
        assert len(walk) == K.NUM_CU and _is_partition(walk, _items(M, N, bn, hybrid, fold)), label
        assert sum(len(wg) for wg in walk) == items, (label, "the work items the case table claims")
        n += 1
    assert n == len(K.WALK_DENSE) + len(K.WALK_CONV) + 4
    for G in (8, 250, 256):                                  # synthetic grids: ragged rounds, one item per slot, many rounds
        for (M, N, bn, hybrid, fold) in [(256 * 7, 640, 320, None, False), (256 * 300 + 5, 320, 320, None, False), (256 * 3, 10240, 320, None, False),
                                         (256 * 33 + 9, 8192, 256, None, False), (256 * 9, 384, 128, None, False), (256 * 140, 640, 320, (256, 3), False),
                                         (256 * 70, 320, 320, None, True), (256, 320, 320, None, False)]:
            walk = K.big_walk(M, N, bn, hybrid, fold, num_cu=G)
            want = _items(M, N, bn, hybrid, fold)
            assert len(walk) == min(G, len(want)) and _is_partition(walk, want), (G, M, N, bn, hybrid, fold)
            assert max(map(len, walk)) - min(map(len, walk)) <= 1
    # the XCD permutation: with G % 8 == 0 workgroup L takes slot (L & 7) * G / 8 + (L >> 3); the identity otherwise
    assert [wg[0][0] for wg in K.big_walk(256 * 16, 320, 320, num_cu=16)] == [0, 2, 4, 6, 8, 10, 12, 14, 1, 3, 5, 7, 9, 11, 13, 15]
    assert [wg[0][0] for wg in K.big_walk(256 * 10, 320, 320, num_cu=10)] == list(range(10))
    assert K.big_walk(256 * 5, 10240, 320, num_cu=64)[8] == [(3, 0), (4, 0), (5, 0)]         # chunked: 160 tiles, q = 2, r = 32; workgroup 8 has slot 1
    assert K.big_walk(256 * 5, 640, 320, num_cu=8)[1] == [(1, 0), (9, 0)]                    # strided: slot 1 of G = 8, 10 tiles


def test_walk_cases_follow_their_rule():
    """At least NUM_CU + 2 work items and at most NUM_CU + 32, a ragged last m-tile, some workgroup with two items; the
    chunked cases get the chunked walk and no other does; consecutive tiles enter the LDS ring on different stages."""
    for label, M, N, bn, hybrid, fold, items, chunked in K.walk_launches():
        walk = K.big_walk(M, N, bn, hybrid, fold)
        assert items >= K.NUM_CU + 2 and M % 256 != 0, label
        assert max(map(len, walk)) >= 2, label
        assert K.big_walk_chunked(M, N, bn, hybrid, fold) == chunked, label
        assert items <= K.NUM_CU + 32, label                 # a second round of a few tiles, no more
    for shape, epi, _ in K.WALK_CHUNKED:                     # 32 workgroups take two consecutive n-tiles of one m-tile
        walk = K.big_walk(shape[0], shape[1], K.walk_dense_width(shape, epi))
        two = [wg for wg in walk if len(wg) == 2]
        assert len(two) == 32 and all(b[0] == a[0] + 1 and a[0] // 32 == b[0] // 32 for a, b in two)
    # ring stages: the 2-stage kernels' tiles enter on the other stage when the K-tile count is odd (all but the K = 128 case, kept
    # for its two K-tiles); the 3-stage kernel's at 2, 0 and 1 stages (mod 3) behind
    assert sorted({s[2] // 64 % 3 for s, e, _ in K.WALK_DENSE if s[1] == 384}) == [0, 1, 2]
    assert all(s[2] // 64 % 2 == 1 for s, e, _ in K.WALK_DENSE if s[1] != 384 and s[2] != 128)
    assert all(9 * s[3] // 64 == 9 for s, _, _, _ in K.WALK_CONV + [K.WALK_GST])
    for shape, epi, _ in K.WALK_DENSE:                       # the persistent kernel takes each, on the tile width its comment names
        geglu = epi.startswith("geglu")
        assert K.family_takes("big", *shape, geglu=geglu, geglu_period=32 if "32" in epi else 64, self_ln=epi.endswith("self")), (shape, epi)
        assert K.split_plan("big", *shape, geglu=geglu) == [shape[2] // 64]
    assert [K.walk_dense_width(s, e) for s, e, _ in K.WALK_DENSE] == [320, 320, 320, 256, 256, 128, 128, 128, 320, 256, 320, 256, 320, 320, 320, 320,
                                                                     256, 320, 256, 320]
    # the fused q | k | v case: whole 320-wide tiles on either side of vt_col0, 16-token stores
    (M, N, _), _, _ = K.WALK_DENSE[12]
    assert N % 320 == 0 and K.WALK_VT_COL0 % 320 == 0 and 0 < K.WALK_VT_COL0 < N and M % 16 == 0 and M % 256 == 80
    # GST: whole 64-row chunks per sample, groups inside a wave's 160 columns, and a sample boundary inside a tile
    (B, H, W_, _, Cout, _, _), _, _, _ = K.WALK_GST
    assert (H * W_) % 64 == 0 and 160 % (Cout // 32) == 0 and (H * W_) % 256 == 128
    for shape in K.WALK_SAME_ROWS:
        assert any(s == shape for s, _, _ in K.WALK_DENSE)


def test_hybrid_plans_are_what_the_case_comments_claim():
    (M, N, Kk), _ = K.WALK_HYBRID_DENSE
    assert K.hybrid_plan(M, N, Kk) == K.WALK_HYBRID_EXPECTED["dense"]
    Mc, Nc, Kc, kw = K.conv_dispatch_args(*K.WALK_HYBRID_CONV)
    assert Kc // 64 == 18 and K.hybrid_plan(Mc, Nc, Kc) == K.WALK_HYBRID_EXPECTED["conv"] and K.family_takes("big", Mc, Nc, Kc, **kw)
    for (m, n, plan) in ((M, N, K.WALK_HYBRID_EXPECTED["dense"]), (Mc, Nc, K.WALK_HYBRID_EXPECTED["conv"])):
        walk = K.big_walk(m, n, 320, (plan["whole"], plan["S"]))
        both = [wg for wg in walk if len(wg) == 2]
        assert len(both) == plan["rem"] * plan["S"]          # e.g. eight workgroups run a whole tile and then a slice
        assert all(a[0] < plan["whole"] and a[1] == 0 and b[0] >= plan["whole"] for a, b in both)
        assert {it for wg in both for it in wg[1:]} == {(t, s) for t in range(plan["whole"], plan["whole"] + plan["rem"]) for s in range(plan["S"])}
        assert plan["tail_m0"] % 256 == 0 and plan["tail_m0"] < m
    # what test_big_kernel_hybrid_tail_split's comments say of its shapes: 288 tiles -> 5 slices of 4; 576 tiles -> 2 slices; K = 320: none
    assert K.hybrid_plan(18 * 4096, 320, 1280)["S"] == 5 and K.hybrid_plan(18 * 4096, 640, 640)["S"] == 2
    assert K.hybrid_plan(18 * 4096, 320, 320) is None
    # a grid at or above the bar launches unsplit
    assert K.hybrid_plan(256 * 230, 320, 1280) is None


def _second_round_tile(M, N, bn, num_cu=K.NUM_CU):
    """(tile, the tile its workgroup ran before it) -- the first such pair whose tiles both have all 256 rows."""
    tiles_n = N // bn
    for wg in K.big_walk(M, N, bn, num_cu=num_cu):
        for (prev, _), (tile, _) in zip(wg, wg[1:]):
            if (tile // tiles_n + 1) * 256 <= M and (prev // tiles_n + 1) * 256 <= M:
                return tile, prev
    raise AssertionError("no workgroup runs two whole tiles")


def _block(tile, N, bn):
    m_tile, n_tile = divmod(tile, N // bn)
    return slice(m_tile * 256, m_tile * 256 + 256), slice(n_tile * bn, n_tile * bn + bn)


def _walk_failure_models(want, y_last, M, N, bn, num_cu=K.NUM_CU):
    """The three failures the walk cases aim at, applied to a correct result ``want`` [M, N] (fp64; the epilogue is linear in the
    accumulator) whose last K-tile contributes ``y_last``: -> name -> mutated result."""
    tile, prev = _second_round_tile(M, N, bn, num_cu)
    (r, c), (rp, cp) = _block(tile, N, bn), _block(prev, N, bn)
    stale = want.clone()                                     # the last K-tile of `tile` read from a ring stage that still holds `prev`'s
    stale[r, c] += y_last[rp, cp] - y_last[r, c]
    moved = want.clone()                                     # the tile's block stored at the position of its n-neighbour
    n_tile = tile % (N // bn)
    cn = _block(tile - n_tile + (n_tile + 1) % (N // bn), N, bn)[1]
    moved[r, cn] = want[r, c]
    skipped = want.clone()                                   # one wave's 64-row strip never stored
    skipped[r.start + 64:r.start + 128, c] = float("nan")
    return dict(stale=stale, moved=moved, skipped=skipped), (tile, prev)


@pytest.mark.parametrize("dt", DTS)
def test_the_bound_rejects_the_walk_failures_dense(dt):
    """The 128-wide walk case (22172, 384, 192): the reference rounded to the type is inside the bound; a stale ring stage, a
    misplaced block and a skipped wave are outside.  On identical rows (A[m] = A[m % 256]) the stale stage breaks the equality of
    the 256-row blocks: the tile follows, in its workgroup, a tile of ANOTHER n-tile, so the stale operands are other weights."""
    shape, epi, _ = K.WALK_DENSE[6]
    M, N, Kk = shape
    assert (shape, epi) == ((22172, 384, 192), "bias_rowbias")
    case = K.walk_dense_case(shape, epi, dt)
    want, slack = K.walk_want(case)
    T = K.DTYPES[dt]
    assert K.outside(want.to(T), want, slack, dt)[0] == 0
    y_last = case["a"][:, Kk - 64:].double() @ case["w"][:, Kk - 64:].double().t()
    models, (tile, prev) = _walk_failure_models(want, y_last, M, N, 128)
    assert tile % 3 != prev % 3
    for name, got in models.items():
        assert K.outside(got.to(T), want, slack, dt)[0] > 0, name
    same = K.same_rows_case(shape, dt)
    want, _ = K.gemm_want(same)
    good = want[:256].repeat(-(-M // 256), 1)[:M].contiguous()       # what identical arithmetic on identical rows stores
    assert K.same_rows_mismatch(good.to(T)) == 0
    y_last = same["a"][:, Kk - 64:].double() @ same["w"][:, Kk - 64:].double().t()
    stale = _walk_failure_models(good, y_last, M, N, 128)[0]["stale"]
    assert K.same_rows_mismatch(stale.to(T)) > 0
    ragged = good.clone()                                    # ... and the ragged last block is compared too
    ragged[-1, 5] += 1.0
    assert K.same_rows_mismatch(ragged.to(T)) == 1


@pytest.mark.parametrize("dt", DTS)
def test_the_bound_rejects_the_walk_failures_conv(dt):
    """The 320-wide conv walk case (64 -> 640, bias + row bias + residual; its last K-tile is tap (2, 2)), shrunk for the CPU to
    3 x 20 x 22 pixels on a mirror of 8 workgroups: 12 tiles, the ninth a whole tile behind tile 0, samples straddling tiles."""
    (_, _, _, Cin, Cout, stride, up), opts, pad_lo, _ = K.WALK_CONV[0]
    shape = (3, 20, 22, Cin, Cout, stride, up)
    case = K.conv_case(shape, opts, dt, pad_lo=pad_lo)
    want, slack = K.conv_want(case)
    M, N, Kk, _ = K.conv_dispatch_args(shape, opts, pad_lo)
    assert K.big_tiles(M, N, 320) == 8 + 4 and M % 256 != 0 and (20 * 22) % 256 != 0
    T = K.DTYPES[dt]
    assert K.outside(want.to(T), want, slack, dt)[0] == 0
    w_last = torch.zeros_like(case["w"])
    w_last[:, Kk - 64:] = case["w"][:, Kk - 64:]
    y_last, _ = K.conv3x3_ref(case["x"], w_last, stride=stride, up=up, pad_lo=pad_lo)
    models, (tile, prev) = _walk_failure_models(want.reshape(M, N), y_last.reshape(M, N), M, N, 320, num_cu=8)
    assert (tile, prev) == (8, 0)
    for name, got in models.items():
        assert K.outside(got.to(T), want, slack, dt)[0] > 0, name


def test_gn_partial_errors_sees_wrong_partials():
    """The comparison test_conv3x3_gn_partial and the GST walk case share: exact partials give ~0; a chunk's mean off by 1e-4 of
    its standard deviation, an M2 off by 0.1 % and a NaN are over its tolerances (2e-5, 2e-4)."""
    out = K.gen((2, 8, 16, 64), 750).to(torch.bfloat16)
    v = out.double().reshape(2, 2, 64, 32, 2).permute(0, 1, 3, 2, 4).reshape(2, 2, 32, 128)
    mean = v.mean(-1)
    part = torch.stack([mean, ((v - mean[..., None]) ** 2).sum(-1)], -1).float()
    e_mean, e_m2 = K.gn_partial_errors(part, out)
    assert e_mean < 1e-6 and e_m2 < 1e-6
    bad = part.clone()
    bad[1, 1, 7, 0] += 1e-4 * float(v[1, 1, 7].std())
    assert K.gn_partial_errors(bad, out)[0] > 2e-5
    bad = part.clone()
    bad[0, 1, 31, 1] *= 1.001
    assert K.gn_partial_errors(bad, out)[1] > 2e-4
    bad = part.clone()
    bad[0, 0, 0, 0] = float("nan")
    assert K.gn_partial_errors(bad, out)[0] == float("inf")
    swapped = part.flip(1)                                   # the chunks of a sample in the wrong order
    assert K.gn_partial_errors(swapped, out)[0] > 2e-5
