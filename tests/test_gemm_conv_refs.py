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
