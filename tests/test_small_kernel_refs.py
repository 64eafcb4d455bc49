"""tests/small_kernel_cases.py proved on the CPU, before a GPU is involved: its fp64 references agree with the project's fp32 ones,
``within_one_rounding`` passes a correctly rounded result on every case the GPU tests run, and it fails the two results the GPU
tests exist to catch -- an fp16 output that went through bf16 once, and a LayerNorm whose variance is E[x^2] - mu^2 in fp32."""
import pytest
import torch

from oracle import ref_cpu
from tests import small_kernel_cases as K
from tests.emul_ops import EmulOps


def _agree(want64, ref32, what):
    err = K.relmax(ref32, want64)
    assert err < 1e-5, (what, err)


def test_references_agree_with_the_fp32_ones():
    ref = EmulOps(torch.float32)
    inp = K.gn_inputs((2, 64, 128), "bf16")
    for silu in (False, True):
        got = ref.groupnorm(inp["x"].float(), torch.empty(2, 64, 128), inp["gamma"], inp["beta"], K.GN_EPS, silu)
        _agree(K.gn_want(inp, silu), got, "groupnorm")
    inp = K.ln_inputs((37, 320), "bf16")
    _agree(K.ln_want(inp), ref.layernorm(inp["x"].float(), torch.empty(37, 320), inp["gamma"], inp["beta"], K.LN_EPS), "layernorm")
    st = ref.row_stats(inp["x"].float(), torch.empty(37, 2), K.LN_EPS)
    mu, rstd = K.row_stats_ref(inp["x"], K.LN_EPS)
    _agree(mu, st[:, 0], "row mean")
    _agree(rstd, st[:, 1], "row rstd")
    inp = K.lnp_inputs((2, 4, 6, 96), "bf16")
    _agree(K.lnp_want(inp), ref.layernorm_patch2(inp["x"].float(), torch.zeros(12, 384), inp["gamma"], inp["beta"], K.LN_EPS),
           "layernorm_patch2")
    inp = K.dw_inputs((2, 9, 11, 24), "bf16")
    _agree(K.dw_want(inp), ref.dwconv7x7(inp["x"].float(), inp["w"], inp["bias"], torch.empty(2, 9, 11, 24)), "dwconv7x7")
    inp = K.seg_inputs((2, 30, 8, 48))
    _agree(K.seg_want(inp), ref.seg_in_conv(inp["segs"], inp["w"], inp["bias"], torch.zeros(8, 48)), "seg_in_conv")
    inp = K.conv_in_inputs((2, 4, 6, 9, 32))
    _agree(K.conv_in_want(inp), ref.conv_in(inp["x"], inp["w"], inp["bias"], torch.empty(2, 6, 9, 32)), "conv_in")
    inp = K.uni_inputs((5, 768, 40))
    _agree(K.uni_want(inp), ref.unifusion_embed(inp["text"], inp["loc"], inp["tmask"], inp["lmask"], inp["null_text"],
                                                inp["null_loc"], inp["freqs"], torch.empty(5, 768 + 32 * 40)), "unifusion_embed")
    # ScaleU against the reference algorithm (FFT, fp32) and the timestep embedding against the oracle's
    inp = K.scaleu_inputs((2, 8, 12, 16, 24), "bf16")
    want = K.scaleu_want(inp)
    filt = ref_cpu.fourier_filter(inp["skip"].float().permute(0, 3, 1, 2), 1, inp["sm1"] + 1).permute(0, 2, 3, 1)
    _agree(want[..., 16:], filt, "fourier_filter")
    _agree(want[..., :16], inp["h"].float() * inp["hscale"], "h * hscale")
    t = torch.tensor([1.0, 37.0, 2.5])                       # small angles: the fp32 cos / sin of the oracle are good to 1e-7
    _agree(K.timestep_embedding_ref(t, 320), ref_cpu.timestep_embedding(t, 320), "timestep_embedding")


def test_patch_and_stem_layouts_are_the_documented_ones():
    """One-hot probes through the two references that permute: a pixel lands in the row and column the kernels document."""
    x = torch.zeros(1, 4, 6, 8)
    g, b = torch.ones(8), torch.zeros(8)
    x[0, 3, 4] = torch.arange(8.0)                            # the only row with variance
    out = K.layernorm_patch2_ref(x, g, b, 1e-6)
    row, col = (3 // 2) * 3 + 4 // 2, ((3 & 1) * 2 + (4 & 1)) * 8
    assert out[row, col:col + 8].abs().max() > 1 and out.abs().sum() == out[row, col:col + 8].abs().sum()
    segs = torch.zeros(1, 1, 8, 8)
    segs[0, 0, 5, 2] = 1.0
    w = torch.zeros(3, 1, 3, 3)
    w[1, 0, 1, 1] = 1.0                                       # channel 1 = identity
    out = K.seg_in_conv_ref(segs, w, torch.zeros(3))
    assert out[(5 // 4) * 2 + 2 // 4, 1 * 16 + (5 & 3) * 4 + (2 & 3)] == 1.0 and out.sum() == 1.0


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_a_correctly_rounded_result_is_inside_the_bound(dt):
    n = 0
    for what, want in K.all_wants(dt):
        assert bool(torch.isfinite(want).all()), what
        assert K.within_one_rounding(want.to(K.DTYPES[dt]), want, dt) == 0.0, what
        assert K.relmax(want.to(K.DTYPES[dt]), want) < K.U[dt], what
        if want.numel() >= K.RMS_MIN_ELEMS:
            assert K.rel_rms(want.to(K.DTYPES[dt]), want) < K.RMS_BAR[dt], what
        n += 1
    assert n == 2 * len(K.GN_CASES) + 2 + len(K.LN_CASES) + 1 + len(K.LNP_CASES) + len(K.DW_CASES) + len(K.SEG_CASES) \
        + len(K.SCALEU_CASES) + len(K.TEMB_CASES) + len(K.UNI_CASES) + len(K.CONV_IN_CASES)


def test_one_bf16_intermediate_in_an_fp16_kernel_is_outside_the_bound():
    """The failure the GPU tests exist to catch: an fp16 instantiation that rounds through bf16 once."""
    n = 0
    for what, want in K.all_wants("fp16"):
        if want.numel() <= 64:
            continue
        assert K.within_one_rounding(want.to(torch.bfloat16).to(torch.float16), want, "fp16") > 0.0, what
        n += 1
    assert n >= 50


def test_a_nan_is_outside_the_bound():
    want = K.gen((8, 8), 1).double()
    got = want.clone()
    got[3, 3] = float("nan")
    assert K.within_one_rounding(got, want, "bf16") == 1 / 64


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_single_pass_variance_on_large_mean_rows_is_outside_the_bound(dt):
    """The bound is not trivially tight: LayerNorm with var = E[x^2] - mu^2 in fp32 on rows of mean 256, std 1.63 fails it, while
    the same arithmetic in two passes (what ln_kernel does) passes."""
    inp = K.ln_inputs(K.LN_LARGE_MEAN, dt, large=True)
    want = K.ln_want(inp)
    x = inp["x"].float()
    C = x.shape[-1]
    mu = x.sum(-1, keepdim=True) / C
    one_pass = (x * x).sum(-1, keepdim=True) / C - mu * mu
    bad = (x - mu) * torch.rsqrt(one_pass + K.LN_EPS) * inp["gamma"] + inp["beta"]
    assert K.within_one_rounding(bad.to(K.DTYPES[dt]), want, dt) > 0.0
    two_pass = ((x - mu) ** 2).sum(-1, keepdim=True) / C
    good = (x - mu) * torch.rsqrt(two_pass + K.LN_EPS) * inp["gamma"] + inp["beta"]
    assert K.within_one_rounding(good.to(K.DTYPES[dt]), want, dt) == 0.0


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_cast16_inputs_hold_every_special_value(dt):
    x = K.cast16_input(257, dt)
    y = x.to(K.DTYPES[dt])
    assert bool(torch.isnan(y).any()) and bool(torch.isinf(y[torch.isfinite(x)]).any())      # nan, and a finite value -> inf
    assert bool((y == 0).any()) and bool(torch.signbit(y[y == 0]).any())                     # -0
    fin = y[torch.isfinite(y)].float()
    assert float(fin.max()) == float(torch.finfo(K.DTYPES[dt]).max)
    if dt == "fp16":
        tiny = float(torch.finfo(torch.float16).tiny)
        assert bool(((fin > 0) & (fin < tiny)).any()) and bool((fin == tiny).any())          # subnormals, the smallest normal
        assert bool(torch.isinf(torch.tensor([1e5, -1e5]).to(torch.float16)).all())
    for n in (1, 7, 257, 4099):
        assert K.cast16_input(n, dt).numel() == n
