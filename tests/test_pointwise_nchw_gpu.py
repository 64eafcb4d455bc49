"""``idf_pointwise_nchw`` (the fp32 entry of VAE decode: 1 / scale_factor and post_quant_conv) on a real MI355X, per element against
float64: channel counts from 1 to the limit of 16 inputs and past 16 outputs, pixel counts below, at and past the 256-thread block,
with and without bias, with and without the input scale, input and output 16-B aligned or one float into their allocation.

The bound per element is (Cin + 2) 2^-24 (|bias| + sum_ci |w| |in_scale x|): one rounding of the scaled input and Cin FMAs.  The output
lives in a NaN-filled buffer with 64 guard elements behind it (and one in front of an offset view), which must stay NaN."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GUARD = 64
NAN = float("nan")
CHANNELS = [(1, 1), (4, 4), (3, 6), (16, 8), (4, 17)]
PIXELS = [(3, 35), (1, 255), (2, 257), (3, 960)]                   # (B, HW)
SCALES = [1.0 / 0.18215, 1.0]


@functools.lru_cache(maxsize=None)
def _ops():
    from instancediffusion_amd.ops import HipOps
    return HipOps(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _case(cin, cout, B, HW):
    """x, w, bias on the CPU (shared: left unchanged)."""
    g = torch.Generator().manual_seed(9000 + 100 * cin + cout + HW)
    return torch.randn(B, cin, HW, generator=g) * 2.0, torch.randn(cout, cin, generator=g), torch.randn(cout, generator=g)


def _ref64(x, w, bias, in_scale):
    """-> (the float64 value, the sum of magnitudes the bound scales with); in_scale is the fp32 value the kernel receives."""
    s = float(np.float32(in_scale))
    xs = x.double() * s
    ref = torch.einsum("oc,bcp->bop", w.double(), xs)
    mag = torch.einsum("oc,bcp->bop", w.double().abs(), xs.abs())
    if bias is not None:
        ref = ref + bias.double().view(1, -1, 1)
        mag = mag + bias.double().abs().view(1, -1, 1)
    return ref, mag


def _dev(t, offset):
    buf = torch.empty(t.numel() + offset, device="cuda", dtype=torch.float32)
    v = buf[offset:]
    v.copy_(t.reshape(-1))
    assert (v.data_ptr() % 16 != 0) == bool(offset)
    return v.view(t.shape)


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("cin,cout", CHANNELS)
def test_pointwise_nchw_is_inside_the_rounding_bound(cin, cout, offset):
    ops = _ops()
    for B, HW in PIXELS:
        x, w, bias = _case(cin, cout, B, HW)
        xd, wd, bd = _dev(x, offset), w.cuda(), bias.cuda()
        n = B * cout * HW
        for with_bias in (True, False):
            for in_scale in SCALES:
                buf = torch.full((offset + n + GUARD,), NAN, device="cuda", dtype=torch.float32)
                out = buf[offset:offset + n].view(B, cout, HW)
                assert ops.pointwise_nchw(xd, wd, bd if with_bias else None, out, in_scale) is out
                got = out.cpu()
                ref, mag = _ref64(x, w, bias if with_bias else None, in_scale)
                err, bound = (got.double() - ref).abs(), (cin + 2) * 2.0 ** -24 * mag
                assert not torch.isnan(got).any() and bool((err <= bound).all()), \
                    ((B, HW), with_bias, in_scale, int((err > bound).sum()), float((err / bound.clamp_min(1e-300)).max()))
                assert bool(torch.isnan(buf[:offset]).all()) and bool(torch.isnan(buf[offset + n:]).all()), ((B, HW), with_bias, in_scale)


def test_argument_errors_return_before_any_launch():
    """Cin above 16, a null pointer or a non-positive size: IDF_E_ARG, the NaN-filled output untouched; the same call with nothing
    wrong returns 0 and writes exactly the output."""
    from instancediffusion_amd import _lib
    lib = _lib.load()
    B, cin, cout, HW = 2, 4, 4, 35
    x, w, bias = _case(cin, cout, B, HW)
    xd, wd, bd = x.cuda(), w.cuda(), bias.cuda()
    x17, w17 = torch.randn(B, 17, HW).cuda(), torch.randn(cout, 17).cuda()
    n = B * cout * HW
    buf = torch.full((n + GUARD,), NAN, device="cuda", dtype=torch.float32)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def call(x=xd, w=wd, bias=bd, out=buf, B=B, cin=cin, cout=cout, HW=HW):
        return lib.idf_pointwise_nchw(P(x), P(w), P(bias), P(out), B, cin, cout, HW, 1.0, stream)
    bad = [call(x=x17, w=w17, cin=17), call(x=None), call(w=None), call(out=None), call(B=0), call(B=-1), call(cin=0), call(cin=-4),
           call(cout=0), call(cout=-1), call(HW=0), call(HW=-35)]
    assert bad == [-1] * len(bad), bad
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())
    assert call() == 0 and call(bias=None) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(buf[:n]).any()) and bool(torch.isnan(buf[n:]).all())
