"""``idf_q_sample`` and ``idf_resize_planes`` on a real MI355X against their fp32 torch expressions evaluated on the CPU
(tests/hires_cases.py): BIT identity (``torch.equal``), the 16-B and the scalar paths, aliasing, offset views, clamped table entries,
argument errors before any launch, graph replay; the resize also within 20 u max|x| of ``F.interpolate`` on float64 input.

Every output lives in a NaN-filled buffer with at least 64 guard elements behind it (and in front of an offset view), which must
stay NaN.  Inputs are built once on the CPU and shared.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import hires_cases as hc

pytestmark = pytest.mark.gpu
GUARD = 64
NS = [64, 60, 1600]                                 # whole vectors in one block; whole vectors, no whole wave; more than one block
# (Hi, Wi, Ho, Wo)
RESIZE_SIZES = [(16, 16, 24, 24), (8, 12, 20, 17), (64, 64, 96, 96), (16, 16, 8, 8), (3, 3, 64, 64), (1, 1, 4, 4), (16, 16, 16, 16)]
PLANES = [1, 3, 8]
# The bound against F.interpolate on float64 input: a 4 + 4-term dot product in fp32 plus the weights' rounding, 10 u, times
# sum |wy wx| <= 1.375^2 = 1.89 (the A = -0.75 cubic's absolute weight sum, squared): 20 u max|x|.  Observed on the CPU: <= 3.5 u.
RESIZE_BOUND_U = 20.0


@functools.lru_cache(maxsize=None)
def _ops():
    from instancediffusion_amd.ops import HipOps
    return HipOps(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _coeffs():
    """(sqrt_ac, sqrt_1m_ac) of t = 1, 500, 999: the diffusion's float32 buffers."""
    from instancediffusion_amd.host.diffusion import LatentDiffusion
    d = LatentDiffusion(linear_start=0.00085, linear_end=0.012, timesteps=1000)
    return [(float(d.sqrt_alphas_cumprod[t]), float(d.sqrt_one_minus_alphas_cumprod[t])) for t in (1, 500, 999)]


@functools.lru_cache(maxsize=None)
def _pool(n):
    g = torch.Generator().manual_seed(300 + n)
    return torch.randn(n, generator=g) * 3.0, torch.randn(n, generator=g)


def _dev(t, offset=0):
    """A device copy of t; offset 1: a view one float into its allocation (4-B aligned only -> the scalar path)."""
    buf = torch.empty(t.numel() + offset, device="cuda", dtype=t.dtype)
    v = buf[offset:]
    v.copy_(t.reshape(-1))
    return v.view(t.shape)


def _guarded(shape, offset):
    n = int(np.prod(shape))
    buf = torch.full((offset + n + GUARD,), float("nan"), device="cuda", dtype=torch.float32)
    return buf, buf[offset:offset + n].view(shape)


def _guards_intact(buf, offset, n):
    return bool(torch.isnan(buf[:offset]).all()) and bool(torch.isnan(buf[offset + n:]).all()) and buf.numel() - offset - n >= GUARD


# ---- idf_q_sample -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fresh", "in_place", "offset1"])
def test_q_sample_is_bit_identical(mode):
    ops = _ops()
    offset = 1 if mode == "offset1" else 0
    for n in NS:
        x0, nz = _pool(n)
        for sa, s1 in _coeffs():
            want = hc.q_sample_expr(x0, nz, sa, s1)
            buf, out = _guarded((n,), offset)
            if mode == "in_place":                                          # out aliases x0
                out.copy_(x0)
                ops.q_sample(out, _dev(nz), sa, s1, out)
            else:
                ops.q_sample(_dev(x0, offset), _dev(nz, offset), sa, s1, out)
            assert torch.equal(out.cpu(), want), (n, sa)
            assert _guards_intact(buf, offset, n), (n, sa)


def test_q_sample_on_latents_is_the_diffusions_q_sample():
    from instancediffusion_amd.host.diffusion import LatentDiffusion
    d = LatentDiffusion(linear_start=0.00085, linear_end=0.012, timesteps=1000)
    x0, nz = hc.seeded((2, 4, 24, 24)), hc.seeded((2, 4, 24, 24), seed=hc.SEED + 1)
    out = _ops().q_sample(_dev(x0), _dev(nz), float(d.sqrt_alphas_cumprod[401]), float(d.sqrt_one_minus_alphas_cumprod[401]),
                          torch.empty(2, 4, 24, 24, device="cuda"))
    assert torch.equal(out.cpu(), d.q_sample(x0, torch.full((2,), 401, dtype=torch.long), nz))


# ---- idf_resize_planes --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _planes(planes, Hi, Wi):
    return hc.seeded((planes, Hi, Wi), seed=17 * planes + 100 * Hi + Wi)


@functools.lru_cache(maxsize=None)
def _tables(Hi, Wi, Ho, Wo, mode):
    from instancediffusion_amd.host.hires import resize_tables
    xi, xw = resize_tables(Wi, Wo, mode)
    yi, yw = resize_tables(Hi, Ho, mode)
    return xi, xw, yi, yw


def _resize(src, size, tables, offset=0):
    buf, out = _guarded(tuple(src.shape[:-2]) + tuple(size), offset)
    _ops().resize_planes(_dev(src), out, *(_dev(torch.from_numpy(np.ascontiguousarray(t))) for t in tables))
    return buf, out


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "dst_offset1"])
@pytest.mark.parametrize("mode", ["bicubic", "bilinear"])
@pytest.mark.parametrize("size", RESIZE_SIZES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_resize_planes_is_bit_identical_and_within_20u_of_float64(size, mode, offset):
    """16^2 -> 24^2 and 64^2 -> 96^2 (16-B stores), 8x12 -> 20x17 (Wo % 4 != 0: scalar stores, a tail), 16^2 -> 8^2 (a downscale, no
    antialias, as torch), 3^2 -> 64^2 (border taps clamped on both sides), 1x1 -> 4x4, the identity; ``dst_offset1``: a dst view one
    float into its allocation (scalar stores at every size)."""
    Hi, Wi, Ho, Wo = size
    for planes in PLANES:
        src = _planes(planes, Hi, Wi)
        want = hc.resize_expr(src, (Ho, Wo), mode)
        buf, out = _resize(src, (Ho, Wo), _tables(Hi, Wi, Ho, Wo, mode), offset)
        got = out.cpu()
        assert torch.equal(got, want), (planes, size, mode)
        assert _guards_intact(buf, offset, want.numel()), (planes, size, mode)
        err = float((got.double() - hc.interpolate64(src, (Ho, Wo), mode)).abs().max()) / (hc.U * float(src.abs().max()))
        assert err <= RESIZE_BOUND_U, (planes, size, mode, err)
        if (Hi, Wi) == (Ho, Wo):
            assert torch.equal(got, src)


@pytest.mark.parametrize("mode", ["bicubic", "bilinear"])
def test_resize_planes_on_a_4d_latent_batch(mode):
    src = hc.seeded((2, 4, 16, 16))
    buf, out = _resize(src, hc.HIRES_SIZE, _tables(16, 16, 24, 24, mode))
    assert tuple(out.shape) == (2, 4, 24, 24) and torch.equal(out.cpu(), hc.resize_expr(src, hc.HIRES_SIZE, mode))


@pytest.mark.parametrize("mode", ["bicubic", "bilinear"])
def test_out_of_range_table_entries_are_clamped(mode):
    """The launcher cannot read the device tables: whatever first tap they hold, every tap index is clamped to [0, n - 1] where it
    becomes an address -- the result is the one of the clamped taps (``apply_tables`` clamps idx + k in int64), and nothing behind dst
    is written."""
    Hi, Wi, Ho, Wo = 8, 12, 20, 17
    xi, xw, yi, yw = (t.copy() for t in _tables(Hi, Wi, Ho, Wo, mode))
    xi[0], xi[3], xi[5], xi[-1] = -7, Wi + 5, 2 ** 31 - 1, -2 ** 31
    yi[1], yi[2], yi[-1], yi[-2] = Hi, -100, 2 ** 31 - 2, -2 ** 31 + 1
    src = _planes(3, Hi, Wi)
    want = hc.apply_tables(src, xi, xw, yi, yw)
    buf, out = _resize(src, (Ho, Wo), (xi, xw, yi, yw))
    assert torch.equal(out.cpu(), want) and _guards_intact(buf, 0, want.numel())
    assert not torch.equal(want, hc.resize_expr(src, (Ho, Wo), mode))


def test_argument_errors_return_before_any_launch():
    """Every IDF_E_ARG / IDF_E_UNSUPPORTED case of include/idf.h, and the NaN-filled outputs are untouched."""
    from instancediffusion_amd import _lib
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: None if t is None else C.c_void_p(t if isinstance(t, int) else t.data_ptr())
    n = 256
    x0, nz = (_dev(t) for t in _pool(n))
    buf = torch.full((n + GUARD,), float("nan"), device="cuda", dtype=torch.float32)
    nan, inf = float("nan"), float("inf")

    def qs(x0=x0, nz=nz, sa=0.65, s1=0.76, out=buf, n=n):
        return lib.idf_q_sample(P(x0), P(nz), sa, s1, P(out), n, stream)
    bad = [qs(x0=None), qs(nz=None), qs(out=None), qs(n=0), qs(n=-4), qs(sa=nan), qs(sa=inf), qs(s1=nan), qs(s1=-inf)]
    assert bad == [-1] * len(bad), bad

    planes, Hi, Wi, Ho, Wo = 3, 8, 12, 20, 17
    both = torch.full((planes * (Hi * Wi + Ho * Wo) + GUARD,), float("nan"), device="cuda", dtype=torch.float32)
    src, dst = both[:planes * Hi * Wi], both[planes * Hi * Wi:]
    tabs = [_dev(torch.from_numpy(t)) for t in _tables(Hi, Wi, Ho, Wo, "bicubic")]

    def rs(src=src, dst=dst, xi=tabs[0], xw=tabs[1], yi=tabs[2], yw=tabs[3], taps=4, planes=planes, Hi=Hi, Wi=Wi, Ho=Ho, Wo=Wo):
        return lib.idf_resize_planes(P(src), P(dst), P(xi), P(xw), P(yi), P(yw), taps, planes, Hi, Wi, Ho, Wo, stream)
    bad = [rs(src=None), rs(dst=None), rs(xi=None), rs(xw=None), rs(yi=None), rs(yw=None), rs(taps=0), rs(taps=3), rs(taps=5),
           rs(planes=0), rs(Hi=0), rs(Wi=0), rs(Ho=-1), rs(Wo=0),
           rs(dst=src), rs(dst=both[planes * Hi * Wi - 1:]), rs(src=both[1:], dst=both)]             # dst overlaps src
    assert bad == [-1] * len(bad), bad
    # planes Ho Wo = 2^31: refused by size (a dst address far from src, never touched: nothing is launched)
    assert rs(dst=1 << 45, planes=1 << 19, Hi=1, Wi=1, Ho=64, Wo=64) == _lib.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all()) and bool(torch.isnan(both).all())
    src.copy_(_planes(planes, Hi, Wi).reshape(-1))
    assert qs() == 0 and rs() == 0                                          # the same calls with nothing wrong go through
    torch.cuda.synchronize()
    assert not bool(torch.isnan(buf[:n]).any()) and bool(torch.isnan(buf[n:]).all())
    assert not bool(torch.isnan(dst[:planes * Ho * Wo]).any()) and bool(torch.isnan(dst[planes * Ho * Wo:]).all())


def test_both_launches_replay_from_a_captured_graph():
    """Upscale, then q_sample on the result: one capture, two replays."""
    from instancediffusion_amd.engine import capture_graph
    ops = _ops()
    src = _dev(hc.seeded((2, 4, 16, 16)))
    nz = _dev(hc.seeded((2, 4, 24, 24), seed=hc.SEED + 1))
    tabs = [_dev(torch.from_numpy(t)) for t in _tables(16, 16, 24, 24, "bicubic")]
    sa, s1 = _coeffs()[1]

    def step(up, out):
        ops.resize_planes(src, up, *tabs)
        ops.q_sample(up, nz, sa, s1, out)
    bufs = [_guarded((2, 4, 24, 24), 0) for _ in range(4)]
    step(bufs[0][1], bufs[1][1])                                            # eager (also the warm-up outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with capture_graph(graph):
        step(bufs[2][1], bufs[3][1])
    for _ in range(2):
        bufs[2][1].fill_(float("nan"))
        bufs[3][1].fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bufs[2][1], bufs[0][1]) and torch.equal(bufs[3][1], bufs[1][1])
        assert not bool(torch.isnan(bufs[3][1]).any())
    want = hc.q_sample_expr(hc.resize_expr(src.cpu(), (24, 24), "bicubic"), nz.cpu(), sa, s1)
    assert torch.equal(bufs[3][1].cpu(), want)
    assert all(_guards_intact(b, 0, v.numel()) for b, v in bufs)
