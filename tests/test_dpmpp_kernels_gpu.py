"""``idf_dpmpp_update`` on a real MI355X against the fp32 torch expression evaluated on the CPU (``dpmpp_cases.dpmpp_update_expr``): BIT
identity (``torch.equal``) of both outputs, 16-B and scalar paths, order 1 and 2, guided and unguided, aliasing, argument errors,
graph replay.

Every output lives in a NaN-filled buffer with at least 64 guard elements behind it (and in front of an offset view), which must
stay NaN.  Inputs and the expected values are built once on the CPU and shared.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import dpmpp_cases as dc

pytestmark = pytest.mark.gpu
GUARD = 64
NS = [4 * 16, 4 * 15, 4 * 400]        # one partial block of vectors, fewer than a wave, more than one block (1600 = 6.25 x 256)
STEPS = [0, 2, 4]                     # loop positions of the S = 5 schedule: first, middle, last step


@functools.lru_cache(maxsize=None)
def _ops():
    from instancediffusion_amd.ops import HipOps
    return HipOps(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _coeffs(i, order):
    """(sqrt_at, sqrt_1m_at, c_x, c_0, c_1) of loop step i of the S = 5 uniform schedule, from the host code under test's caller side:
    the sampler's own schedule arrays and ``dpmpp_coeffs``."""
    from instancediffusion_amd.host.samplers import dpmpp_coeffs
    steps, a, a_prev, sqrt_a, s1m = dc.schedule(dc.S)
    index = dc.S - i - 1
    a_last = a[index + 1] if (order == 2 and i > 0) else None
    if order == 2 and i == 0:
        a_last = np.float32(0.5 * a[index])                       # the first step has no history in a run; the kernel takes any
    c = dpmpp_coeffs(a[index], a_prev[index], a_last)
    return tuple(float(v) for v in (sqrt_a[index], s1m[index]) + c)


@functools.lru_cache(maxsize=None)
def _pool(n):
    """x, eps_cond, eps_uncond, x0_last of n elements (CPU fp32, left unchanged)."""
    g = torch.Generator().manual_seed(300 + n)
    return tuple(torch.randn(n, generator=g) * s for s in (3.0, 1.0, 1.0, 2.0))


@functools.lru_cache(maxsize=None)
def _want(n, i, order, guided):
    x, ec, eu, last = _pool(n)
    return dc.dpmpp_update_expr(x, ec, eu if guided else None, dc.GUIDANCE, *_coeffs(i, order), last if order == 2 else None)


def _dev(t, offset):
    """A device copy of t; offset 1: a view one float into its allocation (4-B aligned only -> the scalar path)."""
    if t is None:
        return None
    buf = torch.empty(t.numel() + offset, device="cuda", dtype=torch.float32)
    v = buf[offset:]
    v.copy_(t.reshape(-1))
    return v.view(t.shape)


def _guarded(n, offset):
    buf = torch.full((offset + n + GUARD,), float("nan"), device="cuda", dtype=torch.float32)
    return buf, buf[offset:offset + n]


def _guards_intact(buf, offset, n):
    return bool(torch.isnan(buf[:offset]).all()) and bool(torch.isnan(buf[offset + n:]).all()) and buf.numel() - offset - n >= GUARD


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("order", [1, 2], ids=["order1", "order2"])
@pytest.mark.parametrize("guided", [True, False], ids=["guided", "unguided"])
def test_dpmpp_update_is_bit_identical(guided, order, offset):
    ops = _ops()
    for n in NS:
        x, ec, eu, last = _pool(n)
        for i in STEPS:
            want, want_p = _want(n, i, order, guided)
            buf, out = _guarded(n, offset)
            pbuf, p0 = _guarded(n, offset)
            got = ops.dpmpp_update(_dev(x, offset), _dev(ec, offset), _dev(eu, offset) if guided else None, dc.GUIDANCE, *_coeffs(i, order),
                                   _dev(last, offset) if order == 2 else None, out, p0)
            assert got is out
            assert torch.equal(out.cpu(), want) and torch.equal(p0.cpu(), want_p), (n, i)
            assert _guards_intact(buf, offset, n) and _guards_intact(pbuf, offset, n), (n, i)


def test_one_misaligned_pointer_takes_the_scalar_path_and_order_one_ignores_c1():
    """Only x0_last sits one float into its allocation: the launch must fall back to scalar accesses for all (a 16-B load there would
    be misaligned).  And with x0_last NULL c_1 is not read: any value, NaN included, gives the order-1 result."""
    ops = _ops()
    n = NS[2]
    x, ec, eu, last = _pool(n)
    want, want_p = _want(n, 2, 2, True)
    buf, out = _guarded(n, 0)
    pbuf, p0 = _guarded(n, 0)
    ops.dpmpp_update(_dev(x, 0), _dev(ec, 0), _dev(eu, 0), dc.GUIDANCE, *_coeffs(2, 2), _dev(last, 1), out, p0)
    assert torch.equal(out.cpu(), want) and torch.equal(p0.cpu(), want_p) and _guards_intact(buf, 0, n) and _guards_intact(pbuf, 0, n)
    want, want_p = _want(n, 2, 1, True)
    c = _coeffs(2, 1)
    buf, out = _guarded(n, 0)
    pbuf, p0 = _guarded(n, 0)
    ops.dpmpp_update(_dev(x, 0), _dev(ec, 0), _dev(eu, 0), dc.GUIDANCE, *c[:4], float("nan"), None, out, p0)
    assert torch.equal(out.cpu(), want) and torch.equal(p0.cpu(), want_p)


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
def test_outputs_may_alias_their_inputs(offset):
    """x_prev aliasing x and x0_out aliasing x0_last, both at once."""
    ops = _ops()
    for n in NS:
        x, ec, eu, last = _pool(n)
        want, want_p = _want(n, 2, 2, True)
        buf, xio = _guarded(n, offset)
        pbuf, pio = _guarded(n, offset)
        xio.copy_(x)
        pio.copy_(last)
        ops.dpmpp_update(xio, _dev(ec, offset), _dev(eu, offset), dc.GUIDANCE, *_coeffs(2, 2), pio, xio, pio)
        assert torch.equal(xio.cpu(), want) and torch.equal(pio.cpu(), want_p), n
        assert _guards_intact(buf, offset, n) and _guards_intact(pbuf, offset, n), n


def test_argument_errors_return_before_any_launch():
    """Every IDF_E_ARG case of include/idf.h: -1, and the NaN-filled outputs are untouched."""
    from instancediffusion_amd import _lib
    lib = _lib.load()
    n = 256
    x, ec, eu, last = (_dev(t, 0) for t in _pool(n))
    buf = torch.full((n + GUARD,), float("nan"), device="cuda", dtype=torch.float32)
    pbuf = torch.full((n + GUARD,), float("nan"), device="cuda", dtype=torch.float32)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    sa, s1m, c_x, c_0, c_1 = _coeffs(2, 2)
    nan, inf = float("nan"), float("inf")

    def upd(x=x, ec=ec, eu=eu, sa=sa, s1m=s1m, c_x=c_x, c_0=c_0, c_1=c_1, last=last, out=buf, p0=pbuf, n=n):
        return lib.idf_dpmpp_update(P(x), P(ec), P(eu), 7.5, sa, s1m, c_x, c_0, c_1, P(last), P(out), P(p0), n, stream)
    bad = [upd(x=None), upd(ec=None), upd(out=None), upd(p0=None), upd(n=0), upd(n=-4), upd(sa=0.0), upd(sa=-0.1), upd(sa=nan), upd(sa=inf),
           upd(s1m=nan), upd(c_x=nan), upd(c_x=inf), upd(c_0=nan), upd(c_0=-inf), upd(c_1=nan), upd(c_1=inf), upd(c_x=nan, last=None)]
    assert bad == [-1] * len(bad), bad
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all()) and bool(torch.isnan(pbuf).all())
    assert upd() == 0 and upd(last=None, c_1=nan) == 0 and upd(eu=None) == 0   # the same call with nothing wrong goes through
    torch.cuda.synchronize()
    for b in (buf, pbuf):
        assert not bool(torch.isnan(b[:n]).any()) and bool(torch.isnan(b[n:]).all())


def test_the_launch_replays_from_a_captured_graph():
    """One capture of two chained steps (order 1, then order 2 on its history), two replays."""
    from instancediffusion_amd.engine import capture_graph
    ops = _ops()
    n = NS[2]
    x, ec, eu, _ = (_dev(v, 0) for v in _pool(n))

    def steps(mid, hist, out, hist2):
        ops.dpmpp_update(x, ec, eu, dc.GUIDANCE, *_coeffs(0, 1)[:4], 0.0, None, mid, hist)
        ops.dpmpp_update(mid, ec, eu, dc.GUIDANCE, *_coeffs(1, 2), hist, out, hist2)
    eager = [_guarded(n, 0) for _ in range(4)]
    steps(*[v for _, v in eager])                                   # eager (also the warm-up outside the capture)
    torch.cuda.synchronize()
    xc, ecc, euc, _ = _pool(n)
    m, h = dc.dpmpp_update_expr(xc, ecc, euc, dc.GUIDANCE, *_coeffs(0, 1), None)
    want, want_h = dc.dpmpp_update_expr(m, ecc, euc, dc.GUIDANCE, *_coeffs(1, 2), h)
    assert torch.equal(eager[2][1].cpu(), want) and torch.equal(eager[3][1].cpu(), want_h)
    bufs = [_guarded(n, 0) for _ in range(4)]
    graph = torch.cuda.CUDAGraph()
    with capture_graph(graph):
        steps(*[v for _, v in bufs])
    for _ in range(2):
        for b, _v in bufs:
            b.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(bufs[k][1], eager[k][1]) for k in range(4))
        assert all(_guards_intact(b, 0, n) for b, _v in bufs)
