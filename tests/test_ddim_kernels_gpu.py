"""``idf_ddim_update`` and ``idf_q_sample_blend`` on a real MI355X against the reference's fp32 torch expressions evaluated on the CPU
(tests/ddim_cases.py): BIT identity (``torch.equal``), scalar and 16-B paths, aliasing, offset views, argument errors, graph replay.

Every output lives in a NaN-filled buffer with at least 64 guard elements behind it (and in front of an offset view), which must
stay NaN.  Inputs are built once on the CPU and shared.
"""
import ctypes as C
import functools

import pytest
import torch

from tests import ddim_cases

pytestmark = pytest.mark.gpu
GUARD = 64
NS = [1, 3, 255, 256, 257, 2048, 32768]
SHAPES = [(1, 4, 1, 1), (2, 4, 3, 5), (3, 4, 16, 16), (2, 4, 64, 64)]
S1M = [float(torch.sqrt(1.0 - torch.tensor(t[0], dtype=torch.float32))) for t in ddim_cases.TRIPLES]


@functools.lru_cache(maxsize=None)
def _ops():
    from instancediffusion_amd.ops import HipOps
    return HipOps(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _pool(n):
    """x, eps_cond, eps_uncond, noise of n elements (CPU fp32, left unchanged)."""
    g = torch.Generator().manual_seed(100 + n)
    return tuple(torch.randn(n, generator=g) * s for s in (3.0, 1.0, 1.0, 1.0))


def _dev(t, offset):
    """A device copy of t; offset 1: a view one float into its allocation (4-B aligned only -> the scalar path)."""
    if t is None:
        return None
    buf = torch.empty(t.numel() + offset, device="cuda", dtype=torch.float32)
    v = buf[offset:]
    v.copy_(t.reshape(-1))
    return v.view(t.shape)


def _guarded(shape, offset):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((offset + n + GUARD,), float("nan"), device="cuda", dtype=torch.float32)
    return buf, buf[offset:offset + n].view(shape)


def _guards_intact(buf, offset, n):
    return bool(torch.isnan(buf[:offset]).all()) and bool(torch.isnan(buf[offset + n:]).all()) and buf.numel() - offset - n >= GUARD


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("want_p0", [False, True], ids=["x_prev", "x_prev+pred_x0"])
@pytest.mark.parametrize("noisy", [False, True], ids=["sigma0", "sigma>0"])
@pytest.mark.parametrize("guided", [True, False], ids=["guided", "unguided"])
def test_ddim_update_is_bit_identical(guided, noisy, want_p0, offset):
    ops = _ops()
    for n in NS:
        x, ec, eu, nz = _pool(n)
        for (a_t, a_prev, sigma), s1m in zip(ddim_cases.TRIPLES, S1M):
            sig = sigma if noisy else 0.0
            want, want_p = ddim_cases.ddim_update_expr(x, ec, eu if guided else None, ddim_cases.GUIDANCE, a_t, a_prev, sig, s1m,
                                                       nz if noisy else None)
            buf, out = _guarded((n,), offset)
            pbuf, p0 = _guarded((n,), offset) if want_p0 else (None, None)
            ops.ddim_update(_dev(x, offset), _dev(ec, offset), _dev(eu, offset) if guided else None, ddim_cases.GUIDANCE, a_t, a_prev,
                            sig, s1m, _dev(nz, offset) if noisy else None, out, pred_x0=p0)
            assert torch.equal(out.cpu(), want), (n, a_t)
            assert _guards_intact(buf, offset, n), (n, a_t)
            if want_p0:
                assert torch.equal(p0.cpu(), want_p) and _guards_intact(pbuf, offset, n), (n, a_t)


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
def test_ddim_update_in_place(offset):
    ops = _ops()
    a_t, a_prev, sigma = ddim_cases.TRIPLES[1]
    for n in NS:
        x, ec, eu, nz = _pool(n)
        want, _ = ddim_cases.ddim_update_expr(x, ec, eu, ddim_cases.GUIDANCE, a_t, a_prev, sigma, S1M[1], nz)
        buf, xio = _guarded((n,), offset)
        xio.copy_(x)
        ops.ddim_update(xio, _dev(ec, offset), _dev(eu, offset), ddim_cases.GUIDANCE, a_t, a_prev, sigma, S1M[1], _dev(nz, offset), xio)
        assert torch.equal(xio.cpu(), want) and _guards_intact(buf, offset, n), n


@functools.lru_cache(maxsize=None)
def _blend_pool(shape, mask_c, soft):
    B, Cc, H, W = shape
    g = torch.Generator().manual_seed(7 + B * H * W + mask_c)
    x0, nz, img = (torch.randn(shape, generator=g) for _ in range(3))
    mask = (torch.rand(B, mask_c, H, W, generator=g) > 0.5).float()
    if soft:
        mask = torch.where(torch.rand(B, mask_c, H, W, generator=g) > 0.5, mask, torch.full_like(mask, 0.25))
    return x0, nz, mask, img


@pytest.mark.parametrize("mode", ["fresh", "in_place", "offset1"])
@pytest.mark.parametrize("soft", [False, True], ids=["mask01", "mask_soft"])
@pytest.mark.parametrize("per_channel", [False, True], ids=["mask_B1HW", "mask_BCHW"])
@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
def test_q_sample_blend_is_bit_identical(shape, per_channel, soft, mode):
    ops = _ops()
    x0, nz, mask, img = _blend_pool(shape, shape[1] if per_channel else 1, soft)
    sa, s1 = 0.6503041982650757, 0.7596831917762756               # sqrt(ac), sqrt(1 - ac) of one timestep, fp32 values
    want = ddim_cases.q_sample_blend_expr(x0, nz, mask, img, sa, s1)
    offset = 1 if mode == "offset1" else 0
    n = want.numel()
    buf, out = _guarded(shape, offset)
    if mode == "in_place":
        out.copy_(img)
        ops.q_sample_blend(_dev(x0, 0), _dev(nz, 0), _dev(mask, 0), out, sa, s1, out)
    else:
        ops.q_sample_blend(_dev(x0, offset), _dev(nz, offset), _dev(mask, offset), _dev(img, offset), sa, s1, out)
    assert torch.equal(out.cpu(), want)
    assert _guards_intact(buf, offset, n)
    if not soft and not per_channel:                              # a {0, 1} mask selects: kept pixels are q_sample, the others img
        keep = mask.expand(shape) > 0
        assert torch.equal(out.cpu()[~keep], img[~keep])


def test_argument_errors_return_before_any_launch():
    """Every IDF_E_ARG case of include/idf.h: -1, and the NaN-filled output is untouched."""
    from instancediffusion_amd import _lib
    lib = _lib.load()
    n = 256
    x, ec, eu, nz = (_dev(t, 0) for t in _pool(n))
    buf = torch.full((n + GUARD,), float("nan"), device="cuda", dtype=torch.float32)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    a_t, a_prev, sigma = ddim_cases.TRIPLES[1]

    def upd(x=x, ec=ec, eu=eu, a_t=a_t, a_prev=a_prev, sigma=sigma, nz=nz, out=buf, n=n):
        return lib.idf_ddim_update(P(x), P(ec), P(eu), 7.5, a_t, a_prev, sigma, S1M[1], P(nz), P(out), None, n, stream)
    bad = [upd(x=None), upd(ec=None), upd(out=None), upd(n=0), upd(n=-4), upd(a_t=0.0), upd(a_t=-0.1), upd(a_prev=-0.1), upd(sigma=-0.1),
           upd(a_prev=0.9, sigma=0.5),                            # (1 - a_prev) - sigma^2 < 0
           upd(nz=None),                                          # sigma != 0 without noise
           upd(a_t=float("nan"))]
    assert bad == [-1] * len(bad), bad
    B, Cc, H, W = 2, 4, 4, 8
    t = [_dev(v, 0) for v in _blend_pool((B, Cc, H, W), 1, False)]

    def blend(x0=t[0], nz=t[1], mask=t[2], img=t[3], out=buf, B=B, Cc=Cc, HW=H * W, mc=1):
        return lib.idf_q_sample_blend(P(x0), P(nz), P(mask), P(img), 0.6, 0.8, P(out), B, Cc, HW, mc, stream)
    bad = [blend(x0=None), blend(nz=None), blend(mask=None), blend(img=None), blend(out=None), blend(B=0), blend(Cc=0), blend(HW=0),
           blend(mc=0), blend(mc=2), blend(mc=3)]
    assert bad == [-1] * len(bad), bad
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())
    assert upd() == 0 and blend(mc=1) == 0                        # the same calls with nothing wrong go through
    torch.cuda.synchronize()
    assert not bool(torch.isnan(buf[:n]).any()) and bool(torch.isnan(buf[n:]).all())


def test_both_launches_replay_from_a_captured_graph():
    from instancediffusion_amd.engine import capture_graph
    ops = _ops()
    shape = (2, 4, 16, 16)
    x0, nz, mask, img = (_dev(v, 0) for v in _blend_pool(shape, 1, False))
    _, ec, eu, nz2 = (_dev(v, 0).view(shape) for v in _pool(2 * 4 * 16 * 16))
    a_t, a_prev, sigma = ddim_cases.TRIPLES[1]

    def step(blended, out):
        ops.q_sample_blend(x0, nz, mask, img, 0.6503041982650757, 0.7596831917762756, blended)
        ops.ddim_update(blended, ec, eu, ddim_cases.GUIDANCE, a_t, a_prev, sigma, S1M[1], nz2, out)
    bufs = [_guarded(shape, 0) for _ in range(4)]
    step(bufs[0][1], bufs[1][1])                                  # eager (also the warm-up outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with capture_graph(graph):
        step(bufs[2][1], bufs[3][1])
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bufs[2][1], bufs[0][1]) and torch.equal(bufs[3][1], bufs[1][1])
    assert not bool(torch.isnan(bufs[3][1]).any())
    assert all(_guards_intact(b, 0, v.numel()) for b, v in bufs)
