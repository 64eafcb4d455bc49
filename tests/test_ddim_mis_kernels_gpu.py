"""``idf_ddim_update_units`` and ``idf_q_sample_blend_units`` on a real MI355X against a row gather + the reference's fp32 torch
expressions on the CPU (tests/emul_ops_ddim_mis.py over tests/ddim_cases.py): BIT identity (``torch.equal``).

Shapes: U = 3 units over B = 2 images with the non-monotone table [1, 0, 1]; C = 4 with HW = 16 (16-B accesses), HW = 15 (scalar) and
HW = 400 (several workgroups); views one float into their allocation (scalar); U == B without a table (the plain kernel); a table
holding -1 and B, which must act as 0 and B - 1.  Every output lives in a NaN-filled buffer with 64 guard elements behind it (and one
in front of an offset view), which must stay NaN.  Inputs are built once on the CPU and shared.
"""
import functools

import pytest
import torch

from tests import ddim_cases
from tests.emul_ops_ddim_mis import ddim_update_units_expr, q_sample_blend_units_expr

pytestmark = pytest.mark.gpu
GUARD = 64
U, B, C = 3, 2, 4
TABLE = [1, 0, 1]
HWS = [16, 15, 400]
S1M = [float(torch.sqrt(1.0 - torch.tensor(t[0], dtype=torch.float32))) for t in ddim_cases.TRIPLES]
SA, S1 = 0.6503041982650757, 0.7596831917762756                  # sqrt(ac), sqrt(1 - ac) of one timestep, fp32 values


@functools.lru_cache(maxsize=None)
def _ops():
    from instancediffusion_amd.ops import HipOps
    return HipOps(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _pool(hw, u=U, b=B):
    """x, eps_cond, eps_uncond [u, C, hw, 1]; noise, x0, q_sample noise [b, C, hw, 1]; masks [b, 1, hw, 1] / [b, C, hw, 1] (soft entries
    included).  CPU fp32, left unchanged."""
    g = torch.Generator().manual_seed(500 + hw + 7 * u)
    x, ec, eu = (torch.randn(u, C, hw, 1, generator=g) * s for s in (3.0, 1.0, 1.0))
    nz, x0, qn = (torch.randn(b, C, hw, 1, generator=g) for _ in range(3))
    masks = {}
    for mc_ in (1, C):
        m = (torch.rand(b, mc_, hw, 1, generator=g) > 0.5).float()
        masks[mc_] = torch.where(torch.rand(b, mc_, hw, 1, generator=g) > 0.25, m, torch.full_like(m, 0.25))
    return x, ec, eu, nz, x0, qn, masks


def _dev(t, offset=0):
    """A device copy of t; offset 1: a view one float into its allocation (4-B aligned only -> the scalar path)."""
    if t is None:
        return None
    buf = torch.empty(t.numel() + offset, device="cuda", dtype=torch.float32)
    v = buf[offset:]
    v.copy_(t.reshape(-1))
    return v.view(t.shape)


def _table(entries):
    return torch.tensor(entries, dtype=torch.int32, device="cuda")


def _guarded(shape, offset=0):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((offset + n + GUARD,), float("nan"), device="cuda", dtype=torch.float32)
    return buf, buf[offset:offset + n].view(shape)


def _guards_intact(buf, offset, n):
    return bool(torch.isnan(buf[:offset]).all()) and bool(torch.isnan(buf[offset + n:]).all()) and buf.numel() - offset - n >= GUARD


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("noisy", [False, True], ids=["sigma0", "sigma>0"])
@pytest.mark.parametrize("guided", [True, False], ids=["guided", "unguided"])
@pytest.mark.parametrize("hw", HWS)
def test_ddim_update_units_is_bit_identical(hw, guided, noisy, offset):
    ops = _ops()
    x, ec, eu, nz, _, _, _ = _pool(hw)
    tab = _table(TABLE)
    for (a_t, a_prev, sigma), s1m in zip(ddim_cases.TRIPLES, S1M):
        sig = sigma if noisy else 0.0
        want, want_p = ddim_update_units_expr(x, ec, eu if guided else None, ddim_cases.GUIDANCE, a_t, a_prev, sig, s1m,
                                              nz if noisy else None, TABLE)
        buf, out = _guarded(x.shape, offset)
        pbuf, p0 = _guarded(x.shape, offset)
        ops.ddim_update_units(_dev(x, offset), _dev(ec, offset), _dev(eu, offset) if guided else None, ddim_cases.GUIDANCE, a_t, a_prev,
                              sig, s1m, _dev(nz, offset) if noisy else None, tab, out, pred_x0=p0)
        assert torch.equal(out.cpu(), want) and _guards_intact(buf, offset, x.numel()), a_t
        assert torch.equal(p0.cpu(), want_p) and _guards_intact(pbuf, offset, x.numel()), a_t
    if noisy:                                                       # the table is what is tested: another one gives another result
        other, _ = ddim_update_units_expr(x, ec, eu if guided else None, ddim_cases.GUIDANCE, a_t, a_prev, sig, s1m, nz, [0, 1, 0])
        assert not torch.equal(other, want)


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("hw", HWS)
def test_ddim_update_units_in_place(hw, offset):
    ops = _ops()
    x, ec, eu, nz, _, _, _ = _pool(hw)
    a_t, a_prev, sigma = ddim_cases.TRIPLES[1]
    want, _ = ddim_update_units_expr(x, ec, eu, ddim_cases.GUIDANCE, a_t, a_prev, sigma, S1M[1], nz, TABLE)
    buf, xio = _guarded(x.shape, offset)
    xio.copy_(x)
    ops.ddim_update_units(xio, _dev(ec, offset), _dev(eu, offset), ddim_cases.GUIDANCE, a_t, a_prev, sigma, S1M[1], _dev(nz, offset),
                          _table(TABLE), xio)
    assert torch.equal(xio.cpu(), want) and _guards_intact(buf, offset, x.numel())


@pytest.mark.parametrize("hw", HWS)
def test_without_a_table_it_is_the_plain_kernel(hw):
    """U == B and img_of == NULL: ``idf_ddim_update``'s result bit for bit (and the CPU expression's)."""
    ops = _ops()
    x, ec, eu, nz, _, _, _ = _pool(hw, B, B)
    a_t, a_prev, sigma = ddim_cases.TRIPLES[0]
    want, _ = ddim_cases.ddim_update_expr(x, ec, eu, ddim_cases.GUIDANCE, a_t, a_prev, sigma, S1M[0], nz)
    dx, dc, du, dn = (_dev(t) for t in (x, ec, eu, nz))
    buf, out = _guarded(x.shape)
    ops.ddim_update_units(dx, dc, du, ddim_cases.GUIDANCE, a_t, a_prev, sigma, S1M[0], dn, None, out)
    buf2, out2 = _guarded(x.shape)
    ops.ddim_update(dx, dc, du, ddim_cases.GUIDANCE, a_t, a_prev, sigma, S1M[0], dn, out2)
    assert torch.equal(out, out2) and torch.equal(out.cpu(), want)
    assert _guards_intact(buf, 0, x.numel()) and _guards_intact(buf2, 0, x.numel())
    # the identity table through the unit kernel: the same values again
    buf3, out3 = _guarded(x.shape)
    ops.ddim_update_units(dx, dc, du, ddim_cases.GUIDANCE, a_t, a_prev, sigma, S1M[0], dn, _table(list(range(B))), out3)
    assert torch.equal(out3, out2) and _guards_intact(buf3, 0, x.numel())


@pytest.mark.parametrize("mode", ["fresh", "in_place", "offset1"])
@pytest.mark.parametrize("per_channel", [False, True], ids=["mask_B1HW", "mask_BCHW"])
@pytest.mark.parametrize("hw", HWS)
def test_q_sample_blend_units_is_bit_identical(hw, per_channel, mode):
    ops = _ops()
    img, _, _, _, x0, qn, masks = _pool(hw)
    mask = masks[C if per_channel else 1]
    want = q_sample_blend_units_expr(x0, qn, mask, img, TABLE, SA, S1)
    offset = 1 if mode == "offset1" else 0
    buf, out = _guarded(img.shape, offset)
    if mode == "in_place":
        out.copy_(img)
        ops.q_sample_blend_units(_dev(x0), _dev(qn), _dev(mask), out, _table(TABLE), SA, S1, out)
    else:
        ops.q_sample_blend_units(_dev(x0, offset), _dev(qn, offset), _dev(mask, offset), _dev(img, offset), _table(TABLE), SA, S1, out)
    assert torch.equal(out.cpu(), want) and _guards_intact(buf, offset, img.numel())
    assert not torch.equal(q_sample_blend_units_expr(x0, qn, mask, img, [0, 1, 0], SA, S1), want)
    if hw == HWS[0] and mode == "fresh":                          # the identity table: the plain kernel's values
        x2 = img[:B].contiguous()
        buf1, out1 = _guarded(x2.shape)
        ops.q_sample_blend_units(_dev(x0), _dev(qn), _dev(mask), _dev(x2), _table(list(range(B))), SA, S1, out1)
        buf2, out2 = _guarded(x2.shape)
        ops.q_sample_blend(_dev(x0), _dev(qn), _dev(mask), _dev(x2), SA, S1, out2)
        assert torch.equal(out1, out2) and _guards_intact(buf1, 0, x2.numel()) and _guards_intact(buf2, 0, x2.numel())


@pytest.mark.parametrize("hw", HWS[:2])
def test_out_of_range_table_entries_are_clamped(hw):
    """-1 acts as image 0 and B as image B - 1; nothing outside the buffers is touched (the per-image operands are exact-size
    allocations, the outputs are guarded)."""
    ops = _ops()
    x, ec, eu, nz, x0, qn, masks = _pool(hw)
    bad, clamped = [-1, B, 0], [0, B - 1, 0]
    a_t, a_prev, sigma = ddim_cases.TRIPLES[1]
    want, _ = ddim_update_units_expr(x, ec, eu, ddim_cases.GUIDANCE, a_t, a_prev, sigma, S1M[1], nz, clamped)
    buf, out = _guarded(x.shape)
    ops.ddim_update_units(_dev(x), _dev(ec), _dev(eu), ddim_cases.GUIDANCE, a_t, a_prev, sigma, S1M[1], _dev(nz), _table(bad), out)
    assert torch.equal(out.cpu(), want) and _guards_intact(buf, 0, x.numel())
    for mc_ in (1, C):
        want = q_sample_blend_units_expr(x0, qn, masks[mc_], x, clamped, SA, S1)
        buf, out = _guarded(x.shape)
        ops.q_sample_blend_units(_dev(x0), _dev(qn), _dev(masks[mc_]), _dev(x), _table(bad), SA, S1, out)
        assert torch.equal(out.cpu(), want) and _guards_intact(buf, 0, x.numel()), mc_


def test_argument_errors_return_before_any_launch():
    import ctypes as Ct
    from instancediffusion_amd import _lib
    lib = _lib.load()
    x, ec, eu, nz, x0, qn, masks = (_dev(t) if torch.is_tensor(t) else t for t in _pool(16))
    mask = _dev(masks[1])
    tab = _table(TABLE)
    buf = torch.full((x.numel() + GUARD,), float("nan"), device="cuda", dtype=torch.float32)
    stream = Ct.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: None if t is None else Ct.c_void_p(t.data_ptr())
    a_t, a_prev, sigma = ddim_cases.TRIPLES[1]

    def upd(x=x, ec=ec, a_t=a_t, a_prev=a_prev, sigma=sigma, nz=nz, tab=tab, out=buf, U=U, B=B, chw=C * 16):
        return lib.idf_ddim_update_units(P(x), P(ec), P(eu), 7.5, a_t, a_prev, sigma, S1M[1], P(nz), P(tab), P(out), None, U, B, chw, stream)
    bad = [upd(x=None), upd(ec=None), upd(out=None), upd(a_t=0.0), upd(a_prev=-0.1), upd(sigma=-0.1), upd(a_prev=0.9, sigma=0.5),
           upd(nz=None), upd(a_t=float("nan")), upd(U=0), upd(B=0), upd(chw=0), upd(tab=None)]
    assert bad == [-1] * len(bad), bad

    def blend(x0=x0, nz=qn, mask=mask, img=x, tab=tab, out=buf, U=U, B=B, Cc=C, HW=16, mc_=1):
        return lib.idf_q_sample_blend_units(P(x0), P(nz), P(mask), P(img), P(tab), 0.6, 0.8, P(out), U, B, Cc, HW, mc_, stream)
    bad = [blend(x0=None), blend(nz=None), blend(mask=None), blend(img=None), blend(out=None), blend(tab=None), blend(U=0), blend(B=0),
           blend(Cc=0), blend(HW=0), blend(mc_=0), blend(mc_=2)]
    assert bad == [-1] * len(bad), bad
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())
    assert upd() == 0 and blend() == 0                             # the same calls with nothing wrong go through
    torch.cuda.synchronize()
    assert not bool(torch.isnan(buf[:x.numel()]).any()) and bool(torch.isnan(buf[x.numel():]).all())


def test_both_launches_replay_from_a_captured_graph():
    from instancediffusion_amd.engine import capture_graph
    ops = _ops()
    x, ec, eu, nz, x0, qn, masks = (_dev(t) if torch.is_tensor(t) else t for t in _pool(16))
    mask, tab = _dev(masks[1]), _table(TABLE)
    a_t, a_prev, sigma = ddim_cases.TRIPLES[1]

    def step(blended, out):
        ops.q_sample_blend_units(x0, qn, mask, x, tab, SA, S1, blended)
        ops.ddim_update_units(blended, ec, eu, ddim_cases.GUIDANCE, a_t, a_prev, sigma, S1M[1], nz, tab, out)
    bufs = [_guarded(x.shape) for _ in range(4)]
    step(bufs[0][1], bufs[1][1])                                  # eager (also the warm-up outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with capture_graph(graph):
        step(bufs[2][1], bufs[3][1])
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bufs[2][1], bufs[0][1]) and torch.equal(bufs[3][1], bufs[1][1])
    assert not bool(torch.isnan(bufs[3][1]).any()) and all(_guards_intact(b, 0, v.numel()) for b, v in bufs)
