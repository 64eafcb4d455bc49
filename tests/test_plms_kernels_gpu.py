"""``idf_cfg_combine``, ``idf_plms_update`` and ``idf_mis_merge`` on a real MI355X against torch's fp32 expressions evaluated on the
CPU (tests/plms_cases.py): BIT identity (``torch.equal``) at sizes below, at and past the 256-thread block, on 16-B aligned buffers
and on views one float into their allocation, for every mode and three scalar triples of the S = 5 schedule; operands a mode does
not read passed as NULL and as NaN; the five-step chain of ``samplers._plms_step``; argument errors; graph replay.

Every output lives in a NaN-filled buffer with at least 64 guard elements behind it (and in front of an offset view), which must
stay NaN.  Inputs and the expected values are built once on the CPU and shared (tests/test_plms_host.py shows what they tell apart).
"""
import ctypes as C
import functools

import pytest
import torch

from tests import plms_cases as pc

pytestmark = pytest.mark.gpu
GUARD = 64
NAN = float("nan")


@functools.lru_cache(maxsize=None)
def _ops():
    from instancediffusion_amd.ops import HipOps
    return HipOps(torch.bfloat16)


def _dev(t, offset=0):
    """A device copy of t; offset 1: a view one float into its allocation (4-B aligned only)."""
    if t is None:
        return None
    buf = torch.empty(t.numel() + offset, device="cuda", dtype=torch.float32)
    v = buf[offset:]
    v.copy_(t.reshape(-1))
    assert (v.data_ptr() % 16 != 0) == bool(offset)
    return v.view(t.shape)


def _guarded(n, offset=0):
    buf = torch.full((offset + n + GUARD,), NAN, device="cuda", dtype=torch.float32)
    return buf, buf[offset:offset + n]


def _guards_intact(buf, offset, n):
    return bool(torch.isnan(buf[:offset]).all()) and bool(torch.isnan(buf[offset + n:]).all()) and buf.numel() - offset - n >= GUARD


def _differ(got, want):
    return int((got != want).sum())


# ---- idf_cfg_combine ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("halves", [False, True], ids=["separate", "halves"])
def test_cfg_combine_is_bit_identical(halves, offset):
    """``halves``: the operands are e2[:n] and e2[n:] of one [cond | uncond] buffer, as ``samplers._eps`` passes them."""
    ops = _ops()
    bad = {}
    for n in pc.NS:
        p = pc.pool(n)
        if halves:
            e2 = _dev(torch.cat([p["ec"], p["eu"]]), offset)
            ec, eu = e2[:n], e2[n:]
        else:
            ec, eu = _dev(p["ec"], offset), _dev(p["eu"], offset)
        for g in (7.5, 1.0, 0.0):
            buf, out = _guarded(n, offset)
            assert ops.cfg_combine(ec, eu, g, out) is out
            k = _differ(out.cpu(), pc.want_cfg(n, g))
            print(f"[plms] cfg_combine n = {n} guidance {g}: {k} of {n} elements differ from torch's fp32 expression")
            if k:
                bad[(n, g)] = k
            assert _guards_intact(buf, offset, n), (n, g)
    assert not bad, bad


# ---- idf_plms_update ---------------------------------------------------------------------------------------------------
def _operands(p, mode, offset, unread):
    """(old, e_next) for ``HipOps.plms_update``: what the mode reads from the pool, what it does not read as NULL (``unread`` None)
    or as NaN-filled buffers (``unread`` "nan")."""
    n = p["x"].numel()
    filler = (lambda: _dev(torch.full((n,), NAN), offset)) if unread == "nan" else (lambda: None)
    hist = [_dev(h, offset) for h in pc.history(p)]
    reads = max(mode - 1, 0)                                       # history entries the mode reads: old[-1] .. old[-reads]
    old = [filler() for _ in range(3 - reads)] + hist[3 - reads:]
    if unread is None:
        old = hist[3 - reads:] if reads else []
    e_next = _dev(p["en"], offset) if mode == 1 else filler()
    return old, e_next


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("mode", pc.MODES)
def test_plms_update_is_bit_identical(mode, offset):
    ops = _ops()
    bad = {}
    for n in pc.NS:
        p = pc.pool(n)
        x, e_t = _dev(p["x"], offset), _dev(p["ec"], offset)
        old, e_next = _operands(p, mode, offset, None)
        for index in pc.STEP_INDICES:
            buf, out = _guarded(n, offset)
            assert ops.plms_update(x, e_t, old, e_next, mode, *pc.scalars(index), out) is out
            k = _differ(out.cpu(), pc.want_plms(n, mode, index))
            print(f"[plms] plms_update mode {mode} n = {n} index {index}: {k} of {n} elements differ from torch's fp32 expression")
            if k:
                bad[(n, index)] = k
            assert _guards_intact(buf, offset, n), (n, index)
    assert not bad, bad


@pytest.mark.parametrize("mode", pc.MODES)
def test_unread_operands_are_not_read(mode):
    """The history pointers and e_next a mode does not read, as NULL and as NaN-filled buffers (mode 1: NaN e1 .. e3; mode >= 2: a NaN
    e_next): the same result."""
    ops = _ops()
    index = pc.STEP_INDICES[1]
    for n in pc.NS:
        p = pc.pool(n)
        x, e_t = _dev(p["x"]), _dev(p["ec"])
        got = []
        for unread in (None, "nan"):
            old, e_next = _operands(p, mode, 0, unread)
            assert (unread is None) or len(old) == 3 and (mode == 1 or e_next is not None)
            buf, out = _guarded(n)
            ops.plms_update(x, e_t, old, e_next, mode, *pc.scalars(index), out)
            got.append(out.cpu())
            assert _guards_intact(buf, 0, n), (n, unread)
        assert not torch.isnan(got[1]).any(), (n, "a NaN operand the mode does not read was read")
        assert torch.equal(got[0], got[1]) and torch.equal(got[0], pc.want_plms(n, mode, index)), n


# ---- the five steps of a run -------------------------------------------------------------------------------------------
def _chain_on(ops, bufs):
    """``plms_cases.chain``'s two callables on the HIP ops; every output is a guarded buffer, collected in ``bufs``."""
    def out(n):
        b, v = _guarded(n)
        bufs.append((b, v))
        return v

    def cfg(ec, eu, g):
        return ops.cfg_combine(ec, eu, g, out(ec.numel()))

    def update(x, e_t, old, e_next, mode, a_t, a_prev, s1m):
        return ops.plms_update(x, e_t, old, e_next, mode, a_t, a_prev, s1m, out(x.numel()))
    return cfg, update


def _chain_table_dev():
    x, table = pc.chain_table()
    n = pc.CHAIN_N
    e2s = [_dev(torch.cat(pair)) for pair in table]                # [cond | uncond], as the engine's eps buffer
    return _dev(x), [(e2[:n], e2[n:]) for e2 in e2s]


def test_five_step_chain_through_hipops():
    """cfg, mode 0, cfg, mode 1, then (cfg, mode 2), (cfg, mode 3), (cfg, mode 4), (cfg, mode 4) with the history rotation, on table
    eps: the x after every step, the final one included, equals the CPU chain of the expressions."""
    bufs = []
    x, table = _chain_table_dev()
    xs = pc.chain(*_chain_on(_ops(), bufs), x, table)
    torch.cuda.synchronize()
    k = [_differ(g.cpu(), w) for g, w in zip(xs, pc.chain_want())]
    print(f"[plms] chain: {k} of {pc.CHAIN_N} elements differ after steps 1..5")
    assert len(bufs) == 12 and all(_guards_intact(b, 0, pc.CHAIN_N) for b, _ in bufs)
    assert torch.equal(xs[-1].cpu(), pc.chain_want()[-1]) and k == [0] * pc.S, k


def test_the_launches_replay_from_a_captured_graph():
    """One capture of cfg, mode 0, cfg, mode 1, cfg, mode 2; two replays: every buffer equals the eager run, the guards are intact."""
    from instancediffusion_amd.engine import capture_graph
    ops = _ops()
    n = pc.CHAIN_N
    x, table = _chain_table_dev()

    def steps(bufs):
        e_t, x_pred, e_next, x1, e_2, x2 = (v for _b, v in bufs)
        sc = pc.scalars(4)
        ops.cfg_combine(*table[0], pc.GUIDANCE, e_t)
        ops.plms_update(x, e_t, [], None, 0, *sc, x_pred)
        ops.cfg_combine(*table[1], pc.GUIDANCE, e_next)
        ops.plms_update(x, e_t, [], e_next, 1, *sc, x1)
        ops.cfg_combine(*table[2], pc.GUIDANCE, e_2)
        ops.plms_update(x1, e_2, [e_t], None, 2, *pc.scalars(3), x2)
    eager = [_guarded(n) for _ in range(6)]
    steps(eager)                                                    # eager (also the warm-up outside the capture)
    torch.cuda.synchronize()
    assert torch.equal(eager[5][1].cpu(), pc.chain_want()[1])
    bufs = [_guarded(n) for _ in range(6)]
    graph = torch.cuda.CUDAGraph()
    with capture_graph(graph):
        steps(bufs)
    for _ in range(2):
        for b, _v in bufs:
            b.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(bufs[k][1], eager[k][1]) for k in range(6))
        assert all(_guards_intact(b, 0, n) for b, _v in bufs)


# ---- idf_mis_merge -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", pc.MERGE_SHAPES, ids=["2x3x5x7", "1x4x24x40", "3x4x16x16"])
@pytest.mark.parametrize("mode", [0, 1], ids=["mean", "paste"])
def test_mis_merge_is_bit_identical(mode, shape):
    ops = _ops()
    B, Cc, H, W = shape
    per = B * Cc * H * W
    for n_inst in pc.MERGE_N_INST:
        lat = pc.merge_lat(n_inst, shape)
        boxes = pc.merge_boxes_for(n_inst, H, W)
        want = pc.mis_merge_expr(lat, boxes, mode)
        lat_buf = torch.full(((n_inst + 2) * per,), NAN, device="cuda")          # a spare NaN instance behind the last one
        lat_d = lat_buf[:(n_inst + 1) * per].view(lat.shape)
        lat_d.copy_(lat)
        box_d = boxes.cuda() if n_inst else torch.zeros(1, 4, dtype=torch.int32, device="cuda")
        buf, out = _guarded(per)
        ops.mis_merge(lat_d, box_d, out.view(shape), mode)
        got = out.cpu().view(shape)
        assert not torch.isnan(got).any(), "the spare NaN instance behind lat was read"
        assert torch.equal(got, want), (n_inst, _differ(got, want))
        assert _guards_intact(buf, 0, per), n_inst
        if mode == 0:   # n_inst + 1 sequential fp32 adds and one division, against the float64 mean
            l64 = lat.double()
            bound = (n_inst + 2) * 2.0 ** -24 * l64.abs().sum(0) / (n_inst + 1)
            err = (got.double() - l64.sum(0) / (n_inst + 1)).abs()
            assert bool((err <= bound).all()), (n_inst, float((err - bound).max()))


# ---- argument errors ---------------------------------------------------------------------------------------------------
def test_argument_errors_return_before_any_launch():
    """Every IDF_E_ARG case of include/idf.h for the three entry points: -1, and the NaN-filled output is untouched; the same call
    with nothing wrong returns 0."""
    from instancediffusion_amd import _lib
    lib = _lib.load()
    n = 256
    p = pc.pool(257)
    x, e_t, h1, h2, h3, en = (_dev(p[k][:n].clone()) for k in ("x", "ec", "h1", "h2", "h3", "en"))
    eu = _dev(p["eu"][:n].clone())
    buf = torch.full((n + GUARD,), NAN, device="cuda", dtype=torch.float32)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    a_t, a_prev, s1m = pc.scalars(2)
    inf = float("inf")

    def cfg(ec=e_t, eu=eu, out=buf, n=n):
        return lib.idf_cfg_combine(P(ec), P(eu), 7.5, P(out), n, stream)

    def upd(x=x, e_t=e_t, e1=h1, e2=h2, e3=h3, en=en, mode=4, a_t=a_t, a_prev=a_prev, s1m=s1m, out=buf, n=n):
        return lib.idf_plms_update(P(x), P(e_t), P(e1), P(e2), P(e3), P(en), mode, a_t, a_prev, s1m, P(out), n, stream)
    B, Cc, H, W = 1, 1, 16, 16
    lat = _dev(pc.merge_lat(3, (3, 4, 16, 16))[:, :1, :1].contiguous())
    boxes = pc.merge_boxes_for(3, H, W).cuda()

    def mrg(lat=lat, boxes=boxes, out=buf, n_inst=3, B=B, Cc=Cc, H=H, W=W, mode=1):
        return lib.idf_mis_merge(P(lat), P(boxes), P(out), n_inst, B, Cc, H, W, mode, stream)
    bad = [cfg(ec=None), cfg(eu=None), cfg(out=None), cfg(n=0), cfg(n=-4),
           upd(x=None), upd(e_t=None), upd(out=None), upd(n=0), upd(n=-4), upd(mode=-1), upd(mode=5),
           upd(mode=1, en=None), upd(mode=2, e1=None), upd(mode=3, e2=None), upd(mode=4, e3=None), upd(mode=4, e1=None),
           upd(a_t=0.0), upd(a_t=-0.1), upd(a_t=NAN), upd(a_t=inf), upd(a_prev=-0.1), upd(a_prev=1.5), upd(a_prev=NAN),
           upd(a_prev=inf), upd(s1m=NAN), upd(s1m=inf), upd(s1m=-inf),
           mrg(lat=None), mrg(out=None), mrg(n_inst=-1), mrg(B=0), mrg(Cc=0), mrg(H=0), mrg(W=-1), mrg(mode=2), mrg(mode=-1),
           mrg(boxes=None)]
    assert bad == [-1] * len(bad), bad
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())
    good = [cfg, upd, lambda: upd(mode=0, e1=None, e2=None, e3=None, en=None), lambda: upd(mode=1, e1=None, e2=None, e3=None),
            lambda: upd(mode=2, e2=None, e3=None, en=None), lambda: upd(a_prev=0.0), lambda: upd(a_prev=1.0), mrg,
            lambda: mrg(mode=0, boxes=None), lambda: mrg(mode=0, n_inst=0, boxes=None)]
    for call in good:                                               # the same calls with nothing wrong go through
        buf.fill_(NAN)
        assert call() == 0
        torch.cuda.synchronize()
        assert not bool(torch.isnan(buf[:n]).any()) and bool(torch.isnan(buf[n:]).all())
