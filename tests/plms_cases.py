"""PLMS step-kernel test support: the fp32 torch expressions ``idf_cfg_combine``, ``idf_plms_update`` and ``idf_mis_merge`` must
reproduce bit for bit, the element pools and schedule scalars their tests share, a CPU chain of the five steps of an S = 5 run, and
the wrong variants (contracted products, swapped history slots, ...) that tests/test_plms_host.py shows the pools tell apart.

Only torch / numpy are imported at module level; the repository's modules are imported inside the functions that need them.
"""
from __future__ import annotations

import functools
from typing import List

import numpy as np
import torch

S, GUIDANCE = 5, 7.5
NS = [60, 255, 257, 1603]       # fewer than a wave; one short of a 256-thread block; one past it; odd, more than six blocks
STEP_INDICES = [4, 2, 0]        # schedule index of the first, the middle and the last step of the S = 5 run
MODES = [0, 1, 2, 3, 4]
# sixteen hand-placed values: exact zeros of both signs, magnitudes from 1e-30 to 1e18 (no NaN, inf or subnormal: NaN payloads
# differ between hosts and devices)
SPECIAL = [0.0, -0.0, 1e-30, -1e-30, 1e-20, -3e-12, 1e-6, -1e-3, 1.0, -1.0, 255.5, -65504.0, 1e9, -1e12, 1e18, -1e18]
POOL_NAMES = ("x", "ec", "eu", "h1", "h2", "h3", "en")   # h1 is the NEWEST history entry (old[-1]), h3 the oldest (old[-3])


# ---- the kernels' reference expressions ---------------------------------------------------------------------------
def cfg_combine_expr(e_cond, e_uncond, guidance):
    """plms.py:126 as torch evaluates it in fp32: a subtraction, a product with the scalar, an addition, each rounded."""
    return e_uncond + guidance * (e_cond - e_uncond)


def _e_prime(e_t, old, e_next, mode):
    """plms.py:148-163, the five rules as the reference writes them; ``old``: the eps history, newest last."""
    if mode == 0:
        return e_t
    if mode == 1:
        return (e_t + e_next) / 2
    if mode == 2:
        return (3 * e_t - old[-1]) / 2
    if mode == 3:
        return (23 * e_t - 16 * old[-1] + 5 * old[-2]) / 12
    assert mode == 4
    return (55 * e_t - 59 * old[-1] + 37 * old[-2] - 9 * old[-3]) / 24


def _roots(a_t, a_prev):
    """sqrt(a_t), sqrt(a_prev), sqrt(1 - a_prev): the correctly rounded fp32 square root of fp32 scalars (numpy's = C's ``sqrtf``,
    which the launcher uses), for the reason given in ``ddim_cases.ddim_update_expr``; the radicand 1 - a_prev is ONE fp32
    subtraction."""
    f32 = np.float32
    return np.sqrt(f32(a_t)), np.sqrt(f32(a_prev)), np.sqrt(f32(1.0) - f32(a_prev))


def _full(x, v):
    return torch.full((1,) * x.dim(), float(v), dtype=torch.float32)          # plms.py:132-135


def plms_update_expr(x, e_t, old, e_next, mode, a_t, a_prev, sqrt_1m_at):
    """plms.py:130-165 with sigma = 0 (so no noise term and dir_xt = sqrt(1 - a_prev) e'), as torch evaluates it in fp32.
    mode 0: e' = e_t (the first step's predictor); 1: the first step's corrector with ``e_next``; 2-4: Adams-Bashforth on ``old``."""
    ep = _e_prime(e_t, old, e_next, mode)
    sqrt_at, sqrt_aprev, dc = (_full(x, v) for v in _roots(a_t, a_prev))
    pred_x0 = (x - _full(x, sqrt_1m_at) * ep) / sqrt_at                       # :138
    return sqrt_aprev * pred_x0 + dc * ep                                     # :141-143


def mis_merge_expr(lat, boxes, mode):
    """lat [n_inst + 1, B, C, H, W] fp32 -> [B, C, H, W].  Mode 0: the loop include/idf.h states, s = 0; s = s + lat[k] in order;
    s / float(count).  Mode 1: the slicing loop of plms_instance.py:112-132 on dims 2 and 3 with box[0]:box[2] and box[1]:box[3];
    later instances win.  boxes: int32 [n_inst, 4], coordinates >= 0."""
    n1 = lat.shape[0]
    if mode == 0:
        s = torch.zeros_like(lat[0])
        for k in range(n1):
            s = s + lat[k]
        return s / float(n1)
    assert mode == 1
    v = lat[0].clone()
    for k in range(n1 - 1):
        b = [int(c) for c in boxes[k].tolist()]
        assert min(b) >= 0
        v[:, :, b[0]:b[2], b[1]:b[3]] = lat[k + 1][:, :, b[0]:b[2], b[1]:b[3]]
    return v


# ---- wrong variants (CPU only: tests/test_plms_host.py) -------------------------------------------------------------
def _fma(a, b, c):
    """a * b + c with one rounding: the fp32 rounding of the float64 value (the product of two fp32 numbers is exact there)."""
    a, b, c = (v if torch.is_tensor(v) else torch.tensor(float(v), dtype=torch.float32) for v in (a, b, c))
    return (a.double() * b.double() + c.double()).float()


def contracted_cfg(e_cond, e_uncond, guidance):
    """u + g * (ec - u) with the product feeding an FMA: what a kernel compiled with contraction allowed computes."""
    return _fma(guidance, e_cond - e_uncond, e_uncond)


def contracted_plms(x, e_t, old, e_next, mode, a_t, a_prev, sqrt_1m_at):
    """``plms_update_expr`` with the three FMAs the kernel had when it was compiled with contraction allowed (read from its gfx950
    assembly): 3 e_t - old[-1] in mode 2, 23 e_t - 16 old[-1] in mode 3 (the product 16 old[-1] unrounded), x - sqrt_1m_at e' in
    every mode.  Mode 4's four products and the last sum's two were packed multiplies, each rounded."""
    if mode == 2:
        ep = _fma(3.0, e_t, -old[-1]) / 2
    elif mode == 3:
        ep = (_fma(-16.0, old[-1], 23 * e_t) + 5 * old[-2]) / 12
    else:
        ep = _e_prime(e_t, old, e_next, mode)
    sqrt_at, sqrt_aprev, dc = (_full(x, v) for v in _roots(a_t, a_prev))
    pred_x0 = _fma(-_full(x, sqrt_1m_at), ep, x) / sqrt_at
    return sqrt_aprev * pred_x0 + dc * ep


def plms_swapped_history(x, e_t, old, e_next, mode, a_t, a_prev, sqrt_1m_at):
    """old[-1] and old[-2] exchanged (modes 3 and 4 read both)."""
    old = list(old)
    old[-1], old[-2] = old[-2], old[-1]
    return plms_update_expr(x, e_t, old, e_next, mode, a_t, a_prev, sqrt_1m_at)


def plms_mode_off_by_one(x, e_t, old, e_next, mode, a_t, a_prev, sqrt_1m_at):
    return plms_update_expr(x, e_t, old, e_next, (mode + 1) % 5, a_t, a_prev, sqrt_1m_at)


def plms_dir_from_a_t(x, e_t, old, e_next, mode, a_t, a_prev, sqrt_1m_at):
    """sqrt(1 - a_t) in place of sqrt(1 - a_prev) in front of e'."""
    ep = _e_prime(e_t, old, e_next, mode)
    sqrt_at, sqrt_aprev, _ = (_full(x, v) for v in _roots(a_t, a_prev))
    dc = _full(x, np.sqrt(np.float32(1.0) - np.float32(a_t)))
    pred_x0 = (x - _full(x, sqrt_1m_at) * ep) / sqrt_at
    return sqrt_aprev * pred_x0 + dc * ep


def merge_hw_swapped(lat, boxes, mode):
    """Mode 1 with the pixel index decomposed as if the image were W rows of H pixels."""
    n1, B, C, H, W = lat.shape
    flat = lat.reshape(n1, B, C, H * W)
    v = flat[0].clone()
    p = torch.arange(H * W)
    h, w = (p // H) % W, p % H
    for k in range(n1 - 1):
        b = [int(c) for c in boxes[k].tolist()]
        inside = (h >= b[0]) & (h < b[2]) & (w >= b[1]) & (w < b[3])
        v[:, :, inside] = flat[k + 1][:, :, inside]
    return v.reshape(B, C, H, W)


def merge_box_axes_swapped(lat, boxes, mode):
    """Mode 1 with box[1]:box[3] on dim 2 and box[0]:box[2] on dim 3."""
    return mis_merge_expr(lat, boxes[:, [1, 0, 3, 2]], 1)


def merge_earlier_wins(lat, boxes, mode):
    """Mode 1 with the instances pasted in reverse order."""
    n1 = lat.shape[0]
    order = [0] + list(range(n1 - 1, 0, -1))
    return mis_merge_expr(lat[order], boxes.flip(0), 1)


def merge_divisor_n_inst(lat, boxes, mode):
    """Mode 0 divided by n_inst instead of n_inst + 1 (n_inst >= 1)."""
    n1 = lat.shape[0]
    s = torch.zeros_like(lat[0])
    for k in range(n1):
        s = s + lat[k]
    return s / float(n1 - 1)


# ---- the pools and scalars the tests share -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pool(n: int) -> dict:
    """x (scaled by 3), eps_cond, eps_uncond, the three history tensors and e_next of n elements: ``randn`` with fixed seeds, then
    the sixteen SPECIAL values at sixteen places spread from element 0 to element n - 1, rotated by three places from one tensor to
    the next so that every tensor meets other values there.  CPU fp32, shared: leave them unchanged."""
    g = torch.Generator().manual_seed(7000 + n)
    at = [round(i * (n - 1) / 15) for i in range(16)]
    out = {}
    for j, name in enumerate(POOL_NAMES):
        t = torch.randn(n, generator=g) * (3.0 if name == "x" else 1.0)
        t[at] = torch.tensor(SPECIAL[3 * j % 16:] + SPECIAL[:3 * j % 16], dtype=torch.float32)
        out[name] = t
    return out


def history(p: dict) -> List[torch.Tensor]:
    """The pool's history as the list ``plms_update`` takes: oldest first, old[-1] = h1."""
    return [p["h3"], p["h2"], p["h1"]]


@functools.lru_cache(maxsize=None)
def scalars(index: int):
    """(a_t, a_prev, sqrt_1m_at) at ``index`` of the S = 5 schedule of ``oracle.ref_cpu._schedule`` as Python floats holding fp32
    values; sqrt_1m_at = sqrt(float32(1) - a_t) in fp32."""
    from oracle import ref_cpu
    _, a, a_prev = ref_cpu._schedule(S)
    return float(a[index]), float(a_prev[index]), float(np.sqrt(np.float32(1.0) - np.float32(a[index])))


@functools.lru_cache(maxsize=None)
def want_cfg(n: int, guidance: float):
    p = pool(n)
    return cfg_combine_expr(p["ec"], p["eu"], guidance)


@functools.lru_cache(maxsize=None)
def want_plms(n: int, mode: int, index: int):
    """``plms_update_expr`` on the pool: e_t is the pool's eps_cond (any tensor serves as the guided eps here)."""
    p = pool(n)
    return plms_update_expr(p["x"], p["ec"], history(p), p["en"], mode, *scalars(index))


# ---- the five steps of an S = 5 run over table eps ---------------------------------------------------------------------
CHAIN_N = 1603
CHAIN_CALLS = 6                  # model evaluations of the run: two in the first step (predictor, corrector), one in each later step


@functools.lru_cache(maxsize=None)
def chain_table():
    """The [cond, uncond] eps pair every model evaluation of the chain returns, in call order, and the start x."""
    g = torch.Generator().manual_seed(7777)
    x = torch.randn(CHAIN_N, generator=g) * 3.0
    return x, [(torch.randn(CHAIN_N, generator=g), torch.randn(CHAIN_N, generator=g)) for _ in range(CHAIN_CALLS)]


def chain(cfg, update, x, table, guidance=GUIDANCE):
    """The sequence ``samplers._plms_step`` runs over the five steps: cfg, mode 0, cfg, mode 1, then (cfg, mode 2), (cfg, mode 3),
    (cfg, mode 4), (cfg, mode 4), with the history rotation of plms.py:109-111.  ``cfg(ec, eu, g) -> e`` and
    ``update(x, e_t, old, e_next, mode, a_t, a_prev, s1m) -> x_prev`` are the expressions (or the kernels) under test.
    -> the x after every step."""
    it = iter(table)
    old: list = []
    xs = []
    for i in range(S):
        sc = scalars(S - i - 1)
        e_t = cfg(*next(it), guidance)
        if not old:
            x_pred = update(x, e_t, [], None, 0, *sc)
            e_next = cfg(*next(it), guidance)
            x = update(x, e_t, [], e_next, 1, *sc)
        else:
            x = update(x, e_t, old, None, min(len(old), 3) + 1, *sc)
        old.append(e_t)
        if len(old) >= 4:
            old.pop(0)
        xs.append(x)
    return xs


@functools.lru_cache(maxsize=None)
def chain_want():
    x, table = chain_table()
    return chain(cfg_combine_expr, plms_update_expr, x, table)


# ---- the merge cases -------------------------------------------------------------------------------------------------
MERGE_SHAPES = [(2, 3, 5, 7), (1, 4, 24, 40), (3, 4, 16, 16)]   # 105 elements per image (odd, under one block); fifteen blocks, H != W
MERGE_N_INST = [0, 1, 3, 8]


def merge_boxes(H: int, W: int) -> torch.Tensor:
    """Eight boxes (h0, w0, h1, w1), in this order: two overlapping ones (their common area must hold the later one), an empty one
    (b0 == b2), an inverted one, a one-pixel one, one that reaches past H and W, one that touches the last row and column, one that
    covers the image.  n_inst = 1 takes the first, 3 the first three, 8 all."""
    return torch.tensor([[1, 1, H - 1, W - 2], [H // 2, 0, H, W // 2 + 1], [2, 1, 2, W], [H - 1, W - 1, 1, 1],
                         [H // 2, W // 2, H // 2 + 1, W // 2 + 1], [H - 2, W - 3, H + 5, W + 9], [H - 2, W - 2, H, W],
                         [0, 0, H, W]], dtype=torch.int32)


def merge_boxes_for(n_inst: int, H: int, W: int) -> torch.Tensor:
    """The first n_inst boxes; with all eight the image-covering one moves from the last place to the fourth, so that the boxes
    behind it are seen on top of it and not hidden by it."""
    b = merge_boxes(H, W)
    if n_inst == 8:
        b = b[[0, 1, 2, 7, 3, 4, 5, 6]]
    return b[:n_inst].contiguous()


@functools.lru_cache(maxsize=None)
def merge_lat(n_inst: int, shape) -> torch.Tensor:
    g = torch.Generator().manual_seed(7100 + n_inst + 16 * shape[2])
    lat = torch.randn((n_inst + 1,) + tuple(shape), generator=g)
    flat = lat.view(n_inst + 1, -1)
    m = min(16, flat.shape[1])
    for k in range(n_inst + 1):                                              # the SPECIAL values in front, rotated per instance
        flat[k, :m] = torch.tensor((SPECIAL[k % 16:] + SPECIAL[:k % 16])[:m], dtype=torch.float32)
    return lat
