"""Call scripts for the engines' replay state (tests/test_replay_cases.py, tests/test_engine_replay_emulated.py,
tests/test_engine_replay_gpu.py).  TEST INFRASTRUCTURE: no GPU, no HIP library.

The engines replay captured hipGraphs over static buffers: ``UNetEngine._graphs`` keyed (B, H, W, fuser_on, paired), one static
``Cond`` slot per batch size that the graphs read by raw pointer, ``_bufs`` shared by every graph of an engine, the ``forward()``
conditioning cache, the VAE engines' ``_replay`` caches and the CLIP engines' per-chunk buffers.  A mistake there does not fault: a
graph replays over a stale pointer or a stale slot and returns the previous call's plausible numbers.  A SCRIPT is a list of calls
on ONE engine that walks those transitions -- back to an earlier key after another one was captured, another resolution on a live
engine, another conditioning layout at one batch size, paired and unpaired calls at one B.  Every call (``Step``) is
self-contained: it builds its inputs from seeds of its own and the objects that must keep their identity across calls (a Cond
handed in twice, the tensors of a ``forward()`` cache hit) live in the per-engine ``Env``, so that the very same step run ALONE
on a fresh engine with graphs off is its oracle.  Equality is bitwise.

Sizes: the reduced-width ``tiny`` variants at the smallest latents their depth allows.  The tiny UNet has four levels (three
stride-2 convs), so H and W are multiples of 8 and the LEVEL-0 token count is always a multiple of 64; the zero-initialised
``st.vt`` buffer whose pad columns are assumed to stay zero is shared at the deeper levels instead: 8x16 gives 32 and 8 tokens at
levels 1 and 2, 8x8 gives 16 and 4, both round up to the same ``st.vt`` shapes (B, 128, 64) / (B, 256, 64), and the 8x8 call that
follows an 8x16 one finds V values in columns where a fresh engine has zeros.
"""
from __future__ import annotations

import dataclasses
import functools
from typing import Callable, List, Optional, Tuple

import torch

from instancediffusion_amd import synth
from tests import cases

DIFFER = 3e-3             # rel-RMS: the fp16 forward bar of tests/test_engine_gpu.py, the tightest one a forward is held to


class Env:
    """The named objects of one engine's run through a script (conds, banks, tensors whose identity matters)."""

    def __init__(self, eng):
        self.eng = eng
        self.dev = eng.device
        self._named = {}

    def get(self, name: str, make: Callable):
        if name not in self._named:
            self._named[name] = make()
        return self._named[name]


@dataclasses.dataclass
class Step:
    name: str
    run: Callable[[Env], object]              # -> tensor or tuple of tensors
    group: tuple                              # calls of one group could be confused: same (B, H, W) / same shapes
    capture: int = 0                          # graphs this call must capture; 0 = a replay of what an earlier call captured
    raises: Optional[type] = None             # the call is an error path: raises before any launch
    same_as: Optional[str] = None             # repeats the inputs of that step on purpose (equal expected output)
    shared_oracle: bool = False               # cache-filling call: its oracle is one eager engine shared among such steps
    post: Optional[Callable[[Env], None]] = None      # check on the engine under test after the call


@dataclasses.dataclass
class Script:
    name: str
    kind: str                                 # which engine: unet_box | unet_mask | vae_dec | vae_enc | clip_text | clip_vision
    steps: List[Step]
    graphs: bool = True                       # False: the engine has static buffers but no graphs (CLIP)


def _g(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def outputs(r) -> Tuple[torch.Tensor, ...]:
    return tuple(t for t in (r if isinstance(r, (tuple, list)) else (r,)) if t is not None)


# ---- models (one per process and kind: weights are key-seeded, engines pack their own copies) ----------------------------------
@functools.lru_cache(maxsize=None)
def unet_model(kind: str):
    from tests.test_engine_emulated import build_model
    if kind == "unet_box":
        return build_model(cases.cfg_for("test_box.yaml", "tiny"))
    assert kind == "unet_mask"
    return build_model(cases.cfg_for("test_mask.yaml", "tiny"), efficient_attention=False)      # Cond.vis is live


@functools.lru_cache(maxsize=None)
def vae_model():
    return cases.build_vae(cases.vae_cfg_for("tiny"))


CLIP_MAX_BATCH = 4        # the scripts run the CLIP engines with this chunk size (the attribute, default 64)


# ---- UNet inputs -----------------------------------------------------------------------------------------------------------------
def latent(env: Env, seed: int, B: int, H: int, W: int):
    g = _g(seed)
    x = torch.randn(B, 4, H, W, generator=g)
    t = torch.randint(1, 1000, (B,), generator=g).float()
    return x.to(env.dev), t.to(env.dev)


def conditioning(seed: int, B: int, n_ctx: int = 77, masked: bool = False):
    """(context [B, n_ctx, 768], grounding dict) on the CPU: three seeded boxes per sample with their text embeddings."""
    g = _g(seed)
    boxes = synth.random_boxes(3, g)
    gb = synth.make_grounding_batch(B, boxes, g, seg_size=64)
    gr = {k: gb[k] for k in ("boxes", "masks", "scribbles", "polygons", "segs", "points")}
    gr["positive_embeddings"] = gb["text_embeddings"]
    if masked:                                             # one box-shaped visibility plane per instance (host/input.py)
        att = torch.zeros(B, gb["boxes"].shape[1], 64, 64)
        for i in range(3):
            x1, y1, x2, y2 = (int(round(float(v) * 64)) for v in boxes[i])
            att[:, i, x1:x2, y1:y2] = 1
        gr["att_masks"] = att
    return torch.randn(B, n_ctx, 768, generator=g), gr


def cond(env: Env, name: str, seed: int, B: int, n_ctx: int = 77, masked: bool = False, strip_vis: bool = False):
    """The Cond ``name`` of this engine (built once: a later step that names it again hands in the same object)."""
    def make():
        ctx, gr = conditioning(seed, B, n_ctx, masked)
        c = env.eng.prepare_cond(ctx.to(env.dev), {k: v.to(env.dev) for k, v in gr.items()})
        if strip_vis:
            c.vis = []                                     # the layout of a conditioning without visibility words
        return c
    return env.get(name, make)


def _fwd(cname, cseed, xseed, B, H, W, *, scale=None, paired=False, half=False, break_pair=False, **ckw):
    def run(env: Env):
        if scale is not None:
            env.eng.set_fuser_scale(scale)
        c = cond(env, cname, cseed, B, **ckw)
        n = B // 2 if paired else B
        x, t = latent(env, xseed, n, H, W)
        if paired and not half:
            x, t = torch.cat([x, x]), torch.cat([t, t])
            if break_pair:
                x[n:] += 1e-3
        return env.eng.forward_cond(x, t, c, paired=paired)
    return run


def _keys_return() -> Script:
    S = (8, 8)
    return Script("keys-return", "unet_box", [
        Step("B1", _fwd("c1", 100, 101, 1, *S), (1, *S), capture=1),
        Step("B2", _fwd("c2", 110, 111, 2, *S), (2, *S), capture=1),
        Step("B3", _fwd("c3", 120, 121, 3, *S), (3, *S), capture=1),
        Step("B1-new", _fwd("c1b", 130, 131, 1, *S), (1, *S)),
        Step("B2-first-again", _fwd("c2", 110, 111, 2, *S), (2, *S), same_as="B2"),
        Step("B3-new", _fwd("c3b", 140, 141, 3, *S), (3, *S)),
    ])


def _resolution() -> Script:
    """8x16 -> 8x8 -> 8x16: see the module docstring for the shared ``st.vt`` buffers; 16x8 is 8x16's transpose (the same element
    counts in every buffer, so the same ``_bufs`` entries wherever the role's shape is flat, under other (H, W))."""
    B = 2
    mk = lambda i, H, W, **kw: Step(f"{H}x{W}#{i}", _fwd(f"c{i}", 200 + 10 * i, 201 + 10 * i, B, H, W), (B, H, W), **kw)
    return Script("resolution", "unet_box", [
        mk(0, 8, 16, capture=1), mk(1, 8, 8, capture=1), mk(2, 8, 16), mk(3, 16, 8, capture=1), mk(4, 8, 16), mk(5, 8, 8),
        mk(6, 16, 8),
    ])


def _fuser() -> Script:
    """Scale 0.3 replays the graph captured at 1.0 with new gate values; 0.0 is another key (the fuser launches are skipped)."""
    k = (1, 8, 8)
    mk = lambda i, s, **kw: Step(f"scale{s}#{i}", _fwd(f"c{i}", 300 + 10 * i, 301 + 10 * i, 1, 8, 8, scale=s), k, **kw)
    return Script("fuser", "unet_box", [mk(0, 1.0, capture=1), mk(1, 0.0, capture=1), mk(2, 0.3), mk(3, 1.0), mk(4, 0.0)])


def _paired() -> Script:
    B, S = 2, (8, 8)
    k = (B, *S)
    return Script("paired", "unet_box", [
        Step("unpaired", _fwd("c0", 400, 401, B, *S), k, capture=1),
        Step("paired-half", _fwd("c1", 410, 411, B, *S, paired=True, half=True), k, capture=1),
        Step("paired-full-broken", _fwd("c2", 420, 421, B, *S, paired=True, break_pair=True), k, raises=ValueError),
        Step("paired-full", _fwd("c3", 430, 431, B, *S, paired=True), k),
        Step("unpaired-again", _fwd("c4", 440, 441, B, *S), k),
        Step("paired-half-again", _fwd("c5", 450, 451, B, *S, paired=True, half=True), k),
    ])


def _cond_bind() -> Script:
    """A, B, A of one layout take the copy path.  A conditioning of another layout at the same B (no visibility words; another
    context length) replaces the slot, so every graph of that B must be dropped and captured again, also on the way back to A."""
    B, S = 1, (8, 8)
    k = (B, *S)
    mk = lambda name, cname, cseed, xseed, cap=0, **ckw: Step(name, _fwd(cname, cseed, xseed, B, *S, masked=True, **ckw), k, capture=cap)
    return Script("cond-bind", "unet_mask", [
        mk("A", "A", 500, 501, 1), mk("B", "B", 510, 511), mk("A-again", "A", 500, 521),
        mk("no-vis", "C", 530, 531, 1, strip_vis=True), mk("A-after-no-vis", "A", 500, 541, 1),
        mk("n_ctx-40", "D", 550, 551, 1, n_ctx=40), mk("A-after-n_ctx", "A", 500, 561, 1), mk("B-again", "B", 510, 571),
    ])


def _gather() -> Script:
    """``gather_cond`` refills of one length replay; another length is another slot; a bank of another layout at a length that
    already has a slot replaces it, so the graphs of that batch size must go."""
    S = (8, 8)

    def step(name, bank, bseed, idx, xseed, cap=0, n_ctx=77):
        def run(env: Env):
            b = cond(env, bank, bseed, 4, n_ctx=n_ctx)
            slot = env.eng.gather_cond(b, torch.tensor(idx, device=env.dev))
            x, t = latent(env, xseed, len(idx), *S)
            return env.eng.forward_cond(x, t, slot)
        return Step(name, run, (len(idx), *S), capture=cap)
    return Script("gather", "unet_box", [
        step("len3", "bank", 600, [0, 1, 3], 601, 1), step("len3-repeated-rows", "bank", 600, [2, 2, 0], 611),
        step("len2", "bank", 600, [3, 1], 621, 1), step("len3-permutation", "bank", 600, [3, 0, 1], 631),
        step("len2-repeated-rows", "bank", 600, [0, 0], 641),
        step("len3-other-layout", "bank40", 650, [1, 3, 3], 651, 1, n_ctx=40),
        step("len3-first-layout", "bank", 600, [1, 2, 3], 661, 1), step("len2-again", "bank", 600, [2, 0], 671),
    ])


FILL = 63                 # forward() keeps 64 conditionings and clears its cache when one more arrives


def _forward_cache() -> Script:
    """The ``model(dict(...))`` entry point, whose conditioning cache is keyed on ``data_ptr`` / ``_version``."""
    k = (1, 8, 8)

    def call(env: Env, ctx, gr, xseed):
        x, t = latent(env, xseed, 1, 8, 8)
        model = env.eng.model
        model._engine = env.eng
        return model(dict(x=x, timesteps=t, context=ctx, grounding_input=gr))

    def tensors(env: Env, name, seed):
        def make():
            ctx, gr = conditioning(seed, 1)
            return ctx.to(env.dev), {k_: v.to(env.dev) for k_, v in gr.items()}
        return env.get(name, make)

    def first(xseed, edit=False):
        def run(env: Env):
            ctx, gr = tensors(env, "A", 700)
            if edit and not env.get("A-edited", lambda: False):
                ctx.copy_(conditioning(705, 1)[0])                         # in place: same data_ptr, _version bumped
                env._named["A-edited"] = True
            return call(env, ctx, gr, xseed)
        return run

    def fresh(i):
        def run(env: Env):
            ctx, gr = tensors(env, f"N{i}", 720 + 3 * i)
            return call(env, ctx, gr, 721 + 3 * i)
        return run

    def cleared_once(env: Env):
        assert len(env.eng._cond_cache) == 2, "the conditioning cache was to be cleared exactly once (the last filler and A are left)"

    steps = [Step("A", first(701), k, capture=1), Step("A-hit", first(702), k), Step("A-edited-in-place", first(703, edit=True), k),
             Step("new-tensors", fresh(0), k)]
    steps += [Step(f"fill{i}", fresh(i), k, shared_oracle=True) for i in range(1, FILL + 1)]
    steps += [Step("A-after-clear", first(704, edit=True), k, post=cleared_once)]
    return Script("forward-cache", "unet_box", steps)


# ---- VAE -------------------------------------------------------------------------------------------------------------------------
def _vae_decode() -> Script:
    """The tiny decoder (two upsamples; the mid attention needs h*w % 64 == 0): keys (1,h,w), (2,h,w), (1,h,2w), (1,h,w) again."""
    def step(name, seed, B, H, W, cap=0):
        def run(env: Env):
            return env.eng.decode((torch.randn(B, 4, H, W, generator=_g(seed)) * 0.18215 * 4.0).to(env.dev))
        return Step(name, run, (B, H, W), capture=cap)
    return Script("vae-decode", "vae_dec", [
        step("1x8x8", 800, 1, 8, 8, 1), step("2x8x8", 801, 2, 8, 8, 1), step("1x8x16", 802, 1, 8, 16, 1), step("1x8x8-again", 803, 1, 8, 8),
        step("2x8x8-again", 804, 2, 8, 8), step("1x8x16-again", 805, 1, 8, 16),
    ])


def _vae_encode() -> Script:
    """The noise flag is part of the key: with, without, with again at one size; a second size and back."""
    from tests.vae_encode_cases import encode_image

    def step(name, seed, H, W, noise, cap=0):
        def run(env: Env):
            x = encode_image(1, H, seed, width=W).to(env.dev)
            n = torch.randn(1, 4, H // 4, W // 4, generator=_g(seed + 50)).to(env.dev) if noise else None
            return env.eng.encode(x, n)
        return Step(name, run, (1, H, W), capture=cap)
    return Script("vae-encode", "vae_enc", [
        step("32-noise", 900, 32, 32, True, 1), step("32-mode", 901, 32, 32, False, 1), step("32-noise-again", 902, 32, 32, True),
        step("32x64-noise", 903, 32, 64, True, 1), step("32-noise-back", 904, 32, 32, True), step("32-mode-back", 905, 32, 32, False),
        step("32x64-noise-again", 906, 32, 64, True),
    ])


# ---- CLIP (static per-chunk buffers, no graphs) -------------------------------------------------------------------------------------
def clip_ids(B: int, seed: int, T: int = 77) -> torch.Tensor:
    """Id rows shaped like the tokenizer's for tests/clip_cases.TINY_CONFIG: 510, word ids, 511 from a seeded position on."""
    g = _g(seed)
    ids = torch.full((B, T), 511, dtype=torch.long)
    ids[:, 0] = 510
    for r in range(B):
        p = int(torch.randint(2, T, (1,), generator=g))
        ids[r, 1:p] = torch.randint(3, 500, (p - 1,), generator=g)
    return ids


def _clip(kind: str) -> Script:
    """A call longer than ``max_batch`` (two whole chunks and a ragged one), one shorter than a chunk, the first one again."""
    n_long, n_short = 2 * CLIP_MAX_BATCH + 1, CLIP_MAX_BATCH - 1

    def step(name, B, seed, **kw):
        def run(env: Env):
            if kind == "clip_text":
                return env.eng.encode_ids(clip_ids(B, seed))
            from tests.clip_vision_cases import TINY_VISION, pixel_values
            return env.eng.encode_pixels(pixel_values(B, TINY_VISION["image_size"], seed))
        return Step(name, run, (B,), **kw)
    return Script(kind.replace("_", "-"), kind, [
        step("long", n_long, 1000), step("short", n_short, 1001), step("long-first-again", n_long, 1000, same_as="long"),
        step("long-new", n_long, 1002), step("short-new", n_short, 1003),
    ], graphs=False)


UNET_SCRIPTS = [_keys_return(), _resolution(), _fuser(), _paired(), _cond_bind(), _gather(), _forward_cache()]
VAE_SCRIPTS = [_vae_decode(), _vae_encode()]
CLIP_SCRIPTS = [_clip("clip_text"), _clip("clip_vision")]
SCRIPTS = {s.name: s for s in UNET_SCRIPTS + VAE_SCRIPTS + CLIP_SCRIPTS}


# ---- the stale slot handle (not a script: the second use of the handle is an error) ------------------------------------------------
def stale_handle(eng, fresh_engine):
    """``slot = gather_cond(..)``, a forward with ANOTHER cond of that batch size, then ``forward_cond(x, t, slot)``: the slot now
    holds the other conditioning, so the engine must raise and name the slot instead of returning the other cond's eps.  A new
    ``gather_cond`` makes the handle good again.  ``fresh_engine()``: a new engine with graphs off, the oracle."""
    import pytest
    env = Env(eng)
    idx = torch.tensor([2, 0], device=env.dev)
    with torch.no_grad():
        bank = cond(env, "bank", 1100, 3)
        slot = eng.gather_cond(bank, idx)
        x, t = latent(env, 1101, 2, 8, 8)
        first = eng.forward_cond(x, t, slot)
        other = eng.forward_cond(*latent(env, 1103, 2, 8, 8), cond(env, "other", 1102, 2))
        with pytest.raises(RuntimeError, match=r"slot of batch size 2 .*overwritten"):
            eng.forward_cond(x, t, slot)
        again = eng.forward_cond(x, t, eng.gather_cond(bank, idx))
        o = Env(fresh_engine())
        want = o.eng.forward_cond(x, t, o.eng.gather_cond(cond(o, "bank", 1100, 3), idx))
    assert torch.equal(first, want) and torch.equal(again, want) and not torch.equal(other, want)


# ---- the runner ----------------------------------------------------------------------------------------------------------------------
def run_script(script: Script, eng, fresh_engine: Callable, counts: Callable[[], Tuple[int, int]]):
    """Run ``script`` on ``eng`` (graphs on).  Per call the oracle is ``fresh_engine()`` -- a NEW engine with graphs off -- given that
    call's inputs only; equality is ``torch.equal``.  ``counts() -> (captures, replays)`` so far: a call must capture exactly
    ``step.capture`` graphs and replay once.  Returns (captures, replays) of the whole script."""
    import pytest
    env, shared = Env(eng), None
    start = counts()
    with torch.no_grad():
        for step in script.steps:
            c0 = counts()
            if step.raises is not None:
                with pytest.raises(step.raises):
                    step.run(env)
                assert counts() == c0, f"{script.name}/{step.name}: an error path must return before any launch"
                continue
            got = outputs(step.run(env))
            c1 = counts()
            if step.post is not None:
                step.post(env)
            if step.shared_oracle:
                shared = shared or Env(fresh_engine())
                want = outputs(step.run(shared))
            else:
                want = outputs(step.run(Env(fresh_engine())))
            assert len(got) == len(want)
            for i, (a, b) in enumerate(zip(got, want)):
                assert a.shape == b.shape and torch.equal(a, b), (
                    f"{script.name}/{step.name}: output {i} differs from a fresh eager engine's on the same inputs "
                    f"(rel-RMS {cases.rel_rms(a.float().cpu(), b.float().cpu()):.3e})")
            if script.graphs:
                assert c1[0] - c0[0] == step.capture, (
                    f"{script.name}/{step.name}: {c1[0] - c0[0]} graph(s) captured, the script expects {step.capture}")
                assert c1[1] - c0[1] == 1, f"{script.name}/{step.name}: {c1[1] - c0[1]} replays in one call"
    end = counts()
    return end[0] - start[0], end[1] - start[1]
