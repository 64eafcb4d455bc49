"""A recording stand-in for ``torch.cuda.CUDAGraph`` + ``engine_base.capture_graph`` -- TEST DOUBLE ONLY, installed per test with
``monkeypatch`` -- so that the engines' replay state machine (``_bind``, ``_graphs``, ``_bufs``, ``EngineBase._replay``) runs on a
machine without a GPU.  ``_replay`` is the one place that captures, so ``engine_base`` is the one module patched.

What a hipGraph is for this purpose: a fixed launch list over fixed storage.  While "capturing", every ``EmulOps`` method the
engine calls is recorded with its argument tensors BY REFERENCE (the ops still execute), and so is every in-place torch call the
engine issues between ops (``_dup``'s copies: kernels of the real graph too).  ``replay()`` re-issues the recorded calls on those
same tensors.  A graph that was captured over a buffer the engine has since replaced therefore reads and writes the orphaned
storage and returns the previous numbers, exactly as a hipGraph would.

The double fails the test when a capture records nothing, when anything allocates inside a capture (``ops.empty`` / ``ops.zeros``,
or a torch call of the engine's whose result is new storage: the real graph would allocate on every replay, or keep a pointer
into memory the allocator hands out again), and when a capture is nested.  It counts captures, replays and synchronisations.
"""
from __future__ import annotations

import contextlib

import torch
from torch.utils._python_dispatch import TorchDispatchMode
from torch.utils._pytree import tree_leaves

_PURE = {"mlp_supported", "mlp_pack", "gn_partial_shape"}          # shape / packing helpers: no launch


class Tape:
    def __init__(self):
        self.capturing = None          # the FakeGraph being recorded
        self.depth = 0                 # > 0 inside an op (its own torch calls are the op's business)
        self.captures = self.replays = self.syncs = self.recorded = 0

    def counts(self):
        return self.captures, self.replays


class FakeGraph:
    def __init__(self, tape: Tape):
        self.tape = tape
        self.calls = []

    def replay(self):
        tape = self.tape
        assert tape.capturing is None, "replay inside a capture"
        assert self.calls, "replay of a graph that recorded no launch"
        tape.replays += 1
        tape.depth += 1
        try:
            for fn, args, kwargs in self.calls:
                fn(*args, **kwargs)
        finally:
            tape.depth -= 1


class _Watch(TorchDispatchMode):
    """The engine's own torch calls inside a capture: in-place ones are launches of the graph, views are free, anything that
    returns new storage is an allocation."""

    def __init__(self, tape: Tape, graph: FakeGraph):
        super().__init__()
        self.tape, self.graph = tape, graph

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        out = func(*args, **kwargs)
        if self.tape.depth == 0:
            if func._schema.is_mutable:
                self.graph.calls.append((func, args, kwargs))
            else:
                have = {t.untyped_storage().data_ptr() for t in tree_leaves((args, kwargs)) if isinstance(t, torch.Tensor)}
                for t in tree_leaves(out):
                    if isinstance(t, torch.Tensor) and t.untyped_storage().data_ptr() not in have:
                        raise AssertionError(f"allocation inside a graph capture: {func}")
        return out


class RecordingOps:
    """Proxy around an ``EmulOps``: the same op set, every launch recorded into the graph that is being captured."""

    def __init__(self, inner, tape: Tape):
        self.__dict__["_inner"] = inner
        self.__dict__["_tape"] = tape

    def __setattr__(self, name, value):
        setattr(self._inner, name, value)

    def __getattr__(self, name):
        attr = getattr(self._inner, name)              # AttributeError for an op the emulation lacks, as ``hasattr`` needs
        if not callable(attr) or name.startswith("_") or name in _PURE:
            return attr
        tape = self._tape
        if name in ("empty", "zeros"):
            def alloc(*a, **k):
                assert tape.capturing is None, f"ops.{name} inside a graph capture: the eager warm-up was to size every buffer"
                return attr(*a, **k)
            return alloc

        def launch(*a, **k):
            if tape.capturing is not None and tape.depth == 0:
                tape.capturing.calls.append((attr, a, k))
                tape.recorded += 1
            tape.depth += 1
            try:
                return attr(*a, **k)
            finally:
                tape.depth -= 1
        return launch


def install(monkeypatch) -> Tape:
    """Route graph construction, capture and ``torch.cuda.synchronize`` of ``EngineBase._replay`` to the double."""
    from instancediffusion_amd import engine_base
    tape = Tape()

    @contextlib.contextmanager
    def capture_graph(graph):
        assert isinstance(graph, FakeGraph) and tape.capturing is None, "nested capture"
        tape.capturing = graph
        tape.captures += 1
        try:
            with _Watch(tape, graph):
                yield
        finally:
            tape.capturing = None
        assert graph.calls, "a capture recorded zero launches"

    def synchronize(*a, **k):
        tape.syncs += 1

    monkeypatch.setattr(engine_base, "capture_graph", capture_graph)
    monkeypatch.setattr(torch.cuda, "CUDAGraph", lambda: FakeGraph(tape))
    monkeypatch.setattr(torch.cuda, "synchronize", synchronize)
    return tape


def count_real_graphs(monkeypatch) -> Tape:
    """On the GPU: the real capture and replay, counted (``Tape.counts()``)."""
    from instancediffusion_amd import engine_base
    tape = Tape()
    real_capture, real_replay = engine_base.capture_graph, torch.cuda.CUDAGraph.replay

    @contextlib.contextmanager
    def capture_graph(graph):
        tape.captures += 1
        with real_capture(graph):
            yield

    def replay(self):
        tape.replays += 1
        return real_replay(self)

    monkeypatch.setattr(engine_base, "capture_graph", capture_graph)
    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", replay)
    return tape
