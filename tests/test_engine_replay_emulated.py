"""The engines' hipGraph replay state across interleaved calls, without a GPU: every UNet and VAE script of tests/replay_cases.py
on the fp32 emulated engines with graphs ON, the graph being the recording double of tests/replay_double.py (a fixed launch list
over fixed storage).  Per call the oracle is a FRESH engine with graphs off given that call's inputs only; equality is
``torch.equal``.  Later visits to a key must be replays, not recaptures, except where the script says the graphs were dropped.

Three deliberately wrong engines (in the spirit of the ``mut`` kernels of tests/attention_cases.py) show that the scripts see the
failures they are for; the real engine passes all of them.
"""
import os
import subprocess
import sys

import pytest
import torch

from instancediffusion_amd.engine import UNetEngine
from tests import replay_cases as rc, replay_double
from tests.test_replay_cases import eager_engine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def graph_engine(kind, tape, cls=None):
    """The emulated engine for ``kind`` with the recording ops and graphs on (the constructor turns them off on a CPU device)."""
    from tests.emul_ops import EmulOps
    from tests.vae_encode_cases import EncEmulOps
    if kind in ("unet_box", "unet_mask"):
        eng = (cls or UNetEngine)(rc.unet_model(kind), ops=replay_double.RecordingOps(EmulOps(torch.float32), tape))
    else:
        from instancediffusion_amd.vae_engine import VAEDecoderEngine, VAEEncoderEngine
        eng = (VAEDecoderEngine if kind == "vae_dec" else VAEEncoderEngine)(
            rc.vae_model(), ops=replay_double.RecordingOps(EncEmulOps(torch.float32), tape))
    assert eng.use_graphs is False
    eng.use_graphs = True
    return eng


def run(script, monkeypatch, cls=None):
    tape = replay_double.install(monkeypatch)
    eng = graph_engine(script.kind, tape, cls)
    captures, replays = rc.run_script(script, eng, lambda: eager_engine(script.kind), tape.counts)
    calls = sum(1 for st in script.steps if st.raises is None)
    assert captures == sum(st.capture for st in script.steps) and replays == calls
    assert tape.syncs == captures and tape.recorded > 0
    print(f"[replay] {script.name}: {calls} calls, {captures} captures, {replays} replays, {tape.recorded} launches recorded")


@pytest.mark.parametrize("name", [s.name for s in rc.UNET_SCRIPTS + rc.VAE_SCRIPTS])
def test_script_replays_equal_fresh_eager_engines(name, monkeypatch):
    run(rc.SCRIPTS[name], monkeypatch)


def test_stale_slot_handle_raises(monkeypatch):
    tape = replay_double.install(monkeypatch)
    rc.stale_handle(graph_engine("unet_box", tape), lambda: eager_engine("unet_box"))
    assert tape.captures == 1 and tape.replays == 3          # the refused call launched nothing


def test_the_double_refuses_an_empty_capture_and_an_allocation_in_a_capture(monkeypatch):
    from instancediffusion_amd import engine_base as engine_mod      # where ``install`` patches capture_graph
    from tests.emul_ops import EmulOps
    tape = replay_double.install(monkeypatch)
    ops = replay_double.RecordingOps(EmulOps(torch.float32), tape)
    with pytest.raises(AssertionError, match="zero launches"):
        with engine_mod.capture_graph(torch.cuda.CUDAGraph()):
            pass
    with pytest.raises(AssertionError, match="inside a graph capture"):
        with engine_mod.capture_graph(torch.cuda.CUDAGraph()):
            ops.empty((2, 2))
    a = torch.ones(2, 2)
    with pytest.raises(AssertionError, match="allocation inside a graph capture"):
        with engine_mod.capture_graph(torch.cuda.CUDAGraph()):
            a + 1
    g, b = torch.cuda.CUDAGraph(), torch.zeros(2, 2)
    with engine_mod.capture_graph(g):
        ops.cast16(a[:1], b[:1])                           # views are free, the op is a launch
        b[1].copy_(a[1])                                   # ... and so is an in-place call of the engine's own
    assert len(g.calls) == 2 and bool((b == 1).all())
    a.fill_(5.0)
    g.replay()                                             # the same launches on the same storage: the new values arrive
    assert bool((b == 5).all()) and tape.counts() == (4, 1)
    with pytest.raises(AssertionError, match="recorded no launch"):
        torch.cuda.CUDAGraph().replay()


def test_clip_and_vae_engines_load_without_the_unet_engine():
    """The shared base lives in ``engine_base``: a fresh interpreter imports the CLIP and VAE engines without ``engine`` (and its
    ``host.unet``), so a value of ``IDF_LN_SELF`` that the UNet engine refuses does not reach them.  Nor does it reach an import of
    ``engine`` itself: the environment is read when a ``UNetEngine`` is constructed (``EngineKnobs.from_env``), and that raises."""
    env = dict(os.environ, IDF_LN_SELF="7", HIP_VISIBLE_DEVICES="-1")
    code = ("import sys, instancediffusion_amd.clip_engine, instancediffusion_amd.vae_engine; "
            "bad = [m for m in ('instancediffusion_amd.engine', 'instancediffusion_amd.host.unet') if m in sys.modules]; "
            "print('loaded:', bad); sys.exit(1 if bad else 0)")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=REPO, env=env)
    assert r.returncode == 0 and "loaded: []" in r.stdout, r.stdout + r.stderr
    code = ("import types, torch, instancediffusion_amd.engine as E\n"
            "from tests.emul_ops import EmulOps\n"
            "print('imported')\n"
            "try:\n"
            "    E.UNetEngine(types.SimpleNamespace(num_heads=8), ops=EmulOps(torch.float32), use_graphs=False)\n"
            "except ValueError as e:\n"
            "    print('refused:', e)\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=REPO, env=env)
    assert r.returncode == 0 and "imported" in r.stdout and "refused: IDF_LN_SELF=7: must be 0, 1 or 2" in r.stdout, r.stdout + r.stderr


# ---- deliberately wrong engines ---------------------------------------------------------------------------------------------------
class BindSkipsCopy(UNetEngine):
    """``_bind`` that marks another cond of the slot's layout as bound without copying it in."""

    def _bind(self, cond):
        slot = self._slots.get(cond.B)
        if slot is not None and cond is not slot and slot.same_layout(cond) and self._slot_bound[cond.B] != cond.uid:
            self._slot_bound[cond.B] = cond.uid
            return slot
        return super()._bind(cond)


class GatherKeepsGraphs(UNetEngine):
    """``gather_cond`` that replaces the slot of a batch size and keeps that batch size's graphs."""

    def gather_cond(self, bank, idx):
        kept = {k: v for k, v in self._graphs.items() if k[0] == int(idx.numel())}
        slot = super().gather_cond(bank, idx)
        self._graphs.update(kept)
        return slot


class BufIgnoresShape(UNetEngine):
    """``buf`` keyed on (role, dtype) alone: a role asked for at another shape gets a new tensor, under graphs captured on the old."""

    def buf(self, role, shape, dtype=None, zero=False):
        dtype = dtype or self.dtype
        shape = tuple(int(s) for s in shape)
        t = self._bufs.get((role, dtype))
        if t is None or tuple(t.shape) != shape:
            t = (self.ops.zeros if zero else self.ops.empty)(shape, dtype)
            self._bufs[(role, dtype)] = t
        return t


@pytest.mark.parametrize("cls,name,what", [
    (BindSkipsCopy, "cond-bind", "cond-bind/B: output 0 differs"),
    (BindSkipsCopy, "keys-return", "keys-return/B1-new: output 0 differs"),
    (GatherKeepsGraphs, "gather", "gather/len3-other-layout: output 0 differs"),
    (BufIgnoresShape, "keys-return", "inside a graph capture"),
])
def test_wrong_engine_fails_its_script(cls, name, what, monkeypatch):
    with pytest.raises(AssertionError, match=what):
        run(rc.SCRIPTS[name], monkeypatch, cls)
