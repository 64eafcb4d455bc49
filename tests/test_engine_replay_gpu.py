"""The engines' hipGraph replay state across interleaved calls on a real MI355X: the scripts of tests/replay_cases.py on ``HipOps`` in
bf16 and fp16 with graphs on.  Per call the oracle is a FRESH engine of the same dtype with ``use_graphs=False``, built from the same
weights and given that call's inputs only; equality is ``torch.equal`` -- no tolerance: the suite already holds replay bitwise equal
to the eager launch sequence, and the kernels' dispatch depends on shapes and knobs, not on addresses.  Every capture is
single-stream.  A test function is one script; tiny variants at the smallest latents only.
"""
import time

import pytest
import torch

from tests import replay_cases as rc, replay_double

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


def engine(kind, dtype, use_graphs=True):
    if kind in ("unet_box", "unet_mask"):
        from instancediffusion_amd.engine import UNetEngine
        return UNetEngine(rc.unet_model(kind), dtype=dtype, use_graphs=use_graphs)
    if kind in ("vae_dec", "vae_enc"):
        from instancediffusion_amd.vae_engine import VAEDecoderEngine, VAEEncoderEngine
        return (VAEDecoderEngine if kind == "vae_dec" else VAEEncoderEngine)(rc.vae_model(), dtype=dtype, use_graphs=use_graphs)
    from tests import clip_cases, clip_vision_cases
    if kind == "clip_text":
        from instancediffusion_amd.clip_engine import CLIPTextEngine
        eng = CLIPTextEngine(clip_cases.tiny_transformer(), dtype=dtype)
    else:
        from instancediffusion_amd.clip_engine import CLIPVisionEngine
        eng = CLIPVisionEngine(clip_vision_cases.tiny_vision(), dtype=dtype)
    eng.max_batch = rc.CLIP_MAX_BATCH
    return eng


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("name", list(rc.SCRIPTS))
def test_script_replays_equal_fresh_eager_engines(name, dtype, monkeypatch):
    script, dt = rc.SCRIPTS[name], DTYPES[dtype]
    tape = replay_double.count_real_graphs(monkeypatch)
    t0 = time.perf_counter()
    eng = engine(script.kind, dt)
    assert getattr(eng, "use_graphs", False) is script.graphs
    captures, replays = rc.run_script(script, eng, lambda: engine(script.kind, dt, use_graphs=False), tape.counts)
    torch.cuda.synchronize()
    calls = sum(1 for st in script.steps if st.raises is None)
    print(f"[replay] {name} {dtype}: {calls} calls, {captures} captures, {replays} replays, {time.perf_counter() - t0:.2f} s")
    if script.graphs:
        assert captures == sum(st.capture for st in script.steps) and replays == calls


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_stale_slot_handle_raises(dtype, monkeypatch):
    tape = replay_double.count_real_graphs(monkeypatch)
    rc.stale_handle(engine("unet_box", DTYPES[dtype]), lambda: engine("unet_box", DTYPES[dtype], use_graphs=False))
    assert tape.counts() == (1, 3)                         # the refused call launched nothing


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_unet_and_vae_engines_called_alternately_in_one_process(dtype, monkeypatch):
    """A UNet engine, a VAE decoder and a VAE encoder live side by side and are called in turn, as inference.py does (encode the
    input image, denoise, decode): each engine's results equal its own fresh eager engine's, and each replays its own graphs."""
    dt = DTYPES[dtype]
    tape = replay_double.count_real_graphs(monkeypatch)
    scripts = [rc.SCRIPTS["vae-encode"], rc.SCRIPTS["keys-return"], rc.SCRIPTS["vae-decode"]]
    envs = [rc.Env(engine(s.kind, dt)) for s in scripts]
    n = 0
    with torch.no_grad():
        for i in range(max(len(s.steps) for s in scripts)):
            for s, env in zip(scripts, envs):
                if i >= len(s.steps):
                    continue
                st = s.steps[i]
                c0 = tape.counts()
                got = rc.outputs(st.run(env))
                c1 = tape.counts()
                want = rc.outputs(st.run(rc.Env(engine(s.kind, dt, use_graphs=False))))
                assert all(torch.equal(a, b) for a, b in zip(got, want)), f"{s.name}/{st.name} among the other engines' calls"
                assert (c1[0] - c0[0], c1[1] - c0[1]) == (st.capture, 1), f"{s.name}/{st.name}"
                n += 1
    assert n == sum(len(s.steps) for s in scripts)
