"""The call scripts of tests/replay_cases.py can detect the failure they are for (no GPU): a stale replay returns an EARLIER call's
result, so every two calls of a script that could be confused -- the same (B, H, W), for the VAE / CLIP scripts the same shapes --
must have expected outputs that differ by more than 3e-3 rel-RMS, the fp16 forward bar of tests/test_engine_gpu.py and the
tightest bar the project holds a forward to: a stale result could then not pass for the right one under any check the project
has.  This is a condition on the scripts' inputs (their seeds and scales), checked on the fp32 emulated engines with graphs off.
"""
import itertools

import pytest
import torch

from tests import cases, replay_cases as rc


def eager_engine(kind):
    """A fresh fp32 emulated engine with graphs off for the script kind."""
    from tests.vae_encode_cases import EncEmulOps
    if kind in ("unet_box", "unet_mask"):
        from instancediffusion_amd.engine import UNetEngine
        from tests.emul_ops import EmulOps
        return UNetEngine(rc.unet_model(kind), ops=EmulOps(torch.float32), use_graphs=False)
    if kind in ("vae_dec", "vae_enc"):
        from instancediffusion_amd.vae_engine import VAEDecoderEngine, VAEEncoderEngine
        return (VAEDecoderEngine if kind == "vae_dec" else VAEEncoderEngine)(rc.vae_model(), ops=EncEmulOps(torch.float32), use_graphs=False)
    from tests import clip_cases, clip_vision_cases
    if kind == "clip_text":
        from instancediffusion_amd.clip_engine import CLIPTextEngine
        eng = CLIPTextEngine(clip_cases.tiny_transformer(), ops=clip_cases.ClipEmulOps(torch.float32))
    else:
        from instancediffusion_amd.clip_engine import CLIPVisionEngine
        eng = CLIPVisionEngine(clip_vision_cases.tiny_vision(), ops=clip_vision_cases.ClipVisionEmulOps(torch.float32))
    eng.max_batch = rc.CLIP_MAX_BATCH
    return eng


def test_every_transition_the_scripts_are_for_is_in_them():
    s = rc.SCRIPTS
    assert [st.group[0] for st in s["keys-return"].steps[:5]] == [1, 2, 3, 1, 2] and s["keys-return"].steps[4].same_as == "B2"
    res = [st.group[1:] for st in s["resolution"].steps]
    assert res[:3] == [(8, 16), (8, 8), (8, 16)] and (16, 8) in res
    assert [st.name.split("#")[0] for st in s["fuser"].steps[:4]] == ["scale1.0", "scale0.0", "scale0.3", "scale1.0"]
    assert [st.name for st in s["paired"].steps[:5]] == ["unpaired", "paired-half", "paired-full-broken", "paired-full", "unpaired-again"]
    assert s["paired"].steps[2].raises is ValueError
    assert sum(st.capture for st in s["cond-bind"].steps) == 5              # A, and four slot replacements
    assert len({st.group[0] for st in s["gather"].steps}) == 2
    assert len(s["forward-cache"].steps) - 2 > 64          # distinct conditionings: all but the cache hit and the last call
    assert all(st.capture == 0 for sc in rc.CLIP_SCRIPTS for st in sc.steps) and not any(sc.graphs for sc in rc.CLIP_SCRIPTS)
    assert s["clip-text"].steps[0].group[0] > 2 * rc.CLIP_MAX_BATCH > 2 * s["clip-text"].steps[1].group[0]


def test_resolution_script_shares_the_zeroed_vt_buffers_between_its_sizes():
    """The property the resolution script is built on (module docstring of tests/replay_cases.py): 8x16 and 8x8 use the same
    zero-initialised ``st.vt`` buffers at the two deeper levels with different token counts, neither a multiple of 64."""
    eng = eager_engine("unet_box")
    env = rc.Env(eng)
    with torch.no_grad():
        for st in rc.SCRIPTS["resolution"].steps[:2]:
            before = {k for k in eng._bufs if k[0] == "st.vt"}
            st.run(env)
            now = {k[1] for k in eng._bufs if k[0] == "st.vt"}
            assert {(2, 128, 64), (2, 256, 64)} <= now
    assert {(2, 128, 64), (2, 256, 64)} <= {k[1] for k in before}, "the 8x8 call was to find its deeper-level st.vt buffers used"
    assert (2, 64, 128) in now and (2, 64, 64) in now              # level 0: 128 and 64 tokens, buffers of their own
    # after the 8x8 call (16 and 4 tokens) the columns behind its tokens hold the 8x16 call's V values, not a fresh engine's zeros
    vt1, vt2 = eng._bufs[("st.vt", (2, 128, 64), torch.float32)], eng._bufs[("st.vt", (2, 256, 64), torch.float32)]
    assert bool((vt1[:, :, 16:32] != 0).any()) and bool((vt2[:, :, 4:8] != 0).any())
    assert not bool(vt1[:, :, 32:].any()) and not bool(vt2[:, :, 8:].any())


@pytest.mark.parametrize("name", list(rc.SCRIPTS))
def test_confusable_calls_have_distinct_expected_outputs(name):
    script = rc.SCRIPTS[name]
    want, shared = {}, None
    with torch.no_grad():
        for st in script.steps:
            if st.raises is not None:
                with pytest.raises(st.raises):
                    st.run(rc.Env(eager_engine(script.kind)))
                continue
            if st.shared_oracle:
                shared = shared or rc.Env(eager_engine(script.kind))
                want[st.name] = rc.outputs(st.run(shared))
            else:
                want[st.name] = rc.outputs(st.run(rc.Env(eager_engine(script.kind))))
            assert all(torch.isfinite(t).all() for t in want[st.name]), st.name
    by_name = {st.name: st for st in script.steps}
    pairs = 0
    for a, b in itertools.combinations(want, 2):
        sa, sb = by_name[a], by_name[b]
        if sa.group != sb.group:
            continue
        if sb.same_as == a or sa.same_as == b:
            assert all(torch.equal(x, y) for x, y in zip(want[a], want[b])), f"{name}: {b} repeats {a}'s inputs"
            continue
        for x, y in zip(want[a], want[b]):
            d = min(cases.rel_rms(x, y), cases.rel_rms(y, x))
            assert d > rc.DIFFER, f"{name}: {a} and {b} could be confused (rel-RMS {d:.2e})"
        pairs += 1
    assert pairs > 0
