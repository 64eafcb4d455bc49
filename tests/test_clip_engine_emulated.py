"""CPU tests of the CLIP text engine's host logic (weight packing, LayerNorm folding, op sequencing, chunking, the pooled row)
over an fp32 emulation of the op set (tests/clip_cases.ClipEmulOps), against the reference class's golden outputs, and of the
``backend`` switch of ``FrozenCLIPEmbedder``.  The kernels themselves are tested on the GPU (tests/test_clip_engine_gpu.py).
"""
import os

import pytest
import torch

from tests import clip_cases

pytest.importorskip("transformers")

FULL = os.environ.get("IDF_FULL_CPU_SUITE") == "1"


def _engine(tr, **kw):
    from instancediffusion_amd.clip_engine import CLIPTextEngine
    return CLIPTextEngine(tr, ops=clip_cases.ClipEmulOps(torch.float32, **kw))


@pytest.fixture(scope="module")
def tiny():
    return clip_cases.load_golden("clip_engine_tiny"), clip_cases.tiny_transformer()


def test_tiny_golden_is_the_committed_case():
    gold = clip_cases.load_golden("clip_engine_tiny")
    assert torch.equal(gold["input_ids"], clip_cases.tiny_input_ids()) and gold["meta"]["config"] == clip_cases.TINY_CONFIG
    assert tuple(gold["meta"]["eos_positions"]) == clip_cases.TINY_EOS_POSITIONS and gold["meta"]["salt"] == clip_cases.TINY_SALT
    assert float(gold["last_hidden_state"][0].std(0).mean()) > 1e-3, "degenerate golden"
    for case in ("tiny", "clip_text"):
        for dt in ("bf16", "fp16"):
            for out in ("last_hidden_state", "pooler_output"):
                assert 1e-4 < gold["floors"][case][dt][out] < 2e-2


def test_engine_fp32_emulation_matches_reference_tiny(tiny):
    gold, tr = tiny
    z, pooled = _engine(tr).encode_ids(gold["input_ids"])
    ez, ep = clip_cases.rel_rms(z, gold["last_hidden_state"]), clip_cases.rel_rms(pooled, gold["pooler_output"])
    print(f"[parity] CLIP engine, fp32 emulation vs the reference class (tiny): last_hidden_state {ez:.2e}, pooler_output {ep:.2e}")
    assert z.dtype == torch.float32 and tuple(z.shape) == (3, 77, 128) and tuple(pooled.shape) == (3, 128)
    assert ez <= 1e-4 and ep <= 1e-4


@pytest.mark.skipif(not FULL, reason="full-size CLIP-L/14 on the CPU emulation: set IDF_FULL_CPU_SUITE=1 (the GPU parity test covers it)")
def test_engine_fp32_emulation_matches_reference_full_size():
    gold = clip_cases.load_golden("clip_text")
    z, pooled = _engine(clip_cases.full_transformer()).encode_ids(gold["input_ids"])
    ez, ep = clip_cases.rel_rms(z, gold["last_hidden_state"]), clip_cases.rel_rms(pooled, gold["pooler_output"])
    print(f"[parity] CLIP engine, fp32 emulation vs the reference class (full size): last_hidden_state {ez:.2e}, pooler_output {ep:.2e}")
    assert ez <= 1e-4 and ep <= 1e-4


def test_chunking_does_not_change_a_bit(tiny):
    gold, tr = tiny
    eng = _engine(tr, batch_invariant=True)
    assert eng.max_batch == 64
    z64, p64 = eng.encode_ids(gold["input_ids"])
    eng.max_batch = 1
    z1, p1 = eng.encode_ids(gold["input_ids"])
    assert torch.equal(z64, z1) and torch.equal(p64, p1)


def test_pooled_row_is_the_hidden_state_at_the_first_eos(tiny):
    gold, tr = tiny
    eng = _engine(tr)
    z, pooled = eng.encode_ids(gold["input_ids"])
    for r, p in enumerate(clip_cases.TINY_EOS_POSITIONS):
        assert torch.equal(pooled[r], z[r, p])
    # the rule of a config with the real eos id: the FIRST <|endoftext|>, although the padding repeats it and other ids are larger
    eng.eos_token_id = 7
    ids = torch.tensor([[510, 9, 7, 300, 7, 7], [510, 7, 400, 7, 7, 7]])
    assert eng.pooled_index(ids).tolist() == [2, 1]


def test_pad_rows_and_garbage_never_reach_the_outputs(tiny):
    """Static buffers are handed out poisoned (NaN) by the emulation: everything an output reads must have been written."""
    gold, tr = tiny
    z, pooled = _engine(tr).encode_ids(gold["input_ids"][:1])
    assert bool(torch.isfinite(z).all()) and bool(torch.isfinite(pooled).all())


def test_engine_rejects_what_it_cannot_run(tiny):
    gold, tr = tiny
    eng = _engine(tr)
    with pytest.raises(ValueError):
        eng.encode_ids(torch.zeros((1, 78), dtype=torch.long))          # longer than the position table
    with pytest.raises(ValueError):
        eng.encode_ids(torch.zeros((77,), dtype=torch.long))


# ---- the public switch ------------------------------------------------------------------------------------------------
def _wrapper(**kw):
    from ldm.modules.encoders.modules import FrozenCLIPEmbedder
    return FrozenCLIPEmbedder(device="cpu", **kw)


@pytest.fixture(scope="module")
def wrapper_hf():
    return _wrapper(backend="hf")


def test_backend_defaults_to_hf_and_rejects_unknown(monkeypatch, wrapper_hf):
    monkeypatch.delenv("IDF_CLIP_BACKEND", raising=False)
    assert _wrapper().backend == "hf" and wrapper_hf.backend == "hf"
    with pytest.raises(ValueError):
        _wrapper(backend="bogus")


def test_backend_environment_variable_is_honoured(monkeypatch):
    monkeypatch.setenv("IDF_CLIP_BACKEND", "hip")
    assert _wrapper().backend == "hip"
    assert _wrapper(backend="hf").backend == "hf"               # the keyword wins over the environment's default
    monkeypatch.setenv("IDF_CLIP_BACKEND", "bogus")
    with pytest.raises(ValueError):
        _wrapper()


def test_hf_backend_is_the_transformers_call(wrapper_hf):
    """backend="hf": forward is exactly transformer(input_ids) -- last_hidden_state and pooler_output of the module, untouched."""
    enc = wrapper_hf
    ids = torch.randint(0, 49000, (2, 77), generator=torch.Generator().manual_seed(5))
    ids[:, -1] = 49407

    class FixedTokenizer:
        def __call__(self, text, **kw):
            return {"input_ids": ids[:len(text)]}
    enc._tokenizer = FixedTokenizer()
    try:
        want = enc.transformer(input_ids=ids)
        z, pooled = enc.encode(["a", "b"], return_pooler_output=True)
        assert torch.equal(z, want.last_hidden_state) and torch.equal(pooled, want.pooler_output)
        assert torch.equal(enc(["a", "b"]), want.last_hidden_state) and enc._engine is None
    finally:
        enc._tokenizer = None


def test_hip_backend_without_the_engine_raises_instead_of_falling_back(wrapper_hf, monkeypatch):
    import instancediffusion_amd.clip_engine as ce

    def broken(*a, **k):
        raise RuntimeError("libidf_gfx950.so is missing")
    monkeypatch.setattr(ce, "CLIPTextEngine", broken)
    enc = wrapper_hf
    ids = torch.full((1, 77), 49407)

    class FixedTokenizer:
        def __call__(self, text, **kw):
            return {"input_ids": ids}
    enc._tokenizer = FixedTokenizer()
    monkeypatch.setattr(enc, "backend", "hip")
    try:
        with pytest.raises(RuntimeError, match="no fallback"):
            enc.encode(["a"])
    finally:
        enc._tokenizer = None


def test_load_state_dict_drops_the_engine(wrapper_hf):
    enc = wrapper_hf
    enc._engine = object()
    enc.load_state_dict({k: v for k, v in enc.state_dict().items() if "final_layer_norm" in k}, strict=False)
    assert enc._engine is None
