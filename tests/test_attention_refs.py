"""CPU proofs of tests/attention_cases.py, the module tests/test_attention_edges_gpu.py judges the attention kernels with:

* the fp64 references agree with the project's fp32 emulation (tests/emul_ops.py, tests/clip_cases.py, tests/clip_vision_cases.py);
* the fp32 replay of the kernels' arithmetic has NO element outside the per-element bound, on every case the GPU tests run, in both
  storage types, and meets the census bound exactly as stated;
* the bounds reject a list of subtly wrong kernels, each on a named case (``MUTANTS``);
* the mirror of the dispatch rules sends every GPU case to the kernel the case claims to test.

Large cases (the resident-key shapes have 262 000 queries) are proved on a subset of their queries: every query is independent of the
others in the reference, the bound and the replay alike.
"""
import pytest
import torch

from tests import attention_cases as A
from tests.emul_ops import EmulOps

DTS = ["bf16", "fp16"]
FP32_AGREE = 2.0 ** -16                                     # rel-RMS of an fp32 evaluation against the fp64 one: 256 fp32 roundoffs


def unique_attn_dims():
    dims = []
    for fam in A.FAMILIES:
        dims += A.family_cases(fam)
    dims += A.mask_cases() + A.RES_CASES + [A.RES_PLAIN, A.RES_BELOW]
    return list(dict.fromkeys(dims))


def build(dims, dt):
    return A.attn_case(*dims[:6], dt, kind=dims[6], mask=dims[7])


def emul_attention(c, qsel):
    """tests/emul_ops.EmulOps.attention in fp32 on the case (P left unrounded: EmulOps(torch.float32))."""
    f = lambda t: None if t is None else torch.nan_to_num(t.float())
    kw = {}
    if c["n1"]:
        kw.update(k1=f(c["k1"]), vt1=f(c["vt1"]), n1=c["n1"])
    if c.get("qbits") is not None:
        kw.update(qbits=c["qbits"], kbits0=c["kbits0"], kbits1=c["kbits1"])
        qsel = None                                         # the emulation finds a query's own token by its row number
    q = c["q"].float() if qsel is None else c["q"][:, qsel].float()
    return EmulOps(torch.float32).attention(q, f(c["k0"]), f(c["vt0"]), c["n0"], torch.empty(q.shape), c["H"], **kw), qsel


@pytest.mark.parametrize("dt", DTS)
def test_replay_is_inside_the_bound_and_the_reference_agrees_with_the_emulation(dt):
    """Every idf_attention case of the GPU file: 0 elements of the fp32 replay outside the bound; the census inside (u + 2^-21) |want|;
    the fp64 reference equal to EmulOps.attention up to fp32 arithmetic."""
    worst, fails = 0.0, []
    for dims in unique_attn_dims():
        c = build(dims, dt)
        qsel = A.subset(c["nq"]) if c.get("qbits") is None else None
        want, bound = A.attention_ref(c, qsel)
        rep = A.attention_replay(c, qsel)
        bad, ratio = A.outside(rep, want, bound)
        worst = max(worst, ratio)
        if bad or not bool(torch.isfinite(want).all()):
            fails.append((dims, "bound", bad, ratio))
        if dims[6] == "census" and A.outside(rep, want, A.census_bound(want, dt))[0]:
            fails.append((dims, "census bound"))
        emu, _ = emul_attention(c, qsel)
        if A.rel_rms(emu, want) > FP32_AGREE or A.outside(emu, want, bound)[0]:
            fails.append((dims, "emulation", A.rel_rms(emu, want)))
    print(f"[parity] attention replay {dt}: {len(unique_attn_dims())} cases, worst error / bound {worst:.3f}")
    assert not fails, fails[:10]
    assert worst < 1.0


@pytest.mark.parametrize("dt", DTS)
def test_fused_qkv_references_and_replay(dt):
    from tests.clip_cases import causal_attention_ref
    from tests.clip_vision_cases import full_attention_ref
    for (B, T, H, causal, kind) in A.qkv_cases():
        c = A.qkv_case(B, T, H, dt, causal, kind)
        want, bound = A.qkv_attention_ref(c)
        rep = A.qkv_replay(c)
        assert A.outside(rep, want, bound)[0] == 0, (B, T, H, causal, kind)
        if kind == "census":
            assert A.outside(rep, want, A.census_bound(want, dt))[0] == 0, (T, causal)
        other = (causal_attention_ref if causal else full_attention_ref)(torch.nan_to_num(c["qkv"].float()), B, T, H)
        assert A.rel_rms(other, want) <= FP32_AGREE and A.outside(other, want, bound)[0] == 0, (B, T, H, causal)
    c = A.qkv_case(1, 65, 1, dt, True, "census")                                     # the causal mask off by one (j < t)
    want, _ = A.qkv_attention_ref(c)
    assert A.outside(A.qkv_replay(c, off_by_one=True), want, A.census_bound(want, dt))[0] > 0


@pytest.mark.parametrize("dt", DTS)
def test_softmax_rows_reference_and_replay(dt):
    for n in A.SOFTMAX_N:
        for rows in A.SOFTMAX_ROWS:
            c = A.softmax_case(rows, n, dt)
            want, bound = A.softmax_rows_ref(c["s"], c["scale"], dt)
            assert A.outside(A.softmax_rows_replay(c["s"], c["scale"], dt), want, bound)[0] == 0, (rows, n)
            emu = EmulOps(torch.float32).softmax_rows(c["s"].contiguous(), torch.empty(rows, n), c["scale"])
            assert A.rel_rms(emu, want) <= FP32_AGREE
            assert float(want[0, n // 2]) > 0.999 or n == 4                           # the dominant entry takes the row
            wrong = torch.softmax(c["s"].double() * c["scale"] * 1.01, -1)             # a scale off by one per cent
            assert rows == 1 or A.outside(wrong[1:], want[1:], bound[1:])[0] > 0, (rows, n)   # (row 0 is one-hot either way)


# ---- wrong kernels: every one rejected by a named case ---------------------------------------------------------------------------------
CENSUS_ND = [(72, 40), (264, 40), (1208, 40), (4280, 40), (520, 80), (264, 160), (2048, 24)]
TWO_LD = (2, 2, 40, 65, 264, 184, "normal", False)          # ldv0 = 320, ldv1 = 192
SHORT_D = (1, 2, 8, 65, 72, 8, "normal", False)             # d = 8: (d + 8)^-0.5 is 0.71 of the scale
ONE_SEG = (1, 2, 40, 33, 77, 0, "normal", False)            # 51 NaN pad columns behind 77 keys
MASKED = (2, 2, 40, 130, 136, 184, "normal", True)
MASKED_CENSUS = (1, 2, 40, 65, 136, 184, "census", True)
MUTANTS = {                                                 # wrong kernel -> the case whose bound rejects it
    "dropped last key": "census at every (n, d) of CENSUS_ND",
    "dropped 64-key tile": "census at every (n, d) of CENSUS_ND",
    "duplicated first key": "census at every (n, d) of CENSUS_ND",
    "one zero pad key counted": "negative (1, 2, 40, 33, 72 + 8) and (1, 2, 40, 33, 1208 + 0)",
    "scale of the padded head dim": "normal d = 8 (1, 2, 8, 65, 72, 8)",
    "V of head h + 1": "normal (2, 2, 40, 65, 264, 184)",
    "segment-1 V^T with segment 0's leading dimension": "normal (2, 2, 40, 65, 264, 184)",
    "NaN pad times a zero weight": "normal (1, 2, 40, 33, 77, 0)",
    "causal mask off by one": "causal census T = 65 (test_fused_qkv_references_and_replay)",
    "own-token diagonal in segment 1 too": "masked census (1, 2, 40, 65, 136, 184) and masked normal (2, 2, 40, 130, 136, 184)",
    "word-0 query sees unconditional keys": "masked census and masked normal, as above",
    "fp16 kernel rounds P to bf16": "fp16 normal (2, 2, 40, 65, 264, 184): rel-RMS above 2 x the replay's",
}


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n,d", CENSUS_ND)
def test_census_rejects_a_dropped_or_duplicated_key(n, d, dt):
    c = A.attn_case(1, 1, d, 4, n, 0, dt, kind="census")
    want, bound = A.attention_ref(c)
    cb = A.census_bound(want, dt)
    assert A.outside(A.attention_replay(c), want, cb)[0] == 0 and A.outside(A.attention_replay(c), want, bound)[0] == 0
    tile = torch.arange(64, 128) if n >= 128 else torch.arange(0, 64)
    for name, mut in (("last key", dict(drop_keys=torch.tensor([n - 1]))), ("tile", dict(drop_keys=tile)), ("dup", dict(dup_key=0))):
        assert A.outside(A.attention_replay(c, **mut), want, cb)[0] > 0, name


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n0,n1", [(72, 8), (1208, 0)])
def test_negative_scores_reject_a_zero_pad_key(n0, n1, dt):
    c = A.attn_case(1, 2, 40, 33, n0, n1, dt, kind="negative")
    want, bound = A.attention_ref(c)
    assert A.outside(A.attention_replay(c), want, bound)[0] == 0
    wrong = A.attention_replay(c, zero_pad_key=True)
    assert A.outside(wrong, want, bound)[0] > 0 and A.relmax(wrong, want) > 0.9        # the pad key takes the whole softmax


@pytest.mark.parametrize("dt", DTS)
def test_bound_rejects_wrong_scale_head_leading_dimension_and_nan_pad(dt):
    for dims, mut in ((SHORT_D, dict(scale=16 ** -0.5)), (TWO_LD, dict(head_shift=True)), (TWO_LD, dict(vt1_ld0=True)),
                      (ONE_SEG, dict(nan_pad=True))):
        c = build(dims, dt)
        want, bound = A.attention_ref(c)
        assert A.outside(A.attention_replay(c), want, bound)[0] == 0
        assert A.outside(A.attention_replay(c, **mut), want, bound)[0] > 0, mut
    assert build(TWO_LD, dt)["vt0"].shape[-1] != build(TWO_LD, dt)["vt1"].shape[-1]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("dims", [MASKED, MASKED_CENSUS], ids=["normal", "census"])
def test_bound_rejects_wrong_mask_rules(dims, dt):
    c = build(dims, dt)
    want, bound = A.attention_ref(c)
    if dims[6] == "census":
        bound = A.census_bound(want, dt)
    assert A.outside(A.attention_replay(c), want, bound)[0] == 0
    for mut in (dict(diag_seg1=True), dict(word0_sees_all=True)):
        assert A.outside(A.attention_replay(c, **mut), want, bound)[0] > 0, mut


def test_rms_bar_rejects_bf16_p_in_an_fp16_kernel():
    """The excess rounding stays INSIDE the worst-case bound of most elements; the 2 x rel-RMS bar over the replay is what rejects it."""
    c = build(TWO_LD, "fp16")
    want, _ = A.attention_ref(c)
    good, wrong = A.rel_rms(A.attention_replay(c), want), A.rel_rms(A.attention_replay(c, p_type=torch.bfloat16), want)
    print(f"[parity] fp16 replay rel-rms {good:.2e}; with P rounded to bf16 {wrong:.2e} ({wrong / good:.1f} x)")
    assert wrong > A.RMS_FACTOR * good
    # the kernels that do not pre-round Q (32-query, CLIP) are below the replay, never above the bar
    assert A.rel_rms(A.attention_replay(c, prescale=False), want) <= A.RMS_FACTOR * good


@pytest.mark.parametrize("kind", ["first", "overflow"])
def test_fp16_reference_value_above_the_row_maximum_fails_the_bound(kind):
    """What the GPU file found in attention4.hip / attention4w.hip: with the reference value 7 log2 units above the first tile's
    maximum (the largest P at 2^-7), an fp16 query whose first tile holds a spike sums the bulk of its keys as denormals.  Replayed
    here: shift 7 leaves elements outside the bound (measured on the MI355X before the fix: 18 and 11 of 51200, worst error / bound
    2.82 and 2.31 -- the figures this replay gives), shift 0 none; bf16 has the exponent range and passes with 7."""
    c = build((1, 2, 40, 640, 640, 184, kind, False), "fp16")
    want, bound = A.attention_ref(c)
    old, new = A.outside(A.rebase_replay(c, 7.0), want, bound), A.outside(A.rebase_replay(c, 0.0), want, bound)
    print(f"[parity] fp16 {kind}: reference shift 7 -> {old[0]} outside, worst {old[1]:.2f}; shift 0 -> {new[0]} outside, worst {new[1]:.2f}")
    assert old[0] > 0 and new[0] == 0
    cb = build((1, 2, 40, 640, 640, 184, kind, False), "bf16")
    wb, bb = A.attention_ref(cb)
    assert A.outside(A.rebase_replay(cb, 7.0), wb, bb)[0] == 0


def test_every_mutant_names_its_case():
    assert len(MUTANTS) == 12 and all(MUTANTS.values())


# ---- the dispatch mirror -----------------------------------------------------------------------------------------------------------------
def test_dispatch_mirror_sends_every_case_to_the_kernel_it_claims():
    for fam, (a2, a8, kernel, ds) in A.FAMILIES.items():
        for (B, H, d, nq, n0, n1, kind, mask) in A.family_cases(fam):
            got = A.dispatch(d, nq, n0, n1, B, H, attn2=a2, attn8=a8, mask=mask)
            assert got["kernel"] == kernel, (fam, B, H, d, nq, n0, n1, got)
            assert d in ds
    for (B, H, d, nq, n0, n1, kind, mask) in A.mask_cases():
        for a2, a8 in ((0, 0), (5, 1)):                                           # a mask goes to the 32-query kernel whatever the knobs
            assert A.dispatch(d, nq, n0, n1, B, H, attn2=a2, attn8=a8, mask=True)["kernel"] == "attn32_mask"
    for dims in A.RES_CASES + [A.RES_PLAIN]:
        B, H, d, nq, n0, n1 = dims[:6]
        got = A.dispatch(d, nq, n0, n1, B, H, attn2=0, attn8=0)
        assert got == dict(kernel="attn32_res", qb=256, counter="res"), dims
        nqb = -(-nq // 128)
        assert 2048 <= B * H * nqb < 3072 and -(-n0 // 64) + -(-n1 // 64) == 2 and nqb % 2 == 1
    nqb = -(-A.RES_NQ // 128)
    assert A.RES_NQ % 128 == 5 and (4 * 4 * -(-nqb // 2)) % 8 == 0                       # the remap is on at 1040 workgroups ...
    nqb_plain = -(-A.RES_PLAIN[3] // 128)
    assert nqb_plain % 2 == 1 and (3 * 3 * -(-nqb_plain // 2)) % 8 != 0                    # ... and off at RES_PLAIN's 1035
    B, H, d, nq, n0, n1 = A.RES_BELOW[:6]
    assert A.dispatch(d, nq, n0, n1, B, H, attn2=0, attn8=0)["kernel"] == "attn32" and B * H * -(-nq // 128) < 2048


def test_dispatch_mirror_workgroup_sizes_and_gates():
    D = A.dispatch
    assert [D(40, 600, 64, 8, 1, 1, attn2=m, attn8=0)["qb"] for m in (1, 2, 3, 4, 5)] == [256, 512, 256, 512, 256]
    assert [D(40, 600, 64, 8, 1, 1, attn2=m, attn8=0)["kernel"] for m in (1, 4, 5, 6)] == ["attn4", "attn4w", "attn4w", "attn4"]
    assert [D(24, 600, 64, 8, 1, 1, attn2=m, attn8=0)["kernel"] for m in (4, 5)] == ["attn4", "attn4"]     # other head dims run as mode 1
    assert [D(80, 600, 64, 8, 1, 1, attn2=0, attn8=m)["qb"] for m in (1, 2, 3, 4, 5, 6)] == [128, 256, 128, 128, 128, 256]
    assert [D(160, 600, 64, 8, 1, 1, attn2=0, attn8=m)["qb"] for m in (1, 2, 3, 4, 5, 6)] == [256, 256, 256, 128, 256, 256]
    assert [D(160, nq, 64, 8, 1, 1, attn2=0, attn8=1)["qb"] for nq in (255, 256)] == [128, 256]
    assert D(160, 255, 64, 8, 1, 1, attn2=0, attn8=2)["qb"] == 256
    for kw in (dict(ldo=84), dict(so=88 * 5 + 4)):                                  # ldo % 8 == 4; an unaligned batch stride
        assert D(40, 64, 64, 8, 2, 2, attn2=5, attn8=1, **kw)["kernel"] == "attn32"
        assert D(80, 64, 64, 8, 2, 1, attn2=5, attn8=1, **kw)["kernel"] == "attn32"
    for n0, n1 in ((77, 8), (72, 5)):                                               # n % 8 != 0 in either segment
        assert D(40, 64, n0, n1, 1, 2, attn2=1, attn8=1)["kernel"] == "attn32"
        assert D(160, 64, n0, n1, 1, 2, attn2=1, attn8=1)["kernel"] == "attn32"
    assert D(80, 64, 64, 8, 1, 2, attn2=5, attn8=0)["kernel"] == "attn32"
    assert D(40, 64, 64, 8, 1, 2, attn2=0, attn8=1)["kernel"] == "attn32"
    # the resident-key rule: tiles <= 2, at least two query blocks, qpw = clamp(blocks / 1024, 1, 8) > 1
    assert D(40, 128 * 128, 77, 0, 4, 4, attn2=0, attn8=0) == dict(kernel="attn32_res", qb=256, counter="res")
    assert D(40, 128 * 128, 129, 0, 4, 4, attn2=0, attn8=0)["kernel"] == "attn32"    # three key tiles
    assert D(40, 128 * 128, 64, 65, 4, 4, attn2=0, attn8=0)["kernel"] == "attn32"    # 1 + 2 tiles
    assert D(40, 128, 77, 0, 64, 64, attn2=0, attn8=0)["kernel"] == "attn32"         # one query block per head
    assert D(40, 128 * 1024, 77, 0, 4, 4, attn2=0, attn8=0)["qb"] == 128 * 8         # qpw clamps at 8


def test_unsupported_head_dims_are_classified():
    for d in A.UNSUPPORTED_D:
        for a2, a8, mask in ((0, 0, False), (5, 1, False), (5, 1, True)):
            assert A.dispatch(d, 64, 64, 8, 1, 1, attn2=a2, attn8=a8, mask=mask)["kernel"] == "unsupported"
    for d in A.SUPPORTED_D:
        assert A.dispatch(d, 64, 64, 8, 1, 1, attn2=0, attn8=0)["kernel"] == "attn32"
    assert sorted(A.SUPPORTED_D + A.UNSUPPORTED_D) == list(range(8, 161, 8))
