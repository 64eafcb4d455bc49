"""Proves tests/shadow_ops.py on the CPU (no GPU, no HIP library), the way tests/test_gemm_conv_refs.py proves tests/gemm_conv_cases.py:

  * the forms the judge evaluates on sampled rows equal the project's references (the tap gather against ``conv3x3_ref`` for stride 1 / 2,
    up 0 / 1, pad_lo 0 / 1; the phase convolutions against the upsampled 3x3 conv; the loop-free patch layouts; the GEGLU unpacking);
  * the row sampler keeps its promises;
  * the emulation passes: every launch of the tiny UNet (mask, scribble, the paired forward), VAE and CLIP engines over ``EmulOps`` is inside
    its bound at the fp16 table, nothing is written beside a view, and what passes unjudged is exactly the allow-list;
  * a wrong launch is caught AT that launch: an inner ops that is wrong in exactly one launch fails the judge at that index and at no
    earlier one, for each way a launch can be wrong that the judge claims to see;
  * with ``conv_up2x`` / ``conv3x3_skip`` doubles (written here from the pack functions' documented layouts) a forward on the CPU takes the
    engine's ``up_fold`` and ``skip_fold`` paths and still meets the golden at the 3e-4 of tests/test_engine_emulated.py.
fp32 storage is judged at the fp16 table: bf16 matmuls on the CPU take minutes, and every adapter -- unpacking, views, aliasing,
sampling -- is exercised all the same.
"""
import dataclasses

import pytest
import torch
import torch.nn.functional as F

from instancediffusion_amd.engine import Cond, EngineKnobs, UNetEngine, pack_conv_up2x, pack_geglu
from grounding_input.text_grounding_tokinzer_input import GroundingNetInput
from tests import cases
from tests import gemm_conv_cases as K
from tests import shadow_ops as SO
from tests import small_kernel_cases as SK
from tests import vae_encode_cases as vc
from tests.emul_ops import EmulOps
from tests.shadow_ops import LaunchOutside, ShadowOps
from tests.test_engine_emulated import build_model

UNET_ALLOW = {"empty", "zeros", "gn_partial_shape", "mlp_supported"}


class EmulPlus(vc.EncEmulOps):
    """The emulation plus the two doubles it lacked.  Both are written from the documented layouts (``engine.pack_conv_up2x``,
    ``engine.pack_conv3x3_skip``), not from the kernels or the judge."""

    def conv_up2x(self, x, wf, out, *, bias=None):
        self._count("conv_up2x")
        B, H, W_, Cin = x.shape
        Cout = wf.shape[1]
        xp = F.pad(x.float().permute(0, 3, 1, 2), (1, 1, 1, 1))
        for py in range(2):
            for px in range(2):
                k = wf[py * 2 + px].float().reshape(Cout, 2, 2, Cin).permute(0, 3, 1, 2)
                y = F.conv2d(xp, k)                                       # [B, Cout, H + 1, W + 1]: window origin (y - 1, x - 1)
                y = y[:, :, py:py + H, px:px + W_]
                if bias is not None:
                    y = y + bias.view(1, -1, 1, 1)
                out[:, py::2, px::2] = y.permute(0, 2, 3, 1).to(out.dtype)
        return True

    def conv3x3_skip(self, g2, w_packed, x, out, *, bias=None, gn_partial=None):
        self._count("conv3x3_skip")
        C2 = g2.shape[-1]
        xs = x.float() @ w_packed[:, 9 * C2:].float().t()
        self.conv3x3(g2, w_packed[:, :9 * C2], out, bias=bias, res=xs, gn_partial=gn_partial)
        return True


# ---- the forms the judge evaluates equal the references ----------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("up", [0, 1])
@pytest.mark.parametrize("pad_lo", [0, 1])
def test_tap_gather_equals_conv3x3_ref(stride, up, pad_lo):
    B, H, W_, Cin, Cout = 2, 5, 6, 8, 7
    x, w = SK.gen((B, H, W_, Cin), 1).half(), SK.gen((Cout, 9 * Cin), 2, 0.1).half()
    Ho, Wo = K.conv_out_hw(H, W_, stride, up, pad_lo)
    kw = dict(bias=SK.gen((Cout,), 3), rowbias=SK.gen((B, Cout), 4).half(), res=SK.gen((B, Ho, Wo, Cout), 5).half())
    want, slack = K.conv3x3_ref(x, w, stride=stride, up=up, pad_lo=pad_lo, **kw)
    rows = torch.arange(B * Ho * Wo)
    got, gslack = SO.conv_rows_ref(x, w, rows, stride=stride, up=up, pad_lo=pad_lo, **kw)
    assert float((got - want.reshape(-1, Cout)).abs().max()) <= 1e-13 * float(want.abs().max())
    assert float((gslack - slack.reshape(-1, Cout)).abs().max()) <= 1e-13 * float(slack.abs().max())
    some = torch.tensor([0, 3, B * Ho * Wo - 1])
    assert torch.equal(SO.conv_rows_ref(x, w, some, stride=stride, up=up, pad_lo=pad_lo, **kw)[0], got[some])


def test_phase_convs_equal_the_upsampled_conv():
    """Integer weights: the fold's sums are exact, so the four phase convolutions equal conv3x3(nearest-x2(x)) to fp64 rounding."""
    B, H, W_, Cin, Cout = 2, 3, 4, 8, 5
    w4 = torch.randint(-2, 3, (Cout, Cin, 3, 3), generator=torch.Generator().manual_seed(6)).float()
    x, bias = SK.gen((B, H, W_, Cin), 7).half(), SK.gen((Cout,), 8)
    want, _ = K.conv3x3_ref(x, w4.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin), bias=bias, up=1)
    got, slack = SO.conv_up2x_rows_ref(x, pack_conv_up2x(w4), torch.arange(B * 4 * H * W_), bias)
    assert float((got - want.reshape(-1, Cout)).abs().max()) <= 1e-13 * float(want.abs().max())
    assert bool((slack > 0).all()) and float(slack.max()) < 1e-3
    dbl = EmulPlus(torch.float32)                            # the double agrees with the same reference
    out = torch.empty(B, 2 * H, 2 * W_, Cout)
    assert dbl.conv_up2x(x.float(), pack_conv_up2x(w4), out, bias=bias) is True
    assert float((out.double() - want).abs().max()) <= 1e-5 * float(want.abs().max())


def test_loop_free_layouts_equal_the_references():
    inp = SK.lnp_inputs((2, 4, 6, 8), "fp16")
    assert torch.equal(SO.layernorm_patch2_fast(inp["x"], inp["gamma"], inp["beta"], SK.LN_EPS), SK.lnp_want(inp))
    seg = SK.seg_inputs((2, 5, 8, 64))
    assert float((SO.seg_in_conv_fast(seg["segs"], seg["w"], seg["bias"]) - SK.seg_want(seg)).abs().max()) <= 1e-13
    w, b = SK.gen((128, 4), 9), SK.gen((128,), 10)
    for period in (32, 64):
        wp, bp = pack_geglu(w, b, period)
        assert torch.equal(SO.unpack_geglu(wp, period), w) and torch.equal(SO.unpack_geglu(bp, period), b)


def test_reference_edits_keep_their_values():
    """``groupnorm_ref(stats=)`` with x's own statistics is ``groupnorm_ref``; merged conv partials are those statistics; ``gemm_ref``'s
    row-bias index is what it was."""
    inp = SK.gn_inputs((2, 128, 64), "fp16")
    x = inp["x"]
    xd = x.double().view(2, 128, 32, 2)
    mu = xd.mean(dim=(1, 3))
    var = (xd - mu[:, None, :, None]).pow(2).mean(dim=(1, 3))
    want = SK.groupnorm_ref(x, inp["gamma"], inp["beta"], 1e-5, True)
    assert float((SK.groupnorm_ref(x, inp["gamma"], inp["beta"], 1e-5, True, stats=(mu, var)) - want).abs().max()) <= 1e-12
    part = torch.empty(2, 2, 32, 2)
    EmulPlus(torch.float32).conv3x3(torch.zeros(2, 8, 16, 64), torch.zeros(64, 576), x.float().view(2, 8, 16, 64).clone(), res=x.float().view(2, 8, 16, 64),
                                    gn_partial=part)
    m2, v2 = SO.gn_stats_from_partial(part, 128, 64)
    assert float((m2 - mu).abs().max()) < 1e-5 and float((v2 / var - 1).abs().max()) < 1e-4
    case = K.gemm_case(130, 136, 128, "fp16", "bias_rowbias")
    want, _ = K.gemm_want(case)
    idx = torch.arange(130) // 50
    plain = case["a"].double() @ case["w"].double().t() + case["kw"]["bias"].double() + case["kw"]["rowbias"].double()[idx]
    assert torch.equal(want, plain)


def test_row_sampler():
    assert SO.sample_rows(1024, 1024, 0) is None
    border = SO.conv_border_rows(3, 40, 40)
    rows = SO.sample_rows(4800, 1024, 5, batch_rows=1600, border=border)
    got = set(rows.tolist())
    assert rows.numel() == 1024 and len(got) == 1024 and rows.tolist() == sorted(got)
    assert set(range(64)) <= got and set(range(4800 - 64, 4800)) <= got and border <= got
    assert len(border) == 2 * (4 * 40 - 4) and (2 * 1600 + 7 * 40 + 39) in border and (1600 + 39) not in border
    assert torch.equal(rows, SO.sample_rows(4800, 1024, 5, batch_rows=1600, border=border))          # seeded
    many = SO.sample_rows(64 * 300, 1024, 1, batch_rows=300)                                          # 64 batch entries: one row of each
    assert {int(r) // 300 for r in many.tolist()} == set(range(64))
    assert SO.sample_rows(9000, 1024, 2, border=set(range(100, 700))).numel() == 1024                 # 600 border rows: too many, left out


# ---- the emulation passes --------------------------------------------------------------------------------------------------------------
_MODELS = {}


def tiny(tag):
    if tag not in _MODELS:
        gold = cases.load_golden(tag)
        meta = gold["meta"]
        _MODELS[tag] = (gold, cases.build_inputs(meta), build_model(cases.cfg_for(meta["cfg"], meta["variant"])))
    return _MODELS[tag]


def shadow_engine(model, inner=None, **kw):
    sh = ShadowOps(inner or EmulPlus(torch.float32), "fp16", **kw)
    eng = UNetEngine(model, ops=sh, use_graphs=False)
    sh.engine = eng
    return sh, eng


def clean(sh, allow, what):
    sh.print_summary(what)
    assert not sh.failures(), sh.line(sh.failures()[0])
    assert sh.passed == allow, sh.passed
    assert all(p["outside"] == 0 for r in sh.records for p in r["parts"]) and all(r["stray"] == 0 for r in sh.records)


@pytest.mark.parametrize("tag", ["tiny_mask", "tiny_scribble"])
def test_emulated_unet_passes_and_takes_the_folded_paths(tag):
    """prepare_cond + forward, every launch judged; with the doubles the forward takes ``conv_up2x`` and ``conv3x3_skip`` and still meets
    the golden at 3e-4."""
    gold, inp, model = tiny(tag)
    sh, eng = shadow_engine(model)
    assert hasattr(sh, "conv_up2x") and hasattr(sh, "conv3x3_skip") and not hasattr(ShadowOps(EmulOps(torch.float32), "fp16"), "conv_up2x")
    with torch.no_grad():
        cond = eng.prepare_cond(inp["context"], GroundingNetInput().prepare(inp["gb"]))
        eps = eng.forward_cond(inp["x"], inp["t"], cond)
    clean(sh, UNET_ALLOW, tag)
    ops = {r["op"] for r in sh.records}
    assert {"gemm", "conv3x3", "conv3x3_skip", "conv_up2x", "attention", "groupnorm", "layernorm", "scaleu_concat", "conv_in", "cast16",
            "timestep_embedding", "unifusion_embed", "seg_in_conv", "dwconv7x7", "layernorm_patch2"} <= ops
    assert all(sh.returned["conv_up2x"]) and all(sh.returned["conv3x3_skip"])
    flags = {r["flags"] for r in sh.records if r["op"] == "gemm"}
    assert any("vt_out" in f and "ln_stats_out" in f for f in flags) and any("ln_col" in f for f in flags)
    assert any("gate" in f and "res" in f for f in flags) and any("geglu32" in f for f in flags)
    assert any("gn_partial" in r["flags"] for r in sh.records if r["op"] == "conv3x3_skip")
    assert any("partial" in r["flags"] for r in sh.records if r["op"] == "groupnorm")
    assert cases.rel_rms(eps, gold["eps_cond"]) < 3e-4


def test_emulated_paired_forward_passes():
    gold, inp, model = tiny("tiny_mask")
    sh, eng = shadow_engine(model)
    eng.knobs = dataclasses.replace(eng.knobs, pair_hoist=True)
    gi = GroundingNetInput()
    with torch.no_grad():
        pair = Cond.cat([eng.prepare_cond(inp["context"], gi.prepare(inp["gb"])), eng.prepare_cond(inp["uc"], gi.get_null_input(batch=1))])
        both = eng.forward_cond(inp["x"], inp["t"], pair, paired=True)
    clean(sh, UNET_ALLOW, "paired")
    assert cases.rel_rms(both[:1], gold["eps_cond"]) < 3e-4 and cases.rel_rms(both[1:], gold["eps_uncond"]) < 3e-4


def test_emulated_vae_passes():
    from instancediffusion_amd.vae_engine import VAEDecoderEngine, VAEEncoderEngine
    gold = cases.load_golden("vae_tiny")
    meta = gold["meta"]
    sh = ShadowOps(EmulPlus(torch.float32), "fp16")
    eng = VAEDecoderEngine(cases.build_vae(cases.vae_cfg_for(meta["variant"]), meta["salt"]), ops=sh, use_graphs=False)
    sh.engine = eng
    with torch.no_grad():
        img = eng.decode(cases.vae_latent(meta))
    clean(sh, {"empty"}, "vae decode")
    assert {"pointwise_nchw", "conv_in", "softmax_rows", "gemm", "conv3x3", "groupnorm"} <= {r["op"] for r in sh.records}
    assert cases.rel_rms(img, gold["img"]) < 3e-4
    ae, x, egold = vc.build("vae_enc_tiny")
    sh = ShadowOps(EmulPlus(torch.float32), "fp16")
    enc = VAEEncoderEngine(ae, ops=sh, use_graphs=False)
    sh.engine = enc
    E = egold["moments"].shape[1] // 2
    with torch.no_grad():
        z, moments = enc.encode(x, SK.gen(tuple(egold["moments"][:, :E].shape), 11))
    clean(sh, {"empty"}, "vae encode")
    assert {"conv3x3_down", "vae_posterior"} <= {r["op"] for r in sh.records}
    assert cases.rel_rms(moments, egold["moments"]) < 3e-4


def test_emulated_clip_passes():
    pytest.importorskip("transformers")
    from instancediffusion_amd.clip_engine import CLIPTextEngine, CLIPVisionEngine
    from tests import clip_cases
    from tests import clip_vision_cases as cv
    gold = clip_cases.load_golden("clip_engine_tiny")
    sh = ShadowOps(cv.ClipVisionEmulOps(torch.float32), "fp16")
    eng = CLIPTextEngine(clip_cases.tiny_transformer(), ops=sh)
    sh.engine = eng
    z, _ = eng.encode_ids(gold["input_ids"])
    clean(sh, {"empty"}, "clip text")
    assert {"clip_embed", "attention_causal", "gemm", "layernorm"} <= {r["op"] for r in sh.records}
    assert clip_cases.rel_rms(z, gold["last_hidden_state"]) <= 1e-4
    sh = ShadowOps(cv.ClipVisionEmulOps(torch.float32), "fp16")
    ve = CLIPVisionEngine(cv.tiny_vision(), ops=sh)
    sh.engine = ve
    ve.encode_pixels(cv.pixel_values(3, 56))
    clean(sh, {"empty"}, "clip vision")
    assert {"clip_patchify", "attention_qkv", "gemm", "layernorm"} <= {r["op"] for r in sh.records}


# ---- a wrong launch is caught at that launch ---------------------------------------------------------------------------------------------
class Mutant:
    """An ops object that is ``inner`` but for launch ``at`` (counted over the judged ops, as the judge counts), where ``kind`` applies."""

    def __init__(self, inner, at, kind):
        self.__dict__.update(inner=inner, at=at, kind=kind, n=0)

    def __getattr__(self, name):
        attr = getattr(self.__dict__["inner"], name)
        if name not in SO.JUDGED:
            return attr

        def call(*a, **k):
            i = self.n
            self.__dict__["n"] = i + 1
            return attr(*a, **k) if i != self.at else getattr(self, "_m_" + self.kind)(attr, a, k)
        return call

    def _m_no_bias(self, op, a, k):
        return op(*a, **dict(k, bias=torch.zeros_like(k["bias"])))

    def _m_no_gate(self, op, a, k):
        return op(*a, **dict(k, gate=torch.ones_like(k["gate"])))

    def _m_vt_untransposed(self, op, a, k):
        ret = op(*a, **k)
        vt, M = k["vt_out"], a[0].shape[0]
        vt[:, :M] = vt[:, :M].t().contiguous().view(vt.shape[0], M)
        return ret

    def _m_conv_origin(self, op, a, k):
        return op(torch.roll(a[0], 1, dims=2), *a[1:], **k)

    def _m_pad_key(self, op, a, k):
        q, k0, vt0, n0 = a[:4]
        k0p = torch.cat([k0[:, :n0], torch.zeros_like(k0[:, :1])], 1)
        return op(q, k0p, vt0, n0 + 1, *a[4:], **k)

    def _m_gn_ignores_partial(self, op, a, k):
        return op(*a, **dict(k, partial=None))

    def _m_stray(self, op, a, k):
        ret = op(*a, **k)
        out = a[2]
        SO._flat(out)[out.storage_offset() + out.shape[-1]] += 1.0      # the element beside row 0 of the view
        return ret

    def _m_input(self, op, a, k):
        ret = op(*a, **k)
        a[1][(0,) * a[1].dim()] += 1.0                                   # the weight
        return ret

    def _m_declined_wrote(self, op, a, k):
        a[2][0, 0, 0, 0] = 1.0                                           # a fresh buffer holds NaN: store a number
        return False

    def _m_last_row(self, op, a, k):
        ret = op(*a, **k)
        a[2][-1, -1] += 1.0
        return ret

    def _m_border_pixel(self, op, a, k):
        ret = op(*a, **k)
        a[2][-1, 7, -1, 0] += 1.0
        return ret


_CLEAN = {}


def clean_records():
    """The launch list of the clean tiny_mask run (prepare_cond + forward): the mutations pick their launch from its flags."""
    if not _CLEAN:
        _, inp, model = tiny("tiny_mask")
        sh, eng = shadow_engine(model)
        with torch.no_grad():
            eng.forward_cond(inp["x"], inp["t"], eng.prepare_cond(inp["context"], GroundingNetInput().prepare(inp["gb"])))
        _CLEAN["records"] = sh.records
    return _CLEAN["records"]


def first(op, pred=lambda r: True):
    return next(r["index"] for r in clean_records() if r["op"] == op and pred(r))


MUTATIONS = {
    "no_bias": lambda: first("gemm", lambda r: r["flags"].startswith("bias") and "ln_" not in r["flags"]),
    "no_gate": lambda: first("gemm", lambda r: "gate" in r["flags"]),
    "vt_untransposed": lambda: first("gemm", lambda r: "vt_out" in r["flags"]),
    "conv_origin": lambda: first("conv3x3"),
    "pad_key": lambda: first("attention", lambda r: "n0=77" in r["flags"]),
    "stray": lambda: first("gemm", lambda r: r["args"]["out"][1][-2] != r["args"]["out"][0][-1]),
    "input": lambda: first("gemm", lambda r: r["index"] > 40),
    "declined_wrote": lambda: first("conv_up2x"),
}


@pytest.mark.parametrize("kind", list(MUTATIONS))
def test_one_wrong_launch_fails_the_judge_at_its_index(kind):
    at = MUTATIONS[kind]()
    _, inp, model = tiny("tiny_mask")
    sh, eng = shadow_engine(model, inner=Mutant(EmulPlus(torch.float32), at, kind))
    with pytest.raises(LaunchOutside) as exc, torch.no_grad():
        eng.forward_cond(inp["x"], inp["t"], eng.prepare_cond(inp["context"], GroundingNetInput().prepare(inp["gb"])))
    rec = exc.value.record
    print(f"[mutation] {kind}: {exc.value}")
    assert exc.value.index == at and len(sh.records) == at + 1 and all(r["ok"] for r in sh.records[:at])
    assert f"launch {at} " in str(exc.value) and "@" in str(exc.value)        # names the launch and its engine buffer roles
    if kind == "stray":
        assert rec["stray"] == 1 and all(p["outside"] == 0 for p in rec["parts"])
    elif kind == "input":
        assert rec["inputs_modified"] == ["w"]
    elif kind == "declined_wrote":
        assert rec["stray"] == 1 and rec["note"] == "launch declined"
    else:
        assert any(p["outside"] > 0 for p in rec["parts"]) and rec["stray"] == 0
    if kind == "vt_untransposed":
        assert [p["part"] for p in rec["parts"] if p["outside"]] == ["vt_out"]


def _conv_then_groupnorm(inner):
    """conv3x3 leaves partials, the host shifts them (they no longer are the statistics of the conv's output), the GroupNorm is handed
    them: by ``groupnorm(.., partial=)``'s contract it normalises with what it is handed."""
    sh = ShadowOps(inner, "fp16")
    x, w = SK.gen((1, 8, 8, 64), 20), SK.gen((64, 576), 21, 0.05)
    out, part = torch.empty(1, 8, 8, 64), torch.empty(1, 1, 32, 2)
    sh.conv3x3(x, w, out, bias=SK.gen((64,), 22), gn_partial=part)
    part[..., 0] += 0.5
    gm, bt = SK.affine(64, 23)
    sh.groupnorm(out, torch.empty_like(out), gm, bt, 1e-5, True, partial=part)
    return sh


def test_groupnorm_that_ignores_its_partial_is_caught():
    assert not _conv_then_groupnorm(EmulPlus(torch.float32)).failures()
    with pytest.raises(LaunchOutside) as exc:
        _conv_then_groupnorm(Mutant(EmulPlus(torch.float32), 1, "gn_ignores_partial"))
    assert exc.value.index == 1 and exc.value.record["op"] == "groupnorm"


def _big_launches(inner):
    """Launches above the row cap: a 3000-row GEMM with a row bias per 1000 rows, a 3 x 20 x 20 conv (cap 512)."""
    sh = ShadowOps(inner, "fp16", row_cap=512)
    a, w = SK.gen((3000, 64), 30), SK.gen((72, 64), 31, 0.125)
    sh.gemm(a, w, torch.empty(3000, 72), bias=SK.gen((72,), 32), rowbias=SK.gen((3, 72), 33), rows_per_batch=1000)
    x, wc = SK.gen((3, 20, 20, 64), 34), SK.gen((64, 576), 35, 0.05)
    sh.conv3x3(x, wc, torch.empty(3, 20, 20, 64), bias=SK.gen((64,), 36))
    return sh


def test_wrong_rows_the_sampling_rule_must_include_are_caught():
    sh = _big_launches(EmulPlus(torch.float32))
    assert not sh.failures() and [r["parts"][0]["rows"] for r in sh.records] == [512, 512]
    assert [r["parts"][0]["total"] for r in sh.records] == [3000, 1200]
    for at, kind in ((0, "last_row"), (1, "border_pixel")):       # the last row of the last batch entry; pixel (7, last column) of the last sample
        with pytest.raises(LaunchOutside) as exc:
            _big_launches(Mutant(EmulPlus(torch.float32), at, kind))
        assert exc.value.index == at and exc.value.record["parts"][0]["outside"] == 1
