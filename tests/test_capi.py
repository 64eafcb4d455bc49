"""-m "not gpu": the C-ABI library loads and exports every symbol include/idf.h declares (no compute calls),
argument validation returns IDF_E_* codes without touching a GPU, and the reference's YAML configs instantiate."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    src = open(os.path.join(REPO, "include", "idf.h")).read()
    return sorted(set(re.findall(r"\b(idf_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from instancediffusion_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    declared = _declared_symbols()
    assert len(declared) >= 16
    for name in declared:
        assert hasattr(lib, name), f"libidf_gfx950.so does not export {name}"
        assert name in _lib.SYMBOLS, f"_lib.SYMBOLS has no prototype for {name}"
    assert lib.idf_abi_version() == 5
    assert b"gfx950" in lib.idf_build_info()


def test_single_hip_runtime_whatever_the_import_order():
    """Loading the C-ABI library before the caller ever imported torch must not bring a second libamdhip64 into the
    process (two runtimes -> hipErrorNoDevice on torch's streams)."""
    import subprocess
    import sys
    code = ("import instancediffusion_amd._lib as L; L.load(); import torch; "
            "m = {l.split()[-1] for l in open('/proc/self/maps') if 'amdhip64' in l}; print(len(m))")
    out = subprocess.run([sys.executable, "-c", code], cwd=REPO, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-500:]
    assert out.stdout.strip().splitlines()[-1] == "1", out.stdout


def test_argument_validation_without_gpu():
    from instancediffusion_amd import _lib
    lib = _lib.load()
    a = _lib.GemmArgs()                      # all-zero: null pointers
    assert lib.idf_gemm(ctypes.byref(a), None) == -1
    c = _lib.ConvArgs()
    assert lib.idf_conv3x3(ctypes.byref(c), None) == -1
    t = _lib.AttnArgs()
    assert lib.idf_attention(ctypes.byref(t), None) == -1
    assert lib.idf_layernorm(None, 0, None, 0, None, None, 1, 8, 1e-5, 0, None) == -1
    assert lib.idf_groupnorm_ws_floats(2, 4096) == 2 * 64 * 32 * 2
    assert lib.idf_softmax_rows(None, None, 4, 64, 64, 64, 1.0, 0, None) == -1
    assert lib.idf_pointwise_nchw(None, None, None, None, 1, 4, 4, 16, 1.0, None) == -1
    assert lib.idf_pointwise_nchw(0x10000, 0x20000, None, 0x30000, 1, 17, 4, 16, 1.0, None) == -1      # Cin <= 16
    assert lib.idf_pointwise_nchw(0x10000, 0x20000, None, 0x30000, 1, 4, 4, 0, 1.0, None) == -1
    # the PLMS step kernels and the merge (fake, never dereferenced pointers): every IDF_E_ARG case of include/idf.h
    def cfg(ec=0x10000, eu=0x20000, out=0x30000, n=256):
        return lib.idf_cfg_combine(ec, eu, 7.5, out, n, None)
    assert [cfg(ec=None), cfg(eu=None), cfg(out=None), cfg(n=0), cfg(n=-4)] == [-1] * 5

    def upd(x=0x10000, e_t=0x20000, e1=0x30000, e2=0x40000, e3=0x50000, en=0x60000, mode=4, a_t=0.42, a_prev=0.75, s1m=0.76,
            out=0x70000, n=256):
        return lib.idf_plms_update(x, e_t, e1, e2, e3, en, mode, a_t, a_prev, s1m, out, n, None)
    nan, inf = float("nan"), float("inf")
    bad = [upd(x=None), upd(e_t=None), upd(out=None), upd(n=0), upd(n=-4), upd(mode=-1), upd(mode=5), upd(mode=1, en=None),
           upd(mode=2, e1=None), upd(mode=3, e2=None), upd(mode=4, e3=None), upd(a_t=0.0), upd(a_t=-0.1), upd(a_t=nan), upd(a_t=inf),
           upd(a_prev=-0.1), upd(a_prev=1.5), upd(a_prev=nan), upd(a_prev=inf), upd(s1m=nan), upd(s1m=inf), upd(s1m=-inf)]
    assert bad == [-1] * len(bad), bad

    def mrg(lat=0x10000, boxes=0x20000, out=0x30000, n_inst=3, B=1, C=4, H=16, W=16, mode=1):
        return lib.idf_mis_merge(lat, boxes, out, n_inst, B, C, H, W, mode, None)
    bad = [mrg(lat=None), mrg(out=None), mrg(n_inst=-1), mrg(B=0), mrg(C=0), mrg(H=0), mrg(W=-1), mrg(mode=2), mrg(mode=-1),
           mrg(boxes=None)]
    assert bad == [-1] * len(bad), bad
    with pytest.raises(_lib.IdfError):
        _lib.check(-2, "x")
    # self-normalising LN_ROW (ln_stats == NULL): rejected before any launch when batched, without eps, on rows longer
    # than the statistics kernels hold, or with a misaligned statistics output (fake, never dereferenced pointers)
    def ln_args(**kw):
        g = _lib.GemmArgs(A=0x10000, W=0x20000, out=0x30000, bias=0x40000, M=256, N=320, K=320, lda=320, ldw=320, ldo=320,
                          batch=1, epi=_lib.EPI_BIAS | _lib.EPI_LN_ROW, dtype=0, ln_c=0x50000, ln_eps=1e-5)
        for k, v in kw.items():
            setattr(g, k, v)
        return g
    assert lib.idf_gemm(ctypes.byref(ln_args(batch=2, strideA=81920, strideO=81920)), None) == -1
    assert lib.idf_gemm(ctypes.byref(ln_args(ln_eps=0.0)), None) == -1
    assert lib.idf_gemm(ctypes.byref(ln_args(K=1600, lda=1600, ldw=1600)), None) == -1
    assert lib.idf_gemm(ctypes.byref(ln_args(ln_stats_out=0x60004)), None) == -2
    assert lib.idf_gemm(ctypes.byref(ln_args(epi=_lib.EPI_LN_ROW)), None) == -1          # the beta term travels as bias
    # fused q | k | v projection (ABI 3: vt_out / ld_vt / vt_col0): argument errors are reported before any launch
    def vt_args(**kw):
        g = ln_args(N=960, vt_out=0x70000, ld_vt=256, vt_col0=640, ldo=640, ln_stats_out=0x60000)
        for k, v in kw.items():
            setattr(g, k, v)
        return g
    assert lib.idf_gemm(ctypes.byref(vt_args(vt_col0=0)), None) == -1                     # nothing left for `out`
    assert lib.idf_gemm(ctypes.byref(vt_args(vt_col0=960)), None) == -1                   # nothing to transpose
    assert lib.idf_gemm(ctypes.byref(vt_args(ld_vt=128)), None) == -1                     # rows of V^T shorter than M
    assert lib.idf_gemm(ctypes.byref(vt_args(ld_vt=260)), None) == -1                     # 16-B row alignment
    assert lib.idf_gemm(ctypes.byref(vt_args(batch=2, strideA=81920, strideO=163840)), None) == -1
    assert lib.idf_gemm(ctypes.byref(vt_args(epi=_lib.EPI_BIAS | _lib.EPI_LN_ROW | _lib.EPI_SILU)), None) == -1
    assert lib.idf_gemm(ctypes.byref(vt_args(out_stats=0x80000)), None) == -1
    assert lib.idf_gemm(ctypes.byref(vt_args(ln_stats_out=None)), None) == -1             # self-normalising fallback needs them
    # a BIAS-only fused q | k | v call (no LN_ROW) is rejected during validation -- it used to fail in the two-GEMM
    # fallback after the q | k GEMM had already been launched, i.e. depending on tuning mode and CU count
    assert lib.idf_gemm(ctypes.byref(vt_args(epi=_lib.EPI_BIAS, ln_stats_out=None)), None) == -1
    # fused GEGLU feed-forward (ABI 4): null / misaligned operands and shapes the kernel does not take, before any launch
    def mlp_args(**kw):
        m = _lib.MlpArgs(x=0x10000, ldx=320, ln_stats=0x20000, w1=0x30000, ldw1=320, cd=0x40000, w2p=0x50000, ldw2=1280,
                         b2=0x60000, out=0x70000, ldo=320, M=256, C=320, dtype=0)
        for k, v in kw.items():
            setattr(m, k, v)
        return m
    assert lib.idf_mlp_geglu(None, None) == -1
    assert lib.idf_mlp_geglu(ctypes.byref(mlp_args(cd=None)), None) == -1
    assert lib.idf_mlp_geglu(ctypes.byref(mlp_args(dtype=7)), None) == -1
    assert lib.idf_mlp_geglu(ctypes.byref(mlp_args(C=640, ldx=640, ldo=640, ldw1=640, ldw2=2560)), None) == -3   # only C = 320
    assert lib.idf_mlp_geglu(ctypes.byref(mlp_args(M=200)), None) == -3                   # whole 128-row tiles only
    assert lib.idf_mlp_geglu(ctypes.byref(mlp_args(ldo=324)), None) == -2                 # 16-B row alignment
    assert lib.idf_mlp_geglu(ctypes.byref(mlp_args(ln_stats=0x20004)), None) == -2
    assert lib.idf_mlp_geglu(ctypes.byref(mlp_args(ldw2=640)), None) == -1                # rows of W2 shorter than 4C
    # GroupNorm partial statistics (ABI 5): the conv's gn_partial contract and the split GroupNorm entry points validate before any launch
    def conv_args(**kw):
        c = _lib.ConvArgs(x=0x10000, W=0x20000, out=0x30000, bias=0x40000, B=2, Hin=16, Win=16, Cin=320, Cout=320, stride=1,
                          upsample=0, ldx=320, ldo=320, epi=_lib.EPI_BIAS, dtype=0, gn_partial=0x50000)
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    assert lib.idf_conv3x3(ctypes.byref(conv_args(Hin=10, Win=10)), None) == -1           # 100 output rows per sample: not whole 64-row chunks
    assert lib.idf_conv3x3(ctypes.byref(conv_args(Cout=336, ldo=336)), None) == -1        # 336 channels: not 32 groups
    assert lib.idf_conv3x3(ctypes.byref(conv_args(ldo=640)), None) == -1                  # the output must be the dense NHWC matrix
    assert lib.idf_conv3x3(ctypes.byref(conv_args(epi=_lib.EPI_BIAS | _lib.EPI_OUT_F32)), None) == -1
    assert lib.idf_conv3x3(ctypes.byref(conv_args(gn_partial=0x50004)), None) == -2       # 8-B aligned (mean, M2) pairs
    assert lib.idf_groupnorm_stats(None, 0x1000, 1, 64, 320, 1, 0, None) == -1
    assert lib.idf_groupnorm_stats(0x10000, 0x20000, 1, 64, 330, 1, 0, None) == -1         # C % 32
    assert lib.idf_groupnorm_stats(0x10000, 0x20000, 1, 64, 320, 0, 0, None) == -1         # nchunks >= 1
    assert lib.idf_groupnorm_stats(0x10000, 0x20000, 1, 64, 320, 65, 0, None) == -1        # more chunks than rows
    assert lib.idf_groupnorm_stats(0x10008, 0x20000, 1, 64, 320, 1, 0, None) == -2
    assert lib.idf_groupnorm_apply(0x10000, 0x20000, 0x30000, 0x40000, None, 1, 64, 320, 1, 1e-5, 1, 0, None) == -1
    assert lib.idf_groupnorm_apply(0x10000, 0x20008, 0x30000, 0x40000, 0x50000, 1, 64, 320, 1, 1e-5, 1, 0, None) == -2
    assert lib.idf_groupnorm_apply(0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 1, 64, 320, 1, 1e-5, 1, 7, None) == -3
    # the pruned knobs are gone: unknown knob / value -> IDF_E_ARG, the remaining ones round-trip
    assert lib.idf_set_tuning(8, 0) == -1 and lib.idf_set_tuning(1, 7) == -1 and lib.idf_set_tuning(0, 4) == -1      # (round 6: attention modes 4 / 5 = attention4w.hip, 6 = its persistent form in experiment builds)
    # round 5 (ABI 5): the d = 80 / 160 LDS-DMA attention kernel's knob and launch counter
    assert lib.idf_set_tuning(_lib.IDF_TUNE_ATTN8, 7) == -1 and lib.idf_set_tuning(_lib.IDF_TUNE_ATTN8, -1) == -1
    prev = lib.idf_set_tuning(_lib.IDF_TUNE_ATTN8, 3)
    assert prev in range(7) and lib.idf_set_tuning(_lib.IDF_TUNE_ATTN8, prev) == 3
    assert lib.idf_get_stat(_lib.IDF_STAT_ATTN8_LAUNCHES) == 0
    prev = lib.idf_set_tuning(1, 2)
    assert prev in (0, 1, 2, 3, 4, 5, 6) and lib.idf_set_tuning(1, prev) == 2
    # round 6: which kernel serves idf_mlp_geglu (0 = 8 waves, 1 = one generated instruction stream per SIMD; default 1)
    assert lib.idf_set_tuning(_lib.IDF_TUNE_MLP, 2) == -1 and lib.idf_set_tuning(_lib.IDF_TUNE_MLP, -1) == -1
    prev = lib.idf_set_tuning(_lib.IDF_TUNE_MLP, 0)
    assert prev == 1 and lib.idf_set_tuning(_lib.IDF_TUNE_MLP, prev) == 0
    # round 6: the fused q | k | v projection of the C = 320 level on the row-resident kernel (0 = never, 1 = when the shape qualifies)
    assert lib.idf_set_tuning(_lib.IDF_TUNE_QKV_ROW, 2) == -1 and lib.idf_get_stat(_lib.IDF_STAT_QKV_ROW_LAUNCHES) == 0
    prev = lib.idf_set_tuning(_lib.IDF_TUNE_QKV_ROW, 0)
    assert prev == 1 and lib.idf_set_tuning(_lib.IDF_TUNE_QKV_ROW, prev) == 0
    # ... and the GEGLU projection of the C = 640 level (geglu_fused.hip)
    assert lib.idf_set_tuning(_lib.IDF_TUNE_GEGLU_ROW, 2) == -1 and lib.idf_get_stat(_lib.IDF_STAT_GEGLU_ROW_LAUNCHES) == 0
    prev = lib.idf_set_tuning(_lib.IDF_TUNE_GEGLU_ROW, 0)
    assert prev == 1 and lib.idf_set_tuning(_lib.IDF_TUNE_GEGLU_ROW, prev) == 0
    # round 4: tile-count threshold of the latency kernel (0 = never), and its launch counter
    assert lib.idf_set_tuning(_lib.IDF_TUNE_GEMM_RING, -1) == -1
    prev = lib.idf_set_tuning(_lib.IDF_TUNE_GEMM_RING, 77)
    assert prev >= 0 and lib.idf_set_tuning(_lib.IDF_TUNE_GEMM_RING, prev) == 77
    assert lib.idf_get_stat(_lib.IDF_STAT_GEMM_RING_LAUNCHES) == 0 and lib.idf_get_stat(5) == -1 and lib.idf_get_stat(_lib.IDF_STAT_GN_EPI_LAUNCHES) == 0
    assert lib.idf_set_tuning(_lib.IDF_TUNE_BIG_MIN_EFF, 0) == -1 and lib.idf_set_tuning(_lib.IDF_TUNE_BIG_MIN_EFF, 101) == -1
    prev = lib.idf_set_tuning(_lib.IDF_TUNE_BIG_MIN_EFF, 60)
    assert 1 <= prev <= 100 and lib.idf_set_tuning(_lib.IDF_TUNE_BIG_MIN_EFF, prev) == 60


def test_fuser_type_values_of_the_reference_are_accepted():
    """openaimodel.py:349 accepts gatedSA / gatedSA2 / gatedCA and attention.py:325 builds a GatedSelfAttentionDense whatever
    the value: all three must construct the same network here."""
    import torch
    from instancediffusion_amd.host.config import instantiate_from_config, load_yaml
    cfg = load_yaml(os.path.join(REPO, "configs", "test_box.yaml"))
    keys = {}
    for ft in ("gatedSA", "gatedSA2", "gatedCA"):
        cfg["model"]["params"]["fuser_type"] = ft
        with torch.device("meta"):
            m = instantiate_from_config(cfg["model"])
        keys[ft] = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert keys["gatedSA"] == keys["gatedSA2"] == keys["gatedCA"] and len(keys["gatedSA"]) == 1199


def test_stale_tuning_values_in_the_environment_fall_back_to_the_default():
    """IDF_ATTN2 / IDF_GEMM_BIG values outside the range idf_set_tuning accepts (e.g. an attention mode of ABI 2)
    are ignored instead of selecting a kernel by accident."""
    import subprocess
    import sys
    code = ("import instancediffusion_amd._lib as L; lib = L.load(); a = lib.idf_set_tuning(1, 1); b = lib.idf_set_tuning(0, 1); "
            "c = lib.idf_set_tuning(L.IDF_TUNE_GEMM_RING, 256); d = lib.idf_set_tuning(L.IDF_TUNE_BIG_MIN_EFF, 50); print(a, b, c, d)")
    env = dict(os.environ, IDF_ATTN2="9", IDF_GEMM_BIG="-5", IDF_GEMM_RING="-3", IDF_BIG_MIN_EFF="250")
    out = subprocess.run([sys.executable, "-c", code], cwd=REPO, capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-500:]
    assert out.stdout.strip().splitlines()[-1] == "5 1 256 50", out.stdout        # the library defaults
    # in-range values ARE taken from the environment
    env = dict(os.environ, IDF_GEMM_RING="0", IDF_BIG_MIN_EFF="80")
    out = subprocess.run([sys.executable, "-c", code], cwd=REPO, capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and out.stdout.strip().splitlines()[-1].split()[2:] == ["0", "80"], out.stdout + out.stderr[-300:]


def test_attention4w_asm_owned_registers_are_left_alone_by_the_compiler():
    """attention4w.hip keeps its accumulators, Q and V^T fragments in AGPRs named in inline asm.  The register allocator knows
    them only as clobbers: a compiler-generated v_accvgpr_* (an AGPR used as VGPR spill space) or any scratch access inside the
    kernel would silently corrupt them (it happened: 7 VGPRs spilled into a0..a6 in the first two-waves-per-SIMD build).
    tools/check_attn4w_isa.py compiles the file with the library's flags and scans the listing of all four instantiations."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("check_attn4w_isa", os.path.join(REPO, "tools", "check_attn4w_isa.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rep = mod.check()
    assert len(rep) == 4, sorted(rep)               # bf16 / fp16 x 128 / 64 queries per wave
    for name, r in rep.items():
        assert not r["stray_accvgpr"] and r["scratch_ops"] == 0 and r["mfma"] > 50, (name, r["stray_accvgpr"][:3], r["scratch_ops"])


ROW_KERNELS = [   # (stream generator, prefix of its options in the environment, source file, kernel, MFMAs per instantiation at least)
    ("gen_mlpw_stream.py", "MW_", "mlp_fused.hip", "mlp320w_kernel", 200),        # x fragments a0..a79, output accumulators a80..a239
    ("gen_qkvw_stream.py", "QW_", "qkv_fused.hip", "qkv320w_kernel", 200),        # x fragments a0..a159, mean fragments, statistics: a0..a171
    ("gen_qkv640w_stream.py", "QM_", "qkv640_fused.hip", "qkv640w_kernel", 100),  # x fragments a0..a159, statistics a160:161
    ("gen_gegluw_stream.py", "GW_", "geglu_fused.hip", "geglu640w_kernel", 100),  # the same block
]


def test_mlp320w_stream_is_current_and_its_registers_are_left_alone():
    """The row-resident kernels (csrc/mw_row.h), mlp_fused.hip's one-wave-per-SIMD kernel first: (1) the checked-in instruction
    stream (csrc/*_stream.inc) is what its generator writes with its default options; (2) the asm-owned AGPR block is not touched
    by compiler-generated code and the kernel has no scratch (a scratch access would also break the counted vmcnt waits), in both
    element types."""
    import importlib.util
    import subprocess
    import sys
    spec = importlib.util.spec_from_file_location("check_attn4w_isa", os.path.join(REPO, "tools", "check_attn4w_isa.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for gen, prefix, src, kernel, mfma_floor in ROW_KERNELS:
        env = {k: v for k, v in os.environ.items() if not k.startswith(prefix)}
        assert subprocess.run([sys.executable, os.path.join(REPO, "tools", gen), "--check"], env=env).returncode == 0, gen
        rep = mod.check(src=os.path.join(REPO, "instancediffusion_amd", "csrc", src), kernel=kernel)
        assert len(rep) == 2, sorted(rep)
        for name, r in rep.items():
            assert not r["stray_accvgpr"] and r["scratch_ops"] == 0 and r["mfma"] > mfma_floor, (name, r["stray_accvgpr"][:3], r["scratch_ops"])


def test_schema_matches_reference():
    import json
    from tests import cases
    ref = json.load(open(os.path.join(REPO, "tests", "golden", "unet_schema.json")))
    mine = cases.unet_schema(cases.cfg_for("test_box.yaml", "full"))
    assert set(ref) == set(mine) and len(ref) == 1199
    assert all(tuple(ref[k]) == tuple(mine[k]) for k in ref)


@pytest.mark.parametrize("name", ["test_box.yaml", "test_mask.yaml", "test_point.yaml", "test_scribble.yaml"])
def test_reference_yaml_instantiates(name):
    """The reference's own YAMLs (as parsed, golden ``ref_configs.json``, oracle/make_golden.py:gen_ref_configs) and this
    repo's configs/ copy of them resolve to this implementation unchanged."""
    import json
    import torch
    from instancediffusion_amd.host.config import instantiate_from_config, load_yaml
    ref = json.load(open(os.path.join(REPO, "tests", "golden", "ref_configs.json")))[name]
    for cfg in (ref, load_yaml(os.path.join(REPO, "configs", name))):
        with torch.device("meta"):
            model = instantiate_from_config(cfg["model"])
        diffusion = instantiate_from_config(cfg["diffusion"])
        gi = instantiate_from_config(cfg["grounding_tokenizer_input"])
        assert type(model).__module__.startswith("instancediffusion_amd")
        assert diffusion.num_timesteps == 1000 and abs(float(diffusion.betas[0]) - 0.00085) < 1e-9
        assert model.position_net.eval_drops() is not None and hasattr(gi, "get_null_input")


def test_inference_cli_input_builder():
    """inference.py parses the reference's demo-JSON format and builds prepare_batch tensors through the mirrors."""
    import json
    import torch
    import inference
    from instancediffusion_amd import synth
    from instancediffusion_amd.host.input import meta_from_demo_json, prepare_instance_meta
    from grounding_input.text_grounding_tokinzer_input import GroundingNetInput
    data = json.load(open(os.path.join(REPO, "demos", "demo_four_boxes.json")))
    meta = meta_from_demo_json(data, 0.75)
    enc = inference.SyntheticTextEncoder()
    gi = GroundingNetInput()
    noise = torch.zeros(2, 4, 64, 64)
    inp, uc = inference.get_model_inputs(meta, gi, enc, enc, 2, "cpu", noise, "bad")
    g = inp["grounding_input"]
    assert g["boxes"].shape == (2, 30, 4) and g["segs"].shape == (2, 30, 512, 512) and uc.shape == (2, 77, 768)
    assert torch.allclose(g["boxes"][0, :4], torch.tensor(synth.C1_BOXES), atol=2e-3)
    assert g["masks"][0].sum() == 4 and inp["context"].shape == (2, 77, 768)
    assert torch.allclose(g["points"][0, 0], (g["boxes"][0, 0, :2] + g["boxes"][0, 0, 2:]) / 2)
    assert torch.equal(g["positive_embeddings"][0, 1], enc.pooled(data["annos"][1]["caption"]))
    inst, uc_i = inference.get_model_inputs(prepare_instance_meta(meta, 2), gi, enc, enc, 2, "cpu", noise,
                                            instance_input=True)
    gi2 = inst["grounding_input"]
    assert uc_i is None and torch.equal(gi2["boxes"][:, 0], g["boxes"][:, 2]) and gi2["masks"].sum() == 2
    null = gi.get_null_input()
    assert null["segs"].shape == (2, 30, 512, 512) and null["segs"].stride(0) == 0
