"""img2img starts and the hi-res second pass without a GPU: the resize tables (exact-integer geometry, float64 weights) against
``F.interpolate`` on float64 input, ``steps_for_strength``, the C ABI of ``idf_q_sample`` / ``idf_resize_planes`` (argument errors before
any launch) and ``inference.py``'s new flags and refusals."""
import os
import sys

import numpy as np
import pytest
import torch

from instancediffusion_amd.host import hires
from instancediffusion_amd.host.diffusion import LatentDiffusion
from instancediffusion_amd.host.samplers import DDIMSampler, DPMSolverSampler, PLMSSampler
from tests import hires_cases as hc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- tables ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bicubic", "bilinear"])
@pytest.mark.parametrize("size", hc.TABLE_SIZES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_tables_reproduce_interpolate_on_float64(size, mode):
    """The fixed expression in float64 over the fp32-rounded tables against ``F.interpolate`` on float64 input: weight rounding only.
    At most two fp32-rounded weights meet in a term (relative error 2 u) and sum |wy wx| <= 1.375^2 = 1.89, so 3.8 u max|x| is the outer
    bound; the bar is 2 u max|x| (observed <= 0.76 u)."""
    Hi, Wi, Ho, Wo = size
    x = hc.seeded((3, Hi, Wi), seed=Hi * 1000 + Wo)
    got = hc.resize_expr(x, (Ho, Wo), mode, torch.float64)
    want = hc.interpolate64(x, (Ho, Wo), mode)
    err = float((got - want).abs().max()) / (hc.U * float(x.abs().max()))
    print(f"[tables] {mode} {Hi}x{Wi} -> {Ho}x{Wo}: {err:.2f} u max|x| (bar 2)")
    assert got.dtype == torch.float64 and err <= 2.0
    if (Hi, Wi) == (Ho, Wo):
        assert torch.equal(hc.resize_expr(x, (Ho, Wo), mode, torch.float32), x), "the identity size is exact"
    # the host's own CPU twin is the same expression, bit for bit in both precisions
    assert torch.equal(hires.resize_reference(x, (Ho, Wo), mode, torch.float32), hc.resize_expr(x, (Ho, Wo), mode, torch.float32))
    assert torch.equal(hires.resize_reference(x, (Ho, Wo), mode, torch.float64), got)


@pytest.mark.parametrize("mode", ["bicubic", "bilinear"])
@pytest.mark.parametrize("size", hc.TABLE_SIZES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_table_rows_sum_to_one_and_indices_stay_next_to_the_source(size, mode):
    """Every row of weights sums to 1 within 2 u.  First taps: bilinear in [0, n_in - 1]; bicubic first tap = floor(src) - 1 with
    floor(src) in [-1, n_in - 1] -- src > -1/2 always, and floor(src) = -1 exactly where an UPSCALE's first outputs lie left of source
    pixel 0 -- so the first tap is in [-2, n_in - 2], and -2 occurs only with floor(src) = -1.  Every tap the expression reads after
    its clamp is in [0, n_in - 1]."""
    for n_in, n_out in ((size[0], size[2]), (size[1], size[3])):
        first, w = hires.resize_tables(n_in, n_out, mode)
        taps = hires.MODES[mode]
        assert first.dtype == np.int32 and w.dtype == np.float32 and first.shape == (n_out,) and w.shape == (n_out, taps)
        assert float(np.abs(w.astype(np.float64).sum(1) - 1.0).max()) <= 2 * hc.U
        floor_src = [((2 * o + 1) * n_in - n_out) // (2 * n_out) for o in range(n_out)]
        assert min(floor_src) >= -1 and max(floor_src) <= n_in - 1
        if taps == 2:
            assert first.min() >= 0 and first.max() <= n_in - 1
            assert first.tolist() == [max(f, 0) for f in floor_src]
        else:
            assert first.tolist() == [f - 1 for f in floor_src]
            assert first.min() >= -2 and first.max() <= n_in - 2
            assert (first.min() == -2) == (n_out > n_in or (n_in == 1 and n_out > 1))
        if n_in == n_out:                                                   # the identity: one weight of exactly 1 on the pixel itself
            k = 0 if taps == 2 else 1
            assert (first + k).tolist() == list(range(n_in)) and (w[:, k] == 1).all() and (np.delete(w, k, 1) == 0).all()


def test_table_value_errors():
    with pytest.raises(ValueError):
        hires.resize_tables(16, 24, "nearest")
    with pytest.raises(ValueError):
        hires.resize_tables(0, 24, "bicubic")
    with pytest.raises(ValueError):
        hires.resize_tables(16, 0, "bilinear")


def test_bicubic_weights_are_torchs_cubic():
    """16 -> 24, output 1: src = (3 * 16 - 24) / 48 = 1/2 exactly -> f = 0, t = 1/2: the A = -0.75 cubic at 3/2, 1/2, 1/2, 3/2."""
    first, w = hires.resize_tables(16, 24, "bicubic")
    assert first[1] == -1
    assert w[1].tolist() == [np.float32(-0.09375), np.float32(0.59375), np.float32(0.59375), np.float32(-0.09375)]
    first, w = hires.resize_tables(16, 24, "bilinear")
    assert first[1] == 0 and w[1].tolist() == [0.5, 0.5] and first[0] == 0 and w[0].tolist() == [1.0, 0.0]   # src clamped to 0


# ---- steps_for_strength -----------------------------------------------------------------------------------------------
def _diffusion():
    return LatentDiffusion(linear_start=0.00085, linear_end=0.012, timesteps=1000)


# (S, strength) -> steps run
N_RUN = {(1, 0.01): 1, (1, 0.35): 1, (1, 0.5): 1, (1, 0.58): 1, (1, 1.0): 1,
         (5, 0.01): 1, (5, 0.35): 1, (5, 0.5): 2, (5, 0.58): 2, (5, 1.0): 5,
         (20, 0.01): 1, (20, 0.35): 7, (20, 0.5): 10, (20, 0.58): 11, (20, 1.0): 20,
         (50, 0.01): 1, (50, 0.35): 17, (50, 0.5): 25, (50, 0.58): 29, (50, 1.0): 50}


@pytest.mark.parametrize("cls", [PLMSSampler, DDIMSampler, DPMSolverSampler])
def test_steps_for_strength_table(cls):
    """``t`` is the timestep the loop then visits first: step ``start`` of the flipped schedule."""
    s = cls(_diffusion(), model=None)
    for (S, strength), n_run in N_RUN.items():
        start, t = hires.steps_for_strength(S, strength)
        assert start == S - n_run and 0 <= start < S
        s.make_schedule(S)
        assert t == int(np.flip(s.ddim_timesteps)[start]) == int(s.ddim_timesteps[n_run - 1])
        assert hires.steps_for_strength(S, strength, s.ddim_timesteps) == (start, t)
    assert hires.steps_for_strength(50, 0.35) == (33, 321) and hires.steps_for_strength(5, 0.6) == (2, 401)
    assert hires.steps_for_strength(50, 0.58) == (21, 561)                  # 50 * 0.58 = 28.999999999999996: the 1e-6 guards the floor


def test_steps_for_strength_follows_the_logsnr_spacing():
    s = DPMSolverSampler(_diffusion(), model=None)
    s.make_schedule(5, "logsnr")
    assert hires.steps_for_strength(5, 0.6, s.ddim_timesteps) == (2, 280)       # [1, 33, 280, 703, 999]


@pytest.mark.parametrize("strength", [0.0, -0.1, 1.0001, float("nan"), None, "0.5"])
def test_strength_outside_the_half_open_interval(strength):
    with pytest.raises(ValueError):
        hires.steps_for_strength(50, strength)


@pytest.mark.parametrize("cls", [PLMSSampler, DDIMSampler, DPMSolverSampler])
@pytest.mark.parametrize("start", [-1, 5, 7, 2.0, "2", None, True])
def test_start_outside_the_schedule_is_refused_before_any_forward(cls, start):
    """model=None: anything beyond the argument check would raise AttributeError, not ValueError."""
    s = cls(_diffusion(), model=None)
    with pytest.raises(ValueError):
        s.sample_from(5, (1, 4, 8, 8), dict(x=torch.zeros(1, 4, 8, 8)), start)


def test_the_multi_instance_samplers_take_no_start():
    from instancediffusion_amd.host.samplers import DDIMSamplerInst, DPMSolverSamplerInst, PLMSSamplerInst
    import inspect
    for cls in (PLMSSamplerInst, DDIMSamplerInst, DPMSolverSamplerInst):
        assert not hasattr(cls, "sample_from") and "start" not in inspect.signature(cls.sample).parameters
    assert inspect.signature(PLMSSampler.sample).parameters["start"].default == 0
    assert inspect.signature(PLMSSampler.plms_sampling).parameters["start"].default == 0


# ---- C ABI ------------------------------------------------------------------------------------------------------------
def test_abi_symbols_prototypes_and_argument_validation_without_gpu():
    """Both symbols are exported with their prototypes inside ABI 5, the header declares them, and every argument error is reported
    before anything touches a device (fake, never dereferenced pointers, as tests/test_capi.py does)."""
    from instancediffusion_amd import _lib
    lib = _lib.load()
    assert len(_lib.SYMBOLS["idf_q_sample"][1]) == 7 and len(_lib.SYMBOLS["idf_resize_planes"][1]) == 13
    assert len(lib.idf_q_sample.argtypes) == 7 and len(lib.idf_resize_planes.argtypes) == 13 and lib.idf_abi_version() == 5
    header = open(os.path.join(REPO, "include", "idf.h")).read()
    assert "int idf_q_sample(const float* x0, const float* noise, float sqrt_ac, float sqrt_1m_ac, float* out, long long n, void* stream);" in header
    assert "int idf_resize_planes(const float* src, float* dst, const int* xi, const float* xw, const int* yi, const float* yw, int taps" in header
    assert "#define IDF_ABI_VERSION 5" in header
    nan, inf = float("nan"), float("inf")

    def qs(x0=0x10000, nz=0x20000, sa=0.65, s1=0.76, out=0x30000, n=256):
        return lib.idf_q_sample(x0, nz, sa, s1, out, n, None)
    bad = [qs(x0=None), qs(nz=None), qs(out=None), qs(n=0), qs(n=-4), qs(sa=nan), qs(sa=inf), qs(s1=nan), qs(s1=-inf)]
    assert bad == [-1] * len(bad), bad

    def rs(src=0x100000, dst=0x900000, xi=0x10000, xw=0x20000, yi=0x30000, yw=0x40000, taps=4, planes=8, Hi=16, Wi=16, Ho=24, Wo=24):
        return lib.idf_resize_planes(src, dst, xi, xw, yi, yw, taps, planes, Hi, Wi, Ho, Wo, None)
    bad = [rs(src=None), rs(dst=None), rs(xi=None), rs(xw=None), rs(yi=None), rs(yw=None), rs(taps=0), rs(taps=1), rs(taps=3), rs(taps=8),
           rs(planes=0), rs(Hi=0), rs(Wi=-1), rs(Ho=0), rs(Wo=0),
           rs(dst=0x100000),                                # dst == src
           rs(dst=0x100000 + 8 * 16 * 16 * 4 - 4),          # dst begins on src's last float
           rs(src=0x900000 + 8 * 24 * 24 * 4 - 4)]          # src begins on dst's last float
    assert bad == [-1] * len(bad), bad
    # planes * Ho * Wo >= 2^31: unsupported, before any launch (2^19 planes of 64 x 64 outputs)
    assert rs(src=0x1000, dst=1 << 44, planes=1 << 19, Hi=1, Wi=1, Ho=64, Wo=64) == _lib.E_UNSUPPORTED
    assert rs(src=0x1000, dst=1 << 44, planes=1 << 30, Hi=1, Wi=1, Ho=2, Wo=1) == _lib.E_UNSUPPORTED

    # idf_q_sample_blend is unchanged: its null-pointer refusals
    def blend(x0=0x10000, nz=0x20000, mask=0x30000, img=0x40000, out=0x50000):
        return lib.idf_q_sample_blend(x0, nz, mask, img, 0.6, 0.8, out, 2, 4, 32, 1, None)
    assert [blend(x0=None), blend(nz=None), blend(mask=None), blend(img=None), blend(out=None)] == [-1] * 5


# ---- inference.py -----------------------------------------------------------------------------------------------------
def _refused(monkeypatch, argv):
    import inference
    built = []
    monkeypatch.setattr(inference, "instantiate_from_config", lambda *a, **k: built.append(a) or (_ for _ in ()).throw(AssertionError("built")))
    monkeypatch.setattr(inference, "load_yaml", lambda *a, **k: built.append(a) or {})
    monkeypatch.setattr(sys, "argv", ["inference.py", "--synthetic_weights"] + argv)
    with pytest.raises(SystemExit) as e:
        inference.main()
    assert isinstance(e.value.code, str) and e.value.code, "a message, not an exit status"
    assert not built, "refused before any model is built"
    return e.value.code


@pytest.mark.parametrize("argv, word", [
    (["--init_image", "a.png", "--strength", "0.5", "--inpaint_mask", "m.png", "--mis", "0"], "--inpaint_mask"),
    (["--strength", "0.5", "--mis", "0"], "--init_image"),
    (["--init_image", "a.png", "--strength", "0", "--mis", "0"], "(0, 1]"),
    (["--init_image", "a.png", "--strength", "1.2", "--mis", "0"], "(0, 1]"),
    (["--init_image", "a.png", "--strength", "0.7"], "1 - mis"),                                   # default --mis 0.36: limit 0.64
    (["--init_image", "a.png", "--strength", "0.5", "--mis", "0.6"], "1 - mis"),
    (["--hires_scale", "1.5", "--hires_strength", "0.7"], "1 - mis"),
    (["--hires_scale", "1.5", "--hires_strength", "0.5", "--hires_steps", "20", "--mis", "0.55"], "1 - mis"),
    (["--hires_scale", "1.0"], "> 1"),
    (["--hires_scale", "0.5"], "> 1"),
    (["--hires_scale", "1.5", "--hires_strength", "0"], "(0, 1]"),
    (["--hires_scale", "1.5", "--hires_steps", "0"], "--hires_steps"),
    (["--hires_scale", "1.5", "--input_json", "a.json", "b.json"], "one --input_json"),
    (["--init_image", "a.png", "--strength", "0.5", "--input_json", "a.json", "b.json"], "one --input_json"),
    (["--hires_scale", "1.5", "--use_masked_att"], "--use_masked_att"),
    (["--init_image", "a.png", "--strength", "0.5", "--use_masked_att"], "--use_masked_att"),
    (["--hires_scale", "1.5", "--init_image", "a.png", "--inpaint_mask", "m.png", "--sampler", "ddim", "--mis", "0"], "inpainting"),
])
def test_cli_refusals(monkeypatch, argv, word):
    assert word in _refused(monkeypatch, argv)


def test_init_image_without_strength_keeps_its_message(monkeypatch):
    assert _refused(monkeypatch, ["--mis", "0", "--init_image", "a.png"]) == "inpainting needs both --init_image and --inpaint_mask"


def test_the_mis_limit_is_stated_and_a_start_behind_phase_one_passes():
    import inference
    with pytest.raises(SystemExit) as e:
        inference.refuse_start_inside_mis("--strength", 50, 0.7, 0.36)
    assert "strength <= 1 - mis = 0.64" in e.value.code and "step 15" in e.value.code and "steps 0 .. 17" in e.value.code
    inference.refuse_start_inside_mis("--strength", 50, 0.64, 0.36)         # start 18 = int(50 * 0.36): the first step of phase 2
    inference.refuse_start_inside_mis("--strength", 50, 1.0, 0.0)
    inference.refuse_start_inside_mis("--hires_strength", 5, 0.5, 0.36)


def test_hires_side_names_the_nearest_valid_scales():
    import inference
    assert inference.hires_side(64, 1.5) == 96 and inference.hires_side(64, 2) == 128 and inference.hires_side(16, 1.5) == 24
    assert inference.hires_side(64, 1.125) == 72
    with pytest.raises(SystemExit) as e:
        inference.hires_side(64, 1.4)                                        # 90 x 90
    assert "1.375 (88 x 88 latents)" in e.value.code and "1.5 (96 x 96 latents)" in e.value.code
    with pytest.raises(SystemExit) as e:
        inference.hires_side(64, 1.05)                                       # 67: 64 is no enlargement, only 72 is named
    assert "1.125 (72 x 72 latents)" in e.value.code and "(64 x 64" not in e.value.code
    with pytest.raises(SystemExit):
        inference.hires_side(64, 1.0)
    with pytest.raises(SystemExit):
        inference.hires_side(64, 1.001)                                      # rounds to 64
