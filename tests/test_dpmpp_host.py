"""DPM-Solver++(2M) without a GPU: the host coefficients and the logsnr spacing, the convergence order on a model with a known
exact solution, ``DPMSolverSampler`` over the CPU op emulation (tests/emul_ops_dpmpp.py) against the composed oracle
(tests/dpmpp_cases.py) and against DDIM at order 1, the ``ldm`` shim and the C ABI of ``idf_dpmpp_update``."""
import inspect
import os
from functools import partial

import numpy as np
import pytest
import torch

from instancediffusion_amd import synth
from instancediffusion_amd.engine import UNetEngine
from instancediffusion_amd.host.alpha import alpha_generator, set_alpha_scale
from instancediffusion_amd.host.diffusion import LatentDiffusion
from instancediffusion_amd.host.samplers import DPMSolverSampler, _PLMSBase, dpmpp_coeffs, dpmpp_coeffs64, logsnr_timesteps
from grounding_input.text_grounding_tokinzer_input import GroundingNetInput
from oracle import ref_cpu
from tests import cases, ddim_cases
from tests import dpmpp_cases as dc
from tests.emul_ops_dpmpp import EmulOpsDPMpp
from tests.test_engine_emulated import build_model

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL_TRAJ_TOL = 5e-3            # the bar of the DDIM emulated tests (tests/test_ddim_host.py)
ORDER1_VS_DDIM_TOL = 1e-4       # order 1 is DDIM with eta 0; only the rounding of the coefficients differs


def _diffusion():
    return LatentDiffusion(linear_start=0.00085, linear_end=0.012, timesteps=1000)


def _ac():
    return _diffusion().alphas_cumprod.numpy()


def _schedule(S, discretize):
    s = DPMSolverSampler(_diffusion(), model=None)
    s.make_schedule(S, discretize)
    return s


# ---- coefficients -------------------------------------------------------------------------------------------------------
def _lam(a):
    a = np.float64(a)
    return np.log(np.sqrt(a) / np.sqrt(1 - a))


@pytest.mark.parametrize("discretize", ["uniform", "logsnr"])
@pytest.mark.parametrize("S", [5, 20, 50])
def test_order_one_is_ddim_eta_zero_and_the_order_two_weights_sum_to_bc(S, discretize):
    s = _schedule(S, discretize)
    assert s.ddim_alphas.dtype == np.float32 and s.ddim_alphas_prev.dtype == np.float32 and len(s.ddim_alphas) == S
    for index in range(S):
        a_t, a_prev = s.ddim_alphas[index], s.ddim_alphas_prev[index]
        a64, p64 = np.float64(a_t), np.float64(a_prev)
        # DDIM with eta 0 is x_prev = sqrt(a_prev) x0 + sqrt(1 - a_prev) e with e = (x - sqrt(a_t) x0) / sqrt(1 - a_t)
        want_x = np.sqrt(1 - p64) / np.sqrt(1 - a64)
        want_0 = np.sqrt(p64) - np.sqrt(1 - p64) * np.sqrt(a64) / np.sqrt(1 - a64)
        c_x, c_0, c_1 = dpmpp_coeffs64(a_t, a_prev)
        assert abs(c_x - want_x) <= 1e-9 * abs(want_x) and abs(c_0 - want_0) <= 1e-9 * abs(want_0) and c_1 == 0, index
        got = dpmpp_coeffs(a_t, a_prev)
        assert all(isinstance(c, np.float32) for c in got) and got == (np.float32(c_x), np.float32(c_0), np.float32(0))
        # r = 1: the step before was as long in lambda, lambda_last = 2 lambda_t - lambda_prev
        l_last = 2 * _lam(a_t) - _lam(a_prev)
        a_last = 1 / (1 + np.exp(-2 * l_last))
        d_x, d_0, d_1 = dpmpp_coeffs64(a_t, a_prev, a_last)
        assert d_x == c_x and abs((d_0 + d_1) - c_0) <= 1e-9 * abs(c_0), index
        assert abs(d_0 - 1.5 * c_0) <= 1e-6 * c_0 and abs(d_1 + 0.5 * c_0) <= 1e-6 * c_0
    for index in range(S - 1):                                                  # the run's own order-2 triples, rounded once
        args = (s.ddim_alphas[index], s.ddim_alphas_prev[index], s.ddim_alphas[index + 1])
        got = dpmpp_coeffs(*args)
        assert got == tuple(np.float32(c) for c in dpmpp_coeffs64(*args)) and got[2] < 0 < got[1]
        assert np.allclose(np.float64(got), np.float64(dc.coeffs(*args)), rtol=2.0 ** -22, atol=0)   # the test-side restatement


# ---- timesteps ----------------------------------------------------------------------------------------------------------
def test_logsnr_recorded_values():
    ac = _ac()
    assert logsnr_timesteps(5, ac).tolist() == [1, 33, 280, 703, 999]
    t10 = logsnr_timesteps(10, ac).tolist()
    assert t10[:8] == [1, 6, 24, 77, 195, 376, 572, 742] and t10[-2:] == [882, 999] and len(t10) == 10
    assert dc.timesteps(5, "logsnr").tolist() == [1, 33, 280, 703, 999]          # the test-side restatement agrees
    s = _schedule(5, "logsnr")
    assert s.ddim_timesteps.tolist() == [1, 33, 280, 703, 999]
    assert s.ddim_alphas.tolist() == ac[[1, 33, 280, 703, 999]].tolist()
    assert s.ddim_alphas_prev.tolist() == ac[[0, 1, 33, 280, 703]].tolist()


def test_logsnr_is_strictly_increasing_from_1_to_999_for_every_s():
    ac = _ac()
    assert logsnr_timesteps(1, ac).tolist() == [999]
    for S in range(2, 201):
        t = logsnr_timesteps(S, ac)
        assert len(t) == S and t[0] == 1 and t[-1] == 999 and bool((np.diff(t) > 0).all()) and len(set(t.tolist())) == S, S
    t = logsnr_timesteps(999, ac)
    assert t.tolist() == list(range(1, 1000))


def test_uniform_stays_the_default_and_is_plms_timesteps():
    from instancediffusion_amd.host.samplers import PLMSSampler
    p = PLMSSampler(_diffusion(), model=None)
    p.make_schedule(20)
    s = DPMSolverSampler(_diffusion(), model=None)
    s.make_schedule(20)
    assert s.ddim_timesteps.tolist() == p.ddim_timesteps.tolist() and s.ddim_alphas.tolist() == p.ddim_alphas.tolist()
    assert inspect.signature(DPMSolverSampler.sample).parameters["discretize"].default == "uniform"
    with pytest.raises(NotImplementedError):                                     # PLMS itself gains no new spacing
        p.make_schedule(20, "logsnr")


@pytest.mark.parametrize("S", [0, -1, 1000, 5000])
def test_logsnr_value_errors(S):
    with pytest.raises(ValueError):
        logsnr_timesteps(S, _ac())
    with pytest.raises(ValueError):
        _schedule(S, "logsnr")


# ---- convergence on the analytic Gaussian model -----------------------------------------------------------------------
def _gaussian_error(S, order, s2):
    """Data ~ N(0, s2): eps*(x, a) = sqrt(1 - a) x / (a s2 + 1 - a); the exact flow keeps x / sqrt(a s2 + 1 - a) constant.  float64
    throughout: ``dpmpp_coeffs64``, i.e. ``dpmpp_coeffs`` in front of its rounding to float32, which would hide the order below ~1e-7."""
    ac = _ac()
    t = logsnr_timesteps(S, ac)
    a = ac[t].astype(np.float64)
    a_prev = np.concatenate([[np.float64(ac[0])], a[:-1]])
    x = np.array([1.0, -0.7, 2.0])
    start = x / np.sqrt(a[-1] * s2 + 1 - a[-1])
    last, a_last = None, None
    for index in range(S - 1, -1, -1):
        a_t, a_p = a[index], a_prev[index]
        e = np.sqrt(1 - a_t) * x / (a_t * s2 + 1 - a_t)
        p = (x - np.sqrt(1 - a_t) * e) / np.sqrt(a_t)
        c_x, c_0, c_1 = dpmpp_coeffs64(a_t, a_p, a_last if (order == 2 and last is not None) else None)
        x = c_x * x + c_0 * p + (c_1 * last if (order == 2 and last is not None) else 0.0)
        last, a_last = p, a_t
    exact = start * np.sqrt(a_prev[0] * s2 + 1 - a_prev[0])
    return float(np.abs(x - exact).max() / np.abs(exact).max())


@pytest.mark.parametrize("s2", [0.25, 4.0])
def test_convergence_order(s2):
    e1 = {S: _gaussian_error(S, 1, s2) for S in (10, 20, 40)}
    e2 = {S: _gaussian_error(S, 2, s2) for S in (10, 20, 40)}
    print(f"[dpmpp] s2 {s2}: order 1 errors {e1}, ratios {e1[10] / e1[20]:.2f} {e1[20] / e1[40]:.2f}; "
          f"order 2 errors {e2}, ratios {e2[10] / e2[20]:.2f} {e2[20] / e2[40]:.2f}; gap at S = 20: {e1[20] / e2[20]:.1f}")
    assert e2[10] / e2[20] >= 3 and e2[20] / e2[40] >= 3
    assert 1.7 <= e1[10] / e1[20] <= 2.3 and 1.7 <= e1[20] / e1[40] <= 2.3
    assert e2[20] <= e1[20] / 5


# ---- the sampler on the emulation ---------------------------------------------------------------------------------------
def _setup():
    gold = cases.load_golden(dc.TAG)
    meta = gold["meta"]
    assert meta["S"] == dc.S
    cfg = cases.cfg_for(meta["cfg"], meta["variant"])
    inp = cases.build_inputs(meta)
    model = build_model(cfg)
    model._engine = UNetEngine(model, ops=EmulOpsDPMpp(torch.float32), use_graphs=False)
    model.first_conv_sd_override = synth.synth_first_conv_sd()
    gi = GroundingNetInput()
    model.grounding_tokenizer_input = gi
    sampler = DPMSolverSampler(_diffusion(), model, alpha_generator_func=partial(alpha_generator, type=meta["alpha_type"]),
                               set_alpha_scale=set_alpha_scale)
    return meta, inp, model, gi, sampler


def _oracle(meta):
    cfg = cases.cfg_for(meta["cfg"], meta["variant"])
    return ref_cpu.OracleModel(synth.synth_state_dict(cases.unet_schema(cfg)), cfg, synth.synth_first_conv_sd())


def _oracle_input(inp):
    return dict(x=inp["x"].clone(), timesteps=None, context=inp["context"], grounding_input=ref_cpu.prepare_grounding(inp["gb"]))


def _sampler_input(inp, gi):
    return dict(x=inp["x"].clone(), timesteps=None, context=inp["context"], grounding_input=gi.prepare(inp["gb"]))


def _inpaint(shape):
    from tests import ddim_mis_cases
    return ddim_mis_cases.make_inpaint(shape)


def _run(sampler, inp, gi, order, mask=None, x0=None, noises=(), discretize="uniform"):
    from tests import ddim_mis_cases
    drawn = ddim_mis_cases.replay(sampler, list(noises))
    calls = sampler.engine.ops.calls
    before = dict(calls)
    i0 = _sampler_input(inp, gi)
    out = sampler.sample(dc.S, tuple(inp["x"].shape), i0, uc=inp["uc"], guidance_scale=dc.GUIDANCE, mask=mask, x0=x0, order=order,
                         discretize=discretize)
    assert i0["x"] is out and int(i0["timesteps"][0]) == int(sampler.ddim_timesteps[0])
    return out, len(drawn), {k: v - before.get(k, 0) for k, v in calls.items() if v != before.get(k, 0)}


def test_order_one_is_ddim_eta_zero_on_the_trajectory():
    meta, inp, model, gi, sampler = _setup()
    with torch.no_grad():
        want = ddim_cases.ddim_reference(_oracle(meta), dc.S, _oracle_input(inp), inp["uc"], dc.GUIDANCE, eta=0.0,
                                         alpha_type=meta["alpha_type"], noises=[torch.zeros_like(inp["x"])] * dc.S)
        # the emulated engine against the oracle model is part of that figure: measure it with DDIM's own op on the same engine
        got, _, counts = _run(sampler, inp, gi, 1)
    err = cases.rel_rms(got, want)
    print(f"[emulated] tiny_box DPM-Solver++ order 1 vs ddim_reference eta 0: rel-rms {err:.3e} (bar {ORDER1_VS_DDIM_TOL:.0e})")
    assert counts.get("dpmpp_update") == dc.S and "dpmpp_update_order2" not in counts and "ddim_update" not in counts
    assert err < ORDER1_VS_DDIM_TOL


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "mask"])
@pytest.mark.parametrize("order", [1, 2])
def test_sampler_matches_the_composed_reference(order, masked):
    meta, inp, model, gi, sampler = _setup()
    shape = tuple(inp["x"].shape)
    mask, x0 = _inpaint(shape) if masked else (None, None)
    noises = dc.make_noises(shape, dc.S, masked)
    with torch.no_grad():
        want = dc.dpmpp_reference(_oracle(meta), dc.S, _oracle_input(inp), inp["uc"], dc.GUIDANCE, order=order,
                                  alpha_type=meta["alpha_type"], mask=mask, x0=x0, noises=noises)
    got, n, counts = _run(sampler, inp, gi, order, mask, x0, noises)
    err = cases.rel_rms(got, want)
    print(f"[emulated] tiny_box DPM-Solver++ order {order} mask {masked}: rel-rms {err:.3e} against dpmpp_reference (bar {EMUL_TRAJ_TOL:.0e})")
    assert n == len(noises) and torch.isfinite(got).all() and err < EMUL_TRAJ_TOL
    # per step: one forward, one dpmpp_update, no cfg_combine, one q_sample_blend iff masked
    assert counts.get("dpmpp_update") == dc.S and counts.get("dpmpp_update_order2", 0) == (dc.S - 1 if order == 2 else 0)
    assert counts.get("q_sample_blend", 0) == (dc.S if masked else 0)
    assert "cfg_combine" not in counts and "ddim_update" not in counts and "plms_update" not in counts
    assert _forwards(counts) == dc.S, counts


def _forwards(counts):
    """UNet forwards of a run: the emulation counts the first conv once per forward."""
    return counts.get("conv_in", -1)


def test_orders_differ_and_logsnr_runs():
    meta, inp, model, gi, sampler = _setup()
    o1, _, _ = _run(sampler, inp, gi, 1)
    o2, _, _ = _run(sampler, inp, gi, 2)
    assert not torch.equal(o1, o2)
    lg, _, counts = _run(sampler, inp, gi, 2, discretize="logsnr")
    assert sampler.ddim_timesteps.tolist() == [1, 33, 280, 703, 999] and torch.isfinite(lg).all() and counts["dpmpp_update"] == dc.S
    assert not torch.equal(lg, o2)


def test_an_all_zero_mask_is_no_mask():
    meta, inp, model, gi, sampler = _setup()
    shape = tuple(inp["x"].shape)
    _, x0 = _inpaint(shape)
    plain, n0, _ = _run(sampler, inp, gi, 2)
    masked, n1, _ = _run(sampler, inp, gi, 2, torch.zeros(shape[0], 1, *shape[2:]), x0, dc.make_noises(shape, dc.S, True))
    assert (n0, n1) == (0, dc.S) and torch.equal(plain, masked)


@pytest.mark.parametrize("order", [0, 3, "2", None, 1.5])
def test_order_must_be_one_or_two(order):
    sampler = DPMSolverSampler(_diffusion(), model=None)
    with pytest.raises(ValueError):
        sampler.sample(5, (1, 4, 8, 8), dict(x=None), order=order)


# ---- the shim -----------------------------------------------------------------------------------------------------------
def test_ldm_shim_and_signatures():
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler as Shim, DPMSolverSamplerInst as ShimInst
    from instancediffusion_amd.host.samplers import DDIMSamplerInst, DPMSolverSamplerInst, PLMSSamplerInst
    assert Shim is DPMSolverSampler and ShimInst is DPMSolverSamplerInst
    assert issubclass(Shim, _PLMSBase) and issubclass(ShimInst, DDIMSamplerInst)
    p = inspect.signature(Shim.sample).parameters
    assert list(p) == ["self", "S", "shape", "input", "uc", "guidance_scale", "mask", "x0", "order", "discretize"]
    assert (p["order"].default, p["discretize"].default, p["mask"].default, p["x0"].default) == (2, "uniform", None, None)
    assert list(inspect.signature(ShimInst.sample).parameters) == list(p)
    assert inspect.signature(ShimInst.__init__) == inspect.signature(PLMSSamplerInst.__init__)
    pl = inspect.signature(ShimInst.sample_layouts).parameters
    assert list(pl) == ["self", "S", "layouts", "uc", "guidance_scale", "order", "discretize", "masks", "x0s"]
    assert "eta" not in p and "eta" not in pl


# ---- C ABI --------------------------------------------------------------------------------------------------------------
def test_abi_symbol_prototype_and_argument_validation_without_gpu():
    """The symbol is exported with its prototype, the ABI version did not move, the header declares it, and every argument error is
    reported before anything touches a device (fake, never dereferenced pointers, as tests/test_capi.py does)."""
    from instancediffusion_amd import _lib
    lib = _lib.load()
    assert "idf_dpmpp_update" in _lib.SYMBOLS and len(_lib.SYMBOLS["idf_dpmpp_update"][1]) == 14
    assert lib.idf_dpmpp_update.argtypes is not None and len(lib.idf_dpmpp_update.argtypes) == 14
    assert lib.idf_abi_version() == 5
    header = open(os.path.join(REPO, "include", "idf.h")).read()
    assert "int idf_dpmpp_update(const float* x, const float* eps_cond, const float* eps_uncond" in header
    assert "#define IDF_ABI_VERSION 5" in header
    nan, inf = float("nan"), float("inf")

    def upd(x=0x10000, ec=0x20000, eu=0x30000, sa=0.65, s1m=0.76, c_x=0.9, c_0=0.2, c_1=-0.05, last=0x40000, out=0x50000, p0=0x60000, n=256):
        return lib.idf_dpmpp_update(x, ec, eu, 7.5, sa, s1m, c_x, c_0, c_1, last, out, p0, n, None)
    bad = [upd(x=None), upd(ec=None), upd(out=None), upd(p0=None), upd(n=0), upd(n=-4), upd(sa=0.0), upd(sa=-0.5), upd(sa=nan), upd(sa=inf),
           upd(s1m=nan), upd(c_x=nan), upd(c_x=inf), upd(c_0=nan), upd(c_0=-inf), upd(c_1=nan), upd(c_1=inf),
           upd(x=None, last=None), upd(c_0=nan, last=None, eu=None)]
    assert bad == [-1] * len(bad), bad
