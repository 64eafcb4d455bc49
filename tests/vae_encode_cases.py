"""Shared pieces of the VAE encoder tests (tests/test_vae_encode_emulated.py, tests/test_vae_encode_gpu.py) and of the
fixture generator tests/make_vae_encode_golden.py: the cases, the seeded input image, the fingerprints that tie a fixture
to its inputs, and the CPU emulation of the two encoder-only ops (TEST DOUBLE, as tests/emul_ops.py)."""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from tests.emul_ops import EmulOps

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SALT = 7                    # weights: synth.synth_state_dict(schema, salt=7), as the decoder goldens
NOISE_SEED = 5              # torch.manual_seed(NOISE_SEED); ae.encode(x) -- the posterior noise is the CPU default generator's
CASES = {                   # tag -> (VAE variant of tests/cases.py, batch, image size, image seed)
    "vae_enc_tiny": dict(variant="tiny", batch=2, size=64, seed=101),
    "vae_enc_full_128": dict(variant="full", batch=1, size=128, seed=102),
    "vae_enc_full_512": dict(variant="full", batch=1, size=512, seed=103),
}
FP_WEIGHTS = ("encoder.conv_in.weight", "encoder.down.1.downsample.conv.weight", "quant_conv.weight")


def fp(t: torch.Tensor) -> dict:
    t = t.detach().float()
    return dict(std=float(t.std()), head=t.flatten()[:32].clone())


def fp_matches(t: torch.Tensor, want: dict) -> bool:
    got = fp(t)
    return abs(got["std"] - want["std"]) <= 1e-6 * max(1.0, abs(want["std"])) and torch.allclose(got["head"], want["head"], atol=1e-6, rtol=1e-6)


def encode_image(batch: int, size: int, seed: int, width: int = 0) -> torch.Tensor:
    """Smooth, image-like input in [-1, 1]: seeded uniform noise, reflect-pad + 5x5 box blur, x2."""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(batch, 3, size, width or size, generator=g) * 2 - 1
    u = F.avg_pool2d(F.pad(u, (2, 2, 2, 2), mode="reflect"), 5, stride=1)
    return (u * 2).clamp(-1, 1).contiguous()


def load(tag: str) -> dict:
    return torch.load(os.path.join(GOLD, f"{tag}.pt"), weights_only=False)


def build(tag: str):
    """(host AutoencoderKL with the fixture's weights, input image, fixture); asserts the fingerprints of both."""
    from tests import cases
    gold = load(tag)
    c = CASES[tag]
    assert gold["meta"] == dict(c, tag=tag, salt=SALT, noise_seed=NOISE_SEED), "stale fixture: regenerate with tests/make_vae_encode_golden.py"
    ae = cases.build_vae(cases.vae_cfg_for(c["variant"]), SALT)
    x = encode_image(c["batch"], c["size"], c["seed"])
    assert fp_matches(x, gold["x_fp"]), "stale fixture: the input image is not the one the reference saw"
    sd = ae.state_dict()
    for k in FP_WEIGHTS:
        assert fp_matches(sd[k], gold["w_fp"][k]), f"stale fixture: {k} is not the weight the reference saw"
    return ae, x, gold


def down_reference(x_nchw: torch.Tensor, w_oihw: torch.Tensor, bias=None) -> torch.Tensor:
    """The encoder's Downsample: zero-pad right and bottom only, then 3x3 stride 2 without padding."""
    return F.conv2d(F.pad(x_nchw, (0, 1, 0, 1)), w_oihw, bias, stride=2)


class EncEmulOps(EmulOps):
    """EmulOps + the two ops only the encoder uses."""

    def conv3x3_down(self, x, w, out, *, bias=None, res=None, gn_partial=None):
        self._count("conv3x3_down")
        assert gn_partial is None
        B, H, W_, Cin = x.shape
        assert Cin % 64 == 0 and H >= 2 and W_ >= 2
        Cout = w.shape[0]
        wt = w.float().reshape(Cout, 3, 3, Cin).permute(0, 3, 1, 2)
        y = down_reference(x.float().permute(0, 3, 1, 2), wt)
        if bias is not None:
            y = y + bias.view(1, -1, 1, 1)
        if res is not None:
            y = y + res.float().permute(0, 3, 1, 2)
        out.copy_(y.permute(0, 2, 3, 1))
        return out

    def vae_posterior(self, h, w, bias, noise, scale, z, moments=None):
        self._count("vae_posterior")
        m = torch.einsum("oc,bchw->bohw", w, h)
        if bias is not None:
            m = m + bias.view(1, -1, 1, 1)
        mean, logvar = torch.chunk(m, 2, dim=1)
        logvar = torch.clamp(logvar, -30.0, 20.0)
        v = mean if noise is None else mean + torch.exp(0.5 * logvar) * noise
        z.copy_(v * scale)
        if moments is not None:
            moments.copy_(torch.cat([mean, logvar], 1))
        return z


def moment_errors(moments: torch.Tensor, want: torch.Tensor) -> dict:
    """rel-RMS of the moments, max-abs and RMS error of the (clamped) logvar half -- the figures a fixture's `floor` holds."""
    a, b = moments.double().cpu(), want.double().cpu()
    E = b.shape[1] // 2
    d = a[:, E:] - b[:, E:]
    rel = float(((a - b).pow(2).mean() / b.pow(2).mean().clamp_min(1e-30)).sqrt())
    return dict(moments_rel_rms=rel, logvar_max_abs=float(d.abs().max()), logvar_rms=float(d.pow(2).mean().sqrt()))
