"""Writes tests/golden/vae_enc_{tiny,full_128,full_512}.pt: ``AutoencoderKL.encode`` of the UNMODIFIED reference.

    IDF_REFERENCE=/path/to/InstanceDiffusion python tests/make_vae_encode_golden.py [--only TAG]

Generation time only: the reference tree (IDF_REFERENCE, default /root/reference) is imported as it is, its ``AutoencoderKL`` is
instantiated from its own configs/test_box.yaml (PyYAML; the variants of tests/vae_encode_cases.py override ddconfig), and the
key-name-seeded weights ``synth.synth_state_dict(schema, salt=7)`` are loaded with strict=True, as oracle/make_golden.py does for
the decoder goldens.  Tests never read the reference; a fixture holds tensors, floats and strings only:

  meta      the case (variant, batch, size, image seed), weight salt, noise seed
  x_fp      fingerprint (std, first 32 values) of the input image, rebuilt by tests/vae_encode_cases.encode_image
  w_fp      fingerprints of three weights
  moments   [B, 2E, H/f, W/f] fp32: posterior mean | logvar clamped to [-30, 20]  (DiagonalGaussianDistribution)
  z         ``torch.manual_seed(5); ae.encode(x)`` -- the posterior sample times scale_factor, noise from the CPU default generator
  probes    fingerprints of conv_in, every level's last block / downsample, the mid block, conv_out
  floor     the reference's OWN error when the same call runs under torch.autocast("cpu", dtype=torch.bfloat16), against its fp32
            result: moments rel-RMS, logvar max-abs and RMS error
  logvar_range   (min, max) of the unclamped logvar
"""
import argparse
import importlib.util
import os
import sys
import time

import torch
import yaml

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("IDF_REFERENCE", "/root/reference")


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@torch.no_grad()
def gen(tag, vc, synth, variants):
    from ldm.util import instantiate_from_config
    from ldm.modules.distributions.distributions import DiagonalGaussianDistribution
    c = vc.CASES[tag]
    t0 = time.time()
    cfg = yaml.safe_load(open(os.path.join(REF, "configs", "test_box.yaml")))["autoencoder"]
    v = dict(variants[c["variant"]])
    if "ch_mult" in v:
        v["ch_mult"] = list(v["ch_mult"])
    cfg["params"]["ddconfig"].update(v)
    ae = instantiate_from_config(cfg).eval()
    schema = {k: tuple(p.shape) for k, p in ae.state_dict().items()}
    sd = synth.synth_state_dict(schema, salt=vc.SALT)
    ae.load_state_dict(sd, strict=True)
    x = vc.encode_image(c["batch"], c["size"], c["seed"])

    probes, raw = {}, {}
    enc = ae.encoder
    hooks = [enc.conv_in.register_forward_hook(lambda m, a, o: probes.__setitem__("conv_in", vc.fp(o))),
             enc.mid.block_2.register_forward_hook(lambda m, a, o: probes.__setitem__("mid.block_2", vc.fp(o))),
             enc.conv_out.register_forward_hook(lambda m, a, o: probes.__setitem__("conv_out", vc.fp(o)))]
    qhook = ae.quant_conv.register_forward_hook(lambda m, a, o: raw.__setitem__("moments", o.detach().float().clone()))
    for i in range(enc.num_resolutions):
        hooks.append(enc.down[i].block[-1].register_forward_hook(lambda m, a, o, i=i: probes.__setitem__(f"down.{i}", vc.fp(o))))
        if i != enc.num_resolutions - 1:
            hooks.append(enc.down[i].downsample.register_forward_hook(
                lambda m, a, o, i=i: probes.__setitem__(f"down.{i}.downsample", vc.fp(o))))
    torch.manual_seed(vc.NOISE_SEED)
    z = ae.encode(x)
    torch.manual_seed(vc.NOISE_SEED)
    assert torch.equal(z, ae.encode(x)), "encode is not reproducible from torch.manual_seed"
    for h in hooks:
        h.remove()
    post = DiagonalGaussianDistribution(raw["moments"])
    moments = torch.cat([post.mean, post.logvar], 1).clone()
    lv_raw = torch.chunk(raw["moments"], 2, dim=1)[1]
    with torch.autocast("cpu", dtype=torch.bfloat16):
        ae.encode(x)
    qhook.remove()
    post16 = DiagonalGaussianDistribution(raw["moments"])
    floor = vc.moment_errors(torch.cat([post16.mean, post16.logvar], 1), moments)
    out = dict(meta=dict(c, tag=tag, salt=vc.SALT, noise_seed=vc.NOISE_SEED), x_fp=vc.fp(x),
               w_fp={k: vc.fp(sd[k]) for k in vc.FP_WEIGHTS}, moments=moments, z=z.detach().float().clone(), probes=probes,
               floor=floor, logvar_range=(float(lv_raw.min()), float(lv_raw.max())), scale_factor=float(ae.scale_factor),
               torch=str(torch.__version__))
    path = os.path.join(vc.GOLD, f"{tag}.pt")
    torch.save(out, path)
    print(f"[golden] {tag}: moments {list(moments.shape)}, logvar in [{out['logvar_range'][0]:.2f}, {out['logvar_range'][1]:.2f}], "
          f"bf16-autocast floor {floor}, {os.path.getsize(path) / 1024:.0f} KB, {time.time() - t0:.0f} s", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="all")
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    from tests import vae_encode_cases as vc           # torch only: nothing of this repository's ``ldm`` mirror is imported
    synth = _load("idf_synth", os.path.join(REPO, "instancediffusion_amd", "synth.py"))
    variants = {"full": {}, "tiny": dict(ch=64, ch_mult=[1, 2, 2], num_res_blocks=1)}     # = tests/cases.py VAE_VARIANTS
    # the reference tree must win over this repository's same-named ``ldm`` mirror package
    sys.path = [p for p in sys.path if os.path.abspath(p or ".") != REPO]
    sys.path.insert(0, REF)
    os.chdir(REF)
    for tag in vc.CASES:
        if args.only in ("all", tag):
            gen(tag, vc, synth, variants)


if __name__ == "__main__":
    main()
