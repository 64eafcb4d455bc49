"""Writes tests/golden/cli_ddim_latents.pt: the final latent tests/test_ddim_cli_gpu.py compares ``inference.py --sampler ddim`` with.

    python tests/make_cli_ddim_latents.py            # eight full-size fp32 CPU forwards

Like tests/golden/cli_latents.pt the fixture is ORACLE output, not reference output (``inference.py --synthetic_weights`` has no
counterpart a reference run could produce offline): ``tests/ddim_cases.ddim_reference`` over ``oracle/ref_cpu.OracleModel``, both
pinned to the reference's goldens by the CPU suite.  Everything that shapes the result is recorded next to it.
"""
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    from tests import test_ddim_cli_gpu as t
    t0 = time.time()
    lat, n = t._oracle_latent()
    out = dict(steps=t.STEPS, alpha=t.ALPHA, seed=t.SEED, eta=t.ETA, negative_prompt=t.DEFAULT_NEG, cfg=t.CFG, input_json=t.INPUT_JSON,
               torch=str(torch.__version__), latent=lat.float().contiguous(), n_forward=n)
    print(f"{n} oracle forwards in {time.time() - t0:.0f} s, latent rms {float(lat.float().pow(2).mean().sqrt()):.4f}", flush=True)
    torch.save(out, t.FIXTURE)
    print("wrote", t.FIXTURE)


if __name__ == "__main__":
    main()
