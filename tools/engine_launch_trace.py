"""Launch trace of the UNet engine's forward on the CPU op emulation, across the engine's host-side knobs (engine.EngineKnobs).

For every combination it prints one markdown table row: the number of ops calls of one forward, a hash of the trace and a hash of
eps.  The trace has one line per ops call (allocations included, so the moment a buffer is first asked for is part of it): the
method, and per argument the shape, dtype, strides and buffer identity of a tensor -- its role in ``eng._bufs``, or for weights
and conditioning the ordinal of first appearance, plus the storage offset -- or the value of a scalar, None included.  A change
to the engine's host code that is meant to leave the launch sequence alone must reproduce the table in
profiles/engine_stats_routing.md:

    python tools/engine_launch_trace.py > table.md          # the full matrix, a few minutes
    python tools/engine_launch_trace.py --dump DIR          # ... and every trace in full under DIR, to diff one that moved

Inputs: the `mid` model of test_box.yaml at 16 x 16 latents, batch 2 + 2 as a [cond | uncond] pair (the 320-channel level has 256
tokens: fused q | k | v; the deeper levels take the unfused path).
"""
import dataclasses
import hashlib
import inspect
import itertools
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests.emul_ops import EmulOps  # noqa: E402

QUERIES = ("mlp_supported", "mlp_pack", "proj_row_takes", "gn_partial_shape")        # they launch and allocate nothing


class Takes(EmulOps):
    def proj_row_takes(self, M, C):
        return C == 320


class DeclinesFold(EmulOps):
    def conv_up2x(self, x, w, out, bias=None):
        return False


class Recorder:
    """Forwards to ``inner`` and, once ``eng`` is set, logs every call that is not a query."""

    def __init__(self, inner):
        self.inner, self.eng, self.log, self.ordinals = inner, None, [], {}

    def __getattr__(self, name):
        f = getattr(self.inner, name)
        if not callable(f) or name in QUERIES or self.eng is None:
            return f

        def call(*a, **k):
            bound = inspect.signature(f).bind(*a, **k)
            bound.apply_defaults()
            self.log.append(f"{name}(" + ", ".join(f"{n}={self.desc(v)}" for n, v in bound.arguments.items()) + ")")
            return f(*a, **k)
        return call

    def desc(self, v):
        if isinstance(v, (tuple, list)):
            return "(" + ", ".join(self.desc(e) for e in v) + ")"
        if not torch.is_tensor(v):
            return repr(v)
        ptr = v.untyped_storage().data_ptr()
        roles = {t.untyped_storage().data_ptr(): f"{role}{list(shape)}" for (role, shape, _), t in self.eng._bufs.items()}
        ident = roles.get(ptr) or f"w{self.ordinals.setdefault(ptr, len(self.ordinals))}"
        return f"<{ident}+{v.storage_offset()} {list(v.shape)} {str(v.dtype)[6:]} {list(v.stride())}>"


def make_engine(model, ops, **kn):
    from instancediffusion_amd.engine import EngineKnobs, UNetEngine
    return UNetEngine(model, ops=ops, use_graphs=False, knobs=dataclasses.replace(EngineKnobs.from_env(), **kn))


def combinations():
    """(name, knob values, fuser scale, paired, ops class)"""
    for ln, row, mm, fz, pr, tk, (vg, vn) in itertools.product((0, 1, 2), (True, False), (0, 1 << 30), (1.0, 0.0), (True, False),
                                                               (True, False), ((True, 256), (True, 1024), (False, 256))):
        yield (f"ln_self {ln}, qkv_row {int(row)}, mlp_min_m {mm}, fuser {fz:g}, paired {int(pr)}, takes {int(tk)}, vt ({int(vg)}, {vn})",
               dict(ln_self=ln, qkv_row=row, mlp_min_m=mm, vt_global=vg, vt_min_n=vn), fz, pr, Takes if tk else EmulOps)
    for name, kn, cls in (("gn_epi 0", dict(gn_epi=False), EmulOps), ("up_fold 1, conv_up2x declines", dict(up_fold=True), DeclinesFold),
                          ("up_fold 0, conv_up2x declines", dict(up_fold=False), DeclinesFold), ("pair_hoist 0", dict(pair_hoist=False), EmulOps),
                          ("geglu_period 64", dict(geglu_period=64, mlp_fused=False), EmulOps), ("defaults", {}, EmulOps)):
        yield name + ", fuser 1, paired 1", kn, 1.0, True, cls


def main():
    from grounding_input.text_grounding_tokinzer_input import GroundingNetInput
    from instancediffusion_amd import synth
    from instancediffusion_amd.engine import Cond
    from tests import cases
    from tests.test_engine_emulated import build_model
    dump = sys.argv[sys.argv.index("--dump") + 1] if "--dump" in sys.argv else None
    model = build_model(cases.cfg_for("test_box.yaml", "mid"))
    g = torch.Generator().manual_seed(41)
    gb = synth.make_grounding_batch(2, synth.random_boxes(3, g), g)
    x = torch.randn(2, 4, 16, 16, generator=g)
    ctx, uc = torch.randn(2, 77, 768, generator=g), torch.randn(2, 77, 768, generator=g)
    t = torch.tensor([700.0, 300.0])
    gi = GroundingNetInput()
    grounding, null = gi.prepare(gb), gi.get_null_input(batch=2)
    print("| combination | ops calls | trace sha256 | eps sha256 |\n|---|---|---|---|")
    for i, (name, kn, scale, paired, cls) in enumerate(combinations()):
        rec = Recorder(cls(torch.float32, batch_invariant=True))
        with torch.no_grad():
            eng = make_engine(model, rec, **kn)
            eng.set_fuser_scale(scale)
            pair = Cond.cat([eng.prepare_cond(ctx, grounding), eng.prepare_cond(uc, null)])
            rec.eng = eng
            eps = eng.forward_cond(torch.cat([x, x]), torch.cat([t, t]), pair, paired=paired)
        rec.eng = None                                       # (the engine and its ops refer to each other: let the weights go now)
        assert torch.isfinite(eps).all(), name
        trace = "\n".join(rec.log) + "\n"
        if dump:
            os.makedirs(dump, exist_ok=True)
            with open(os.path.join(dump, f"{i:03d}.txt"), "w") as fh:
                fh.write(name + "\n" + trace)
        print(f"| {name} | {len(rec.log)} | {hashlib.sha256(trace.encode()).hexdigest()[:16]} | "
              f"{hashlib.sha256(eps.numpy().tobytes()).hexdigest()[:16]} |", flush=True)


if __name__ == "__main__":
    main()
