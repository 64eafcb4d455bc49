"""Generate ``tests/golden/clip_vision_full.pt`` with ``transformers`` on the CPU.  TEST INFRASTRUCTURE.
Run: ``python tests/make_clip_vision_golden.py`` (minutes: a ViT-L/14 forward in fp32, bf16 and fp16).

Stored, for the full-size image tower of tests/clip_vision_cases.py (key-seeded weights, B = 2 seeded images): the fp32 outputs
``image_embeds``, ``pooler_output`` and nine rows of ``last_hidden_state`` (the class row and ``FULL_ROWS``), and the FLOORS: the
rel-RMS of the same module cast to bf16 / fp16 against its own fp32 output, per output (``last_hidden_state``: over the nine
stored rows).  And for ``text_features``: ``CLIPModel.get_text_features`` of the full-size text transformer of
tests/golden/clip_text.pt under a key-seeded ``text_projection``, on that golden's ids, with its floors.
tests/test_clip_vision_gpu.py holds the HIP engines to 1.5 x these floors.
"""
from __future__ import annotations

import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tests import clip_cases, clip_vision_cases as vc  # noqa: E402


def stored_rows(z: torch.Tensor) -> torch.Tensor:
    return z[:, (0,) + vc.FULL_ROWS].clone()


def main():
    import transformers
    torch.manual_seed(0)
    px = vc.pixel_values(2, vc.FULL_VISION["image_size"])

    def run(m):
        out = vc.vision_reference(m, px)
        out["last_hidden_state"] = stored_rows(out["last_hidden_state"])
        return out
    ref, floors = vc.with_floors(vc.full_vision(), run)
    for k, v in ref.items():
        assert bool(torch.isfinite(v).all()) and float(v.std()) > 1e-3, f"degenerate golden: {k}"
        for dt in floors:
            assert 1e-5 < floors[dt][k] < 0.1, (dt, k, floors[dt][k])
    print(f"[golden] vision floors {floors}")

    text = clip_cases.load_golden("clip_text")
    ids = text["input_ids"]
    model = vc.full_text_clip_model()
    tref, tfloors = vc.with_floors(model, lambda m: dict(text_features=vc.features(m.get_text_features(input_ids=ids)).float()))
    assert float(tref["text_features"].std()) > 1e-3
    print(f"[golden] text_features {tuple(tref['text_features'].shape)} floors {tfloors}")

    out = dict(meta=dict(tag="clip_vision_full", config=dict(vc.FULL_VISION), salt=vc.FULL_SALT, proj_salt=vc.PROJ_SALT, batch=2,
                         rows=[0] + list(vc.FULL_ROWS), transformers=transformers.__version__),
               last_hidden_state_rows=ref["last_hidden_state"], pooler_output=ref["pooler_output"], image_embeds=ref["image_embeds"],
               floors=floors, text_features=tref["text_features"], text_floors={dt: v["text_features"] for dt, v in tfloors.items()})
    path = os.path.join(REPO, "tests", "golden", "clip_vision_full.pt")
    torch.save(out, path)
    assert os.path.getsize(path) < 1_000_000
    print(f"[golden] wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
