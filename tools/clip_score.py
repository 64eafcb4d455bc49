#!/usr/bin/env python
"""Local CLIP score (the reference's ``eval/eval_attribute_binding.py:19-60,180-208``, HF branch) of the PNGs ``inference.py`` wrote
for a demo JSON: every instance box is cropped out of every image and compared with its instance prompt.

    python tools/clip_score.py --input_json demos/demo_four_boxes.json --images OUTPUT/gc7.5-seed0-alpha0.75 \\
        (--clip_path LOCAL_DIR | --synthetic_weights) [--backend hip|hf] [--dtype bf16|fp16] [--batched]

``--clip_path``: a local directory with ``openai/clip-vit-large-patch14`` (weights, ``vocab.json``, ``merges.txt``), loaded with
``local_files_only=True``: nothing is ever fetched.  ``--synthetic_weights``: a key-seeded ViT-L/14 ``CLIPModel`` (a dry run of the
whole path; the scores mean nothing); phrases are tokenised with the BPE vocabulary under ``$IDF_CLIP_PATH`` when there is one,
else with ``host.clip_score.hash_tokenize`` (documented there).  ``--backend hf`` (default) is ``transformers`` eager in fp32,
``--backend hip`` the HIP engines in ``--dtype`` storage.  Prints ONE JSON line: per image the per-instance scores, and the mean of
the per-image means.  ``--batched`` scores all PNGs in one ``score_batch`` call (same JSON keys): the same pixels as the per-image
path, bit for bit; on ``hip`` the features may differ by the GEMM kernel a chunk's row count selects (tests/test_clip_preproc_gpu.py).
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from instancediffusion_amd.host.clip_score import load_clip, synthetic_clip_model  # noqa: E402,F401  (the model lives in the package)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--input_json", required=True, help="the demo JSON inference.py was run on")
    ap.add_argument("--images", required=True, help="the folder inference.py wrote its PNGs into")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--clip_path", help="local directory of openai/clip-vit-large-patch14 (local_files_only)")
    src.add_argument("--synthetic_weights", action="store_true", help="key-seeded ViT-L/14 CLIPModel: a dry run")
    ap.add_argument("--backend", choices=["hf", "hip"], default="hf")
    ap.add_argument("--dtype", choices=["bf16", "fp16"], default="bf16", help="storage type of --backend hip")
    ap.add_argument("--batched", action="store_true",
                    help="read all PNGs (one size) into one uint8 batch and score it with InstanceClipScorer.score_batch: on --backend hip "
                         "crop and resize run on the device (idf_clip_crop_resize) and the tower sees all crops at once")
    ap.add_argument("--device", default=None, help="device of --backend hf (default: cuda when there is one)")
    args = ap.parse_args()

    import torch
    from PIL import Image
    from instancediffusion_amd.host import clip_score as cs
    data = json.load(open(args.input_json))
    boxes, phrases = cs.instances_from_demo_json(data)
    names = sorted((n for n in os.listdir(args.images) if n.lower().endswith(".png")),
                   key=lambda n: (0, int(n[:-4])) if n[:-4].isdigit() else (1, n))
    if not names:
        raise SystemExit(f"no PNG in {args.images}")
    model, tokenize, tokenizer = load_clip(None if args.synthetic_weights else args.clip_path)
    dev = args.device or ("cuda" if torch.cuda.is_available() else "cpu")
    model = model.to(dev)
    scorer = cs.InstanceClipScorer(model, tokenize, backend=args.backend,
                                   dtype=torch.bfloat16 if args.dtype == "bf16" else torch.float16)
    images = {}
    if args.batched:
        import numpy as np
        arrs = []
        for n in names:
            with Image.open(os.path.join(args.images, n)) as im:
                arrs.append(np.asarray(im.convert("RGB"), dtype=np.uint8))
        if len({a.shape for a in arrs}) != 1:
            raise SystemExit("--batched needs PNGs of one size")
        batch = torch.from_numpy(np.stack(arrs))
        for n, sc in zip(names, scorer.score_batch(batch.to(dev) if args.backend == "hip" else batch, boxes, phrases)):
            images[n] = [round(s, 6) for s in sc]
    else:
        for n in names:
            with Image.open(os.path.join(args.images, n)) as im:
                images[n] = [round(s, 6) for s in scorer.score(im.convert("RGB"), boxes, phrases)]
    means = [sum(v) / len(v) for v in images.values() if v]
    print(json.dumps(dict(metric="local CLIP score (eval_attribute_binding.py, HF branch)", input_json=args.input_json,
                          backend=args.backend, dtype=args.dtype if args.backend == "hip" else "fp32", tokenizer=tokenizer,
                          weights="synthetic" if args.synthetic_weights else args.clip_path, phrases=phrases, images=images,
                          mean=round(sum(means) / len(means), 6))))


if __name__ == "__main__":
    main()
