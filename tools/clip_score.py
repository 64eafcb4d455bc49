#!/usr/bin/env python
"""Local CLIP score (the reference's ``eval/eval_attribute_binding.py:19-60,180-208``, HF branch) of the PNGs ``inference.py`` wrote
for a demo JSON: every instance box is cropped out of every image and compared with its instance prompt.

    python tools/clip_score.py --input_json demos/demo_four_boxes.json --images OUTPUT/gc7.5-seed0-alpha0.75 \\
        (--clip_path LOCAL_DIR | --synthetic_weights) [--backend hip|hf] [--dtype bf16|fp16]

``--clip_path``: a local directory with ``openai/clip-vit-large-patch14`` (weights, ``vocab.json``, ``merges.txt``), loaded with
``local_files_only=True``: nothing is ever fetched.  ``--synthetic_weights``: a key-seeded ViT-L/14 ``CLIPModel`` (a dry run of the
whole path; the scores mean nothing); phrases are tokenised with the BPE vocabulary under ``$IDF_CLIP_PATH`` when there is one,
else with ``host.clip_score.hash_tokenize`` (documented there).  ``--backend hf`` (default) is ``transformers`` eager in fp32,
``--backend hip`` the HIP engines in ``--dtype`` storage.  Prints ONE JSON line: per image the per-instance scores, and the mean of
the per-image means.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# openai/clip-vit-large-patch14
CLIP_L14_VISION = dict(hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16, image_size=224,
                       patch_size=14, projection_dim=768, hidden_act="quick_gelu", layer_norm_eps=1e-5)
SYNTH_SALT = 31


def synthetic_clip_model():
    from transformers import CLIPConfig, CLIPModel
    from instancediffusion_amd import synth
    from instancediffusion_amd.host.text_encoder import CLIP_L14_TEXT
    model = CLIPModel(CLIPConfig(text_config=dict(CLIP_L14_TEXT), vision_config=dict(CLIP_L14_VISION), projection_dim=768)).eval()
    model.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items() if v.is_floating_point()},
                                                 SYNTH_SALT), strict=False)
    return model


def local_tokenizer(path):
    """The BPE tokenizer ``host/text_encoder.py`` uses, from local files only; None when the vocabulary is not there."""
    from transformers import CLIPTokenizer
    from instancediffusion_amd.host.text_encoder import CLIP_L14_TEXT
    try:
        tok = CLIPTokenizer.from_pretrained(path, local_files_only=True)
    except Exception:
        return None
    return tok if len(tok) >= CLIP_L14_TEXT["vocab_size"] else None     # transformers >= 5 builds an EMPTY tokenizer without files


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--input_json", required=True, help="the demo JSON inference.py was run on")
    ap.add_argument("--images", required=True, help="the folder inference.py wrote its PNGs into")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--clip_path", help="local directory of openai/clip-vit-large-patch14 (local_files_only)")
    src.add_argument("--synthetic_weights", action="store_true", help="key-seeded ViT-L/14 CLIPModel: a dry run")
    ap.add_argument("--backend", choices=["hf", "hip"], default="hf")
    ap.add_argument("--dtype", choices=["bf16", "fp16"], default="bf16", help="storage type of --backend hip")
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
    if args.synthetic_weights:
        model = synthetic_clip_model()
        tok = local_tokenizer(os.environ.get("IDF_CLIP_PATH", "openai/clip-vit-large-patch14"))
        tokenizer = "bpe" if tok is not None else "hash"
    else:
        from transformers import CLIPModel
        model = CLIPModel.from_pretrained(args.clip_path, local_files_only=True).eval()
        tok = local_tokenizer(args.clip_path)
        if tok is None:
            raise SystemExit(f"no CLIP BPE vocabulary (vocab.json, merges.txt) in {args.clip_path}")
        tokenizer = "bpe"
    vocab = int(model.config.text_config.vocab_size)
    tokenize = (lambda p: tok(p, truncation=True, max_length=77, return_tensors="pt")) if tok is not None \
        else (lambda p: cs.hash_tokenize(p, vocab))
    dev = args.device or ("cuda" if torch.cuda.is_available() else "cpu")
    model = model.to(dev)
    scorer = cs.InstanceClipScorer(model, tokenize, backend=args.backend,
                                   dtype=torch.bfloat16 if args.dtype == "bf16" else torch.float16)
    images = {}
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
