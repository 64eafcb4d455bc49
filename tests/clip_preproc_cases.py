"""The cases of the crop + bicubic-resize tests (tests/test_clip_preproc_host.py on the CPU, tests/test_clip_preproc_gpu.py on an
MI355X): seeded random uint8 source images and crop rectangles, chosen for the paths of Pillow's resample rule and of
``idf_clip_crop_resize``.  TEST INFRASTRUCTURE.

A case is (name, (B, H, W), [(image, x0, y0, x1, y1), ...]); ``cases(S)`` builds the list for target size S (one case depends on it).
"""
from __future__ import annotations

import functools

import numpy as np
import torch

SIZES = (56, 224)


def cases(S: int) -> list:
    return [
        # upscaling with both window ends clamped: every output index sees the whole 1- or 3/5-pixel axis
        ("crop 1x1", (1, 40, 48), [(0, 5, 7, 6, 8)]),
        ("crop 5x3", (1, 40, 48), [(0, 10, 20, 15, 23)]),
        ("whole 512x512 image", (1, 512, 512), [(0, 0, 0, 512, 512)]),                       # 11 taps at S = 224
        # the long side resizes well past S: only the centred window is computed
        ("crop 37x211", (1, 256, 64), [(0, 3, 5, 40, 216)]),
        ("crop 300x90", (1, 128, 320), [(0, 10, 20, 310, 110)]),
        ("short side exactly S", (1, S + 90, S + 8), [(0, 4, 7, 4 + S, 7 + S + 76)]),       # the horizontal pass is the identity
        ("crop 448x449", (1, 456, 456), [(0, 1, 2, 449, 451)]),                             # 8 taps across, 9 down at S = 224 (ksize 9 and 11)
        ("768x768 source", (1, 768, 768), [(0, 0, 0, 768, 768)]),                           # 15 taps at S = 224
        ("boxes touching all four edges", (1, 150, 200), [(0, 0, 0, 80, 60), (0, 120, 0, 200, 70), (0, 0, 90, 90, 150),
                                                         (0, 100, 80, 200, 150)]),
        ("crops from three images", (3, 96, 128), [(2, 5, 6, 100, 90), (0, 0, 0, 128, 96), (1, 30, 10, 60, 80)]),
        ("Ncrop = 7", (2, 120, 160), [(0, 0, 12, 80, 108), (1, 40, 0, 160, 72), (0, 64, 54, 152, 120), (1, 3, 3, 4, 100),
                                      (0, 0, 0, 160, 1), (1, 17, 19, 130, 111), (0, 80, 60, 81, 61)]),
    ]


@functools.lru_cache(maxsize=None)
def source_u8(shape, seed: int = 0) -> np.ndarray:
    """Seeded random uint8 [B, H, W, 3]."""
    B, H, W = shape
    return torch.randint(0, 256, (B, H, W, 3), generator=torch.Generator().manual_seed(1000 + seed + H * 7 + W), dtype=torch.uint8).numpy()


def quantiser_probes() -> torch.Tensor:
    """fp32 values that decide whether a quantiser follows ``inference.save_images`` (clamp to [-1, 1], * 0.5 + 0.5, * 255 in fp32,
    truncation): for every byte k the value (k / 255 - 0.5) * 2 and its two fp32 neighbours, -0.0, +-1 and their neighbours, and
    values beyond +-1."""
    k = torch.arange(256, dtype=torch.float32)
    v = ((k / 255 - 0.5) * 2).numpy()
    extra = np.array([-0.0, 0.0, 1.0, -1.0, 1.5, -1.5, 3.0e4, -3.0e4, 1e-30, -1e-30], dtype=np.float32)
    one = np.array([1.0, -1.0], dtype=np.float32)
    return torch.from_numpy(np.concatenate([v, np.nextafter(v, np.float32(2)), np.nextafter(v, np.float32(-2)), extra,
                                            np.nextafter(one, np.float32(2)), np.nextafter(one, np.float32(-2))]).astype(np.float32))


@functools.lru_cache(maxsize=None)
def source_f32(shape, seed: int = 0) -> torch.Tensor:
    """Seeded fp32 [B, 3, H, W] as a decoder would return it: half the elements uniform in [-1.2, 1.2], half drawn from
    ``quantiser_probes``; the first elements of every channel plane of image 0 list the probes in order where they fit."""
    B, H, W = shape
    g = torch.Generator().manual_seed(2000 + seed + H * 7 + W)
    probes = quantiser_probes()
    x = torch.rand((B, 3, H, W), generator=g) * 2.4 - 1.2
    pick = torch.randint(0, probes.numel(), (B, 3, H, W), generator=g)
    x = torch.where(torch.rand((B, 3, H, W), generator=g) < 0.5, probes[pick], x)
    n = min(probes.numel(), H * W)
    x[0].view(3, -1)[:, :n] = probes[:n]
    return x.contiguous()


def save_images_u8(images: torch.Tensor) -> np.ndarray:
    """The conversion of ``inference.save_images``, expression for expression, for a whole batch: fp32 [B, 3, H, W] -> uint8
    [B, H, W, 3]."""
    out = []
    for sample in images:
        sample = torch.clamp(sample, min=-1, max=1) * 0.5 + 0.5
        out.append((sample.float().cpu().numpy().transpose(1, 2, 0) * 255).astype(np.uint8))
    return np.stack(out)


def pil_reference(src_u8: np.ndarray, crops, S: int) -> torch.Tensor:
    """The PIL path: ``Image.crop`` + ``host.clip_score.preprocess`` per crop -> fp32 [N, 3, S, S]."""
    from PIL import Image
    from instancediffusion_amd.host.clip_score import preprocess
    pil = [Image.fromarray(a) for a in src_u8]
    return torch.stack([preprocess(pil[b].crop((x0, y0, x1, y1)), S) for b, x0, y0, x1, y1 in crops])
