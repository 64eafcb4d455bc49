"""COCO run-length instance masks of the demo JSONs (``annos[i]["mask"] = {"size": [h, w], "counts": ..}``): parsing, the CPU
decoder, and the packed tables ``idf_rle_decode_planes`` (csrc/mask_input.hip) reads.

The reference decodes these with ``pycocotools`` and resizes with Pillow ``NEAREST`` to 512 x 512 (utils/input.py:161-186); this
module is that route without ``pycocotools``.  The format (cocoapi, maskApi.c ``rleFrString``): runs alternate 0, 1, 0, .. over the
COLUMN-MAJOR pixel index p = x * h + y, zero-length runs are legal; ``counts`` is a list of run lengths, or a string in which every
char minus 48 carries 5 value bits (low bits first), bit 0x20 = "another char follows", bit 0x10 of a count's last char = its sign;
from the fourth count on a value is a delta against the count two places before it.

Everything the kernel's launcher cannot check (its tables live in device memory) is checked here, before upload."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

Parsed = Tuple[int, int, np.ndarray]                  # (h, w, counts uint32)


def _counts_from_string(s) -> np.ndarray:
    if isinstance(s, str):
        s = s.encode("ascii", "strict") if s.isascii() else None
    if s is None:
        raise ValueError("RLE counts string is not ASCII")
    c = np.frombuffer(bytes(s), dtype=np.uint8).astype(np.int64) - 48
    if c.size == 0:
        return np.zeros(0, dtype=np.int64)
    if c.min() < 0 or c.max() > 63:
        raise ValueError("RLE counts string holds a char outside '0' .. 'o'")
    more = (c & 0x20) != 0
    if more[-1]:
        raise ValueError("RLE counts string is truncated: its last char announces another")
    last = np.flatnonzero(~more)                                   # the closing char of every count
    first = np.concatenate([[0], last[:-1] + 1])
    length = last - first + 1
    if length.max() > 7:                                           # 35 value bits: no count of a mask below 2^31 pixels needs more
        raise ValueError("RLE counts string holds a count of more than 7 chars")
    k = np.arange(c.size) - np.repeat(first, length)               # a char's place within its count
    x = np.add.reduceat((c & 0x1f) << (5 * k), first)
    x = np.where(c[last] & 0x10, x - (np.int64(1) << (5 * length)), x)                     # sign extension
    # counts[i] = x[i] + counts[i - 2] for i > 2: one running sum over the odd places, one over the even places from 2 on
    out = x.copy()
    out[1::2] = np.cumsum(x[1::2])
    out[2::2] = np.cumsum(x[2::2])
    return out


def parse_rle(mask) -> Parsed:
    """``{"size": [h, w], "counts": list of ints | compressed string}`` -> (h, w, counts uint32).  ValueError: a missing or
    malformed size, a truncated or malformed string, a negative count, sum(counts) != h * w, h * w >= 2^31."""
    if not isinstance(mask, dict) or "size" not in mask or "counts" not in mask:
        raise ValueError("an RLE mask is a dict with 'size' and 'counts'")
    size = mask["size"]
    if (not isinstance(size, (list, tuple)) or len(size) != 2
            or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1 for v in size)):
        raise ValueError(f"RLE size must be two positive ints [h, w], got {size!r}")
    h, w = int(size[0]), int(size[1])
    if h * w >= 2 ** 31:
        raise ValueError(f"RLE mask of {h} x {w} pixels: the decoder indexes pixels with 31 bits")
    counts = mask["counts"]
    if isinstance(counts, (str, bytes)):
        counts = _counts_from_string(counts)
    else:
        try:
            arr = np.asarray(counts)
        except Exception as e:                                     # a ragged list
            raise ValueError(f"RLE counts: {e}")
        if arr.ndim != 1 or (arr.size and not np.issubdtype(arr.dtype, np.integer)):
            raise ValueError("RLE counts must be a flat list of ints or a compressed string")
        counts = arr.astype(np.int64)
    if counts.size and counts.min() < 0:
        raise ValueError("RLE mask holds a negative run length")
    if int(counts.sum()) != h * w:
        raise ValueError(f"RLE runs cover {int(counts.sum())} pixels, the mask has {h} x {w} = {h * w}")
    return h, w, counts.astype(np.uint32)


def _parsed(mask) -> Parsed:
    return mask if isinstance(mask, tuple) else parse_rle(mask)


def nearest_index(n_out: int, n_in: int) -> np.ndarray:
    """Source index of every output index of Pillow's ``NEAREST`` resize n_in -> n_out: ((2 i + 1) n_in) // (2 n_out)."""
    return ((2 * np.arange(n_out, dtype=np.int64) + 1) * n_in) // (2 * n_out)


def decode_rle_reference(mask, size: Optional[int] = None) -> np.ndarray:
    """The CPU twin of ``idf_rle_decode_planes``: mask (dict or ``parse_rle`` result) -> uint8 {0, 1} [h, w], or [size, size] after
    ``PIL.Image.resize((size, size), NEAREST)`` -- the reference's ``annToMask`` + resize (utils/input.py:161-186)."""
    h, w, counts = _parsed(mask)
    values = (np.arange(counts.size) & 1).astype(np.uint8)
    m = np.ascontiguousarray(np.repeat(values, counts.astype(np.int64)).reshape(w, h).T)
    if size is None:
        return m
    from PIL import Image
    return np.asarray(Image.fromarray(m).resize((size, size), Image.NEAREST)).copy()


def pack_masks(parsed: Sequence[Parsed], size: Optional[int] = None) -> dict:
    """The tables of one ``idf_rle_decode_planes`` call, job m = ``parsed[m]``: ``ends`` uint32, the CUMULATIVE run ends of the
    masks, one after the other (an entry that IS an earlier entry -- one mask sent to two planes -- shares its runs);
    ``run_begin`` / ``run_end`` int32 [M], job m's range in ``ends``; ``src_hw`` int32 [M, 2].  Validated here, because the launcher
    cannot read device memory: the runs of every mask sum to h * w < 2^31 (so every end fits), and with ``size`` the output side
    times the longer source side stays below 2^31 (the kernel's 32-bit index arithmetic)."""
    M = len(parsed)
    chunks: List[np.ndarray] = []
    seen = {}
    rb, re, hw = np.zeros(M, np.int32), np.zeros(M, np.int32), np.zeros((M, 2), np.int32)
    total = 0
    for m, (h, w, counts) in enumerate(parsed):
        h, w = int(h), int(w)
        counts = np.asarray(counts)
        if h < 1 or w < 1 or h * w >= 2 ** 31 or counts.ndim != 1 or counts.dtype != np.uint32:
            raise ValueError(f"mask {m}: not a parse_rle result")
        if int(counts.sum(dtype=np.int64)) != h * w:
            raise ValueError(f"mask {m}: runs cover {int(counts.sum(dtype=np.int64))} pixels of {h} x {w}")
        if size is not None and max(h, w) * int(size) >= 2 ** 31:
            raise ValueError(f"mask {m}: {h} x {w} resized to {size} leaves the decoder's 32-bit index range")
        key = id(parsed[m][2])
        if key not in seen:
            seen[key] = (total, total + counts.size)
            chunks.append(np.cumsum(counts, dtype=np.int64).astype(np.uint32))
            total += counts.size
        rb[m], re[m] = seen[key]
        hw[m] = (h, w)
    if total >= 2 ** 31:
        raise ValueError("more than 2^31 runs in one call")
    ends = np.concatenate(chunks) if chunks else np.zeros(0, np.uint32)
    return dict(ends=ends, run_begin=rb, run_end=re, src_hw=hw)


def table_bytes(table: dict) -> int:
    """Bytes a ``pack_masks`` table (plus one destination plane per job) puts on the bus."""
    return int(table["ends"].nbytes + table["run_begin"].nbytes + table["run_end"].nbytes + table["src_hw"].nbytes
               + 4 * table["run_begin"].size)
