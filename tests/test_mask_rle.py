"""COCO run-length masks on the host (instancediffusion_amd/host/masks.py): the parser against the recorded results of the upstream
"corgi kitchen" demo's eight masks (tests/golden/rle_masks.json), a round trip through a test-side encoder written from the format's
description (cocoapi ``rleToString``), every rejection, the integer form of Pillow's NEAREST index the kernel uses, and the
unchanged default of ``meta_from_demo_json``.  The device half is tests/test_mask_rle_gpu.py; shared cases live here."""
import json
import os

import numpy as np
import pytest

from instancediffusion_amd.host.masks import decode_rle_reference, nearest_index, pack_masks, parse_rle

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fixture():
    with open(os.path.join(REPO, "tests", "golden", "rle_masks.json")) as f:
        return json.load(f)


# ---- test-side encoder (independent of the parser: cocoapi's rleEncode / rleToString, written as loops) -------------------------
def encode_counts(mask: np.ndarray) -> list:
    """uint8 {0, 1} [h, w] -> run lengths over the column-major pixel order, the first run counting zeros."""
    counts, cur, n = [], 0, 0
    for v in mask.T.reshape(-1).tolist():
        if v != cur:
            counts.append(n)
            cur, n = v, 0
        n += 1
    counts.append(n)
    return counts


def compress(counts) -> str:
    out = []
    for i, x in enumerate(counts):
        x = int(x)
        if i > 2:
            x -= int(counts[i - 2])
        more = True
        while more:
            c = x & 0x1f
            x >>= 5
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            out.append(chr(c + 48))
    return "".join(out)


def blobs(h, w, seed, n=6):
    """A random mask of a few filled ellipses: long and short runs, columns without foreground."""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w), np.uint8)
    for _ in range(n):
        cy, cx, ry, rx = g.uniform(0, h), g.uniform(0, w), g.uniform(1, h / 3 + 1), g.uniform(1, w / 3 + 1)
        m |= (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1).astype(np.uint8)
    return m


def round_trip_cases():
    g = np.random.default_rng(11)
    cases = {"1x1_one": np.ones((1, 1), np.uint8), "1x1_zero": np.zeros((1, 1), np.uint8)}
    for h, w in ((3, 5), (7, 1), (64, 48)):
        cases[f"{h}x{w}"] = (g.random((h, w)) < 0.5).astype(np.uint8)
    cases["64x48_blobs"] = blobs(64, 48, 3)
    cases["all_zero"] = np.zeros((9, 4), np.uint8)
    cases["all_one"] = np.ones((9, 4), np.uint8)
    return cases


# ---- the parser against the fixture ---------------------------------------------------------------------------------------------
def test_fixture_masks_decode_to_the_recorded_areas_and_boxes():
    fx = fixture()
    assert len(fx["masks"]) == 8
    areas = []
    for m in fx["masks"]:
        h, w, counts = parse_rle(m)
        assert (h, w) == (512, 512) and counts.dtype == np.uint32 and int(counts.sum()) == 512 * 512
        d = decode_rle_reference(m)
        assert d.shape == (512, 512) and d.dtype == np.uint8 and set(np.unique(d)) <= {0, 1}
        areas.append(int(d.sum()))
        ys, xs = np.nonzero(d)
        x0, y0, x1, y1 = xs.min(), ys.min(), xs.max() + 1, ys.max() + 1
        bx, by, bw, bh = m["bbox"]
        assert x0 >= bx - 16 and y0 >= by - 16 and x1 <= bx + bw + 16 and y1 <= by + bh + 16, (m["bbox"], (x0, y0, x1, y1))
        if "tight_box" in m:
            assert [x0, y0, x1 - x0, y1 - y0] == m["tight_box"]
        assert np.array_equal(decode_rle_reference(m, 512), d)                    # 512 -> 512 NEAREST is the identity
    assert areas == [46505, 2325, 5083, 6161, 2474, 2709, 15018, 72389] == [m["area"] for m in fx["masks"]]


def test_fixture_strings_survive_the_test_side_encoder():
    for m in fixture()["masks"]:
        counts = parse_rle(m)[2]
        assert compress(counts.tolist()) == m["counts"]
        assert encode_counts(decode_rle_reference(m)) == counts.tolist()


# ---- round trip -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(round_trip_cases()))
def test_round_trip(name):
    mask = round_trip_cases()[name]
    h, w = mask.shape
    counts = encode_counts(mask)
    if name == "all_one":
        assert counts == [0, h * w]
    if name == "all_zero":
        assert counts == [h * w]
    for form in (counts, compress(counts), compress(counts).encode()):
        ph, pw, pc = parse_rle({"size": [h, w], "counts": form})
        assert (ph, pw) == (h, w) and pc.dtype == np.uint32 and pc.tolist() == counts
        assert np.array_equal(decode_rle_reference({"size": [h, w], "counts": form}), mask)


def test_zero_length_run_in_the_middle():
    counts = [5, 3, 0, 4, 6, 0, 0, 2]                         # 20 pixels of a 4 x 5 mask: the zero runs flip the parity in place
    want = np.repeat(np.arange(8) & 1, counts).astype(np.uint8).reshape(5, 4).T
    for form in (counts, compress(counts)):
        h, w, pc = parse_rle({"size": [4, 5], "counts": form})
        assert pc.tolist() == counts
        assert np.array_equal(decode_rle_reference((h, w, pc)), want)
    assert want.sum() == 3 + 4 + 2                            # runs 1, 3, 7 are ones (5 is an empty one-run)


def test_large_deltas_and_negative_deltas_round_trip():
    counts = [100000, 1, 70000, 65535, 3, 1, 40000]
    n = sum(counts)
    assert parse_rle({"size": [n, 1], "counts": compress(counts)})[2].tolist() == counts


# ---- rejections -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", [
    {"counts": [4]},                                          # no size
    {"size": [2, 2]},                                         # no counts
    {"size": [2], "counts": [4]},
    {"size": "2x2", "counts": [4]},
    {"size": [2, 0], "counts": []},
    {"size": [2, -2], "counts": [4]},
    {"size": [2.0, 2], "counts": [4]},
    {"size": [2, 2], "counts": [3]},                          # sum != h * w
    {"size": [2, 2], "counts": [2, 3]},
    {"size": [2, 2], "counts": [5, -1]},                      # negative run in a list
    {"size": [2, 2], "counts": [1.5, 2.5]},
    {"size": [2, 2], "counts": [[4]]},
    {"size": [2, 2], "counts": chr(((ord(compress([4])) - 48) | 0x20) + 48)},                # "more" on the last char: truncated
    {"size": [40, 1], "counts": compress([36, 4])[:1]},       # cut inside a two-char count
    {"size": [2, 2], "counts": "4~"},                         # a char outside the alphabet
    {"size": [2, 2], "counts": "4é"},
    {"size": [46341, 46341], "counts": [46341 * 46341]},      # h * w >= 2^31
    {"size": [1, 2 ** 31], "counts": [2 ** 31]},
    None, [4],
])
def test_parse_rle_rejects(mask):
    with pytest.raises(ValueError):
        parse_rle(mask)


def test_negative_count_after_delta_decoding_is_rejected():
    s = compress([3, 2, 1, 1]) + chr(48 + 0x1d)               # a fifth count of delta -3 against counts[2] = 1: -2
    with pytest.raises(ValueError, match="negative"):
        parse_rle({"size": [5, 1], "counts": s})
    assert 36 >= 32 and len(compress([36, 4])) == 3           # the two-char count the truncation case above cuts


def test_pack_masks_tables_and_validation():
    a = parse_rle({"size": [3, 5], "counts": [4, 3, 8]})
    b = parse_rle({"size": [2, 2], "counts": [0, 4]})
    t = pack_masks([a, b, a], size=8)
    assert t["ends"].dtype == np.uint32 and t["ends"].tolist() == [4, 7, 15, 0, 4]             # the shared mask is stored once
    assert t["run_begin"].tolist() == [0, 3, 0] and t["run_end"].tolist() == [3, 5, 3]
    assert t["src_hw"].tolist() == [[3, 5], [2, 2], [3, 5]] and t["src_hw"].dtype == np.int32 and t["run_begin"].dtype == np.int32
    assert pack_masks([])["ends"].size == 0
    with pytest.raises(ValueError):
        pack_masks([(3, 5, np.array([4, 3, 7], np.uint32))])                                   # runs do not cover the mask
    with pytest.raises(ValueError):
        pack_masks([(3, 5, np.array([4, 3, 8], np.int64))])                                    # not a parse_rle result
    with pytest.raises(ValueError):
        pack_masks([(2 ** 22, 1, np.array([2 ** 22], np.uint32))], size=512)                   # S * h leaves 32-bit index arithmetic


# ---- Pillow's NEAREST is the integer index the kernel computes ----------------------------------------------------------------------
def test_nearest_index_is_pillow_nearest_for_every_source_size():
    from PIL import Image
    for size in (512, 64):
        for n in range(1, 1101):
            ramp = np.arange(n, dtype=np.int32)                                                # a pixel's value is its index
            got_x = np.asarray(Image.fromarray(ramp[None, :].repeat(2, 0), mode="I").resize((size, 2), Image.NEAREST))[0]
            got_y = np.asarray(Image.fromarray(ramp[:, None].repeat(2, 1), mode="I").resize((2, size), Image.NEAREST))[:, 0]
            want = nearest_index(size, n)
            assert np.array_equal(got_x, want) and np.array_equal(got_y, want), (n, size)


def test_reference_resize_uses_that_index():
    m = blobs(37, 53, 5)
    counts = encode_counts(m)
    got = decode_rle_reference({"size": [37, 53], "counts": counts}, 64)
    assert np.array_equal(got, m[nearest_index(64, 37)][:, nearest_index(64, 53)]) and got.dtype == np.uint8


# ---- the default of meta_from_demo_json is what it was ------------------------------------------------------------------------------
# sha256 (first 16 hex digits) of json.dumps of the meta without ``segs``, recorded from the code before ``instance_masks`` existed
META_DIGEST = {"demo_four_boxes.json": "4e75e71921228f96", "demo_points.json": "62c34491ac648868",
               "demo_scribbles.json": "3587ff4534a46cec"}


@pytest.mark.parametrize("demo", sorted(META_DIGEST))
def test_meta_from_demo_json_default_is_unchanged(demo):
    import hashlib
    from instancediffusion_amd.host.input import meta_from_demo_json, prepare_instance_meta, rescale_box
    data = json.load(open(os.path.join(REPO, "demos", demo)))
    meta = meta_from_demo_json(json.loads(json.dumps(data)), 0.75, ckpt="c", save_folder_name="f")
    again = meta_from_demo_json(json.loads(json.dumps(data)), 0.75, ckpt="c", save_folder_name="f", instance_masks="ignore")
    n = len(data["annos"])
    assert list(meta) == ["ckpt", "prompt", "phrases", "polygons", "scribbles", "segs", "locations", "points", "alpha_type",
                          "save_folder_name"]                                                  # no new key, the old order
    assert list(again) == list(meta)
    for k in meta:
        assert np.array_equal(np.asarray(meta[k], dtype=object), np.asarray(again[k], dtype=object)) if k != "segs" \
            else np.array_equal(meta[k], again[k])
    assert meta["segs"].shape == (n, 512, 512) and meta["segs"].dtype == np.float32 and not meta["segs"].any()
    assert meta["polygons"] == [[0.0] * 512] * n and meta["phrases"] == [a["caption"] for a in data["annos"]]
    assert meta["locations"] == [rescale_box(a.get("bbox", [0, 0, 0, 0]), data["width"], data["height"]) for a in data["annos"]]
    for m in (meta, again):
        rest = {k: v for k, v in m.items() if k != "segs"}
        assert hashlib.sha256(json.dumps(rest).encode()).hexdigest()[:16] == META_DIGEST[demo]
    assert meta["alpha_type"] == [0.75, 0.0, 0.25] and meta["prompt"] == data["caption"]
    assert list(prepare_instance_meta(meta, 0)) == ["ckpt", "phrases", "locations", "polygons", "segs", "scribbles", "points",
                                                    "alpha_type", "prompt", "file_name", "save_folder_name"]
    with pytest.raises(ValueError):
        meta_from_demo_json(data, 0.75, instance_masks="yes")


def test_meta_from_demo_json_with_masks_and_the_host_route():
    import torch
    from instancediffusion_amd.host.input import meta_from_demo_json, prepare_batch, prepare_instance_meta
    fx = fixture()
    annos = [dict(bbox=m["bbox"], mask=dict(size=m["size"], counts=m["counts"]), caption=f"thing {i}")
             for i, m in enumerate(fx["masks"][:2])]
    annos.append(dict(bbox=[10, 10, 50, 50], mask=[], caption="no mask"))
    annos.append(dict(bbox=[10, 10, 50, 50], caption="no mask key"))
    data = dict(caption="a scene", width=512, height=512, annos=annos)
    meta = meta_from_demo_json(data, 0.75, instance_masks="json")
    assert [r is None for r in meta["rle"]] == [False, False, True, True] and not meta["segs"].any()
    assert meta["rle"][1][2].tolist() == parse_rle(annos[1]["mask"])[2].tolist()
    im = prepare_instance_meta(meta, 1)
    assert im["rle"] == [meta["rle"][1]]

    class Enc:
        def pooled(self, phrase):
            return torch.ones(768)
    meta["instance_meta"] = [prepare_instance_meta(meta, i) for i in range(4)]
    b = prepare_batch(meta, batch=2, max_objs=30, model=Enc(), device="cpu")
    assert b["mask_areas"] == [fx["masks"][0]["area"], fx["masks"][1]["area"], -1, -1]
    assert b["segs"].shape == (2, 30, 512, 512) and b["segs"].stride(0) == 0
    for k in range(2):
        want = torch.from_numpy(decode_rle_reference(annos[k]["mask"], 512).astype(np.float32))
        assert torch.equal(b["segs"][1, k], want)
        assert torch.equal(b["instance_meta"][k]["segs"][0, 0], want) and not b["instance_meta"][k]["segs"][0, 1:].any()
    assert not b["segs"][0, 2:].any() and not b["instance_meta"][2]["segs"].any()
    bad = json.loads(json.dumps(data))
    bad["annos"][0]["mask"]["counts"] = bad["annos"][0]["mask"]["counts"][:-3]
    with pytest.raises(ValueError):
        meta_from_demo_json(bad, 0.75, instance_masks="json")
    assert "rle" not in meta_from_demo_json(bad, 0.75)                                         # ignored masks are not even parsed
