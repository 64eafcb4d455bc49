"""Host mirror of ``utils/input.py``: the grounding-input builder that feeds the sampling path.

Same functions, argument meaning and output dict as the reference (``prepare_batch`` utils/input.py:41-125,
``prepare_instance_meta`` :128-144, ``get_attmask_w_box`` :34-37, ``complete_mask`` :22-31, ``convert_points`` :152-159,
``create_zero_input_tensors`` :9-20).  MI355X-first differences, none of which changes a value:
  * every tensor is assembled ONCE on the host and crosses PCIe once; the batch dimension of the two large tensors
    (``segs`` 30 x 512 x 512 fp32 = 31 MB per sample, ``att_masks``) is a stride-0 ``expand`` view on the device instead
    of the reference's ``.repeat(batch, ...)`` copies (31 MB x batch x (N+1) instance inputs in HBM and on the bus) --
    ``.shape`` / indexing / ``.sum()`` behave identically, and the engine's tokenizer detects the broadcast and runs the
    ConvNeXt mask backbone once per distinct mask stack;
  * text features come from ``get_clip_feature`` (utils/model.py:130-152 mirror below), which accepts either the HF
    CLIP model + processor the reference passes, or any object with ``.pooled(phrase) -> [768]`` (offline stand-in).
COCO-polygon helpers of the reference file (``annToMask``, ``prepare_scribble_and_instmask``) are dataset-evaluation
utilities that need pycocotools and are not on the inference path; they are not mirrored.  Their run-length half is: a meta that
carries ``rle`` (``meta_from_demo_json(.., instance_masks="json")``, host/masks.py) has its ``segs`` planes decoded from the JSON's
masks -- on the device, by one ``idf_rle_decode_planes`` launch per call, when ``prepare_batch`` / ``prepare_layout_inputs`` are
handed the HIP ``ops``; with numpy + Pillow otherwise.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional

import numpy as np
import torch


def create_zero_input_tensors(max_objs, n_polygon_points, n_scribble_points):
    """utils/input.py:9-20."""
    masks = torch.zeros(max_objs)
    text_masks = torch.zeros(max_objs)
    text_embeddings = torch.zeros(max_objs, 768)
    boxes_embeddings = torch.zeros(max_objs, 4)
    polygons_embeddings = torch.zeros(max_objs, n_polygon_points * 2)
    scribbles_embeddings = torch.zeros(max_objs, n_scribble_points * 2)
    segs_embeddings = torch.zeros(max_objs, 512, 512)
    points_embeddings = torch.zeros(max_objs, 2)
    return (boxes_embeddings, masks, text_masks, text_embeddings, polygons_embeddings, scribbles_embeddings,
            segs_embeddings, points_embeddings)


def complete_mask(has_mask, max_objs):
    """utils/input.py:22-31 (also inference.py:26-36)."""
    mask = torch.ones(1, max_objs)
    if has_mask is None:
        return mask
    if type(has_mask) == int or type(has_mask) == float:
        return mask * has_mask
    for idx, value in enumerate(has_mask):
        mask[0, idx] = value
    return mask


def get_attmask_w_box(att_masks, idx, box, image_size):
    """utils/input.py:34-37.  NOTE the reference's index order, kept: dim-0 of the mask is sliced with the box's
    x-range and dim-1 with its y-range."""
    x1, y1, x2, y2 = (int(np.round(box[0] * image_size)), int(np.round(box[1] * image_size)),
                      int(np.round(box[2] * image_size)), int(np.round(box[3] * image_size)))
    att_masks[idx][x1:x2, y1:y2] = 1
    return att_masks


def get_clip_feature(model, processor, input, is_image=False):
    """utils/model.py:130-152: pooled CLIP text feature [1, 768] of a phrase (None for a None phrase)."""
    if input is None:
        return None
    if hasattr(model, "pooled"):                                   # offline stand-in encoder
        return model.pooled(input).reshape(1, -1)
    inputs = processor(text=input, return_tensors="pt", padding=True)
    dev = next(model.parameters()).device
    inputs["input_ids"] = inputs["input_ids"].to(dev)
    inputs["pixel_values"] = torch.ones(1, 3, 224, 224, device=dev)          # placeholder, as in the reference
    inputs["attention_mask"] = inputs["attention_mask"].to(dev)
    outputs = model(**inputs)
    return outputs.text_model_output.pooler_output


def batch_to_device(batch, device):
    """dataset/jsondataset.py:59-69."""
    for k in batch:
        if isinstance(batch[k], torch.Tensor):
            batch[k] = batch[k].to(device)
        if isinstance(batch[k], list):
            for i in range(len(batch[k])):
                if isinstance(batch[k][i], dict):
                    for j in batch[k][i]:
                        if isinstance(batch[k][i][j], torch.Tensor):
                            batch[k][i][j] = batch[k][i][j].to(device)
    return batch


_BIG = ("segs", "att_masks")


def _batched(d: Dict[str, torch.Tensor], batch: int, device) -> Dict[str, torch.Tensor]:
    """[..] -> [batch, ..] on ``device``: small tensors are real copies (the reference's ``repeat``); the large ones are
    moved once and broadcast over the batch with a stride-0 view."""
    out = {}
    for k, v in d.items():
        v = v.to(device)
        if k in _BIG:
            out[k] = v.unsqueeze(0).expand(batch, *v.shape)
        else:
            out[k] = v.unsqueeze(0).repeat(batch, *([1] * v.dim()))
    return out


def _t(v) -> torch.Tensor:
    return torch.as_tensor(np.asarray(v), dtype=torch.float32)


def _padded_slots(entries, max_objs: int, text_mask_spec, att_rows=None, image_size: int = 64) -> Dict[str, torch.Tensor]:
    """One sample's [max_objs, ...] grounding tensors.  ``entries``: per live instance a tuple
    (box, text_feature | None, polygon | None, scribble | None, seg | None, point | None); slot k takes entry k, the
    remaining slots stay zero (``create_zero_input_tensors``).  ``att_rows``: optional per-entry [S, S] visibility
    masks for the masked gated self-attention."""
    (boxes, masks, text_masks, text_emb, polygons, scribbles, segs, points) = create_zero_input_tensors(
        max_objs, N_POLYGON_POINTS, N_SCRIBBLE_POINTS)
    fields = (None, None, polygons, scribbles, segs, points)
    for k, entry in enumerate(entries):
        boxes[k] = _t(entry[0])
        masks[k] = 1
        if entry[1] is not None:
            text_emb[k] = entry[1].detach().float().cpu().reshape(-1)
            text_masks[k] = 1
        for dst, val in zip(fields[2:], entry[2:]):
            if val is not None:
                dst[k] = _t(val).reshape(dst[k].shape)
    out = dict(boxes=boxes, masks=masks, text_masks=text_masks * complete_mask(text_mask_spec, max_objs)[0],
               text_embeddings=text_emb, polygons=polygons, scribbles=scribbles, segs=segs, points=points)
    if att_rows is not None:
        att = torch.zeros(max_objs, image_size, image_size)
        for k, row in enumerate(att_rows):
            att[k] = row
        out["att_masks"] = att
    return out


N_SCRIBBLE_POINTS, N_POLYGON_POINTS = 20, 256


SEGS_SIZE = 512                                        # side of a ``segs`` plane (create_zero_input_tensors)


class _DeviceSegs:
    """The ``segs`` stacks of every conditioning row of one call (global rows and instance rows, over all layouts), decoded from
    run-length masks by ONE ``idf_rle_decode_planes`` launch into one [rows with masks, max_objs, 512, 512] allocation.  A row's
    dict gets its stack as a batch-broadcast (stride-0) view; a row without any mask gets ``zero(batch)``."""
    ROWS_PER_LAUNCH = 256                              # 256 x 30 x 512^2 < 2^31 elements: what one launch addresses

    def __init__(self, ops, max_objs, device):
        self.ops, self.max_objs, self.device = ops, max_objs, device
        self.rows, self.fills = [], []

    def add(self, d, rles, batch):
        """``d``: the row's batched dict, without ``segs``; ``rles[k]``: slot k's ``parse_rle`` result or None."""
        jobs = [(k, r) for k, r in enumerate(rles) if r is not None]
        self.fills.append((d, len(self.rows) if jobs else None, batch, len(rles)))
        if jobs:
            self.rows.append(jobs)

    def finish(self, zero):
        from .masks import pack_masks
        stacks, areas = [], []
        for r0 in range(0, len(self.rows), self.ROWS_PER_LAUNCH):
            rows = self.rows[r0:r0 + self.ROWS_PER_LAUNCH]
            parsed = [p for jobs in rows for _, p in jobs]
            dst = [r * self.max_objs + k for r, jobs in enumerate(rows) for k, _ in jobs]
            stack = torch.empty(len(rows), self.max_objs, SEGS_SIZE, SEGS_SIZE, dtype=torch.float32, device=self.device)
            _, area = self.ops.rle_decode_planes(pack_masks(parsed, SEGS_SIZE), dst, stack)
            stacks.append(stack)
            areas.append(area)
        area = torch.cat(areas).cpu().tolist() if areas else []
        first = [0]
        for jobs in self.rows:
            first.append(first[-1] + len(jobs))
        for d, row, batch, n in self.fills:
            d["mask_areas"] = [-1] * n
            if row is None:
                d["segs"] = zero(batch)
                continue
            for j, (k, _) in enumerate(self.rows[row]):
                d["mask_areas"][k] = int(area[first[row] + j])
            stack, r = stacks[row // self.ROWS_PER_LAUNCH], row % self.ROWS_PER_LAUNCH
            d["segs"] = stack[r:r + 1].expand(batch, -1, -1, -1)


def _on_device(ops, device) -> bool:
    """The device route of the masks: the HIP backend (an ops object with ``rle_decode_planes``) and a GPU to write to."""
    return ops is not None and hasattr(ops, "rle_decode_planes") and torch.device(device).type == "cuda"


def _has_masks(meta) -> bool:
    return any(r is not None for r in (meta.get("rle") or []))


def _prepare_batch(meta, batch, max_objs, model, processor, image_size, use_masked_att, device, plan):
    """``prepare_batch``; with ``plan`` (a ``_DeviceSegs``) and masks in ``meta`` the dicts come back WITHOUT ``segs`` until
    ``plan.finish``."""
    phrases = meta.get("phrases")
    phrases = [None] * len(meta["locations"]) if phrases is None else phrases
    text_features = [get_clip_feature(model, processor, phrase, is_image=False) for phrase in phrases]
    rle = meta.get("rle") if _has_masks(meta) else None
    segs, areas = meta.get("segs"), None
    if rle is not None and plan is None:                 # host route: numpy decode + Pillow NEAREST, the kernel's CPU twin
        from .masks import decode_rle_reference
        planes = [None if r is None else decode_rle_reference(r, SEGS_SIZE) for r in rle]
        areas = [-1 if p is None else int(p.sum()) for p in planes]
        segs = [s if p is None else p.astype(np.float32) for s, p in zip(segs, planes)]
    if rle is not None and plan is not None:
        segs = [None] * len(meta["locations"])
    entries = list(zip(meta["locations"], text_features, meta.get("polygons"), meta.get("scribbles"), segs,
                       meta.get("points")))
    att_rows = None
    if use_masked_att:                                   # one box-shaped visibility plane per instance (:34-37)
        planes = torch.zeros(len(entries), image_size, image_size)
        for k, e in enumerate(entries):
            get_attmask_w_box(planes, k, e[0], image_size)
        att_rows = list(planes)

    def batched(slots, rles):
        if rle is None or plan is None:
            return _batched(slots, batch, device)
        slots.pop("segs")                                # never filled, never uploaded: the kernel writes the stack on the device
        d = _batched(slots, batch, device)
        plan.add(d, rles, batch)
        return d

    out: Dict[str, Any] = batched(_padded_slots(entries, max_objs, meta.get("text_mask"), att_rows, image_size), rle)
    if areas is not None:
        out["mask_areas"] = areas
    if "instance_meta" in meta:
        # the Multi-instance Sampler's per-instance inputs: instance i alone, in slot 0 (:92-120)
        out["instance_meta"] = []
        for i, im in enumerate(meta["instance_meta"]):
            entry = (im["locations"][0], text_features[i], im["polygons"][0], im["scribbles"][0],
                     segs[i] if rle is not None else im["segs"][0], im["points"][0])
            one = _padded_slots([entry], max_objs, im.get("text_mask"), None if att_rows is None else [att_rows[i]],
                                image_size)
            out["instance_meta"].append(batched(one, None if rle is None else [rle[i]]))
    return out


@torch.no_grad()
def prepare_batch(meta, batch=1, max_objs=30, model=None, processor=None, image_size=64, use_masked_att=False,
                  device="cuda", ops=None):
    """utils/input.py:39-125: meta (phrases, locations, polygons, scribbles, segs, points[, text_mask,
    instance_meta]) -> ``{boxes, masks, text_masks, text_embeddings, polygons, scribbles, segs, points[, att_masks,
    instance_meta: [same dict per instance]]}``, every tensor [batch, max_objs, ...] on ``device``.

    A meta with ``rle`` (``meta_from_demo_json(.., instance_masks="json")``): slot k's ``segs`` plane is mask k, nearest-resized to
    512 x 512 (utils/input.py:161-186), and instance i's own dict carries it in slot 0.  With ``ops`` the HIP backend the planes
    of all rows of the call are decoded on the device by one ``idf_rle_decode_planes`` launch; otherwise by
    ``masks.decode_rle_reference`` on the host -- the same bits.  The dict then also holds ``mask_areas``: per instance the mask's
    foreground pixels at 512 x 512, -1 without a mask."""
    plan = _DeviceSegs(ops, max_objs, device) if _has_masks(meta) and _on_device(ops, device) else None
    out = _prepare_batch(meta, batch, max_objs, model, processor, image_size, use_masked_att, device, plan)
    if plan is not None:
        zeros = {}

        def zero(b):
            if "z" not in zeros:
                zeros["z"] = torch.zeros(1, max_objs, SEGS_SIZE, SEGS_SIZE, device=device)
            return zeros["z"].expand(b, -1, -1, -1)
        plan.finish(zero)
    return out


@torch.no_grad()
def prepare_instance_meta(test_info, i, file_name=None, save_folder_name=None, ckpt=None):
    """utils/input.py:127-144: the single-instance meta the Multi-instance Sampler's input i+1 is built from."""
    rle = {"rle": [test_info["rle"][i]]} if "rle" in test_info else {}          # the instance's run-length mask, when the JSON's are used
    return {
        **rle,
        "ckpt": test_info.get("ckpt", None),
        "phrases": [test_info["phrases"][i]],
        "locations": [test_info["locations"][i]],
        "polygons": [test_info["polygons"][i]],
        "segs": [test_info["segs"][i]],
        "scribbles": [test_info["scribbles"][i]],
        "points": [test_info["points"][i]],
        "alpha_type": test_info["alpha_type"],
        "prompt": test_info["phrases"][i],
        "file_name": file_name,
        "save_folder_name": save_folder_name,
    }


@torch.no_grad()
def prepare_layout_inputs(metas, starting_noises, grounding_input, text_encoder, phrase_model, processor=None, instances=True,
                          max_objs=30, device="cuda", ops=None):
    """A batch of DIFFERENT layouts for one sampler call, from their metas (``meta_from_demo_json``) and start latents
    (``starting_noises[l]``: [K_l, 4, H, W], the K_l images of layout l).  ``text_encoder.encode(prompts) -> [n, 77, 768]``,
    ``phrase_model`` / ``processor`` as in ``prepare_batch``, ``grounding_input``: the model's ``GroundingNetInput``.

    ``instances=True`` (Multi-instance Sampler): the ``layouts`` argument of ``PLMSSamplerInst.sample_layouts`` -- per layout the
    list [global, instance 1, .., instance N_l] of input dicts, conditioning at batch 1 (``prepare_batch`` on the meta, and on
    ``prepare_instance_meta(meta, i)`` per instance), ``x`` the layout's start latents, shared by its dicts.
    ``instances=False`` (``mis == 0``): ONE ordinary ``PLMSSampler`` / ``DDIMSampler`` input whose rows differ -- layout l's K_l
    rows are ``prepare_batch(meta_l, batch=K_l)``, stacked layout after layout.

    All-zero ``segs`` (30 x 512 x 512 fp32 = 31 MB per stack) are never copied: every all-zero stack of the call is ONE zero plane
    set, and the rows of the stacked input broadcast it with a stride-0 view.

    Metas with ``rle`` (``meta_from_demo_json(.., instance_masks="json")``) condition on their masks as in ``prepare_batch``; with
    ``ops`` the HIP backend the ``segs`` stacks of ALL rows of the call -- global and instance rows, over all layouts -- come from
    ONE ``idf_rle_decode_planes`` launch into one allocation.  A global row's dict (``instances=False``: the returned dict, one
    list per layout) then carries ``mask_areas``."""
    image_size = int(starting_noises[0].shape[-1])
    zero_plane = {}

    def shared_zero(segs):
        """segs [b, max_objs, S, S] -> the call's one zero plane set, broadcast over b, when all of it is zero."""
        if bool(segs[:1].any()) if segs.stride(0) == 0 else bool(segs.any()):
            return segs
        key = (tuple(segs.shape[1:]), segs.dtype, segs.device)
        if key not in zero_plane:
            zero_plane[key] = torch.zeros((1,) + key[0], dtype=segs.dtype, device=segs.device)
        return zero_plane[key].expand(segs.shape[0], -1, -1, -1)

    plan = _DeviceSegs(ops, max_objs, device) if _on_device(ops, device) and any(_has_masks(m) for m in metas) else None
    pending = []

    def one(meta, batch, x):
        """The row's input dict; its ``grounding_input`` is filled in by ``settle`` once the call's masks are decoded."""
        b = _prepare_batch(meta, batch, max_objs, phrase_model, processor, image_size, False, device, plan)
        d = dict(x=x, timesteps=None, context=text_encoder.encode([meta["prompt"]] * batch).to(device), grounding_input=None)
        pending.append((d, b))
        return d

    def settle():
        if plan is not None:                                               # ONE launch for every row of the call
            key = ((max_objs, SEGS_SIZE, SEGS_SIZE), torch.float32, torch.empty(0, device=device).device)   # shared_zero's key

            def zero(batch):
                if key not in zero_plane:
                    zero_plane[key] = torch.zeros((1,) + key[0], dtype=key[1], device=key[2])
                return zero_plane[key].expand(batch, -1, -1, -1)
            plan.finish(zero)
        for d, b in pending:
            if max(b.get("mask_areas", [-1])) <= 0:                        # no mask, or only empty ones: maybe all zero
                b["segs"] = shared_zero(b["segs"])
            d["grounding_input"] = grounding_input.prepare(b)
            if "mask_areas" in b:
                d["mask_areas"] = b["mask_areas"]

    if instances:
        layouts = []
        for meta, x in zip(metas, starting_noises):
            lay = [one(meta, 1, x)]
            for i in range(len(meta["phrases"])):
                lay.append(one(prepare_instance_meta(meta, i), 1, x))
            layouts.append(lay)
        settle()
        return layouts
    rows = [one(meta, int(x.shape[0]), x) for meta, x in zip(metas, starting_noises)]
    settle()
    g = {k: torch.cat([r["grounding_input"][k] for r in rows], 0) for k in rows[0]["grounding_input"] if k != "segs"}
    segs = [r["grounding_input"]["segs"] for r in rows]
    n = sum(int(s.shape[0]) for s in segs)
    zeros = {z.data_ptr() for z in zero_plane.values()}
    if all(s.data_ptr() in zeros and s.data_ptr() == segs[0].data_ptr() for s in segs):
        g["segs"] = segs[0][:1].expand(n, -1, -1, -1)                     # one plane set for every row
    else:
        g["segs"] = torch.cat(segs, 0)
    out = dict(x=torch.cat(list(starting_noises), 0), timesteps=None, context=torch.cat([r["context"] for r in rows], 0),
               grounding_input=g)
    if any("mask_areas" in r for r in rows):
        out["mask_areas"] = [r.get("mask_areas") for r in rows]
    return out


def convert_points(points: List[float], img_info: Dict[str, int]) -> List[float]:
    """utils/input.py:152-159: absolute [x0,y0,x1,y1,...] -> relative, clipped at 1."""
    for i in range(len(points)):
        if i % 2 == 0:
            points[i] = min(points[i] / img_info["width"], 1.0)
        else:
            points[i] = min(points[i] / img_info["height"], 1.0)
    return points


# ---- demo-JSON parsing (inference.py:189-297) --------------------------------------------------------------------
def equally_spaced_sampling_with_replacement(points_list, sample_size):
    """dataset/decode_item.py:79-100."""
    if sample_size <= len(points_list):
        gap_size = len(points_list) // sample_size
        return [points_list[i * gap_size] for i in range(sample_size)]
    return [points_list[(i * len(points_list)) // sample_size % len(points_list)] for i in range(sample_size)]


def reorder_scribbles(scribbles):
    """dataset/decode_item.py:102-108 (called by inference.py:258 on the LIST of per-instance scribbles, as there)."""
    center = np.array([0, 0])
    scribbles = sorted(scribbles, key=lambda x: np.linalg.norm(np.array(x) - center))
    scribbles = equally_spaced_sampling_with_replacement(scribbles, 20)
    return sorted(scribbles, key=lambda x: np.linalg.norm(np.array(x) - center))


def rescale_box(bbox, width, height):
    """inference.py:132-137: xywh pixels -> normalised xyxy."""
    return [bbox[0] / width, bbox[1] / height, (bbox[0] + bbox[2]) / width, (bbox[1] + bbox[3]) / height]


def meta_from_demo_json(data: dict, alpha: float, ckpt: Optional[str] = None, save_folder_name: Optional[str] = None,
                        instance_masks: str = "ignore") -> dict:
    """inference.py:189-297: demo JSON (caption, width, height, annos[{bbox, mask, point, scribble, caption}]) -> the
    ``meta`` dict ``prepare_batch`` consumes.  As in the reference script, instance masks are NOT used (it re-initialises
    its mask list to zeros at :249), so ``segs`` and ``polygons`` are zero and scribbles default to zeros.

    ``instance_masks="json"``: the meta also carries ``rle``, per anno the parsed run-length mask (``masks.parse_rle``; ValueError
    for a malformed one) or None where the anno has no (or an empty) ``mask``; ``prepare_batch`` turns them into ``segs`` planes
    as the reference's ``eval_local.py`` route does (utils/input.py:161-186).  ``segs`` itself stays zero here, ``polygons`` stay
    zero and scribbles are the JSON's own, as above: the reference derives both from the mask (skimage contours, unseeded random
    points), see DESIGN.md section 8."""
    if instance_masks not in ("ignore", "json"):
        raise ValueError(f"instance_masks must be 'ignore' or 'json', got {instance_masks!r}")
    W, H = data["width"], data["height"]
    annos = data["annos"]
    boxes = [a["bbox"] if "bbox" in a else [0, 0, 0, 0] for a in annos]
    points_list = [a["point"] for a in annos if "point" in a]
    scribbles_list = [a["scribble"] for a in annos if "scribble" in a]
    phrases = [a["caption"] for a in annos]
    locations = [rescale_box(b, W, H) for b in boxes]
    if len(points_list) == 0:
        points = [[(b[0] + b[2]) / 2.0, (b[1] + b[3]) / 2.0] for b in locations]
    else:
        points = [[p[0] / float(W), p[1] / float(H)] for p in points_list]
    n = len(locations)
    if len(scribbles_list) == 0:
        scribbles = [[0.0] * 40 for _ in range(n)]                 # sample_random_points_from_mask(zeros) -> zeros
    else:
        scribbles = [[[s[0] / float(W), s[1] / float(H)] for s in sc] for sc in scribbles_list]
        scribbles = reorder_scribbles(scribbles)
    polygons = [[0.0] * 512 for _ in range(n)]
    segs = np.zeros((n, 512, 512), dtype=np.float32)
    meta = dict(ckpt=ckpt, prompt=data["caption"], phrases=phrases, polygons=polygons, scribbles=scribbles, segs=segs,
                locations=locations, points=points, alpha_type=[alpha, 0.0, 1 - alpha],
                save_folder_name=save_folder_name)
    if instance_masks == "json":
        from .masks import parse_rle
        meta["rle"] = [parse_rle(a["mask"]) if a.get("mask") else None for a in annos]
    return meta
