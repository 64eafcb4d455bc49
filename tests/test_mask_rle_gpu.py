"""``idf_rle_decode_planes`` (csrc/mask_input.hip) and the ``--instance_masks json`` route on a real MI355X.

1. Every decoded plane is ``torch.equal`` to ``host.masks.decode_rle_reference`` (numpy decode + Pillow NEAREST): up- and downsampling,
   non-square sources, the eight demo masks, all-zero / all-one masks, zero-length runs, masks whose runs are searched in LDS and
   masks with more runs than the LDS budget (global-memory search) in ONE launch.  ``area`` is the oracle's sum, planes no job names
   stay zero, and the guard rows behind ``out`` and ``area`` keep their fill.
2. Jobs whose table entries are out of range write nothing; bad arguments are refused before any launch.
3. A reduced model conditioned on ``segs`` from the device route gives the very output of the host route, and not that of zero masks.
4. ``inference.py --instance_masks json`` reproduces a run whose masks went through the host route, bit for bit, and differs from
   ``--instance_masks ignore``; two JSONs, one with masks and one without, run in one batch."""
import contextlib
import ctypes as C
import io
import json
import os
import sys

import numpy as np
import pytest
import torch

from instancediffusion_amd.host.masks import decode_rle_reference, pack_masks, parse_rle
from tests.test_mask_rle import blobs, encode_counts, fixture

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = -12345                                   # fill of the int32 guard behind ``area``
LDS_RUNS = 4096                                  # RLE_LDS_RUNS of csrc/mask_input.hip


@pytest.fixture(scope="module")
def ops():
    from instancediffusion_amd.ops import HipOps
    return HipOps()


def rle_of(mask):
    return parse_rle({"size": list(mask.shape), "counts": encode_counts(mask)})


def decode(ops, parsed, S, dst=None, P=None):
    """One launch over ``parsed`` into a NaN-guarded [P, S, S] buffer -> (out on the host, area list); checks the guards, the planes
    no job names, and every named plane and area against the oracle."""
    M = len(parsed)
    dst = list(range(M)) if dst is None else dst
    P = (max(dst) + 1 if dst else 1) if P is None else P
    buf = torch.full((P + 1, S, S), float("nan"), device="cuda")
    abuf = torch.full((M + 1,), GUARD, dtype=torch.int32, device="cuda")
    out, area = ops.rle_decode_planes(pack_masks(parsed, S), dst, buf[:P], area=abuf[:M])
    torch.cuda.synchronize()
    assert out.data_ptr() == buf.data_ptr() and area.data_ptr() == abuf.data_ptr()
    assert torch.isnan(buf[P]).all() and int(abuf[M]) == GUARD, "guard rows behind out / area were written"
    got, areas = buf[:P].cpu(), abuf[:M].cpu().tolist()
    for p in range(P):
        if p not in dst:
            assert not got[p].any(), f"plane {p} is named by no job and must be zero"
    for m, (pm, d) in enumerate(zip(parsed, dst)):
        want = torch.from_numpy(decode_rle_reference(pm, S).astype(np.float32))
        assert torch.equal(got[d], want), f"job {m} -> plane {d}: {int((got[d] != want).sum())} of {want.numel()} pixels differ"
        assert areas[m] == int(want.sum()), (m, areas[m], int(want.sum()))
    return got, areas


def alternation(h, w):
    """Every pixel its own run over the column-major order: h * w runs."""
    return (h, w, np.ones(h * w, np.uint32))


def checkerboard(n):
    yy, xx = np.mgrid[0:n, 0:n]
    return ((yy + xx) & 1).astype(np.uint8)


# ---- 1. parity with the CPU twin -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,S", [("1x1", 8), ("3x5", 8), ("7x1", 12), ("427x640", 512), ("427x640", 64), ("all_zero", 8), ("all_one", 8),
                                    ("zero_runs", 8), ("leading_zero_run", 16)])
def test_small_cases_equal_the_reference(ops, name, S):
    g = np.random.default_rng(5)
    masks = {
        "1x1": [rle_of(np.ones((1, 1), np.uint8)), rle_of(np.zeros((1, 1), np.uint8))],
        "3x5": [rle_of((g.random((3, 5)) < 0.5).astype(np.uint8))],
        "7x1": [rle_of((g.random((7, 1)) < 0.5).astype(np.uint8)), rle_of((g.random((1, 7)) < 0.5).astype(np.uint8))],
        "427x640": [rle_of(blobs(427, 640, 9)), rle_of(blobs(640, 427, 10))],
        "all_zero": [rle_of(np.zeros((9, 4), np.uint8))],
        "all_one": [rle_of(np.ones((9, 4), np.uint8))],
        "zero_runs": [parse_rle({"size": [4, 5], "counts": [5, 3, 0, 4, 6, 0, 0, 2]})],
        "leading_zero_run": [parse_rle({"size": [6, 3], "counts": [0, 7, 0, 0, 5, 6]})],
    }[name]
    if name == "all_one":
        assert masks[0][2].tolist() == [0, 36]
    decode(ops, masks, S)


@pytest.mark.parametrize("S", [512, 64])
def test_the_eight_demo_masks(ops, S):
    fx = fixture()
    _, areas = decode(ops, [parse_rle(m) for m in fx["masks"]], S)
    if S == 512:
        assert areas == [m["area"] for m in fx["masks"]]


def test_lds_and_global_search_in_one_launch(ops):
    """A per-pixel alternation (262 144 runs) and a true checkerboard (one run fewer per column edge) are far over the LDS budget; the
    small masks between them stage their runs in LDS -- same launch; a tall alternation steps over several runs per output row."""
    board, small, tall = rle_of(checkerboard(512)), rle_of(blobs(48, 64, 2)), alternation(1024, 16)
    alt = alternation(512, 512)
    fits = (37, 53, np.ones(37 * 53, np.uint32))                  # 1961 runs: inside the budget, not a handful
    assert alt[2].size == 262144 and board[2].size > LDS_RUNS and tall[2].size > LDS_RUNS
    assert small[2].size <= LDS_RUNS and fits[2].size <= LDS_RUNS
    got, _ = decode(ops, [alt, small, board, fits, tall], 512)
    assert torch.equal(got[2], torch.from_numpy(checkerboard(512).astype(np.float32)))
    decode(ops, [board, small, alt], 64)


def test_budget_edge(ops):
    """Exactly RLE_LDS_RUNS runs (LDS) and one more (global memory)."""
    at = (LDS_RUNS, 1, np.ones(LDS_RUNS, np.uint32))
    over = (LDS_RUNS + 1, 1, np.ones(LDS_RUNS + 1, np.uint32))
    decode(ops, [at, over], 64)


def test_one_mask_to_two_planes_and_untouched_planes(ops):
    fx = fixture()
    a, b = parse_rle(fx["masks"][1]), parse_rle(fx["masks"][4])
    parsed, dst = [a, b, a], [4, 0, 31]                          # a layout's global row (slot k) and its instance row (slot 0)
    table = pack_masks(parsed, 64)
    assert table["run_begin"][0] == table["run_begin"][2] and table["ends"].size == a[2].size + b[2].size
    got, areas = decode(ops, parsed, 64, dst=dst, P=33)
    assert torch.equal(got[4], got[31]) and areas[0] == areas[2] > 0


# ---- 2. guards ------------------------------------------------------------------------------------------------------------------
def test_out_of_range_jobs_write_nothing(ops):
    """The tables are device memory the launcher cannot read: the kernel checks every entry where it becomes an address."""
    S, P = 16, 3
    good = rle_of(blobs(20, 12, 1))
    t = pack_masks([good], S)
    n = int(t["ends"].size)
    #         ok  plane=P  plane<0  begin>end  end>n  begin<0  h=0   w<0   h*w>=2^31
    rb = [0, 0, 0, 5, 0, -1, 0, 0, 0]
    re = [n, n, n, 4, n + 1, n, n, n, n]
    dst = [1, P, -1, 0, 0, 0, 0, 2, 2]
    hw = [[20, 12]] * 6 + [[0, 12], [20, -3], [65536, 65536]]
    M = len(rb)
    dev = lambda a, dt=torch.int32: torch.tensor(a, dtype=dt).cuda()      # noqa: E731
    ends = torch.from_numpy(t["ends"].view(np.int32)).cuda()
    buf = torch.full((P + 1, S, S), float("nan"), device="cuda")
    area = torch.zeros(M + 1, dtype=torch.int32, device="cuda")
    tabs = [dev(rb), dev(re), dev(hw), dev(dst)]
    p = lambda x: C.c_void_p(x.data_ptr())                                # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert ops.lib.idf_rle_decode_planes(p(ends), n, p(tabs[0]), p(tabs[1]), p(tabs[2]), p(tabs[3]), M, p(buf), P, S, p(area), st) == 0
    torch.cuda.synchronize()
    got = buf.cpu()
    want = torch.from_numpy(decode_rle_reference(good, S).astype(np.float32))
    assert torch.equal(got[1], want)
    assert torch.isnan(got[0]).all() and torch.isnan(got[2]).all() and torch.isnan(got[3]).all()
    assert area.cpu().tolist() == [int(want.sum())] + [0] * M


def test_bad_arguments_are_refused_before_any_launch(ops):
    S, P = 16, 2
    good = rle_of(blobs(20, 12, 1))
    t = pack_masks([good], S)
    buf = torch.full((P, S, S), float("nan"), device="cuda")
    area = torch.full((2,), GUARD, dtype=torch.int32, device="cuda")
    ints = torch.from_numpy(np.concatenate([t["run_begin"], t["run_end"], t["src_hw"].reshape(-1), np.zeros(1, np.int32),
                                            t["ends"].view(np.int32)])).cuda()
    at = lambda k: C.c_void_p(ints.data_ptr() + 4 * k)                    # noqa: E731
    p = lambda x: C.c_void_p(x.data_ptr())                                # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    n = int(t["ends"].size)

    def call(ends=at(5), n_ends=n, rb=at(0), re=at(1), hw=at(2), dst=at(4), M=1, out=p(buf), planes=P, size=S, ar=p(area)):
        return ops.lib.idf_rle_decode_planes(ends, n_ends, rb, re, hw, dst, M, out, planes, size, ar, st)

    E_ARG, E_ALIGN, E_UNSUPPORTED = -1, -2, -3
    assert call(size=0) == E_ARG and call(size=-4) == E_ARG and call(M=-1) == E_ARG and call(planes=0) == E_ARG and call(n_ends=-1) == E_ARG
    for name in ("ends", "rb", "re", "hw", "dst", "out", "ar"):
        assert call(**{name: None}) == E_ARG, name
    assert call(size=18) == E_UNSUPPORTED                                   # S % 4
    assert call(planes=8192, size=512) == E_UNSUPPORTED                     # P * S * S = 2^31
    assert call(M=65536) == E_UNSUPPORTED
    assert call(out=C.c_void_p(buf.data_ptr() + 4)) == E_ALIGN and call(rb=C.c_void_p(ints.data_ptr() + 2)) == E_ALIGN
    assert call(M=0) == 0                                                   # nothing to do: no launch either
    torch.cuda.synchronize()
    assert torch.isnan(buf).all() and area.cpu().tolist() == [GUARD, GUARD], "a refused call reached the device"
    # the wrapper: what the launcher cannot see is refused on the host
    out = buf[:1]
    for table, dst, o in [
            (t, [P], buf), (t, [-1], buf), (t, [0, 1], buf),                                      # plane out of range / job count
            (pack_masks([good, good], S), [1, 1], buf),                                           # one plane named twice
            (dict(t, run_end=t["run_end"] + 1), [0], buf), (dict(t, run_begin=t["run_end"] + 1), [0], buf),
            (dict(t, ends=t["ends"].astype(np.int64)), [0], buf),
            (t, [0], torch.empty(1, 18, 18, device="cuda")), (t, [0], buf.cpu()), (t, [0], buf.double()), (t, [0], buf[:, :, ::2])]:
        with pytest.raises(ValueError):
            ops.rle_decode_planes(table, dst, o)
    torch.cuda.synchronize()
    assert torch.isnan(buf).all() and out.data_ptr() == buf.data_ptr()
    assert call() == 0                                                      # and the same arguments, unbroken, do launch
    torch.cuda.synchronize()
    assert torch.equal(buf[0].cpu(), torch.from_numpy(decode_rle_reference(good, S).astype(np.float32))) and torch.isnan(buf[1]).all()


# ---- 3. the masks reach the model -----------------------------------------------------------------------------------------------
def demo_json(n_masks=2, extra_plain=1):
    """A demo JSON written from the fixture: ``n_masks`` instances with masks, ``extra_plain`` without."""
    fx = fixture()
    annos = [dict(bbox=m["bbox"], mask=dict(size=m["size"], counts=m["counts"]), caption=c)
             for m, c in zip([fx["masks"][0], fx["masks"][3]][:n_masks], ["a corgi", "a chocolate cupcake"])]
    annos += [dict(bbox=[300, 20, 120, 90], caption="a painting on the wall")] * extra_plain
    return dict(caption="a corgi at a table with a cupcake", width=512, height=512, annos=annos)


class _Enc:
    def pooled(self, phrase):
        return torch.randn(768, generator=torch.Generator().manual_seed(len(phrase)))


def test_reduced_model_forward_device_route_equals_host_route_and_sees_the_masks(ops):
    from grounding_input.text_grounding_tokinzer_input import GroundingNetInput
    from instancediffusion_amd.host.input import meta_from_demo_json, prepare_batch, prepare_instance_meta
    from tests import cases
    from tests.test_engine_emulated import build_model
    model = build_model(cases.cfg_for("test_mask.yaml", "tiny"))
    gi = GroundingNetInput()
    model.grounding_tokenizer_input = gi
    meta = meta_from_demo_json(demo_json(), 0.75, instance_masks="json")
    meta["instance_meta"] = [prepare_instance_meta(meta, i) for i in range(3)]
    kw = dict(batch=2, max_objs=30, model=_Enc(), image_size=16, device="cuda")
    dev = prepare_batch(meta, ops=model.engine.ops, **kw)
    host = prepare_batch(meta, **kw)
    assert dev["mask_areas"] == host["mask_areas"] == [46505, 6161, -1]
    rows_dev, rows_host = [dev] + dev["instance_meta"], [host] + host["instance_meta"]
    for a, b in zip(rows_dev, rows_host):
        assert set(a) - {"instance_meta", "mask_areas"} == set(b) - {"instance_meta", "mask_areas"}
        for k in b:
            if torch.is_tensor(b[k]):
                assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
        assert a["segs"].stride(0) == 0                                     # the batch broadcast stays a view
    # all rows with masks of the call share ONE allocation; the row without a mask holds the zero plane set
    base = dev["segs"].untyped_storage().data_ptr()
    assert [r["segs"].untyped_storage().data_ptr() == base for r in rows_dev] == [True, True, True, False]
    assert dev["segs"].untyped_storage().nbytes() == 3 * 30 * 512 * 512 * 4 and not rows_dev[3]["segs"].any()
    g = torch.Generator().manual_seed(2)
    x, ctx, t = torch.randn(2, 4, 16, 16, generator=g).cuda(), torch.randn(2, 77, 768, generator=g).cuda(), torch.tensor([801, 801]).cuda()

    def forward(batch):
        with torch.no_grad():
            return model(dict(x=x, timesteps=t, context=ctx, grounding_input=gi.prepare(batch))).float().cpu()
    e_dev, e_host = forward(dev), forward(host)
    e_zero = forward(dict(host, segs=torch.zeros_like(host["segs"][:1]).expand(2, -1, -1, -1)))
    assert torch.isfinite(e_dev).all() and torch.equal(e_dev, e_host)
    assert not torch.equal(e_dev, e_zero), "the masks do not reach the model"
    print(f"[parity] reduced model, segs from idf_rle_decode_planes vs host-built: equal; vs zero masks: rel-rms "
          f"{cases.rel_rms(e_dev, e_zero):.3e}")


def test_prepare_layout_inputs_one_launch_for_all_rows(ops, monkeypatch):
    from grounding_input.text_grounding_tokinzer_input import GroundingNetInput
    from instancediffusion_amd.host.input import meta_from_demo_json, prepare_layout_inputs
    metas = [meta_from_demo_json(demo_json(2, 1), 0.75, instance_masks="json"), meta_from_demo_json(demo_json(0, 2), 0.75, instance_masks="json"),
             meta_from_demo_json(demo_json(1, 0), 0.75)]
    noises = [torch.zeros(2, 4, 16, 16, device="cuda")] * 3
    calls = []
    real = type(ops).rle_decode_planes
    monkeypatch.setattr(type(ops), "rle_decode_planes", lambda self, *a, **k: (calls.append(len(a[1])), real(self, *a, **k))[1])

    class Text:
        def encode(self, prompts):
            return torch.zeros(len(prompts), 77, 768)
    kw = dict(grounding_input=GroundingNetInput(), text_encoder=Text(), phrase_model=_Enc(), max_objs=30, device="cuda")
    dev = prepare_layout_inputs(metas, noises, instances=True, ops=ops, **kw)
    assert calls == [2 + 1 + 1]                                             # global row: 2 jobs; two instance rows: 1 each; ONE launch
    host = prepare_layout_inputs(metas, noises, instances=True, **kw)
    assert calls == [4]
    assert [len(lay) for lay in dev] == [4, 3, 2] and dev[0][0]["mask_areas"] == host[0][0]["mask_areas"] == [46505, 6161, -1]
    zero_ptr = dev[1][0]["grounding_input"]["segs"].data_ptr()
    for ld, lh in zip(dev, host):
        for a, b in zip(ld, lh):
            for k, v in b["grounding_input"].items():
                assert torch.equal(a["grounding_input"][k], v), k
    masked = [(0, 0), (0, 1), (0, 2)]
    for l, lay in enumerate(dev):
        for j, d in enumerate(lay):
            segs = d["grounding_input"]["segs"]
            assert (segs.data_ptr() != zero_ptr) == ((l, j) in masked), (l, j)      # every other row: the call's one zero plane set
    flat = prepare_layout_inputs(metas, noises, instances=False, ops=ops, **kw)
    flat_host = prepare_layout_inputs(metas, noises, instances=False, **kw)
    assert calls == [4, 2] and flat["mask_areas"][0] == [46505, 6161, -1] and flat["mask_areas"][2] is None
    assert tuple(flat["grounding_input"]["segs"].shape) == (6, 30, 512, 512)
    assert torch.equal(flat["grounding_input"]["segs"], flat_host["grounding_input"]["segs"])


# ---- 4. the CLI -----------------------------------------------------------------------------------------------------------------
STEPS, SEED = 2, 3
FOLDER = f"gc7.5-seed{SEED}-alpha0.75"


def _main(out_dir, jsons, masks, host_route=False):
    """``inference.py`` in process, as tests/test_inference_cli_gpu.py runs it.  ``host_route``: the same run with the ``ops`` argument
    withheld from the input builders, so that the masks are decoded by numpy + Pillow and uploaded.  -> what it printed."""
    import inference
    argv = ["inference.py", "--synthetic_weights", "--steps", str(STEPS), "--num_images", "1", "--save_latents", "--seed", str(SEED),
            "--output", str(out_dir), "--instance_masks", masks, "--input_json"] + [str(j) for j in jsons]
    old, cwd = sys.argv, os.getcwd()
    saved = inference.prepare_batch, inference.prepare_layout_inputs
    if host_route:
        inference.prepare_batch = lambda *a, **k: saved[0](*a, **dict(k, ops=None))
        inference.prepare_layout_inputs = lambda *a, **k: saved[1](*a, **dict(k, ops=None))
    sys.argv = argv
    os.chdir(REPO)
    text = io.StringIO()
    try:
        with contextlib.redirect_stdout(text):
            inference.main()
    finally:
        sys.argv = old
        os.chdir(cwd)
        inference.prepare_batch, inference.prepare_layout_inputs = saved
    return text.getvalue()


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    root = tmp_path_factory.mktemp("mask_cli")
    with open(root / "two_masks.json", "w") as f:
        json.dump(demo_json(2, 1), f)
    said = {name: _main(root / name, [root / "two_masks.json"], masks, host) for name, masks, host in
            [("device", "json", False), ("host", "json", True), ("ignore", "ignore", False)]}
    said["both"] = _main(root / "both", [root / "two_masks.json", os.path.join(REPO, "demos", "demo_four_boxes.json")], "json")
    return root, said


def _latents(root, name, stem=None):
    folder = root / name / FOLDER
    return torch.load((folder / stem if stem else folder) / "latents.pt")["latents"]


def test_cli_masks_change_the_latents_and_match_the_host_route(cli):
    root, said = cli
    dev, host, ignore = _latents(root, "device"), _latents(root, "host"), _latents(root, "ignore")
    assert tuple(dev.shape) == (1, 4, 64, 64) and torch.isfinite(dev).all()
    assert torch.equal(dev, host), "device-decoded masks and host-decoded masks must give the same run"
    assert not torch.equal(dev, ignore), "--instance_masks json did not change the sampled latents"
    for name in ("device", "host"):
        line = [ln for ln in said[name].splitlines() if ln.startswith("masks ")]
        assert len(line) == 1 and "2 of 3 instances carry a mask" in line[0] and "none is empty" in line[0], said[name]
    assert "masks " not in said["ignore"]


def test_cli_two_jsons_one_with_masks_one_without(cli):
    from tests import cases
    root, said = cli
    lines = [ln for ln in said["both"].splitlines() if ln.startswith("masks ")]
    assert len(lines) == 2 and "2 of 3 instances carry a mask" in lines[0] and "0 of 4 instances carry a mask" in lines[1], said["both"]
    assert sorted(os.listdir(root / "both" / FOLDER)) == ["demo_four_boxes", "two_masks"]
    both, plain = _latents(root, "both", "two_masks"), _latents(root, "both", "demo_four_boxes")
    assert tuple(both.shape) == tuple(plain.shape) == (1, 4, 64, 64) and torch.isfinite(both).all() and torch.isfinite(plain).all()
    err = cases.rel_rms(both.float(), _latents(root, "device").float())
    print(f"[parity] inference.py --instance_masks json, the masked layout in a two-layout batch against its single-JSON run: "
          f"latent rel-rms {err:.3e} (tol 5e-2, the bf16 trajectory bar of tests/test_layouts_cli_gpu.py)")
    assert err < 5e-2
    assert not torch.equal(both, _latents(root, "ignore"))


def test_cli_refuses_masks_with_a_config_that_drops_them(tmp_path):
    with open(tmp_path / "m.json", "w") as f:
        json.dump(demo_json(1, 0), f)
    import inference
    old = sys.argv
    sys.argv = ["inference.py", "--synthetic_weights", "--instance_masks", "json", "--test_config", os.path.join(REPO, "configs", "test_box.yaml"),
                "--output", str(tmp_path / "out"), "--input_json", str(tmp_path / "m.json")]
    try:
        with pytest.raises(SystemExit, match="drops masks"):
            inference.main()
    finally:
        sys.argv = old
    assert not os.path.exists(tmp_path / "out")
