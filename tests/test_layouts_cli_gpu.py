"""``inference.py --input_json A.json B.json`` end to end on a real MI355X, in process, as tests/test_inference_cli_gpu.py runs the CLI:
two demo layouts sampled in ONE batch write two folders (OUTPUT/<save_folder_name>/<json stem>/) with one PNG of the right size each,
and each ``latents.pt`` is within the bf16 trajectory bar (rel-RMS 5e-2, tests/test_layouts_gpu.py) of the single-JSON run of that
file -- the existing CLI path, which still writes to the old folder."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JSONS = ["demos/demo_four_boxes.json", "demos/demo_points.json"]
STEPS, SEED, ALPHA = 4, 3, 0.75
FOLDER = f"gc7.5-seed{SEED}-alpha{ALPHA}"
TRAJ_TOL = 5e-2


def _main(out_dir, jsons):
    import inference
    argv = ["inference.py", "--synthetic_weights", "--steps", str(STEPS), "--num_images", "1", "--save_latents", "--seed", str(SEED),
            "--alpha", str(ALPHA), "--test_config", os.path.join(REPO, "configs", "test_box.yaml"), "--output", str(out_dir),
            "--dtype", "bf16", "--input_json"] + [os.path.join(REPO, j) for j in jsons]
    old, cwd = sys.argv, os.getcwd()
    sys.argv = argv
    os.chdir(REPO)
    try:
        inference.main()
    finally:
        sys.argv = old
        os.chdir(cwd)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """One two-JSON run and the single-JSON run of each file, each into its own output root."""
    root = tmp_path_factory.mktemp("layouts_cli")
    _main(root / "both", JSONS)
    for k, j in enumerate(JSONS):
        _main(root / f"single{k}", [j])
    return root


def test_two_jsons_write_two_folders_with_one_image_each(runs):
    from PIL import Image
    base = runs / "both" / FOLDER
    assert sorted(os.listdir(base)) == ["demo_four_boxes", "demo_points"]
    for stem in ("demo_four_boxes", "demo_points"):
        pngs = sorted(p for p in os.listdir(base / stem) if p.endswith(".png"))
        assert len(pngs) == 1, (stem, pngs)
        img = Image.open(base / stem / pngs[0])
        assert img.size == (512, 512) and img.mode == "RGB"
        lat = torch.load(base / stem / "latents.pt")["latents"]
        assert tuple(lat.shape) == (1, 4, 64, 64) and torch.isfinite(lat).all()


def test_each_layout_reproduces_its_single_json_run(runs):
    from tests import cases
    for k, stem in enumerate(("demo_four_boxes", "demo_points")):
        old = runs / f"single{k}" / FOLDER                              # a one-path run still writes to the old folder
        assert os.path.isfile(old / "latents.pt") and os.path.isfile(old / "0.png") and not os.path.isdir(old / stem)
        one, both = torch.load(old / "latents.pt"), torch.load(runs / "both" / FOLDER / stem / "latents.pt")
        assert one["phrases"] == both["phrases"] and one["caption"] == both["caption"]
        err = cases.rel_rms(both["latents"].float(), one["latents"].float())
        print(f"[parity] inference.py, {stem} in a two-layout batch against its single-JSON run (S={STEPS}, bf16): latent rel-rms "
              f"{err:.3e} (tol {TRAJ_TOL:.0e})")
        assert err < TRAJ_TOL
