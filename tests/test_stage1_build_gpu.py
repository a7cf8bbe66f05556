"""motion.build_stage1 end to end on the GPU: a 48 x 48 input folder -> MOM/train_data.pth, MOM/scene_flow.pth, MOM/Flow_viz and the
pixel video, through render_pcd, estimate_flows (the hint field as the motion), optimize_motion on the device sampler and
resampler, and the same through the command line.  One build is shared by the tests."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
pkg = "iclr2025_3d-mom_amd"
motion = importlib.import_module(pkg + ".motion")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE, SEED = 48, 4822
BUILD = dict(size=32, train_iteration=3, n_frames=4, video_size=64)


def write_folder(path):
    """image.png (noise), image_json/mask.png (a disc), image.json (two labelme hints and a polygon) and depth.npy: smooth, about
    the 4.3 the internal poses turn around, so that their five views keep the cloud in a 48-pixel image at stage 1's focal length."""
    from PIL import Image
    rng = np.random.default_rng(48)
    os.makedirs(os.path.join(path, "image_json"))
    Image.fromarray(rng.integers(0, 256, (SIDE, SIDE, 3), dtype=np.uint8)).save(os.path.join(path, "image.png"))
    y, x = np.mgrid[0:SIDE, 0:SIDE]
    Image.fromarray((((x - 26) ** 2 + (y - 22) ** 2 <= 15 ** 2) * 255).astype(np.uint8)).save(os.path.join(path, "image_json", "mask.png"))
    with open(os.path.join(path, "image.json"), "w") as f:
        json.dump({"shapes": [{"label": "hint1", "points": [[20.4, 18.0], [33.0, 24.7]]},
                              {"label": "water", "points": [[5, 5], [40, 5], [40, 40]]},
                              {"label": "hint2", "points": [[30.0, 30.2], [22.5, 40.0]]}]}, f)
    np.save(os.path.join(path, "depth.npy"), (4.3 + 0.15 * np.sin(x / 11.0) + 0.1 * np.cos(y / 7.0)).astype(np.float32))
    return path


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    folder = write_folder(str(tmp_path_factory.mktemp("stage1") / "scene"))
    np.random.seed(SEED)
    data, flow = motion.build_stage1(folder, np.load(os.path.join(folder, "depth.npy")), video="pixels",
                                     render_poses=motion.pcd_gen_poses("lookaround")[:2], **BUILD)
    return folder, data, flow


def test_train_data_is_what_stage_2_reads(built):
    folder, data, _ = built
    loaded = importlib.import_module(pkg + ".scene.dataset_readers").load_train_data(os.path.join(folder, "MOM", "train_data.pth"))
    assert loaded["W"] == loaded["H"] == SIDE and loaded["pcd_points"].shape == (3, SIDE * SIDE)
    # the first render pose's five internal views; the second's, 20 degrees away, see nothing of 48 pixels and are dropped
    assert len(loaded["frames"]) == len(data["frames"]) == 5
    for fr in loaded["frames"]:
        assert len(fr["T2C_flow"]) == 1 and len(fr["our_flow"]) == 1
        assert fr["T2C_flow"][0].shape == (1, 2, SIDE, SIDE) and fr["our_flow"][0].shape == (1, 2, SIDE, SIDE)
        assert fr["image"].size == (SIDE, SIDE) and fr["mask"].size == (SIDE, SIDE)
        assert torch.isfinite(fr["T2C_flow"][0]).all() and torch.isfinite(fr["our_flow"][0]).all()
    assert any(float(fr["T2C_flow"][0].abs().max()) > 1e-3 for fr in loaded["frames"])


def test_scene_flow_is_the_refit_of_the_file(built):
    folder, _, flow = built
    path = os.path.join(folder, "MOM", "scene_flow.pth")
    written = torch.load(path, map_location="cpu")
    assert written.shape == (3, SIDE * SIDE) and torch.equal(written, flow) and float(written.abs().max()) > 0
    refit = motion.refit_scene_flow(folder, BUILD["train_iteration"], sampler="device")
    assert torch.equal(refit, written)


def test_video_and_flow_images(built):
    from PIL import Image
    folder, data, _ = built
    video = os.path.join(folder, "MOM", "video")
    assert sorted(os.listdir(video)) == [f"{i:06d}.png" for i in range(BUILD["n_frames"])]
    viz = os.path.join(folder, "MOM", "Flow_viz")
    assert sorted(os.listdir(viz)) == [f"{i:03d}.png" for i in range(len(data["frames"]))]
    for d in (video, viz):
        for name in os.listdir(d):
            im = Image.open(os.path.join(d, name))
            im.load()
            assert im.size == (SIDE, SIDE) and im.mode == "RGB"
    first = np.asarray(Image.open(os.path.join(viz, "000.png")))
    assert np.array_equal(first, motion.flow_image(data["frames"][0]["our_flow"][0][0]))


def test_the_command_line_builds_the_same_scene_flow(built, tmp_path):
    folder, _, flow = built
    second = write_folder(str(tmp_path / "scene"))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    argv = ["--input_dir", second, "--build", "--depth", os.path.join(second, "depth.npy"), "--flow", "hints", "--video", "pixels",
            "--render_poses", "2", "--seed", str(SEED), "--size", str(BUILD["size"]), "--train_iteration", str(BUILD["train_iteration"]),
            "--n_frames", str(BUILD["n_frames"]), "--video_size", str(BUILD["video_size"])]
    code = f"import importlib; importlib.import_module('{pkg}.motion').main({argv!r})"
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    assert torch.equal(torch.load(os.path.join(second, "MOM", "scene_flow.pth"), map_location="cpu"), flow)
    assert len(os.listdir(os.path.join(second, "MOM", "video"))) == BUILD["n_frames"]
