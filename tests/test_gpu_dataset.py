"""``Dataset`` on the synthetic reconstruction of tests/colmap_cases.py with 97 x 61 PNGs of random bytes (DESIGN.md section
6l): what it loads, every target against the oracle, the point cloud into ``from_pcd``, three training steps, and the
training tool in a process of its own."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import colmap_cases as CC
import undistort_cases as UC
import undistort_oracle as UO
from tinysplat_amd import Dataset, colmap, formats, from_pcd
from tinysplat_amd.dataset import camera_from_colmap
from tinysplat_amd.ops import kernel_timer
from tinysplat_amd.training import fit

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
DEV = "cuda:0"


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    base = tmp_path_factory.mktemp("scene")
    CC.write(base / "colmap" / "sparse" / "0")
    pixels = CC.write_images(base / "images")
    return base, pixels


@pytest.fixture(scope="module")
def loaded(scene):
    base, _ = scene
    out = {}
    for mode in ("reference", "center"):
        kernel_timer.start()
        ds = Dataset(base / "colmap" / "sparse" / "0", base / "images", device=DEV, principal_point=mode)
        out[mode] = (ds, kernel_timer.stop().get("ts_undistort_image", (0, 0.0))[0])
    return out


@pytest.mark.parametrize("mode", ["reference", "center"])
def test_counts_names_sizes_and_order(scene, loaded, mode):
    ds, launches = loaded[mode]
    _, images, points = CC.reconstruction()
    assert len(ds.cameras) == len(ds.targets) == 6
    assert [c.name for c in ds.cameras] == [im["name"].split("/")[-1] for im in images]          # images.bin order
    for cam, im, target in zip(ds.cameras, images, ds.targets):
        assert (cam.width, cam.height) == (CC.W, CC.H) and tuple(target.shape) == (CC.H, CC.W, 3)
        assert target.dtype == torch.float32 and target.is_cuda and 0 <= float(target.min()) and float(target.max()) <= 1
        want = im["point3D_ids"][im["point3D_ids"] != -1]
        assert cam.visible_point_ids.is_cuda and cam.visible_point_ids.cpu().tolist() == want.tolist()
    assert all(t.dtype == torch.uint8 for t in ds.targets.images_u8)
    # the centred pinhole (camera 1: images 0 and 4) is never resampled; every other camera is
    assert ds.resampled == [False, True, True, True, False, True] and launches == 4
    centres = np.array([c[3] for c in CC._IMAGES])
    extent = 1.1 * np.linalg.norm(centres - centres.mean(0), axis=1).max()
    assert abs(ds.spatial_extent - extent) < 1e-9
    ids = sorted(p["point3D_id"] for p in points)
    assert ds.pcd.point_ids.cpu().tolist() == ids and ds.pcd.xyz.shape == (60, 3) and ds.pcd.colors.dtype == torch.uint8
    by_id = {p["point3D_id"]: p for p in points}
    assert np.array_equal(ds.pcd.xyz.cpu().numpy(), np.stack([by_id[i]["xyz"] for i in ids]))
    assert np.array_equal(ds.pcd.colors.cpu().numpy(), np.stack([by_id[i]["rgb"] for i in ids]))
    assert ds.pcd.errors.cpu().tolist() == [by_id[i]["error"] for i in ids]


@pytest.mark.parametrize("mode", ["reference", "center"])
def test_targets_are_the_oracle_s(scene, loaded, mode):
    base, pixels = scene
    ds, _ = loaded[mode]
    rec = colmap.read_reconstruction(base / "colmap" / "sparse" / "0")
    for image, got in zip(rec.images.values(), ds.targets.images_u8):
        src = pixels[image.name]
        setup = camera_from_colmap(rec.cameras[image.camera_id], image, (CC.W, CC.H), mode)
        if not setup.resample:
            assert np.array_equal(got.cpu().numpy(), src), image.name                            # the file's pixels
            continue
        levels = UO.remap(src, setup.src_k, setup.dst_k, setup.dist, setup.out_size)
        UO.check_uint8(got.cpu().numpy(), levels, UC.TAU, f"{mode} {image.name}")
    i = 2
    assert torch.equal(ds.targets[i], ds.targets.images_u8[i].float() / 255.0)


def test_downscaled_dataset(scene):
    base, pixels = scene
    ds = Dataset(base / "colmap" / "sparse" / "0", base / "images", max_image_dimension=40, device=DEV,
                 principal_point="center")
    assert all(ds.resampled) and all(tuple(t.shape) == (25, 40, 3) for t in ds.targets)
    assert all((c.width, c.height) == (40, 25) for c in ds.cameras)
    rec = colmap.read_reconstruction(base / "colmap" / "sparse" / "0")
    image = rec.images[3]
    setup = camera_from_colmap(rec.cameras[7], image, (CC.W, CC.H), "center", 40)
    levels = UO.remap(pixels[image.name], setup.src_k, setup.dst_k, setup.dist, (40, 25))
    UO.check_uint8(ds.targets.images_u8[2].cpu().numpy(), levels, UC.TAU, "downscaled view_c")


def test_point_cloud_builds_a_model_and_training_runs(loaded):
    ds, _ = loaded["center"]
    model = from_pcd(ds.pcd, sh_degree=1, device=DEV, generator=torch.Generator().manual_seed(0))
    assert model.means.shape == (60, 3) and torch.isfinite(model.scales).all()
    assert torch.equal(model.means.cpu(), ds.pcd.xyz.float().cpu())
    losses = []
    out = fit(model, ds.cameras, ds.targets, DEV, max_iter=3, rng=np.random.default_rng(0),
              generator=torch.Generator().manual_seed(0), on_step=lambda s, o: losses.append(float(o["loss"])))
    assert len(losses) == 3 and np.isfinite(losses).all() and np.isfinite(float(out["loss"]))


def test_loader_refuses_a_fisheye_camera_and_a_cpu_device(scene, tmp_path):
    base, _ = scene
    cams = [dict(c) for c in CC.CAMERAS]
    cams[1] = {"camera_id": 2, "model_id": 5, "width": CC.W, "height": CC.H,
               "params": [80.0, 78.0, 48.5, 30.5, 0.01, 0.0, 0.0, 0.0]}
    CC.write(tmp_path / "sparse", cameras=cams)
    with pytest.raises(ValueError, match="OPENCV_FISHEYE"):
        Dataset(tmp_path / "sparse", base / "images", device=DEV)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Dataset(base / "colmap" / "sparse" / "0", base / "images", device="cpu")


def test_training_tool_runs_in_a_process_of_its_own(scene, tmp_path):
    base, _ = scene
    out = tmp_path / "scene.ply"
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "train.py"), "--dataset-dir", str(base), "--max-iter", "2",
                        "--sh-degree", "1", "--principal-point", "center", "--max-image-dimension", "64",
                        "--output", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "6 cameras (6 resampled), 60 points" in r.stdout and "wrote" in r.stdout
    model = formats.load_ply(out, DEV)
    assert model.means.shape == (60, 3) and model.colors_rest.shape == (60, 3, 3) and torch.isfinite(model.means).all()
