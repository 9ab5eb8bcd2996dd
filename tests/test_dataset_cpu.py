"""``camera_from_colmap`` without a GPU (tinysplat_amd/dataset.py), on the synthetic reconstruction of
tests/colmap_cases.py: the camera a training step renders with must see every 3-D point where COLMAP observed it."""
import math

import numpy as np
import pytest
import torch

import colmap_cases as CC
import undistort_oracle as UO
from tinysplat_amd import colmap
from tinysplat_amd.dataset import camera_from_colmap
from tinysplat_amd.synthetic import quat_to_rot_matrix

W, H = CC.W, CC.H


@pytest.fixture(scope="module")
def rec(tmp_path_factory):
    return colmap.read_reconstruction(CC.write(tmp_path_factory.mktemp("colmap")))


def _rendered_pixel(camera, xyz):
    """Where the rasteriser puts world points: its optical axis is the frame's centre, x_pix = 0.5 W x_ndc + W / 2 - 0.5
    (oracle/gsplat_oracle.py).  ``project_points`` gives the NDC; its own screen coordinates keep a quirk of the
    reference (x scaled by the height), so they are not used."""
    ndc = camera.project_points(torch.as_tensor(xyz, dtype=torch.float32), screen_coordinates=False).double().numpy()
    return 0.5 * camera.width * ndc[:, 0] + camera.width / 2 - 0.5, 0.5 * camera.height * ndc[:, 1] + camera.height / 2 - 0.5


def _residual(rec, image, setup):
    """max distance, in source pixels, between COLMAP's observations (as indices: coordinates - 0.5) and the rendered
    positions of their 3-D points pushed through the oracle's destination -> source map"""
    seen = image.point3D_ids != -1
    xyz = np.stack([rec.points3D[int(i)].xyz for i in image.point3D_ids[seen]])
    u, v = _rendered_pixel(setup.camera, xyz)
    (sx, ex), (sy, ey) = UO.map_points(setup.src_k, setup.dst_k, setup.dist, u, v)
    obs = image.xys[seen] - 0.5
    return float(np.hypot(sx + ex - obs[:, 0], sy + ey - obs[:, 1]).max()), int(seen.sum())


def test_center_mode_puts_every_observation_where_colmap_saw_it(rec):
    total = 0
    for image in rec.images.values():
        for max_dim in (None, 40):
            setup = camera_from_colmap(rec.cameras[image.camera_id], image, (W, H), "center", max_dim)
            worst, count = _residual(rec, image, setup)
            print(f"{image.name} (camera {image.camera_id}, max_image_dimension {max_dim}): {count} observations, "
                  f"worst {worst:.2e} px")
            assert worst <= 1e-3
            total += count
        assert setup.dst_k[2] == (setup.out_size[0] - 1) / 2 and setup.dst_k[3] == (setup.out_size[1] - 1) / 2
    assert total > 400


def test_reference_mode_is_right_for_the_centred_pinhole(rec):
    """cx = W / 2, cy = H / 2: the focal hack multiplies by 1, nothing is resampled, and the frame's centre is the axis."""
    images = [im for im in rec.images.values() if im.camera_id == 1]
    assert len(images) == 2
    for image in images:
        setup = camera_from_colmap(rec.cameras[1], image, (W, H), "reference")
        assert not setup.resample and setup.src_k.tolist() == setup.dst_k.tolist() == [80.0, 78.0, 48.5, 30.5]
        worst, count = _residual(rec, image, setup)
        print(f"{image.name}: {count} observations, worst {worst:.2e} px")
        assert worst <= 1e-3 and count > 30


def test_reference_mode_follows_the_reference_quirk_for_quirk(rec):
    image = rec.images[3]
    cam = rec.cameras[7]                                                # OPENCV, cx = 46.8, cy = 32.2
    setup = camera_from_colmap(cam, image, (W, H))
    fx, fy = 85.0 * (W / 2 / 46.8), 83.0 * (H / 2 / 32.2)              # dataset.py:54-55
    assert np.allclose(setup.src_k, [fx, fy, 46.8, 32.2], rtol=1e-15)   # cx, cy unshifted
    assert setup.dist.tolist() == [-0.10, 0.02, 0.004, -0.003, 0, 0, 0, 0] and setup.resample
    want = UO.new_matrix_reference(setup.src_k, setup.dist, W, H)
    assert np.allclose(setup.dst_k, want, rtol=1e-12) and setup.out_size == (W, H)
    c = setup.camera
    assert (c.f_x, c.f_y, c.width, c.height) == (setup.dst_k[0], setup.dst_k[1], W, H)
    assert c.fov_x == 2 * math.atan(W / (2 * c.f_x)) and c.fov_y == 2 * math.atan(H / (2 * c.f_y))
    # a pinhole model is not undistorted, whatever its principal point; a distortion model with zeros is (an identity)
    pin = colmap.Camera(9, 1, "PINHOLE", W, H, np.array([85.0, 83.0, 46.8, 32.2]))
    s = camera_from_colmap(pin, image, (W, H))
    assert not s.resample and s.src_k.tolist() == s.dst_k.tolist() and np.allclose(s.src_k[:2], [fx, fy], rtol=1e-15)
    zero = colmap.Camera(9, 4, "OPENCV", W, H, np.array([85.0, 83.0, 46.8, 32.2, 0, 0, 0, 0]))
    s = camera_from_colmap(zero, image, (W, H))
    assert not s.resample and np.abs(s.dst_k - s.src_k).max() < 1e-9
    # center mode resamples that pinhole: its principal point is off the centre
    s = camera_from_colmap(pin, image, (W, H), "center")
    assert s.resample and np.allclose(s.src_k, [85.0, 83.0, 46.3, 31.7], rtol=1e-15) and s.dst_k[2:].tolist() == [48.0, 30.0]
    # ... and not the centred one
    s = camera_from_colmap(rec.cameras[1], image, (W, H), "center")
    assert not s.resample and np.abs(s.dst_k - [80.0, 78.0, 48.0, 30.0]).max() < 1e-12
    with pytest.raises(ValueError, match="principal_point"):
        camera_from_colmap(cam, image, (W, H), "centre")


def test_view_matrix_position_and_visible_points(rec):
    _, images, _ = CC.reconstruction()
    for src, image in zip(images, rec.images.values()):
        c = camera_from_colmap(rec.cameras[image.camera_id], image, (W, H)).camera
        rot = quat_to_rot_matrix(src["qvec"])
        view = np.eye(4)
        view[:3, :3], view[:3, 3] = rot, src["tvec"]
        assert c.view_matrix.dtype == torch.float32 and np.abs(c.view_matrix.numpy() - view).max() < 1e-6
        assert np.abs(c.position - (-rot.T @ src["tvec"])).max() < 1e-12
        assert np.abs(np.linalg.norm(c.position) - np.linalg.norm(CC._IMAGES[images.index(src)][3])) < 1e-9
        assert c.name == src["name"].split("/")[-1]
        want = src["point3D_ids"][src["point3D_ids"] != -1]
        assert c.visible_point_ids.dtype == torch.int64 and c.visible_point_ids.tolist() == want.tolist()
        assert len(want) < len(src["point3D_ids"])
        p = c.proj_matrix.numpy()
        assert abs(p[0, 0] - 1 / math.tan(c.fov_x / 2)) < 1e-6 and abs(p[1, 1] - 1 / math.tan(c.fov_y / 2)) < 1e-6
        assert abs(p[2, 2] - 1000.001 / 999.999) < 1e-6 and p[3, 2] == 1


@pytest.mark.parametrize("max_dim,size", [(40, (40, 25)), (96, (96, 60)), (97, (97, 61)), (500, (97, 61)), (1, (1, 1))])
def test_max_image_dimension_scales_size_and_intrinsics(rec, max_dim, size):
    image, cam = rec.images[3], rec.cameras[7]
    for mode in ("reference", "center"):
        full = camera_from_colmap(cam, image, (W, H), mode)
        s = camera_from_colmap(cam, image, (W, H), mode, max_dim)
        assert s.out_size == size and (s.camera.width, s.camera.height) == size and s.resample
        assert s.src_k.tolist() == full.src_k.tolist()
        want_size, want_k = UO.scaled(full.dst_k, W, H, max_dim)
        assert want_size == size and np.allclose(s.dst_k, want_k, rtol=1e-14)
        sx, sy = size[0] / W, size[1] / H
        assert np.allclose(s.dst_k, [full.dst_k[0] * sx, full.dst_k[1] * sy, (full.dst_k[2] + 0.5) * sx - 0.5,
                                     (full.dst_k[3] + 0.5) * sy - 0.5], rtol=1e-14)
        assert (s.camera.f_x, s.camera.f_y) == (s.dst_k[0], s.dst_k[1])
        assert s.camera.fov_x == 2 * math.atan(size[0] / (2 * s.camera.f_x))
        if mode == "center":
            assert np.allclose(s.dst_k[2:], [(size[0] - 1) / 2, (size[1] - 1) / 2], atol=1e-12)


def test_image_file_of_another_size_than_the_camera(rec):
    """center mode scales COLMAP's intrinsics about the pixel-corner origin to the file's size."""
    cam = colmap.Camera(9, 4, "OPENCV", 2 * W, 2 * H, np.array([170.0, 166.0, 93.6, 64.4, -0.10, 0.02, 0.004, -0.003]))
    s = camera_from_colmap(cam, rec.images[3], (W, H), "center")
    assert np.allclose(s.src_k, [85.0, 83.0, 46.3, 31.7], rtol=1e-14)
    same = camera_from_colmap(rec.cameras[7], rec.images[3], (W, H), "center")
    assert np.allclose(s.dst_k, same.dst_k, rtol=1e-12)
