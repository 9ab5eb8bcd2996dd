"""The COLMAP binary reader (tinysplat_amd/colmap.py) against the independent writer of
tests/colmap_cases.py: every field read back, ids past 2^31, every camera model stepped over, and files that are cut
short, go on too long or name a count their bytes cannot hold."""
import struct

import numpy as np
import pytest

import colmap_cases as CC
from tinysplat_amd import colmap
from tinysplat_amd.dataset import camera_from_colmap


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    return CC.write(tmp_path_factory.mktemp("colmap") / "sparse" / "0")


def test_every_field_is_read_back(folder):
    cameras, images, points = CC.reconstruction()
    rec = colmap.read_reconstruction(folder)
    assert list(rec.cameras) == [c["camera_id"] for c in cameras]                     # file order
    for c in cameras:
        got = rec.cameras[c["camera_id"]]
        assert (got.camera_id, got.model_id, got.width, got.height) == (c["camera_id"], c["model_id"], CC.W, CC.H)
        assert got.model == colmap.CAMERA_MODELS[c["model_id"]][0]
        assert got.params.dtype == np.float64 and got.params.tolist() == c["params"]
    assert list(rec.images) == [im["image_id"] for im in images]
    for im in images:
        got = rec.images[im["image_id"]]
        assert (got.image_id, got.camera_id, got.name) == (im["image_id"], im["camera_id"], im["name"])
        assert np.array_equal(got.qvec, im["qvec"]) and np.array_equal(got.tvec, im["tvec"])
        assert got.xys.shape == (len(im["point3D_ids"]), 2) and np.array_equal(got.xys, im["xys"])
        assert got.point3D_ids.dtype == np.int64 and np.array_equal(got.point3D_ids, im["point3D_ids"])
        assert (got.point3D_ids == -1).any()
    assert list(rec.points3D) == [p["point3D_id"] for p in points]
    for p in points:
        got = rec.points3D[p["point3D_id"]]
        assert got.point3D_id == p["point3D_id"] and np.array_equal(got.xyz, p["xyz"]) and got.error == p["error"]
        assert got.rgb.dtype == np.uint8 and np.array_equal(got.rgb, p["rgb"])
        assert got.track.shape == p["track"].shape and np.array_equal(got.track, p["track"])
    # a track element names the 2-D point that names the 3-D point
    for p in rec.points3D.values():
        for image_id, idx in p.track:
            assert rec.images[int(image_id)].point3D_ids[idx] == p.point3D_id


def test_ids_past_two_to_the_31_survive(folder):
    rec = colmap.read_reconstruction(folder)
    assert CC.BIG + 5 in rec.cameras and CC.BIG + 9 in rec.images and rec.images[CC.BIG + 9].camera_id == CC.BIG + 5
    big = [pid for pid in rec.points3D if pid >= CC.BIG]
    assert len(big) == 20 and all(isinstance(pid, int) for pid in big)
    assert int(rec.images[CC.BIG + 9].point3D_ids.max()) >= CC.BIG
    pts = [{"point3D_id": (1 << 63) + 7, "xyz": np.zeros(3), "rgb": np.zeros(3, np.uint8), "error": 0.5,
            "track": np.array([[0xFFFFFFFF, 0xFFFFFFFE]], dtype=np.uint32)}]
    CC.write(folder.parent / "huge", points=pts)
    got = colmap.read_points3D(folder.parent / "huge" / "points3D.bin")
    assert list(got) == [(1 << 63) + 7] and got[(1 << 63) + 7].track.tolist() == [[0xFFFFFFFF, 0xFFFFFFFE]]


def test_every_model_is_stepped_over_and_the_loader_names_the_ones_it_refuses(tmp_path):
    cams = [{"camera_id": m + 1, "model_id": m, "width": 640, "height": 480,
             "params": ([500.0 + m] * (2 if m in (1, 4, 5, 6, 10) else 1) + [320.0, 240.0]
                        + [0.001 * (i + 1) for i in range(n)])[:n]} for m, n in CC.NUM_PARAMS.items()]
    (tmp_path / "cameras.bin").write_bytes(CC.cameras_bytes(cams))
    got = colmap.read_cameras(tmp_path / "cameras.bin")
    assert [c.model_id for c in got.values()] == list(range(11))
    assert all(got[m + 1].params.tolist() == cams[m]["params"] for m in range(11))
    image = colmap.Image(1, np.array([1.0, 0, 0, 0]), np.zeros(3), 1, "x.png", np.zeros((0, 2)), np.zeros(0, np.int64))
    for m in (0, 1, 2, 3, 4, 6):
        camera_from_colmap(got[m + 1], image, (640, 480))
    for m in (5, 7, 8, 9, 10):
        with pytest.raises(ValueError, match=colmap.CAMERA_MODELS[m][0]):
            camera_from_colmap(got[m + 1], image, (640, 480))
    for bad in ([0.0, 320, 240], [500.0, -1, 240], [np.nan, 320, 240]):                # what a file may hold
        with pytest.raises(ValueError, match="camera 3"):
            camera_from_colmap(colmap.Camera(3, 0, "SIMPLE_PINHOLE", 640, 480, np.array(bad)), image, (640, 480))
    with pytest.raises(ValueError, match="does not converge"):
        camera_from_colmap(colmap.Camera(3, 2, "SIMPLE_RADIAL", 640, 480, np.array([100.0, 320, 240, -5.0])), image,
                           (640, 480))
    (tmp_path / "cameras.bin").write_bytes(struct.pack("<QIiQQ", 1, 1, 11, 640, 480) + bytes(96))
    with pytest.raises(ValueError, match="unknown model id 11"):
        colmap.read_cameras(tmp_path / "cameras.bin")


@pytest.mark.parametrize("name,reader", [("cameras.bin", colmap.read_cameras), ("images.bin", colmap.read_images),
                                         ("points3D.bin", colmap.read_points3D)])
def test_truncated_and_overlong_files_raise_value_error(folder, tmp_path, name, reader):
    blob = (folder / name).read_bytes()
    reader(folder / name)
    for cut in (4, 8 + 13, len(blob) // 2, len(blob) - 1):
        (tmp_path / name).write_bytes(blob[:cut])
        with pytest.raises(ValueError, match=f"{name}.*offset"):
            reader(tmp_path / name)
    (tmp_path / name).write_bytes(blob + b"\0")
    with pytest.raises(ValueError, match=f"{name}.*over-long.*offset {len(blob)}"):
        reader(tmp_path / name)
    (tmp_path / name).write_bytes(b"")
    with pytest.raises(ValueError, match="truncated"):
        reader(tmp_path / name)


def test_garbage_counts_raise_value_error_without_allocating(folder, tmp_path):
    """A count of 2^60 anywhere: refused from the bytes that remain, before anything of that size is made."""
    huge = struct.pack("<Q", 1 << 60)
    for name, reader in (("cameras.bin", colmap.read_cameras), ("images.bin", colmap.read_images),
                         ("points3D.bin", colmap.read_points3D)):
        blob = (folder / name).read_bytes()
        (tmp_path / name).write_bytes(huge + blob[8:])
        with pytest.raises(ValueError, match="does not fit"):
            reader(tmp_path / name)
    cameras, images, points = CC.reconstruction()
    # the 2-D point count of the first image, and the track length of the first point
    blob = bytearray(CC.images_bytes(images))
    at = 8 + 4 + 56 + 4 + len(images[0]["name"]) + 1
    assert struct.unpack_from("<Q", blob, at)[0] == len(images[0]["point3D_ids"])
    blob[at:at + 8] = huge
    (tmp_path / "images.bin").write_bytes(bytes(blob))
    with pytest.raises(ValueError, match="2-D points do not fit"):
        colmap.read_images(tmp_path / "images.bin")
    blob = bytearray(CC.points_bytes(points))
    at = 8 + 8 + 24 + 3 + 8
    assert struct.unpack_from("<Q", blob, at)[0] == len(points[0]["track"])
    blob[at:at + 8] = huge
    (tmp_path / "points3D.bin").write_bytes(bytes(blob))
    with pytest.raises(ValueError, match="track elements do not fit"):
        colmap.read_points3D(tmp_path / "points3D.bin")
    one = CC.images_bytes(images[:1])
    (tmp_path / "images.bin").write_bytes(one[:8 + 4 + 56 + 4] + b"a" * 40)                 # a name without its NUL
    with pytest.raises(ValueError, match="NUL"):
        colmap.read_images(tmp_path / "images.bin")


def test_text_models_and_missing_files_are_told_apart(tmp_path):
    for n in ("cameras", "images", "points3D"):
        (tmp_path / f"{n}.txt").write_text("# text model\n")
    with pytest.raises(ValueError, match="text"):
        colmap.read_reconstruction(tmp_path)
    with pytest.raises(FileNotFoundError):
        colmap.read_reconstruction(tmp_path / "nowhere")
