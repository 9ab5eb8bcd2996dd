"""Reader of COLMAP's binary sparse model: ``cameras.bin``, ``images.bin``, ``points3D.bin``.

What the reference gets from ``pycolmap.Reconstruction(path)`` (tinysplat/dataset.py:22-26), in numpy and ``struct``
on the host.  All three files are little-endian and start with a ``uint64`` record count.  A file that ends early, goes
on after its last record or names a count its bytes cannot hold raises ``ValueError`` with the file and the offset;
nothing is allocated from a count before it is checked against the bytes that remain.  The text variants (``*.txt``)
are not read.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass
from pathlib import Path
from typing import Dict

import numpy as np

# model id -> (name, number of parameters): the reader needs every count to step through cameras.bin
CAMERA_MODELS = {
    0: ("SIMPLE_PINHOLE", 3), 1: ("PINHOLE", 4), 2: ("SIMPLE_RADIAL", 4), 3: ("RADIAL", 5), 4: ("OPENCV", 8),
    5: ("OPENCV_FISHEYE", 8), 6: ("FULL_OPENCV", 12), 7: ("FOV", 5), 8: ("SIMPLE_RADIAL_FISHEYE", 4),
    9: ("RADIAL_FISHEYE", 5), 10: ("THIN_PRISM_FISHEYE", 12),
}

_POINT2D = np.dtype([("x", "<f8"), ("y", "<f8"), ("point3D_id", "<i8")])
_TRACK = np.dtype([("image_id", "<u4"), ("point2D_idx", "<u4")])


@dataclass
class Camera:
    camera_id: int
    model_id: int
    model: str
    width: int
    height: int
    params: np.ndarray          # float64 [P(model)]


@dataclass
class Image:
    image_id: int
    qvec: np.ndarray            # float64 [4], w x y z, world -> camera
    tvec: np.ndarray            # float64 [3]
    camera_id: int
    name: str
    xys: np.ndarray             # float64 [m, 2], COLMAP pixel coordinates (the first pixel's centre is 0.5)
    point3D_ids: np.ndarray     # int64 [m], -1: no 3-D point


@dataclass
class Point3D:
    point3D_id: int
    xyz: np.ndarray             # float64 [3]
    rgb: np.ndarray             # uint8 [3]
    error: float
    track: np.ndarray           # uint32 [track_len, 2]: image_id, point2D_idx


@dataclass
class Reconstruction:
    """The three files' records by id, each dict in file order."""
    cameras: Dict[int, Camera]
    images: Dict[int, Image]
    points3D: Dict[int, Point3D]


class _Cursor:
    def __init__(self, path: Path):
        self.path = path
        self.buf = path.read_bytes()
        self.at = 0

    def fail(self, what: str):
        raise ValueError(f"{self.path}: {what} at offset {self.at} of {len(self.buf)} bytes")

    def need(self, size: int, what: str) -> None:
        if size > len(self.buf) - self.at:
            self.fail(f"truncated: {what} needs {size} bytes")

    def take(self, fmt: str, what: str):
        size = struct.calcsize(fmt)
        self.need(size, what)
        out = struct.unpack_from(fmt, self.buf, self.at)
        self.at += size
        return out

    def count(self, smallest_record: int, what: str) -> int:
        """The file's leading record count, refused where the remaining bytes cannot hold that many records."""
        n, = self.take("<Q", f"the {what} count")
        if n * smallest_record > len(self.buf) - self.at:
            self.fail(f"a count of {n} {what} does not fit the file")
        return n

    def array(self, dtype, count: int, what: str) -> np.ndarray:
        dtype = np.dtype(dtype)
        if count > (len(self.buf) - self.at) // dtype.itemsize:
            self.fail(f"truncated: {count} {what} do not fit the file")
        out = np.frombuffer(self.buf, dtype=dtype, count=count, offset=self.at).copy()
        self.at += count * dtype.itemsize
        return out

    def cstring(self, what: str) -> str:
        end = self.buf.find(b"\0", self.at)
        if end < 0:
            self.fail(f"truncated: {what} has no terminating NUL")
        out = self.buf[self.at:end].decode("utf-8", errors="replace")
        self.at = end + 1
        return out

    def done(self) -> None:
        if self.at != len(self.buf):
            self.fail(f"over-long: {len(self.buf) - self.at} bytes follow the last record")


def read_cameras(path) -> Dict[int, Camera]:
    c = _Cursor(Path(path))
    cameras = {}
    for _ in range(c.count(24 + 3 * 8, "cameras")):
        camera_id, model_id, width, height = c.take("<IiQQ", "a camera")
        if model_id not in CAMERA_MODELS:
            c.fail(f"camera {camera_id} has the unknown model id {model_id}")
        name, num_params = CAMERA_MODELS[model_id]
        cameras[camera_id] = Camera(camera_id, model_id, name, width, height,
                                    c.array("<f8", num_params, "camera parameters"))
    c.done()
    return cameras


def read_images(path) -> Dict[int, Image]:
    c = _Cursor(Path(path))
    images = {}
    for _ in range(c.count(4 + 56 + 4 + 1 + 8, "images")):
        image_id, = c.take("<I", "an image id")
        pose = c.array("<f8", 7, "pose values")
        camera_id, = c.take("<I", "an image's camera id")
        name = c.cstring("an image name")
        m, = c.take("<Q", "a 2-D point count")
        pts = c.array(_POINT2D, m, "2-D points")
        images[image_id] = Image(image_id, pose[:4].copy(), pose[4:].copy(), camera_id, name,
                                 np.stack([pts["x"], pts["y"]], axis=1), pts["point3D_id"].copy())
    c.done()
    return images


def read_points3D(path) -> Dict[int, Point3D]:
    c = _Cursor(Path(path))
    points = {}
    for _ in range(c.count(8 + 24 + 3 + 8 + 8, "points")):
        point3D_id, = c.take("<Q", "a point id")
        xyz = c.array("<f8", 3, "coordinates")
        rgb = c.array("u1", 3, "colour bytes")
        error, track_len = c.take("<dQ", "a point's error and track length")
        track = c.array(_TRACK, track_len, "track elements")
        points[point3D_id] = Point3D(point3D_id, xyz, rgb, error,
                                     np.stack([track["image_id"], track["point2D_idx"]], axis=1))
    c.done()
    return points


def read_reconstruction(path) -> Reconstruction:
    """``path``: the folder of a sparse model (``.../sparse/0``)."""
    path = Path(path)
    names = ("cameras", "images", "points3D")
    missing = [n for n in names if not (path / f"{n}.bin").exists()]
    if missing:
        text = [n for n in missing if (path / f"{n}.txt").exists()]
        if text:
            raise ValueError(f"{path}: only the text model ({', '.join(n + '.txt' for n in text)}) is here; the binary "
                             "files are read, not the text ones (convert with COLMAP's model_converter)")
        raise FileNotFoundError(f"{path}: {', '.join(n + '.bin' for n in missing)} missing")
    return Reconstruction(read_cameras(path / "cameras.bin"), read_images(path / "images.bin"),
                          read_points3D(path / "points3D.bin"))
