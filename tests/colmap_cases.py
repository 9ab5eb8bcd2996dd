"""A writer of COLMAP's three binary files and a synthetic reconstruction for the reader's and the loader's tests
(DESIGN.md section 6l).  Independent of tinysplat_amd/colmap.py: records are plain dicts, packed with ``struct``."""
import functools
import struct

import numpy as np

import undistort_oracle as UO

W, H = UO.SIZE
BIG = 1 << 31                                   # ids at and past 2^31 must survive the reader
NUM_PARAMS = {0: 3, 1: 4, 2: 4, 3: 5, 4: 8, 5: 8, 6: 12, 7: 5, 8: 4, 9: 5, 10: 12}

# camera_id -> record; COLMAP pixel coordinates (the first pixel's centre is 0.5): index intrinsics + 0.5.  Camera 1 is the
# centred pinhole: cx = W / 2, cy = H / 2.
CAMERAS = [
    {"camera_id": 1, "model_id": 1, "width": W, "height": H, "params": [80.0, 78.0, 48.5, 30.5]},
    {"camera_id": 2, "model_id": 2, "width": W, "height": H, "params": [80.0, 48.5, 30.5, -0.12]},
    {"camera_id": 7, "model_id": 4, "width": W, "height": H,
     "params": [85.0, 83.0, 46.8, 32.2, -0.10, 0.02, 0.004, -0.003]},
    {"camera_id": BIG + 5, "model_id": 6, "width": W, "height": H,
     "params": [85.0, 83.0, 46.8, 32.2, -0.10, 0.02, 0.004, -0.003, 0.001, 0.02, 0.001, 0.0]},
]
# image_id, camera_id, name, camera centre
_IMAGES = [(1, 1, "view_a.png", (0.3, -0.2, -4.0)), (2, 2, "view_b.png", (2.6, 0.4, -3.0)),
           (3, 7, "sub/view_c.png", (-2.8, -0.5, -2.9)), (BIG + 9, BIG + 5, "view_d.png", (0.5, 2.0, -3.5)),
           (11, 1, "view_e.png", (-0.4, 0.3, -3.6)), (12, 7, "view_f.png", (1.5, -1.8, -3.2))]


def intrinsics(cam):
    """(fx, fy, cx, cy) in COLMAP coordinates and d[8] of a camera record (models 0-4 and 6)"""
    p = cam["params"]
    nf = 2 if cam["model_id"] in (1, 4, 6) else 1
    d = np.zeros(8)
    extra = p[nf + 2:]
    d[:len(extra)] = extra
    return (p[0], p[nf - 1], p[nf], p[nf + 1]), d


def rotation_looking_at_origin(centre, roll=0.0):
    """world -> camera rotation of a camera at ``centre`` whose +z axis points at the origin (x right, y down)"""
    z = -np.asarray(centre, dtype=float)
    z /= np.linalg.norm(z)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    c, s = np.cos(roll), np.sin(roll)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]) @ np.stack([x, y, z])


def quaternion(rot):
    """3 x 3 rotation -> unit (w, x, y, z), w >= 0 (these poses are far from a half turn)"""
    w = np.sqrt(1.0 + np.trace(rot)) / 2
    return np.array([w, (rot[2, 1] - rot[1, 2]) / (4 * w), (rot[0, 2] - rot[2, 0]) / (4 * w),
                     (rot[1, 0] - rot[0, 1]) / (4 * w)])


@functools.lru_cache(maxsize=None)
def reconstruction():
    """-> (cameras, images, points): lists of dicts in file order.  About 60 points in a cube around the origin, every
    image's observations made by projecting them through its camera's distorted model, plus a few 2-D points that
    belong to no 3-D point."""
    rng = np.random.default_rng(2024)
    cams = {c["camera_id"]: c for c in CAMERAS}
    ids = [int(v) for v in np.concatenate([rng.choice(5000, 40, replace=False) + 1,
                                           BIG + 100 + rng.choice(5000, 20, replace=False)])]
    rng.shuffle(ids)                                                   # file order is not id order
    points = [{"point3D_id": pid, "xyz": rng.uniform(-1.5, 1.5, 3), "rgb": rng.integers(0, 256, 3).astype(np.uint8),
               "error": float(rng.uniform(0.1, 2.0)), "track": []} for pid in ids]
    images = []
    for k, (image_id, camera_id, name, centre) in enumerate(_IMAGES):
        rot = rotation_looking_at_origin(centre, roll=0.1 * k)
        tvec = -rot @ np.asarray(centre, dtype=float)
        (fx, fy, cx, cy), d = intrinsics(cams[camera_id])
        xys, pids = [], []
        for p in points:
            pc = rot @ p["xyz"] + tvec
            xd, yd = UO.distort(d, pc[0] / pc[2], pc[1] / pc[2])
            xy = np.array([fx * xd + cx, fy * yd + cy])
            if rng.random() < 0.15:                                    # not matched in this image
                continue
            if 1.0 < xy[0] < W - 1.0 and 1.0 < xy[1] < H - 1.0:
                if rng.random() < 0.2:                                 # a detection without a 3-D point in between
                    xys.append(rng.uniform(0, 1, 2) * (W, H))
                    pids.append(-1)
                p["track"].append((image_id, len(xys)))
                xys.append(xy)
                pids.append(p["point3D_id"])
        images.append({"image_id": image_id, "qvec": quaternion(rot), "tvec": tvec, "camera_id": camera_id, "name": name,
                       "xys": np.array(xys).reshape(-1, 2), "point3D_ids": np.array(pids, dtype=np.int64)})
    for p in points:
        p["track"] = np.array(p["track"], dtype=np.uint32).reshape(-1, 2)
    return CAMERAS, images, points


# ------------------------------------------------------------------------------------------------ the writer
def cameras_bytes(cameras):
    out = [struct.pack("<Q", len(cameras))]
    for c in cameras:
        assert len(c["params"]) == NUM_PARAMS[c["model_id"]]
        out.append(struct.pack("<IiQQ", c["camera_id"], c["model_id"], c["width"], c["height"]))
        out.append(struct.pack(f"<{len(c['params'])}d", *c["params"]))
    return b"".join(out)


def images_bytes(images):
    out = [struct.pack("<Q", len(images))]
    for im in images:
        out.append(struct.pack("<I4d3dI", im["image_id"], *im["qvec"], *im["tvec"], im["camera_id"]))
        out.append(im["name"].encode("utf-8") + b"\0")
        out.append(struct.pack("<Q", len(im["point3D_ids"])))
        for (x, y), pid in zip(im["xys"], im["point3D_ids"]):
            out.append(struct.pack("<ddq", x, y, int(pid)))
    return b"".join(out)


def points_bytes(points):
    out = [struct.pack("<Q", len(points))]
    for p in points:
        out.append(struct.pack("<Q3d3BdQ", p["point3D_id"], *p["xyz"], *[int(v) for v in p["rgb"]], p["error"],
                               len(p["track"])))
        for image_id, idx in p["track"]:
            out.append(struct.pack("<II", int(image_id), int(idx)))
    return b"".join(out)


def write(folder, cameras=None, images=None, points=None):
    """writes the three files of the synthetic reconstruction (or of the given records) into ``folder``"""
    c, i, p = reconstruction()
    folder.mkdir(parents=True, exist_ok=True)
    (folder / "cameras.bin").write_bytes(cameras_bytes(c if cameras is None else cameras))
    (folder / "images.bin").write_bytes(images_bytes(i if images is None else images))
    (folder / "points3D.bin").write_bytes(points_bytes(p if points is None else points))
    return folder


def write_images(folder, seed=0):
    """one 97 x 61 PNG of random bytes per image of the synthetic reconstruction -> name -> uint8 [H, W, 3]"""
    from PIL import Image
    rng = np.random.default_rng(seed)
    out = {}
    for im in reconstruction()[1]:
        pixels = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        (folder / im["name"]).parent.mkdir(parents=True, exist_ok=True)
        Image.fromarray(pixels).save(folder / im["name"])
        out[im["name"]] = pixels
    return out
