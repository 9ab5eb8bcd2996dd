"""Point-cloud initialisation without a GPU: the k-NN oracle against the reference's fixtures, the PLY
reader, and the argument checks of the new C entries and Python API (nothing reaches a device)."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import GOLD
from knn_oracle import knn_oracle


@pytest.mark.parametrize("name", ["n600", "n4", "n300_f64"])
def test_oracle_matches_the_reference_fixture(name):
    z = np.load(GOLD / f"init_{name}.npz")
    d, _ = knn_oracle(z["xyz"], z["xyz"], 4)                   # at the input precision, as the reference searches
    md = np.mean(d[:, 1:].numpy(), axis=1).astype(np.float32)
    assert np.array_equal(md, z["mean_dist"])
    with np.errstate(divide="ignore"):
        assert np.array_equal(np.log(md), z["scales"][:, 0])
    assert (d[:, 0] == 0).all()
    if name == "n600":
        assert np.isinf(z["scales"][:, 0]).sum() == 11          # the block of 11 coincident points


def test_oracle_orders_ties_by_index():
    pts = torch.tensor([[0.0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, 0, 0], [2, 0, 0]])
    d, i = knn_oracle(pts[:1], pts, 5)
    assert i[0].tolist() == [0, 4, 1, 2, 3]
    assert d[0].tolist() == [0.0, 0.0, 1.0, 1.0, 1.0]


def test_read_point_cloud_ply_round_trip(tmp_path):
    from tinysplat_amd.init import read_point_cloud_ply
    g = np.random.default_rng(0)
    n = 37
    rec = np.zeros(n, dtype=[("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                             ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    for a in ("x", "y", "z", "nx", "ny", "nz"):
        rec[a] = g.normal(size=n)
    for a in ("red", "green", "blue"):
        rec[a] = g.integers(0, 256, size=n)
    types = {"<f8": "double", "<f4": "float", "u1": "uchar"}
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {n}"]
    head += [f"property {types[rec.dtype[a].str.replace('|', '')]} {a}" for a in rec.dtype.names]
    head += ["element face 0", "property list uchar int vertex_indices", "end_header"]
    path = tmp_path / "points.ply"
    path.write_bytes(("\n".join(head) + "\n").encode() + rec.tobytes())
    pcd = read_point_cloud_ply(path)
    assert pcd.xyz.dtype == torch.float64 and pcd.xyz.shape == (n, 3)
    assert np.array_equal(pcd.xyz.numpy(), np.stack([rec["x"], rec["y"], rec["z"]], 1))
    assert np.array_equal(pcd.colors.numpy(), np.stack([rec["red"], rec["green"], rec["blue"]], 1))
    assert pcd.point_ids.tolist() == list(range(n)) and (pcd.errors == 0).all()
    xyz, col, _ = pcd.get_points(torch.tensor([5, 2]))
    assert torch.equal(xyz, pcd.xyz[[5, 2]]) and torch.equal(col, pcd.colors[[5, 2]])
    bad = tmp_path / "ascii.ply"
    bad.write_bytes(b"ply\nformat ascii 1.0\nelement vertex 0\nend_header\n")
    with pytest.raises(ValueError):
        read_point_cloud_ply(bad)


def test_point_cloud_sorts_by_id():
    from tinysplat_amd import PointCloud
    pcd = PointCloud(torch.tensor([7, 3, 5]), torch.arange(9.0).view(3, 3), torch.zeros(3, 3), torch.tensor([1., 2, 3]))
    assert pcd.point_ids.tolist() == [3, 5, 7] and pcd.errors.tolist() == [2.0, 3.0, 1.0]


def test_knn_entries_reject_bad_arguments_without_a_gpu():
    from tinysplat_amd import _lib
    lib = _lib.load()
    one = (ctypes.c_float * 64)()
    ws = (ctypes.c_uint8 * 256)()
    assert lib.ts_knn_ws_bytes(1000, 1000, 4) > 0
    assert lib.ts_knn_ws_bytes(1000, 0, 16) > 0
    assert lib.ts_knn_ws_bytes(0, 10, 1) == -1 and lib.ts_knn_ws_bytes(10, 10, 0) == -1
    assert lib.ts_knn_ws_bytes(10, 10, 17) == -1 and lib.ts_knn_ws_bytes(3, 3, 4) == -1
    assert lib.ts_knn_ws_bytes(10, -1, 4) == -1
    # n < 1, k outside 1..16, k > n, NULL pointers with n > 0
    assert lib.ts_knn(0, one, 1, one, 1, one, one, ws, None, None) == -1
    assert lib.ts_knn(8, one, 8, one, 0, one, one, ws, None, None) == -1
    assert lib.ts_knn(20, one, 8, one, 17, one, one, ws, None, None) == -1
    assert lib.ts_knn(3, one, 3, one, 4, one, one, ws, None, None) == -1
    assert lib.ts_knn(8, None, 8, one, 4, one, one, ws, None, None) == -1
    assert lib.ts_knn(8, one, 8, None, 4, one, one, ws, None, None) == -1
    assert lib.ts_knn(8, one, 8, one, 4, None, one, ws, None, None) == -1
    assert lib.ts_knn(8, one, 8, one, 4, one, None, ws, None, None) == -1
    assert lib.ts_knn(8, one, 8, one, 4, one, one, None, None, None) == -1
    assert lib.ts_knn(8, one, -1, one, 4, one, one, ws, None, None) == -1
    args = [one] * 4 + [ws] + [one] * 7
    assert lib.ts_init_from_points(3, 15, *args, None, None) == -1            # fewer than 4 points
    assert lib.ts_init_from_points(8, -1, *args, None, None) == -1
    for j in range(12):
        if j == 8:
            continue                                                        # colors_rest: checked below
        a = list(args)
        a[j] = None
        assert lib.ts_init_from_points(8, 15, *a, None, None) == -1, j
    a = list(args)
    a[8] = None
    assert lib.ts_init_from_points(8, 15, *a, None, None) == -1             # colors_rest needed for k_rest > 0


def test_python_api_checks_before_any_device_call():
    from tinysplat_amd import PointCloud, from_pcd, knn_points
    x = torch.rand(10, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        knn_points(x, x, 4)
    for n in (0, 1, 3):
        pcd = PointCloud(torch.arange(n), torch.rand(n, 3), torch.zeros(n, 3, dtype=torch.uint8), torch.zeros(n))
        with pytest.raises(ValueError, match="at least 4"):
            from_pcd(pcd, device="cpu")
    xyz = torch.rand(6, 3)
    xyz[2, 1] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        from_pcd(PointCloud(torch.arange(6), xyz, torch.zeros(6, 3), torch.zeros(6)), device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        from_pcd(PointCloud(torch.arange(6), torch.rand(6, 3), torch.zeros(6, 3), torch.zeros(6)), device="cpu")
