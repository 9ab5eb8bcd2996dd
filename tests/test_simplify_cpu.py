"""The mesh simplifier without a GPU: csrc/simplify_math.h, built for the host from
tests/hostmath/simplify.cpp, against numpy (the cell of a coordinate, the Jacobi eigen-solve against
``numpy.linalg.eigh``, the representative against the oracle's); known answers of the oracle (tests/simplify_oracle.py);
the whole definition on the float64 meshes of tests/mesh_oracle.py; the configs; the C entries' argument checks."""
import ctypes
import functools
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import mesh_oracle as MO
import simplify_oracle as SO

ROOT = Path(__file__).resolve().parent.parent
F32P, F64P, I32P, I64P = (ctypes.POINTER(t) for t in (ctypes.c_float, ctypes.c_double, ctypes.c_int32, ctypes.c_int64))
SEED = 11
BOUNDS = ((-1.55, -1.52, 1.85), (1.53, 1.56, 4.2))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """g++ build of tests/hostmath/simplify.cpp: the kernels' header compiled for the host."""
    so = tmp_path_factory.mktemp("simplify") / "_simplify.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                    str(ROOT / "tests" / "hostmath" / "simplify.cpp"), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    f, d, i32, i64 = ctypes.c_float, ctypes.c_double, ctypes.c_int32, ctypes.c_int64
    lib.sm_cells.restype, lib.sm_cells.argtypes = i32, [f, f, f]
    lib.sm_cell.restype, lib.sm_cell.argtypes = i32, [f, f, f, i32]
    lib.sm_keys.restype, lib.sm_keys.argtypes = None, [i64, F32P, F32P, f, I32P, I64P]
    lib.sm_centre.restype, lib.sm_centre.argtypes = d, [f, f, i32]
    lib.sm_face_term.restype, lib.sm_face_term.argtypes = None, [F32P, F32P, F32P, F64P, F64P]
    lib.sm_jacobi.restype, lib.sm_jacobi.argtypes = None, [i64, F64P, i32, F64P, F64P]
    lib.sm_representative.restype, lib.sm_representative.argtypes = None, [i64, F64P, F64P, d, d, F64P]
    lib.sm_sweeps.restype, lib.sm_sweeps.argtypes = i32, []
    return lib


def _p(a, t):
    return a.ctypes.data_as(t)


def _host_keys(host, pts, lo, c, n):
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    keys = np.zeros(pts.shape[0], np.int64)
    lo, n = np.ascontiguousarray(lo, dtype=np.float32), np.ascontiguousarray(n, dtype=np.int32)
    host.sm_keys(pts.shape[0], _p(pts, F32P), _p(lo, F32P), np.float32(c), _p(n, I32P), _p(keys, I64P))
    return keys


def _host_representative(host, quad, vs, c, tau=SO.TAU):
    quad, vs = np.ascontiguousarray(quad, dtype=np.float64), np.ascontiguousarray(vs, dtype=np.float64)
    x = np.zeros((quad.shape[0], 3))
    host.sm_representative(quad.shape[0], _p(quad, F64P), _p(vs, F64P), float(c), tau, _p(x, F64P))
    return x


# ------------------------------------------------------------------------------------------------ the key function
def test_cell_of_a_coordinate(host):
    lo, c = np.float32(-1.25), np.float32(0.3)
    hi = np.float32(lo + np.float32(7.5) * c)
    n = host.sm_cells(lo, hi, c)
    assert n == 8 == int(SO.cells_per_axis(np.array([lo]), np.array([hi]), c)[0])
    # points exactly on cell faces: the float32 lo + i c may fall on either side of the face; the header and numpy agree
    walls = np.array([lo + np.float32(i) * c for i in range(9)], dtype=np.float32)
    around = np.concatenate([walls, np.nextafter(walls, np.float32(np.inf)), np.nextafter(walls, np.float32(-np.inf))])
    around = around[around >= lo]
    want = SO.cell_of(np.stack((around,) * 3, -1), np.array([lo] * 3), c, np.array([n] * 3))[:, 0]
    got = np.array([host.sm_cell(p, lo, c, n) for p in around])
    assert np.array_equal(got, want) and got.min() == 0 and got.max() == n - 1
    assert host.sm_cell(lo, lo, c, n) == 0 and host.sm_cell(np.float32(lo + c), lo, c, n) in (0, 1)
    # a power-of-two grid: the walls are exact, and a point on wall i opens cell i
    for i in range(8):
        assert host.sm_cell(np.float32(2.0 + 0.25 * i), np.float32(2.0), np.float32(0.25), 8) == i
    # the upper bound lies on the last wall (or beyond it): clamped into the last cell
    assert host.sm_cell(np.float32(4.0), np.float32(2.0), np.float32(0.25), 8) == 7
    assert host.sm_cell(hi, lo, c, n) == n - 1 and host.sm_cell(np.float32(1e30), lo, c, n) == n - 1
    for r in (1, 2, 3, 7, 37, 1000, 1 << 20):
        a, b = np.float32(0.1), np.float32(0.7)
        cc = SO.edge_at(np.array([a]), np.array([b]), r)
        nn = host.sm_cells(a, b, cc)
        assert nn in (r, r + 1) and host.sm_cell(b, a, cc, nn) == nn - 1
    # an axis of one cell: everything in cell 0, even with no extent at all; below lo and not-a-number: cell 0
    assert host.sm_cells(np.float32(1.0), np.float32(1.0), c) == 1 and host.sm_cells(lo, np.float32(lo + 0.2), c) == 1
    assert host.sm_cell(np.float32(1.0), np.float32(1.0), c, 1) == 0 and host.sm_cell(np.float32(9.0), lo, c, 1) == 0
    assert host.sm_cell(np.float32(-5.0), lo, c, n) == 0 and host.sm_cell(np.float32(np.nan), lo, c, n) == 0
    # keys over a random cloud with flat axes, against the oracle
    rng = np.random.default_rng(0)
    pts = rng.random((5000, 3), dtype=np.float32) * np.array([2.0, 0.0, 0.31], dtype=np.float32) + np.float32(3.0)
    plo, phi = pts.min(0), pts.max(0)
    for r in (1, 5, 64, 4097):
        cc = SO.edge_at(plo, phi, r)
        nn = SO.cells_per_axis(plo, phi, cc)
        assert nn[1] == 1 and [host.sm_cells(plo[a], phi[a], cc) for a in range(3)] == nn.tolist()
        assert np.array_equal(_host_keys(host, pts, plo, cc, nn), SO.keys_of(SO.cell_of(pts, plo, cc, nn), nn))
    assert abs(host.sm_centre(lo, c, 3) - (float(lo) + 3.5 * float(c))) < 1e-15


# ------------------------------------------------------------------------------------------------ the eigen-solve
def _psd_matrices(count=10_000, seed=5):
    """Seeded symmetric PSD matrices [count,3,3]: full rank over nine decades of conditioning, rank 2 (a crease), rank 1
    (a plane), equal eigenvalues (two and three), already diagonal, and the zero matrix."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((count, 3, 3)))
    lam = 10.0 ** rng.uniform(-6, 3, (count, 3))
    kind = np.arange(count) % 8
    lam[kind == 1, 0] = 0.0                                             # rank 2
    lam[kind == 2, :2] = 0.0                                            # rank 1
    lam[kind == 3, 1] = lam[kind == 3, 0]                               # a double eigenvalue
    lam[kind == 4] = lam[kind == 4, :1]                                 # a multiple of the identity
    q[kind == 5] = np.eye(3)                                            # diagonal already
    lam[kind == 6] = 0.0                                                # zero
    lam[kind == 7] *= 1e12                                              # large entries: area-weighted normals squared
    A = np.einsum("nij,nj,nkj->nik", q, lam, q)
    return 0.5 * (A + A.transpose(0, 2, 1)), lam


def _six(A):
    return np.ascontiguousarray(np.stack((A[:, 0, 0], A[:, 0, 1], A[:, 0, 2], A[:, 1, 1], A[:, 1, 2], A[:, 2, 2]), -1))


def test_jacobi_against_eigh(host):
    """Reconstruction V diag(lambda) V^T - A and orthonormality after the header's sweep count, and after fewer: the
    sweep at which the worst of 10 000 matrices has converged is printed and must leave a margin."""
    A, _ = _psd_matrices()
    six = _six(A)
    count = A.shape[0]
    scale = np.maximum(np.abs(A).max((1, 2)), 1e-300)
    worst = {}
    for sweeps in range(1, host.sm_sweeps() + 1):
        lam, vec = np.zeros((count, 3)), np.zeros((count, 3, 3))
        host.sm_jacobi(count, _p(six, F64P), sweeps, _p(lam, F64P), _p(vec, F64P))
        rec = np.einsum("nij,nj,nkj->nik", vec, lam, vec)
        worst[sweeps] = (float((np.abs(rec - A).max((1, 2)) / scale).max()),
                         float(np.abs(np.einsum("nji,njk->nik", vec, vec) - np.eye(3)).max()))
    print("\nJacobi sweeps -> worst relative reconstruction error, worst |V^T V - I|:")
    for s, (a, b) in worst.items():
        print(f"  {s}: {a:.3e} {b:.3e}")
    converged = min(s for s, (a, b) in worst.items() if a < 1e-14 and b < 1e-14)
    assert converged <= host.sm_sweeps() - 2, worst
    assert worst[host.sm_sweeps()][0] < 1e-14 and worst[host.sm_sweeps()][1] < 1e-14
    # the eigenvalues are eigh's (sorted), to the rounding of the largest
    ref = np.linalg.eigvalsh(A)
    assert float((np.abs(np.sort(lam, -1) - ref).max(-1) / scale).max()) < 1e-14


def test_representative_against_the_oracle(host):
    """The truncated pseudo-inverse solution of the header against the oracle's eigh solve on the same sums: equal to
    the conditioning 1 / tau wherever no eigenvalue ratio sits at tau and the solution is not at the cell's wall."""
    A, _ = _psd_matrices()
    count = A.shape[0]
    rng = np.random.default_rng(9)
    c = 0.25
    n_hat = rng.standard_normal((count, 3))
    quad = np.zeros((count, 10))
    quad[:, :6] = _six(A)
    # b = -A x* for a point x* inside (or, for a third, outside) the cell, so that the minimiser is x* on A's range
    xs = rng.uniform(-0.12, 0.12, (count, 3)) * np.where(np.arange(count)[:, None] % 3 == 0, 3.0, 1.0)
    quad[:, 6:9] = -np.einsum("nij,nj->ni", A, xs)
    quad[:, 9] = np.einsum("ni,ni->n", xs, -quad[:, 6:9])
    vs = np.concatenate((rng.uniform(-0.1, 0.1, (count, 3)), np.ones((count, 1))), 1) * rng.integers(1, 9, (count, 1))
    x, m, y, lam, used = SO.representative(quad, vs, c, parts=True)
    got = _host_representative(host, quad, vs, c)
    stable = ~SO.unstable({"lam": lam, "y": y, "c": c})
    assert stable.mean() > 0.99 and 0.2 < used.mean() < 0.95
    err = np.abs(got - x).max(-1)
    print(f"\nrepresentative: worst |x - oracle| / c over {int(stable.sum())} stable problems {err[stable].max() / c:.3e}")
    assert err[stable].max() <= 1e-11 * c                   # 1 / tau = 1e3 times double rounding, with room
    assert bool((np.abs(got) <= c / 2).all())
    # the zero matrix and one not finite: the mean itself, to the bit
    zero = np.flatnonzero(~(lam[:, 2] > 0))
    assert zero.size > 1000 and np.array_equal(got[zero], m[zero])
    bad = quad[:4].copy()
    bad[0, 0], bad[1, 4], bad[2, 6], bad[3, 9] = np.inf, np.nan, np.nan, np.nan
    gb = _host_representative(host, bad, vs[:4], c)
    assert np.array_equal(gb[:3], vs[:3, :3] / vs[:3, 3:]) and bool(np.isfinite(gb).all())


def _cluster_sums(host, pts, faces, c=1.0):
    """The sums of one cell [0, c)^3 around vertices ``pts`` (all inside it) from ``faces`` through the header."""
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    g = np.full(3, 0.5 * c)
    quad = np.zeros(10)
    for f in faces:
        q = np.zeros(10)
        a, b, cc = (np.ascontiguousarray(pts[i]) for i in f)
        for _ in range(3):                                              # its three corners lie in this one cluster
            host.sm_face_term(_p(a, F32P), _p(b, F32P), _p(cc, F32P), _p(g, F64P), _p(q, F64P))
            quad += q
    vs = np.concatenate(((pts.astype(np.float64) - g).sum(0), [pts.shape[0]]))
    return quad, vs, g


def test_known_answers(host):
    rng = np.random.default_rng(2)
    # vertices on a plane inside one cell: the representative is the projection of the mean onto the plane, i.e. the mean
    nrm = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    basis = np.linalg.svd(nrm[None, :])[2][1:]
    pts = (np.array([0.5, 0.45, 0.55]) + rng.uniform(-0.2, 0.2, (12, 2)) @ basis).astype(np.float32)
    faces = [(0, 1, 2), (2, 3, 4), (5, 6, 7), (8, 9, 10), (1, 11, 4)]
    quad, vs, g = _cluster_sums(host, pts, faces)
    x = _host_representative(host, quad[None], vs[None], 1.0)[0]
    m = vs[:3] / vs[3]
    assert np.abs(x - m).max() < 1e-7 and abs(np.dot(nrm, g + x - np.array([0.5, 0.45, 0.55]))) < 1e-7
    xo = SO.representative(quad[None], vs[None], 1.0)[0]
    assert np.abs(x - xo).max() < 1e-12
    # the same faces, the mean pushed off the plane by a vertex no face uses: projected back along the normal
    off = np.concatenate((pts, (np.array([0.5, 0.45, 0.55]) + 0.2 * nrm)[None].astype(np.float32)))
    quad2, vs2, _ = _cluster_sums(host, off, faces)
    x2 = _host_representative(host, quad2[None], vs2[None], 1.0)[0]
    m2 = vs2[:3] / vs2[3]
    foot = m2 - nrm * np.dot(nrm, g + m2 - np.array([0.5, 0.45, 0.55]))
    assert np.abs(x2 - foot).max() < 1e-6 and np.abs(m2 - foot).max() > 1e-2
    # three mutually orthogonal planes: their corner when it lies inside the cell ...
    for corner, inside in ((np.array([0.4, 0.6, 0.3]), True), (np.array([0.4, 0.6, 1.3]), False)):
        tri = []
        for ax in range(3):
            for _ in range(2):
                t = rng.uniform(0.1, 0.9, (3, 3))
                t[:, ax] = corner[ax]
                tri.append(t)
        pts = np.concatenate(tri).astype(np.float32)
        faces = [(3 * i, 3 * i + 1, 3 * i + 2) for i in range(6)]
        quad, vs, g = _cluster_sums(host, pts, faces)
        x = _host_representative(host, quad[None], vs[None], 1.0)[0]
        if inside:
            assert np.abs(g + x - corner).max() < 1e-6
        else:                                                           # ... otherwise the mean, to the bit
            assert np.array_equal(x, vs[:3] / vs[3])
        assert np.abs(x - SO.representative(quad[None], vs[None], 1.0)[0]).max() < 1e-12
    # a single vertex, with or without faces (all their area outside the cell: any plane through it leaves it in place)
    p = np.array([[0.3, 0.7, 0.2]], dtype=np.float32)
    x = _host_representative(host, np.zeros((1, 10)), np.array([[*(p[0].astype(np.float64) - 0.5), 1.0]]), 1.0)[0]
    assert np.array_equal((0.5 + x).astype(np.float32), p[0])
    fan = np.concatenate((p, np.array([[3.0, 0.1, 0.2], [0.2, 4.0, 0.1], [0.1, 0.3, 5.0]], dtype=np.float32)))
    quad = np.zeros(10)
    q = np.zeros(10)
    for f in ((0, 1, 2), (0, 2, 3), (0, 3, 1)):
        a, b, cc = (np.ascontiguousarray(fan[i]) for i in f)
        host.sm_face_term(_p(a, F32P), _p(b, F32P), _p(cc, F32P), _p(np.full(3, 0.5), F64P), _p(q, F64P))
        quad += q
    x = _host_representative(host, quad[None], np.array([[*(p[0].astype(np.float64) - 0.5), 1.0]]), 1.0)[0]
    assert np.array_equal((0.5 + x).astype(np.float32), p[0])
    # the oracle end to end on a single far-apart triangle and on one whose corners share a cell
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float32)
    ov, of = SO.simplify(v, [[0, 1, 2]], cell_size=0.25)
    assert np.array_equal(ov, v) and np.array_equal(of, [[0, 1, 2]])
    ov, of = SO.simplify(v, [[0, 1, 2]], cell_size=2.0)
    assert ov.shape == (0, 3) and of.shape == (0, 3) and of.dtype == np.int32


# ------------------------------------------------------------------------------------------------ the whole definition
@functools.lru_cache(maxsize=None)
def _meshes():
    """The float64 oracle's meshes, as float32 vertices: the analytic sphere and the sheet-and-blob scene."""
    out = {}
    params = MO.sphere_params()
    lo, h, cells = MO.make_grid((-1.03, -0.98, -1.01), (0.97, 1.02, 0.99), 24)
    pos = MO.corner_positions(lo, h, cells)
    d, _ = MO.corner_densities(params, pos, torch.float64)
    m = MO.march(d, 0.3, pos)
    _, faces, verts = MO.weld(m["keys"], m["pos"])
    out["sphere"] = (verts.astype(np.float32), faces.astype(np.int32))
    lo, h, cells = MO.make_grid(*BOUNDS, 37)
    pos = MO.corner_positions(lo, h, cells)
    d, _ = MO.corner_densities(MO.sheet_scene(SEED), pos, torch.float64)
    m = MO.march(d, 0.3, pos)
    _, faces, verts = MO.weld(m["keys"], m["pos"])
    out["sheet"] = (verts.astype(np.float32), faces.astype(np.int32))
    return out


@pytest.mark.parametrize("name", ["sphere", "sheet"])
def test_the_definition_on_the_oracle_meshes(host, name):
    verts, faces = _meshes()[name]
    f = faces.shape[0]
    assert f > 2000
    for target in (10, 200, 2000):
        ov, of, info = SO.simplify(verts, faces, target=target, parts=True)
        lo, c, n = info["lo"], info["c"], info["cells"]
        assert of.shape[0] <= target and of.dtype == np.int32 and ov.dtype == np.float32
        if info["r"] == 1:                      # a budget below what two clusters per axis leave: the empty mesh
            assert target == 10 and of.shape == (0, 3) and ov.shape == (0, 3)
            continue
        assert of.shape[0] > target // 4
        hi = verts.max(0)
        assert SO.count(verts, faces, lo, hi, info["r"]) <= target < SO.count(verts, faces, lo, hi, info["r"] + 1) \
            or info["r"] == SO.R_MAX
        # no face with a repeated index, the smallest first, no duplicate rows, ascending
        assert bool(((of[:, 0] < of[:, 1]) & (of[:, 0] < of[:, 2]) & (of[:, 1] != of[:, 2])).all())
        assert np.unique(of, axis=0).shape[0] == of.shape[0]
        assert np.array_equal(of, of[np.lexsort((of[:, 2], of[:, 1], of[:, 0]))])
        # every vertex referenced, in ascending key order
        assert np.array_equal(np.unique(of), np.arange(ov.shape[0])) and bool(np.all(np.diff(info["keys"]) > 0))
        # every vertex within its cluster's cell, to one float32 ulp
        wall_lo = lo.astype(np.float64) + info["cell"] * np.float64(c)
        wall_hi = wall_lo + np.float64(c)
        ulp = np.spacing(np.maximum(np.abs(ov), np.float32(c)).astype(np.float32)).astype(np.float64)
        assert bool(((ov >= wall_lo - ulp) & (ov <= wall_hi + ulp)).all())
        # the header's keys and representatives on the oracle's clusters
        assert np.array_equal(np.unique(_host_keys(host, verts, lo, c, n)),
                              np.unique(SO.keys_of(SO.cell_of(verts, lo, c, n), n)))
        got = _host_representative(host, info["quad"], info["vsum"], c)
        stable = ~SO.unstable(info)
        share = 1.0 - stable.mean()
        dev = np.abs(got - info["x"]).max(-1) / float(c)
        print(f"\n{name} target {target}: r {info['r']} ({info['probes']} probes), {ov.shape[0]} vertices, "
              f"{of.shape[0]} faces, unstable clusters {share:.4%}, solution kept {info['used'].mean():.3f}, header "
              f"against oracle {dev[stable].max():.3e} c (all clusters {dev.max():.3e} c)")
        assert share <= 0.01 and dev[stable].max() < 1e-9
    # identity when the budget already holds
    ov, of = SO.simplify(verts, faces, target=f)
    assert ov is verts and np.array_equal(of, faces)
    # a cell below the shortest edge: every vertex its own cluster, the faces unchanged up to rotation and order
    e = np.concatenate([np.linalg.norm(verts[faces[:, k]] - verts[faces[:, (k + 1) % 3]], axis=1) for k in range(3)])
    ov, of, info = SO.simplify(verts, faces, cell_size=float(e[e > 0].min()) / 2.0, parts=True)
    if np.all(e > 0):
        assert ov.shape == verts.shape and MO.rotation_set(info["keys"][of]) == MO.rotation_set(
            SO.keys_of(SO.cell_of(verts, info["lo"], info["c"], info["cells"]), info["cells"])[faces])


def test_oracle_drops_unreferenced_vertices_and_keeps_mirrored_pairs():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [9, 9, 9], [0.01, 0, 0]], dtype=np.float32)
    ov, of = SO.simplify(v, [[0, 1, 2], [2, 1, 0], [1, 2, 4], [0, 1, 2]], cell_size=0.25)
    # vertex 3 is in no face: it widens no bound and makes no cluster; 0 and 4 share a cell; (0,1,2) twice is one row;
    # (0,1,2) and (0,2,1) are the same corners wound both ways, and both stay
    assert ov.shape == (3, 3) and of.tolist() == [[0, 1, 2], [0, 2, 1]]


# ------------------------------------------------------------------------------------------------ configs and entries
def test_configs():
    from tinysplat_amd import MeshConfig, SimplifyConfig
    cfg = SimplifyConfig()
    assert cfg.target_faces == 250_000 and cfg.cell_size is None and cfg.singular_threshold == 1e-3
    assert cfg.max_workspace_bytes == 256 << 20 and MeshConfig().target_faces is None
    assert SimplifyConfig(target_faces=None, cell_size=0.1).target_faces is None
    assert MeshConfig(target_faces=1).target_faces == 1
    for bad in (dict(target_faces=0), dict(target_faces=-3), dict(target_faces=None), dict(cell_size=0.0),
                dict(cell_size=-1.0), dict(cell_size=float("nan")), dict(cell_size=float("inf")),
                dict(singular_threshold=0.0), dict(singular_threshold=1.0), dict(singular_threshold=-0.1),
                dict(singular_threshold=float("nan")), dict(max_workspace_bytes=0)):
        with pytest.raises(ValueError):
            SimplifyConfig(**bad)
    for bad in (0, -1):
        with pytest.raises(ValueError):
            MeshConfig(target_faces=bad)


def test_simplify_mesh_refuses_before_any_launch():
    from tinysplat_amd import SimplifyConfig, TriangleMesh, simplify_mesh
    v = torch.zeros((4, 3))
    f = torch.zeros((2, 3), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        simplify_mesh(TriangleMesh(v, f, None), SimplifyConfig(target_faces=1))
    with pytest.raises(ValueError):
        simplify_mesh(TriangleMesh(v[:, :2], f, None))
    with pytest.raises(ValueError):
        simplify_mesh(TriangleMesh(v, f.long(), None))
    with pytest.raises(ValueError):
        simplify_mesh(TriangleMesh(v.double(), f, None))
    with pytest.raises(ValueError):
        simplify_mesh(TriangleMesh(v, f, None), color_sh_degree=4)


def test_entry_argument_checks():
    from tinysplat_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(16)
    grid = (ctypes.c_float * 4)(0.0, 0.0, 0.0, 0.5)
    cells = (ctypes.c_int32 * 3)(4, 4, 4)
    bad_grids = [((ctypes.c_float * 4)(0.0, 0.0, 0.0, 0.0), cells), ((ctypes.c_float * 4)(0.0, 0.0, 0.0, -1.0), cells),
                 ((ctypes.c_float * 4)(float("nan"), 0.0, 0.0, 0.5), cells),
                 ((ctypes.c_float * 4)(0.0, 0.0, 0.0, float("inf")), cells), (grid, (ctypes.c_int32 * 3)(4, 0, 4)),
                 (grid, (ctypes.c_int32 * 3)(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)), (None, cells), (grid, None)]

    def check(fn, good, pointers, sizes, grid_at, empty, nullable=()):
        """``good``: arguments that would launch; every NULL pointer, negative size and bad grid is refused, and the
        ``empty`` changes (nothing to do) succeed without a launch whatever the pointers."""
        def call(**change):
            a = list(good)
            for i, v in change.items():
                a[int(i[1:])] = v
            return fn(*a)
        for i in pointers:
            assert call(**{f"a{i}": None}) == (0 if i in nullable else -1), (fn.__name__, i)
        for i in sizes:
            assert call(**{f"a{i}": -1}) == -1, (fn.__name__, i)
        for g, c in bad_grids:
            assert call(**{f"a{grid_at}": g, f"a{grid_at + 1}": c}) == -1, fn.__name__
        for change in empty:
            a = list(good)
            for i in pointers:
                a[i] = None
            for i, v in change.items():
                a[i] = v
            assert fn(*a) == 0, (fn.__name__, change)
        return call

    # v, f, vertices, faces, grid_host, cells_host, block_counts, stream
    call = check(lib.ts_simplify_count, [8, 4, p, p, grid, cells, p, None], (2, 3, 6), (0, 1), 4, [{1: 0}, {0: 0, 1: 0}])
    assert call(a0=0) == -1                                             # faces without vertices
    # v, vertices, grid_host, cells_host, keys, stream
    check(lib.ts_simplify_keys, [8, p, grid, cells, p, None], (1, 4), (0,), 2, [{0: 0}])
    # v, f, clusters, vertices, faces, grid, cells, what, entries, clusters_sorted, order, chunk0, chunks, sums, ws, stream
    good = [8, 100, 5, p, p, grid, cells, 0, 300, p, p, 0, 3, p, p, None]
    call = check(lib.ts_simplify_accumulate, good, (3, 4, 9, 10, 13, 14), (0, 1, 2, 8, 11, 12), 5,
                 [{12: 0}, {1: 0, 8: 0, 12: 0}])
    assert call(a7=2) == -1 and call(a7=-1) == -1                       # an unknown kind of entry
    assert call(a8=299) == -1 and call(a7=1) == -1                      # entries must be 3 f, or v for the vertices
    assert call(a12=4) == -1 and call(a11=3, a12=1) == -1 and call(a11=2, a12=2) == -1      # 300 entries: 3 chunks
    assert call(a0=0) == -1 and call(a2=0) == -1
    assert lib.ts_simplify_accumulate(8, 0, 5, p, None, grid, cells, 1, 8, p, p, 0, 1, p, None, None) == -1   # ws NULL
    assert lib.ts_simplify_accumulate(8, 0, 5, None, None, grid, cells, 1, 8, None, None, 1, 0, None, None, None) == 0
    assert lib.ts_simplify_ws_bytes(0) == -1 and lib.ts_simplify_ws_bytes(-2) == -1
    assert lib.ts_simplify_ws_bytes((1 << 40) + 1) == -1
    assert lib.ts_simplify_ws_bytes(1) == 768 and lib.ts_simplify_ws_bytes(1000) == 2 * 80128 + 4096
    # clusters, cluster_keys, grid, cells, quadrics, vertex_sums, singular_threshold, representatives, stream
    call = check(lib.ts_simplify_solve, [5, p, grid, cells, p, p, 1e-3, p, None], (1, 4, 5, 7), (0,), 2, [{0: 0}])
    for tau in (0.0, 1.0, -0.5, 2.0, float("nan")):
        assert call(a6=tau) == -1 and call(a0=0, a6=tau) == -1
    # v, f, faces, vertex_cluster, out_faces, keep, stream
    good = [8, 4, p, p, p, p, None]
    for i in (2, 3, 4, 5):
        a = list(good)
        a[i] = None
        assert lib.ts_simplify_faces(*a) == -1, i
    assert lib.ts_simplify_faces(-1, 4, p, p, p, p, None) == -1 and lib.ts_simplify_faces(8, -1, p, p, p, p, None) == -1
    assert lib.ts_simplify_faces(0, 4, p, p, p, p, None) == -1
    assert lib.ts_simplify_faces(8, 0, None, None, None, None, None) == 0
    assert lib.ts_simplify_faces(0, 0, None, None, None, None, None) == 0
    assert lib.ts_abi_version() == 9 == _lib.ABI_VERSION
