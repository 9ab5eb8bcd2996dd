"""The mesh clean-up without a GPU: csrc/clean_math.h, built for the host from
tests/hostmath/clean.cpp, against numpy; known answers of the oracle (tests/clean_oracle.py); the definition on the
float64 oracle's meshes of the test scenes, unsimplified and simplified by tests/simplify_oracle.py; the configs; the C
entries' argument checks.  Every comparison is on integers or on doubles formed by identical IEEE operations: equality."""
import ctypes
import functools
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import clean_cases as CC
import clean_oracle as CO
import simplify_oracle as SO
import tinysplat_amd.clean  # noqa: F401  the feature under test: without it nothing here is collected

ROOT = Path(__file__).resolve().parent.parent
F32P, F64P, I32P, I64P = (ctypes.POINTER(t) for t in (ctypes.c_float, ctypes.c_double, ctypes.c_int32, ctypes.c_int64))
# the edge-valence histograms of the oracle's simplified meshes: {(scene, budget): (faces, {valence: edges})}
VALENCES = {("sphere", 2000): (1948, {2: 2865, 3: 18, 4: 15}), ("sphere", 200): (187, {2: 274, 3: 3, 4: 1}),
            ("sheet", 2000): (1877, {2: 2751, 3: 3, 4: 30}), ("sheet", 200): (134, {2: 59, 4: 68, 6: 2})}
SHEET_COMPONENTS = [13420, 984]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """g++ build of tests/hostmath/clean.cpp: the kernels' header compiled for the host."""
    so = tmp_path_factory.mktemp("clean") / "_clean.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                    str(ROOT / "tests" / "hostmath" / "clean.cpp"), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.cm_edge_keys.restype, lib.cm_edge_keys.argtypes = None, [ctypes.c_int64, ctypes.c_int32, I32P, I64P]
    lib.cm_face_weights.restype, lib.cm_face_weights.argtypes = None, [ctypes.c_int64, F32P, I32P, F64P]
    return lib


def _p(a, t):
    return a.ctypes.data_as(t)


def _meshes():
    from test_simplify_cpu import _meshes as oracle_meshes
    return oracle_meshes()


@functools.lru_cache(maxsize=None)
def _simplified(name, target):
    verts, faces = _meshes()[name]
    return SO.simplify(verts, faces, target=target)


# ------------------------------------------------------------------------------------------------ the header
def test_header_against_numpy(host):
    rng = np.random.default_rng(7)
    v, f = 5000, 20_000
    faces = rng.integers(0, v, (f, 3)).astype(np.int32)
    faces[:50, 1] = faces[:50, 0]                                       # self-edges have a key too
    keys = np.zeros(3 * f, np.int64)
    host.cm_edge_keys(f, v, _p(faces, I32P), _p(keys, I64P))
    assert np.array_equal(keys, CO.edge_keys(faces, v))
    a, b = faces[:, [0, 1, 2]].astype(np.int64), faces[:, [1, 2, 0]].astype(np.int64)
    assert np.array_equal(keys.reshape(-1, 3), np.minimum(a, b) * v + np.maximum(a, b))
    # the largest mesh int32 faces can name: the key stays below 2^62
    big = np.array([[2 ** 31 - 2, 2 ** 31 - 3, 0]], dtype=np.int32)
    keys = np.zeros(3, np.int64)
    host.cm_edge_keys(1, 2 ** 31 - 1, _p(big, I32P), _p(keys, I64P))
    assert keys.tolist() == [(2 ** 31 - 3) * (2 ** 31 - 1) + 2 ** 31 - 2, 2 ** 31 - 3, 2 ** 31 - 2]
    for scale in (1.0, 1e3):
        verts = (rng.standard_normal((v, 3)) * scale).astype(np.float32)
        verts[:10] = verts[0]                                           # zero area: three corners in one place,
        faces[50:60] = np.arange(30).reshape(10, 3) % 10
        verts[10:13] = verts[13] + np.outer([0.0, 1.0, 2.5], np.float32([1, 2, -1]))     # and on one line
        faces[60] = (10, 11, 12)
        w = np.zeros(f)
        host.cm_face_weights(f, _p(verts, F32P), _p(faces, I32P), _p(w, F64P))
        want = CO.face_weights(verts, faces)
        assert np.array_equal(w, want) and bool((w >= 0).all()) and bool((w[50:60] == 0).all())
        assert w[60] <= 1e-6 * scale ** 4 and np.median(w) > 0.1 * scale ** 4


# ------------------------------------------------------------------------------------------------ known answers
@pytest.mark.parametrize("k", [3, 4, 5])
def test_oracle_books(k):
    verts, faces, heights = CC.book(k)
    marked, edges = CO.nonmanifold_faces(verts, faces)
    assert edges == 1 and np.array_equal(np.flatnonzero(~marked), np.sort(np.argsort(-heights)[:2]))
    assert not np.array_equal(np.flatnonzero(~marked), [0, 1])          # the answer is not the first two by accident
    ov, of, info = CO.clean(verts, faces)
    assert of.shape == (2, 3) and ov.shape == (4, 3) and info["removed_nonmanifold_faces"] == k - 2
    assert np.array_equal(ov[of], verts[faces[~marked]])
    # equal areas, a k-way tie: the two lowest face indices stay
    verts, faces, _ = CC.book(k, equal=True)
    assert np.unique(CO.face_weights(verts, faces)).tolist() == [1.0] and faces.shape[0] == k
    marked, edges = CO.nonmanifold_faces(verts, faces)
    assert edges == 1 and np.flatnonzero(~marked).tolist() == [0, 1]
    # without the step nothing goes
    ov, of, info = CO.clean(verts, faces, manifold_edges=False)
    assert np.array_equal(of, faces) and info["removed_nonmanifold_faces"] == 0


def test_oracle_components_and_degenerate_faces():
    verts, faces = CC.tetrahedra(3, seed=1)
    vl, fl, labels, sizes = CO.components(faces, verts.shape[0])
    assert labels.size == 3 and sizes.tolist() == [4, 4, 4] and labels[0] == 0
    assert all(vl[faces[i]].tolist() == [fl[i]] * 3 for i in range(12))
    assert np.array_equal(labels, np.unique([faces[4 * t:4 * t + 4].min() for t in range(3)]))
    # two sheets that touch in one vertex are one component; an unreferenced vertex is labelled itself
    v = np.zeros((8, 3), np.float32)
    vl, fl, labels, sizes = CO.components([[1, 2, 3], [3, 4, 5]], 8)
    assert vl.tolist() == [0, 1, 1, 1, 1, 1, 6, 7] and labels.tolist() == [1] and sizes.tolist() == [2]
    # a face with two equal indices goes; a zero-area face with three distinct indices stays
    v[1], v[2], v[3] = (1, 0, 0), (2, 0, 0), (3, 0, 0)
    ov, of, info = CO.clean(v, [[1, 1, 2], [1, 2, 3], [5, 4, 5]])
    assert info["face_kept"].tolist() == [False, True, False] and of.tolist() == [[0, 1, 2]] and ov.shape == (3, 3)


# ------------------------------------------------------------------------------------------------ the oracle's meshes
@pytest.mark.parametrize("name", ["sphere", "sheet"])
def test_unsimplified_meshes_pass_the_edge_step_unchanged(name):
    verts, faces = _meshes()[name]
    hist = CO.valence_histogram(faces, verts.shape[0])
    print(f"\n{name}: {faces.shape[0]} faces, edge valences {hist}")
    assert hist == {2: {"sphere": 11976, "sheet": 21606}[name]}
    marked, edges = CO.nonmanifold_faces(verts, faces)
    assert edges == 0 and not marked.any() and not CO.degenerate(faces).any()
    ov, of, info = CO.clean(verts, faces)
    assert np.array_equal(ov, verts) and np.array_equal(of, faces) and info["face_kept"].all()


@pytest.mark.parametrize("name,target", sorted(VALENCES))
def test_simplified_meshes_lose_every_edge_above_valence_two(name, target):
    verts, faces = _simplified(name, target)
    want_faces, want_hist = VALENCES[(name, target)]
    hist = CO.valence_histogram(faces, verts.shape[0])
    print(f"\n{name} -> {target}: {faces.shape[0]} faces, edge valences {hist}")
    assert faces.shape[0] == want_faces and hist == want_hist
    ov, of, info = CO.clean(verts, faces)
    after = CO.valence_histogram(of, ov.shape[0])
    print(f"  cleaned: {of.shape[0]} faces ({info['removed_nonmanifold_faces']} removed at "
          f"{info['nonmanifold_edges']} edges), edge valences {after}")
    assert max(after) <= 2 and info["nonmanifold_edges"] == sum(n for val, n in want_hist.items() if val > 2)
    assert 0 < info["removed_nonmanifold_faces"] == faces.shape[0] - of.shape[0]
    # order kept, vertices untouched: the kept faces' corners are the input's, row for row
    assert np.array_equal(ov[of], verts[faces[info["face_kept"]]])
    assert np.array_equal(ov, verts[info["vertex_kept"]])
    # a second pass finds nothing
    again_v, again_f, again = CO.clean(ov, of)
    assert np.array_equal(again_f, of) and np.array_equal(again_v, ov) and again["removed_nonmanifold_faces"] == 0


def test_the_sheet_has_two_components_and_each_filter_drops_the_blob():
    verts, faces = _meshes()["sheet"]
    vl, fl, labels, sizes = CO.components(faces, verts.shape[0])
    # in label order the blob comes first here: it holds vertex 0
    assert sorted(sizes.tolist(), reverse=True) == SHEET_COMPONENTS and labels[0] == 0
    big, small = SHEET_COMPONENTS
    sheet_label, blob_label = labels[np.argmax(sizes)], labels[np.argmin(sizes)]
    blob = fl == blob_label
    for cfg in (dict(min_component_faces=small + 1), dict(min_component_fraction=(small + 1) / big),
                dict(keep_largest=1)):
        ov, of, info = CO.clean(verts, faces, **cfg)
        assert np.array_equal(info["face_kept"], ~blob) and info["kept_components"].tolist() == [sheet_label], cfg
        assert of.shape[0] == big and ov.shape[0] == int((vl == sheet_label).sum())
        assert np.array_equal(ov[of], verts[faces[~blob]])
    # at the threshold itself the blob stays
    for cfg in (dict(min_component_faces=small), dict(min_component_fraction=small / big), dict(keep_largest=2)):
        ov, of, info = CO.clean(verts, faces, **cfg)
        assert info["face_kept"].all() and np.array_equal(of, faces), cfg
    # a bar nothing meets: the empty mesh
    ov, of, info = CO.clean(verts, faces, min_component_faces=big + 1)
    assert ov.shape == (0, 3) and of.shape == (0, 3) and of.dtype == np.int32 and info["kept_components"].size == 0
    # the sphere is one component
    verts, faces = _meshes()["sphere"]
    assert CO.components(faces, verts.shape[0])[3].tolist() == [faces.shape[0]]


# ------------------------------------------------------------------------------------------------ configs and entries
def test_configs():
    from tinysplat_amd import CleanConfig, MeshConfig
    cfg = CleanConfig()
    assert cfg.manifold_edges is True and cfg.min_component_faces == 0 and cfg.min_component_fraction == 0.0
    assert cfg.keep_largest is None and MeshConfig().clean is None
    assert MeshConfig(clean=cfg).clean is cfg
    assert CleanConfig(min_component_fraction=1.0, keep_largest=1, min_component_faces=10 ** 9).keep_largest == 1
    assert CleanConfig(min_component_faces=np.int64(3), keep_largest=np.int32(2)).min_component_faces == 3
    for bad in (dict(min_component_faces=-1), dict(min_component_fraction=-0.01), dict(min_component_fraction=1.01),
                dict(min_component_fraction=float("nan")), dict(min_component_fraction=float("inf")),
                dict(keep_largest=0), dict(keep_largest=-2), dict(min_component_faces=2.7), dict(keep_largest=1.5),
                dict(min_component_faces=True), dict(min_component_faces=None)):
        with pytest.raises(ValueError):
            CleanConfig(**bad)
    with pytest.raises(ValueError):
        MeshConfig(clean=True)


def test_clean_mesh_refuses_before_any_launch():
    from tinysplat_amd import TriangleMesh, clean_mesh, mesh_components
    v = torch.zeros((4, 3))
    f = torch.zeros((2, 3), dtype=torch.int32)
    for fn in (clean_mesh, mesh_components):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(TriangleMesh(v, f, None))
        with pytest.raises(ValueError):
            fn(TriangleMesh(v[:, :2], f, None))
        with pytest.raises(ValueError):
            fn(TriangleMesh(v, f[:, :2], None))
        with pytest.raises(ValueError):
            fn(TriangleMesh(v, f.long(), None))
        with pytest.raises(ValueError):
            fn(TriangleMesh(v.double(), f, None))
        with pytest.raises(TypeError):
            fn(TriangleMesh(v.numpy(), f, None))


def test_entry_argument_checks():
    """None of these needs a device: every refusal, and every call with nothing to do, returns before a launch."""
    from tinysplat_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(16)
    # f, faces, flags, stream
    assert lib.ts_clean_degenerate(-1, p, p, None) == -1
    assert lib.ts_clean_degenerate(4, None, p, None) == -1 and lib.ts_clean_degenerate(4, p, None, None) == -1
    assert lib.ts_clean_degenerate(0, None, None, None) == 0
    # v, f, faces, keys, stream
    assert lib.ts_clean_edge_keys(-1, 4, p, p, None) == -1 and lib.ts_clean_edge_keys(8, -1, p, p, None) == -1
    assert lib.ts_clean_edge_keys(0, 4, p, p, None) == -1                # faces without vertices
    assert lib.ts_clean_edge_keys(8, 4, None, p, None) == -1 and lib.ts_clean_edge_keys(8, 4, p, None, None) == -1
    assert lib.ts_clean_edge_keys(8, 0, None, None, None) == 0 and lib.ts_clean_edge_keys(0, 0, None, None, None) == 0
    # v, f, vertices, faces, weights, stream
    good = [8, 4, p, p, p, None]
    for i in (2, 3, 4):
        a = list(good)
        a[i] = None
        assert lib.ts_clean_face_weights(*a) == -1, i
    assert lib.ts_clean_face_weights(-1, 4, p, p, p, None) == -1 and lib.ts_clean_face_weights(8, -1, p, p, p, None) == -1
    assert lib.ts_clean_face_weights(0, 4, p, p, p, None) == -1
    assert lib.ts_clean_face_weights(8, 0, None, None, None, None) == 0
    # f, entries, sorted_keys, order, marks, stream
    good = [4, 12, p, p, p, None]
    for i in (2, 3, 4):
        a = list(good)
        a[i] = None
        assert lib.ts_clean_mark(*a) == -1, i
    assert lib.ts_clean_mark(-1, -3, p, p, p, None) == -1
    for entries in (11, 13, 4, 0, -12):                                 # entries must be 3 f
        assert lib.ts_clean_mark(4, entries, p, p, p, None) == -1, entries
    assert lib.ts_clean_mark(0, 0, None, None, None, None) == 0 and lib.ts_clean_mark(0, 3, p, p, p, None) == -1
    # v, f, faces, parent, labels, stream
    good = [8, 4, p, p, p, None]
    for i in (2, 3, 4):
        a = list(good)
        a[i] = None
        assert lib.ts_clean_components(*a) == -1, i
    assert lib.ts_clean_components(-1, 4, p, p, p, None) == -1 and lib.ts_clean_components(8, -1, p, p, p, None) == -1
    assert lib.ts_clean_components(0, 4, p, p, p, None) == -1            # faces without vertices
    assert lib.ts_clean_components(8, 0, None, None, p, None) == -1      # the labels are still written
    assert lib.ts_clean_components(8, 0, None, p, None, None) == -1
    assert lib.ts_clean_components(0, 0, None, None, None, None) == 0
    assert lib.ts_abi_version() == 9 == _lib.ABI_VERSION
