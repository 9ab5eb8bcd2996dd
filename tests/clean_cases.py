"""Small meshes with known answers for the clean-up tests (tests/test_clean_cpu.py, tests/test_gpu_clean.py)."""
import numpy as np


def book(k, equal=False, seed=4):
    """``k`` triangles ("pages") on the spine edge (0, 1): page i is (0, 1, 2 + i), its far corner a unit from the spine
    at angle i.  Distinct areas: the far corner of page i lies ``heights[i]`` from the spine, a seeded permutation, so
    that the two largest pages are not the first two; ``equal`` (k <= 5): every far corner exactly a unit from the spine
    (A2 of a page is x^2 + y^2 of its far corner, whatever its z), at the quarter turns, the fifth on the first's
    half-plane at another height: coordinates float32 holds exactly, so every A2 is 1.0 to the bit.
    -> (vertices float32, faces int32, heights)."""
    spine = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    if equal:
        assert k <= 5
        heights = np.ones(k)
        far = np.array([[1.0, 0.0, 0.5], [0.0, 1.0, 0.5], [-1.0, 0.0, 0.5], [0.0, -1.0, 0.5], [1.0, 0.0, 0.25]])[:k]
    else:
        heights = 1.0 + np.random.default_rng(seed).permutation(k).astype(np.float64)
        ang = 2 * np.pi * np.arange(k) / k
        far = np.stack((heights * np.cos(ang), heights * np.sin(ang), np.full(k, 0.5)), -1)
    verts = np.concatenate((spine, far)).astype(np.float32)
    faces = np.stack((np.zeros(k, np.int64), np.ones(k, np.int64), 2 + np.arange(k)), -1).astype(np.int32)
    return verts, faces, heights


def renumbered(verts, faces, perm):
    """The mesh with vertex i renamed ``perm[i]``."""
    perm = np.asarray(perm)
    out = np.empty_like(verts)
    out[perm] = verts
    return out, perm[faces].astype(np.int32)


def tetrahedra(k, seed=0):
    """``k`` disjoint tetrahedra (4 k vertices, 4 k faces), the vertices numbered by a seeded shuffle."""
    rng = np.random.default_rng(seed)
    base = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32)
    verts = (base[None] * 0.5 + 2.0 * np.arange(k, dtype=np.float32)[:, None, None] * np.array([1, 0, 0], np.float32))
    verts = verts.reshape(-1, 3).astype(np.float32)
    tri = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])
    faces = (tri[None] + 4 * np.arange(k)[:, None, None]).reshape(-1, 3)
    return renumbered(verts, faces, rng.permutation(4 * k))


def strip(f, numbering="ascending", seed=0):
    """One triangle strip of ``f`` faces over ``f + 2`` vertices; ``numbering``: ascending, descending or random."""
    n = f + 2
    i = np.arange(n)
    verts = np.stack((0.5 * i, (i % 2).astype(np.float64), np.zeros(n)), -1).astype(np.float32)
    j = np.arange(f)
    faces = np.where((j % 2 == 0)[:, None], np.stack((j, j + 1, j + 2), -1), np.stack((j + 1, j, j + 2), -1))
    perm = {"ascending": i, "descending": i[::-1].copy(),
            "random": np.random.default_rng(seed).permutation(n)}[numbering]
    return renumbered(verts, faces, perm)


def fan(k):
    """``k`` triangles around one hub (an open fan over ``k + 2`` vertices); the hub has the largest index."""
    ang = np.pi * np.arange(k + 1) / k
    rim = np.stack((np.cos(ang), np.sin(ang), np.zeros(k + 1)), -1)
    verts = np.concatenate((rim, [[0.0, 0.0, 0.0]])).astype(np.float32)
    hub = k + 1
    faces = np.stack((np.full(k, hub), np.arange(k), np.arange(k) + 1), -1).astype(np.int32)
    return verts, faces


def grids(n, pieces=3, seed=0):
    """``pieces`` disjoint n x n height fields (2 (n - 1)^2 faces each), faces shuffled, vertices numbered at random."""
    rng = np.random.default_rng(seed)
    ij = np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 2)
    at = lambda i, j: i * n + j
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    i, j = i.reshape(-1), j.reshape(-1)
    one = np.concatenate((np.stack((at(i, j), at(i + 1, j), at(i, j + 1)), -1),
                          np.stack((at(i + 1, j), at(i + 1, j + 1), at(i, j + 1)), -1)))
    flat = np.zeros((n * n, 1))
    verts = np.concatenate([np.concatenate((0.1 * ij + 0.1 * (n + 3) * p, flat), 1) for p in range(pieces)])
    faces = np.concatenate([one + p * n * n for p in range(pieces)])
    rng.shuffle(faces)
    return renumbered(verts.astype(np.float32), faces, rng.permutation(pieces * n * n))
