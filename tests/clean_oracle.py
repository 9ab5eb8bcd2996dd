"""numpy restatement of the mesh clean-up (tinysplat_amd.clean), for the tests.

Everything here is integers, or doubles formed by the IEEE operations the kernels form (csrc/clean_math.h), so every
comparison against the GPU is for equality.  The components come from scipy's ``connected_components`` over the graph of
the faces' edges, relabelled by each component's smallest vertex: another algorithm than the kernel's union-find.
"""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components


def edge_keys(faces, v):
    """int64 [3 F]: entry 3 face + k is min V + max of the edge from corner k to corner (k + 1) % 3."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    a, b = faces, np.roll(faces, -1, axis=1)
    return (np.minimum(a, b) * np.int64(v) + np.maximum(a, b)).reshape(-1)


def face_weights(vertices, faces):
    """float64 [F]: A2 = (n_x n_x + n_y n_y) + n_z n_z, n = (b - a) x (c - a), in double from the float32 positions; the
    differences first, each cross component one product minus another."""
    p = np.asarray(vertices, dtype=np.float32).astype(np.float64)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    a, b, c = p[faces[:, 0]], p[faces[:, 1]], p[faces[:, 2]]
    u, w = b - a, c - a
    nx = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
    ny = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
    nz = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
    return (nx * nx + ny * ny) + nz * nz


def valence_histogram(faces, v):
    """{valence: number of undirected edges that this many faces use}."""
    _, counts = np.unique(edge_keys(faces, v), return_counts=True)
    val, n = np.unique(counts, return_counts=True)
    return {int(a): int(b) for a, b in zip(val, n)}


def degenerate(faces):
    """bool [F]: two equal indices."""
    faces = np.asarray(faces).reshape(-1, 3)
    return (faces[:, 0] == faces[:, 1]) | (faces[:, 1] == faces[:, 2]) | (faces[:, 0] == faces[:, 2])


def nonmanifold_faces(vertices, faces):
    """bool [F]: the faces that step 1 removes - at every edge of more than two faces, those of rank two and above by
    (A2 descending, face index ascending) - and the number of such edges.  No face may be degenerate."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    f = faces.shape[0]
    marked = np.zeros(f, dtype=bool)
    if f == 0:
        return marked, 0
    keys = edge_keys(faces, np.asarray(vertices).shape[0])
    face = np.repeat(np.arange(f), 3)
    a2 = np.repeat(face_weights(vertices, faces), 3)
    order = np.lexsort((face, -a2, keys))
    sk = keys[order]
    start = np.flatnonzero(np.concatenate(([True], sk[1:] != sk[:-1])))
    length = np.diff(np.concatenate((start, [sk.size])))
    rank = np.arange(sk.size) - np.repeat(start, length)
    marked[face[order][rank >= 2]] = True
    return marked, int((length > 2).sum())


def components(faces, v):
    """``(vertex_labels int32 [V], face_labels int32 [F], labels int32 [C], sizes int64 [C])``: a component's label is its
    smallest vertex index; a vertex in no face is labelled itself; the components with a face, ascending."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    rows = np.concatenate((faces[:, 0], faces[:, 1]))
    cols = np.concatenate((faces[:, 1], faces[:, 2]))
    graph = coo_matrix((np.ones(rows.size, dtype=np.int8), (rows, cols)), shape=(v, v))
    _, comp = connected_components(graph, directed=False)
    smallest = np.full(comp.max() + 1 if v else 0, v, dtype=np.int64)
    np.minimum.at(smallest, comp, np.arange(v))
    vertex_labels = smallest[comp].astype(np.int32)
    face_labels = vertex_labels[faces[:, 0]]
    labels, sizes = np.unique(face_labels, return_counts=True)
    return vertex_labels, face_labels.astype(np.int32), labels.astype(np.int32), sizes.astype(np.int64)


def kept_components(sizes, min_faces=0, min_fraction=0.0, keep_largest=None):
    """bool [C] over components in ascending label order."""
    sizes = np.asarray(sizes, dtype=np.int64)
    keep = sizes >= int(min_faces)
    if sizes.size:
        keep &= sizes.astype(np.float64) >= np.float64(min_fraction) * np.float64(sizes.max())
        if keep_largest is not None:
            ranked = np.lexsort((np.arange(sizes.size), -sizes))        # size descending, label ascending
            among = np.zeros(sizes.size, dtype=bool)
            among[ranked[:int(keep_largest)]] = True
            keep &= among
    return keep


def clean(vertices, faces, manifold_edges=True, min_component_faces=0, min_component_fraction=0.0, keep_largest=None):
    """-> ``(vertices, faces, info)``: ``info`` holds ``face_kept`` bool [F] and ``vertex_kept`` bool [V] over the input,
    ``removed_nonmanifold_faces``, ``nonmanifold_edges``, ``components``, ``sizes`` and ``kept_components``."""
    vertices = np.asarray(vertices, dtype=np.float32)
    faces = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    v = vertices.shape[0]
    at = np.flatnonzero(~degenerate(faces))                             # the input rows still alive
    removed_nm, nm_edges = 0, 0
    if manifold_edges:
        marked, nm_edges = nonmanifold_faces(vertices, faces[at])
        removed_nm = int(marked.sum())
        at = at[~marked]
    _, face_labels, labels, sizes = components(faces[at], v)
    keep = kept_components(sizes, min_component_faces, min_component_fraction, keep_largest)
    at = at[np.isin(face_labels, labels[keep])]
    face_kept = np.zeros(faces.shape[0], dtype=bool)
    face_kept[at] = True
    vertex_kept = np.zeros(v, dtype=bool)
    vertex_kept[faces[at].reshape(-1)] = True
    renumber = np.cumsum(vertex_kept) - 1
    info = dict(face_kept=face_kept, vertex_kept=vertex_kept, removed_nonmanifold_faces=removed_nm,
                nonmanifold_edges=nm_edges, components=labels, sizes=sizes, kept_components=labels[keep])
    return vertices[vertex_kept], renumber[faces[at]].astype(np.int32).reshape(-1, 3), info
