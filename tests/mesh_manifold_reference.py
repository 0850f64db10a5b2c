"""The rule of DESIGN.md section 3.9e (include/qf_mesh_manifold.h) restated in numpy: a mesh is cut along its edges with
three or more faces and every vertex is split into one copy per fan.  Vectorised, so that a few hundred thousand faces
take seconds; the step numbers are the header's.  Also the builders the tests share."""
import numpy as np

from tests import mesh_decimate_open_reference as oref
from tests import mesh_decimate_reference as ref

COUNT_NAMES = ("vertices", "split_vertices", "complex_edges", "complex_faces", "boundary_edges", "same_direction_edges",
               "degenerate_faces", "invalid_faces")


def proper(f):
    return (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])


def edges(faces, n_vertices):
    """Stage A of section 3.9c, vectorised: ``(edges int64 [E,2], face_edges int64 [F,3])``, the edges numbered in the
    order of their lowest half-edge, -1 on degenerate faces.  The faces must be valid."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    face_edges = np.full(f.shape, -1, dtype=np.int64)
    ok = proper(f)
    a, b = f[ok], np.roll(f[ok], -1, axis=1)
    key = (np.minimum(a, b) * np.int64(n_vertices) + np.maximum(a, b)).reshape(-1)
    uniq, first, inverse = np.unique(key, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")                     # ids by first appearance
    rank = np.empty_like(order)
    rank[order] = np.arange(order.shape[0])
    face_edges[ok] = rank[inverse.reshape(-1)].reshape(-1, 3)
    uniq = uniq[order]
    return np.stack([uniq // n_vertices, uniq % n_vertices], axis=1).reshape(-1, 2), face_edges


def _roots(n, a, b):
    """The lowest node of every connected component of the graph on n nodes with arcs (a[i], b[i])."""
    lab = np.arange(n, dtype=np.int64)
    while True:
        m = np.minimum(lab[a], lab[b])
        np.minimum.at(lab, a, m)
        np.minimum.at(lab, b, m)
        nxt = lab[lab]
        if np.array_equal(nxt[a], nxt[b]) and np.array_equal(nxt, lab):
            return lab
        lab = nxt


def cut(vertices, faces, face_edges=None, n_edges=None):
    """``(out_vertices fp64 [V',3], out_faces int64 [F,3], vertex_map int64 [V'], counts int64 [8])``.  ``face_edges`` and
    ``n_edges`` default to stage A's for these faces.  With an invalid face the arrays are None and only counts[7] is
    set."""
    v = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.ascontiguousarray(faces, dtype=np.int64).reshape(-1, 3)
    n_v, n_f = v.shape[0], f.shape[0]
    counts = np.zeros(8, dtype=np.int64)
    bad_index = ((f < 0) | (f >= n_v)).any(axis=1)
    ok = np.zeros(n_f, dtype=bool)
    ok[~bad_index] = proper(f[~bad_index])                      # 2. proper faces
    if face_edges is None:
        if bad_index.any():
            counts[7] = int(bad_index.sum())
            return None, None, None, counts
        n_edges = edges(f, n_v)[0].shape[0]
        face_edges = edges(f, n_v)[1]
    fe = np.asarray(face_edges, dtype=np.int64).reshape(-1, 3)
    invalid = bad_index | (ok & ((fe < 0) | (fe >= n_edges)).any(axis=1))      # 1. validity
    if invalid.any():
        counts[7] = int(invalid.sum())
        return None, None, None, counts
    corner_vertex = f.reshape(-1)
    corner_ok = np.repeat(ok, 3)
    half = np.nonzero(corner_ok)[0]                              # the half-edges of proper faces, ascending
    e_of = fe.reshape(-1)[half]
    uses = np.bincount(e_of, minlength=n_edges)                  # 3. uses
    by_edge = half[np.argsort(e_of, kind="stable")]              # half-edges grouped by edge, ascending inside a group
    start = np.cumsum(uses) - uses
    pair = np.nonzero(uses == 2)[0]
    h0, h1 = by_edge[start[pair]], by_edge[start[pair] + 1]      # 4. the pair of every edge with two uses

    def nxt(h):
        return 3 * (h // 3) + (h % 3 + 1) % 3

    a0, a1, b0, b1 = h0, nxt(h0), h1, nxt(h1)
    same = (corner_vertex[a0] == corner_vertex[b0]) & (corner_vertex[a1] == corner_vertex[b1])
    opposite = (corner_vertex[a0] == corner_vertex[b1]) & (corner_vertex[a1] == corner_vertex[b0])
    link_a = np.concatenate([a0[same], a1[same], a0[opposite], a1[opposite]])
    link_b = np.concatenate([b0[same], b1[same], b1[opposite], b0[opposite]])
    assert (corner_vertex[link_a] == corner_vertex[link_b]).all()
    root = _roots(3 * n_f, link_a, link_b)                       # 5. classes, named by their lowest corner
    corner = np.arange(3 * n_f)
    is_root = corner_ok & (root == corner)
    vmin = np.full(n_v, 3 * n_f, dtype=np.int64)                 # 6. the lowest class of every vertex keeps its index
    np.minimum.at(vmin, corner_vertex[is_root], corner[is_root])
    extra = is_root & (corner != vmin[corner_vertex])
    rank = np.cumsum(extra) - extra
    index = np.where(corner_ok & (root != vmin[corner_vertex]), n_v + rank[root], corner_vertex)
    vertex_map = np.concatenate([np.arange(n_v, dtype=np.int64), corner_vertex[extra]])      # 7. output
    out_v = np.ascontiguousarray(v.view(np.uint64)[vertex_map]).view(np.float64)
    counts[:] = (vertex_map.shape[0], np.unique(corner_vertex[extra]).shape[0], int((uses > 2).sum()),
                 int((ok & (uses[np.where(ok[:, None], fe, 0)] > 2).any(axis=1)).sum()) if n_edges else 0,
                 int((uses == 1).sum()), int(same.sum()), int((~ok).sum()), 0)
    return out_v, index.reshape(n_f, 3).astype(np.int64), vertex_map, counts


def edge_uses(f, n_v):
    """The uses of every edge of the proper faces of f."""
    e, fe = edges(f, n_v)
    return np.bincount(fe[fe >= 0], minlength=e.shape[0]), e


def complex_vertices(v, f):
    """The number of used vertices that ``oref.vertex_classes`` locks as complex (section 3.9d, step 2 in collapse mode)."""
    f = f[proper(f)]
    uses, e = edge_uses(f, v.shape[0])
    cls, _ = oref.vertex_classes(v.shape[0], e, uses, np.zeros(v.shape[0], np.uint8))
    used = np.zeros(v.shape[0], dtype=bool)
    used[f.reshape(-1)] = True
    return int((used & (cls == oref.LOCKED)).sum())


# ---- builders ------------------------------------------------------------------------------------------------------------

def masked(v, f, seed):
    """The mesh under a seeded independent 50 % face mask, unreferenced vertices dropped."""
    keep = np.random.default_rng(seed).random(f.shape[0]) < 0.5
    return oref._drop_unreferenced(v, f[keep])


def book(pages):
    """``pages`` triangles on the spine (0, 1), wound alternately: 2 + pages vertices."""
    ang = 2.0 * np.pi * np.arange(pages) / pages
    v = np.concatenate([[(0.0, 0.0, 0.0), (0.0, 0.0, 1.0)], np.stack([np.cos(ang), np.sin(ang), 0.5 + 0 * ang], axis=1)])
    f = [(0, 1, 2 + p) if p % 2 == 0 else (1, 0, 2 + p) for p in range(pages)]
    return v, np.array(f, dtype=np.int64)


def two_tetrahedra():
    """Two tetrahedra that share the edge (0, 1) and nothing else: 6 vertices, 8 faces, closed."""
    tv, tf = ref.tetrahedron()
    v = np.concatenate([tv, tv[0] + tv[1] - tv[2:]])
    return v, np.concatenate([tf, np.array([0, 1, 4, 5])[tf]])


def same_direction_pair():
    v = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, -1, 0)], dtype=np.float64)
    return v, np.array([(0, 1, 2), (0, 1, 3)], dtype=np.int64)


def degenerate_beside_bowtie():
    v = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (-1, 0, 0), (-1, -1, 0), (0, 2, 0)], dtype=np.float64)
    return v, np.array([(0, 1, 2), (0, 0, 5), (0, 3, 4)], dtype=np.int64)


def unreferenced_vertex():
    v, f = oref.one_triangle()
    return np.concatenate([v, [[5.0, 5.0, 5.0]]]), f


def strip(n_faces, seed=0):
    """Exactly ``n_faces`` faces of a two-row strip under a seeded 50 % mask (so it has bow-ties), every vertex kept."""
    m = 2 * n_faces + 8
    x = np.arange(m + 1, dtype=np.float64)
    v = np.concatenate([np.stack([x, 0 * x, 0 * x], axis=1), np.stack([x, 1 + 0 * x, 0 * x], axis=1)])
    i = np.arange(m)
    f = np.stack([np.stack([i, i + 1, i + m + 2], axis=1), np.stack([i, i + m + 2, i + m + 1], axis=1)], axis=1).reshape(-1, 3)
    keep = np.nonzero(np.random.default_rng(seed).random(f.shape[0]) < 0.5)[0]
    assert keep.shape[0] >= n_faces
    return v, f[keep[:n_faces]].astype(np.int64)


def pinched_fan(n=48):
    """``n`` triangles round the apex 0 with every second one removed: the apex has n / 2 fans."""
    ang = 2.0 * np.pi * np.arange(n) / n
    v = np.concatenate([[(0.0, 0.0, 0.0)], np.stack([np.cos(ang), np.sin(ang), 0 * ang], axis=1)])
    i = np.arange(0, n, 2)
    return v, np.stack([0 * i, 1 + i, 1 + (i + 1) % n], axis=1).astype(np.int64)


def ring(n_faces=2048):
    """A closed band of ``n_faces`` triangles between two circles: manifold, two boundary loops."""
    n = n_faces // 2
    ang = 2.0 * np.pi * np.arange(n) / n
    v = np.concatenate([np.stack([np.cos(ang), np.sin(ang), 0 * ang], axis=1), np.stack([np.cos(ang), np.sin(ang), 1 + 0 * ang], axis=1)])
    i = np.arange(n)
    j = (i + 1) % n
    f = np.stack([np.stack([i, j, i + n], axis=1), np.stack([j, j + n, i + n], axis=1)], axis=1).reshape(-1, 3)
    return v, f.astype(np.int64)
