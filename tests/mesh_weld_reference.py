"""The rule of DESIGN.md section 3.9g (include/qf_mesh_weld.h) restated in numpy: vertices at the same place, or within a
tolerance h of one another, become one vertex, transitively.  Three restatements that share nothing but the numbering:
``weld_brute`` (the O(V^2) link matrix, h > 0, small V), ``weld_cells`` (the same links found through the search cells,
h > 0, larger V) and ``weld_exact`` (h == 0: ``np.unique`` on the canonicalised rows).  ``weld`` picks one.  The step
numbers are the header's.  Also the builders the tests share."""
import numpy as np

COUNT_NAMES = ("vertices", "merged_classes", "largest_class", "collapsed_faces", "largest_cell", "loose_vertices",
               "out_of_range_vertices", "invalid_faces")
CELL_LIMIT = 2.0 ** 51


def cell_edge(h):
    """Rule 1's cell edge s for h > 0: 2 max(h, 2^-510), +inf when h * h is not finite."""
    h = np.float64(h)
    with np.errstate(over="ignore"):
        return np.float64(2.0) * max(h, np.float64(2.0 ** -510)) if np.isfinite(h * h) else np.float64(np.inf)


def _inputs(vertices, faces, h):
    v = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.zeros((0, 3), np.int64) if faces is None else np.ascontiguousarray(faces, dtype=np.int64).reshape(-1, 3)
    h = np.float64(h)
    if not (np.isfinite(h) and h >= 0):
        raise ValueError(f"tolerance must be finite and >= 0, got {h}")
    return v, f, h


def cells(v, h):
    """``(cell fp64 [V,3], in_range bool [V])`` of rule 1 for h > 0; the rows of loose vertices mean nothing."""
    with np.errstate(all="ignore"):
        c = np.floor(v / cell_edge(h)) + 0.0                    # -0.0 (a negative x over +inf) is cell 0
        return c, (np.abs(c) < CELL_LIMIT).all(axis=1)          # a c that is not finite fails the comparison too


def linked(a, b, h):
    """Rule 2 for h > 0 between the rows of a [n,3] and b [m,3]: bool [n,m].  Every operation is one fp64 numpy
    operation, rounded on its own."""
    with np.errstate(all="ignore"):
        dx = a[:, None, 0] - b[None, :, 0]
        dy = a[:, None, 1] - b[None, :, 1]
        dz = a[:, None, 2] - b[None, :, 2]
        return ((dx * dx + dy * dy) + dz * dz) <= h * h


def _roots(n, a, b):
    """The lowest node of every connected component of the graph on n nodes with arcs (a[i], b[i])."""
    lab = np.arange(n, dtype=np.int64)
    while True:
        new = lab.copy()
        m = np.minimum(lab[a], lab[b])
        np.minimum.at(new, a, m)
        np.minimum.at(new, b, m)
        new = new[new]
        if np.array_equal(new, lab):
            return lab
        lab = new


def _refusal(v, f, h):
    """Rule 1: ``(finite bool [V], counts)``; counts is None unless the mesh is refused."""
    finite = np.isfinite(v).all(axis=1)
    counts = np.zeros(8, dtype=np.int64)
    counts[7] = int(((f < 0) | (f >= v.shape[0])).any(axis=1).sum())
    if h > 0:
        counts[6] = int((finite & ~cells(v, h)[1]).sum())
    return finite, (counts if counts[6] or counts[7] else None)


def _finish(v, f, h, finite, lab):
    """Rules 4 to 6 from the root of every vertex."""
    n_v = v.shape[0]
    root = lab == np.arange(n_v)
    vertex_map = np.flatnonzero(root).astype(np.int64)
    vertex_class = (np.cumsum(root) - 1)[lab].astype(np.int64)
    out_f = vertex_class[f]
    sizes = np.bincount(lab, minlength=n_v)
    before = (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 2] == f[:, 0])
    after = (out_f[:, 0] == out_f[:, 1]) | (out_f[:, 1] == out_f[:, 2]) | (out_f[:, 2] == out_f[:, 0])
    counts = np.zeros(8, dtype=np.int64)
    counts[0], counts[1], counts[2] = vertex_map.shape[0], int((sizes >= 2).sum()), int(sizes.max())
    counts[3] = int((~before & after).sum())
    if h > 0 and finite.any():
        counts[4] = int(np.unique(cells(v, h)[0][finite], axis=0, return_counts=True)[1].max())
    counts[5] = int((~finite).sum())
    return v[vertex_map], out_f, vertex_map, vertex_class, counts


def weld_brute(vertices, faces, h):
    """h > 0 by the full link matrix: ``(out_vertices, out_faces, vertex_map, vertex_class, counts)``; the arrays are None
    when the mesh is refused."""
    v, f, h = _inputs(vertices, faces, h)
    assert h > 0
    finite, refused = _refusal(v, f, h)
    if refused is not None:
        return None, None, None, None, refused
    link = linked(v, v, h) & finite[:, None] & finite[None, :]
    assert np.array_equal(link, link.T)
    a, b = np.nonzero(np.triu(link, 1))
    return _finish(v, f, h, finite, _roots(v.shape[0], a, b))


_HALF = [(x, y, z) for z in (-1, 0, 1) for y in (-1, 0, 1) for x in (-1, 0, 1) if (z, y, x) > (0, 0, 0)]   # 13 of the 26


def weld_cells(vertices, faces, h):
    """h > 0 with the links looked for only between a cell and the 27 around it."""
    v, f, h = _inputs(vertices, faces, h)
    assert h > 0
    finite, refused = _refusal(v, f, h)
    if refused is not None:
        return None, None, None, None, refused
    idx = np.flatnonzero(finite)
    c = cells(v, h)[0][idx].astype(np.int64)
    members = {}
    if idx.shape[0]:
        uniq, inverse = np.unique(c, axis=0, return_inverse=True)
        order = np.argsort(inverse.reshape(-1), kind="stable")
        bounds = np.searchsorted(inverse.reshape(-1)[order], np.arange(uniq.shape[0] + 1))
        members = {tuple(uniq[i]): idx[order[bounds[i]:bounds[i + 1]]] for i in range(uniq.shape[0])}
    arcs_a, arcs_b = [], []
    for key, mine in members.items():
        a, b = np.nonzero(np.triu(linked(v[mine], v[mine], h), 1))
        arcs_a.append(mine[a])
        arcs_b.append(mine[b])
        for off in _HALF:
            other = members.get((key[0] + off[0], key[1] + off[1], key[2] + off[2]))
            if other is not None:
                a, b = np.nonzero(linked(v[mine], v[other], h))
                arcs_a.append(mine[a])
                arcs_b.append(other[b])
    a = np.concatenate(arcs_a) if arcs_a else np.zeros(0, np.int64)
    b = np.concatenate(arcs_b) if arcs_b else np.zeros(0, np.int64)
    return _finish(v, f, h, finite, _roots(v.shape[0], a, b))


def canonical_bits(v):
    """The coordinates as 64-bit words with -0.0 made +0.0: two finite values compare equal iff these words do."""
    bits = np.ascontiguousarray(v, dtype=np.float64).view(np.int64).copy()
    bits[bits == np.int64(-2 ** 63)] = 0
    return bits


def weld_exact(vertices, faces):
    """h == 0: the classes are the distinct canonicalised rows, the first occurrence is the root."""
    v, f, h = _inputs(vertices, faces, 0.0)
    finite, refused = _refusal(v, f, h)
    if refused is not None:
        return None, None, None, None, refused
    lab = np.arange(v.shape[0], dtype=np.int64)
    idx = np.flatnonzero(finite)
    if idx.shape[0]:
        _, first, inverse = np.unique(canonical_bits(v[idx]), axis=0, return_index=True, return_inverse=True)
        lab[idx] = idx[first[inverse.reshape(-1)]]
    return _finish(v, f, h, finite, lab)


def weld(vertices, faces, h, brute_below=600):
    if np.float64(h) == 0:
        return weld_exact(vertices, faces)
    n = np.asarray(vertices).reshape(-1, 3).shape[0]
    return weld_brute(vertices, faces, h) if n < brute_below else weld_cells(vertices, faces, h)


# ---- builders ----------------------------------------------------------------------------------------------------------
def soup(vertices, faces):
    """The unwelded mesh: one vertex per corner, ``faces = arange(3F).reshape(-1, 3)``."""
    v = np.ascontiguousarray(np.asarray(vertices, np.float64)[np.asarray(faces)].reshape(-1, 3))
    return v, np.arange(v.shape[0], dtype=np.int64).reshape(-1, 3)


def lattice_cloud(n, seed, step=1.0):
    """n points drawn with a seed from the 8 x 8 x 8 lattice of the given step (centred, so both signs occur)."""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 8, (n, 3)).astype(np.float64) - 4.0) * step


def chain(n, spacing):
    """n points along the diagonal, `spacing` apart (in distance, up to rounding)."""
    t = np.arange(n, dtype=np.float64) * (spacing / np.sqrt(3.0))
    return np.stack([t, t, t], axis=1) - t[n // 2]


def copies_and_distinct(n):
    """n copies of one point interleaved with n distinct ones inside the unit cell around it."""
    v = np.empty((2 * n, 3), dtype=np.float64)
    v[0::2] = (0.25, 0.5, 0.75)
    t = np.arange(n, dtype=np.float64)
    v[1::2] = np.stack([0.001 + t / (2.0 * n), 0.002 + ((7 * t) % n) / (2.0 * n), 0.003 + ((13 * t) % n) / (2.0 * n)], axis=1)
    return v


def repeated_sphere(level, seed, h):
    """Every vertex of the icosphere repeated 1 to 4 times with jitter below h / 4 per axis, shuffled; ``(vertices,
    source vertex of every row)``."""
    from tests import mesh_decimate_reference as ref
    v, _ = ref.icosphere(level)
    rng = np.random.default_rng(seed)
    src = np.repeat(np.arange(v.shape[0]), rng.integers(1, 5, v.shape[0]))
    src = src[rng.permutation(src.shape[0])]
    return v[src] + rng.uniform(-h / 4, h / 4, (src.shape[0], 3)) * 0.999, src
