"""Literal numpy restatement of the vertex-clustering rules of DESIGN.md section 3.9 (``csrc/vertex_clustering.hip``).

Every fp64 operation below is one correctly rounded numpy ufunc on float64 arrays (numpy does not contract a * b + c),
in the expression order the kernel uses.  Sums that the rules order run sequentially: ``np.add.at`` applies its
updates one at a time in index order, and every accumulator starts at +0.0, so a vertex's quadric is
``((0 + p_f1 p_f1^T) + p_f2 p_f2^T) + ...`` over its faces in ascending index and a cell's sums are taken over its
vertices in ascending index -- never numpy's pairwise ``np.sum``.
"""
import numpy as np

TAU = 1e-6
MAX_AXIS_CELLS = 1 << 21
CONTRACTIONS = ("average", "quadric")


class ClusteringError(ValueError):
    pass


def cells(vertices: np.ndarray, s: float):
    """``(lo, idx)``: lo [3] and each vertex's integer cell [V,3]; raises ClusteringError for refused input."""
    v = np.asarray(vertices, np.float64)
    s = float(s)
    if not (np.isfinite(s) and s > 0):
        raise ClusteringError(f"voxel size {s} is not positive and finite")
    bad = int((~np.isfinite(v).all(axis=1)).sum())
    if bad:
        raise ClusteringError(f"{bad} vertices are not finite")
    lo = v.min(axis=0) - 0.5 * s
    need = np.floor((v.max(axis=0) - lo) / s) + 1.0
    if (need > MAX_AXIS_CELLS).any():
        raise ClusteringError(f"{int(need.max())} cells along an axis; at most 2^21")
    idx = np.floor((v - lo) / s).astype(np.int64)
    return lo, idx


def face_planes(vertices: np.ndarray, faces: np.ndarray) -> np.ndarray:
    """[F,4] planes (n, d): n = (b - a) x (c - a) / |.|, d = -(n . a); the zero plane for a zero normal."""
    a, b, c = (vertices[faces[:, k]] for k in range(3))
    u = b - a
    w = c - a
    n0 = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
    n1 = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
    n2 = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
    ln = np.sqrt((n0 * n0 + n1 * n1) + n2 * n2)
    p = np.zeros((len(faces), 4), np.float64)
    ok = ln != 0.0
    m0, m1, m2 = n0[ok] / ln[ok], n1[ok] / ln[ok], n2[ok] / ln[ok]
    p[ok, 0], p[ok, 1], p[ok, 2] = m0, m1, m2
    p[ok, 3] = -((m0 * a[ok, 0] + m1 * a[ok, 1]) + m2 * a[ok, 2])
    return p


def outer10(p: np.ndarray) -> np.ndarray:
    """p p^T's upper triangle, q00 q01 q02 q03 q11 q12 q13 q22 q23 q33."""
    return np.stack([p[:, i] * p[:, j] for i in range(4) for j in range(i, 4)], axis=1)


def solve(Q: np.ndarray, mean: np.ndarray, idx: np.ndarray, lo: np.ndarray, s: float):
    """``(x, accepted, det, thresh)`` per cell: the adjugate solve about the mean, its two acceptance tests."""
    a00, a01, a02, q03, a11, a12, q13, a22, q23 = (Q[:, k] for k in range(9))
    b0, b1, b2 = -q03, -q13, -q23
    m0, m1, m2 = mean[:, 0], mean[:, 1], mean[:, 2]
    r0 = b0 - ((a00 * m0 + a01 * m1) + a02 * m2)
    r1 = b1 - ((a01 * m0 + a11 * m1) + a12 * m2)
    r2 = b2 - ((a02 * m0 + a12 * m1) + a22 * m2)
    c00 = a11 * a22 - a12 * a12
    c01 = a12 * a02 - a01 * a22
    c02 = a01 * a12 - a11 * a02
    c11 = a00 * a22 - a02 * a02
    c12 = a01 * a02 - a00 * a12
    c22 = a00 * a11 - a01 * a01
    det = (a00 * c00 + a01 * c01) + a02 * c02
    t3 = ((a00 + a11) + a22) / 3.0
    thresh = TAU * ((t3 * t3) * t3)
    accept = det > thresh
    with np.errstate(divide="ignore", invalid="ignore"):
        y0 = ((c00 * r0 + c01 * r1) + c02 * r2) / det
        y1 = ((c01 * r0 + c11 * r1) + c12 * r2) / det
        y2 = ((c02 * r0 + c12 * r1) + c22 * r2) / det
        z = np.stack([m0 + y0, m1 + y1, m2 + y2], axis=1)
        fi = idx.astype(np.float64)
        box_lo = lo + (fi - 0.5) * s
        box_hi = lo + (fi + 1.5) * s
        inside = ((z >= box_lo) & (z <= box_hi)).all(axis=1)
    accept = accept & inside
    x = np.where(accept[:, None], z, mean)
    return x, accept, det, thresh


def simplify(vertices, faces, s, contraction="quadric", details=False):
    """``(vertices [C,3] fp64, faces [F',3] int64)`` under the rules; with ``details`` also a dict of the per-cell
    ``accepted``, ``det``, ``thresh``, ``cell`` (integer cell of each output vertex) and ``vertex_cell``."""
    if contraction not in CONTRACTIONS:
        raise ClusteringError(f"unknown contraction {contraction!r}")
    v = np.ascontiguousarray(vertices, np.float64).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int64).reshape(-1, 3)
    n_v = len(v)
    if n_v >= 2 ** 31 or len(f) >= 2 ** 31:
        raise ClusteringError("V and F must be < 2^31")
    bad_f = int(((f < 0) | (f >= n_v)).any(axis=1).sum())
    if bad_f:
        raise ClusteringError(f"{bad_f} faces index outside [0, {n_v})")
    lo, idx = cells(v, s)
    key = (idx[:, 0] << 42) | (idx[:, 1] << 21) | idx[:, 2]

    # cells in order of their smallest vertex index
    _, first, inverse = np.unique(key, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    vcell = rank[inverse.reshape(-1)]
    n_cells = len(order)
    cell_idx = idx[first[order]]

    # average: sequential sum in ascending vertex index, one division
    total = np.zeros((n_cells, 3), np.float64)
    np.add.at(total, vcell, v)
    count = np.bincount(vcell, minlength=n_cells).astype(np.float64)
    mean = total / count[:, None]
    out_v = mean
    info = {"cell": cell_idx, "vertex_cell": vcell}
    if contraction == "quadric":
        pp = outer10(face_planes(v, f)) if len(f) else np.zeros((0, 10))
        # distinct (vertex, face) incidences in ascending face index
        dup = np.zeros(f.shape, bool)
        dup[:, 1] = f[:, 1] == f[:, 0]
        dup[:, 2] = (f[:, 2] == f[:, 0]) | (f[:, 2] == f[:, 1])
        inc_v = f.reshape(-1)[~dup.reshape(-1)]
        inc_f = np.repeat(np.arange(len(f)), 3)[~dup.reshape(-1)]
        Qv = np.zeros((n_v, 10), np.float64)
        np.add.at(Qv, inc_v, pp[inc_f])
        Qc = np.zeros((n_cells, 10), np.float64)
        np.add.at(Qc, vcell, Qv)
        out_v, acc, det, thresh = solve(Qc, mean, cell_idx, lo, float(s))
        info.update(accepted=acc, det=det, thresh=thresh, mean=mean)

    # faces: map, drop, rotate, dedup keeping the first, in order of that first face
    c = vcell[f] if len(f) else np.zeros((0, 3), np.int64)
    keep = (c[:, 0] != c[:, 1]) & (c[:, 1] != c[:, 2]) & (c[:, 0] != c[:, 2])
    c = c[keep]
    src = np.nonzero(keep)[0]
    shift = np.argmin(c, axis=1) if len(c) else np.zeros(0, np.int64)
    rows = np.arange(len(c))
    rot = np.stack([c[rows, shift], c[rows, (shift + 1) % 3], c[rows, (shift + 2) % 3]], axis=1)
    if len(rot):
        _, first_f = np.unique(rot, axis=0, return_index=True)
        first_f = np.sort(first_f)
        out_f = rot[first_f]
    else:
        out_f = np.zeros((0, 3), np.int64)
    info["face_source"] = src[first_f] if len(rot) else np.zeros(0, np.int64)
    out_f = out_f.astype(np.int64)
    if details:
        return out_v, out_f, info
    return out_v, out_f
