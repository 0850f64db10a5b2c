"""numpy restatement of the mesh refinement rules (include/qf_mesh_subdivide.h): the edges of a
mesh numbered by first appearance, and the conforming midpoint split along marked edges.  Written for reading, not speed:
both stages are plain Python loops over the faces."""
import numpy as np

EDGE_COUNT_NAMES = ("edges", "degenerate_faces", "invalid_faces", "boundary_edges")
SPLIT_COUNT_NAMES = ("faces", "vertices", "faces_0_marked", "faces_1_marked", "faces_2_marked", "faces_3_marked",
                     "invalid_faces")


def _faces(faces):
    return np.ascontiguousarray(faces, dtype=np.int64).reshape(-1, 3)


def edges(faces, n_vertices):
    """Stage A: ``(edges int64 [E,2], face_edges int64 [F,3], counts int64 [4])`` in the order of ``EDGE_COUNT_NAMES``.
    With an invalid face the arrays are empty and only counts[2] is set."""
    f = _faces(faces)
    counts = np.zeros(4, dtype=np.int64)
    invalid = ((f < 0) | (f >= n_vertices)).any(axis=1)
    if invalid.any():
        counts[2] = int(invalid.sum())
        return np.zeros((0, 2), np.int64), np.zeros((0, 3), np.int64), counts
    ids, uses, out = {}, [], []
    face_edges = np.full(f.shape, -1, dtype=np.int64)
    for i, (a, b, c) in enumerate(f.tolist()):
        if a == b or b == c or a == c:
            counts[1] += 1
            continue
        for k, (x, y) in enumerate(((a, b), (b, c), (c, a))):      # half-edge 3 i + k, in this order: first appearance
            key = (min(x, y), max(x, y))
            if key not in ids:
                ids[key] = len(out)
                out.append(key)
                uses.append(0)
            uses[ids[key]] += 1
            face_edges[i, k] = ids[key]
    counts[0] = len(out)
    counts[3] = sum(1 for u in uses if u == 1)
    return np.array(out, dtype=np.int64).reshape(-1, 2), face_edges, counts


def children(v, m, marked):
    """Rule 3: the children of the face with indices ``v``, midpoint vertices ``m`` (per edge k) and ``marked`` (per edge
    k), as a list of index triples."""
    n = sum(marked)
    if n == 0:
        return [(v[0], v[1], v[2])]
    if n == 1:
        k = marked.index(True)
        u = (v[k], v[(k + 1) % 3], v[(k + 2) % 3])
        return [(u[0], m[k], u[2]), (m[k], u[1], u[2])]
    if n == 2:
        j = marked.index(False)
        u = (v[(j + 1) % 3], v[(j + 2) % 3], v[j])
        a, b = m[(j + 1) % 3], m[(j + 2) % 3]                      # mid(u0, u1), mid(u1, u2)
        if u[0] < u[2]:
            return [(a, u[1], b), (u[0], a, b), (u[0], b, u[2])]
        return [(a, u[1], b), (u[0], a, u[2]), (a, b, u[2])]
    return [(v[0], m[0], m[2]), (m[0], v[1], m[1]), (m[2], m[1], v[2]), (m[0], m[1], m[2])]


def subdivide(vertices, faces, edge_mark=None, edge_list=None, face_edges=None):
    """Stage B: ``(out_vertices fp64 [V',3], out_faces int64 [F',3], face_map int64 [F'], vertex_parents int64 [V',2],
    counts int64 [7])`` in the order of ``SPLIT_COUNT_NAMES``; ``edge_mark`` None marks every edge; ``edge_list`` and
    ``face_edges`` default to stage A's.  With an invalid face the arrays are empty and only counts[6] is set."""
    p = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = _faces(faces)
    n_v = p.shape[0]
    counts = np.zeros(7, dtype=np.int64)
    empty = (np.zeros((0, 3), np.float64), np.zeros((0, 3), np.int64), np.zeros(0, np.int64), np.zeros((0, 2), np.int64))
    if edge_list is None or face_edges is None:
        edge_list, face_edges, c = edges(f, n_v)
        if c[2]:
            counts[6] = c[2]
            return empty + (counts,)
    edge_list, face_edges = np.asarray(edge_list, np.int64).reshape(-1, 2), np.asarray(face_edges, np.int64).reshape(-1, 3)
    n_e = edge_list.shape[0]
    mark = np.ones(n_e, dtype=bool) if edge_mark is None else np.asarray(edge_mark).reshape(-1) != 0
    assert mark.shape[0] == n_e
    degenerate = (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])
    invalid = ((f < 0) | (f >= n_v)).any(axis=1)
    invalid |= ~invalid & ~degenerate & ((face_edges < 0) | (face_edges >= n_e)).any(axis=1)
    if invalid.any():
        counts[6] = int(invalid.sum())
        return empty + (counts,)
    # 1. new vertices: one per marked edge, in edge order
    new_id = n_v + np.cumsum(mark) - mark                          # exclusive scan
    lo, hi = edge_list[mark, 0], edge_list[mark, 1]
    out_v = np.concatenate([p, 0.5 * (p[lo] + p[hi])])
    parents = np.concatenate([np.repeat(np.arange(n_v, dtype=np.int64)[:, None], 2, axis=1),
                              np.stack([lo, hi], axis=1)]).reshape(-1, 2)
    # 2. and 3. children, parents in input order
    out_f, face_map = [], []
    for i, v in enumerate(f.tolist()):
        if degenerate[i]:
            kids = [tuple(v)]
            counts[2] += 1
        else:
            e = face_edges[i]
            marked = [bool(mark[e[k]]) for k in range(3)]
            kids = children(v, [int(new_id[e[k]]) for k in range(3)], marked)
            counts[2 + sum(marked)] += 1
        out_f += kids
        face_map += [i] * len(kids)
    counts[0], counts[1] = len(out_f), out_v.shape[0]
    return (out_v, np.array(out_f, dtype=np.int64).reshape(-1, 3), np.array(face_map, dtype=np.int64), parents, counts)


def directed_edge_balance(faces):
    """Number of directed edges (u, v) whose count differs from that of (v, u): zero on a closed manifold without a
    T-junction."""
    f = _faces(faces)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    fwd, n_fwd = np.unique(d, axis=0, return_counts=True)
    table = {tuple(e): int(n) for e, n in zip(fwd.tolist(), n_fwd.tolist())}
    return sum(1 for (u, v), n in table.items() if table.get((v, u), 0) != n)


def octahedron(levels=0):
    """A closed manifold: the octahedron, uniformly split ``levels`` times."""
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], dtype=np.int64)
    for _ in range(levels):
        v, f = subdivide(v, f)[:2]
    return v, f
