"""numpy restatement of decimation with ``boundary="collapse"`` (include/qf_mesh_decimate_open.h):
the rules of tests/mesh_decimate_reference.py extended by boundary quadrics, vertex classes, the three candidate kinds and
the prefix budget, in the device code's operation order, so that the two agree bit for bit.  Builders of small open meshes
are at the end."""
import numpy as np

from tests import mesh_decimate_reference as ref
from tests import mesh_subdivide_reference as sub

STOP_TARGET, STOP_NO_EDGE, STOP_MAX_ROUNDS = ref.STOP_TARGET, ref.STOP_NO_EDGE, ref.STOP_MAX_ROUNDS
INTERIOR, BORDER, LOCKED = 0, 1, 2
PAIRS = ((0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3))


def _uses(face_edges, n_e):
    return np.bincount(face_edges[face_edges >= 0], minlength=n_e)


def boundary_planes(p, f, edges, face_edges, uses):
    """The constraint plane (m, d) of every edge with uses == 1, fp64 [E,4]; the zero row for every other edge, for an
    edge whose face has the zero plane and for one of length 0."""
    planes = ref.face_planes(p, f)
    out = np.zeros((edges.shape[0], 4), dtype=np.float64)
    for i in range(f.shape[0]):
        for k in range(3):
            e = int(face_edges[i, k])
            if e < 0 or uses[e] != 1:
                continue
            n0, n1, n2 = planes[i, 0], planes[i, 1], planes[i, 2]
            if n0 == 0.0 and n1 == 0.0 and n2 == 0.0:
                continue
            pa, pb = p[edges[e, 0]], p[edges[e, 1]]
            d0, d1, d2 = pb[0] - pa[0], pb[1] - pa[1], pb[2] - pa[2]
            m0 = d1 * n2 - d2 * n1
            m1 = d2 * n0 - d0 * n2
            m2 = d0 * n1 - d1 * n0
            length = np.sqrt((m0 * m0 + m1 * m1) + m2 * m2)
            if length == 0.0:
                continue
            m0, m1, m2 = m0 / length, m1 / length, m2 / length
            out[e] = (m0, m1, m2, -((m0 * pa[0] + m1 * pa[1]) + m2 * pa[2]))
    return out


def add_boundary_quadrics(p, f, q, weight):
    """Q[a] and Q[b] of every boundary edge gain ``weight * (pl_r * pl_c)`` per component, a vertex's edges in ascending
    edge index.  Returns the new Q."""
    edges, face_edges, _ = sub.edges(f, p.shape[0])
    uses = _uses(face_edges, edges.shape[0])
    planes = boundary_planes(p, f, edges, face_edges, uses)
    q = q.copy()
    weight = np.float64(weight)
    for e in range(edges.shape[0]):
        pl = planes[e]
        if pl[0] == 0.0 and pl[1] == 0.0 and pl[2] == 0.0:
            continue
        outer = np.array([weight * (pl[r] * pl[c]) for r, c in PAIRS])
        for x in edges[e]:
            q[x] = q[x] + outer
    return q


def vertex_classes(n_v, edges, uses, lock):
    """Step 2: ``(cls uint8 [V], nb int [V])``."""
    nb = np.zeros(n_v, dtype=np.int64)
    bad = np.zeros(n_v, dtype=bool)
    for e in range(edges.shape[0]):
        if uses[e] == 1:
            nb[edges[e]] += 1
        elif uses[e] != 2:
            bad[edges[e]] = True
    cls = np.full(n_v, LOCKED, dtype=np.uint8)
    free = ~lock.astype(bool) & ~bad
    cls[free & (nb == 0)] = INTERIOR
    cls[free & (nb == 2)] = BORDER
    return cls, nb


def cost_at(qe, z):
    z0, z1, z2 = z[:, 0], z[:, 1], z[:, 2]
    s0 = ((qe[:, 0] * z0 + qe[:, 1] * z1) + qe[:, 2] * z2) + qe[:, 3]
    s1 = ((qe[:, 1] * z0 + qe[:, 4] * z1) + qe[:, 5] * z2) + qe[:, 6]
    s2 = ((qe[:, 2] * z0 + qe[:, 5] * z1) + qe[:, 7] * z2) + qe[:, 8]
    s3 = ((qe[:, 3] * z0 + qe[:, 6] * z1) + qe[:, 8] * z2) + qe[:, 9]
    c = ((s0 * z0 + s1 * z1) + s2 * z2) + s3
    return np.where(c > 0.0, c, 0.0)


def select_round(p, f, q, lock, target_left, max_cost, rnd):
    """Steps 1 to 7 in collapse mode: ``(edges, taken edge ids in budget order, z, Qe, counts)`` with counts =
    (candidates, legal, selected, taken, boundary_taken)."""
    n_v = p.shape[0]
    edges, face_edges, _ = sub.edges(f, n_v)
    n_e = edges.shape[0]
    uses = _uses(face_edges, n_e)
    cls, _ = vertex_classes(n_v, edges, uses, lock)
    ea, eb = edges[:, 0], edges[:, 1]
    isolated = np.zeros(n_e, dtype=bool)                       # every edge of a face whose three edges are boundary edges
    for i in range(f.shape[0]):
        fe = face_edges[i]
        if (fe >= 0).all() and (uses[fe] == 1).all():
            isolated[fe] = True
    ca, cb = cls[ea], cls[eb]
    free = (ca != LOCKED) & (cb != LOCKED)
    kind_a = free & (uses == 2) & (ca == INTERIOR) & (cb == INTERIOR)
    kind_b = free & (uses == 2) & (ca != cb)
    kind_c = free & (uses == 1) & ~isolated
    ids = np.nonzero(kind_a | kind_b | kind_c)[0]
    qe, z, cost = ref.collapse_points(p, q, ea[ids], eb[ids])
    pinned = kind_b[ids]
    if pinned.any():
        end = np.where(ca[ids] == BORDER, ea[ids], eb[ids])
        z = np.where(pinned[:, None], p[end], z)
        cost = np.where(pinned, cost_at(qe, z), cost)
    keep = ~(cost > max_cost)
    ids, qe, z, cost = ids[keep], qe[keep], z[keep], cost[keep]
    n_candidates = len(ids)

    nbr = [set() for _ in range(n_v)]
    for a, b in edges.tolist():
        nbr[a].add(b)
        nbr[b].add(a)
    faces_of = [[] for _ in range(n_v)]
    fl = f.tolist()
    for i, t in enumerate(fl):
        if t[0] != t[1] and t[1] != t[2] and t[0] != t[2]:
            for x in t:
                faces_of[x].append(i)
    pl = [tuple(x) for x in p.tolist()]

    legal = np.zeros(n_candidates, dtype=bool)
    for j, e in enumerate(ids.tolist()):
        a, b = int(ea[e]), int(eb[e])
        if len(nbr[a] & nbr[b]) != uses[e]:                                         # (L1)
            continue
        fa = [fl[i] for i in faces_of[a] if b not in fl[i]]
        fb = [fl[i] for i in faces_of[b] if a not in fl[i]]
        pairs_a = {frozenset(x for x in t if x != a) for t in fa}
        if any(frozenset(x for x in t if x != b) in pairs_a for t in fb):            # (L2)
            continue
        zj = tuple(z[j].tolist())
        if all(ref._keeps_side(pl, t, a, zj) for t in fa) and all(ref._keeps_side(pl, t, b, zj) for t in fb):   # (L3)
            legal[j] = True
    ids, qe, z, cost = ids[legal], qe[legal], z[legal], cost[legal]
    bits = cost.view(np.uint64)
    pair = ea[ids].astype(np.uint64) << np.uint64(32) | eb[ids].astype(np.uint64)
    key = ((bits >> np.uint64(52)) << np.uint64(52)) | ((ref.mix(pair, rnd) & np.uint64(0x1FFFFF)) << np.uint64(31)) \
        | ids.astype(np.uint64)

    m1 = np.full(n_v, ref.NONE, dtype=np.uint64)
    np.minimum.at(m1, ea[ids], key)
    np.minimum.at(m1, eb[ids], key)
    m2 = m1.copy()
    for v in range(n_v):
        for x in nbr[v]:
            if m1[x] < m2[v]:
                m2[v] = m1[x]
    sel = (key == m2[ea[ids]]) & (key == m2[eb[ids]])
    ids, qe, z, bits = ids[sel], qe[sel], z[sel], bits[sel]
    order = np.lexsort((ids, bits))                                                  # by (cost_bits, e)
    before = np.cumsum(uses[ids[order]]) - uses[ids[order]]                          # faces removed by the edges in front
    order = order[before < max(target_left, 0)]
    taken = ids[order]
    return edges, taken, z[order], qe[order], (n_candidates, int(legal.sum()), int(sel.sum()), len(order),
                                               int((uses[taken] == 1).sum()))


def decimate(vertices, faces, target_faces, max_cost=None, vertex_lock=None, max_rounds=128, boundary_weight=1.0):
    """``ref.decimate`` with ``boundary="collapse"``; stats gain the per-round list ``boundary_taken``."""
    p = np.array(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.array(faces, dtype=np.int64).reshape(-1, 3)
    n_v0 = p.shape[0]
    lock = np.zeros(n_v0, np.uint8) if vertex_lock is None else (np.asarray(vertex_lock).reshape(-1) != 0).astype(np.uint8)
    max_cost = np.inf if max_cost is None else float(max_cost)
    face_map = np.arange(f.shape[0], dtype=np.int64)
    target = np.arange(n_v0, dtype=np.int64)
    stats = {"rounds": 0, "faces": [], "candidates": [], "legal": [], "selected": [], "taken": [], "boundary_taken": [],
             "stop": None}
    q = None
    while True:
        if f.shape[0] <= target_faces:
            stats["stop"] = STOP_TARGET
            break
        if stats["rounds"] >= max_rounds:
            stats["stop"] = STOP_MAX_ROUNDS
            break
        if q is None:
            q = add_boundary_quadrics(p, f, ref.vertex_quadrics(p, f), boundary_weight)
        edges, taken, z, qe, counts = select_round(p, f, q, lock, f.shape[0] - target_faces, max_cost, stats["rounds"])
        stats["rounds"] += 1
        for name, c in zip(("candidates", "legal", "selected", "taken", "boundary_taken"), counts):
            stats[name].append(int(c))
        if len(taken) == 0:
            stats["faces"].append(int(f.shape[0]))
            stats["stop"] = STOP_NO_EDGE
            break
        remap = np.arange(p.shape[0], dtype=np.int64)
        a, b = edges[taken, 0], edges[taken, 1]
        p[a], q[a], remap[b] = z, qe, a
        f = remap[f]
        live = target >= 0
        target[live] = remap[target[live]]
        keep_f = ref._proper(f)
        f, face_map = f[keep_f], face_map[keep_f]
        used = np.zeros(p.shape[0], dtype=bool)
        used[f.reshape(-1)] = True
        new_index = np.where(used, np.cumsum(used) - 1, -1)
        p, q, lock, f = p[used], q[used], lock[used], new_index[f]
        target[live] = new_index[target[live]]
        stats["faces"].append(int(f.shape[0]))
    return p, f, face_map, target, stats


# ---- mesh builders and measures -------------------------------------------------------------------------------------------

def _drop_unreferenced(v, f):
    used = np.zeros(v.shape[0], dtype=bool)
    used[f.reshape(-1)] = True
    return v[used], (np.cumsum(used) - 1)[f]


def hemisphere(level):
    """The faces of the unit icosphere whose centroid has z > 0, unreferenced vertices dropped."""
    v, f = ref.icosphere(level)
    return _drop_unreferenced(v, f[v[f].mean(axis=1)[:, 2] > 0.0])


def holed(n, lo, hi):
    """``ref.grid(n)`` without the cells (i, j) in [lo, hi)^2, unreferenced vertices dropped."""
    v, f = ref.grid(n)
    cell = np.arange(f.shape[0]) // 2
    i, j = cell % (n - 1), cell // (n - 1)
    return _drop_unreferenced(v, f[~((i >= lo) & (i < hi) & (j >= lo) & (j < hi))])


def bowtie():
    """Two 5 x 5 grids that share one corner vertex: ``(vertices, faces, index of the shared vertex)``."""
    v, f = ref.grid(5)
    g = f + 24                                                   # the second grid's vertex 0 is the first's vertex 24
    return np.concatenate([v, v[1:] + np.array([1.0, 1.0, 0.0])]), np.concatenate([f, g]), 24


def two_triangles():
    v = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)], dtype=np.float64)
    return v, np.array([(0, 1, 2), (0, 2, 3)], dtype=np.int64)


def one_triangle():
    return two_triangles()[0][:3], np.array([(0, 1, 2)], dtype=np.int64)


def topology(v, f):
    """``(V - E + F, boundary loops, components, edge uses, edges)`` of the referenced part of a mesh."""
    f = f[ref._proper(f)]
    edges, face_edges, _ = sub.edges(f, v.shape[0])
    uses = _uses(face_edges, edges.shape[0])
    n_used = len(np.unique(f))

    def components(n, pairs):
        parent = list(range(n))

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x

        for a, b in pairs:
            parent[find(a)] = find(b)
        return parent, find

    _, find = components(v.shape[0], edges.tolist())
    n_comp = len({find(int(x)) for x in np.unique(f)})
    border = edges[uses == 1]
    # loops: boundary edges joined where they share a vertex (a complex vertex joins the loops through it)
    ids = {int(x): k for k, x in enumerate(np.unique(border))}
    _, find_b = components(len(ids), [(ids[int(a)], ids[int(b)]) for a, b in border])
    n_loops = len({find_b(k) for k in range(len(ids))})
    return n_used - edges.shape[0] + f.shape[0], n_loops, n_comp, uses, edges
