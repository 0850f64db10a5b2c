"""numpy restatement of the mesh decimation rules (include/qf_mesh_decimate.h): rounds of
independent quadric edge collapses to a face count, with the same operation order as the device code, so that the two
agree bit for bit.  The arithmetic of a candidate is vectorised over the edges (numpy rounds every product and sum on its
own); legality and selection are plain Python loops.  Small mesh builders for the tests are at the end."""
import numpy as np

from tests import mesh_subdivide_reference as sub

STOP_TARGET, STOP_NO_EDGE, STOP_MAX_ROUNDS = "target reached", "no edge taken", "max_rounds reached"
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
TAU = 1e-6


def face_planes(v, f):
    """Section 3.9's plane per face: unit normal and offset, the zero plane where the cross product has length 0."""
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    u, w = b - a, c - a
    n0 = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
    n1 = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
    n2 = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
    length = np.sqrt((n0 * n0 + n1 * n1) + n2 * n2)
    ok = length != 0.0
    safe = np.where(ok, length, 1.0)
    n0, n1, n2 = (np.where(ok, n / safe, 0.0) for n in (n0, n1, n2))
    d = np.where(ok, -((n0 * a[:, 0] + n1 * a[:, 1]) + n2 * a[:, 2]), 0.0)
    return np.stack([n0, n1, n2, d], axis=1)


def _proper(f):
    return (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])


def vertex_quadrics(v, f):
    """Q fp64 [V,10] (q00 q01 q02 q03 q11 q12 q13 q22 q23 q33): the faces of a vertex summed in ascending face index from
    +0.0.  Faces with two equal indices have the zero plane and are left out."""
    planes = face_planes(v, f)
    q = np.zeros((v.shape[0], 10), dtype=np.float64)
    pairs = ((0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3))
    proper = _proper(f)
    for i in range(f.shape[0]):                    # ascending face index; a vertex appears once in a proper face
        if not proper[i]:
            continue
        p = planes[i]
        outer = np.array([p[r] * p[c] for r, c in pairs])
        for x in f[i]:
            q[x] = q[x] + outer
    return q


def mix(x, rnd):
    """splitmix64's finaliser of x + (round + 1) * golden, on uint64 arrays (wrapping)."""
    with np.errstate(over="ignore"):
        s = x + np.uint64(((rnd + 1) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF)
        s = s ^ (s >> np.uint64(30))
        s = s * np.uint64(0xBF58476D1CE4E5B9)
        s = s ^ (s >> np.uint64(27))
        s = s * np.uint64(0x94D049BB133111EB)
        s = s ^ (s >> np.uint64(31))
    return s


def collapse_points(p, q, a, b):
    """Step 3 for the edges (a[i], b[i]): ``(Qe [n,10], z [n,3], cost [n])``."""
    qe = q[a] + q[b]
    pa, pb = p[a], p[b]
    m = (pa + pb) * 0.5
    a00, a01, a02, a11, a12, a22 = qe[:, 0], qe[:, 1], qe[:, 2], qe[:, 4], qe[:, 5], qe[:, 7]
    b0, b1, b2 = -qe[:, 3], -qe[:, 6], -qe[:, 8]
    m0, m1, m2 = m[:, 0], m[:, 1], m[:, 2]
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
    solve = det > TAU * ((t3 * t3) * t3)
    safe = np.where(solve, det, 1.0)
    y = np.stack([m0 + ((c00 * r0 + c01 * r1) + c02 * r2) / safe,
                  m1 + ((c01 * r0 + c11 * r1) + c12 * r2) / safe,
                  m2 + ((c02 * r0 + c12 * r1) + c22 * r2) / safe], axis=1)
    d = np.abs(pa - pb)
    span = np.maximum(np.maximum(d[:, 0], d[:, 1]), d[:, 2])[:, None]
    inside = ((y >= np.minimum(pa, pb) - span) & (y <= np.maximum(pa, pb) + span)).all(axis=1)
    z = np.where((solve & inside)[:, None], y, m)
    z0, z1, z2 = z[:, 0], z[:, 1], z[:, 2]
    s0 = ((qe[:, 0] * z0 + qe[:, 1] * z1) + qe[:, 2] * z2) + qe[:, 3]
    s1 = ((qe[:, 1] * z0 + qe[:, 4] * z1) + qe[:, 5] * z2) + qe[:, 6]
    s2 = ((qe[:, 2] * z0 + qe[:, 5] * z1) + qe[:, 7] * z2) + qe[:, 8]
    s3 = ((qe[:, 3] * z0 + qe[:, 6] * z1) + qe[:, 8] * z2) + qe[:, 9]
    c = ((s0 * z0 + s1 * z1) + s2 * z2) + s3
    return qe, z, np.where(c > 0.0, c, 0.0)


def _cross(p0, p1, p2):
    u0, u1, u2 = p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]
    w0, w1, w2 = p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]
    return u1 * w2 - u2 * w1, u2 * w0 - u0 * w2, u0 * w1 - u1 * w0


def _keeps_side(p, t, v, z):
    """(L3) for face t, which uses v once: the normals before and after v moves to z have a positive dot product."""
    n = _cross(p[t[0]], p[t[1]], p[t[2]])
    k = _cross(*(z if x == v else p[x] for x in t))
    return (n[0] * k[0] + n[1] * k[1]) + n[2] * k[2] > 0.0


def select_round(p, f, q, lock, target_left, max_cost, rnd):
    """Steps 1 to 7 on the current mesh: ``(edges, taken edge ids in budget order, z of each, Qe of each, counts)`` with
    counts = (candidates, legal, selected, taken).  ``target_left`` is F - target_faces."""
    n_v = p.shape[0]
    edges, face_edges, _ = sub.edges(f, n_v)
    n_e = edges.shape[0]
    uses = np.bincount(face_edges[face_edges >= 0], minlength=n_e)
    locked = lock.astype(bool).copy()
    locked[edges[uses != 2].reshape(-1)] = True
    ea, eb = edges[:, 0], edges[:, 1]
    ids = np.nonzero(~locked[ea] & ~locked[eb])[0]
    qe, z, cost = collapse_points(p, q, ea[ids], eb[ids])
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
        if all(_keeps_side(pl, t, a, zj) for t in fa) and all(_keeps_side(pl, t, b, zj) for t in fb):   # (L3)
            legal[j] = True
    ids, qe, z, cost = ids[legal], qe[legal], z[legal], cost[legal]
    bits = cost.view(np.uint64)
    pair = ea[ids].astype(np.uint64) << np.uint64(32) | eb[ids].astype(np.uint64)
    key = ((bits >> np.uint64(52)) << np.uint64(52)) | ((mix(pair, rnd) & np.uint64(0x1FFFFF)) << np.uint64(31)) \
        | ids.astype(np.uint64)

    m1 = np.full(n_v, NONE, dtype=np.uint64)
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
    max_take = (max(target_left, 0) + 1) // 2                                        # every candidate has two faces
    order = order[:max_take]
    return edges, ids[order], z[order], qe[order], (n_candidates, int(legal.sum()), int(sel.sum()), len(order))


def decimate(vertices, faces, target_faces, max_cost=None, vertex_lock=None, max_rounds=128):
    """``(vertices fp64 [V',3], faces int64 [F',3], face_map int64 [F'], vertex_target int64 [V], stats)``.  stats:
    ``rounds``, the per-round lists ``faces`` (after the round), ``candidates``, ``legal``, ``selected``, ``taken``, and
    ``stop``.  A round that takes no edge leaves the mesh as it was."""
    p = np.array(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.array(faces, dtype=np.int64).reshape(-1, 3)
    n_v0 = p.shape[0]
    lock = np.zeros(n_v0, np.uint8) if vertex_lock is None else (np.asarray(vertex_lock).reshape(-1) != 0).astype(np.uint8)
    max_cost = np.inf if max_cost is None else float(max_cost)
    face_map = np.arange(f.shape[0], dtype=np.int64)
    target = np.arange(n_v0, dtype=np.int64)
    stats = {"rounds": 0, "faces": [], "candidates": [], "legal": [], "selected": [], "taken": [], "stop": None}
    q = None
    while True:
        if f.shape[0] <= target_faces:
            stats["stop"] = STOP_TARGET
            break
        if stats["rounds"] >= max_rounds:
            stats["stop"] = STOP_MAX_ROUNDS
            break
        if q is None:
            q = vertex_quadrics(p, f)
        edges, taken, z, qe, counts = select_round(p, f, q, lock, f.shape[0] - target_faces, max_cost, stats["rounds"])
        stats["rounds"] += 1
        for name, c in zip(("candidates", "legal", "selected", "taken"), counts):
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
        # compaction: degenerate faces, then unreferenced vertices
        keep_f = _proper(f)
        f, face_map = f[keep_f], face_map[keep_f]
        used = np.zeros(p.shape[0], dtype=bool)
        used[f.reshape(-1)] = True
        new_index = np.where(used, np.cumsum(used) - 1, -1)
        p, q, lock, f = p[used], q[used], lock[used], new_index[f]
        target[live] = new_index[target[live]]
        stats["faces"].append(int(f.shape[0]))
    return p, f, face_map, target, stats


# ---- mesh builders ------------------------------------------------------------------------------------------------------

def icosphere(level):
    """A unit icosphere: 20 * 4^level faces, every vertex normalised."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
         (9, 8, 1)]
    v = [np.array(x, dtype=np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        mid, out = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = out
    return np.array(v, dtype=np.float64), np.array(f, dtype=np.int64)


def grid(n):
    """The unit square in the plane z = 0 as n x n vertices and 2 (n - 1)^2 faces, normals along +z."""
    x = np.arange(n, dtype=np.float64) / (n - 1)
    v = np.stack([np.tile(x, n), np.repeat(x, n), np.zeros(n * n)], axis=1)
    f = []
    for j in range(n - 1):
        for i in range(n - 1):
            a = j * n + i
            f += [(a, a + 1, a + n + 1), (a, a + n + 1, a + n)]
    return v, np.array(f, dtype=np.int64)


def tetrahedron():
    v = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)], dtype=np.float64)
    return v, np.array([(0, 2, 1), (0, 1, 3), (0, 3, 2), (1, 2, 3)], dtype=np.int64)


def fan():
    """Three faces on the edge (0, 1): a non-manifold edge."""
    v = np.array([(0, 0, 0), (1, 0, 0), (0.5, 1, 0), (0.5, -0.5, 1), (0.5, -0.5, -1)], dtype=np.float64)
    return v, np.array([(0, 1, 2), (0, 1, 3), (0, 1, 4)], dtype=np.int64)


def padded(n_edges_target, seed=0):
    """A grid strip whose proper faces have about ``n_edges_target`` edges, plus an isolated vertex and a face with two
    equal indices: ``(vertices, faces, edge count)``.  The strip is jittered so that costs are not all zero."""
    n = 3
    while True:
        v, f = grid(n)
        if sub.edges(f, v.shape[0])[2][0] >= n_edges_target:
            break
        n += 1
    n_f = f.shape[0]
    while n_f > 1 and sub.edges(f[:n_f - 1], v.shape[0])[2][0] >= n_edges_target:
        n_f -= 1
    f = f[:n_f]
    rng = np.random.default_rng(seed)
    v = v + rng.uniform(-0.2, 0.2, v.shape) / n
    v = np.concatenate([v, [[2.0, 2.0, 2.0]]])
    f = np.concatenate([f[: n_f // 2], [[0, 0, 1]], f[n_f // 2:]])
    return v, f, int(sub.edges(f, v.shape[0])[2][0])
