"""numpy restatement of the marching-cubes rules of DESIGN.md section 3.8 (csrc/marching_cubes.hip).

Numbering: corner c = d0 | d1 << 1 | d2 << 2 (d_axis = the corner's offset along that axis); local edge 4 * axis + m,
where m holds the lower corner's offsets along the two other axes, the smaller axis in bit 0.

The polygons of a cell depend only on its 8 inside bits and on the decider of its ambiguous faces, so they are built
per distinct (bits, decider) key by ``cell_polygons`` and assembled over the volume with numpy.
"""
import numpy as np

_OTHER = {0: (1, 2), 1: (0, 2), 2: (0, 1)}


def face_corners():
    """[6][4]: the corners of face (axis a, side s), index 2a + s, counter-clockwise seen from outside the cell.
    With (b, c) = (a+1, a+2) mod 3, the high side walks (b, c) offsets (0,0) (1,0) (1,1) (0,1), the low side the
    reverse (0,0) (0,1) (1,1) (1,0)."""
    out = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        for s in (0, 1):
            walk = [(0, 0), (0, 1), (1, 1), (1, 0)] if s == 0 else [(0, 0), (1, 0), (1, 1), (0, 1)]
            out.append([(s << a) | (ob << b) | (oc << c) for ob, oc in walk])
    return out


FACE_CORNERS = face_corners()


def edge_of_corners(c0, c1):
    d, lo = c0 ^ c1, c0 & c1
    ax = {1: 0, 2: 1, 4: 2}[d]
    o1, o2 = _OTHER[ax]
    return 4 * ax + (((lo >> o1) & 1) | (((lo >> o2) & 1) << 1))


def edge_lower_corner(e):
    ax, m = e >> 2, e & 3
    o1, o2 = _OTHER[ax]
    return ((m & 1) << o1) | ((m >> 1) << o2)


def cell_loops(bits, join):
    """Directed loops of a cell: bits = the 8 inside bits, join[f] = the decider of face f (used only where the face
    is ambiguous).  Returns the loops as lists of local edges, each starting at its smallest edge, in order of it."""
    inside = [(bits >> c) & 1 for c in range(8)]
    nxt = {}
    for f, q in enumerate(FACE_CORNERS):
        s = [inside[c] for c in q]
        E = [edge_of_corners(q[k], q[(k + 1) % 4]) for k in range(4)]
        if sum(s) in (0, 4):
            continue
        if s[0] == s[2] and s[1] == s[3]:                  # four crossings
            for k in range(4):
                if s[k] and not join[f]:
                    nxt[E[(k - 1) % 4]] = E[k]             # cut the inside corner off
                if not s[k] and join[f]:
                    nxt[E[k]] = E[(k - 1) % 4]             # cut the outside corner off
        else:                                              # entry (out -> in) to exit (in -> out), walking the face
            entry = [E[k] for k in range(4) if not s[k] and s[(k + 1) % 4]]
            exit_ = [E[k] for k in range(4) if s[k] and not s[(k + 1) % 4]]
            nxt[entry[0]] = exit_[0]
    loops, seen = [], set()
    for e in sorted(nxt):
        if e in seen:
            continue
        loop, v = [], e
        while v not in seen:
            seen.add(v)
            loop.append(v)
            v = nxt[v]
        assert v == e, "segments do not close"
        loops.append(loop)
    return loops


def cell_triangles(bits, join):
    """Fan triangulation of every loop from its smallest local edge: [(e0, e1, e2), ...] in emission order."""
    return [(lp[0], lp[i], lp[i + 1]) for lp in cell_loops(bits, join) for i in range(1, len(lp) - 1)]


def _edge_land(alo, ahi, g):
    """Per edge: status 0 none / 1 edge vertex / 2 on the lower point / 3 on the upper point, and x (fp32)."""
    crossed = (alo > 0) != (ahi > 0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        t = (alo / (alo - ahi)).astype(np.float32)
        x = (g.astype(np.float32) + t).astype(np.float32)
    status = np.where(x == g.astype(np.float32), 2, np.where(x == (g + 1).astype(np.float32), 3, 1))
    return np.where(crossed, status, 0), x


def marching_cubes(volume, level):
    """(verts fp32 [V,3], faces int32 [F,3]) by the rules of DESIGN.md section 3.8."""
    v = np.ascontiguousarray(volume, dtype=np.float32)
    assert v.ndim == 3 and min(v.shape) >= 2
    a = (v - np.float32(level)).astype(np.float32)
    n = np.array(v.shape)
    idx = np.indices(v.shape)                              # [3, n0, n1, n2]

    # per grid point and axis: the edge to +axis (status, x); missing edges at the far side are not crossed
    status = np.zeros((3,) + v.shape, np.int8)
    xs = np.zeros((3,) + v.shape, np.float32)
    for ax in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        st, x = _edge_land(a[tuple(lo)], a[tuple(hi)], idx[ax][tuple(lo)])
        status[ax][tuple(lo)] = st
        xs[ax][tuple(lo)] = x
    corner = np.zeros(v.shape, bool)
    for ax in range(3):
        corner |= status[ax] == 2
        up = np.zeros(v.shape, bool)
        sl_dst = [slice(None)] * 3
        sl_src = [slice(None)] * 3
        sl_dst[ax], sl_src[ax] = slice(1, None), slice(0, -1)
        up[tuple(sl_dst)] = status[ax][tuple(sl_src)] == 3
        corner |= up
    slots = np.stack([corner] + [status[ax] == 1 for ax in range(3)], -1)   # [n0, n1, n2, 4]
    counts = slots.sum(-1).reshape(-1)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)  # C order of grid points
    slot_id = first[:, None] + np.cumsum(slots.reshape(-1, 4), 1) - slots.reshape(-1, 4)

    # vertices
    pts = np.repeat(np.arange(counts.size), counts)
    which = slots.reshape(-1, 4).nonzero()[1]
    coord = np.stack([idx[k].reshape(-1) for k in range(3)], 1).astype(np.float32)
    verts = coord[pts].copy()
    for ax in range(3):
        m = which == ax + 1
        verts[m, ax] = xs[ax].reshape(-1)[pts[m]]

    # the vertex id each (point, axis) edge resolves to
    lin = np.arange(counts.size).reshape(v.shape)
    edge_vid = np.full((3, counts.size), -1, np.int64)
    for ax in range(3):
        st = status[ax].reshape(-1)
        up = lin + (n[1] * n[2], n[2], 1)[ax]
        edge_vid[ax] = np.where(st == 1, slot_id[:, ax + 1], np.where(st == 2, first, -1))
        m = st == 3
        edge_vid[ax][m] = first[up.reshape(-1)[m]]

    # cells: inside bits and face deciders
    c0 = a[:-1, :-1, :-1]
    corner_vals = []
    for c in range(8):
        d = [(c >> k) & 1 for k in range(3)]
        corner_vals.append(a[d[0]:d[0] + n[0] - 1, d[1]:d[1] + n[1] - 1, d[2]:d[2] + n[2] - 1].reshape(-1))
    cv = np.stack(corner_vals, 1)                          # [cells, 8]
    bits = ((cv > 0).astype(np.int64) << np.arange(8)).sum(1)
    key = bits.copy()
    for f, q in enumerate(FACE_CORNERS):
        cq = cv[:, q].astype(np.float64)
        ins = cq > 0
        # inside diagonal (q0, q2) or (q1, q3); the decider is only read where the face is ambiguous
        d02 = cq[:, 0] * cq[:, 2] - cq[:, 1] * cq[:, 3]
        join = np.where(ins[:, 0], d02 > 0, -d02 > 0)
        amb = (ins[:, 0] == ins[:, 2]) & (ins[:, 1] == ins[:, 3]) & (ins[:, 0] != ins[:, 1])
        key |= (join & amb).astype(np.int64) << (8 + f)
    del c0
    uniq, inv = np.unique(key, return_inverse=True)
    tris = [np.array(cell_triangles(int(k) & 255, [(int(k) >> (8 + f)) & 1 for f in range(6)]), np.int64).reshape(-1, 3)
            for k in uniq]
    nf = np.array([len(t) for t in tris])[inv]
    if nf.sum() == 0:
        return verts, np.zeros((0, 3), np.int32)
    cell = np.repeat(np.arange(bits.size), nf)
    start = np.concatenate([[0], np.cumsum(nf)[:-1]])
    local = np.arange(nf.sum()) - np.repeat(start, nf)
    offs = np.concatenate([[0], np.cumsum([len(t) for t in tris])])
    allt = np.concatenate(tris)
    le = allt[offs[inv[cell]] + local]                     # [F, 3] local edges
    ci = np.stack(np.unravel_index(cell, tuple(n - 1)), 1)
    faces = np.empty(le.shape, np.int64)
    for j in range(3):
        e = le[:, j]
        lc = np.array([edge_lower_corner(k) for k in range(12)])[e]
        g = ci + np.stack([(lc >> k) & 1 for k in range(3)], 1)
        gl = (g[:, 0] * n[1] + g[:, 1]) * n[2] + g[:, 2]
        faces[:, j] = edge_vid[e >> 2, gl]
    assert (faces >= 0).all()
    return verts, faces.astype(np.int32)


def euler_characteristic(verts, faces):
    """V - E + F of the mesh (edges undirected)."""
    e = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), 1)
    return len(np.unique(faces)) - len(np.unique(e, axis=0)) + len(faces)


def signed_volume(verts, faces):
    t = verts.astype(np.float64)[faces]
    return np.einsum("ij,ij->i", t[:, 0], np.cross(t[:, 1], t[:, 2])).sum() / 6.0
