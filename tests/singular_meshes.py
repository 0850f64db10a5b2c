"""Lattice-aligned meshes, rays and cameras (host only, numpy): the inputs on which the decisions of the intersector that
are measure-zero in general position -- u == 0, v == 0, u + v == 1, det == 0, several triangles at one t, zero direction
components, hits exactly min_sep apart -- happen on most rays.  Every lattice coordinate is a small dyadic rational,
exact in fp32; everything is built on the host so that the brute force and the device see the same bits.

``mt_events`` restates ``mt_hit`` (csrc/exact_common.h, oracle/intersect_ref.c) in numpy fp32 in the same operation
order and reports which boundary each accepted hit sits on; with ``strict=True`` every inequality of it is strict.
"""
import functools
from types import SimpleNamespace

import numpy as np

F32 = np.float32


# ------------------------------------------------------------------------------------------------ meshes
def _weld(quads):
    """[Q,4,3] corner coordinates (ccw seen from outside) -> (vertices fp32 [V,3], faces int32 [2Q,3]); the diagonal
    alternates with the quad's parity so that both diagonals occur."""
    pts = quads.reshape(-1, 3)
    uniq, inv = np.unique(pts, axis=0, return_inverse=True)
    q = inv.reshape(-1, 4)
    par = (np.arange(q.shape[0]) & 1).astype(bool)
    a = np.where(par[:, None], q[:, [0, 1, 2]], q[:, [1, 2, 3]])
    b = np.where(par[:, None], q[:, [0, 2, 3]], q[:, [1, 3, 0]])
    faces = np.stack([a, b], axis=1).reshape(-1, 3)
    return uniq.astype(F32), faces.astype(np.int32)


def voxel_ball(n=16, r=6.2):
    """The boundary faces of the voxels whose centre lies within ``r`` cells of the lattice's centre, n^3 lattice scaled
    to [-1, 1]: every coordinate is k * 2 / n.  n = 16, r = 6.2: 1 440 faces, 722 vertices."""
    c = np.arange(n) + 0.5 - n / 2.0
    solid = (c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2) <= r * r
    pad = np.pad(solid, 1)
    quads = []
    for ax in range(3):
        b, cc = (ax + 1) % 3, (ax + 2) % 3
        for side in (0, 1):
            shift = np.roll(pad, -1 if side else 1, axis=ax)
            idx = np.argwhere(pad & ~shift) - 1                       # voxels whose neighbour on that side is empty
            walk = [(0, 0), (1, 0), (1, 1), (0, 1)] if side else [(0, 0), (0, 1), (1, 1), (1, 0)]
            corners = np.zeros((idx.shape[0], 4, 3))
            for k, (ob, oc) in enumerate(walk):
                corners[:, k, ax] = idx[:, ax] + side
                corners[:, k, b] = idx[:, b] + ob
                corners[:, k, cc] = idx[:, cc] + oc
            quads.append(corners)
    quads = np.concatenate(quads) * (2.0 / n) - 1.0
    return _weld(quads)


def stacked_planes(layers=6, cells=8, spacing=2.0 ** -3, z0=None):
    """``layers`` triangulated grids z = z0 + l * spacing over [-1, 1]^2, ``cells`` x ``cells`` quads each (a power of
    two): every leaf box is flat, and an axis ray meets every layer at a lattice depth."""
    if z0 is None:
        z0 = -spacing * (layers // 2)
    g = np.arange(cells + 1) * (2.0 / cells) - 1.0
    quads = []
    for l in range(layers):
        z = z0 + l * spacing
        x0, y0 = np.meshgrid(g[:-1], g[:-1], indexing="ij")
        x1, y1 = np.meshgrid(g[1:], g[1:], indexing="ij")
        q = np.stack([np.stack([x0, y0], -1), np.stack([x1, y0], -1), np.stack([x1, y1], -1), np.stack([x0, y1], -1)], 2)
        q = q.reshape(-1, 4, 2)
        quads.append(np.concatenate([q, np.full(q.shape[:2] + (1,), z)], -1))
    return _weld(np.concatenate(quads))


def fan(n=48):
    """A cone of ``n`` triangles around the apex (0, 0, 1/2) with its rim at z = -1/2, and a flat fan of ``n`` triangles
    around (0, 0, -3/4) under it: two vertices of valence ``n``.  The rim points are rounded to multiples of 1/64; the
    centre takes each of the three corner slots in turn."""
    assert 3 <= n <= 48
    ang = 2.0 * np.pi * np.arange(n) / n
    rim = np.round(np.stack([np.cos(ang), np.sin(ang)], 1) * 64.0) / 64.0
    assert np.unique(rim, axis=0).shape[0] == n
    verts = np.concatenate([[[0.0, 0.0, 0.5]], np.concatenate([rim, np.full((n, 1), -0.5)], 1),
                            [[0.0, 0.0, -0.75]], np.concatenate([rim, np.full((n, 1), -0.75)], 1)])
    faces = []
    for base in (0, n + 1):
        for i in range(n):
            tri = [base, base + 1 + i, base + 1 + (i + 1) % n]
            faces.append(tri[i % 3:] + tri[:i % 3])
    return verts.astype(F32), np.array(faces, dtype=np.int32)


def mc_ball(res=17, radius=5.0):
    """Marching cubes (tests/marching_cubes_reference.py) of the distance from the centre of a res^3 lattice at level
    ``radius``, scaled to [-1, 1].  With an integer radius the lattice points at an integer distance (on the axes and at
    the Pythagorean offsets (3, 4, 0)) lie exactly on the surface: those vertices are lattice points, every other one has
    two lattice coordinates."""
    from tests.marching_cubes_reference import marching_cubes
    assert res <= 24
    c = (res - 1) / 2.0
    g = np.arange(res, dtype=np.float64) - c
    vol = np.sqrt(g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2).astype(F32)
    v, f = marching_cubes(vol, radius)
    used = np.unique(f)
    remap = np.full(v.shape[0], -1, np.int64)
    remap[used] = np.arange(used.size)
    v = (v[used].astype(np.float64) - c) * (1.0 / c)
    return v.astype(F32), remap[f].astype(np.int32)


def with_junk(vertices, faces):
    """The mesh with junk appended -> (vertices, faces, junk): two zero-area faces (two equal corners; three collinear
    corners, through a new vertex at the midpoint of an edge), face 0 again with reversed winding and a vertex no face
    refers to.  ``junk.zero_area``: the ids no ray may ever report; ``junk.twin``: (original, reversed copy) -- both
    faces count, so the copy is hit like any face (on an edge not always together with the original: b and c exchange
    their roles in mt_hit, and with them u and v)."""
    v, f = np.asarray(vertices, F32), np.asarray(faces, np.int32)
    nv, nf = v.shape[0], f.shape[0]
    tri = v.astype(np.float64)[f]
    area = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    a, b, c = f[nf // 2 + int(np.argmax(area[nf // 2:] > 0))]          # (marching cubes has zero-area faces of its own)
    mid = ((v[a].astype(np.float64) + v[b].astype(np.float64)) * 0.5).astype(F32)
    assert np.array_equal(mid.astype(np.float64) * 2.0, v[a].astype(np.float64) + v[b].astype(np.float64))
    v2 = np.concatenate([v, mid[None], np.array([[1.5, -1.25, 1.75]], F32)])
    extra = np.array([[a, a, c], [a, nv, b], [f[0, 0], f[0, 2], f[0, 1]]], np.int32)
    f2 = np.concatenate([f, extra])
    return v2, f2, SimpleNamespace(zero_area=np.array([nf, nf + 1]), twin=(0, nf + 2), unreferenced=nv + 1)


MESHES = {
    "voxel_ball": lambda: voxel_ball(16, 6.2),
    "stacked_planes": lambda: stacked_planes(6, 8, 2.0 ** -3),
    "fan": lambda: fan(48),
    "mc_ball": lambda: mc_ball(17, 5.0),
}
PITCH = {"voxel_ball": 1.0 / 8, "stacked_planes": 1.0 / 4, "fan": 1.0 / 8, "mc_ball": 1.0 / 8}
PLANE_SPACING = 2.0 ** -3


@functools.lru_cache(maxsize=None)
def mesh(name, junk=False):
    """(vertices fp32, faces int32, junk record or None), read-only and shared."""
    v, f = MESHES[name]()
    j = None
    if junk:
        v, f, j = with_junk(v, f)
    v, f = np.ascontiguousarray(v, F32), np.ascontiguousarray(f, np.int32)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f, j


# ------------------------------------------------------------------------------------------------ rays
AXES = [(ax, sgn) for ax in range(3) for sgn in (1.0, -1.0)]


def _grid(pitch, extent=1.0):
    n = int(round(extent / pitch))
    return np.arange(-n, n + 1) * pitch


def axis_rays(pitch, signed_zero=True):
    """The six axis directions from the lattice and half-lattice points (``pitch / 2`` apart) of the planes at +-2; the
    zero components alternate between +0.0 and -0.0."""
    g = _grid(pitch / 2.0)
    o_all, d_all = [], []
    for ax, sgn in AXES:
        b, c = (ax + 1) % 3, (ax + 2) % 3
        gb, gc = np.meshgrid(g, g, indexing="ij")
        o = np.zeros((gb.size, 3))
        o[:, ax], o[:, b], o[:, c] = -2.0 * sgn, gb.reshape(-1), gc.reshape(-1)
        d = np.zeros((gb.size, 3), F32)
        d[:, ax] = sgn
        if signed_zero:
            flip = (np.arange(gb.size) & 1).astype(bool)
            d[flip, b] = -0.0
            d[~flip, c] = -0.0
        o_all.append(o)
        d_all.append(d)
    return np.concatenate(o_all).astype(F32), np.concatenate(d_all).astype(F32)


def diagonal_rays(pitch):
    """Face diagonals (+-1, +-1, 0) / sqrt 2 (and the other two planes) from lattice points: both non-zero components are
    the same fp32 number, so the ray stays in a lattice plane x -+ y = const and passes through lattice edges."""
    g = _grid(pitch)
    s = F32(np.sqrt(0.5))
    o_all, d_all = [], []
    for ax in range(3):                                   # the zero component
        b, c = (ax + 1) % 3, (ax + 2) % 3
        for sb, sc in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
            ga, gt = np.meshgrid(g, _grid(pitch, 2.0), indexing="ij")          # along the axis / across the diagonal
            o = np.zeros((ga.size, 3))
            o[:, ax] = ga.reshape(-1)
            o[:, b] = -2.0 * sb + gt.reshape(-1) * sb
            o[:, c] = -2.0 * sc - gt.reshape(-1) * sc
            d = np.zeros((ga.size, 3), F32)
            d[:, b], d[:, c] = sb * s, sc * s
            o_all.append(o)
            d_all.append(d)
    return np.concatenate(o_all).astype(F32), np.concatenate(d_all).astype(F32)


def surface_rays(vertices, faces, n_faces=160):
    """Origins exactly on the surface -- a face's first corner and the midpoint of its first edge, for ``n_faces`` faces
    spread over the mesh -- and at the origin (inside the solid), each with all six axis directions: the contract
    excludes the face the origin lies on (t > 0), and an axis direction in the plane of a face has det == 0 there."""
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces)
    pick = f[np.linspace(0, f.shape[0] - 1, min(n_faces, f.shape[0])).astype(np.int64)]
    pts = np.concatenate([v[pick[:, 0]], (v[pick[:, 0]] + v[pick[:, 1]]) * 0.5, np.zeros((1, 3)),
                          np.full((1, 3), 1.0 / 16)])
    o = np.repeat(pts, 6, axis=0)
    d = np.zeros((6, 3), F32)
    for k, (ax, sgn) in enumerate(AXES):
        d[k, ax] = sgn
    return o.astype(F32), np.tile(d, (pts.shape[0], 1)).astype(F32)


def tiny_component_rays(pitch):
    """Axis rays whose two other direction components are 1e-35 (below safe_inv's 1e-30) and 1e-20, with either sign."""
    o, d = axis_rays(pitch, signed_zero=False)
    ax = np.abs(d).argmax(axis=1)
    r = np.arange(d.shape[0])
    d = d.copy()
    d[r, (ax + 1) % 3] = np.where(r & 1, F32(1e-35), F32(-1e-35))
    d[r, (ax + 2) % 3] = np.where(r & 2, F32(1e-20), F32(-1e-20))
    return o, d.astype(F32)


def scaled_rays(pitch):
    """Axis and diagonal rays with the direction scaled by 2 and by 1/2 (exact): t halves / doubles (min_sep = 0 only)."""
    o1, d1 = axis_rays(pitch)
    o2, d2 = diagonal_rays(pitch)
    o, d = np.concatenate([o1[::2], o2[::3]]), np.concatenate([d1[::2], d2[::3]])
    scale = np.where(np.arange(o.shape[0]) & 1, F32(2.0), F32(0.5))[:, None]
    return o, (d * scale).astype(F32)


def zero_rays():
    """The all-zero direction (det == 0 for every face: no hit), from inside and outside, with both signs of zero."""
    o = np.array([[0, 0, 0], [0.5, 0.25, -0.5], [2, 2, 2], [-2, 0, 0]], F32)
    d = np.array([[0.0, 0.0, 0.0], [-0.0, 0.0, -0.0], [0.0, -0.0, 0.0], [-0.0, -0.0, -0.0]], F32)
    return o, d


@functools.lru_cache(maxsize=None)
def rays(mesh_name, family, junk=False):
    """(origins, directions) fp32 of one family on one mesh, read-only and shared."""
    pitch = PITCH[mesh_name]
    if family == "axis":
        o, d = axis_rays(pitch)
    elif family == "diagonal":
        o, d = diagonal_rays(pitch)
    elif family == "surface":
        v, f, _ = mesh(mesh_name, junk)
        o, d = surface_rays(v, f)
    elif family == "tiny":
        o, d = tiny_component_rays(pitch)
    elif family == "scaled":
        o, d = scaled_rays(pitch)
    elif family == "zero":
        o, d = zero_rays()
    else:
        raise KeyError(family)
    o, d = np.ascontiguousarray(o, F32), np.ascontiguousarray(d, F32)
    assert np.isfinite(o).all() and np.isfinite(d).all()
    o.setflags(write=False)
    d.setflags(write=False)
    return o, d


FAMILIES = ["axis", "diagonal", "surface", "tiny", "scaled", "zero"]
#: the boundary events each family exists for (keys of ``mt_events``' counts); "zero" exists for det == 0 alone
FAMILY_EVENTS = {
    "axis": ("u0", "v0", "uv1", "tie"),
    "diagonal": ("u0", "v0", "tie"),
    "surface": ("det0", "tie"),
    "tiny": ("tie",),
    "scaled": ("u0", "v0", "uv1", "tie"),
    "zero": ("det0",),
}


# ------------------------------------------------------------------------------------------------ cameras
CAM_W, CAM_H = 96, 64
CAM_FOCAL = 64.0
CAM_DIST = 4.0


def axis_cameras(pose="centres", dist=CAM_DIST, focal=CAM_FOCAL):
    """Six c2w [3,4] fp32 with rotation entries exactly 0 / +-1, looking at the origin along each axis and sign from
    ``dist`` (a power of two) away.  A lattice vertex k / 8 in the plane through the origin projects to focal * (k / 8) /
    dist = 2 k px from the principal point: ``pose = "corners"`` leaves it there, on a pixel corner; ``"centres"`` moves
    the camera by half a pixel's footprint at that depth (dist / (2 focal) = 1 / 32) along right and up, so that the
    vertex lands on a pixel centre."""
    off = {"corners": 0.0, "centres": 0.5 * dist / focal}[pose]
    out = []
    for ax, sgn in AXES:
        back = np.zeros(3)
        back[ax] = sgn
        up = np.zeros(3)
        up[(ax + 1) % 3] = 1.0
        right = np.cross(up, back)
        pos = back * dist + off * right + off * up
        out.append(np.stack([right, up, back, pos], axis=1).astype(F32))
    return out


# ------------------------------------------------------------------------------------------------ mt_hit, restated
def mt_events(vertices, faces, o, d, strict=False, chunk=256):
    """``mt_hit`` on every (ray, face) pair in numpy fp32, operation by operation -> a record with ``hit`` [R,F] bool,
    ``t`` [R,F] fp32 and the counts: accepted hits with u == 0 (``u0``), v == 0 (``v0``), u + v == 1 (``uv1``), hits whose
    t is bit-equal to another hit's of the same ray (``tie``), and (ray, face) pairs with det == 0 (``det0``).
    ``strict``: every inequality strict (0 < u < 1, v > 0, u + v < 1): what a kernel wrong on the boundary computes."""
    tri = np.asarray(vertices, F32)[np.asarray(faces)]
    a, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    o, d = np.asarray(o, F32), np.asarray(d, F32)
    n_r, n_f = o.shape[0], tri.shape[0]
    hit = np.zeros((n_r, n_f), bool)
    t_out = np.full((n_r, n_f), np.inf, F32)
    counts = dict(u0=0, v0=0, uv1=0, tie=0, det0=0, hits=0)
    with np.errstate(all="ignore"):
        for r0 in range(0, n_r, chunk):
            oo, dd = o[r0:r0 + chunk, None, :], d[r0:r0 + chunk, None, :]
            ox, oy, oz = oo[..., 0], oo[..., 1], oo[..., 2]
            dx, dy, dz = dd[..., 0], dd[..., 1], dd[..., 2]
            e1x, e1y, e1z = e1[None, :, 0], e1[None, :, 1], e1[None, :, 2]
            e2x, e2y, e2z = e2[None, :, 0], e2[None, :, 1], e2[None, :, 2]
            px = dy * e2z - dz * e2y
            py = dz * e2x - dx * e2z
            pz = dx * e2y - dy * e2x
            det = (e1x * px + e1y * py) + e1z * pz
            ok = det != 0
            inv = F32(1.0) / det
            tx, ty, tz = ox - a[None, :, 0], oy - a[None, :, 1], oz - a[None, :, 2]
            u = ((tx * px + ty * py) + tz * pz) * inv
            qx = ty * e1z - tz * e1y
            qy = tz * e1x - tx * e1z
            qz = tx * e1y - ty * e1x
            v = ((dx * qx + dy * qy) + dz * qz) * inv
            t = ((e2x * qx + e2y * qy) + e2z * qz) * inv
            if strict:
                ok = ok & (u > 0) & (u < 1) & (v > 0) & (u + v < 1) & (t > 0)
            else:
                ok = ok & (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1) & (t > 0)
            assert det.dtype == F32 and u.dtype == F32 and t.dtype == F32
            hit[r0:r0 + chunk] = ok
            t_out[r0:r0 + chunk] = np.where(ok, t, np.inf)
            counts["det0"] += int((det == 0).sum())
            counts["u0"] += int((ok & (u == 0)).sum())
            counts["v0"] += int((ok & (v == 0)).sum())
            counts["uv1"] += int((ok & (u + v == 1)).sum())
    ts = np.sort(t_out, axis=1)
    eq = (ts[:, 1:] == ts[:, :-1]) & np.isfinite(ts[:, 1:])
    tied = np.zeros(ts.shape, bool)
    tied[:, 1:] |= eq
    tied[:, :-1] |= eq
    counts["tie"] = int(tied.sum())
    counts["hits"] = int(hit.sum())
    return SimpleNamespace(hit=hit, t=t_out, counts=counts)


def lists_from_events(ev, k):
    """The (tri, t, count) lists of the brute force's shape from ``mt_events`` (min_sep = 0): ascending (t, tri)."""
    n_r, n_f = ev.hit.shape
    order = np.lexsort((np.broadcast_to(np.arange(n_f), ev.t.shape), ev.t), axis=1)[:, :k]
    t = np.take_along_axis(ev.t, order, axis=1)
    tri = np.where(np.isfinite(t), order, -1).astype(np.int32)
    if t.shape[1] < k:
        t = np.pad(t, ((0, 0), (0, k - t.shape[1])), constant_values=np.inf)
        tri = np.pad(tri, ((0, 0), (0, k - tri.shape[1])), constant_values=-1)
    return tri, t.astype(F32), np.minimum(ev.hit.sum(axis=1), k).astype(np.int32)
