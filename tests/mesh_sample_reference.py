"""Numpy restatement of the surface-sampling rule (include/qf_mesh_sample.h).  Every
floating-point operation is one numpy fp64 operation, rounded on its own; the hashes and the scan are uint64 arithmetic
modulo 2^64.  Vectorised over the samples; the device output is compared with this bit for bit."""
import numpy as np

COUNT_NAMES = ("nonfinite_vertices", "invalid_faces", "bad_weights", "nonfinite_measures", "unsampled_faces", "no_measure")

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
TWO32 = 4294967296.0
_U = np.uint64


def fin(x):
    """splitmix64's finaliser on a uint64 array."""
    x = np.asarray(x, dtype=np.uint64).copy()
    x ^= x >> _U(30)
    x *= _U(0xBF58476D1CE4E5B9)
    x ^= x >> _U(27)
    x *= _U(0x94D049BB133111EB)
    x ^= x >> _U(31)
    return x


def hashes(n_samples, seed):
    """h_0, h_1, h_2 of rule 5 for samples 0 .. N-1: uint64 [3, N]."""
    i = np.arange(n_samples, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return np.stack([fin(_U(seed) + (_U(3) * i + _U(k + 1)) * GOLDEN) for k in range(3)])


def measures(vertices, faces, face_weight=None):
    """Rules 1 and 2: (m fp64 [F], counts of rule 1 as a list of four)."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    n_v = v.shape[0]
    nonfinite_v = int((~np.isfinite(v).all(axis=1)).sum())
    invalid = ((f < 0) | (f >= n_v)).any(axis=1)
    bad_w = 0
    if face_weight is not None:
        w = np.asarray(face_weight, dtype=np.float64).reshape(-1)
        assert w.shape[0] == f.shape[0]
        bad_w = int((~(w >= 0.0) | ~np.isfinite(w)).sum())
    degenerate = (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 2] == f[:, 0])
    g = np.where(invalid[:, None], 0, f)
    a, b, c = v[g[:, 0]], v[g[:, 1]], v[g[:, 2]]
    with np.errstate(all="ignore"):
        u, ww = b - a, c - a
        n0 = u[:, 1] * ww[:, 2] - u[:, 2] * ww[:, 1]
        n1 = u[:, 2] * ww[:, 0] - u[:, 0] * ww[:, 2]
        n2 = u[:, 0] * ww[:, 1] - u[:, 1] * ww[:, 0]
        m = np.sqrt((n0 * n0 + n1 * n1) + n2 * n2)
        if face_weight is not None:
            m = m * w
    m = np.where(invalid | degenerate, 0.0, m)
    nonfinite_m = int((~np.isfinite(m) & ~invalid).sum())
    return m, [nonfinite_v, int(invalid.sum()), bad_w, nonfinite_m]


def quantise(m):
    """Rules 3 and 4 on valid measures: (q uint64 [F], S_f uint64 [F]), or (None, None) when the largest is zero."""
    m = np.asarray(m, dtype=np.float64)
    big = m.max()
    if not big > 0.0:
        return None, None
    q = np.floor(m / big * TWO32).astype(np.uint64)
    return q, np.cumsum(q, dtype=np.uint64)


def faces_of(cum, n_samples, seed, h0=None):
    """Rules 5 and 6: the face int64 [N] of every sample."""
    n = int(n_samples)
    h0 = hashes(n, seed)[0] if h0 is None else h0
    total = cum[-1]
    xi = (h0 >> _U(11)).astype(np.float64) * 2.0 ** -53
    u = (np.arange(n, dtype=np.float64) + xi) / np.float64(n)
    t = np.minimum(np.floor(u * np.float64(total)).astype(np.uint64), total - _U(1))
    return np.searchsorted(cum, t, side="right").astype(np.int64)          # the smallest f with S_f > t


def prepare(vertices, faces, face_weight=None):
    """Rules 1 to 4: (q uint64 [F], S_f uint64 [F], counts int64 [6]); q and S_f are None when nothing can be sampled."""
    m, bad = measures(vertices, faces, face_weight)
    counts = np.array(bad + [0, 0], dtype=np.int64)
    if any(bad):
        return None, None, counts
    q, cum = quantise(m)
    if q is None:
        counts[5] = 1
        return None, None, counts
    counts[4] = int((q == 0).sum())
    return q, cum, counts


def emit(vertices, faces, cum, n_samples, seed):
    """Rules 5 to 8: (points fp64 [N,3], face int64 [N], bary fp64 [N,3])."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    n = int(n_samples)
    if n == 0:
        return np.zeros((0, 3)), np.zeros((0,), dtype=np.int64), np.zeros((0, 3))
    h = hashes(n, seed)
    face = faces_of(cum, n, seed, h[0])
    r1 = (h[1] >> _U(11)).astype(np.float64) * 2.0 ** -53
    r2 = (h[2] >> _U(11)).astype(np.float64) * 2.0 ** -53
    flip = r1 + r2 > 1.0
    r1, r2 = np.where(flip, 1.0 - r1, r1), np.where(flip, 1.0 - r2, r2)
    b0 = np.maximum((1.0 - r1) - r2, 0.0)
    bary = np.stack([b0, r1, r2], axis=1)
    a, b, c = v[f[face, 0]], v[f[face, 1]], v[f[face, 2]]
    points = (a * b0[:, None] + b * r1[:, None]) + c * r2[:, None]
    return points, face, bary


def sample(vertices, faces, n_samples, seed=0, face_weight=None):
    """The whole rule: (points, face, bary, counts); the first three are None when nothing can be sampled (the device
    then writes nothing)."""
    q, cum, counts = prepare(vertices, faces, face_weight)
    if q is None:
        return None, None, None, counts
    return emit(vertices, faces, cum, n_samples, seed) + (counts,)


# ---------------------------------------------------------------------------------------------------------------- meshes
def icosphere(level):
    """The unit icosphere after `level` midpoint subdivisions: (vertices fp64 [V,3], faces int64 [F,3])."""
    p = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1),
         (-p, 0, -1), (-p, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, dtype=np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        mid, out = {}, []

        def midpoint(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                m = v[i] + v[j]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = out
    return np.array(v, dtype=np.float64), np.array(f, dtype=np.int64)


def soup(n_faces, seed, zero_every=0):
    """A triangle soup with 3 F vertices of its own; with `zero_every` = k every k-th face is a sliver of no area (its
    third corner is its first)."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1.0, 1.0, size=(3 * n_faces, 3))
    f = np.arange(3 * n_faces, dtype=np.int64).reshape(n_faces, 3)
    if zero_every:
        v[3 * np.arange(0, n_faces, zero_every) + 2] = v[3 * np.arange(0, n_faces, zero_every)]
    return v, f


def grid_square(nx, ny, x0, x1, y0, y1, z=0.0):
    """The rectangle [x0, x1] x [y0, y1] at height z as an nx by ny grid of quads, two triangles each."""
    xs, ys = np.linspace(x0, x1, nx + 1), np.linspace(y0, y1, ny + 1)
    gx, gy = np.meshgrid(xs, ys, indexing="ij")
    v = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, z)], axis=1)
    idx = np.arange((nx + 1) * (ny + 1)).reshape(nx + 1, ny + 1)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    f = np.concatenate([np.stack([a, b, c], axis=1), np.stack([a, c, d], axis=1)]).astype(np.int64)
    return v, f


def two_tessellation_square():
    """The unit square at z = 0: the half x <= 0.5 as a 32 x 64 grid, the half x >= 0.5 as two triangles."""
    v, f = grid_square(32, 64, 0.0, 0.5, 0.0, 1.0)
    n = v.shape[0]
    w = np.array([[0.5, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 1.0, 0.0], [0.5, 1.0, 0.0]])
    g = np.array([[n, n + 1, n + 2], [n, n + 2, n + 3]], dtype=np.int64)
    return np.concatenate([v, w]), np.concatenate([f, g])


def slanted_plane():
    """The plane z = x / 2 over [-1, 2]^2 as two triangles."""
    v = np.array([[-1.0, -1.0, -0.5], [2.0, -1.0, 1.0], [2.0, 2.0, 1.0], [-1.0, 2.0, -0.5]])
    return v, np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int64)
