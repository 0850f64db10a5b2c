"""Meshes, triangles and query sets shared by tests/test_closest_point_host.py and tests/test_gpu_closest_point.py (the
rule is DESIGN.md section 3.9f, restated in tests/closest_point_reference.py).  Everything is seeded or closed-form."""
import functools

import numpy as np

from tests import closest_point_reference as cp
from tests import mesh_decimate_reference as ref

F32, F64 = np.float32, np.float64

# The triangle (0,0,0), (1,0,0), (0,1,0) and one query per region, worked by hand:
#   query            region      (v, w)          closest point      dist2
HAND_TRIANGLE = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], F32)
HAND = [
    ((-1.0, -1.0, 0.0), "A", (0.0, 0.0), 2.0),            # beyond the corner a: (0,0,0), 1 + 1
    ((2.0, -0.5, 0.0), "B", (1.0, 0.0), 1.25),            # beyond b: (1,0,0), 1 + 0.25
    ((0.5, -1.0, 0.0), "AB", (0.5, 0.0), 1.0),            # below the edge ab: (0.5,0,0), 1
    ((-0.5, 2.0, 0.0), "C", (0.0, 1.0), 1.25),            # beyond c: (0,1,0), 0.25 + 1
    ((-1.0, 0.5, 0.0), "AC", (0.0, 0.5), 1.0),            # left of the edge ac: (0,0.5,0), 1
    ((1.0, 1.0, 0.0), "BC", (0.5, 0.5), 0.5),             # across the hypotenuse: (0.5,0.5,0), 0.25 + 0.25
    ((0.25, 0.25, 1.0), "interior", (0.25, 0.25), 1.0),   # above the inside: (0.25,0.25,0), 1
]


def zero_area_triangles():
    """name -> one fp32 triangle [1,3,3] without area (or, the sliver, with a 1e-7 of it).  The collinear ones lie on the
    line o + t d with dyadic o, d and t, so they are collinear exactly, each vertex in the middle in turn."""
    o, d = np.array([0.25, 0.125, 0.5]), np.array([1.0, 0.5, -0.25])
    at = lambda t: o + t * d
    p, q, r = at(-1.0), at(0.0), at(0.75)
    g, h = np.array([0.5, -0.25, 0.75]), np.array([-0.75, 0.5, 0.25])
    out = {
        "point": [g, g, g],
        "a_is_b": [g, g, h], "b_is_c": [h, g, g], "a_is_c": [g, h, g],
        "collinear_a_mid": [q, p, r], "collinear_b_mid": [p, q, r], "collinear_c_mid": [p, r, q],
        "sliver": [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.5, 1e-7, 0.0]],
    }
    res = {}
    for name, tri in out.items():
        t32 = np.array([tri], F32)
        if name != "sliver":
            assert np.array_equal(t32.astype(F64), np.array([tri], F64)), name      # exactly representable
        res[name] = t32
    return res


def box_queries(n, seed, half=2.0):
    return np.random.default_rng(seed).uniform(-half, half, (n, 3))


@functools.lru_cache(maxsize=None)
def grid_mesh(n=5):
    """tests/mesh_decimate_reference.grid: the unit square, coordinates k / (n - 1) (dyadic for n = 5, 65)."""
    v, f = ref.grid(n)
    assert np.array_equal(v.astype(F32).astype(F64), v)
    return v, f


def grid_tie_queries(n=5, heights=(0.0, 0.25, 0.5)):
    """Queries at the grid's vertices, at the midpoints of its edges and at the lattice points above both, with the face
    every one of them must get: the lowest id among the faces that hold the vertex / the edge."""
    v, f = grid_mesh(n)
    pts, want = [], []
    for i in range(v.shape[0]):
        pts.append(v[i])
        want.append(int(np.nonzero((f == i).any(axis=1))[0][0]))
    edges = {tuple(sorted((int(face[k]), int(face[(k + 1) % 3])))) for face in f for k in range(3)}
    for a, b in sorted(edges):
        pts.append((v[a] + v[b]) * 0.5)
        want.append(int(np.nonzero((f == a).any(axis=1) & (f == b).any(axis=1))[0][0]))
    pts, want = np.array(pts), np.array(want)
    q = np.concatenate([pts + np.array([0.0, 0.0, z]) for z in heights])
    return q, np.tile(want, len(heights)), np.repeat(np.array(heights), pts.shape[0])


def duplicated_face_mesh(n=5, face=7):
    """The grid with face `face` appended once more as the last face."""
    v, f = grid_mesh(n)
    return v, np.concatenate([f, f[face:face + 1]])


@functools.lru_cache(maxsize=None)
def sphere(level):
    return ref.icosphere(level)


def sphere_feature_queries(level=3):
    """Exactly on the vertices (as the tree holds them: rounded to fp32), and on the edge midpoints and centroids of the
    rounded triangles."""
    v, f = sphere(level)
    t = cp.triangles_of(v, f).astype(F64)
    mids = np.concatenate([(t[:, k] + t[:, (k + 1) % 3]) * 0.5 for k in range(3)])
    return np.concatenate([v.astype(F32).astype(F64), mids, ((t[:, 0] + t[:, 1]) + t[:, 2]) / 3.0])


def small_meshes():
    """name -> (vertices fp64, faces): 1, 8 and 9 triangles (a leaf of the wide tree holds 8) and 65."""
    rng = np.random.default_rng(11)
    out = {}
    for n in (1, 8, 9, 65):
        out[f"soup{n}"] = (rng.uniform(-1, 1, (3 * n, 3)).astype(F32).astype(F64), np.arange(3 * n).reshape(n, 3))
    return out


def answer_boxes(triangles, tri):
    t = np.asarray(triangles, F64)[tri]
    return t.min(axis=1), t.max(axis=1)
