"""numpy restatement of the mesh clean-up rules (include/qf_mesh_compact.h) and of
``qf_mark_hit_faces``.  Written for reading, not speed: the union-find is a plain Python loop."""
import numpy as np

COUNT_NAMES = ("faces", "vertices", "dropped_mask", "dropped_degenerate", "dropped_duplicate", "dropped_island",
               "components", "invalid_faces")


def _find(parent, x):
    while parent[x] != x:
        parent[x] = parent[parent[x]]
        x = parent[x]
    return x


def component_labels(faces, alive, n_vertices):
    """Label of every vertex: the smallest vertex index connected to it through the faces with ``alive`` set."""
    parent = list(range(n_vertices))
    for f in np.nonzero(alive)[0]:
        a, b, c = (int(i) for i in faces[f])
        for x, y in ((a, b), (b, c)):
            rx, ry = _find(parent, x), _find(parent, y)
            if rx != ry:
                parent[max(rx, ry)] = min(rx, ry)
    return np.array([_find(parent, v) for v in range(n_vertices)], dtype=np.int64)


def compact(vertices, faces, keep=None, *, remove_degenerate=False, remove_duplicates=False, min_component_faces=0,
            remove_unreferenced=True):
    """``(out_vertices, out_faces, face_map, vertex_map, counts)``: fp64 [V',3], int64 [F',3], int64 [F'], int64 [V'] and
    int64 [8] in the order of ``COUNT_NAMES``.  With an invalid face the arrays are empty and only counts[7] is set."""
    v = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.ascontiguousarray(faces, dtype=np.int64).reshape(-1, 3)
    n_v, n_f = v.shape[0], f.shape[0]
    counts = np.zeros(8, dtype=np.int64)
    # 1. validity
    invalid = ((f < 0) | (f >= n_v)).any(axis=1)
    if invalid.any():
        counts[7] = int(invalid.sum())
        return (np.zeros((0, 3), np.float64), np.zeros((0, 3), np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64),
                counts)
    # 2. mask
    alive = np.ones(n_f, dtype=bool) if keep is None else np.asarray(keep).reshape(-1) != 0
    counts[2] = int((~alive).sum())
    # 3. degenerate
    if remove_degenerate:
        deg = alive & ((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2]))
        counts[3] = int(deg.sum())
        alive &= ~deg
    # 4. duplicates: the lowest surviving face of every sorted triple stays
    if remove_duplicates:
        seen = set()
        for i in np.nonzero(alive)[0]:
            key = tuple(sorted(int(x) for x in f[i]))
            if key in seen:
                alive[i] = False
                counts[4] += 1
            else:
                seen.add(key)
    # 5. components and islands
    labels = component_labels(f, alive, n_v)
    face_label = labels[f[:, 0]]
    roots, sizes = np.unique(face_label[alive], return_counts=True)
    counts[6] = len(roots)
    if min_component_faces >= 2:
        small = set(roots[sizes < min_component_faces].tolist())
        island = alive & np.array([int(l) in small for l in face_label], dtype=bool)
        counts[5] = int(island.sum())
        alive &= ~island
    # 6. unreferenced vertices
    face_map = np.nonzero(alive)[0].astype(np.int64)
    out_f = f[face_map]
    if remove_unreferenced:
        used = np.zeros(n_v, dtype=bool)
        used[out_f.reshape(-1)] = True
        vertex_map = np.nonzero(used)[0].astype(np.int64)
        new_index = np.cumsum(used) - used                 # the number of kept vertices below each vertex
        out_f = new_index[out_f].astype(np.int64).reshape(-1, 3)
    else:
        vertex_map = np.arange(n_v, dtype=np.int64)
    counts[0], counts[1] = len(face_map), len(vertex_map)
    return v[vertex_map].copy(), out_f, face_map, vertex_map, counts


def mark_hit_faces(hit_tri, hit_count, n_faces, mask=None):
    """``(mask, out_of_range)``: uint8 [n_faces] with the bytes of the considered ids set on top of ``mask``."""
    t = np.asarray(hit_tri)
    n_rays, k = t.shape
    out = np.zeros(n_faces, dtype=np.uint8) if mask is None else np.array(mask, dtype=np.uint8)
    if hit_count is None:
        considered = t >= 0
    else:
        c = np.minimum(np.asarray(hit_count).reshape(-1), k)
        considered = np.arange(k)[None, :] < c[:, None]
    ids = t[considered]
    ok = (ids >= 0) & (ids < n_faces)
    out[ids[ok]] = 1
    return out, int((~ok).sum())
