"""CPU: the numpy restatement of the texel-position map (tests/texel_fill_reference.py) on hand-checked cases, and the
argument checks of ``baking.texel_positions`` / ``qf_texel_positions`` that fire before any device use."""
import numpy as np
import pytest

from quadraturefields_amd.mesh_io import TriMesh
from tests import texel_fill_reference as ref


def _mesh(corners_rc, H, W, verts=None, faces=None):
    """Mesh whose uv puts vertex k at texel corners_rc[k] of an H x W map (exactly: uv = (r / H, c / W))."""
    rc = np.asarray(corners_rc, dtype=np.float64)
    uv = np.stack([rc[:, 0] / H, rc[:, 1] / W], 1)
    v = np.concatenate([rc, np.zeros((len(rc), 1))], 1) if verts is None else np.asarray(verts, dtype=np.float64)
    f = np.arange(len(rc)).reshape(-1, 3) if faces is None else np.asarray(faces)
    return TriMesh(v, f, uv)


def _cover(mesh, H, W):
    _, q = ref.scaled_corners(mesh.visual.uv, H, W)
    idx, r, c, keep = ref._candidates(q[mesh.faces], np.arange(len(mesh.faces)), None)
    return [set(zip(r[keep & (idx == f)].tolist(), c[keep & (idx == f)].tolist())) for f in range(len(mesh.faces))]


def _run(mesh, H, W, untouched="last_face"):
    return ref.texel_positions(mesh.vertices, mesh.faces, mesh.visual.uv, H, W, untouched)


def test_right_triangle_covers_fifteen_texels():
    m = _mesh([(0, 0), (0, 4), (4, 0)], 8, 8)
    cover = _cover(m, 8, 8)[0]
    assert cover == {(r, c) for r in range(5) for c in range(5) if r + c <= 4}
    V, tri_size = _run(m, 8, 8)
    assert tri_size.tolist() == [15]
    for r, c in cover:                        # vertices placed at their own texels: V is the identity there
        assert V[r, c].tolist() == [r, c, 0.0]


def test_horizontal_and_vertical_edges():
    """Corners (1,1), (1,6), (5,1): a horizontal edge along row 1 and a vertical one along column 1, both inside."""
    m = _mesh([(1, 1), (1, 6), (5, 1)], 8, 8)
    cover = _cover(m, 8, 8)[0]
    assert {(1, c) for c in range(1, 7)} <= cover and {(r, 1) for r in range(1, 6)} <= cover
    # the hypotenuse from (1,6) to (5,1): (r - 1) * 5 + (c - 1) * 4 <= 20
    assert cover == {(r, c) for r in range(1, 6) for c in range(1, 7) if (r - 1) * 5 + (c - 1) * 4 <= 20}


def test_overlapping_faces_later_one_wins():
    verts = np.array([[0, 0, 0], [0, 4, 0], [4, 0, 0], [10, 10, 10], [10, 14, 10], [14, 10, 10]], dtype=np.float64)
    m = _mesh([(0, 0), (0, 4), (4, 0), (0, 0), (0, 4), (4, 0)], 8, 8, verts=verts)
    V, tri_size = _run(m, 8, 8)
    assert tri_size.tolist() == [15, 15]                                  # both counted, whoever owns the texel
    assert V[2, 1].tolist() == [12.0, 11.0, 10.0]                          # face 1's vertices
    m2 = _mesh([(0, 0), (0, 4), (4, 0), (0, 0), (0, 2), (2, 0)], 8, 8, verts=verts)
    V2, ts2 = _run(m2, 8, 8)
    assert ts2.tolist() == [15, 6]
    assert V2[0, 1].tolist() == [10.0, 12.0, 10.0]                         # inside face 1: face 1
    assert V2[3, 1].tolist() == [3.0, 1.0, 0.0]                            # outside it: face 0


def test_degenerate_face_gets_its_centroid():
    verts = np.array([[0, 0, 0], [1, 2, 3], [5, 7, 11]], dtype=np.float64)
    m = _mesh([(2, 1), (2, 3), (2, 5)], 8, 8, verts=verts)                # collinear along row 2
    V, tri_size = _run(m, 8, 8)
    assert tri_size.tolist() == [5]
    cen = (verts.sum(0) / 3).astype(np.float32)
    for c in range(1, 6):
        assert np.array_equal(V[2, c], cen)


def test_uv_outside_unit_square_is_clipped():
    m = TriMesh(np.eye(3), [[0, 1, 2]], np.array([[-0.5, -0.5], [-0.5, 3.0], [2.0, -1.0]]))
    s, q = ref.scaled_corners(m.visual.uv, 6, 4)
    assert q.tolist() == [[0, 0], [0, 3], [5, 0]]
    assert s.min() >= 0 and s[:, 0].max() == 5 and s[:, 1].max() == 3
    V, tri_size = _run(m, 6, 4)
    assert tri_size.tolist() == [len(_cover(m, 6, 4)[0])]


def test_rows_and_columns_of_a_non_square_map():
    """uv[:,0] picks the row (scaled by H), uv[:,1] the column (scaled by W)."""
    H, W = 16, 4
    m = TriMesh(np.eye(3), [[0, 1, 2]], np.array([[0.5, 0.25], [0.5, 0.25], [0.5, 0.25]]))
    _, q = ref.scaled_corners(m.visual.uv, H, W)
    assert q[0].tolist() == [8, 1]
    V, tri_size = _run(m, H, W)
    assert tri_size.tolist() == [1] and V.shape == (H, W, 3)
    cen = np.full(3, 1.0 / 3.0, dtype=np.float32)                         # degenerate face (one point): its centroid
    assert np.array_equal(V[8, 1], cen)


def test_untouched_texels_in_both_modes():
    verts = np.array([[0, 0, 0], [0, 2, 0], [2, 0, 0], [9, 9, 9], [9, 12, 9], [12, 9, 9]], dtype=np.float64)
    m = _mesh([(0, 0), (0, 2), (2, 0), (5, 5), (5, 7), (7, 5)], 8, 8, verts=verts)
    last = (verts[3:].sum(0) / 3).astype(np.float32)
    V, _ = _run(m, 8, 8, "last_face")
    assert np.array_equal(V[0, 7], last)                                  # far from both faces: face F-1's centroid
    Vz, _ = _run(m, 8, 8, "zero")
    assert Vz[0, 7].tolist() == [0.0, 0.0, 0.0]
    assert np.array_equal(V[0, 0], Vz[0, 0])                              # owned texels do not depend on the mode


def test_edge_touch_without_cover_gets_the_edge_face_centroid():
    """A sliver whose truncated corners cover one texel: its edge samples (on the unrounded corners) touch more."""
    H = W = 8
    verts = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [7, 7, 7], [7, 8, 7], [8, 7, 7]], dtype=np.float64)
    uv = np.array([[0.99, 0.99], [3.99, 1.5], [1.5, 3.99], [7.0, 7.0], [7.0, 7.9], [7.9, 7.0]]) / np.array([H, W])
    m = TriMesh(verts, [[0, 1, 2], [3, 4, 5]], uv)
    V, tri_size = _run(m, H, W, "zero")
    cover = _cover(m, H, W)[0]
    touched = {(int(r), int(c)) for a, b in ((0, 1), (1, 2), (2, 0)) for r, c in
               (uv[b] * (H, W) * ref.W_SAMPLES[:, None] + uv[a] * (H, W) * (1 - ref.W_SAMPLES[:, None])).astype(int)}
    extra = touched - cover
    assert extra
    cen = (verts[:3].sum(0) / 3).astype(np.float32)
    for r, c in extra:
        assert np.array_equal(V[r, c], cen)


def test_owned_corner_texel_is_the_vertex_in_fp32():
    rng = np.random.default_rng(3)
    verts = rng.normal(size=(3, 3))
    m = _mesh([(2, 3), (2, 30), (25, 9)], 32, 32, verts=verts)
    V, _ = _run(m, 32, 32)
    for k, (r, c) in enumerate([(2, 3), (2, 30), (25, 9)]):
        assert np.array_equal(V[r, c], verts[k].astype(np.float32))


# ------------------------------------------------------------------------------------------- argument checks
def _tri():
    return TriMesh(np.eye(3), [[0, 1, 2]], np.array([[0.1, 0.1], [0.1, 0.5], [0.5, 0.1]]))


@pytest.mark.parametrize("kwargs, what", [
    (dict(height=0), "height"), (dict(height=16385), "height"), (dict(height=64, width=0), "width"),
    (dict(height=64, width=16385), "width"), (dict(height=64.0), "height"), (dict(height=64, untouched="nan"), "untouched"),
])
def test_texel_positions_refuses_bad_arguments(kwargs, what):
    from quadraturefields_amd import baking
    with pytest.raises(ValueError, match=what):
        baking.texel_positions(_tri(), **kwargs)


def test_texel_positions_refuses_bad_meshes():
    from quadraturefields_amd import baking
    with pytest.raises(ValueError, match="UV"):
        baking.texel_positions(TriMesh(np.eye(3), [[0, 1, 2]]), 64)
    with pytest.raises(ValueError, match="face indices"):
        baking.texel_positions(TriMesh(np.eye(3), [[0, 1, 3]], np.zeros((3, 2))), 64)
    with pytest.raises(ValueError, match="at least one face"):
        baking.texel_positions(TriMesh(np.eye(3), np.zeros((0, 3)), np.zeros((3, 2))), 64)
    with pytest.raises(ValueError, match="finite"):
        baking.texel_positions(TriMesh(np.eye(3), [[0, 1, 2]], np.array([[0, 0], [np.nan, 0], [0, 1]])), 64)
    with pytest.raises(ValueError, match=r"uv must be \[V, 2\]"):
        baking.texel_positions(TriMesh(np.eye(3), [[0, 1, 2]], np.zeros((2, 2))), 64)


def test_c_entry_refuses_before_any_launch(lib):
    """Every check of qf_texel_positions runs on the host before the first launch: no device is needed to see them."""
    assert lib.qf_texel_positions_workspace_bytes(1, 64, 64) > 2 * 4 * 64 * 64
    for n_faces, h, w in [(0, 64, 64), (1, 0, 64), (1, 64, 16385), (1, 16385, 1)]:
        assert lib.qf_texel_positions_workspace_bytes(n_faces, h, w) == -1
    p = 4096                                                               # any non-NULL address: nothing is touched
    ws = lib.qf_texel_positions_workspace_bytes(1, 64, 64)
    good = [p, 3, p, 1, p, 64, 64, 0, p, p, p, ws, None]
    assert lib.qf_texel_positions(*good[:4], None, *good[5:]) == -1       # NULL uv
    assert lib.qf_texel_positions(*good[:8], None, *good[9:]) == -1       # NULL out
    assert lib.qf_texel_positions(*good[:10], None, *good[11:]) == -1     # NULL workspace
    assert lib.qf_texel_positions(*good[:11], ws - 1, None) == -1         # short workspace
    assert lib.qf_texel_positions(*good[:7], 2, *good[8:]) == -1          # unknown untouched mode
    assert lib.qf_texel_positions(*good[:3], 0, *good[4:]) == -1          # no face
    assert lib.qf_texel_positions(*good[:5], 16385, *good[6:]) == -1      # height out of range
    assert lib.qf_texel_positions(p, 0, *good[2:]) == -1                  # no vertex
