"""Host: the numpy restatement of the vertex-clustering rules (tests/vertex_clustering_reference.py) on hand-derived
cases, DESIGN.md section 3.9."""
import numpy as np
import pytest

from tests import vertex_clustering_reference as ref


def test_two_faces_inside_one_cell_collapse_to_nothing():
    v = np.array([[0.1, 0.1, 0.1], [0.2, 0.1, 0.1], [0.1, 0.2, 0.1], [0.2, 0.2, 0.1]])
    f = np.array([[0, 1, 2], [1, 3, 2]])
    for c in ref.CONTRACTIONS:
        ov, of = ref.simplify(v, f, 1.0, c)
        assert ov.shape == (1, 3) and of.shape == (0, 3)
    ov, _ = ref.simplify(v, f, 1.0, "average")
    assert np.array_equal(ov[0], ((((v[0] + v[1]) + v[2]) + v[3]) / 4))


def test_strip_across_cells_keeps_winding_under_rotation():
    # one vertex per unit cell (lo = -0.5, s = 1): cell ids follow first appearance 0..4
    v = np.array([[4.0, 0, 0], [0, 0, 0], [1, 0, 0], [2, 1, 0], [3, 1, 0]])
    f = np.array([[2, 0, 1], [3, 1, 4], [1, 3, 2]])
    _, of = ref.simplify(v, f, 1.0, "average")
    # (2, 0, 1) -> rotated (0, 1, 2); (3, 1, 4) -> (1, 4, 3); (1, 3, 2) -> (1, 3, 2)
    assert of.tolist() == [[0, 1, 2], [1, 4, 3], [1, 3, 2]]
    for a, b in zip(f, of):
        # same cyclic order
        assert any(list(np.roll(a, k)) == list(b) for k in range(3))


def test_duplicates_same_winding_once_opposite_winding_kept():
    v = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0.1, 0.1, 0], [5, 5, 5], [6, 5, 5]])
    # faces 0 and 2 map to the same triple (vertex 3 shares vertex 0's cell); face 1 is its opposite winding;
    # face 3 is unrelated and comes in between
    f = np.array([[0, 1, 2], [0, 2, 1], [1, 2, 3], [1, 4, 5], [3, 1, 2], [2, 1, 3]])
    _, of, info = ref.simplify(v, f, 1.0, "average", details=True)
    assert of.tolist() == [[0, 1, 2], [0, 2, 1], [1, 3, 4]]
    assert info["face_source"].tolist() == [0, 1, 3]


def test_first_appearance_numbering():
    v = np.array([[5.0, 0, 0], [0, 0, 0], [5.2, 0, 0], [2, 0, 0], [0.1, 0, 0]])
    ov, _, info = ref.simplify(v, np.zeros((0, 3), np.int64), 1.0, "average", details=True)
    assert info["vertex_cell"].tolist() == [0, 1, 0, 2, 1]
    assert np.array_equal(ov[0], (v[0] + v[2]) / 2) and np.array_equal(ov[2], v[3])


def test_vertex_without_faces_keeps_its_cell():
    v = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [9, 9, 9]])
    ov, of = ref.simplify(v, np.array([[0, 1, 2]]), 1.0, "quadric")
    assert len(ov) == 4 and np.array_equal(ov[3], v[3]) and of.tolist() == [[0, 1, 2]]


def _corner_patch(s=1.0):
    """Three axis-aligned faces meeting at the corner (1, 1, 1) of a cube [0,1]^3, cut finely; s = 1 puts the corner
    region's vertices into a cell whose mean is off the corner."""
    vs, fs = [], []

    def quad(p, du, dv):
        base = len(vs)
        for a in range(3):
            for b in range(3):
                vs.append(p + a * 0.2 * du + b * 0.2 * dv)
        for a in range(2):
            for b in range(2):
                i = base + 3 * a + b
                fs.append([i, i + 3, i + 4])
                fs.append([i, i + 4, i + 1])

    e = np.eye(3)
    c = np.array([1.0, 1.0, 1.0])
    quad(c, -e[1], -e[2])
    quad(c, -e[2], -e[0])
    quad(c, -e[0], -e[1])
    return np.array(vs), np.array(fs)


def test_cube_corner_quadric_lands_on_the_corner():
    v, f = _corner_patch()
    ov, _, info = ref.simplify(v, f, 1.0, "quadric", details=True)
    # lo = 0.6 - 0.5 = 0.1: every vertex in [0.6, 1] lies in cell (0, 0, 0) -> one cell, three orthogonal plane sets
    assert len(ov) == 1 and info["accepted"].all()
    assert ov[0].tolist() == [1.0, 1.0, 1.0]
    assert not np.array_equal(info["mean"][0], ov[0])


def test_flat_patch_and_crease_fall_back_to_the_mean():
    v, f = _corner_patch()
    flat = f[:8]                                   # the x = 1 face alone
    ov, _, info = ref.simplify(v, flat, 1.0, "quadric", details=True)
    assert not info["accepted"][0] and np.array_equal(ov[0], info["mean"][0])
    crease = f[:16]                                # x = 1 and y = 1: a line of minimisers
    ov, _, info = ref.simplify(v, crease, 1.0, "quadric", details=True)
    assert not info["accepted"][0] and np.array_equal(ov[0], info["mean"][0])


def test_ill_conditioned_cell_trips_the_box_guard():
    """Three nearly parallel planes through points far apart: det A clears the threshold but the intersection lies far
    outside the cell."""
    v = np.array([[0.0, 0, 0], [0.3, 0, 0], [0, 0.3, 0],                    # z = 0
                  [0.0, 0, 0.3], [0.3, 0, 0.3], [0, 0.3, 0.33],             # tilted a little about y
                  [0.0, 0, 0.15], [0.3, 0, 0.18], [0, 0.3, 0.15]])          # tilted a little about x
    f = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]])
    ov, _, info = ref.simplify(v, f, 1.0, "quadric", details=True)
    assert len(ov) == 1
    assert info["det"][0] > info["thresh"][0]      # the determinant test alone would accept
    assert not info["accepted"][0] and np.array_equal(ov[0], info["mean"][0])


def test_voxel_larger_than_the_mesh_gives_one_vertex_and_no_faces():
    rng = np.random.default_rng(0)
    v = rng.uniform(-1, 1, size=(50, 3))
    f = rng.integers(0, 50, size=(80, 3))
    for c in ref.CONTRACTIONS:
        ov, of = ref.simplify(v, f, 10.0, c)
        assert ov.shape == (1, 3) and of.shape == (0, 3)
        lo = v.min(axis=0) - 5.0
        assert ((ov >= lo - 5.0) & (ov <= lo + 15.0)).all()


def test_output_vertices_stay_in_their_grown_cell():
    rng = np.random.default_rng(3)
    v = rng.normal(size=(400, 3))
    f = rng.integers(0, 400, size=(900, 3))
    s = 0.5
    ov, of, info = ref.simplify(v, f, s, "quadric", details=True)
    lo = v.min(axis=0) - 0.5 * s
    assert ((ov >= lo + (info["cell"] - 0.5) * s) & (ov <= lo + (info["cell"] + 1.5) * s)).all()
    assert (of[:, 0] < of[:, 1]).all() and (of[:, 0] < of[:, 2]).all()
    assert len(np.unique(of, axis=0)) == len(of)


def test_repeated_index_face_has_a_zero_plane_and_is_dropped():
    """Marching cubes keeps faces such as (v, v, w): their plane is zero, and they map to a repeated cell id."""
    v, f = _corner_patch()
    g = np.concatenate([f[:4], [[0, 0, 5]], f[4:]])
    assert not ref.face_planes(v, g[4:5]).any()
    a = ref.simplify(v, f, 0.25, "quadric")
    b = ref.simplify(v, g, 0.25, "quadric")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("bad", ["s0", "sneg", "sinf", "nan", "face_hi", "face_neg", "cells"])
def test_errors(bad):
    v = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
    f = np.array([[0, 1, 2]])
    s = 0.5
    if bad == "s0":
        s = 0.0
    elif bad == "sneg":
        s = -1.0
    elif bad == "sinf":
        s = float("inf")
    elif bad == "nan":
        v[1, 2] = np.nan
    elif bad == "face_hi":
        f = np.array([[0, 1, 3]])
    elif bad == "face_neg":
        f = np.array([[0, -1, 2]])
    elif bad == "cells":
        s = 1.0 / (1 << 21)
    with pytest.raises(ref.ClusteringError):
        ref.simplify(v, f, s)
