"""CPU: the numpy restatement of the per-triangle UV atlas (tests/uv_atlas_reference.py) against
hand-derived cases, and its composition with the texel-position map's restatement and the baked path's lookup."""
import numpy as np
import pytest

from tests import texel_fill_reference as fill
from tests import uv_atlas_reference as ref

D = 1.0 / 16.0
UNIT = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])       # |n| = 1, l = 1; the hypotenuse faces corner 0


def _copies(n, zero_area=0):
    """n unit right triangles then ``zero_area`` collapsed ones, unshared."""
    tri = [UNIT] * n + [UNIT[[0, 0, 1]]] * zero_area
    v = np.concatenate(tri)
    return v, np.arange(len(v)).reshape(-1, 3)


def test_two_equal_faces_share_one_block():
    """S = 8, N = 2, rho = 2.5: both faces are class 2 and equal in every key, so face 0 takes the lower half and face 1
    the upper half of the 3 x 4 block at (0, 0)."""
    v, f = _copies(2)
    a = ref.atlas(v, f, 8, texels_per_unit=2.5, N=2)
    assert a["face_class"].tolist() == [2, 2] and a["face_half"].tolist() == [0, 1]
    assert a["face_origin"].tolist() == [[0, 0], [0, 0]]
    assert a["class_counts"].tolist() == [0, 0, 2] and a["rows_used"] == 3 and a["texels_used"] == 12
    want = np.array([[D, D], [3 - 2 * D, D], [D, 3 - 2 * D],
                     [3 - D, 4 - D], [2 * D, 4 - D], [3 - D, 1 + 2 * D]]) / 8.0
    assert np.array_equal(a["uv"], want)
    # truncated corners: (0,0),(k,0),(0,k) and (k,k+1),(0,k+1),(k,1)
    assert np.floor(a["uv"] * 8).astype(int).tolist() == [[0, 0], [2, 0], [0, 2], [2, 3], [0, 3], [2, 1]]


def test_right_angle_goes_opposite_the_longest_edge():
    """The same triangle with its corners rotated: p0 follows the corner opposite the hypotenuse, p1 and p2 the cycle."""
    want = np.array([[D, D], [3 - 2 * D, D], [D, 3 - 2 * D]]) / 8.0
    for shift in range(3):
        v = np.roll(UNIT, shift, axis=0)                   # the right angle is now corner ``shift``
        a = ref.atlas(v, np.arange(3).reshape(1, 3), 8, texels_per_unit=2.5, N=2)
        assert np.array_equal(a["uv"], np.roll(want, shift, axis=0))


def test_odd_class_count_leaves_the_last_block_half_full():
    """S = 16, N = 2: P_2 = 15 // 4 = 3 blocks per shelf; three faces fill block 0 and the lower half of block 1."""
    v, f = _copies(3)
    a = ref.atlas(v, f, 16, texels_per_unit=2.0, N=2)
    assert a["face_origin"].tolist() == [[0, 0], [0, 0], [0, 4]] and a["face_half"].tolist() == [0, 1, 0]
    assert a["rows_used"] == 3 and a["texels_used"] == 18
    assert np.array_equal(a["uv"][6:], np.array([[D, 4 + D], [3 - 2 * D, 4 + D], [D, 7 - 2 * D]]) / 16.0)


def test_a_class_wraps_to_a_second_shelf_and_shorter_classes_follow():
    """S = 16, N = 2: seven class-2 faces need four blocks, one more than a shelf holds; three zero-area faces are class
    0 and start below the two class-2 shelves, 1 x 2 blocks, seven to a shelf."""
    v, f = _copies(7, zero_area=3)
    a = ref.atlas(v, f, 16, texels_per_unit=2.0, N=2)
    assert a["face_class"].tolist() == [2] * 7 + [0] * 3 and a["class_counts"].tolist() == [3, 0, 7]
    assert a["face_origin"][:7].tolist() == [[0, 0], [0, 0], [0, 4], [0, 4], [0, 8], [0, 8], [3, 0]]
    assert a["face_origin"][7:].tolist() == [[6, 0], [6, 0], [6, 2]] and a["face_half"][7:].tolist() == [0, 1, 0]
    assert a["rows_used"] == 7 and a["texels_used"] == 7 * 6 + 3
    # a class-0 chart is one texel: lower (r, c), upper (r, c + 1)
    assert np.floor(a["uv"][21:] * 16).astype(int).reshape(3, 3, 2).tolist() == [[[6, 0]] * 3, [[6, 1]] * 3, [[6, 2]] * 3]


def _soup(n=300, n_zero=12, seed=3):
    """Unshared random triangles whose areas spread over 100x (legs over 10x), ``n_zero`` of them with zero area."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-1, 1, size=(n, 1, 3))
    leg = np.exp(rng.uniform(np.log(0.05), np.log(0.5), size=(n, 1, 1)))
    tri = centre + leg * rng.normal(size=(n, 3, 3))
    h = n_zero // 2
    tri[:h, 2] = tri[:h, 1]                                              # two equal corners
    tri[h:n_zero] = np.round(tri[h:n_zero] * 64) / 64                    # dyadic corners: c = 2 b - a is exact,
    tri[h:n_zero, 2] = 2 * tri[h:n_zero, 1] - tri[h:n_zero, 0]           # so the cross product is exactly zero
    return tri.reshape(-1, 3), np.arange(3 * n).reshape(-1, 3)


def test_search_ends_between_a_density_that_fits_and_one_that_does_not():
    """The searched rho fits and the bound the bisection ended on, at most 2^-40 of the doubling gap above it, does not;
    a saturated histogram ends the doubling with rho = hi."""
    v, f = _soup()
    ell = ref.measure(v, f)[0]
    assert (ell == 0).sum() >= 12 and (ell.max() / ell[ell > 0].min()) ** 2 > 100     # l^2 is the area (times two)
    rho, hi = ref.search(ell, 64, 15)
    assert ref.probe(rho, ell, 64, 15)[0] and not ref.probe(hi, ell, 64, 15)[0]
    # hi doubled to 2^m, then 40 halvings of a gap of 2^(m-1)
    m = np.ceil(np.log2(hi))
    assert 0 < hi - rho <= 2.0 ** (m - 1 - ref.BISECTIONS)
    # one face in a large atlas: the histogram saturates at the first power of two that reaches class N, and that is rho
    rho, hi = ref.search(np.array([1.0, 0.0]), 256, 63)
    assert rho == hi == 64.0


def test_max_leg_zero_saturates_at_once_whatever_the_areas():
    """N = 0: every face is class N at any density, faces without area included, so the doubling ends at hi = 1."""
    assert ref.search(np.array([1.0, 0.0, 2.0]), 64, 0) == (1.0, 1.0)
    assert ref.search(np.array([0.0, np.nan]), 64, 0) == (1.0, 1.0)
    v, f = _copies(3, zero_area=2)
    a = ref.atlas(v, f, 8, N=0)
    assert a["rho"] == 1.0 and a["class_counts"].tolist() == [5] and a["face_class"].tolist() == [0] * 5
    # one class: Morton order alone; the collapsed faces' centroid (1/3, 0, 0) comes before the others' (1/3, 1/3, 0)
    assert a["face_origin"].tolist() == [[0, 2], [0, 2], [0, 4], [0, 0], [0, 0]] and a["rows_used"] == 1
    assert a["face_half"].tolist() == [0, 1, 0, 0, 1]
    # faces without area never reach class N > 0 and do not hold the search up either
    assert ref.search(np.array([1.0, 0.0, np.nan]), 256, 3) == (4.0, 4.0)


class _Shape:
    """Stands in for a mesh too large to build: broadcast views with the shapes of its arrays."""

    def __init__(self, n_vertices, n_faces):
        self.vertices = np.broadcast_to(np.zeros((1, 3)), (n_vertices, 3))
        self.faces = np.broadcast_to(np.zeros((1, 3), dtype=np.int64), (n_faces, 3))


def test_sizes_are_refused_before_the_mesh_is_copied_or_the_library_loaded(monkeypatch):
    from quadraturefields_amd import uv_atlas

    def no_library():
        raise AssertionError("the library was asked for")

    monkeypatch.setattr(uv_atlas._C, "lib", no_library)
    first_refused = -(-2 ** 31 // 3)                                        # the smallest F with 3 F >= 2^31
    for mesh in (_Shape(4, first_refused), _Shape(4, 0), _Shape(2 ** 31, 2), _Shape(0, 2)):
        with pytest.raises(ValueError, match="faces|vertices"):
            uv_atlas.per_triangle_atlas(mesh, 128)
    with pytest.raises(AssertionError, match="library"):                    # one face fewer passes the size checks
        uv_atlas.per_triangle_atlas(_Shape(4, 2), 128, device="cuda:0")


def test_too_many_faces_are_refused_with_the_capacity():
    """S = 8: 7 usable rows of 3 class-0 blocks, two faces each."""
    assert ref.capacity(8) == 42
    v, f = _copies(42)
    assert ref.atlas(v, f, 8, N=2)["rows_used"] == 7
    v, f = _copies(43)
    with pytest.raises(ValueError, match="42"):
        ref.atlas(v, f, 8, N=2)
    with pytest.raises(ValueError, match="rows_used"):
        ref.atlas(*_copies(8), 8, texels_per_unit=2.5, N=2)               # 4 blocks of 3 rows: 12 > 7


def test_composition_with_the_texel_position_map_and_the_lookup():
    S, N = 64, 15
    v, f = _soup()
    F = len(f)
    a = ref.atlas(v, f, S, N=N)
    k = a["face_class"].astype(np.int64)
    assert len(np.unique(k)) >= 5 and (k == 0).sum() >= 12
    assert (a["uv"] >= 0).all() and (a["uv"] < 1).all()
    size = (k + 1) * (k + 2) // 2
    assert np.array_equal(fill.cover_counts(f, a["uv"], S, S), size)
    V, tri_size = fill.texel_positions(v, f, a["uv"], S, S, "zero")
    assert np.array_equal(tri_size, size) and size.sum() == a["texels_used"]
    filled = (V != 0).any(-1)
    assert filled.sum() == size.sum()                                      # no texel has two owners
    assert not filled[-1].any() and not filled[:, -1].any() and a["rows_used"] <= S - 1
    texel = ref.lookup(a["uv"], S, ref.lookup_points(F))
    ok = ref.in_staircase(texel, k[:, None], a["face_origin"].astype(np.int64)[:, None], a["face_half"][:, None])
    assert ok.all(), np.argwhere(~ok)[:5]
    # and the staircases are what the map drew: every texel of face f's chart holds a point of face f
    owner = np.full((S, S), -1)
    for face in range(F):
        t = ref.staircase(k[face], a["face_origin"][face], a["face_half"][face])
        assert (owner[t[:, 0], t[:, 1]] == -1).all()
        owner[t[:, 0], t[:, 1]] = face
    assert np.array_equal(owner >= 0, filled)


def test_obj_export_round_trips(tmp_path):
    """``TriMesh.export_obj`` writes v / vt / f a/a b/b c/c with enough digits for ``load_mesh`` to return the same arrays."""
    from quadraturefields_amd.mesh_io import TriMesh, load_mesh
    v, f = _soup(n=40, n_zero=4)
    a = ref.atlas(v, f, 64, N=15)
    mesh = TriMesh(v, f, a["uv"])
    path = str(tmp_path / "atlas.obj")
    mesh.export_obj(path)
    lines = open(path).read().split("\n")
    assert lines[0].startswith("v ") and lines[len(v)].startswith("vt ") and lines[2 * len(v)] == "f 1/1 2/2 3/3"
    back = load_mesh(path)
    assert np.array_equal(back.vertices.view(np.uint64), mesh.vertices.view(np.uint64))
    assert np.array_equal(back.faces, mesh.faces)
    assert np.array_equal(back.visual.uv.view(np.uint64), mesh.visual.uv.view(np.uint64))
    TriMesh(v, f).export_obj(path)
    back = load_mesh(path)
    assert np.array_equal(back.vertices, v) and np.array_equal(back.faces, f) and back.visual.uv is None
