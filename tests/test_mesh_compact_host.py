"""CPU: the mesh clean-up rules as ``tests/mesh_compact_reference.py`` restates them -- the
hand-worked case of the section, the union-find against scipy's connected components --, the refusals that
``qf_mesh_compact_*`` / ``qf_mark_hit_faces`` and their wrappers decide before any launch, and ``remap_vertex_features``."""
import numpy as np
import pytest
import torch

from tests import mesh_compact_reference as ref

# V = 10, the mask is zero only at f6
HAND_FACES = np.array([[1, 2, 3], [3, 2, 1], [2, 3, 4], [4, 4, 5], [6, 7, 8], [7, 8, 6], [3, 4, 6]], dtype=np.int64)
HAND_MASK = np.array([1, 1, 1, 1, 1, 1, 0], dtype=np.uint8)
HAND_VERTS = np.arange(30, dtype=np.float64).reshape(10, 3) * 0.25
ALL = dict(remove_degenerate=True, remove_duplicates=True, remove_unreferenced=True)

# (keep, options) -> faces, face_map, vertex_map, counts
HAND_CASES = {
    "all_flags_m2": (HAND_MASK, dict(ALL, min_component_faces=2),
                     [(0, 1, 2), (1, 2, 3)], [0, 2], [1, 2, 3, 4], [2, 4, 1, 1, 2, 1, 2, 0]),
    "all_flags_m0": (HAND_MASK, dict(ALL, min_component_faces=0),
                     [(0, 1, 2), (1, 2, 3), (4, 5, 6)], [0, 2, 4], [1, 2, 3, 4, 6, 7, 8], [3, 7, 1, 1, 2, 0, 2, 0]),
    "degenerate_off_m2": (HAND_MASK, dict(ALL, remove_degenerate=False, min_component_faces=2),
                          [(0, 1, 2), (1, 2, 3), (3, 3, 4)], [0, 2, 3], [1, 2, 3, 4, 5], [3, 5, 1, 0, 2, 1, 2, 0]),
    "no_mask_m2": (None, dict(ALL, min_component_faces=2),
                   [(0, 1, 2), (1, 2, 3), (4, 5, 6), (2, 3, 4)], [0, 2, 4, 6], [1, 2, 3, 4, 6, 7, 8],
                   [4, 7, 0, 1, 2, 0, 1, 0]),
}


@pytest.mark.parametrize("name", sorted(HAND_CASES))
def test_hand_worked_case(name):
    keep, options, faces, face_map, vertex_map, counts = HAND_CASES[name]
    v, f, fm, vm, c = ref.compact(HAND_VERTS, HAND_FACES, keep, **options)
    assert f.tolist() == [list(t) for t in faces]
    assert fm.tolist() == face_map and vm.tolist() == vertex_map and c.tolist() == counts
    assert np.array_equal(v.view(np.int64), HAND_VERTS[vertex_map].view(np.int64))
    # the output is the same triangle soup as the kept input faces
    assert np.array_equal(v[f], HAND_VERTS[HAND_FACES[fm]])


def test_reference_corner_rules():
    # a duplicate whose earlier copy the mask dropped stays; with the vertices kept nothing is renumbered
    f = np.array([[0, 1, 2], [2, 1, 0], [1, 2, 0], [3, 3, 3]], dtype=np.int64)
    v = np.zeros((5, 3))
    out = ref.compact(v, f, [0, 1, 1, 1], remove_duplicates=True, remove_unreferenced=False)
    assert out[2].tolist() == [1, 3] and out[1].tolist() == [[2, 1, 0], [3, 3, 3]] and out[3].tolist() == [0, 1, 2, 3, 4]
    assert out[4].tolist() == [2, 5, 1, 0, 1, 0, 2, 0]
    # an invalid index: nothing is produced, only its count
    bad = ref.compact(v, np.array([[0, 1, 5], [0, -1, 2], [0, 1, 2]]), None)
    assert bad[0].shape == (0, 3) and bad[1].shape == (0, 3) and bad[4].tolist() == [0, 0, 0, 0, 0, 0, 0, 2]
    # no faces: every vertex is unreferenced
    empty = ref.compact(v, np.zeros((0, 3), np.int64))
    assert empty[0].shape == (0, 3) and empty[4].tolist() == [0] * 8
    assert ref.compact(v, np.zeros((0, 3), np.int64), remove_unreferenced=False)[4].tolist() == [0, 5, 0, 0, 0, 0, 0, 0]


def test_components_match_scipy():
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    from scipy.sparse import coo_matrix
    rng = np.random.default_rng(3)
    for n_v, n_f in ((40, 25), (300, 180), (2000, 900)):
        f = rng.integers(0, n_v, size=(n_f, 3))
        alive = rng.random(n_f) < 0.7
        labels = ref.component_labels(f, alive, n_v)
        fa = f[alive]
        rows = np.concatenate([fa[:, 0], fa[:, 1]])
        cols = np.concatenate([fa[:, 1], fa[:, 2]])
        graph = coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(n_v, n_v))
        n_comp, want = csgraph.connected_components(graph, directed=False)
        # the same partition, and every label is its class's smallest vertex
        assert len(np.unique(labels)) == n_comp
        smallest = np.full(n_comp, n_v)
        np.minimum.at(smallest, want, np.arange(n_v))
        assert np.array_equal(labels, smallest[want])
        # counts[6] counts the classes that hold a surviving face
        counts = ref.compact(np.zeros((n_v, 3)), f, alive)[4]
        assert counts[6] == len(np.unique(want[fa[:, 0]]))


def test_mark_hit_faces_reference():
    tri = np.array([[3, 1, -1], [7, 9, 2], [-1, -1, -1], [0, 12, 4]], dtype=np.int32)
    m, bad = ref.mark_hit_faces(tri, None, 10)
    assert np.nonzero(m)[0].tolist() == [0, 1, 2, 3, 4, 7, 9] and bad == 1
    m, bad = ref.mark_hit_faces(tri, np.array([3, 1, 0, 5], np.int32), 10)        # slot (0, 2) = -1 is considered: counted
    assert np.nonzero(m)[0].tolist() == [0, 1, 3, 4, 7] and bad == 2
    m2, _ = ref.mark_hit_faces(np.array([[8]], np.int32), None, 10, mask=m)
    assert np.nonzero(m2)[0].tolist() == [0, 1, 3, 4, 7, 8]


def test_entry_points_refuse_before_any_launch(lib):
    """Sizes out of range, NULL pointers, a short workspace and unknown flags are decided on the host: status -1 without
    a device."""
    assert lib.qf_mesh_compact_workspace_bytes(0, 5) == -1
    assert lib.qf_mesh_compact_workspace_bytes(2 ** 31, 5) == -1
    assert lib.qf_mesh_compact_workspace_bytes(5, -1) == -1
    assert lib.qf_mesh_compact_workspace_bytes(5, 2 ** 31) == -1
    need = lib.qf_mesh_compact_workspace_bytes(100, 200)
    assert need > 0 and lib.qf_mesh_compact_workspace_bytes(100, 0) > 0
    p = 4096                         # a non-NULL address that is never dereferenced: every call below is refused first
    ok = dict(v=p, V=100, f=p, F=200, keep=None, flags=7, M=0, ws=p, ws_bytes=need, counts=p)

    def count(**kw):
        a = dict(ok, **kw)
        return lib.qf_mesh_compact_count(a["v"], a["V"], a["f"], a["F"], a["keep"], a["flags"], a["M"], a["ws"],
                                         a["ws_bytes"], a["counts"], None)

    def emit(n_ov=0, n_of=0, ov=None, of=None, **kw):
        a = dict(ok, **kw)
        return lib.qf_mesh_compact_emit(a["v"], a["V"], a["f"], a["F"], a["keep"], a["flags"], a["M"], a["ws"],
                                        a["ws_bytes"], ov, n_ov, of, n_of, None, None, None)

    for call in (count, emit):
        for bad in (dict(V=0), dict(V=2 ** 31), dict(F=-1), dict(F=2 ** 31), dict(v=None), dict(f=None), dict(ws=None),
                    dict(ws_bytes=need - 1), dict(flags=8), dict(flags=-1), dict(M=-1), dict(M=2 ** 31)):
            assert call(**bad) == -1, (call.__name__, bad)
    assert count(counts=None) == -1
    assert emit(n_ov=101, ov=p) == -1 and emit(n_of=201, of=p) == -1 and emit(n_ov=-1) == -1 and emit(n_of=-1) == -1
    assert emit(n_ov=1) == -1 and emit(n_of=1) == -1               # a capacity without a buffer
    mark = lib.qf_mark_hit_faces
    assert mark(p, None, -1, 5, 10, p, None, None) == -1
    assert mark(p, None, 4, 0, 10, p, None, None) == -1
    assert mark(p, None, 4, 5, -1, p, None, None) == -1
    assert mark(p, None, 4, 5, 2 ** 31, p, None, None) == -1
    assert mark(p, None, 2 ** 38, 4, 10, p, None, None) == -1
    assert mark(None, None, 4, 5, 10, p, None, None) == -1
    assert mark(p, None, 4, 5, 10, None, None, None) == -1
    assert mark(None, None, 0, 5, 10, None, None, None) == 0       # no rays: nothing to do


def test_wrappers_validate_arguments():
    from quadraturefields_amd import baking, mc_utils
    v, f = torch.zeros((4, 3), dtype=torch.float64), torch.zeros((2, 3), dtype=torch.int64)
    with pytest.raises(ValueError, match="device tensors"):
        mc_utils.compact_mesh_device(v, f)
    with pytest.raises(TypeError):
        mc_utils.compact_mesh_device(v.numpy(), f)
    with pytest.raises(ValueError):
        mc_utils.compact_mesh_device(v[:, :2], f)
    with pytest.raises(TypeError):
        mc_utils.compact_mesh_device(v.to(torch.int32), f)
    with pytest.raises(TypeError):
        mc_utils.compact_mesh_device(v, f.to(torch.float32))
    for m in (-1, 2 ** 31, 2.5):
        with pytest.raises(ValueError, match="min_component_faces"):
            mc_utils.compact_mesh_device(v, f, min_component_faces=m)
    with pytest.raises(ValueError, match="device tensors"):
        mc_utils.mark_hit_faces(torch.zeros((2, 3), dtype=torch.int32), None, torch.zeros(4, dtype=torch.uint8))
    with pytest.raises(TypeError):
        mc_utils.train_visibility_mask(object(), [])
    from quadraturefields_amd.mesh_io import TriMesh
    with pytest.raises(ValueError, match="compact=True"):
        baking.prune_faces(TriMesh(v.numpy(), f.numpy()), np.ones(2, bool), min_component_faces=3)


def test_prune_faces_default_and_maps():
    """Without ``compact`` the mesh is what it always was; ``return_maps`` names the kept faces and every vertex."""
    from quadraturefields_amd import baking
    from quadraturefields_amd.mesh_io import TriMesh
    rng = np.random.default_rng(0)
    mesh = TriMesh(rng.normal(size=(9, 3)), rng.integers(0, 9, size=(12, 3)), rng.random((9, 2)))
    w = rng.random(12).astype(np.float32)
    a = baking.prune_faces(mesh, w, 0.5)
    b, fm, vm = baking.prune_faces(mesh, w, 0.5, return_maps=True)
    assert np.array_equal(a.faces, mesh.faces[w > 0.5]) and np.array_equal(a.vertices, mesh.vertices)
    assert np.array_equal(a.faces, b.faces) and np.array_equal(a.visual.uv, mesh.visual.uv)
    assert np.array_equal(fm, np.nonzero(w > 0.5)[0]) and np.array_equal(vm, np.arange(9))


def test_remap_vertex_features_cpu():
    from quadraturefields_amd import _C, baking
    rng = np.random.default_rng(1)
    feats = torch.from_numpy(rng.normal(size=(7, 3 + 7 * 2 + 1)).astype(np.float32))
    vmap = np.array([1, 2, 5], dtype=np.int64)
    out = baking.remap_vertex_features(feats, vmap)
    assert type(out) is torch.Tensor and torch.equal(out, feats[[1, 2, 5]])
    assert torch.equal(baking.remap_vertex_features(feats, torch.from_numpy(vmap)), out)
    module = baking.VertexBakedFeatures(feats, train_density=False)
    remapped = baking.remap_vertex_features(module, vmap)
    assert isinstance(remapped, baking.VertexBakedFeatures) and remapped.n_lobes == 2 and not remapped.train_density
    assert remapped.table.shape == (3, _C.vertex_row_stride(2))
    assert torch.equal(remapped.table.detach(), module.table.detach()[[1, 2, 5]])
    with pytest.raises(IndexError):
        baking.remap_vertex_features(feats, np.array([0, 7]))
    with pytest.raises(ValueError):
        baking.remap_vertex_features(feats, np.array([0.0, 1.0]))
    quantised = object.__new__(baking.QuantisedVertexFeatures)
    with pytest.raises(TypeError, match="quantise after compaction"):
        baking.remap_vertex_features(quantised, vmap)
