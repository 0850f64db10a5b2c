"""CPU: the numpy restatement of the pruning stage on a hand-worked case, ``baking.prune_faces`` and the stage's file
writer (names, dtypes and shapes round-trip through ``mesh_io``)."""
import os

import numpy as np

from tests import prune_reference as ref

THR = np.float32(1e-3)

# six triangles over seven vertices (a fan), two views
VERTS = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [-1, 1, 0], [-1, 0, 0], [-1, -1, 0]], dtype=np.float64)
FACES = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 5], [0, 5, 6], [0, 6, 1]], dtype=np.int64)
# view A: triangle 0 twice (0.5 wins), triangle 1 below the threshold, triangle 2 EXACTLY the threshold, triangle 4 low
VIEW_A = (np.array([0.2, 0.5, 0.0004, THR, 0.0002], dtype=np.float32), np.array([0, 0, 1, 2, 4]))
# view B: triangle 1 still below, triangle 2 below its own maximum, triangle 4 lifted above, triangle 5 seen once;
# triangle 3 is never hit
VIEW_B = (np.array([0.0009, 0.0005, 0.25, 0.75, 0.1], dtype=np.float32), np.array([1, 2, 4, 5, 0]))
WANT_TW = np.array([0.5, 0.0009, THR, 0.0, 0.25, 0.75], dtype=np.float32)
WANT_MASK = np.array([True, False, False, False, True, True])


def test_hand_worked_case():
    tw, mask, verts, faces, ns, nv = ref.prune(VERTS, FACES, [VIEW_A, VIEW_B])
    assert tw.dtype == np.float32 and np.array_equal(tw, WANT_TW)
    assert np.array_equal(mask, WANT_MASK)
    assert not mask[3], "a triangle no sample lands on is dropped"
    assert tw[2] == THR and not mask[2], "a maximum equal to the threshold is dropped: the comparison is strict"
    assert np.array_equal(verts, VERTS), "vertices are kept as they are"
    assert np.array_equal(faces, FACES[[0, 4, 5]]), "kept faces, in their order"
    assert ns.dtype == nv.dtype == np.int64
    assert ns.tolist() == [5, 5]
    assert nv.tolist() == [2, 3]          # A: 0.2, 0.5 (the threshold itself is not above it); B: 0.25, 0.75, 0.1


def test_view_order_does_not_matter():
    a = ref.prune(VERTS, FACES, [VIEW_A, VIEW_B])
    b = ref.prune(VERTS, FACES, [VIEW_B, VIEW_A])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])
    assert a[4].tolist() == b[4].tolist()[::-1] and a[5].tolist() == b[5].tolist()[::-1]


def test_prune_faces_takes_weights_or_a_mask():
    from quadraturefields_amd import baking
    from quadraturefields_amd.mesh_io import TriMesh
    import torch
    uv = np.linspace(0, 1, 14).reshape(7, 2)
    mesh = TriMesh(VERTS, FACES, uv)
    for arg in (WANT_TW, torch.from_numpy(WANT_TW), WANT_MASK, torch.from_numpy(WANT_MASK)):
        got = baking.prune_faces(mesh, arg, 1e-3)
        assert np.array_equal(got.faces, FACES[WANT_MASK]) and got.faces.dtype == np.int64
        assert np.array_equal(got.vertices, VERTS) and np.array_equal(got.visual.uv, uv)
    assert np.array_equal(mesh.faces, FACES), "the input mesh is not modified"


def test_the_four_files_round_trip(tmp_path):
    from quadraturefields_amd import pruning
    from quadraturefields_amd.mesh_io import TriMesh, load_mesh
    import torch
    tw, mask, _, faces, ns, nv = ref.prune(VERTS, FACES, [VIEW_A, VIEW_B])
    out = str(tmp_path / "mesh_dir")
    pruned = pruning.write_pruning_files(out, TriMesh(VERTS, FACES), torch.from_numpy(tw), ns, nv, threshold=1e-3)
    assert sorted(os.listdir(out)) == sorted(pruning.FILES) == ["mesh_updated.ply", "num_samples.npy",
                                                                 "num_valid_samples.npy", "triangle_weights.npy"]
    got_tw = np.load(os.path.join(out, "triangle_weights.npy"))
    assert got_tw.dtype == np.float32 and got_tw.shape == (6,) and np.array_equal(got_tw, tw)
    for name, want in (("num_samples.npy", ns), ("num_valid_samples.npy", nv)):
        got = np.load(os.path.join(out, name))
        assert got.dtype == np.int64 and got.shape == (2,) and np.array_equal(got, want)
    mesh = load_mesh(os.path.join(out, "mesh_updated.ply"))
    assert np.array_equal(mesh.faces, faces) and np.array_equal(pruned.faces, faces)
    assert mesh.vertices.shape == VERTS.shape and np.array_equal(mesh.vertices, VERTS)    # small integers: exact in fp32
