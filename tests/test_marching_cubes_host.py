"""CPU: the numpy restatement of the marching-cubes rules (tests/marching_cubes_reference.py) on hand-derived cases and
mesh invariants, and the argument checks of ``mc_utils.marching_cubes`` / ``qf_marching_cubes_*`` that fire before
any device use."""
import itertools

import numpy as np
import pytest
import torch

from tests import marching_cubes_reference as ref


def _cell(inside, values=None):
    """A 2x2x2 volume: corner c (= d0 | d1 << 1 | d2 << 2) is +1 if inside, -1 otherwise (or values[c])."""
    v = np.empty((2, 2, 2), np.float32)
    for c in range(8):
        v[c & 1, (c >> 1) & 1, (c >> 2) & 1] = (values[c] if values is not None else (1.0 if c in inside else -1.0))
    return v


def _directed_edges(faces):
    return np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])


def test_one_inside_corner_gives_one_outward_triangle():
    v = _cell([], [3, -1, -1, -1, -1, -1, -1, -1])        # corner 0 inside: t = 3 / 4 on its three edges
    verts, faces = ref.marching_cubes(v, 0.0)
    assert verts.tolist() == [[0.75, 0, 0], [0, 0.75, 0], [0, 0, 0.75]]
    assert faces.tolist() == [[0, 1, 2]]
    n = np.cross(verts[1] - verts[0], verts[2] - verts[0])
    assert (n > 0).all()                                   # away from the inside corner


def test_inside_edge_gives_two_triangles():
    verts, faces = ref.marching_cubes(_cell([0, 1]), 0.0)  # the axis-0 edge at the origin
    assert len(verts) == 4 and len(faces) == 2
    assert len(np.unique(faces)) == 4
    assert all(v[0] in (0.0, 1.0) for v in verts)         # the crossed edges run along axes 1 and 2


@pytest.mark.parametrize("ap,aq,ar,as_,joined", [(2, 2, -1, -1, True), (1, 1, -2, -2, False), (2, 1, -1, -2, False),
                                                  (3, 1, -1, -2, True)])
def test_ambiguous_face_decider(ap, aq, ar, as_, joined):
    """Face axis 2 low (corners 0, 2, 3, 1): 0 and 3 inside.  Inside corners 4..7 close nothing off, so the decider
    of this face alone decides whether 0 and 3 are joined (one loop) or separated (two).  The tie a_p a_q = a_r a_s
    (2 * 1 = -1 * -2) separates them."""
    vals = [ap, ar, as_, aq, -5, -5, -5, -5]
    verts, faces = ref.marching_cubes(_cell([], vals), 0.0)
    assert len(verts) == 6                                  # 3 crossed edges at each inside corner
    assert len(faces) == (4 if joined else 2)               # one loop of 6 edges, or two of 3
    assert ref.cell_loops(0b1001, [0] * 6) != ref.cell_loops(0b1001, [0, 0, 0, 0, 1, 0])


def test_corner_at_the_level_merges():
    """Corner 0 exactly at the level (outside, a = 0); corners 1, 2, 4 inside: the three edges from corner 0 land on
    grid point 0 and share one vertex, listed first."""
    v = _cell([], [0, 1, 1, -1, 1, -1, -1, -1])
    verts, faces = ref.marching_cubes(v, 0.0)
    assert verts[0].tolist() == [0, 0, 0]
    assert (verts[1:] != 0).any(1).all()
    used = faces.reshape(-1)
    assert (used == 0).sum() >= 1
    assert len(np.unique(verts, axis=0)) == len(verts)


def test_non_cubic_shape():
    rng = np.random.default_rng(3)
    v = rng.normal(size=(2, 3, 7)).astype(np.float32)
    verts, faces = ref.marching_cubes(v, 0.1)
    assert verts.shape[1] == 3 and faces.max() < len(verts)
    assert (verts.max(0) <= [1, 2, 6]).all() and (verts.min(0) >= 0).all()


def test_all_256_patterns_give_closed_loops():
    for bits in range(256):
        for join in itertools.product([0, 1], repeat=6):
            loops = ref.cell_loops(bits, join)
            edges = [e for lp in loops for e in lp]
            inside = [(bits >> c) & 1 for c in range(8)]
            crossed = [e for e in range(12)
                       if inside[ref.edge_lower_corner(e)] != inside[ref.edge_lower_corner(e) | (1 << (e >> 2))]]
            assert sorted(edges) == crossed, (bits, join)
            assert all(len(lp) >= 3 for lp in loops)
            if not any(join):
                break                                       # join only matters on ambiguous faces; spot-check below
    for bits in (0b10010110, 0b01101001, 0b10000001, 0b00100100):
        for join in itertools.product([0, 1], repeat=6):
            loops = ref.cell_loops(bits, join)
            assert sorted(e for lp in loops for e in lp) == sorted(set(e for lp in loops for e in lp))


def _balanced(faces):
    """Every directed edge (u, v) appears as often as (v, u)."""
    d = _directed_edges(faces).astype(np.int64)
    fwd, cf = np.unique(d[:, 0] * (1 << 32) + d[:, 1], return_counts=True)
    rev, cr = np.unique(d[:, 1] * (1 << 32) + d[:, 0], return_counts=True)
    return np.array_equal(fwd, rev) and np.array_equal(cf, cr)


def test_closed_on_padded_random_volume():
    """±U[1,3] inside a -1 pad: t in [1/4, 3/4], nothing merges, and the surface is closed: directed edges balance.
    A directed edge may appear twice: a fan diagonal across an ambiguous face can join the same two vertices as the
    neighbouring cell's fan diagonal.  Nothing else repeats."""
    rng = np.random.default_rng(0)
    v = -np.ones((18, 17, 16), np.float32)
    inner = rng.uniform(1, 3, size=(16, 15, 14)) * rng.choice([-1, 1], size=(16, 15, 14))
    v[1:-1, 1:-1, 1:-1] = inner
    verts, faces = ref.marching_cubes(v, 0.0)
    assert _balanced(faces)
    _, cnt = np.unique(np.sort(_directed_edges(faces), 1), axis=0, return_counts=True)
    assert set(cnt.tolist()) <= {2, 4} and (cnt == 2).mean() > 0.98
    assert len(np.unique(verts, axis=0)) == len(verts)
    assert len(np.unique(faces)) == len(verts)


def test_smooth_ball_is_a_two_manifold():
    """No ambiguous face: every directed edge once, every undirected edge in exactly two faces."""
    verts, faces = ref.marching_cubes(_ball(40, 15.3), 0.0)
    d = _directed_edges(faces)
    assert len(np.unique(d, axis=0)) == len(d)
    _, cnt = np.unique(np.sort(d, 1), axis=0, return_counts=True)
    assert (cnt == 2).all()


def _ball(n, r, c=None):
    c = [(n - 1) / 2] * 3 if c is None else c
    x = np.indices((n, n, n)).astype(np.float64) - np.asarray(c, np.float64).reshape(3, 1, 1, 1)
    return (r - np.sqrt((x ** 2).sum(0))).astype(np.float32)


def test_euler_characteristic():
    assert ref.euler_characteristic(*ref.marching_cubes(_ball(32, 10.3), 0.0)) == 2
    two = np.maximum(_ball(40, 7.2, (12, 12, 12)), _ball(40, 7.2, (27, 27, 27)))
    assert ref.euler_characteristic(*ref.marching_cubes(two, 0.0)) == 4
    x = np.indices((48, 48, 48)).astype(np.float64) - 23.5
    rho = np.sqrt(x[0] ** 2 + x[1] ** 2)
    torus = (5.1 - np.sqrt((rho - 13.0) ** 2 + x[2] ** 2)).astype(np.float32)
    assert ref.euler_characteristic(*ref.marching_cubes(torus, 0.0)) == 0


def test_signed_volume_of_a_ball():
    r = 11.4
    vol = ref.signed_volume(*ref.marching_cubes(_ball(32, r), 0.0))
    exact = 4 / 3 * np.pi * r ** 3
    assert vol > 0 and abs(vol - exact) / exact < 0.01


def test_host_tensor_is_refused():
    from quadraturefields_amd import mc_utils
    with pytest.raises(ValueError):
        mc_utils.marching_cubes(torch.zeros(4, 4, 4), 0.0)     # host tensor: no CPU fallback


def test_workspace_bytes_refuses_sizes(lib):
    assert lib.qf_marching_cubes_workspace_bytes(1, 4, 4) == -1
    assert lib.qf_marching_cubes_workspace_bytes(4, 4, 1) == -1
    assert lib.qf_marching_cubes_workspace_bytes(2, 1 << 15, 1 << 15) == -1          # 2^31 points
    assert lib.qf_marching_cubes_workspace_bytes((1 << 24) + 1, 2, 2) == -1
    assert lib.qf_marching_cubes_workspace_bytes(1024, 1024, 1024) >= 4 * 1024 ** 3
    assert lib.qf_marching_cubes_workspace_bytes(1024, 1024, 1024) <= 4 * 1024 ** 3 + 2 * 24 * 1024 ** 3 // 4096


def test_entry_points_refuse_bad_arguments_before_any_launch(lib):
    from quadraturefields_amd import _C
    fake = _C.c_void_p(256)                                  # never dereferenced: every call below fails its checks
    ws_bytes = lib.qf_marching_cubes_workspace_bytes(4, 4, 4)
    bad = -1
    assert lib.qf_marching_cubes_count(None, 4, 4, 4, 0.0, fake, ws_bytes, fake, None) == bad
    assert lib.qf_marching_cubes_count(fake, 4, 4, 4, 0.0, fake, ws_bytes - 1, fake, None) == bad
    assert lib.qf_marching_cubes_count(fake, 4, 4, 4, float("nan"), fake, ws_bytes, fake, None) == bad
    assert lib.qf_marching_cubes_count(fake, 4, 1, 4, 0.0, fake, ws_bytes, fake, None) == bad
    assert lib.qf_marching_cubes_count(fake, 4, 4, 4, 0.0, None, ws_bytes, fake, None) == bad
    assert lib.qf_marching_cubes_count(fake, 4, 4, 4, 0.0, fake, ws_bytes, None, None) == bad
    assert lib.qf_marching_cubes_emit(fake, 4, 4, 4, 0.0, fake, ws_bytes, None, 3, fake, 1, None) == bad
    assert lib.qf_marching_cubes_emit(fake, 4, 4, 4, 0.0, fake, ws_bytes, fake, 3, None, 1, None) == bad
    assert lib.qf_marching_cubes_emit(fake, 4, 4, 4, 0.0, fake, ws_bytes, fake, 1 << 31, fake, 1, None) == bad
    assert lib.qf_marching_cubes_emit(fake, 4, 4, 4, 0.0, fake, ws_bytes, fake, -1, fake, 1, None) == bad
    assert lib.qf_marching_cubes_emit(fake, 4, 4, 4, float("inf"), fake, ws_bytes, fake, 3, fake, 1, None) == bad
    assert lib.qf_marching_cubes_emit(fake, 4, 4, 4, 0.0, fake, ws_bytes, fake, 0, fake, 0, None) == 0   # nothing
