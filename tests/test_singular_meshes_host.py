"""Host: the lattice-aligned fixtures of tests/singular_meshes.py are what they claim, shown with the oracle alone.

For every mesh x ray family that tests/test_gpu_singular_rays.py uses, a numpy restatement of ``mt_hit`` in the same
operation order (``singular_meshes.mt_events``) counts the accepted hits with u == 0, v == 0, u + v == 1, a bit-equal t
neighbour, and the (ray, face) pairs with det == 0.  Each count a family exists for must be positive; the restatement,
the brute force and the oracle's BVH walk agree bit for bit; the brute force's list (128) is longer than its largest
count, so "every hit" is honest; and the restatement with strict inequalities gives another answer on every family that
has a hit at all -- a kernel that is wrong on the boundary cannot pass.  The counts are printed (``pytest -s``).
"""
import numpy as np
import pytest

from oracle import meshpath as om
from tests import singular_meshes as sm

ALL = 128
MESH_NAMES = list(sm.MESHES)


def test_the_meshes_are_what_they_claim():
    v, f, _ = sm.mesh("voxel_ball")
    assert v.shape == (722, 3) and f.shape == (1440, 3)
    assert np.array_equal(v * 8, np.round(v * 8)) and np.abs(v).max() <= 1           # every coordinate k / 8
    tri = v[f]
    normal = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert ((normal != 0).sum(axis=1) == 1).all()                                     # every face in an axis plane
    assert (np.einsum("ij,ij->i", normal, tri.mean(axis=1)) > 0).all()                # wound outwards

    v, f, _ = sm.mesh("stacked_planes")
    tri = v[f]
    assert (tri[:, :, 2].max(axis=1) == tri[:, :, 2].min(axis=1)).all()               # flat: a leaf box has no thickness
    z = np.unique(v[:, 2])
    assert z.size == 6 and np.array_equal(np.diff(z), np.full(5, sm.PLANE_SPACING, np.float32))
    assert np.array_equal(v * 8, np.round(v * 8))

    v, f, _ = sm.mesh("fan")
    assert f.shape == (96, 3) and np.array_equal(v * 64, np.round(v * 64))
    valence = np.bincount(f.reshape(-1), minlength=v.shape[0])
    assert sorted(valence)[-2:] == [48, 48]
    for slot in range(3):                                                             # the apex takes every corner slot
        assert (f[:, slot] == 0).any() and (f[:, slot] == 49).any()

    v, f, _ = sm.mesh("mc_ball")
    assert 500 < f.shape[0] < 6000
    lattice = np.array_equal((v * 8)[:, 0], np.round(v * 8)[:, 0])
    on_lattice = (v * 8 == np.round(v * 8))
    assert (on_lattice.sum(axis=1) >= 2).all()                                        # a vertex lies on a lattice edge
    assert (on_lattice.sum(axis=1) == 3).sum() >= 6 + 24                              # (5,0,0) and (3,4,0) and their images
    assert not lattice                                                                # ... and most are not lattice points


@pytest.mark.parametrize("name", MESH_NAMES)
def test_the_junk_is_junk(name):
    v0, f0, _ = sm.mesh(name)
    v, f, junk = sm.mesh(name, junk=True)
    assert np.array_equal(v[:v0.shape[0]], v0) and np.array_equal(f[:f0.shape[0]], f0)
    tri = v.astype(np.float64)[f]
    area = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    assert (area[junk.zero_area] == 0).all()
    # (marching cubes makes zero-area faces of its own where a vertex lands on a lattice point: the other meshes have none)
    assert ((area[:f0.shape[0]] == 0).sum() > 0) == (name == "mc_ball")
    two_equal, collinear = f[junk.zero_area]
    assert len(set(two_equal.tolist())) == 2 and len(set(collinear.tolist())) == 3
    a, b = junk.twin
    assert f[b].tolist() == [f[a, 0], f[a, 2], f[a, 1]]
    assert not (f == junk.unreferenced).any() and (np.abs(v[junk.unreferenced]) > 1).all()


_SEEN = {}


def _record(name, family):
    """(events, brute-force lists) of one mesh (with junk) x family, computed once."""
    if (name, family) not in _SEEN:
        v, f, junk = sm.mesh(name, junk=True)
        o, d = sm.rays(name, family, junk=True)
        ev = sm.mt_events(v, f, o, d)
        lists = om.BruteForceIntersector(v, f, min_separation=0).hits(o, d, ALL)
        _SEEN[(name, family)] = (ev, lists)
    return _SEEN[(name, family)]


@pytest.mark.parametrize("family", sm.FAMILIES)
@pytest.mark.parametrize("name", MESH_NAMES)
def test_every_family_sits_on_its_boundaries(name, family):
    v, f, junk = sm.mesh(name, junk=True)
    o, d = sm.rays(name, family, junk=True)
    assert o.shape[0] <= 10000 and o.dtype == np.float32 and d.dtype == np.float32
    ev, (tri, t, cnt) = _record(name, family)
    print("\nEVENTS %-14s %-8s rays %5d max/ray %3d %s" % (name, family, o.shape[0], cnt.max(), ev.counts))
    for what in sm.FAMILY_EVENTS[family]:
        assert ev.counts[what] > 0, what
    # "every hit" is honest, and the restatement IS the brute force
    assert cnt.max() < ALL
    r_tri, r_t, r_cnt = sm.lists_from_events(ev, ALL)
    assert np.array_equal(r_cnt, cnt) and np.array_equal(r_tri, tri) and np.array_equal(r_t, t)
    # no ray reports a zero-area face
    assert not np.isin(tri, junk.zero_area).any()
    # the oracle's own BVH walk
    for min_sep in (0, "trimesh"):
        brute = om.BruteForceIntersector(v, f, min_separation=min_sep).hits(o, d, ALL)
        walk = om.BVHIntersector(v, f, min_separation=min_sep).hits(o, d, ALL)
        assert all(np.array_equal(x, y) for x, y in zip(brute, walk))
        assert brute[2].max() < ALL
    # strict inequalities change the answer (the all-zero direction has no hit to lose: it exists for det == 0)
    strict = sm.mt_events(v, f, o, d, strict=True)
    if family == "zero":
        assert ev.counts["hits"] == 0 and strict.counts["hits"] == 0 and ev.counts["det0"] == o.shape[0] * f.shape[0]
    else:
        assert not np.array_equal(strict.hit, ev.hit)
        assert strict.counts["hits"] < ev.counts["hits"]


def test_zero_components_carry_both_signs():
    o, d = sm.rays("voxel_ball", "axis")
    zero = d == 0
    assert (zero.sum(axis=1) == 2).all()
    assert np.signbit(d[zero]).any() and (~np.signbit(d[zero])).any()
    o, d = sm.rays("voxel_ball", "tiny")
    mags = np.sort(np.abs(d), axis=1)
    assert (mags[:, 0] == np.float32(1e-35)).all() and (mags[:, 1] == np.float32(1e-20)).all() and (mags[:, 2] == 1).all()
    assert np.float32(1e-35) < np.float32(1e-30) and np.float32(1e-35) > np.finfo(np.float32).tiny      # a normal number
    o, d = sm.rays("voxel_ball", "diagonal")
    nz = np.sort(np.abs(d), axis=1)
    assert (nz[:, 0] == 0).all() and (nz[:, 1] == nz[:, 2]).all()


@pytest.mark.parametrize("pose", ["corners", "centres"])
def test_axis_cameras_put_lattice_vertices_on_pixel_corners_and_centres(pose):
    cams = sm.axis_cameras(pose)
    assert len(cams) == 6
    v, _, _ = sm.mesh("voxel_ball")
    for c2w in cams:
        rot, pos = c2w[:, :3].astype(np.float64), c2w[:, 3].astype(np.float64)
        assert np.isin(rot, [0.0, 1.0, -1.0]).all() and np.array_equal(rot.T @ rot, np.eye(3))
        assert np.isclose(np.linalg.det(rot), 1.0)
        pc = (v.astype(np.float64) - pos) @ rot
        mid = pc[:, 2] == -sm.CAM_DIST                                                # the lattice plane through the origin
        assert mid.sum() >= 48
        sx = sm.CAM_FOCAL * pc[mid, 0] / sm.CAM_DIST + sm.CAM_W / 2.0                 # exact: powers of two and k / 8
        sy = -sm.CAM_FOCAL * pc[mid, 1] / sm.CAM_DIST + sm.CAM_H / 2.0
        frac = 0.0 if pose == "corners" else 0.5
        assert np.array_equal(sx - np.floor(sx), np.full(sx.shape, frac))
        assert np.array_equal(sy - np.floor(sy), np.full(sy.shape, frac))


@pytest.mark.parametrize("name", ["voxel_ball", "mc_ball", "stacked_planes"])
def test_camera_frames_stay_below_the_list_length(name):
    import torch
    from quadraturefields_amd import synthetic
    v, f, _ = sm.mesh(name, junk=True)
    brute, walk = om.BruteForceIntersector(v, f, min_separation=0), om.BVHIntersector(v, f, min_separation=0)
    for pose in ("corners", "centres"):
        for i, c2w in enumerate(sm.axis_cameras(pose)):
            o, d = synthetic.camera_rays(torch.from_numpy(c2w), sm.CAM_FOCAL, sm.CAM_W, sm.CAM_H)
            o, d = o.numpy(), d.numpy()
            tri, t, cnt = brute.hits(o, d, ALL)
            assert 0 < cnt.max() < ALL
            assert all(np.array_equal(x, y) for x, y in zip((tri, t, cnt), walk.hits(o, d, ALL)))
            ties = int(((t[:, 1:] == t[:, :-1]) & np.isfinite(t[:, 1:])).sum())
            print("\nCAMERA %-14s %-7s %d: rays hit %5d, max/ray %3d, bit-equal t neighbours %d" % (
                name, pose, i, int((cnt > 0).sum()), cnt.max(), ties))
