"""GPU: intersection and packing on the lattice-aligned meshes, rays and cameras of tests/singular_meshes.py, where u == 0,
v == 0, u + v == 1, det == 0, bit-equal t on several triangles, zero direction components and hits exactly min_sep apart
happen on most rays (tests/test_singular_meshes_host.py counts them).  Every comparison is bit-exact against the brute
force that returns every hit (``oracle.meshpath.BruteForceIntersector``, list length 128); no tolerance appears anywhere.

(a) the general traversal, both builders, both instantiations of ``oct_traverse_ray``, with list pages; (b) refit and
rebuild to a moved lattice; (c) every camera-coherent pass through the C ABI with the harness of
tests/test_gpu_raster_passes.py (sentinel-filled outputs, raw counts, no repair); (d) the packs on those tie-laden lists;
(e) one frame through the default policy.
"""
import functools
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import meshpath as om
from tests import singular_meshes as sm
from tests.test_gpu_raster_passes import (ALL, _apply_rule, _call, _check_plain, _check_selected, _keys, _nearest,
                                          _sorted_rows)

pytestmark = pytest.mark.gpu

MESH_NAMES = list(sm.MESHES)
KS = [1, 3, 25, 64]
SPACING = sm.PLANE_SPACING
MIN_SEPS = ["0", "trimesh", "spacing", "spacing+", "spacing-"]
SAMPLE_NAMES = ["xyzs", "dirs", "index_ray", "ts", "index_tri", "origins"]


def _min_sep(name, which):
    """The re-origin distances of the cases: 0, trimesh's, exactly the plane spacing and the spacing x (1 +- 2^-20)."""
    v = sm.mesh(name, True)[0]
    return {"0": 0.0, "trimesh": om.trimesh_ray_offset(v), "spacing": SPACING, "spacing+": SPACING * (1.0 + 2.0 ** -20),
            "spacing-": SPACING * (1.0 - 2.0 ** -20)}[which]


# ------------------------------------------------------------------------------------------------ shared state
def _to(a, device):
    """A host array (the shared ones are read-only: copied) as a device tensor."""
    return torch.from_numpy(np.array(a)).to(device)


_TRUTH = {}


def _truth(mesh_key, rays_key, v, f, o, d, min_sep):
    """The brute force's (tri, t, cnt) at list length 128, once per (mesh, rays, rule), read-only."""
    key = (mesh_key, rays_key, float(np.float32(min_sep)))
    if key not in _TRUTH:
        tri, t, cnt = om.BruteForceIntersector(v, f, min_separation=min_sep).hits(o, d, ALL)
        assert cnt.max(initial=0) < ALL
        for a in (tri, t, cnt):
            a.setflags(write=False)
        _TRUTH[key] = SimpleNamespace(tri=tri, t=t, cnt=cnt, _dev=None)
    return _TRUTH[key]


def _first(T, k):
    """The brute force asked for ``k`` hits: the chain's first k kept hits (a prefix of its longer list)."""
    return SimpleNamespace(tri=T.tri[:, :k], t=T.t[:, :k], cnt=np.minimum(T.cnt, k))


def _truth_dev(T, device):
    if T._dev is None:
        T._dev = tuple(_to(a, device) for a in (T.tri, T.t, T.cnt))
    return T._dev


_HANDLES = {}


def _ri(name, builder="host", fresh=False, **kw):
    from quadraturefields_amd.mesh_io import TriMesh
    from quadraturefields_amd.mesh_utils import RayIntersector
    v, f, _ = sm.mesh(name, True)
    if fresh:
        return RayIntersector(TriMesh(v, f), builder=builder, **kw)
    if (name, builder) not in _HANDLES:
        _HANDLES[(name, builder)] = RayIntersector(TriMesh(v, f), max_hits=25, min_separation=0, builder=builder)
    return _HANDLES[(name, builder)]


def _ordered(lib, ri, k):
    """``bvh_launch``'s rule, restated: front-to-back child order iff the mesh's depth complexity (fp32) >= K / 2."""
    dc = np.float32(lib.qf_bvh_depth_complexity(ri._handle))
    return bool(dc >= np.float32(0.5) * np.float32(k))


def _pages(T0, k, min_sep):
    """Rays whose first list page (the K nearest) is full while the chain keeps fewer than K of it: the traversal has to
    run again behind the page.  -> (rays that page, rays among them whose first page keeps one hit only)."""
    keys = _sorted_rows(T0.t[:, :k], T0.tri[:, :k], T0.cnt)[0]
    _, kept = _apply_rule(keys, np.minimum(T0.cnt, k), min_sep)
    paging = (T0.cnt > k) & (kept < k)
    return int(paging.sum()), int((paging & (kept == 1)).sum())


# ------------------------------------------------------------------------------------------------ (a) general traversal
@pytest.mark.parametrize("builder", ["host", "device"])
@pytest.mark.parametrize("name", MESH_NAMES)
def test_general_traversal_on_every_family(device, lib, name, builder):
    """``RayIntersector.hits`` == the brute force, bit for bit: every family, K, re-origin distance, plain batch and the
    tile-ordered ``image_width = 64``.  (Scaled directions: min_sep = 0 only, see the ``RayIntersector`` docstring.)"""
    v, f, junk = sm.mesh(name, True)
    ri = _ri(name, builder)
    assert int(lib.qf_bvh_num_triangles(ri._handle)) == f.shape[0]
    junk_dev = _to(junk.zero_area.astype(np.int32), device)
    paged = {}
    for family in sm.FAMILIES:
        o, d = sm.rays(name, family, True)
        o_dev, d_dev = _to(o, device), _to(d, device)
        T0 = _truth(name, family, v, f, o, d, 0.0)
        for which in MIN_SEPS:
            if family == "scaled" and which != "0":
                continue
            ms = _min_sep(name, which)
            T = _truth(name, family, v, f, o, d, ms)
            t_tri, t_t, t_cnt = _truth_dev(T, device)
            ri.set_min_separation(ms)
            for k in KS:
                if ms > 0 and family == "axis":
                    paged[(which, k)] = _pages(T0, k, ms)
                for width in (0, 64):
                    n = o.shape[0] if width == 0 else o.shape[0] // 64 * 64
                    if n == 0:
                        continue
                    tri, t, cnt, _, _ = ri.hits(o_dev[:n], d_dev[:n], k, image_width=width)
                    what = (name, builder, family, which, k, width)
                    assert ri.last_route == "bvh"
                    assert torch.equal(cnt, t_cnt[:n].clamp(max=k)), what
                    assert torch.equal(tri, t_tri[:n, :k]), what
                    assert torch.equal(t, t_t[:n, :k]), what                  # (+inf padding included)
                    assert not torch.isin(tri, junk_dev).any(), what
    ri.set_min_separation(0.0)
    print("\nPAGING %s/%s (axis rays; rays that page, of them keeping one hit of the first page):" % (name, builder), paged)
    if name in ("fan", "stacked_planes"):
        # the list fills with equal (fan: 48 triangles at the apex) or near-equal t (planes exactly min_sep apart) and
        # the chain drops most of it: the traversal must page
        for which in ("spacing", "spacing+") if name == "stacked_planes" else ("trimesh", "spacing"):
            assert paged[(which, 3)][0] > 0 and paged[(which, 3)][1] > 0, (which, paged)


def test_the_cases_take_both_traversal_instantiations(device, lib):
    """``bvh_launch`` picks ``oct_traverse_ray<true>`` when the handle's depth complexity is at least K / 2.  The stacked
    planes (2 area / box area = 3.7) and the voxel ball (1.67) are ordered at K = 1 and 3 and unordered at 25 and 64; the
    marching-cubes ball (1.03) and the fan (0.85) are ordered at K = 1 only -- the balls with K = 25 take the other
    instantiation.  No case sits near the threshold, and the two builders agree.  (The handle sees the triangles: the
    unreferenced vertex does not stretch its box.)"""
    from quadraturefields_amd.mesh_utils import mesh_depth_complexity
    taken = {}
    for name in MESH_NAMES:
        v, f, _ = sm.mesh(name, True)
        used = np.unique(f)
        want = mesh_depth_complexity(v[used], np.searchsorted(used, f))
        for builder in ("host", "device"):
            ri = _ri(name, builder)
            dc = float(lib.qf_bvh_depth_complexity(ri._handle))
            assert abs(dc - want) <= 1e-4 * want, (name, builder, dc, want)
            for k in KS:
                assert abs(dc - 0.5 * k) > 0.01 * k
                taken[(name, builder, k)] = _ordered(lib, ri, k)
    print("\nORDERED", {k: v for k, v in taken.items() if k[1] == "host"})
    for builder in ("host", "device"):
        assert taken[("stacked_planes", builder, 1)] and taken[("stacked_planes", builder, 3)]
        assert taken[("voxel_ball", builder, 3)] and taken[("fan", builder, 1)] and not taken[("fan", builder, 3)]
        assert not taken[("stacked_planes", builder, 25)] and not taken[("stacked_planes", builder, 64)]
        assert not taken[("voxel_ball", builder, 25)] and not taken[("mc_ball", builder, 25)]
    assert set(taken.values()) == {True, False}


# ------------------------------------------------------------------------------------------------ (b) refit
MOVE_SHIFT = np.array([0.25, -0.5, 1.0], dtype=np.float32)            # multiples of every mesh's lattice pitch


@pytest.mark.parametrize("builder", ["host", "device"])
@pytest.mark.parametrize("name", MESH_NAMES)
def test_refit_and_rebuild_to_a_moved_lattice(device, lib, name, builder):
    """Vertices scaled by 2 and shifted by lattice multiples (exact in fp32: the mesh stays lattice-aligned), rays moved
    with them: the device refit, the host refit, a fresh intersector and ``rebuild`` all give the brute force's lists on
    the moved mesh, rule off and with hits exactly min_sep apart (the moved planes are 2 x spacing apart)."""
    from quadraturefields_amd.mesh_io import TriMesh
    from quadraturefields_amd.mesh_utils import RayIntersector
    v, f, _ = sm.mesh(name, True)
    moved = (v * np.float32(2.0) + MOVE_SHIFT).astype(np.float32)
    assert np.array_equal(moved.astype(np.float64), v.astype(np.float64) * 2.0 + MOVE_SHIFT.astype(np.float64))
    k = 25
    batches = []
    for family in ("axis", "diagonal", "surface", "tiny"):
        o, d = sm.rays(name, family, True)
        o2 = (o * np.float32(2.0) + MOVE_SHIFT).astype(np.float32)
        batches.append((family, o2, d, _to(o2, device), _to(d, device)))
    fresh = RayIntersector(TriMesh(moved, f), max_hits=k, min_separation=0, builder=builder)
    ri = _ri(name, builder, fresh=True, max_hits=k, min_separation=0)

    def check(who, intersector):
        for ms in (0.0, 2.0 * SPACING):
            intersector.set_min_separation(ms)
            for family, o2, d, o_dev, d_dev in batches:
                T = _truth((name, "moved"), family, moved, f, o2, d, ms)
                t_tri, t_t, t_cnt = _truth_dev(T, device)
                tri, t, cnt, _, _ = intersector.hits(o_dev, d_dev, k)
                what = (who, name, builder, family, ms)
                assert torch.equal(cnt, t_cnt.clamp(max=k)), what
                assert torch.equal(tri, t_tri[:, :k]) and torch.equal(t, t_t[:, :k]), what

    check("fresh", fresh)
    ri.update_intersector(_to(moved, device))        # qf_bvh_refit_device
    check("device refit", ri)
    ri.update_intersector(v)                                         # back, through the host refit ...
    ri.update_intersector(moved)                                     # ... and there again (qf_bvh_refit)
    check("host refit", ri)
    ri.rebuild(_to(moved, device))
    check("rebuild", ri)
    ri.update_intersector(_to(moved, device))        # a refit of the rebuilt tree
    check("refit after rebuild", ri)


# ------------------------------------------------------------------------------------------------ cameras
@functools.lru_cache(maxsize=None)
def _cview(i, pose, w=sm.CAM_W, h=sm.CAM_H):
    """Axis camera ``i`` of ``pose`` as the view record of tests/test_gpu_raster_passes.py (rays made on the host)."""
    from quadraturefields_amd import synthetic
    from quadraturefields_amd.mesh_utils import make_camera
    c2w = torch.from_numpy(sm.axis_cameras(pose)[i])
    o, d = synthetic.camera_rays(c2w, sm.CAM_FOCAL, w, h)
    return SimpleNamespace(key=("axis camera", i, pose, w, h), c2w=c2w.numpy().astype(np.float64), c2w_t=c2w, focal=sm.CAM_FOCAL,
                           w=w, h=h, n=w * h, cam=make_camera(c2w, sm.CAM_FOCAL, w, h), o=o.numpy(), d=d.numpy(), _dev=None)


CAMERAS = [(i, pose) for pose in ("corners", "centres") for i in range(6)]
CAMERA_MESHES = ["voxel_ball", "mc_ball", "stacked_planes"]


def _rule(name):
    """The rule-on distance of the camera cases: exactly the plane spacing for the planes (an axis camera's central
    rays meet the layers that far apart), trimesh's for the balls."""
    return SPACING if name == "stacked_planes" else _min_sep(name, "trimesh")


def _check_tiles(out, T, view, k):
    """qf_raster_intersect_tiles, no bin past its capacity: the cursors count every candidate, the counts are the brute
    force's, the mask marks the pixels beyond K and a bin's records are exactly the hits of its tile's pixels."""
    w, h = view.w, view.h
    assert out.flag == 0
    tiles_x, tiles_y = (w + 7) // 8, (h + 7) // 8
    per_tile = lambda a: a.reshape(tiles_y, 8, tiles_x, 8).transpose(0, 2, 1, 3).reshape(tiles_y * tiles_x, 64)
    true_img = np.zeros((tiles_y * 8, tiles_x * 8), dtype=np.int64)
    true_img[:h, :w] = T.cnt.reshape(h, w)
    true_t = per_tile(true_img)
    assert np.array_equal(out.cursor, true_t.sum(axis=1))
    assert (out.cursor <= 64 * k).all()
    assert np.array_equal(out.count, T.cnt)
    assert out.overflow == int(np.maximum(T.cnt - k, 0).sum())
    bits = ((out.mask[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
    assert np.array_equal(bits, true_t > k)
    ray_of = per_tile(np.arange(tiles_y * 8 * tiles_x * 8).reshape(tiles_y * 8, tiles_x * 8))
    all_keys = _keys(T.t, T.tri)
    for tile in np.flatnonzero(out.cursor > 0):
        rec = out.bins[tile, :out.cursor[tile]]
        t_bits, word = rec & np.uint64(0xFFFFFFFF), rec >> np.uint64(32)
        pix, tri = (word & np.uint64(63)).astype(np.int64), (word >> np.uint64(6)).astype(np.int64)
        got = np.sort((pix.astype(np.uint64) << np.uint64(58)) ^ ((t_bits << np.uint64(26)) | tri.astype(np.uint64)))
        want = []
        for p in range(64):
            y, x = divmod(int(ray_of[tile, p]), tiles_x * 8)
            if y < h and x < w and T.cnt[y * w + x]:
                kk = all_keys[y * w + x, :T.cnt[y * w + x]]
                want.append((np.uint64(p) << np.uint64(58)) ^ (((kk >> np.uint64(32)) << np.uint64(26)) | (kk & np.uint64(0x3FFFFFF))))
        assert np.array_equal(got, np.sort(np.concatenate(want))), "a bin's records are exactly the hits of its tile's pixels"


@pytest.mark.parametrize("i,pose", CAMERAS)
@pytest.mark.parametrize("name", CAMERA_MESHES)
def test_every_camera_pass_on_the_axis_cameras(device, lib, name, i, pose):
    """(c) every camera-coherent pass, raw: the plain and the culled pass (K above and below the deepest pixel), the tile
    bins, the wide pass plain and culled and the depth slabs (2 and 5), rule off and on.  Every checker asserts that the
    ray flag stayed down: the pass under test produced the answer.  (d) ``qf_filter_hits`` on the plain pass's lists."""
    from quadraturefields_amd import _C
    v, f, _ = sm.mesh(name, True)
    view = _cview(i, pose)
    ri = _ri(name)
    rule = _rule(name)
    T = _truth(name, view.key, v, f, view.o, view.d, 0.0)
    Tr = _truth(name, view.key, v, f, view.o, view.d, rule)
    deepest = int(T.cnt.max())
    assert 0 < deepest <= 25 and (T.cnt > 0).sum() > 300
    assert (Tr.cnt < T.cnt).any()                                    # the rule has something to drop
    for cull in (0, 1):
        _check_plain(_call(lib, ri, view, 25, "plain", cull=cull), T, 25)
        _check_plain(_call(lib, ri, view, 25, "plain", cull=cull, sort_lists=2), T, 25, ids=False)
        if deepest > 3:
            _check_plain(_call(lib, ri, view, 3, "plain", cull=cull), T, 3)
        out = _call(lib, ri, view, 25, "plain", cull=cull, sort_lists=1, min_sep=rule)
        assert out.flag == 0 and out.overflow == 0
        assert np.array_equal(out.count, Tr.cnt) and np.array_equal(out.tri, Tr.tri[:, :25]) and np.array_equal(out.t, Tr.t[:, :25])
        # (d) the filter on the arrival-order lists: sorted, the rule applied, padded
        out = _call(lib, ri, view, 25, "plain", cull=cull, min_sep=rule)
        dv = out.dev
        _C.check(lib.qf_filter_hits(ri._handle, view.n, 25, _C.ptr(dv.tri), _C.ptr(dv.t), _C.ptr(dv.cnt), _C.stream()),
                 "qf_filter_hits")
        assert np.array_equal(dv.cnt.cpu().numpy(), Tr.cnt)
        assert np.array_equal(dv.tri.cpu().numpy(), Tr.tri[:, :25]) and np.array_equal(dv.t.cpu().numpy(), Tr.t[:, :25])
    _check_tiles(_call(lib, ri, view, 25, "tiles"), T, view, 25)
    for ms, truth_rule in ((0.0, None), (rule, Tr)):
        for k, wide in ((3, 32), (25, 40)):
            T_rule = None if truth_rule is None else _first(truth_rule, k)
            for cull in (0, 1):
                out = _call(lib, ri, view, k, "wide", cull=cull, wide=wide, min_sep=ms)
                _check_selected(out, T, T_rule, k, wide, ms, exact_overflow=True)
            for n_slabs in (2, 5):
                out = _call(lib, ri, view, k, "slabs", wide=wide, slabs=n_slabs, min_sep=ms)
                assert out.overflow == 0
                _check_selected(out, T, T_rule, k, wide, ms, exact_overflow=False)
                if k == 25 and ms == 0:
                    # K above the deepest pixel: the row IS every hit -- each one landed in exactly one slab's pass
                    assert np.array_equal(out.count, T.cnt)
                    assert np.array_equal(_sorted_rows(out.t, out.tri, out.count)[0], _nearest(T, 25))
    ri.set_min_separation(0.0)


# ---- slab edges on layer depths
SLAB_W, SLAB_H = 95, 63                      # odd: the central pixel's ray is the camera axis itself


def _slab_edges_restated(z_front, z_back, cam_z, n_slabs):
    """``slab_cull_kernel`` / ``slab_range`` / ``slab_edges`` (csrc/raster.hip) in fp32, operation by operation, for the
    camera at (0, 0, cam_z) looking down -z at planes over [-1, 1]^2 between z_back and z_front, every chunk in view.
    The chunk boxes are the triangles' exact bounds; the nearest box point is (0, 0, z_front) (some chunk holds the
    triangles around the axis), the farthest box corner (+-1, +-1, z_back)."""
    f = np.float32
    nz = f(cam_z) - f(z_front)
    dmin = f(np.sqrt(f(f(f(0) * f(0) + f(0) * f(0)) + nz * nz))) * f(0.9999)
    fx, fy, fz = f(1), f(1), f(cam_z) - f(z_back)
    dmax = f(f(np.sqrt(f(f(fx * fx + fy * fy) + fz * fz))) * f(1.0001)) + f(1e-30)
    lo, hi = f(dmin * f(0.999)), f(dmax * f(1.001))
    w = f(max(f(hi - lo), f(1e-12)) / f(n_slabs))
    return [f(lo + f(f(j) * w)) for j in range(1, n_slabs)]


@functools.lru_cache(maxsize=None)
def _slab_scene(on_edges):
    """Five planes seen by the axis camera at (0, 0, 4): the first and the last fix the slab range, the three between them
    lie EXACTLY at the depths of the inner edges 1 .. 3 of a 5-slab call (``on_edges``) or at the lattice depths."""
    z_front, z_back = 0.25, -0.375
    edges = _slab_edges_restated(z_front, z_back, sm.CAM_DIST, 5)
    if on_edges:
        inner = [float(np.float32(sm.CAM_DIST) - e) for e in edges[:3]]
        assert all(z_back < z < z_front for z in inner)
    else:
        inner = [0.125, 0.0, -0.25]
    layers = [sm.stacked_planes(1, 8, SPACING, z0=z) for z in [z_front] + inner + [z_back]]
    nv = np.cumsum([0] + [m[0].shape[0] for m in layers[:-1]])
    v = np.concatenate([m[0] for m in layers]).astype(np.float32)
    f = np.concatenate([m[1] + o for m, o in zip(layers, nv)]).astype(np.int32)
    return v, f, [np.float32(e) for e in edges]


@pytest.mark.parametrize("on_edges", [True, False])
def test_slab_edges_that_coincide_with_a_layers_depth(device, lib, on_edges):
    """The slab passes accept ``t_lo <= t < t_hi``.  With 5 slabs the three inner planes lie exactly on the edges 1 .. 3
    along the central ray (its t is bit-equal to the edge: asserted against the brute force), so that layer's hits there
    belong to the slab that STARTS at the edge, and a pass that used ``<`` on both sides, or ``<=``, would lose or double
    them.  4 slabs, and the lattice depths: edges that coincide with nothing.  Every hit lands in exactly one pass."""
    from quadraturefields_amd.mesh_io import TriMesh
    from quadraturefields_amd.mesh_utils import RayIntersector
    v, f, edges = _slab_scene(on_edges)
    view = _cview(4, "corners", SLAB_W, SLAB_H)                      # camera at (0, 0, 4), looking down -z
    assert np.array_equal(view.o[0], np.array([0, 0, sm.CAM_DIST], np.float32))
    centre = (SLAB_H // 2) * SLAB_W + SLAB_W // 2
    assert np.array_equal(np.abs(view.d[centre]), np.array([0, 0, 1], np.float32))
    key = ("slab scene", on_edges)
    T = _truth(key, view.key, v, f, view.o, view.d, 0.0)
    on_edge = np.isin(T.t.view(np.uint32), np.array(edges, np.float32).view(np.uint32)) & np.isfinite(T.t)
    print("\nSLAB EDGES", on_edges, [float(e) for e in edges], "hits with t bit-equal to an edge:", int(on_edge.sum()))
    if on_edges:
        assert on_edge[centre].sum() >= 3 * 2 and set(T.t[centre][on_edge[centre]].tolist()) == set(map(float, edges[:3]))
    else:
        assert not on_edge.any()
    ri = RayIntersector(TriMesh(v, f), max_hits=32, min_separation=0)
    for n_slabs in (5, 4, 2):
        for k, wide in ((32, 48), (3, 32)):               # (the central ray meets 5 x 6 triangles: K = 32 holds them all)
            out = _call(lib, ri, view, k, "slabs", wide=wide, slabs=n_slabs)
            assert out.overflow == 0
            _check_selected(out, T, None, k, wide, 0.0, exact_overflow=False)
            if k == 32:
                assert T.cnt.max() == 30 and np.array_equal(out.count, T.cnt)
                assert np.array_equal(_sorted_rows(out.t, out.tri, out.count)[0], _nearest(T, 32))


# ------------------------------------------------------------------------------------------------ (d) packing
def _assert_samples(got, want, what):
    """The six sample tensors against the oracle's.  Everything is compared exactly, except the order of the triangle ids
    WITHIN a group of samples of one ray with bit-equal t: the contract calls those interchangeable (exact_common.h,
    ``sort_row_32``: "equal t alone are interchangeable samples" -- position, direction and depth of such samples are
    identical), so the ids of a group are compared as a set.  -> were the ids in the oracle's order too?"""
    if want is None:
        assert got is None, what
        return True
    g = [x.cpu() for x in got]
    for i in (0, 1, 2, 3, 5):
        assert g[i].shape == want[i].shape, (what, SAMPLE_NAMES[i])
        assert torch.equal(g[i], want[i]), (what, SAMPLE_NAMES[i])
    if torch.equal(g[4], want[4]):
        return True
    ray, ts = want[2].numpy(), want[3].numpy().view(np.uint32)
    group = np.cumsum(np.r_[True, (ray[1:] != ray[:-1]) | (ts[1:] != ts[:-1])])
    a, b = g[4].numpy(), want[4].numpy()
    assert np.array_equal(a[np.lexsort((a, group))], b[np.lexsort((b, group))]), (what, "index_tri")
    return False


def _oracle_samples(v, f, o, d, k, min_sep):
    s = om.sampling_raytrace_numpy(om.BruteForceIntersector(v, f, min_separation=min_sep), d, o, k)
    return None if s is None else om.to_loader_tensors(s)


@pytest.mark.parametrize("which", ["0", "trimesh", "spacing"])
@pytest.mark.parametrize("name", MESH_NAMES)
def test_ray_major_pack_and_resort_on_tie_laden_lists(device, lib, name, which):
    """``qf_pack_samples`` behind the traversal (plain batches) and ``qf_resort_samples`` on its output, against
    ``sampling_raytrace_numpy`` / ``sampling_indexing``: sample order, ids, depths, positions."""
    _pack_and_resort(device, name, which, 25)


@pytest.mark.parametrize("which", ["0", "trimesh", "spacing"])
@pytest.mark.parametrize("name", MESH_NAMES)
def test_ray_major_pack_and_resort_on_tie_laden_lists_above_32(device, lib, name, which):
    """The same at K = 40: above 32 the pack kernel sorts its rows by insertion in LDS, no longer in the register
    networks, and these meshes have rays with up to 97 crossings, most of them tied (tests/test_gpu_long_lists.py has
    long lists without natural ties)."""
    _pack_and_resort(device, name, which, 40)


def _pack_and_resort(device, name, which, k):
    from quadraturefields_amd.mesh_utils import MeshIntersection
    from quadraturefields_amd.mesh_io import TriMesh
    v, f, _ = sm.mesh(name, True)
    ms = _min_sep(name, which)
    ri = _ri(name, "host", fresh=True, max_hits=k, min_separation=ms)
    exact = {}
    for family in ("axis", "diagonal", "surface", "tiny", "zero"):
        o, d = sm.rays(name, family, True)
        want = _oracle_samples(v, f, o, d, k, ms)
        got = ri.sample_device(_to(o, device), _to(d, device), k)
        assert ri.last_route == "bvh"
        exact[family] = _assert_samples(got, want, (name, which, family))
        if want is None or family != "axis":
            continue
        # the re-sort after a deformation: depths mirrored (8 - ts), so every ray's order reverses and its ties stay
        # ties; the sort is stable, like the oracle's lexsort
        pts, dirs, ridx, ts, tri, org = want
        depth = (8.0 - ts).to(torch.float32)
        assert ms > 0 or bool(((depth[1:] == depth[:-1]) & (ridx[1:] == ridx[:-1])).any())      # rule off: ties to keep stable
        ref = om.sampling_indexing(pts, org, dirs, ridx, depth, tri)
        mi = MeshIntersection(TriMesh(v, f), simplify_mesh=False, scale=1.0, num_intersections=k)
        dev = lambda x: x.to(device)
        out = mi.sampling_indexing(dev(pts), dev(org), dev(dirs), dev(ridx), dev(depth), dev(tri))
        for j, (a, b) in enumerate(zip(out, ref)):
            assert torch.equal(a.cpu(), b), (name, which, "resort", j)
    print("\nPACK %s %s: ids in the oracle's order on" % (name, which), exact)


def _frame_rows(frame_out, w, h):
    """A render-only frame's kept samples as sorted rows of (x, y, z, depth, tri) bit patterns."""
    from tests.test_gpu_hit_bins import _kept_index
    idx = _kept_index(frame_out, w, h)
    rows = torch.cat([frame_out["xyz"][idx], frame_out["depth"][idx][:, None]], dim=1).cpu().numpy().view(np.int32)
    rows = np.concatenate([rows, frame_out["tri"][idx].cpu().numpy()[:, None]], axis=1)
    return rows[np.lexsort(rows.T[::-1])]


@pytest.mark.parametrize("i,pose", CAMERAS)
@pytest.mark.parametrize("name", CAMERA_MESHES)
def test_frame_packs_on_the_axis_cameras(device, lib, name, i, pose):
    """(d) a camera frame's lists through ``qf_pack_samples`` (ray-major), ``qf_pack_tiles`` (per-ray lists) and
    ``qf_pack_tiles_bins`` (the tiles' bins), rule off and on.  The ray-major samples are the oracle's; the tile packs
    write the same samples in tile order: per-pixel counts and the multiset of (position, depth, id) are the oracle's."""
    from tests.test_gpu_hit_bins import _sample
    v, f, _ = sm.mesh(name, True)
    view = _cview(i, pose)
    o_dev, d_dev = _to(view.o, device), _to(view.d, device)
    k = 25
    for ms in (0.0, _rule(name)):
        ri = _ri(name, "host", fresh=True, max_hits=k, min_separation=ms)
        want = _oracle_samples(v, f, view.o, view.d, k, ms)
        got = ri.sample_device(o_dev, d_dev, k, camera=view.cam)
        assert ri.last_route == "plain" and ri.camera_mismatch_frames == 0 and ri._raster_backoff == 0
        _assert_samples(got, want, (name, i, pose, ms, "pack_samples"))
        want_rows = np.concatenate([want[0].numpy().view(np.int32), want[3].numpy().view(np.int32)[:, None],
                                    want[4].numpy().astype(np.int32)[:, None]], axis=1)
        want_rows = want_rows[np.lexsort(want_rows.T[::-1])]
        per_ray = torch.bincount(want[2], minlength=view.n).to(torch.int32)
        # (with ties and the rule on, the ray-major pack's optimistic check was refuted and the next frames would decide
        # the rule up front, which also keeps a frame off the bins: each route is put into its state explicitly)
        for route, upfront in (("bins", 0), ("lists", 0), ("lists", 8)):
            ri._rule_upfront = upfront
            out = _sample(ri, o_dev, d_dev, view.cam, route, k=k, want_tri=True)
            assert ri.last_route == ("bins" if route == "bins" else "plain")
            assert (ri.last_frame._keep[3][0] is not None) == (upfront > 0 and ms > 0)     # keep masks from the repair
            assert ri.camera_mismatch_frames == 0 and ri._raster_backoff == 0
            assert out["samples"] == want[0].shape[0], (route, ms)
            assert torch.equal(out["final_count"].cpu(), per_ray), (route, ms)
            assert np.array_equal(_frame_rows(out, view.w, view.h), want_rows), (route, ms)


# ------------------------------------------------------------------------------------------------ (e) default policy
@pytest.mark.parametrize("i,pose", CAMERAS)
def test_one_frame_through_the_default_policy(device, lib, i, pose):
    """A default ``RayIntersector`` (K = 25, trimesh's re-origin distance, host builder) on the marching-cubes ball: the
    first frame of each axis camera takes the plain camera-coherent pass, equals the brute force, and leaves the policy
    where it was -- no camera mismatch, no back-off."""
    from quadraturefields_amd.mesh_io import TriMesh
    from quadraturefields_amd.mesh_utils import RayIntersector
    v, f, _ = sm.mesh("mc_ball", True)
    view = _cview(i, pose)
    o_dev, d_dev = _to(view.o, device), _to(view.d, device)
    ri = RayIntersector(TriMesh(v, f), max_hits=25)
    assert ri.min_separation == om.trimesh_ray_offset(v)
    T = _truth("mc_ball", view.key, v, f, view.o, view.d, ri.min_separation)
    with warnings.catch_warnings():
        warnings.simplefilter("error", UserWarning)                  # (the mismatch warning would be an error here)
        tri, t, cnt, _, _ = ri.hits(o_dev, d_dev, camera=view.cam)
        assert ri.last_route == "plain"
        assert np.array_equal(cnt.cpu().numpy(), T.cnt)
        assert np.array_equal(tri.cpu().numpy(), T.tri[:, :25]) and np.array_equal(t.cpu().numpy(), T.t[:, :25])
        frame = ri.sample_frame_device(o_dev, d_dev, camera=view.cam)
        assert ri.last_route == "bins"
        assert ri.frame_samples(frame) == int(T.cnt.sum())
        assert torch.equal(frame.hit_count.cpu(), torch.from_numpy(T.cnt.copy()))
        got = ri.sample_device(o_dev, d_dev, camera=view.cam)
        assert ri.last_route == "plain"
        _assert_samples(got, _oracle_samples(v, f, view.o, view.d, 25, "trimesh"), ("default policy", i, pose))
    assert ri.camera_mismatch_frames == 0 and ri._raster_backoff == 0 and ri.repaired_frames == 0
    assert ri.raster_wide == 0
