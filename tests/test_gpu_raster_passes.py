"""GPU: every device route of the camera-coherent intersector (csrc/raster.hip), called through the C ABI with NO repair
launch, no ``RayIntersector.hits`` and no policy behind it, against the brute force that returns every hit
(``oracle.meshpath.BruteForceIntersector``, ``max_hits = 128``).

``qf_bvh_repair_overflow`` re-traverses every ray whose count exceeds K (every ray when the ray flag is up), so a pass that
wrongly reports overflow, wrongly raises its flag or hands most of the image to the repair still yields bit-identical
samples through ``RayIntersector``.  Here the raw outputs are read: counts, the overflow word, the ray flag, the lists
(ids and t bit for bit, as sets where the order is the arrival order) and the slots no hit was written to (they must
still hold the sentinel the test filled them with).  No tolerance appears anywhere.

Part 2: the chunk culling made observable (``qf_bvh_copy_visible_chunks``): must <= visible <= may against an fp64
restatement of the chunk boxes, the counter-parity scheme over consecutive calls, and the boxes after a refit.
"""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import meshpath as om

pytestmark = pytest.mark.gpu

W, H = 96, 64
SENT_TRI = -7                         # hit_tri is filled with this, hit_t with NaN, before every call
GARBAGE = 0x5A5A5A5                   # ... and the words the call has to zero (counts | overflow | ray flag) with this
ALL = 128                             # the brute force's list length: every hit of every ray of these scenes (max 24)
CHUNK = 64                            # kCullChunk
GUARD = 0.25                          # kRasterGuard
SELECT_HEADROOM = 8                   # kSelectHeadroom
RULE = 0.05                           # the re-origin distance of the rule-on cases (handle and brute force alike)
BIG = np.uint64(0xFFFFFFFFFFFFFFFF)
MOVE_SCALE = np.array([0.6, 1.3, 0.9], dtype=np.float32)
MOVE_SHIFT = np.array([0.2, -0.1, 0.0], dtype=np.float32)


def raster_lanes(n_rays, n_tri):
    """The lanes-per-triangle rule of csrc/raster.hip, restated: it picks the kernel instantiation."""
    p = n_rays // n_tri
    return 16 if p > 64 else (8 if p > 8 else 4)


# ------------------------------------------------------------------------------------------------ scenes and truth
@functools.lru_cache(maxsize=None)
def _mesh(shells, subdiv):
    from quadraturefields_amd import synthetic
    return synthetic.shell_mesh(n_shells=shells, subdivisions=subdiv)


@functools.lru_cache(maxsize=None)
def _vertices(shells, subdiv, moved=False):
    v = np.ascontiguousarray(_mesh(shells, subdiv).vertices, dtype=np.float32)
    return np.ascontiguousarray(v * MOVE_SCALE + MOVE_SHIFT, dtype=np.float32) if moved else v


def _f0():
    from quadraturefields_amd import synthetic
    return synthetic.lego_focal(800) * 96 / 800.0


@functools.lru_cache(maxsize=None)
def _view(pose="orbit", focal_scale=1.0, w=W, h=H, band=None, zero_x=False, struct=None):
    """One camera's pixel grid (or rows ``band`` of it, with ``parallel.band_camera``): rays generated on the host -- the
    brute force and the device see the same bits.  ``pose = "general"``: the camera of tests/asymmetric_inputs.py -- fy =
    0.62 fx, the principal point off the image centre, 25 degrees of roll, looking past the origin; ``struct`` =
    ``"swapped"`` / ``"centred"`` hands the pass the SAME rays with a struct whose fx and fy are exchanged / whose
    principal point is the image centre (a camera that does not describe them)."""
    from quadraturefields_amd import parallel, synthetic
    from quadraturefields_amd.mesh_utils import make_camera
    if pose == "general":
        from tests import asymmetric_inputs as asym
        assert not zero_x
        cam, c2w, k = asym.general_camera(w, h, focal_scale=focal_scale, band=band)
        o, d = asym.rays_from_k(c2w, *k, w, h)
        y0, y1 = (0, h) if band is None else band
        if struct is not None:
            fx, fy, cx, cy = k
            wrong = {"swapped": (fy, fx, cx, cy - y0), "centred": (fx, fy, w / 2.0, h / 2.0 - y0)}[struct]
            cam = asym.set_intrinsics(cam, *wrong)
        o, d = o[y0 * w:y1 * w].contiguous(), d[y0 * w:y1 * w].contiguous()
        # (the key names the RAYS: the brute force's answer is shared by every struct that is handed the same ones)
        return SimpleNamespace(key=(pose, focal_scale, w, h, band, zero_x), c2w=c2w.numpy().astype(np.float64), focal=k[0],
                               w=w, h=y1 - y0, n=(y1 - y0) * w, cam=cam, o=o.numpy(), d=d.numpy(), _dev=None)
    assert struct is None
    c2w = synthetic.orbit_cameras(1, seed=1)[0].clone()
    if pose == "inside":
        c2w[:, 3] *= 0.2                          # inside the shells: box corners behind the camera plane
    elif pose == "behind":
        c2w[:, 0] *= -1.0                         # turned half round about its up axis: the object is wholly behind it
        c2w[:, 2] *= -1.0
    if zero_x:                                    # a centre with a zero coordinate (-0.0 == 0.0, but not bitwise), still
        pos = c2w[:, 3].numpy().astype(np.float64)            # looking at the origin
        pos[0] = 0.0
        back = pos / np.linalg.norm(pos)
        right = np.cross([0.0, 0.0, 1.0], back)
        right /= np.linalg.norm(right)
        c2w = torch.from_numpy(np.stack([right, np.cross(back, right), back, pos], axis=1).astype(np.float32))
    focal = _f0() * focal_scale
    o, d = synthetic.camera_rays(c2w, focal, w, h)
    y0, y1 = (0, h) if band is None else band
    cam = make_camera(c2w, focal, w, h) if band is None else parallel.band_camera(c2w, focal, w, h, y0, y1)
    o, d = o[y0 * w:y1 * w].contiguous(), d[y0 * w:y1 * w].contiguous()
    return SimpleNamespace(key=(pose, focal_scale, w, h, band, zero_x), c2w=c2w.numpy().astype(np.float64), focal=focal,
                           w=w, h=y1 - y0, n=(y1 - y0) * w, cam=cam, o=o.numpy(), d=d.numpy(), _dev=None)


def _dev_rays(view, device):
    if view._dev is None:
        view._dev = (torch.from_numpy(view.o).to(device), torch.from_numpy(view.d).to(device))
    return view._dev


_TRUTH = {}


def _truth(mesh_key, view, min_sep=0.0, k=ALL):
    """(tri [R,k], t [R,k], count [R]) of the brute force, computed once per (mesh, rays, rule, k) and never modified."""
    key = (mesh_key, view.key, float(min_sep), k)
    if key not in _TRUTH:
        shells, subdiv = mesh_key[:2]
        brute = om.BruteForceIntersector(_vertices(*mesh_key), _mesh(shells, subdiv).faces, min_separation=min_sep)
        tri, t, cnt = brute.hits(view.o, view.d, k)
        if min_sep == 0 and k == ALL:
            assert cnt.max() < ALL                # the list really holds every hit
        for a in (tri, t, cnt):
            a.setflags(write=False)
        _TRUTH[key] = SimpleNamespace(tri=tri, t=t, cnt=cnt)
    return _TRUTH[key]


_HANDLES = {}


def _ri(mesh_key, fresh=False):
    """A ``RayIntersector`` (only its BVH handle is used here).  The shared ones are never refitted."""
    from quadraturefields_amd.mesh_io import TriMesh
    from quadraturefields_amd.mesh_utils import RayIntersector
    if fresh or mesh_key not in _HANDLES:
        m = _mesh(*mesh_key)
        ri = RayIntersector(TriMesh(_vertices(*mesh_key), m.faces), max_hits=25, min_separation=0)
        if fresh:
            return ri
        _HANDLES[mesh_key] = ri
    return _HANDLES[mesh_key]


# ------------------------------------------------------------------------------------------------ the raw calls
def _call(lib, ri, view, k, route="plain", cull=0, sort_lists=0, wide=0, slabs=0, min_sep=0.0, o=None, d=None):
    """One entry point, outputs pre-filled with sentinels, ``hit_count | overflow | ray_flag`` back to back; returns the raw
    arrays (host copies) and the device tensors (``.dev``) for a follow-up call."""
    from quadraturefields_amd import _C
    dev = ri.device
    ri.set_min_separation(min_sep)
    o_dev, d_dev = _dev_rays(view, dev)
    o = o_dev if o is None else o
    d = d_dev if d is None else d
    n = view.n
    tri = torch.full((n, k), SENT_TRI, dtype=torch.int32, device=dev)
    t = torch.full((n, k), float("nan"), dtype=torch.float32, device=dev)
    words = torch.full((n + 2,), GARBAGE, dtype=torch.int32, device=dev)
    cnt, ovf, flag = words[:n], words[n:n + 1], words[n + 1:]
    P, st, cam, h = _C.ptr, _C.stream(), ctypes.byref(view.cam), ri._handle
    out = SimpleNamespace()
    if route == "plain":
        _C.check(lib.qf_raster_intersect(h, cam, P(o), P(d), n, k, P(tri), P(t), P(cnt), P(ovf), sort_lists, cull, P(flag),
                                         st), "qf_raster_intersect")
    elif route == "wide":
        wtri = torch.full((wide, n), SENT_TRI, dtype=torch.int32, device=dev)
        wt = torch.full((wide, n), float("nan"), dtype=torch.float32, device=dev)
        _C.check(lib.qf_raster_intersect_wide(h, cam, P(o), P(d), n, k, wide, P(wtri), P(wt), P(tri), P(t), P(cnt), P(ovf),
                                              cull, P(flag), st), "qf_raster_intersect_wide")
    elif route == "slabs":
        keys = torch.full((wide, n), -1, dtype=torch.int64, device=dev)
        _C.check(lib.qf_raster_intersect_slabs(h, cam, P(o), P(d), n, k, wide, slabs, P(keys), P(tri), P(t), P(cnt), P(ovf),
                                               P(flag), st), "qf_raster_intersect_slabs")
    elif route == "tiles":
        n_tiles = ((view.w + 7) // 8) * ((view.h + 7) // 8)
        nbytes = int(lib.qf_hit_bins_bytes(view.w, view.h, k))
        assert nbytes == n_tiles * 64 * k * 8
        cursor = torch.full((n_tiles,), GARBAGE, dtype=torch.int32, device=dev)
        mask = torch.full((n_tiles,), GARBAGE, dtype=torch.int64, device=dev)
        bins = torch.full((nbytes // 8,), -1, dtype=torch.int64, device=dev)
        _C.check(lib.qf_raster_intersect_tiles(h, cam, P(o), P(d), n, k, P(cursor), P(mask), P(bins), nbytes, P(cnt), P(ovf),
                                               P(flag), st), "qf_raster_intersect_tiles")
        out.cursor = cursor.cpu().numpy()
        out.mask = mask.cpu().numpy().view(np.uint64)
        out.bins = bins.cpu().numpy().view(np.uint64).reshape(n_tiles, 64 * k)
    else:
        raise ValueError(route)
    out.dev = SimpleNamespace(tri=tri, t=t, cnt=cnt, flag=flag, o=o, d=d)
    out.tri, out.t = tri.cpu().numpy(), t.cpu().numpy()
    w_host = words.cpu().numpy()
    out.count, out.overflow, out.flag = w_host[:n], int(w_host[n]), int(w_host[n + 1])
    return out


def _visible(lib, ri):
    """The visible-chunk list of the handle's last culled call (sorted), checked for duplicates."""
    from quadraturefields_amd import _C
    n_chunks = (int(lib.qf_bvh_num_triangles(ri._handle)) + CHUNK - 1) // CHUNK
    buf = np.full(n_chunks, -1, dtype=np.int32)
    n = int(lib.qf_bvh_copy_visible_chunks(ri._handle, buf.ctypes.data_as(ctypes.c_void_p), n_chunks, _C.stream()))
    assert 0 <= n <= n_chunks, n
    vis = buf[:n]
    assert vis.min(initial=0) >= 0 and vis.max(initial=0) < n_chunks
    assert np.unique(vis).size == n, "a chunk is listed twice"
    return np.sort(vis)


# ------------------------------------------------------------------------------------------------ comparisons
def _keys(t, tri):
    """(t bits << 32 | tri): the device's hit key; its unsigned order is the (t, tri) order for the positive t of a hit."""
    return (np.ascontiguousarray(t).view(np.uint32).astype(np.uint64) << np.uint64(32)) | \
        np.ascontiguousarray(tri).astype(np.uint32).astype(np.uint64)


def _sorted_rows(t, tri, count):
    """Every ray's first min(count, K) slots as ascending keys, the slots behind as BIG; and the mask of those slots."""
    k = t.shape[1]
    valid = np.arange(k)[None, :] < np.minimum(count, k)[:, None]
    return np.sort(np.where(valid, _keys(t, tri), BIG), axis=1), valid


def _nearest(T, k):
    """The brute force's K nearest of every ray as sorted key rows (its lists are ascending in (t, tri))."""
    return _sorted_rows(T.t[:, :k], T.tri[:, :k], T.cnt)[0]


def _assert_sentinel_behind(out, rays, valid):
    assert (out.tri[rays][~valid[rays]] == SENT_TRI).all(), "a slot behind a ray's hits was written"
    assert np.isnan(out.t[rays][~valid[rays]]).all(), "a slot behind a ray's hits was written"


def _check_plain(out, T, k, ids=True):
    """qf_raster_intersect, lists in arrival order (sort_lists 0 / 2)."""
    assert out.flag == 0
    assert np.array_equal(out.count, T.cnt), "past K the pass keeps counting: hit_count == the brute force's count"
    assert out.overflow == int(np.maximum(T.cnt - k, 0).sum())
    full = T.cnt <= k
    if ids:
        tri, t_tri = out.tri, T.tri
    else:
        assert (out.tri == SENT_TRI).all(), "sort_lists = 2 leaves hit_tri alone"
        tri, t_tri = np.zeros_like(out.tri), np.zeros_like(T.tri)
    got, valid = _sorted_rows(out.t, tri, out.count)
    want = _sorted_rows(T.t[:, :k], t_tri[:, :k], T.cnt)[0]
    assert np.array_equal(got[full], want[full])
    assert np.isnan(out.t[full][~valid[full]]).all() and (out.tri[full][~valid[full]] == SENT_TRI).all()
    if (~full).any():                             # a full list: K distinct hits of the ray's own (which K is not defined)
        g = got[~full]
        every = _sorted_rows(T.t, t_tri, T.cnt)[0][~full]
        assert (g[:, :, None] == every[:, None, :]).any(axis=2).all()
        assert not ids or (g[:, 1:] > g[:, :-1]).all()


def _apply_rule(keys_sorted, n, min_sep):
    """The re-origin rule over ascending key rows (first ``n`` valid), in fp32 as the device applies it: the first hit is
    kept, a later one iff t > t_last_kept + min_sep.  -> (keys of the kept hits [R,K] padded with BIG, kept [R])."""
    r, k = keys_sorted.shape
    t = (keys_sorted >> np.uint64(32)).astype(np.uint32).view(np.float32)
    out = np.full((r, k), BIG, dtype=np.uint64)
    kept = np.zeros(r, dtype=np.int64)
    last = np.full(r, -np.inf, dtype=np.float32)
    ms = np.float32(min_sep)
    with np.errstate(invalid="ignore"):
        for i in range(k):
            ok = (i < n) & ((kept == 0) | (t[:, i] > last + ms))
            rows = np.flatnonzero(ok)
            out[rows, kept[rows]] = keys_sorted[rows, i]
            last[rows] = t[rows, i]
            kept[rows] += 1
    return out, kept


def _expected_unanswered(T, k, wide, min_sep):
    """Which rays a wide / slab pass may leave at hit_count > K (for the repair), from the brute force alone: those with
    more candidates than ``wide`` slots; and, rule on, those whose chain over the held prefix (the select capacity nearest)
    kept fewer than K while candidates remained (select_nearest_kernel)."""
    lost = T.cnt > wide
    if min_sep > 0:
        cap = min(k + SELECT_HEADROOM, wide)
        prefix = _sorted_rows(T.t[:, :cap], T.tri[:, :cap], T.cnt)[0]
        _, kept = _apply_rule(prefix, np.minimum(T.cnt, cap), min_sep)
        lost = lost | ((T.cnt > k) & (T.cnt > cap) & (np.minimum(kept, k) < k))
    return lost


def _check_selected(out, T, Tr, k, wide, min_sep, exact_overflow):
    """The K-nearest selection of the wide and the slab pass.  ``Tr``: brute force with the rule on (rule-on cases)."""
    assert out.flag == 0
    lost = _expected_unanswered(T, k, wide, min_sep)
    answered = ~lost
    if exact_overflow:                            # (the wide pass collects every crossing; the slab pass stops early)
        assert out.overflow == int(np.maximum(T.cnt - wide, 0).sum())
        assert np.array_equal(out.count[T.cnt > wide], T.cnt[T.cnt > wide]), "a ray beyond `wide` keeps its raw count"
    assert (out.count[lost] > k).all()
    assert (out.count[answered] <= k).all(), "a ray the pass could answer itself was left to the repair"
    got, valid = _sorted_rows(out.t, out.tri, out.count)
    _assert_sentinel_behind(out, answered, valid)
    if not min_sep > 0:
        assert np.array_equal(out.count[answered], np.minimum(T.cnt, k)[answered])
        assert np.array_equal(got[answered], _nearest(T, k)[answered]), "the row is not the ray's K nearest under (t, tri)"
        return
    # rule on.  Rays with at most K candidates are copied as they are (the rule is the filter's / the pack's job): all
    # their hits; the others went through the chain.  Either way the row, put through the rule, is the brute force's
    few = answered & (T.cnt <= k)
    assert np.array_equal(out.count[few], T.cnt[few]) and np.array_equal(got[few], _nearest(T, k)[few])
    filt, kept = _apply_rule(got, np.minimum(out.count, k), min_sep)
    want = _sorted_rows(Tr.t, Tr.tri, Tr.cnt)[0]
    assert np.array_equal(kept[answered], Tr.cnt[answered])
    assert np.array_equal(filt[answered], want[answered])
    chained = answered & (T.cnt > k)
    assert np.array_equal(out.count[chained], Tr.cnt[chained]) and np.array_equal(got[chained], want[chained])


# ------------------------------------------------------------------------------------------------ part 1: the routes
# (mesh, pose, band, K): the smallest scenes that reach every raster_lanes instantiation, partial chunks, lists that
# overflow K and cameras with box corners / the whole object behind the camera plane
PLAIN_CASES = [
    ((1, 0), "orbit", None, 25),           # 20 triangles = one partial chunk; 307 px / triangle: 16 lanes
    ((1, 0), "orbit", (24, 40), 3),        # a band's n_rays is its own: 1536 / 20 = 76: still 16 lanes
    ((1, 0), "orbit", (27, 35), 5),        # 768 / 20 = 38: 8 lanes
    ((1, 1), "orbit", None, 5),            # 80 triangles: two chunks, the second partial; 76: 16 lanes
    ((3, 1), "orbit", None, 3),            # 240 triangles = 3.75 chunks; 25: 8 lanes; 30 % of the rays overflow K = 3
    ((3, 1), "orbit", None, 25),
    ((3, 1), "orbit", (24, 32), 5),        # 768 / 240 = 3: 4 lanes
    ((3, 1), "inside", None, 3),
    ((4, 3), "orbit", None, 3),            # 5120 triangles; 1.2: 4 lanes
    ((4, 3), "orbit", None, 5),
    ((4, 3), "orbit", None, 25),
    ((4, 3), "inside", None, 5),
    ((4, 3), "behind", None, 5),
    ((8, 3), "orbit", None, 3),
    ((8, 3), "orbit", None, 5),
    ((8, 3), "orbit", None, 25),
    ((8, 3), "inside", None, 5),           # 10 .. 12 hits on every ray: every list overflows
    ((4, 3), "general", None, 5),          # fx != fy, an off-centre principal point, roll (tests/asymmetric_inputs.py)
    ((4, 3), "general", None, 25),
    ((8, 3), "general", None, 5),
    ((8, 3), "general", None, 25),
]


def test_the_cases_reach_every_lane_count_on_both_passes():
    """4, 8 and 16 lanes per triangle are separate kernel instantiations of the plain and of the culled pass (both run
    every case below)."""
    lanes = {raster_lanes(_view(pose, band=band).n, _mesh(*mesh).faces.shape[0]) for mesh, pose, band, _ in PLAIN_CASES}
    assert lanes == {4, 8, 16}
    assert raster_lanes(65 * 20, 20) == 16 and raster_lanes(64 * 20 + 19, 20) == 8        # the ranges' edges
    assert raster_lanes(9 * 20, 20) == 8 and raster_lanes(8 * 20 + 19, 20) == 4


@pytest.mark.parametrize("cull", [0, 1])
@pytest.mark.parametrize("mesh,pose,band,k", PLAIN_CASES)
def test_plain_and_culled_pass_raw_lists(device, lib, mesh, pose, band, k, cull):
    view = _view(pose, band=band)
    T = _truth(mesh, view)
    if pose == "inside" and mesh[0] >= 3:
        assert T.cnt.min() > 0                    # inside the shells: every ray hits
    if pose == "behind":
        assert T.cnt.max() == 0
    out = _call(lib, _ri(mesh), view, k, "plain", cull=cull, sort_lists=0)
    _check_plain(out, T, k)
    out = _call(lib, _ri(mesh), view, k, "plain", cull=cull, sort_lists=2)
    _check_plain(out, T, k, ids=False)


@pytest.mark.parametrize("cull", [0, 1])
@pytest.mark.parametrize("mesh,k", [((4, 3), 3), ((4, 3), 5), ((8, 3), 5)])
def test_plain_pass_counts_the_overflow_exactly(device, lib, mesh, k, cull):
    view = _view("orbit")
    T = _truth(mesh, view)
    assert (T.cnt > k).mean() > 0.05              # the scene does what the test is about
    out = _call(lib, _ri(mesh), view, k, "plain", cull=cull)
    assert out.overflow == int(np.maximum(T.cnt - k, 0).sum()) > 0
    assert np.array_equal(out.count, T.cnt)


@pytest.mark.parametrize("cull", [0, 1])
@pytest.mark.parametrize("mesh,pose,k", [((3, 1), "orbit", 5), ((4, 3), "orbit", 5), ((8, 3), "orbit", 25), ((4, 3), "inside", 25)])
def test_sorted_lists_with_the_rule_on(device, lib, mesh, pose, k, cull):
    """sort_lists = 1, rule on: the rows of rays with at most K raw hits are the brute force's with the same rule, padding
    included (the others are the repair's)."""
    view = _view(pose)
    T, Tr = _truth(mesh, view), _truth(mesh, view, RULE, k)
    out = _call(lib, _ri(mesh), view, k, "plain", cull=cull, sort_lists=1, min_sep=RULE)
    assert out.flag == 0 and out.overflow == int(np.maximum(T.cnt - k, 0).sum())
    full = T.cnt <= k
    assert full.sum() > 100 and (Tr.cnt[full] != T.cnt[full]).any()        # the rule drops hits of rays that are compared
    assert np.array_equal(out.count[full], Tr.cnt[full])
    assert np.array_equal(out.tri[full], Tr.tri[full])
    assert np.array_equal(out.t[full], Tr.t[full])


WIDE_CASES = [((8, 3), "orbit", 5, 7), ((8, 3), "orbit", 5, 24), ((8, 3), "orbit", 3, 7), ((4, 3), "orbit", 3, 7),
              ((8, 3), "inside", 5, 24), ((3, 1), "orbit", 3, 24), ((1, 1), "orbit", 5, 7), ((8, 3), "orbit", 25, 25),
              ((4, 3), "general", 5, 7), ((8, 3), "general", 5, 7), ((8, 3), "general", 5, 24), ((4, 3), "general", 25, 25),
              ((8, 3), "general", 25, 25)]


@pytest.mark.parametrize("min_sep", [0.0, RULE])
@pytest.mark.parametrize("cull", [0, 1])
@pytest.mark.parametrize("mesh,pose,k,wide", WIDE_CASES)
def test_wide_pass_selects_the_k_nearest(device, lib, mesh, pose, k, wide, cull, min_sep):
    view = _view(pose)
    T = _truth(mesh, view)
    Tr = _truth(mesh, view, min_sep, k) if min_sep > 0 else None
    if mesh == (8, 3) and pose == "orbit" and k < 25:
        assert (T.cnt > k).mean() > 0.05
        assert (T.cnt > wide).any() == (wide == 7)        # wide = 7: some rays lose candidates even at `wide`
    out = _call(lib, _ri(mesh), view, k, "wide", cull=cull, wide=wide, min_sep=min_sep)
    _check_selected(out, T, Tr, k, wide, min_sep, exact_overflow=True)


def _bvh_lists(lib, ri, view, k):
    from quadraturefields_amd import _C
    o, d = _dev_rays(view, ri.device)
    tri = torch.empty((view.n, k), dtype=torch.int32, device=ri.device)
    t = torch.empty((view.n, k), dtype=torch.float32, device=ri.device)
    cnt = torch.empty((view.n,), dtype=torch.int32, device=ri.device)
    _C.check(lib.qf_bvh_intersect(ri._handle, _C.ptr(o), _C.ptr(d), view.n, k, view.w, _C.ptr(tri), _C.ptr(t), _C.ptr(cnt),
                                  _C.stream()), "qf_bvh_intersect")
    return tri.cpu().numpy(), t.cpu().numpy(), cnt.cpu().numpy()


SLAB_CASES = [((8, 3), "orbit", 5, 7, 2, 0.0), ((8, 3), "orbit", 5, 7, 8, 0.0), ((8, 3), "orbit", 5, 24, 2, 0.0),
              ((8, 3), "orbit", 5, 24, 8, 0.0), ((8, 3), "orbit", 3, 24, 8, RULE), ((8, 3), "orbit", 5, 24, 2, RULE),
              ((8, 3), "inside", 5, 24, 8, 0.0), ((8, 3), "inside", 5, 24, 2, RULE), ((4, 3), "orbit", 3, 7, 8, 0.0),
              ((3, 1), "orbit", 3, 24, 2, RULE), ((1, 0), "orbit", 3, 7, 2, 0.0),
              ((4, 3), "general", 5, 7, 2, 0.0), ((8, 3), "general", 5, 7, 8, 0.0), ((8, 3), "general", 5, 24, 8, 0.0),
              ((4, 3), "general", 5, 24, 2, RULE), ((4, 3), "general", 25, 32, 2, 0.0), ((8, 3), "general", 25, 32, 8, 0.0)]


@pytest.mark.parametrize("mesh,pose,k,wide,slabs,min_sep", SLAB_CASES)
def test_slab_pass_selects_the_k_nearest_and_repairs_to_the_bvh(device, lib, mesh, pose, k, wide, slabs, min_sep):
    from quadraturefields_amd import _C
    view = _view(pose)
    ri = _ri(mesh)
    T = _truth(mesh, view)
    Tr = _truth(mesh, view, min_sep, k) if min_sep > 0 else None
    assert wide > min(k + SELECT_HEADROOM if min_sep > 0 else k, wide) + 1        # what the entry point demands
    out = _call(lib, ri, view, k, "slabs", wide=wide, slabs=slabs, min_sep=min_sep)
    if not (T.cnt > wide).any():
        assert out.overflow == 0
        _check_selected(out, T, Tr, k, wide, min_sep, exact_overflow=False)
    else:
        # rays with more crossings than slots may or may not be answered (a pixel that filled up in an earlier slab is
        # skipped); every ray within `wide` is answered by the pass itself
        assert min_sep == 0
        within = T.cnt <= wide
        got, valid = _sorted_rows(out.t, out.tri, out.count)
        assert np.array_equal(out.count[within], np.minimum(T.cnt, k)[within])
        assert np.array_equal(got[within], _nearest(T, k)[within])
        _assert_sentinel_behind(out, within, valid)
        rest = ~within & (out.count <= k)
        assert np.array_equal(got[rest], _nearest(T, k)[rest]) and (out.count[rest] == k).all()
    # the repair (with the flag) and the filter afterwards: exactly qf_bvh_intersect's lists
    dv = out.dev
    _C.check(lib.qf_bvh_repair_overflow(ri._handle, _C.ptr(dv.o), _C.ptr(dv.d), view.n, k, view.w, _C.ptr(dv.tri), _C.ptr(dv.t),
                                        _C.ptr(dv.cnt), None, None, _C.ptr(dv.flag), _C.stream()), "qf_bvh_repair_overflow")
    _C.check(lib.qf_filter_hits(ri._handle, view.n, k, _C.ptr(dv.tri), _C.ptr(dv.t), _C.ptr(dv.cnt), _C.stream()), "qf_filter_hits")
    tri_b, t_b, cnt_b = _bvh_lists(lib, ri, view, k)
    tri, t, cnt = dv.tri.cpu().numpy(), dv.t.cpu().numpy(), dv.cnt.cpu().numpy()
    assert np.array_equal(cnt, cnt_b)
    if min_sep > 0:                               # the filter sorts and pads
        assert np.array_equal(tri, tri_b) and np.array_equal(t, t_b)
        assert np.array_equal(cnt, Tr.cnt) and np.array_equal(tri, Tr.tri) and np.array_equal(t, Tr.t)
    else:                                         # rule off: no filter launch, the rows stay in arrival order
        assert np.array_equal(_sorted_rows(t, tri, cnt)[0], _sorted_rows(t_b, tri_b, cnt_b)[0])
        assert np.array_equal(_sorted_rows(t, tri, cnt)[0], _nearest(T, k))


@pytest.mark.parametrize("mesh,pose,w,h,k", [((8, 3), "orbit", 96, 64, 3), ((8, 3), "orbit", 93, 61, 3), ((8, 3), "orbit", 93, 61, 5),
                                             ((4, 3), "orbit", 93, 61, 5), ((4, 3), "orbit", 96, 64, 25), ((3, 1), "inside", 93, 61, 3),
                                             ((1, 0), "orbit", 90, 60, 5), ((4, 3), "behind", 93, 61, 5),
                                             ((4, 3), "general", 93, 61, 5), ((4, 3), "general", 96, 64, 25),
                                             ((8, 3), "general", 96, 64, 5), ((8, 3), "general", 93, 61, 25)])
def test_tile_bins_hold_exactly_the_hits(device, lib, mesh, pose, w, h, k):
    """93 x 61 and 90 x 60: ragged right and bottom tiles (5 resp. 2 of 8 columns, 5 resp. 4 of 8 rows inside the image)."""
    view = _view(pose, w=w, h=h)
    T = _truth(mesh, view)
    out = _call(lib, _ri(mesh), view, k, "tiles")
    assert out.flag == 0
    tiles_x, tiles_y = (w + 7) // 8, (h + 7) // 8
    cap = 64 * k
    true_img = np.zeros((tiles_y * 8, tiles_x * 8), dtype=np.int64)
    true_img[:h, :w] = T.cnt.reshape(h, w)
    got_img = np.full((tiles_y * 8, tiles_x * 8), -1, dtype=np.int64)
    got_img[:h, :w] = out.count.reshape(h, w)
    inside_img = np.zeros((tiles_y * 8, tiles_x * 8), dtype=bool)
    inside_img[:h, :w] = True
    per_tile = lambda a: a.reshape(tiles_y, 8, tiles_x, 8).transpose(0, 2, 1, 3).reshape(tiles_y * tiles_x, 64)
    true_t, got_t, inside_t = per_tile(true_img), per_tile(got_img), per_tile(inside_img)
    assert np.array_equal(out.cursor, true_t.sum(axis=1)), "the cursor counts every candidate of its tile, past the capacity too"
    over = out.cursor > cap
    if mesh == (8, 3) and k == 3:
        assert over.sum() >= 3 and (~over & (true_t > k).any(axis=1)).sum() >= 3        # both kinds of overflow occur
    bits = ((out.mask[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
    # tiles whose bin held everything: counts, mask bits and records
    fine = ~over
    assert np.array_equal(got_t[fine][inside_t[fine]], true_t[fine][inside_t[fine]])
    assert np.array_equal(bits[fine], (true_t > k)[fine])
    # tiles whose cursor ran past the capacity: every in-image pixel goes to the repair
    assert (got_t[over][inside_t[over]] > k).all()
    assert np.array_equal(bits[over], inside_t[over])
    if not over.any():
        assert out.overflow == int(np.maximum(T.cnt - k, 0).sum())
    ray_of = per_tile(np.arange(tiles_y * 8 * tiles_x * 8).reshape(tiles_y * 8, tiles_x * 8))      # padded-image index
    all_keys = _keys(T.t, T.tri)
    for tile in np.flatnonzero(fine & (out.cursor > 0)):
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


def test_a_handle_without_triangles_answers_nothing(device, lib):
    """qf_bvh_create accepts n_tri = 0 (not constructible through ``MeshIntersection``): every pass zeroes its words and
    returns without a hit, and there is no visible-chunk list to copy."""
    from quadraturefields_amd import _C
    handle = ctypes.c_void_p()
    _C.check(lib.qf_bvh_create(None, 0, ctypes.byref(handle)), "qf_bvh_create")
    try:
        assert lib.qf_bvh_num_triangles(handle) == 0
        empty = SimpleNamespace(_handle=handle, device=device,
                                set_min_separation=lambda ms: _C.check(lib.qf_bvh_set_min_separation(handle, ms), "min_sep"))
        view = _view("orbit", w=93, h=61)
        for route, kw in (("plain", dict(cull=0)), ("plain", dict(cull=1)), ("plain", dict(cull=1, sort_lists=2)),
                          ("wide", dict(cull=0, wide=7)), ("wide", dict(cull=1, wide=7)), ("slabs", dict(wide=7, slabs=2)),
                          ("tiles", {})):
            out = _call(lib, empty, view, 5, route, **kw)
            assert out.flag == 0 and out.overflow == 0 and not out.count.any(), (route, kw)
            assert (out.tri == SENT_TRI).all() and np.isnan(out.t).all(), (route, kw)
            if route == "tiles":
                assert not out.cursor.any() and not out.mask.any()
        assert lib.qf_bvh_copy_visible_chunks(handle, None, 0, _C.stream()) < 0
    finally:
        lib.qf_bvh_destroy(handle)


def _half_pixel_off(view, i):
    """Ray i's direction moved half a pixel along the image's x axis."""
    right, back = view.c2w[:, 0], view.c2w[:, 2]
    d = view.d[i].astype(np.float64)
    v = d / -(d @ back) + 0.5 / view.focal * right
    return (v / np.linalg.norm(v)).astype(np.float32)


@pytest.mark.parametrize("mesh,route", [((4, 3), "plain"), ((1, 0), "plain"), ((4, 3), "wide")])
def test_ray_flag_through_the_culling_launch(device, lib, mesh, route):
    """With cull_chunks the ray check rides in cull_chunks_kernel, one lane per chunk with that grid's stride: ray 0 and
    the very last ray of a batch that is no multiple of 256, each with a single-bit origin change, a direction half a pixel
    off and a non-unit direction.  A raised flag: all counts 0, no list slot has left its sentinel."""
    view = _view("orbit", band=(20, 35), zero_x=True)
    assert view.n % 256 != 0 and float(view.o[0, 0]) == 0.0
    ri = _ri(mesh)
    k, wide = 5, 7
    T = _truth(mesh, view)
    assert T.cnt.sum() > 0
    out = _call(lib, ri, view, k, route, cull=1, wide=wide)
    assert out.flag == 0
    if route == "plain":
        _check_plain(out, T, k)
    else:
        _check_selected(out, T, None, k, wide, 0.0, exact_overflow=True)
    o_dev, d_dev = _dev_rays(view, ri.device)
    for i in (0, view.n - 1):
        for what in ("origin bit", "half a pixel", "not unit"):
            o, d = o_dev.clone(), d_dev.clone()
            if what == "origin bit":
                o[i, 0] = -0.0
                assert torch.equal(o, o_dev) and not np.array_equal(o.cpu().numpy().view(np.uint32), view.o.view(np.uint32))
            elif what == "half a pixel":
                d[i] = torch.from_numpy(_half_pixel_off(view, i)).to(d.device)
            else:
                d[i] = d[i] * 1.01
            out = _call(lib, ri, view, k, route, cull=1, wide=wide, o=o, d=d)
            assert out.flag == 1, (i, what)
            assert out.overflow == 0 and not out.count.any(), (i, what)
            assert (out.tri == SENT_TRI).all() and np.isnan(out.t).all(), (i, what)


@pytest.mark.parametrize("struct", ["swapped", "centred"])
@pytest.mark.parametrize("mesh,route,cull,k", [((4, 3), "plain", 0, 5), ((4, 3), "plain", 1, 25), ((8, 3), "wide", 1, 5),
                                               ((8, 3), "slabs", 0, 5), ((4, 3), "tiles", 0, 25)])
def test_general_camera_rays_with_another_cameras_struct_raise_the_flag(device, lib, mesh, route, cull, k, struct):
    """The general camera's rays with a struct whose fx and fy are exchanged, or whose principal point is the image centre:
    the struct does not describe the rays, so every pass must raise the flag and write nothing; the repair then answers
    every ray through the BVH, and the lists are the brute force's.  With the RIGHT struct the same rays pass the check
    (flag 0) in the case lists above: the check reads fx, fy, cx and cy where the struct keeps them."""
    from quadraturefields_amd import _C
    good, view = _view("general"), _view("general", struct=struct)
    assert np.array_equal(view.o, good.o) and np.array_equal(view.d, good.d) and view.key == good.key
    assert (view.cam.fx, view.cam.fy, view.cam.cx, view.cam.cy) != (good.cam.fx, good.cam.fy, good.cam.cx, good.cam.cy)
    ri = _ri(mesh)
    T = _truth(mesh, view)
    assert (T.cnt > 0).mean() > 0.2
    wide, slabs = 24, 2
    assert _call(lib, ri, good, k, route, cull=cull, wide=wide, slabs=slabs).flag == 0
    out = _call(lib, ri, view, k, route, cull=cull, wide=wide, slabs=slabs)
    assert out.flag == 1
    assert out.overflow == 0 and not out.count.any()
    assert (out.tri == SENT_TRI).all() and np.isnan(out.t).all()
    if route == "tiles":
        assert not out.cursor.any() and not out.mask.any()
        return                                    # (the bins' consumer is the frame's tile pack, not this repair)
    dv = out.dev
    _C.check(lib.qf_bvh_repair_overflow(ri._handle, _C.ptr(dv.o), _C.ptr(dv.d), view.n, k, view.w, _C.ptr(dv.tri), _C.ptr(dv.t),
                                        _C.ptr(dv.cnt), None, None, _C.ptr(dv.flag), _C.stream()), "qf_bvh_repair_overflow")
    tri, t, cnt = dv.tri.cpu().numpy(), dv.t.cpu().numpy(), dv.cnt.cpu().numpy()
    assert np.array_equal(cnt, np.minimum(T.cnt, k))
    assert np.array_equal(_sorted_rows(t, tri, cnt)[0], _nearest(T, k))


# ------------------------------------------------------------------------------------------------ part 2: the culling
def _chunk_geometry(lib, ri, mesh_key):
    """The chunks restated on the host in fp64: 64 consecutive triangles in leaf order (``qf_bvh_copy_tri_ids``) ->
    (box lo [C,3], box hi [C,3], chunk of every ORIGINAL triangle id)."""
    faces = _mesh(*mesh_key[:2]).faces
    n_tri = faces.shape[0]
    assert int(lib.qf_bvh_num_triangles(ri._handle)) == n_tri
    ids = np.empty(n_tri, dtype=np.int32)
    assert lib.qf_bvh_copy_tri_ids(ri._handle, ids.ctypes.data_as(ctypes.c_void_p), n_tri) == 0
    assert np.array_equal(np.sort(ids), np.arange(n_tri))
    n_chunks = (n_tri + CHUNK - 1) // CHUNK
    corners = _vertices(*mesh_key).astype(np.float64)[faces[ids]].reshape(n_tri, 3, 3)
    lo = np.stack([corners[c * CHUNK:(c + 1) * CHUNK].reshape(-1, 3).min(axis=0) for c in range(n_chunks)])
    hi = np.stack([corners[c * CHUNK:(c + 1) * CHUNK].reshape(-1, 3).max(axis=0) for c in range(n_chunks)])
    chunk_of = np.empty(n_tri, dtype=np.int64)
    chunk_of[ids] = np.arange(n_tri) // CHUNK
    return lo, hi, chunk_of


def _must(T, chunk_of):
    """Chunks that hold a triangle the brute force reports for any ray."""
    valid = np.arange(T.tri.shape[1])[None, :] < T.cnt[:, None]
    return np.unique(chunk_of[T.tri[valid]])


def _may(view, lo, hi):
    """Chunks with a box corner at or behind the camera plane (the kernel's 1e-4, with room for its fp32 rounding), or
    whose exactly projected corner box, grown by kRasterGuard + 2 px, touches the view's image.  -> (may, behind)."""
    cam = view.cam
    rot, centre = view.c2w[:, :3], view.c2w[:, 3]
    sel = np.array([[(k >> a) & 1 for a in range(3)] for k in range(8)], dtype=bool)              # [8,3]
    corners = np.where(sel[None], hi[:, None, :], lo[:, None, :]) - centre                          # [C,8,3]
    pc = corners @ rot                                                                              # R^T (v - c)
    zv = -pc[..., 2]
    front = zv > 2e-4
    with np.errstate(divide="ignore", invalid="ignore"):
        sx = np.where(front, float(cam.fx) * pc[..., 0] / zv + (float(cam.cx) - 0.5), np.nan)
        sy = np.where(front, -float(cam.fy) * pc[..., 1] / zv + (float(cam.cy) - 0.5), np.nan)
    g = GUARD + 2.0
    # (a corner that is not in front keeps its chunk whatever the others project to: -inf / +inf stand in for it)
    touches = (np.where(front, sx, np.inf).max(axis=1) + g >= 0) & (np.where(front, sy, np.inf).max(axis=1) + g >= 0) & \
        (np.where(front, sx, -np.inf).min(axis=1) - g <= cam.width - 1) & (np.where(front, sy, -np.inf).min(axis=1) - g <= cam.height - 1)
    may = np.flatnonzero((~front).any(axis=1) | touches)
    behind = np.flatnonzero((zv <= 0.5e-4).any(axis=1))
    return may, behind


def _check_culled_call(lib, ri, mesh_key, view, geometry, k=25):
    """One culled call: part 1's invariants on its raw lists, and must <= visible <= may.  -> (visible, must, may)."""
    T = _truth(mesh_key, view)
    out = _call(lib, ri, view, k, "plain", cull=1)
    vis = _visible(lib, ri)
    lo, hi, chunk_of = geometry
    must = _must(T, chunk_of)
    may, behind = _may(view, lo, hi)
    assert np.isin(must, vis).all(), "a chunk with a hit was culled"
    assert np.isin(behind, vis).all(), "a chunk with a corner behind the camera plane was culled"
    assert np.isin(vis, may).all(), "a chunk that cannot touch the image was kept"
    _check_plain(out, T, k)
    return vis, must, may


CULL_BANDS = [None, (0, 8), (56, 64), (8, 16), (24, 40), (40, 48), (16, 17)]


@pytest.mark.parametrize("mesh", [(1, 0), (3, 1), (4, 3)])
def test_culling_is_conservative_and_tight(device, lib, mesh):
    """Half the focal length: rows 11 .. 51 of the 64 have hits.  Bands [0, 8) and [56, 64) hit nothing -- the culled
    kernel then runs over a (possibly) empty list -- [8, 16) is one tile row at the object's edge, [16, 17) a single row."""
    ri = _ri(mesh)
    geometry = _chunk_geometry(lib, ri, mesh)
    n_chunks = geometry[0].shape[0]
    sizes = []
    for pose in ("orbit", "inside", "general"):
        for band in CULL_BANDS:
            view = _view(pose, 0.5, band=band)
            vis, must, may = _check_culled_call(lib, ri, mesh, view, geometry)
            for k in (3, 5):
                _check_plain(_call(lib, ri, view, k, "plain", cull=1), _truth(mesh, view), k)
                assert np.array_equal(_visible(lib, ri), vis)
            sizes.append((pose, band, len(must), len(vis), len(may)))
            if pose == "orbit" and band in ((0, 8), (56, 64)):
                assert len(must) == 0 and _truth(mesh, view).cnt.max() == 0
            if pose == "inside" and mesh[0] >= 3:
                assert _truth(mesh, view).cnt.min() > 0
    print(mesh, n_chunks, sizes)
    if mesh == (4, 3):
        T = _truth(mesh, _view("orbit", 0.5, band=(8, 16)))
        assert np.unique(T.tri[np.arange(ALL)[None, :] < T.cnt[:, None]]).size == 101
        # the upper bound is what makes "shrinks with the band" an assertion: it must bite for some band
        assert any(0 < n_may < n_chunks / 2 for _, _, _, _, n_may in sizes), sizes
        assert any(0 < n_vis < n_chunks / 2 for _, _, _, n_vis, _ in sizes), sizes


def _canon(out):
    return _sorted_rows(out.t, out.tri, out.count)[0], out.count.copy(), out.overflow, out.flag


def test_counter_parity_over_consecutive_culled_calls(device, lib):
    """The visible list is appended to through counters[parity], and each call zeroes the other counter for the next one.
    Five culled calls alternating two bands, an unculled and a slab call (which reuses the list's memory) in between: every
    call's visible set and raw hits are those of a fresh handle's first call."""
    from quadraturefields_amd import _C
    mesh = (4, 3)
    views = {"a": _view("orbit", 0.5, band=(24, 40)), "b": _view("orbit", 0.5, band=(8, 16))}
    want = {}
    for name, view in views.items():
        fresh = _ri(mesh, fresh=True)
        assert lib.qf_bvh_copy_visible_chunks(fresh._handle, None, 0, _C.stream()) < 0      # no culled call has run
        out = _call(lib, fresh, view, 25, "plain", cull=1)
        want[name] = (_visible(lib, fresh), _canon(out))
        _check_plain(out, _truth(mesh, view), 25)
    assert len(want["a"][0]) != len(want["b"][0]) and len(want["b"][0]) > 0
    ri = _ri(mesh, fresh=True)
    full = _view("orbit", 0.5)
    for step in ("a", "b", "unculled", "a", "slabs", "b", "a", "wide b", "a"):
        if step == "unculled":
            _check_plain(_call(lib, ri, full, 25, "plain", cull=0), _truth(mesh, full), 25)
            continue
        if step == "slabs":
            _call(lib, ri, full, 5, "slabs", wide=24, slabs=2)
            assert lib.qf_bvh_copy_visible_chunks(ri._handle, None, 0, _C.stream()) < 0     # the list was overwritten
            continue
        if step == "wide b":
            out = _call(lib, ri, views["b"], 5, "wide", cull=1, wide=24)
            assert np.array_equal(_visible(lib, ri), want["b"][0])
            _check_selected(out, _truth(mesh, views["b"]), None, 5, 24, 0.0, exact_overflow=True)
            continue
        out = _call(lib, ri, views[step], 25, "plain", cull=1)
        vis, got = _visible(lib, ri), _canon(out)
        assert np.array_equal(vis, want[step][0]), step
        assert all(np.array_equal(x, y) for x, y in zip(got, want[step][1])), step


REFIT_BANDS = [(40, 41), (38, 40), (14, 15), (8, 16), (24, 40)]


@pytest.mark.parametrize("where", ["host", "device"])
def test_chunk_boxes_follow_a_refit(device, lib, where):
    """After qf_bvh_refit / qf_bvh_refit_device the next culled call works on the moved mesh's boxes: part 1's invariants
    and must <= visible <= may against a brute force built on the moved vertices, on every band.  The move squeezes the
    object from rows 11 .. 51 into rows 14 .. 40 (row 40 receives what was ten rows further down): among the bands must be
    one where stale boxes lose hits -- the moved mesh's must set is not contained in what was visible there before the
    refit.  On the 5120-triangle mesh no band is: a chunk is a twentieth of a shell, and everything that arrives in a
    band was visible there before; hence the 81 920 triangles (1280 chunks, four rows each) here."""
    from quadraturefields_amd import _C
    mesh, moved = (4, 5), (4, 5, True)
    ri = _ri(mesh, fresh=True)
    geometry = _chunk_geometry(lib, ri, mesh)
    before = {}
    for band in REFIT_BANDS:                      # (these calls also compute the boxes a missed refit would leave behind)
        before[band] = _check_culled_call(lib, ri, mesh, _view("orbit", 0.5, band=band), geometry)[0]
    tri = np.ascontiguousarray(_vertices(*moved)[_mesh(*mesh).faces].reshape(-1, 9))
    if where == "host":
        _C.check(lib.qf_bvh_refit(ri._handle, tri.ctypes.data_as(ctypes.c_void_p), tri.shape[0]), "qf_bvh_refit")
    else:
        tri_dev = torch.from_numpy(tri).to(ri.device)
        _C.check(lib.qf_bvh_refit_device(ri._handle, _C.ptr(tri_dev), tri.shape[0], _C.stream()), "qf_bvh_refit_device")
    geometry_moved = _chunk_geometry(lib, ri, moved)
    assert np.array_equal(geometry_moved[2], geometry[2])                  # same topology, same leaf order
    telling = []
    for band in REFIT_BANDS:
        must = _must(_truth(moved, _view("orbit", 0.5, band=band)), geometry_moved[2])
        if not np.isin(must, before[band]).all():
            telling.append(band)
    print("bands that tell stale boxes from fresh ones:", telling)
    assert telling, "no band can tell stale boxes from fresh ones"
    for band in REFIT_BANDS:
        view = _view("orbit", 0.5, band=band)
        _check_culled_call(lib, ri, moved, view, geometry_moved)
        for k in (3, 5):
            _check_plain(_call(lib, ri, view, k, "plain", cull=1), _truth(moved, view), k)
