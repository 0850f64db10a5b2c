"""GPU: the device BVH build (``qf_bvh_create_device``, csrc/bvh_build_device.hip) -- byte parity with the numpy
restatement of its rules (tests/bvh_device_build_reference.py), and every route that takes a ``qf_bvh`` on a device-built
handle against the brute force (``oracle.meshpath.BruteForceIntersector``), bit for bit."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import meshpath as om
from tests import bvh_device_build_reference as ref

pytestmark = pytest.mark.gpu

BIG = np.uint64(0xFFFFFFFFFFFFFFFF)
MAX_STACK = 384                       # QF_BVH8_MAX_STACK


# ------------------------------------------------------------------------------------------------ scenes and helpers
@functools.lru_cache(maxsize=None)
def _mesh(shells, subdiv):
    from quadraturefields_amd import synthetic
    return synthetic.shell_mesh(n_shells=shells, subdivisions=subdiv)


def _soup(mesh):
    return np.ascontiguousarray(mesh.vertices.astype(np.float32)[mesh.faces])


def _soup_mesh(tri):
    """A TriMesh of the triangle soup ``tri`` [n,3,3]."""
    from quadraturefields_amd.mesh_io import TriMesh
    n = tri.shape[0]
    return TriMesh(tri.reshape(-1, 3), np.arange(3 * n, dtype=np.int64).reshape(-1, 3))


def _rays(n, seed=0, radius=4.0, targets=None):
    rng = np.random.default_rng(seed)
    o = rng.normal(size=(n, 3))
    o = (o / np.linalg.norm(o, axis=1, keepdims=True) * radius).astype(np.float32)
    if targets is None:
        target = rng.uniform(-1.0, 1.0, size=(n, 3)).astype(np.float32)
    else:                             # aim at points of the triangles ``targets`` [m,3,3] (few of them would be missed)
        w = rng.dirichlet(np.ones(3), size=n)
        target = np.einsum("nk,nkc->nc", w, targets[rng.integers(0, targets.shape[0], size=n)].astype(np.float64))
        target = (target + rng.normal(size=(n, 3)) * 1e-3).astype(np.float32)
    d = target - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return o, d


def _special_rays(n, seed):
    """Random rays plus rays from inside the object, axis-aligned rays (zero direction components) and misses."""
    o, d = _rays(n, seed=seed)
    o[:50] = 0.0
    d[50:53] = np.array([[1, 0, 0], [0, -1, 0], [0, 0, 1]], dtype=np.float32)
    o[53:60] = np.array([10, 10, 10], dtype=np.float32)
    return o, d


def _raw_build(lib, tri_dev, n=None):
    from quadraturefields_amd import _C
    handle = ctypes.c_void_p()
    n = tri_dev.shape[0] if n is None else n
    rc = lib.qf_bvh_create_device(_C.ptr(tri_dev) if tri_dev is not None else None, n, _C.stream(), ctypes.byref(handle))
    return rc, handle


def _dump(lib, handle):
    n8 = int(lib.qf_bvh_num_wide_nodes(handle))
    n_tri = int(lib.qf_bvh_num_triangles(handle))
    nodes = np.full((n8, 64), np.nan, dtype=np.float32)
    ids = np.full(n_tri, -1, dtype=np.int32)
    starts = np.full(128, -1, dtype=np.int32)
    assert lib.qf_bvh_copy_wide_nodes(handle, nodes.ctypes.data_as(ctypes.c_void_p), n8) == 0
    assert lib.qf_bvh_copy_tri_ids(handle, ids.ctypes.data_as(ctypes.c_void_p), n_tri) == 0
    n_starts = int(lib.qf_bvh_copy_level_starts(handle, starts.ctypes.data_as(ctypes.c_void_p), 128))
    return dict(nodes=nodes, tri_ids=ids, level_start=starts[:n_starts].tolist(), max_stack=int(lib.qf_bvh_max_stack(handle)))


def _assert_hits_equal(got, want):
    tri, t, cnt = got
    tri_o, t_o, cnt_o = want
    assert np.array_equal(cnt.cpu().numpy(), cnt_o)
    assert np.array_equal(tri.cpu().numpy(), tri_o)
    assert np.array_equal(t.cpu().numpy().view(np.uint32), t_o.view(np.uint32))


def _device_ri(mesh, k, **kw):
    from quadraturefields_amd.mesh_utils import RayIntersector
    return RayIntersector(mesh, max_hits=k, builder="device", **kw)


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("shells,subdiv", [(3, 3), (2, 3)])
def test_device_build_equals_the_restatement_byte_for_byte(device, lib, shells, subdiv):
    tri = _soup(_mesh(shells, subdiv))
    want = ref.build(tri)
    tri_dev = torch.from_numpy(tri).to(device)
    dumps = []
    for _ in range(2):
        rc, handle = _raw_build(lib, tri_dev)
        assert rc == 0
        try:
            dumps.append(_dump(lib, handle))
            levels = len(dumps[-1]["level_start"]) - 1
            # no binary tree: no binary nodes, nothing copied, the depth is the number of wide levels
            assert int(lib.qf_bvh_num_nodes(handle)) == 0 and int(lib.qf_bvh_max_depth(handle)) == levels
            untouched = np.full(16, 7.0, dtype=np.float32)
            assert lib.qf_bvh_copy_nodes(handle, untouched.ctypes.data_as(ctypes.c_void_p), 1) == 0
            assert bool((untouched == 7.0).all())
        finally:
            lib.qf_bvh_destroy(handle)
    got = dumps[0]
    tok, tok_w = got["nodes"].reshape(-1, 8, 8)[:, :, 6].view(np.int32), want["nodes"].reshape(-1, 8, 8)[:, :, 6].view(np.int32)
    assert got["level_start"] == want["level_start"]
    assert np.array_equal(got["tri_ids"], want["tri_ids"])
    assert np.array_equal(tok, tok_w)
    assert np.array_equal(got["nodes"].view(np.uint32), want["nodes"].view(np.uint32))      # boxes, tokens and padding
    assert got["max_stack"] == want["max_stack"]
    for key in ("nodes", "tri_ids"):
        assert np.array_equal(dumps[0][key].view(np.uint32), dumps[1][key].view(np.uint32))
    assert dumps[0]["level_start"] == dumps[1]["level_start"] and dumps[0]["max_stack"] == dumps[1]["max_stack"]


# ------------------------------------------------------------------------------------------------ hits
@functools.lru_cache(maxsize=None)
def _brute(shells, subdiv):
    m = _mesh(shells, subdiv)
    return om.BruteForceIntersector(m.vertices, m.faces)


@pytest.mark.parametrize("max_hits", [1, 5, 25])
def test_hits_bit_equal_to_brute_force_and_to_the_host_built_tree(device, max_hits):
    from quadraturefields_amd.mesh_utils import RayIntersector
    mesh = _mesh(4, 3)
    o, d = _special_rays(3000, seed=max_hits)
    want = _brute(4, 3).hits(o, d, max_hits)
    ri = _device_ri(mesh, max_hits)
    assert ri.num_nodes == 0 and ri.num_wide_nodes > 0 and ri.max_stack <= MAX_STACK
    got = ri.hits(o, d)
    _assert_hits_equal(got[:3], want)
    host = RayIntersector(mesh, max_hits=max_hits).hits(o, d)
    for x, y in zip(got[:3], host[:3]):
        assert torch.equal(x, y)
    assert want[2].max() == max_hits or max_hits == 25
    a = ri.hits(o[:2048], d[:2048], image_width=0)
    b = ri.hits(o[:2048], d[:2048], image_width=64)
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("n", [1, 2, 8, 9, 16, 17, 63, 64, 65, 72, 73])
def test_small_meshes_against_brute_force(device, n):
    tri = _soup(_mesh(2, 3))[:n]
    mesh = _soup_mesh(tri)
    o, d = _rays(512, seed=n, targets=tri)
    want = om.BruteForceIntersector(mesh.vertices, mesh.faces, min_separation=0.0).hits(o, d, 10)
    assert want[2].sum() >= 256                                # the rays do meet these few triangles
    ri = _device_ri(mesh, 10, min_separation=0.0)
    assert ri.num_wide_nodes >= 1 and (n > 8 or (ri.num_wide_nodes, ri.max_depth, ri.max_stack) == (1, 1, 2))
    _assert_hits_equal(ri.hits(o, d)[:3], want)


def test_empty_mesh_through_the_raw_abi(device, lib):
    from quadraturefields_amd import _C, synthetic
    from quadraturefields_amd.mesh_utils import make_camera
    rc, handle = _raw_build(lib, None, n=0)
    assert rc == 0 and handle.value
    try:
        assert int(lib.qf_bvh_num_triangles(handle)) == 0 and int(lib.qf_bvh_num_wide_nodes(handle)) == 0
        w, h, k = 16, 8, 4
        c2w, focal = synthetic.orbit_cameras(1, seed=1)[0], synthetic.lego_focal(800) * w / 800.0
        o, d = synthetic.camera_rays(c2w, focal, w, h, device=device)
        cam = make_camera(c2w, focal, w, h)
        n = w * h
        P, st = _C.ptr, _C.stream()

        def outputs():
            return (torch.full((n, k), -7, dtype=torch.int32, device=device), torch.full((n, k), 3.0, device=device),
                    torch.full((n + 2,), 99, dtype=torch.int32, device=device))

        tri, t, words = outputs()
        _C.check(lib.qf_bvh_intersect(handle, P(o), P(d), n, k, 0, P(tri), P(t), P(words[:n]), st), "qf_bvh_intersect")
        assert int(words[:n].abs().sum()) == 0 and bool((tri == -1).all()) and bool(torch.isinf(t).all())
        for cull in (0, 1):
            tri, t, words = outputs()
            _C.check(lib.qf_raster_intersect(handle, ctypes.byref(cam), P(o), P(d), n, k, P(tri), P(t), P(words[:n]),
                                             P(words[n:n + 1]), 1, cull, P(words[n + 1:]), st), "qf_raster_intersect")
            assert int(words[:n + 1].abs().sum()) == 0
        tri, t, words = outputs()
        keys = torch.zeros((16, n), dtype=torch.int64, device=device)
        _C.check(lib.qf_raster_intersect_slabs(handle, ctypes.byref(cam), P(o), P(d), n, k, 16, 4, P(keys), P(tri), P(t),
                                               P(words[:n]), P(words[n:n + 1]), P(words[n + 1:]), st), "qf_raster_intersect_slabs")
        assert int(words[:n + 1].abs().sum()) == 0
    finally:
        lib.qf_bvh_destroy(handle)


# ------------------------------------------------------------------------------------------------ degenerate keys
def _copies():
    one = np.array([[[-0.5, -0.4, 0.1], [0.6, -0.3, 0.0], [0.0, 0.7, -0.1]]], dtype=np.float32)
    return np.ascontiguousarray(np.repeat(one, 4096, axis=0))


def _flat_grid():
    """32 x 32 cells x 2 triangles in the plane z = 0.25: one zero-extent axis."""
    g = np.linspace(-1.0, 1.0, 33).astype(np.float32)
    x0, y0 = np.meshgrid(g[:-1], g[:-1], indexing="ij")
    x1, y1 = np.meshgrid(g[1:], g[1:], indexing="ij")
    z = np.full_like(x0, 0.25)
    a, b, c, e = (np.stack(p, axis=-1) for p in ((x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)))
    tri = np.concatenate([np.stack([a, b, c], axis=-2).reshape(-1, 3, 3), np.stack([a, c, e], axis=-2).reshape(-1, 3, 3)])
    assert tri.shape[0] == 2048
    return np.ascontiguousarray(tri, dtype=np.float32)


def _growing():
    """The lopsided case: triangles along +x, each twice as far and twice as large as the previous, so every Morton split
    peels the far end off.  fp32 holds 256 doublings, not 4096: the 4096 triangles are 16 interleaved runs of 256
    doublings (2^-136 .. 2^119), run g scaled by 1 + g / 16 so that no two triangles coincide."""
    j, g = np.meshgrid(np.arange(256, dtype=np.float64), np.arange(16, dtype=np.float64), indexing="ij")
    x = (np.exp2(j - 136.0) * (1.0 + g / 16.0)).reshape(-1)
    s = x * 0.02
    z = np.zeros_like(x)
    tri = np.stack([np.stack([x, -s, -s], 1), np.stack([x, s, -s], 1), np.stack([x, z, s], 1)], 1)
    assert tri.shape == (4096, 3, 3)
    return np.ascontiguousarray(tri.astype(np.float32))


def _growing_rays(m=1024):
    rng = np.random.default_rng(0)
    o = np.zeros((m, 3), np.float32)
    o[:, 0] = -1.0
    d = np.stack([np.ones(m), rng.normal(size=m) * 5e-3, rng.normal(size=m) * 5e-3], 1)
    return o, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("case", ["copies", "flat", "growing"])
def test_degenerate_keys_against_brute_force(device, case):
    tri = {"copies": _copies, "flat": _flat_grid, "growing": _growing}[case]()
    mesh = _soup_mesh(tri)
    k = 25
    o, d = _growing_rays() if case == "growing" else _rays(1024, seed=11, targets=tri)
    want = om.BruteForceIntersector(mesh.vertices, mesh.faces, min_separation=0.0).hits(o, d, k)
    assert want[2].sum() > 200
    ri = _device_ri(mesh, k, min_separation=0.0)
    assert ri.max_stack <= MAX_STACK
    _assert_hits_equal(ri.hits(o, d)[:3], want)
    if case == "copies":
        assert want[2].max() == k                              # 4096 coincident hits: the K-list fills


# ------------------------------------------------------------------------------------------------ camera-coherent routes
def _sorted_keys(tri, t, cnt):
    key = (np.ascontiguousarray(t).view(np.uint32).astype(np.uint64) << np.uint64(32)) | \
        np.ascontiguousarray(tri).astype(np.uint32).astype(np.uint64)
    key[np.arange(key.shape[1])[None, :] >= cnt[:, None]] = BIG
    return np.sort(key, axis=1)


@pytest.mark.parametrize("route", ["plain", "cull", "slabs"])
def test_camera_coherent_passes_on_a_device_built_handle(device, lib, route):
    """The pass through the C ABI, then the per-ray repair of the rays it reports as overflowed -- the pipeline of a
    frame -- equals the traversal and the brute force; most rays are answered by the pass itself."""
    from quadraturefields_amd import _C, synthetic
    from quadraturefields_amd.mesh_utils import make_camera
    w, h, k = 64, 48, 5
    mesh = _mesh(3, 3)
    ri = _device_ri(mesh, k, min_separation=0.0)
    c2w, focal = synthetic.orbit_cameras(1, seed=1)[0], synthetic.lego_focal(800) * w / 800.0
    o, d = synthetic.camera_rays(c2w, focal, w, h)
    cam = make_camera(c2w, focal, w, h)
    brute = om.BruteForceIntersector(mesh.vertices, mesh.faces, min_separation=0.0)
    want = brute.hits(o.numpy(), d.numpy(), k)
    total = brute.hits(o.numpy(), d.numpy(), 64)[2]             # every crossing
    own = total <= k                                            # rays the pass answers by itself, without the repair
    assert ((total > 0) & own).mean() > 0.15 and 0 < (~own).sum()
    o, d = o.to(device), d.to(device)
    n = w * h
    tri = torch.full((n, k), -7, dtype=torch.int32, device=device)
    t = torch.full((n, k), float("nan"), device=device)
    words = torch.full((n + 2,), 99, dtype=torch.int32, device=device)
    cnt, ovf, flag = words[:n], words[n:n + 1], words[n + 1:]
    P, st = _C.ptr, _C.stream()
    if route == "slabs":
        wide = 24
        keys = torch.full((wide, n), -1, dtype=torch.int64, device=device)
        _C.check(lib.qf_raster_intersect_slabs(ri._handle, ctypes.byref(cam), P(o), P(d), n, k, wide, 8, P(keys), P(tri), P(t),
                                               P(cnt), P(ovf), P(flag), st), "qf_raster_intersect_slabs")
    else:
        _C.check(lib.qf_raster_intersect(ri._handle, ctypes.byref(cam), P(o), P(d), n, k, P(tri), P(t), P(cnt), P(ovf), 0,
                                         1 if route == "cull" else 0, P(flag), st), "qf_raster_intersect")
    raw = cnt.cpu().numpy().copy()
    assert int(flag.item()) == 0
    # before the repair: the plain pass leaves the raw count of a ray with more than K crossings, the slab pass selects
    # the K nearest itself and keeps a count above K only for a ray that lost candidates
    assert np.array_equal(raw[own], total[own])
    assert bool((raw[~own] >= k).all() if route == "slabs" else (raw[~own] > k).all())
    _C.check(lib.qf_bvh_repair_overflow(ri._handle, P(o), P(d), n, k, w, P(tri), P(t), P(cnt), None, None, P(flag), st),
             "qf_bvh_repair_overflow")
    got_cnt = cnt.cpu().numpy()
    assert np.array_equal(got_cnt, want[2])
    assert np.array_equal(_sorted_keys(tri.cpu().numpy(), t.cpu().numpy(), got_cnt), _sorted_keys(*want))
    trav = ri.hits(o, d, image_width=w)
    assert ri.last_route == "bvh"
    _assert_hits_equal(trav[:3], want)


def test_one_call_frame_pixels_equal_the_host_built_handle(device):
    from quadraturefields_amd import synthetic
    from quadraturefields_amd.mesh_utils import MeshIntersection, make_camera
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceField
    from quadraturefields_amd.render import FrameRenderer
    size, log2_t = 64, 14
    mesh = _mesh(4, 3)
    field = NGPRadianceField(aabb=[-1.5] * 3 + [1.5] * 3, log2_hashmap_size=log2_t)
    field.load_state_dict(synthetic.seeded_ngp_state(log2_t, field.mlp_base.grid.n_rows), strict=False)
    field = field.to(device).eval()
    c2w, focal = synthetic.orbit_cameras(1, seed=2)[0], synthetic.lego_focal(800) * size / 800.0
    o, d = synthetic.camera_rays(c2w, focal, size, size, device=device)
    frames = {}
    for builder in ("host", "device"):
        mi = MeshIntersection(mesh, simplify_mesh=False, num_intersections=25, render_step_size=5e-3, device=device,
                              bvh_builder=builder)
        assert mi.rayintersector.builder == builder and (mi.rayintersector.num_nodes == 0) == (builder == "device")
        rgb, _, depth, n = FrameRenderer(mi, field).render(o, d, camera=make_camera(c2w, focal, size, size))
        assert n > 0
        frames[builder] = (rgb.clone(), depth.clone(), n)
    assert frames["host"][2] == frames["device"][2]
    assert torch.equal(frames["host"][0], frames["device"][0]) and torch.equal(frames["host"][1], frames["device"][1])


# ------------------------------------------------------------------------------------------------ refit and rebuild
@pytest.mark.parametrize("how", ["refit_device", "refit_host", "rebuild_device", "rebuild_host"])
def test_refit_and_rebuild_give_the_moved_mesh(device, how):
    mesh = _mesh(3, 3)
    rng = np.random.default_rng(5)
    moved = (mesh.vertices * np.array([0.8, 1.15, 1.0]) + rng.normal(size=mesh.vertices.shape) * 0.01).astype(np.float32)
    o, d = _rays(1500, seed=8)
    ri = _device_ri(mesh, 10)
    want0 = om.BruteForceIntersector(mesh.vertices, mesh.faces).hits(o, d, 10)
    _assert_hits_equal(ri.hits(o, d)[:3], want0)
    ri._raster_backoff, ri.repaired_frames = 3, 2              # policy state: must survive
    arg = torch.from_numpy(moved).to(device) if how.endswith("device") else moved
    old = ri._handle.value
    if how.startswith("refit"):
        ri.update_intersector(arg)
        assert ri._handle.value == old
    else:
        ri.rebuild(arg)
        assert ri._handle.value and ri.num_nodes == 0
    assert (ri._raster_backoff, ri.repaired_frames) == (3, 2)
    want = om.BruteForceIntersector(moved.astype(np.float64), mesh.faces).hits(o, d, 10)
    assert ri.min_separation == pytest.approx(om.BruteForceIntersector(moved.astype(np.float64), mesh.faces).min_separation)
    assert not np.array_equal(want[0], want0[0])
    _assert_hits_equal(ri.hits(o, d)[:3], want)
    # the flattened triangle soup is accepted too
    if how == "rebuild_device":
        ri.rebuild(torch.from_numpy(moved[mesh.faces].reshape(-1)).to(device))
        _assert_hits_equal(ri.hits(o, d)[:3], want)


# ------------------------------------------------------------------------------------------------ interface
def test_intersector_takes_a_device_tensor(device):
    from quadraturefields_amd import intersector
    mesh = _mesh(2, 3)
    soup = mesh.vertices[mesh.faces].flatten().astype(np.float32)
    o, d = _rays(300, seed=5)
    rays = np.concatenate([o, d], 1).flatten()
    on_dev = intersector.Intersector(torch.from_numpy(soup).to(device), 8, 0)
    on_host = intersector.Intersector(soup, 8, 0)
    assert on_dev.core.builder == "device" and on_host.core.builder == "host"
    assert on_dev.core.num_nodes == 0 and on_host.core.num_nodes > 0
    a, b = np.array(on_dev.find_intersections(rays)), np.array(on_host.find_intersections(rays))
    assert a.shape == (300 * 8,) and np.array_equal(a, b) and (a >= 0).sum() > 100


def test_arguments_are_checked(device, lib):
    from quadraturefields_amd.mesh_utils import RayIntersector
    mesh = _mesh(2, 3)
    with pytest.raises(ValueError):
        RayIntersector(mesh, max_hits=4, builder="nope")
    tri = _soup(mesh).copy()
    tri[17, 1, 2] = np.nan
    with pytest.raises(ValueError):
        _device_ri(_soup_mesh(tri), 4, min_separation=0.0)
    tri_dev = torch.from_numpy(_soup(mesh)).to(device)
    rc, handle = _raw_build(lib, None, n=5)
    assert rc == -1 and not handle.value                       # QF_ERR_INVALID_ARGUMENT
    rc, handle = _raw_build(lib, tri_dev, n=1 << 28)            # refused before anything is read
    assert rc == -1 and not handle.value
    bad = torch.from_numpy(tri).to(device)
    rc, handle = _raw_build(lib, bad)
    assert rc == -1 and not handle.value


def test_depth_complexity_matches_the_fp64_formula(device, lib):
    from quadraturefields_amd.mesh_utils import mesh_depth_complexity
    mesh = _mesh(4, 3)
    tri = _soup(mesh)
    rc, handle = _raw_build(lib, torch.from_numpy(tri).to(device))
    assert rc == 0
    try:
        got = float(lib.qf_bvh_depth_complexity(handle))
    finally:
        lib.qf_bvh_destroy(handle)
    want = mesh_depth_complexity(tri.reshape(-1, 3).astype(np.float64), np.arange(tri.shape[0] * 3).reshape(-1, 3))
    print("depth complexity", got, want, abs(got - want) / want)
    # an fp64 sum of n <= 10^6 terms carries about n * 2^-53 relative error
    assert want > 1.0 and abs(got - want) <= 1e-9 * want
