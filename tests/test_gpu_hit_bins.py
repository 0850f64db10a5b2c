"""The hit-bin route of a render-only camera frame (qf_raster_intersect_tiles -> qf_bvh_repair_overflow -> qf_tile_offsets ->
qf_pack_tiles_bins): the same frame, bit for bit, as the per-ray-list route (``RayIntersector.hit_bins = False``) and as
the camera-less BVH route -- samples, counts, tile bases, total and pixels."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K = 25


def _field(device, log2_T=14):
    from quadraturefields_amd import synthetic
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceField
    field = NGPRadianceField(aabb=[-1.5] * 3 + [1.5] * 3, log2_hashmap_size=log2_T)
    field.load_state_dict(synthetic.seeded_ngp_state(log2_T, field.mlp_base.grid.n_rows), strict=False)
    return field.to(device)


def _sample(ri, o, d, cam, route, k=K, want_tri=False):
    """One frame through ``sample_frame_device`` on ``route`` ("bins", "lists" or "bvh"), every output cloned."""
    ri._raster_backoff = 1 if route == "bvh" else 0
    ri.hit_bins = route == "bins"
    if route == "bins":
        assert ri._hit_bins_ready(k, cam), "the frame is not on the plain pass: the binned route would not be taken"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        frame = ri.sample_frame_device(o, d, k, cam, want_tri=want_tri)
        _, xyz_c, dirs_c = ri.last_layout
        total = int(frame.total_dev.item())
        n = ri.frame_samples(frame)
    out = dict(xyz=xyz_c[:total].clone(), dirs=dirs_c[:total].clone(), depth=frame.depth_c[:total].clone(),
               final_count=frame.hit_count.clone(), tile_base=frame.tile_base.clone(), total=total, samples=n)
    if want_tri:
        out["tri"] = frame.tri_c[:total].clone()
    ri.hit_bins = True
    return out


def _kept_index(f, w, h):
    """Positions of a frame's kept samples in its coherent arrays: tile T's are the first sum(final_count over T) slots
    from tile_base[T] (what the re-origin rule dropped leaves a gap at the END of the tile's slots)."""
    tx, ty = (w + 7) // 8, (h + 7) // 8
    c = torch.zeros((ty * 8, tx * 8), dtype=torch.int64, device=f["final_count"].device)
    c[:h, :w] = f["final_count"].reshape(h, w)
    kept = c.reshape(ty, 8, tx, 8).sum(dim=(1, 3)).reshape(-1)
    first = torch.repeat_interleave(f["tile_base"] - (torch.cumsum(kept, 0) - kept), kept)
    return first + torch.arange(int(kept.sum()), device=first.device)


def _same(a, b, what, shape=None):
    """Bitwise equal frames.  ``shape`` = (w, h): ``b`` is the BVH route's frame, whose traversal applies the re-origin
    rule before the slots are allotted -- no gaps, other tile bases -- so the KEPT samples are compared, tile by tile."""
    assert a["samples"] == b["samples"], (what, a["samples"], b["samples"])
    assert torch.equal(a["final_count"], b["final_count"]), (what, "final_count")
    if shape is None:
        assert a["total"] == b["total"], (what, a["total"], b["total"])
        for key in a:
            if torch.is_tensor(a[key]):
                assert torch.equal(a[key], b[key]), (what, key)
        return
    ia, ib = _kept_index(a, *shape), _kept_index(b, *shape)
    assert ia.numel() == ib.numel() == a["samples"]
    for key in ("xyz", "dirs", "depth", "tri"):
        if key in a:
            assert torch.equal(a[key][ia], b[key][ib]), (what, key)


def _poses():
    from quadraturefields_amd import synthetic
    close = synthetic.orbit_cameras(1, seed=5)[0].clone()
    close[:, 3] *= 0.3                                   # the grazing close-up of test_raster_guard_band_is_conservative
    return {"orbit": synthetic.orbit_cameras(3, seed=11)[1], "close": close}


@pytest.fixture(scope="module")
def bench_scene(device):
    """The bench scene: 12 shells, 983 040 triangles."""
    from quadraturefields_amd import synthetic
    from quadraturefields_amd.mesh_utils import MeshIntersection
    mesh = synthetic.shell_mesh(n_shells=12, subdivisions=6)
    mi = MeshIntersection(mesh, simplify_mesh=False, scale=1.0, num_intersections=K)
    return mi, _field(device)


@pytest.mark.parametrize("w,h,pose", [(800, 800, "orbit"), (1920, 1080, "orbit"), (800, 800, "close")])
def test_binned_frame_equals_the_list_route_and_the_bvh(device, bench_scene, w, h, pose):
    """800x800, 1080p (135 tile rows: the last row of tiles is half outside the image) and the grazing close-up:
    ``sample_frame_device`` and ``qf_frame_render`` (``render_async``) on the bins == on the per-ray lists == the
    camera-less BVH route, bitwise."""
    from quadraturefields_amd import synthetic
    from quadraturefields_amd.mesh_utils import make_camera
    from quadraturefields_amd.render import FrameRenderer
    mi, field = bench_scene
    ri = mi.rayintersector
    focal = synthetic.lego_focal(w)
    c2w = _poses()[pose]
    o, d = synthetic.camera_rays(c2w, focal, w, h, device=device)
    cam = make_camera(c2w, focal, w, h)
    bins = _sample(ri, o, d, cam, "bins")
    assert bins["total"] > 100000
    _same(bins, _sample(ri, o, d, cam, "lists"), "lists")
    _same(bins, _sample(ri, o, d, cam, "bvh"), "bvh", (w, h))
    fr = FrameRenderer(mi, field)
    images = {}
    for route in ("bins", "lists"):
        ri._raster_backoff = 0
        ri.hit_bins = route == "bins"
        assert ri.fused_frame_ready(cam, K)
        rgb, alpha, depth, frame = fr.render_async(o, d, cam)
        images[route] = (rgb.clone(), alpha.clone(), depth.clone(), frame.hit_count.clone(), frame.tile_base.clone(),
                         int(frame.total_dev.item()))
        ri._settle_fused_policy(0)
    ri.hit_bins = True
    want = fr.render(o, d, image_width=w)                 # camera-less: the BVH traversal
    for a, b in zip(images["bins"][:5], images["lists"][:5]):
        assert torch.equal(a, b)
    assert images["bins"][5] == images["lists"][5] == bins["total"]
    assert torch.equal(images["bins"][3], bins["final_count"]) and torch.equal(images["bins"][4], bins["tile_base"])
    for a, b in zip(images["bins"][:3], want[:3]):
        assert torch.equal(a, b)


def test_overflowed_pixels_and_tiles_are_repaired_exactly(device):
    """K = 23 on the 12-shell mesh (subdivision 3, 200x200, orbit seed 3): rays through the innermost shell meet 24
    faces.  Measured on the CPU oracle (oracle.meshpath.BVHIntersector, every hit): 242 679 candidates, 1 341 of them
    beyond K = 0.55 %, on 1 341 pixels = 3.4 % of the rays (the policy leaves the plain pass above 5 % of the ray count),
    and 21 central tiles hold more than 64 K candidates, so their whole bin overflows.  The samples must be the BVH
    route's."""
    from quadraturefields_amd import synthetic
    from quadraturefields_amd.mesh_utils import MeshIntersection, make_camera
    k = 23
    mesh = synthetic.shell_mesh(n_shells=12, subdivisions=3)
    mi = MeshIntersection(mesh, simplify_mesh=False, scale=1.0, num_intersections=k)
    ri = mi.rayintersector
    w = h = 200
    focal = synthetic.lego_focal(800) * w / 800.0
    c2w = synthetic.orbit_cameras(1, seed=3)[0]
    o, d = synthetic.camera_rays(c2w, focal, w, h, device=device)
    cam = make_camera(c2w, focal, w, h)
    bins = _sample(ri, o, d, cam, "bins", k=k)
    # what the route saw on the device: both kinds of overflow occurred
    cursor, mask, _records = next(iter(ri._bin_scratch_sets.values()))
    n_tiles = (w // 8) * (h // 8)
    cursor, mask = cursor[:n_tiles].cpu().numpy(), mask[:n_tiles].cpu().numpy().view(np.uint64)
    assert int((cursor > 64 * k).sum()) >= 10, "no tile bin overflowed"
    assert np.all(mask[cursor > 64 * k] == np.uint64(0xFFFFFFFFFFFFFFFF))
    partly = (cursor <= 64 * k) & (mask != 0)
    assert int(partly.sum()) >= 1, "no tile with single overflowed pixels"
    assert abs(int(cursor.sum()) - 242679) <= 16          # the oracle's count (rays through a shared edge count twice here)
    ri._settle_deferred_policy()
    assert int(ri.raster_wide) <= k and ri._raster_backoff <= 0, "0.55 % of the candidates moved the policy off the plain pass"
    _same(bins, _sample(ri, o, d, cam, "bvh", k=k), "bvh", (w, h))
    _same(bins, _sample(ri, o, d, cam, "lists", k=k), "lists")


def test_raised_ray_flag_sends_the_binned_frame_through_the_bvh(device):
    """Half-pixel jitter and a stale camera: the pass's ray check raises its flag, the bins stay empty, the repair launch
    traverses every ray and the pack reads the per-ray rows -- the camera-less BVH frame, bit for bit."""
    from quadraturefields_amd import synthetic
    from quadraturefields_amd.mesh_utils import MeshIntersection, make_camera
    mesh = synthetic.shell_mesh(n_shells=4, subdivisions=4)
    mi = MeshIntersection(mesh, simplify_mesh=False, scale=1.0, num_intersections=K)
    ri = mi.rayintersector
    w, h = 136, 96
    focal = synthetic.lego_focal(800) * w / 800.0
    cams = synthetic.orbit_cameras(2, seed=5)
    o, d = synthetic.camera_rays(cams[1], focal, w, h, device=device)
    cam = make_camera(cams[1], focal, w, h)
    g = torch.Generator().manual_seed(1)
    dj = d + (torch.rand(w * h, 3, generator=g).to(device) - 0.5) * (1.0 / focal)
    dj = (dj / dj.norm(dim=1, keepdim=True)).contiguous()
    stale = make_camera(cams[0], focal, w, h)
    for o2, d2, cam2 in ((o, dj, cam), (o, d, stale)):
        before = ri.camera_mismatch_frames
        bins = _sample(ri, o2, d2, cam2, "bins")
        ri._settle_deferred_policy()
        assert ri.camera_mismatch_frames == before + 1
        assert bins["total"] > 1000
        _same(bins, _sample(ri, o2, d2, cam2, "bvh"), "bvh", (w, h))


def test_binned_frame_with_triangle_ids_and_the_baked_texture_frame(device):
    """Ids wanted: the samples' triangle ids come out of the bins' records as out of the per-ray lists; and the
    baked-texture frame (``render_baked_async``) equals ``render_baked``."""
    from quadraturefields_amd import synthetic
    from quadraturefields_amd.mesh_utils import MeshIntersection, make_camera
    from quadraturefields_amd.render import FrameRenderer
    mesh = synthetic.shell_mesh(n_shells=6, subdivisions=4)
    mi = MeshIntersection(mesh, simplify_mesh=False, scale=1.0, num_intersections=K)
    ri = mi.rayintersector
    w, h = 264, 200
    focal = synthetic.lego_focal(800) * w / 800.0
    c2w = synthetic.orbit_cameras(1, seed=2)[0]
    o, d = synthetic.camera_rays(c2w, focal, w, h, device=device)
    cam = make_camera(c2w, focal, w, h)
    bins = _sample(ri, o, d, cam, "bins", want_tri=True)
    assert int(bins["tri"].max()) > 0
    _same(bins, _sample(ri, o, d, cam, "lists", want_tri=True), "lists")
    _same(bins, _sample(ri, o, d, cam, "bvh", want_tri=True), "bvh", (w, h))
    # the baked-texture frame on both sampling routes it can take: the one-call sampling half (qf_frame_render without a
    # field has no field outputs to carve bins from and stays on the per-ray lists) and sample_frame_device on the bins
    from quadraturefields_amd.texture_utils import FeatureCompression
    lobes, size = 6, 256
    tex = synthetic.random_textures(size, lobes, seed=1)
    comp = FeatureCompression.from_arrays(tex["alpha"], tex["diffuse"], tex["colors"], tex["lambdas"],
                                          compression_type="sigmoid", lambda_thres=7.5)
    uv = torch.from_numpy(synthetic.scaled_uv(mesh, size)).to(device)
    fr = FrameRenderer(mi, _field(device))
    ri._raster_backoff = 0
    want = fr.render_baked(o, d, uv, comp, camera=cam)
    for one_call in (True, False):
        ri._raster_backoff = 0
        if not one_call:
            ri.fused_frame_ready = lambda *a, **k: False      # -> sample_frame_device(want_tri=True)
        got = fr.render_baked_async(o, d, uv, comp, cam)
        assert ri.frame_samples() == want[3]
        for a_, b_ in zip(got[:3], want[:3]):
            assert torch.equal(a_, b_)
    del ri.fused_frame_ready


def test_a_frame_after_a_frame_leaves_nothing_behind(device, bench_scene):
    """A, B, A on one intersector (another pose, then another resolution in between): cursors and bins are per frame."""
    from quadraturefields_amd import synthetic
    from quadraturefields_amd.mesh_utils import make_camera
    mi, _ = bench_scene
    ri = mi.rayintersector
    cams = synthetic.orbit_cameras(3, seed=7)

    def frame(c2w, w, h):
        focal = synthetic.lego_focal(800) * w / 800.0
        o, d = synthetic.camera_rays(c2w, focal, w, h, device=device)
        return _sample(ri, o, d, make_camera(c2w, focal, w, h), "bins")

    a0 = frame(cams[0], 400, 400)
    frame(cams[1], 400, 400)
    a1 = frame(cams[0], 400, 400)
    _same(a0, a1, "A B A")
    frame(cams[2], 640, 360)                              # more tiles per row, fewer rows: every tile's bin moves
    frame(cams[2], 200, 120)
    _same(a0, frame(cams[0], 400, 400), "A after other resolutions")
