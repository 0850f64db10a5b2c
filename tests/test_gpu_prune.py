"""Pruning on the device: ``qf_composite_tiles_trimax`` against ``qf_composite_tiles`` +
``qf_scatter_max``, ``qf_frame_prune`` against ``qf_frame_render`` + those two, ``pruning.MeshPruner`` against the
reference-shaped loop, and the example's ``--synthetic`` mode.  Every comparison is exact: the per-sample arithmetic is
the same and a maximum does not depend on the order it is taken in."""
import ctypes
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 44, 20                    # 6 x 3 tiles, partial on both axes
DELTA = 5e-3
VALID = 1e-3


def _C():
    from quadraturefields_amd import _C as c
    return c


def _samples(device, k, max_count, n_tri, seed, bad=0):
    """A synthetic frame in the coherent order: counts (clamped at ``k`` when ``max_count`` > k), tile bases from the
    library's own offsets call, sigma * delta log-uniform over 1e-3 .. 1e4, random colours / depths / triangle ids."""
    C = _C()
    g = torch.Generator().manual_seed(seed)
    hit = torch.randint(0, max_count + 1, (H, W), generator=g, dtype=torch.int32)
    if k == 25:
        hit[0:8, 8:24] = 0       # two whole tiles (and more) without a sample
    hit = hit.reshape(-1).to(device)
    tiles = ((W + 7) // 8) * ((H + 7) // 8)
    tile_base = torch.empty((tiles,), dtype=torch.int64, device=device)
    total = torch.zeros((3,), dtype=torch.int64, device=device)
    C.check(C.lib().qf_tile_offsets(C.ptr(hit), k, W, H, C.ptr(tile_base), C.ptr(total), None, None, None, None, C.stream()),
            "qf_tile_offsets")
    n = int(total[0].item())
    assert n == int(hit.clamp(max=k).sum().item()) and n > 0
    tau = torch.exp(torch.rand(n, generator=g) * (np.log(1e4) - np.log(1e-3)) + np.log(1e-3))
    tri = torch.randint(0, n_tri, (n,), generator=g, dtype=torch.int32)
    planted = 0
    if bad:
        where = torch.randperm(n, generator=g)[:bad]
        tri[where[: bad // 2]] = -1
        tri[where[bad // 2:]] = n_tri
        planted = bad
    return dict(k=k, n=n, hit=hit, tile_base=tile_base, sigma=(tau / DELTA).float().to(device),
                rgb=torch.rand(n, 3, generator=g).to(device), depth=(torch.rand(n, generator=g) * 4 + 2).to(device),
                tri=tri.to(device), n_tri=n_tri, bad=planted)


def _images(device):
    n = W * H
    return [torch.full((n, 3), -7.0, device=device), torch.full((n, 1), -7.0, device=device),
            torch.full((n, 1), -7.0, device=device)]


def _unfused(s, tw, device):
    """qf_composite_tiles(weights_c) then qf_scatter_max over the valid ids, into ``tw`` in place.  Returns (images,
    samples, samples above VALID, ids outside the mesh)."""
    C = _C()
    img = _images(device)
    weights = torch.full((s["n"],), -1.0, device=device)
    C.check(C.lib().qf_composite_tiles(C.ptr(s["rgb"]), C.ptr(s["sigma"]), C.ptr(s["depth"]), DELTA, C.ptr(s["hit"]), s["k"],
                                       C.ptr(s["tile_base"]), W, H, C.BG_WHITE, None, C.ptr(img[0]), C.ptr(img[1]),
                                       C.ptr(img[2]), C.ptr(weights), None, C.stream()), "qf_composite_tiles")
    assert bool((weights >= 0).all()), "every slot of the frame carries a weight"
    ids = s["tri"].long()
    ok = (ids >= 0) & (ids < s["n_tri"])
    w_ok, i_ok = weights[ok].contiguous(), ids[ok].contiguous()
    C.check(C.lib().qf_scatter_max(C.ptr(w_ok), C.ptr(i_ok), w_ok.shape[0], s["n_tri"], C.ptr(tw), C.stream()), "qf_scatter_max")
    return img, s["n"], int((weights > VALID).sum().item()), int((~ok).sum().item()), weights


def _trimax(s, tw, counts, bad, device, image=True):
    C = _C()
    img = _images(device) if image else [None, None, None]
    C.check(C.lib().qf_composite_tiles_trimax(
        C.ptr(s["rgb"]), C.ptr(s["sigma"]), C.ptr(s["depth"]), DELTA, C.ptr(s["hit"]), s["k"], C.ptr(s["tile_base"]), W, H,
        C.BG_WHITE, None, C.ptr(img[0]), C.ptr(img[1]), C.ptr(img[2]), None, C.ptr(s["tri"]), C.ptr(tw), s["n_tri"], VALID,
        C.ptr(counts), C.ptr(bad), C.stream()), "qf_composite_tiles_trimax")
    return img


@pytest.mark.parametrize("k,max_count,n_tri,seeded", [(4, 7, 5, False), (4, 7, 100003, True), (25, 25, 5, True),
                                                      (25, 25, 100003, False)])
def test_trimax_compositor_equals_composite_then_scatter_max(device, k, max_count, n_tri, seeded):
    s = _samples(device, k, max_count, n_tri, seed=100 + k + n_tri % 7, bad=6 if seeded else 0)
    if k == 4:
        assert int(s["hit"].max()) > k, "no count beyond K: clamping is not exercised"
    g = torch.Generator().manual_seed(3)
    start = (torch.rand(n_tri, generator=g) * 0.5).to(device) if seeded else torch.zeros(n_tri, device=device)
    want_tw = start.clone()
    want_img, want_n, want_valid, want_bad, weights = _unfused(s, want_tw, device)
    assert want_bad == s["bad"]
    # the inputs span the cases that matter: weights below the threshold, near one, and exact zeros after saturation
    assert bool((weights == 0).any()) and bool((weights > 0.9).any()) and bool(((weights > 0) & (weights < VALID)).any())
    tw = start.clone()
    counts = torch.zeros((2,), dtype=torch.int64, device=device)
    bad = torch.zeros((1,), dtype=torch.int32, device=device)
    img = _trimax(s, tw, counts, bad, device)
    assert torch.equal(tw, want_tw)
    assert counts.tolist() == [want_n, want_valid] and want_valid < want_n
    assert int(bad.item()) == s["bad"]
    for a, b in zip(img, want_img):
        assert torch.equal(a, b)
    # without an image: the same maxima; counters are added to
    tw2 = start.clone()
    _trimax(s, tw2, counts, bad, device, image=False)
    assert torch.equal(tw2, want_tw)
    assert counts.tolist() == [2 * want_n, 2 * want_valid] and int(bad.item()) == 2 * s["bad"]
    # a second pass over settled maxima changes nothing (every sample loses the read-before-atomic comparison)
    _trimax(s, tw2, counts, bad, device, image=False)
    assert torch.equal(tw2, want_tw)


@pytest.mark.parametrize("n_tri", [5, 100003])
def test_trimax_does_not_depend_on_the_order_of_the_calls(device, n_tri):
    a = _samples(device, 25, 25, n_tri, seed=11)
    b = _samples(device, 4, 7, n_tri, seed=12)
    out = []
    for order in ((a, b), (b, a)):
        tw = torch.zeros(n_tri, device=device)
        counts = torch.zeros((2,), dtype=torch.int64, device=device)
        bad = torch.zeros((1,), dtype=torch.int32, device=device)
        for s in order:
            _trimax(s, tw, counts, bad, device, image=False)
        out.append((tw, counts))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    want = torch.zeros(n_tri, device=device)
    _unfused(a, want, device)
    _unfused(b, want, device)
    assert torch.equal(out[0][0], want)


def test_trimax_refuses_a_half_given_image(device):
    C = _C()
    s = _samples(device, 4, 7, 5, seed=1)
    tw = torch.zeros(5, device=device)
    img = _images(device)
    rc = C.lib().qf_composite_tiles_trimax(
        C.ptr(s["rgb"]), C.ptr(s["sigma"]), C.ptr(s["depth"]), DELTA, C.ptr(s["hit"]), 4, C.ptr(s["tile_base"]), W, H,
        C.BG_WHITE, None, C.ptr(img[0]), None, None, None, C.ptr(s["tri"]), C.ptr(tw), 5, VALID, None, None, C.stream())
    assert rc == -1
    rc = C.lib().qf_composite_tiles_trimax(
        C.ptr(s["rgb"]), C.ptr(s["sigma"]), C.ptr(s["depth"]), DELTA, C.ptr(s["hit"]), 4, C.ptr(s["tile_base"]), W, H,
        C.BG_WHITE, None, None, None, None, None, None, C.ptr(tw), 5, VALID, None, None, C.stream())
    assert rc == -1              # no triangle ids


# ---------------------------------------------------------------------------------------------------------
FW, FH = 48, 40


@pytest.fixture(scope="module")
def scene(device):
    from quadraturefields_amd import synthetic
    from quadraturefields_amd.mesh_utils import make_camera
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceField
    mesh = synthetic.shell_mesh(n_shells=3, subdivisions=2)
    field = NGPRadianceField(aabb=[-1.5] * 3 + [1.5] * 3, log2_hashmap_size=12)
    field.load_state_dict(synthetic.seeded_ngp_state(12, field.mlp_base.grid.n_rows), strict=False)
    field = field.to(device)
    focal = synthetic.lego_focal(800) * FW / 800.0 * 2.0            # the shells fill the frame
    views = []
    deep = _intersection(mesh, 16)
    for c2w in synthetic.orbit_cameras(3, seed=9):
        o, d = synthetic.camera_rays(c2w, focal, FW, FH, device=device)
        views.append((o, d, make_camera(c2w, focal, FW, FH)))
        # central rays cross every shell twice: at K = 4 their lists clamp, at K = 8 they do not
        crossings = int(torch.bincount(deep.sampling_raytrace_device(d, o)[2]).max())
        assert 4 < crossings <= 8, crossings
    return mesh, field, views, focal


def _intersection(mesh, k):
    from quadraturefields_amd.mesh_utils import MeshIntersection
    mi = MeshIntersection(mesh, simplify_mesh=False, scale=1.0, num_intersections=k, render_step_size=DELTA)
    assert mi.rayintersector.min_separation > 0
    return mi


def _plain_pass(ri, bins):
    """Keep the intersector on the plain camera-coherent pass (what qf_frame_render / qf_frame_prune compose), whatever
    the overflow counts of the earlier frames said: at K = 4 most central rays overflow."""
    ri._settle_fused_policy(0)
    ri._policy_seeded, ri.raster_wide, ri._raster_backoff, ri._rule_upfront = True, 0, 0, 0
    ri.hit_bins = bins


def _job(fr, ri, view, k, bins):
    _plain_pass(ri, bins)
    o, d, cam = view
    assert ri.fused_frame_ready(cam, k)
    prepared = fr._one_call_job(o, d, cam, k, None, False, want_tri=True)
    assert prepared is not None
    return prepared


@pytest.mark.parametrize("k", [4, 8])
@pytest.mark.parametrize("route", ["bins", "lists"])
def test_frame_prune_only_composes(device, scene, k, route):
    C = _C()
    from quadraturefields_amd.render import FrameRenderer
    mesh, field, views, _ = scene
    mi = _intersection(mesh, k)
    ri = mi.rayintersector
    fr = FrameRenderer(mi, field)
    n_tri = int(mesh.faces.shape[0])
    bins = route == "bins"
    tw = torch.zeros(n_tri, device=device)
    want_tw = torch.zeros(n_tri, device=device)
    counts = torch.zeros((len(views), 2), dtype=torch.int64, device=device)
    bad = torch.zeros((1,), dtype=torch.int32, device=device)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i, view in enumerate(views):
            def render():
                job, frame, token, keep, img = _job(fr, ri, view, k, bins)
                C.check(C.lib().qf_frame_render(ri._handle, ctypes.byref(job), C.stream()), "qf_frame_render")
                ri.fused_frame_done(frame, token)
                return frame, keep, [t.clone() for t in img[:3]]

            frame, keep, before = render()
            rgbs, sigmas = keep[0], keep[1]
            # the unfused composition on the frame's own arrays
            cap = frame.total
            weights = torch.full((cap,), -1.0, device=device)
            img = [torch.empty((FW * FH, c), device=device) for c in (3, 1, 1)]
            C.check(C.lib().qf_composite_tiles(C.ptr(rgbs), C.ptr(sigmas), C.ptr(frame.depth_c), DELTA, C.ptr(frame.hit_count),
                                               k, C.ptr(frame.tile_base), FW, FH, C.BG_WHITE, None, C.ptr(img[0]),
                                               C.ptr(img[1]), C.ptr(img[2]), C.ptr(weights), None, C.stream()),
                    "qf_composite_tiles")
            live = weights >= 0
            n = int(live.sum().item())
            assert n == int(frame.hit_count.sum().item()) == ri.frame_samples(frame) and n > 500
            w_l, i_l = weights[live].contiguous(), frame.tri_c[live].long().contiguous()
            assert int(i_l.min()) >= 0 and int(i_l.max()) < n_tri
            C.check(C.lib().qf_scatter_max(C.ptr(w_l), C.ptr(i_l), n, n_tri, C.ptr(want_tw), C.stream()), "qf_scatter_max")
            want_counts = [n, int((w_l > VALID).sum().item())]
            for a, b in zip(img, before):
                assert torch.equal(a, b)
            # the one call
            job, pframe, token, pkeep, pimg = _job(fr, ri, view, k, bins)
            C.check(C.lib().qf_frame_prune(ri._handle, ctypes.byref(job), C.ptr(tw), n_tri, VALID, C.ptr(counts[i]),
                                           C.ptr(bad), C.stream()), "qf_frame_prune")
            ri.fused_frame_done(pframe, token)
            assert torch.equal(tw, want_tw), f"view {i}"
            assert counts[i].tolist() == want_counts
            for a, b in zip(pimg[:3], before):
                assert torch.equal(a, b)
            assert torch.equal(pframe.tri_c[live], frame.tri_c[live])
            # ... and qf_frame_render afterwards draws what it drew before
            _, _, after = render()
            for a, b in zip(after, before):
                assert torch.equal(a, b)
        assert int(bad.item()) == 0
        assert bool((want_tw > 0).any()) and bool((want_tw == 0).any())
        # validated before the first launch: no field, no ids, no maxima
        job, frame, token, keep, _ = _job(fr, ri, views[0], k, bins)
        saved = job.tri_c
        job.tri_c = None
        assert C.lib().qf_frame_prune(ri._handle, ctypes.byref(job), C.ptr(tw), n_tri, VALID, None, None, C.stream()) == -1
        job.tri_c = saved
        assert C.lib().qf_frame_prune(ri._handle, ctypes.byref(job), None, n_tri, VALID, None, None, C.stream()) == -1
        job.out_alpha = None         # a half-given image
        assert C.lib().qf_frame_prune(ri._handle, ctypes.byref(job), C.ptr(tw), n_tri, VALID, None, None, C.stream()) == -1
        job.out_rgb = job.out_depth = None
        C.check(C.lib().qf_frame_prune(ri._handle, ctypes.byref(job), C.ptr(tw), n_tri, VALID, None, None, C.stream()),
                "qf_frame_prune without an image")
        ri.fused_frame_done(frame, token)
        assert torch.equal(tw, want_tw)
        ri._settle_fused_policy(0)
    ri.hit_bins = True


def _loader_route(mi, field, views, device, camera=True):
    """The reference-shaped loop: render_image_finetune_with_occgrid(scaling=0) -> weights, index_tri -> scatter-max per
    view -> running maximum; the per-view host counts."""
    from quadraturefields_amd import baking, utils
    from quadraturefields_amd.datasets.utils import Rays
    n_tri = int(mi.mesh.faces.shape[0])
    tw = torch.zeros(n_tri, device=device)
    samples, num, valid = [], [], []
    for o, d, cam in views:
        data = mi.sampling_raytrace_device(d, o, camera=cam) if camera else mi.sampling_raytrace_device(d, o, image_width=FW)
        out = utils.render_image_finetune_with_occgrid(field, None, None, Rays(origins=o, viewdirs=d), data,
                                                       render_step_size=DELTA, mesh_intersect=mi, scaling=0.0)
        weights, index_tri = out[4], out[8]
        num.append(len(weights))
        valid.append(int(torch.sum(weights > 0.001).item()))
        tw_i = baking.triangle_max_weights(weights[:, 0], index_tri, torch.zeros_like(tw))
        tw = torch.maximum(tw, tw_i)
        samples.append((weights, index_tri))
    return tw, num, valid, samples


@pytest.mark.parametrize("k", [4, 8])
def test_mesh_pruner_equals_the_reference_shaped_loop(device, scene, k):
    from quadraturefields_amd.pruning import MeshPruner
    mesh, field, views, focal = scene
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want_tw, want_num, want_valid, samples = _loader_route(_intersection(mesh, k), field, views, device)
        thr = float(want_tw.median().item())
        want_mask = want_tw > thr
        assert bool(want_mask.any()) and not bool(want_mask.all())

        mi = _intersection(mesh, k)
        pruner = MeshPruner(mi, field, threshold=thr)
        for o, d, cam in views:
            pruner.add_view(o, d, cam)
        assert pruner.triangle_weights.is_cuda and pruner.triangle_weights.shape == (mesh.faces.shape[0],)
        diff = torch.nonzero(pruner.triangle_weights != want_tw)
        assert diff.numel() == 0, f"triangle_weights first differs at face {int(diff[0])}"
        num, valid = pruner.sample_counts()
        assert num.dtype == valid.dtype == np.int64
        assert num.tolist() == want_num and valid.tolist() == want_valid
        assert torch.equal(pruner.keep_mask(), want_mask)
        pruned = pruner.pruned_mesh()
        assert np.array_equal(pruned.faces, mesh.faces[want_mask.cpu().numpy()])
        assert np.array_equal(pruned.vertices, mesh.vertices) and np.array_equal(pruned.visual.uv, mesh.visual.uv)

        # the general route over the same samples
        general = MeshPruner(_intersection(mesh, k), field, threshold=thr)
        for weights, index_tri in samples:
            general.add_samples(weights, index_tri)
        assert torch.equal(general.triangle_weights, want_tw)
        num, valid = general.sample_counts()
        assert num.tolist() == want_num and valid.tolist() == want_valid
        bad_ids = samples[0][1].clone()
        bad_ids[0] = mesh.faces.shape[0]
        general.add_samples(samples[0][0], bad_ids)
        with pytest.raises(IndexError):
            general.sample_counts()

        # rays that are not their camera's pixel grid (jittered directions): the device-side check sends the view through
        # the BVH; same weights as the camera-less loop on those rays
        g = torch.Generator().manual_seed(1)
        jittered = []
        for o, d, cam in views:
            dj = d + (torch.rand(FW * FH, 3, generator=g).to(device) - 0.5) * (1.0 / focal)
            jittered.append((o, (dj / dj.norm(dim=1, keepdim=True)).contiguous(), cam))
        want_j, num_j, valid_j, _ = _loader_route(_intersection(mesh, k), field, jittered, device, camera=False)
        mi_j = _intersection(mesh, k)
        pj = MeshPruner(mi_j, field)
        for o, d, cam in jittered:
            pj.add_view(o, d, cam)
        assert torch.equal(pj.triangle_weights, want_j)
        num, valid = pj.sample_counts()
        assert num.tolist() == num_j and valid.tolist() == valid_j
        mi_j.rayintersector._settle_deferred_policy()
        assert mi_j.rayintersector.camera_mismatch_frames >= 1


def test_counts_table_grows(device, scene):
    """More views than the table's first capacity: rows keep their values across the growth."""
    from quadraturefields_amd.pruning import MeshPruner
    mesh, field, views, _ = scene
    pruner = MeshPruner(_intersection(mesh, 8), field)
    o, d, cam = views[0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for _ in range(pruner._counts.shape[0] + 1):
            pruner.add_view(o, d, cam)
    num, valid = pruner.sample_counts()
    assert num.shape == (pruner.n_views,) and len(set(num.tolist())) == 1 and len(set(valid.tolist())) == 1 and num[0] > 0


def test_synthetic_example_writes_the_four_files(device, tmp_path):
    from quadraturefields_amd.mesh_io import load_mesh
    out = str(tmp_path / "prune")
    cmd = [sys.executable, os.path.join(ROOT, "examples", "prune_mesh_after_finetuning.py"), "--synthetic", out, "--size", "96",
           "--up_sample", "2", "--views", "4", "--shells", "3", "--subdivisions", "3", "--max_hits", "8",
           "--log2_hashmap_size", "12", "--optix", "False", "--exp_name", "unused"]
    proc = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    for name in ("triangle_weights.npy", "mesh_updated.ply", "num_samples.npy", "num_valid_samples.npy"):
        assert os.path.exists(os.path.join(out, name)), name
    before, after = load_mesh(os.path.join(out, "mesh.ply")), load_mesh(os.path.join(out, "mesh_updated.ply"))
    tw = np.load(os.path.join(out, "triangle_weights.npy"))
    assert tw.dtype == np.float32 and tw.shape == (before.faces.shape[0],)
    assert 0 < after.faces.shape[0] < before.faces.shape[0]
    assert after.faces.shape[0] == int((tw > np.float32(1e-3)).sum())
    assert after.vertices.shape == before.vertices.shape
    ns, nv = np.load(os.path.join(out, "num_samples.npy")), np.load(os.path.join(out, "num_valid_samples.npy"))
    assert ns.shape == nv.shape == (4,) and ns.dtype == nv.dtype == np.int64 and bool((nv <= ns).all()) and bool((ns > 0).all())
    assert "Number of faces after pruning" in proc.stdout
