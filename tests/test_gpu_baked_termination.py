"""The front-to-back baked frame with early ray termination (``qf_texture_composite_tiles`` / ``qf_frame_render_baked``,
``FrameRenderer.render_baked(..., early_stop_eps=)``) against code that exists without it:

* ``eps = 0`` is ``render_baked`` without the keyword, bit for bit;
* ``eps > 0`` is the existing unfused shading (``utils.shade_baked_points``) on the ray-major samples, truncated on the
  host by the numpy rule of ``tests/baked_termination_reference.py`` and composited by ``utils.derive_properties`` --
  counts and pixels exactly;
* the one bound call equals the separately bound launches and refuses a spoiled job before its first launch.

Shapes: 37x29 (partial tiles on both edges), 8x8 (one tile), 64x40; K in {1, 5, 25} (K = 5 truncates pixels that have up
to 16 hits); 1 and 6 lobes; white and black background; both colour codecs; a texture set whose alpha plane holds the
codes 0 and 255.  The eleven combinations below cover every value of every axis and every pair (frame, K)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import baked_termination_reference as T

pytestmark = pytest.mark.gpu

DELTA = 5e-3
SIZE = 256
# (width, height, K, lobes, background, compression_type, alpha plane)
CONFIGS = [
    (37, 29, 25, 6, "white", "sigmoid", "random"),          # the named scene of test_baked_termination_host.py
    (37, 29, 25, 1, "black", "sigma", "extremes"),
    (37, 29, 5, 6, "black", "sigmoid", "extremes"),
    (37, 29, 1, 1, "white", "sigma", "random"),
    (8, 8, 25, 6, "white", "sigma", "extremes"),
    (8, 8, 5, 1, "black", "sigmoid", "random"),
    (8, 8, 1, 6, "black", "sigma", "random"),
    (64, 40, 25, 1, "white", "sigmoid", "extremes"),
    (64, 40, 5, 6, "white", "sigma", "random"),
    (64, 40, 1, 1, "black", "sigmoid", "extremes"),
    (64, 40, 25, 6, "black", "sigma", "random"),
]
_IDS = ["-".join(str(v) for v in c) for c in CONFIGS]
_cache = {}


def _mesh():
    from quadraturefields_amd import synthetic
    if "mesh" not in _cache:
        _cache["mesh"] = synthetic.shell_mesh(n_shells=8, subdivisions=2)
    return _cache["mesh"]


def _intersection(k):
    from quadraturefields_amd.mesh_utils import MeshIntersection
    if ("mi", k) not in _cache:
        _cache[("mi", k)] = MeshIntersection(_mesh(), simplify_mesh=False, scale=1.0, num_intersections=k)
    return _cache[("mi", k)]


def _textures(lobes, plane):
    from quadraturefields_amd import synthetic
    tex = synthetic.random_textures(SIZE, lobes, seed=1)
    if plane == "extremes":            # fully transparent and fully opaque codes next to each other, all over the charts
        tex["alpha"][::3, ::5] = 255
        tex["alpha"][1::4, ::2] = 0
        assert (tex["alpha"] == 0).any() and (tex["alpha"] == 255).any()
    elif plane == "opaque":
        tex["alpha"][:] = 255
    return tex


def _compressor(device, lobes, codec, plane):
    from quadraturefields_amd.texture_utils import FeatureCompression
    key = ("comp", lobes, codec, plane)
    if key not in _cache:
        tex = _textures(lobes, plane)
        _cache[key] = FeatureCompression.from_arrays(tex["alpha"], tex["diffuse"], tex["colors"], tex["lambdas"],
                                                     compression_type=codec, lambda_thres=7.5, device=device)
    return _cache[key]


def _scene(device, w, h, k, lobes, bg, codec, plane):
    """Renderer, rays, camera, uv and texture set of one configuration, and (computed once per configuration, never
    modified) the ray-major samples with the colours and densities of the existing unfused shading."""
    from quadraturefields_amd import synthetic, utils
    from quadraturefields_amd.mesh_utils import make_camera
    from quadraturefields_amd.render import FrameRenderer
    key = ("scene", w, h, k, lobes, bg, codec, plane)
    if key in _cache:
        return _cache[key]
    mi = _intersection(k)
    comp = _compressor(device, lobes, codec, plane)
    if "uv" not in _cache:
        _cache["uv"] = torch.from_numpy(synthetic.scaled_uv(_mesh(), SIZE)).to(device)
    uv = _cache["uv"]
    c2w = synthetic.orbit_cameras(1, seed=4)[0]
    focal = synthetic.lego_focal(800) * w / 800.0
    o, d = synthetic.camera_rays(c2w, focal, w, h, device=device)
    cam = make_camera(c2w, focal, w, h)
    fr = FrameRenderer(mi, None, bg_color=bg)
    assert fr.render_step_size == DELTA
    xyzs, dirs, index_ray, ts, index_tri, _ = mi.sampling_raytrace_device(d, o, camera=cam, layout=False)
    rgbs, sigmas = utils.shade_baked_points(mi, uv, comp, xyzs, index_tri, dirs)
    counts = np.bincount(index_ray.cpu().numpy(), minlength=w * h)
    s = dict(fr=fr, mi=mi, o=o, d=d, cam=cam, uv=uv, comp=comp, n_rays=w * h, k=k, bg=bg, rgbs=rgbs, sigmas=sigmas, ts=ts,
             index_ray=index_ray, counts=counts, sigma_host=sigmas.cpu().numpy())
    _cache[key] = s
    return s


def _reference(s, eps):
    """The existing shading, truncated by the numpy rule, composited by the existing ray-major compositor."""
    from quadraturefields_amd import utils
    kept = T.contributing_counts(s["sigma_host"], s["counts"], DELTA, T.stop_tau(eps))
    rgbs, sigmas, ts, index_ray = T.truncate(s["counts"], kept, s["rgbs"], s["sigmas"], s["ts"], s["index_ray"])
    rgb, alpha, _, depth, _ = utils.derive_properties(rgbs, sigmas, ts, DELTA, None, index_ray, bg_color=s["bg"],
                                                      N=s["n_rays"])
    return kept, rgb, alpha, depth


@pytest.mark.parametrize("cfg", CONFIGS, ids=_IDS)
def test_eps_zero_is_the_existing_route_bit_for_bit(device, cfg):
    from quadraturefields_amd import utils
    s = _scene(device, *cfg)
    fr, ri = s["fr"], s["mi"].rayintersector
    want = fr.render_baked(s["o"], s["d"], s["uv"], s["comp"], camera=s["cam"])
    got = fr.render_baked(s["o"], s["d"], s["uv"], s["comp"], camera=s["cam"], early_stop_eps=0.0)
    frame = ri.last_frame
    assert got[3] == want[3] == int(s["counts"].sum())
    for a, b in zip(got[:3], want[:3]):
        assert a.shape == b.shape and torch.equal(a, b)
    assert frame.shaded_count.dtype == torch.int32 and frame.shaded_count.shape == (s["n_rays"],)
    assert torch.equal(frame.shaded_count, frame.hit_count)
    assert frame.shaded_count.cpu().numpy().tolist() == s["counts"].tolist()
    # the packed output equals the three arrays
    _, xyz_c, dirs_c = ri.last_layout
    packed = utils.shade_composite_baked_frame(s["mi"], s["uv"], s["comp"], xyz_c, dirs_c, frame, DELTA, math.inf,
                                               bg_color=s["bg"], packed=True)
    assert packed[1] is None and packed[2] is None and torch.equal(packed[0], torch.cat(got[:3], dim=1))
    assert torch.equal(packed[3], frame.shaded_count)
    # ... and so does the frame without a host wait
    asy = fr.render_baked_async(s["o"], s["d"], s["uv"], s["comp"], s["cam"], early_stop_eps=0)
    for a, b in zip(asy[:3], want[:3]):
        assert torch.equal(a, b)
    assert torch.equal(asy[3].shaded_count, asy[3].hit_count)


@pytest.mark.parametrize("eps", [1e-2, 1e-3])
@pytest.mark.parametrize("cfg", CONFIGS, ids=_IDS)
def test_early_stop_equals_the_truncated_unfused_route(device, cfg, eps):
    """Counts and pixels exactly.  With K = 1 no frame can shade fewer samples than it has (a pixel's first sample always
    contributes: cum = 0), so there the strict inequality is the equality; for every K > 1 it is asserted strictly."""
    s = _scene(device, *cfg)
    fr, ri = s["fr"], s["mi"].rayintersector
    kept, rgb_w, alpha_w, depth_w = _reference(s, eps)
    rgb, alpha, depth, n = fr.render_baked(s["o"], s["d"], s["uv"], s["comp"], camera=s["cam"], early_stop_eps=eps)
    shaded = ri.last_frame.shaded_count.cpu().numpy()
    n_hit, n_early = int((s["counts"] > 0).sum()), int((kept < s["counts"]).sum())
    print(f"{cfg} eps {eps}: {int(shaded.sum())} of {n} samples shaded, reference {int(kept.sum())}; "
          f"{n_early} of {n_hit} hit rays stop early")
    assert n == int(s["counts"].sum())
    assert shaded.tolist() == kept.tolist()
    assert torch.equal(rgb, rgb_w) and torch.equal(alpha, alpha_w) and torch.equal(depth, depth_w)
    rgb_0 = fr.render_baked(s["o"], s["d"], s["uv"], s["comp"], camera=s["cam"])[0]
    assert float((rgb - rgb_0).abs().max()) <= 3 * eps
    if s["k"] > 1:
        assert int(shaded.sum()) < n
    else:
        assert int(shaded.sum()) == n
    if cfg == CONFIGS[0]:              # the named scene: neither never nor always (the oracle's own numbers, host test)
        assert 0.25 * n_hit <= n_early <= 0.75 * n_hit
    # without a host wait: the same frame
    asy = fr.render_baked_async(s["o"], s["d"], s["uv"], s["comp"], s["cam"], early_stop_eps=eps)
    assert torch.equal(asy[0], rgb) and torch.equal(asy[1], alpha) and torch.equal(asy[2], depth)
    assert asy[3].shaded_count.cpu().numpy().tolist() == kept.tolist()


def _plain_pass(ri):
    """Put the intersector's frame policy on the plain camera-coherent pass with the re-origin rule left to the tile pack
    (what ``fused_frame_ready`` asks for), whatever the frames before have moved it to."""
    ri._raster_backoff = 0
    ri._rule_upfront = 0


def _bound_call(ri, job, shading, stop_tau, shaded):
    from quadraturefields_amd import _C
    return _C.lib().qf_frame_render_baked(ri._handle, ctypes.byref(job), ctypes.byref(shading), stop_tau, _C.ptr(shaded),
                                          _C.stream())


@pytest.mark.parametrize("cfg", [CONFIGS[0], CONFIGS[1], CONFIGS[4], CONFIGS[10]], ids=[_IDS[0], _IDS[1], _IDS[4], _IDS[10]])
def test_one_bound_call_equals_the_separate_launches(device, cfg):
    from quadraturefields_amd import _C, utils
    s = _scene(device, *cfg)
    ri = s["mi"].rayintersector
    n = s["n_rays"]
    mode = utils._BG[s["bg"]]
    shading, keep = utils.baked_shading(s["mi"], s["uv"], s["comp"])
    for eps in (0.0, 1e-2):
        stop = float(T.stop_tau(eps))
        # the separately bound launches: sampling, then the kernel (both frames leave the re-origin rule to the tile pack:
        # the named scene has one hit that the rule drops, so a tile of it ends in a gap)
        _plain_pass(ri)
        frame = ri.sample_frame_device(s["o"], s["d"], s["k"], s["cam"], want_tri=True)
        _, xyz_c, dirs_c = ri.last_layout
        want = utils.shade_composite_baked_frame(s["mi"], s["uv"], s["comp"], xyz_c, dirs_c, frame, DELTA, stop,
                                                 bg_color=s["bg"])
        ri._settle_deferred_policy()
        _plain_pass(ri)
        assert ri.fused_frame_ready(s["cam"], s["k"]), (ri._raster_backoff, ri.raster_wide, ri._rule_upfront)
        job, frame2, token = ri.fused_frame_job(s["o"], s["d"], s["k"], s["cam"], want_tri=True)
        rgb, alpha, depth = (torch.full((n, c), -7.0, device=device) for c in (3, 1, 1))
        shaded = torch.full((n,), -7, dtype=torch.int32, device=device)
        job.out_rgb, job.out_alpha, job.out_depth = rgb.data_ptr(), alpha.data_ptr(), depth.data_ptr()
        job.delta_const, job.bg_mode = DELTA, mode
        _C.check(_bound_call(ri, job, shading, stop, shaded), "qf_frame_render_baked")
        ri.fused_frame_done(frame2, token)
        assert torch.equal(rgb, want[0]) and torch.equal(alpha, want[1]) and torch.equal(depth, want[2])
        assert torch.equal(shaded, want[3])
        assert torch.equal(frame2.hit_count, frame.hit_count) and torch.equal(frame2.tile_base, frame.tile_base)
        ri._settle_fused_policy(0)


def test_spoiled_job_is_refused_before_the_first_launch(device):
    """Field not NULL, tri_c NULL, stop_tau NaN (and negative), n_lobes out of range: refused with every output buffer,
    the tile bases and the pinned block untouched (the pattern of test_frame_job_is_validated)."""
    from quadraturefields_amd import _C, utils
    s = _scene(device, *CONFIGS[0])
    ri = s["mi"].rayintersector
    n = s["n_rays"]
    desc = _C.FieldDesc()

    def spoil_field(j, sh): j.field = ctypes.addressof(desc); return 1.0
    def spoil_tri(j, sh): j.tri_c = None; return 1.0
    def spoil_nan(j, sh): return math.nan
    def spoil_negative(j, sh): return -1.0
    def spoil_lobes_high(j, sh): sh.n_lobes = _C.QF_MAX_LOBES + 1; return 1.0
    def spoil_lobes_zero(j, sh): sh.n_lobes = 0; return 1.0
    def spoil_no_image(j, sh): j.out_rgb = None; return 1.0

    for spoil in (spoil_field, spoil_tri, spoil_nan, spoil_negative, spoil_lobes_high, spoil_lobes_zero, spoil_no_image):
        _plain_pass(ri)
        shading, keep = utils.baked_shading(s["mi"], s["uv"], s["comp"])
        job, frame, token = ri.fused_frame_job(s["o"], s["d"], s["k"], s["cam"], want_tri=True)
        rgb, alpha, depth = (torch.full((n, c), -7.0, device=device) for c in (3, 1, 1))
        shaded = torch.full((n,), -7, dtype=torch.int32, device=device)
        job.out_rgb, job.out_alpha, job.out_depth = rgb.data_ptr(), alpha.data_ptr(), depth.data_ptr()
        job.delta_const, job.bg_mode = DELTA, _C.BG_WHITE
        stop = spoil(job, shading)
        torch.cuda.synchronize()
        host = ri._frame_scratch(n)[2]
        host[:] = -5                                      # the pinned block: any launch of the frame would rewrite it
        frame.tile_base.fill_(-9)
        frame.hit_count.fill_(-9)
        with pytest.raises((ValueError, _C.QFError)):
            _C.check(_bound_call(ri, job, shading, stop, shaded), "qf_frame_render_baked")
        torch.cuda.synchronize()
        assert host.tolist() == [-5, -5, -5, -5], spoil.__name__
        assert bool((frame.tile_base == -9).all()) and bool((frame.hit_count == -9).all()), spoil.__name__
        assert bool((rgb == -7).all()) and bool((alpha == -7).all()) and bool((depth == -7).all()), spoil.__name__
        assert bool((shaded == -7).all()), spoil.__name__
    # the kernel's own entry point refuses a NaN / negative threshold as well
    frame = ri.sample_frame_device(s["o"], s["d"], s["k"], s["cam"], want_tri=True)
    _, xyz_c, dirs_c = ri.last_layout
    for bad in (math.nan, -1.0):
        with pytest.raises(ValueError):
            utils.shade_composite_baked_frame(s["mi"], s["uv"], s["comp"], xyz_c, dirs_c, frame, DELTA, bad)
    ri._settle_deferred_policy()


def test_invalid_early_stop_eps(device):
    s = _scene(device, *CONFIGS[0])
    fr = s["fr"]
    for bad in (-0.1, 1.0, math.nan, math.inf):
        with pytest.raises(ValueError):
            fr.render_baked(s["o"], s["d"], s["uv"], s["comp"], camera=s["cam"], early_stop_eps=bad)
        with pytest.raises(ValueError):
            fr.render_baked_async(s["o"], s["d"], s["uv"], s["comp"], s["cam"], early_stop_eps=bad)
    # the ray-major route shades every sample: the keyword is refused there, never ignored
    with pytest.raises(NotImplementedError):
        fr.render_baked(s["o"], s["d"], s["uv"], s["comp"], image_width=37, early_stop_eps=1e-3)
    with pytest.raises(NotImplementedError):
        fr.render_baked_async(s["o"], s["d"], s["uv"], s["comp"], None, early_stop_eps=1e-3)


@pytest.mark.parametrize("codec", ["sigmoid", "sigma"])
@pytest.mark.parametrize("eps", [1e-2, 1e-3])
def test_fully_opaque_alpha_plane_shades_one_sample_per_pixel(device, codec, eps):
    """All alpha codes 255.  The existing dequantiser (texture_utils.py:61-65: ``-log(clip(1 - a, 1e-6)) / 0.005``, the same
    under both colour codecs) gives code 255 the density 2763.1, not infinity: tau = -log(1e-6) = 13.8 per sample, above
    both thresholds (4.6, 6.9), so every hit pixel stops behind its first sample.  (An infinite density cannot reach the
    kernel through a texture set; the rule's behaviour there is pinned by the numpy rule's own test.)"""
    s = _scene(device, 37, 29, 25, 6, "white", codec, "opaque")
    ri = s["mi"].rayintersector
    assert float(s["sigmas"].min()) == float(s["sigmas"].max()) and 2763.0 < float(s["sigmas"].max()) < 2764.0
    kept, rgb_w, alpha_w, depth_w = _reference(s, eps)
    rgb, alpha, depth, n = s["fr"].render_baked(s["o"], s["d"], s["uv"], s["comp"], camera=s["cam"], early_stop_eps=eps)
    shaded = ri.last_frame.shaded_count.cpu().numpy()
    hit = s["counts"] > 0
    assert hit.any() and (s["counts"] > 1).any()
    assert (shaded[hit] == 1).all() and (shaded[~hit] == 0).all() and shaded.tolist() == kept.tolist()
    assert bool(torch.isfinite(rgb).all()) and bool(torch.isfinite(alpha).all()) and bool(torch.isfinite(depth).all())
    assert torch.equal(rgb, rgb_w) and torch.equal(alpha, alpha_w) and torch.equal(depth, depth_w)
