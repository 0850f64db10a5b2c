"""GPU: the texel-position map (``baking.texel_positions`` / ``qf_texel_positions``) against its numpy restatement
(tests/texel_fill_reference.py), bit for bit, and the whole route mesh -> map -> baked textures -> rendered frame."""
import numpy as np
import pytest
import torch

from quadraturefields_amd.mesh_io import TriMesh
from tests import texel_fill_reference as ref

pytestmark = pytest.mark.gpu


def _device_map(mesh, H, W, untouched="last_face"):
    from quadraturefields_amd import baking
    V, tri_size = baking.texel_positions(mesh, H, W, untouched=untouched)
    torch.cuda.synchronize()
    assert V.is_cuda and V.dtype == torch.float32 and V.shape == (H, W, 3)
    assert tri_size.is_cuda and tri_size.dtype == torch.int64 and tri_size.shape == (len(mesh.faces),)
    return V.cpu().numpy(), tri_size.cpu().numpy()


def _assert_exact(mesh, H, W, untouched="last_face"):
    V, ts = _device_map(mesh, H, W, untouched)
    V_ref, ts_ref = ref.texel_positions(mesh.vertices, mesh.faces, mesh.visual.uv, H, W, untouched)
    assert np.array_equal(ts, ts_ref)
    bad = np.argwhere(V.view(np.uint32) != V_ref.view(np.uint32))
    assert bad.size == 0, (bad[:5], V[tuple(bad[0][:2])], V_ref[tuple(bad[0][:2])])
    return V, ts


def _random_triangles(H, W, n=400, n_large=6, seed=5):
    """Overlapping random triangles, ``n_large`` of them spanning more than 10^4 texels, in random index order."""
    rng = np.random.default_rng(seed)
    small = rng.uniform(0, 1, size=(n, 1, 2)) + rng.normal(scale=12.0 / H, size=(n, 3, 2))
    big = np.array([[0.1, 0.1], [0.1, 0.9], [0.8, 0.2]]) + rng.normal(scale=0.02, size=(n_large, 3, 2))
    uv = np.concatenate([small, big])[rng.permutation(n + n_large)].reshape(-1, 2)
    verts = rng.normal(size=(uv.shape[0], 3))
    return TriMesh(verts, np.arange(uv.shape[0]).reshape(-1, 3), uv)


@pytest.mark.parametrize("H,W", [(256, 256), (512, 384)])
def test_shell_mesh_is_bit_exact(device, H, W):
    from quadraturefields_amd import synthetic
    _assert_exact(synthetic.shell_mesh(n_shells=2, subdivisions=3), H, W)


@pytest.mark.parametrize("untouched", ["last_face", "zero"])
def test_per_triangle_charts_are_bit_exact(device, untouched):
    """Random 4-texel charts leave most of the atlas untouched: both fill modes."""
    from quadraturefields_amd import synthetic
    mesh, _ = synthetic.per_triangle_charts(synthetic.shell_mesh(n_shells=2, subdivisions=3), 256)
    V, _ = _assert_exact(mesh, 256, 256, untouched)
    empty = (V == 0).all(-1).mean()
    assert (empty > 0.5) if untouched == "zero" else (empty == 0)


def test_random_overlapping_and_large_faces_are_bit_exact(device):
    """Overlaps (the largest face index wins) and faces of more than 10^4 texels next to faces of a few (the cover
    pass balances candidate texels, not faces)."""
    mesh = _random_triangles(512, 512)
    _, ts = _assert_exact(mesh, 512, 512)
    assert ts.max() > 10_000 and np.median(ts) < 200


def test_degenerate_faces_are_bit_exact(device):
    """Collinear and coincident integer corners: the whole face gets its centroid."""
    rng = np.random.default_rng(9)
    H = W = 128
    rc = np.array([[[10, 10], [10, 40], [10, 70]], [[20, 5], [50, 5], [35, 5]], [[60, 60], [60, 60], [60, 60]],
                   [[70, 70], [80, 80], [90, 90]], [[5, 5], [5, 100], [100, 5]]], dtype=np.float64)
    uv = (rc + rng.uniform(0, 0.9, size=rc.shape)) / np.array([H, W])       # same integer corners, fractional parts
    mesh = TriMesh(rng.normal(size=(15, 3)), np.arange(15).reshape(-1, 3), uv.reshape(-1, 2))
    _assert_exact(mesh, H, W)
    _assert_exact(TriMesh(mesh.vertices, mesh.faces[:4], mesh.visual.uv), H, W, "zero")


def test_runs_are_bit_identical_and_the_wrapper_matches(device):
    from quadraturefields_amd import baking, synthetic
    from quadraturefields_amd.parameterization_utils import fill_triangles_fill_boundary
    mesh = _random_triangles(384, 320, seed=11)
    a, ta = baking.texel_positions(mesh, 384, 320)
    b, tb = baking.texel_positions(mesh, 384, 320)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(ta, tb)
    mesh = synthetic.shell_mesh(n_shells=2, subdivisions=3)
    V, ts = fill_triangles_fill_boundary(mesh, 256, 192)
    Vt, tst = baking.texel_positions(mesh, 256, 192)
    assert isinstance(V, np.ndarray) and V.dtype == np.float32 and isinstance(ts, list)
    assert np.array_equal(V.view(np.uint32), Vt.cpu().numpy().view(np.uint32)) and ts == tst.cpu().tolist()


def test_bench_mesh_at_4096(device):
    """The bench mesh (983 040 faces) at 4096^2: finite everywhere; a 256^2 window equals the restatement run on only
    the faces that reach it (the rules are local); tri_size's total equals the restatement's."""
    from quadraturefields_amd import baking, synthetic
    mesh = synthetic.shell_mesh()
    H = W = 4096
    V, ts = baking.texel_positions(mesh, H, W)
    assert bool(torch.isfinite(V).all())
    for window in [(1200, 1700, 256, 256), (0, 3840, 256, 256)]:
        ids = ref.faces_reaching(mesh.visual.uv, mesh.faces, H, W, window)
        V_ref, _ = ref.texel_positions(mesh.vertices, mesh.faces, mesh.visual.uv, H, W, window=window, face_ids=ids)
        r0, c0, h, w = window
        got = V[r0:r0 + h, c0:c0 + w].cpu().numpy()
        assert np.array_equal(got.view(np.uint32), V_ref.view(np.uint32))
    assert int(ts.sum()) == int(ref.cover_counts(mesh.faces, mesh.visual.uv, H, W).sum())


def _e2e_scene(device):
    from quadraturefields_amd import synthetic
    from quadraturefields_amd.mesh_utils import MeshIntersection
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceFieldSGNew
    lobes = 3
    mesh = synthetic.shell_mesh(n_shells=3, subdivisions=4)
    mi = MeshIntersection(mesh, simplify_mesh=False, scale=1.0, num_intersections=25)
    sg = NGPRadianceFieldSGNew(aabb=[-1.5] * 3 + [1.5] * 3, use_viewdirs=False, num_g_lobes=lobes, log2_hashmap_size=12)
    sg.load_state_dict(synthetic.seeded_ngp_state(12, sg.mlp_base.grid.n_rows, sg_lobes=lobes), strict=False)
    return mesh, mi, sg.to(device), lobes


def test_mesh_to_baked_frame_end_to_end(device):
    """texel_positions -> bake_texture_images -> render_image_bake_texture_images_with_occgrid, against the same scene
    rendered from the SG field itself (render_image_finetune_with_occgrid, no deformation: train_finetune.py's route
    with num_lobes > 0).  The SG field is also the density field of the bake, as after the reference's SG fit.
    Measured on MI355X: 33.53 dB; the control -- the same bake from V rolled by 16 rows (about 23 degrees of azimuth
    on a shell) -- 32.50 dB.  The bar, 33.0 dB, sits half-way; every step is deterministic, so both values repeat run to
    run.  The gap is small because the seeded field varies slowly and the uint8 codecs set a floor near 33.5 dB."""
    from quadraturefields_amd import baking, synthetic, utils
    from quadraturefields_amd.datasets.utils import Rays
    from quadraturefields_amd.render import psnr
    from quadraturefields_amd.texture_utils import FeatureCompression
    mesh, mi, sg, lobes = _e2e_scene(device)
    size = 1024
    V, _ = baking.texel_positions(mesh, size)
    uv = torch.from_numpy(synthetic.scaled_uv(mesh, size)).to(device)
    w = h = 100
    c2w = synthetic.orbit_cameras(1, seed=3)[0]
    o, d = synthetic.camera_rays(c2w, synthetic.lego_focal(800) * w / 800.0, w, h)
    rays = Rays(origins=o.reshape(h, w, 3), viewdirs=d.reshape(h, w, 3))
    data = mi.sampling_raytrace_device(d, o)
    direct = utils.render_image_finetune_with_occgrid(sg, None, None, rays, data, render_step_size=5e-3,
                                                      mesh_intersect=mi, scaling=0)[0]

    def baked(V_map):
        comp = FeatureCompression(lobes, initialize=True, texture_size=size, compression_type="sigmoid", lambda_thres=7.5)
        mask = baking.bake_texture_images(sg, sg, V_map, comp, batch_size=1 << 18)
        # untouched="last_face" fills every texel; only a point whose fp32 coordinates sum to 0 is skipped
        assert mask.is_cuda and float(mask.float().mean()) > 0.999
        return utils.render_image_bake_texture_images_with_occgrid(sg, rays, data, uv=uv, render_step_size=5e-3,
                                                                   mesh_intersect=mi, compressor=comp)[0]

    good = psnr(baked(V), direct)
    control = psnr(baked(torch.roll(V, 16, dims=0)), direct)
    print(f"baked frame vs SG field frame: {good:.2f} dB, V rolled by 16 rows: {control:.2f} dB")
    assert good >= E2E_PSNR_BAR, good
    assert control < E2E_PSNR_BAR, control


E2E_PSNR_BAR = 33.0
