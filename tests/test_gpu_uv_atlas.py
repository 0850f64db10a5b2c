"""GPU: the per-triangle UV atlas (``uv_atlas.per_triangle_atlas`` / ``qf_uv_atlas_*``) against its numpy restatement
(tests/uv_atlas_reference.py), bit for bit; its composition with the texel-position map and the baked path's lookup on
the device; and the whole route mesh without UVs -> atlas -> map -> baked textures -> rendered frame."""
import functools

import numpy as np
import pytest
import torch

from quadraturefields_amd.mesh_io import TriMesh, load_mesh
from tests import uv_atlas_reference as ref

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _shell():
    from quadraturefields_amd import synthetic
    m = synthetic.shell_mesh(n_shells=2, subdivisions=3)                  # 2 560 faces
    return TriMesh(m.vertices, m.faces)


@functools.lru_cache(maxsize=None)
def _soup():
    """1 000 random triangles, edge lengths over 100x, 20 faces of zero area; the vertex array is shuffled."""
    rng = np.random.default_rng(17)
    n = 1000
    centre = rng.uniform(-1, 1, size=(n, 1, 3))
    size = np.exp(rng.uniform(np.log(0.01), np.log(1.0), size=(n, 1, 1)))
    tri = centre + size * rng.normal(size=(n, 3, 3))
    tri[:10, 2] = tri[:10, 1]                                               # two equal corners
    tri[10:20] = np.round(tri[10:20] * 64) / 64                            # dyadic, so that c = 2 b - a is exactly collinear
    tri[10:20, 2] = 2 * tri[10:20, 1] - tri[10:20, 0]
    order = rng.permutation(3 * n)                                          # vertices in another order than the faces use
    v = np.empty((3 * n, 3))
    v[order] = tri.reshape(-1, 3)
    return TriMesh(v, order.reshape(-1, 3))


@functools.lru_cache(maxsize=None)
def _mc_sphere():
    """Marching cubes of a 32^3 ball whose radius and centre are integers: grid points lie exactly on the level, their
    crossings merge into corner vertices and some faces repeat an index."""
    from quadraturefields_amd import mc_utils
    ax = torch.arange(32, device="cuda", dtype=torch.float32) - 16
    vol = 10.0 - torch.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2)
    verts, faces = mc_utils.marching_cubes(vol, 0.0)
    return TriMesh(mc_utils.normalise_vertices(verts, 32).cpu().numpy(), faces.cpu().numpy())


@functools.lru_cache(maxsize=None)
def _reference(name, S, max_leg, texels_per_unit=None):
    mesh = MESHES[name]()
    return ref.atlas(mesh.vertices, mesh.faces, S, texels_per_unit, max_leg)


MESHES = {"shell": _shell, "soup": _soup, "mc_sphere": _mc_sphere}


def _assert_exact(name, S, max_leg, texels_per_unit=None):
    from quadraturefields_amd import uv_atlas
    mesh = MESHES[name]()
    want = _reference(name, S, max_leg, texels_per_unit)
    mesh_uv, info = uv_atlas.per_triangle_atlas(mesh, S, texels_per_unit=texels_per_unit, max_leg=max_leg)
    F = len(mesh.faces)
    assert info.face_class.is_cuda and info.face_class.dtype == torch.int32 and info.face_class.shape == (F,)
    assert info.face_origin.is_cuda and info.face_origin.dtype == torch.int32 and info.face_origin.shape == (F, 2)
    assert info.face_half.is_cuda and info.face_half.dtype == torch.uint8 and info.face_half.shape == (F,)
    assert info.class_counts.dtype == np.int64 and info.class_counts.shape == (max_leg + 1,)
    assert info.rho == want["rho"], (info.rho, want["rho"])
    assert np.array_equal(info.class_counts, want["class_counts"])
    assert info.rows_used == want["rows_used"] and info.texels_used == want["texels_used"]
    assert np.array_equal(info.face_class.cpu().numpy(), want["face_class"])
    assert np.array_equal(info.face_half.cpu().numpy(), want["face_half"])
    assert np.array_equal(info.face_origin.cpu().numpy(), want["face_origin"])
    uv = mesh_uv.visual.uv
    assert uv.dtype == np.float64 and uv.shape == (3 * F, 2) and (uv >= 0).all() and (uv < 1).all()
    bad = np.nonzero((uv.view(np.uint64) != want["uv"].view(np.uint64)).any(axis=1))[0]
    assert bad.size == 0, (bad[:5], uv[bad[0]], want["uv"][bad[0]])
    assert np.array_equal(mesh_uv.faces, np.arange(3 * F).reshape(-1, 3))
    assert np.array_equal(mesh_uv.triangles.view(np.uint64), mesh.triangles.view(np.uint64))
    return want


@pytest.mark.parametrize("max_leg", [63, 3])
def test_shell_mesh_is_bit_exact(device, max_leg):
    want = _assert_exact("shell", 256, max_leg)
    assert want["rows_used"] <= 255
    _assert_exact("shell", 256, max_leg, texels_per_unit=0.75 * want["rho"])


def test_random_soup_is_bit_exact(device):
    mesh = _soup()
    t = mesh.triangles
    edges = np.linalg.norm(t - np.roll(t, 1, axis=1), axis=2)
    assert edges[20:].max() / edges[20:].min() > 100
    want = _assert_exact("soup", 128, 63)
    assert (want["face_class"][:20] == 0).all() and (ref.measure(mesh.vertices, mesh.faces)[0][:20] == 0).all()
    assert (want["class_counts"] % 2 == 1).sum() >= 2                       # half-full last blocks
    _assert_exact("soup", 128, 63, texels_per_unit=0.5 * want["rho"])


def test_marching_cubes_mesh_is_bit_exact(device):
    f = _mc_sphere().faces
    assert ((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).any()
    want = _assert_exact("mc_sphere", 512, 63)
    _assert_exact("mc_sphere", 512, 63, texels_per_unit=0.5 * want["rho"])


@pytest.mark.parametrize("name,S", [("soup", 128), ("mc_sphere", 512)])
def test_max_leg_zero_is_bit_exact(device, name, S):
    """N = 0 on meshes with zero-area faces: every face is class 0 = N, the search saturates at rho = 1."""
    mesh = MESHES[name]()
    assert (ref.measure(mesh.vertices, mesh.faces)[0] == 0).any()
    want = _assert_exact(name, S, 0)
    assert want["rho"] == 1.0 and want["class_counts"].tolist() == [len(mesh.faces)]
    _assert_exact(name, S, 0, texels_per_unit=0.5)


def test_runs_are_bit_identical(device):
    from quadraturefields_amd import uv_atlas
    mesh = _soup()
    a, ia = uv_atlas.per_triangle_atlas(mesh, 128)
    b, ib = uv_atlas.per_triangle_atlas(mesh, 128)
    assert ia.rho == ib.rho and np.array_equal(a.visual.uv.view(np.uint64), b.visual.uv.view(np.uint64))
    assert np.array_equal(a.vertices.view(np.uint64), b.vertices.view(np.uint64))
    assert torch.equal(ia.face_class, ib.face_class) and torch.equal(ia.face_origin, ib.face_origin)
    assert torch.equal(ia.face_half, ib.face_half) and np.array_equal(ia.class_counts, ib.class_counts)
    # the returned mesh's triangles are the input's, face by face
    assert np.array_equal(a.triangles.view(np.uint64), mesh.triangles.view(np.uint64))


def test_composition_with_the_texel_position_map_and_the_lookup(device):
    """Every face's cover in the device map is exactly its staircase, no texel has two owners, and the baked path's
    nearest-texel lookup of points all over face f lands inside face f's own staircase."""
    from quadraturefields_amd import baking, synthetic, utils, uv_atlas
    from quadraturefields_amd.mesh_utils import MeshIntersection
    S = 256
    mesh = _shell()
    mesh_uv, info = uv_atlas.per_triangle_atlas(mesh, S)
    k = info.face_class.to(torch.int64)
    V, tri_size = baking.texel_positions(mesh_uv, S, untouched="zero")
    assert torch.equal(tri_size, (k + 1) * (k + 2) // 2)
    assert int(tri_size.sum()) == info.texels_used == int((V != 0).any(-1).sum())
    assert not bool((V[-1] != 0).any()) and not bool((V[:, -1] != 0).any())

    F = len(mesh.faces)
    w = ref.lookup_points(F)                                                   # [F, 206, 3]
    pts = np.einsum("fnk,fkd->fnd", w, mesh_uv.triangles).reshape(-1, 3)
    tri = np.repeat(np.arange(F), w.shape[1])
    mi = MeshIntersection(mesh_uv, simplify_mesh=False, scale=1.0, num_intersections=8)
    uv = torch.from_numpy(synthetic.scaled_uv(mesh_uv, S)).to(device)
    texel = utils.texel_indices(mi, uv, torch.from_numpy(pts.astype(np.float32)).to(device),
                                torch.from_numpy(tri).to(device), S).cpu().numpy()
    kk, origin, half = k.cpu().numpy()[tri], info.face_origin.cpu().numpy().astype(np.int64)[tri], info.face_half.cpu().numpy()[tri]
    ok = ref.in_staircase(texel, kk, origin, half)
    assert ok.all(), (np.nonzero(~ok)[0][:5], texel[~ok][:5])


class _CountingLib:
    """Stands in for the loaded library: passes calls through and records their names."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        self.calls.append(name)
        return getattr(self._real, name)


def test_refusals(device, monkeypatch):
    """Each refusal raises ValueError; what the host can see is refused before the library is touched, what only the
    device can see (non-finite vertices, face indices) right after the measure call, with nothing launched after it."""
    from quadraturefields_amd import _C, uv_atlas
    counting = _CountingLib(_C.lib())
    monkeypatch.setattr(uv_atlas._C, "lib", lambda: counting)
    v = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    f = np.array([[0, 1, 2], [1, 2, 3]])
    good = TriMesh(v, f)
    host_side = [
        (TriMesh(v, np.zeros((0, 3), np.int64)), dict(texture_size=128)),                # F = 0
        (good, dict(texture_size=65)),                                                    # S < max_leg + 3
        (good, dict(texture_size=16385, max_leg=3)),
        (good, dict(texture_size=64, max_leg=-1)),
        (good, dict(texture_size=128, max_leg=64)),
        (good, dict(texture_size=64.0, max_leg=3)),
        (good, dict(texture_size=128, texels_per_unit=0.0)),
        (good, dict(texture_size=128, texels_per_unit=-1.0)),
        (good, dict(texture_size=128, texels_per_unit=float("inf"))),
        (good, dict(texture_size=128, texels_per_unit=float("nan"))),
    ]
    from tests.test_uv_atlas_host import _Shape                             # shapes of meshes too large to build
    host_side += [(_Shape(4, -(-2 ** 31 // 3)), dict(texture_size=128)), (_Shape(2 ** 31, 2), dict(texture_size=128))]
    for mesh, kw in host_side:
        with pytest.raises(ValueError):
            uv_atlas.per_triangle_atlas(mesh, **kw)
        assert counting.calls == [], (kw, counting.calls)
    bad_vertex = v.copy()
    bad_vertex[3, 1] = np.nan
    device_side = [(TriMesh(bad_vertex, f), "1 vertices"), (TriMesh(np.where(np.isnan(bad_vertex), np.inf, bad_vertex), f), "1 vertices"),
                   (TriMesh(v, np.array([[0, 1, 2], [1, 2, 4]])), "1 faces"), (TriMesh(v, np.array([[0, -1, 2], [1, 2, 3]])), "1 faces")]
    for mesh, what in device_side:
        counting.calls.clear()
        with pytest.raises(ValueError, match=what):
            uv_atlas.per_triangle_atlas(mesh, 128)
        assert counting.calls == ["qf_uv_atlas_workspace_bytes", "qf_uv_atlas_measure"], counting.calls
    # the C entries after a refused measure: zeros and fits = 0, no mesh
    lib = counting._real
    vd, fd = torch.from_numpy(bad_vertex).to(device), torch.from_numpy(f).to(device)
    ws_bytes = int(lib.qf_uv_atlas_workspace_bytes(2))
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=device)
    counts = torch.zeros(3, dtype=torch.int64, device=device)
    _C.check(lib.qf_uv_atlas_measure(_C.ptr(vd), 4, _C.ptr(fd), 2, _C.ptr(ws), ws_bytes, _C.ptr(counts), _C.stream()), "measure")
    result = torch.full((4,), -1, dtype=torch.int64, device=device)
    _C.check(lib.qf_uv_atlas_probe(2, 1.0, 3, 128, _C.ptr(ws), ws_bytes, _C.ptr(result), _C.stream()), "probe")
    assert counts.tolist() == [1, 0, 0] and result.tolist() == [0, 0, 0, 0]
    out_v, out_uv = torch.full((18,), -1.0, dtype=torch.float64, device=device), torch.full((12,), -1.0, dtype=torch.float64, device=device)
    fc, fo = torch.full((2,), -1, dtype=torch.int32, device=device), torch.full((2, 2), -1, dtype=torch.int32, device=device)
    fh, cc = torch.full((2,), 9, dtype=torch.uint8, device=device), torch.full((4,), -1, dtype=torch.int64, device=device)
    result.fill_(-1)
    _C.check(lib.qf_uv_atlas_emit(_C.ptr(vd), 4, _C.ptr(fd), 2, 1.0, 3, 128, _C.ptr(ws), ws_bytes, _C.ptr(out_v), _C.ptr(out_uv),
                                  _C.ptr(fc), _C.ptr(fo), _C.ptr(fh), _C.ptr(cc), _C.ptr(result), _C.stream()), "emit")
    assert result.tolist() == [0, 0, 0, 0] and cc.tolist() == [0, 0, 0, 0]
    assert bool((out_v == -1).all()) and bool((out_uv == -1).all()) and bool((fc == -1).all()) and bool((fo == -1).all())
    assert bool((fh == 9).all())
    # a density that does not fit names rows_used; too many faces name the capacity (S = 8: 42 faces)
    counting.calls.clear()
    with pytest.raises(ValueError, match="rows_used = 126"):                 # three class-62 faces: two blocks, one per shelf
        uv_atlas.per_triangle_atlas(TriMesh(np.tile(v[:3], (3, 1)), np.arange(9).reshape(-1, 3)), 66, texels_per_unit=1e3,
                                    max_leg=62)
    assert "qf_uv_atlas_emit" not in counting.calls
    many = TriMesh(np.tile(v[:3], (43, 1)), np.arange(129).reshape(-1, 3))
    with pytest.raises(ValueError, match="at most 42 faces"):
        uv_atlas.per_triangle_atlas(many, 8, max_leg=2)
    torch.cuda.synchronize()


def test_obj_round_trip(device, tmp_path):
    from quadraturefields_amd import uv_atlas
    mesh_uv, _ = uv_atlas.per_triangle_atlas(_soup(), 128)
    path = str(tmp_path / "atlas.obj")
    mesh_uv.export_obj(path)
    back = load_mesh(path)
    assert np.array_equal(back.vertices.view(np.uint64), mesh_uv.vertices.view(np.uint64))
    assert np.array_equal(back.faces, mesh_uv.faces)
    assert np.array_equal(back.visual.uv.view(np.uint64), mesh_uv.visual.uv.view(np.uint64))
    plain = TriMesh(_soup().vertices, _soup().faces)
    plain.export_obj(path)
    back = load_mesh(path)
    assert np.array_equal(back.vertices, plain.vertices) and np.array_equal(back.faces, plain.faces) and back.visual.uv is None


def _e2e_scene(device):
    """The scene of test_gpu_texel_fill's end-to-end test: three nested shells and a seeded SG field."""
    from quadraturefields_amd import synthetic
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceFieldSGNew
    lobes = 3
    mesh = synthetic.shell_mesh(n_shells=3, subdivisions=4)
    sg = NGPRadianceFieldSGNew(aabb=[-1.5] * 3 + [1.5] * 3, use_viewdirs=False, num_g_lobes=lobes, log2_hashmap_size=12)
    sg.load_state_dict(synthetic.seeded_ngp_state(12, sg.mlp_base.grid.n_rows, sg_lobes=lobes), strict=False)
    return mesh, sg.to(device), lobes


E2E_PSNR_BAR = 33.75


def e2e_psnrs(device, with_analytic=False):
    """(atlas route, control, analytic-chart route or None) in dB, against the SG field's own frame; also info."""
    from quadraturefields_amd import baking, synthetic, utils, uv_atlas
    from quadraturefields_amd.datasets.utils import Rays
    from quadraturefields_amd.mesh_utils import MeshIntersection
    from quadraturefields_amd.render import psnr
    from quadraturefields_amd.texture_utils import FeatureCompression
    charted, sg, lobes = _e2e_scene(device)
    size = 1024
    w = h = 100
    c2w = synthetic.orbit_cameras(1, seed=3)[0]
    o, d = synthetic.camera_rays(c2w, synthetic.lego_focal(800) * w / 800.0, w, h)
    rays = Rays(origins=o.reshape(h, w, 3), viewdirs=d.reshape(h, w, 3))

    def frames(mesh, V_maps):
        mi = MeshIntersection(mesh, simplify_mesh=False, scale=1.0, num_intersections=25)     # rebuilt per mesh
        uv = torch.from_numpy(synthetic.scaled_uv(mesh, size)).to(device)
        data = mi.sampling_raytrace_device(d, o)
        direct = utils.render_image_finetune_with_occgrid(sg, None, None, rays, data, render_step_size=5e-3,
                                                          mesh_intersect=mi, scaling=0)[0]
        out = []
        for V_map in V_maps:
            comp = FeatureCompression(lobes, initialize=True, texture_size=size, compression_type="sigmoid", lambda_thres=7.5)
            baking.bake_texture_images(sg, sg, V_map, comp, batch_size=1 << 18)
            baked = utils.render_image_bake_texture_images_with_occgrid(sg, rays, data, uv=uv, render_step_size=5e-3,
                                                                        mesh_intersect=mi, compressor=comp)[0]
            out.append(psnr(baked, direct))
        return out

    mesh_uv, info = uv_atlas.per_triangle_atlas(TriMesh(charted.vertices, charted.faces), size)
    V, _ = baking.texel_positions(mesh_uv, size)
    good, control = frames(mesh_uv, [V, torch.roll(V, 16, dims=0)])
    analytic = frames(charted, [baking.texel_positions(charted, size)[0]])[0] if with_analytic else None
    return good, control, analytic, info


def test_mesh_without_uvs_to_baked_frame_end_to_end(device):
    """per_triangle_atlas -> texel_positions -> bake_texture_images -> render_image_bake_texture_images_with_occgrid on
    the mesh of test_gpu_texel_fill's end-to-end test with its UVs stripped, against the same scene rendered from the SG
    field itself; the intersector is rebuilt on the unshared mesh.  The control is the same bake from V rolled by 16
    rows; the bar sits half-way between the two, as in that test.
    Measured on MI355X: 34.90 dB (rho = 179.45, 995 270 of 1024^2 texels used); the control 32.61 dB; the bar, 33.75 dB,
    sits half-way.  Every step is deterministic, so the values repeat run to run.  For context only, and not asserted: the
    analytic (azimuth, elevation) charts of that test give 33.53 dB in the same run (``e2e_psnrs(with_analytic=True)``) --
    they spend the atlas unevenly, the per-triangle atlas spends 95 % of it in proportion to area."""
    good, control, _, info = e2e_psnrs(device)
    print(f"per-triangle atlas (rho = {info.rho:.4f}, {info.texels_used} texels): {good:.2f} dB, V rolled by 16 rows: "
          f"{control:.2f} dB")
    assert good >= E2E_PSNR_BAR, good
    assert control < E2E_PSNR_BAR, control
