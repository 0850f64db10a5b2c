"""GPU: stage 6c as a fixed launch sequence -- ``qf_bake_compact_texels``, ``qf_bake_encode_texels``,
``baking.bake_texture_set`` -- and the command lines of stages 5, 6c and 6d (``examples/fit_sg_synthetic.py``,
``bake_texture_images.py``, ``evaluate_baked_textures.py``).

Measured on an MI355X (shares of texels whose code differs by one step; nothing differs by more; every test prints
its figures before it asserts, DESIGN.md section 3.17 records them):

* codec alone against ``oracle.quantize.compress_features`` (fp32, CPU): 2.1e-4 of ``lambda_axis_1`` at 3 lobes (one
  texel), every other plane of the 16 cases equal;
* ``bake_texture_set`` against the oracle's features + quantisers: 3.4e-4 of one elevation channel, everything else equal;
* ``bake_texture_set`` against ``bake_texture_images`` on the same device ``V``: no byte differs at 64 x 64 (at 4096 x 4096
  and 8192 x 8192 about one texel in 10^5 per plane, ``profiles/bake/bake_bench.json``).
"""
import ctypes
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from oracle import fields as ofields
from oracle import quantize as oq
from tests import helpers

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _example(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------------ compaction
def _compaction_map():
    t = 70
    rng = np.random.default_rng(3)
    v = rng.uniform(-1.2, 1.2, size=(t, t, 3)).astype(np.float32)
    v[rng.random((t, t)) < 0.3] = 0.0
    v[32:48] = 0.0                                        # the band [32, 48) of the 16-row split is entirely empty
    v[5, 7] = (1.0, 1e8, -1e8)                            # (1 + 1e8) + -1e8 == 0 in fp32: empty, as numpy's sum says
    v[5, 8] = (1.0, -1.0, 0.0)                            # empty
    v[5, 9] = (-0.0, 0.0, 0.0)                            # empty
    v[5, 10] = (1e8, -1e8, 1.0)                           # (1e8 - 1e8) + 1 == 1: valid -- the order matters
    v[69, 69] = (0.25, 0.5, 0.125)                        # the last texel of the map
    v[0, 0] = (0.5, 0.25, 0.125)
    return v


def _compact(v_d, row, rows, mask=None):
    from quadraturefields_amd import _C
    t = v_d.shape[0]
    dev = v_d.device
    cap = rows * t
    ws_bytes = int(_C.lib().qf_bake_compact_workspace_bytes(cap))
    assert ws_bytes > 0
    texel = torch.full((cap + 8,), -7, dtype=torch.int32, device=dev)
    pos = torch.full((cap + 8, 3), -7.0, dtype=torch.float32, device=dev)
    count = torch.full((1,), -7, dtype=torch.int64, device=dev)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    _C.check(_C.lib().qf_bake_compact_texels(_C.ptr(v_d), t, row, rows, _C.ptr(texel), _C.ptr(pos), _C.ptr(count),
                                             _C.ptr(mask) if mask is not None else None, _C.ptr(ws), ws_bytes, _C.stream()),
             "qf_bake_compact_texels")
    return texel, pos, count


@pytest.mark.parametrize("band_rows", [70, 16, 1])
def test_compact_texels(device, band_rows):
    v = _compaction_map()
    t = v.shape[0]
    v_d = torch.from_numpy(v).to(device)
    want_mask = torch.from_numpy(v.sum(-1) != 0)          # numpy's fp32 sum over the last axis: (x + y) + z
    assert not want_mask[5, 7] and not want_mask[5, 8] and not want_mask[5, 9] and want_mask[5, 10]
    mask = torch.full((t, t), 1, dtype=torch.uint8, device=device).view(torch.bool)
    total = 0
    for row in range(0, t, band_rows):
        rows = min(band_rows, t - row)
        texel, pos, count = _compact(v_d, row, rows, mask)
        band = want_mask[row:row + rows]
        want = torch.nonzero(band.reshape(-1)).reshape(-1) + row * t        # flat r * T + c, ascending
        n = int(count.item())
        assert n == int(band.sum()) == want.shape[0]
        assert torch.equal(texel[:n].cpu().long(), want)
        got_pos = pos[:n].cpu()
        want_pos = torch.from_numpy(v[row:row + rows][band.numpy()])
        assert torch.equal(got_pos.view(torch.int32), want_pos.view(torch.int32))      # bitwise
        # nothing past the count is written (an empty band writes nothing at all)
        assert bool((texel[n:] == -7).all()) and bool((pos[n:] == -7.0).all())
        total += n
    assert total == int(want_mask.sum())
    assert torch.equal(mask.cpu(), want_mask)
    # the 16-row split has an entirely empty band
    if band_rows == 16:
        assert int(want_mask[32:48].sum()) == 0
    # the same band twice gives the same list (no atomics decide the order)
    a = _compact(v_d, 0, min(band_rows, t))
    b = _compact(v_d, 0, min(band_rows, t))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_compact_texels_mask_is_optional_and_arguments_are_checked(device):
    from quadraturefields_amd import _C
    v_d = torch.from_numpy(_compaction_map()).to(device)
    texel, pos, count = _compact(v_d, 3, 5, None)
    assert int(count.item()) == int((v_d[3:8].cpu().numpy().sum(-1) != 0).sum())
    lib = _C.lib()
    p = _C.ptr
    ws = torch.empty((64,), dtype=torch.uint8, device=device)
    for t, row, rows in ((70, 0, 0), (70, 66, 5), (70, -1, 2), (0, 0, 1), (16385, 0, 1)):
        assert lib.qf_bake_compact_texels(p(v_d), t, row, rows, p(texel), p(pos), p(count), None, p(ws), 64, _C.stream()) == -1
    assert lib.qf_bake_compact_texels(p(v_d), 70, 0, 70, p(texel), p(pos), p(count), None, p(ws), 4, _C.stream()) == -1
    assert lib.qf_bake_compact_texels(None, 70, 0, 70, p(texel), p(pos), p(count), None, p(ws), 64, _C.stream()) == -1
    assert lib.qf_bake_compact_workspace_bytes(0) == -1 and lib.qf_bake_compact_workspace_bytes(4900) == 12


# ------------------------------------------------------------------------------------------------ codec alone
def _codec_inputs(lobes, seed):
    """4900 feature rows N(0, 3^2) with densities U(0, 400) and the edge rows of the issue."""
    n = 4900
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(n, 3 + 7 * lobes + 1, generator=g) * 3.0
    sigma = torch.rand(n, generator=g) * 400.0
    feats[0, 3:6] = 0.0                                   # zero axis of lobe 0: azimuth 128, elevation 128
    feats[1, 3 + 3] = 0.0                                 # lambda = 0 of lobe 0: code 0
    feats[2, :3] = 50.0                                   # colours beyond the clip
    feats[2, 3 + 4:3 + 7] = -50.0
    feats[3, :3] = -50.0
    feats[3, 3 + 4:3 + 7] = 50.0
    sigma[4] = 0.0
    sigma[5] = 1e9
    feats[:, -1] = 123456.0                               # the last column is ignored: sigma comes separately
    return feats, sigma


def _planes(t, lobes, fill, device):
    from quadraturefields_amd.texture_utils import FeatureCompression
    z = lambda *s: np.full(s, fill, dtype=np.uint8)
    return lambda ctype, thres: FeatureCompression.from_arrays(
        z(t, t), z(t, t, 3), [z(t, t, 3) for _ in range(lobes)], [z(t, t, 3) for _ in range(lobes)],
        compression_type=ctype, lambda_thres=thres, device=device)


def _step_stats(got, want, wrap=False):
    """(largest difference in code steps, share of entries that differ) of two uint8 tensors."""
    d = (got.to(torch.int16) - want.to(torch.int16)).abs()
    if wrap:
        d = torch.minimum(d % 256, 256 - d % 256)
    return int(d.max()), float((d > 0).float().mean())


@pytest.mark.parametrize("lambda_thres", [7.5, 5.0])
@pytest.mark.parametrize("ctype", ["sigmoid", "sigma"])
@pytest.mark.parametrize("lobes", [1, 3, 6, 8])
def test_encode_texels_against_the_oracle(device, lobes, ctype, lambda_thres):
    from quadraturefields_amd import _C
    t, n, short = 70, 4900, 37
    feats, sigma = _codec_inputs(lobes, seed=11 + lobes)
    perm = torch.randperm(t * t, generator=torch.Generator().manual_seed(5))[:n].to(torch.int32)     # every texel once
    comp = _planes(t, lobes, 0xAB, device)(ctype, lambda_thres)
    n_dev = torch.tensor([n - short], dtype=torch.int64, device=device)
    tex = comp.texture_set()
    feats_d, sigma_d, perm_d = feats.to(device), sigma.to(device), perm.to(device)
    _C.check(_C.lib().qf_bake_encode_texels(ctypes.byref(tex), _C.ptr(feats_d), feats.shape[1], _C.ptr(sigma_d),
                                            _C.ptr(perm_d), n, _C.ptr(n_dev), _C.stream()), "qf_bake_encode_texels")
    full = feats.clone()
    full[:, -1] = sigma
    want = oq.compress_features(full, lobes, ctype, lambda_thres)
    done, rest = perm[:n - short].long(), perm[n - short:].long()
    flat = lambda p, c=3: p.cpu().reshape(t * t, c) if c > 1 else p.cpu().reshape(t * t)
    planes = [("alpha", flat(comp.alpha, 1)[:, None], want["alpha"][:, None]), ("diffuse", flat(comp.diffuse), want["diffuse"])]
    for i in range(lobes):
        planes += [(f"color_{i}", flat(comp.sg_colors[i]), want["colors"][i]),
                   (f"lambda_axis_{i}", flat(comp.lambdas[i]), want["lambdas"][i])]
    worst = 0.0
    for name, got, ref in planes:
        # rows past *n_device (and, with n == T*T, there is no other texel) keep the fill byte
        assert bool((got[rest] == 0xAB).all()), name
        d = (got[done].to(torch.int16) - ref[:n - short].to(torch.int16)).abs()
        if name.startswith("lambda_axis"):                # channel 1 is the azimuth: codes 0 and 255 are neighbours
            d[:, 1] = torch.minimum(d[:, 1] % 256, 256 - d[:, 1] % 256)
        steps, texel_share = int(d.max()), float((d.amax(dim=-1) > 0).float().mean())
        print(f"encode L={lobes} {ctype} thres={lambda_thres} {name}: max step {steps}, texels differing {texel_share:.5f}")
        if ctype != "sigma" and (name == "diffuse" or name.startswith("color_")):
            assert steps == 0, name                       # the clip branch is arithmetic only: equal everywhere
        else:
            assert steps <= 1 and texel_share < 0.002, (name, steps, texel_share)
        worst = max(worst, texel_share)
    print(f"encode L={lobes} {ctype} thres={lambda_thres}: worst plane {worst:.5f}")
    # the edge rows
    lam0 = flat(comp.lambdas[0])
    assert lam0[perm[0].item()].tolist()[1:] == [128, 128]                               # zero axis
    assert lam0[perm[1].item()].tolist()[0] == 0                                         # lambda = 0
    assert flat(comp.alpha, 1)[perm[4].item()].item() == 0 and flat(comp.alpha, 1)[perm[5].item()].item() == 255
    if ctype != "sigma":
        assert flat(comp.diffuse)[perm[2].item()].tolist() == [255] * 3 and flat(comp.diffuse)[perm[3].item()].tolist() == [0] * 3
        assert flat(comp.sg_colors[0])[perm[2].item()].tolist() == [0] * 3


def test_encode_texels_touches_only_the_listed_texels(device):
    """A sparse list: every byte of every plane outside the listed texels keeps its fill; an index outside the set is
    skipped; a count above the capacity is clamped; arguments are checked before the launch."""
    from quadraturefields_amd import _C
    t, lobes, n = 70, 3, 500
    feats, sigma = _codec_inputs(lobes, seed=2)
    feats, sigma = feats[:n].contiguous(), sigma[:n].contiguous()
    perm = torch.randperm(t * t, generator=torch.Generator().manual_seed(9))[:n].to(torch.int32)
    perm[17], perm[18] = -1, t * t                                                       # not texels of this set
    comp = _planes(t, lobes, 0xAB, device)("sigmoid", 7.5)
    tex = comp.texture_set()
    n_dev = torch.tensor([10 ** 12], dtype=torch.int64, device=device)
    feats_d, sigma_d, perm_d = feats.to(device), sigma.to(device), perm.to(device)
    args = (_C.ptr(feats_d), feats.shape[1], _C.ptr(sigma_d), _C.ptr(perm_d), n, _C.ptr(n_dev))
    _C.check(_C.lib().qf_bake_encode_texels(ctypes.byref(tex), *args, _C.stream()), "qf_bake_encode_texels")
    listed = torch.zeros(t * t, dtype=torch.bool)
    keep = torch.ones(n, dtype=torch.bool)
    keep[17] = keep[18] = False
    listed[perm[keep].long()] = True
    full = feats.clone()
    full[:, -1] = sigma
    want = oq.compress_features(full, lobes, "sigmoid", 7.5)
    for plane in [comp.alpha.reshape(t * t, 1), comp.diffuse.reshape(t * t, 3)] + \
            [comp.sg_colors[i].reshape(t * t, 3) for i in range(lobes)] + [comp.lambdas[i].reshape(t * t, 3) for i in range(lobes)]:
        assert bool((plane.cpu()[~listed] == 0xAB).all())
    assert torch.equal(comp.diffuse.reshape(t * t, 3).cpu()[perm[keep].long()], want["diffuse"][keep])
    lib = _C.lib()
    assert lib.qf_bake_encode_texels(ctypes.byref(tex), args[0], feats.shape[1] - 1, *args[2:], _C.stream()) == -1
    assert lib.qf_bake_encode_texels(ctypes.byref(tex), args[0], args[1], args[2], args[3], -1, args[5], _C.stream()) == -1
    assert lib.qf_bake_encode_texels(ctypes.byref(tex), args[0], args[1], args[2], args[3], n, None, _C.stream()) == -1
    assert lib.qf_bake_encode_texels(None, *args, _C.stream()) == -1
    tex.n_lobes = 9
    assert lib.qf_bake_encode_texels(ctypes.byref(tex), *args, _C.stream()) != 0


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def producer_scene(device):
    """The scene of test_bake_texture_images_producer: T = 64, 3 lobes, log2_hashmap_size 12, 30 % empty texels; the
    oracle's codes are computed once."""
    from quadraturefields_amd import synthetic
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceField, NGPRadianceFieldSGNew
    lobes, t = 3, 64
    aabb = [-1.5] * 3 + [1.5] * 3
    sg = NGPRadianceFieldSGNew(aabb=aabb, use_viewdirs=False, num_g_lobes=lobes, log2_hashmap_size=12)
    sg.load_state_dict(synthetic.seeded_ngp_state(12, sg.mlp_base.grid.n_rows, sg_lobes=lobes), strict=False)
    nf = NGPRadianceField(aabb=aabb, log2_hashmap_size=12)
    nf.load_state_dict(synthetic.seeded_ngp_state(12, nf.mlp_base.grid.n_rows, seed=7), strict=False)
    sg, nf = sg.to(device), nf.to(device)
    rng = np.random.default_rng(0)
    V = rng.uniform(-1.2, 1.2, size=(t, t, 3)).astype(np.float32)
    V[rng.random((t, t)) < 0.3] = 0.0
    mask = V.sum(-1) != 0
    ind = np.argwhere(mask)
    pts = torch.from_numpy(V[ind[:, 0], ind[:, 1]])
    with torch.no_grad():
        feats = ofields.sg_features(pts, helpers.oracle_ngp_weights(sg))
        feats[:, -1] = ofields.query_density(pts, helpers.oracle_ngp_weights(nf)).flatten()
    want = oq.compress_features(feats, lobes, "sigmoid", 7.5)
    return {"lobes": lobes, "t": t, "sg": sg, "nf": nf, "V": V, "mask": mask, "ind": ind, "want": want}


def _set_planes(comp):
    n = comp.num_lobes
    return [("alpha", comp.alpha), ("diffuse", comp.diffuse)] + [(f"color_{i}", comp.sg_colors[i]) for i in range(n)] + \
           [(f"lambda_axis_{i}", comp.lambdas[i]) for i in range(n)]


def test_bake_texture_set_end_to_end(device, producer_scene, tmp_path):
    from quadraturefields_amd import baking
    from quadraturefields_amd.texture_utils import FeatureCompression
    s = producer_scene
    lobes, t, mask_np, ind, want = s["lobes"], s["t"], s["mask"], s["ind"], s["want"]
    V_d = torch.from_numpy(s["V"]).to(device)
    new = lambda: FeatureCompression(lobes, initialize=True, texture_size=t, compression_type="sigmoid", lambda_thres=7.5)
    comp, comp24, old = new(), new(), new()
    mask, count = baking.bake_texture_set(s["sg"], s["nf"], V_d, comp, rows_per_chunk=64)
    mask24, count24 = baking.bake_texture_set(s["sg"], s["nf"], V_d, comp24, rows_per_chunk=24)       # bands 24, 24, 16
    assert mask.dtype == torch.bool and mask.shape == (t, t) and count.dtype == torch.int64 and count.is_cuda
    assert torch.equal(mask.cpu(), torch.from_numpy(mask_np)) and torch.equal(mask24, mask)
    assert int(count) == int(count24) == int(mask_np.sum())
    for (name, a), (_, b) in zip(_set_planes(comp), _set_planes(comp24)):
        assert torch.equal(a, b), name                                                   # the chunking changes no byte
    for name, a in _set_planes(comp):
        assert int((a.cpu().numpy()[~mask_np] != 0).sum()) == 0, name                    # empty texels stay zero
    # default chunking (one band here) and the records cache: a set baked twice is read back fresh
    comp.records()
    baking.bake_texture_set(s["sg"], s["nf"], V_d, comp)
    assert getattr(comp, "_records", None) is None
    # against the oracle's features + quantisers: the bars of test_bake_texture_images_producer
    r, c = ind[:, 0], ind[:, 1]
    checks = [("alpha", comp.alpha[r, c].cpu(), want["alpha"], False), ("diffuse", comp.diffuse[r, c].cpu(), want["diffuse"], False)]
    for i in range(lobes):
        lam = comp.lambdas[i][r, c].cpu()
        checks += [(f"color_{i}", comp.sg_colors[i][r, c].cpu(), want["colors"][i], False),
                   (f"lambda_{i}", lam[:, 0], want["lambdas"][i][:, 0], False),
                   (f"azimuth_{i}", lam[:, 1], want["lambdas"][i][:, 1], True),
                   (f"elevation_{i}", lam[:, 2], want["lambdas"][i][:, 2], False)]
    for name, got, ref, wrap in checks:
        steps, share = _step_stats(got, ref, wrap)
        print(f"bake_texture_set vs oracle, {name}: max step {steps}, share {share:.5f}")
        assert steps <= 1 and share < 0.02, (name, steps, share)
    # against the reference's loop on the same device V: at most one step; the share is recorded, not bounded
    got_mask = baking.bake_texture_images(s["sg"], s["nf"], V_d, old, batch_size=1000)
    assert torch.equal(got_mask, mask)
    for (name, a), (_, b) in zip(_set_planes(comp), _set_planes(old)):
        a, b = a.cpu(), b.cpu()
        if name.startswith("lambda_axis"):
            parts = [(name + ".lambda", a[..., 0], b[..., 0], False), (name + ".azimuth", a[..., 1], b[..., 1], True),
                     (name + ".elevation", a[..., 2], b[..., 2], False)]
        else:
            parts = [(name, a, b, False)]
        for pname, pa, pb, wrap in parts:
            steps, share = _step_stats(pa, pb, wrap)
            print(f"bake_texture_set vs bake_texture_images, {pname}: max step {steps}, differing share {share:.6f}")
            assert steps <= 1, (pname, steps)
    # PNG save and reload
    comp.save_to_file(str(tmp_path) + "/")
    back = FeatureCompression(lobes, initialize=False, texture_size=t, path=str(tmp_path) + "/", compression_type="sigmoid",
                              lambda_thres=7.5)
    for (name, a), (_, b) in zip(_set_planes(comp), _set_planes(back)):
        assert torch.equal(a, b), name


# ------------------------------------------------------------------------------------------------ drivers
def test_bake_and_evaluate_drivers(device, tmp_path):
    from quadraturefields_amd import baking, synthetic, uv_atlas
    from quadraturefields_amd.mesh_io import load_mesh
    from quadraturefields_amd.mesh_utils import MeshIntersection, make_camera
    from quadraturefields_amd.metrics import FrameScorer
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceField
    from quadraturefields_amd.render import FrameRenderer
    from quadraturefields_amd.texture_utils import FeatureCompression, _read_png
    size, lobes, log2_t = 256, 3, 12
    root = str(tmp_path)
    mesh_uv, _ = uv_atlas.per_triangle_atlas(synthetic.shell_mesh(n_shells=2, subdivisions=1), size)
    mesh_path = os.path.join(root, f"mesh_segmentation_{size}.obj")
    mesh_uv.export_obj(mesh_path)
    V, _ = baking.texel_positions(mesh_uv, size)
    np.save(os.path.join(root, f"V_{size}.npy"), V.cpu().numpy())
    common = ["--mesh_path", mesh_path, "--texture_size", str(size), "--num_lobes", str(lobes), "--num_layers", "2",
              "--log2_hashmap_size", str(log2_t), "--scale", "1.5", "--compression_type", "linear", "--lambda_thres", "7.5"]
    bake = _example("bake_texture_images")
    bake.main(common + ["--synthetic"])
    tex_dir = os.path.join(root, f"texture_{size}")
    names = ["alpha.png", "diffuse.png"] + [f"color_{i}.png" for i in range(lobes)] + [f"lambda_axis_{i}.png" for i in range(lobes)]
    assert all(os.path.exists(os.path.join(tex_dir, n)) for n in names)
    mask_png = _read_png(os.path.join(root, f"mask_V_{size}.png"))
    # a direct bake of the same fields
    args = bake.parse(common + ["--synthetic"])
    sg, field = bake.load_fields(args, device)
    direct = FeatureCompression(lobes, initialize=True, texture_size=size, compression_type="linear", lambda_thres=7.5)
    mask, count = baking.bake_texture_set(sg, field, V, direct)
    assert np.array_equal(mask_png > 0, mask.cpu().numpy()) and int(count) == int(mask.sum())
    back = FeatureCompression(lobes, initialize=False, texture_size=size, path=tex_dir + "/", compression_type="linear",
                              lambda_thres=7.5)
    for (name, a), (_, b) in zip(_set_planes(direct), _set_planes(back)):
        assert torch.equal(a, b), name

    # stage 6d on those files
    ev = _example("evaluate_baked_textures")
    ev_args = common + ["--synthetic", "--root", root + "/", "--scene", "shells", "--exp_name", "bake", "--max_hits", "25",
                        "--size", "64", "--views", "2", "--up_sample", "2"]
    out = ev.main(ev_args)
    out_dir = os.path.join(root, "results", "shells", "bake")
    with open(os.path.join(out_dir, f"results_baking_textureimage_{size}_False_2.0.json")) as fh:
        res = json.load(fh)
    assert np.isfinite(res["psnr"]) and np.isfinite(res["ssim"]) and res["psnr"] == out["psnr"]
    for i in range(2):
        assert os.path.exists(os.path.join(out_dir, f"depth_baking_new_{size}_False_{i}.png"))
    # view 0 again, directly: render_baked + scorer
    mesh = load_mesh(mesh_path)
    mi = MeshIntersection(mesh, simplify_mesh=False, scale=1.0, num_intersections=25, render_step_size=5e-3, device=device)
    uv = torch.from_numpy(synthetic.scaled_uv(mesh, size)).to(device)
    fr = FrameRenderer(mi, NGPRadianceField(aabb=[-1.5] * 3 + [1.5] * 3, log2_hashmap_size=12).to(device))
    c2w = synthetic.orbit_cameras(2)[0]
    focal = synthetic.lego_focal(64)
    o, d = synthetic.camera_rays(c2w, focal, 64, 64, device=device)
    pixels = FrameRenderer(mi, sg).render(o, d, camera=make_camera(c2w, focal, 64, 64))[0]
    o2, d2 = synthetic.camera_rays(c2w, focal * 2, 128, 128, device=device)
    cam2 = make_camera(c2w, focal * 2, 128, 128)

    def psnr_of(compressor, image=None):
        scorer = FrameScorer(64, 64, up_sample=2, capacity=1, device=device)
        rgb = fr.render_baked(o2, d2, uv, compressor, camera=cam2)[0]
        scorer.score(rgb, pixels, images=True)
        if image is not None:
            assert np.array_equal(scorer.last_images()[0].cpu().numpy(), image)
        return float(scorer.results()["psnr"][0])

    psnr_baked = psnr_of(back, _read_png(os.path.join(out_dir, f"rgb_test_baking_new_{size}_False_0.png")))
    assert abs(psnr_baked - out["psnrs"][0]) <= 1e-9
    zero = FeatureCompression(lobes, initialize=True, texture_size=size, compression_type="linear", lambda_thres=7.5)
    psnr_zero = psnr_of(zero)
    print(f"PSNR of the baked set {psnr_baked:.3f} dB, of an all-zero set {psnr_zero:.3f} dB")
    assert psnr_baked > psnr_zero                                                        # the codes landed in the right texels


def test_fit_sg_driver_writes_a_checkpoint_the_bake_script_loads(device, tmp_path):
    fit = _example("fit_sg_synthetic")
    ckpt = os.path.join(str(tmp_path), "fit_sg.pth")
    with torch.enable_grad():
        res = fit.main(["--steps", "30", "--out", ckpt, "--size", "32", "--views", "4", "--rays", "1024", "--shells", "6",
                        "--subdivisions", "2", "--num_lobes", "3", "--log2_hashmap_size", "12"])
    print(res)
    assert res["steps"] == 30 and res["falling"] and np.isfinite(res["loss_last"])
    saved = torch.load(ckpt, map_location="cpu")
    assert set(saved) == {"estimator", "radiance_field"}
    bake = _example("bake_texture_images")
    args = bake.parse(["--mesh_path", "x.obj", "--num_lobes", "3", "--num_layers", "2", "--log2_hashmap_size", "12",
                       "--ckpt_path_sg", ckpt, "--synthetic"])
    sg, _ = bake.load_fields(args, device)
    for k, v in saved["radiance_field"].items():
        assert torch.equal(sg.state_dict()[k].cpu(), v), k
