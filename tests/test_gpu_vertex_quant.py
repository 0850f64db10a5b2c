"""The quantised vertex-baked renderer on the GPU (``include/qf_vertex_quant.h``): layout and
codes, decode, a reference-anchored blend, the shader and the frames against the fp32 route on the decoded table (bit for
bit), the one bound call, the side stream and the example.

Mesh, field, cameras and ``CONFIGS`` are ``tests/vertex_baked_reference``'s (the scenes of ``tests/test_gpu_vertex_baked.py``,
whose scene cache is shared); the codec inputs are ``tests/test_gpu_bake.py``'s kind of table at V = 5000 rows (T = 71: the
last row of the vertex texture is partly padding).  ``tests/test_vertex_quant_host.py`` checks on the CPU what the
early-termination cases rely on."""
import ctypes
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

from oracle import quantize as oq
from tests import baked_termination_reference as T
from tests import stream_harness as sh
from tests import test_gpu_vertex_baked as VB
from tests import vertex_baked_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DELTA = R.DELTA
CONFIGS, IDS = R.CONFIGS, R.IDS
STOPPING, STOPPING_IDS = VB.STOPPING, VB.STOPPING_IDS
CODECS = [("sigmoid", 7.5), ("linear", 5.0), ("sigma", 7.5)]       # "sigmoid" is NOT the sigmoid codec (B-7)
V_SYNTH, T_SYNTH = 5000, 71
_cache = {}
_bits = VB._bits


def _codec_table(lobes, seed):
    """5000 feature rows N(0, 3^2) with densities U(0, 400) in the last column and the edge rows of test_gpu_bake's codec
    inputs: zero axis, lambda = 0, colours beyond +-12 both ways, sigma = 0, a huge sigma."""
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(V_SYNTH, 3 + 7 * lobes + 1, generator=g) * 3.0
    feats[:, -1] = torch.rand(V_SYNTH, generator=g) * 400.0
    feats[0, 3:6] = 0.0
    feats[1, 3 + 3] = 0.0
    feats[2, :3] = 50.0
    feats[2, 3 + 4:3 + 7] = -50.0
    feats[3, :3] = -50.0
    feats[3, 3 + 4:3 + 7] = 50.0
    feats[4, -1] = 0.0
    feats[5, -1] = 1e9
    return feats


def _synthetic(device, lobes, ctype, thres):
    """(table on the host, its QuantisedVertexFeatures): built once per case, never modified."""
    from quadraturefields_amd import baking
    key = ("synthetic", lobes, ctype, thres)
    if key not in _cache:
        table = _codec_table(lobes, seed=11 + lobes)
        _cache[key] = (table, baking.quantise_vertex_features(table.to(device), compression_type=ctype, lambda_thres=thres))
    return _cache[key]


def _planes_of(comp):
    """[(name, plane on the host)] in the order of the PNG set."""
    out = [("alpha", comp.alpha.cpu()), ("diffuse", comp.diffuse.cpu())]
    for i in range(comp.num_lobes):
        out += [(f"color_{i}", comp.sg_colors[i].cpu()), (f"lambda_axis_{i}", comp.lambdas[i].cpu())]
    return out


def _vertex_texels(n, t, device):
    v = torch.arange(n, dtype=torch.int64, device=device)
    return torch.stack([v // t, v % t], dim=1)


def _quantised_scene(device, cfg, ctype="linear", override=False):
    """The scene of a configuration with its baked table quantised (``override``: the early-termination density column
    first), and that asset's decoded table."""
    from quadraturefields_amd import baking
    s = VB._scene(device, *cfg)
    key = ("q", s["lobes"], ctype, override)
    if key not in _cache:
        feats = R.override_density(s["feats"]) if override else s["feats"]
        q = baking.quantise_vertex_features(feats, compression_type=ctype)
        _cache[key] = (q, q.dequantise())
    return s, _cache[key][0], _cache[key][1]


# ------------------------------------------------------------------------------------------------ 1. layout and codes
@pytest.mark.parametrize("ctype,thres", CODECS)
@pytest.mark.parametrize("lobes", [1, 3, 6, 8])
def test_layout_and_codes(device, tmp_path, lobes, ctype, thres):
    from quadraturefields_amd import _C, baking
    from quadraturefields_amd.texture_utils import FeatureCompression
    table, q = _synthetic(device, lobes, ctype, thres)
    t, n = T_SYNTH, V_SYNTH
    assert (q.n_vertices, q.n_lobes, q.compressor.texture_size) == (n, lobes, t) and baking.vertex_texture_size(n) == t
    records = q.records()
    assert records.dtype == torch.uint8 and records.shape == (t * t, 64) and records.data_ptr() % 16 == 0
    # a direct encode launch on a zeroed 71 x 71 set with texel = arange(V): the same bytes; texels >= V are zero
    z = lambda *s: np.zeros(s, dtype=np.uint8)
    direct = FeatureCompression.from_arrays(z(t, t), z(t, t, 3), [z(t, t, 3) for _ in range(lobes)], [z(t, t, 3) for _ in range(lobes)],
                                            compression_type=ctype, lambda_thres=thres, device=device)
    tex = direct.texture_set()
    feats_d = table.to(device)
    sigma_d, texel = feats_d[:, -1].contiguous(), torch.arange(n, dtype=torch.int32, device=device)
    n_dev = torch.tensor([n], dtype=torch.int64, device=device)
    _C.check(_C.lib().qf_bake_encode_texels(ctypes.byref(tex), _C.ptr(feats_d), feats_d.shape[1], _C.ptr(sigma_d), _C.ptr(texel), n,
                                            _C.ptr(n_dev), _C.stream()), "qf_bake_encode_texels")
    want = oq.compress_features(table, lobes, ctype, thres)
    ref = [("alpha", want["alpha"][:, None]), ("diffuse", want["diffuse"])]
    for i in range(lobes):
        ref += [(f"color_{i}", want["colors"][i]), (f"lambda_axis_{i}", want["lambdas"][i])]
    worst = 0.0
    for (name, got), (_, dir_plane), (_, code) in zip(_planes_of(q.compressor), _planes_of(direct), ref):
        assert got.dtype == torch.uint8 and got.shape[:2] == (t, t)
        assert torch.equal(got, dir_plane), name
        flat = got.reshape(t * t, -1)
        assert not bool(flat[n:].any()), name
        # against the oracle's codes: the bars of tests/test_gpu_bake.py for the same kernel
        d = (flat[:n].to(torch.int16) - code.to(torch.int16)).abs()
        if name.startswith("lambda_axis"):                # channel 1 is the azimuth: codes 0 and 255 are neighbours
            d[:, 1] = torch.minimum(d[:, 1] % 256, 256 - d[:, 1] % 256)
        steps, share = int(d.max()), float((d.amax(dim=-1) > 0).float().mean())
        print(f"L={lobes} {ctype} thres={thres} {name}: max step {steps}, rows differing {share:.5f}")
        if ctype != "sigma" and (name == "diffuse" or name.startswith("color_")):
            assert steps == 0, name
        else:
            assert steps <= 1 and share < 0.002, (name, steps, share)
        worst = max(worst, share)
    print(f"L={lobes} {ctype} thres={thres}: worst plane {worst:.5f}")
    # save -> load: equal planes, hence equal records
    prefix = str(tmp_path / "vq_")
    q.save(prefix)
    back = baking.QuantisedVertexFeatures.load(prefix, n, lobes, compression_type=ctype, lambda_thres=thres, device=device)
    assert (back.n_vertices, back.n_lobes, back.compressor.texture_size) == (n, lobes, t)
    for (name, a), (_, b) in zip(_planes_of(q.compressor), _planes_of(back.compressor)):
        assert a.shape == b.shape and torch.equal(a, b), name
    assert torch.equal(back.records(), records)
    with pytest.raises(ValueError):
        baking.QuantisedVertexFeatures.load(prefix, t * t + 1, lobes, device=device)


# ---------------------------------------------------------------------------------------------------------- 2. decode
@pytest.mark.parametrize("ctype,thres", CODECS)
@pytest.mark.parametrize("lobes", [1, 3, 6, 8])
def test_decode_equals_the_texture_fetch_bit_for_bit(device, lobes, ctype, thres):
    _, q = _synthetic(device, lobes, ctype, thres)
    want = q.compressor.get_features_from_texture_map(_vertex_texels(V_SYNTH, T_SYNTH, device))
    got = q.dequantise()
    assert got.shape == (V_SYNTH, R.row_width(lobes)) and got.dtype == torch.float32
    assert np.array_equal(_bits(got), _bits(want))
    padded = q.dequantise(padded=True)
    assert padded.shape == (V_SYNTH, R.row_stride(lobes)) and padded.data_ptr() % 64 == 0
    assert np.array_equal(_bits(padded[:, :want.shape[1]]), _bits(want)) and not bool(padded[:, want.shape[1]:].any())


def test_decode_of_every_code_equals_the_texture_fetch(device):
    """The 256 x 256 set of test_gpu_golden.test_hip_quantisers_all_256_codes_vs_reference -- every code and every
    (azimuth, elevation) pair -- read as a vertex texture of V = 65 536: the new decoder equals qf_texture_fetch, which that
    test ties to the reference fixture."""
    from quadraturefields_amd import _C, baking
    from quadraturefields_amd.texture_utils import FeatureCompression
    codes = torch.arange(256, dtype=torch.uint8)
    ci = codes[:, None].expand(256, 256).contiguous()
    cj = codes[None, :].expand(256, 256).contiguous()
    idx = _vertex_texels(65536, 256, device)
    for codec, thres in CODECS:
        comp = FeatureCompression.from_arrays(
            ci, torch.stack([ci, cj, ci], -1), [torch.stack([cj, ci, cj], -1)], [torch.stack([ci, ci, cj], -1)],
            compression_type=codec, lambda_thres=thres, device=device)
        q = baking.QuantisedVertexFeatures(comp, 65536)
        want = comp.get_features_from_texture_map(idx)
        assert np.array_equal(_bits(q.dequantise()), _bits(want)), codec
        padded = q.dequantise(padded=True)
        assert np.array_equal(_bits(padded[:, :11]), _bits(want)) and not bool(padded[:, 11:].any()), codec
    # the entry point's own refusals
    rec, out = q.records(), torch.empty((65536, 16), device=device)
    call = lambda r=rec, n=65536, l=1, o=out, st=16: _C.lib().qf_vertex_quant_decode(_C.ptr(r), n, l, 0, 7.5, _C.ptr(o), st, _C.stream())
    assert call() == 0 and call(st=11) == 0
    for bad in (dict(r=None), dict(r=rec.reshape(-1)[4:]), dict(n=0), dict(l=0), dict(l=9), dict(o=None), dict(st=12), dict(st=32)):
        assert call(**bad) != 0, bad
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------- 3. the reference-anchored blend
def test_blend_is_anchored_to_the_reference_decoders(device):
    """CONFIGS[0]'s samples, linear codec.  The 3 + 3L colour columns: the linear decoder is exact, so the blend of
    ``code / 255 * 24 - 12`` in numpy fp32 must come out bit for bit.  The sigma, lambda and axis columns: against the blend
    of ``oracle.quantize.features_from_texture_map``'s rows.  A decoded value differs from the oracle's by at most e = atol
    + rtol |f| with test_gpu_golden's (atol, rtol) for that column -- sigma (1e-6, 2e-6), lambda (1e-7, 2e-6), axis (3e-7,
    0) -- and enters the blend once, weighted by |b_k| (the barycentrics lie in [-1e-4, 1 + 1e-4], host test of the parent);
    on top of that come 4 ulp of the result (fp32 spacing at |reference blend|) for the blend's own roundings."""
    from quadraturefields_amd import utils
    s, q, _ = _quantised_scene(device, CONFIGS[0])
    lobes, m = s["lobes"], R.mesh()
    n_v, t = m.vertices.shape[0], q.compressor.texture_size
    _, _, got = utils.shade_vertex_baked_points(s["mi"], q, s["xyzs"], s["index_tri"], s["dirs"], want_features=True)
    got = got.cpu().numpy()
    xyzs, tri = s["xyzs"].cpu().numpy(), s["index_tri"].cpu().numpy()
    comp = q.compressor
    flat = lambda p: p.cpu().numpy().reshape(t * t, -1)[:n_v]
    dec = lambda code: (code.astype(np.float32) / np.float32(255)) * np.float32(24) - np.float32(12)
    colour_cols = [0, 1, 2] + [3 + 7 * l + j for l in range(lobes) for j in (4, 5, 6)]
    colours = np.concatenate([dec(flat(comp.diffuse))] + [dec(flat(comp.sg_colors[l])) for l in range(lobes)], axis=1)
    want = R.blend(colours, m.vertices, m.faces, xyzs, tri)
    assert want.shape == (xyzs.shape[0], 3 + 3 * lobes)
    assert np.array_equal(_bits(got[:, colour_cols]), _bits(want))
    # the transcendental columns
    rows = oq.features_from_texture_map(_vertex_texels(n_v, t, "cpu"), comp.alpha.cpu(), comp.diffuse.cpu(),
                                        [comp.sg_colors[l].cpu() for l in range(lobes)], [comp.lambdas[l].cpu() for l in range(lobes)],
                                        "linear", 7.5).numpy().astype(np.float32)
    ref = R.blend(rows, m.vertices, m.faces, xyzs, tri).astype(np.float64)
    b = np.abs(R.barycentrics(m.vertices, m.faces, xyzs, tri).astype(np.float64))
    assert b.max() <= 1 + 1e-4
    corner = np.abs(rows.astype(np.float64))[m.faces[tri]]                      # [n, 3, W]
    bars = {R.row_width(lobes) - 1: (1e-6, 2e-6)}
    for l in range(lobes):
        bars.update({3 + 7 * l + j: (3e-7, 0.0) for j in range(3)})
        bars[3 + 7 * l + 3] = (1e-7, 2e-6)
    assert sorted(list(bars) + colour_cols) == list(range(R.row_width(lobes)))  # every column is held to one of the two bars
    worst = 0.0
    for c, (atol, rtol) in bars.items():
        decode = (b * (atol + rtol * corner[:, :, c])).sum(axis=1)
        bound = decode + 4.0 * np.spacing(np.abs(ref[:, c]).astype(np.float32)).astype(np.float64)
        err = np.abs(got[:, c].astype(np.float64) - ref[:, c])
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (c, float(err.max()), float((err / bound).max()))
    print(f"transcendental columns: worst error / bound {worst:.3f}")


# --------------------------------------------------------------------------------- 4. the shader against the fp32 route
@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_shader_equals_the_fp32_route_on_the_decoded_table(device, cfg):
    from quadraturefields_amd import _C, utils
    ctype = "sigma" if CONFIGS.index(cfg) % 2 else "linear"
    s, q, table = _quantised_scene(device, cfg, ctype)
    mi, n, wdt = s["mi"], s["xyzs"].shape[0], R.row_width(s["lobes"])
    want = utils.shade_vertex_baked_points(mi, table, s["xyzs"], s["index_tri"], s["dirs"], want_features=True)
    got = utils.shade_vertex_baked_points(mi, q, s["xyzs"], s["index_tri"], s["dirs"], want_features=True)
    assert got[2].shape == (n, wdt)
    for a, b, name in zip(got, want, ("rgb", "sigma", "features")):
        assert np.array_equal(_bits(a), _bits(b)), name
    assert bool(torch.isfinite(got[0]).all())
    got32 = utils.shade_vertex_baked_points(mi, q, s["xyzs"], s["index_tri"].to(torch.int32), s["dirs"], want_features=True)
    assert all(torch.equal(a, b) for a, b in zip(got32, got))
    rgb_only = utils.shade_vertex_baked_points(mi, q, s["xyzs"], s["index_tri"], s["dirs"])
    assert len(rgb_only) == 2 and torch.equal(rgb_only[0], got[0]) and torch.equal(rgb_only[1], got[1])
    # n_device short of n: the rows up to it as above, the rows beyond untouched (both id types)
    records, tri_records = utils.vertex_quant_shading(mi, q)
    points, dirs = _C.f32c(s["xyzs"]), _C.f32c(s["dirs"])
    nd = max(n - 37, 0)
    n_dev = torch.tensor([nd], dtype=torch.int64, device=device)
    for tri64, tri32 in ((s["index_tri"].contiguous(), None), (None, s["index_tri"].to(torch.int32))):
        o_f, o_rgb, o_sig = (torch.full(shape, -7.0, device=device) for shape in ((n, wdt), (n, 3), (n,)))
        _C.check(_C.lib().qf_vertex_quant_shade_points(
            _C.ptr(records), q.n_vertices, q.n_lobes, q.sigmoid_codec, 7.5, _C.ptr(tri_records), _C.ptr(points), _C.ptr(tri64),
            _C.ptr(tri32), _C.ptr(dirs), n, _C.ptr(n_dev), _C.ptr(o_f), _C.ptr(o_rgb), _C.ptr(o_sig), _C.stream()),
            "qf_vertex_quant_shade_points")
        assert torch.equal(o_f[:nd], got[2][:nd]) and torch.equal(o_rgb[:nd], got[0][:nd]) and torch.equal(o_sig[:nd], got[1][:nd])
        assert bool((o_f[nd:] == -7).all()) and bool((o_rgb[nd:] == -7).all()) and bool((o_sig[nd:] == -7).all())


def test_degenerate_face_shades_nan_at_the_same_positions(device):
    from quadraturefields_amd import _C, baking
    lobes = 3
    v = torch.tensor([[0, 0, 0], [2, 0, 0], [0, 3, 0], [1, 1, 1], [0, 0, 2]], dtype=torch.float64, device=device)
    f = torch.tensor([[0, 1, 2], [3, 3, 3], [2, 1, 4], [0, 1, 1]], dtype=torch.int64, device=device)
    tri_records = torch.empty((4, 128), dtype=torch.uint8, device=device)
    _C.check(_C.lib().qf_vertex_records_pack(_C.ptr(v), 5, _C.ptr(f), 4, _C.ptr(tri_records), _C.stream()), "qf_vertex_records_pack")
    q = baking.quantise_vertex_features(_codec_table(lobes, 3)[6:11].to(device))
    assert q.compressor.texture_size == 3
    table = q.dequantise(padded=True)
    pts = torch.tensor([[0.5, 0.5, 0.0], [1, 1, 1], [0.5, 1.0, 0.5], [1, 0, 0], [0.2, 0.1, 0.0], [1, 1, 1]], device=device)
    tri = torch.tensor([0, 1, 2, 3, 0, 1], dtype=torch.int64, device=device)
    dirs = torch.nn.functional.normalize(torch.tensor([[0.0, 0.6, 0.8]], device=device).expand(6, 3), dim=1).contiguous()
    n, wdt = 6, R.row_width(lobes)
    outs = []
    for quant in (False, True):
        o_f, o_rgb, o_sig = (torch.full(shape, -7.0, device=device) for shape in ((n, wdt), (n, 3), (n,)))
        tail = (_C.ptr(tri_records), _C.ptr(pts), _C.ptr(tri), None, _C.ptr(dirs), n, None, _C.ptr(o_f), _C.ptr(o_rgb), _C.ptr(o_sig),
                _C.stream())
        if quant:
            rc = _C.lib().qf_vertex_quant_shade_points(_C.ptr(q.records()), 5, lobes, 0, 7.5, *tail)
        else:
            rc = _C.lib().qf_vertex_shade_points(_C.ptr(table), table.shape[1], lobes, *tail)
        assert rc == 0
        outs.append((o_f, o_rgb, o_sig))
    for a, b in zip(*outs):                                   # NaN at the same positions (a NaN's sign and payload are the
        a, b = a.cpu().numpy(), b.cpu().numpy()               # instruction selection's), the same bits everywhere else
        assert np.array_equal(np.isnan(a), np.isnan(b))
        assert np.array_equal(_bits(a)[~np.isnan(a)], _bits(b)[~np.isnan(b)])
    nan_rows = torch.isnan(outs[1][1]).all(dim=1).cpu().tolist()
    assert nan_rows == [False, True, False, True, False, True]


def test_shade_points_refuses_what_the_header_says(device):
    """Each refusal with its status, and nothing launched: the outputs keep their fill."""
    from quadraturefields_amd import _C, utils
    s, q, _ = _quantised_scene(device, CONFIGS[0])
    records, tri_records = utils.vertex_quant_shading(s["mi"], q)
    n = 8
    pts, dirs, tri = _C.f32c(s["xyzs"][:n]), _C.f32c(s["dirs"][:n]), s["index_tri"][:n].contiguous()
    tri32 = tri.to(torch.int32)
    rgb, sig = torch.full((n, 3), -7.0, device=device), torch.full((n,), -7.0, device=device)
    feats = torch.full((n, R.row_width(s["lobes"])), -7.0, device=device)
    P = _C.ptr

    def call(rec=records, lobes=s["lobes"], t64=tri, t32=None, d=dirs, f=feats, r=rgb, sg=sig, nv=q.n_vertices):
        return _C.lib().qf_vertex_quant_shade_points(P(rec), nv, lobes, 0, 7.5, P(tri_records), P(pts), P(t64), P(t32), P(d), n, None,
                                                     P(f), P(r), P(sg), _C.stream())

    invalid, unsupported = -1, -3                        # QF_ERR_INVALID_ARGUMENT, QF_ERR_UNSUPPORTED (include/qf_hip.h)
    refusals = [(dict(rec=None), invalid), (dict(rec=records.reshape(-1)[4:]), invalid), (dict(nv=0), invalid),
                (dict(lobes=0), unsupported), (dict(lobes=9), unsupported), (dict(t32=tri32), invalid), (dict(t64=None), invalid),
                (dict(d=None), invalid), (dict(f=None, r=None, sg=None), invalid), (dict(sg=None), invalid), (dict(r=None), invalid)]
    for bad, status in refusals:
        assert call(**bad) == status, bad
    torch.cuda.synchronize()
    assert bool((rgb == -7).all()) and bool((sig == -7).all()) and bool((feats == -7).all())
    assert call() == 0 and call(f=None) == 0 and call(r=None, sg=None, d=None) == 0
    torch.cuda.synchronize()
    assert not bool((rgb == -7).any())


# ---------------------------------------------------------------------------------------------------------- 5. frames
@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_frames_equal_the_fp32_route_on_the_decoded_table(device, cfg):
    from quadraturefields_amd import utils
    from quadraturefields_amd.datasets.utils import Rays
    ctype = "sigma" if CONFIGS.index(cfg) % 2 else "linear"
    s, q, table = _quantised_scene(device, cfg, ctype)
    fr, ri = s["fr"], s["mi"].rayintersector
    major = utils.render_image_finetune_baking_with_occgrid(None, None, Rays(origins=s["o"], viewdirs=s["d"]), s["data"],
                                                            render_step_size=DELTA, mesh_intersect=s["mi"], vertex_features=q,
                                                            bg_color=s["bg"])
    got = fr.render_vertex_baked(s["o"], s["d"], q, camera=s["cam"])
    dec = fr.render_vertex_baked(s["o"], s["d"], table, camera=s["cam"])
    assert got[3] == dec[3] == major[3] == int(s["counts"].sum())
    for a, b, c in zip(got[:3], major[:3], dec[:3]):
        assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(c))
    plain = fr.render_vertex_baked(s["o"], s["d"], q, image_width=s["w"])
    assert all(torch.equal(a, b) for a, b in zip(plain[:3], got[:3]))
    # early_stop_eps = 0: the default route bit for bit, through the fused launch
    zero = fr.render_vertex_baked(s["o"], s["d"], q, camera=s["cam"], early_stop_eps=0.0)
    assert all(torch.equal(a, b) for a, b in zip(zero[:3], got[:3])) and zero[3] == got[3]
    assert ri.last_frame.shaded_count.cpu().numpy().tolist() == s["counts"].tolist()
    asy = fr.render_vertex_baked_async(s["o"], s["d"], q, s["cam"])
    assert all(torch.equal(a, b) for a, b in zip(asy[:3], got[:3])) and torch.equal(asy[3].shaded_count, asy[3].hit_count)
    # the separately bound launch, and its packed output
    frame = ri.sample_frame_device(s["o"], s["d"], s["k"], s["cam"], want_tri=True)
    _, xyz_c, dirs_c = ri.last_layout
    sep = utils.shade_composite_vertex_baked_frame(s["mi"], q, xyz_c, dirs_c, frame, DELTA, math.inf, bg_color=s["bg"])
    packed = utils.shade_composite_vertex_baked_frame(s["mi"], q, xyz_c, dirs_c, frame, DELTA, math.inf, bg_color=s["bg"], packed=True)
    ri._settle_deferred_policy()
    assert all(torch.equal(a, b) for a, b in zip(sep[:3], got[:3])) and torch.equal(sep[3], frame.hit_count)
    assert packed[1] is None and torch.equal(packed[0], torch.cat(got[:3], dim=1))
    # a table of another mesh is refused before anything is sampled
    from quadraturefields_amd import baking
    with pytest.raises(ValueError):
        fr.render_vertex_baked(s["o"], s["d"], baking.quantise_vertex_features(s["feats"][:-1]), camera=s["cam"])


@pytest.mark.parametrize("eps", [1e-2, 1e-3])
@pytest.mark.parametrize("cfg", STOPPING, ids=STOPPING_IDS)
def test_early_stop_equals_the_truncated_unfused_route(device, cfg, eps):
    """Counts and pixels exactly, on the overridden density quantised with the rest of the table (class 0: code 254, sigma
    1108; class 1: code 0); the 10 % / 10 % shares hold on the GPU's counts too."""
    s, q, table = _quantised_scene(device, cfg, "linear", override=True)
    fr, ri = s["fr"], s["mi"].rayintersector
    kept, rgb_w, alpha_w, depth_w = VB._stopping_reference(s, q, eps)          # the unfused QUANTISED shader, truncated
    rgb, alpha, depth, n = fr.render_vertex_baked(s["o"], s["d"], q, camera=s["cam"], early_stop_eps=eps)
    shaded = ri.last_frame.shaded_count.cpu().numpy()
    early, never = R.stop_shares(s["counts"], shaded)
    print(f"{cfg} eps {eps}: {int(shaded.sum())} of {n} samples shaded, reference {int(kept.sum())}; {early:.1%} of the pixels "
          f"with samples stop early, {never:.1%} never stop")
    assert early >= 0.10 and never >= 0.10
    assert n == int(s["counts"].sum()) and shaded.tolist() == kept.tolist() and int(shaded.sum()) < n
    assert torch.equal(rgb, rgb_w) and torch.equal(alpha, alpha_w) and torch.equal(depth, depth_w)
    # ... and the fp32 fused route on the decoded table: the same frame
    dec = fr.render_vertex_baked(s["o"], s["d"], table, camera=s["cam"], early_stop_eps=eps)
    assert all(torch.equal(a, b) for a, b in zip(dec[:3], (rgb, alpha, depth)))
    assert ri.last_frame.shaded_count.cpu().numpy().tolist() == kept.tolist()


def _bound_call(ri, job, shading, stop_tau, shaded):
    from quadraturefields_amd import _C
    return _C.lib().qf_frame_render_vertex_quant(ri._handle, ctypes.byref(job), ctypes.byref(shading), stop_tau, _C.ptr(shaded),
                                                 _C.stream())


@pytest.mark.parametrize("cfg", [CONFIGS[0], CONFIGS[6]], ids=[IDS[0], IDS[6]])
def test_one_bound_call_equals_the_separate_launches(device, cfg):
    from quadraturefields_amd import _C, utils
    s, q, _ = _quantised_scene(device, cfg, "linear", override=True)
    ri, n, mode = s["mi"].rayintersector, s["n_rays"], utils._BG[s["bg"]]
    shading, keep = utils.vertex_quant_shading_struct(s["mi"], q)
    for eps in (0.0, 1e-2):
        stop = float(T.stop_tau(eps))
        VB._plain_pass(ri)
        frame = ri.sample_frame_device(s["o"], s["d"], s["k"], s["cam"], want_tri=True)
        _, xyz_c, dirs_c = ri.last_layout
        want = utils.shade_composite_vertex_baked_frame(s["mi"], q, xyz_c, dirs_c, frame, DELTA, stop, bg_color=s["bg"])
        ri._settle_deferred_policy()
        VB._plain_pass(ri)
        assert ri.fused_frame_ready(s["cam"], s["k"])
        job, frame2, token = ri.fused_frame_job(s["o"], s["d"], s["k"], s["cam"], want_tri=True)
        rgb, alpha, depth = (torch.full((n, c), -7.0, device=device) for c in (3, 1, 1))
        shaded = torch.full((n,), -7, dtype=torch.int32, device=device)
        job.out_rgb, job.out_alpha, job.out_depth = rgb.data_ptr(), alpha.data_ptr(), depth.data_ptr()
        job.delta_const, job.bg_mode = DELTA, mode
        _C.check(_bound_call(ri, job, shading, stop, shaded), "qf_frame_render_vertex_quant")
        ri.fused_frame_done(frame2, token)
        assert torch.equal(rgb, want[0]) and torch.equal(alpha, want[1]) and torch.equal(depth, want[2])
        assert torch.equal(shaded, want[3])
        ri._settle_fused_policy(0)
        # the renderer takes the bound call on this frame: the same pixels
        VB._plain_pass(ri)
        asy = s["fr"].render_vertex_baked_async(s["o"], s["d"], q, s["cam"], early_stop_eps=eps)
        assert ri.last_route in ("frame", "frame+cull")
        assert torch.equal(asy[0], want[0]) and torch.equal(asy[3].shaded_count, want[3])


def test_spoiled_job_is_refused_before_the_first_launch(device):
    """A field in the job, no tri_c, a bad stop_tau, a bad shading struct: refused with every output buffer, the tile bases
    and the pinned block untouched."""
    from quadraturefields_amd import _C, utils
    s, q, _ = _quantised_scene(device, CONFIGS[0])
    ri, n = s["mi"].rayintersector, s["n_rays"]
    desc = _C.FieldDesc()

    def spoil_field(j, sh): j.field = ctypes.addressof(desc); return 1.0
    def spoil_tri(j, sh): j.tri_c = None; return 1.0
    def spoil_negative(j, sh): return -1.0
    def spoil_nan(j, sh): return math.nan
    def spoil_records(j, sh): sh.records = None; return 1.0
    def spoil_alignment(j, sh): sh.records = sh.records + 4; return 1.0
    def spoil_tri_records(j, sh): sh.tri_records = None; return 1.0
    def spoil_vertices(j, sh): sh.n_vertices = 0; return 1.0
    def spoil_lobes_zero(j, sh): sh.n_lobes = 0; return 1.0
    def spoil_lobes_nine(j, sh): sh.n_lobes = 9; return 1.0

    for spoil in (spoil_field, spoil_tri, spoil_negative, spoil_nan, spoil_records, spoil_alignment, spoil_tri_records,
                  spoil_vertices, spoil_lobes_zero, spoil_lobes_nine):
        VB._plain_pass(ri)
        shading, keep = utils.vertex_quant_shading_struct(s["mi"], q)
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
            _C.check(_bound_call(ri, job, shading, stop, shaded), "qf_frame_render_vertex_quant")
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
            utils.shade_composite_vertex_baked_frame(s["mi"], q, xyz_c, dirs_c, frame, DELTA, bad)
    ri._settle_deferred_policy()


# --------------------------------------------------------------------------------------------------------- 6. streams
# One case per new entry point.  The FRESH and the STALE set differ in the records' codes, positions and directions only
# (``records`` is an integer tensor, but one of values: named in ``varies``); mesh, triangle ids and counts are the same.
def _live_records(q, records):
    """A QuantisedVertexFeatures whose records are the case's live buffer (the harness refills it in place)."""
    from quadraturefields_amd import baking

    class Live(baking.QuantisedVertexFeatures):
        def __init__(self):                                   # the asset's own attributes, the live records
            self.compressor, self.n_vertices, self.n_lobes = q.compressor, q.n_vertices, q.n_lobes

        def records(self):
            return records

    return Live()


def _with_records(build):
    def wrapped(seed, device):
        from quadraturefields_amd import baking
        d = build(seed, device)
        q = baking.quantise_vertex_features(d.pop("table"))
        d["records"] = q.records().clone()
        d["q"] = _live_records(q, d["records"])
        torch.cuda.synchronize()
        return d
    return wrapped


def _decode_build(seed, device):
    from quadraturefields_amd import baking
    q = baking.quantise_vertex_features(VB._stream_table(seed, 700, device))
    records = q.records().clone()
    torch.cuda.synchronize()
    return dict(records=records, q=_live_records(q, records))


def _decode_call(i):
    return (i["q"].dequantise(padded=True),)


def _shade_call(i):
    from quadraturefields_amd import utils
    return utils.shade_vertex_baked_points(i["mi"], i["q"], i["points"], i["tri"], i["dirs"], want_features=True)


def _composite_call(i):
    from tests.test_gpu_streams import STEP, _frame_of
    from quadraturefields_amd import utils
    return utils.shade_composite_vertex_baked_frame(i["mi"], i["q"], i["xyz_c"], i["dirs_c"], _frame_of(i), STEP,
                                                    utils.early_stop_tau(1e-2))


def _bound_case_call(i):
    ri = i["mi"].rayintersector
    ri._raster_backoff = 0
    assert ri.fused_frame_ready(i["cam"], i["k"]), "the frame is not on the one-call route"
    rgb, alpha, depth, frame = i["fr"].render_vertex_baked_async(i["rays_o"], i["rays_d"], i["q"], i["cam"], early_stop_eps=1e-2)
    assert ri.last_route in ("frame", "frame+cull"), ri.last_route
    return rgb, alpha, depth, frame.shaded_count


_CASE = dict(varies=("records",), cpu_buildable=False)
STREAM_CASES = [
    sh.Case("vertex_quant_decode", _decode_build, _decode_call, entry_points=("qf_vertex_quant_decode",), **_CASE),
    sh.Case("vertex_quant_shade_points", _with_records(VB._shade_build), _shade_call,
            entry_points=("qf_vertex_quant_shade_points",), **_CASE),
    sh.Case("vertex_quant_composite_tiles", _with_records(VB._composite_build(40, 24, 5)), _composite_call,
            entry_points=("qf_vertex_quant_composite_tiles",), **_CASE),
    sh.Case("frame_render_vertex_quant-40x24", _with_records(VB._bound_build(40, 24, 25)), _bound_case_call,
            entry_points=("qf_frame_render_vertex_quant",), **_CASE),
]


def test_every_new_entry_point_has_a_stream_case():
    from quadraturefields_amd import _C
    assert sorted(ep for c in STREAM_CASES for ep in c.entry_points) == sorted(_C._VERTEX_QUANT_SIGNATURES)
    assert not any(c.host_wait for c in STREAM_CASES)                   # none waits on the host: the busy check applies


@pytest.mark.parametrize("name", [c.name for c in STREAM_CASES])
def test_entry_point_runs_entirely_on_the_callers_stream(device, lib, name):
    case = {c.name: c for c in STREAM_CASES}[name]
    issue_ms, delay_ms = sh.run_case(case, device)
    print(f"{name}: issue {issue_ms:.3f} ms, delay {delay_ms:.0f} ms")


# --------------------------------------------------------------------------------------------------------- 7. example
def test_example_quantises_saves_and_loads(device, tmp_path, capsys):
    """``examples/evaluate_vertex_baked.py --synthetic --quantise linear --save_quantised ...`` at its defaults prints a
    finite PSNR against the fp32 vertex frame; a second run with ``--load_quantised`` prints the same figures."""
    spec = importlib.util.spec_from_file_location("evaluate_vertex_baked", os.path.join(ROOT, "examples", "evaluate_vertex_baked.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    prefix = str(tmp_path / "asset" / "vq_")
    base = ["--synthetic", "--root", str(tmp_path / "run")]
    first = mod.main(base + ["--quantise", "linear", "--save_quantised", prefix])
    text = capsys.readouterr().out
    assert "psnr vs fp32 vertex frame:" in text and json.loads(text.strip().split("\n")[-1]) == first
    assert math.isfinite(first["psnr_vs_fp32_vertex"])
    assert math.isfinite(first["psnr"]) and os.path.exists(prefix + "alpha.png") and os.path.exists(prefix + "lambda_axis_5.png")
    second = mod.main(base + ["--load_quantised", prefix])
    assert second == first
    print(f"example: psnr {first['psnr']:.3f} dB against the field, {first['psnr_vs_fp32_vertex']:.3f} dB against the fp32 vertex frame")
