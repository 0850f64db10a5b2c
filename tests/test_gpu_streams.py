"""The C ABI on a side stream: every exported entry point that takes a ``void *stream`` either has a case here -- run
"stale, then fresh behind a delay" by ``tests/stream_harness.py`` -- or sits in ``SINGLE_LAUNCH`` with the reason, and
``test_every_stream_entry_point_is_accounted_for`` (no GPU needed) holds the two lists against include/qf_hip.h and the
sources.

Sizes are the smallest that still take every launch of the entry point: frames of 40x24 and 9x1, tables of 2^12 to
2^14, 4101 points (more than one workgroup and a ragged tail), meshes of shell_mesh(3, 1) to (4, 3), K in {5, 25}.  The
two input sets of a case differ in value arrays only; where an entry point's whole input is structural (the offset
scans, the layouts) the stale set is chosen so that any mixture of the two stays inside the outputs, which carry K
spare slots.  Rays of a camera frame differ by a direction jitter of ~0.004 px: far inside the 0.02 px the passes' ray
check allows, so the stale set is a valid pixel grid too, and still every hit distance differs in its low bits.
"""
import ctypes
import functools
import glob
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import stream_harness as sh
from tests.stream_harness import Case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_POINTS = 4101
FRAMES = [(40, 24), (9, 1)]
STEP = 5e-3


def _C():
    from quadraturefields_amd import _C as c
    return c


def _P(t, dtype=None):
    return _C().ptr(t, dtype)


def _st():
    return _C().stream()


def _ok(status, what):
    _C().check(status, what)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _unit(n, g):
    d = torch.randn(n, 3, generator=g)
    return (d / d.norm(dim=-1, keepdim=True)).contiguous()


def _sentinel(shape, dtype, device):
    """An output buffer; the harness fills it before every run."""
    return torch.zeros(shape, dtype=dtype, device=device)


# ====================================================================================================================
# synthetic frames: per-pixel hit lists that no intersector made (CPU-buildable)
# ====================================================================================================================
N_TRI = 5000


def _tile_scan(count, w, h, k):
    """(tile_base [tiles] int64, total) of the per-pixel counts clamped to k: the exclusive scan of the 8x8-tile totals."""
    tx, ty = (w + 7) // 8, (h + 7) // 8
    c = torch.zeros((ty * 8, tx * 8), dtype=torch.int64)
    c[:h, :w] = count.to(torch.int64).clamp(max=k).reshape(h, w)
    tot = c.reshape(ty, 8, tx, 8).sum(dim=(1, 3)).reshape(-1)
    return (torch.cumsum(tot, 0) - tot).contiguous(), int(tot.sum())


def _counts(seed, w, h, k, over=0):
    g = _gen(seed)
    c = torch.randint(0, k + 1 + over, (w * h,), generator=g, dtype=torch.int32)
    c[torch.rand(w * h, generator=g) < 0.2] = 0
    c[0] = k
    return c


def _swapped_in_tiles(count, w, h, seed):
    """The same counts with pixels swapped inside their 8x8 tile: other per-ray offsets, the same tile totals, tile bases
    and grand total -- whatever mixture of the two sets a launch sees, every index it forms stays below total + K."""
    g = _gen(seed)
    img = count.reshape(h, w).clone()
    for y0 in range(0, h, 8):
        for x0 in range(0, w, 8):
            blk = img[y0:y0 + 8, x0:x0 + 8]
            flat = blk.reshape(-1)
            img[y0:y0 + 8, x0:x0 + 8] = flat[torch.randperm(flat.numel(), generator=g)].reshape(blk.shape)
    return img.reshape(-1).contiguous()


def _lists(seed, w, h, k):
    """Value arrays of a frame: rays, sorted hit distances.  Structure (counts, ids) comes from a fixed seed."""
    g = _gen(seed)
    n = w * h
    o = (torch.tensor([[0.3, -2.0, 1.1]]) + 0.01 * seed).repeat(n, 1).contiguous()
    d = _unit(n, g)
    t = torch.sort(torch.rand(n, k, generator=g) * 3.0 + 2.0, dim=1)[0].contiguous()
    return o, d, t


def _structure(w, h, k):
    gs = _gen(7000 + w * h + k)
    count = _counts(7100 + w * h + k, w, h, k)
    tri = torch.randint(0, N_TRI, (w * h, k), generator=gs, dtype=torch.int32)
    return count, tri


def _to(d, device):
    return {k: (v.to(device) if isinstance(v, torch.Tensor) and not v.is_pinned() else v) for k, v in d.items()}


# --- qf_frame_offsets / qf_tile_offsets: wholly structural inputs -----------------------------------------------------
def _offsets_build(w, h, k, tiles, pinned):
    def build(seed, device):
        n = w * h
        count = _counts(7200 + w * h + k, w, h, k, over=3)          # raw counts above K too: the scans clamp
        if seed != 1:
            count = _swapped_in_tiles(count, w, h, seed)
        n_tiles = ((w + 7) // 8) * ((h + 7) // 8)
        d = dict(hit_count=count, words=torch.tensor([3 * seed, seed - 1], dtype=torch.int32),
                 out_ray_offset=_sentinel((n + 1,), torch.int64, "cpu"), out_tile_base=_sentinel((n_tiles,), torch.int64, "cpu"),
                 out_total=_sentinel((1,), torch.int64, "cpu"), out_zero=_sentinel((1,), torch.int32, "cpu"))
        d = _to(d, device)
        if str(device) != "cpu":
            nbytes = int(_C().lib().qf_frame_offsets_temp_bytes(n))
            d["tmp_scan"] = torch.zeros((max(nbytes, 8),), dtype=torch.uint8, device=device)
            if pinned:
                d["out_host"] = torch.zeros((4,), dtype=torch.int64).pin_memory()
        d.update(w=w, h=h, k=k, tiles=tiles)
        return d
    return build


def _frame_offsets_call(i):
    lib, n = _C().lib(), i["w"] * i["h"]
    words = i["words"]
    _ok(lib.qf_frame_offsets(_P(i["hit_count"]), n, i["k"], i["w"] if i["tiles"] else 0, i["h"] if i["tiles"] else 0,
                             _P(i["out_ray_offset"]), _P(i["out_tile_base"]) if i["tiles"] else None, _P(i["tmp_scan"]),
                             i["tmp_scan"].numel(), _P(words[:1]), _P(words[1:]),
                             ctypes.c_void_p(i["out_host"].data_ptr()) if "out_host" in i else None, 0, _st()),
        "qf_frame_offsets")
    outs = [i["out_ray_offset"]] + ([i["out_tile_base"]] if i["tiles"] else [])
    return tuple(outs + ([i["out_host"]] if "out_host" in i else []))


def _host_block(idx):
    """The pinned block's words the entry point writes ([2] is the pack's)."""
    def post(i, outs):
        return tuple(o[idx] if (not o.is_cuda and o.numel() == 4) else o for o in outs)
    return post


def _tile_offsets_call(i):
    lib = _C().lib()
    words = i["words"]
    _ok(lib.qf_tile_offsets(_P(i["hit_count"]), i["k"], i["w"], i["h"], _P(i["out_tile_base"]), _P(i["out_total"]),
                            _P(words[:1]), _P(words[1:]),
                            ctypes.c_void_p(i["out_host"].data_ptr()) if "out_host" in i else None, _P(i["out_zero"]), _st()),
        "qf_tile_offsets")
    return (i["out_tile_base"], i["out_total"], i["out_zero"]) + ((i["out_host"],) if "out_host" in i else ())


# --- qf_coherent_layout / qf_split_layout -----------------------------------------------------------------------------
def _layout_build(w, h, k):
    def build(seed, device):
        count = _counts(7300 + w * h + k, w, h, k)
        if seed != 1:
            count = _swapped_in_tiles(count, w, h, seed)
        tile_base, total = _tile_scan(count, w, h, k)
        c64 = count.to(torch.int64)
        ray_offset = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(c64, 0)])
        index_ray = torch.repeat_interleave(torch.arange(w * h), c64).contiguous()
        d = dict(hit_count=count, ray_offset=ray_offset, tile_base=tile_base, index_ray=index_ray,
                 out_order=_sentinel((total + k,), torch.int32, "cpu"), out_inverse=_sentinel((total + k,), torch.int32, "cpu"),
                 tmp_hit_count=torch.zeros_like(count), tmp_ray_offset=torch.zeros_like(ray_offset),
                 tmp_tile_base=torch.zeros_like(tile_base), out_invalid=_sentinel((1,), torch.int32, "cpu"))
        d = _to(d, device)
        d.update(w=w, h=h, total=total)
        return d
    return build


def _coherent_layout_call(i):
    _ok(_C().lib().qf_coherent_layout(_P(i["hit_count"]), _P(i["ray_offset"]), _P(i["tile_base"]), i["w"], i["h"],
                                      _P(i["out_order"]), _P(i["out_inverse"]), 0, _st()), "qf_coherent_layout")
    return i["out_order"][:i["total"]], i["out_inverse"][:i["total"]]


def _split_layout_call(i):
    _ok(_C().lib().qf_split_layout(_P(i["index_ray"]), i["total"], i["w"], i["h"], _P(i["tmp_hit_count"]),
                                   _P(i["tmp_ray_offset"]), _P(i["tmp_tile_base"]), _P(i["out_invalid"]), _P(i["out_order"]),
                                   _P(i["out_inverse"]), _st()), "qf_split_layout")
    return (i["out_order"][:i["total"]], i["out_inverse"][:i["total"]], i["out_invalid"], i["tmp_hit_count"],
            i["tmp_ray_offset"], i["tmp_tile_base"])


# --- the packs on synthetic lists -------------------------------------------------------------------------------------
MIN_SEP = 0.05          # the re-origin rule on: sorted distances 3 / K apart on average, so it drops hits


def _pack_build(w, h, k):
    def build(seed, device):
        n = w * h
        count, tri = _structure(w, h, k)
        o, dd, t = _lists(seed, w, h, k)
        tile_base, total = _tile_scan(count, w, h, k)
        c64 = count.to(torch.int64)
        ray_offset = (torch.cumsum(c64, 0) - c64).contiguous()
        inverse = torch.randperm(total, generator=_gen(7400 + n + k)).to(torch.int32)
        f32 = lambda *s: _sentinel(s, torch.float32, "cpu")            # noqa: E731
        d = dict(rays_o=o, rays_d=dd, hit_t=t, hit_tri=tri, hit_count=count, ray_offset=ray_offset, tile_base=tile_base,
                 total_dev=torch.tensor([total], dtype=torch.int64), inverse=inverse,
                 out_xyz=f32(total, 3), out_dirs=f32(total, 3), out_depth=f32(total), out_origins=f32(total, 3),
                 out_index_ray=_sentinel((total,), torch.int64, "cpu"), out_index_tri=_sentinel((total,), torch.int64, "cpu"),
                 out_xyz_c=f32(total, 3), out_dirs_c=f32(total, 3), out_depth_c=f32(total),
                 out_tri_c=_sentinel((total,), torch.int32, "cpu"), out_final=_sentinel((n,), torch.int32, "cpu"),
                 out_dropped=_sentinel((1,), torch.int32, "cpu"), acc_close=torch.zeros(1, dtype=torch.int32))
        d = _to(d, device)
        d.update(w=w, h=h, k=k, total=total)
        return d
    return build


def _pack_samples_call(i):
    n = i["w"] * i["h"]
    _ok(_C().lib().qf_pack_samples(
        _P(i["rays_o"]), _P(i["rays_d"]), n, i["k"], _P(i["hit_tri"]), _P(i["hit_t"]), _P(i["hit_count"]),
        _P(i["ray_offset"]), _P(i["out_xyz"]), _P(i["out_dirs"]), _P(i["out_index_ray"]), _P(i["out_depth"]),
        _P(i["out_index_tri"]), _P(i["out_origins"]), _P(i["inverse"]), _P(i["out_xyz_c"]), _P(i["out_dirs_c"]),
        _P(i["out_depth_c"]), None, None, MIN_SEP, _P(i["acc_close"]), _st()), "qf_pack_samples")
    return tuple(i[k] for k in ("out_xyz", "out_dirs", "out_index_ray", "out_depth", "out_index_tri", "out_origins",
                                "out_xyz_c", "out_dirs_c", "out_depth_c", "acc_close"))


def _pack_tiles_call(i):
    _ok(_C().lib().qf_pack_tiles(
        _P(i["rays_o"]), _P(i["rays_d"]), i["w"], i["h"], i["k"], _P(i["hit_tri"]), _P(i["hit_t"]), _P(i["hit_count"]),
        _P(i["tile_base"]), _P(i["total_dev"]), _P(i["out_xyz_c"]), _P(i["out_dirs_c"]), _P(i["out_depth_c"]),
        _P(i["out_tri_c"]), None, None, MIN_SEP, _P(i["out_final"]), _P(i["out_dropped"]), None, 0, _st()), "qf_pack_tiles")
    return tuple(i[k] for k in ("out_xyz_c", "out_dirs_c", "out_depth_c", "out_tri_c", "out_final", "out_dropped"))


# --- qf_resort_samples ------------------------------------------------------------------------------------------------
def _resort_build(seed, device):
    g = _gen(seed)
    w, h, k = 40, 24, 5
    count, _ = _structure(w, h, k)
    c64 = count.to(torch.int64)
    n = int(c64.sum())
    index_ray = torch.repeat_interleave(torch.arange(w * h), c64).contiguous()
    gs = _gen(7500)
    d = dict(index_ray=index_ray, depth=(torch.rand(n, generator=g) * 3 + 2), points=torch.randn(n, 3, generator=g),
             origins=torch.randn(n, 3, generator=g), vectors=_unit(n, g),
             index_tri=torch.randint(0, N_TRI, (n,), generator=gs), inverse=torch.randperm(n, generator=gs).to(torch.int32),
             out_perm=_sentinel((n,), torch.int64, "cpu"), out_points=_sentinel((n, 3), torch.float32, "cpu"),
             out_depth=_sentinel((n,), torch.float32, "cpu"), out_origins=_sentinel((n, 3), torch.float32, "cpu"),
             out_vectors=_sentinel((n, 3), torch.float32, "cpu"), out_index_tri=_sentinel((n,), torch.int64, "cpu"),
             out_boundary=_sentinel((n,), torch.uint8, "cpu"), out_points_c=_sentinel((n, 3), torch.float32, "cpu"),
             out_vectors_c=_sentinel((n, 3), torch.float32, "cpu"))
    d = _to(d, device)
    d["n"] = n
    return d


def _resort_call(i):
    outs = ("out_perm", "out_points", "out_depth", "out_origins", "out_vectors", "out_index_tri", "out_boundary")
    _ok(_C().lib().qf_resort_samples(_P(i["index_ray"]), _P(i["depth"]), i["n"], _P(i["points"]), _P(i["origins"]),
                                     _P(i["vectors"]), _P(i["index_tri"]), *[_P(i[k]) for k in outs], _P(i["inverse"]),
                                     _P(i["out_points_c"]), _P(i["out_vectors_c"]), _st()), "qf_resort_samples")
    return tuple(i[k] for k in outs + ("out_points_c", "out_vectors_c"))


# --- the tile compositors on a synthetic frame ------------------------------------------------------------------------
def _composite_build(w, h, k, trimax=False):
    def build(seed, device):
        g = _gen(seed)
        count, _ = _structure(w, h, k)
        tile_base, total = _tile_scan(count, w, h, k)
        gs = _gen(7600 + w * h)
        d = dict(rgb_c=torch.rand(total, 3, generator=g), sigma_c=torch.rand(total, generator=g) * 40.0,
                 depth_c=torch.rand(total, generator=g) * 3 + 2, hit_count=count, tile_base=tile_base,
                 tri_c=torch.randint(0, N_TRI, (total,), generator=gs, dtype=torch.int32),
                 acc_tri_weight=torch.zeros(N_TRI), acc_counts=torch.zeros(2, dtype=torch.int64),
                 acc_bad=torch.zeros(1, dtype=torch.int32), out_packed=_sentinel((w * h, 5), torch.float32, "cpu"))
        d = _to(d, device)
        d.update(w=w, h=h, k=k, total=total)
        return d
    return build


def _frame_of(i):
    return SimpleNamespace(depth_c=i["depth_c"], hit_count=i["hit_count"], max_hits=i["k"], tile_base=i["tile_base"],
                           width=i["w"], height=i["h"], total=i["total"], tri_c=i.get("tri_c"))


def _composite_call(i):
    from quadraturefields_amd import utils
    rgb, alpha, depth, weights = utils.composite_frame(i["rgb_c"], i["sigma_c"], _frame_of(i), STEP, want_weights=True)
    return rgb, alpha, depth, weights


def _trimax_call(i):
    c = _C()
    _ok(c.lib().qf_composite_tiles_trimax(
        _P(i["rgb_c"]), _P(i["sigma_c"]), _P(i["depth_c"]), STEP, _P(i["hit_count"]), i["k"], _P(i["tile_base"]), i["w"], i["h"],
        c.BG_WHITE, None, None, None, None, _P(i["out_packed"]), _P(i["tri_c"]), _P(i["acc_tri_weight"]), N_TRI, 1e-3,
        _P(i["acc_counts"]), _P(i["acc_bad"]), _st()), "qf_composite_tiles_trimax")
    return i["out_packed"], i["acc_tri_weight"], i["acc_counts"], i["acc_bad"]


# ====================================================================================================================
# the intersector: a real handle, a real camera
# ====================================================================================================================
@functools.lru_cache(maxsize=None)
def _mesh(shells, subdiv):
    from quadraturefields_amd import synthetic
    return synthetic.shell_mesh(n_shells=shells, subdivisions=subdiv)


_RI = {}
_ONCE = {}


def _ri(shells, subdiv, k):
    from quadraturefields_amd.mesh_io import TriMesh
    from quadraturefields_amd.mesh_utils import RayIntersector
    key = (shells, subdiv, k)
    if key not in _RI:
        m = _mesh(shells, subdiv)
        _RI[key] = RayIntersector(TriMesh(np.asarray(m.vertices, dtype=np.float32), m.faces), max_hits=k, min_separation=0)
    return _RI[key]


def _camera_rays(seed, w, h, device):
    """(cam, o, d): the pixel grid of one fixed camera; seed != 1 jitters every direction by ~0.004 px (module docstring)."""
    from quadraturefields_amd import synthetic
    from quadraturefields_amd.mesh_utils import make_camera
    c2w = synthetic.orbit_cameras(1, seed=1)[0]
    focal = synthetic.lego_focal(800) * max(w, 24) / 800.0
    o, d = synthetic.camera_rays(c2w, focal, w, h)
    if seed != 1:
        d = d + torch.randn(d.shape, generator=_gen(seed)) * (0.004 / focal / 1.7)
        d = d / d.norm(dim=-1, keepdim=True)
    return make_camera(c2w, focal, w, h), o.contiguous().to(device), d.contiguous().to(device)


def _random_rays(seed, n, device, radius=4.0):
    g = _gen(seed)
    o = _unit(n, g) * radius
    target = (torch.rand(n, 3, generator=g) * 2 - 1) * 0.9
    d = target - o
    return o.contiguous().to(device), (d / d.norm(dim=-1, keepdim=True)).contiguous().to(device)


def _hit_buffers(n, k, device, wide=0):
    d = dict(out_tri=_sentinel((n, k), torch.int32, device), out_t=_sentinel((n, k), torch.float32, device),
             out_words=_sentinel((n + 2,), torch.int32, device))
    if wide:
        d.update(tmp_wtri=torch.zeros((wide, n), dtype=torch.int32, device=device),
                 tmp_wt=torch.zeros((wide, n), dtype=torch.float32, device=device),
                 tmp_keys=torch.zeros((wide, n), dtype=torch.int64, device=device))
    return d


def _raster_build(shells, subdiv, w, h, k, wide=0, tiles=False):
    def build(seed, device):
        cam, o, d = _camera_rays(seed, w, h, device)
        i = dict(rays_o=o, rays_d=d, cam=cam, ri=_ri(shells, subdiv, k), w=w, h=h, k=k, wide=wide)
        i.update(_hit_buffers(w * h, k, device, wide))
        if tiles:
            n_tiles = ((w + 7) // 8) * ((h + 7) // 8)
            nbytes = int(_C().lib().qf_hit_bins_bytes(w, h, k))
            i.update(out_cursor=_sentinel((n_tiles,), torch.int32, device), out_mask=_sentinel((n_tiles,), torch.int64, device),
                     out_bins=_sentinel((nbytes // 8,), torch.int64, device), nbytes=nbytes)
        return i
    return build


def _words(i):
    n = i["w"] * i["h"]
    wd = i["out_words"]
    return wd[:n], wd[n:n + 1], wd[n + 1:]


def _raster_call(route, cull=0, sort_lists=1, slabs=2):
    def call(i):
        lib, n, k = _C().lib(), i["w"] * i["h"], i["k"]
        cnt, ovf, flag = _words(i)
        h, cam, o, d = i["ri"]._handle, ctypes.byref(i["cam"]), _P(i["rays_o"]), _P(i["rays_d"])
        i["ri"].set_min_separation(0.0)
        if route == "plain":
            _ok(lib.qf_raster_intersect(h, cam, o, d, n, k, _P(i["out_tri"]), _P(i["out_t"]), _P(cnt), _P(ovf), sort_lists, cull,
                                        _P(flag), _st()), "qf_raster_intersect")
        elif route == "wide":
            _ok(lib.qf_raster_intersect_wide(h, cam, o, d, n, k, i["wide"], _P(i["tmp_wtri"]), _P(i["tmp_wt"]), _P(i["out_tri"]),
                                             _P(i["out_t"]), _P(cnt), _P(ovf), cull, _P(flag), _st()), "qf_raster_intersect_wide")
        elif route == "slabs":
            _ok(lib.qf_raster_intersect_slabs(h, cam, o, d, n, k, i["wide"], slabs, _P(i["tmp_keys"]), _P(i["out_tri"]),
                                              _P(i["out_t"]), _P(cnt), _P(ovf), _P(flag), _st()), "qf_raster_intersect_slabs")
        else:
            _ok(lib.qf_raster_intersect_tiles(h, cam, o, d, n, k, _P(i["out_cursor"]), _P(i["out_mask"]), _P(i["out_bins"]),
                                              i["nbytes"], _P(cnt), _P(ovf), _P(flag), _st()), "qf_raster_intersect_tiles")
            return i["out_words"], i["out_cursor"], i["out_mask"], i["out_bins"]
        return i["out_tri"], i["out_t"], i["out_words"]
    return call


def _sorted_lists(i, outs):
    """Lists in arrival order compare as sets: every row's (t bits << 32 | tri) keys sorted (unwritten slots keep the
    sentinel in both runs), as tests/test_gpu_raster_passes.py compares them."""
    tri, t, words = outs
    keys = (t.view(torch.int32).to(torch.int64) << 32) | (tri.to(torch.int64) & 0xFFFFFFFF)
    keys = torch.sort(keys, dim=1)[0]
    lost = words[:keys.shape[0]] > tri.shape[1]          # a ray that lost candidates: its list is for the repair to rewrite
    return torch.where(lost[:, None], torch.zeros_like(keys), keys), words


def _sorted_bins(i, outs):
    """Bins hold their records in arrival order: every tile's row sorted.  A tile whose cursor ran past the capacity
    (64 K) keeps whichever records arrived first, its pixels are only known to be overflowed (count > K) and the overflow
    word is only specified without such a tile (tests/test_gpu_raster_passes.py reads no more of them): those are masked."""
    words, cursor, mask, bins = outs
    w, h, k = i["w"], i["h"], i["k"]
    n, n_tiles, tx = w * h, cursor.shape[0], (w + 7) // 8
    over = cursor > 64 * k
    rows = torch.sort(bins.reshape(n_tiles, -1), dim=1)[0]
    rows = torch.where(over[:, None], torch.zeros_like(rows), rows)
    ys, xs = torch.arange(h, device=words.device)[:, None], torch.arange(w, device=words.device)[None, :]
    tile_of = ((ys // 8) * tx + xs // 8).reshape(-1)
    cnt = words[:n]
    cnt = torch.where(over[tile_of] & (cnt > k), torch.full_like(cnt, k + 1), cnt)
    tail = torch.where(over.any(), torch.zeros_like(words[n:n + 1]), words[n:n + 1])
    return torch.cat([cnt, tail, words[n + 1:]]), cursor, mask, rows


def _bvh_intersect_build(seed, device):
    n, k = N_POINTS, 5
    o, d = _random_rays(seed, n, device)
    return dict(rays_o=o, rays_d=d, ri=_ri(4, 3, k), n=n, k=k, out_tri=_sentinel((n, k), torch.int32, device),
                out_t=_sentinel((n, k), torch.float32, device), out_cnt=_sentinel((n,), torch.int32, device))


def _bvh_intersect_call(i):
    i["ri"].set_min_separation(MIN_SEP)
    try:
        _ok(_C().lib().qf_bvh_intersect(i["ri"]._handle, _P(i["rays_o"]), _P(i["rays_d"]), i["n"], i["k"], 0, _P(i["out_tri"]),
                                        _P(i["out_t"]), _P(i["out_cnt"]), _st()), "qf_bvh_intersect")
    finally:
        i["ri"].set_min_separation(0.0)
    return i["out_tri"], i["out_t"], i["out_cnt"]


def _repair_build(seed, device):
    """The lists of a plain pass (arrival order, raw counts: K = 5 on three shells overflows) as the repair's in/out
    arrays.  Ids and counts are the FRESH rays' in both sets; the stale set differs in the rays and the distances."""
    w, h, k = 40, 24, 5
    cam, o, d = _camera_rays(seed, w, h, device)
    if "repair" not in _ONCE:                      # arrival order differs from run to run: ONE pass serves both sets
        i = _raster_build(3, 2, w, h, k)(1, device)
        _raster_call("plain", sort_lists=0)(i)
        torch.cuda.synchronize()
        _ONCE["repair"] = i
    i = _ONCE["repair"]
    n = w * h
    assert int((i["out_words"][:n] > k).sum()) > 0, "no pixel overflows: the repair would have nothing to do"
    t = i["out_t"].clone()
    t = torch.where(torch.isfinite(t) & (t.abs() < 1e10), t, torch.zeros_like(t))      # unwritten slots
    if seed != 1:
        t = t * (1.0 + 2.0 ** -12)
    return dict(rays_o=o, rays_d=d, hit_tri=i["out_tri"].clone(), hit_t=t, words=i["out_words"].clone(), ri=i["ri"], w=w, h=h,
                k=k, out_keep=_sentinel((n,), torch.int64, device), out_raw=_sentinel((n,), torch.int32, device))


def _repair_call(i):
    n = i["w"] * i["h"]
    wd = i["words"]
    i["ri"].set_min_separation(MIN_SEP)
    try:
        _ok(_C().lib().qf_bvh_repair_overflow(i["ri"]._handle, _P(i["rays_o"]), _P(i["rays_d"]), n, i["k"], i["w"], _P(i["hit_tri"]),
                                              _P(i["hit_t"]), _P(wd[:n]), _P(i["out_keep"]), _P(i["out_raw"]), _P(wd[n + 1:]),
                                              _st()), "qf_bvh_repair_overflow")
    finally:
        i["ri"].set_min_separation(0.0)
    return i["hit_tri"], i["hit_t"], i["words"], i["out_keep"], i["out_raw"]


def _repair_post(i, outs):
    """Rows the repair does not rewrite stay in arrival order; rows it rewrites come out sorted: compare sorted keys."""
    tri, t, words, keep, raw = outs
    keys, _ = _sorted_lists(i, (tri, t, words))
    return keys, words, keep, raw


def _filter_build(seed, device):
    w, h, k = 40, 24, 25
    count, tri = _structure(w, h, k)
    _, _, t = _lists(seed, w, h, k)
    t = t[torch.arange(w * h)[:, None], torch.argsort(torch.rand(w * h, k, generator=_gen(7700)), dim=1)].contiguous()
    d = _to(dict(hit_tri=tri, hit_t=t, hit_count=count), device)
    d.update(n=w * h, k=k, ri=_ri(3, 1, 25) if str(device) != "cpu" else None)
    return d


def _filter_call(i):
    i["ri"].set_min_separation(MIN_SEP)
    try:
        _ok(_C().lib().qf_filter_hits(i["ri"]._handle, i["n"], i["k"], _P(i["hit_tri"]), _P(i["hit_t"]), _P(i["hit_count"]),
                                      _st()), "qf_filter_hits")
    finally:
        i["ri"].set_min_separation(0.0)
    return i["hit_tri"], i["hit_t"], i["hit_count"]


def _filter_post(i, outs):
    """Only the first hit_count entries of a row are specified."""
    tri, t, cnt = outs
    live = torch.arange(tri.shape[1], device=tri.device)[None, :] < cnt[:, None]
    return torch.where(live, tri, -1), torch.where(live, t, 0.0), cnt


def _pack_bins_build(seed, device):
    """qf_raster_intersect_tiles -> repair -> qf_tile_offsets on the fresh rays (default stream, synchronised) make the bins,
    rows, counts and tile bases of BOTH sets; the stale set's rays and per-ray distances differ."""
    w, h, k = 40, 24, 5
    lib = _C().lib()
    cam, o, d = _camera_rays(seed, w, h, device)
    n = w * h
    if "bins" not in _ONCE:                        # the bins are in arrival order: ONE pass serves both sets
        i = _raster_build(3, 2, w, h, k, tiles=True)(1, device)
        sh._prefill(i)
        _raster_call("tiles")(i)
        cnt, ovf, flag = _words(i)
        _ok(lib.qf_bvh_repair_overflow(i["ri"]._handle, _P(i["rays_o"]), _P(i["rays_d"]), n, k, w, _P(i["out_tri"]), _P(i["out_t"]),
                                       _P(cnt), None, None, _P(flag), _st()), "qf_bvh_repair_overflow")
        n_tiles = i["out_cursor"].shape[0]
        tile_base = torch.zeros((n_tiles,), dtype=torch.int64, device=device)
        total = torch.zeros((1,), dtype=torch.int64, device=device)
        _ok(lib.qf_tile_offsets(_P(cnt), k, w, h, _P(tile_base), _P(total), None, None, None, None, _st()), "qf_tile_offsets")
        torch.cuda.synchronize()
        _ONCE["bins"] = (i, tile_base, total)
    i, tile_base, total = _ONCE["bins"]
    assert int(i["out_mask"].ne(0).sum()) > 0, "no overflowed pixel: the per-ray rows would not be read"
    cap = int(total.item())
    t = i["out_t"]
    t = torch.where(torch.isfinite(t) & (t.abs() < 1e10), t, torch.zeros_like(t))      # unwritten rows, +inf padding
    if seed != 1:
        t = t * (1.0 + 2.0 ** -12)
    f32 = lambda *s: _sentinel(s, torch.float32, device)            # noqa: E731
    return dict(rays_o=o, rays_d=d, hit_t=t.contiguous(), hit_tri=i["out_tri"].clone(), words=i["out_words"].clone(),
                tile_base=tile_base.clone(), total_dev=total.clone(), cursor=i["out_cursor"].clone(), mask=i["out_mask"].clone(),
                bins=i["out_bins"].clone(), out_xyz_c=f32(cap, 3), out_dirs_c=f32(cap, 3), out_depth_c=f32(cap),
                out_tri_c=_sentinel((cap,), torch.int32, device), out_final=_sentinel((n,), torch.int32, device),
                out_dropped=_sentinel((1,), torch.int32, device), w=w, h=h, k=k)


def _pack_bins_call(i):
    n = i["w"] * i["h"]
    wd = i["words"]
    _ok(_C().lib().qf_pack_tiles_bins(
        _P(i["rays_o"]), _P(i["rays_d"]), i["w"], i["h"], i["k"], _P(i["hit_tri"]), _P(i["hit_t"]), _P(wd[:n]), _P(i["tile_base"]),
        _P(i["total_dev"]), _P(i["out_xyz_c"]), _P(i["out_dirs_c"]), _P(i["out_depth_c"]), _P(i["out_tri_c"]), MIN_SEP,
        _P(i["out_final"]), _P(i["out_dropped"]), None, 0, _P(i["cursor"]), _P(i["mask"]), _P(i["bins"]), _P(wd[n + 1:]), _st()),
        "qf_pack_tiles_bins")
    return tuple(i[k] for k in ("out_xyz_c", "out_dirs_c", "out_depth_c", "out_tri_c", "out_final", "out_dropped"))


def _visible_build(seed, device):
    i = _raster_build(4, 3, 40, 24, 25)(seed, device)
    i["n_chunks"] = (int(_C().lib().qf_bvh_num_triangles(i["ri"]._handle)) + 63) // 64
    return i


def _visible_call(i):
    """A culled pass, then the host copy of its visible-chunk list (which waits for the stream)."""
    outs = _raster_call("plain", cull=1)(i)
    buf = np.full(i["n_chunks"], -1, dtype=np.int32)
    n = int(_C().lib().qf_bvh_copy_visible_chunks(i["ri"]._handle, buf.ctypes.data_as(ctypes.c_void_p), i["n_chunks"], _st()))
    assert 0 < n <= i["n_chunks"], n
    vis = torch.from_numpy(np.sort(buf[:n]))
    return outs + (vis,)


# ====================================================================================================================
# BVH build and refit: observed through qf_bvh_intersect with fixed rays on the same stream
# ====================================================================================================================
def _soup(seed, shells, subdiv):
    m = _mesh(shells, subdiv)
    v = torch.from_numpy(np.asarray(m.vertices, dtype=np.float32))
    if seed != 1:
        v = v * torch.tensor([0.9, 1.1, 0.95]) + 0.02 * torch.randn(v.shape, generator=_gen(seed))
    return v, torch.from_numpy(np.asarray(m.faces, dtype=np.int64))


def _probe(i, handle):
    n, k = i["n"], i["k"]
    _ok(_C().lib().qf_bvh_intersect(handle, _P(i["probe_o"]), _P(i["probe_d"]), n, k, 0, _P(i["out_tri"]), _P(i["out_t"]),
                                    _P(i["out_cnt"]), _st()), "qf_bvh_intersect")
    return i["out_tri"], i["out_t"], i["out_cnt"]


def _bvh_build_build(seed, device):
    v, f = _soup(seed, 3, 2)
    n, k = 1000, 5
    o, d = _random_rays(5, n, device)
    return dict(tri=v[f].contiguous().to(device), probe_o=o, probe_d=d, n=n, k=k, handles=[],
                out_tri=_sentinel((n, k), torch.int32, device), out_t=_sentinel((n, k), torch.float32, device),
                out_cnt=_sentinel((n,), torch.int32, device))


def _bvh_build_call(timed):
    def call(i):
        lib = _C().lib()
        while i["handles"]:                       # the previous runs' trees: their readers have long finished
            lib.qf_bvh_destroy(i["handles"].pop())
        handle = ctypes.c_void_p()
        if timed:
            ms, peak = (ctypes.c_float * 7)(), ctypes.c_int64(0)
            _ok(lib.qf_bvh_create_device_timed(_P(i["tri"]), i["tri"].shape[0], _st(), ctypes.cast(ms, ctypes.c_void_p),
                                               ctypes.cast(ctypes.pointer(peak), ctypes.c_void_p), ctypes.byref(handle)),
                "qf_bvh_create_device_timed")
            assert peak.value > 0
        else:
            _ok(lib.qf_bvh_create_device(_P(i["tri"]), i["tri"].shape[0], _st(), ctypes.byref(handle)), "qf_bvh_create_device")
        i["handles"].append(handle)
        return _probe(i, handle)
    return call


def _bvh_refit_build(host):
    def build(seed, device):
        from quadraturefields_amd.mesh_io import TriMesh
        from quadraturefields_amd.mesh_utils import RayIntersector
        v, f = _soup(seed, 3, 2)
        n, k = 1000, 5
        o, d = _random_rays(5, n, device)
        v0, _ = _soup(1, 3, 2)
        ri = RayIntersector(TriMesh(v0.numpy(), f.numpy()), max_hits=k, min_separation=0) if seed == 1 else None
        return dict(vertices=v.contiguous() if host else v.contiguous().to(device), probe_o=o, probe_d=d, n=n, k=k, ri=ri,
                    out_tri=_sentinel((n, k), torch.int32, device), out_t=_sentinel((n, k), torch.float32, device),
                    out_cnt=_sentinel((n,), torch.int32, device))
    return build


def _bvh_refit_call(i):
    v = i["vertices"]
    i["ri"].update_intersector(v if v.is_cuda else v.numpy())
    return _probe(i, i["ri"]._handle)


# ====================================================================================================================
# fields
# ====================================================================================================================
def _points(seed, device, half=1.5):
    from tests import helpers
    x, d = helpers.random_points(N_POINTS, aabb_half=half, seed=seed)
    return x.contiguous().to(device), d.contiguous().to(device)


_MODULES = {}


def _module(kind, device):
    """One module per kind, shared by the two builds of a case (the parameters are not what differs)."""
    key = (kind, str(device))
    if key not in _MODULES:
        from quadraturefields_amd.radiance_fields.ngp import NGPRadianceField, NGPRadianceFieldSGNew
        from tests.test_gpu_fp16 import _make
        if kind.startswith("ngp"):
            m = _make(NGPRadianceField, device, log2_T=12)
            m.compute_dtype = kind.split("-")[1]
        elif kind.startswith("sg"):
            m = _make(NGPRadianceFieldSGNew, device, log2_T=12, use_viewdirs=False, num_g_lobes=2)
            m.compute_dtype = kind.split("-")[1]
        elif kind.startswith("deform"):
            from tests.test_gpu_deform_fp16 import _field
            m = _field(device, log2_T=14)[0]
            m.compute_dtype = kind.split("-")[1]
        elif kind.startswith("extract"):
            from tests.test_gpu_grid_extract import _field
            m = _field(device, "elu", 16, log2_T=14)
            m = m[0] if isinstance(m, tuple) else m
            m.compute_dtype = kind.split("-")[1]
        else:
            raise KeyError(kind)
        _MODULES[key] = m
    return _MODULES[key]


def _field_build(kind):
    def build(seed, device):
        x, d = _points(seed, device, half=1.4 if kind.startswith("deform") else 1.5)
        return dict(x=x, d=d, module=_module(kind, device), kind=kind)
    return build


def _field_call(i):
    m = i["module"]
    if i["kind"].startswith("deform"):
        return (m(i["x"], return_grad=False)[0],)
    rgb, sigma = m(i["x"], i["d"])
    return rgb, sigma


def _features_call(i):
    """qf_field_forward's feature head and the density head with the geometry features."""
    m = i["module"]
    density, geo = m.query_density(i["x"], return_feat=True)
    return m.features(i["x"]), density, geo


def _grid_mlp_call(i):
    return (i["module"].mlp_base((i["x"] / 3.0 + 0.5).contiguous()),)


def _extract_build(kind):
    def build(seed, device):
        from quadraturefields_amd import field_utils
        m = _module(kind, device)
        g = 12
        axis = field_utils.lattice_axis(g, float(m.scale)) * (1.0 if seed == 1 else 0.97)
        return dict(axis=axis.contiguous().to(device), module=m, g=g, out_value=_sentinel((g, g, g), torch.float32, device),
                    out_grad=_sentinel((g, g, g), torch.float16, device))
    return build


def _extract_call(i):
    from quadraturefields_amd import field_utils
    field_utils._fused_slab(i["module"], i["axis"], i["g"], 0, i["g"], i["out_value"], i["out_grad"], pool=2)
    return i["out_value"], i["out_grad"]


def _adam_build(seed, device):
    g = _gen(seed)
    n = (1 << 14) + 37
    return _to(dict(param=torch.randn(n, generator=g), grad=torch.randn(n, generator=g) * 1e-2,
                    exp_avg=torch.randn(n, generator=g) * 1e-3, exp_avg_sq=torch.rand(n, generator=g) * 1e-4), device) | {"n": n}


def _adam_call(i):
    _ok(_C().lib().qf_adam_step(_P(i["param"]), _P(i["grad"]), _P(i["exp_avg"]), _P(i["exp_avg_sq"]), i["n"], 1e-2, 0.9, 0.999,
                                1e-15, 0.0, 0, 3, _st()), "qf_adam_step")
    return i["param"], i["exp_avg"], i["exp_avg_sq"]


# ====================================================================================================================
# training kernels (accumulating weight gradients: float atomics -- compared as their own tests compare them)
# ====================================================================================================================
def _asserting(fn):
    """An assertion-style check of an existing test as a harness ``compare``: None, or the assertion's text."""
    try:
        fn()
    except AssertionError as e:
        return str(e) or "assertion failed"
    return None


def _bits(got, want, idx):
    for j in idx:
        if not sh.same_bits(got[j], want[j]):
            return f"output {j}: {int((got[j] != want[j]).sum())} of {got[j].numel()} elements differ"
    return None


def _ngp_bwd_build(seed, device):
    from tests import test_gpu_mlp_backward as T
    c = T._ngp_case(_C().lib(), device, N_POINTS, seed=40 + seed, prefill=False)
    enc, dirs, sel, d_rgb, d_sigma, base_w, head_w = c["inputs"]
    return dict(enc=enc, dirs=dirs, sel=sel, d_rgb=d_rgb.contiguous(), d_sigma=d_sigma.contiguous(), base_w=base_w, head_w=head_w,
                ref=c["ref"], acc_g_base=torch.zeros(3072, device=device), acc_g_head=torch.zeros(7168, device=device),
                out_d_enc=_sentinel((N_POINTS, 32), torch.float32, device))


def _ngp_bwd_call(i):
    _ok(_C().lib().qf_ngp_mlp_backward(_P(i["enc"]), _P(i["dirs"]), _P(i["sel"]), _P(i["d_rgb"]), _P(i["d_sigma"]), _P(i["base_w"]),
                                       _P(i["head_w"]), N_POINTS, _P(i["out_d_enc"]), _P(i["acc_g_base"]), _P(i["acc_g_head"]),
                                       _st()), "qf_ngp_mlp_backward")
    return i["out_d_enc"], i["acc_g_base"], i["acc_g_head"]


def _ngp_bwd_compare(got, want, fresh):
    from tests import test_gpu_mlp_backward as T
    ref = fresh["ref"]
    return _bits(got, want, [0]) or _asserting(lambda: (
        T.check_weights("ngp", "stream", "grad_base_w", got[1], ref["grad_base_w"]),
        T.check_weights("ngp", "stream", "grad_head_w", got[2], ref["grad_head_w"])))


SG_LOBES = 2


def _sg_bwd_build(seed, device):
    from tests import mlp_backward_reference as R
    from tests import test_gpu_mlp_backward as T
    c = T._sg_case(_C().lib(), device, N_POINTS, SG_LOBES, seed=60 + seed, prefill=False)
    base_w, head = T._sg_weights(device, SG_LOBES)
    d = dict(enc=c["enc"], sel=c["sel"], d_feat=torch.nan_to_num(c["d_feat"], nan=0.0).contiguous(), d_sigma=c["d_sigma"].contiguous(),
             base_w=base_w, ref=c["ref"], acc_g_base=torch.zeros(3072, device=device),
             out_d_enc=_sentinel((N_POINTS, 32), torch.float32, device))
    for k in R.SG_HEAD_NAMES:
        d["head_" + k] = head[k]
        d["acc_g_" + k] = torch.zeros_like(head[k])
    return d


def _sg_bwd_call(i):
    from tests import mlp_backward_reference as R
    c = _C()
    h = c.SGHead(*[_P(i["head_" + k]) for k in R.SG_HEAD_NAMES])
    gh = c.SGHead(*[_P(i["acc_g_" + k]) for k in R.SG_HEAD_NAMES])
    _ok(c.lib().qf_sg_mlp_backward(_P(i["enc"]), _P(i["sel"]), _P(i["d_feat"]), i["d_feat"].shape[1], _P(i["d_sigma"]),
                                   _P(i["base_w"]), ctypes.byref(h), SG_LOBES, N_POINTS, _P(i["out_d_enc"]), _P(i["acc_g_base"]),
                                   ctypes.byref(gh), _st()), "qf_sg_mlp_backward")
    return (i["out_d_enc"], i["acc_g_base"]) + tuple(i["acc_g_" + k] for k in R.SG_HEAD_NAMES)


def _sg_bwd_compare(got, want, fresh):
    from tests import mlp_backward_reference as R
    from tests import test_gpu_mlp_backward as T
    ref = fresh["ref"]
    return _bits(got, want, [0]) or _asserting(lambda: [
        T.check_weights("sg", "stream", name, g, ref[name]) for name, g in zip(("grad_base_w",) + R.SG_HEAD_NAMES, got[1:])])


def _deform_bwd_build(seed, device):
    from tests import mlp_backward_reference as R
    from tests import test_gpu_mlp_backward as T
    c = T._deform_case(_C().lib(), device, N_POINTS, seed=80 + seed, prefill=False)
    w = T._deform_weights(device)
    d = dict(enc=c["enc"], x01=c["x01"], d_out=c["d_out"].contiguous(), ref=c["ref"],
             out_d_enc=_sentinel((N_POINTS, 32), torch.float32, device), out_d_x01=_sentinel((N_POINTS, 3), torch.float32, device))
    for k in R.DEFORM_NAMES:
        d["w_" + k] = w[k]
        d["acc_g_" + k] = torch.zeros_like(w[k])
    return d


def _deform_bwd_call(i):
    from tests import mlp_backward_reference as R
    _ok(_C().lib().qf_deform_mlp_backward(_P(i["enc"]), _P(i["x01"]), _P(i["d_out"]), *[_P(i["w_" + k]) for k in R.DEFORM_NAMES[:5]],
                                          N_POINTS, _P(i["out_d_enc"]), _P(i["out_d_x01"]),
                                          *[_P(i["acc_g_" + k]) for k in R.DEFORM_NAMES], _st()), "qf_deform_mlp_backward")
    return (i["out_d_enc"], i["out_d_x01"]) + tuple(i["acc_g_" + k] for k in R.DEFORM_NAMES)


def _deform_bwd_compare(got, want, fresh):
    from tests import mlp_backward_reference as R
    from tests import test_gpu_mlp_backward as T
    ref = fresh["ref"]
    return _bits(got, want, [0, 1]) or _asserting(lambda: [
        T.check_weights("deform", "stream", name, g, ref[name]) for name, g in zip(R.DEFORM_NAMES, got[2:])])


def _field_loss_build(seed, device):
    from tests import field_loss_reference as R
    from tests.test_gpu_field_loss import _field
    f, wts = _field(device, "hashed")
    inp, _ = R.clean_inputs(N_POINTS, seed=300 + seed, wts=wts)
    ref = R.reference(inp, wts, upstream=1.0)
    dv = inp.to(device)
    c = _C()
    d = dict(x=dv.x, dirs=dv.dirs, weights=dv.weights, weights_rev=dv.weights_rev, field=f, ref=ref,
             out_loss=_sentinel((1,), torch.float64, device), out_value=_sentinel((N_POINTS,), torch.float32, device),
             out_grad=_sentinel((N_POINTS, 3), torch.float32, device), out_d_enc=_sentinel((N_POINTS, 32), torch.float32, device),
             tmp_ws=torch.zeros((c.FIELD_LOSS_WORKSPACE_BYTES,), dtype=torch.uint8, device=device))
    for k in R.NAMES:
        d["acc_g_" + k] = torch.zeros(ref[k][1].shape, dtype=torch.float32, device=device)
    return d


def _field_loss_call(i):
    from tests import field_loss_reference as R
    c, f = _C(), i["field"]
    _ok(c.lib().qf_field_quadrature_loss(
        f.xyz_encoder.grid.desc, _P(f.xyz_encoder.params.detach()), float(f.scale), f.hidden_size, f.activation_code,
        *[_P(t) for t in f.decoder_arrays()], _P(i["x"]), _P(i["dirs"]), _P(i["weights"]), _P(i["weights_rev"]), N_POINTS, None,
        _P(i["out_loss"]), _P(i["out_value"]), _P(i["out_grad"]), _P(i["out_d_enc"]), *[_P(i["acc_g_" + k]) for k in R.NAMES],
        _P(i["tmp_ws"]), c.FIELD_LOSS_WORKSPACE_BYTES, _st()), "qf_field_quadrature_loss")
    return (i["out_loss"], i["out_value"], i["out_grad"], i["out_d_enc"]) + tuple(i["acc_g_" + k] for k in R.NAMES)


def _field_loss_compare(got, want, fresh):
    from tests import field_loss_reference as R
    from tests import test_gpu_field_loss as T
    ref = fresh["ref"]
    return _bits(got, want, [0, 1, 2, 3]) or _asserting(lambda: [
        T.check_weights("stream", name, g, ref[name]) for name, g in zip(R.NAMES, got[4:])])


def _distortion_build(seed, device):
    from tests.test_gpu_distortion import LENGTHS, make_rays
    w, m, d, ray_id, n_rays = make_rays(LENGTHS * 4, 500 + seed)
    return _to(dict(w=torch.from_numpy(w), m=torch.from_numpy(m), interval=torch.from_numpy(d),
                    ray_id=torch.from_numpy(ray_id)), device) | {"n_rays": n_rays}


def _distortion_call(i):
    from quadraturefields_amd import losses
    loss, grad = losses._launch(i["w"], i["m"], i["interval"], 0.0, i["ray_id"], 0, i["n_rays"], True)
    return loss.reshape(1), grad


# --- hash-grid backward: the scatter routes tests/test_gpu_grid_backward.py reaches -----------------------------------
def _grid_desc(config):
    from tests import grid_backward_reference as R
    c = _C()
    if config == "small":
        from oracle import fields as ofields
        return c.make_grid_desc(16, 14, 16, ofields.ngp_per_level_scale(4096, 16, 16))
    log2_t, base, b = R.init_args(config)
    return c.make_grid_desc(16, log2_t, base, b)


def _grid_bwd_build(config, n, second=False):
    def build(seed, device):
        from tests import grid_backward_reference as R
        from tests.test_gpu_grid_backward import _inputs
        desc = _grid_desc(config)
        x, table, dfeat, v = _inputs(desc, n, device, seed=900 + seed)
        ref = R.grid_double_backward_ref(desc, x, table, dfeat, v) if second else R.grid_backward_ref(desc, x, table, dfeat)
        nbytes = int(_C().lib().qf_grid_backward_workspace_bytes(n))
        return dict(x=x, table=table, dfeat=dfeat, v=v, desc=desc, n=n, ref=ref, acc_grad_table=torch.zeros_like(table),
                    out_dx=_sentinel((n, 3), torch.float32, device), out_g_dfeat=_sentinel((n, 32), torch.float32, device),
                    tmp_ws=torch.zeros((max(nbytes, 1),), dtype=torch.uint8, device=device), ws_bytes=nbytes)
    return build


def _grid_bwd_call(route):
    def call(i):
        lib, n = _C().lib(), i["n"]
        d = ctypes.byref(i["desc"])
        if route == "plain":
            _ok(lib.qf_grid_encode_backward(d, _P(i["table"]), _P(i["x"]), _P(i["dfeat"]), n, _P(i["acc_grad_table"]), _P(i["out_dx"]),
                                            _st()), "qf_grid_encode_backward")
        elif route == "ws":
            _ok(lib.qf_grid_encode_backward_ws(d, _P(i["table"]), _P(i["x"]), _P(i["dfeat"]), n, _P(i["acc_grad_table"]),
                                               _P(i["out_dx"]), _P(i["tmp_ws"]), i["ws_bytes"], _st()), "qf_grid_encode_backward_ws")
        else:
            _ok(lib.qf_grid_encode_double_backward(d, _P(i["table"]), _P(i["x"]), _P(i["dfeat"]), _P(i["v"]), n, _P(i["out_g_dfeat"]),
                                                   _P(i["out_dx"]), _P(i["acc_grad_table"]), _P(i["tmp_ws"]), i["ws_bytes"], _st()),
                "qf_grid_encode_double_backward")
            return i["out_g_dfeat"], i["out_dx"], i["acc_grad_table"]
        return i["out_dx"], i["acc_grad_table"]
    return call


def _grid_bwd_compare(got, want, fresh):
    """Per-point outputs bit for bit; the table gradient (fp32 atomics) against the fp64 reference at the bar of
    tests/test_gpu_grid_backward.py: (k + 8) u M."""
    from tests.test_gpu_grid_backward import check
    ref = fresh["ref"]
    return _bits(got, want, range(len(got) - 1)) or _asserting(
        lambda: check("stream", "grad_table", got[-1], ref["grad_table"], ref["k"]))


# ====================================================================================================================
# geometry stages
# ====================================================================================================================
def _mc_build(seed, device):
    n = 20
    ax = torch.linspace(-1, 1, n)
    p = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), dim=-1)
    vol = 0.8 - p.norm(dim=-1) * (1.0 + 0.1 * torch.rand(n, n, n, generator=_gen(seed)))
    return dict(volume=vol.contiguous().to(device))


def _mc_call(i):
    from quadraturefields_amd import mc_utils
    return mc_utils.marching_cubes(i["volume"], 0.3)


def _cluster_build(seed, device):
    v, f = _soup(seed, 3, 1)
    return dict(vertices=v.to(torch.float64).contiguous().to(device), faces=f.contiguous().to(device))


def _cluster_call(i):
    from quadraturefields_amd import mc_utils
    return mc_utils.simplify_vertex_clustering(i["vertices"], i["faces"], 0.2, "quadric")


# The two wrappers above read the counts back between their count and emit calls: by then the delay has drained, so they
# say nothing about the emit.  The cases below bind count and emit back to back through the C ABI, with the output
# capacities of a synchronised run; the stale set has the same STRUCTURE (sign pattern against the level; cells), so the
# counts, the capacities and every offset in the workspace agree whatever mixture a launch sees.
MC_LEVEL, MC_N = 0.3, 20


def _mc_raw_build(seed, device):
    fresh = _mc_build(1, "cpu")["volume"]
    vol = fresh
    if seed != 1:       # the same side of the level everywhere, another distance from it: other vertices, the same topology
        vol = (MC_LEVEL + (fresh - MC_LEVEL) * (0.5 + torch.rand(fresh.shape, generator=_gen(seed)))).contiguous()
        assert torch.equal(vol > MC_LEVEL, fresh > MC_LEVEL) and not bool((vol == MC_LEVEL).any())
    d = dict(volume=vol.to(device), out_counts=_sentinel((3,), torch.int64, device))
    if str(device) != "cpu":
        from quadraturefields_amd import mc_utils
        if "mc" not in _ONCE:
            verts, faces = mc_utils.marching_cubes(fresh.to(device), MC_LEVEL)
            torch.cuda.synchronize()
            _ONCE["mc"] = (int(verts.shape[0]), int(faces.shape[0]))
        nv, nf = _ONCE["mc"]
        assert nv > 100 and nf > 100                       # a real surface: more than one workgroup of cells emit
        nbytes = int(_C().lib().qf_marching_cubes_workspace_bytes(MC_N, MC_N, MC_N))
        d.update(nv=nv, nf=nf, ws_bytes=nbytes, tmp_ws=torch.zeros((nbytes,), dtype=torch.uint8, device=device),
                 out_verts=_sentinel((nv, 3), torch.float32, device), out_faces=_sentinel((nf, 3), torch.int32, device))
    return d


def _mc_raw_call(i):
    lib, n = _C().lib(), MC_N
    _ok(lib.qf_marching_cubes_count(_P(i["volume"]), n, n, n, MC_LEVEL, _P(i["tmp_ws"]), i["ws_bytes"], _P(i["out_counts"]), _st()),
        "qf_marching_cubes_count")
    _ok(lib.qf_marching_cubes_emit(_P(i["volume"]), n, n, n, MC_LEVEL, _P(i["tmp_ws"]), i["ws_bytes"], _P(i["out_verts"]), i["nv"],
                                   _P(i["out_faces"]), i["nf"], _st()), "qf_marching_cubes_emit")
    return i["out_counts"], i["out_verts"], i["out_faces"]


def _mc_raw_post(i, outs):
    assert outs[0].tolist() == [i["nv"], i["nf"], 0], (outs[0].tolist(), i["nv"], i["nf"])
    return outs


CLUSTER_S = 0.2


def _cluster_cells(v):
    lo = v.min(dim=0)[0] - 0.5 * CLUSTER_S
    return torch.floor((v - lo) / CLUSTER_S)


def _cluster_raw_build(seed, device):
    v, f = _soup(1, 3, 1)
    v = v.to(torch.float64)
    if seed != 1:       # every vertex moves inside its own cell (the ones that set the lower corner sit at 0.5 and stay)
        lo = v.min(dim=0)[0] - 0.5 * CLUSTER_S
        q = (v - lo) / CLUSTER_S
        cell = torch.floor(q)
        moved = lo + (cell + 0.1 + 0.8 * (q - cell)) * CLUSTER_S
        assert torch.equal(_cluster_cells(moved), _cluster_cells(v)) and not torch.equal(moved, v)
        v = moved
    nv_in, nf_in = int(v.shape[0]), int(f.shape[0])
    d = dict(vertices=v.contiguous().to(device), faces=f.contiguous().to(device), nv_in=nv_in, nf_in=nf_in,
             out_counts=_sentinel((5,), torch.int64, device), acc_fallback=torch.zeros((1,), dtype=torch.int64, device=device))
    if str(device) != "cpu":
        from quadraturefields_amd import mc_utils
        if "cluster" not in _ONCE:
            v0, _ = _soup(1, 3, 1)
            ov, of = mc_utils.simplify_vertex_clustering(v0.to(torch.float64).to(device), f.to(device), CLUSTER_S, "quadric")
            torch.cuda.synchronize()
            _ONCE["cluster"] = (int(ov.shape[0]), int(of.shape[0]))
        nc, no = _ONCE["cluster"]
        assert 10 < nc < nv_in and no > 10
        nbytes = int(_C().lib().qf_vertex_clustering_workspace_bytes(nv_in, nf_in))
        d.update(nc=nc, no=no, ws_bytes=nbytes, tmp_ws=torch.zeros((nbytes,), dtype=torch.uint8, device=device),
                 out_v=_sentinel((nc, 3), torch.float64, device), out_f=_sentinel((no, 3), torch.int64, device))
    return d


def _cluster_raw_call(i):
    lib = _C().lib()
    v, f, ws, nb = _P(i["vertices"]), _P(i["faces"]), _P(i["tmp_ws"]), i["ws_bytes"]
    _ok(lib.qf_vertex_clustering_count(v, i["nv_in"], f, i["nf_in"], CLUSTER_S, ws, nb, _P(i["out_counts"]), _st()),
        "qf_vertex_clustering_count")
    _ok(lib.qf_vertex_clustering_emit(v, i["nv_in"], f, i["nf_in"], CLUSTER_S, 1, ws, nb, _P(i["out_v"]), i["nc"], _P(i["out_f"]),
                                      i["no"], _P(i["acc_fallback"]), _st()), "qf_vertex_clustering_emit")
    return i["out_counts"], i["out_v"], i["out_f"], i["acc_fallback"]


def _cluster_raw_post(i, outs):
    assert outs[0].tolist()[:4] == [i["nc"], i["no"], 0, 0], (outs[0].tolist(), i["nc"], i["no"])
    return outs


ATLAS_S, ATLAS_LEG, ATLAS_RHO = 128, 8, 6.0


def _atlas_build(seed, device):
    v, f = _soup(seed, 3, 1)
    nf = f.shape[0]
    d = dict(vertices=v.to(torch.float64).contiguous().to(device), faces=f.contiguous().to(device), nf=nf, nv=v.shape[0],
             out_counts=_sentinel((3,), torch.int64, device), out_probe=_sentinel((4,), torch.int64, device),
             out_vertices=_sentinel((3 * nf, 3), torch.float64, device), out_uv=_sentinel((3 * nf, 2), torch.float64, device),
             out_class=_sentinel((nf,), torch.int32, device), out_origin=_sentinel((nf, 2), torch.int32, device),
             out_half=_sentinel((nf,), torch.uint8, device), out_class_counts=_sentinel((ATLAS_LEG + 1,), torch.int64, device),
             out_result=_sentinel((4,), torch.int64, device))
    if str(device) != "cpu":
        nbytes = int(_C().lib().qf_uv_atlas_workspace_bytes(nf))
        d.update(tmp_ws=torch.zeros((nbytes,), dtype=torch.uint8, device=device), ws_bytes=nbytes)
    return d


def _atlas_call(i):
    lib = _C().lib()
    v, f, ws, nb = _P(i["vertices"]), _P(i["faces"]), _P(i["tmp_ws"]), i["ws_bytes"]
    _ok(lib.qf_uv_atlas_measure(v, i["nv"], f, i["nf"], ws, nb, _P(i["out_counts"]), _st()), "qf_uv_atlas_measure")
    _ok(lib.qf_uv_atlas_probe(i["nf"], ATLAS_RHO, ATLAS_LEG, ATLAS_S, ws, nb, _P(i["out_probe"]), _st()), "qf_uv_atlas_probe")
    _ok(lib.qf_uv_atlas_emit(v, i["nv"], f, i["nf"], ATLAS_RHO, ATLAS_LEG, ATLAS_S, ws, nb, _P(i["out_vertices"]), _P(i["out_uv"]),
                             _P(i["out_class"]), _P(i["out_origin"]), _P(i["out_half"]), _P(i["out_class_counts"]),
                             _P(i["out_result"]), _st()), "qf_uv_atlas_emit")
    return tuple(i[k] for k in ("out_counts", "out_probe", "out_vertices", "out_uv", "out_class", "out_origin", "out_half",
                                "out_class_counts", "out_result"))


def _atlas_post(i, outs):
    assert int(outs[-1][3]) == 1, "the atlas does not fit: nothing but the counts was written"
    return outs


TEXEL_H, TEXEL_W = 96, 80


def _texel_build(seed, device):
    from quadraturefields_amd import synthetic
    mesh, _ = synthetic.per_triangle_charts(_mesh(3, 1), 64)
    v = torch.from_numpy(np.asarray(mesh.vertices, dtype=np.float64))
    if seed != 1:
        v = v * 1.05 + 0.01
    nf = int(mesh.faces.shape[0])
    d = dict(vertices=v.contiguous().to(device), faces=torch.from_numpy(np.asarray(mesh.faces, dtype=np.int64)).to(device),
             uv=torch.from_numpy(np.ascontiguousarray(mesh.visual.uv, dtype=np.float64)).to(device), nf=nf, nv=v.shape[0],
             out_map=_sentinel((TEXEL_H, TEXEL_W, 3), torch.float32, device), out_tri_size=_sentinel((nf,), torch.int64, device))
    if str(device) != "cpu":
        nbytes = int(_C().lib().qf_texel_positions_workspace_bytes(nf, TEXEL_H, TEXEL_W))
        d.update(tmp_ws=torch.zeros((nbytes,), dtype=torch.uint8, device=device), ws_bytes=nbytes)
    return d


def _texel_call(i):
    c = _C()
    _ok(c.lib().qf_texel_positions(_P(i["vertices"]), i["nv"], _P(i["faces"]), i["nf"], _P(i["uv"]), TEXEL_H, TEXEL_W,
                                   c.UNTOUCHED_LAST_FACE, _P(i["out_map"]), _P(i["out_tri_size"]), _P(i["tmp_ws"]), i["ws_bytes"],
                                   _st()), "qf_texel_positions")
    return i["out_map"], i["out_tri_size"]


# ====================================================================================================================
# baking, textures, metrics, volumetric frames
# ====================================================================================================================
BAKE_T = 48


def _bake_compact_build(seed, device):
    g = _gen(seed)
    v = (torch.rand(BAKE_T, BAKE_T, 3, generator=g) * 2.4 - 1.2)
    v[torch.rand(BAKE_T, BAKE_T, generator=_gen(1234)) < 0.3] = 0.0          # the same texels are empty in both sets
    cap = BAKE_T * BAKE_T
    d = dict(v=v.contiguous().to(device), out_texel=_sentinel((cap,), torch.int32, device),
             out_pos=_sentinel((cap, 3), torch.float32, device), out_count=_sentinel((1,), torch.int64, device),
             out_mask=_sentinel((BAKE_T, BAKE_T), torch.uint8, device))
    if str(device) != "cpu":
        nbytes = int(_C().lib().qf_bake_compact_workspace_bytes(cap))
        d.update(tmp_ws=torch.zeros((max(nbytes, 8),), dtype=torch.uint8, device=device), ws_bytes=nbytes)
    return d


def _bake_compact_call(i):
    _ok(_C().lib().qf_bake_compact_texels(_P(i["v"]), BAKE_T, 0, BAKE_T, _P(i["out_texel"]), _P(i["out_pos"]), _P(i["out_count"]),
                                          _P(i["out_mask"]), _P(i["tmp_ws"]), i["ws_bytes"], _st()), "qf_bake_compact_texels")
    return i["out_texel"], i["out_pos"], i["out_count"], i["out_mask"]


def _bake_encode_build(seed, device):
    from tests.test_gpu_bake import _planes
    lobes = 2
    g = _gen(seed)
    n = 2000
    feats = torch.randn(n, 3 + 7 * lobes + 1, generator=g) * 3.0
    sigma = torch.rand(n, generator=g) * 400.0
    texel = torch.randperm(BAKE_T * BAKE_T, generator=_gen(4321))[:n].to(torch.int32)
    d = _to(dict(features=feats, sigma=sigma, texel=texel, n_dev=torch.tensor([n - 37], dtype=torch.int64)), device)
    d.update(n=n, lobes=lobes)
    if str(device) != "cpu":
        comp = _planes(BAKE_T, lobes, 7, device)("sigma", 7.5)
        d["comp"] = comp
        d["acc_alpha"], d["acc_diffuse"] = comp.alpha, comp.diffuse
        for l in range(lobes):
            d[f"acc_colors{l}"], d[f"acc_lambdas{l}"] = comp.sg_colors[l], comp.lambdas[l]
    return d


def _bake_encode_call(i):
    comp = i["comp"]
    tex = comp.texture_set()
    _ok(_C().lib().qf_bake_encode_texels(ctypes.byref(tex), _P(i["features"]), i["features"].shape[1], _P(i["sigma"]), _P(i["texel"]),
                                         i["n"], _P(i["n_dev"]), _st()), "qf_bake_encode_texels")
    return tuple(v for k, v in i.items() if k.startswith("acc_"))


def _texture_owner(device):
    key = ("texture", str(device))
    if key not in _MODULES:
        from quadraturefields_amd import synthetic
        from quadraturefields_amd.mesh_utils import MeshIntersection
        from quadraturefields_amd.texture_utils import FeatureCompression
        size = 64
        tex = synthetic.random_textures(size, 2, seed=1)
        comp = FeatureCompression.from_arrays(tex["alpha"], tex["diffuse"], tex["colors"], tex["lambdas"], compression_type="sigma",
                                              lambda_thres=7.5, device=device)
        mesh = _mesh(3, 2)
        mi = MeshIntersection(mesh, simplify_mesh=False, scale=1.0, num_intersections=5)
        uv = torch.from_numpy(synthetic.scaled_uv(mesh, size)).to(device)
        _MODULES[key] = (mi, uv, comp)
    return _MODULES[key]


def _surface_points(seed, mesh, n):
    g = _gen(seed)
    v = torch.from_numpy(np.asarray(mesh.vertices, dtype=np.float32))
    f = torch.from_numpy(np.asarray(mesh.faces, dtype=np.int64))
    tri = torch.randint(0, f.shape[0], (n,), generator=_gen(77))
    w = torch.rand(n, 3, generator=g) + 0.05
    w = w / w.sum(dim=1, keepdim=True)
    return (v[f[tri]] * w[:, :, None]).sum(dim=1).contiguous(), tri, _unit(n, g)


def _shade_points_build(seed, device):
    mi, uv, comp = _texture_owner(device)
    pts, tri, dirs = _surface_points(seed, _mesh(3, 2), N_POINTS)
    return dict(points=pts.to(device), tri=tri.to(device), dirs=dirs.to(device), owner=(mi, uv, comp))


def _shade_points_call(i):
    from quadraturefields_amd import utils
    mi, uv, comp = i["owner"]
    return utils.shade_baked_points(mi, uv, comp, i["points"], i["tri"], i["dirs"])


def _tex_composite_build(w, h, k):
    def build(seed, device):
        mi, uv, comp = _texture_owner(device)
        count, _ = _structure(w, h, k)
        tile_base, total = _tile_scan(count, w, h, k)
        pts, tri, dirs = _surface_points(seed, _mesh(3, 2), total)
        d = _to(dict(xyz_c=pts, dirs_c=dirs, depth_c=torch.rand(total, generator=_gen(seed)) * 3 + 2, tri_c=tri.to(torch.int32),
                     hit_count=count, tile_base=tile_base), device)
        d.update(w=w, h=h, k=k, total=total, owner=(mi, uv, comp))
        return d
    return build


def _tex_composite_call(i):
    from quadraturefields_amd import utils
    mi, uv, comp = i["owner"]
    return utils.shade_composite_baked_frame(mi, uv, comp, i["xyz_c"], i["dirs_c"], _frame_of(i), STEP, utils.early_stop_tau(1e-2))


def _front_build(w, h, k):
    def build(seed, device):
        count, _ = _structure(w, h, k)
        tile_base, total = _tile_scan(count, w, h, k)
        x, d = _points(seed, device)
        reps = -(-total // N_POINTS)
        dd = _to(dict(hit_count=count, tile_base=tile_base, depth_c=torch.rand(total, generator=_gen(seed)) * 3 + 2), device)
        dd.update(xyz_c=x.repeat(reps, 1)[:total].contiguous(), dirs_c=d.repeat(reps, 1)[:total].contiguous(), w=w, h=h, k=k,
                  total=total, module=_module("ngp-fp32", device))
        return dd
    return build


def _front_call(i):
    from quadraturefields_amd import utils
    return utils.render_field_front(i["module"], i["xyz_c"], i["dirs_c"], _frame_of(i), STEP, utils.early_stop_tau(1e-2), None)


def _score_build(seed, device):
    from quadraturefields_amd.metrics import FrameScorer
    g = _gen(seed)
    h, w, f = 24, 40, 2
    d = _to(dict(rgb=torch.rand(h * f, w * f, 3, generator=g), depth=torch.rand(h * f, w * f, generator=g) * 4,
                 pixels=torch.rand(h, w, 3, generator=g)), device)
    d["scorer"] = FrameScorer(h, w, up_sample=f, capacity=4, device=device) if seed == 1 else None
    return d


def _score_call(i):
    s = i["scorer"]
    s.reset()
    slot = s.score(i["rgb"], i["pixels"], i["depth"], images=True, ssim_map=True)
    return (s._table[slot], s._rgb_small, s._depth_small, s._ssim_map) + tuple(s._images)


def _derive_build(seed, device):
    from tests import helpers
    g = _gen(seed)
    index_ray, _ = helpers.packed_segments(960, 25, seed=5)
    n = index_ray.shape[0]
    return _to(dict(rgb=torch.rand(n, 3, generator=g), sigma=torch.rand(n, generator=g) * 40.0,
                    depth=torch.sort(torch.rand(n, generator=g) * 3 + 2)[0], index_ray=index_ray), device) | {"n_rays": 960}


def _derive_call(i):
    from quadraturefields_amd import utils
    rgb, alpha, _, depth, weights = utils.derive_properties(i["rgb"], i["sigma"], i["depth"], STEP, None, i["index_ray"],
                                                            bg_color="white", N=i["n_rays"])
    return rgb, alpha, depth, weights


def _update_d_build(n):
    def build(seed, device):
        g = _gen(seed)
        d = _to(dict(d=torch.randn(n, 3, generator=g) * 1e-2, w=torch.rand(n, generator=g),
                     index_tri=torch.randint(0, N_TRI, (n,), generator=_gen(99)),
                     acc_cache=torch.zeros(N_TRI, 4), acc_skipped=torch.zeros(1, dtype=torch.int32)), device)
        d["n"] = n
        return d
    return build


def _update_d_call(i):
    _ok(_C().lib().qf_mesh_update_d(_P(i["d"]), _P(i["w"]), _P(i["index_tri"]), i["n"], N_TRI, _P(i["acc_cache"]),
                                    _P(i["acc_skipped"]), _st()), "qf_mesh_update_d")
    return i["acc_cache"], i["acc_skipped"]


def _volumetric_build(seed, device):
    from quadraturefields_amd.estimators import OccGridEstimator
    from tests.test_gpu_occgrid import _grid
    key = ("estimator", str(device))
    if key not in _MODULES:
        est = OccGridEstimator(roi_aabb=[-1.5] * 3 + [1.5] * 3, resolution=32, levels=1).to(device)
        est.binaries.copy_(torch.from_numpy(_grid(32, seed=32))[None].to(device))
        _MODULES[key] = est
    o, d = _random_rays(seed, 960, device)
    return dict(origins=o, viewdirs=d, estimator=_MODULES[key], module=_module("ngp-fp32", device))


def _volumetric_call(i):
    from quadraturefields_amd import utils
    from quadraturefields_amd.utils import Rays
    rgb, opacity, depth, total, _ = utils.render_image_with_occgrid_test(
        256, i["module"], i["estimator"], Rays(origins=i["origins"], viewdirs=i["viewdirs"]), render_step_size=0.02,
        early_stop_eps=1e-2)
    return rgb, opacity, depth, torch.tensor([total])


# The renderer above waits for the stream once per round, so only round 1's count and write sit behind the delay and the
# accumulate never does.  On the C ABI, without a host wait: a count / scan / write round, and an accumulate on
# synthetic runs.
VOL_RAYS, VOL_STEP = 960, 0.02


def _round_build(seed, device):
    est = None
    if str(device) != "cpu":
        est = _volumetric_build(seed, device)["estimator"]
    o, d = _random_rays(seed, VOL_RAYS, device)
    n = VOL_RAYS
    alive = (torch.rand(n, generator=_gen(31)) < 0.8).to(torch.uint8)
    state = torch.zeros(8, dtype=torch.int64)
    state[0] = n // 8                                     # alive rays entering the round: quota = 8 samples a ray
    i = _to(dict(origins=o, viewdirs=d, near=torch.rand(n, generator=_gen(seed)) * 0.5, alive=alive, state=state,
                 tmp_count=torch.zeros(n, dtype=torch.int32), tmp_csum=torch.zeros(n, dtype=torch.int64),
                 out_term=_sentinel((n,), torch.float32, "cpu"), out_ts=_sentinel((n,), torch.float32, "cpu"),
                 out_te=_sentinel((n,), torch.float32, "cpu"), out_ridx=_sentinel((n,), torch.int64, "cpu"),
                 out_xyz=_sentinel((n, 3), torch.float32, "cpu"), out_dirs=_sentinel((n, 3), torch.float32, "cpu")), device)
    i["estimator"] = est
    return i


def _round_call(i):
    lib, est, n = _C().lib(), i["estimator"], VOL_RAYS
    aabb, res = est._host_geometry()
    march = (aabb, res, _P(est.binaries[0]), _P(i["origins"]), _P(i["viewdirs"]), _P(i["near"]), _P(i["alive"]), n, 0.0, 1e10,
             VOL_STEP, _P(i["state"]))
    _ok(lib.qf_grid_march_round_count(*march, 0, _P(i["tmp_count"]), _P(i["out_term"]), _st()), "qf_grid_march_round_count")
    torch.cumsum(i["tmp_count"], dim=0, out=i["tmp_csum"])
    _ok(lib.qf_grid_march_round_write(*march, 0, _P(i["tmp_count"]), _P(i["tmp_csum"]), n, _P(i["out_ts"]), _P(i["out_te"]),
                                      _P(i["out_ridx"]), _P(i["out_xyz"]), _P(i["out_dirs"]), _st()), "qf_grid_march_round_write")
    return tuple(i[k] for k in ("tmp_count", "tmp_csum", "out_term", "out_ts", "out_te", "out_ridx", "out_xyz", "out_dirs", "state"))


def _round_post(i, outs):
    assert int(outs[8][3]) > 200 and int(outs[8][4]) == 8, outs[8].tolist()      # samples marched; the round's quota
    return outs


def _accumulate_build(seed, device):
    n, quota = VOL_RAYS, 4
    gs, g = _gen(41), _gen(seed)
    count = torch.randint(0, quota + 1, (n,), generator=gs, dtype=torch.int32)
    count[::3] = quota
    alive = (torch.rand(n, generator=gs) < 0.85).to(torch.uint8)
    count = count * alive.to(torch.int32)                  # the count launch leaves 0 for dead rays
    csum = torch.cumsum(count.to(torch.int64), 0)
    total = int(csum[-1])
    ts = torch.rand(total, generator=g) * 3.0 + 2.0
    state = torch.zeros(8, dtype=torch.int64)
    state[0], state[4] = n // quota, quota
    i = _to(dict(t_starts=ts, t_ends=ts + VOL_STEP * (1.0 + torch.rand(total, generator=g)), sigmas=torch.rand(total, generator=g) * 60.0,
                 rgbs=torch.rand(total, 3, generator=g), count=count, csum=csum, term=torch.rand(n, generator=g) * 3.0 + 2.0,
                 state=state, near=torch.rand(n, generator=g), alive=alive, opacity=torch.rand(n, generator=g) * 0.5,
                 acc_rgb=torch.zeros(n, 3), acc_depth=torch.zeros(n)), device)
    i["total"] = total
    return i


def _accumulate_call(i):
    _ok(_C().lib().qf_volumetric_accumulate(
        _P(i["t_starts"]), _P(i["t_ends"]), _P(i["sigmas"]), _P(i["rgbs"]), _P(i["count"]), _P(i["csum"]), _P(i["term"]), VOL_RAYS,
        i["total"], 1e-2, 1e-2, _P(i["state"]), 0, _P(i["acc_rgb"]), _P(i["opacity"]), _P(i["acc_depth"]), _P(i["near"]),
        _P(i["alive"]), _st()), "qf_volumetric_accumulate")
    return i["acc_rgb"], i["opacity"], i["acc_depth"], i["near"], i["alive"], i["state"]


# ====================================================================================================================
# bound frames (one host call each), through the package's own callers
# ====================================================================================================================
def _frame_scene(device, k):
    key = ("frame", str(device), k)
    if key not in _MODULES:
        from quadraturefields_amd.mesh_utils import MeshIntersection
        mi = MeshIntersection(_mesh(4, 3), simplify_mesh=False, scale=1.0, num_intersections=k)
        _MODULES[key] = mi
    return _MODULES[key]


def _bound_build(kind, w, h, k=25):
    def build(seed, device):
        from quadraturefields_amd.pruning import MeshPruner
        from quadraturefields_amd.render import FrameRenderer
        cam, o, d = _camera_rays(seed, w, h, device)
        mi = _frame_scene(device, k)
        i = dict(rays_o=o, rays_d=d, cam=cam, mi=mi, kind=kind, k=k)
        if kind == "baked":
            _, uv, comp = _texture_owner(device)
            from quadraturefields_amd import synthetic
            i.update(fr=FrameRenderer(mi, None), comp=comp,
                     uv=torch.from_numpy(synthetic.scaled_uv(_mesh(4, 3), 64)).to(device))
        elif kind == "prune" and seed == 1:
            i["pruner"] = MeshPruner(mi, _module("ngp-fp32", device))
            i["acc_tri_weight"] = i["pruner"].triangle_weights
        elif kind == "prune":
            i["pruner"] = None
            i["acc_tri_weight"] = torch.zeros((int(mi.mesh.faces.shape[0]),), dtype=torch.float32, device=device)
        else:
            i["fr"] = FrameRenderer(mi, _module("ngp-fp32", device))
        return i
    return build


def _bound_call(i):
    ri = i["mi"].rayintersector
    ri._raster_backoff = 0
    kind, o, d, cam = i["kind"], i["rays_o"], i["rays_d"], i["cam"]
    assert ri.fused_frame_ready(cam, i["k"]), "the frame is not on the one-call route"
    if kind == "render":
        rgb, alpha, depth, frame = i["fr"].render_async(o, d, cam)
        outs = (rgb, alpha, depth, frame.hit_count)
    elif kind == "front":
        rgb, alpha, depth, frame = i["fr"].render_async(o, d, cam, early_stop_eps=1e-2)
        outs = (rgb, alpha, depth, frame.shaded_count, frame.evaluated_count)
    elif kind == "baked":
        rgb, alpha, depth, frame = i["fr"].render_baked_async(o, d, i["uv"], i["comp"], cam, early_stop_eps=1e-2)
        outs = (rgb, alpha, depth, frame.shaded_count)
    else:
        p = i["pruner"]
        p.n_views = 0
        p._counts.zero_()
        frame = p.add_view(o, d, cam)
        outs = (i["acc_tri_weight"], p._counts[0], frame.hit_count)
    assert ri.last_route in ("frame", "frame+cull"), ri.last_route
    return outs


# ====================================================================================================================
# the registry
# ====================================================================================================================
def _cases():
    c = []
    add = lambda *a, **k: c.append(Case(*a, **k))          # noqa: E731
    for w, h in FRAMES:
        add(f"frame_offsets-tiles-{w}x{h}", _offsets_build(w, h, 5, True, True), _frame_offsets_call, varies=("hit_count", "words"),
            post=_host_block([0, 1, 3]), entry_points=("qf_frame_offsets",))
        add(f"tile_offsets-{w}x{h}", _offsets_build(w, h, 25, True, True), _tile_offsets_call, varies=("hit_count", "words"),
            post=_host_block([0, 1, 3]), entry_points=("qf_tile_offsets",))
        add(f"coherent_layout-{w}x{h}", _layout_build(w, h, 5), _coherent_layout_call,
            varies=("hit_count", "ray_offset", "index_ray"), entry_points=("qf_coherent_layout",))
        add(f"split_layout-{w}x{h}", _layout_build(w, h, 5), _split_layout_call,
            varies=("hit_count", "ray_offset", "index_ray"), entry_points=("qf_split_layout",))
        add(f"pack_samples-{w}x{h}", _pack_build(w, h, 5), _pack_samples_call, entry_points=("qf_pack_samples",))
        add(f"pack_tiles-{w}x{h}", _pack_build(w, h, 25), _pack_tiles_call, entry_points=("qf_pack_tiles",))
        add(f"composite_tiles-{w}x{h}", _composite_build(w, h, 25), _composite_call, entry_points=("qf_composite_tiles",))
    add("frame_offsets-rays", _offsets_build(40, 24, 25, False, False), _frame_offsets_call, varies=("hit_count", "words"),
        entry_points=("qf_frame_offsets",))
    add("composite_tiles_trimax", _composite_build(40, 24, 5), _trimax_call, entry_points=("qf_composite_tiles_trimax",))
    add("resort_samples", _resort_build, _resort_call, entry_points=("qf_resort_samples",))
    add("filter_hits", _filter_build, _filter_call, post=_filter_post, entry_points=("qf_filter_hits",))
    # the intersector
    gpu = dict(cpu_buildable=False)
    add("raster_intersect-cull", _raster_build(4, 3, 40, 24, 25), _raster_call("plain", cull=1), entry_points=("qf_raster_intersect",),
        **gpu)
    add("raster_intersect-9x1", _raster_build(3, 1, 9, 1, 25), _raster_call("plain"), entry_points=("qf_raster_intersect",), **gpu)
    add("raster_intersect_wide-cull", _raster_build(4, 3, 40, 24, 5, wide=7), _raster_call("wide", cull=1), post=_sorted_lists,
        entry_points=("qf_raster_intersect_wide",), **gpu)
    add("raster_intersect_slabs", _raster_build(4, 3, 40, 24, 5, wide=24), _raster_call("slabs", slabs=4), post=_sorted_lists,
        entry_points=("qf_raster_intersect_slabs",), **gpu)
    add("raster_intersect_tiles", _raster_build(3, 2, 40, 24, 5, tiles=True), _raster_call("tiles"), post=_sorted_bins,
        entry_points=("qf_raster_intersect_tiles",), **gpu)
    add("bvh_repair_overflow", _repair_build, _repair_call, post=_repair_post, entry_points=("qf_bvh_repair_overflow",), **gpu)
    add("bvh_intersect", _bvh_intersect_build, _bvh_intersect_call, entry_points=("qf_bvh_intersect",), **gpu)
    add("pack_tiles_bins", _pack_bins_build, _pack_bins_call, entry_points=("qf_pack_tiles_bins",), **gpu)
    add("bvh_copy_visible_chunks", _visible_build, _visible_call, host_wait=True, entry_points=("qf_bvh_copy_visible_chunks",), **gpu)
    add("bvh_create_device", _bvh_build_build, _bvh_build_call(False), host_wait=True, entry_points=("qf_bvh_create_device",), **gpu)
    add("bvh_create_device_timed", _bvh_build_build, _bvh_build_call(True), host_wait=True,
        entry_points=("qf_bvh_create_device_timed",), **gpu)
    add("bvh_refit_device", _bvh_refit_build(False), _bvh_refit_call, entry_points=("qf_bvh_refit_device",), **gpu)
    add("bvh_refit-host", _bvh_refit_build(True), _bvh_refit_call, host_wait=True, entry_points=("qf_bvh_refit",), **gpu)
    # fields
    add("field_forward", _field_build("ngp-fp32"), _field_call, entry_points=("qf_field_forward",), **gpu)
    add("field_forward-sg", _field_build("sg-fp32"), _field_call, entry_points=("qf_field_forward",), **gpu)
    add("field_forward-features", _field_build("sg-fp32"), _features_call, entry_points=("qf_field_forward",), **gpu)
    add("field_forward_bf16", _field_build("ngp-bf16"), _field_call, entry_points=("qf_field_forward_bf16",), **gpu)
    add("field_forward_f16", _field_build("sg-fp16"), _field_call, entry_points=("qf_field_forward_f16",), **gpu)
    add("deform_field_forward", _field_build("deform-fp32"), _field_call, entry_points=("qf_deform_field_forward",), **gpu)
    add("deform_field_forward_f16", _field_build("deform-fp16"), _field_call, entry_points=("qf_deform_field_forward_f16",), **gpu)
    add("grid_mlp_forward", _field_build("ngp-fp32"), _grid_mlp_call, entry_points=("qf_grid_mlp_forward",), **gpu)
    add("field_grid_extract", _extract_build("extract-fp32"), _extract_call, entry_points=("qf_field_grid_extract",), **gpu)
    add("field_grid_extract_f16", _extract_build("extract-fp16"), _extract_call, entry_points=("qf_field_grid_extract_f16",), **gpu)
    add("adam_step", _adam_build, _adam_call, entry_points=("qf_adam_step",))
    # training
    add("ngp_mlp_backward", _ngp_bwd_build, _ngp_bwd_call, compare=_ngp_bwd_compare, varies=("sel",),
        entry_points=("qf_ngp_mlp_backward",), **gpu)
    add("sg_mlp_backward", _sg_bwd_build, _sg_bwd_call, compare=_sg_bwd_compare, varies=("sel",),
        entry_points=("qf_sg_mlp_backward",), **gpu)
    add("deform_mlp_backward", _deform_bwd_build, _deform_bwd_call, compare=_deform_bwd_compare,
        entry_points=("qf_deform_mlp_backward",), **gpu)
    add("field_quadrature_loss", _field_loss_build, _field_loss_call, compare=_field_loss_compare,
        entry_points=("qf_field_quadrature_loss",), **gpu)
    add("distortion_loss", _distortion_build, _distortion_call, entry_points=("qf_distortion_loss",))
    add("grid_encode_backward", _grid_bwd_build("small", N_POINTS), _grid_bwd_call("plain"), compare=_grid_bwd_compare,
        entry_points=("qf_grid_encode_backward",), **gpu)
    add("grid_encode_backward_ws-small-batch", _grid_bwd_build("small", N_POINTS), _grid_bwd_call("ws"), compare=_grid_bwd_compare,
        entry_points=("qf_grid_encode_backward_ws",), **gpu)
    add("grid_encode_backward_ws-lds-walk", _grid_bwd_build("small", (1 << 15) + 8193), _grid_bwd_call("ws"),
        compare=_grid_bwd_compare, entry_points=("qf_grid_encode_backward_ws",), **gpu)
    add("grid_encode_backward_ws-walk-and-atomics", _grid_bwd_build("edges", (1 << 15) + 8193), _grid_bwd_call("ws"),
        compare=_grid_bwd_compare, entry_points=("qf_grid_encode_backward_ws",), **gpu)
    add("grid_encode_double_backward", _grid_bwd_build("small", N_POINTS, True), _grid_bwd_call("double"), compare=_grid_bwd_compare,
        entry_points=("qf_grid_encode_double_backward",), **gpu)
    add("grid_encode_double_backward-lds-walk", _grid_bwd_build("small", (1 << 15) + 8193, True), _grid_bwd_call("double"),
        compare=_grid_bwd_compare, entry_points=("qf_grid_encode_double_backward",), **gpu)
    # geometry
    add("marching_cubes", _mc_raw_build, _mc_raw_call, post=_mc_raw_post,
        entry_points=("qf_marching_cubes_count", "qf_marching_cubes_emit"))
    add("vertex_clustering", _cluster_raw_build, _cluster_raw_call, post=_cluster_raw_post,
        entry_points=("qf_vertex_clustering_count", "qf_vertex_clustering_emit"))
    # the wrappers wait for their counts between count and emit: they show the wrapper's own plumbing, not the emit
    add("marching_cubes-wrapper", _mc_build, _mc_call, host_wait=True)
    add("vertex_clustering-wrapper", _cluster_build, _cluster_call, host_wait=True)
    add("uv_atlas", _atlas_build, _atlas_call, post=_atlas_post,
        entry_points=("qf_uv_atlas_measure", "qf_uv_atlas_probe", "qf_uv_atlas_emit"))
    add("texel_positions", _texel_build, _texel_call, entry_points=("qf_texel_positions",))
    # baking, textures, metrics, volumetric frames
    add("bake_compact_texels", _bake_compact_build, _bake_compact_call, entry_points=("qf_bake_compact_texels",))
    add("bake_encode_texels", _bake_encode_build, _bake_encode_call, entry_points=("qf_bake_encode_texels",))
    add("texture_shade_points", _shade_points_build, _shade_points_call, entry_points=("qf_texture_shade_points",), **gpu)
    add("texture_composite_tiles", _tex_composite_build(40, 24, 5), _tex_composite_call,
        entry_points=("qf_texture_composite_tiles",), **gpu)
    add("front_select_finish", _front_build(40, 24, 25), _front_call, entry_points=("qf_front_select", "qf_front_finish"), **gpu)
    add("frame_score", _score_build, _score_call, entry_points=("qf_frame_score", "qf_frame_images_u8"), **gpu)
    add("derive_properties", _derive_build, _derive_call, entry_points=("qf_derive_properties",))
    add("mesh_update_d", _update_d_build(N_POINTS), _update_d_call, tol=(1e-5, 1e-6), entry_points=("qf_mesh_update_d",))
    add("grid_march_round", _round_build, _round_call, post=_round_post,
        entry_points=("qf_grid_march_round_count", "qf_grid_march_round_write"))
    add("volumetric_accumulate", _accumulate_build, _accumulate_call, entry_points=("qf_volumetric_accumulate",))
    # the renderer waits once per round: only its first count and write are behind the delay
    add("volumetric_rounds-wrapper", _volumetric_build, _volumetric_call, host_wait=True, **gpu)
    # bound frames
    for kind, ep in (("render", "qf_frame_render"), ("front", "qf_frame_render_front"), ("baked", "qf_frame_render_baked"),
                     ("prune", "qf_frame_prune")):
        add(f"frame_{kind}-40x24", _bound_build(kind, 40, 24), _bound_call, entry_points=(ep,), **gpu)
    add("frame_render-9x1", _bound_build("render", 9, 1), _bound_call, entry_points=("qf_frame_render",), **gpu)
    return c


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# Entry points that take a stream and have no case: the body is argument checks plus exactly ONE launch on the caller's
# stream (test_every_stream_entry_point_is_accounted_for reads the sources and holds each entry to that), so there is no
# second launch, fill or copy that could go elsewhere, and the one launch's stream argument is in plain sight.
SINGLE_LAUNCH = {
    "qf_grid_encode": "one grid_encode launch",
    "qf_sg_features_to_rgb": "one elementwise launch",
    "qf_sg_features_to_rgb_backward": "one elementwise launch",
    "qf_apply_deformation": "one elementwise launch",
    "qf_mark_pack_boundaries": "one elementwise launch",
    "qf_exponential_integration": "one launch, a thread per segment",
    "qf_sum_reduce": "one launch, a thread per segment",
    "qf_derive_properties_backward": "one launch, a thread per ray",
    "qf_pack_info": "one launch, a thread per ray",
    "qf_exclusive_scan": "one launch, a thread per ray",
    "qf_accumulate_along_rays": "one launch, a thread per ray",
    "qf_render_from_density": "one launch, a thread per ray",
    "qf_grid_march_count": "one launch, a thread per ray",
    "qf_grid_march_write": "one launch, a thread per ray",
    "qf_mark_visited_cells": "one elementwise launch",
    "qf_generate_rays": "one launch, a thread per pixel",
    "qf_scatter_max": "one launch of atomic maxima",
    "qf_tile_totals": "one launch, a wave per tile",
    "qf_row_sample_counts": "one launch, a workgroup per row",
    "qf_deform_resort_tiles": "one launch, a wave per tile",
    "qf_resort_by_depth": "one launch, a thread per sample",
    "qf_texel_records_pack": "one launch, a thread per face",
    "qf_texel_indices_packed": "one launch, a thread per sample",
    "qf_texture_fetch": "one launch, a thread per sample",
    "qf_texture_pack": "one launch, a thread per texel",
    "qf_texture_shade_packed": "one launch, a thread per sample",
}

# What the issue names as mandatory: none of these may sit in SINGLE_LAUNCH.
MANDATORY = """
qf_frame_offsets qf_tile_offsets qf_raster_intersect qf_raster_intersect_wide qf_raster_intersect_slabs qf_raster_intersect_tiles
qf_bvh_repair_overflow qf_bvh_intersect qf_filter_hits qf_pack_samples qf_pack_tiles qf_pack_tiles_bins qf_resort_samples
qf_split_layout qf_coherent_layout qf_distortion_loss qf_field_quadrature_loss qf_ngp_mlp_backward qf_sg_mlp_backward
qf_deform_mlp_backward qf_grid_encode_backward_ws qf_grid_encode_double_backward qf_texel_positions qf_uv_atlas_measure
qf_uv_atlas_probe qf_uv_atlas_emit qf_vertex_clustering_count qf_vertex_clustering_emit qf_marching_cubes_count
qf_marching_cubes_emit qf_field_grid_extract qf_bake_compact_texels qf_bake_encode_texels qf_frame_score
qf_grid_march_round_count qf_grid_march_round_write qf_volumetric_accumulate qf_bvh_create_device qf_bvh_refit_device qf_bvh_refit
qf_frame_render qf_frame_prune qf_frame_render_baked qf_frame_render_front qf_field_forward qf_field_forward_bf16
qf_field_forward_f16 qf_deform_field_forward qf_deform_field_forward_f16 qf_composite_tiles qf_composite_tiles_trimax
qf_texture_composite_tiles qf_adam_step
""".split()


# ====================================================================================================================
# without a GPU: completeness, the sets' safety conditions, the harness's host-side parts
# ====================================================================================================================
def _prototypes():
    """{name: parameter text} of every function include/qf_hip.h declares."""
    text = open(os.path.join(ROOT, "include", "qf_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    out = {}
    for stmt in text.split(";"):
        m = re.search(r"\b(qf_\w+)\s*\(([^()]*)\)\s*$", stmt.strip(), flags=re.S)
        if m and "typedef" not in stmt and "#define" not in stmt.split(m.group(1))[0].splitlines()[-1]:
            out[m.group(1)] = m.group(2)
    return out


def _definition(name):
    """The body of the ``extern "C"`` definition of ``name`` in csrc/."""
    for path in sorted(glob.glob(os.path.join(ROOT, "quadraturefields_amd", "csrc", "*.*"))):
        src = open(path).read()
        m = re.search(r'extern "C"[^;{}()]*\b' + name + r"\s*\(", src)
        if not m:
            continue
        k, depth = m.end(), 1
        while depth:
            depth += {"(": 1, ")": -1}.get(src[k], 0)
            k += 1
        k = src.index("{", k)
        start, depth = k, 0
        while True:
            depth += {"{": 1, "}": -1}.get(src[k], 0)
            k += 1
            if depth == 0:
                return src[start:k]
    raise AssertionError(f"{name}: no extern \"C\" definition under csrc/")


_LAUNCH = re.compile(r"hipLaunchKernelGGL|<<<|QF_SIMPLE_LAUNCH")
_OTHER_WORK = re.compile(r"hipMem(set|cpy)\w*|hipStreamSynchronize|hipDeviceSynchronize|hipMalloc|hipFree")
_PLAIN_CALLS = {"if", "for", "while", "return", "sizeof", "dim3", "switch", "static_cast", "reinterpret_cast", "const_cast",
                "qf_stream", "qf_grid_1d", "qf_div_up", "fill_grid_args", "fill_march_args", "fill_tex_args", "QF_LAUNCH_CHECK",
                "QF_SIMPLE_LAUNCH", "hipLaunchKernelGGL", "int", "unsigned", "float", "int64_t", "int32_t", "size_t", "defined"}


def test_every_stream_entry_point_is_accounted_for():
    protos = _prototypes()
    assert len(protos) > 100 and "qf_abi_version" in protos
    streamed = sorted(n for n, params in protos.items() if re.search(r"void\s*\*\s*stream\b", params))
    assert len(streamed) >= 85, len(streamed)
    # qf_bvh_refit takes no stream (it waits for the whole device) but re-uploads: the issue lists it
    covered = {ep for c in CASES for ep in c.entry_points}
    assert "qf_bvh_refit" in covered
    assert set(MANDATORY) <= set(protos), sorted(set(MANDATORY) - set(protos))
    assert not set(MANDATORY) & set(SINGLE_LAUNCH), sorted(set(MANDATORY) & set(SINGLE_LAUNCH))
    assert set(MANDATORY) <= covered, sorted(set(MANDATORY) - covered)
    assert covered <= set(protos), sorted(covered - set(protos))
    both = covered & set(SINGLE_LAUNCH)
    assert not both, f"in the registry AND in SINGLE_LAUNCH: {sorted(both)}"
    missing = [n for n in streamed if n not in covered and n not in SINGLE_LAUNCH]
    assert not missing, (f"{missing}: exported with a stream parameter but neither in the registry of tests/test_gpu_streams.py "
                         "nor in SINGLE_LAUNCH -- decide which list each belongs in")
    stale = sorted(set(SINGLE_LAUNCH) - set(streamed))
    assert not stale, f"SINGLE_LAUNCH names {stale}, which include/qf_hip.h does not export with a stream"
    for name, reason in SINGLE_LAUNCH.items():
        assert reason.strip(), name
        body = _definition(name)
        assert len(_LAUNCH.findall(body)) == 1, f"{name}: {len(_LAUNCH.findall(body))} launches in its body, SINGLE_LAUNCH allows one"
        assert not _OTHER_WORK.search(body), f"{name}: a fill, copy, allocation or wait besides its launch"
        assert "QF_SIMPLE_LAUNCH" in body or re.search(r"hipLaunchKernelGGL\([^;]*qf_stream\(stream\)", body, flags=re.S), \
            f"{name}: the launch does not take the caller's stream"
        calls = set(re.findall(r"\b([A-Za-z_]\w*)\s*\(", body)) - _PLAIN_CALLS
        calls = {c for c in calls if not c.endswith("_kernel")}
        assert not calls, f"{name}: calls {sorted(calls)} -- a helper may launch; give the entry point a case instead"


def test_the_simple_launch_macro_takes_the_callers_stream():
    src = open(os.path.join(ROOT, "quadraturefields_amd", "csrc", "qf_common.h")).read()
    m = re.search(r"#define QF_SIMPLE_LAUNCH\(kernel, count, \.\.\.\)(.*?)\n\n", src, flags=re.S)
    assert m and "qf_stream(stream)" in m.group(1)


@pytest.mark.parametrize("name", [c.name for c in CASES if c.cpu_buildable])
def test_stale_and_fresh_sets_differ_in_value_arrays_only(name):
    """The safety conditions of the two input sets, checked where the builders need no device: same shapes, every
    structural (integer) array identical unless the case declares it wholly structural, all values finite."""
    case = BY_NAME[name]
    sh.check_sets(case, case.build(1, "cpu"), case.build(2, "cpu"))


def test_wholly_structural_stale_sets_keep_every_mixture_in_bounds():
    """qf_frame_offsets / qf_tile_offsets / the layouts: the stale counts are the fresh ones permuted inside their 8x8
    tile, so tile totals, tile bases and the grand total agree, and the largest index any mixture of the two sets can form
    -- an offset of one set plus a count of the other -- stays below total + K, the size of the outputs."""
    for w, h in FRAMES:
        for k in (5, 25):
            a = _counts(7300 + w * h + k, w, h, k)
            b = _swapped_in_tiles(a, w, h, 2)
            assert not torch.equal(a, b) or w * h < 16
            (base_a, total_a), (base_b, total_b) = _tile_scan(a, w, h, k), _tile_scan(b, w, h, k)
            assert torch.equal(base_a, base_b) and total_a == total_b
            off_a = torch.cumsum(a.long(), 0) - a.long()
            off_b = torch.cumsum(b.long(), 0) - b.long()
            assert int(torch.maximum(off_a, off_b).max()) + k <= total_a + k
            assert int((off_a + b.long()).max()) <= total_a + k and int((off_b + a.long()).max()) <= total_a + k


def test_delay_rule_and_comparison_host_side():
    assert sh.delay_ms_for(0.0) == sh.MIN_DELAY_MS and sh.delay_ms_for(5.0) == 50.0 and sh.delay_ms_for(100.0) == sh.MAX_DELAY_MS
    case = Case("t", None, None)
    a = torch.tensor([1.0, float("nan"), -0.0])
    assert sh.same_bits(a, a.clone()) and not sh.same_bits(a, torch.tensor([1.0, float("nan"), 0.0]))
    assert sh.outputs_match(case, (a,), (a.clone(),)) is None
    assert "output 0" in sh.outputs_match(case, (a,), (a + 1,))
    assert sh.outputs_match(case, (a,), (a[:2],)) is not None                # another shape never matches
    tol = Case("t", None, None, tol=(0.0, 1e-3))
    assert sh.outputs_match(tol, (torch.ones(3),), (torch.ones(3) + 5e-4,)) is None
    assert sh.outputs_match(tol, (torch.ones(3),), (torch.ones(3) + 5e-3,)) is not None
    with pytest.raises(AssertionError, match="structural input"):
        sh.check_sets(case, {"idx": torch.tensor([1, 2]), "x": torch.ones(2)}, {"idx": torch.tensor([2, 1]), "x": torch.zeros(2)})
    with pytest.raises(AssertionError, match="not finite"):
        sh.check_sets(case, {"x": torch.tensor([float("inf")])}, {"x": torch.zeros(1)})
    with pytest.raises(AssertionError, match="are the same"):
        sh.check_sets(case, {"x": torch.ones(2)}, {"x": torch.ones(2)})


# ====================================================================================================================
# on the GPU
# ====================================================================================================================
def _two_step(wrong):
    """A pure-torch two-step "entry point": tmp = a * 2; out = tmp + b -- with ``wrong`` the second step is issued on the
    default stream, whatever stream the caller made current."""
    def build(seed, device):
        g = _gen(seed)
        return _to(dict(a=torch.randn(N_POINTS, generator=g), b=torch.randn(N_POINTS, generator=g), tmp_mid=torch.zeros(N_POINTS),
                        out_y=torch.zeros(N_POINTS)), device)

    def call(i):
        torch.mul(i["a"], 2.0, out=i["tmp_mid"])
        if wrong:
            with torch.cuda.stream(torch.cuda.default_stream()):
                torch.add(i["tmp_mid"], i["b"], out=i["out_y"])
        else:
            torch.add(i["tmp_mid"], i["b"], out=i["out_y"])
        return (i["out_y"],)
    return Case("two-step-" + ("wrong" if wrong else "right"), build, call)


@pytest.mark.gpu
def test_the_harness_detects_a_launch_on_the_wrong_stream(device):
    """The delay bites on this machine: the same function passes with both steps on the caller's stream and is reported
    as a mismatch (with the stale inputs' result) when its second step goes to the default stream."""
    sh.run_case(_two_step(False), device)
    with pytest.raises(sh.StreamMismatch, match="STALE"):
        sh.run_case(_two_step(True), device)
    print(f"delay calibration: {sh.cycles_per_ms():.0f} sleep cycles per ms")


@pytest.mark.gpu
def test_a_delay_that_has_run_out_fails_the_case(device, monkeypatch):
    """``busy`` is a condition: with no delay at all the side stream is idle when the call returns, and the case fails as
    "delay too short" although its result is right."""
    monkeypatch.setattr(sh, "delay", lambda ms: None)
    case = _two_step(False)
    slow = Case(case.name, case.build, lambda i: (case.call(i), torch.cuda.current_stream().synchronize())[0])
    with pytest.raises(sh.DelayTooShort):
        sh.run_case(slow, device)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_entry_point_runs_entirely_on_the_callers_stream(device, lib, name):
    issue_ms, delay_ms = sh.run_case(BY_NAME[name], device)
    print(f"STREAM_CASE {name}: issue {issue_ms:.3f} ms, delay {delay_ms:.0f} ms")
