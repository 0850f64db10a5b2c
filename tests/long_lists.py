"""Scenes, brute-force truth and plain numpy references for hit lists of 33 to 64 entries (tests/test_gpu_long_lists.py
runs them on the device, tests/test_long_lists_host.py checks on the CPU that they are what they claim to be).

Scenes: 36 concentric shells of 80 triangles each (``synthetic.shell_mesh(36, 1)``: 2 880 triangles, a ray through the
centre crosses 72 times), seen by one orbit camera as a 48 x 40 frame (tile-aligned) and a 45 x 37 frame (ragged right
and bottom tiles), and by a plain batch of 2 000 (+ 77) rays from the radius-3 sphere aimed at points of uniformly random
radius in [0, 1.3].  A second mesh, 48 shells between radius 1.0 and 1.2, has a mean depth above 32: the only way to the
front-to-back instantiation of the general traversal at K > 32 (``ordered`` below).

Truth: ``oracle.meshpath.BruteForceIntersector(...).hits(o, d, 128)``, every hit of every ray, computed once per (mesh,
rays, rule) and frozen.

References, all in numpy: the re-origin rule over sorted lists (fp32, as the device applies it), the keep masks of
``qf_bvh_repair_overflow``, the six sample arrays of ``qf_pack_samples`` (``sampling_raytrace_numpy``'s arithmetic: positions
o + t d in float64 rounded once, depth |p - o| in float64, directions d / (|d| + 1e-7) in float32), the coherent tile
order of ``qf_pack_tiles`` written slot by slot, and ``np.lexsort((depth, ray))`` for ``qf_resort_samples``.
"""
import functools
from types import SimpleNamespace

import numpy as np

from oracle import meshpath as om

ALL = 128                              # the brute force's list length: every hit of every ray (at most 96)
RULE = 0.05                            # the re-origin distance of the rule-on cases: about two shell spacings
MESH = (36, 1, 0.3)                    # (shells, subdivisions, r_min): the long-list scene
DENSE = (48, 1, 1.0)                   # mean depth > 32: front-to-back traversal for every K <= 64
FRAMES = {"aligned": (48, 40), "ragged": (45, 37)}
BATCH, BATCH_TAIL = 2000, 77           # 2 077 rays: the last workgroup of the 128-ray kernels is partial
BIG = np.uint64(0xFFFFFFFFFFFFFFFF)


# ------------------------------------------------------------------------------------------------ scenes
@functools.lru_cache(maxsize=None)
def mesh(key=MESH):
    from quadraturefields_amd import synthetic
    shells, subdiv, r_min = key
    return synthetic.shell_mesh(n_shells=shells, subdivisions=subdiv, r_min=r_min)


@functools.lru_cache(maxsize=None)
def vertices(key=MESH):
    v = np.ascontiguousarray(mesh(key).vertices, dtype=np.float32)
    v.setflags(write=False)
    return v


def depth_complexity(key=MESH):
    """2 area(mesh) / area(bounding box) in fp64: ``qf_bvh_depth_complexity`` restated."""
    v = vertices(key).astype(np.float64)
    c = v[mesh(key).faces]
    area = 0.5 * np.linalg.norm(np.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]), axis=1).sum()
    e = v.max(axis=0) - v.min(axis=0)
    return 2.0 * area / (2.0 * (e[0] * e[1] + e[1] * e[2] + e[2] * e[0]))


def ordered(key, k):
    """bvh_launch's choice between bvh8_traverse_kernel<true> (front to back) and <false>, restated."""
    return depth_complexity(key) >= 0.5 * k


def _rays(key, o, d, w=0, h=0, cam=None):
    o, d = np.ascontiguousarray(o, dtype=np.float32), np.ascontiguousarray(d, dtype=np.float32)
    return SimpleNamespace(key=key, o=o, d=d, n=o.shape[0], w=w, h=h, cam=cam, _dev=None)


@functools.lru_cache(maxsize=None)
def frame(name):
    """One camera's pixel grid, rays generated on the host (the brute force and the device see the same bits); the same
    attributes as the views of tests/test_gpu_raster_passes.py, whose call helpers take it."""
    from quadraturefields_amd import synthetic
    from quadraturefields_amd.mesh_utils import make_camera
    w, h = FRAMES[name]
    c2w = synthetic.orbit_cameras(1, seed=3)[0]
    focal = synthetic.lego_focal(800) * w / 800.0
    o, d = synthetic.camera_rays(c2w, focal, w, h)
    view = _rays(("long-lists frame", name), o.numpy(), d.numpy(), w, h, make_camera(c2w, focal, w, h))
    view.c2w, view.focal = c2w, focal
    return view


@functools.lru_cache(maxsize=None)
def batch(tail=False):
    """Origins on the radius-3 sphere, each ray aimed at a point of uniformly random radius in [0, 1.3]; unit
    directions.  ``tail``: 77 rays more (another draw of the same generator, behind the first 2 000)."""
    rng = np.random.default_rng(20)
    n = BATCH + BATCH_TAIL

    def sphere(m):
        v = rng.normal(size=(m, 3))
        return v / np.linalg.norm(v, axis=1, keepdims=True)

    o = 3.0 * sphere(n)
    target = sphere(n) * rng.uniform(0.0, 1.3, size=(n, 1))
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    m = n if tail else BATCH
    return _rays(("long-lists batch", m), o[:m], d[:m])


def rays(name):
    return {"batch": lambda: batch(False), "batch+77": lambda: batch(True)}.get(name, lambda: frame(name))()


# ------------------------------------------------------------------------------------------------ truth
_TRUTH = {}


def truth(view, min_sep=0.0, key=MESH):
    """(tri [R,128], t [R,128], cnt [R]) of the brute force, ascending in (t, tri), padded with -1 / +inf; computed once
    and read-only.  ``min_sep``: 0, a distance or "trimesh"."""
    at = (key, view.key, min_sep)
    if at not in _TRUTH:
        brute = om.BruteForceIntersector(vertices(key), mesh(key).faces, min_separation=min_sep)
        tri, t, cnt = brute.hits(view.o, view.d, ALL)
        assert cnt.max() < ALL                    # the list really holds every hit
        for a in (tri, t, cnt):
            a.setflags(write=False)
        _TRUTH[at] = SimpleNamespace(tri=tri, t=t, cnt=cnt, min_sep=brute.min_separation)
    return _TRUTH[at]


def first_k(T, k):
    """The K nearest of a truth: what an intersector with ``max_hits = k`` answers (same padding)."""
    return SimpleNamespace(tri=T.tri[:, :k], t=T.t[:, :k], cnt=np.minimum(T.cnt, k))


def crossing_shares(cnt):
    """Shares of rays with 0, 1..16, 17..32, 33..64 and more than 64 hits."""
    edges = [(0, 0), (1, 16), (17, 32), (33, 64), (65, ALL)]
    return [float(((cnt >= lo) & (cnt <= hi)).mean()) for lo, hi in edges]


# ------------------------------------------------------------------------------------------------ keys and the rule
def keys(t, tri):
    """(t bits << 32 | tri): the device's hit key; its unsigned order is the (t, tri) order for the positive t of a hit."""
    return (np.ascontiguousarray(t).view(np.uint32).astype(np.uint64) << np.uint64(32)) | \
        np.ascontiguousarray(tri).astype(np.uint32).astype(np.uint64)


def key_t(k):
    return (k >> np.uint64(32)).astype(np.uint32).view(np.float32)


def key_tri(k):
    return (k & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)


def apply_rule(t_sorted, n, min_sep, strict=True):
    """The re-origin rule over rows ascending in t (first ``n`` valid), in fp32 as the device applies it: the first hit
    is kept, a later one iff t > t_last_kept + min_sep.  -> keep [R,K] bool.  (``strict=False``: the wrong rule, >=, for
    the host test that shows ``spaced_lists`` can tell the two apart.)"""
    t_sorted = np.asarray(t_sorted, dtype=np.float32)
    r, k = t_sorted.shape
    keep = np.zeros((r, k), dtype=bool)
    last = np.full(r, -np.inf, dtype=np.float32)
    ms = np.float32(min_sep)
    with np.errstate(invalid="ignore"):
        for i in range(k):
            reach = last + ms
            ok = (i < n) & ((i == 0) | (t_sorted[:, i] > reach if strict else t_sorted[:, i] >= reach))
            keep[:, i] = ok
            last = np.where(ok, t_sorted[:, i], last)
    return keep


def compact(keep, *rows, pads):
    """Each row's kept entries moved to its front in order, the rest ``pads`` -> (arrays..., kept [R])."""
    order = np.argsort(~keep, axis=1, kind="stable")
    kept = keep.sum(axis=1)
    valid = np.arange(keep.shape[1])[None, :] < kept[:, None]
    return tuple(np.where(valid, np.take_along_axis(a, order, axis=1), p).astype(a.dtype) for a, p in zip(rows, pads)) + (kept,)


def mask_words(keep):
    """keep [R,K<=64] bool -> uint64 words, bit i = column i."""
    bits = np.uint64(1) << np.arange(keep.shape[1], dtype=np.uint64)
    return np.where(keep, bits[None, :], np.uint64(0)).sum(axis=1, dtype=np.uint64)


# ------------------------------------------------------------------------------------------------ lists for the packers
def shuffled_lists(T, k, seed, plus3_every=10):
    """What a pack kernel is handed: each ray's K nearest hits permuted within the row ("lists in ANY order"), the row
    tail +inf / -1, and on every ``plus3_every``-th ray with a full list the count K + 3, which the kernels clamp.
    -> (tri [R,k] int32, t [R,k] fp32, count [R] int32 as handed over, n [R] = min(count, k))."""
    rng = np.random.default_rng(seed)
    r = T.cnt.shape[0]
    n = np.minimum(T.cnt, k).astype(np.int32)
    valid = np.arange(k)[None, :] < n[:, None]
    # a random key per entry, the padding's above every real one: argsort permutes the valid prefix only
    order = np.argsort(np.where(valid, rng.random((r, k)), 2.0), axis=1)
    tri = np.ascontiguousarray(np.take_along_axis(T.tri[:, :k], order, axis=1))
    t = np.ascontiguousarray(np.take_along_axis(T.t[:, :k], order, axis=1))
    assert (tri[~valid] == -1).all() and np.isinf(t[~valid]).all()
    count = n.copy()
    if plus3_every:
        full = np.flatnonzero(n == k)
        count[full[::plus3_every]] = k + 3
    return tri, t, count, n


def sort_rows(tri, t, n):
    """Each row's first ``n`` entries ascending in (t, tri), the rest behind them as they were."""
    k = t.shape[1]
    key = np.where(np.arange(k)[None, :] < np.asarray(n)[:, None], keys(t, tri), BIG)
    order = np.argsort(key, axis=1, kind="stable")
    return np.take_along_axis(tri, order, axis=1), np.take_along_axis(t, order, axis=1)


def tied_lists(T, k):
    """The K nearest with every second distance replaced by its predecessor's: pairs of hits at one t with different
    triangle ids (the scenes themselves have no ties), in (t, tri) order.  Same fields as ``first_k``."""
    n = np.minimum(T.cnt, k)
    tri, t = T.tri[:, :k].copy(), T.t[:, :k].copy()
    half = k // 2
    second = np.arange(1, 2 * half, 2)[None, :] < n[:, None]
    t[:, 1:2 * half:2] = np.where(second, t[:, 0:2 * half:2], t[:, 1:2 * half:2])
    tri, t = sort_rows(tri, t, n)
    return SimpleNamespace(tri=tri, t=t, cnt=n)


def spaced_lists(T, k, min_sep):
    """The K nearest with every third distance replaced by fl32(predecessor + min_sep): hits that lie EXACTLY min_sep
    behind another one, which the rule drops (t > t_last + min_sep is false) when that one was kept.  In (t, tri) order;
    same fields as ``first_k``."""
    n = np.minimum(T.cnt, k)
    tri, t = T.tri[:, :k].copy(), T.t[:, :k].copy()
    ms = np.float32(min_sep)
    for i in range(2, k, 3):
        t[:, i] = np.where(i < n, t[:, i - 1] + ms, t[:, i])
    assert t.dtype == np.float32
    tri, t = sort_rows(tri, t, n)
    return SimpleNamespace(tri=tri, t=t, cnt=n)


# ------------------------------------------------------------------------------------------------ the sample arrays
def pack_reference(o, d, tri, t, n):
    """The six arrays of sampling_raytrace_numpy (mesh_utils.py:343-387) from per-ray lists ascending in (t, tri) (first
    ``n`` of each row): -> dict(rank [S] of each sample within its ray, xyz fp32 [S,3], dirs fp32 [S,3], index_ray int64, depth fp32, index_tri int64, origins
    fp32 [S,3]), ray-major.  The float64 depth never reverses the (t, tri) order (asserted), so there is no second sort."""
    k = t.shape[1]
    ray, rank = np.nonzero(np.arange(k)[None, :] < np.asarray(n)[:, None])         # row-major: (ray, rank) ascending
    o32, d32 = np.asarray(o, dtype=np.float32)[ray], np.asarray(d, dtype=np.float32)[ray]
    o64, d64 = o32.astype(np.float64), d32.astype(np.float64)
    p = o64 + t[ray, rank].astype(np.float64)[:, None] * d64
    q = p - o64
    depth = np.sqrt((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2])
    same = ray[1:] == ray[:-1]
    assert not (depth[:-1][same] > depth[1:][same]).any(), "the float64 depth reversed two hits: a case for the re-sort"
    nrm = np.sqrt((d32[:, 0] * d32[:, 0] + d32[:, 1] * d32[:, 1]) + d32[:, 2] * d32[:, 2]) + np.float32(1e-7)
    assert nrm.dtype == np.float32
    return dict(rank=rank, xyz=p.astype(np.float32), dirs=d32 / nrm[:, None], index_ray=ray.astype(np.int64),
                depth=depth.astype(np.float32), index_tri=tri[ray, rank].astype(np.int64), origins=o32.copy())


def tile_reference(w, h, alloc_counts, kept_counts):
    """The coherent order, written out: tile (row-major 8 x 8 tiles), then rank, then pixel within the tile (row-major).
    The tiles are allotted from ``alloc_counts`` (the counts before the rule: ``tile_base`` is their exclusive scan over
    tiles) and filled with ``kept_counts`` samples per pixel.  -> (slot [R,K] int64 of sample (ray, rank), -1 where the ray
    has no such sample; tile_base [n_tiles]; total; gaps: (first slot, end slot, ray whose first sample fills them) for
    every tile the rule left unused slots in)."""
    kept = np.asarray(kept_counts).reshape(h, w)
    alloc = np.asarray(alloc_counts).reshape(h, w)
    tiles_x, tiles_y = (w + 7) // 8, (h + 7) // 8
    slot = np.full((h * w, max(int(kept.max()), 1)), -1, dtype=np.int64)
    tile_total = np.zeros(tiles_x * tiles_y, dtype=np.int64)
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            tile_total[ty * tiles_x + tx] = alloc[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8].sum()
    tile_base = np.concatenate([[0], np.cumsum(tile_total)[:-1]]).astype(np.int64)
    total = int(tile_total.sum())
    gaps = []
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            tile = ty * tiles_x + tx
            at = int(tile_base[tile])
            ys, xs = np.meshgrid(np.arange(ty * 8, min(ty * 8 + 8, h)), np.arange(tx * 8, min(tx * 8 + 8, w)), indexing="ij")
            pix = (ys * w + xs).reshape(-1)                       # the tile's pixels in lane order
            c = kept.reshape(-1)[pix]
            for rank in range(int(c.max(initial=0))):
                has = pix[c > rank]
                slot[has, rank] = at + np.arange(has.size)
                at += has.size
            end = int(tile_base[tile] + tile_total[tile])
            if at < end:
                gaps.append((at, end, int(pix[np.flatnonzero(c > 0)[0]])))
    return slot, tile_base, total, gaps


# ------------------------------------------------------------------------------------------------ qf_resort_samples
def resort_case(n_rays=48, seed=4):
    """48 rays of 63 or 64 samples -- fifteen of 64 and one of 63, then 64 and 63 alternating -- so that ray 16 starts at
    local offset 1 023 of the first 1 024-sample chunk and its 64 samples end exactly where the 64-sample halo ends, and
    other rays start on, just before and just after the chunk edges; depths descending within each ray and tied in
    pairs.  -> dict of the inputs and the lexsort reference."""
    rng = np.random.default_rng(seed)
    lengths = np.where(np.arange(n_rays) % 2 == 0, 64, 63)
    lengths[:15] = 64
    ray = np.repeat(np.arange(n_rays, dtype=np.int64) * 3 + 5, lengths)            # grouped, ascending, with gaps
    n = ray.size
    start = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    within = np.arange(n) - np.repeat(start, lengths)
    depth = (2.0 + (63 - within) // 2 * 0.03125 + np.repeat(rng.random(n_rays), lengths)).astype(np.float32)
    perm = np.lexsort((depth, ray))
    return dict(index_ray=ray, depth=depth, n=n, start=start, lengths=lengths, perm=perm,
                points=rng.normal(size=(n, 3)).astype(np.float32), origins=rng.normal(size=(n, 3)).astype(np.float32),
                vectors=rng.normal(size=(n, 3)).astype(np.float32), index_tri=rng.integers(0, 1 << 40, size=n),
                boundary=np.concatenate([[1], (ray[1:] != ray[:-1]).astype(np.uint8)]).astype(np.uint8),
                inverse=rng.permutation(n).astype(np.int32))
