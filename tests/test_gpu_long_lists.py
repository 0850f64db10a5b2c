"""GPU: hit lists of 33 to 64 entries on every intersector and pack route, against the brute force that returns every hit
(tests/long_lists.py holds the scenes, the truth and the numpy references; tests/test_long_lists_host.py asserts on the CPU
that a fifth of the frames' rays and a third of the batch's really have 33 .. 64 crossings, more have over 64, and no two
hits of a ray tie).

Above 32 entries the code leaves the register sort networks: pack_samples_kernel stages rows with a strided loop and
insertion-sorts them in LDS, pack_tiles_kernel stages tile rows and insertion-sorts by t or (t, tri), filter_hits_kernel
insertion-sorts, the repair's list headroom min(K + 8, 64) shrinks from K = 56 on, keep masks use bits 32 .. 63 and the
hit bins are switched off.  (a) the general traversal, (b) every camera-coherent pass and the repair with keep masks,
called through the C ABI as tests/test_gpu_raster_passes.py calls them, (c) qf_pack_samples and qf_pack_tiles called
directly on lists the test builds from the truth and shuffles, (d) qf_resort_samples on full-length rays across its chunk
edges, (e) the same lists through ``MeshIntersection`` on every route of the policy, and one rendered frame.

Everything is compared bit for bit (floats as int32 views) unless said otherwise; outputs are filled with sentinels before
each call and the slots nobody should write must still hold them.

Not reached, on purpose: the depth re-sort of the two pack kernels (``if (!sorted)``).  Every operation of sample_depth64 is
monotone in t for t >= 0, so after the (t, tri) sort ``prev > dk`` cannot hold for finite inputs: there is no case to hunt for.
"""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import meshpath as om
from tests import long_lists as ll
from tests.test_gpu_raster_passes import (GARBAGE, SELECT_HEADROOM, SENT_TRI, _apply_rule, _assert_sentinel_behind, _call,
                                          _check_plain, _check_selected, _expected_unanswered, _nearest, _sorted_rows)

pytestmark = pytest.mark.gpu

RULE = ll.RULE
LONG_K = [33, 34, 40, 63, 64]                     # the staged rows and insertion sorts of the pack kernels
NETWORK_K = [1, 3, 16, 17, 31, 32]                # the 16- and the 32-key network, every quartet-tail length
PAD = 24                                          # sentinel slots behind every packed array
QF_ERR_INVALID_ARGUMENT = -1


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _same(got, want):
    """Bit for bit: floats as int32 views, everything else by value."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    return np.array_equal(_bits(got), _bits(want)) if got.dtype == np.float32 else np.array_equal(got, want)


_RI = {}


def _ri(key=ll.MESH, builder="host"):
    """One ``RayIntersector`` per (mesh, builder), shared by every K and rule (only its BVH handle is used)."""
    from quadraturefields_amd.mesh_io import TriMesh
    from quadraturefields_amd.mesh_utils import RayIntersector
    if (key, builder) not in _RI:
        _RI[key, builder] = RayIntersector(TriMesh(ll.vertices(key), ll.mesh(key).faces), max_hits=64, min_separation=0,
                                           builder=builder)
    return _RI[key, builder]


def _dev(view, device):
    if view._dev is None:
        view._dev = (torch.from_numpy(view.o).to(device), torch.from_numpy(view.d).to(device))
    return view._dev


def _up(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


# ------------------------------------------------------------------------------------------------ (a) general traversal
def _bvh_lists(lib, ri, view, k, min_sep):
    from quadraturefields_amd import _C
    ri.set_min_separation(min_sep)
    o, d = _dev(view, ri.device)
    tri = torch.full((view.n, k), SENT_TRI, dtype=torch.int32, device=ri.device)
    t = torch.full((view.n, k), float("nan"), dtype=torch.float32, device=ri.device)
    cnt = torch.full((view.n,), GARBAGE, dtype=torch.int32, device=ri.device)
    _C.check(lib.qf_bvh_intersect(ri._handle, _C.ptr(o), _C.ptr(d), view.n, k, view.w, _C.ptr(tri), _C.ptr(t), _C.ptr(cnt),
                                  _C.stream()), "qf_bvh_intersect")
    return tri.cpu().numpy(), t.cpu().numpy(), cnt.cpu().numpy()


def _check_bvh_lists(lib, ri, key, view, k, rule):
    Tr = ll.truth(view, rule, key)
    want = ll.first_k(Tr, k)
    tri, t, cnt = _bvh_lists(lib, ri, view, k, Tr.min_sep)
    assert np.array_equal(cnt, want.cnt)
    assert np.array_equal(tri, want.tri), "ids, the -1 padding included"
    assert _same(t, want.t), "distances, the +inf padding included"
    return Tr


@pytest.mark.parametrize("k", [33, 40, 48, 56, 57, 63, 64])
@pytest.mark.parametrize("rule", [0.0, RULE, "trimesh"])
@pytest.mark.parametrize("builder", ["host", "device"])
@pytest.mark.parametrize("name", ["batch", "batch+77", "aligned", "ragged"])
def test_general_traversal_keeps_the_k_nearest(device, lib, name, builder, rule, k):
    """qf_bvh_intersect: counts min(n, K) and the K nearest (t, tri) after the rule, padding included; plain batches and
    the image_width route.  On the 36 shells (mean depth 15.7 < K / 2) every K here runs bvh8_traverse_kernel<false>."""
    ri = _ri(ll.MESH, builder)
    assert not lib.qf_bvh_depth_complexity(ri._handle) >= 0.5 * k
    Tr = _check_bvh_lists(lib, ri, ll.MESH, ll.rays(name), k, rule)
    if rule == 0.0:
        # truncated lists and long complete ones (crossings come in pairs: the latter from K = 34 on)
        assert (Tr.cnt > k).any() and (k == 33 or ((Tr.cnt > 32) & (Tr.cnt <= k)).any())


@pytest.mark.parametrize("k", [33, 40, 48, 56, 57, 63, 64])
@pytest.mark.parametrize("rule", [0.0, RULE])
@pytest.mark.parametrize("builder", ["host", "device"])
@pytest.mark.parametrize("name", ["batch+77", "aligned"])
def test_general_traversal_front_to_back(device, lib, name, builder, rule, k):
    """The 48 shells between radius 1.0 and 1.2 (mean depth 39 >= K / 2 for every K): bvh8_traverse_kernel<true>, whose
    distance limit closes in once the list is full -- up to 96 crossings for 33 .. 64 slots."""
    ri = _ri(ll.DENSE, builder)
    assert lib.qf_bvh_depth_complexity(ri._handle) >= 0.5 * k
    Tr = _check_bvh_lists(lib, ri, ll.DENSE, ll.rays(name), k, rule)
    if rule == 0.0:
        assert (Tr.cnt > 64).mean() > 0.4


# ------------------------------------------------------------------------------------------------ (b) the camera passes
FRAME_NAMES = ["aligned", "ragged"]


def _rule_truth(view, k, min_sep):
    return ll.first_k(ll.truth(view, min_sep), k) if min_sep else None


@pytest.mark.parametrize("cull", [0, 1])
@pytest.mark.parametrize("k", [40, 64])
@pytest.mark.parametrize("name", FRAME_NAMES)
def test_plain_and_culled_pass_raw_lists(device, lib, name, k, cull):
    """Lists as sets, counts exact (past K the pass keeps counting), the overflow word = the candidates beyond K summed
    over the rays with more than K hits -- non-zero exactly when there is such a ray."""
    view, T = ll.frame(name), ll.truth(ll.frame(name))
    out = _call(lib, _ri(), view, k, "plain", cull=cull, sort_lists=0)
    _check_plain(out, T, k)
    assert (out.overflow > 0) == bool((T.cnt > k).any()) and int((out.count > k).sum()) == int((T.cnt > k).sum()) > 0
    assert ((T.cnt > 32) & (T.cnt <= k)).sum() > 50
    _check_plain(_call(lib, _ri(), view, k, "plain", cull=cull, sort_lists=2), T, k, ids=False)


@pytest.mark.parametrize("min_sep", [0.0, RULE])
@pytest.mark.parametrize("k", [33, 40, 64])
@pytest.mark.parametrize("name", FRAME_NAMES)
def test_sorted_lists_up_to_64_long(device, lib, name, k, min_sep):
    """sort_lists = 1: filter_hits_kernel's insertion sort (K > 32) and rule.  The rows of rays with at most K raw hits are
    the brute force's with the same rule, padding included (the others are the repair's)."""
    view = ll.frame(name)
    T, Tr = ll.truth(view), ll.first_k(ll.truth(view, min_sep), k)
    out = _call(lib, _ri(), view, k, "plain", sort_lists=1, min_sep=min_sep)
    assert out.flag == 0 and out.overflow == int(np.maximum(T.cnt - k, 0).sum())
    full = T.cnt <= k
    # lists longer than 32 among the compared rows (crossings come in pairs: none at K = 33, where the insertion sort runs
    # on shorter ones)
    assert k == 33 or (full & (T.cnt > 32)).sum() > 50
    if min_sep:
        assert (Tr.cnt[full] != T.cnt[full]).any()
    assert np.array_equal(out.count[full], Tr.cnt[full])
    assert np.array_equal(out.tri[full], Tr.tri[full])
    assert _same(out.t[full], Tr.t[full])


@pytest.mark.parametrize("min_sep", [0.0, RULE])
@pytest.mark.parametrize("cull", [0, 1])
@pytest.mark.parametrize("k,wide", [(40, 40), (40, 128), (64, 64), (64, 128)])
@pytest.mark.parametrize("name", FRAME_NAMES)
def test_wide_pass_selects_the_k_nearest(device, lib, name, k, wide, cull, min_sep):
    view = ll.frame(name)
    T = ll.truth(view)
    out = _call(lib, _ri(), view, k, "wide", cull=cull, wide=wide, min_sep=min_sep)
    _check_selected(out, T, _rule_truth(view, k, min_sep), k, wide, min_sep, exact_overflow=True)
    assert ((T.cnt > k) & (T.cnt <= wide)).any() == (wide > k)            # rays whose K nearest are SELECTED from more


def _repair(lib, ri, view, k, dv, mask=None, raw=None):
    from quadraturefields_amd import _C
    _C.check(lib.qf_bvh_repair_overflow(ri._handle, _C.ptr(dv.o), _C.ptr(dv.d), view.n, k, view.w, _C.ptr(dv.tri), _C.ptr(dv.t),
                                        _C.ptr(dv.cnt), _C.ptr(mask), _C.ptr(raw), _C.ptr(dv.flag), _C.stream()),
             "qf_bvh_repair_overflow")
    return dv.tri.cpu().numpy(), dv.t.cpu().numpy(), dv.cnt.cpu().numpy()


@pytest.mark.parametrize("min_sep", [0.0, RULE])
@pytest.mark.parametrize("slabs", [2, 8])
@pytest.mark.parametrize("wide", ["smallest", 128])
@pytest.mark.parametrize("name", FRAME_NAMES)
def test_slab_pass_selects_the_k_nearest_and_repairs(device, lib, name, wide, slabs, min_sep):
    """K = 40; ``wide``: the smallest the entry point admits (selection capacity + 2), and 128."""
    from quadraturefields_amd import _C
    k = 40
    capacity = k + SELECT_HEADROOM if min_sep > 0 else k
    if wide == "smallest":
        wide = capacity + 2
        with pytest.raises(ValueError):
            _call(lib, _ri(), ll.frame(name), k, "slabs", wide=wide - 1, slabs=slabs, min_sep=min_sep)
    view, ri = ll.frame(name), _ri()
    T, Tr = ll.truth(view), _rule_truth(view, k, min_sep)
    out = _call(lib, ri, view, k, "slabs", wide=wide, slabs=slabs, min_sep=min_sep)
    # rays with more crossings than slots may or may not be answered (a pixel that filled up in an earlier slab is
    # skipped); every ray within `wide` is answered by the pass itself -- unless, rule on, its chain over the held prefix
    # kept fewer than K while candidates remained
    assert out.flag == 0 and (T.cnt > wide).any() == (wide < 72)
    within = T.cnt <= wide
    got, valid = _sorted_rows(out.t, out.tri, out.count)
    _assert_sentinel_behind(out, within, valid)
    answered = out.count <= k
    assert answered[within & ~_expected_unanswered(T, k, wide, min_sep)].all()
    if not min_sep:
        assert np.array_equal(out.count[within], np.minimum(T.cnt, k)[within])
        assert np.array_equal(got[answered], _nearest(T, k)[answered]) and (out.count[answered & ~within] == k).all()
    else:
        filt, kept = _apply_rule(got, np.minimum(out.count, k), min_sep)
        assert np.array_equal(kept[answered], Tr.cnt[answered])
        assert np.array_equal(filt[answered], _sorted_rows(Tr.t, Tr.tri, Tr.cnt)[0][answered])
    # the repair and the filter afterwards: the brute force's lists
    tri, t, cnt = _repair(lib, ri, view, k, out.dev)
    _C.check(lib.qf_filter_hits(ri._handle, view.n, k, _C.ptr(out.dev.tri), _C.ptr(out.dev.t), _C.ptr(out.dev.cnt), _C.stream()),
             "qf_filter_hits")
    if min_sep:
        assert np.array_equal(out.dev.cnt.cpu().numpy(), Tr.cnt) and np.array_equal(out.dev.tri.cpu().numpy(), Tr.tri)
        assert _same(out.dev.t.cpu().numpy(), Tr.t)
    else:
        assert np.array_equal(cnt, np.minimum(T.cnt, k)) and np.array_equal(_sorted_rows(t, tri, cnt)[0], _nearest(T, k))


@pytest.mark.parametrize("k", [40, 55, 56, 57, 60, 64])
@pytest.mark.parametrize("rule", [RULE, "trimesh"])
@pytest.mark.parametrize("name", FRAME_NAMES)
def test_repair_with_keep_masks(device, lib, name, rule, k):
    """qf_bvh_repair_overflow after the plain pass, rule on, with keep masks.  A ray with more than K candidates is
    traversed again, in a list of min(K + 8, 64) slots -- no spare slot at K = 64, where the rule has to page: its row is
    the brute force's with the rule (padded), its mask the low bits.  Every other ray keeps its row in arrival order;
    bit i of its mask = the i-th hit in (t, tri) order is kept, raw_count = the row's length, hit_count = the kept."""
    view, ri = ll.frame(name), _ri()
    T, Tr_all = ll.truth(view), ll.truth(view, rule)
    Tr, sep = ll.first_k(Tr_all, k), Tr_all.min_sep
    out = _call(lib, ri, view, k, "plain", sort_lists=0, min_sep=sep)
    before_t, before_tri = out.t.copy(), out.tri.copy()
    mask = torch.full((view.n,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=device)
    raw = torch.full((view.n,), GARBAGE, dtype=torch.int32, device=device)
    tri, t, cnt = _repair(lib, ri, view, k, out.dev, mask, raw)
    mask, raw = mask.cpu().numpy().view(np.uint64), raw.cpu().numpy()
    again = T.cnt > k
    assert again.sum() > 50 and (~again & (T.cnt > 32)).sum() > 50
    assert np.array_equal(cnt, Tr.cnt), "hit_count = the hits the rule keeps, at most K"
    # traversed again
    assert np.array_equal(tri[again], Tr.tri[again]) and _same(t[again], Tr.t[again])
    assert np.array_equal(raw[again], Tr.cnt[again])
    assert np.array_equal(mask[again], ll.mask_words(np.arange(64)[None, :] < Tr.cnt[again, None]))
    # decided in place
    rest = ~again
    assert np.array_equal(tri[rest], before_tri[rest]) and _same(t[rest], before_t[rest]), "a complete list was rewritten"
    assert np.array_equal(raw[rest], T.cnt[rest])
    keep = ll.apply_rule(T.t[:, :k], np.minimum(T.cnt, k), sep)
    assert np.array_equal(mask[rest], ll.mask_words(keep)[rest])
    long_rows = rest & (T.cnt > 32)
    in_list = np.arange(32, k)[None, :] < T.cnt[long_rows, None]
    assert (keep[long_rows][:, 32:] & in_list).any(), "no checked ray has a mask bit at position >= 32 set"
    if rule == RULE:                              # (the reference's own distance drops a handful of hits in the whole frame)
        assert (~keep[long_rows][:, 32:] & in_list).any(), "no checked ray has a mask bit at position >= 32 cleared"
        assert (Tr.cnt[again] < k).all()          # K = 40 holds every list the rule keeps: the paging ends by exhaustion


@pytest.mark.parametrize("crafted", ["none", "ties", "spaced"])
@pytest.mark.parametrize("k", [33, 40, 64])
def test_filter_hits_on_shuffled_lists(device, lib, k, crafted):
    """qf_filter_hits called directly on 2 077 shuffled rows (the last workgroup is partial): sorted by (t, tri), the rule
    applied, padded, counted.  ``ties``: pairs of hits at one t; ``spaced``: hits exactly min_sep behind another."""
    from quadraturefields_amd import _C
    view, ri = ll.rays("batch+77"), _ri()
    T = ll.truth(view)
    L = {"none": ll.first_k, "ties": ll.tied_lists, "spaced": lambda T, k: ll.spaced_lists(T, k, RULE)}[crafted](T, k)
    tri, t, count, n = ll.shuffled_lists(L, k, seed=400 + k)
    keep = ll.apply_rule(L.t, n, RULE)
    want_tri, want_t, kept = ll.compact(keep, L.tri, L.t, pads=(-1, np.inf))
    assert (kept > 12).any() and (kept < n).mean() > 0.5
    ri.set_min_separation(RULE)
    dtri, dt, dc = _up(tri, device), _up(t, device), _up(count.astype(np.int32), device)
    _C.check(lib.qf_filter_hits(ri._handle, view.n, k, _C.ptr(dtri), _C.ptr(dt), _C.ptr(dc), _C.stream()), "qf_filter_hits")
    assert np.array_equal(dc.cpu().numpy(), kept)
    assert np.array_equal(dtri.cpu().numpy(), want_tri) and _same(dt.cpu().numpy(), want_t)


def _repair_lds_bytes(k, stack, rule=True, masks=True):
    """bvh_launch's dynamic LDS of the repair launch, restated: 32 rays x (list slots x 8 bytes, twice with the rule, + the
    odd-strided stack) and, with keep masks, 256 x K distance columns."""
    list_cap = min(k + 8, 64) if rule else k
    lds = 32 * (list_cap * 8 * (2 if rule else 1) + (max(stack, 2) | 1) * 4)
    return (lds + 3) // 4 * 4 + 256 * k * 4 if (rule and masks) else lds


@pytest.mark.parametrize("builder", ["host", "device"])
@pytest.mark.parametrize("key", [ll.MESH, ll.DENSE])
def test_the_largest_repair_launch_is_far_from_the_refusal(device, lib, key, builder):
    """bvh_launch refuses (QF_ERR_UNSUPPORTED) above 160 KiB - 2048 bytes of LDS.  The largest footprint a supported K can
    ask for is the repair with keep masks at K = 64: 96 KiB of lists and distance columns + 128 bytes per stack entry, so
    the refusal needs a tree whose traversal stack bound reaches 496 entries.  These trees stay under half of that (and
    every K of this file is answered: test_repair_with_keep_masks, test_general_traversal_*)."""
    limit = 160 * 1024 - 2048
    assert _repair_lds_bytes(64, 495) <= limit < _repair_lds_bytes(64, 497)
    assert all(_repair_lds_bytes(k, 495) <= _repair_lds_bytes(64, 495) for k in range(1, 65))
    stack = int(lib.qf_bvh_max_stack(_ri(key, builder)._handle))
    print(key, builder, "max stack", stack, "repair LDS at K = 64:", _repair_lds_bytes(64, stack))
    assert 0 < stack < 248 and _repair_lds_bytes(64, stack) < limit - 32 * 1024


# ------------------------------------------------------------------------------------------------ (c) the pack kernels
def _filled(shape, dtype, device):
    if dtype == torch.float32:
        return torch.full(shape, float("nan"), dtype=dtype, device=device)
    return torch.full(shape, SENT_TRI, dtype=dtype, device=device)


def _pack_samples(lib, device, view, k, tri, t, count, per_ray, inverse=None, mask=None, raw=None, min_sep=0.0, flag=None,
                  ray_major=True):
    """qf_pack_samples on host lists; ``per_ray`` = the samples each ray must produce (its offsets are their scan).
    -> dict of host arrays, PAD sentinel slots behind each."""
    from quadraturefields_amd import _C
    o, d = _dev(view, device)
    total = int(per_ray.sum())
    offsets = _up(np.concatenate([[0], np.cumsum(per_ray)]).astype(np.int64), device)
    s = total + PAD
    out = dict(index_ray=_filled((s,), torch.int64, device), depth=_filled((s,), torch.float32, device),
               index_tri=_filled((s,), torch.int64, device))
    for name in ("xyz", "dirs", "origins"):
        out[name] = _filled((s, 3), torch.float32, device) if ray_major else None
    inv = None
    if inverse is not None:
        inv = _up(inverse.astype(np.int32), device)
        out.update(xyz_c=_filled((s, 3), torch.float32, device), dirs_c=_filled((s, 3), torch.float32, device),
                   depth_c=_filled((s,), torch.float32, device))
    P = _C.ptr
    keep = (None, None) if mask is None else (_up(mask.view(np.int64), device), _up(raw.astype(np.int32), device))
    dt, dtri, dc = _up(t, device), _up(tri, device), _up(count.astype(np.int32), device)
    _C.check(lib.qf_pack_samples(P(o), P(d), view.n, k, P(dtri), P(dt), P(dc), P(offsets), P(out["xyz"]), P(out["dirs"]),
                                 P(out["index_ray"]), P(out["depth"]), P(out["index_tri"]), P(out["origins"]), P(inv),
                                 P(out.get("xyz_c")), P(out.get("dirs_c")), P(out.get("depth_c")), P(keep[0]), P(keep[1]),
                                 float(min_sep), P(flag), _C.stream()), "qf_pack_samples")
    return {name: a.cpu().numpy() for name, a in out.items() if a is not None}, total


def _check_samples(got, total, ref, inverse=None):
    """The six arrays, the coherent copies through ``inverse``, and the sentinels behind."""
    assert total == ref["index_ray"].shape[0]
    for name in ("xyz", "dirs", "index_ray", "depth", "index_tri", "origins"):
        if name in got:
            assert _same(got[name][:total], ref[name]), name
    if inverse is not None:
        for name, src in (("xyz_c", "xyz"), ("dirs_c", "dirs"), ("depth_c", "depth")):
            assert _same(got[name][:total][inverse], ref[src]), name
    for name, a in got.items():
        tail = a[total:]
        assert np.isnan(tail).all() if a.dtype == np.float32 else (tail == SENT_TRI).all(), name + ": written past the end"


def _random_masks(n, k, seed):
    """Keep bits over each ray's ``n`` sorted entries, about two thirds set, on both sides of bit 32 where the list is
    that long.  -> (keep [R,k] bool, words uint64)"""
    rng = np.random.default_rng(seed)
    keep = (rng.random((n.shape[0], k)) < 0.65) & (np.arange(k)[None, :] < n[:, None])
    return keep, ll.mask_words(keep)


@pytest.mark.parametrize("k", NETWORK_K + LONG_K)
def test_pack_samples_from_shuffled_lists(device, lib, k):
    """2 077 rays (the last workgroup holds 29), each ray's K nearest shuffled within its row, +inf / -1 behind, every
    tenth full list with the count K + 3.  Plain; with a random ``inverse`` and the coherent copies (also without the
    ray-major arrays); with keep masks."""
    view = ll.rays("batch+77")
    T = ll.truth(view)
    tri, t, count, n = ll.shuffled_lists(T, k, seed=k)
    assert (count == k + 3).sum() > 10 and view.n % 128 == 29
    if k > 32:
        # (crossings of closed shells come in pairs: no ray has exactly 33)
        assert (k <= 34 or ((n > 32) & (n < k)).any()) and (n == k).mean() > 0.3
    ref = ll.pack_reference(view.o, view.d, T.tri[:, :k], T.t[:, :k], n)
    got, total = _pack_samples(lib, device, view, k, tri, t, count, n)
    _check_samples(got, total, ref)
    inverse = np.random.default_rng(k).permutation(total)
    got, total = _pack_samples(lib, device, view, k, tri, t, count, n, inverse=inverse)
    _check_samples(got, total, ref, inverse)
    got, total = _pack_samples(lib, device, view, k, tri, t, count, n, inverse=inverse, ray_major=False)
    assert "xyz" not in got
    _check_samples(got, total, ref, inverse)
    # keep masks over the sorted list: raw_count = the stored list's length, hit_count = the bits set
    keep, words = _random_masks(n, k, seed=100 + k)
    if k > 33:
        rows = n > 33
        assert keep[rows][:, 32:].any() and (~keep[rows][:, 32:33]).any() and keep[rows][:, :32].any()
    ktri, kt, kept = ll.compact(keep, T.tri[:, :k], T.t[:, :k], pads=(-1, np.inf))
    ref = ll.pack_reference(view.o, view.d, ktri, kt, kept)
    got, total = _pack_samples(lib, device, view, k, tri, t, kept, kept, mask=words, raw=count)
    _check_samples(got, total, ref)


@pytest.mark.parametrize("k", [17, 40, 64])
def test_pack_samples_close_flag(device, lib, k):
    """The optimistic route: *close_flag is raised exactly when some ray has two packed hits not more than min_sep apart
    (fp32: not t[i] > t[i-1] + min_sep), and the samples are packed as if the rule dropped nothing either way."""
    view = ll.rays("batch+77")
    T = ll.truth(view)
    tri, t, count, n = ll.shuffled_lists(T, k, seed=k)
    ref = ll.pack_reference(view.o, view.d, T.tri[:, :k], T.t[:, :k], n)
    valid = np.arange(1, k)[None, :] < n[:, None]
    with np.errstate(invalid="ignore"):
        gap = float(np.where(valid, T.t[:, 1:k] - T.t[:, :k - 1], np.inf).min())
    for min_sep in (gap * 0.99, gap * 1.01, RULE, 1e-5):
        ms = np.float32(min_sep)
        with np.errstate(invalid="ignore"):
            close = bool((valid & ~(T.t[:, 1:k] > T.t[:, :k - 1] + ms)).any())
        assert close == (min_sep > gap)
        flag = torch.zeros((1,), dtype=torch.int32, device=device)
        got, total = _pack_samples(lib, device, view, k, tri, t, count, n, min_sep=float(ms), flag=flag)
        assert int(flag.item()) == int(close), min_sep
        _check_samples(got, total, ref)


@pytest.mark.parametrize("k", [17, 40, 64])
def test_pack_kernels_order_equal_distances_by_triangle_id(device, lib, k):
    """The scenes have no two hits at one t (tests/test_long_lists_host.py), so their lists cannot tell a sort by t from
    one by (t, tri).  Here every second distance of a row is replaced by its predecessor's: the packed ids must come out
    in (t, tri) order, from qf_pack_samples and from qf_pack_tiles with tri_c."""
    view = ll.frame("ragged")
    Tt = ll.tied_lists(ll.truth(view), k)
    assert ((Tt.t[:, 1:] == Tt.t[:, :-1]) & (Tt.tri[:, 1:] > Tt.tri[:, :-1]) & (np.arange(1, k)[None, :] < Tt.cnt[:, None])).sum() > 1000
    tri, t, count, n = ll.shuffled_lists(Tt, k, seed=300 + k)
    ref = ll.pack_reference(view.o, view.d, Tt.tri, Tt.t, n)
    got, total = _pack_samples(lib, device, view, k, tri, t, count, n)
    _check_samples(got, total, ref)
    slot, tile_base, total, gaps = ll.tile_reference(view.w, view.h, n, n)
    got = _pack_tiles(lib, device, view, k, tri, t, count, tile_base, total, True)
    _check_tiles(got, view, ref, slot, total, gaps, True)


@pytest.mark.parametrize("with_tri", [True, False])
@pytest.mark.parametrize("k", [17, 40, 64])
def test_tile_pack_drops_a_hit_exactly_min_sep_behind(device, lib, k, with_tri):
    """The tile kernel's own rule on lists with hits exactly min_sep behind another (t > t_last + min_sep is false there)."""
    view = ll.frame("ragged")
    L = ll.spaced_lists(ll.truth(view), k, RULE)
    tri, t, count, n = ll.shuffled_lists(L, k, seed=500 + k)
    keep = ll.apply_rule(L.t, n, RULE)
    ktri, kt, kept = ll.compact(keep, L.tri, L.t, pads=(-1, np.inf))
    ref = ll.pack_reference(view.o, view.d, ktri, kt, kept)
    slot, tile_base, total, gaps = ll.tile_reference(view.w, view.h, n, kept)
    got = _pack_tiles(lib, device, view, k, tri, t, count, tile_base, total, with_tri, min_sep=RULE, want_final=True)
    _check_tiles(got, view, ref, slot, total, gaps, with_tri)
    assert np.array_equal(got["final_count"], kept) and int(got["dropped"][0]) == int((n - kept).sum()) > 0


def _pack_tiles(lib, device, view, k, tri, t, count, tile_base, total, with_tri, mask=None, raw=None, min_sep=0.0,
                want_final=False, host_out=False):
    from quadraturefields_amd import _C
    o, d = _dev(view, device)
    s = total + PAD
    out = dict(xyz_c=_filled((s, 3), torch.float32, device), dirs_c=_filled((s, 3), torch.float32, device),
               depth_c=_filled((s,), torch.float32, device))
    if with_tri:
        out["tri_c"] = _filled((s,), torch.int32, device)
    if want_final:
        out["final_count"] = torch.full((view.n,), GARBAGE, dtype=torch.int32, device=device)
        # with host_out the counter must be zero on entry and is zero again afterwards; without, the call zeroes it
        out["dropped"] = torch.full((1,), 0 if host_out else GARBAGE, dtype=torch.int32, device=device)
    host = torch.full((4,), -5, dtype=torch.int64).pin_memory() if host_out else None
    P = _C.ptr
    keep = (None, None) if mask is None else (_up(mask.view(np.int64), device), _up(raw.astype(np.int32), device))
    dt, dc = _up(t, device), _up(count.astype(np.int32), device)
    dtri = _up(tri, device) if with_tri else None                    # without tri_c the ids are not read at all
    dbase, dtotal = _up(tile_base, device), _up(np.array([total], dtype=np.int64), device)
    _C.check(lib.qf_pack_tiles(P(o), P(d), view.w, view.h, k, P(dtri), P(dt), P(dc), P(dbase),
                               P(dtotal), P(out["xyz_c"]), P(out["dirs_c"]),
                               P(out["depth_c"]), P(out.get("tri_c")), P(keep[0]), P(keep[1]), float(min_sep),
                               P(out.get("final_count")), P(out.get("dropped")),
                               ctypes.c_void_p(host.data_ptr()) if host_out else None, 0, _C.stream()), "qf_pack_tiles")
    torch.cuda.synchronize()
    got = {name: a.cpu().numpy() for name, a in out.items()}
    if host_out:
        got["host_out"] = host.numpy().copy()
    return got


def _check_tiles(got, view, ref, slot, total, gaps, with_tri):
    """The exact slot of every sample; the rule's gaps; nothing else written."""
    at = slot[ref["index_ray"], ref["rank"]]
    assert (at >= 0).all() and np.unique(at).size == at.size
    want = dict(xyz_c=np.full((total + PAD, 3), np.nan, np.float32), dirs_c=np.full((total + PAD, 3), np.nan, np.float32),
                depth_c=np.full((total + PAD,), np.nan, np.float32), tri_c=np.full((total + PAD,), SENT_TRI, np.int32))
    want["xyz_c"][at], want["dirs_c"][at], want["depth_c"][at] = ref["xyz"], ref["dirs"], ref["depth"]
    want["tri_c"][at] = ref["index_tri"].astype(np.int32)
    first = np.flatnonzero(ref["rank"] == 0)
    first_of = dict(zip(ref["index_ray"][first].tolist(), first.tolist()))
    for lo, hi, ray in gaps:                      # the tile's first sample: position, direction and id, depth 0
        src = first_of[ray]
        want["xyz_c"][lo:hi], want["dirs_c"][lo:hi], want["depth_c"][lo:hi] = ref["xyz"][src], ref["dirs"][src], 0.0
        want["tri_c"][lo:hi] = ref["index_tri"][src]
    for name in ("xyz_c", "dirs_c", "depth_c") + (("tri_c",) if with_tri else ()):
        assert _same(got[name], want[name]), name


@pytest.mark.parametrize("with_tri", [True, False])
@pytest.mark.parametrize("k", NETWORK_K + LONG_K)
@pytest.mark.parametrize("name", FRAME_NAMES)
def test_pack_tiles_from_shuffled_lists(device, lib, name, k, with_tri):
    """qf_pack_tiles, both kTri instantiations (without tri_c the rows are sorted by t alone), on a tile-aligned frame and
    one with ragged right and bottom tiles.  Rule off; rule on in the kernel (final_count, dropped, host_out[2], the gap
    slots); keep masks."""
    view = ll.frame(name)
    T = ll.truth(view)
    tri, t, count, n = ll.shuffled_lists(T, k, seed=k)
    assert (count == k + 3).sum() > 5
    if k > 32:
        assert ((n > 32) & (n < k)).any() or k <= 34
    ref = ll.pack_reference(view.o, view.d, T.tri[:, :k], T.t[:, :k], n)
    slot, tile_base, total, gaps = ll.tile_reference(view.w, view.h, n, n)
    assert not gaps
    got = _pack_tiles(lib, device, view, k, tri, t, count, tile_base, total, with_tri)
    _check_tiles(got, view, ref, slot, total, gaps, with_tri)
    got = _pack_tiles(lib, device, view, k, tri, t, count, tile_base, total, with_tri, want_final=True)
    _check_tiles(got, view, ref, slot, total, gaps, with_tri)
    assert np.array_equal(got["final_count"], n) and int(got["dropped"][0]) == 0      # final_count without the rule
    # the rule applied by the tile kernel itself, on the sorted K nearest it was handed
    keep = ll.apply_rule(T.t[:, :k], n, RULE)
    ktri, kt, kept = ll.compact(keep, T.tri[:, :k], T.t[:, :k], pads=(-1, np.inf))
    ref_r = ll.pack_reference(view.o, view.d, ktri, kt, kept)
    slot_r, base_r, total_r, gaps_r = ll.tile_reference(view.w, view.h, n, kept)
    assert np.array_equal(base_r, tile_base) and total_r == total and (bool(gaps_r) == (k > 1))
    for host_out in (False, True):
        got = _pack_tiles(lib, device, view, k, tri, t, count, tile_base, total, with_tri, min_sep=RULE, want_final=True,
                          host_out=host_out)
        _check_tiles(got, view, ref_r, slot_r, total, gaps_r, with_tri)
        assert np.array_equal(got["final_count"], kept)
        dropped = int((n - kept).sum())
        if host_out:
            assert got["host_out"].tolist() == [-5, -5, dropped, -5] and int(got["dropped"][0]) == 0
        else:
            assert int(got["dropped"][0]) == dropped
    # keep masks: the counts (and so the tiles' slots) already count only the kept
    keep, words = _random_masks(n, k, seed=200 + k)
    ktri, kt, kept = ll.compact(keep, T.tri[:, :k], T.t[:, :k], pads=(-1, np.inf))
    ref_m = ll.pack_reference(view.o, view.d, ktri, kt, kept)
    slot_m, base_m, total_m, gaps_m = ll.tile_reference(view.w, view.h, kept, kept)
    got = _pack_tiles(lib, device, view, k, tri, t, kept, base_m, total_m, with_tri, mask=words, raw=count, min_sep=RULE,
                      want_final=True)
    _check_tiles(got, view, ref_m, slot_m, total_m, gaps_m, with_tri)
    assert np.array_equal(got["final_count"], kept) and int(got["dropped"][0]) == 0


def test_hit_bins_stop_at_32(device, lib):
    """qf_pack_tiles_bins refuses K = 33 before any launch, and a ``RayIntersector`` frame at K = 40 takes a lists route."""
    from quadraturefields_amd import _C
    view, k = ll.frame("aligned"), 33
    o, d = _dev(view, device)
    n_tiles = ((view.w + 7) // 8) * ((view.h + 7) // 8)
    z32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=device)                    # noqa: E731
    z64 = lambda *s: torch.zeros(s, dtype=torch.int64, device=device)                    # noqa: E731
    out = [_filled((8, 3), torch.float32, device), _filled((8, 3), torch.float32, device), _filled((8,), torch.float32, device)]
    P = _C.ptr
    keep_alive = []

    def args(kk):
        a = [z32(view.n, kk), torch.zeros((view.n, kk), device=device), z32(view.n), z64(n_tiles), z64(1), z32(n_tiles),
             z64(n_tiles), z64(n_tiles * 64 * kk)]
        keep_alive.append(a)
        return (P(o), P(d), view.w, view.h, kk, P(a[0]), P(a[1]), P(a[2]), P(a[3]), P(a[4]), P(out[0]), P(out[1]), P(out[2]),
                None, 0.0, None, None, None, 0, P(a[5]), P(a[6]), P(a[7]), None, _C.stream())

    assert lib.qf_pack_tiles_bins(*args(33)) == QF_ERR_INVALID_ARGUMENT
    assert lib.qf_pack_tiles_bins(*args(64)) == QF_ERR_INVALID_ARGUMENT
    assert lib.qf_pack_tiles_bins(*args(32)) == 0                         # (all counts zero: nothing to write)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(a).all()) for a in out)
    ri = _policy_mi(40, 0.0).rayintersector
    _reset_policy(ri)
    assert ri._hit_bins_ready(25, view.cam) and not ri._hit_bins_ready(40, view.cam)
    ri.sample_frame_device(o, d, 40, camera=view.cam)
    assert ri.last_route == "plain"
    ri.frame_samples()


# ------------------------------------------------------------------------------------------------ (d) qf_resort_samples
@pytest.mark.parametrize("optional", ["all", "none", "perm", "inverse", "boundary"])
def test_resort_full_length_rays_across_the_chunk_edges(device, lib, optional):
    """48 rays of 63 / 64 samples, depths reversed and tied in pairs: np.lexsort((depth, ray)), stable; with and without
    perm, inverse (the coherent copies) and boundary."""
    from quadraturefields_amd import _C
    c = ll.resort_case()
    n, perm_want = c["n"], c["perm"]
    want_perm, want_inv, want_bnd = (optional in ("all", x) for x in ("perm", "inverse", "boundary"))
    s = n + PAD
    out = SimpleNamespace(points=_filled((s, 3), torch.float32, device), depth=_filled((s,), torch.float32, device),
                          origins=_filled((s, 3), torch.float32, device), vectors=_filled((s, 3), torch.float32, device),
                          tri=_filled((s,), torch.int64, device),
                          perm=_filled((s,), torch.int64, device) if want_perm else None,
                          boundary=torch.full((s,), 77, dtype=torch.uint8, device=device) if want_bnd else None,
                          points_c=_filled((s, 3), torch.float32, device) if want_inv else None,
                          vectors_c=_filled((s, 3), torch.float32, device) if want_inv else None)
    P = _C.ptr
    inv = _up(c["inverse"], device) if want_inv else None
    src = {name: _up(c[name], device) for name in ("index_ray", "depth", "points", "origins", "vectors", "index_tri")}
    _C.check(lib.qf_resort_samples(P(src["index_ray"]), P(src["depth"]), n, P(src["points"]),
                                   P(src["origins"]), P(src["vectors"]), P(src["index_tri"]),
                                   P(out.perm), P(out.points), P(out.depth), P(out.origins), P(out.vectors), P(out.tri),
                                   P(out.boundary), P(inv), P(out.points_c), P(out.vectors_c), _C.stream()), "qf_resort_samples")
    host = {name: a.cpu().numpy() for name, a in vars(out).items() if a is not None}
    for name, src in (("points", "points"), ("depth", "depth"), ("origins", "origins"), ("vectors", "vectors"), ("tri", "index_tri")):
        assert _same(host[name][:n], c[src][perm_want]), name
    if want_perm:
        assert np.array_equal(host["perm"][:n], perm_want)
    if want_bnd:
        assert np.array_equal(host["boundary"][:n], c["boundary"]) and (host["boundary"][n:] == 77).all()
    if want_inv:
        assert _same(host["points_c"][:n][c["inverse"]], c["points"][perm_want])
        assert _same(host["vectors_c"][:n][c["inverse"]], c["vectors"][perm_want])
    for name, a in host.items():
        if name != "boundary":
            assert np.isnan(a[n:]).all() if a.dtype == np.float32 else (a[n:] == SENT_TRI).all(), name


# ------------------------------------------------------------------------------------------------ (e) through the policy
_MI, _WANT = {}, {}


def _policy_mi(k, rule):
    from quadraturefields_amd.mesh_utils import MeshIntersection
    if (k, rule) not in _MI:
        _MI[k, rule] = MeshIntersection(ll.mesh(), simplify_mesh=False, scale=1.0, num_intersections=k, min_hit_separation=rule)
    return _MI[k, rule]


def _reset_policy(ri, wide=0, slabs=0, upfront=0):
    """The policy's state, set by hand: which camera-coherent pass the next frame takes."""
    ri._settle_deferred_policy()
    ri._policy_seeded, ri._raster_backoff, ri._raster_streak, ri._raster_trying = True, 0, 0, False
    ri.raster_wide, ri.raster_slabs, ri._rule_upfront, ri._rule_pending = wide, slabs, upfront, None


def _oracle_samples(name, k, rule):
    if (name, k, rule) not in _WANT:
        view = ll.rays(name)
        brute = om.BruteForceIntersector(ll.vertices(), ll.mesh().faces, min_separation=rule)
        _WANT[name, k, rule] = om.to_loader_tensors(om.sampling_raytrace_numpy(brute, view.d, view.o, k))
    return _WANT[name, k, rule]


@pytest.mark.parametrize("route", ["bvh", "bvh image", "plain", "wide", "slabs", "masks"])
@pytest.mark.parametrize("rule", ["trimesh", RULE])
@pytest.mark.parametrize("k", [40, 64])
@pytest.mark.parametrize("name", FRAME_NAMES)
def test_sampling_raytrace_device_on_every_route(device, name, k, rule, route):
    """``MeshIntersection.sampling_raytrace_device`` against ``sampling_raytrace_numpy`` on the brute force: six tensors,
    bit for bit, whichever pass answered."""
    view, mi = ll.frame(name), _policy_mi(k, rule)
    ri = mi.rayintersector
    o, d = _dev(view, device)
    wide = min(ri.RASTER_WIDE_FACTOR * k, ri.RASTER_WIDE_MAX)
    assert wide > k
    _reset_policy(ri, **{"bvh": {}, "bvh image": {}, "plain": {}, "wide": dict(wide=wide), "slabs": dict(wide=wide, slabs=3),
                         "masks": dict(upfront=1)}[route])
    redone = ri.rule_redone_frames
    if route == "bvh":
        got = mi.sampling_raytrace_device(d, o)
    elif route == "bvh image":
        got = mi.sampling_raytrace_device(d, o, image_width=view.w)
    else:
        got = mi.sampling_raytrace_device(d, o, camera=view.cam)
    assert ri.last_route == {"bvh image": "bvh", "masks": "plain"}.get(route, route)
    assert ri.camera_mismatch_frames == 0
    if route == "masks":
        assert ri._rule_upfront == 0 and ri.rule_redone_frames == redone      # decided up front: not packed twice
    elif route in ("plain", "wide", "slabs") and rule == RULE:
        assert ri.rule_redone_frames == redone + 1                            # the optimistic pack was refuted and redone
    want = _oracle_samples(name, k, rule)
    for what, g, w in zip(["xyzs", "dirs", "index_ray", "ts", "index_tri", "origins"], got, want):
        assert _same(g.cpu().numpy(), w.numpy()), what
    assert int(torch.bincount(want[2]).max()) > (32 if rule == RULE else k - 1)


def test_rendered_frame_at_k_40(device):
    """One frame through ``FrameRenderer.render`` at K = 40 against the oracle's render of the brute force's samples, with
    the tolerance of tests/test_gpu_render.py (per-pixel |rgb - oracle| <= 2e-4, PSNR >= 70 dB).  Above K = 32 there are no
    hit bins: the frame is the lists pipeline, not the K = 25 one the benchmark runs."""
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceField
    from quadraturefields_amd import synthetic
    from quadraturefields_amd.render import FrameRenderer, psnr
    from tests import helpers
    k, view = 40, ll.frame("aligned")
    mi = _policy_mi(k, "trimesh")
    _reset_policy(mi.rayintersector)
    field = NGPRadianceField(aabb=[-1.5] * 3 + [1.5] * 3, log2_hashmap_size=14)
    field.load_state_dict(synthetic.seeded_ngp_state(14, field.mlp_base.grid.n_rows), strict=False)
    field = field.to(device)
    o, d = _dev(view, device)
    rgb, alpha, depth, n = FrameRenderer(mi, field).render(o, d, camera=view.cam)
    assert mi.rayintersector.last_route in ("plain", "frame"), mi.rayintersector.last_route
    data_o = _oracle_samples("aligned", k, "trimesh")
    assert n == data_o[0].shape[0]
    rgb_o, alpha_o, dep_o = om.render_image_finetune(helpers.oracle_ngp_weights(field), None, data_o, view.n)[:3]
    err = (rgb.reshape(-1, 3).cpu() - rgb_o).abs().max().item()
    print("max |rgb - oracle| at K = 40:", err)
    assert err <= 2e-4, err
    assert psnr(rgb.reshape(-1, 3).cpu(), rgb_o) >= 70.0
    assert torch.allclose(alpha.reshape(-1, 1).cpu(), alpha_o, atol=2e-4)
