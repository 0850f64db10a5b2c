"""CPU: the scenes of tests/long_lists.py do what tests/test_gpu_long_lists.py needs them for, asserted from the oracle alone
(a change to ``synthetic`` cannot quietly empty the device tests), and the numpy references in that module are pinned
against the oracle they restate."""
import numpy as np
import pytest

from oracle import meshpath as om
from tests import long_lists as ll

RAYS = ["aligned", "ragged", "batch", "batch+77"]


def test_the_mesh_is_the_one_the_cases_were_measured_on():
    assert ll.mesh().faces.shape == (2880, 3)
    # the general traversal picks its child order by depth_complexity >= K / 2: the 36 shells stay below 16.5, so every
    # K > 32 runs the unordered instantiation on them; the 48 shells stay above 32, so every K <= 64 runs the ordered one
    assert 15.0 < ll.depth_complexity(ll.MESH) < 16.5
    assert ll.depth_complexity(ll.DENSE) > 33.0
    assert not any(ll.ordered(ll.MESH, k) for k in (33, 64)) and all(ll.ordered(ll.DENSE, k) for k in (33, 64))


@pytest.mark.parametrize("name", RAYS)
def test_the_share_of_rays_on_every_list_route(name):
    view = ll.rays(name)
    assert view.n == {"aligned": 1920, "ragged": 1665, "batch": 2000, "batch+77": 2077}[name]
    T = ll.truth(view)
    none, short, mid, long_, beyond = ll.crossing_shares(T.cnt)
    print(name, ll.crossing_shares(T.cnt), int(T.cnt.max()))
    assert T.cnt.max() == 72                      # a ray through the centre crosses every shell twice
    is_batch = name.startswith("batch")
    assert long_ >= (0.30 if is_batch else 0.15)  # 33..64 crossings: the insertion sorts, mask bits 32..63
    assert beyond >= (0.30 if is_batch else 0.04) # more than 64: truncation to the K nearest at every K
    assert short >= 0.10                          # ... beside short lists in the same workgroups and tiles
    assert none >= (0.02 if is_batch else 0.20)   # ... and background (the batch is aimed at the object: a few grazing rays)


@pytest.mark.parametrize("name", RAYS)
def test_the_rule_keeps_long_lists_and_drops_from_longer_ones(name):
    view = ll.rays(name)
    T, Tr = ll.truth(view), ll.truth(view, ll.RULE)
    print(name, float((Tr.cnt > 32).mean()), int(Tr.cnt.max()))
    assert (Tr.cnt > 32).mean() >= 0.03           # kept lists longer than 32: mask bits / final counts past 32
    assert Tr.cnt.max() <= 40                     # ... and short enough that K = 40 holds every kept list
    assert (T.cnt[Tr.cnt > 32] > 64).any()        # raw lists of such rays still exceed 64
    # the reference's own distance drops something too, and far less
    Tt = ll.truth(view, "trimesh")
    assert 0 < (Tt.cnt != T.cnt).sum() < 0.01 * view.n


@pytest.mark.parametrize("name", RAYS)
def test_no_two_hits_of_a_ray_tie(name):
    """"Bit for bit" must not depend on the order of equal distances (tests/test_gpu_singular_rays.py is about those)."""
    T = ll.truth(ll.rays(name))
    valid = np.arange(1, ll.ALL)[None, :] < T.cnt[:, None]
    with np.errstate(invalid="ignore"):
        gaps = np.where(valid, T.t[:, 1:] - T.t[:, :-1], np.inf)
    print(name, float(gaps.min()))
    assert gaps.min() >= 1e-4
    k = ll.keys(T.t, T.tri)
    assert (np.where(valid, k[:, 1:] > k[:, :-1], True)).all()           # ascending in (t, tri): what `keys` orders by


@pytest.mark.parametrize("name", ["aligned", "batch+77"])
@pytest.mark.parametrize("min_sep", [ll.RULE, "trimesh"])
def test_the_restated_rule_is_the_oracles(name, min_sep):
    """``apply_rule`` over the all-hits truth = the brute force run with the rule; so are the keep masks built from it."""
    view = ll.rays(name)
    T, Tr = ll.truth(view), ll.truth(view, min_sep)
    keep = ll.apply_rule(T.t, T.cnt, Tr.min_sep)
    tri, t, kept = ll.compact(keep, T.tri, T.t, pads=(-1, np.inf))
    assert np.array_equal(kept, Tr.cnt) and np.array_equal(tri, Tr.tri)
    assert np.array_equal(t.view(np.int32), Tr.t.view(np.int32))
    words = ll.mask_words(keep[:, :64])
    bit = lambda i: (words >> np.uint64(i)) & np.uint64(1)              # noqa: E731
    assert all(np.array_equal(bit(i).astype(bool), keep[:, i]) for i in (0, 31, 32, 63))


@pytest.mark.parametrize("k", [3, 33, 64])
def test_the_pack_reference_is_sampling_raytrace_numpy(k):
    """The six arrays, bit for bit, rule off and on; and from shuffled rows once they are sorted again."""
    view = ll.rays("batch+77")
    for min_sep in (0.0, ll.RULE):
        Tk = ll.first_k(ll.truth(view, min_sep), k)
        got = ll.pack_reference(view.o, view.d, Tk.tri, Tk.t, Tk.cnt)
        brute = om.BruteForceIntersector(ll.vertices(), ll.mesh().faces, min_separation=min_sep)
        want = om.to_loader_tensors(om.sampling_raytrace_numpy(brute, view.d, view.o, k))
        for name, w in zip(["xyz", "dirs", "index_ray", "depth", "index_tri", "origins"], want):
            w = w.numpy()
            if w.dtype == np.float32:
                assert np.array_equal(got[name].view(np.int32), w.view(np.int32)), name
            else:
                assert np.array_equal(got[name], w), name
    T = ll.truth(view)
    tri, t, count, n = ll.shuffled_lists(T, k, seed=1)
    assert (count[count > k] == k + 3).all() and 0 < (count > k).sum() <= (n == k).sum() // 10 + 1
    moved = (np.arange(k)[None, :] < n[:, None]) & (tri != T.tri[:, :k])
    assert k == 1 or moved.any(axis=1).mean() > 0.5                       # the rows really are out of order
    back = np.sort(ll.keys(t, tri), axis=1)
    assert np.array_equal(back, np.sort(ll.keys(T.t[:, :k], T.tri[:, :k]), axis=1))


@pytest.mark.parametrize("name", ["aligned", "ragged"])
def test_the_tile_reference_is_a_bijection_onto_the_allotted_slots(name):
    view = ll.frame(name)
    T, k = ll.truth(view), 40
    alloc = np.minimum(T.cnt, k)
    slot, base, total, gaps = ll.tile_reference(view.w, view.h, alloc, alloc)
    assert not gaps and total == alloc.sum()
    used = slot[slot >= 0]
    assert np.array_equal(np.sort(used), np.arange(total))               # every slot exactly once
    assert ((slot >= 0) == (np.arange(slot.shape[1])[None, :] < alloc[:, None])).all()
    # with the rule the tiles keep their allotment and lose samples: the gaps are what is left
    keep = ll.apply_rule(T.t[:, :k], alloc, ll.RULE)
    kept = keep.sum(axis=1)
    slot, base2, total2, gaps = ll.tile_reference(view.w, view.h, alloc, kept)
    assert np.array_equal(base, base2) and total2 == total and len(gaps) > 5
    assert sum(e - s for s, e, _ in gaps) == (alloc - kept).sum()
    free = np.concatenate([np.arange(s, e) for s, e, _ in gaps])
    assert np.array_equal(np.sort(np.concatenate([slot[slot >= 0], free])), np.arange(total))
    assert all(kept[r] > 0 for _, _, r in gaps)
    if name == "ragged":                          # 45 x 37: 5 columns of the last tile column, 5 rows of the last tile row
        assert view.w % 8 == 5 and view.h % 8 == 5


def test_the_resort_case_straddles_the_chunk_edges():
    c = ll.resort_case()
    assert c["index_ray"].size == c["n"] == c["lengths"].sum() and set(c["lengths"]) == {63, 64} and len(c["lengths"]) == 48
    assert c["n"] > 2048 + 64                     # three chunks
    local = c["start"] % 1024
    # a ray that starts on a chunk's last sample: its 64 samples end exactly with the halo
    at_edge = np.flatnonzero(local == 1023)
    assert at_edge.size == 1 and c["lengths"][at_edge[0]] == 64
    assert ((local > 960) & (local < 1023)).any() and ((local > 0) & (local < 64)).any()      # just before / just after
    assert (local == 0).any()
    d, r = c["depth"], c["index_ray"]
    same = r[1:] == r[:-1]
    assert (d[1:][same] <= d[:-1][same]).all() and (d[1:][same] == d[:-1][same]).mean() > 0.4    # reversed, with ties
    assert np.array_equal(np.sort(c["perm"]), np.arange(c["n"]))
    # stable: tied depths keep their input order
    ds, ps = d[c["perm"]], c["perm"]
    tied = (ds[1:] == ds[:-1]) & (r[c["perm"]][1:] == r[c["perm"]][:-1])
    assert tied.any() and (ps[1:][tied] > ps[:-1][tied]).all()


@pytest.mark.parametrize("k", [17, 40, 64])
def test_the_crafted_lists_tell_the_sort_and_the_rule_apart(k):
    """The scenes have no ties and no two hits exactly ``min_sep`` apart, so a sort by t alone, or a rule with >= for >,
    would pass on them.  ``tied_lists`` and ``spaced_lists`` are where those show."""
    view = ll.frame("ragged")
    T = ll.truth(view)
    Tt = ll.tied_lists(T, k)
    valid = np.arange(1, k)[None, :] < Tt.cnt[:, None]
    ties = valid & (Tt.t[:, 1:] == Tt.t[:, :-1])
    assert ties.sum() > 1000 and (Tt.tri[:, 1:] > Tt.tri[:, :-1])[ties].all()
    keys = ll.keys(Tt.t, Tt.tri)
    assert np.where(valid, keys[:, 1:] > keys[:, :-1], True).all()
    Ts = ll.spaced_lists(T, k, ll.RULE)
    keys = ll.keys(Ts.t, Ts.tri)
    assert np.where(valid, keys[:, 1:] > keys[:, :-1], True).all()
    right, wrong = ll.apply_rule(Ts.t, Ts.cnt, ll.RULE), ll.apply_rule(Ts.t, Ts.cnt, ll.RULE, strict=False)
    assert (right != wrong).any(axis=1).sum() > 100
    assert (right.sum(axis=1) > 1).mean() > 0.4
