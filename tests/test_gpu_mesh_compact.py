"""GPU: mesh clean-up (``mc_utils.compact_mesh_device`` / ``qf_mesh_compact_*``) and the visibility
mask (``qf_mark_hit_faces``, ``mc_utils.prunning_mesh_train_visibility``) against their numpy restatement
(tests/mesh_compact_reference.py).  Every comparison is exact: faces, vertices (by bits), maps and counts."""
import itertools
import os

import numpy as np
import pytest
import torch

from tests import mesh_compact_reference as ref
from tests import stream_harness as sh
from tests import vertex_baked_reference as R
from tests.test_mesh_compact_host import HAND_CASES, HAND_FACES, HAND_VERTS

pytestmark = pytest.mark.gpu

ALL = dict(remove_degenerate=True, remove_duplicates=True, remove_unreferenced=True)
SIZES = (0, 1, 63, 64, 65, 1023, 1025, 4097)
_cache = {}


def _mc():
    from quadraturefields_amd import mc_utils
    return mc_utils


def _device_run(v, f, keep=None, **options):
    out = _mc().compact_mesh_device(torch.from_numpy(np.asarray(v, np.float64)).cuda(),
                                    torch.from_numpy(np.asarray(f, np.int64).reshape(-1, 3)).cuda(),
                                    None if keep is None else torch.from_numpy(np.asarray(keep)).cuda(), **options)
    torch.cuda.synchronize()
    assert out.vertices.dtype == torch.float64 and out.vertices.is_cuda
    assert out.faces.dtype == out.face_map.dtype == out.vertex_map.dtype == torch.int64
    return out


def _assert_matches(v, f, keep=None, **options):
    """The device result equals the restatement: returns (device record, reference counts)."""
    got = _device_run(v, f, keep, **options)
    rv, rf, rfm, rvm, rc = ref.compact(v, f, keep, **options)
    assert torch.equal(got.faces.cpu(), torch.from_numpy(rf)), options
    assert torch.equal(got.face_map.cpu(), torch.from_numpy(rfm)), options
    assert torch.equal(got.vertex_map.cpu(), torch.from_numpy(rvm)), options
    assert got.vertices.shape == rv.shape
    assert torch.equal(got.vertices.cpu().view(torch.int64), torch.from_numpy(rv).view(torch.int64)), options
    assert torch.equal(torch.tensor(list(got.stats.values())), torch.from_numpy(rc)), (got.stats, rc)
    assert list(got.stats) == list(ref.COUNT_NAMES)
    return got, rc


# --------------------------------------------------------------------------------------------------------- 1. the rules
@pytest.mark.parametrize("name", sorted(HAND_CASES))
def test_hand_worked_case(device, name):
    keep, options, faces, face_map, vertex_map, counts = HAND_CASES[name]
    got = _device_run(HAND_VERTS, HAND_FACES, keep, **options)
    assert got.faces.tolist() == [list(t) for t in faces]
    assert got.face_map.tolist() == face_map and got.vertex_map.tolist() == vertex_map
    assert list(got.stats.values()) == counts
    _assert_matches(HAND_VERTS, HAND_FACES, keep, **options)


def _patterned_mesh(n_v, n_f, seed):
    """Faces over vertices 1 .. n_v - 2 only (vertex 0 and n_v - 1 are unreferenced, and so is a long run in the middle),
    with a keep mask of long kept and dropped runs that cross the 1 024-item scan blocks."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n_v, 3))
    v[n_v // 2] = [np.nan, np.inf, -0.0]                   # coordinates are copied, never read
    if n_f == 0 or n_v < 4:
        f = np.zeros((n_f, 3), np.int64) + (1 if n_v > 1 else 0)
        f = np.minimum(f, n_v - 1)
    else:
        lo_run, hi_run = n_v // 3, n_v // 3 + max(n_v // 4, 1)   # a run of vertices nobody uses
        pool = np.array([i for i in range(1, n_v - 1) if not lo_run <= i < hi_run] or [1])
        f = pool[rng.integers(0, len(pool), size=(n_f, 3))]
    keep = np.ones(n_f, np.uint8)
    for start in range(0, n_f, 700):                       # runs of 350 dropped, 350 kept
        keep[start:start + 350] = 0
    keep[-1:] = 1
    return v, f, keep


@pytest.mark.parametrize("n_f", SIZES)
def test_face_counts_around_block_and_wave_edges(device, n_f):
    v, f, keep = _patterned_mesh(1500, n_f, seed=n_f)
    _assert_matches(v, f, keep, **ALL, min_component_faces=0)
    _assert_matches(v, f, None, remove_unreferenced=True)
    _assert_matches(v, f, keep, remove_unreferenced=False)


@pytest.mark.parametrize("n_v", SIZES[1:])
def test_vertex_counts_around_block_and_wave_edges(device, n_v):
    v, f, keep = _patterned_mesh(n_v, 2500, seed=100 + n_v)
    got, rc = _assert_matches(v, f, keep, **ALL, min_component_faces=0)
    if n_v >= 63:
        vm = got.vertex_map.cpu().numpy()
        assert 0 not in vm and n_v - 1 not in vm and rc[1] < n_v
    _assert_matches(v, f, None, remove_duplicates=True)


def _random_mesh(n_v, n_f, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n_v, 3)), rng.integers(0, n_v, size=(n_f, 3)), (rng.random(n_f) < 0.6).astype(np.uint8)


def _soup(seed=7, n_v=5000, n_f=20000):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n_v, 3))
    f = rng.integers(0, n_v, size=(n_f, 3))
    f[1000:1200] = f[3000:3200][:, [1, 2, 0]]              # rotated duplicates whose first copy comes later ...
    f[5000:5200] = f[200:400][:, [0, 2, 1]]                # ... and earlier; opposite windings
    f[7000:7100] = f[200:300][:, [2, 0, 1]]                # triples of copies (200..300, 5000..5100, 7000..7100)
    f[9000:9100, 1] = f[9000:9100, 0]                      # (a, a, b)
    f[9100:9150] = f[9100:9150, :1]                        # (a, a, a)
    f[9150:9170] = f[9000:9020][:, [2, 1, 0]]              # duplicates of degenerate faces
    keep = (rng.random(n_f) < 0.6).astype(np.uint8)
    keep[200:250] = 0                                      # duplicates whose first copy is masked out
    keep[5000:5050] = 1
    keep[7000:7050] = 1
    return v, f, keep


@pytest.mark.parametrize("degenerate,duplicates,unreferenced", list(itertools.product((False, True), repeat=3)))
def test_every_flag_combination_on_a_random_soup(device, degenerate, duplicates, unreferenced):
    v, f, keep = _soup()
    options = dict(remove_degenerate=degenerate, remove_duplicates=duplicates, remove_unreferenced=unreferenced)
    for mask, m in ((keep, 0), (keep, 3), (None, 2)):
        got, rc = _assert_matches(v, f, mask, **options, min_component_faces=m)
        if duplicates and mask is not None:
            fm = set(got.face_map.tolist())
            assert not fm & set(range(200, 250))           # masked out ...
            if m == 0:
                assert set(range(5000, 5050)) <= fm            # ... so the next copy is the survivor
                assert not fm & set(range(7000, 7050))
        assert rc[4] > 0 if duplicates else rc[4] == 0
        assert rc[3] > 0 if degenerate else rc[3] == 0


# --------------------------------------------------------------------------------------------------------- 2. components
def test_long_strip_with_shuffled_ids(device):
    """3 000 faces in one chain, vertex ids and face order shuffled: the chain crosses every workgroup."""
    rng = np.random.default_rng(11)
    n = 3000
    ids = rng.permutation(n + 2 + 500)[:n + 2]            # 500 further vertices stay unreferenced
    f = np.stack([ids[:-2], ids[1:-1], ids[2:]], axis=1)[rng.permutation(n)]
    v = rng.normal(size=(n + 502, 3))
    got, rc = _assert_matches(v, f, None, **ALL, min_component_faces=n)
    assert rc[6] == 1 and rc[0] == n and rc[5] == 0
    got, rc = _assert_matches(v, f, None, **ALL, min_component_faces=n + 1)
    assert rc[0] == 0 and rc[5] == n and rc[1] == 0
    # cut in the middle by the mask: two components of 1 499 and 1 498 faces (the cut face's neighbours share no vertex
    # across it only when three consecutive faces go)
    keep = np.ones(n, np.uint8)
    order = {tuple(t): i for i, t in enumerate(map(tuple, f))}
    for j in (1499, 1500, 1501):
        keep[order[(ids[j], ids[j + 1], ids[j + 2])]] = 0
    got, rc = _assert_matches(v, f, keep, **ALL, min_component_faces=1499)
    assert rc[6] == 2 and rc[0] == 1499 and rc[5] == 1498


def test_fan_around_one_vertex(device):
    """5 000 faces share vertex 9 999 (the largest id, so every union moves the hot root's tree)."""
    n = 5000
    rim = np.random.default_rng(2).permutation(n)
    hub = 2 * n - 1
    f = np.stack([np.full(n, hub), rim, n + (rim * 7) % (n - 1)], axis=1)
    v = np.zeros((2 * n, 3))
    got, rc = _assert_matches(v, f, None, **ALL, min_component_faces=2)
    assert rc[6] == 1
    _assert_matches(v, f[:, [1, 0, 2]], None, min_component_faces=n + 1)


def test_bodies_joined_only_by_a_dropped_face(device):
    a = np.array([[0, 1, 2], [1, 2, 3], [2, 3, 4]])               # body A: 3 faces
    b = a + 10                                                     # body B: 3 faces
    v = np.zeros((20, 3))
    for name, bridge, keep, options in (
            ("masked", [[4, 10, 11]], [1] * 6 + [0], {}),
            ("degenerate", [[4, 4, 10]], None, dict(remove_degenerate=True))):
        f = np.concatenate([a, b, np.array(bridge)])
        got, rc = _assert_matches(v, f, keep, min_component_faces=2, **options)
        assert rc[6] == 2 and rc[0] == 6, name
    # with the degenerate flag off the same face joins them
    f = np.concatenate([a, b, np.array([[4, 4, 10]])])
    got, rc = _assert_matches(v, f, None, min_component_faces=2)
    assert rc[6] == 1 and rc[0] == 7
    # the bridge twice: the copy goes, the first joins them; with the first masked out the copy stays and joins them;
    # with both masked out they fall apart, and at M = 4 both bodies go
    f = np.concatenate([a, b, np.array([[4, 10, 11], [11, 4, 10]])])
    for keep, faces, dropped in (([1] * 8, [0, 1, 2, 3, 4, 5, 6], 1), ([1] * 6 + [0, 1], [0, 1, 2, 3, 4, 5, 7], 0)):
        got, rc = _assert_matches(v, f, keep, remove_duplicates=True, min_component_faces=4)
        assert rc[6] == 1 and got.face_map.tolist() == faces and rc[4] == dropped
    got, rc = _assert_matches(v, f, [1] * 6 + [0, 0], remove_duplicates=True, min_component_faces=4)
    assert rc[6] == 2 and rc[0] == 0 and rc[5] == 6


@pytest.mark.parametrize("m", [2, 5, 64, 65])
def test_islands_of_exactly_m_minus_one_and_m_faces(device, m):
    def strip(n, base):
        i = np.arange(n) + base
        return np.stack([i, i + 1, i + 2], axis=1)
    f = np.concatenate([strip(m - 1, 0), strip(m, 200), strip(m + 1, 400), strip(1, 600)])
    rng = np.random.default_rng(m)
    f = f[rng.permutation(len(f))]
    got, rc = _assert_matches(rng.normal(size=(700, 3)), f, None, **ALL, min_component_faces=m)
    assert rc[6] == 4 and rc[0] == 2 * m + 1 and rc[5] == m
    assert int(got.vertex_map.min()) == 200


# ----------------------------------------------------------------------------------------------------------- 3. refusals
def test_invalid_index_raises_with_the_count_and_writes_nothing(device):
    from quadraturefields_amd import _C
    v, f, keep = _random_mesh(600, 2000, 1)
    f[17, 1], f[1500, 2], f[1999, 0] = 600, -1, 2 ** 40
    with pytest.raises(ValueError, match=r"\b3 faces have an index outside \[0, 600\)"):
        _device_run(v, f, keep, **ALL)
    # the entry points themselves: counts[7] alone, and emit leaves the buffers as they were
    vd, fd = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    lib = _C.lib()
    ws_bytes = int(lib.qf_mesh_compact_workspace_bytes(600, 2000))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=device)
    counts = torch.full((8,), -5, dtype=torch.int64, device=device)
    args = (_C.ptr(vd), 600, _C.ptr(fd), 2000, None, 7, 2, _C.ptr(ws), ws_bytes)
    _C.check(lib.qf_mesh_compact_count(*args, _C.ptr(counts), _C.stream()), "count")
    assert counts.tolist() == [0, 0, 0, 0, 0, 0, 0, 3]
    ov = torch.full((600, 3), -7.0, dtype=torch.float64, device=device)
    of = torch.full((2000, 3), -7, dtype=torch.int64, device=device)
    fm, vm = torch.full((2000,), -7, dtype=torch.int64, device=device), torch.full((600,), -7, dtype=torch.int64, device=device)
    _C.check(lib.qf_mesh_compact_emit(*args, _C.ptr(ov), 600, _C.ptr(of), 2000, _C.ptr(fm), _C.ptr(vm), _C.stream()), "emit")
    torch.cuda.synchronize()
    assert bool((ov == -7).all()) and bool((of == -7).all()) and bool((fm == -7).all()) and bool((vm == -7).all())


def test_bad_sizes_and_flags_return_the_status_before_any_launch(device):
    from quadraturefields_amd import _C
    lib = _C.lib()
    v, f, _ = _random_mesh(100, 50, 2)
    vd, fd = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    need = int(lib.qf_mesh_compact_workspace_bytes(100, 50))
    ws = torch.empty((need,), dtype=torch.uint8, device=device)
    counts = torch.full((8,), -5, dtype=torch.int64, device=device)

    def count(V=100, F=50, flags=7, m=0, ws_bytes=need, vp=_C.ptr(vd), fp=_C.ptr(fd), wp=_C.ptr(ws), cp=_C.ptr(counts)):
        return lib.qf_mesh_compact_count(vp, V, fp, F, None, flags, m, wp, ws_bytes, cp, _C.stream())

    for bad in (dict(V=0), dict(V=2 ** 31), dict(F=-1), dict(F=2 ** 31), dict(flags=8), dict(flags=16 | 7), dict(m=-1),
                dict(m=2 ** 31), dict(ws_bytes=need - 1), dict(vp=None), dict(fp=None), dict(wp=None), dict(cp=None)):
        assert count(**bad) == -1, bad
    torch.cuda.synchronize()
    assert counts.tolist() == [-5] * 8                     # nothing ran
    assert count() == 0
    assert lib.qf_mesh_compact_emit(_C.ptr(vd), 100, _C.ptr(fd), 50, None, 7, 0, _C.ptr(ws), need, None, 1, None, 0, None,
                                    None, _C.stream()) == -1
    assert lib.qf_mesh_compact_emit(_C.ptr(vd), 100, _C.ptr(fd), 50, None, 7, 0, _C.ptr(ws), need, _C.ptr(vd), 101, None, 0,
                                    None, None, _C.stream()) == -1
    with pytest.raises(ValueError):
        _mc().compact_mesh_device(vd, fd, torch.ones(49, dtype=torch.uint8, device=device))
    # the maps may be NULL and a capacity may be short: rows beyond it are not written
    c = counts.tolist()
    ov = torch.full((c[1], 3), -7.0, dtype=torch.float64, device=device)
    of = torch.full((c[0], 3), -7, dtype=torch.int64, device=device)
    _C.check(lib.qf_mesh_compact_emit(_C.ptr(vd), 100, _C.ptr(fd), 50, None, 7, 0, _C.ptr(ws), need, _C.ptr(ov), c[1] - 3,
                                      _C.ptr(of), c[0] - 2, None, None, _C.stream()), "emit")
    want = ref.compact(v, f, None, **ALL)
    assert torch.equal(of[:-2].cpu(), torch.from_numpy(want[1][:-2])) and bool((of[-2:] == -7).all())
    assert torch.equal(ov[:-3].cpu(), torch.from_numpy(want[0][:-3])) and bool((ov[-3:] == -7).all())


# -------------------------------------------------------------------------------------------------------- 4. determinism
def test_two_runs_give_identical_bytes(device):
    v, f, keep = _soup(seed=9)
    runs = [_device_run(v, f, keep, **ALL, min_component_faces=3) for _ in range(2)]
    for a, b in zip(runs[0][:4], runs[1][:4]):
        assert sh.same_bits(a, b)
    assert runs[0].stats == runs[1].stats


def _stream_mesh(seed, device):
    """Same faces in both sets; the vertices (values) and the keep mask (named in ``varies``) differ."""
    v, f, _ = _random_mesh(3000, 9000, 21)
    rng = np.random.default_rng(seed)
    return dict(vertices=torch.from_numpy(rng.normal(size=v.shape)).to(device), faces=torch.from_numpy(f).to(device),
                keep=torch.from_numpy((rng.random(9000) < 0.5).astype(np.uint8)).to(device))


def _count_build(seed, device):
    from quadraturefields_amd import _C
    d = _stream_mesh(seed, device)
    n = int(_C.lib().qf_mesh_compact_workspace_bytes(3000, 9000))
    d.update(tmp_ws=torch.zeros((n,), dtype=torch.uint8, device=device), out_counts=torch.zeros((8,), dtype=torch.int64, device=device))
    return d


def _count_call(i):
    from quadraturefields_amd import _C
    _C.check(_C.lib().qf_mesh_compact_count(_C.ptr(i["vertices"]), 3000, _C.ptr(i["faces"]), 9000, _C.ptr(i["keep"]), 7, 3,
                                            _C.ptr(i["tmp_ws"]), i["tmp_ws"].shape[0], _C.ptr(i["out_counts"]), _C.stream()),
             "qf_mesh_compact_count")
    return (i["out_counts"],)


def _emit_build(seed, device):
    d = _count_build(seed, device)
    d.update(out_v=torch.zeros((3000, 3), dtype=torch.float64, device=device),
             out_f=torch.zeros((9000, 3), dtype=torch.int64, device=device),
             out_fm=torch.zeros((9000,), dtype=torch.int64, device=device),
             out_vm=torch.zeros((3000,), dtype=torch.int64, device=device))
    return d


def _emit_call(i):
    """Count, then emit at full capacity with no host wait in between: the rows beyond the counts keep the sentinel."""
    from quadraturefields_amd import _C
    _count_call(i)
    _C.check(_C.lib().qf_mesh_compact_emit(_C.ptr(i["vertices"]), 3000, _C.ptr(i["faces"]), 9000, _C.ptr(i["keep"]), 7, 3,
                                           _C.ptr(i["tmp_ws"]), i["tmp_ws"].shape[0], _C.ptr(i["out_v"]), 3000,
                                           _C.ptr(i["out_f"]), 9000, _C.ptr(i["out_fm"]), _C.ptr(i["out_vm"]), _C.stream()),
             "qf_mesh_compact_emit")
    return i["out_v"], i["out_f"], i["out_fm"], i["out_vm"], i["out_counts"]


def _mark_build(seed, device):
    g = torch.Generator().manual_seed(seed)
    tri = torch.randint(-1, 5000, (20000, 5), generator=g, dtype=torch.int32)
    return dict(hit_tri=tri.to(device), hit_count=torch.randint(0, 7, (20000,), generator=torch.Generator().manual_seed(5),
                                                                dtype=torch.int32).to(device),
                acc_mask=torch.zeros((4000,), dtype=torch.uint8, device=device),
                acc_bad=torch.zeros((1,), dtype=torch.int64, device=device))


def _mark_call(i):
    _mc().mark_hit_faces(i["hit_tri"], i["hit_count"], i["acc_mask"], i["acc_bad"])
    return i["acc_mask"], i["acc_bad"]


STREAM_CASES = [
    sh.Case("mesh_compact_count", _count_build, _count_call, varies=("keep",), entry_points=("qf_mesh_compact_count",)),
    sh.Case("mesh_compact_emit", _emit_build, _emit_call, varies=("keep",), entry_points=("qf_mesh_compact_emit",)),
    sh.Case("mark_hit_faces", _mark_build, _mark_call, varies=("hit_tri",), entry_points=("qf_mark_hit_faces",)),
]


def test_every_device_entry_point_has_a_stream_case():
    from quadraturefields_amd import _C
    covered = sorted(ep for c in STREAM_CASES for ep in c.entry_points)
    assert covered == sorted(set(_C._MESH_COMPACT_SIGNATURES) - {"qf_mesh_compact_workspace_bytes"})
    assert not any(c.host_wait for c in STREAM_CASES)


@pytest.mark.parametrize("name", [c.name for c in STREAM_CASES])
def test_entry_point_runs_entirely_on_the_callers_stream(device, lib, name):
    case = {c.name: c for c in STREAM_CASES}[name]
    issue_ms, delay_ms = sh.run_case(case, device)
    print(f"{name}: issue {issue_ms:.3f} ms, delay {delay_ms:.0f} ms")


def test_wrapper_on_a_side_stream_gives_the_same_bytes(device):
    v, f, keep = _soup(seed=9)
    want = _device_run(v, f, keep, **ALL, min_component_faces=3)
    s = torch.cuda.Stream(device=device)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        got = _device_run(v, f, keep, **ALL, min_component_faces=3)
    for a, b in zip(got[:4], want[:4]):
        assert sh.same_bits(a, b)
    assert got.stats == want.stats


# ---------------------------------------------------------------------------------------------------- 5. mark_hit_faces
def test_mark_hit_faces_matches_numpy(device):
    rng = np.random.default_rng(4)
    n_rays, k, n_faces = 4099, 5, 3001
    tri = rng.integers(0, n_faces, size=(n_rays, k)).astype(np.int32)
    filled = rng.integers(0, k + 1, size=n_rays)
    tri[np.arange(k)[None, :] >= filled[:, None]] = -1            # -1 padding
    tri[rng.integers(0, n_rays, 40), 0] = n_faces + rng.integers(0, 5, 40)      # ids beyond the mesh
    tri[5, 0], tri[6, 0] = 2 ** 31 - 1, -2 ** 31
    count = np.minimum(filled, rng.integers(0, k + 3, size=n_rays)).astype(np.int32)     # smaller than the filled slots
    count[:50] = k + 4                                              # beyond max_hits: clamped, the padding is then counted
    t, c = torch.from_numpy(tri).to(device), torch.from_numpy(count).to(device)
    for hc, hc_np in ((c, count), (None, None)):
        mask = torch.zeros((n_faces,), dtype=torch.uint8, device=device)
        bad = torch.zeros((1,), dtype=torch.int64, device=device)
        _mc().mark_hit_faces(t, hc, mask, bad)
        want, want_bad = ref.mark_hit_faces(tri, hc_np, n_faces)
        assert torch.equal(mask.cpu(), torch.from_numpy(want)) and int(bad.item()) == want_bad and want_bad > 0
        assert 0 < int(mask.sum()) < n_faces
    # two views accumulate into one mask (bool masks are accepted), and the counter is added to
    tri2 = rng.integers(-1, n_faces, size=(777, 3)).astype(np.int32)
    mask_b = mask.clone().to(torch.bool)
    _mc().mark_hit_faces(torch.from_numpy(tri2).to(device), None, mask_b, bad)
    want2, bad2 = ref.mark_hit_faces(tri2, None, n_faces, mask=want)
    assert torch.equal(mask_b.cpu().to(torch.uint8), torch.from_numpy(want2)) and int(bad.item()) == want_bad + bad2
    assert int(want2.sum()) > int(want.sum())
    # no out_of_range counter, no rays
    _mc().mark_hit_faces(t, None, mask, None)
    _mc().mark_hit_faces(t[:0], None, mask, None)


# ---------------------------------------------------------------------------------------------- 6. end-to-end visibility
def _visibility_scene(device):
    from quadraturefields_amd import synthetic
    from quadraturefields_amd.datasets.utils import Rays
    if "vis" not in _cache:
        mesh = synthetic.shell_mesh()
        focal = synthetic.lego_focal(64)
        items = []
        for c2w in synthetic.orbit_cameras(3, seed=8):
            o, d = synthetic.camera_rays(c2w, focal, 64, 64, device=device)
            items.append({"rays": Rays(origins=o.reshape(64, 64, 3), viewdirs=d.reshape(64, 64, 3))})
        _cache["vis"] = (mesh, items)
    return _cache["vis"]


def test_visibility_pruning_equals_the_reference_shaped_loop(device):
    from quadraturefields_amd.mesh_utils import MeshIntersection, RayIntersector
    mesh, items = _visibility_scene(device)
    n_f = mesh.faces.shape[0]
    # the reference-shaped loop: the intersector's ids per view, np.unique, then the numpy rules
    ri = RayIntersector(mesh, max_hits=5, device=device)
    seen = []
    for item in items:
        ids = ri.hits(item["rays"].origins.reshape(-1, 3), item["rays"].viewdirs.reshape(-1, 3), 5)[0].cpu().numpy().flatten()
        seen.append(np.unique(ids[ids >= 0]))
    want_mask = np.zeros(n_f, dtype=bool)
    want_mask[np.unique(np.concatenate(seen))] = True
    assert 100 < want_mask.sum() < n_f // 2
    wv, wf, _, wvm, _ = ref.compact(mesh.vertices, mesh.faces, want_mask, remove_duplicates=True, remove_unreferenced=True)

    cleaned, mask = _mc().prunning_mesh_train_visibility(mesh, items, max_hits=5)
    assert mask.dtype == np.bool_ and np.array_equal(mask, want_mask)
    assert np.array_equal(cleaned.faces, wf) and np.array_equal(cleaned.vertices.view(np.int64), wv.view(np.int64))
    assert np.array_equal(cleaned.visual.uv, mesh.visual.uv[wvm])
    assert mesh.faces.shape[0] == n_f                      # the input is left alone

    # an existing MeshIntersection is used as it is; the complement's two halves partition the faces
    mi = MeshIntersection(mesh, simplify_mesh=False, num_intersections=5, device=device)
    vis, inv, mask_c = _mc().prunning_mesh_train_visibility_complement(mi, items, max_hits=5)
    assert np.array_equal(mask_c, want_mask)
    assert np.array_equal(vis.faces, mesh.faces[want_mask]) and np.array_equal(inv.faces, mesh.faces[~want_mask])
    assert len(vis.faces) + len(inv.faces) == n_f
    assert np.array_equal(vis.vertices, mesh.vertices) and np.array_equal(inv.vertices, mesh.vertices)


# ------------------------------------------------------------------------------------------------- 7. nothing else moves
def _padded_mesh():
    """The scenes' shell mesh with unreferenced vertices added: one at index 0, one at the end and a run in the middle."""
    from quadraturefields_amd.mesh_io import TriMesh
    if "padded" not in _cache:
        m = R.mesh()
        n = m.vertices.shape[0]
        rng = np.random.default_rng(6)
        cut = n // 2
        new_index = np.concatenate([np.arange(cut) + 1, np.arange(cut, n) + 1 + 300])
        v = rng.normal(size=(n + 302, 3)) * 5.0
        uv = rng.random((n + 302, 2))
        v[new_index], uv[new_index] = m.vertices, m.visual.uv
        _cache["padded"] = (TriMesh(v, new_index[m.faces], uv), new_index)
    return _cache["padded"]


def _frame(mesh, device, table=None):
    """A 64 x 64, K = 5 frame of ``mesh``: (hit counts, pixels) of ``FrameRenderer.render`` or, with a table, the
    pixels of ``render_vertex_baked``."""
    from quadraturefields_amd.mesh_utils import MeshIntersection, make_camera
    from quadraturefields_amd.render import FrameRenderer
    c2w, focal, o, d = R.camera(64, 64)
    o, d = o.to(device), d.to(device)
    cam = make_camera(c2w, focal, 64, 64)
    mi = MeshIntersection(mesh, simplify_mesh=False, scale=1.0, num_intersections=5, device=device)
    fr = FrameRenderer(mi, R.sg_field(2, device))
    if table is not None:
        out = fr.render_vertex_baked(o, d, table, camera=cam)
        return [t.clone() for t in out[:3]]
    rgb, alpha, depth, n = fr.render(o, d, camera=cam)
    hit_tri, _, hit_count, _, _ = mi.rayintersector.hits(o, d, 5, camera=cam)
    return hit_count.clone(), hit_tri.clone(), [rgb.clone(), alpha.clone(), depth.clone()], n


def test_removing_unreferenced_vertices_changes_no_pixel(device):
    from quadraturefields_amd import baking
    from quadraturefields_amd.mesh_utils import MeshIntersection
    padded, new_index = _padded_mesh()
    cleaned, face_map, vertex_map = _mc().compact_mesh(padded)
    assert np.array_equal(vertex_map, new_index) and np.array_equal(face_map, np.arange(len(padded.faces)))
    assert np.array_equal(cleaned.vertices[cleaned.faces], padded.vertices[padded.faces])      # the same triangle soup
    assert np.array_equal(cleaned.visual.uv, padded.visual.uv[vertex_map])
    count_a, tri_a, img_a, n_a = _frame(padded, device)
    count_b, tri_b, img_b, n_b = _frame(cleaned, device)
    assert n_a == n_b and n_a > 0 and torch.equal(count_a, count_b) and torch.equal(tri_a, tri_b)
    for a, b in zip(img_a, img_b):
        assert sh.same_bits(a, b)
    # the vertex-baked table follows the vertices through the map
    mi = MeshIntersection(padded, simplify_mesh=False, scale=1.0, num_intersections=5, device=device)
    table = baking.bake_vertex_features(R.sg_field(2, device), mi)
    small = baking.remap_vertex_features(table, vertex_map)
    assert small.shape == (len(vertex_map), table.shape[1])
    for a, b in zip(_frame(padded, device, table), _frame(cleaned, device, small)):
        assert sh.same_bits(a, b)
    module = baking.remap_vertex_features(baking.VertexBakedFeatures(table), vertex_map)
    for a, b in zip(_frame(padded, device, table), _frame(cleaned, device, module)):
        assert sh.same_bits(a, b)


def test_triangle_ids_map_back_through_face_map(device):
    from quadraturefields_amd.mesh_io import TriMesh
    padded, _ = _padded_mesh()
    keep = np.random.default_rng(12).random(len(padded.faces)) < 0.7
    cleaned, face_map, vertex_map = _mc().compact_mesh(padded, keep, min_component_faces=2)
    assert 0 < len(face_map) <= keep.sum() and len(vertex_map) < len(padded.vertices)
    # the same faces with every vertex kept: the same soup, so the same lists
    uncompacted = TriMesh(padded.vertices, padded.faces[face_map], padded.visual.uv)
    count_a, tri_a, img_a, _ = _frame(uncompacted, device)
    count_b, tri_b, img_b, _ = _frame(cleaned, device)
    assert torch.equal(count_a, count_b) and torch.equal(tri_a, tri_b)
    for x, y in zip(img_a, img_b):
        assert sh.same_bits(x, y)
    b = tri_b.cpu().numpy()
    assert (b >= 0).any()
    hit = face_map[b[b >= 0]]
    assert keep[hit].all()
    # every hit triangle of the cleaned mesh is the source face's triangle
    assert np.array_equal(cleaned.vertices[cleaned.faces[b[b >= 0]]], padded.vertices[padded.faces[hit]])


# -------------------------------------------------------------------------------------------------------- 8. the pruner
def test_pruner_defaults_are_unchanged_and_compact_equals_compact_mesh(device, tmp_path):
    from quadraturefields_amd import baking
    from quadraturefields_amd.mesh_io import load_mesh
    from quadraturefields_amd.mesh_utils import MeshIntersection
    from quadraturefields_amd.pruning import FILES, MAP_FILES, MeshPruner
    padded, _ = _padded_mesh()
    mi = MeshIntersection(padded, simplify_mesh=False, scale=1.0, num_intersections=5, device=device)
    pruner = MeshPruner(mi, R.sg_field(2, device))
    g = torch.Generator().manual_seed(3)
    pruner.triangle_weights.copy_(torch.rand(pruner.n_faces, generator=g) * 2e-3)
    keep = (pruner.triangle_weights > 1e-3).cpu().numpy()
    assert 0 < keep.sum() < len(keep)

    default = pruner.pruned_mesh()
    assert np.array_equal(default.faces, padded.faces[keep]) and np.array_equal(default.vertices, padded.vertices)
    assert np.array_equal(default.visual.uv, padded.visual.uv)
    a, b = tmp_path / "default", tmp_path / "compact"
    saved = pruner.save(str(a))
    assert sorted(os.listdir(a)) == sorted(FILES)
    assert np.array_equal(saved.faces, default.faces) and np.array_equal(saved.vertices, default.vertices)
    on_disk = load_mesh(str(a / FILES[1]))
    assert np.array_equal(on_disk.faces, default.faces) and len(on_disk.vertices) == len(padded.vertices)

    want, want_fm, want_vm = _mc().compact_mesh(default)
    got = pruner.pruned_mesh(compact=True)
    assert np.array_equal(got.faces, want.faces) and np.array_equal(got.vertices.view(np.int64), want.vertices.view(np.int64))
    assert np.array_equal(got.visual.uv, want.visual.uv) and len(got.vertices) < len(padded.vertices)
    saved = pruner.save(str(b), compact=True)
    assert sorted(os.listdir(b)) == sorted(FILES + MAP_FILES)
    assert np.array_equal(saved.faces, want.faces)
    assert np.array_equal(np.load(b / MAP_FILES[0]), np.nonzero(keep)[0][want_fm])
    assert np.array_equal(np.load(b / MAP_FILES[1]), want_vm)
    # the per-face array still describes the original mesh
    assert np.array_equal(np.load(b / FILES[0]), np.load(a / FILES[0])) and len(np.load(b / FILES[0])) == len(padded.faces)
    # islands: the same as compact_mesh with the threshold
    islands = pruner.pruned_mesh(compact=True, min_component_faces=4)
    want_i = _mc().compact_mesh(default, min_component_faces=4)[0]
    assert np.array_equal(islands.faces, want_i.faces) and np.array_equal(islands.vertices, want_i.vertices)
    with pytest.raises(TypeError, match="quantise after compaction"):
        baking.remap_vertex_features(baking.quantise_vertex_features(
            baking.bake_vertex_features(R.sg_field(2, device), mi)), want_vm)
