"""CPU: the table of capped launches (``tests/grid_caps.py``) against the sources it describes, the sizes the GPU tests
derive from it, the fp64 references of ``tests/test_gpu_grid_caps.py`` against torch, and the hash construction of the
``qf_mesh_update_d`` id sets."""
import os
import re

import numpy as np
import pytest
import torch

from tests import grid_caps as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quadraturefields_amd", "csrc")
CUS = (64, 104, 256, 304)
_KEYS = [r.key for r in GC.ROWS]


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


@pytest.mark.parametrize("key", _KEYS)
def test_launch_expression_is_still_in_the_source(key):
    """A change of launch shape fails here and names the row to revisit (its cap, its test's size)."""
    row = GC.BY_KEY[key]
    assert _source(row.file).count(row.launch) == row.times, (row.key, row.file, row.launch)


def test_every_capped_launch_of_the_sources_has_a_row():
    """Every ``qf_grid_1d(`` / ``QF_SIMPLE_LAUNCH(`` line of csrc (the definitions in qf_common.h aside) lies in some
    row's launch expression, and so does every direct use of the CU count outside the dealt field kernels."""
    dealt = {"field_eval.hip", "field_eval_bf16.hip", "field_train.hip", "grid_extract.hip"}
    for name in sorted(os.listdir(CSRC)):
        if name in ("qf_common.h", "misc.cpp") or not name.endswith((".hip", ".cpp", ".h")):
            continue
        src = _source(name)
        launches = [r.launch.split("\n")[0] for r in GC.ROWS if r.file == name] + \
                   [line for r in GC.ROWS if r.file == name for line in r.launch.split("\n")]
        for line in src.split("\n"):
            capped = "qf_grid_1d(" in line or "QF_SIMPLE_LAUNCH(" in line or \
                     ("qf_cu_count_cached" in line and name not in dealt)
            if capped:
                assert any(l.strip() in line or line.strip() in l for l in launches), (name, line.strip())


@pytest.mark.parametrize("cu", CUS)
def test_past_exceeds_the_cap(cu):
    for row in GC.ROWS:
        if row.per_trip is None:
            continue
        cap, n = GC.cap_items(row, cu), GC.past(row, cu)
        assert n > cap and n % 2 == (cap + cap // 3 + 1) % 2
        if row.wg_per_cu is not None:
            trips = -(-n // row.per_trip)                       # workgroup trips over the grid of wg_per_cu * cu workgroups
            grid = row.wg_per_cu * cu
            assert grid < trips < 2 * grid                      # some workgroups take two trips, the others one
            assert n % row.per_trip or row.per_trip < 64        # the last trip is ragged


def test_caps_of_the_issue_table():
    at = lambda key: GC.cap_items(key, 256)                     # noqa: E731
    assert at("scatter_max") == 524288 and at("vertex_tiles") == 8192 and at("update_d_merged") == 2097152
    assert at("grid_march") == at("march_round_count") == 1048576 and at("adam") == 4194304 and at("vertex_train") == 524288
    assert at("derive_properties") == at("resort_samples") == 65536 * 1024


def test_every_row_has_a_verdict_and_its_test_exists():
    with open(os.path.join(ROOT, GC.NEW)) as f:
        new = f.read()
    for row in GC.ROWS:
        assert row.verdict.startswith(("covered by ", "unreachable because ")), (row.key, row.verdict)
        for name, case in re.findall(GC.NEW.replace(".", r"\.") + r"::(test_\w+)(?:\[([\w-]+)\])?", row.verdict):
            assert f"def {name}(" in new, (row.key, name)
            if case:
                assert f'"{case}"' in new, (row.key, case)


# ------------------------------------------------------------------------------------------------ the fp64 references
def test_update_d_reference_is_index_add():
    rng = np.random.default_rng(0)
    n, n_faces = 5000, 37
    d, w = (rng.standard_normal((n, 3)) * 0.01).astype(np.float32), rng.random(n).astype(np.float32)
    ids = rng.integers(-2, n_faces + 2, n)
    ref, bound, k = GC.update_d_reference(d, w, ids, n_faces)
    ok = torch.from_numpy((ids >= 0) & (ids < n_faces))
    terms = torch.cat([torch.from_numpy(d) * torch.from_numpy(w)[:, None], torch.from_numpy(w)[:, None]], dim=1)
    assert terms.dtype == torch.float32
    want = torch.zeros(n_faces, 4, dtype=torch.float64).index_add_(0, torch.from_numpy(ids)[ok], terms[ok].double())
    assert np.allclose(ref, want.numpy(), rtol=1e-13, atol=0)
    assert k.sum() == int(ok.sum()) and k.tolist() == torch.bincount(torch.from_numpy(ids)[ok], minlength=n_faces).tolist()
    # the bound holds for fp32 summation in the given order, and is not vacuous: within a factor 2^12 of the error
    got = torch.zeros(n_faces, 4).index_add_(0, torch.from_numpy(ids)[ok], terms[ok]).numpy()
    err = np.abs(got.astype(np.float64) - ref)
    assert (err <= bound).all() and (bound > 0).all() and (bound < 2.0 ** -12 * np.abs(ref).max()).all()


def test_scatter_max_reference_is_scatter_reduce_amax():
    rng = np.random.default_rng(1)
    n, n_out = 3000, 41
    v = rng.standard_normal(n).astype(np.float32)
    v[::11], v[3::17], v[5::19] = np.inf, -np.inf, -0.0
    idx = rng.integers(0, n_out - 3, n)
    for fill in (0.0, -1.0, -np.inf):
        want = torch.full((n_out,), fill).scatter_reduce(0, torch.from_numpy(idx), torch.from_numpy(v), reduce="amax")
        assert np.array_equal(GC.scatter_max_reference(fill, n_out, idx, v), want.numpy())
    # NaN values and ids out of range are skipped; -0.0 counts: max(-1, -0.0) = 0
    v[::7] = np.nan
    idx2 = idx.copy()
    idx2[::5] = n_out + 3
    idx2[1::5] = -1
    keep = ~np.isnan(v) & (idx2 >= 0) & (idx2 < n_out)
    want = torch.full((n_out,), -1.0).scatter_reduce(0, torch.from_numpy(idx2[keep]), torch.from_numpy(v[keep]), reduce="amax")
    assert np.array_equal(GC.scatter_max_reference(-1.0, n_out, idx2, v), want.numpy())
    assert GC.scatter_max_reference(-1.0, 1, np.array([0]), np.array([-0.0], np.float32)).tolist() == [0.0]


def test_segment_sums_is_index_add():
    g = torch.Generator().manual_seed(2)
    counts = torch.randint(0, 5, (300,), generator=g)
    counts[0] = counts[-1] = 0
    counts[-2] = 4
    starts = torch.cumsum(counts, 0) - counts
    x = torch.rand(int(counts.sum()), 3, generator=g)
    ridx = torch.repeat_interleave(torch.arange(300), counts)
    want = torch.zeros(300, 3, dtype=torch.float64).index_add_(0, ridx, x.double())
    assert np.allclose(GC.segment_sums(x.numpy(), starts.numpy(), counts.numpy()), want.numpy(), rtol=1e-14, atol=0)


# --------------------------------------------------------------------------------------- the ids of the update_d tests
def test_hash_is_the_kernels():
    src = _source("composite.hip")
    assert "unsigned h = ((unsigned)key * 2654435761u) >> (32 - 11);" in src
    assert "constexpr int kUdBlock = 256, kUdChunk = 1024, kUdSlots = 2048;" in src
    assert "n >= 8 * kUdChunk" in src                           # the route switch: n = 8191 plain, n = 8192 merged
    assert GC.update_d_hash([0, 1, 2 ** 31 - 1]).tolist() == [0, (2654435761 >> 21), ((2 ** 31 - 1) * 2654435761 % 2 ** 32) >> 21]


@pytest.mark.parametrize("n", [8191, 8192, GC.past("update_d_merged", 64), GC.past("update_d_merged", 256),
                               GC.past("update_d_merged", 304)])
def test_update_d_id_sets(n):
    full = n // GC.UD_CHUNK
    for kind in GC.UPDATE_D_KINDS:
        ids, n_faces, n_bad = GC.update_d_ids(kind, n)
        bad = (ids < 0) | (ids >= n_faces)
        assert ids.dtype == np.int64 and ids.shape == (n,) and int(bad.sum()) == n_bad == 5
        assert bad[:GC.UD_CHUNK].any() and bad[n - 1] and (ids[bad] < 0).any() and (ids[bad] >= n_faces).any()
        chunks = np.where(bad, -1, ids)[:full * GC.UD_CHUNK].reshape(full, GC.UD_CHUNK)
        srt = np.sort(chunks, axis=1)
        distinct = 1 + (srt[:, 1:] != srt[:, :-1]).sum(axis=1) - (srt[:, 0] == -1)
        if kind == "seven":
            assert n_faces == 7 and (distinct == 7).all()
        if kind == "distinct":
            # a table of 2048 slots half full: nearly every sample of a chunk probes for a slot of its own
            assert n_faces == 1 << 22 and (distinct >= 1000).all() and (distinct < GC.UD_CHUNK).any()
        if kind == "wrap":
            h = np.where(chunks >= 0, GC.update_d_hash(np.maximum(chunks, 0)), -1)
            last = np.array([np.unique(c[x == GC.UD_SLOTS - 1]).shape[0] for c, x in zip(chunks, h)])
            assert (last >= 4).all(), int(last.min())           # at least three of them wrap to slot 0 and beyond
            assert ((h >= GC.UD_SLOTS - 8) & (h < GC.UD_SLOTS - 1)).sum(axis=1).min() >= 8
            assert (distinct < GC.UD_SLOTS // 2).all()          # the probe always ends: the table never fills
