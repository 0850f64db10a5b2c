"""GPU: every entry point of include/qf_mesh_weld.h on a side stream, through tests/stream_harness.py (DESIGN.md section
3.9g; the rest of the pass's GPU tests is tests/test_gpu_mesh_weld.py).

The cases live in a file of their own that sorts after tests/test_gpu_streams.py on purpose, for the reason DESIGN.md
section 3.9e records: every ``run_case`` takes a new ``torch.cuda.Stream``, and that file's detection test depends on how
many side streams the session has handed out before it.  Behind it these cases change nothing it sees."""
import functools

import numpy as np
import pytest
import torch

from tests import mesh_decimate_reference as ref
from tests import mesh_weld_reference as wref
from tests import stream_harness as sh

pytestmark = pytest.mark.gpu

TOLERANCE = 0.004


@functools.lru_cache(maxsize=None)
def _stream_mesh(seed):
    """The soup of the level-4 icosphere with seeded jitter of up to 0.6 tolerances per axis: most corners of a vertex
    weld back together at ``TOLERANCE`` (the link pass runs) and some do not, so the counts are the seed's too."""
    v, f = ref.icosphere(4)
    sv, sf = wref.soup(v, f)
    return sv + np.random.default_rng(seed).uniform(-0.6 * TOLERANCE, 0.6 * TOLERANCE, sv.shape), sf


def _stream_build(seed, device):
    from quadraturefields_amd import _C
    v, f = _stream_mesh(seed)
    n_v, n_f = v.shape[0], f.shape[0]
    n = int(_C.lib().qf_mesh_weld_workspace_bytes(n_v, n_f))
    return dict(vertices=torch.from_numpy(v).to(device), faces=torch.from_numpy(f).to(device),
                tmp_ws=torch.zeros((n,), dtype=torch.uint8, device=device),
                out_counts=torch.zeros((8,), dtype=torch.int64, device=device),
                out_v=torch.zeros((n_v, 3), dtype=torch.float64, device=device),
                out_f=torch.zeros((n_f, 3), dtype=torch.int64, device=device),
                out_map=torch.zeros((n_v,), dtype=torch.int64, device=device),
                out_class=torch.zeros((n_v,), dtype=torch.int64, device=device))


def _count_call(i):
    from quadraturefields_amd import _C
    _C.check(_C.lib().qf_mesh_weld_count(_C.ptr(i["vertices"]), i["vertices"].shape[0], _C.ptr(i["faces"]), i["faces"].shape[0],
                                         TOLERANCE, _C.ptr(i["tmp_ws"]), i["tmp_ws"].shape[0], _C.ptr(i["out_counts"]),
                                         _C.stream()), "qf_mesh_weld_count")
    return (i["out_counts"],)


def _emit_call(i):
    """Count, then emit at full capacity with no host wait in between: the rows beyond V' keep the sentinel."""
    from quadraturefields_amd import _C
    _count_call(i)
    _C.check(_C.lib().qf_mesh_weld_emit(_C.ptr(i["vertices"]), i["vertices"].shape[0], _C.ptr(i["faces"]), i["faces"].shape[0],
                                        _C.ptr(i["tmp_ws"]), i["tmp_ws"].shape[0], _C.ptr(i["out_v"]), i["out_v"].shape[0],
                                        _C.ptr(i["out_f"]), _C.ptr(i["out_map"]), _C.ptr(i["out_class"]), _C.stream()),
             "qf_mesh_weld_emit")
    return i["out_v"], i["out_f"], i["out_map"], i["out_class"], i["out_counts"]


STREAM_CASES = [
    sh.Case("mesh_weld_count", _stream_build, _count_call, entry_points=("qf_mesh_weld_count",)),
    sh.Case("mesh_weld_emit", _stream_build, _emit_call, entry_points=("qf_mesh_weld_emit",)),
]


def test_every_device_entry_point_has_a_stream_case():
    from quadraturefields_amd import _C
    covered = sorted(ep for c in STREAM_CASES for ep in c.entry_points)
    assert covered == sorted(set(_C._MESH_WELD_SIGNATURES) - {"qf_mesh_weld_workspace_bytes"})
    assert not any(c.host_wait for c in STREAM_CASES)


@pytest.mark.parametrize("name", [c.name for c in STREAM_CASES])
def test_entry_point_runs_entirely_on_the_callers_stream(device, lib, name):
    case = {c.name: c for c in STREAM_CASES}[name]
    issue_ms, delay_ms = sh.run_case(case, device)
    print(f"{name}: issue {issue_ms:.3f} ms, delay {delay_ms:.0f} ms")
