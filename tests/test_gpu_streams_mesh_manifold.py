"""GPU: every entry point of include/qf_mesh_manifold.h on a side stream, through tests/stream_harness.py, as the
open-decimation test does (the rest of the pass's GPU tests is tests/test_gpu_mesh_manifold.py).

The cases live in a file of their own that sorts after tests/test_gpu_streams.py on purpose.  Every ``run_case`` takes a
new ``torch.cuda.Stream``, and the first GPU test of that file,
``test_the_harness_detects_a_launch_on_the_wrong_stream``, depends on how many side streams the session has handed out
before it.  Measured on an MI355X, one fresh process per n: after n side streams its deliberately mis-streamed launch was
noticed for n = 0 .. 5, 7, 12 and 44 and went unnoticed for n = 6, 14 and 46 -- every eighth side stream runs in order
with the default stream, so a launch that strays there waits behind the delay like a correct one.  The suite hands out
44 before that test's mis-streamed run; with these two cases in front it was 46.  Behind it they change nothing it sees,
and a case here that lands on such a stream only loses its power to notice, never fails for it."""
import functools

import numpy as np
import pytest
import torch

from tests import mesh_decimate_reference as ref
from tests import mesh_manifold_reference as mref
from tests import stream_harness as sh

pytestmark = pytest.mark.gpu

@functools.lru_cache(maxsize=None)
def _stream_mesh(seed):
    """Exactly half the faces of the level-4 icosphere, chosen by the seed (the faces and their edge ids are named in
    ``varies``), every vertex kept, with seeded coordinates."""
    v, f = ref.icosphere(4)
    rng = np.random.default_rng(seed)
    f = f[np.sort(rng.permutation(f.shape[0])[: f.shape[0] // 2])]
    return v + rng.uniform(-0.01, 0.01, v.shape), f, mref.edges(f, v.shape[0])[1]


def _stream_build(seed, device):
    from quadraturefields_amd import _C
    v, f, fe = _stream_mesh(seed)
    n_v, n_f = v.shape[0], f.shape[0]
    n = int(_C.lib().qf_mesh_manifold_workspace_bytes(n_v, n_f, 3 * n_f))           # an edge count both sets stay below
    return dict(vertices=torch.from_numpy(v).to(device), faces=torch.from_numpy(f).to(device),
                face_edges=torch.from_numpy(fe).to(device), tmp_ws=torch.zeros((n,), dtype=torch.uint8, device=device),
                out_counts=torch.zeros((8,), dtype=torch.int64, device=device),
                out_v=torch.zeros((n_v + 3 * n_f, 3), dtype=torch.float64, device=device),
                out_f=torch.zeros((n_f, 3), dtype=torch.int64, device=device),
                out_map=torch.zeros((n_v + 3 * n_f,), dtype=torch.int64, device=device))


def _count_call(i):
    from quadraturefields_amd import _C
    n_f = i["faces"].shape[0]
    _C.check(_C.lib().qf_mesh_manifold_count(_C.ptr(i["faces"]), n_f, i["vertices"].shape[0], _C.ptr(i["face_edges"]), 3 * n_f,
                                             _C.ptr(i["tmp_ws"]), i["tmp_ws"].shape[0], _C.ptr(i["out_counts"]), _C.stream()),
             "qf_mesh_manifold_count")
    return (i["out_counts"],)


def _emit_call(i):
    """Count, then emit at full capacity with no host wait in between: the rows beyond V' keep the sentinel."""
    from quadraturefields_amd import _C
    _count_call(i)
    _C.check(_C.lib().qf_mesh_manifold_emit(_C.ptr(i["vertices"]), _C.ptr(i["faces"]), i["faces"].shape[0], i["vertices"].shape[0],
                                            _C.ptr(i["tmp_ws"]), i["tmp_ws"].shape[0], _C.ptr(i["out_v"]), i["out_v"].shape[0],
                                            _C.ptr(i["out_f"]), _C.ptr(i["out_map"]), _C.stream()), "qf_mesh_manifold_emit")
    return i["out_v"], i["out_f"], i["out_map"], i["out_counts"]


STREAM_CASES = [
    sh.Case("mesh_manifold_count", _stream_build, _count_call, varies=("faces", "face_edges"),
            entry_points=("qf_mesh_manifold_count",)),
    sh.Case("mesh_manifold_emit", _stream_build, _emit_call, varies=("faces", "face_edges"),
            entry_points=("qf_mesh_manifold_emit",)),
]


def test_every_device_entry_point_has_a_stream_case():
    from quadraturefields_amd import _C
    covered = sorted(ep for c in STREAM_CASES for ep in c.entry_points)
    assert covered == sorted(set(_C._MESH_MANIFOLD_SIGNATURES) - {"qf_mesh_manifold_workspace_bytes"})
    assert not any(c.host_wait for c in STREAM_CASES)


@pytest.mark.parametrize("name", [c.name for c in STREAM_CASES])
def test_entry_point_runs_entirely_on_the_callers_stream(device, lib, name):
    case = {c.name: c for c in STREAM_CASES}[name]
    issue_ms, delay_ms = sh.run_case(case, device)
    print(f"{name}: issue {issue_ms:.3f} ms, delay {delay_ms:.0f} ms")
