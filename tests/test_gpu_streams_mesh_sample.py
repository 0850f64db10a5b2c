"""GPU: every entry point of include/qf_mesh_sample.h on a side stream, through tests/stream_harness.py (DESIGN.md section
3.9h; the rest of the pass's GPU tests is tests/test_gpu_mesh_sample.py).

The cases live in a file of their own that sorts after tests/test_gpu_streams.py on purpose, for the reason DESIGN.md
section 3.9e records: every ``run_case`` takes a new ``torch.cuda.Stream``, and that file's detection test depends on how
many side streams the session has handed out before it.  Behind it these cases change nothing it sees."""
import functools

import numpy as np
import pytest
import torch

from tests import mesh_sample_reference as ref
from tests import stream_harness as sh

pytestmark = pytest.mark.gpu

N_SAMPLES = 50_000
SEED = 11


@functools.lru_cache(maxsize=None)
def _stream_mesh(seed):
    """The level-4 icosphere with seeded jitter and seeded weights, 100 * seed of them zero: the faces (the only integers)
    are the same in both sets; the measures, with them every sample's face, point and barycentrics, and the count of
    faces that are never sampled are the seed's."""
    v, f = ref.icosphere(4)
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.2, 1.0, f.shape[0])
    w[rng.permutation(f.shape[0])[: 100 * seed]] = 0.0
    return v + rng.uniform(-0.01, 0.01, v.shape), f, w


def _stream_build(seed, device):
    from quadraturefields_amd import _C
    v, f, w = _stream_mesh(seed)
    n = int(_C.lib().qf_mesh_sample_workspace_bytes(v.shape[0], f.shape[0]))
    return dict(vertices=torch.from_numpy(v).to(device), faces=torch.from_numpy(f).to(device),
                weights=torch.from_numpy(w).to(device),
                tmp_ws=torch.zeros((n,), dtype=torch.uint8, device=device),
                out_counts=torch.zeros((6,), dtype=torch.int64, device=device),
                out_points=torch.zeros((N_SAMPLES, 3), dtype=torch.float64, device=device),
                out_face=torch.zeros((N_SAMPLES,), dtype=torch.int64, device=device),
                out_bary=torch.zeros((N_SAMPLES, 3), dtype=torch.float64, device=device))


def _prepare_call(i):
    from quadraturefields_amd import _C
    _C.check(_C.lib().qf_mesh_sample_prepare(_C.ptr(i["vertices"]), i["vertices"].shape[0], _C.ptr(i["faces"]),
                                             i["faces"].shape[0], _C.ptr(i["weights"]), _C.ptr(i["tmp_ws"]),
                                             i["tmp_ws"].shape[0], _C.ptr(i["out_counts"]), _C.stream()),
             "qf_mesh_sample_prepare")
    return (i["out_counts"],)


def _emit_call(i):
    """Prepare, then emit with no host wait in between."""
    from quadraturefields_amd import _C
    _prepare_call(i)
    _C.check(_C.lib().qf_mesh_sample_emit(_C.ptr(i["vertices"]), i["vertices"].shape[0], _C.ptr(i["faces"]), i["faces"].shape[0],
                                          _C.ptr(i["tmp_ws"]), i["tmp_ws"].shape[0], N_SAMPLES, SEED, _C.ptr(i["out_points"]),
                                          _C.ptr(i["out_face"]), _C.ptr(i["out_bary"]), _C.stream()), "qf_mesh_sample_emit")
    return i["out_points"], i["out_face"], i["out_bary"], i["out_counts"]


STREAM_CASES = [
    sh.Case("mesh_sample_prepare", _stream_build, _prepare_call, entry_points=("qf_mesh_sample_prepare",)),
    sh.Case("mesh_sample_emit", _stream_build, _emit_call, entry_points=("qf_mesh_sample_emit",)),
]


def test_every_device_entry_point_has_a_stream_case():
    from quadraturefields_amd import _C
    covered = sorted(ep for c in STREAM_CASES for ep in c.entry_points)
    assert covered == sorted(set(_C._MESH_SAMPLE_SIGNATURES) - {"qf_mesh_sample_workspace_bytes"})
    assert not any(c.host_wait for c in STREAM_CASES)


@pytest.mark.parametrize("name", [c.name for c in STREAM_CASES])
def test_entry_point_runs_entirely_on_the_callers_stream(device, lib, name):
    case = {c.name: c for c in STREAM_CASES}[name]
    issue_ms, delay_ms = sh.run_case(case, device)
    print(f"{name}: issue {issue_ms:.3f} ms, delay {delay_ms:.0f} ms")
