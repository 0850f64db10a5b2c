"""GPU: both entry points of include/qf_vertex_fit.h on a side stream, through tests/stream_harness.py (DESIGN.md section
3.9i; the rest of the pass's GPU tests is tests/test_gpu_vertex_fit.py).

The cases live in a file of their own that sorts after tests/test_gpu_streams.py on purpose, for the reason DESIGN.md
section 3.9e records: every ``run_case`` takes a new ``torch.cuda.Stream``, and that file's detection test depends on how
many side streams the session has handed out before it.  Behind it these cases change nothing it sees."""
import functools

import numpy as np
import pytest
import torch

from tests import mesh_sample_reference as sampler
from tests import stream_harness as sh

pytestmark = pytest.mark.gpu

N_COLUMNS = 16
STEPS = 8
LAMBDA = 1.0 / 64


@functools.lru_cache(maxsize=None)
def _stream_samples():
    """The level-4 icosphere with eight samples a face: the integers (faces, sample faces) are the same in both sets."""
    v, f = sampler.icosphere(4)
    _, face, bary, _ = sampler.sample(v, f, 8 * f.shape[0], seed=5)
    return v.shape[0], f, face, bary


def _stream_build(seed, device):
    from quadraturefields_amd import _C
    n_v, f, face, bary = _stream_samples()
    rng = np.random.default_rng(seed)
    n = int(_C.lib().qf_vertex_fit_workspace_bytes(n_v, f.shape[0], face.shape[0], N_COLUMNS))
    return dict(faces=torch.from_numpy(f).to(device), sample_face=torch.from_numpy(face).to(device),
                sample_bary=torch.from_numpy(rng.dirichlet(np.ones(3), face.shape[0])).to(device),   # the set's own
                targets=torch.from_numpy(rng.normal(size=(face.shape[0], N_COLUMNS)).astype(np.float32)).to(device),
                prior=torch.from_numpy(rng.normal(size=(n_v, N_COLUMNS)).astype(np.float32)).to(device),
                tmp_ws=torch.zeros((n,), dtype=torch.uint8, device=device),
                out_gram=torch.zeros((f.shape[0], 9), dtype=torch.float64, device=device),
                out_mass=torch.zeros((n_v,), dtype=torch.float64, device=device),
                out_rhs=torch.zeros((n_v, N_COLUMNS), dtype=torch.float64, device=device),
                out_counts=torch.zeros((8,), dtype=torch.int64, device=device),
                out_table=torch.zeros((n_v, N_COLUMNS), dtype=torch.float32, device=device),
                out_stats=torch.zeros((N_COLUMNS, 2), dtype=torch.float64, device=device))


def _assemble_call(i):
    from quadraturefields_amd import _C
    p = _C.ptr
    _C.check(_C.lib().qf_vertex_fit_assemble(p(i["faces"]), i["faces"].shape[0], i["prior"].shape[0], p(i["sample_face"]),
                                             p(i["sample_bary"]), i["sample_face"].shape[0], p(i["targets"]), N_COLUMNS,
                                             p(i["prior"]), N_COLUMNS, N_COLUMNS, LAMBDA, p(i["out_gram"]), p(i["out_mass"]),
                                             p(i["out_rhs"]), p(i["tmp_ws"]), i["tmp_ws"].shape[0], p(i["out_counts"]),
                                             _C.stream()), "qf_vertex_fit_assemble")
    return i["out_gram"], i["out_mass"], i["out_rhs"], i["out_counts"]


def _solve_call(i):
    """Assemble, then solve with no host wait in between."""
    from quadraturefields_amd import _C
    p = _C.ptr
    _assemble_call(i)
    _C.check(_C.lib().qf_vertex_fit_solve(p(i["faces"]), i["faces"].shape[0], i["prior"].shape[0], p(i["prior"]), N_COLUMNS,
                                          N_COLUMNS, p(i["out_gram"]), p(i["out_mass"]), p(i["out_rhs"]), STEPS,
                                          1 << (N_COLUMNS - 1), p(i["tmp_ws"]), i["tmp_ws"].shape[0], p(i["out_table"]),
                                          N_COLUMNS, p(i["out_stats"]), p(i["out_counts"]), _C.stream()),
             "qf_vertex_fit_solve")
    return i["out_table"], i["out_stats"], i["out_counts"], i["out_rhs"]


STREAM_CASES = [
    sh.Case("vertex_fit_assemble", _stream_build, _assemble_call, entry_points=("qf_vertex_fit_assemble",)),
    sh.Case("vertex_fit_solve", _stream_build, _solve_call, entry_points=("qf_vertex_fit_solve",)),
]


def test_every_device_entry_point_has_a_stream_case():
    from quadraturefields_amd import _C
    covered = sorted(ep for c in STREAM_CASES for ep in c.entry_points)
    assert covered == sorted(set(_C._VERTEX_FIT_SIGNATURES) - {"qf_vertex_fit_workspace_bytes"})
    assert not any(c.host_wait for c in STREAM_CASES)


@pytest.mark.parametrize("name", [c.name for c in STREAM_CASES])
def test_entry_point_runs_entirely_on_the_callers_stream(device, lib, name):
    case = {c.name: c for c in STREAM_CASES}[name]
    issue_ms, delay_ms = sh.run_case(case, device)
    print(f"{name}: issue {issue_ms:.3f} ms, delay {delay_ms:.0f} ms")
