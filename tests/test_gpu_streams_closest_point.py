"""GPU: the entry point of include/qf_closest_point.h on a side stream, through tests/stream_harness.py: the zeroing of
the counts and the traversal must both run on the caller's stream (the rest of the query's GPU tests is
tests/test_gpu_closest_point.py).

The case lives in a file of its own that sorts after tests/test_gpu_streams.py, for the reason DESIGN.md section 3.9e
and tests/test_gpu_streams_mesh_manifold.py give: the first GPU test of that file depends on how many side streams the
session has handed out before it, and a case in front of it would change that number."""
import functools

import pytest
import torch

from tests import closest_point_cases as cases
from tests import stream_harness as sh

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _owner(device):
    """One tree (the level-4 icosphere, built on the device) for the fresh and the stale set: only the queries differ."""
    from quadraturefields_amd.mesh_io import TriMesh
    from quadraturefields_amd.mesh_utils import RayIntersector
    v, f = cases.sphere(4)
    return RayIntersector(TriMesh(v, f), device=device, builder="device")


def _stream_build(seed, device):
    n = 1 << 16
    q = cases.box_queries(n, seed=100 + seed, half=1.5)
    return dict(owner=_owner(str(device)), points=torch.from_numpy(q).to(device),
                out_tri=torch.zeros((n,), dtype=torch.int32, device=device),
                out_bary=torch.zeros((n, 3), dtype=torch.float64, device=device),
                out_dist2=torch.zeros((n,), dtype=torch.float64, device=device),
                out_counts=torch.zeros((2,), dtype=torch.int64, device=device))


def _call(i):
    from quadraturefields_amd import _C
    _C.check(_C.lib().qf_bvh_closest_points(i["owner"]._handle, _C.ptr(i["points"]), i["points"].shape[0], 1.0, _C.ptr(i["out_tri"]),
                                            _C.ptr(i["out_bary"]), _C.ptr(i["out_dist2"]), _C.ptr(i["out_counts"]), _C.stream()),
             "qf_bvh_closest_points")
    return i["out_tri"], i["out_bary"], i["out_dist2"], i["out_counts"]


STREAM_CASES = [
    sh.Case("bvh_closest_points", _stream_build, _call, entry_points=("qf_bvh_closest_points",), cpu_buildable=False),
]


def test_every_device_entry_point_has_a_stream_case():
    from quadraturefields_amd import _C
    assert sorted(ep for c in STREAM_CASES for ep in c.entry_points) == sorted(_C._CLOSEST_POINT_SIGNATURES)
    assert not any(c.host_wait for c in STREAM_CASES)


@pytest.mark.parametrize("name", [c.name for c in STREAM_CASES])
def test_entry_point_runs_entirely_on_the_callers_stream(device, lib, name):
    case = {c.name: c for c in STREAM_CASES}[name]
    issue_ms, delay_ms = sh.run_case(case, device)
    print(f"{name}: issue {issue_ms:.3f} ms, delay {delay_ms:.0f} ms")
