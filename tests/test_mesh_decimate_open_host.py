"""The numpy restatement of decimation with ``boundary="collapse"`` (tests/mesh_decimate_open_reference.py, DESIGN.md
section 3.9d) pinned on open meshes whose outcome can be stated without running it: the face count is reached, the
topology (Euler characteristic, boundary loops, components) is the input's, flat meshes keep their outline when the
boundary planes have weight; and the new header against its binding."""
import ctypes
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import mesh_decimate_open_reference as oref
from tests import mesh_decimate_reference as ref

WEIGHTS = (0.0, 1.0, 100.0)


def _area(v, f):
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    return 0.5 * np.sqrt((n * n).sum(axis=1)).sum()


def _complex_vertices(v, f):
    """Vertices that are neither interior nor border: on an edge without one or two uses, or with a number of boundary
    edges other than 0 or 2."""
    _, _, _, uses, edges = oref.topology(v, f)
    cls, _ = oref.vertex_classes(v.shape[0], edges, uses, np.zeros(v.shape[0], np.uint8))
    used = np.zeros(v.shape[0], dtype=bool)
    used[f.reshape(-1)] = True
    return set(np.nonzero((cls == oref.LOCKED) & used)[0].tolist())


def _assert_open_invariants(v0, f0, out):
    """What every collapse-mode output keeps: the maps, the topology, edges used at most twice, no duplicate vertex set,
    and two boundary edges at every border vertex unless it descends from a vertex that was complex in the input."""
    v, f, face_map, target, stats = out
    assert f.shape[0] == face_map.shape[0] and target.shape[0] == v0.shape[0]
    assert f.min(initial=0) >= 0 and f.max(initial=-1) < v.shape[0]
    assert (np.diff(face_map) > 0).all()
    np.testing.assert_array_equal(target[f0[face_map]], f)
    assert stats["rounds"] == len(stats["faces"]) == len(stats["taken"]) == len(stats["boundary_taken"])
    assert all(b <= t for b, t in zip(stats["boundary_taken"], stats["taken"]))
    before, after = oref.topology(v0, f0), oref.topology(v, f)
    assert after[:3] == before[:3], (before[:3], after[:3])
    assert after[3].max(initial=0) <= max(2, before[3].max(initial=0))
    assert len({tuple(sorted(t)) for t in f.tolist()}) == f.shape[0]
    allowed = {int(target[x]) for x in _complex_vertices(v0, f0)}
    assert _complex_vertices(v, f) <= allowed


@functools.lru_cache(maxsize=None)
def _run(name, weight):
    v, f, target = {"grid9": lambda: ref.grid(9) + (12,), "grid17": lambda: ref.grid(17) + (51,),
                    "holed": lambda: oref.holed(13, 4, 8) + (25,), "hemisphere": lambda: oref.hemisphere(3) + (62,)}[name]()
    return v, f, target, oref.decimate(v, f, target, boundary_weight=weight)


@pytest.mark.parametrize("weight", WEIGHTS)
@pytest.mark.parametrize("name", ["grid9", "grid17"])
def test_flat_grid_reaches_its_target_and_keeps_its_outline_under_weight(name, weight):
    v, f, target, out = _run(name, weight)
    w, g, _, vt, stats = out
    print(name, weight, stats["rounds"], g.shape[0], _area(w, g), sum(stats["boundary_taken"]))
    _assert_open_invariants(v, f, out)
    assert stats["stop"] == ref.STOP_TARGET and target - 1 <= g.shape[0] <= target
    assert sum(stats["boundary_taken"]) > 0
    assert (w[:, 2] == 0.0).all()
    if weight > 0.0:
        assert w[:, :2].min() >= 0.0 and w[:, :2].max() <= 1.0
        corners = np.nonzero(np.isin(v[:, 0], (0.0, 1.0)) & np.isin(v[:, 1], (0.0, 1.0)))[0]
        assert len(corners) == 4 and (vt[corners] >= 0).all() and w[vt[corners]].tobytes() == v[corners].tobytes()
        assert abs(_area(w, g) - 1.0) <= 1e-12
    else:
        assert _area(w, g) < 1.0 - 1e-3                          # without the planes nothing holds the outline


@pytest.mark.parametrize("weight", WEIGHTS)
def test_holed_grid_keeps_both_loops(weight):
    v, f, target, out = _run("holed", weight)
    w, g, _, _, stats = out
    print(weight, stats["rounds"], g.shape[0], _area(w, g))
    assert f.shape[0] == 256 and oref.topology(v, f)[:3] == (0, 2, 1)
    _assert_open_invariants(v, f, out)
    assert stats["stop"] == ref.STOP_TARGET and target - 1 <= g.shape[0] <= target
    if weight == 100.0:
        assert abs(_area(w, g) - 8.0 / 9.0) <= 1e-12


@pytest.mark.parametrize("weight", WEIGHTS)
def test_hemisphere_reaches_its_target(weight):
    v, f, target, out = _run("hemisphere", weight)
    w, g, _, _, stats = out
    err = float(np.abs(np.linalg.norm(w, axis=1) - 1.0).max())
    print(weight, stats["rounds"], g.shape[0], err)
    assert f.shape[0] == 624 and oref.topology(v, f)[:3] == (1, 1, 1)
    _assert_open_invariants(v, f, out)
    assert stats["stop"] == ref.STOP_TARGET and target - 1 <= g.shape[0] <= target
    if weight == 1.0:
        assert err <= 0.05                                        # the cap of the closed level-3 sphere


def test_lock_mode_stalls_where_collapse_mode_does_not():
    v, f = ref.grid(9)
    stalled = ref.decimate(v, f, 12)
    assert stalled[4]["stop"] == ref.STOP_NO_EDGE and stalled[1].shape[0] == 32


def test_bowtie_keeps_its_shared_vertex():
    v, f, shared = oref.bowtie()
    assert f.shape[0] == 64 and shared in _complex_vertices(v, f)
    out = oref.decimate(v, f, 8)
    w, g, _, vt, stats = out
    _assert_open_invariants(v, f, out)
    assert stats["stop"] == ref.STOP_TARGET and 7 <= g.shape[0] <= 8
    assert vt[shared] >= 0 and w[vt[shared]].tobytes() == v[shared].tobytes()
    assert int(vt[shared]) in _complex_vertices(w, g)


def test_fan_does_not_move():
    v, f = ref.fan()
    out = oref.decimate(v, f, 1)
    assert out[4]["stop"] == ref.STOP_NO_EDGE and out[4]["candidates"] == [0] and out[4]["boundary_taken"] == [0]
    assert out[0].tobytes() == v.tobytes() and out[1].tobytes() == f.tobytes()


def test_single_triangle_is_not_taken():
    v, f = oref.one_triangle()
    out = oref.decimate(v, f, 0)
    assert out[4]["stop"] == ref.STOP_NO_EDGE and out[4]["candidates"] == [0]
    assert out[0].tobytes() == v.tobytes() and out[1].tobytes() == f.tobytes()


def test_two_triangles_become_one():
    v, f = oref.two_triangles()
    out = oref.decimate(v, f, 1)
    _assert_open_invariants(v, f, out)
    assert out[1].shape[0] == 1 and out[4]["stop"] == ref.STOP_TARGET and out[4]["boundary_taken"] == [1]


@pytest.mark.parametrize("weight", WEIGHTS)
def test_closed_mesh_equals_lock_mode(weight):
    v, f = ref.icosphere(2)
    got, want = oref.decimate(v, f, 80, boundary_weight=weight), ref.decimate(v, f, 80)
    assert got[0].tobytes() == want[0].tobytes()
    for k in (1, 2, 3):
        assert np.array_equal(got[k], want[k])
    assert all(got[4][name] == want[4][name] for name in want[4])
    assert sum(got[4]["boundary_taken"]) == 0


def test_locked_border_equals_lock_mode():
    v, f = ref.grid(9)
    lock = ((v[:, :2] == 0.0) | (v[:, :2] == 1.0)).any(axis=1)
    got, want = oref.decimate(v, f, 12, vertex_lock=lock), ref.decimate(v, f, 12, vertex_lock=lock)
    assert got[0].tobytes() == want[0].tobytes()
    for k in (1, 2, 3):
        assert np.array_equal(got[k], want[k])
    assert all(got[4][name] == want[4][name] for name in want[4])


def test_budget_prefix_ends_between_a_one_face_and_a_two_face_collapse():
    """The level-3 hemisphere, five faces to remove: the cheapest selected edges of round 0 are four boundary edges (one
    face each) and then edges with two faces, so the prefix 1 + 1 + 1 + 1 + 2 is the shortest that reaches five, and it
    removes six."""
    v, f = oref.hemisphere(3)
    out = oref.decimate(v, f, f.shape[0] - BUDGET_FACES, max_rounds=1)
    stats = out[4]
    assert stats["selected"][0] > stats["taken"][0] and 0 < stats["boundary_taken"][0] < stats["taken"][0]
    removed = f.shape[0] - out[1].shape[0]
    assert removed == 2 * stats["taken"][0] - stats["boundary_taken"][0]
    assert stats["taken"] == [5] and stats["boundary_taken"] == [4] and removed == BUDGET_FACES + 1


BUDGET_FACES = 5


# ------------------------------------------------------------------------------------------------------- the new header
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_NAME = "qf_mesh_decimate_open.h"
HEADER = os.path.join(ROOT, "include", HEADER_NAME)
WORKSPACE = "qf_mesh_decimate_open_workspace_bytes"
NEW_FUNCTIONS = sorted([WORKSPACE, "qf_mesh_boundary_quadrics", "qf_mesh_collapse_select_open",
                        "qf_mesh_collapse_apply_open"])


def _strip_comments(text):
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def _functions(path):
    return sorted(set(re.findall(r"\b(qf_[a-z0-9_]+)\s*\(", _strip_comments(open(path).read()))))


def _prototypes(path):
    out = {}
    for stmt in _strip_comments(open(path).read()).split(";"):
        m = re.search(r"\b(qf_\w+)\s*\(([^()]*)\)\s*$", stmt.strip(), flags=re.S)
        if m and "typedef" not in stmt:
            out[m.group(1)] = m.group(2)
    return out


def test_header_and_binding_agree(lib):
    from quadraturefields_amd import _C
    assert _functions(HEADER) == NEW_FUNCTIONS == sorted(_C._MESH_DECIMATE_OPEN_SIGNATURES)
    assert not set(NEW_FUNCTIONS) & set(_C.EXPORTED_SYMBOLS) and _C.ABI_VERSION == 6
    assert not set(NEW_FUNCTIONS) & set(_C._MESH_DECIMATE_SIGNATURES)
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if other != HEADER_NAME:
            assert not set(NEW_FUNCTIONS) & set(_functions(os.path.join(ROOT, "include", other))), other
    raw = ctypes.CDLL(_C.LIB_PATH)
    for name in NEW_FUNCTIONS:
        getattr(raw, name)                               # AttributeError if the library does not export it
        fn = getattr(lib, name)
        restype, argtypes = _C._MESH_DECIMATE_OPEN_SIGNATURES[name]
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)
    assert len(_C.MESH_BOUNDARY_COUNTS) == 2 and len(_C.MESH_COLLAPSE_OPEN_COUNTS) == 8
    assert _C.MESH_COLLAPSE_OPEN_COUNTS[:6] == _C.MESH_COLLAPSE_COUNTS


def test_every_new_entry_point_takes_the_callers_stream_and_is_indexed():
    from quadraturefields_amd import _C
    protos = _prototypes(HEADER)
    assert sorted(protos) == NEW_FUNCTIONS
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, params in protos.items():
        if name != WORKSPACE:                            # a host computation: no device work, no stream
            assert re.search(r"void\s*\*\s*stream\s*$", params.strip()), f"{name}: the last parameter is not void *stream"
        assert len([p for p in params.split(",") if p.strip()]) == len(_C._MESH_DECIMATE_OPEN_SIGNATURES[name][1]), name
        assert f"`{name}`" in text, f"INTEGRATION.md does not name {name}"


def test_new_header_is_plain_c(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "plain.c"
    src.write_text("\n".join(['#include <stdio.h>', f'#include "{HEADER_NAME}"', "int main(void) {",
                              'printf("%d %d %d\\n", QF_MESH_BOUNDARY_COUNTS, QF_MESH_COLLAPSE_OPEN_COUNTS, QF_ABI_VERSION);',
                              "return 0;", "}"]))
    exe = tmp_path / "plain"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split() == ["2", "8", "6"]


def test_build_lists_the_new_header():
    from quadraturefields_amd import build
    assert dict(build.SOURCES)["mesh_decimate.hip"] == ["-ffp-contract=off"]
    assert HEADER in build._deps("mesh_decimate.hip")
    assert f'#include "{HEADER_NAME}"' in open(os.path.join(build.CSRC, "mesh_decimate.hip")).read()


def test_wrappers_refuse_bad_boundary_arguments_before_any_work():
    import torch
    from quadraturefields_amd import mc_utils
    from quadraturefields_amd.mesh_io import TriMesh
    v, f = oref.two_triangles()
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    for bad in ("open", "Collapse", None, 1):
        with pytest.raises(ValueError, match="boundary must be one of"):
            mc_utils.decimate_mesh_device(tv, tf, 1, boundary=bad)
        with pytest.raises(ValueError, match="boundary must be one of"):
            mc_utils.decimate_mesh(TriMesh(v, f), 1, boundary=bad)
        with pytest.raises(ValueError, match="boundary must be one of"):
            mc_utils.down_sample_quadraic(TriMesh(v, f), boundary=bad)
        with pytest.raises(ValueError, match="boundary must be one of"):
            mc_utils.clean_mesh(TriMesh(v, f), agg=None, boundary=bad)
    for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="boundary_weight"):
            mc_utils.decimate_mesh_device(tv, tf, 1, boundary="collapse", boundary_weight=bad)
        with pytest.raises(ValueError, match="boundary_weight"):
            mc_utils.decimate_mesh(TriMesh(v, f), 1, boundary_weight=bad)
    with pytest.raises(ValueError, match="device tensors"):
        mc_utils.decimate_mesh_device(tv, tf, 1, boundary="collapse")
    mesh = TriMesh(v, f)
    assert mc_utils.clean_mesh(mesh, agg=None, boundary="collapse") is mesh
