"""The numpy restatement of the decimation rules (tests/mesh_decimate_reference.py) pinned on
meshes whose outcome can be stated without running it: what must not move does not move, what must stay closed and
manifold does, and the face count is reached; and the new header against its binding."""
import ctypes
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import mesh_decimate_reference as ref
from tests import mesh_subdivide_reference as sub


def _edge_uses(f, n_v):
    edges, face_edges, counts = sub.edges(f, n_v)
    return edges, np.bincount(face_edges[face_edges >= 0], minlength=len(edges)), counts


def _euler(v, f):
    return v.shape[0] - _edge_uses(f, v.shape[0])[0].shape[0] + f.shape[0]


def _area(v, f):
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    return 0.5 * np.sqrt((n * n).sum(axis=1)).sum()


def _assert_maps(v0, f0, out):
    v, f, face_map, target, stats = out
    assert f.shape[0] == face_map.shape[0] and target.shape[0] == v0.shape[0]
    assert f.min(initial=0) >= 0 and f.max(initial=-1) < v.shape[0]
    assert (np.diff(face_map) > 0).all()                       # relative order kept, no face twice
    assert target.max(initial=-1) < v.shape[0] and target.min(initial=0) >= -1
    # an output face is its source face with every corner sent to where it ended up, in the same winding
    np.testing.assert_array_equal(target[f0[face_map]], f)
    assert stats["rounds"] == len(stats["faces"]) == len(stats["taken"]) == len(stats["selected"])


def test_tetrahedron_has_no_legal_edge():
    v, f = ref.tetrahedron()
    out = ref.decimate(v, f, 2)
    assert out[4]["stop"] == ref.STOP_NO_EDGE and out[4]["rounds"] == 1
    assert out[4]["candidates"] == [6] and out[4]["legal"] == [0]
    np.testing.assert_array_equal(out[0], v)
    np.testing.assert_array_equal(out[1], f)
    np.testing.assert_array_equal(out[2], np.arange(4))
    np.testing.assert_array_equal(out[3], np.arange(4))


def test_flat_grid_halves_and_keeps_plane_boundary_area_and_topology():
    v, f = ref.grid(9)
    assert f.shape[0] == 128
    out = ref.decimate(v, f, 64)
    w, g, _, target, stats = out
    _assert_maps(v, f, out)
    assert stats["stop"] == ref.STOP_TARGET and g.shape[0] == 64
    assert (w[:, 2] == 0.0).all()
    boundary = np.nonzero((v[:, :2] == 0.0).any(axis=1) | (v[:, :2] == 1.0).any(axis=1))[0]
    assert len(boundary) == 32 and (target[boundary] >= 0).all()
    assert w[target[boundary]].tobytes() == v[boundary].tobytes()
    assert abs(_area(w, g) - 1.0) <= 1e-12
    assert _euler(w, g) == 1


@functools.lru_cache(maxsize=None)
def _sphere_run(level, divisor):
    v, f = ref.icosphere(level)
    return v, f, ref.decimate(v, f, f.shape[0] // divisor, max_rounds=64)


@pytest.mark.parametrize("level,divisor", [(2, 4), (2, 10), (3, 4), (3, 10)])
def test_icosphere_stays_closed_and_manifold(level, divisor):
    v, f, out = _sphere_run(level, divisor)
    w, g, _, _, stats = out
    print(level, divisor, stats["rounds"], stats["faces"][-1], float(np.abs(np.linalg.norm(w, axis=1) - 1).max()))
    _assert_maps(v, f, out)
    assert stats["stop"] == ref.STOP_TARGET and g.shape[0] <= f.shape[0] // divisor and stats["rounds"] <= 64
    assert g.shape[0] >= f.shape[0] // divisor - 1             # a collapse removes two faces
    assert _euler(w, g) == 2
    edges, uses, counts = _edge_uses(g, w.shape[0])
    assert (uses == 2).all() and counts[1] == 0
    assert len({tuple(sorted(t)) for t in g.tolist()}) == g.shape[0]
    if (level, divisor) == (3, 4):
        assert np.abs(np.linalg.norm(w, axis=1) - 1.0).max() <= 0.05


def test_fan_vertices_are_locked():
    v, f = ref.fan()
    out = ref.decimate(v, f, 1)
    assert out[4]["stop"] == ref.STOP_NO_EDGE and out[4]["candidates"] == [0]
    np.testing.assert_array_equal(out[0], v)
    np.testing.assert_array_equal(out[1], f)


def test_fan_glued_to_a_sphere_does_not_move():
    v, f = ref.icosphere(1)
    n = v.shape[0]
    a, b = (int(x) for x in f[0, :2])
    v2 = np.concatenate([v, [v[a] * 2.0 + v[b]]])
    f2 = np.concatenate([f, [[a, b, n]]])                      # a third face on the edge (a, b)
    w, g, _, target, stats = ref.decimate(v2, f2, 20)
    for x in (a, b, n):
        assert target[x] >= 0 and w[target[x]].tobytes() == v2[x].tobytes()
    assert stats["taken"][0] > 0


def test_lock_everywhere_returns_the_input():
    v, f = ref.icosphere(2)
    out = ref.decimate(v, f, 10, vertex_lock=np.ones(v.shape[0], np.uint8))
    assert out[4]["stop"] == ref.STOP_NO_EDGE and out[4]["candidates"] == [0]
    assert out[0].tobytes() == v.tobytes() and out[1].tobytes() == f.tobytes()


def test_locked_vertices_keep_their_bits():
    v, f = ref.icosphere(2)
    lock = np.zeros(v.shape[0], np.uint8)
    lock[::3] = 1
    w, _, _, target, stats = ref.decimate(v, f, 160, vertex_lock=lock)
    ids = np.nonzero(lock)[0]
    assert (target[ids] >= 0).all() and w[target[ids]].tobytes() == v[ids].tobytes()
    assert sum(stats["taken"]) > 0


def test_max_cost_zero_takes_nothing_on_a_sphere():
    v, f = ref.icosphere(3)
    out = ref.decimate(v, f, 128, max_cost=0.0)
    assert out[4]["stop"] == ref.STOP_NO_EDGE and out[4]["candidates"] == [0]
    assert out[0].tobytes() == v.tobytes() and out[1].tobytes() == f.tobytes()


def test_target_at_or_above_the_face_count_returns_the_input():
    v, f = ref.icosphere(1)
    for target in (f.shape[0], f.shape[0] + 5):
        out = ref.decimate(v, f, target)
        assert out[4]["stop"] == ref.STOP_TARGET and out[4]["rounds"] == 0
        assert out[0].tobytes() == v.tobytes() and out[1].tobytes() == f.tobytes()


def test_max_rounds_is_reported():
    v, f = ref.icosphere(2)
    out = ref.decimate(v, f, 32, max_rounds=2)
    assert out[4]["stop"] == ref.STOP_MAX_ROUNDS and out[4]["rounds"] == 2 and out[1].shape[0] > 32


def test_budget_takes_the_cheapest_selected_edges():
    v, f = ref.icosphere(2)
    out = ref.decimate(v, f, f.shape[0] - 4, max_rounds=1)
    assert out[4]["taken"] == [2] and out[4]["selected"][0] > 2 and out[1].shape[0] == f.shape[0] - 4


def test_padded_builder_has_an_isolated_vertex_and_a_degenerate_face():
    for n in (63, 64, 65, 1025):
        v, f, n_e = ref.padded(n)
        assert n <= n_e <= n + 2
        assert not (f == v.shape[0] - 1).any() and (f[:, 0] == f[:, 1]).sum() == 1


# ------------------------------------------------------------------------------------------------------- the new header
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qf_mesh_decimate.h")
NEW_FUNCTIONS = sorted(["qf_mesh_decimate_workspace_bytes", "qf_mesh_vertex_quadrics", "qf_mesh_collapse_select",
                        "qf_mesh_collapse_apply", "qf_mesh_collapse_gather"])


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
    assert _functions(HEADER) == NEW_FUNCTIONS == sorted(_C._MESH_DECIMATE_SIGNATURES)
    assert not set(NEW_FUNCTIONS) & set(_C.EXPORTED_SYMBOLS) and _C.ABI_VERSION == 6
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if other != "qf_mesh_decimate.h":
            assert not set(NEW_FUNCTIONS) & set(_functions(os.path.join(ROOT, "include", other))), other
    raw = ctypes.CDLL(_C.LIB_PATH)
    for name in NEW_FUNCTIONS:
        getattr(raw, name)                               # AttributeError if the library does not export it
        fn = getattr(lib, name)
        restype, argtypes = _C._MESH_DECIMATE_SIGNATURES[name]
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)
    assert len(_C.MESH_QUADRIC_COUNTS) == 2 and len(_C.MESH_COLLAPSE_COUNTS) == 6


def test_every_new_entry_point_takes_the_callers_stream_and_is_indexed():
    from quadraturefields_amd import _C
    protos = _prototypes(HEADER)
    assert sorted(protos) == NEW_FUNCTIONS
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, params in protos.items():
        if name != "qf_mesh_decimate_workspace_bytes":   # a host computation: no device work, no stream
            assert re.search(r"void\s*\*\s*stream\s*$", params.strip()), f"{name}: the last parameter is not void *stream"
        assert len([p for p in params.split(",") if p.strip()]) == len(_C._MESH_DECIMATE_SIGNATURES[name][1]), name
        assert f"`{name}`" in text, f"INTEGRATION.md does not name {name}"


def test_new_header_is_plain_c(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "plain.c"
    src.write_text("\n".join(['#include <stdio.h>', '#include "qf_mesh_decimate.h"', "int main(void) {",
                              'printf("%d %d %d\\n", QF_MESH_QUADRIC_COUNTS, QF_MESH_COLLAPSE_COUNTS, QF_ABI_VERSION);',
                              "return 0;", "}"]))
    exe = tmp_path / "plain"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split() == ["2", "6", "6"]


def test_build_lists_the_new_source_and_header():
    from quadraturefields_amd import build
    assert dict(build.SOURCES)["mesh_decimate.hip"] == ["-ffp-contract=off"]
    assert HEADER in build._deps("mesh_decimate.hip")


def test_wrappers_refuse_host_tensors_and_bad_arguments():
    import torch
    from quadraturefields_amd import mc_utils
    from quadraturefields_amd.mesh_io import TriMesh
    v, f = ref.tetrahedron()
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    with pytest.raises(ValueError, match="device tensors"):
        mc_utils.decimate_mesh_device(tv, tf, 2)
    with pytest.raises(TypeError):
        mc_utils.decimate_mesh_device(v, tf, 2)
    with pytest.raises(ValueError):
        mc_utils.decimate_mesh_device(tv, tf[:, :2], 2)
    with pytest.raises(NotImplementedError):
        mc_utils.clean_mesh(TriMesh(v, f), agg=1, remove_non_manifold_edges=True)
    mesh = TriMesh(v, f)
    assert mc_utils.clean_mesh(mesh, agg=None) is mesh and mc_utils.clean_mesh(mesh, agg=0) is mesh
    from quadraturefields_amd.dropin import mc_utils as dropin
    assert dropin.clean_mesh is mc_utils.clean_mesh and dropin.down_sample_quadraic is mc_utils.down_sample_quadraic
