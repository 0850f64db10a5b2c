"""The numpy restatement of the manifold rule (tests/mesh_manifold_reference.py) pinned on meshes
whose outcome is worked out by hand, its guarantees on those and on masked spheres, what the cut buys the restated
decimation, and the new header against its binding."""
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
from tests import mesh_manifold_reference as mref
from tests import mesh_subdivide_reference as sub


def _bowtie_faces():
    f = oref.bowtie()[1].copy()
    f[32, 0] = f[33, 0] = 49           # the second grid's two faces at the shared vertex 24
    return f.tolist()


# name -> (builder, out_faces, vertex_map, counts): worked by hand from the rule
HAND_CASES = {
    # two 5 x 5 grids that share vertex 24: its corners in faces 30, 31 form the class of corner 92, which keeps 24; those
    # in faces 32, 33 the class of corner 96, which is extra
    "bowtie": (lambda: oref.bowtie()[:2], _bowtie_faces(), list(range(49)) + [24], [50, 1, 0, 0, 32, 0, 0, 0]),
    # three faces on (0, 1): nothing is linked there, so faces 1 and 2 get their own copies of 0 and 1; the extra corners
    # are 3 (vertex 1), 4 (vertex 0), 6 (vertex 0), 7 (vertex 1)
    "book3": (lambda: mref.book(3), [[0, 1, 2], [5, 6, 3], [7, 8, 4]], [0, 1, 2, 3, 4, 1, 0, 0, 1], [9, 2, 1, 3, 6, 0, 0, 0]),
    "book4": (lambda: mref.book(4), [[0, 1, 2], [6, 7, 3], [8, 9, 4], [10, 11, 5]], [0, 1, 2, 3, 4, 5, 1, 0, 0, 1, 1, 0],
              [12, 2, 1, 4, 8, 0, 0, 0]),
    # each tetrahedron's three corners at 0 (and at 1) are joined through its two manifold edges there; the second one's
    # classes start at corners 12 (vertex 0) and 14 (vertex 1)
    "two_tetrahedra": (mref.two_tetrahedra, [[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3], [6, 4, 7], [6, 7, 5], [6, 5, 4], [7, 4, 5]],
                       [0, 1, 2, 3, 4, 5, 0, 1], [8, 2, 1, 4, 0, 0, 0, 0]),
    "same_direction_pair": (mref.same_direction_pair, [[0, 1, 2], [0, 1, 3]], [0, 1, 2, 3], [4, 0, 0, 0, 4, 1, 0, 0]),
    "degenerate_beside_bowtie": (mref.degenerate_beside_bowtie, [[0, 1, 2], [0, 0, 5], [6, 3, 4]], [0, 1, 2, 3, 4, 5, 0],
                                 [7, 1, 0, 0, 6, 0, 1, 0]),
    "unreferenced_vertex": (mref.unreferenced_vertex, [[0, 1, 2]], [0, 1, 2, 3], [4, 0, 0, 0, 3, 0, 0, 0]),
    "no_faces": (lambda: (np.arange(9, dtype=np.float64).reshape(3, 3), np.zeros((0, 3), np.int64)), [], [0, 1, 2],
                 [3, 0, 0, 0, 0, 0, 0, 0]),
}


@functools.lru_cache(maxsize=None)
def masked_sphere(level, seed):
    return mref.masked(*ref.icosphere(level), seed)


def guarantee_meshes():
    out = {name: case[0]() for name, case in HAND_CASES.items()}
    out.update(icosphere2=ref.icosphere(2), hemisphere2=oref.hemisphere(2), masked_seed0=masked_sphere(3, 0),
               masked_seed1=masked_sphere(3, 1))
    return out


@pytest.mark.parametrize("name", sorted(HAND_CASES))
def test_hand_worked_case(name):
    build, faces, vertex_map, counts = HAND_CASES[name]
    v, f = build()
    out_v, out_f, vmap, c = mref.cut(v, f)
    assert out_f.tolist() == faces and vmap.tolist() == vertex_map and c.tolist() == counts
    assert out_v.tobytes() == np.ascontiguousarray(v, np.float64)[vertex_map].tobytes()


def test_case_table_says_what_the_issue_says():
    shapes = {name: (case[0]()[0].shape[0], case[3][0]) for name, case in HAND_CASES.items()}
    assert shapes["bowtie"] == (49, 50) and shapes["book3"] == (5, 9) and shapes["book4"] == (6, 12)
    assert shapes["two_tetrahedra"] == (6, 8) and shapes["same_direction_pair"] == (4, 4)
    assert HAND_CASES["bowtie"][2][49] == 24 and HAND_CASES["book3"][3][1:3] == [2, 1]
    v, f = mref.two_tetrahedra()
    out_v, out_f, _, c = mref.cut(v, f)
    assert c[4] == 0 and (mref.edge_uses(out_f, out_v.shape[0])[0] == 2).all()        # closed before and after


def test_vectorised_edges_are_stage_a():
    for name, (v, f) in guarantee_meshes().items():
        e, fe, _ = sub.edges(f, v.shape[0])
        got_e, got_fe = mref.edges(f, v.shape[0])
        assert np.array_equal(got_e, e) and np.array_equal(got_fe, fe), name


@pytest.mark.parametrize("name", sorted(guarantee_meshes()))
def test_guarantees(name):
    v, f = guarantee_meshes()[name]
    out_v, out_f, vmap, c = mref.cut(v, f)
    assert out_v[out_f].tobytes() == np.ascontiguousarray(v[f]).tobytes()                      # the same triangle soup
    assert np.array_equal(vmap[:v.shape[0]], np.arange(v.shape[0])) and c[0] == out_v.shape[0] == vmap.shape[0]
    uses, _ = mref.edge_uses(out_f, out_v.shape[0])
    assert uses.max(initial=0) <= 2                                                            # no complex edge
    assert mref.complex_vertices(out_v, out_f) == 0                                            # one fan at every vertex
    again = mref.cut(out_v, out_f)                                                             # idempotent
    assert again[0].tobytes() == out_v.tobytes() and np.array_equal(again[1], out_f)
    assert np.array_equal(again[2], np.arange(out_v.shape[0])) and again[3][1] == again[3][2] == again[3][3] == 0
    assert again[3][4] == (uses == 1).sum()
    if name in ("icosphere2", "hemisphere2"):                                                  # a manifold is left alone
        assert out_v.tobytes() == v.tobytes() and out_f.tobytes() == f.tobytes() and c[0] == v.shape[0]
    if name.startswith("masked"):
        assert c[1] == mref.complex_vertices(v, f) > 0 and c[4] == (uses == 1).sum()           # the borders are the input's


def test_prototype_figures_of_the_masked_sphere():
    v, f = masked_sphere(3, 0)
    c = mref.cut(v, f)[3]
    assert (f.shape[0], v.shape[0]) == (617, 636) and c.tolist() == [985, 331, 0, 0, 981, 0, 0, 0]


def test_duplicate_faces_are_cut_apart():
    v, f = ref.icosphere(1)
    c = mref.cut(v, np.concatenate([f, f[:5]]))[3]
    assert c[0] - v.shape[0] == 30 and c[2] > 0


@pytest.mark.parametrize("seed", [0, 1])
def test_cut_mesh_decimates_further(seed):
    v, f = masked_sphere(3, seed)
    target = f.shape[0] // 10
    plain = oref.decimate(v, f, target)
    out_v, out_f = mref.cut(v, f)[:2]
    cut = oref.decimate(out_v, out_f, target)
    print(f"seed {seed}: {f.shape[0]} faces to {target}: as it is {plain[1].shape[0]} ({plain[4]['stop']}, "
          f"{plain[4]['rounds']} rounds), cut {cut[1].shape[0]} ({cut[4]['stop']}, {cut[4]['rounds']} rounds)")
    assert cut[1].shape[0] < plain[1].shape[0]


def test_invalid_faces_produce_nothing():
    v, f = mref.book(3)
    bad = f.copy()
    bad[1, 2] = 5
    assert mref.cut(v, bad)[3].tolist() == [0] * 7 + [1] and mref.cut(v, bad)[0] is None
    fe = mref.edges(f, 5)[1]
    assert fe.tolist() == [[0, 1, 2], [0, 3, 4], [0, 5, 6]]
    assert mref.cut(v, f, fe, 4)[3].tolist() == [0] * 7 + [2]           # faces 1 and 2 have an edge id outside [0, 4)


# ------------------------------------------------------------------------------------------------------- the new header
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_NAME = "qf_mesh_manifold.h"
HEADER = os.path.join(ROOT, "include", HEADER_NAME)
WORKSPACE = "qf_mesh_manifold_workspace_bytes"
NEW_FUNCTIONS = sorted([WORKSPACE, "qf_mesh_manifold_count", "qf_mesh_manifold_emit"])


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
    assert _functions(HEADER) == NEW_FUNCTIONS == sorted(_C._MESH_MANIFOLD_SIGNATURES)
    assert not set(NEW_FUNCTIONS) & set(_C.EXPORTED_SYMBOLS) and _C.ABI_VERSION == 6
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if other != HEADER_NAME:
            assert not set(NEW_FUNCTIONS) & set(_functions(os.path.join(ROOT, "include", other))), other
    raw = ctypes.CDLL(_C.LIB_PATH)
    for name in NEW_FUNCTIONS:
        getattr(raw, name)                               # AttributeError if the library does not export it
        fn = getattr(lib, name)
        restype, argtypes = _C._MESH_MANIFOLD_SIGNATURES[name]
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)
    assert _C.MESH_MANIFOLD_COUNTS == mref.COUNT_NAMES and len(mref.COUNT_NAMES) == 8
    assert lib.qf_mesh_manifold_workspace_bytes(0, 0, 0) == -1 and lib.qf_mesh_manifold_workspace_bytes(5, 2 ** 30, 0) == -1
    assert lib.qf_mesh_manifold_workspace_bytes(5, 3, 2 ** 31) == -1 and lib.qf_mesh_manifold_workspace_bytes(2 ** 31, 3, 7) == -1
    assert 0 < lib.qf_mesh_manifold_workspace_bytes(5, 0, 0) < lib.qf_mesh_manifold_workspace_bytes(5, 3, 7)


def test_every_new_entry_point_takes_the_callers_stream_and_is_indexed():
    from quadraturefields_amd import _C
    protos = _prototypes(HEADER)
    assert sorted(protos) == NEW_FUNCTIONS
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, params in protos.items():
        if name != WORKSPACE:                            # a host computation: no device work, no stream
            assert re.search(r"void\s*\*\s*stream\s*$", params.strip()), f"{name}: the last parameter is not void *stream"
        assert len([p for p in params.split(",") if p.strip()]) == len(_C._MESH_MANIFOLD_SIGNATURES[name][1]), name
        assert f"`{name}`" in text, f"INTEGRATION.md does not name {name}"


def test_new_header_is_plain_c(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "plain.c"
    src.write_text("\n".join(['#include <stdio.h>', f'#include "{HEADER_NAME}"', "int main(void) {",
                              'printf("%d %d\\n", QF_MESH_MANIFOLD_COUNTS, QF_ABI_VERSION);', "return 0;", "}"]))
    exe = tmp_path / "plain"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split() == ["8", "6"]


def test_build_lists_the_new_source_and_header():
    from quadraturefields_amd import build
    assert dict(build.SOURCES)["mesh_manifold.hip"] == []            # no arithmetic: nothing to keep from contracting
    assert HEADER in build._deps("mesh_manifold.hip")
    text = open(os.path.join(build.CSRC, "mesh_manifold.hip")).read()
    assert f'#include "{HEADER_NAME}"' in text
    assert not re.search(r"\b(float|double)\b", re.sub(r"//.*", "", text).replace("const double *vertices", "")
                         .replace("double *out_vertices", ""))        # coordinates are only ever moved as words


def test_wrappers_refuse_host_tensors_and_bad_arguments():
    import torch
    from quadraturefields_amd import mc_utils
    from quadraturefields_amd.mesh_io import TriMesh
    v, f = mref.book(3)
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    with pytest.raises(ValueError, match="device tensors"):
        mc_utils.make_manifold_device(tv, tf)
    with pytest.raises(TypeError):
        mc_utils.make_manifold_device(v, tf)
    with pytest.raises(TypeError):
        mc_utils.make_manifold_device(tv, f)
    with pytest.raises(ValueError):
        mc_utils.make_manifold_device(tv, tf[:, :2])
    with pytest.raises(ValueError):
        mc_utils.make_manifold_device(tv[:, :2], tf)
    with pytest.raises(TypeError):
        mc_utils.make_manifold_device(tv, tf.to(torch.float32))
    with pytest.raises(NotImplementedError, match="make_manifold"):
        mc_utils.clean_mesh(TriMesh(v, f), agg=1, remove_non_manifold_edges=True)
    assert mc_utils.ManifoldMesh._fields == ("vertices", "faces", "vertex_map", "stats")
    assert "remap_vertex_features" in mc_utils.make_manifold_device.__doc__ and "remove_duplicates" in mc_utils.make_manifold_device.__doc__
