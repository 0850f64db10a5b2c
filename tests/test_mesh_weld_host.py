"""The numpy restatements of the weld rule (tests/mesh_weld_reference.py) pinned on inputs whose
outcome is worked out by hand, against one another on seeded clouds, and the new header against its binding."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import mesh_decimate_reference as ref
from tests import mesh_weld_reference as wref

NAN_A = 0x7FF8000000ABCDEF          # a NaN with a payload
ONE_ULP = np.nextafter(1.0, 2.0)


def _nan(bits):
    return np.array([bits], dtype=np.uint64).view(np.float64)[0]


def _x(*xs):
    """Points on the x axis."""
    return np.array([[x, 0.0, 0.0] for x in xs], dtype=np.float64)


QUAD = [(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (1.0, 1.0, 0.0), (0.0, 1.0, 0.0)]

# name -> (vertices, faces or None, h, vertex_class, vertex_map, out_faces, counts): worked by hand from the rule.  counts
# is [V', classes of two or more, largest class, faces that collapse, largest cell (h > 0), loose, out of range, invalid].
HAND_CASES = {
    # 0 - 0.6 and 0.6 - 1.2 are 0.6 apart (0.36 <= 0.49), 0 - 1.2 is not (1.44): {0, 1, 2} only by transitivity; {3, 4}
    # coincide.  Face (0, 3, 4) becomes (0, 1, 1) and (1, 2, 3) becomes (0, 0, 1): both collapse.  s = 1.4: the cells
    # along x are 0, 0, 0 and floor(5 / 1.4) = 3, 3: the fullest holds 3.
    "line": (_x(0.0, 0.6, 1.2, 5.0, 5.0), [[0, 3, 4], [1, 2, 3]], 0.7, [0, 0, 0, 1, 1], [0, 3], [[0, 1, 1], [0, 0, 1]],
             [2, 2, 3, 2, 3, 0, 0, 0]),
    # dx * dx = 0.25 <= h * h = 0.25: the ball is closed.  s = 1: both in cell 0.
    "closed_ball": (_x(0.0, 0.5), None, 0.5, [0, 0], [0], [], [1, 1, 2, 0, 2, 0, 0, 0]),
    # h * h = 0.2499900001 < 0.25.  s = 0.99998: 0.5 / s = 0.50001, still cell 0.
    "just_outside": (_x(0.0, 0.5), None, 0.49999, [0, 1], [0, 1], [], [2, 0, 1, 0, 2, 0, 0, 0]),
    # -0.0 == +0.0 in every coordinate
    "signed_zero": (np.array([[-0.0, 0.0, 0.0], [0.0, -0.0, 0.0]]), None, 0.0, [0, 0], [0], [], [1, 1, 2, 0, 0, 0, 0, 0]),
    "one_ulp": (_x(1.0, ONE_ULP), None, 0.0, [0, 1], [0, 1], [], [2, 0, 1, 0, 0, 0, 0, 0]),
    # vertices 0, 2, 3 (NaN; 2 and 3 with the same bits) and 5 (inf) are loose, 1 and 4 coincide
    "loose": (np.array([[np.nan, 0, 0], [1, 1, 1], [_nan(NAN_A), 0, 0], [_nan(NAN_A), 0, 0], [1, 1, 1], [np.inf, 0, 0]]),
              [[0, 1, 4], [2, 3, 5]], 0.0, [0, 1, 2, 3, 1, 4], [0, 1, 2, 3, 5], [[0, 1, 1], [2, 3, 4]], [5, 1, 2, 1, 0, 4, 0, 0]),
    # the same at h = 0.1: s = 0.2, 1 and 4 share the cell (5, 5, 5)
    "loose_tolerance": (np.array([[np.nan, 0, 0], [1, 1, 1], [_nan(NAN_A), 0, 0], [_nan(NAN_A), 0, 0], [1, 1, 1], [np.inf, 0, 0]]),
                        None, 0.1, [0, 1, 2, 3, 1, 4], [0, 1, 2, 3, 5], [], [5, 1, 2, 0, 2, 4, 0, 0]),
    # h = 0.5, s = 1: the pairs (0.9, 1.1), (-0.1, 0.1) and (-1.1, -0.9) are 0.2 apart and straddle the borders 1, 0 and
    # -1; no other pair is within 0.5 (the next nearest are 0.8 apart).  floor puts the six in the cells 0, -1, -2, 1, 0,
    # -1, so the fullest cell holds 2; truncation towards zero would put four in cell 0.
    "straddle": (_x(0.9, -0.1, -1.1, 1.1, 0.1, -0.9), None, 0.5, [0, 1, 2, 0, 1, 2], [0, 1, 2], [], [3, 3, 2, 0, 2, 0, 0, 0]),
    # the unit square as two triangles with a corner each: corners 3 and 4 are corners 0 and 2 again
    "soup_quad": (np.array([QUAD[0], QUAD[1], QUAD[2], QUAD[0], QUAD[2], QUAD[3]]), [[0, 1, 2], [3, 4, 5]], 0.0,
                  [0, 1, 2, 0, 2, 3], [0, 1, 2, 5], [[0, 1, 2], [0, 2, 3]], [4, 2, 2, 0, 0, 0, 0, 0]),
    # 0 and 1 are 0.1 apart: face (0, 1, 2) becomes (0, 0, 1), stays and is counted.  s = 0.4: cells 0, 0, 12, (12, 12).
    "collapse": (np.array([[0, 0, 0], [0.1, 0, 0], [5, 0, 0], [5, 5, 0]], dtype=np.float64), [[0, 1, 2], [0, 2, 3]], 0.2,
                 [0, 0, 1, 2], [0, 2, 3], [[0, 0, 1], [0, 1, 2]], [3, 1, 2, 1, 2, 0, 0, 0]),
    # a face that is degenerate before is not counted
    "degenerate_before": (_x(0.0, 0.0, 1.0), [[0, 0, 2], [0, 1, 2]], 0.0, [0, 0, 1], [0, 2], [[0, 0, 1], [0, 0, 1]],
                          [2, 1, 2, 1, 0, 0, 0, 0]),
    "no_faces": (_x(2.0, 3.0, 2.0), None, 0.0, [0, 1, 0], [0, 1], [], [2, 1, 2, 0, 0, 0, 0, 0]),
    "one_vertex": (_x(7.0), None, 0.0, [0], [0], [], [1, 0, 1, 0, 0, 0, 0, 0]),
    "one_vertex_tolerance": (_x(7.0), None, 0.25, [0], [0], [], [1, 0, 1, 0, 1, 0, 0, 0]),
}

# name -> (vertices, faces, h, counts): refused, nothing is produced
REFUSED_CASES = {
    # 1e300 / 2e-8 = 5e307 is finite and far beyond 2^51
    "out_of_range": (_x(1e300, 0.0), None, 1e-8, [0, 0, 0, 0, 0, 0, 1, 0]),
    # 1e300 / 2^-509 is not finite
    "quotient_overflows": (_x(1e300, 0.0, -1e300), None, 1e-200, [0, 0, 0, 0, 0, 0, 2, 0]),
    "invalid_face": (_x(0.0, 0.0, 1.0), [[0, 1, 2], [0, 1, 3], [-1, 0, 1]], 0.0, [0, 0, 0, 0, 0, 0, 0, 2]),
    "both": (_x(1e300, 0.0), [[0, 1, 2]], 1e-8, [0, 0, 0, 0, 0, 0, 1, 1]),
}


def restatements(h):
    if h == 0:
        return [lambda v, f, h: wref.weld_exact(v, f)]
    return [wref.weld_brute, wref.weld_cells]


def same(a, b):
    """Two restatement tuples agree bit for bit."""
    if a[0] is None or b[0] is None:
        return a[0] is None and b[0] is None and a[4].tolist() == b[4].tolist()
    return (a[0].tobytes() == b[0].tobytes() and all(np.array_equal(x, y) for x, y in zip(a[1:4], b[1:4]))
            and a[4].tolist() == b[4].tolist())


@pytest.mark.parametrize("name", sorted(HAND_CASES))
def test_hand_worked_case(name):
    v, f, h, vertex_class, vertex_map, faces, counts = HAND_CASES[name]
    for weld in restatements(h):
        out_v, out_f, vmap, vcls, c = weld(v, f, h)
        assert vcls.tolist() == vertex_class and vmap.tolist() == vertex_map and out_f.tolist() == faces
        assert c.tolist() == counts
        assert out_v.tobytes() == np.ascontiguousarray(v, np.float64)[vertex_map].tobytes()      # the roots' rows, by bits
        assert np.array_equal(vcls[vmap], np.arange(len(vertex_map)))
    assert same(wref.weld(v, f, h), restatements(h)[0](v, f, h))


@pytest.mark.parametrize("name", sorted(REFUSED_CASES))
def test_refused_case(name):
    v, f, h, counts = REFUSED_CASES[name]
    for weld in restatements(h):
        out = weld(v, f, h)
        assert out[:4] == (None, None, None, None) and out[4].tolist() == counts


def test_tolerance_must_be_finite_and_not_negative():
    for h in (-1.0, -0.0 - 1e-300, np.nan, np.inf):
        with pytest.raises(ValueError):
            wref.weld(_x(0.0), None, h)


def test_cell_edge():
    assert wref.cell_edge(0.5) == 1.0 and wref.cell_edge(1e-200) == 2.0 ** -509 and wref.cell_edge(2.0 ** -510) == 2.0 ** -509
    assert wref.cell_edge(1e154) == 2e154 and wref.cell_edge(1.5e154) == np.inf and wref.cell_edge(1e308) == np.inf
    # with a cell edge of +inf every vertex is in cell 0 and every finite pair links (h * h is +inf)
    out = wref.weld_brute(_x(-1e300, 0.0, 1e300), None, 1.5e154)
    assert out[3].tolist() == [0, 0, 0] and out[4].tolist() == [1, 1, 3, 0, 3, 0, 0, 0]
    assert same(out, wref.weld_cells(_x(-1e300, 0.0, 1e300), None, 1.5e154))


def test_signed_zeros_and_nan_payloads_pass_through():
    v = HAND_CASES["signed_zero"][0]
    out_v = wref.weld_exact(v, None)[0]
    assert out_v.view(np.uint64).tolist() == [[0x8000000000000000, 0, 0]]
    out_v = wref.weld_exact(HAND_CASES["loose"][0], None)[0]
    assert out_v.view(np.uint64)[2, 0] == out_v.view(np.uint64)[3, 0] == NAN_A


def test_identity_on_the_icosphere_and_idempotence():
    v, f = ref.icosphere(2)
    assert v.shape[0] == 162
    for h in (0.0, 1e-3):
        out = wref.weld(v, f, h)
        assert out[0].tobytes() == v.tobytes() and np.array_equal(out[1], f)                   # no linked pair: itself
        assert np.array_equal(out[2], np.arange(162)) and np.array_equal(out[3], np.arange(162))
        assert out[4][:4].tolist() == [162, 0, 1, 0]
    sv, sf = wref.soup(v, f)
    once = wref.weld_exact(sv, sf)
    assert once[4][0] == 162 and once[0][once[1]].tobytes() == sv[sf].tobytes()                # the same triangle soup
    twice = wref.weld_exact(once[0], once[1])
    assert twice[0].tobytes() == once[0].tobytes() and np.array_equal(twice[1], once[1])
    assert np.array_equal(twice[2], np.arange(162)) and twice[4][1] == 0
    jv, src = wref.repeated_sphere(2, 0, 1e-3)
    once = wref.weld(jv, None, 1e-3)
    assert once[4][0] == 162 and all(len(set(src[once[3] == c])) == 1 for c in range(162))
    twice = wref.weld(once[0], None, 1e-3)                                                     # roots are far apart
    assert twice[0].tobytes() == once[0].tobytes() and np.array_equal(twice[2], np.arange(162))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_three_restatements_agree_on_lattice_clouds(seed):
    v = wref.lattice_cloud(512, seed)
    f = np.random.default_rng(seed).integers(0, 512, (300, 3))
    exact = wref.weld_exact(v, f)
    assert 1 < exact[4][0] < 512
    # at a tolerance far below the lattice step the classes are the coincident points again
    for h in (1e-6, 0.25):
        brute, cells = wref.weld_brute(v, f, h), wref.weld_cells(v, f, h)
        assert same(brute, cells)
        assert brute[0].tobytes() == exact[0].tobytes() and all(np.array_equal(a, b) for a, b in zip(brute[1:4], exact[1:4]))
        assert brute[4][[0, 1, 2, 3, 5, 6, 7]].tolist() == exact[4][[0, 1, 2, 3, 5, 6, 7]].tolist()
    # at 0.75 steps nothing more links (the nearest distinct points are a step apart); at one step everything chains
    for h, jitter in ((0.75, 0.0), (1.0, 0.0), (0.3, 0.2)):
        w = v + np.random.default_rng(seed + 7).uniform(-jitter, jitter, v.shape)
        assert same(wref.weld_brute(w, f, h), wref.weld_cells(w, f, h))
    assert wref.weld_brute(v, f, 0.75)[4][0] == exact[4][0] and wref.weld_brute(v, f, 1.0)[4][0] < exact[4][0]


def test_chains_are_single_linkage():
    close, far = wref.chain(64, 0.9 * 0.01), wref.chain(64, 1.1 * 0.01)
    assert same(wref.weld_brute(close, None, 0.01), wref.weld_cells(close, None, 0.01))
    assert wref.weld_cells(close, None, 0.01)[4][:3].tolist() == [1, 1, 64]
    assert wref.weld_cells(far, None, 0.01)[4][:3].tolist() == [64, 0, 1]


# ------------------------------------------------------------------------------------------------------- the new header
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_NAME = "qf_mesh_weld.h"
HEADER = os.path.join(ROOT, "include", HEADER_NAME)
WORKSPACE = "qf_mesh_weld_workspace_bytes"
NEW_FUNCTIONS = sorted([WORKSPACE, "qf_mesh_weld_count", "qf_mesh_weld_emit"])


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
    assert _functions(HEADER) == NEW_FUNCTIONS == sorted(_C._MESH_WELD_SIGNATURES)
    assert not set(NEW_FUNCTIONS) & set(_C.EXPORTED_SYMBOLS) and _C.ABI_VERSION == 6
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if other != HEADER_NAME:
            assert not set(NEW_FUNCTIONS) & set(_functions(os.path.join(ROOT, "include", other))), other
    raw = ctypes.CDLL(_C.LIB_PATH)
    for name in NEW_FUNCTIONS:
        getattr(raw, name)                               # AttributeError if the library does not export it
        fn = getattr(lib, name)
        restype, argtypes = _C._MESH_WELD_SIGNATURES[name]
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)
    assert _C.MESH_WELD_COUNTS == wref.COUNT_NAMES and len(wref.COUNT_NAMES) == 8
    assert lib.qf_mesh_weld_workspace_bytes(0, 0) == -1 and lib.qf_mesh_weld_workspace_bytes(5, 2 ** 31) == -1
    assert lib.qf_mesh_weld_workspace_bytes(2 ** 31, 3) == -1 and lib.qf_mesh_weld_workspace_bytes(5, -1) == -1
    assert 0 < lib.qf_mesh_weld_workspace_bytes(5, 0) < lib.qf_mesh_weld_workspace_bytes(5000, 3)


def test_every_new_entry_point_takes_the_callers_stream_and_is_indexed():
    from quadraturefields_amd import _C
    protos = _prototypes(HEADER)
    assert sorted(protos) == NEW_FUNCTIONS
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, params in protos.items():
        if name != WORKSPACE:                            # a host computation: no device work, no stream
            assert re.search(r"void\s*\*\s*stream\s*$", params.strip()), f"{name}: the last parameter is not void *stream"
        assert len([p for p in params.split(",") if p.strip()]) == len(_C._MESH_WELD_SIGNATURES[name][1]), name
        assert f"`{name}`" in text, f"INTEGRATION.md does not name {name}"


def test_new_header_is_plain_c(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "plain.c"
    src.write_text("\n".join(['#include <stdio.h>', f'#include "{HEADER_NAME}"', "int main(void) {",
                              'printf("%d %d\\n", QF_MESH_WELD_COUNTS, QF_ABI_VERSION);', "return 0;", "}"]))
    exe = tmp_path / "plain"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split() == ["8", "6"]


def test_build_lists_the_new_source_and_header():
    from quadraturefields_amd import build
    assert dict(build.SOURCES)["mesh_weld.hip"] == ["-ffp-contract=off"]
    assert HEADER in build._deps("mesh_weld.hip")
    text = open(os.path.join(build.CSRC, "mesh_weld.hip")).read()
    assert f'#include "{HEADER_NAME}"' in text
    code = re.sub(r"//.*", "", text)
    assert "fma" not in code and "float " not in code          # fp64 only, nothing fused by hand
    assert "hipLaunchCooperativeKernel" not in code and not re.search(r"atomicAdd\s*\(\s*\(?\s*(double|float)", code)


def test_wrappers_refuse_host_tensors_and_bad_arguments():
    import torch
    from quadraturefields_amd import baking, mc_utils
    v, f = HAND_CASES["soup_quad"][0], np.asarray(HAND_CASES["soup_quad"][1])
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    with pytest.raises(ValueError, match="device tensors"):
        mc_utils.weld_vertices_device(tv, tf)
    with pytest.raises(ValueError, match="device tensors"):
        mc_utils.weld_vertices_device(tv)
    with pytest.raises(TypeError):
        mc_utils.weld_vertices_device(v, tf)
    with pytest.raises(ValueError):
        mc_utils.weld_vertices_device(tv[:, :2], tf)
    with pytest.raises(TypeError):
        mc_utils.weld_vertices_device(tv.to(torch.int64), tf)
    for h in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tolerance"):
            mc_utils.weld_vertices_device(tv, tf, h)
    assert mc_utils.WeldedMesh._fields == ("vertices", "faces", "vertex_map", "vertex_class", "stats")
    assert "discards the atlas" in mc_utils.weld_vertices.__doc__
    table = torch.arange(12, dtype=torch.float32).reshape(6, 2)
    with pytest.raises(ValueError, match="reduce"):
        baking.weld_vertex_features(table, HAND_CASES["soup_quad"][3], 4, reduce="sum")
    with pytest.raises(ValueError):
        baking.weld_vertex_features(table, [0, 1, 2], 4)
    with pytest.raises(IndexError):
        baking.weld_vertex_features(table, HAND_CASES["soup_quad"][3], 3)
    with pytest.raises(ValueError, match="without a member"):
        baking.weld_vertex_features(table, HAND_CASES["soup_quad"][3], 5)


def test_weld_vertex_features_on_the_host():
    import torch
    from quadraturefields_amd import baking
    vertex_class, vertex_map = HAND_CASES["soup_quad"][3], HAND_CASES["soup_quad"][4]
    table = torch.tensor([[1.0, -0.0], [2.0, 1e-8], [3.0, 1.0], [5.0, -0.0], [4.0, 1e8], [6.0, 0.5]], dtype=torch.float32)
    first = baking.weld_vertex_features(table, vertex_class, 4)
    assert torch.equal(first.view(torch.int32), baking.remap_vertex_features(table, vertex_map).view(torch.int32))
    mean = baking.weld_vertex_features(table, np.asarray(vertex_class), 4, reduce="mean")
    t = table.numpy().astype(np.float64)
    want = np.stack([(t[0] + t[3]) / 2.0, t[1] / 1.0, (t[2] + t[4]) / 2.0, t[5] / 1.0]).astype(np.float32)
    assert mean.numpy().tobytes() == want.tobytes() and mean.numpy()[0, 1] == 0 and np.signbit(mean.numpy()[0, 1])
    again = baking.weld_vertex_features(table, torch.tensor(vertex_class), 4, reduce="mean")
    assert torch.equal(again.view(torch.int32), mean.view(torch.int32))
