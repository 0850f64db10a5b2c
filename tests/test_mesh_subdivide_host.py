"""CPU: the mesh refinement rules as ``tests/mesh_subdivide_reference.py`` restates them -- the
hand-worked case of the section, the properties a conforming split must have --, ``subdivide_vertex_features`` on torch's
CPU path, the additive header ``include/qf_mesh_subdivide.h`` held to the bars ``tests/test_abi.py`` holds
``include/qf_hip.h`` to, and the refusals ``qf_mesh_edges_*`` / ``qf_mesh_subdivide_*`` decide before any launch."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import mesh_subdivide_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qf_mesh_subdivide.h")
NEW_FUNCTIONS = ["qf_mesh_edges_count", "qf_mesh_edges_emit", "qf_mesh_edges_workspace_bytes", "qf_mesh_subdivide_count",
                 "qf_mesh_subdivide_emit", "qf_mesh_subdivide_workspace_bytes"]
WORKSPACE_FUNCTIONS = {"qf_mesh_edges_workspace_bytes", "qf_mesh_subdivide_workspace_bytes"}

# V = 4, two faces that share edge e1 = (1, 2)
HAND_VERTS = np.array([[0, 0, 0], [1, 0, 0.25], [0, 1, 0.5], [1.5, 1.25, -1]], dtype=np.float64)
HAND_FACES = np.array([[0, 1, 2], [2, 1, 3]], dtype=np.int64)
HAND_EDGES = [[0, 1], [1, 2], [0, 2], [1, 3], [2, 3]]
HAND_FACE_EDGES = [[0, 1, 2], [1, 3, 4]]
# marks -> faces, face_map, vertex_parents[4:], counts
HAND_CASES = {
    "e1": ([0, 1, 0, 0, 0], [(1, 4, 0), (4, 2, 0), (2, 4, 3), (4, 1, 3)], [0, 0, 1, 1], [(1, 2)], [4, 5, 0, 2, 0, 0, 0]),
    "e0_e1": ([1, 1, 0, 0, 0], [(4, 1, 5), (0, 4, 5), (0, 5, 2), (2, 5, 3), (5, 1, 3)], [0, 0, 0, 1, 1], [(0, 1), (1, 2)],
              [5, 6, 0, 1, 1, 0, 0]),
    "all": (None, [(0, 4, 6), (4, 1, 5), (6, 5, 2), (4, 5, 6), (2, 5, 8), (5, 1, 7), (8, 7, 3), (5, 7, 8)],
            [0, 0, 0, 0, 1, 1, 1, 1], [(0, 1), (1, 2), (0, 2), (1, 3), (2, 3)], [8, 9, 0, 0, 0, 2, 0]),
}


def random_mesh(n_v, n_f, seed, degenerate=0.05):
    """A seeded soup: random faces, a share of them degenerate."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n_v, 3))
    f = rng.integers(0, n_v, size=(n_f, 3))
    bad = rng.random(n_f) < degenerate
    f[bad, 1] = f[bad, 0]
    return v, f


# --------------------------------------------------------------------------------------------------------- 1. the rules
def test_hand_worked_edges():
    e, fe, c = ref.edges(HAND_FACES, 4)
    assert e.tolist() == HAND_EDGES and fe.tolist() == HAND_FACE_EDGES and c.tolist() == [5, 0, 0, 4]


@pytest.mark.parametrize("name", sorted(HAND_CASES))
def test_hand_worked_case(name):
    marks, faces, face_map, new_parents, counts = HAND_CASES[name]
    v, f, fm, vp, c = ref.subdivide(HAND_VERTS, HAND_FACES, marks)
    assert f.tolist() == [list(t) for t in faces] and fm.tolist() == face_map and c.tolist() == counts
    assert vp[:4].tolist() == [[i, i] for i in range(4)] and vp[4:].tolist() == [list(t) for t in new_parents]
    assert np.array_equal(v[:4].view(np.int64), HAND_VERTS.view(np.int64))
    for row, (a, b) in zip(v[4:], new_parents):
        assert np.array_equal(row, 0.5 * (HAND_VERTS[a] + HAND_VERTS[b]))


def test_reference_corner_rules():
    v = np.zeros((6, 3))
    # a degenerate face has no edges and is copied unsplit; the quad's cut follows the indices, not the positions
    f = np.array([[0, 1, 2], [3, 3, 4], [2, 1, 0]])
    e, fe, c = ref.edges(f, 6)
    assert fe.tolist() == [[0, 1, 2], [-1, -1, -1], [1, 0, 2]] and c.tolist() == [3, 1, 0, 0]
    out = ref.subdivide(v, f)
    assert out[1][4].tolist() == [3, 3, 4] and out[2].tolist() == [0] * 4 + [1] + [2] * 4 and out[4].tolist() == [9, 9, 1, 0, 0, 2, 0]
    two = ref.subdivide(v, np.array([[5, 1, 0]]), [1, 1, 0])          # edge j = 2 unmarked: u = (5, 1, 0), u0 > u2
    assert two[1].tolist() == [[6, 1, 7], [5, 6, 0], [6, 7, 0]]
    # an invalid index: nothing is produced, only its count
    bad = ref.edges(np.array([[0, 1, 6], [0, -1, 2], [0, 1, 2]]), 6)
    assert bad[0].shape == (0, 2) and bad[2].tolist() == [0, 0, 2, 0]
    bad = ref.subdivide(v, np.array([[0, 1, 6]]))
    assert bad[0].shape == (0, 3) and bad[4].tolist() == [0, 0, 0, 0, 0, 0, 1]
    empty = ref.subdivide(v, np.zeros((0, 3), np.int64))
    assert empty[0].shape == (6, 3) and empty[4].tolist() == [0, 6, 0, 0, 0, 0, 0]


def _area(p):
    return 0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)


@pytest.mark.parametrize("seed,share", [(1, 0.1), (2, 0.5), (3, 1.0)])
def test_children_lie_in_their_parent_and_tile_it(seed, share):
    rng = np.random.default_rng(seed)
    v, f = random_mesh(60, 400, seed)
    n_e = ref.edges(f, 60)[2][0]
    marks = rng.random(n_e) < share
    ov, of, fm, vp, c = ref.subdivide(v, f, marks)
    assert c[0] == len(of) == c[2] + 2 * c[3] + 3 * c[4] + 4 * c[5] and c[1] == 60 + marks.sum() and c[2:6].sum() == 400
    assert np.array_equal(fm, np.sort(fm)) and set(fm.tolist()) == set(range(400))
    # every corner of a child is a corner of its parent or the midpoint of two of them
    parent = f[fm]
    for k in range(3):
        corner = vp[of[:, k]]
        assert ((corner[:, :1] == parent).any(axis=1) & (corner[:, 1:] == parent).any(axis=1)).all()
    # same winding, and the children's areas sum to the parent's
    normal = lambda p: np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    assert (np.einsum("ij,ij->i", normal(ov[of]), normal(v[parent])) >= 0).all()
    total = np.zeros(400)
    np.add.at(total, fm, _area(ov[of]))
    want = _area(v[f])
    assert np.abs(total - want).max() <= 1e-12 * want.max()
    assert (np.abs(total - want) <= 1e-12 * np.maximum(want, 1e-2)).all()          # slivers: relative to a floor


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_closed_manifold_stays_closed_under_any_marks(seed):
    v, f = ref.octahedron(2)
    assert ref.directed_edge_balance(f) == 0 and ref.edges(f, len(v))[2].tolist() == [192, 0, 0, 0]
    rng = np.random.default_rng(seed)
    marks = rng.random(192) < (0.3, 0.5, 0.8)[seed]
    ov, of = ref.subdivide(v, f, marks)[:2]
    assert ref.directed_edge_balance(of) == 0
    assert ref.edges(of, len(ov))[2][3] == 0                       # no boundary edge: a T-junction would make two
    # splitting one face's edge in that face alone leaves a T-junction, and the balance sees it
    broken = np.concatenate([f[1:], [[f[0, 0], len(v), f[0, 2]], [len(v), f[0, 1], f[0, 2]]]])
    assert ref.directed_edge_balance(broken) > 0


# -------------------------------------------------------------------------------------------------- 2. the vertex table
def test_subdivide_vertex_features_cpu():
    from quadraturefields_amd import _C, baking
    rng = np.random.default_rng(5)
    v, f = random_mesh(30, 80, 5)
    marks = rng.random(ref.edges(f, 30)[2][0]) < 0.5
    vp = ref.subdivide(v, f, marks)[3]
    feats = torch.from_numpy(rng.normal(size=(30, 3 + 7 * 2 + 1)).astype(np.float32))
    out = baking.subdivide_vertex_features(feats, vp)
    assert type(out) is torch.Tensor and out.shape == (len(vp), 18) and torch.equal(out[:30], feats)
    want = (feats[vp[30:, 0]] + feats[vp[30:, 1]]) * 0.5
    assert torch.equal(out[30:], want) and len(vp) > 30
    assert torch.equal(baking.subdivide_vertex_features(feats, torch.from_numpy(vp)), out)
    # two levels chained: the second level's parents are rows of the first
    v1, f1 = ref.subdivide(v, f, marks)[:2]
    vp2 = ref.subdivide(v1, f1)[3]
    chained = np.concatenate([vp, vp2[len(vp):]])
    two = baking.subdivide_vertex_features(feats, chained)
    assert torch.equal(two[:len(vp)], out)
    assert torch.equal(two[len(vp):], (out[vp2[len(vp):, 0]] + out[vp2[len(vp):, 1]]) * 0.5)
    module = baking.VertexBakedFeatures(feats, train_density=False)
    refined = baking.subdivide_vertex_features(module, vp)
    assert isinstance(refined, baking.VertexBakedFeatures) and refined.n_lobes == 2 and not refined.train_density
    assert refined.table.shape == (len(vp), _C.vertex_row_stride(2)) and torch.equal(refined.features(), out)
    with pytest.raises(ValueError, match=r"\(v, v\)"):
        baking.subdivide_vertex_features(feats, vp[::-1].copy())
    with pytest.raises(ValueError):
        baking.subdivide_vertex_features(feats, vp[:10])
    with pytest.raises(ValueError):
        baking.subdivide_vertex_features(feats, vp.astype(np.float64))
    with pytest.raises(IndexError):
        baking.subdivide_vertex_features(feats, np.concatenate([vp, [[0, len(vp) + 5]]]))
    with pytest.raises(ValueError, match="not a chain"):
        baking.subdivide_vertex_features(feats, np.concatenate([vp, [[0, len(vp)]]]))
    with pytest.raises(ValueError, match="vertices"):
        baking.subdivide_vertex_features(feats, vp, radiance_field=object())
    quantised = object.__new__(baking.QuantisedVertexFeatures)
    with pytest.raises(TypeError, match="quantise after refining"):
        baking.subdivide_vertex_features(quantised, vp)


def test_mark_edges_longer_than_and_wrapper_refusals():
    from quadraturefields_amd import mc_utils
    v = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 3, 0]], dtype=torch.float64)
    e = torch.tensor([[0, 1], [0, 2], [1, 2]])
    assert mc_utils.mark_edges_longer_than(v, e, 1.0).tolist() == [0, 1, 1]
    assert mc_utils.mark_edges_longer_than(v, e, 3.1).tolist() == [0, 0, 1]
    assert mc_utils.mark_edges_longer_than(v, e, 3.1).dtype == torch.uint8
    f = torch.zeros((2, 3), dtype=torch.int64)
    with pytest.raises(ValueError, match="device tensors"):
        mc_utils.mesh_edges_device(f, 4)
    with pytest.raises(ValueError, match="device tensors"):
        mc_utils.subdivide_mesh_device(v, f)
    with pytest.raises(TypeError):
        mc_utils.mesh_edges_device(f.numpy(), 4)
    with pytest.raises(TypeError):
        mc_utils.mesh_edges_device(f.to(torch.float32), 4)
    with pytest.raises(ValueError):
        mc_utils.mesh_edges_device(f[:, :2], 4)
    from quadraturefields_amd.mesh_io import TriMesh
    with pytest.raises(ValueError, match="levels"):
        mc_utils.subdivide_mesh(TriMesh(v.numpy(), np.array([[0, 1, 2]])), levels=0)


# --------------------------------------------------------------------------------------------------- 3. the new header
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
    assert _functions(HEADER) == NEW_FUNCTIONS == sorted(_C._MESH_SUBDIVIDE_SIGNATURES)
    assert not set(NEW_FUNCTIONS) & set(_C.EXPORTED_SYMBOLS) and _C.ABI_VERSION == 6
    for other in ("qf_hip.h", "qf_mesh_compact.h", "qf_vertex_baked.h", "qf_vertex_train.h", "qf_vertex_quant.h"):
        assert not set(NEW_FUNCTIONS) & set(_functions(os.path.join(ROOT, "include", other)))
    raw = ctypes.CDLL(_C.LIB_PATH)
    for name in NEW_FUNCTIONS:
        getattr(raw, name)                               # AttributeError if the library does not export it
        fn = getattr(lib, name)
        restype, argtypes = _C._MESH_SUBDIVIDE_SIGNATURES[name]
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)
    assert len(_C.MESH_EDGES_COUNTS) == 4 and len(_C.MESH_SUBDIVIDE_COUNTS) == 7
    assert _C.MESH_EDGES_COUNTS == ref.EDGE_COUNT_NAMES and _C.MESH_SUBDIVIDE_COUNTS == ref.SPLIT_COUNT_NAMES


def test_every_new_entry_point_takes_the_callers_stream_and_is_indexed():
    from quadraturefields_amd import _C
    protos = _prototypes(HEADER)
    assert sorted(protos) == NEW_FUNCTIONS
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, params in protos.items():
        if name not in WORKSPACE_FUNCTIONS:              # host computations: no device work, no stream
            assert re.search(r"void\s*\*\s*stream\s*$", params.strip()), f"{name}: the last parameter is not void *stream"
        assert len([p for p in params.split(",") if p.strip()]) == len(_C._MESH_SUBDIVIDE_SIGNATURES[name][1]), name
        assert f"`{name}`" in text, f"INTEGRATION.md does not name {name}"


def test_new_header_is_plain_c(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "plain.c"
    src.write_text("\n".join(['#include <stdio.h>', '#include "qf_mesh_subdivide.h"', "int main(void) {",
                              'printf("%d %d %d\\n", QF_MESH_EDGES_COUNTS, QF_MESH_SUBDIVIDE_COUNTS, QF_ABI_VERSION);',
                              "return 0;", "}"]))
    exe = tmp_path / "plain"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split() == ["4", "7", "6"]


def test_build_lists_the_new_source_and_header():
    from quadraturefields_amd import build
    assert dict(build.SOURCES)["mesh_subdivide.hip"] == ["-ffp-contract=off"]
    assert HEADER in build._deps("mesh_subdivide.hip")


# ----------------------------------------------------------------------------------------------------------- 4. refusals
def test_workspace_bytes_edge_values(lib):
    edges_ws, split_ws = lib.qf_mesh_edges_workspace_bytes, lib.qf_mesh_subdivide_workspace_bytes
    for v, f in ((0, 5), (-1, 5), (2 ** 31, 5), (5, -1), (5, (2 ** 31 - 1) // 3 + 1), (5, 2 ** 31)):
        assert edges_ws(v, f) == -1, (v, f)
    assert edges_ws(1, 0) > 0 and edges_ws(2 ** 31 - 1, 0) > 0 and edges_ws(5, (2 ** 31 - 1) // 3) > 0
    assert edges_ws(100, 201) >= edges_ws(100, 200) > edges_ws(100, 0)
    # the table: a power of two >= 6 F slots of two 4-byte words, on top of 17 bytes per half-edge... at least
    assert edges_ws(100, 200) >= 2 * 4 * 2048 + 9 * 600 + 200
    for v, f, e in ((0, 5, 9), (2 ** 31, 5, 9), (5, -1, 0), (5, 2 ** 29, 9), (5, 5, -1), (5, 5, 16), (2 ** 31 - 10, 5, 10)):
        assert split_ws(v, f, e) == -1, (v, f, e)
    assert split_ws(1, 0, 0) > 0 and split_ws(5, 5, 15) > 0 and split_ws(2 ** 31 - 10, 5, 9) > 0
    assert split_ws(5, 2 ** 29 - 1, 0) > 0
    assert split_ws(100, 200, 300) >= 5 * 200 + 8 * 300


def test_entry_points_refuse_before_any_launch(lib):
    """Sizes out of range, NULL pointers, a short workspace and capacities out of range are decided on the host: status
    -1 without a device."""
    p = 4096                         # a non-NULL address that is never dereferenced: every call below is refused first
    need = lib.qf_mesh_edges_workspace_bytes(100, 200)
    ok = dict(f=p, F=200, V=100, ws=p, ws_bytes=need, counts=p)

    def count(**kw):
        a = dict(ok, **kw)
        return lib.qf_mesh_edges_count(a["f"], a["F"], a["V"], a["ws"], a["ws_bytes"], a["counts"], None)

    def emit(n_e=0, e=None, fe=p, **kw):
        a = dict(ok, **kw)
        return lib.qf_mesh_edges_emit(a["f"], a["F"], a["V"], a["ws"], a["ws_bytes"], e, n_e, fe, None)

    for call in (count, emit):
        for bad in (dict(V=0), dict(V=2 ** 31), dict(F=-1), dict(F=2 ** 30), dict(f=None), dict(ws=None),
                    dict(ws_bytes=need - 1), dict(ws_bytes=0)):
            assert call(**bad) == -1, (call.__name__, bad)
    assert count(counts=None) == -1
    assert emit(n_e=-1) == -1 and emit(n_e=601, e=p) == -1 and emit(n_e=1) == -1 and emit(fe=None) == -1

    need = lib.qf_mesh_subdivide_workspace_bytes(100, 200, 300)
    ok = dict(v=p, f=p, F=200, V=100, fe=p, E=300, mark=p, ws=p, ws_bytes=need, counts=p)

    def scount(**kw):
        a = dict(ok, **kw)
        return lib.qf_mesh_subdivide_count(a["f"], a["F"], a["V"], a["fe"], a["E"], a["mark"], a["ws"], a["ws_bytes"],
                                           a["counts"], None)

    def semit(n_ov=0, n_of=0, ov=None, of=None, **kw):
        a = dict(ok, **kw)
        return lib.qf_mesh_subdivide_emit(a["v"], a["f"], a["F"], a["V"], a["fe"], a["E"], a["mark"], a["ws"], a["ws_bytes"],
                                          ov, n_ov, of, n_of, None, None, None)

    for call in (scount, semit):
        for bad in (dict(V=0), dict(V=2 ** 31), dict(F=-1), dict(F=2 ** 29), dict(E=-1), dict(E=601), dict(V=2 ** 31 - 300),
                    dict(f=None), dict(fe=None), dict(mark=None), dict(ws=None), dict(ws_bytes=need - 1)):
            assert call(**bad) == -1, (call.__name__, bad)
    assert scount(counts=None) == -1 and semit(v=None) == -1
    assert semit(n_ov=-1) == -1 and semit(n_ov=401, ov=p) == -1 and semit(n_of=-1) == -1 and semit(n_of=801, of=p) == -1
    assert semit(n_ov=1) == -1 and semit(n_of=1) == -1               # a capacity without a buffer
