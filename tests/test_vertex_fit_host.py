"""The numpy restatement of the surface fit of the vertex table (tests/vertex_fit_reference.py)
pinned on an input worked out by hand and on the properties the design rests on, with the samples of the project's own
sampler restatement (tests/mesh_sample_reference.py); and the new header against its binding."""
import ctypes
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import mesh_sample_reference as sampler
from tests import vertex_fit_reference as ref

LAMBDA = 1.0 / 64


@functools.lru_cache(maxsize=None)
def sphere_samples(level, per_face, seed=0):
    v, f = sampler.icosphere(level)
    points, face, bary, counts = sampler.sample(v, f, per_face * f.shape[0], seed=seed)
    assert not counts[:4].any()
    return v, f, points, face, bary


def field(p):
    """The held-out check's three columns: two oscillating ones and a positive one with a wide range."""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([np.sin(8 * x) * np.cos(8 * y), np.cos(8 * z + 1), np.exp(3 * np.sin(8 * x + y))], axis=1)


def test_one_triangle_by_hand():
    # Samples at corner 0, at corner 1 and at the midpoint of the edge between them; x0 = (0, 0, 7); y = 1, 2, 4.
    #   M = [[1 + 1/4, 1/4, 0], [1/4, 1 + 1/4, 0], [0, 0, 0]],  m = (3/2, 3/2, 0),  so d = (3/2, 3/2, 0): vertex 2 is inactive.
    #   lambda = 1/2:  a = 5/4 + 3/4 = 2 for vertices 0 and 1, inv = 1/2; vertex 2 has a = 0, inv = 0.
    #   e = y (b_2 is zero, so x0[2] never enters):  B = (1 + 4/2, 2 + 4/2, 0) = (3, 4, 0).
    #   S = P = (3/2, 2, 0), rho = 3 * 3/2 + 4 * 2 = 25/2.
    #   q = A P = (5/4 * 3/2 + 1/4 * 2 + 3/4 * 3/2, 1/4 * 3/2 + 5/4 * 2 + 3/4 * 2, 0) = (7/2, 35/8, 0),
    #   pi = 3/2 * 7/2 + 2 * 35/8 = 14, alpha = 25/28: after one step Z = 25/28 * (3/2, 2, 0).
    #   The exact solution of [[2, 1/4], [1/4, 2]] Z = (3, 4) is Z = (80/63, 116/63); CG on two unknowns is there after
    #   two steps.
    faces = np.array([[0, 1, 2]])
    face = np.array([0, 0, 0])
    bary = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.5, 0.5, 0.0]])
    y = np.array([[1.0], [2.0], [4.0]], dtype=np.float32)
    x0 = np.array([[0.0], [0.0], [7.0]], dtype=np.float32)
    a = ref.assemble(faces, 3, face, bary, y, x0, 0.5)
    assert a.gram.tolist() == [[1.25, 0.25, 0.0, 0.25, 1.25, 0.0, 0.0, 0.0, 0.0]]
    assert a.mass.tolist() == [1.5, 1.5, 0.0] and a.inv.tolist() == [0.5, 0.5, 0.0]
    assert a.rhs.tolist() == [[3.0], [4.0], [0.0]]
    assert a.counts.tolist() == [0, 0, 0, 0, 0, 1, 0, 0]
    assert ref.apply(a, np.array([[1.5], [2.0], [0.0]])).tolist() == [[3.5], [4.375], [0.0]]
    iterates = list(ref.iterate(a, 2))
    assert iterates[0].tolist() == [[0.0], [0.0], [0.0]]
    alpha = 12.5 / 14.0
    assert iterates[1].tolist() == [[alpha * 1.5], [alpha * 2.0], [0.0]]
    assert np.abs(iterates[2][:, 0] - np.array([80.0 / 63.0, 116.0 / 63.0, 0.0])).max() < 1e-15
    table, stats, counts = ref.solve(a, 2)
    assert table.dtype == np.float32 and table[2, 0] == 7.0              # the inactive vertex keeps its prior row
    assert table[:2, 0].tolist() == [np.float32(80.0 / 63.0), np.float32(116.0 / 63.0)]
    assert stats[0, 0] == 5.0 and stats[0, 1] < 1e-15                    # |B| = sqrt(9 + 16)
    # The clamp.  The fitted 80/63 and 116/63 lie inside [0, 4], the range of a corner's prior entry and the face's
    # targets, so clamping the column moves nothing:
    held, _, counts = ref.solve(a, 2, clamp_mask=1)
    assert counts[6] == 0 and np.array_equal(held, table)
    # A third sample that extrapolates, b = (3/2, -1/2, 0), with target 9, prior (1, 2) and lambda = 0: the normal
    # equations [[13/4, -3/4], [-3/4, 5/4]] X = (29/2, -5/2) give X = (65/14, 11/14).  The bounds are [1, 9] at both
    # corners: 11/14 is below them and becomes 1, the only entry moved.
    bary4 = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.5, -0.5, 0.0]])
    y4 = np.array([[1.0], [2.0], [9.0]], dtype=np.float32)
    x4 = np.array([[1.0], [2.0], [7.0]], dtype=np.float32)
    a4 = ref.assemble(faces, 3, face, bary4, y4, x4, 0.0)
    assert a4.lo[:2, 0].tolist() == [1.0, 1.0] and a4.hi[:2, 0].tolist() == [9.0, 9.0]
    free, _, _ = ref.solve(a4, 2)
    held, _, counts = ref.solve(a4, 2, clamp_mask=1)
    assert np.abs(free[:2, 0] - np.array([65.0 / 14.0, 11.0 / 14.0])).max() < 1e-6
    assert counts[6] == 1 and held[0, 0] == free[0, 0] and held[1, 0] == 1.0


def test_counts_and_refusals():
    faces = np.array([[0, 1, 2], [1, 1, 3], [0, 2, 9], [2, 1, 3]])      # one repeated index, one out of range
    face = np.array([0, 1, 1, 2, 3, 3])
    bary = np.full((6, 3), 1.0 / 3.0)
    y = np.ones((6, 2), dtype=np.float32)
    x0 = np.zeros((5, 2), dtype=np.float32)
    a = ref.assemble(faces, 5, face, bary, y, x0, LAMBDA)
    assert a.counts.tolist() == [0, 0, 0, 2, 3, 1, 0, 0]                # vertex 4 has no face at all
    assert (a.gram[1] == 0).all() and (a.gram[2] == 0).all() and a.mass[4] == 0.0
    table, _, _ = ref.solve(a, 4)
    assert table[4].tolist() == [0.0, 0.0] and (table[:4] > 0).all()
    for bad_face, bad_bary, bad_y, want in [(np.array([0, 1, 1, 2, 3, 4]), bary, y, [1, 0, 0]),
                                            (np.array([0, 1, 1, 3, 2, 3]), bary, y, [0, 1, 0]),
                                            (np.array([-1, 1, 1, 2, 3, 3]), bary, y, [1, 0, 0]),
                                            (face, np.where(np.arange(18).reshape(6, 3) == 4, np.inf, bary), y, [0, 0, 1]),
                                            (face, bary, np.where(np.arange(12).reshape(6, 2) % 5 == 0, np.nan, y), [0, 0, 3])]:
        r = ref.assemble(faces, 5, bad_face, bad_bary, bad_y.astype(np.float32), x0, LAMBDA)
        table, stats, counts = ref.solve(r, 4)
        assert counts.tolist() == want + [0, 0, 0, 0, 1] and table is None and not stats.any()
        assert not r.gram.any() and not r.mass.any() and not r.rhs.any()
    # no samples at all: every vertex is inactive and the prior comes back
    prior = np.arange(10, dtype=np.float32).reshape(5, 2) - 3
    table, stats, counts = ref.fit(faces, 5, np.zeros(0, dtype=np.int64), np.zeros((0, 3)), np.zeros((0, 2), np.float32),
                                   prior, LAMBDA, 3, 3)[:3]
    assert (table.view(np.uint32) == prior.view(np.uint32)).all() and counts.tolist() == [0, 0, 0, 2, 0, 5, 0, 0]


def test_dot_is_the_stated_tree():
    rng = np.random.default_rng(1)
    x, y = rng.normal(size=(600, 3)), rng.normal(size=(600, 3))
    got = ref.dot(x, y)
    for c in range(3):
        total = 0.0
        for blk in range(3):
            t = np.zeros(256)
            seg = (x[:, c] * y[:, c])[256 * blk:256 * (blk + 1)]
            t[:seg.shape[0]] = seg
            s = 128
            while s:
                for i in range(s):
                    t[i] += t[i + s]
                s //= 2
            total += t[0]
        assert got[c] == total
    assert np.abs(got - (x * y).sum(axis=0)).max() < 1e-12


def test_eigenvalues_lie_between_lambda_and_one_plus_lambda():
    """Fact 1: barycentrics are convex weights, so G <= D (Jensen) and the spectrum of D^-1 (G + lambda D) lies in
    [lambda, 1 + lambda]."""
    v, f, points, face, bary = sphere_samples(2, 4)
    y = field(points).astype(np.float32)
    a = ref.assemble(f, v.shape[0], face, bary, y, field(v).astype(np.float32), LAMBDA)
    G, d = ref.dense(a, face, bary)
    assert np.abs(d - a.mass).max() < 1e-12 and d.min() > 0
    assert np.abs(np.diag(G) + LAMBDA * d - 1.0 / a.inv).max() < 1e-12
    eig = np.linalg.eigvalsh(G / np.sqrt(d)[:, None] / np.sqrt(d)[None, :])
    print("eigenvalues of D^-1 G:", eig.min(), eig.max())
    assert eig.min() > -1e-12 and eig.max() < 1.0 + 1e-12
    p = np.random.default_rng(0).normal(size=(v.shape[0], 3))
    want = (G + LAMBDA * np.diag(d)) @ p
    assert np.abs(ref.apply(a, p) - want).max() < 1e-12 * np.abs(want).max()


def test_objective_never_rises_over_the_iterates():
    """Fact 2: CG's iterates decrease the objective monotonically, so E(X_K) <= E(x0)."""
    v, f, points, face, bary = sphere_samples(2, 4)
    y = field(points).astype(np.float32)
    x0 = field(v).astype(np.float32)
    a = ref.assemble(f, v.shape[0], face, bary, y, x0, LAMBDA)
    E = np.array([ref.energy(a, face, bary, y, x0.astype(np.float64) + Z) for Z in ref.iterate(a, 32)])
    assert (E[1:] <= E[:-1] * (1 + 1e-12)).all()                         # up to rounding once it has converged
    assert (E[-1] < 0.9 * E[0]).all()
    assert (E[12] <= E[-1] * (1 + 1e-9)).all()                           # kappa <= 65: a dozen steps are most of the way


def test_affine_column_comes_back_as_the_prior():
    """A column affine in position is drawn exactly by the blend of its vertex values: the residual is rounding and the
    correction stays below 1e-12."""
    v, f, points, face, bary = sphere_samples(2, 8)
    w, k = np.array([[0.7, -1.3], [2.1, 0.4], [-0.6, 0.9]]), np.array([0.25, -2.0])
    a = ref.assemble(f, v.shape[0], face, bary, points @ w + k, v @ w + k, LAMBDA, wide=True)
    for Z in ref.iterate(a, 32):
        pass
    print("largest correction of an affine column:", np.abs(Z).max())
    assert np.abs(Z).max() <= 1e-12


@pytest.mark.parametrize("level,per_face", [(2, 4), (2, 8), (3, 4), (3, 8)])
def test_restatement_against_a_dense_solve(level, per_face):
    """32 steps against numpy.linalg.solve of (G + lambda D): at most 1e-9 of the column's largest entry.  The spectrum
    bound gives kappa <= 65, and the relative residual after 32 steps is near 1e-13 (printed), so the error is below
    65 * 1e-13 of the solution with two orders to spare."""
    v, f, points, face, bary = sphere_samples(level, per_face)
    y, x0 = field(points).astype(np.float32), field(v).astype(np.float32)
    table, stats, counts, a = ref.fit(f, v.shape[0], face, bary, y, x0, LAMBDA, 32, 0)
    assert counts[5] == 0
    for Z in ref.iterate(a, 32):
        pass
    G, d = ref.dense(a, face, bary)
    W_rhs = a.rhs
    want = np.linalg.solve(G + LAMBDA * np.diag(d), W_rhs)
    X, X_want = x0.astype(np.float64) + Z, x0.astype(np.float64) + want
    err = np.abs(X - X_want).max(axis=0) / np.abs(X_want).max(axis=0)
    print(f"level {level}, N = {per_face} F: relative residual {stats[:, 1] / stats[:, 0]}, error {err}")
    assert (err <= 1e-9).all()
    assert (stats[:, 1] <= 1e-11 * stats[:, 0]).all()


def test_fit_beats_the_point_bake_on_fresh_samples():
    v, f, points, face, bary = sphere_samples(3, 8)
    bake = field(v).astype(np.float32)
    table, stats, counts, a = ref.fit(f, v.shape[0], face, bary, field(points).astype(np.float32), bake, LAMBDA, 32,
                                      clamp_mask=1 << 2)
    _, _, fresh_points, fresh_face, fresh_bary = sphere_samples(3, 64, seed=12345)
    truth = field(fresh_points)

    def rms(t):
        return np.sqrt(((ref.blend(f, fresh_face, fresh_bary, t) - truth) ** 2).mean(axis=0))

    fitted, baked = rms(table), rms(bake)
    print("held-out RMS, fit against point bake:", fitted, baked, fitted / baked, "clamped", counts[6])
    assert (fitted[:2] <= 0.75 * baked[:2]).all()
    assert (table[:, 2] > 0).all()
    free = ref.solve(a, 32, 0)[0]
    print("smallest unclamped entry of the positive column:", free[:, 2].min())


# ------------------------------------------------------------------------------------------------------- the new header
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_NAME = "qf_vertex_fit.h"
HEADER = os.path.join(ROOT, "include", HEADER_NAME)
WORKSPACE = "qf_vertex_fit_workspace_bytes"
NEW_FUNCTIONS = sorted([WORKSPACE, "qf_vertex_fit_assemble", "qf_vertex_fit_solve"])


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
    assert _functions(HEADER) == NEW_FUNCTIONS == sorted(_C._VERTEX_FIT_SIGNATURES)
    assert not set(NEW_FUNCTIONS) & set(_C.EXPORTED_SYMBOLS) and _C.ABI_VERSION == 6
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if other != HEADER_NAME:
            assert not set(NEW_FUNCTIONS) & set(_functions(os.path.join(ROOT, "include", other))), other
    raw = ctypes.CDLL(_C.LIB_PATH)
    for name in NEW_FUNCTIONS:
        getattr(raw, name)                               # AttributeError if the library does not export it
        fn = getattr(lib, name)
        restype, argtypes = _C._VERTEX_FIT_SIGNATURES[name]
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)
    assert _C.VERTEX_FIT_COUNTS == ref.COUNT_NAMES and len(ref.COUNT_NAMES) == 8
    assert _C.VERTEX_FIT_MAX_COLUMNS == 64


def test_workspace_and_size_refusals(lib):
    """Every refusal comes before the first launch, so it can be asked for without a device: sizes out of range, NULL
    pointers, short strides and a short workspace, with made-up non-NULL addresses that are never dereferenced."""
    bytes_of = lib.qf_vertex_fit_workspace_bytes
    assert bytes_of(0, 1, 1, 4) == -1 and bytes_of(2 ** 31, 1, 1, 4) == -1 and bytes_of(5, -1, 1, 4) == -1
    assert bytes_of(5, (2 ** 31 + 2) // 3, 1, 4) == -1 and bytes_of(5, 1, -1, 4) == -1 and bytes_of(5, 1, 2 ** 31, 4) == -1
    assert bytes_of(5, 1, 1, 0) == -1 and bytes_of(5, 1, 1, 65) == -1
    assert 0 < bytes_of(1, 0, 0, 1) < bytes_of(5000, 3000, 0, 46) < bytes_of(5000, 3000, 0, 64)
    assert bytes_of(5000, 3000, 0, 46) >= 4 * 8 * 5000 * 46 + 2 * 8 * 3 * 3000
    assert bytes_of(5000, 3000, 7, 46) == bytes_of(5000, 3000, 2 ** 31 - 1, 46)          # the samples are walked in place
    need, p, invalid = bytes_of(3, 1, 3, 4), ctypes.c_void_p(4096), -1                    # QF_ERR_INVALID_ARGUMENT
    assemble, solve = lib.qf_vertex_fit_assemble, lib.qf_vertex_fit_solve
    good = [p, 1, 3, p, p, 3, p, 4, p, 4, 4, 0.5, p, p, p, p, need, p, None]
    changes = [(0, None), (3, None), (4, None), (6, None), (8, None), (12, None), (13, None), (14, None), (15, None),
               (17, None), (16, need - 1), (1, -1), (1, (2 ** 31 + 2) // 3), (2, 0), (2, 2 ** 31), (5, -1), (5, 2 ** 31),
               (7, 3), (9, 3), (10, 0), (10, 65), (11, -0.5), (11, float("nan")), (11, float("inf"))]
    for index, value in changes:
        args = list(good)
        args[index] = value
        assert assemble(*args) == invalid, (index, value)
    good = [p, 1, 3, p, 4, 4, p, p, p, 32, 1, p, need, p, 4, p, p, None]
    changes = [(0, None), (3, None), (6, None), (7, None), (8, None), (11, None), (13, None), (15, None), (16, None),
               (12, need - 1), (1, -1), (2, 0), (2, 2 ** 31), (4, 3), (14, 3), (5, 0), (5, 65), (9, -1), (9, 2 ** 31)]
    for index, value in changes:
        args = list(good)
        args[index] = value
        assert solve(*args) == invalid, (index, value)


def test_every_new_entry_point_takes_the_callers_stream_and_is_indexed():
    from quadraturefields_amd import _C
    protos = _prototypes(HEADER)
    assert sorted(protos) == NEW_FUNCTIONS
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, params in protos.items():
        if name != WORKSPACE:                            # a host computation: no device work, no stream
            assert re.search(r"void\s*\*\s*stream\s*$", params.strip()), f"{name}: the last parameter is not void *stream"
        assert len([p for p in params.split(",") if p.strip()]) == len(_C._VERTEX_FIT_SIGNATURES[name][1]), name
        assert f"`{name}`" in text, f"INTEGRATION.md does not name {name}"


def test_new_header_is_plain_c(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "plain.c"
    src.write_text("\n".join(['#include <stdio.h>', f'#include "{HEADER_NAME}"', "int main(void) {",
                              'printf("%d %d %d\\n", QF_VERTEX_FIT_COUNTS, QF_VERTEX_FIT_MAX_COLUMNS, QF_ABI_VERSION);',
                              "return 0;", "}"]))
    exe = tmp_path / "plain"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split() == ["8", "64", "6"]


def test_build_lists_the_new_source_and_header():
    from quadraturefields_amd import build
    assert dict(build.SOURCES)["vertex_fit.hip"] == ["-ffp-contract=off"]
    assert HEADER in build._deps("vertex_fit.hip")
    text = open(os.path.join(build.CSRC, "vertex_fit.hip")).read()
    assert f'#include "{HEADER_NAME}"' in text and '#include "mesh_device.h"' in text
    code = re.sub(r"//.*", "", text)
    assert "fma" not in code                                   # nothing fused by hand
    assert "hipLaunchCooperativeKernel" not in code and not re.search(r"atomicAdd\s*\(\s*\(?\s*(double|float)", code)
    assert "hipStreamSynchronize" not in code and "hipDeviceSynchronize" not in code and "hipMemcpy" not in code


def test_wrappers_refuse_bad_arguments():
    import torch
    from quadraturefields_amd import baking
    assert baking._clamp_mask((-1,), 46) == 1 << 45 and baking._clamp_mask(None, 46) == 0 and baking._clamp_mask((), 4) == 0
    assert baking._clamp_mask("all", 64) == 2 ** 64 - 1 and baking._clamp_mask([0, 2, -1], 4) == 0b1101
    with pytest.raises(IndexError):
        baking._clamp_mask((4,), 4)
    with pytest.raises(ValueError):
        baking._clamp_mask("last", 4)
    faces = torch.zeros((1, 3), dtype=torch.int64)
    with pytest.raises(ValueError, match="device tensors"):
        baking.fit_vertex_table_device(faces, 3, torch.zeros(0, dtype=torch.int64), torch.zeros((0, 3), dtype=torch.float64),
                                       torch.zeros((0, 4)), torch.zeros((3, 4)))
    with pytest.raises(TypeError):
        baking.fit_vertex_table_device(faces, 3, None, None, None, torch.zeros((3, 4), dtype=torch.float64))
    quantised = object.__new__(baking.QuantisedVertexFeatures)
    with pytest.raises(TypeError, match="QuantisedVertexFeatures"):
        baking.fit_vertex_table_device(faces, 3, None, None, None, quantised)
    with pytest.raises(TypeError, match="QuantisedVertexFeatures"):
        baking.fit_vertex_features(None, None, prior=quantised)
    with pytest.raises(TypeError):
        baking.vertex_surface_error(None, None, quantised, 10)
