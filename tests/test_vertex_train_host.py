"""CPU: training through the vertex table -- the additive header ``include/qf_vertex_train.h``
held to the pattern of ``tests/test_vertex_baked_host.py``, the float64 reference gradient pinned by central finite
differences, the conditions of the scenes the GPU tests rely on, and the surface of ``baking.VertexBakedFeatures``."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import vertex_baked_reference as R
from tests import vertex_train_reference as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qf_vertex_train.h")
NEW_FUNCTIONS = ["qf_vertex_shade_points_backward"]


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


# --------------------------------------------------------------------------------------------------- the new header
def test_header_and_binding_agree(lib):
    import ctypes
    from quadraturefields_amd import _C
    assert _functions(HEADER) == NEW_FUNCTIONS                       # exactly the new function, nothing else
    assert sorted(_C._VERTEX_TRAIN_SIGNATURES) == NEW_FUNCTIONS
    assert not set(NEW_FUNCTIONS) & set(_C.EXPORTED_SYMBOLS) and not set(NEW_FUNCTIONS) & set(_C._VERTEX_BAKED_SIGNATURES)
    assert _C.ABI_VERSION == 6
    for other in ("qf_hip.h", "qf_vertex_baked.h"):
        assert not set(NEW_FUNCTIONS) & set(_functions(os.path.join(ROOT, "include", other))), other
    raw = ctypes.CDLL(_C.LIB_PATH)
    for name in NEW_FUNCTIONS:
        getattr(raw, name)                                           # AttributeError if the library does not export it
        fn = getattr(lib, name)
        restype, argtypes = _C._VERTEX_TRAIN_SIGNATURES[name]
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)


def test_the_entry_point_takes_the_callers_stream_and_is_indexed():
    from quadraturefields_amd import _C
    protos = _prototypes(HEADER)
    assert sorted(protos) == NEW_FUNCTIONS
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, params in protos.items():
        assert re.search(r"void\s*\*\s*stream\s*$", params.strip()), f"{name}: the last parameter is not void *stream"
        assert len([p for p in params.split(",") if p.strip()]) == len(_C._VERTEX_TRAIN_SIGNATURES[name][1]) == 15, name
        assert f"`{name}`" in text, f"INTEGRATION.md does not name {name}"


def test_new_header_is_plain_c(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "plain.c"
    src.write_text('#include <stdio.h>\n#include "qf_vertex_train.h"\n'
                   'int main(void) { printf("%d %d\\n", QF_ABI_VERSION, (int)sizeof(&qf_vertex_shade_points_backward)); return 0; }\n')
    obj = tmp_path / "plain.o"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(obj)],
                   check=True)


def test_build_lists_the_new_source_and_header():
    from quadraturefields_amd import build
    flags = dict(build.SOURCES)
    assert "vertex_train.hip" in flags and flags["vertex_train.hip"] == ["-ffp-contract=off"]
    assert HEADER in build._deps("vertex_train.hip") and HEADER in build._deps("vertex_baked.hip")
    assert os.path.exists(os.path.join(build.CSRC, "vertex_train.hip"))


# ------------------------------------------------------------------------- the float64 reference, pinned independently
def _hand_mesh():
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.1, 0.0], [0.1, 1.0, 0.2], [1.1, 1.2, -0.1]], dtype=np.float64)
    f = np.array([[0, 1, 2], [2, 1, 3]], dtype=np.int64)
    return v, f


def _hand_samples(v, f, n, seed):
    g = np.random.default_rng(seed)
    tri = g.integers(0, f.shape[0], size=n)
    w = g.uniform(0.05, 1.0, size=(n, 3))
    w /= w.sum(axis=1, keepdims=True)
    pts = np.einsum("nk,nkd->nd", w, v[f[tri]]).astype(np.float32)
    d = g.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return pts, tri, d


@pytest.mark.parametrize("lobes", [1, 2])
def test_reference_gradient_matches_central_finite_differences(lobes):
    """Every entry of the [4, W] gradient against (L(t + h e) - L(t - h e)) / 2h in float64, h = 1e-6: the truncation
    error is h^2 |L'''| / 6 ~ 1e-12 relative and the rounding error eps |L| / h ~ 1e-9 for |L| ~ 10; the bar is 1e-6 of the
    column's largest entry, three orders above both and far below any wrong term of the formula."""
    v, f = _hand_mesh()
    pts, tri, dirs = _hand_samples(v, f, 24, seed=3)
    g = np.random.default_rng(8)
    table = G.random_table(4, lobes, seed=5)
    d_rgb = g.normal(size=(24, 3))
    d_sigma = g.normal(size=(24,))
    got = G.table_gradient(table, v, f, pts, tri, dirs, d_rgb, d_sigma, lobes)
    b = R.barycentrics(v, f, pts, tri)

    def loss(t64):
        rgb, sigma = G.shade64(torch.from_numpy(t64), f[tri], b, dirs, lobes)
        return float((rgb * torch.from_numpy(d_rgb)).sum() + (sigma * torch.from_numpy(d_sigma)).sum())

    t64 = table.astype(np.float64)
    want = np.zeros_like(t64)
    h = 1e-6
    for r in range(t64.shape[0]):
        for c in range(t64.shape[1]):
            up, dn = t64.copy(), t64.copy()
            up[r, c] += h
            dn[r, c] -= h
            want[r, c] = (loss(up) - loss(dn)) / (2 * h)
    ratio = G.column_ratio(got, want)
    print(f"{lobes} lobes: reference vs central differences, worst column ratio {ratio:.3e}")
    assert np.abs(want).max(axis=0).min() > 0 and ratio <= 1e-6
    # without d_sigma the density column is exactly zero and the others are unchanged
    frozen = G.table_gradient(table, v, f, pts, tri, dirs, d_rgb, None, lobes)
    assert not frozen[:, -1].any() and np.array_equal(frozen[:, :-1], got[:, :-1])


def test_reference_skips_degenerate_and_out_of_range_faces():
    v, f = _hand_mesh()
    f3 = np.concatenate([f, [[3, 3, 3], [0, 1, 7]]])
    pts, tri, dirs = _hand_samples(v, f, 16, seed=4)
    tri2 = np.concatenate([tri, [2, 3, 2, 3]])
    pts2 = np.concatenate([pts, pts[:4]])
    dirs2 = np.concatenate([dirs, dirs[:4]])
    g = np.random.default_rng(2)
    d_rgb, d_sigma = g.normal(size=(20, 3)), g.normal(size=(20,))
    table = G.random_table(4, 2, seed=6)
    a = G.table_gradient(table, v, f, pts, tri, dirs, d_rgb[:16], d_sigma[:16], 2)
    b = G.table_gradient(table, v, f3, pts2, tri2, dirs2, d_rgb, d_sigma, 2)
    assert np.isfinite(b).all() and np.array_equal(a, b)


# ------------------------------------------------------------------------- what the GPU tests rely on, on the CPU oracle
@pytest.mark.parametrize("w,h,k,samples,touched,shared,most", [(37, 29, 25, 5431, 1236, 0.89, 98), (64, 40, 25, 15268, 1252, 0.95, 303),
                                                               (8, 8, 1, 32, 38, None, None)])
def test_scene_conditions(w, h, k, samples, touched, shared, most):
    """Collisions, untouched rows and a frame below one wave: samples, vertices touched, the share of the mesh's
    vertices with at least two contributions, the most contributions to one vertex; barycentrics inside (3e-6, 0.995)."""
    m = R.mesh()
    assert m.vertices.shape[0] == 1296 and m.faces.shape[0] == 2560
    xyzs, _, _, _, index_tri, _ = R.oracle_samples(w, h, k)
    cnt = G.contributions(m.vertices.shape[0], m.faces, index_tri.numpy())
    b = R.barycentrics(m.vertices, m.faces, xyzs.numpy(), index_tri.numpy())
    n_touched = int((cnt > 0).sum())
    share = float((cnt >= 2).sum()) / m.vertices.shape[0]
    print(f"{w}x{h} K={k}: {xyzs.shape[0]} samples, {n_touched} vertices touched, {share:.1%} with >= 2 contributions, "
          f"most {int(cnt.max())}; barycentrics in [{b.min():.3g}, {b.max():.3g}]")
    assert xyzs.shape[0] == samples and n_touched == touched and n_touched < m.vertices.shape[0]
    assert np.isfinite(b).all() and b.min() > 3e-6 and b.max() < 0.995
    if shared is not None:
        assert round(share, 2) == shared and int(cnt.max()) == most
    else:
        assert samples < 64


# ------------------------------------------------------------------------------------------------ the module's surface
def test_vertex_baked_features_module():
    from quadraturefields_amd import _C, baking
    for lobes in (1, 2, 6, 8):
        w = R.row_width(lobes)
        feats = torch.randn(7, w, generator=torch.Generator().manual_seed(lobes))
        m = baking.VertexBakedFeatures(feats)
        params = list(m.parameters())
        assert len(params) == 1 and params[0] is m.table and isinstance(m.table, torch.nn.Parameter)
        assert m.table.shape == (7, _C.vertex_row_stride(lobes)) == (7, R.row_stride(lobes)) and m.table.dtype == torch.float32
        assert m.table.data_ptr() % 64 == 0 and m.table.is_contiguous()
        assert m.n_lobes == lobes and not bool(m.table.detach()[:, w:].any())
        out = m.features()
        assert out.shape == (7, w) and torch.equal(out, feats) and not out.requires_grad
        assert out.data_ptr() == m.table.data_ptr()                  # a view: nothing is copied
    for bad in (torch.zeros(7, 12), torch.zeros(7, 4), torch.zeros(7, 3 + 7 * 9 + 1), torch.zeros(7), torch.zeros(0, 11)):
        with pytest.raises(ValueError):
            baking.VertexBakedFeatures(bad)
    m = baking.VertexBakedFeatures(torch.zeros(7, 46))
    m.check_rows(7)
    with pytest.raises(ValueError):
        m.check_rows(8)
    with pytest.raises(TypeError):
        baking.finetune_vertex_features(torch.zeros(7, 46), None, None, 1)


def test_every_vertex_feature_function_accepts_the_module():
    """Signatures unchanged, and each function's documentation names the module among what ``vertex_features`` takes."""
    from quadraturefields_amd import baking, utils
    from quadraturefields_amd.render import FrameRenderer
    want = {
        utils.vertex_baked_shading: ["mesh_intersect", "vertex_features"],
        utils.vertex_baked_shading_struct: ["mesh_intersect", "vertex_features"],
        utils.shade_vertex_baked_points: ["mesh_intersect", "vertex_features", "points", "index_tri", "dirs", "n_device", "want_features"],
        utils.shade_composite_vertex_baked_frame: ["mesh_intersect", "vertex_features", "xyz_c", "dirs_c", "frame", "render_step_size",
                                                   "stop_tau", "render_bkgd", "bg_color", "packed"],
        FrameRenderer.render_vertex_baked: ["self", "origins", "viewdirs", "vertex_features", "image_width", "camera", "early_stop_eps"],
        FrameRenderer.render_vertex_baked_async: ["self", "origins", "viewdirs", "vertex_features", "camera", "early_stop_eps"],
    }
    for fn, params in want.items():
        assert list(inspect.signature(fn).parameters) == params, fn.__name__
        assert "VertexBakedFeatures" in fn.__doc__, fn.__name__
    sig = inspect.signature(utils.render_image_finetune_baking_with_occgrid)
    assert list(sig.parameters)[-2:] == ["vertex_features", "bg_color"] and sig.parameters["vertex_features"].default is None
    assert "VertexBakedFeatures" in utils.render_image_finetune_baking_with_occgrid.__doc__
    assert utils._vertex_features_lobes(baking.VertexBakedFeatures(torch.zeros(3, 32))) == 4      # the type decides: 32 = width of 4
    assert utils._vertex_features_lobes(torch.zeros(3, 32)) == 4
    assert baking.VertexBakedFeatures(torch.zeros(3, 18)).table.shape[1] == 32                    # ... and the stride of 2
    assert list(inspect.signature(baking.finetune_vertex_features).parameters) == [
        "module", "mesh_intersect", "next_batch", "steps", "lr", "train_density", "bg_color", "render_step_size"]
    assert issubclass(utils._VertexShadeFn, torch.autograd.Function)
