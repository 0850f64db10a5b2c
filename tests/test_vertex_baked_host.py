"""CPU: the vertex-baked route -- the restated blend against the reference's own line, the stride
rule and the record layout, the additive header ``include/qf_vertex_baked.h`` held to the bars ``tests/test_abi.py`` holds
``include/qf_hip.h`` to, and the conditions the GPU tests rely on, checked on the CPU oracle alone."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import baked_termination_reference as T
from tests import vertex_baked_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qf_vertex_baked.h")
NEW_FUNCTIONS = ["qf_frame_render_vertex_baked", "qf_vertex_composite_tiles", "qf_vertex_records_pack", "qf_vertex_shade_points"]


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


# ----------------------------------------------------------------------------------------------------- the arithmetic
def test_restated_blend_is_the_references_sum_within_one_ulp():
    """utils.py:836 is ``torch.sum(features * b_coords, dim=1)`` over the three corners; torch does not fix the order of
    that sum, the kernels do: (f0 b0 + f1 b1) + f2 b2.  10 000 random rows of the widest table (60 columns), barycentrics
    of points inside and slightly outside their triangle."""
    g = torch.Generator().manual_seed(11)
    n, w = 10000, R.row_width(8)
    feats = torch.randn(n, 3, w, generator=g) * 3.0
    b = torch.rand(n, 3, generator=g) + 0.01
    b = b / b.sum(dim=1, keepdim=True)
    b[::7] += torch.tensor([[-1e-4, 5e-5, 5e-5]])                      # outside by what the frame tests allow
    want = torch.sum(feats * b.unsqueeze(2), dim=1).numpy()
    got = R.blend_rows(feats[:, 0].numpy(), feats[:, 1].numpy(), feats[:, 2].numpy(), b.numpy())
    assert got.dtype == np.float32 and got.shape == (n, w)
    ulps = np.abs(got - want) / np.spacing(np.abs(want))               # ulps of the reference's own value
    print(f"restated blend vs torch.sum: max {ulps.max():.2f} ulp, {int((got != want).sum())} of {got.size} values differ")
    assert ulps.max() <= 1.0


def test_stride_rule():
    from quadraturefields_amd import _C
    for lobes, stride in ((1, 16), (2, 32), (6, 48), (8, 64)):
        assert R.row_stride(lobes) == _C.vertex_row_stride(lobes) == stride
    for lobes in range(1, 9):
        s = R.row_stride(lobes)
        assert s % 16 == 0 and s >= R.row_width(lobes) > s - 16
        assert R.row_width(lobes) == 3 + 7 * lobes + 1


def test_record_dtype_is_one_128_byte_line():
    from quadraturefields_amd import _C
    d = R.RECORD_DTYPE
    assert d.itemsize == 128 == _C.QF_VERTEX_TRIANGLE_RECORD_BYTES
    assert [d.fields[n][1] for n in ("ax", "inv", "v", "zero")] == [0, 96, 104, 116]
    # the restatement on a hand-made mesh: a right triangle, a degenerate one, one with an id out of range
    v = np.array([[0, 0, 0], [2, 0, 0], [0, 3, 0], [1, 1, 1]], dtype=np.float64)
    r = R.records(v, np.array([[0, 1, 2], [3, 3, 3], [0, 1, 4]]))
    assert r["v"].tolist() == [[0, 1, 2], [3, 3, 3], [0, 0, 0]] and not r["zero"].any()
    assert (r["d00"][0], r["d01"][0], r["d11"][0], r["inv"][0]) == (4.0, 0.0, 9.0, 1.0 / 36.0)
    assert np.isinf(r["inv"][1]) and np.isinf(r["inv"][2])
    b = R.barycentrics(v, np.array([[0, 1, 2]]), np.array([[0.5, 0.75, 0.0]], dtype=np.float32), np.array([0]))
    assert b.dtype == np.float32 and b.tolist() == [[0.5, 0.25, 0.25]]
    assert np.isnan(R.barycentrics(v, np.array([[3, 3, 3]]), np.array([[1, 1, 1]], dtype=np.float32), np.array([0]))).all()


# --------------------------------------------------------------------------------------------------- the new header
def test_header_and_binding_agree(lib):
    from quadraturefields_amd import _C
    declared = _functions(HEADER)
    own = [f for f in declared if f in NEW_FUNCTIONS]
    assert own == NEW_FUNCTIONS
    assert sorted(_C._VERTEX_BAKED_SIGNATURES) == NEW_FUNCTIONS
    assert not set(NEW_FUNCTIONS) & set(_C.EXPORTED_SYMBOLS) and _C.ABI_VERSION == 6
    # nothing else is declared there, and nothing of it in qf_hip.h as well
    assert set(declared) - set(NEW_FUNCTIONS) == set()
    assert not set(NEW_FUNCTIONS) & set(_functions(os.path.join(ROOT, "include", "qf_hip.h")))
    raw = ctypes.CDLL(_C.LIB_PATH)
    for name in NEW_FUNCTIONS:
        getattr(raw, name)                               # AttributeError if the library does not export it
        fn = getattr(lib, name)
        restype, argtypes = _C._VERTEX_BAKED_SIGNATURES[name]
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)


def test_every_new_entry_point_takes_the_callers_stream_and_is_indexed():
    from quadraturefields_amd import _C
    protos = _prototypes(HEADER)
    assert sorted(protos) == NEW_FUNCTIONS
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, params in protos.items():
        assert re.search(r"void\s*\*\s*stream\s*$", params.strip()), f"{name}: the last parameter is not void *stream"
        assert len([p for p in params.split(",") if p.strip()]) == len(_C._VERTEX_BAKED_SIGNATURES[name][1]), name
        assert f"`{name}`" in text, f"INTEGRATION.md does not name {name}"


def test_new_header_is_plain_c_and_the_struct_layout_matches(tmp_path):
    """A C translation unit that includes ``include/qf_vertex_baked.h`` compiles, and ``qf_vertex_baked_shading`` has the
    size and field offsets of its ctypes mirror (the pattern of test_abi.py::test_struct_layouts_match_the_header)."""
    from quadraturefields_amd import _C
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    cname, cls = "qf_vertex_baked_shading", _C.VertexBakedShading
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "qf_vertex_baked.h"', "int main(void) {",
             f'printf("{cname} size %zu\\n", sizeof({cname}));',
             'printf("record bytes %d\\n", QF_VERTEX_TRIANGLE_RECORD_BYTES);', 'printf("abi version %d\\n", QF_ABI_VERSION);']
    for fname, _ in cls._fields_:
        lines.append(f'printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ["return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {tuple(l.split()[:2]): int(l.split()[2]) for l in out if l.strip()}
    assert got[(cname, "size")] == ctypes.sizeof(cls)
    for fname, _ in cls._fields_:
        assert got[(cname, fname)] == getattr(cls, fname).offset, fname
    assert got[("record", "bytes")] == 128 and got[("abi", "version")] == 6


def test_build_lists_the_new_source_and_header():
    from quadraturefields_amd import build
    flags = dict(build.SOURCES)
    assert flags["vertex_baked.hip"] == ["-ffp-contract=off"]
    assert HEADER in build._deps("vertex_baked.hip") and HEADER in build._deps("frame.cpp")


def test_python_surface():
    import inspect
    from quadraturefields_amd import baking, utils
    from quadraturefields_amd.dropin import utils as dropin_utils
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceField
    from quadraturefields_amd.render import FrameRenderer
    sig = inspect.signature(utils.render_image_finetune_baking_with_occgrid)
    ref = ["radiance_field", "estimator", "rays", "data", "near_plane", "far_plane", "render_step_size", "render_bkgd",
           "cone_angle", "alpha_thre", "test_chunk_size", "timestamps", "mesh_intersect", "mesh_finetune", "scaling"]
    assert list(sig.parameters)[:len(ref)] == ref and sig.parameters["vertex_features"].default is None
    assert sig.parameters["scaling"].default == 1 / 128 and sig.parameters["render_step_size"].default == 1e-3
    assert dropin_utils.render_image_finetune_baking_with_occgrid is utils.render_image_finetune_baking_with_occgrid
    sig = inspect.signature(FrameRenderer.render_vertex_baked)
    assert list(sig.parameters) == ["self", "origins", "viewdirs", "vertex_features", "image_width", "camera", "early_stop_eps"]
    sig = inspect.signature(utils.shade_vertex_baked_points)
    assert list(sig.parameters) == ["mesh_intersect", "vertex_features", "points", "index_tri", "dirs", "n_device", "want_features"]
    field = NGPRadianceField(aabb=[-1.5] * 3 + [1.5] * 3, log2_hashmap_size=8)
    with pytest.raises(NotImplementedError):
        baking.bake_vertex_features(field, None)


# ------------------------------------------------------------------------- what the GPU tests rely on, on the CPU oracle
def test_scenes_cover_every_value_of_every_axis():
    cfgs = R.CONFIGS
    assert {(c[0], c[1]) for c in cfgs} == {(37, 29), (8, 8), (64, 40)}
    assert {c[2] for c in cfgs} == {1, 5, 25} and {c[3] for c in cfgs} == {1, 2, 6, 8} and {c[4] for c in cfgs} == {"white", "black"}
    assert {R.row_stride(c[3]) for c in cfgs} == {16, 32, 48, 64}
    assert {(c[0], c[2]) for c in cfgs} == {(w, k) for w in (37, 8, 64) for k in (1, 5, 25)}


def test_scene_mesh_has_no_degenerate_face():
    m = R.mesh()
    assert m.faces.shape == (2560, 3)
    r = R.records(m.vertices, m.faces)
    assert np.isfinite(r["inv"]).all() and (r["inv"] > 0).all()
    assert (r["v"] == m.faces).all() and int(m.faces.max()) < m.vertices.shape[0]
    assert float(np.abs(m.vertices).max()) <= 1.5                     # the affine test's bound is worked out for |p| <= 1.5


@pytest.mark.parametrize("w,h,k", sorted({(c[0], c[1], c[2]) for c in R.CONFIGS}))
def test_scene_barycentrics_lie_inside_their_triangles(w, h, k):
    m = R.mesh()
    xyzs, _, index_ray, _, index_tri, _ = R.oracle_samples(w, h, k)
    b = R.barycentrics(m.vertices, m.faces, xyzs.numpy(), index_tri.numpy())
    print(f"{w}x{h} K={k}: {b.shape[0]} samples, barycentrics in [{b.min():.3g}, {b.max():.3g}]")
    assert b.shape[0] > 0 and np.isfinite(b).all()
    assert b.min() >= -1e-4 and b.max() <= 1 + 1e-4
    assert float(np.abs(xyzs.numpy()).max()) <= 1.5


@pytest.mark.parametrize("eps", [1e-2, 1e-3])
@pytest.mark.parametrize("cfg", [c for c in R.CONFIGS if c[2] > 1], ids=[i for c, i in zip(R.CONFIGS, R.IDS) if c[2] > 1])
def test_early_stop_shares_hold_on_the_overridden_density(cfg, eps):
    """With the density column overridden per vertex (a third at 2000, a third at 0, the rest as baked) at least 10 % of
    the pixels with samples stop before their last sample and at least 10 % never stop, in every early-termination case
    of the GPU tests (K > 1: with K = 1 a pixel's only sample always contributes)."""
    w, h, k, lobes, _ = cfg
    m = R.mesh()
    assert np.bincount(R.density_classes()).tolist() == [m.vertices.shape[0] // 3] * 3        # a third each
    feats = R.override_density(R.oracle_vertex_features(lobes))
    assert (feats[:, -1] == 2000).sum() >= m.vertices.shape[0] // 3 and (feats[:, -1] == 0).sum() >= m.vertices.shape[0] // 3
    xyzs, _, index_ray, _, index_tri, _ = R.oracle_samples(w, h, k)
    sigma = R.blend(feats[:, -1:], m.vertices, m.faces, xyzs.numpy(), index_tri.numpy())[:, 0]
    counts = np.bincount(index_ray.numpy(), minlength=w * h)
    kept = T.contributing_counts(sigma, counts, R.DELTA, T.stop_tau(eps))
    early, never = R.stop_shares(counts, kept)
    print(f"{cfg} eps {eps}: {early:.1%} of the pixels with samples stop early, {never:.1%} never stop; "
          f"{int(kept.sum())} of {int(counts.sum())} samples contribute")
    assert early >= 0.10 and never >= 0.10
