"""CPU: the quantised vertex-baked route -- the additive header ``include/qf_vertex_quant.h`` held
to the bars ``tests/test_vertex_baked_host.py`` holds ``include/qf_vertex_baked.h`` to, the Python surface, and the
condition the GPU early-termination tests rely on (both branches of the stopping rule on the QUANTISED density), checked
on the CPU oracle alone."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from oracle import quantize as oq
from tests import baked_termination_reference as T
from tests import vertex_baked_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "qf_vertex_quant.h")
OTHER_HEADERS = [os.path.join(INCLUDE, n) for n in ("qf_hip.h", "qf_vertex_baked.h", "qf_vertex_train.h")]
NEW_FUNCTIONS = ["qf_frame_render_vertex_quant", "qf_vertex_quant_composite_tiles", "qf_vertex_quant_decode",
                 "qf_vertex_quant_shade_points"]


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
    from quadraturefields_amd import _C
    declared = _functions(HEADER)
    assert declared == NEW_FUNCTIONS                       # these and nothing else
    assert sorted(_C._VERTEX_QUANT_SIGNATURES) == NEW_FUNCTIONS
    assert _C.ABI_VERSION == 6
    new = set(NEW_FUNCTIONS)
    assert not new & set(_C.EXPORTED_SYMBOLS)
    assert not new & set(_C._VERTEX_BAKED_SIGNATURES) and not new & set(_C._VERTEX_TRAIN_SIGNATURES)
    for other in OTHER_HEADERS:
        assert not new & set(_functions(other)), other
    raw = ctypes.CDLL(_C.LIB_PATH)
    for name in NEW_FUNCTIONS:
        getattr(raw, name)                               # AttributeError if the library does not export it
        fn = getattr(lib, name)
        restype, argtypes = _C._VERTEX_QUANT_SIGNATURES[name]
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)


_CTYPE_OF = [(r"\*", ctypes.c_void_p), (r"\bint64_t\b", ctypes.c_int64), (r"\bint32_t\b", ctypes.c_int32),
             (r"\bfloat\b", ctypes.c_float)]


def _ctype_of(param):
    for pattern, ctype in _CTYPE_OF:
        if re.search(pattern, param):
            return ctype
    raise AssertionError(f"no ctypes type for {param!r}")


def test_prototypes_match_the_signatures_and_are_indexed():
    """Parameter by parameter: a pointer is ``c_void_p`` (or the ``POINTER`` of a mirrored struct), ``int64_t`` /
    ``int32_t`` / ``float`` their ctypes; every function returns int, ends in ``void *stream`` and is named in
    INTEGRATION.md."""
    from quadraturefields_amd import _C
    protos = _prototypes(HEADER)
    assert sorted(protos) == NEW_FUNCTIONS
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    structs = {"qf_frame_job": _C.FrameJob, "qf_vertex_quant_shading": _C.VertexQuantShading}
    for name, params in protos.items():
        assert re.search(r"void\s*\*\s*stream\s*$", params.strip()), f"{name}: the last parameter is not void *stream"
        restype, argtypes = _C._VERTEX_QUANT_SIGNATURES[name]
        assert restype is ctypes.c_int
        plist = [p.strip() for p in params.split(",") if p.strip()]
        assert len(plist) == len(argtypes), name
        for p, a in zip(plist, argtypes):
            m = re.search(r"\b(qf_frame_job|qf_vertex_quant_shading)\b", p)
            want = ctypes.POINTER(structs[m.group(1)]) if m else _ctype_of(p)
            assert a is want, (name, p, a)
        assert f"`{name}`" in text, f"INTEGRATION.md does not name {name}"


def test_new_header_is_plain_c_and_the_struct_layout_matches(tmp_path):
    from quadraturefields_amd import _C
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    cname, cls = "qf_vertex_quant_shading", _C.VertexQuantShading
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "qf_vertex_quant.h"', "int main(void) {",
             f'printf("{cname} size %zu\\n", sizeof({cname}));',
             'printf("record bytes %d\\n", QF_TEXEL_RECORD_BYTES);', 'printf("abi version %d\\n", QF_ABI_VERSION);']
    for fname, _ in cls._fields_:
        lines.append(f'printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ["return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {tuple(l.split()[:2]): int(l.split()[2]) for l in out if l.strip()}
    assert got[(cname, "size")] == ctypes.sizeof(cls)
    for fname, _ in cls._fields_:
        assert got[(cname, fname)] == getattr(cls, fname).offset, fname
    assert got[("record", "bytes")] == 64 == _C.QF_TEXEL_RECORD_BYTES and got[("abi", "version")] == 6


def test_build_lists_the_new_source_and_header():
    from quadraturefields_amd import build
    flags = dict(build.SOURCES)
    assert flags["vertex_quant.hip"] == ["-ffp-contract=off"]
    for src in ("vertex_quant.hip", "frame.cpp"):
        deps = build._deps(src)
        assert HEADER in deps and os.path.join(build.CSRC, "vertex_quant_device.h") in deps
        assert os.path.join(build.CSRC, "vertex_baked_device.h") in deps and os.path.join(build.CSRC, "texture_device.h") in deps


# ------------------------------------------------------------------------------------------------ the Python surface
def test_python_surface():
    from quadraturefields_amd import baking
    assert baking.vertex_texture_size(1296) == 36 and baking.vertex_texture_size(5000) == 71
    assert [baking.vertex_texture_size(v) for v in (1, 2, 4, 5, 9, 10)] == [1, 2, 2, 3, 3, 4]
    with pytest.raises(ValueError):
        baking.vertex_texture_size(0)
    sig = inspect.signature(baking.quantise_vertex_features)
    assert list(sig.parameters) == ["vertex_features", "compression_type", "lambda_thres", "device"]
    assert sig.parameters["compression_type"].default == "linear" and sig.parameters["lambda_thres"].default == 7.5
    cls = baking.QuantisedVertexFeatures
    assert not issubclass(cls, torch.nn.Module)
    for method in ("save", "load", "dequantise", "check_rows", "records"):
        assert callable(getattr(cls, method)), method
    assert list(inspect.signature(cls.load).parameters) == ["path_prefix", "n_vertices", "num_lobes", "compression_type",
                                                            "lambda_thres", "device"]
    # the class on host planes: the T rule is enforced, the attributes are the issue's, a gradient is refused
    from quadraturefields_amd.texture_utils import FeatureCompression
    z = lambda t, *c: np.zeros((t, t) + c, dtype=np.uint8)
    comp = FeatureCompression.from_arrays(z(71), z(71, 3), [z(71, 3)] * 2, [z(71, 3)] * 2, compression_type="linear", device="cpu")
    q = cls(comp, 5000)
    assert (q.compressor, q.n_vertices, q.n_lobes, q.width, q.sigmoid_codec) == (comp, 5000, 2, 18, 0)
    q.check_rows(5000)
    with pytest.raises(ValueError):
        q.check_rows(4999)
    with pytest.raises(ValueError):
        cls(comp, 71 * 71 + 1)                             # needs 72 x 72
    with pytest.raises(ValueError):
        cls(comp, 70 * 70)                                 # needs 70 x 70
    with pytest.raises(TypeError):
        baking.finetune_vertex_features(q, None, None, 1)


# ------------------------------------------------------------------------- what the GPU tests rely on, on the CPU oracle
def quantised_override_density(lobes):
    """``R.override_density`` of the oracle's table with the density column taken through the reference's codec
    (``compress_sigma`` -> ``inverse_of_compressed_sigma``): the densities the quantised route composites."""
    feats = R.override_density(R.oracle_vertex_features(lobes))
    code = oq.compress_sigma(torch.from_numpy(feats[:, -1]))
    feats[:, -1] = oq.inverse_of_compressed_sigma(code).numpy()
    return feats, code.numpy()


@pytest.mark.parametrize("eps", [1e-2, 1e-3])
@pytest.mark.parametrize("cfg", [c for c in R.CONFIGS if c[2] > 1], ids=[i for c, i in zip(R.CONFIGS, R.IDS) if c[2] > 1])
def test_early_stop_shares_hold_on_the_quantised_overridden_density(cfg, eps):
    from quadraturefields_amd import baking
    w, h, k, lobes, _ = cfg
    m = R.mesh()
    feats, code = quantised_override_density(lobes)
    # the scene's table as a vertex texture: V = 1296 = 36^2, every texel a vertex (why layout tests use another table)
    assert baking.vertex_texture_size(feats.shape[0]) ** 2 == feats.shape[0] == 1296
    cls = R.density_classes()
    assert set(code[cls == 0].tolist()) == {254} and set(code[cls == 1].tolist()) == {0}
    assert 1100 < float(feats[cls == 0, -1][0]) < 1115          # code 254: sigma = 1108
    xyzs, _, index_ray, _, index_tri, _ = R.oracle_samples(w, h, k)
    sigma = R.blend(feats[:, -1:], m.vertices, m.faces, xyzs.numpy(), index_tri.numpy())[:, 0]
    counts = np.bincount(index_ray.numpy(), minlength=w * h)
    kept = T.contributing_counts(sigma, counts, R.DELTA, T.stop_tau(eps))
    early, never = R.stop_shares(counts, kept)
    print(f"{cfg} eps {eps}: {early:.1%} of the pixels with samples stop early, {never:.1%} never stop; "
          f"{int(kept.sum())} of {int(counts.sum())} samples contribute")
    assert early >= 0.10 and never >= 0.10
