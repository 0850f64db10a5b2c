"""The numpy restatement of the surface-sampling rule (tests/mesh_sample_reference.py) pinned on
inputs whose outcome is worked out by hand and on the properties the rule promises, and the new header against its
binding."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import mesh_sample_reference as ref

# splitmix64 from state 0: its first three outputs (the published test vector) are h_0, h_1, h_2 of sample 0 at seed 0
SPLITMIX_0 = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]

UNIT = (np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), np.array([[0, 1, 2]]))

# Areas 1 and 3 (cross products of length 2 and 6) with two faces of no area between them: one with a repeated index, one
# with three collinear corners.  M = 6; q_0 = floor(fl(2 / 6) * 2^32) = floor(2^32 / 3) = 1431655765 (fl(1/3) is below 1/3
# by less than 2^-54, far from moving the floor); q_1 = q_2 = 0; q_3 = 2^32.
ONE_THREE = (np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 1.0, 0.0], [3.0, 0.0, 0.0], [0.0, 2.0, 0.0], [1.0, 0.0, 0.0]]),
             np.array([[0, 1, 2], [0, 1, 0], [0, 5, 1], [0, 3, 4]]))


def test_the_hash_is_splitmix64():
    assert ref.hashes(1, 0)[:, 0].tolist() == SPLITMIX_0
    # seed + (3 i + k + 1) golden wraps modulo 2^64: seed 2^64 - 1 is one step back
    want = ref.fin(np.array([(0x9E3779B97F4A7C15 * 4 - 1) % 2 ** 64], dtype=np.uint64))[0]
    assert ref.hashes(2, 2 ** 64 - 1)[0, 1] == want


def test_one_triangle_by_hand():
    v, f = UNIT
    q, cum, counts = ref.prepare(v, f)
    assert q.tolist() == [2 ** 32] and cum.tolist() == [2 ** 32] and counts.tolist() == [0] * 6
    points, face, bary, _ = ref.sample(v, f, 1, seed=0)
    r1, r2 = (SPLITMIX_0[1] >> 11) * 2.0 ** -53, (SPLITMIX_0[2] >> 11) * 2.0 ** -53
    assert 0.43 < r1 < 0.44 and 0.026 < r2 < 0.027         # 0x6E78 / 2^16 and 0x06C4 / 2^16: no flip
    assert face.tolist() == [0]
    assert bary.tolist() == [[(1.0 - r1) - r2, r1, r2]]
    assert points.tolist() == [[r1, r2, 0.0]]               # a * b0 is zero, b = e_x, c = e_y
    points, face, bary, _ = ref.sample(v, f, 1000, seed=3)
    assert (face == 0).all() and points.shape == (1000, 3) and (points[:, 2] == 0).all()
    assert (points[:, 0] == bary[:, 1]).all() and (points[:, 1] == bary[:, 2]).all()


def test_flip_keeps_the_point_inside():
    # sample 2 at seed 0 has r1 + r2 > 1 (found by running the rule): both are reflected
    h = ref.hashes(64, 0)
    r1, r2 = (h[1] >> np.uint64(11)) * 2.0 ** -53, (h[2] >> np.uint64(11)) * 2.0 ** -53
    flipped = np.nonzero(r1 + r2 > 1.0)[0]
    assert 16 < flipped.size < 48
    _, _, bary, _ = ref.sample(*UNIT, 64, seed=0)
    i = flipped[0]
    assert bary[i].tolist() == [max((1.0 - (1.0 - r1[i])) - (1.0 - r2[i]), 0.0), 1.0 - r1[i], 1.0 - r2[i]]


def test_areas_one_and_three_by_hand():
    v, f = ONE_THREE
    m, bad = ref.measures(v, f)
    assert m.tolist() == [2.0, 0.0, 0.0, 6.0] and bad == [0, 0, 0, 0]
    q, cum, counts = ref.prepare(v, f)
    assert q.tolist() == [1431655765, 0, 0, 2 ** 32]
    assert cum.tolist() == [1431655765, 1431655765, 1431655765, 1431655765 + 2 ** 32]
    assert counts.tolist() == [0, 0, 0, 0, 2, 0]
    # four strata of S / 4 = 1431655765.25 each: the first lies in face 0 but for its last quarter unit, the rest in face 3
    _, face, _, _ = ref.sample(v, f, 4, seed=0)
    assert face.tolist() == [0, 3, 3, 3]
    for n in (1, 5, 1000, 4097):
        _, face, _, _ = ref.sample(v, f, n, seed=n)
        count = np.bincount(face, minlength=4)
        assert count[1] == 0 and count[2] == 0
        assert abs(count[0] - n * 1431655765 / (1431655765 + 2 ** 32)) <= 2


def test_n_zero_and_refusals():
    v, f = ONE_THREE
    points, face, bary, counts = ref.sample(v, f, 0)
    assert points.shape == (0, 3) and face.shape == (0,) and bary.shape == (0, 3) and counts[4] == 2
    bad = v.copy()
    bad[5, 1] = np.nan                                       # vertex 5 is a corner of the collinear face only
    assert ref.sample(bad, f, 8)[0] is None
    assert ref.sample(bad, f, 8)[3].tolist() == [1, 0, 0, 1, 0, 0]
    assert ref.sample(v, np.array([[0, 1, 2], [0, 1, 6], [-1, 0, 1]]), 8)[3].tolist() == [0, 2, 0, 0, 0, 0]
    w = np.array([1.0, -1.0, np.nan, np.inf])
    # the measures are 2 * 1, 0 by decree (a repeated index: its weight is not looked at), 0 * NaN and 6 * inf
    assert ref.sample(v, f, 8, face_weight=w)[3].tolist() == [0, 0, 3, 2, 0, 0]
    flat = np.array([[0, 1, 0], [0, 5, 1], [2, 2, 2]])
    assert ref.sample(v, flat, 8)[3].tolist() == [0, 0, 0, 0, 0, 1]
    assert ref.sample(v, f, 8, face_weight=np.zeros(4))[3].tolist() == [0, 0, 0, 0, 0, 1]
    huge = v * 1e200                                         # finite vertices, a cross product that overflows
    assert ref.sample(huge, f, 8)[3].tolist() == [0, 0, 0, 2, 0, 0]


# ------------------------------------------------------------------------------------------------------------ properties
def check_properties(vertices, faces, face_weight, n, points, face, bary):
    """What the rule promises of any output (shared with the device tests)."""
    q, cum, _ = ref.prepare(vertices, faces, face_weight)
    assert face.shape == (n,) and points.shape == (n, 3) and bary.shape == (n, 3)
    assert (np.diff(face) >= 0).all()
    assert (face >= 0).all() and (face < q.shape[0]).all() and (q[face] > 0).all()
    assert (bary >= 0.0).all()
    assert (np.abs(((bary[:, 0] + bary[:, 1]) + bary[:, 2]) - 1.0) <= 2.0 ** -52).all()
    count = np.bincount(face, minlength=q.shape[0])
    share = n * (q.astype(np.float64) / np.float64(cum[-1]))
    assert np.abs(count - share).max() <= 2.0
    corners = np.asarray(vertices, dtype=np.float64)[np.asarray(faces)[face]]
    lo, hi = corners.min(axis=1), corners.max(axis=1)
    span = np.abs(corners).max(axis=1)
    assert (points >= lo - 4e-16 * span).all() and (points <= hi + 4e-16 * span).all()


def test_properties_on_meshes():
    v, f = ref.icosphere(2)
    for n in (1, 63, 4097):
        check_properties(v, f, None, n, *ref.sample(v, f, n, seed=5)[:3])
    v, f = ref.soup(999, 1, zero_every=3)
    w = np.random.default_rng(2).uniform(0.0, 1.0, size=999) ** 4
    check_properties(v, f, w, 5000, *ref.sample(v, f, 5000, seed=9, face_weight=w)[:3])
    assert ref.prepare(v, f)[2][4] == 333


def _measures(kind, n_faces):
    rng = np.random.default_rng(n_faces)
    if kind == "uniform":
        return rng.uniform(0.0, 1.0, size=n_faces)
    if kind == "constant":
        return np.full(n_faces, 0.37)
    m = rng.uniform(0.0, 1.0, size=n_faces) ** 8
    if n_faces >= 3:
        m[rng.permutation(n_faces)[: n_faces // 3]] = 0.0
    return m


@pytest.mark.parametrize("kind", ["uniform", "skewed_with_zeros", "constant"])
@pytest.mark.parametrize("n_faces,n", [(1, 1000), (7, 3), (1000, 100), (1000, 100_000), (50_000, 65_537), (200_000, 300_000)])
def test_stratification(kind, n_faces, n):
    """|count_f - N q_f / S| <= 2 for every face: stratum i is [i S / N, (i + 1) S / N) and face f owns [S_{f-1}, S_f), of
    length q_f.  In exact arithmetic every stratum that lies wholly in the face's interval gives it a sample (more than
    N q_f / S - 2 of them do) and only a stratum that overlaps it can (fewer than N q_f / S + 2 do)."""
    q, cum = ref.quantise(_measures(kind, n_faces))
    face = ref.faces_of(cum, n, seed=n_faces + n)
    assert (np.diff(face) >= 0).all() and (q[face] > 0).all()
    count = np.bincount(face, minlength=n_faces)
    share = n * (q.astype(np.float64) / np.float64(cum[-1]))
    worst = np.abs(count - share).max()
    print(f"{kind} F={n_faces} N={n}: worst |count - share| = {worst:.3f}")
    assert worst <= 2.0


def test_uniform_inside_a_face():
    n = 32_768
    _, _, bary, _ = ref.sample(*UNIT, n, seed=0)
    corner = [(bary[:, k] > 0.5).sum() for k in range(3)]
    middle = n - sum(corner)
    print("midpoint sub-triangles:", corner, middle)
    bound = 6.0 * np.sqrt(n * 3.0 / 16.0)                     # six sigma of a binomial(N, 1/4): 470
    assert 469 < bound < 471
    for c in corner + [middle]:
        assert abs(c - n / 4) <= bound
    # and the first two moments of a uniform point of the triangle: mean 1/3 (sigma of the mean 0.0013), E[b^2] = 1/6
    assert np.abs(bary.mean(axis=0) - 1.0 / 3.0).max() < 0.008
    assert np.abs((bary * bary).mean(axis=0) - 1.0 / 6.0).max() < 0.008


def test_weights_scale_free_zero_weight_and_seeds():
    v, f = ref.icosphere(1)
    w = np.random.default_rng(4).uniform(0.1, 1.0, size=f.shape[0])
    w[::5] = 0.0
    a = ref.sample(v, f, 777, seed=11, face_weight=w)
    b = ref.sample(v, f, 777, seed=11, face_weight=4.0 * w)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert (w[a[1]] > 0).all() and a[3][4] == (w == 0).sum()
    check_properties(v, f, w, 777, *a[:3])
    unweighted = ref.sample(v, f, 777, seed=11)
    assert unweighted[1].tobytes() != a[1].tobytes()
    ones = ref.sample(v, f, 777, seed=11, face_weight=np.ones(f.shape[0]))
    for x, y in zip(unweighted, ones):
        assert x.tobytes() == y.tobytes()
    other = ref.sample(v, f, 777, seed=12)
    assert other[0].tobytes() != unweighted[0].tobytes() and other[2].tobytes() != unweighted[2].tobytes()


def test_the_square_that_shows_why():
    """The two-tessellation unit square against the plane z = x / 2, on the host with the analytic distance |x| / 2 /
    sqrt(1.25): the vertex-and-centroid mean is half the surface integral, the area-weighted samples are within 1.9e-2."""
    v, f = ref.two_tessellation_square()
    exact = 0.25 / np.sqrt(1.25)
    default = np.concatenate([v, v[f].mean(axis=1)])
    assert abs(np.abs(default[:, 0] / 2.0).mean() / np.sqrt(1.25) / exact - 1.0) > 0.4
    for seed in range(4):
        points = ref.sample(v, f, 4096, seed=seed)[0]
        assert abs(np.abs(points[:, 0] / 2.0).mean() / np.sqrt(1.25) / exact - 1.0) < 1.9e-2


# ------------------------------------------------------------------------------------------------------- the new header
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_NAME = "qf_mesh_sample.h"
HEADER = os.path.join(ROOT, "include", HEADER_NAME)
WORKSPACE = "qf_mesh_sample_workspace_bytes"
NEW_FUNCTIONS = sorted([WORKSPACE, "qf_mesh_sample_prepare", "qf_mesh_sample_emit"])


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
    assert _functions(HEADER) == NEW_FUNCTIONS == sorted(_C._MESH_SAMPLE_SIGNATURES)
    assert not set(NEW_FUNCTIONS) & set(_C.EXPORTED_SYMBOLS) and _C.ABI_VERSION == 6
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if other != HEADER_NAME:
            assert not set(NEW_FUNCTIONS) & set(_functions(os.path.join(ROOT, "include", other))), other
    raw = ctypes.CDLL(_C.LIB_PATH)
    for name in NEW_FUNCTIONS:
        getattr(raw, name)                               # AttributeError if the library does not export it
        fn = getattr(lib, name)
        restype, argtypes = _C._MESH_SAMPLE_SIGNATURES[name]
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)
    assert _C.MESH_SAMPLE_COUNTS == ref.COUNT_NAMES and len(ref.COUNT_NAMES) == 6


def test_workspace_and_size_refusals(lib):
    """Every refusal comes before the first launch, so it can be asked for without a device: sizes out of range, NULL
    pointers and a short workspace, with made-up non-NULL addresses that are never dereferenced."""
    bytes_of = lib.qf_mesh_sample_workspace_bytes
    assert bytes_of(0, 1) == -1 and bytes_of(1, 0) == -1 and bytes_of(2 ** 31, 1) == -1 and bytes_of(5, -1) == -1
    assert bytes_of(5, (2 ** 31 + 2) // 3) == -1 and bytes_of(5, 2 ** 31 // 3) > 0       # 3 F < 2^31
    assert 0 < bytes_of(1, 1) < bytes_of(5000, 3000) and bytes_of(5000, 3000) >= 3 * 8 * 3000
    assert bytes_of(7, 3000) == bytes_of(5000, 3000)                                      # the faces alone decide
    need, p = bytes_of(3, 1), ctypes.c_void_p(4096)
    invalid = -1                                                                          # QF_ERR_INVALID_ARGUMENT
    prepare, emit = lib.qf_mesh_sample_prepare, lib.qf_mesh_sample_emit
    for args in [(None, 3, p, 1, None, p, need, p, None), (p, 3, None, 1, None, p, need, p, None),
                 (p, 3, p, 1, None, None, need, p, None), (p, 3, p, 1, None, p, need, None, None),
                 (p, 3, p, 1, None, p, need - 1, p, None), (p, 0, p, 1, None, p, need, p, None),
                 (p, 3, p, 0, None, p, need, p, None), (p, 2 ** 31, p, 1, None, p, need, p, None),
                 (p, 3, p, (2 ** 31 + 2) // 3, None, p, 2 ** 40, p, None)]:
        assert prepare(*args) == invalid, args
    for args in [(None, 3, p, 1, p, need, 4, 0, p, p, p, None), (p, 3, None, 1, p, need, 4, 0, p, p, p, None),
                 (p, 3, p, 1, None, need, 4, 0, p, p, p, None), (p, 3, p, 1, p, need - 1, 4, 0, p, p, p, None),
                 (p, 3, p, 1, p, need, -1, 0, p, p, p, None), (p, 3, p, 1, p, need, 2 ** 31, 0, p, p, p, None),
                 (p, 3, p, 1, p, need, 4, 0, None, p, p, None), (p, 3, p, 1, p, need, 4, 0, p, None, p, None),
                 (p, 3, p, 1, p, need, 4, 0, p, p, None, None), (p, 0, p, 1, p, need, 4, 0, p, p, p, None),
                 (p, 3, p, 0, p, need, 4, 0, p, p, p, None)]:
        assert emit(*args) == invalid, args
    assert emit(p, 3, p, 1, p, need, 0, 2 ** 64 - 1, None, None, None, None) == 0         # N == 0 launches nothing


def test_every_new_entry_point_takes_the_callers_stream_and_is_indexed():
    from quadraturefields_amd import _C
    protos = _prototypes(HEADER)
    assert sorted(protos) == NEW_FUNCTIONS
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, params in protos.items():
        if name != WORKSPACE:                            # a host computation: no device work, no stream
            assert re.search(r"void\s*\*\s*stream\s*$", params.strip()), f"{name}: the last parameter is not void *stream"
        assert len([p for p in params.split(",") if p.strip()]) == len(_C._MESH_SAMPLE_SIGNATURES[name][1]), name
        assert f"`{name}`" in text, f"INTEGRATION.md does not name {name}"


def test_new_header_is_plain_c(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "plain.c"
    src.write_text("\n".join(['#include <stdio.h>', f'#include "{HEADER_NAME}"', "int main(void) {",
                              'printf("%d %d\\n", QF_MESH_SAMPLE_COUNTS, QF_ABI_VERSION);', "return 0;", "}"]))
    exe = tmp_path / "plain"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split() == ["6", "6"]


def test_build_lists_the_new_source_and_header():
    from quadraturefields_amd import build
    assert dict(build.SOURCES)["mesh_sample.hip"] == ["-ffp-contract=off"]
    assert HEADER in build._deps("mesh_sample.hip")
    text = open(os.path.join(build.CSRC, "mesh_sample.hip")).read()
    assert f'#include "{HEADER_NAME}"' in text
    code = re.sub(r"//.*", "", text)
    assert "fma" not in code and "float " not in code          # fp64 only, nothing fused by hand
    assert "hipLaunchCooperativeKernel" not in code and not re.search(r"atomicAdd\s*\(\s*\(?\s*(double|float)", code)
    assert "hipStreamSynchronize" not in code and "hipDeviceSynchronize" not in code and "hipMemcpy" not in code


def test_wrappers_refuse_host_tensors_and_bad_arguments():
    import inspect
    import torch
    from quadraturefields_amd import mc_utils
    tv, tf = torch.from_numpy(UNIT[0]), torch.from_numpy(UNIT[1])
    with pytest.raises(ValueError, match="device tensors"):
        mc_utils.sample_surface_device(tv, tf, 4)
    with pytest.raises(TypeError):
        mc_utils.sample_surface_device(UNIT[0], tf, 4)
    with pytest.raises(ValueError):
        mc_utils.sample_surface_device(tv[:, :2], tf, 4)
    with pytest.raises(TypeError):
        mc_utils.sample_surface_device(tv.to(torch.int64), tf, 4)
    for n in (-1, 2 ** 31):
        with pytest.raises(ValueError, match="n_samples"):
            mc_utils.sample_surface_device(tv, tf, n)
    for seed in (-1, 2 ** 64):
        with pytest.raises(ValueError, match="seed"):
            mc_utils.sample_surface_device(tv, tf, 4, seed=seed)
    assert mc_utils.SurfaceSamples._fields == ("points", "face", "bary")
    for fn in (mc_utils.mesh_distance_device, mc_utils.mesh_distance):
        params = inspect.signature(fn).parameters
        assert params["samples"].default is None and params["seed"].default == 0
    assert "lower bound" in mc_utils.mesh_distance_device.__doc__
