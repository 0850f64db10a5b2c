"""GPU: vertex clustering (``mc_utils.simplify_vertex_clustering`` / ``qf_vertex_clustering_*``) against its numpy
restatement (tests/vertex_clustering_reference.py), and the simplification step of the reference's mesh scripts."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import marching_cubes_reference as mcref
from tests import vertex_clustering_reference as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _device(v, f, s, contraction, **kw):
    from quadraturefields_amd import mc_utils
    out = mc_utils.simplify_vertex_clustering(torch.from_numpy(np.asarray(v, np.float64)).cuda(),
                                              torch.from_numpy(np.asarray(f)).cuda(), s, contraction, **kw)
    torch.cuda.synchronize()
    assert out[0].is_cuda and out[0].dtype == torch.float64 and out[1].dtype == torch.int64
    return (out[0].cpu().numpy(), out[1].cpu().numpy()) + tuple(out[2:])


def _assert_matches(v, f, s):
    """Faces, cell numbering and positions of both contractions bit-exact (fp64 division and square root round
    correctly on gfx950), and the same number of quadric cells falling back to the mean."""
    va, fa = _device(v, f, s, "average")
    ra, rfa = ref.simplify(v, f, s, "average")
    assert va.shape == ra.shape and np.array_equal(fa, rfa)
    assert np.array_equal(va.view(np.int64), ra.view(np.int64))
    vq, fq, n_fb = _device(v, f, s, "quadric", return_fallbacks=True)
    rq, rfq, info = ref.simplify(v, f, s, "quadric", details=True)
    assert vq.shape == rq.shape and np.array_equal(fq, rfq) and np.array_equal(fq, fa)
    bad = np.nonzero((vq.view(np.int64) != rq.view(np.int64)).any(axis=1))[0]
    assert bad.size == 0, (bad[:5], vq[bad[0]], rq[bad[0]], info["det"][bad[0]], info["thresh"][bad[0]])
    assert n_fb == int((~info["accepted"]).sum())
    return int(info["accepted"].sum()), len(rq)


def _mc_mesh(vol, level=0.0):
    from quadraturefields_amd import mc_utils
    vt = torch.from_numpy(np.ascontiguousarray(vol, np.float32)).cuda()
    verts, faces = mc_utils.marching_cubes(vt, level)
    return mc_utils.normalise_vertices(verts, vol.shape[0]), faces


@pytest.mark.parametrize("seed", [0, 1])
def test_random_mesh_matches_restatement(device, seed):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(3000, 3)) * [1.0, 2.0, 0.5]
    f = rng.integers(0, 3000, size=(8000, 3))
    f[:50, 1] = f[:50, 0]                                   # repeated-index faces
    f[100:150] = f[200:250][:, [1, 2, 0]]                   # rotated duplicates
    f[300:350] = f[400:450][:, [0, 2, 1]]                   # opposite windings
    for s in (0.05, 0.3, 1.7):
        _assert_matches(v, f, s)


def test_marching_cubes_mesh_matches_restatement(device):
    rng = np.random.default_rng(5)
    vol = rng.choice(np.array([-2, -1, 0, 0, 1, 2], np.float32), size=(40, 36, 32)) + np.float32(0.5)
    v, f = _mc_mesh(vol, 0.5)
    f = f.cpu().numpy()
    assert ((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).any()
    v = v.cpu().numpy()
    for vx in (7, 20, 150):
        _assert_matches(v, f, 1 / vx)
    # int32 faces, as marching_cubes returns them, give the same result as int64
    a = _device(v, f.astype(np.int32), 1 / 20, "quadric")
    b = _device(v, f.astype(np.int64), 1 / 20, "quadric")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_shell_mesh_matches_restatement(device):
    from quadraturefields_amd import synthetic
    mesh = synthetic.shell_mesh(n_shells=6, subdivisions=5)
    solved = 0
    for vx in (30, 150, 300):
        solved += _assert_matches(mesh.vertices, mesh.faces, 1 / vx)[0]
    assert solved > 0                                       # the solve branch is exercised, not only the mean


def test_two_runs_are_bit_identical(device):
    from quadraturefields_amd import mc_utils, synthetic
    mesh = synthetic.shell_mesh(n_shells=12, subdivisions=6)
    v = torch.from_numpy(mesh.vertices).cuda()
    f = torch.from_numpy(mesh.faces).cuda()
    for c in ("average", "quadric"):
        a = mc_utils.simplify_vertex_clustering(v, f, 1 / 150, c)
        b = mc_utils.simplify_vertex_clustering(v, f, 1 / 150, c)
        assert torch.equal(a[0].view(torch.int64), b[0].view(torch.int64)) and torch.equal(a[1], b[1])


def test_ball_at_256(device):
    """A marching-cubes ball simplified at vx = 150: vertices within their grown cells, the enclosed volume, ray hits."""
    from quadraturefields_amd import mc_utils
    from quadraturefields_amd.mesh_io import TriMesh
    from quadraturefields_amd.mesh_utils import MeshIntersection
    n, R = 256, 100.0
    ax = torch.arange(n, device="cuda", dtype=torch.float32) - (n - 1) / 2
    vol = R - torch.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2)
    verts, faces = mc_utils.marching_cubes(vol, 0.0)
    v = mc_utils.normalise_vertices(verts, n)
    s = 1 / 150
    ov, of = mc_utils.simplify_vertex_clustering(v, faces, s)
    ov, of = ov.cpu().numpy(), of.cpu().numpy()
    assert 100_000 < len(of) < len(faces)            # s is 0.85 of the grid spacing 2 / 255
    vin = v.cpu().numpy()
    lo, idx = ref.cells(vin, s)
    _, _, info = ref.simplify(vin, faces.cpu().numpy(), s, "average", details=True)
    cell = info["cell"]
    assert ((ov >= lo + (cell - 0.5) * s) & (ov <= lo + (cell + 1.5) * s)).all()
    r = R * 2 / (n - 1)
    vol_mesh = mcref.signed_volume(ov, of)
    ball = 4 / 3 * math.pi * r ** 3
    assert abs(vol_mesh - ball) / ball <= 3 * math.sqrt(3) * s / r, (vol_mesh, ball)
    mi = MeshIntersection(TriMesh(ov, of), simplify_mesh=False, scale=1.0, num_intersections=16)
    rng = np.random.default_rng(0)
    d = rng.normal(size=(64, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    origins = (-1.5 * d).astype(np.float32)
    out = mi.sampling_raytrace_numpy(d.astype(np.float32), origins)
    hits = np.bincount(out[2], minlength=64)
    assert (hits >= 2).all(), hits
    first = np.full(64, np.inf)
    np.minimum.at(first, out[2], out[3])
    assert (np.abs(first - (1.5 - r)) <= 2 * math.sqrt(3) * s).all()


def test_shell_dense_512(device):
    """512^3 sin(100 r): tens of millions of faces through marching cubes, normalisation and clustering on the device."""
    from quadraturefields_amd import mc_utils
    n = 512
    ax = torch.arange(n, device="cuda", dtype=torch.float32) - (n - 1) / 2
    r = torch.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2)
    vol = torch.sin(100.0 * (r * (2.0 / (n - 1))))
    del r
    verts, faces = mc_utils.marching_cubes(vol, 0.0)
    del vol
    assert faces.shape[0] > 20_000_000
    v = mc_utils.normalise_vertices(verts, n)
    del verts
    ov, of = mc_utils.simplify_vertex_clustering(v, faces, 1 / 150)
    assert 0 < of.shape[0] < faces.shape[0]
    assert int(of.min()) >= 0 and int(of.max()) < ov.shape[0]
    assert bool((of[:, 0] < of[:, 1]).all()) and bool((of[:, 0] < of[:, 2]).all())
    assert bool(torch.isfinite(ov).all())
    assert float(ov.abs().max()) <= 1.0 + 2 / 150


def test_downsample_mesh(device):
    from quadraturefields_amd import mc_utils, synthetic
    mesh = synthetic.shell_mesh(n_shells=3, subdivisions=4)
    assert mc_utils.downsample_mesh(mesh, 0) is mesh
    out = mc_utils.downsample_mesh(mesh, 150)
    rv, rf = ref.simplify(mesh.vertices, mesh.faces, 1 / 150, "quadric")
    assert np.array_equal(out.faces, rf) and out.vertices.shape == rv.shape


def test_downsample_script_matches_in_process(device, tmp_path):
    from quadraturefields_amd import mc_utils, synthetic
    from quadraturefields_amd.mesh_io import load_mesh
    mesh = synthetic.shell_mesh(n_shells=4, subdivisions=5)
    path = os.path.join(str(tmp_path), "mesh.ply")
    mesh.export(path)
    env = dict(os.environ, PYTHONPATH=ROOT)
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "downsample_mesh.py"), path, "150"], env=env,
                          capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr[-2000:]
    assert "Before mesh simplification" in proc.stdout and "After mesh simplification" in proc.stdout
    want = mc_utils.downsample_mesh(load_mesh(path), 150)
    got = load_mesh(os.path.join(str(tmp_path), "smp_mesh.ply"))
    assert np.array_equal(got.faces, want.faces)
    assert np.array_equal(got.vertices, want.vertices.astype(np.float32).astype(np.float64))


def test_errors(device):
    from quadraturefields_amd import mc_utils
    v = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=torch.float64)
    f = torch.tensor([[0, 1, 2]])
    vd, fd = v.cuda(), f.cuda()
    with pytest.raises(ValueError, match="device"):
        mc_utils.simplify_vertex_clustering(v, f, 0.5)
    with pytest.raises(ValueError, match="device"):
        mc_utils.simplify_vertex_clustering(vd, f, 0.5)
    for s in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="voxel_size"):
            mc_utils.simplify_vertex_clustering(vd, fd, s)
    for bad in ([[0, 1, 3]], [[0, -1, 2]]):
        with pytest.raises(ValueError, match="1 faces have an index outside"):
            mc_utils.simplify_vertex_clustering(vd, torch.tensor(bad, device="cuda"), 0.5)
    vn = vd.clone()
    vn[1, 2] = float("nan")
    vn[2, 0] = float("inf")
    with pytest.raises(ValueError, match="2 vertices are not finite"):
        mc_utils.simplify_vertex_clustering(vn, fd, 0.5)
    with pytest.raises(ValueError, match="cells along an axis"):
        mc_utils.simplify_vertex_clustering(vd, fd, 1.0 / (1 << 21))
    with pytest.raises(ValueError, match="contraction"):
        mc_utils.simplify_vertex_clustering(vd, fd, 0.5, "midpoint")
    # the largest allowed grid: exactly 2^21 cells along x
    ok = torch.tensor([[0.0, 0, 0], [(1 << 21) - 1.0, 0, 0], [0, 1, 0]], dtype=torch.float64, device="cuda")
    out_v, out_f = mc_utils.simplify_vertex_clustering(ok, fd, 1.0)
    assert out_v.shape == (3, 3) and out_f.tolist() == [[0, 1, 2]]
