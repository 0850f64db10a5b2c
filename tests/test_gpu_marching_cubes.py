"""GPU: marching cubes (``mc_utils.marching_cubes`` / ``qf_marching_cubes_*``) against its numpy restatement
(tests/marching_cubes_reference.py), bit for bit, and the extraction route of the reference's marching_cubes.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import marching_cubes_reference as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _device_mesh(vol, level, dtype=torch.float32):
    from quadraturefields_amd import mc_utils
    v, f = mc_utils.marching_cubes(torch.from_numpy(np.ascontiguousarray(vol)).to("cuda", dtype), level)
    torch.cuda.synchronize()
    assert v.is_cuda and v.dtype == torch.float32 and f.dtype == torch.int32
    return v.cpu().numpy(), f.cpu().numpy()


def _assert_exact(vol, level):
    v, f = _device_mesh(vol, level)
    v_ref, f_ref = ref.marching_cubes(vol, level)
    assert v.shape == v_ref.shape and f.shape == f_ref.shape, (v.shape, v_ref.shape, f.shape, f_ref.shape)
    bad = np.argwhere(v.view(np.uint32) != v_ref.view(np.uint32))
    assert bad.size == 0, (bad[:5], v[bad[0][0]], v_ref[bad[0][0]])
    assert np.array_equal(f, f_ref)
    return v, f


@pytest.mark.parametrize("seed", [0, 1])
def test_random_volume_is_bit_exact(device, seed):
    rng = np.random.default_rng(seed)
    _assert_exact(rng.normal(size=(48, 48, 48)).astype(np.float32), 0.1 * seed)


def test_tie_heavy_volume_is_bit_exact(device):
    """A few values around the level: many samples exactly at it (merged vertices) and decider ties."""
    rng = np.random.default_rng(7)
    vol = rng.choice(np.array([-2, -1, 0, 0, 1, 2], np.float32), size=(40, 33, 29)) + np.float32(0.5)
    v, f = _assert_exact(vol, 0.5)
    assert (f[:, 0] == f[:, 1]).any() or (f[:, 1] == f[:, 2]).any() or (f[:, 0] == f[:, 2]).any()
    assert len(np.unique(v, axis=0)) == len(v)


def test_all_single_cell_patterns_are_bit_exact(device):
    """The 256 sign patterns of one cell (random magnitudes, so ambiguous faces go both ways), stacked along axis 0
    with a separating plane at the level between them."""
    rng = np.random.default_rng(11)
    vol = np.zeros((3 * 256, 2, 2), np.float32)
    for bits in range(256):
        for c in range(8):
            s = 1.0 if (bits >> c) & 1 else -1.0
            vol[3 * bits + (c & 1), (c >> 1) & 1, (c >> 2) & 1] = s * rng.uniform(0.25, 4.0)
    _assert_exact(vol, 0.0)


@pytest.mark.parametrize("shape", [(37, 64, 5), (2, 2, 2), (5, 2, 300)])
def test_shapes_are_bit_exact(device, shape):
    rng = np.random.default_rng(sum(shape))
    _assert_exact(rng.normal(size=shape).astype(np.float32), 0.0)


def test_fp16_volume_is_widened_exactly(device):
    rng = np.random.default_rng(2)
    vol = rng.normal(size=(24, 20, 16)).astype(np.float16)
    v, f = _device_mesh(vol, 0.25, torch.float16)
    v_ref, f_ref = ref.marching_cubes(vol.astype(np.float32), 0.25)
    assert np.array_equal(v.view(np.uint32), v_ref.view(np.uint32)) and np.array_equal(f, f_ref)


def test_two_runs_are_bit_identical(device):
    from quadraturefields_amd import mc_utils
    rng = np.random.default_rng(4)
    vol = torch.from_numpy(rng.normal(size=(96, 80, 64)).astype(np.float32)).cuda()
    a = mc_utils.marching_cubes(vol, 0.0)
    b = mc_utils.marching_cubes(vol, 0.0)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])


def test_noisy_sphere_at_512_is_closed(device):
    """512^3: non-degenerate directed edges balance and no two vertices coincide."""
    from quadraturefields_amd import mc_utils
    n = 512
    g = torch.Generator(device="cuda").manual_seed(0)
    ax = torch.arange(n, device="cuda", dtype=torch.float32) - (n - 1) / 2
    r = torch.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2)
    vol = (200.0 - r) + 0.5 * torch.rand((n, n, n), device="cuda", generator=g)
    del r
    v, f = mc_utils.marching_cubes(vol, 0.0)
    del vol
    assert f.shape[0] > 500_000
    f = f.to(torch.int64)
    e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    e = e[e[:, 0] != e[:, 1]]
    key_f, cnt_f = torch.unique(e[:, 0] * (1 << 31) + e[:, 1], return_counts=True)
    key_r, cnt_r = torch.unique(e[:, 1] * (1 << 31) + e[:, 0], return_counts=True)
    assert torch.equal(key_f, key_r) and torch.equal(cnt_f, cnt_r)
    assert torch.unique(v, dim=0).shape[0] == v.shape[0]
    assert int(f.max()) == v.shape[0] - 1 and int(f.min()) == 0


def test_errors(device):
    from quadraturefields_amd import mc_utils
    vol = torch.zeros((8, 8, 8), device="cuda")
    vol[3, 3, 3] = float("nan")
    with pytest.raises(ValueError, match="not finite"):
        mc_utils.marching_cubes(vol, 0.0)
    with pytest.raises(ValueError):
        mc_utils.marching_cubes(torch.zeros((8, 8, 8)), 0.0)
    with pytest.raises(ValueError):
        mc_utils.marching_cubes(torch.zeros((8, 8), device="cuda"), 0.0)
    with pytest.raises(ValueError):
        mc_utils.marching_cubes(torch.zeros((8, 1, 8), device="cuda"), 0.0)
    with pytest.raises(ValueError):
        mc_utils.marching_cubes(torch.zeros((8, 8, 8), device="cuda"), float("inf"))
    v, f = mc_utils.marching_cubes(torch.zeros((8, 8, 8), device="cuda"), 0.0)
    assert v.shape == (0, 3) and f.shape == (0, 3)


def _quantity_fp64(grid, grads, binaries, sigma, include_grad, grad_thres):
    """marching_cubes.py:30-58 in fp64 on the CPU: dense 5^3 conv3d, trilinear upsample, normalise, mask."""
    import math
    import torch.nn.functional as F
    k = torch.arange(5, dtype=torch.float64)
    g1 = 1 / (sigma * math.sqrt(2 * math.pi)) * torch.exp(-((k - 2) / sigma) ** 2 / 2)
    w = g1[:, None, None] * g1[None, :, None] * g1[None, None, :]
    w = (w / w.sum())[None, None]
    g = F.conv3d(torch.from_numpy(grid).double()[None, None], w, padding="same")[0, 0]
    d = F.interpolate(torch.from_numpy(binaries[0]).double()[None, None], size=grid.shape, mode="trilinear",
                      align_corners=True)[0, 0]
    g = g - (g * d).min()
    g = g / ((g * d).max() + 1e-6)
    g = (g - 0.5) * 2
    q = g * d
    if include_grad:
        q = q * (torch.from_numpy(grads).double() > grad_thres)
    return q


def _radial_inputs(n, seed=0):
    rng = np.random.default_rng(seed)
    ax = np.arange(n, dtype=np.float64) - (n - 1) / 2
    r = np.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2)
    grid = (r / (n - 1)).astype(np.float32)
    grads = np.ones((n, n, n), np.float32)
    binaries = np.ones((1, n // 4, n // 4, n // 4), np.float32)
    return grid, grads, binaries, r, rng


def test_preprocessing_matches_fp64_restatement(device):
    from quadraturefields_amd import mc_utils
    rng = np.random.default_rng(5)
    grid = rng.normal(size=(64, 64, 64)).astype(np.float32)
    grads = rng.uniform(0, 0.02, size=(64, 64, 64)).astype(np.float32)
    binaries = (rng.uniform(size=(1, 16, 16, 16)) > 0.3).astype(np.float32)
    for sigma, include_grad in [(100.0, True), (1.5, False)]:
        q = mc_utils.quadrature_quantity(grid, grads, binaries, sigma=sigma, include_grad=include_grad,
                                         grad_thres=0.01)
        q_ref = _quantity_fp64(grid, grads, binaries, sigma, include_grad, 0.01)
        assert q.is_cuda and q.dtype == torch.float32
        assert (q.cpu().double() - q_ref).abs().max().item() < 1e-5


def test_radial_field_gives_shells_at_known_radii(device):
    """256^3 radial field: sin(omega q) = 0 shells, every vertex within one voxel of its analytic shell; rays through
    the centre hit every shell that lies inside the box twice."""
    from quadraturefields_amd import mc_utils
    from quadraturefields_amd.mesh_utils import MeshIntersection
    n, omega = 256, 20.0
    grid, grads, binaries, _, _ = _radial_inputs(n)
    q = _quantity_fp64(grid, grads, binaries, 100.0, True, 0.01)
    mesh = mc_utils.quadrature_surface_mesh(grid, grads, binaries, sigma=100.0, omega=omega)
    assert len(mesh.faces) > 10_000
    vox = (mesh.vertices / 2 + 0.5) * (n - 1)
    idx = np.clip(np.rint(vox).astype(np.int64), 0, n - 1)
    qv = q.numpy()[idx[:, 0], idx[:, 1], idx[:, 2]]
    k = np.rint(omega * qv / np.pi)
    dq_dvox = np.abs(np.diff(q.numpy()[:, n // 2, n // 2])).max()          # |grad q| per voxel, about constant
    assert (np.abs(qv - k * np.pi / omega) <= 1.5 * dq_dvox).all()
    # shell radii along an axis through the centre (voxels), from q along that axis
    line = q.numpy()[:, n // 2, n // 2]
    s = np.sin(omega * line)
    crossings = int(((s[:-1] > 0) != (s[1:] > 0)).sum())
    mi = MeshIntersection(mesh, simplify_mesh=False, scale=1.0, num_intersections=64)
    c = (n // 2) / (n - 1) * 2 - 1
    origins = np.array([[-1.5, c + 1e-4, c + 2e-4], [c + 3e-4, -1.5, c + 1e-4]], np.float32)
    dirs = np.array([[1, 0, 0], [0, 1, 0]], np.float32)
    out = mi.sampling_raytrace_numpy(dirs, origins)
    hits = np.bincount(out[2], minlength=2)
    assert crossings >= 10
    assert hits.tolist() == [crossings, crossings]


def test_extract_mesh_script_matches_in_process(device, tmp_path):
    from quadraturefields_amd import mc_utils
    from quadraturefields_amd.mesh_io import load_mesh
    n = 48
    grid, grads, binaries, r, _ = _radial_inputs(n)
    density = (40.0 * np.exp(-(r / 12.0) ** 2)).astype(np.float16)
    root = str(tmp_path) + "/"
    np.save(root + "grids_valid.npy", grid)
    np.save(root + "grads_valid.npy", grads)
    np.save(root + "binaries.npy", binaries)
    np.save(root + "density_grids_valid.npy", density)
    args = [root, "100.0", "True", "30.0", "0.0", "0", "True", "0.01", "10.0"]
    env = dict(os.environ, PYTHONPATH=ROOT)
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "extract_mesh.py")] + args, env=env,
                          capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr[-2000:]
    quad = mc_utils.quadrature_surface_mesh(grid, grads, binaries, sigma=100.0, omega=30.0, thres=0.0,
                                            grad_thres=0.01)
    nerf = mc_utils.density_surface_mesh(density, 10.0)
    both = mc_utils.combined_mesh(quad, nerf)
    assert len(nerf.faces) > 100 and len(quad.faces) > 100
    for path, m in [("mesh_nerf.ply", nerf), ("mesh.ply", both)]:
        got = load_mesh(os.path.join(root, path))
        assert np.array_equal(got.faces, m.faces)
        assert np.array_equal(got.vertices, m.vertices.astype(np.float32).astype(np.float64))
    assert ref.signed_volume(nerf.vertices, nerf.faces) > 0
