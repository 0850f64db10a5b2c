"""GPU: stage 2's grid extraction (quadraturefields_amd.field_utils, qf_field_grid_extract) against the fp64
restatement of the reference's extract_grid / extract_density_grid (tests/grid_extract_reference.py).

Bars.  Value grid (fp32): every voxel within 2e-5 + 2e-5 |ref|, the deformation field's bar.
Gradient-norm grid (fp16, the fp32 mean rounded once): every voxel within 2e-5 + (2e-5 + 2^-11) |ref| + 2^-25 -- the
same bar on the fp32 mean plus half an fp16 ulp -- and at least 99 % of the voxels equal to the fp64 reference rounded
to fp16.  fp16 mode: the bar of test_gpu_deform_fp16.py (99 % within the fp32 bar, all within 5e-4, plus the fp16 half
ulp for the gradient grid).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import fields as ofields
from tests import grid_extract_reference as ref
from tests import helpers

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALF_ULP = 2.0 ** -11
STAGE2 = dict(scale=0.5, precision=16, L=16, max_res=512, min_res=16, output_dim=1, num_features=2, back_prop=False)


def _field(device, nl, hidden, log2_T=14, seed=7, table_amp=0.5):
    from quadraturefields_amd.field import Field
    f = Field(log2_T=log2_T, hidden_size=hidden, nl=nl, **STAGE2)
    g = torch.Generator().manual_seed(seed)

    def xavier(o, i, gain):
        return (torch.rand(o, i, generator=g) * 2 - 1) * gain * (6.0 / (i + o)) ** 0.5

    n = f.xyz_encoder.params.numel()
    st = {"xyz_encoder.params": (torch.rand(n, generator=g) * 2 - 1) * table_amp,
          "decoder_field.layers.0.weight": xavier(hidden, 35, 1.5),
          "decoder_field.layers.0.bias": (torch.rand(hidden, generator=g) - 0.5) * 0.4,
          "decoder_field.layers.1.weight": xavier(hidden, hidden, 1.5),
          "decoder_field.layers.1.bias": (torch.rand(hidden, generator=g) - 0.5) * 0.4,
          "decoder_field.lout.weight": xavier(1, hidden, 2.0),
          "decoder_field.lout.bias": (torch.rand(1, generator=g) - 0.5) * 0.2}
    f.load_state_dict(st, strict=False)
    return f.to(device)


def _wts(f):
    return helpers.oracle_deform_weights(f)


def _value_ok(got, want):
    got, want = got.detach().cpu().double(), want.double()
    err = (got - want).abs()
    return float((err <= 2e-5 + 2e-5 * want.abs()).double().mean()), float(err.max())


def _grad_ok(got, want):
    """(fraction equal to want rounded to fp16, fraction within the fp16-adjusted bar, max error)."""
    got, want = got.detach().cpu().double(), want.double()
    bar = 2e-5 + (2e-5 + HALF_ULP) * want.abs() + 2.0 ** -25
    err = (got - want).abs()
    eq = float((got == want.half().double()).double().mean())
    return eq, float((err <= bar).double().mean()), float(err.max())


def _grad_bar_ok(nl, within):
    """ELU's derivative is continuous at 0: every voxel within the bar.  ReLU's jumps there: a lattice point whose
    pre-activation is within fp32 rounding of 0 takes the other branch than the fp64 reference, and its voxel's gradient
    norm moves by a weight column's share -- 99.9 % within the bar (measured: 99.994 % at n = 64)."""
    return within == 1.0 if nl == "elu" else within >= 0.999


@pytest.mark.parametrize("nl,hidden", [("elu", 16), ("relu", 32)])
def test_oracle_parity_fp32(device, nl, hidden):
    from quadraturefields_amd import field_utils
    f = _field(device, nl, hidden)
    wts = _wts(f)
    # both ELU branches occur on the lattice
    x = ref.lattice_points(ref.lattice_axis(16, 0.5))
    z1 = F.linear(torch.cat([(x + 0.5) / 1.0, ofields.hash_encode((x + 0.5) / 1.0, wts.table, wts.levels)], 1),
                  *wts.layers[0])
    assert (z1 < 0).double().mean() > 0.1 and (z1 > 0).double().mean() > 0.1
    for n in (32, 64):
        v, g = field_utils.field_grids(f, n)
        assert v.dtype == torch.float32 and g.dtype == torch.float16 and v.shape == g.shape == (n, n, n)
        v_ref, g_ref = ref.extract_grid(wts, nl, n, 0.5)
        frac, mx = _value_ok(v, v_ref)
        eq, within, gmx = _grad_ok(g, g_ref)
        print(f"{nl}/{hidden} n={n}: value within bar {frac:.6f} (max {mx:.2e}); grad == fp16(ref) {eq:.5f}, "
              f"within bar {within:.6f} (max {gmx:.2e})")
        assert frac == 1.0, (n, frac, mx)
        assert _grad_bar_ok(nl, within) and eq >= 0.99, (n, eq, within, gmx)
    # the point-list route of Field.density (inference) for the same configuration
    xs, _ = helpers.random_points(5001, aabb_half=0.5, seed=3, outside_frac=0.0)
    got = f(xs.to(device), return_grad=False)[0][:, 0]
    frac, mx = _value_ok(got, ref.field_value_grad(xs, wts, nl)[0])
    assert frac == 1.0, (frac, mx)


@pytest.mark.parametrize("nl,hidden", [("elu", 16), ("relu", 32)])
def test_oracle_parity_fp16(device, nl, hidden):
    from quadraturefields_amd import field_utils
    f = _field(device, nl, hidden)
    wts = _wts(f)
    f.compute_dtype = "fp16"
    n = 32
    v, g = field_utils.field_grids(f, n)
    v_ref, g_ref = ref.extract_grid(wts, nl, n, 0.5, round16=True)
    frac, mx = _value_ok(v, v_ref)
    gd = (g.cpu().double() - g_ref).abs()
    gfrac = float((gd <= 2e-5 + (2e-5 + HALF_ULP) * g_ref.abs() + 2.0 ** -25).double().mean())
    gmax = float((gd - HALF_ULP * g_ref.abs()).max())
    print(f"fp16 {nl}/{hidden}: value within bar {frac:.5f} (max {mx:.2e}); grad within bar {gfrac:.5f} "
          f"(max beyond the fp16 half ulp {gmax:.2e})")
    assert frac >= 0.99 and mx <= 5e-4
    assert gfrac >= 0.99 and (gmax <= 5e-4 or nl == "relu")      # ReLU: the kink flips of _grad_bar_ok
    # the fp32 kernel is further from the fp16 reference
    f.compute_dtype = "fp32"
    frac32, _ = _value_ok(field_utils.field_grids(f, n)[0], v_ref)
    assert frac32 < frac


def _raw(f, axis, n, xb, xc, pool):
    from quadraturefields_amd import _C
    v = torch.empty((xc, n, n), dtype=torch.float32, device=axis.device)
    g = torch.empty((xc, n, n), dtype=torch.float16, device=axis.device)
    f_ = f
    name, table = f_.extract_entry()
    st = getattr(_C.lib(), name)(
        f_.xyz_encoder.grid.desc, _C.ptr(table), float(f_.scale), f_.hidden_size, f_.activation_code,
        *[_C.ptr(t) for t in f_.decoder_arrays()], _C.ptr(axis), n, xb, xc, pool, None, 0, None, _C.ptr(v), _C.ptr(g),
        _C.stream())
    return st, v, g


def test_pool2_is_cpu_avgpool3d_of_pool1(device):
    """Pool 2 = torch's CPU AvgPool3d of the kernel's own pool-1 lattice values, bit for bit (value grid).  The
    gradient grid's pool-1 output is already fp16, so it pins the gradient pooling to one fp16 ulp only; the value grid
    runs through the same reduction code."""
    from quadraturefields_amd.field_utils import lattice_axis
    f = _field(device, "elu", 16)
    n = 24
    axis = lattice_axis(n, 0.5, device)
    st1, v1, g1 = _raw(f, axis, 2 * n, 0, 2 * n, 1)
    st2, v2, g2 = _raw(f, axis, n, 0, n, 2)
    assert st1 == 0 and st2 == 0
    assert torch.equal(v2.cpu(), F.avg_pool3d(v1.cpu()[None, None], 2, 2)[0, 0])
    gp = F.avg_pool3d(g1.cpu().float()[None, None], 2, 2)[0, 0].half().double()
    assert float((g2.cpu().double() - gp).abs().max()) <= float(gp.abs().max()) * 2.0 ** -10


def test_slabs_are_bit_identical(device):
    from quadraturefields_amd import field_utils
    f = _field(device, "elu", 16)
    v, g = field_utils.field_grids(f, 40)
    for step in (1, 3, 7, 16):
        vs, gs = field_utils.field_grids(f, 40, x_slab=step)
        assert torch.equal(vs, v) and torch.equal(gs, g), step


def test_invalid_arguments_are_refused(device):
    from quadraturefields_amd.field_utils import lattice_axis
    f = _field(device, "elu", 16)
    axis = lattice_axis(8, 0.5, device)
    assert _raw(f, axis, 8, 4, 5, 2)[0] == -1          # slab beyond n
    assert _raw(f, axis, 8, 0, 8, 3)[0] == -3          # pool 3


@pytest.mark.parametrize("nl", ["elu", "relu"])
def test_closed_form_affine_field(device, nl):
    """Feature columns of w1 zeroed and every pre-activation positive: the field is affine in x01, each voxel the
    affine map at the mean of its eight lattice points, every gradient norm |c| / (2 scale)."""
    from quadraturefields_amd import field_utils
    f = _field(device, nl, 16).cpu()
    d = f.decoder_field
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        d.layers[0].weight[:, 3:] = 0
        d.layers[0].weight[:, :3] = torch.rand(16, 3, generator=g) * 2 - 1
        d.layers[0].bias[:] = 4.0
        d.layers[1].weight[:] = (torch.rand(16, 16, generator=g) * 2 - 1) * 0.1
        d.layers[1].bias[:] = 8.0
    f = f.to(device)
    W1, b1 = d.layers[0].weight.double().cpu(), d.layers[0].bias.double().cpu()
    W2, b2 = d.layers[1].weight.double().cpu(), d.layers[1].bias.double().cpu()
    wo, bo = d.lout.weight.double().cpu(), d.lout.bias.double().cpu()
    c = (wo @ W2 @ W1[:, :3])[0]
    c0 = float((wo @ (W2 @ b1 + b2) + bo)[0])
    n = 32
    v, gn = field_utils.field_grids(f, n)
    x01 = ((ref.lattice_axis(n, 0.5) + 0.5) / 1.0).double()                       # the kernel's fp32 x01
    m = (x01[0::2] + x01[1::2]) / 2
    want = c0 + c[0] * m[:, None, None] + c[1] * m[None, :, None] + c[2] * m[None, None, :]
    mag = float(wo.abs() @ (W2.abs() @ (W1.abs()[:, :3].sum(1) + b1.abs()) + b2.abs())) + abs(float(bo))
    assert float((v.cpu().double() - want).abs().max()) <= 2e-6 * mag
    gw = float(c.norm()) / (2 * 0.5)
    assert float((gn.cpu().double() - gw).abs().max()) <= gw * (2.0 ** -10 + 2e-5)


def test_fused_route_matches_the_autograd_route(device):
    """The fused kernel against the reference-shaped route (``Field.forward`` with ``return_grad=True`` through
    autograd: HIP grid encode + torch decoder) on the same field, and a back_prop=True copy takes that route itself."""
    from quadraturefields_amd import field_utils
    from quadraturefields_amd.field import Field
    f = _field(device, "elu", 16)
    n = 16
    v, g = field_utils.field_grids(f, n)
    va, ga = field_utils.field_grids(lambda x: f(x), n, scale=0.5)
    frac, mx = _value_ok(v, va.cpu())
    assert frac == 1.0, mx
    gd = (g.cpu().double() - ga.cpu().double()).abs()
    assert float((gd - 2.0 ** -10 * ga.cpu().double().abs()).max()) <= 2e-5 + 1e-4 * float(ga.abs().max())
    fb = Field(log2_T=14, hidden_size=16, nl="elu", **dict(STAGE2, back_prop=True))
    fb.load_state_dict(f.state_dict())
    fb = fb.to(device)
    assert not field_utils.fused_route(fb) and field_utils.fused_route(f)
    vb, gb = field_utils.field_grids(fb, n)
    assert torch.equal(vb, va)


def _radiance(device, lobes):
    from quadraturefields_amd import synthetic
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceField, NGPRadianceFieldSGNew
    kw = dict(use_viewdirs=False, num_g_lobes=lobes) if lobes else {}
    cls = NGPRadianceFieldSGNew if lobes else NGPRadianceField
    f = cls(aabb=[-1.5, -1.5, -1.5, 1.5, 1.5, 1.5], log2_hashmap_size=14, **kw)
    f.load_state_dict(synthetic.seeded_ngp_state(14, f.mlp_base.grid.n_rows, sg_lobes=lobes), strict=False)
    return f.to(device)


@pytest.mark.parametrize("lobes", [0, 3])
def test_density_grid_matches_the_reference(device, lobes):
    from quadraturefields_amd import field_utils
    m = _radiance(device, lobes)
    n = 32
    got = field_utils.density_grid(m, 1.5, n)
    assert got.dtype == torch.float16 and got.shape == (n, n, n)
    want = ref.extract_density_grid(helpers.oracle_ngp_weights(m), n, 1.5)
    err = (got.cpu().double() - want).abs()
    assert bool((err <= 1e-7 + (5e-5 + HALF_ULP) * want.abs() + 2.0 ** -25).all()), float(err.max())
    assert float(want.max()) > 1.0
    # the lattice's endpoint planes sit on the aabb: the strict selector makes their density 0
    axis = ref.lattice_axis(n, 1.5)
    ends = torch.tensor([axis[0], axis[-1]])
    for pts in (ref.lattice_points(axis, ends), ref.lattice_points(axis, axis)[:: 2 * n]):
        d = m.query_density(pts.to(device))
        on = ((pts.abs() == 1.5).any(1)).to(device)
        assert bool((d[on] == 0).all())


def test_files_and_the_example_script(device, tmp_path):
    from quadraturefields_amd import field_utils
    from quadraturefields_amd.estimators import OccGridEstimator
    from quadraturefields_amd.field import Field
    f = _field(device, "elu", 16)
    n = 24
    field_utils.extract_grid(f, str(tmp_path), scale=0.5, grid_size=n)
    grids = np.load(os.path.join(tmp_path, "grids_valid.npy"))
    grads = np.load(os.path.join(tmp_path, "grads_valid.npy"))
    v, g = field_utils.field_grids(f, n)
    assert grids.dtype == np.float32 and grads.dtype == np.float16 and grids.shape == grads.shape == (n, n, n)
    assert np.array_equal(grids, v.cpu().numpy()) and np.array_equal(grads, g.cpu().numpy())
    m = _radiance(device, 0)
    prefix = str(tmp_path) + "/d_"
    field_utils.extract_density_grid(m, 1.5, prefix, grid_size=n)
    dens = np.load(prefix + "density_grids_valid.npy")
    assert dens.dtype == np.float16 and dens.shape == (n, n, n)
    assert np.array_equal(dens, field_utils.density_grid(m, 1.5, n).cpu().numpy())

    # the example: synthetic stage-1 / stage-2 checkpoints -> the four files -> examples/extract_mesh.py -> mesh.ply
    est = OccGridEstimator(roi_aabb=[-1.5] * 3 + [1.5] * 3, resolution=128, levels=1)
    est.binaries.fill_(True)
    torch.save({"model": {k: t.cpu() for k, t in m.state_dict().items()}, "estimator": est.state_dict()},
               tmp_path / "stage1.pth")
    f2 = Field(log2_T=30, hidden_size=16, nl="elu", **STAGE2)
    sd = f2.state_dict()
    small = _field("cpu", "elu", 16, log2_T=12).state_dict()
    for k in sd:
        if k.startswith("decoder_field"):
            sd[k] = small[k]
    # a smooth field: the radial distance in x01 fed through the w1 column of x01.x (|grad| varies, surfaces exist)
    sd["decoder_field.layers.0.weight"][:, 3:] = 0
    torch.save({"model": sd, "estimator": est.state_dict()}, tmp_path / "stage2.pth")
    del f2, sd
    root = str(tmp_path / "out") + "/"
    env = dict(os.environ, PYTHONPATH=ROOT)
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "extract_field_grids.py"),
                           str(tmp_path / "stage1.pth"), str(tmp_path / "stage2.pth"), root, "--log2_hashmap_size", "14",
                           "--grid_size", "48"], env=env, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-3000:]
    for name, dt in (("binaries.npy", np.bool_), ("density_grids_valid.npy", np.float16),
                     ("grids_valid.npy", np.float32), ("grads_valid.npy", np.float16)):
        a = np.load(root + name)
        assert a.dtype == dt, name
        assert a.shape == ((1, 128, 128, 128) if name == "binaries.npy" else (48, 48, 48)), name
    args = [root, "100.0", "True", "30.0", "0.0", "0", "True", "0.01", "10.0"]
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "extract_mesh.py")] + args, env=env,
                          capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr[-3000:]
    from quadraturefields_amd.mesh_io import load_mesh
    mesh = load_mesh(root + "mesh.ply")
    assert len(mesh.faces) > 0


def test_reference_table_size(device):
    """Stage 2's table (log2_T = 30: 16 dense levels, 39 601 112 rows, 317 MB fp32) at n = 1024: finite outputs, 4096
    random voxels against the oracle, and no per-point intermediates (peak allocation = outputs + a small slack)."""
    from quadraturefields_amd import field_utils
    f = _field(device, "elu", 16, log2_T=30)
    assert f.xyz_encoder.grid.n_rows == 39_601_112
    n = 1024
    out_bytes = n ** 3 * (4 + 2)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    v, g = field_utils.field_grids(f, n)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"n=1024: peak allocation {peak / 2**20:.1f} MiB, outputs {out_bytes / 2**20:.1f} MiB")
    assert peak <= out_bytes + (4 << 20)
    assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(g).all())
    idx = torch.randint(0, n, (4096, 3), generator=torch.Generator().manual_seed(11))
    wts = _wts(f)
    del f
    vr, gr = ref.extract_grid_voxels(wts, "elu", n, 0.5, idx)
    vi = v[idx[:, 0], idx[:, 1], idx[:, 2]].cpu()
    gi = g[idx[:, 0], idx[:, 1], idx[:, 2]].cpu()
    frac, mx = _value_ok(vi, vr)
    eq, within, gmx = _grad_ok(gi, gr)
    print(f"n=1024: value within bar {frac:.5f} (max {mx:.2e}); grad == fp16(ref) {eq:.5f}, within bar {within:.5f} "
          f"(max {gmx:.2e})")
    assert frac == 1.0 and _grad_bar_ok("elu", within) and eq >= 0.99
