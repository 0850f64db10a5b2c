"""``utils.render_image_with_occgrid_test`` and its kernels (volumetric.hip) against the CPU
restatement ``tests/volumetric_frame_reference.py``: the sample lists, alive sets and near planes of every round exactly,
the image within the occupancy-render bar of ``tests/test_gpu_occgrid.py`` (5e-4); ``qf_mark_visited_cells`` and
``mc_utils.transmittance_mask`` exactly.

Threshold margins.  A ray stops when its opacity passes ``opc_thre = 1 - early_stop_eps``; the device composites in fp32,
the restatement in fp64, so a round-end opacity next to the threshold could flip the decision by rounding alone.  Before
any device result is looked at, the analytic cases assert ON THE RESTATEMENT that no ray comes near it.  For a ray that
ends a round below the threshold that means ``opacity < opc_thre - 1e-3``.  A ray that has passed the threshold lies in
(1 - 1e-4, 1] and can never be 1e-3 away from it; for those the margin is the largest the interval allows to state
simply, transmittance ``1 - opacity <= 1e-5``: 9e-5 from the threshold, a hundred times the fp32 rounding of an opacity.
The densities of the analytic scenes (0, 0.15 and 120 at step 0.05; 0, 0.15 and 1.5 with the alpha filter) are chosen so
that both hold.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import fields as ofields
from tests import helpers
from tests import volumetric_frame_reference as vref

AABB = [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]
STEP = 0.05
EPS = 1e-4
TOL = 5e-4                                  # the occupancy-render bar of tests/test_gpu_occgrid.py
SIGMA_LOW, SIGMA_HIGH = 0.15, 120.0        # see "Threshold margins" above


class AnalyticField(torch.nn.Module):
    """Density constant on the cells of a K^3 lattice over the aabb, colour an affine function of position: every
    operation is a basic IEEE one, so the CPU and the device evaluate it to the same bits at the same positions."""

    def __init__(self, table, aabb=AABB):
        super().__init__()
        self.register_buffer("table", torch.as_tensor(table, dtype=torch.float32))
        self.register_buffer("aabb", torch.tensor(aabb, dtype=torch.float32))

    def normalize(self, x):
        x01 = (x - self.aabb[:3]) / (self.aabb[3:] - self.aabb[:3])
        return ((x01 > 0.0) & (x01 < 1.0)).all(dim=-1), x01

    def forward(self, positions, directions):
        k = self.table.shape[0]
        c = torch.floor(self.normalize(positions)[1] * k).long().clamp(0, k - 1)
        sigma = self.table[c[:, 0], c[:, 1], c[:, 2]]
        rgb = (0.5 + 0.25 * positions).clamp(0.0, 1.0) * (0.75 + 0.25 * directions[:, 2:3])
        return rgb, sigma[:, None]


def _sphere_rays(n, seed, radius=3.0, spread=1.1):
    rng = np.random.default_rng(seed)
    o = rng.normal(size=(n, 3))
    o = (o / np.linalg.norm(o, axis=1, keepdims=True) * radius).astype(np.float32)
    d = rng.uniform(-spread, spread, size=(n, 3)).astype(np.float32) - o
    return o, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def _table(seed, k=4, p_high=0.25, p_low=0.5):
    u = np.random.default_rng(seed).random((k, k, k))
    return np.where(u < p_high, SIGMA_HIGH, np.where(u < p_high + p_low, SIGMA_LOW, 0.0)).astype(np.float32)


def _scene(name):
    """(binaries bool [r,r,r], origins, viewdirs (flat fp32), image shape or None, density table, render kwargs)."""
    rng = np.random.default_rng(7)
    kw = {"render_bkgd": [1.0, 1.0, 1.0]}
    shape = None
    table = _table(3)
    if name in ("random8", "black", "alpha_thre"):
        b = rng.random((8, 8, 8)) < 0.45
        o, d = _sphere_rays(1000, 1)
        o[:25] += 40.0                                             # some rays miss the box
        if name == "black":
            kw["render_bkgd"] = [0.0, 0.0, 0.0]
        if name == "alpha_thre":
            # alpha(0.15) = 0.0075 is filtered, alpha(1.5) = 0.072 is not.  A filtered sample attenuates only inside its
            # round, so with opaque cells the opacity could end a round anywhere below the threshold; at 1.5 a full
            # diagonal of 70 samples stays at opacity <= 1 - exp(-5.25) = 0.9948, clear of it
            kw["alpha_thre"] = 0.05
            table = np.where(table == SIGMA_HIGH, np.float32(1.5), table)
    elif name == "image16":
        from quadraturefields_amd import synthetic
        b = np.kron(rng.random((4, 4, 4)) < 0.5, np.ones((4, 4, 4), dtype=bool))
        c2w = synthetic.orbit_cameras(1, radius=3.0, seed=5)[0]
        ot, dt = synthetic.camera_rays(c2w, synthetic.lego_focal(800) * 32 / 800.0 * 0.4, 32, 32)
        o, d, shape = ot.numpy(), dt.numpy(), (32, 32)
    elif name == "inside16":
        b = rng.random((16, 16, 16)) < 0.5
        o = rng.uniform(-0.9, 0.9, size=(1000, 3)).astype(np.float32)
        d = _sphere_rays(1000, 2)[1]
    elif name == "miss":
        b = np.ones((8, 8, 8), dtype=bool)
        o, d = _sphere_rays(1000, 3)
        o += 40.0
    elif name == "slab":
        b = np.ones((8, 8, 8), dtype=bool)
        table = np.zeros((8, 8, 8), dtype=np.float32)
        table[3:5] = SIGMA_HIGH                                    # |x| < 0.25: opaque after two samples
        o, d = _sphere_rays(1000, 4, spread=0.2)
    elif name == "near_empty":
        b = np.zeros((16, 16, 16), dtype=bool)
        b[:, 8, 8] = True                                          # one column of cells along x, density 0.15
        table = np.full((4, 4, 4), SIGMA_LOW, dtype=np.float32)
        o, d = _sphere_rays(1000, 5)
        o[12:] += 40.0                                             # twelve rays can hit, the rest miss
        o[:12] = np.array([-3.0, 0.03, 0.04], dtype=np.float32) + rng.uniform(-0.02, 0.02, (12, 3)).astype(np.float32)
        d[:12] = np.array([1.0, 0.0, 0.0], dtype=np.float32)
    elif name == "all_false":
        b = np.zeros((8, 8, 8), dtype=bool)
        o, d = _sphere_rays(1000, 6)
    else:
        raise KeyError(name)
    return b, np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32), shape, table, kw


CASES = ["random8", "image16", "inside16", "miss", "slab", "near_empty", "alpha_thre", "black", "all_false"]


@functools.lru_cache(maxsize=None)
def _reference(name, max_samples):
    b, o, d, _, table, kw = _scene(name)
    field = AnalyticField(table)

    def field_fn(pos, dirs):
        rgb, sigma = field(torch.from_numpy(pos), torch.from_numpy(dirs))
        return rgb.numpy(), sigma.numpy()

    return vref.render(max_samples, field_fn, AABB, b, o, d, render_step_size=STEP, early_stop_eps=EPS, **kw)


def _assert_margins(rounds):
    """See the module docstring: on the restatement alone, before any device result is compared."""
    opc_thre = float(np.float32(1.0 - EPS))
    entered = np.ones(rounds[0]["alive"].shape[0], dtype=bool)
    for r in rounds:
        op = r["opacity"][entered]
        below = op <= opc_thre
        assert (op[below] < opc_thre - 1e-3).all(), float(op[below].max())
        assert (1.0 - op[~below] <= 1e-5).all(), float((1.0 - op[~below]).max())
        entered = r["alive"]


def _estimator(b, device):
    from quadraturefields_amd.estimators import OccGridEstimator
    est = OccGridEstimator(roi_aabb=AABB, resolution=b.shape[0], levels=1).to(device)
    est.binaries.copy_(torch.from_numpy(b)[None].to(device))
    return est


def _rays(o, d, shape, device):
    from quadraturefields_amd.datasets.utils import Rays
    to = lambda a: torch.from_numpy(a).to(device).reshape((*shape, 3) if shape else (-1, 3))
    return Rays(origins=to(o), viewdirs=to(d))


def _compare_rounds(trace, rounds):
    assert len(trace) == len(rounds)
    for got, want in zip(trace, rounds):
        assert (got["n_alive"], got["n_samples"]) == (want["n_alive"], want["n_samples"])
        assert np.array_equal(got["ray_indices"].cpu().numpy(), want["ray_indices"])
        assert np.array_equal(got["t_starts"].cpu().numpy(), want["t_starts"])
        assert np.array_equal(got["t_ends"].cpu().numpy(), want["t_ends"])
        assert np.array_equal(got["alive"].cpu().numpy(), want["alive"])
        assert np.array_equal(got["near"].cpu().numpy(), want["near"])


@pytest.mark.gpu
@pytest.mark.parametrize("max_samples", [1, 7, 64, 1024])
@pytest.mark.parametrize("name", CASES)
def test_analytic_field_rounds_and_image(device, name, max_samples):
    from quadraturefields_amd import utils
    rounds, (rgb_o, op_o, dep_o, total_o, pos_o) = _reference(name, max_samples)
    _assert_margins(rounds)
    b, o, d, shape, table, kw = _scene(name)
    trace = []
    bk = torch.tensor(kw["render_bkgd"], device=device)
    rgb, opac, depth, total, positions = utils.render_image_with_occgrid_test(
        max_samples, AnalyticField(table).to(device), _estimator(b, device), _rays(o, d, shape, device),
        render_step_size=STEP, render_bkgd=bk, alpha_thre=kw.get("alpha_thre", 0.0), early_stop_eps=EPS, trace=trace)
    lead = shape if shape else (o.shape[0],)
    assert rgb.shape == (*lead, 3) and opac.shape == (*lead, 1) and depth.shape == (*lead, 1)
    _compare_rounds(trace, rounds)
    assert total == total_o
    assert np.array_equal(positions.cpu().numpy(), pos_o)
    err = [float(np.abs(a.reshape(len(o), -1).cpu().numpy().astype(np.float64) - w.reshape(len(o), -1)).max())
           for a, w in ((rgb, rgb_o), (opac, op_o), (depth, dep_o))]
    print(f"{name} max_samples={max_samples}: rounds={len(rounds)} samples={total} max err rgb/opacity/depth = {err}")
    assert max(err) <= TOL, err
    # what each case is about
    if name in ("miss", "all_false"):
        assert len(rounds) == 1 and total == 0 and positions.shape == (0, 3)
        assert torch.equal(rgb, torch.ones_like(rgb)) and not opac.any()
    if max_samples == 1024:
        sizes = [r["n_samples"] for r in rounds]
        if name == "near_empty":
            assert sizes[0] == 1 and max(sizes) == 64 and rounds[1]["n_alive"] <= 12
        if name == "slab":
            # the rays end in the round in which the opacity crosses, with whatever that round still marched behind it
            stopped = (op_o > 1.0 - EPS)
            assert stopped.mean() > 0.5
            per_ray = np.bincount(np.concatenate([r["ray_indices"] for r in rounds]), minlength=len(o))
            whole = vref.march_round(AABB, b, o, d, np.zeros(len(o), np.float32), np.ones(len(o), bool), 1 << 20, 1e10,
                                     STEP)[3]
            assert (per_ray[stopped] < whole[stopped]).all()               # every stopped ray left samples unmarched
            assert per_ray.sum() < 0.6 * whole.sum()
        if name == "alpha_thre":
            assert 0 < total < positions.shape[0]
        if name == "black":
            assert np.array_equal(_reference("random8", 1024)[1][4], pos_o)
        if name == "inside16":
            assert rounds[0]["ray_indices"].shape[0] > 300                 # origins inside the box: samples start at t = 0
            assert float(rounds[0]["t_starts"].min()) == 0.0


@functools.lru_cache(maxsize=None)
def _box_reference(max_samples):
    """The capped rounds on the asymmetric box and the 32 x 16 x 48 grid of tests/asymmetric_inputs.py, its 600 rays."""
    from tests import asymmetric_inputs as asym
    b = asym.binaries()
    o, d = asym.march_rays()
    table = _table(5)
    field = AnalyticField(table, asym.BOX)

    def field_fn(pos, dirs):
        rgb, sigma = field(torch.from_numpy(pos), torch.from_numpy(dirs))
        return rgb.numpy(), sigma.numpy()

    ref = vref.render(max_samples, field_fn, asym.BOX, b, o, d, render_step_size=STEP, early_stop_eps=EPS,
                      render_bkgd=[1.0, 1.0, 1.0])
    return b, o, d, table, ref


@pytest.mark.gpu
@pytest.mark.parametrize("max_samples", [7, 1024])
def test_capped_rounds_on_the_asymmetric_box_and_grid(device, max_samples):
    """``qf_grid_march_round_count`` / ``_write`` (through the renderer's trace) against ``march_round`` where the three
    extents, the three resolutions and the box's centre all differ: every round's sample lists, alive sets and near
    planes exactly, the image within the bar of the cases above."""
    from quadraturefields_amd import utils
    from quadraturefields_amd.estimators import OccGridEstimator
    from tests import asymmetric_inputs as asym
    b, o, d, table, (rounds, (rgb_o, op_o, dep_o, total_o, pos_o)) = _box_reference(max_samples)
    _assert_margins(rounds)
    assert len(rounds) > 3 and total_o > (1000 if max_samples == 1024 else 100)
    assert len({r["n_samples"] for r in rounds}) > 1       # the quota grows as rays retire
    est = OccGridEstimator(roi_aabb=asym.BOX, resolution=list(asym.RES), levels=1).to(device)
    est.binaries.copy_(torch.from_numpy(b)[None].to(device))
    trace = []
    rgb, opac, depth, total, positions = utils.render_image_with_occgrid_test(
        max_samples, AnalyticField(table, asym.BOX).to(device), est, _rays(o, d, None, device), render_step_size=STEP,
        render_bkgd=torch.ones(3, device=device), early_stop_eps=EPS, trace=trace)
    _compare_rounds(trace, rounds)
    assert total == total_o
    assert np.array_equal(positions.cpu().numpy(), pos_o)
    err = [float(np.abs(a.reshape(len(o), -1).cpu().numpy().astype(np.float64) - w.reshape(len(o), -1)).max())
           for a, w in ((rgb, rgb_o), (opac, op_o), (depth, dep_o))]
    print(f"box max_samples={max_samples}: rounds={len(rounds)} samples={total} max err rgb/opacity/depth = {err}")
    assert max(err) <= TOL, err


@functools.lru_cache(maxsize=None)
def _ngp_case(seed=42):
    from quadraturefields_amd import synthetic
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceField
    field = NGPRadianceField(aabb=AABB, log2_hashmap_size=14)
    field.load_state_dict(synthetic.seeded_ngp_state(14, field.mlp_base.grid.n_rows, seed=seed), strict=False)
    field = field.eval()
    b = np.kron(np.random.default_rng(11).random((4, 4, 4)) < 0.5, np.ones((4, 4, 4), dtype=bool))
    c2w = synthetic.orbit_cameras(1, radius=3.0, seed=5)[0]
    o, d = synthetic.camera_rays(c2w, synthetic.lego_focal(800) * 32 / 800.0 * 0.4, 32, 32)
    wts = helpers.oracle_ngp_weights(field)

    def field_fn(pos, dirs):
        rgb, sigma = ofields.ngp_forward(torch.from_numpy(pos), torch.from_numpy(dirs), wts)
        return rgb.numpy(), sigma.reshape(-1).numpy()

    ref = vref.render(1024, field_fn, AABB, b, o.numpy(), d.numpy(), render_step_size=STEP, early_stop_eps=EPS,
                      render_bkgd=[1.0, 1.0, 1.0])
    return field, b, o.numpy(), d.numpy(), ref


@pytest.mark.gpu
def test_ngp_field_frame(device):
    """NGPRadianceField, T = 2^14, fp32, seeded weights, through the fused kernel with the device-side sample count.  The
    restatement evaluates the field with ``oracle/fields.py``.  Rays whose restated opacity ends a round within 1e-4 of
    the threshold may flip and are excluded -- at most 1 % of them, asserted on the restatement."""
    from quadraturefields_amd import utils
    field, b, o, d, (rounds, (rgb_o, op_o, dep_o, total_o, pos_o)) = _ngp_case()
    excluded = vref.threshold_margin(rounds, EPS) <= 1e-4
    assert excluded.mean() <= 0.01, excluded.mean()
    keep = ~excluded
    trace = []
    rgb, opac, depth, total, positions = utils.render_image_with_occgrid_test(
        1024, field.to(device), _estimator(b, device), _rays(o, d, (32, 32), device), render_step_size=STEP,
        render_bkgd=torch.ones(3, device=device), early_stop_eps=EPS, trace=trace)
    assert len(trace) == len(rounds) and total_o > 2000
    for got, want in zip(trace, rounds):
        counts = np.bincount(got["ray_indices"].cpu().numpy(), minlength=len(o))
        assert np.array_equal(counts[keep], want["count"][keep])
    err = [float(np.abs(a.reshape(len(o), -1).cpu().numpy().astype(np.float64) - w.reshape(len(o), -1))[keep].max())
           for a, w in ((rgb, rgb_o), (opac, op_o))]
    print(f"ngp: rounds={len(rounds)} samples={total} excluded={int(excluded.sum())} max err rgb/opacity = {err}")
    assert max(err) <= TOL, err
    if not excluded.any():
        assert total == total_o and np.array_equal(positions.cpu().numpy(), pos_o)


@pytest.mark.gpu
def test_mark_visited_cells(device):
    from quadraturefields_amd import mc_utils
    m = 16
    rng = np.random.default_rng(0)
    p = rng.random((5000, 3)).astype(np.float32)
    p[:8] = np.array([[0, 0, 0], [1, 1, 1], [0, 1, 0.5], [1, 0, 0], [2 / 15, 7 / 15, 1], [1.0000001, 0.5, 0.5],
                      [0.5, -1e-7, 0.5], [0.5, 0.5, np.nan]], dtype=np.float32)
    p[100:140] = rng.uniform(-0.5, 1.5, (40, 3)).astype(np.float32)
    want, bad = vref.mark_visited_cells(p, m)
    assert bad >= 3 and want[0, 0, 0] and want[m - 1, m - 1, m - 1]
    mask = torch.zeros((m, m, m), dtype=torch.bool, device=device)
    counter = torch.zeros((1,), dtype=torch.int64, device=device)
    mc_utils.mark_visited_cells(torch.from_numpy(p).to(device), mask, counter)
    assert np.array_equal(mask.cpu().numpy(), want)
    assert int(counter.item()) == bad
    with pytest.raises(ValueError):
        mc_utils.mark_visited_cells(torch.from_numpy(p), mask)
    with pytest.raises(ValueError):
        mc_utils.mark_visited_cells(torch.from_numpy(p).to(device), mask[:, :, :8])


@pytest.mark.gpu
def test_transmittance_mask(device):
    from quadraturefields_amd import mc_utils
    b, o, d, _, table, _ = _scene("random8")
    o2, d2 = _sphere_rays(1000, 9)
    field = AnalyticField(table)
    views = [(o, d), (o2, d2)]
    coarse = np.zeros((8, 8, 8), dtype=bool)
    for vo, vd in views:
        def field_fn(pos, dirs):
            rgb, sigma = field(torch.from_numpy(pos), torch.from_numpy(dirs))
            return rgb.numpy(), sigma.numpy()
        pos = vref.render(1024, field_fn, AABB, b, vo, vd, render_step_size=STEP, early_stop_eps=EPS,
                          render_bkgd=[1.0, 1.0, 1.0])[1][4]
        got, bad = vref.mark_visited_cells(field.normalize(torch.from_numpy(pos))[1].numpy(), 8)
        assert bad == 0
        coarse |= got
    want = torch.nn.Upsample((32, 32, 32), mode="trilinear", align_corners=False)(
        torch.from_numpy(coarse)[None, None].float())[0, 0] > 0.5
    assert 0.02 < want.float().mean() < 0.98
    bk = torch.ones(3, device=device)
    got = mc_utils.transmittance_mask(
        field.to(device), _estimator(b, device),
        [{"rays": _rays(o, d, None, device), "color_bkgd": bk}, _rays(o2, d2, None, device)],
        max_samples=1024, chunk_size=8, size=32, render_step_size=STEP, early_stop_eps=EPS)
    assert got.dtype == torch.bool and got.shape == (32, 32, 32) and got.is_cuda
    assert torch.equal(got.cpu(), want)


@pytest.mark.gpu
def test_argument_validation(device):
    from quadraturefields_amd import utils
    b, o, d, _, table, _ = _scene("all_false")
    field, est, rays = AnalyticField(table).to(device), _estimator(b, device), _rays(o, d, None, device)
    bk = torch.ones(3, device=device)
    with pytest.raises(NotImplementedError):
        utils.render_image_with_occgrid_test(16, field, est, rays, render_bkgd=bk, cone_angle=0.004)
    with pytest.raises(NotImplementedError):
        utils.render_image_with_occgrid_test(16, field, est, rays, render_bkgd=bk, timestamps=torch.zeros(1, device=device))
    with pytest.raises(ValueError):
        utils.render_image_with_occgrid_test(16, field, est, _rays(o, d, None, "cpu"), render_bkgd=bk)
    for bad in (0, -3):
        with pytest.raises(ValueError):
            utils.render_image_with_occgrid_test(bad, field, est, rays, render_bkgd=bk)


def test_dropin_import():
    from quadraturefields_amd import utils
    from quadraturefields_amd.dropin.utils import render_image_with_occgrid_test
    assert render_image_with_occgrid_test is utils.render_image_with_occgrid_test
