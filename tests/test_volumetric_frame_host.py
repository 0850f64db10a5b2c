"""CPU: hand-worked cases that pin ``tests/volumetric_frame_reference.py``, the restatement the device renderer
``utils.render_image_with_occgrid_test`` is tested against."""
import math

import numpy as np
import pytest

from tests import volumetric_frame_reference as vref

AABB = [-1, -1, -1, 1, 1, 1]
STEP = 0.125


@pytest.fixture(autouse=True)
def _renderer_under_test(lib):
    """The restatement pins a renderer: the function and its entry points must exist for these tests to mean anything."""
    from quadraturefields_amd import utils
    assert callable(utils.render_image_with_occgrid_test)
    for name in ("qf_grid_march_round_count", "qf_grid_march_round_write", "qf_volumetric_accumulate", "qf_mark_visited_cells"):
        getattr(lib, name)


def _column_scene():
    """A 4^3 grid over [-1,1]^3 (cells of 0.5) with two occupied cells on the line y = z = 0.25.  Ray 0 runs along +x
    from x = -2: it enters the box at t = 1, cell 1 spans t in [1.5, 2), cell 3 spans [2.5, 3): four steps of 0.125 in
    each, all of them dyadic, so every t is exact in fp32.  Ray 1 misses the box."""
    b = np.zeros((4, 4, 4), dtype=bool)
    b[1, 2, 2] = b[3, 2, 2] = True
    o = np.array([[-2.0, 0.25, 0.25], [-2.0, 5.0, 5.0]], dtype=np.float32)
    d = np.array([[1.0, 0.0, 0.0], [1.0, 0.0, 0.0]], dtype=np.float32)
    return b, o, d


def _field(sigma_first, sigma_second):
    def fn(pos, dirs):
        sigma = np.where(pos[:, 0] < 0.0, sigma_first, sigma_second)         # cell 1 lies in x < 0, cell 3 in x > 0
        rgb = np.stack([np.full(len(pos), 0.25), 0.5 + 0.25 * pos[:, 0], np.ones(len(pos))], axis=1)
        return rgb, sigma
    return fn


def test_n_samples_schedule():
    n = 1040
    assert [vref.n_samples_for(n, a) for a in (n, n // 2 + 1, n // 2, n // 65, 1)] == [1, 1, 2, 64, 64]
    assert n // (n // 65) == 65                       # the cap, not the quotient, gives the 64
    assert vref.n_samples_for(7, 100) == 1            # more alive rays than rays cannot happen; min_samples = 1 holds anyway


def test_max_samples_is_tested_before_the_round():
    # 100 rays: quotas 1, 2, 2 bring iter_samples to 5 < 6, so a fourth round runs and overshoots to 7
    assert vref.schedule(100, 6, [100, 40, 40, 40, 40, 40]) == [(1, 1), (2, 3), (2, 5), (2, 7)]
    assert vref.schedule(100, 7, [100, 40, 40, 40, 40, 40]) == [(1, 1), (2, 3), (2, 5), (2, 7)]
    assert vref.schedule(100, 1, [100, 40]) == [(1, 1)]
    assert vref.schedule(100, 1024, [100, 0, 40]) == [(1, 1)]              # no ray alive ends the loop
    b, o, d = _column_scene()
    rounds, _ = vref.render(4, _field(0.0, 0.0), AABB, b, o, d, render_step_size=STEP)
    assert [r["n_samples"] for r in rounds] == [1, 2, 2]                   # 1 + 2 = 3 < 4: the third round overshoots to 5


def test_a_ray_stays_alive_iff_it_filled_its_quota():
    b, o, d = _column_scene()
    rounds, out = vref.render(1024, _field(0.0, 0.0), AABB, b, o, d, render_step_size=STEP)
    # round 1: two alive rays, quota 1; ray 1 misses and dies.  Then ray 0 alone: quota 2 // 1 = 2 until its 8 samples
    # are used up -- the fifth round finds only one and the ray leaves the box
    assert [r["n_alive"] for r in rounds] == [2, 1, 1, 1, 1]
    assert [r["n_samples"] for r in rounds] == [1, 2, 2, 2, 2]
    assert [r["count"].tolist() for r in rounds] == [[1, 0], [2, 0], [2, 0], [2, 0], [1, 0]]
    assert [r["alive"].tolist() for r in rounds] == [[True, False]] * 4 + [[False, False]]
    starts = np.concatenate([r["t_starts"] for r in rounds])
    assert starts.tolist() == [1.5, 1.625, 1.75, 1.875, 2.5, 2.625, 2.75, 2.875]
    # the near plane is the end of the last kept sample, and the clipped exit once the ray ran out of box
    assert [float(r["near"][0]) for r in rounds] == [1.625, 1.875, 2.625, 2.875, 3.0]
    assert out[3] == 8 and out[4].shape == (8, 3)
    assert out[4][:, 0].tolist() == [-2.0 + t + 0.0625 for t in starts.tolist()]
    # dead rays emit nothing: every sample belongs to ray 0
    assert all((r["ray_indices"] == 0).all() for r in rounds)


def test_prefix_transmittance_over_rounds_equals_one_pass_and_depth_is_not_normalised():
    b, o, d = _column_scene()
    sigma = 3.0
    rounds, (rgb, opacity, depth, total, _) = vref.render(1024, _field(sigma, sigma), AABB, b, o, d, render_step_size=STEP,
                                                          render_bkgd=[1.0, 1.0, 1.0])
    assert len(rounds) == 5                                                # the eight samples were split over five rounds
    mids = np.array([1.5, 1.625, 1.75, 1.875, 2.5, 2.625, 2.75, 2.875]) + 0.0625
    alpha = 1.0 - math.exp(-sigma * STEP)
    w = np.array([math.exp(-sigma * STEP * i) * alpha for i in range(8)])  # one unsplit pass
    assert abs(opacity[0] - w.sum()) < 1e-14 and abs(w.sum() - (1.0 - math.exp(-sigma))) < 1e-14
    assert abs(depth[0] - (w * mids).sum()) < 1e-13
    assert abs(depth[0] - (w * mids).sum() / w.sum()) > 0.05               # NOT divided by the opacity
    green = 0.5 + 0.25 * (mids - 2.0)
    assert abs(rgb[0, 1] - ((w * green).sum() + 1.0 - w.sum())) < 1e-14
    assert rgb[1].tolist() == [1.0, 1.0, 1.0] and opacity[1] == 0.0 and total == 8


def test_early_stop_ends_the_ray_at_the_round_not_the_sample():
    b, o, d = _column_scene()
    # alpha = 1 - e^-6 per sample: opacity passes 1 - 1e-4 with the second sample.  Round 1 holds one sample, round 2 two:
    # the third sample is still composited, the fourth never marched
    rounds, (_, opacity, _, total, positions) = vref.render(1024, _field(48.0, 48.0), AABB, b, o, d, render_step_size=STEP)
    assert [r["count"][0] for r in rounds] == [1, 2] and not rounds[-1]["alive"].any()
    assert total == 3 and positions.shape[0] == 3
    assert abs(opacity[0] - (1.0 - math.exp(-18.0))) < 1e-15


def test_alpha_filter_drops_contributions_but_not_attenuation():
    b, o, d = _column_scene()
    # cell 1: alpha = 1 - exp(-0.0125) = 0.0124 < 0.05, filtered; cell 3: alpha = a = 1 - exp(-0.5) = 0.39.
    # Rounds hold the samples (1) (2,3) (4,5) (6,7) (8).  Inside a round a filtered sample attenuates what lies behind it:
    # sample 5 sees T = exp(-0.0125) from sample 4.  ACROSS rounds only the opacity is carried (prefix = 1 - opacity), and
    # a filtered sample added nothing to it -- the reference's behaviour, restated, not repaired.
    args = (1024, _field(0.1, 4.0), AABB, b, o, d)
    _, (rgb_f, op_f, _, total_f, pos_f) = vref.render(*args, render_step_size=STEP, alpha_thre=0.05)
    _, (_, op_0, _, total_0, pos_0) = vref.render(*args, render_step_size=STEP)
    assert total_f == 4 and total_0 == 8 and pos_f.shape == pos_0.shape == (8, 3)      # positions precede the filter
    a = 1.0 - math.exp(-0.5)
    w5 = math.exp(-0.0125) * a
    w6 = (1.0 - w5) * a
    w7 = (1.0 - w5) * math.exp(-0.5) * a
    w8 = (1.0 - (w5 + w6 + w7)) * a
    assert abs(op_f[0] - (w5 + w6 + w7 + w8)) < 1e-14
    assert abs(w5 - a) > 4e-3                                              # the filter did not restore T to 1
    assert abs(op_0[0] - (1.0 - math.exp(-0.05 - 2.0))) < 1e-14
    assert abs(rgb_f[0, 0] - 0.25 * op_f[0]) < 1e-14


def test_mark_visited_cells_restatement():
    p = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0.5, 0.25, 0.1], [1.5, 0.5, 0.5], [0.5, -0.01, 0.5]], dtype=np.float32)
    mask, bad = vref.mark_visited_cells(p, 5)
    assert bad == 2
    want = {(0, 0, 0), (4, 4, 4), (2, 1, 0), (2, 1, 1)}                    # 0.5 * 4 = 2 and 0.25 * 4 = 1 are their own ceil
    assert set(map(tuple, np.argwhere(mask).tolist())) == want
