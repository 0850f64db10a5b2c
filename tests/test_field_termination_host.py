"""CPU: the rank windows of the front-to-back field frame -- hand-worked cases for
``tests/field_termination_reference.evaluated_counts``, and the named test scene on the CPU oracle alone: both branches
of the rule fire on it, no decision sits near the threshold, every schedule evaluates what the table below says, and
truncation moves a pixel by less than 3 eps (fp64).

The seeded field's densities have a median near 0.84: at the default step 5e-3 no ray of any test scene ever stops, so
the tests of this feature composite with ``render_step_size = 0.5``."""
import math

import numpy as np
import pytest
import torch

from tests import field_termination_reference as T

DELTA = 0.5
K = 25
SCHEDULES = {"(25)": (25,), "(4,25)": (4, 25), "(2,6,25)": (2, 6, 25), "(1,3,7,15,25)": (1, 3, 7, 15, 25)}
# eps -> rays stopping early, samples contributing, samples evaluated per schedule, measured with the oracle
NAMED = {
    1e-2: dict(early=335, contributing=3899, evaluated={"(25)": 5431, "(4,25)": 4875, "(2,6,25)": 4612, "(1,3,7,15,25)": 4425}),
    1e-3: dict(early=210, contributing=4574, evaluated={"(25)": 5431, "(4,25)": 5177, "(2,6,25)": 5044, "(1,3,7,15,25)": 4953}),
}


def test_evaluated_counts_hand_worked():
    # one ray of 10 samples of which the first 4 contribute, schedule (2, 6, 10): it enters [0,2) and [2,6) (kept 4 > 2),
    # not [6,10) (kept 4 <= 6) -> 6 evaluated
    assert T.evaluated_counts([10], [4], (2, 6, 10)).tolist() == [6]
    # a pixel stopping exactly on a window end: kept == 6 means the rank-6 sample does NOT contribute -> [6,10) is not entered
    assert T.evaluated_counts([10], [6], (2, 6, 10)).tolist() == [6]
    assert T.evaluated_counts([10], [7], (2, 6, 10)).tolist() == [10]
    # ... and on the first window's end
    assert T.evaluated_counts([10], [2], (2, 6, 10)).tolist() == [2]
    assert T.evaluated_counts([10], [1], (2, 6, 10)).tolist() == [2]
    # a ray that never stops is evaluated whole, whatever the schedule; a window is cut at the count
    assert T.evaluated_counts([10, 5, 3], [10, 5, 3], (2, 6, 10)).tolist() == [10, 5, 3]
    assert T.evaluated_counts([5], [3], (2, 6, 10)).tolist() == [5]
    # a window starting beyond every count is entered by nobody
    assert T.evaluated_counts([3, 16], [3, 9], (20, 40)).tolist() == [3, 16]
    assert T.evaluated_counts([3, 16], [3, 9], (4, 20, 40)).tolist() == [3, 16]
    # a single window (K): everything is evaluated, whatever contributes
    assert T.evaluated_counts([10, 4, 1], [1, 4, 1], (25,)).tolist() == [10, 4, 1]
    # count == 0, alone and between rays
    assert T.evaluated_counts([0], [0], (2, 6, 10)).tolist() == [0]
    assert T.evaluated_counts([4, 0, 9], [4, 0, 1], (1, 3, 9)).tolist() == [4, 0, 1]
    assert T.evaluated_counts([], [], (5,)).shape == (0,)
    # the cap of 8 windows, one rank each in front
    assert T.evaluated_counts([25, 25], [3, 25], (1, 2, 3, 4, 5, 6, 7, 25)).tolist() == [3, 25]


def test_evaluated_counts_refuses_a_bad_schedule():
    for bad in ((), (0, 5), (3, 3), (5, 4), (2, 6)):          # empty, first < 1, not increasing (twice), too short
        with pytest.raises(AssertionError):
            T.evaluated_counts([10], [4], bad)
    with pytest.raises(AssertionError):
        T.evaluated_counts([3], [4], (5,))                    # more contributing than there are


def test_the_rule_is_the_baked_frames():
    from tests import baked_termination_reference as B
    assert T.contributing_counts is B.contributing_counts and T.stop_tau is B.stop_tau and T.truncate is B.truncate


@pytest.fixture(scope="module")
def oracle_scene():
    """The named scene on the CPU oracle: 8 shells, one orbit camera, 37 x 29 pixels, K = 25, the seeded NGP field at
    T = 2^12.  Ray-major samples with their colours and densities."""
    from oracle import fields, meshpath as om
    from quadraturefields_amd import synthetic
    w, h = 37, 29
    mesh = synthetic.shell_mesh(n_shells=8, subdivisions=2)
    c2w = synthetic.orbit_cameras(1, seed=4)[0]
    o, d = synthetic.camera_rays(c2w, synthetic.lego_focal(800) * w / 800.0, w, h)
    om.build()
    sample = om.sampling_raytrace_numpy(om.BVHIntersector(mesh.vertices, mesh.faces), d.numpy(), o.numpy(), K)
    xyzs, dirs, index_ray, ts, _, _ = om.to_loader_tensors(sample)
    # the weights as tests/helpers.oracle_ngp_weights builds them, from the state dict directly (no product module)
    lv = fields.grid_levels(16, 12, 16, math.exp(math.log(4096 / 16) / 15))
    sd = synthetic.seeded_ngp_state(12, lv.n_entries)
    p = sd["mlp_base.params"].float()
    base, off = fields.split_tcnn_mlp(p, 32, 1, 64, 16)
    table = p[off:].reshape(-1, 2)
    assert table.shape[0] == lv.n_entries
    wts = fields.NGPWeights(aabb=torch.tensor([-1.5] * 3 + [1.5] * 3), levels=lv, table=table, base=base)
    wts.head_tcnn, _ = fields.split_tcnn_mlp(sd["mlp_head.params"].float(), 32, 2, 64, 16)
    rgbs, sigmas = fields.ngp_forward(xyzs, dirs, wts)
    counts = np.bincount(index_ray.numpy(), minlength=w * h)
    return {"n_rays": w * h, "counts": counts, "sigma": sigmas.reshape(-1).numpy(), "rgb": rgbs.numpy(), "depth": ts.numpy()}


def _composite64(s, kept):
    """White-background pixels of the scene's rays in fp64 from the first ``kept`` samples of each ray."""
    out = np.ones((s["n_rays"], 3))
    alpha = np.zeros(s["n_rays"])
    first = np.concatenate([[0], np.cumsum(s["counts"])[:-1]])
    for r in np.nonzero(s["counts"])[0]:
        sl = slice(first[r], first[r] + kept[r])
        tau = s["sigma"][sl].astype(np.float64) * DELTA
        trans = np.exp(-np.concatenate([[0.0], np.cumsum(tau)[:-1]]))
        wgt = trans * (1.0 - np.exp(-tau))
        a = wgt.sum()
        c = (wgt[:, None] * s["rgb"][sl].astype(np.float64)).sum(0)
        out[r] = (1.0 - a) + a * c              # the reference's white blend (the double-alpha quirk, B-1)
        alpha[r] = a
    return out, alpha


@pytest.mark.parametrize("eps", sorted(NAMED))
def test_named_scene_exercises_both_branches(oracle_scene, eps):
    s, want = oracle_scene, NAMED[eps]
    counts = s["counts"]
    hit = counts > 0
    assert int(hit.sum()) == 763 and s["n_rays"] == 1073 and int(counts.sum()) == 5431 and int(counts.max()) == 16
    print(f"density median {float(np.median(s['sigma'])):.3g}")
    stop = T.stop_tau(eps)
    kept = T.contributing_counts(s["sigma"], counts, DELTA, stop)
    early = kept < counts
    print(f"eps {eps}: {int(early.sum())} of {int(hit.sum())} hit rays stop early, {int(kept.sum())} of "
          f"{int(counts.sum())} samples contribute")
    assert (kept[hit] >= 1).all() and (kept[~hit] == 0).all()
    assert int(early.sum()) == want["early"] and int(kept.sum()) == want["contributing"]
    assert 0.25 * hit.sum() <= early.sum() <= 0.75 * hit.sum()          # neither never nor always
    for name, windows in SCHEDULES.items():
        ev = T.evaluated_counts(counts, kept, windows)
        print(f"eps {eps}: schedule {name} evaluates {int(ev.sum())} samples")
        assert (ev >= kept).all() and (ev <= counts).all() and (ev[~early] == counts[~early]).all()
        assert int(ev.sum()) == want["evaluated"][name]
    # at the default step nothing ever stops on this field: the reason for DELTA above
    assert (T.contributing_counts(s["sigma"], counts, 5e-3, stop) == counts).all()
    # no decision of the scene is near the threshold: every cum the rule tests is thousands of fp32 ulps from stop_tau,
    # so the GPU's exact counts do not hang on a last-bit difference in a density
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    gap = np.inf
    for r in np.nonzero(hit)[0]:
        tau = (s["sigma"][first[r]:first[r] + counts[r]] * np.float32(DELTA)).astype(np.float32)
        cum = np.float32(0)
        for k in range(min(int(kept[r]) + 1, int(counts[r]))):          # every cum the rule compared
            gap = min(gap, abs(float(cum) - float(stop)))
            cum = np.float32(cum + tau[k])
    print(f"eps {eps}: closest cum to stop_tau {gap:.3g} ({gap / float(np.spacing(stop)):.0f} ulps)")
    assert gap >= 100 * float(np.spacing(stop))
    # the error bound: the dropped weights sum to less than eps, colours lie in [0, 1] -> alpha and each colour sum move
    # by less than eps, a white-blended pixel by less than 3 eps
    full, a_full = _composite64(s, counts)
    cut, a_cut = _composite64(s, kept)
    print(f"eps {eps}: largest pixel change {np.abs(full - cut).max():.3g}, largest alpha change {np.abs(a_full - a_cut).max():.3g}")
    assert np.abs(a_full - a_cut).max() < eps
    assert np.abs(full - cut).max() < 3 * eps
    assert np.abs(full - cut).max() > 0.0
