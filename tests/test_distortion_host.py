"""CPU: the contract of the distortion loss (the ordered sum against the Mip-NeRF-360 definition, in fp64), the
closed-form stage-1 regularisers, the drop-in module and the refusal of host tensors."""
import os
import subprocess
import sys
from collections import namedtuple

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import distortion_reference as dref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [0, 1, 2, 63, 64, 65, 0, 0, 130, 700, 3, 1]


def _rays(seed=0, lengths=LENGTHS):
    rng = np.random.default_rng(seed)
    ray_id = np.repeat(np.arange(len(lengths)), lengths)
    w, m, d = [], [], []
    for c in lengths:
        step = 5e-3 * rng.uniform(0.5, 1.5, size=c)
        t = rng.uniform(2.0, 6.0) + np.cumsum(step)
        tau = rng.exponential(1.0, size=c) * step * 20.0
        trans = np.exp(-(np.cumsum(tau) - tau))
        w.append(trans * (1.0 - np.exp(-tau)))
        m.append(t - 0.5 * step)
        d.append(step)
    return np.concatenate(w), np.concatenate(m), np.concatenate(d), ray_id, len(lengths)


def test_ordered_equals_pairwise_on_sorted_positions():
    w, m, d, ray_id, n_rays = _rays()
    lp, gp = dref.pairwise(w, m, d, ray_id, n_rays)
    lo, go = dref.ordered(w, m, d, ray_id, n_rays)
    assert lp > 0
    assert abs(lo - lp) <= 1e-12 * abs(lp)
    assert np.max(np.abs(go - gp)) <= 1e-12 * np.max(np.abs(gp))


def test_ordered_differs_from_pairwise_on_v_shaped_positions():
    """|p . d| along a ray that passes the origin falls and rises again: the ordered sum (what the package and the
    kernel compute) is then NOT the absolute-value definition."""
    w, m, d, ray_id, n_rays = _rays(1, [40, 7])
    m = np.abs(m - np.repeat([m[:40].mean(), m[40:].mean()], [40, 7]))        # V-shaped within each ray
    lp, gp = dref.pairwise(w, m, d, ray_id, n_rays)
    lo, go = dref.ordered(w, m, d, ray_id, n_rays)
    assert abs(lo - lp) > 1e-3 * abs(lp)
    assert np.max(np.abs(go - gp)) > 1e-3 * np.max(np.abs(gp))


def test_regulariser_closed_forms():
    from quadraturefields_amd import losses
    Rays = namedtuple("Rays", ("origins", "viewdirs"))
    g = torch.Generator().manual_seed(5)
    n_rays, n = 5, 23
    acc = torch.rand(n_rays, 1, generator=g)
    extras = {"weights": torch.rand(n, generator=g) * 0.3, "sigmas": torch.rand(n, generator=g) * 40.0}
    rays = Rays(origins=torch.zeros(n_rays, 3), viewdirs=torch.nn.functional.normalize(torch.randn(n_rays, 3, generator=g), dim=-1))
    o_lambda, c_lambda = 1e-3, 1e-4
    a, w, s = acc.double().squeeze(), extras["weights"].double(), extras["sigmas"].double()
    occ = (o_lambda * (-a * torch.log(a + 1e-10))).mean()
    cauchy = c_lambda * torch.log(1 + s ** 2).mean()
    lol_arg = torch.exp(-w) + torch.exp(-torch.abs(1 - w))
    # (fp64 value, error scale).  The bar is the fp32 evaluation's own rounding, not a measured figure: a term
    # c x log(y) carries at most two roundings in y (each moves log(y) by 2^-24 ABSOLUTE, whatever its size), one in
    # the log, two in the products and at most ceil(log2(23)) = 5 in torch's pairwise mean -- fewer than 16 roundings of
    # 2^-24 relative to  mean |c x| (1 + |log y|).
    occ_scale = (o_lambda * a * (1 + torch.log(a + 1e-10).abs())).mean()
    cauchy_scale = (c_lambda * (1 + torch.log(1 + s ** 2))).mean()
    expected = {
        "occ": (occ, occ_scale),
        "entropy": ((o_lambda * (-w * torch.log(w + 1e-7))).mean(), (o_lambda * w * (1 + torch.log(w + 1e-7).abs())).mean()),
        "cauchy": (cauchy, cauchy_scale),
        "both": (occ + cauchy, occ_scale + cauchy_scale),
        "lol": ((o_lambda * torch.log(lol_arg)).mean(), (o_lambda * (1 + torch.log(lol_arg).abs())).mean()),
        "none": (torch.zeros((), dtype=torch.float64), torch.zeros((), dtype=torch.float64)),
    }
    for reg_type, (want, scale) in expected.items():
        got = losses.regulariser(reg_type, acc=acc, extras=extras, rays=rays, o_lambda=o_lambda, c_lambda=c_lambda,
                                 render_step_size=5e-3)
        assert got.shape == () and got.dtype == torch.float32, reg_type
        assert abs(float(got) - float(want)) <= 16 * 2.0 ** -24 * float(scale), (reg_type, float(got), float(want))
    with pytest.raises(ValueError):
        losses.regulariser("l2", acc=acc, extras=extras, rays=rays, o_lambda=o_lambda, c_lambda=c_lambda,
                           render_step_size=5e-3)


def test_dropin_module_exports_the_upstream_names():
    """A fresh interpreter with the drop-in directory first on the path: the import line of train_finetune.py:33."""
    code = ("from torch_efficient_distloss import eff_distloss, eff_distloss_native, flatten_eff_distloss\n"
            "import quadraturefields_amd.losses as l\n"
            "assert flatten_eff_distloss is l.flatten_eff_distloss and eff_distloss is l.eff_distloss\n"
            "assert eff_distloss_native is l.eff_distloss\n")
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "quadraturefields_amd", "dropin"), ROOT])
    subprocess.run([sys.executable, "-c", code], check=True, env=env, cwd=ROOT)


def test_host_tensors_and_bad_arguments_are_refused(lib):
    from quadraturefields_amd import losses
    w, m = torch.rand(6), torch.rand(6)
    ids = torch.tensor([0, 0, 1, 1, 1, 2])
    with pytest.raises(RuntimeError):
        losses.flatten_eff_distloss(w, m, 0.01, ids)
    with pytest.raises(RuntimeError):
        losses.eff_distloss(w.reshape(2, 3), m.reshape(2, 3), 0.01)
    with pytest.raises(RuntimeError):
        losses.ray_distortion(w, m, m + 0.01, ids)
    with pytest.raises(TypeError):
        losses.flatten_eff_distloss(w.double(), m, 0.01, ids)
    with pytest.raises(TypeError):
        losses.flatten_eff_distloss(w, m, 0.01, ids.int())
    with pytest.raises(TypeError):
        losses.flatten_eff_distloss(w, m, "0.01", ids)
    with pytest.raises(TypeError):
        losses.flatten_eff_distloss(w.numpy(), m, 0.01, ids)
    with pytest.raises(ValueError):
        losses.eff_distloss(w.reshape(2, 3), m.reshape(3, 2), 0.01)
    with pytest.raises(ValueError):
        losses.eff_distloss(w.reshape(2, 3), m.reshape(2, 3), torch.rand(6))


def test_entry_point_is_declared_bound_and_indexed(lib):
    from quadraturefields_amd import _C
    assert "qf_distortion_loss" in _C.EXPORTED_SYMBOLS and lib.qf_distortion_loss is not None
    header = open(os.path.join(ROOT, "include", "qf_hip.h")).read()
    assert "int qf_distortion_loss(" in header
    assert f"#define QF_DISTORTION_WORKSPACE_BYTES {_C.DISTORTION_WORKSPACE_BYTES}" in header
    assert "`qf_distortion_loss`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert ("distortion.hip", []) in __import__("quadraturefields_amd.build", fromlist=["SOURCES"]).SOURCES
