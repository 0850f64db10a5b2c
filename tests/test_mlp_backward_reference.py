"""Pins tests/mlp_backward_reference.py (the float64 reference of the fused MLP backward kernels) on the CPU: it must
equal float64 torch.autograd of the same MLPs, with the density activation written as an autograd Function of the
reference's rule, and give the hand-derived clamp values."""
import math

import pytest
import torch

from oracle import fields as ofields
from quadraturefields_amd import synthetic
from tests import mlp_backward_reference as R


@pytest.fixture(autouse=True)
def _autograd_on():
    with torch.enable_grad():
        yield


class _ClampedExp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return torch.exp(x)

    @staticmethod
    def backward(ctx, g):
        x, = ctx.saved_tensors
        return g * torch.exp(torch.clamp(x, max=15.0))


def _inputs(n, seed):
    g = torch.Generator().manual_seed(seed)
    enc = (torch.rand(n, 32, generator=g) * 2 - 1) * 0.5
    dirs = torch.randn(n, 3, generator=g)
    dirs = dirs / dirs.norm(dim=-1, keepdim=True)
    sel = (torch.rand(n, generator=g) > 0.2).to(torch.uint8)
    d_rgb = torch.randn(n, 3, generator=g) * 0.1
    d_rgb[torch.rand(n, generator=g) < 0.1] = 0.0
    d_sigma = torch.randn(n, generator=g) * 0.01
    d_sigma[torch.rand(n, generator=g) < 0.1] = 0.0
    return enc, dirs, sel, d_rgb, d_sigma


def _check(ref, want):
    val, mag = ref
    want = want.detach().reshape(val.shape)
    assert torch.all(mag >= val.abs() * (1 - 1e-12))
    assert torch.allclose(val, want, rtol=1e-11, atol=1e-13 * float(mag.max()) + 1e-300)


def _leaf(t):
    return t.detach().double().clone().requires_grad_(True)


@pytest.mark.parametrize("n", [1, 17, 300])
def test_ngp_reference_equals_fp64_autograd(n):
    st = synthetic.seeded_ngp_state(10, 16)
    p = st["mlp_base.params"]
    base_w, head_w = p[:3072].contiguous(), st["mlp_head.params"]
    enc, dirs, sel, d_rgb, d_sigma = _inputs(n, n)
    # push a few points past the clamp: raw is 1-homogeneous in enc (no bias, ReLU)
    raw = R.ngp_raw(enc, base_w)
    for i, t in zip(range(0, n, 7), (20.0, -3.0, 15.5, 40.0)):
        if raw[i].abs() > 1e-3:
            enc[i] *= float((t + 1.0) / raw[i])
    ref = R.ngp_backward(enc, dirs, sel, d_rgb, d_sigma, base_w, head_w, chunk=128)

    (W1, W2), (V1, V2, V3) = R.ngp_unpack(base_w, head_w)
    W1, W2, V1, V2, V3, e = (_leaf(t) for t in (W1, W2, V1, V2, V3, enc))
    out = ofields.mlp_nobias(e, [W1, W2])
    density = _ClampedExp.apply(out[:, 0] - 1.0) * sel.double()
    u = (((dirs + 1.0) / 2.0) * 2.0 - 1.0).double()
    hin = torch.cat([ofields.sh4(u), out[:, 1:16], torch.ones_like(out[:, :1])], 1)
    rgb = torch.sigmoid(ofields.mlp_nobias(hin, [V1, V2, V3])[:, :3])
    ((rgb * d_rgb.double()).sum() + (density * d_sigma.double()).sum()).backward()
    _check(ref["d_enc"], e.grad)
    _check(ref["grad_base_w"], torch.cat([W1.grad.reshape(-1), W2.grad.reshape(-1)]))
    _check(ref["grad_head_w"], torch.cat([V1.grad.reshape(-1), V2.grad.reshape(-1), V3.grad.reshape(-1)]))
    assert ref["margin"].shape == (n,) and bool(torch.all(ref["margin"] >= 0))


@pytest.mark.parametrize("lobes,n", [(1, 40), (2, 17), (8, 200)])
def test_sg_reference_equals_fp64_autograd(lobes, n):
    st = synthetic.seeded_ngp_state(10, 16, sg_lobes=lobes)
    base_w = st["mlp_base.params"][:3072].contiguous()
    head = dict(zip(R.SG_HEAD_NAMES, (st[f"mlp_head.{k}"] for k in ("layers.0.weight", "layers.0.bias",
                                                                   "layers.1.weight", "layers.1.bias",
                                                                   "lout.weight", "lout.bias"))))
    enc, _, sel, _, d_sigma = _inputs(n, 100 + n)
    n_out = 3 + 7 * lobes
    d_feat = torch.randn(n, n_out + 5, generator=torch.Generator().manual_seed(lobes))
    d_feat[:, n_out:] = float("nan")                                   # padding columns are never read
    raw = R.ngp_raw(enc, base_w)
    if raw[0].abs() > 1e-3:
        enc[0] *= float(61.0 / raw[0])
    ref = R.sg_backward(enc, sel, d_feat, d_sigma, base_w, head, lobes, chunk=64)

    W1, W2, e = _leaf(base_w[:2048].reshape(64, 32)), _leaf(base_w[2048:].reshape(16, 64)), _leaf(enc)
    hd = {k: _leaf(v) for k, v in head.items()}
    out = ofields.mlp_nobias(e, [W1, W2])
    density = _ClampedExp.apply(out[:, 0] - 1.0) * sel.double()
    f = ofields.basic_decoder(out[:, 1:16], [(hd["w1"], hd["b1"]), (hd["w2"], hd["b2"]), (hd["wout"], hd["bout"])])
    ((f * d_feat[:, :n_out].double()).sum() + (density * d_sigma.double()).sum()).backward()
    _check(ref["d_enc"], e.grad)
    _check(ref["grad_base_w"], torch.cat([W1.grad.reshape(-1), W2.grad.reshape(-1)]))
    for k in R.SG_HEAD_NAMES:
        _check(ref[k], hd[k].grad)


@pytest.mark.parametrize("n", [1, 33])
def test_deform_reference_equals_fp64_autograd(n):
    st = synthetic.seeded_deform_state(16)
    ws = [st[f"decoder_field.{k}"] for k in ("layers.0.weight", "layers.0.bias", "layers.1.weight",
                                             "layers.1.bias", "lout.weight", "lout.bias")]
    g = torch.Generator().manual_seed(n)
    enc = (torch.rand(n, 32, generator=g) * 2 - 1) * 0.5
    x01 = torch.rand(n, 3, generator=g)
    d_out = torch.randn(n, generator=g)
    ref = R.deform_backward(enc, x01, d_out, *ws[:5], chunk=16)
    lw = [_leaf(t) for t in ws]
    e, x = _leaf(enc), _leaf(x01)
    y = ofields.basic_decoder(torch.cat([x, e], 1), [(lw[0], lw[1]), (lw[2], lw[3]), (lw[4], lw[5])])
    (y[:, 0] * d_out.double()).sum().backward()
    _check(ref["d_enc"], e.grad)
    _check(ref["d_x01"], x.grad)
    for k, t in zip(R.DEFORM_NAMES, lw):
        _check(ref[k], t.grad)


def test_density_clamp_hand_values():
    """d raw = d_sigma * selector * exp(min(raw - 1, 15)): the raw values are set through the density row alone."""
    base_w = torch.zeros(3072)
    base_w[0] = 1.0                           # hidden 0 = relu(enc[:, 0])
    base_w[2048] = 1.0                        # raw = hidden 0
    x = torch.tensor([15.5, 14.5, 15.5, 100.0, -3.0], dtype=torch.float64)
    enc = torch.zeros(5, 32)
    enc[:, 0] = torch.tensor([16.5, 15.5, 16.5, 101.0, 0.0])  # raw - 1 = x; the last point's hidden unit is off
    sel = torch.tensor([1, 1, 0, 1, 1], dtype=torch.uint8)
    g = torch.tensor([0.5, -2.0, 3.0, 1.0, 1.0])
    head_w = torch.zeros(7168)
    ref = R.ngp_backward(enc, torch.zeros(5, 3), sel, torch.zeros(5, 3), g, base_w, head_w)
    d_enc = ref["d_enc"][0][:, 0]
    want = [math.exp(15.0) * 0.5, math.exp(14.5) * -2.0, 0.0, math.exp(15.0), 0.0]
    for got, w in zip(d_enc.tolist(), want):
        assert got == pytest.approx(w, rel=1e-14, abs=0.0)
    assert R.dtrunc_exp(x).tolist() == pytest.approx([math.exp(15.0), math.exp(14.5), math.exp(15.0),
                                                      math.exp(15.0), math.exp(-3.0)], rel=1e-15)
    # the W2 density-row gradient is d raw * hidden 0, summed
    assert float(ref["grad_base_w"][0][2048]) == pytest.approx(
        math.exp(15.0) * 0.5 * 16.5 + math.exp(14.5) * -2.0 * 15.5 + math.exp(15.0) * 101.0, rel=1e-14)


def test_oracle_and_module_trunc_exp_follow_the_rule():
    """oracle.fields.trunc_exp and ngp.trunc_exp: exp forward, unclamped; exp(min(x, 15)) gradient, which stays
    finite where the forward overflows; the backward is differentiable (create_graph)."""
    from quadraturefields_amd.radiance_fields import ngp
    for fn in (ofields.trunc_exp, ngp.trunc_exp):
        x = torch.tensor([-3.0, 14.5, 15.5, 20.0, 100.0], requires_grad=True)
        y = fn(x)
        assert torch.equal(y.detach(), torch.exp(x.detach()))
        assert math.isinf(float(y[-1].detach()))
        (gx,) = torch.autograd.grad(y.sum(), x, create_graph=True)
        assert torch.equal(gx.detach(), torch.exp(torch.tensor([-3.0, 14.5, 15.0, 15.0, 15.0])))
        (ggx,) = torch.autograd.grad(gx.sum(), x)
        assert torch.equal(ggx, torch.exp(torch.tensor([-3.0, 14.5, 0.0, 0.0, 0.0])) * torch.tensor([1.0, 1, 0, 0, 0]))
