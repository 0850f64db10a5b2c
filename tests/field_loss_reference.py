"""float64 restatement of stage 2's training step (train_field.py:346-350 over field.py:186-259), for the tests of
``qf_field_quadrature_loss``.

From the same fp32 inputs as the kernel: x01 = (x + s) / (s + s) in fp32, the 32 grid features by
``oracle.fields.hash_encode`` in fp32 (as tests/grid_extract_reference.py), everything after that in float64 through
torch's double autograd -- the field, its gradient to the three x01 columns with ``create_graph=True`` (the encoder
sees x01.detach()), the loss mean | max(w, w_rev) - |grad f . d/|d|| | and its gradients to the five weight arrays and
to the grid features (``d_enc``).  ``lout.bias`` does not enter the loss.

``closed_form`` writes the same backward out by hand (the formulas the kernel implements) and, with every factor
replaced by its absolute value, gives the magnitude ``M`` next to each output in the sense of
tests/mlp_backward_reference.py: an fp32 implementation with k-term sums is off by a few k u M per element.  The two
ELU derivative factors phi'(z) = phi''(z) = exp(z) (z <= 0) are not products: their magnitude carries the error of the
exponent, exp(z) (1 + M_z), as that module does for its exp.  An activation's magnitude is phi'(z) M_z + |phi(z)|.

Per point it also returns the smallest margin over the 34 branch quantities: |z| / M_z of the 32 pre-activations (phi''
jumps at 0), |p| / M_p and |r| / M_r (the two signs).  Where it is tiny, fp32 and fp64 may take different branches and
that point's outputs are not comparable to the bar.
"""
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from oracle import fields as ofields

U = 2.0 ** -24
NAMES = ("w1", "b1", "w2", "b2", "wout")


@dataclass
class Inputs:
    x: torch.Tensor          # [n,3] fp32, in [-scale, scale]
    dirs: torch.Tensor       # [n,3] fp32, not normalised
    weights: torch.Tensor    # [n] fp32
    weights_rev: torch.Tensor

    def rows(self, idx):
        return Inputs(self.x[idx], self.dirs[idx], self.weights[idx], self.weights_rev[idx])

    def to(self, device):
        return Inputs(*(t.to(device).contiguous() for t in (self.x, self.dirs, self.weights, self.weights_rev)))


def seeded_weights(log2_T, max_res, seed=7, table_amp=0.5, scale=0.5, L=16, min_res=16) -> ofields.DeformWeights:
    """A stage-2 field (elu, hidden 16) with seeded weights at the scale of a trained one."""
    g = torch.Generator().manual_seed(seed)
    lv = ofields.grid_levels(L, log2_T, min_res, ofields.field_per_level_scale(max_res, scale, min_res, L))

    def xavier(o, i, gain):
        return (torch.rand(o, i, generator=g) * 2 - 1) * gain * (6.0 / (i + o)) ** 0.5

    table = (torch.rand(lv.n_entries, 2, generator=g) * 2 - 1) * table_amp
    layers = [(xavier(16, 35, 1.5), (torch.rand(16, generator=g) - 0.5) * 0.4),
              (xavier(16, 16, 1.5), (torch.rand(16, generator=g) - 0.5) * 0.4),
              (xavier(1, 16, 2.0), (torch.rand(1, generator=g) - 0.5) * 0.2)]
    return ofields.DeformWeights(scale=scale, levels=lv, table=table, layers=layers)


def state_dict_of(wts: ofields.DeformWeights):
    """The ``Field`` state-dict entries of ``wts``."""
    (w1, b1), (w2, b2), (wo, bo) = wts.layers
    return {"xyz_encoder.params": wts.table.reshape(-1), "decoder_field.layers.0.weight": w1,
            "decoder_field.layers.0.bias": b1, "decoder_field.layers.1.weight": w2, "decoder_field.layers.1.bias": b2,
            "decoder_field.lout.weight": wo, "decoder_field.lout.bias": bo}


def seeded_inputs(n, seed, half=0.49, t_scale=1.0) -> Inputs:
    """Points inside [-half, half]^3, unnormalised directions, weights with w = w_rev = 0 on about 20 % of the points
    (empty space)."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(n, 3, generator=g) * 2 - 1) * half
    dirs = torch.randn(n, 3, generator=g) * (0.25 + 3.0 * torch.rand(n, 1, generator=g))
    w = torch.rand(n, generator=g) * t_scale
    w_rev = torch.rand(n, generator=g) * t_scale * 0.7
    empty = torch.rand(n, generator=g) < 0.2
    w[empty] = 0.0
    w_rev[empty] = 0.0
    return Inputs(x, dirs, w, w_rev)


def encode(x, wts):
    """(x01 [n,3], grid features [n,32]) in fp32, as the kernel forms them."""
    s = torch.tensor(wts.scale, dtype=torch.float32)
    x01 = ((x.float().cpu() + s) / (s + s)).float()
    return x01, ofields.hash_encode(x01, wts.table, wts.levels)


def _elu_parts(z):
    d = torch.where(z > 0, torch.ones_like(z), torch.exp(z))        # phi'
    dd = torch.where(z > 0, torch.zeros_like(z), torch.exp(z))      # phi''
    return F.elu(z), d, dd


def closed_form(inp: Inputs, wts, upstream=1.0, n_total=None, enc=None):
    """The step by hand in float64.  Returns {name: (value, M)} for "loss" (0-d), "value" [n], "grad" [n,3], "d_enc"
    [n,32] and the five weight gradients, plus "margin" [n], "p" and "r" [n].  ``n_total``: the n of the mean when
    ``inp`` is a subset of a batch (the probes)."""
    x01, h = encode(inp.x, wts) if enc is None else enc
    n = x01.shape[0]
    n_mean = n if n_total is None else n_total
    two_s = 2.0 * wts.scale
    (W1, b1), (W2, b2), (wo, bo) = [(w.double(), b.double()) for w, b in wts.layers]
    wo = wo.reshape(-1)
    aW1, ab1, aW2, ab2, awo, abo = (t.abs() for t in (W1, b1, W2, b2, wo, bo))
    u = torch.cat([x01.double(), h.double()], 1)
    mu = u.abs()
    z1, mz1 = u @ W1.T + b1, mu @ aW1.T + ab1
    a1, d1, dd1 = _elu_parts(z1)
    md1 = torch.where(z1 > 0, torch.ones_like(z1), d1 * (1.0 + mz1))
    mdd1 = torch.where(z1 > 0, torch.zeros_like(z1), d1 * (1.0 + mz1))
    ma1 = d1 * mz1 + a1.abs()
    z2, mz2 = a1 @ W2.T + b2, ma1 @ aW2.T + ab2
    a2, d2, dd2 = _elu_parts(z2)
    md2 = torch.where(z2 > 0, torch.ones_like(z2), d2 * (1.0 + mz2))
    mdd2 = torch.where(z2 > 0, torch.zeros_like(z2), d2 * (1.0 + mz2))
    ma2 = d2 * mz2 + a2.abs()
    f, mf = a2 @ wo + bo, ma2 @ awo + abo
    # gradient of the scalar output
    delta2, mdelta2 = wo * d2, awo * md2
    c1, mc1 = delta2 @ W2, mdelta2 @ aW2
    delta1, mdelta1 = c1 * d1, mc1 * md1
    g, mg = delta1 @ W1[:, :3] / two_s, mdelta1 @ aW1[:, :3] / two_s
    # loss
    dd = inp.dirs.double().cpu()
    dhat = dd / dd.norm(dim=1, keepdim=True)
    p, mp = (g * dhat).sum(1), (mg * dhat.abs()).sum(1)
    t = torch.maximum(inp.weights.double().cpu(), inp.weights_rev.double().cpu())
    r, mr = t - p.abs(), t.abs() + mp
    loss, mloss = r.abs().sum() / n_mean, mr.sum() / n_mean
    # backward
    coef = -torch.sign(r) * torch.sign(p) * upstream / (two_s * n_mean)
    v, mv = coef[:, None] * dhat, coef.abs()[:, None] * dhat.abs()
    q1, mq1 = v @ W1[:, :3].T, mv @ aW1[:, :3].T
    e1, me1 = q1 * d1, mq1 * md1
    q2, mq2 = e1 @ W2.T, me1 @ aW2.T
    gwo, mgwo = q2 * d2, mq2 * md2
    y2, my2 = q2 * wo * dd2, mq2 * awo * mdd2
    y1, my1 = q1 * c1 * dd1 + (y2 @ W2) * d1, mq1 * mc1 * mdd1 + (my2 @ aW2) * md1
    gW1, mgW1 = y1.T @ u, my1.T @ mu
    gW1[:, :3] += delta1.T @ v
    mgW1[:, :3] += mdelta1.T @ mv
    out = {"loss": (loss, mloss), "value": (f, mf), "grad": (g, mg),
           "d_enc": (y1 @ W1[:, 3:], my1 @ aW1[:, 3:]),
           "w1": (gW1, mgW1), "b1": (y1.sum(0), my1.sum(0)),
           "w2": (delta2.T @ e1 + y2.T @ a1, mdelta2.T @ me1 + my2.T @ ma1), "b2": (y2.sum(0), my2.sum(0)),
           "wout": (gwo.sum(0)[None], mgwo.sum(0)[None])}
    margin = torch.minimum((z1.abs() / mz1).min(1).values, (z2.abs() / mz2).min(1).values)
    margin = torch.minimum(margin, torch.minimum(p.abs() / mp, r.abs() / mr))
    out.update(margin=margin, p=p, r=r)
    return out


def autograd_step(inp: Inputs, wts, upstream=1.0, n_total=None, enc=None):
    """The same step through torch double autograd (create_graph=True).  Returns {name: value} for "loss", "value",
    "grad", "d_enc", the five weight gradients and "bout" (None: lout.bias gets no gradient)."""
    x01, h = encode(inp.x, wts) if enc is None else enc
    n = x01.shape[0]
    n_mean = n if n_total is None else n_total
    two_s = 2.0 * wts.scale
    with torch.enable_grad():
        params = [t.double().clone().requires_grad_(True) for w, b in wts.layers for t in (w, b)]
        W1, b1, W2, b2, wo, bo = params
        xd = x01.double().requires_grad_(True)
        hd = h.double().requires_grad_(True)
        z = torch.cat([xd, hd], 1)
        z = F.elu(F.linear(z, W1, b1))
        z = F.elu(F.linear(z, W2, b2))
        f = F.linear(z, wo, bo)[:, 0]
        g01, = torch.autograd.grad(f.sum(), [xd], create_graph=True)
        g = g01 / two_s
        dd = inp.dirs.double().cpu()
        dhat = dd / dd.norm(dim=1, keepdim=True)
        t = torch.maximum(inp.weights.double().cpu(), inp.weights_rev.double().cpu())
        loss = torch.abs(t - torch.abs((g * dhat).sum(1))).sum() / n_mean
        grads = torch.autograd.grad(loss * upstream, [W1, b1, W2, b2, wo, bo, hd], allow_unused=True)
    out = dict(zip(NAMES + ("bout", "d_enc"), grads))
    out.update(loss=loss.detach(), value=f.detach(), grad=g.detach())
    return out


def reference(inp: Inputs, wts, upstream=1.0, n_total=None):
    """What the tests compare against: the autograd values with the closed form's magnitudes, {name: (value, M)}, plus
    "margin"."""
    enc = encode(inp.x, wts)
    cf = closed_form(inp, wts, upstream, n_total, enc)
    ag = autograd_step(inp, wts, upstream, n_total, enc)
    out = {k: (ag[k].reshape(cf[k][0].shape), cf[k][1]) for k in ("loss", "value", "grad", "d_enc") + NAMES}
    out["margin"] = cf["margin"]
    out["closed_form"] = cf
    return out


def err_ratio(got, ref, mag):
    """|got - ref| / (u M) element-wise in float64 (tests/mlp_backward_reference.err_ratio)."""
    got = got.double().cpu()
    err = (got - ref).abs()
    r = torch.where(mag > 0, err / (U * mag), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    return torch.where(torch.isfinite(got), r, torch.full_like(r, float("inf")))


# ---- the input sets of tests/test_gpu_field_loss.py, shared with the host test that checks their margins
TABLES = {"hashed": dict(log2_T=14, max_res=512), "dense": dict(log2_T=19, max_res=128)}
MARGIN = 2.0 ** -22
SPARE = 64


def clean_inputs(n, seed, wts, t_scale=1.0):
    """``seeded_inputs`` with every point whose margin is below MARGIN replaced by a spare one (drawn with the batch).
    Returns (inputs of n points, share of flagged points among the first n drawn)."""
    inp = seeded_inputs(n + SPARE, seed, t_scale=t_scale)
    margin = closed_form(inp, wts)["margin"]
    bad = margin < MARGIN
    idx = torch.arange(n)
    flagged = torch.nonzero(bad[:n]).flatten()
    spare = n + torch.nonzero(~bad[n:]).flatten()
    assert len(spare) >= len(flagged), (len(spare), len(flagged))
    idx[flagged] = spare[:len(flagged)]
    return inp.rows(idx), len(flagged) / n
