"""float64 reference of the three fused MLP backward kernels of csrc/mlp_train.hip.

``qf_ngp_mlp_backward``, ``qf_sg_mlp_backward`` and ``qf_deform_mlp_backward`` recompute an MLP's forward pass from
the fp32 grid encoding they are given and back-propagate upstream gradients to the encoding and the weights.  This
module does the same from the same fp32 inputs, in float64, chunked over points (on whatever device the inputs live),
with the weight-gradient sums in float64.  It therefore tests the MLP kernels alone, not the hash grid.

Next to every output it returns a magnitude ``M``: the same backward computed with every factor replaced by its
absolute value (|W|, |dz|, |a|) under the fp64 forward's ReLU masks, where |a| of an activation is the magnitude of
the sum that produced it (|W| |a_prev| + |b|, masked), which bounds a's own rounding.  An fp32 implementation with
k-term sums is then off by a few k * u * M per element (u = 2^-24).  Two factors are not products and get the first-order error of their
argument added, where M_x is x's forward magnitude propagated through every layer (|W| M_a + |b|):
  * d sigmoid(c) = s (1 - s): magnitude |d_rgb| s (1 - s) (1 + M_c);
  * the density derivative exp(min(raw - 1, 15)): magnitude |d_sigma| exp(min(raw - 1, 15)) (1 + M_raw) while the
    clamp is not engaged (the exponent carries raw's error), |d_sigma| exp(15) once it is (the derivative is constant).

Per point it also returns the smallest ReLU margin min |z| / M_z over every pre-activation, M_z = |W| |a| + |b| of
that layer with the fp64 activations themselves: where it is tiny fp32 and fp64 may take different ReLU branches, and that point's outputs are not
comparable to the bar.

The density rule is the reference's ``_TruncExp``: the forward density is exp(raw - 1) * selector, unclamped; its
derivative is d_sigma * selector * exp(min(raw - 1, 15)).

Flat layouts are those of include/qf_hip.h: NGP base_w = [W1 64x32 | W2 16x64] (3072), NGP head_w =
[V1 64x32 | V2 64x64 | V3 16x64] (7168), all row-major [out, in].  The NGP head's input is
[SH4(u) (16) | geo15 | 1] with u = ((dir + 1) / 2) * 2 - 1 evaluated in fp32; the SG decoder's input is geo15; the
deformation decoder's input is [x01 (3) | enc (32)].
"""
import torch

U = 2.0 ** -24
CLAMP = 15.0
CHUNK = 1 << 16


def dtrunc_exp(x):
    """Derivative of trunc_exp at x: exp(min(x, 15))."""
    return torch.exp(torch.clamp(x, max=CLAMP))


def _density_grad(raw, m_raw, sel, d_sigma):
    x = raw - 1.0
    e = dtrunc_exp(x)
    live = x < CLAMP + 2.0 ** -12 * m_raw              # the exponent still follows raw (or may, within raw's error)
    s = sel.double()
    return d_sigma * s * e, d_sigma.abs() * s * e * torch.where(live, 1.0 + m_raw, torch.ones_like(m_raw))


def ngp_unpack(base_w, head_w):
    """Flat NGP weights -> ([W1, W2], [V1, V2, V3]) as [out, in] views."""
    return ([base_w[:2048].reshape(64, 32), base_w[2048:3072].reshape(16, 64)],
            [head_w[:2048].reshape(64, 32), head_w[2048:6144].reshape(64, 64), head_w[6144:7168].reshape(16, 64)])


def sh4_with_magnitude(u):
    """Degree-4 real SH basis (tcnn's, as oracle.fields.sh4) of u [n,3] and its magnitude: every term's absolute value
    summed, so that M bounds the rounding of an fp32 evaluation."""
    x, y, z = u[:, 0], u[:, 1], u[:, 2]
    ax, ay, az = x.abs(), y.abs(), z.abs()
    x2, y2, z2 = x * x, y * y, z * z
    c = [0.28209479177387814, 0.48860251190291987, 1.0925484305920792, 0.94617469575755997, 0.31539156525251999,
         0.54627421529603959, 0.59004358992664352, 2.8906114426405538, 0.45704579946446572, 0.3731763325901154,
         1.4453057213202769]
    val = torch.stack([
        torch.full_like(x, c[0]), -c[1] * y, c[1] * z, -c[1] * x, c[2] * x * y, -c[2] * y * z, c[3] * z2 - c[4],
        -c[2] * x * z, c[5] * x2 - c[5] * y2, c[6] * y * (-3.0 * x2 + y2), c[7] * x * y * z,
        c[8] * y * (1.0 - 5.0 * z2), c[9] * z * (5.0 * z2 - 3.0), c[8] * x * (1.0 - 5.0 * z2), c[10] * z * (x2 - y2),
        c[6] * x * (-x2 + 3.0 * y2)], dim=-1)
    mag = torch.stack([
        torch.full_like(x, c[0]), c[1] * ay, c[1] * az, c[1] * ax, c[2] * ax * ay, c[2] * ay * az, c[3] * z2 + c[4],
        c[2] * ax * az, c[5] * x2 + c[5] * y2, c[6] * ay * (3.0 * x2 + y2), c[7] * ax * ay * az,
        c[8] * ay * (1.0 + 5.0 * z2), c[9] * az * (5.0 * z2 + 3.0), c[8] * ax * (1.0 + 5.0 * z2), c[10] * az * (x2 + y2),
        c[6] * ax * (x2 + 3.0 * y2)], dim=-1)
    return val, mag


class _Acc:
    """Per-point outputs written chunk by chunk, weight gradients summed in float64, each with its magnitude."""

    def __init__(self, n, device, point_cols, weight_shapes):
        z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=device)
        self.out = {k: (z(n, c), z(n, c)) for k, c in point_cols.items()}
        self.out.update({k: (z(*s), z(*s)) for k, s in weight_shapes.items()})
        self.margin = torch.full((n,), float("inf"), dtype=torch.float64, device=device)

    def rows(self, key, lo, hi, val, mag):
        self.out[key][0][lo:hi] = val
        self.out[key][1][lo:hi] = mag

    def add(self, key, val, mag):
        self.out[key][0].add_(val)
        self.out[key][1].add_(mag)

    def relu(self, lo, hi, z, m):
        mask = z > 0
        ratio = torch.where(m > 0, z.abs() / m, torch.full_like(m, float("inf")))
        self.margin[lo:hi] = torch.minimum(self.margin[lo:hi], ratio.min(dim=1).values)
        return mask

    def result(self):
        res = dict(self.out)
        res["margin"] = self.margin
        return res


def _outer(dz, mdz, a, ma):
    return dz.T @ a, mdz.T @ ma


def _base_forward(acc, lo, hi, e, W1, W2, aW1, aW2):
    """-> |e|, ReLU mask, h, M_h, out [.,16], M_out = |W2| |h| (for out as an activation), and out's magnitude
    propagated from the input (for the error of raw)."""
    me = e.abs()
    z1, mz1 = e @ W1.T, me @ aW1.T
    m1 = acc.relu(lo, hi, z1, mz1)
    h, mh = z1 * m1, mz1 * m1
    return me, m1, h, mh, h @ W2.T, h.abs() @ aW2.T, mh @ aW2.T


def _base_backward(acc, lo, hi, e, me, m1, h, mh, dout, mdout, W1, W2, aW1, aW2):
    dz1, mdz1 = (dout @ W2) * m1, (mdout @ aW2) * m1
    acc.rows("d_enc", lo, hi, dz1 @ W1, mdz1 @ aW1)
    g1, mg1 = _outer(dz1, mdz1, e, me)
    g2, mg2 = _outer(dout, mdout, h, mh)
    acc.add("grad_base_w", torch.cat([g1.reshape(-1), g2.reshape(-1)]), torch.cat([mg1.reshape(-1), mg2.reshape(-1)]))


def ngp_backward(enc, dirs, selector, d_rgb, d_sigma, base_w, head_w, chunk=CHUNK):
    """Reference of qf_ngp_mlp_backward.  Returns {name: (value, M)} for d_enc [n,32], grad_base_w [3072],
    grad_head_w [7168], plus "margin" [n]."""
    n, dev = enc.shape[0], enc.device
    (W1, W2), (V1, V2, V3) = ngp_unpack(base_w.double(), head_w.double())
    aW1, aW2, aV1, aV2, aV3 = (t.abs() for t in (W1, W2, V1, V2, V3))
    acc = _Acc(n, dev, {"d_enc": 32}, {"grad_base_w": (3072,), "grad_head_w": (7168,)})
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        e = enc[lo:hi].double()
        me, m1, h, mh, out, mout, pout = _base_forward(acc, lo, hi, e, W1, W2, aW1, aW2)
        u = (((dirs[lo:hi].float() + 1.0) / 2.0) * 2.0 - 1.0).double()
        sh, msh = sh4_with_magnitude(u)
        one = torch.ones_like(out[:, :1])
        hin = torch.cat([sh, out[:, 1:16], one], 1)
        mhin = torch.cat([msh, mout[:, 1:16], one], 1)
        phin = torch.cat([msh, pout[:, 1:16], one], 1)           # propagated, for M_c
        y1, my1, py1 = hin @ V1.T, mhin @ aV1.T, phin @ aV1.T
        m2 = acc.relu(lo, hi, y1, hin.abs() @ aV1.T)
        a1, ma1 = y1 * m2, my1 * m2
        y2, my2, py2 = a1 @ V2.T, ma1 @ aV2.T, (py1 * m2) @ aV2.T
        m3 = acc.relu(lo, hi, y2, a1.abs() @ aV2.T)
        a2, ma2 = y2 * m3, my2 * m3
        c, mc = a2 @ V3.T, (py2 * m3) @ aV3.T
        s = torch.sigmoid(c[:, :3])
        dc = torch.zeros_like(c)
        mdc = torch.zeros_like(c)
        dr = d_rgb[lo:hi].double()
        dc[:, :3] = dr * s * (1.0 - s)
        mdc[:, :3] = dr.abs() * s * (1.0 - s) * (1.0 + mc[:, :3])
        dy2, mdy2 = (dc @ V3) * m3, (mdc @ aV3) * m3
        dy1, mdy1 = (dy2 @ V2) * m2, (mdy2 @ aV2) * m2
        dhin, mdhin = dy1 @ V1, mdy1 @ aV1
        dout, mdout = torch.zeros_like(out), torch.zeros_like(out)
        dout[:, 1:16], mdout[:, 1:16] = dhin[:, 16:31], mdhin[:, 16:31]
        dout[:, 0], mdout[:, 0] = _density_grad(out[:, 0], pout[:, 0], selector[lo:hi], d_sigma[lo:hi].double())
        gv = [_outer(dy1, mdy1, hin, mhin), _outer(dy2, mdy2, a1, ma1), _outer(dc, mdc, a2, ma2)]
        acc.add("grad_head_w", torch.cat([g.reshape(-1) for g, _ in gv]), torch.cat([m.reshape(-1) for _, m in gv]))
        _base_backward(acc, lo, hi, e, me, m1, h, mh, dout, mdout, W1, W2, aW1, aW2)
    return acc.result()


SG_HEAD_NAMES = ("w1", "b1", "w2", "b2", "wout", "bout")


def sg_backward(enc, selector, d_features, d_sigma, base_w, head, n_lobes, chunk=CHUNK):
    """Reference of qf_sg_mlp_backward.  head: dict w1 [64,15], b1, w2 [64,64], b2, wout [3+7L,64], bout.
    d_features [n, >= 3+7L] (only the first 3+7L columns are read).  Returns d_enc, grad_base_w and the six head
    gradients (keys "w1" ... "bout", shapes of head), each (value, M), plus "margin"."""
    n, dev = enc.shape[0], enc.device
    n_out = 3 + 7 * n_lobes
    base = base_w.double()
    W1, W2 = base[:2048].reshape(64, 32), base[2048:3072].reshape(16, 64)
    D1, c1, D2, c2, Do = (head[k].double() for k in ("w1", "b1", "w2", "b2", "wout"))
    aW1, aW2, aD1, ac1, aD2, ac2, aDo = (t.abs() for t in (W1, W2, D1, c1, D2, c2, Do))
    acc = _Acc(n, dev, {"d_enc": 32}, dict(grad_base_w=(3072,), **{k: tuple(head[k].shape) for k in SG_HEAD_NAMES}))
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        e = enc[lo:hi].double()
        me, m1, h, mh, out, mout, pout = _base_forward(acc, lo, hi, e, W1, W2, aW1, aW2)
        geo, mgeo = out[:, 1:16], mout[:, 1:16]
        y1, my1 = geo @ D1.T + c1, mgeo @ aD1.T + ac1
        m2 = acc.relu(lo, hi, y1, geo.abs() @ aD1.T + ac1)
        a1, ma1 = y1 * m2, my1 * m2
        y2, my2 = a1 @ D2.T + c2, ma1 @ aD2.T + ac2
        m3 = acc.relu(lo, hi, y2, a1.abs() @ aD2.T + ac2)
        a2, ma2 = y2 * m3, my2 * m3
        df = d_features[lo:hi, :n_out].double()
        mdf = df.abs()
        dy2, mdy2 = (df @ Do) * m3, (mdf @ aDo) * m3
        dy1, mdy1 = (dy2 @ D2) * m2, (mdy2 @ aD2) * m2
        dout = torch.cat([torch.zeros_like(out[:, :1]), dy1 @ D1], 1)
        mdout = torch.cat([torch.zeros_like(out[:, :1]), mdy1 @ aD1], 1)
        dout[:, 0], mdout[:, 0] = _density_grad(out[:, 0], pout[:, 0], selector[lo:hi], d_sigma[lo:hi].double())
        acc.add("wout", *_outer(df, mdf, a2, ma2))
        acc.add("bout", df.sum(0), mdf.sum(0))
        acc.add("w2", *_outer(dy2, mdy2, a1, ma1))
        acc.add("b2", dy2.sum(0), mdy2.sum(0))
        acc.add("w1", *_outer(dy1, mdy1, geo, mgeo))
        acc.add("b1", dy1.sum(0), mdy1.sum(0))
        _base_backward(acc, lo, hi, e, me, m1, h, mh, dout, mdout, W1, W2, aW1, aW2)
    return acc.result()


DEFORM_NAMES = ("w1", "b1", "w2", "b2", "wout", "bout")


def deform_backward(enc, x01, d_out, w1, b1, w2, b2, wout, chunk=CHUNK):
    """Reference of qf_deform_mlp_backward: cat[x01, enc] -> 32 (ReLU) -> 32 (ReLU) -> 1, biases.  Returns d_enc
    [n,32], d_x01 [n,3] and the gradients "w1" [32,35], "b1" [32], "w2" [32,32], "b2" [32], "wout" [32], "bout" [1],
    each (value, M), plus "margin"."""
    n, dev = enc.shape[0], enc.device
    W1, c1, W2, c2 = (t.double() for t in (w1, b1, w2, b2))
    Wo = wout.double().reshape(1, 32)
    aW1, ac1, aW2, ac2, aWo = (t.abs() for t in (W1, c1, W2, c2, Wo))
    acc = _Acc(n, dev, {"d_enc": 32, "d_x01": 3},
               {"w1": (32, 35), "b1": (32,), "w2": (32, 32), "b2": (32,), "wout": (32,), "bout": (1,)})
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        inp = torch.cat([x01[lo:hi].double(), enc[lo:hi].double()], 1)
        minp = inp.abs()
        z1, mz1 = inp @ W1.T + c1, minp @ aW1.T + ac1
        m1 = acc.relu(lo, hi, z1, mz1)
        a1, ma1 = z1 * m1, mz1 * m1
        z2, mz2 = a1 @ W2.T + c2, ma1 @ aW2.T + ac2
        m2 = acc.relu(lo, hi, z2, a1.abs() @ aW2.T + ac2)
        a2, ma2 = z2 * m2, mz2 * m2
        do = d_out[lo:hi].double().reshape(-1, 1)
        mdo = do.abs()
        dz2, mdz2 = (do @ Wo) * m2, (mdo @ aWo) * m2
        dz1, mdz1 = (dz2 @ W2) * m1, (mdz2 @ aW2) * m1
        dinp, mdinp = dz1 @ W1, mdz1 @ aW1
        acc.rows("d_x01", lo, hi, dinp[:, :3], mdinp[:, :3])
        acc.rows("d_enc", lo, hi, dinp[:, 3:], mdinp[:, 3:])
        acc.add("w1", *_outer(dz1, mdz1, inp, minp))
        acc.add("b1", dz1.sum(0), mdz1.sum(0))
        acc.add("w2", *_outer(dz2, mdz2, a1, ma1))
        acc.add("b2", dz2.sum(0), mdz2.sum(0))
        gwo, mgwo = _outer(do, mdo, a2, ma2)
        acc.add("wout", gwo.reshape(-1), mgwo.reshape(-1))
        acc.add("bout", do.sum(0), mdo.sum(0))
    return acc.result()


def ngp_raw(enc, base_w):
    """The base MLP's density output raw [n] in float64 (the density is exp(raw - 1) * selector)."""
    e = enc.double()
    W1, W2 = base_w.double()[:2048].reshape(64, 32), base_w.double()[2048:3072].reshape(16, 64)
    return torch.relu(e @ W1.T) @ W2[0]


def err_ratio(got, ref, mag):
    """|got - ref| / (u M) element-wise, in float64; a non-finite result counts as inf, and where M = 0 only an exact
    match counts as 0."""
    got = got.double()
    err = (got - ref).abs()
    r = torch.where(mag > 0, err / (U * mag), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    return torch.where(torch.isfinite(got), r, torch.full_like(r, float("inf")))
