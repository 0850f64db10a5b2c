"""GPU: stage 2's fused training step (qf_field_quadrature_loss, ``Field.field_loss`` / ``value_and_grad``,
examples/train_field_synthetic.py) against the float64 restatement of tests/field_loss_reference.py.

The kernel is a persistent loop: a wave takes groups of 16 points, keeps its six weight-gradient tiles in registers and
the workgroup flushes them once.  One sweep of the launched grid covers S = 128 * (workgroups) points; the sizes below
straddle a group, a sweep and several sweeps.

Bars, with M the reference's magnitude of each element and u = 2^-24: per point (value, grad, d_enc) 2^-16 M; the five
weight gradients and the loss 2^-14 M; sparse probes 2^-16 M_probe.  Points with a branch margin below 2^-22 (ELU's
second derivative at z = 0, the two signs at p = 0 and r = 0) are replaced by spare points before the call, so a
full-batch sum is never compared across a branch flip.
"""
import importlib.util
import os

import pytest
import torch

from tests import field_loss_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PT_BAR = 2.0 ** -16 / R.U            # in units of u * M
W_BAR = 2.0 ** -14 / R.U
NAN = float("nan")
PAD = 16
STAGE2 = dict(scale=0.5, precision=16, L=16, min_res=16, output_dim=1, num_features=2, back_prop=False)


def _report(case, name, value):
    print(f"ERR_RATIO field_loss {case} {name} {value:.3g}")
    path = os.environ.get("QF_ERR_RATIO_LOG")
    if path:
        with open(path, "a") as f:
            f.write(f"field_loss {case} {name} {value:.6g}\n")


@pytest.fixture(scope="module")
def sweep(lib, device):
    """Points one sweep of the launched grid covers: qf_field_blocks workgroups (one per CU, a multiple of 8 from 64
    on) of 8 waves of 16 points."""
    cu = lib.qf_device_cu_count()
    assert cu > 0
    blocks = cu & ~7 if cu >= 64 else cu
    return 128 * blocks


_FIELDS = {}


def _field(device, table, nl="elu", hidden=16):
    """(Field on the device, oracle weights) of one of the two tables, built once."""
    from quadraturefields_amd.field import Field
    key = (table, nl, hidden)
    if key not in _FIELDS:
        cfg = R.TABLES[table]
        wts = R.seeded_weights(**cfg)
        f = Field(log2_T=cfg["log2_T"], max_res=cfg["max_res"], hidden_size=hidden, nl=nl, **STAGE2)
        if (nl, hidden) == ("elu", 16):
            f.load_state_dict(R.state_dict_of(wts), strict=False)
        _FIELDS[key] = (f.to(device), wts)
    return _FIELDS[key]


def _p(t, dtype=None):
    from quadraturefields_amd import _C
    return _C.ptr(t, dtype)


def call_entry(lib, f, inp, n=None, upstream=None, loss=True, value=True, grad=True, d_enc=True, grads=None,
               hidden=None, activation=None):
    """qf_field_quadrature_loss on device inputs; outputs NaN-filled with PAD spare rows.  Returns (status, dict)."""
    from quadraturefields_amd import _C
    dev = f.xyz_encoder.params.device
    n = inp.x.shape[0] if n is None else n
    out = {}
    if loss:
        out["loss"] = torch.full((1,), NAN, dtype=torch.float64, device=dev)
        out["ws"] = torch.empty((_C.FIELD_LOSS_WORKSPACE_BYTES,), dtype=torch.uint8, device=dev)
    for name, cols, want in (("value", 1, value), ("grad", 3, grad), ("d_enc", 32, d_enc)):
        if want:
            out[name] = torch.full((n + PAD, cols), NAN, dtype=torch.float32, device=dev)
    up = None if upstream is None else torch.tensor([upstream], dtype=torch.float32, device=dev)
    st = lib.qf_field_quadrature_loss(
        f.xyz_encoder.grid.desc, _p(f.xyz_encoder.params.detach()), float(f.scale),
        f.hidden_size if hidden is None else hidden, f.activation_code if activation is None else activation,
        *[_p(t) for t in f.decoder_arrays()], _p(inp.x), _p(inp.dirs), _p(inp.weights), _p(inp.weights_rev), n, _p(up),
        _p(out.get("loss")), _p(out.get("value")), _p(out.get("grad")), _p(out.get("d_enc")),
        *([_p(grads[k]) for k in R.NAMES] if grads is not None else [None] * 5),
        _p(out.get("ws")), _C.FIELD_LOSS_WORKSPACE_BYTES if loss else 0, _C.stream())
    torch.cuda.synchronize()
    return st, out


def check_points(case, name, got, ref, n, bar=PT_BAR):
    val, mag = ref
    assert bool(torch.isnan(got[n:]).all()), f"{case}: {name} wrote past row n"
    got = got[:n].cpu()
    assert bool(torch.isfinite(got).all()), f"{case}: {name} has non-finite rows < n"
    r = R.err_ratio(got.reshape(val.shape), val, mag)
    worst = float(r.max())
    _report(case, name, worst)
    assert worst <= bar, (case, name, worst, int(r.argmax()))


def check_weights(case, name, got, ref, g0=None, bar=W_BAR):
    val, mag = ref
    if g0 is not None:
        val, mag = val + g0.double(), mag + g0.double().abs()
    got = got.cpu()
    assert bool(torch.isfinite(got).all()), f"{case}: {name} not finite"
    r = R.err_ratio(got.reshape(val.shape), val, mag)
    worst = float(r.max())
    _report(case, name, worst)
    assert worst <= bar, (case, name, worst, int(r.argmax()))


def _prefill(ref, seed, device):
    """Random prefill of the gradient buffers at the gradients' own scale: the entry ACCUMULATES."""
    g = torch.Generator().manual_seed(seed)
    g0 = {k: (torch.randn(ref[k][1].shape, generator=g) * float(ref[k][1].mean())).float() for k in R.NAMES}
    return g0, {k: v.clone().to(device) for k, v in g0.items()}


SIZES = ["1", "15", "16", "17", "S-1", "S", "S+1", "3*S+5"]


# ------------------------------------------------------------------------------------------- 1. kernel against fp64
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("table", sorted(R.TABLES))
def test_kernel_vs_fp64(lib, device, sweep, table, size):
    from quadraturefields_amd import _C
    n = int(eval(size, {"S": sweep}))
    f, wts = _field(device, table)
    upstream = -1.75 if n % 2 else None
    inp, share = R.clean_inputs(n, seed=100 + n % 997, wts=wts)
    assert share <= 1e-3, share
    ref = R.reference(inp, wts, upstream=1.0 if upstream is None else upstream)
    g0, grads = _prefill(ref, n, device)
    st, out = call_entry(lib, f, inp.to(device), upstream=upstream, grads=grads)
    _C.check(st, "qf_field_quadrature_loss")
    case = f"{table}-{size}"
    for name in ("value", "grad", "d_enc"):
        check_points(case, name, out[name], ref[name], n)
    for name in R.NAMES:
        check_weights(case, name, grads[name], ref[name], g0[name])
    check_weights(case, "loss", out["loss"], ref["loss"])


# ------------------------------------------------------------------------------------------- 2. sparse probe
def _probe_points(n, sweep_pts):
    """~100 points: the first group, a group in a late sweep and the ragged last group (which holds point n - 1, where
    invalid lanes clamp to), plus a few neighbours."""
    W = sweep_pts // 16
    n_groups = (n + 15) // 16
    late = max(1, n_groups // W - 1) * W + W - 1
    groups = sorted({q for q in (0, 1, W - 1, W, late, n_groups - 1) if 0 <= q < n_groups})
    return torch.cat([torch.arange(16 * q, min(n, 16 * q + 16)) for q in groups]), groups


@pytest.mark.parametrize("table", sorted(R.TABLES))
def test_sparse_probes_catch_a_lost_or_doubled_group(lib, device, sweep, table):
    """Off the probes r = 0 exactly, so v = 0 there: the direction is a signed coordinate axis, p is then the gradient's
    component itself, and the weight is |p| as the kernel computes it (read back from a first call).  On the probes
    the weight is 2 |p|: r = |p|, exactly representable."""
    from quadraturefields_amd import _C
    n = 3 * sweep + 5
    f, wts = _field(device, table)
    pts, groups = _probe_points(n, sweep)
    assert len(pts) <= 128 and (n - 1) in pts.tolist() and len(groups) >= 5
    inp = R.seeded_inputs(n, seed=55)
    g = torch.Generator().manual_seed(56)
    axis = torch.randint(0, 3, (n,), generator=g)
    sign = torch.randint(0, 2, (n,), generator=g).float() * 2 - 1
    inp.dirs = torch.zeros(n, 3)
    inp.dirs[torch.arange(n), axis] = sign
    inp.weights_rev = torch.zeros(n)
    dev_inp = inp.to(device)
    st, first = call_entry(lib, f, dev_inp, loss=False, value=False)        # the training kernel's own gradient
    _C.check(st, "qf_field_quadrature_loss")
    p_abs = first["grad"][:n].cpu()[torch.arange(n), axis].abs()
    is_probe = torch.zeros(n, dtype=torch.bool)
    is_probe[pts] = True
    inp.weights = torch.where(is_probe, 2.0 * p_abs, p_abs)
    probes = inp.rows(pts)
    rp = R.reference(probes, wts, n_total=n)
    live = rp["margin"] >= R.MARGIN
    assert int(live.sum()) >= len(pts) - 2, int(live.sum())
    if not bool(live.all()):                                                # a probe on a branch point: switch it off
        inp.weights[pts[~live]] = p_abs[pts[~live]]
        keep = pts[live]
        rp = R.reference(inp.rows(keep), wts, n_total=n)
    else:
        keep = pts
    grads = {k: torch.zeros(rp[k][1].shape, dtype=torch.float32, device=device) for k in R.NAMES}
    st, out = call_entry(lib, f, inp.to(device), grads=grads)
    _C.check(st, "qf_field_quadrature_loss")
    case = f"{table}-probes"
    for name in R.NAMES:
        check_weights(case, name, grads[name], rp[name], bar=PT_BAR)
    off = torch.ones(n, dtype=torch.bool)
    off[keep] = False
    d_enc = out["d_enc"][:n].cpu()
    assert bool((d_enc[off] == 0).all())
    check_points(case, "d_enc", torch.cat([d_enc[keep], torch.full((1, 32), NAN)]), rp["d_enc"], len(keep))
    # the loss is the probes' alone: r = 0 everywhere else
    check_weights(case, "loss", out["loss"], rp["loss"], bar=PT_BAR)


# ------------------------------------------------------------------------------------------- 3. module level
def _l2(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def test_field_loss_module_matches_the_autograd_route(lib, device):
    from quadraturefields_amd import _C
    n = 4000
    f, wts = _field(device, "hashed")
    inp, _ = R.clean_inputs(n, seed=7, wts=wts)
    d = inp.to(device)
    params = dict(f.named_parameters())
    got = {}
    try:
        for fused in (True, False):
            f.fused_backward = fused
            for p in params.values():
                p.grad = None
            with torch.enable_grad():
                loss = f.field_loss(d.x.clone(), d.weights, d.weights_rev, d.dirs)
                assert loss.dim() == 0 and loss.dtype == torch.float32
                loss.backward()
            assert params["decoder_field.lout.bias"].grad is None
            got[fused] = (loss.detach().clone(), {k: p.grad.detach().clone() for k, p in params.items() if p.grad is not None})
        f.fused_backward = True
        assert abs(float(got[True][0]) - float(got[False][0])) <= 1e-6 * abs(float(got[False][0]))
        assert set(got[True][1]) == set(got[False][1]) and len(got[True][1]) == 6
        for k, v in got[True][1].items():
            rel = _l2(v, got[False][1][k])
            print(f"field_loss module {k}: L2 {rel:.3g}")
            assert rel <= 2e-3, (k, rel)
        # an upstream factor scales every gradient
        for p in params.values():
            p.grad = None
        with torch.enable_grad():
            loss3 = f.field_loss(d.x, d.weights, d.weights_rev, d.dirs)
            (3 * loss3).backward()
        assert torch.equal(loss3.detach(), got[True][0])                     # bit-identical run to run
        for k, v in got[True][1].items():
            assert _l2(params[k].grad, 3 * v) <= 1e-5, k
        assert params["decoder_field.lout.bias"].grad is None
        # no autograd: the loss alone
        assert torch.equal(f.field_loss(d.x, d.weights, d.weights_rev, d.dirs), got[True][0])
    finally:
        f.fused_backward = True
        for p in params.values():
            p.grad = None
    # value_and_grad against fp64
    ref = R.reference(inp, wts)
    value, grad = f.value_and_grad(d.x)
    assert value.shape == (n, 1) and grad.shape == (n, 3)
    pad = lambda t: torch.cat([t, torch.full((1, t.shape[1]), NAN, device=t.device)])
    check_points("module", "value", pad(value), ref["value"], n)
    check_points("module", "grad", pad(grad), ref["grad"], n)
    # |grad| rounded to fp16 against qf_field_grid_extract's point list
    gn = torch.empty((n,), dtype=torch.float16, device=device)
    val = torch.empty((n,), dtype=torch.float32, device=device)
    name, table = f.extract_entry()
    _C.check(getattr(lib, name)(f.xyz_encoder.grid.desc, _C.ptr(table), float(f.scale), f.hidden_size, f.activation_code,
                                *[_C.ptr(t) for t in f.decoder_arrays()], None, 0, 0, 0, 1, _C.ptr(d.x), n, None,
                                _C.ptr(val), _C.ptr(gn), _C.stream()), name)
    mine = grad.norm(dim=1).clamp(max=65504.0).half()
    ulps = (mine.view(torch.int16).int() - gn.view(torch.int16).int()).abs()
    share = float((ulps <= 1).float().mean())
    print(f"field_loss module grad_norm within one fp16 ulp of qf_field_grid_extract: {share:.5f}")
    # both are fp32 norms of the same three numbers up to rounding: their fp16 roundings are neighbours at worst
    assert share == 1.0, share


# ------------------------------------------------------------------------------------------- 4. refusals
def test_unsupported_configurations(lib, device):
    f, wts = _field(device, "hashed")
    inp = R.seeded_inputs(64, seed=9).to(device)
    for kw in (dict(hidden=32), dict(activation=0)):
        st, out = call_entry(lib, f, inp, **kw)
        assert st == -3, (kw, st)                                            # QF_ERR_UNSUPPORTED, before any launch
        assert bool(torch.isnan(out["loss"]).all()) and bool(torch.isnan(out["value"]).all())
    # some but not all of the five gradients
    partial = {k: (None if k == "b2" else torch.zeros(16 * 35, device=device)) for k in R.NAMES}
    st, out = call_entry(lib, f, inp, grads=partial)
    assert st == -1 and bool(torch.isnan(out["value"]).all())                # QF_ERR_INVALID_ARGUMENT
    # n = 0: no launch, the loss is torch's mean of nothing, nothing else is written
    st, out = call_entry(lib, f, inp, n=0)
    assert st == 0 and bool(torch.isnan(out["loss"]).all()) and bool(torch.isnan(out["value"]).all())
    # another configuration still gets the autograd value
    g, _ = _field(device, "hashed", nl="relu", hidden=32)
    x = inp.x.clone()
    with torch.enable_grad():
        got = g.field_loss(x, inp.weights, inp.weights_rev, inp.dirs)
        want = g.compute_field_loss(inp.weights, inp.weights_rev, g(inp.x.clone())[1], inp.dirs)
    assert torch.equal(got.detach(), want.detach()) and got.requires_grad
    empty = torch.zeros((0, 3), device=device)
    assert bool(torch.isnan(f.field_loss(empty, empty[:, 0], empty[:, 0], empty)))


# ------------------------------------------------------------------------------------------- 5. the loop
def test_training_loop_example(device, tmp_path):
    from quadraturefields_amd.field import Field
    spec = importlib.util.spec_from_file_location("train_field_synthetic", os.path.join(ROOT, "examples", "train_field_synthetic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = tmp_path / "stage2.pth"
    with torch.enable_grad():
        res = mod.main(["--steps", "40", "--grid_resolution", "32", "--size", "48", "--views", "4", "--log2_T", "14",
                        "--rays", "512", "--target_samples", "16384", "--step", "0.01", "--out", str(out)])
    assert res["steps"] >= 35 and res["falling"] is True, res
    ckpt = torch.load(out, map_location="cpu")
    assert set(ckpt) == {"estimator", "model"}
    f = Field(log2_T=14, max_res=512, hidden_size=16, nl="elu", **STAGE2)
    f.load_state_dict(ckpt["model"], strict=True)
