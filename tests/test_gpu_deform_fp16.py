"""GPU: the deformation field's fp16 mode (``Field.compute_dtype = "fp16"``: qf_deform_field_forward_f16,
deform_kernel<DeformRowF16>) against the fp16 reference of tests/fp16_deform_reference.py, which rounds the same
quantities to fp16 at the same places (the table; the 32 blended encoding outputs), and on every inference route.

Bars: at least 99 % of the points within 2e-5 + 2e-5 |x| -- the fp32 kernel's own bar against the fp32 oracle
(test_gpu_fields.py) -- and every point within 5e-4.  The kernel blends in fp32 exactly as the reference does, but in
another summation order (fmaf chain against torch's mul + sum), so a blended feature that lands within an fp32 ulp of an
fp16 rounding midpoint can round the other way: one feature one fp16 ulp off, about 32 x 2^-13 = 0.4 % of the points.
Those points carry the maximum; the fraction bar keeps them from hiding a wrong mode.  The fp32 kernel fails the
fraction bar on the same points, so the tests cannot pass without the fp16 route.  Measured on MI355X (fraction within
the bar, maximum): see each test's docstring.  The flips are rarer than the estimate (0.04-0.2 % of the points rather
than 0.4 %): the kernel's fp32 blend equals the reference's bit for bit on most features, so only the features whose
blends differ by an ulp can round the other way.
"""
import dataclasses

import pytest
import torch

from oracle import fields as ofields
from tests import fp16_deform_reference as ref16d
from tests import helpers

pytestmark = pytest.mark.gpu

FRAC_MIN = 0.99
MAX_TOL = 5e-4
QF_OK, QF_ERR_INVALID_ARGUMENT, QF_ERR_UNSUPPORTED = 0, -1, -3      # include/qf_hip.h


def _field(device, log2_T=16):
    from quadraturefields_amd import synthetic
    from quadraturefields_amd.field import Field
    torch.manual_seed(0)
    f = Field(scale=1.5, precision=16, log2_T=log2_T, L=16, max_res=512, min_res=16, output_dim=1, hidden_size=32,
              num_features=2, back_prop=False, nl="relu")
    f.load_state_dict(synthetic.seeded_deform_state(f.xyz_encoder.grid.n_params), strict=False)
    wts = helpers.oracle_deform_weights(f)
    return f.to(device), wts


def _stats(got, want):
    """(fraction of points within 2e-5 + 2e-5 |want|, max |got - want|)."""
    a, b = got.detach().cpu().double().reshape(-1), want.detach().cpu().double().reshape(-1)
    err = (a - b).abs()
    return float((err <= 2e-5 + 2e-5 * b.abs()).double().mean()), float(err.max())


def _check_fp16(f, x, want16, label):
    """fp16 mode passes both bars; the fp32 mode on the same points fails the fraction bar."""
    f.compute_dtype = "fp16"
    frac, mx = _stats(f(x, return_grad=False)[0], want16)
    f.compute_dtype = "fp32"
    frac32, _ = _stats(f(x, return_grad=False)[0], want16)
    print(f"{label}: fp16 within bar {frac:.5f}, max {mx:.3e}; fp32 kernel within bar {frac32:.5f}")
    assert frac >= FRAC_MIN and mx <= MAX_TOL, (label, frac, mx)
    assert frac32 < FRAC_MIN, (label, frac32)


def test_deform_fp16_matches_the_fp16_reference(device):
    """T = 2^16, 3 001 and 70 001 points (the second is enough 16-point groups for the XCD-contiguous mapping).
    Measured: 99.967 % / 99.960 % of the points within the bar, maximum 2.8e-4 / 3.0e-4; the fp32 kernel 20.9 % / 21.5 %."""
    f, wts = _field(device)
    for n, seed in ((3001, 9), (70001, 10)):
        x, _ = helpers.random_points(n, seed=seed, outside_frac=0.0)
        _check_fp16(f, x.to(device), ref16d.deform_field_f16(x, wts), f"T=2^16 n={n}")


def test_deform_fp16_at_the_reference_table_size(device):
    """The reference's table (train_finetune.py:387-399: ``Field(precision=16, log2_T=24)``, 101.6 M rows, levels 0-10
    dense): 4 001 random points and a 2 048-point surface patch a pixel apart, at the same bars.  Measured: 99.925 % /
    99.805 % within the bar, maximum 1.0e-4 / 1.3e-4; the fp32 kernel 16.3 % / 12.8 %."""
    f, wts = _field(device, log2_T=24)
    assert 101_000_000 < f.xyz_encoder.grid.n_rows < 102_000_000
    wts16 = dataclasses.replace(wts, table=ref16d.half_round(wts.table))     # rounded once (the helper's rounding is then exact)
    del wts
    x, _ = helpers.random_points(4001, seed=24, outside_frac=0.0)
    _check_fp16(f, x.to(device), ref16d.deform_field_f16(x, wts16), "T=2^24 random")
    base = torch.tensor([0.31, -0.42, 0.77])
    patch = base + 1e-3 * torch.randn(2048, 3, generator=torch.Generator().manual_seed(3))
    _check_fp16(f, patch.to(device), ref16d.deform_field_f16(patch, wts16), "T=2^24 patch")
    del f, wts16
    torch.cuda.empty_cache()


def test_deform_fp16_order_and_device_count(device):
    """A processing permutation changes nothing, bit for bit; with a device-side count below the capacity exactly the
    first n_device outputs (and encoding rows) are written; the encoding rows are the fp16-rounded features."""
    from quadraturefields_amd import _C
    f, wts = _field(device)
    f.compute_dtype = "fp16"
    n = 5003
    x, _ = helpers.random_points(n, seed=11, outside_frac=0.0)
    x = x.to(device)
    plain = f(x, return_grad=False)[0]
    order = torch.randperm(n, generator=torch.Generator().manual_seed(4)).to(torch.int32).to(device)
    assert torch.equal(f(x, return_grad=False, order=order)[0], plain)
    enc_full = torch.empty((n, 32), dtype=torch.float32, device=device)
    full = f._density_fused(x, enc_out=enc_full)
    assert torch.equal(full, plain)
    assert torch.equal(enc_full, enc_full.half().float())                  # every feature is an fp16 value
    x01 = (x.cpu() + wts.scale) / (2.0 * wts.scale)
    enc_ref = ref16d.half_round(ofields.hash_encode(x01, ref16d.half_round(wts.table), wts.levels))
    assert float((enc_full.cpu() == enc_ref).double().mean()) >= 0.999    # equal but for rounding-midpoint flips
    # the C entry with n_device = 1234 < n: the rest of out / enc_out keeps its sentinel
    nd = 1234
    out = torch.full((n,), float("nan"), device=device)
    enc = torch.full((n, 32), -7.0, device=device)
    d = f.decoder_field
    w = [_C.f32c(t.detach()) for t in (d.layers[0].weight, d.layers[0].bias, d.layers[1].weight, d.layers[1].bias,
                                       d.lout.weight, d.lout.bias)]
    n_dev = torch.tensor([nd], dtype=torch.int64, device=device)
    _C.check(_C.lib().qf_deform_field_forward_f16(
        f.xyz_encoder.grid.desc, _C.ptr(f._half_table()), float(f.scale), 32, *[_C.ptr(t) for t in w], _C.ptr(x), n,
        _C.ptr(n_dev), None, _C.ptr(out), _C.ptr(enc), _C.stream()), "qf_deform_field_forward_f16")
    assert torch.equal(out[:nd], plain[:nd, 0]) and torch.equal(enc[:nd], enc_full[:nd])
    assert bool(out[nd:].isnan().all()) and bool((enc[nd:] == -7.0).all())
    # the same through the module (the route render_async takes)
    got = f(x, return_grad=False, n_device=n_dev)[0]
    assert torch.equal(got[:nd], plain[:nd])
    # the entry's argument rules are the fp32 entry's
    lib = _C.lib()
    args = [f.xyz_encoder.grid.desc, _C.ptr(f._half_table()), float(f.scale), 32, *[_C.ptr(t) for t in w], _C.ptr(x),
            n, None, None, _C.ptr(out), None, _C.stream()]
    bad_hidden = list(args)
    bad_hidden[3] = 64
    assert lib.qf_deform_field_forward_f16(*bad_hidden) == lib.qf_deform_field_forward(*bad_hidden) == QF_ERR_UNSUPPORTED
    no_table = list(args)
    no_table[1] = None
    assert lib.qf_deform_field_forward_f16(*no_table) == QF_ERR_INVALID_ARGUMENT
    no_w1 = list(args)
    no_w1[4] = None
    assert lib.qf_deform_field_forward_f16(*no_w1) == QF_ERR_INVALID_ARGUMENT
    empty = list(args)
    empty[11] = 0
    empty[10] = None                                                             # n == 0: OK, nothing read
    assert lib.qf_deform_field_forward_f16(*empty) == QF_OK


def test_deform_fp16_cache_follows_the_parameters(device):
    """The fp16 table is built once per parameter version: reused across calls, rebuilt after an in-place edit (what an
    optimiser step or load_state_dict does), released by switching back to fp32, which then gives the bits of a fresh
    fp32 Field."""
    f, wts = _field(device)
    f.compute_dtype = "fp16"
    x, _ = helpers.random_points(3001, seed=12, outside_frac=0.0)
    xd = x.to(device)
    first = f(xd, return_grad=False)[0]
    copy0 = f._half_cache[1]
    assert torch.equal(f(xd, return_grad=False)[0], first) and f._half_cache[1] is copy0     # not rebuilt per call
    f.xyz_encoder.params.mul_(-0.75)                                       # in place: the parameter's version moves
    wts_edit = dataclasses.replace(wts, table=wts.table * -0.75)
    got = f(xd, return_grad=False)[0]
    assert f._half_cache[1] is not copy0
    frac, mx = _stats(got, ref16d.deform_field_f16(x, wts_edit))
    assert frac >= FRAC_MIN and mx <= MAX_TOL, (frac, mx)
    assert not torch.equal(got, first)
    f.compute_dtype = "fp32"
    back = f(xd, return_grad=False)[0]
    assert getattr(f, "_half_cache", None) is None                        # released
    fresh, _ = _field(device)
    fresh.xyz_encoder.params.mul_(-0.75)
    assert torch.equal(back, fresh(xd, return_grad=False)[0])


def test_fp16_copies_follow_a_fused_adam_step(device):
    """quadraturefields_amd.optim.Adam updates the parameters through raw pointers; it moves their version counters, so
    the fp16 copies of both fields are rebuilt after its step: the next fp16 evaluation is the fp16 reference of the
    updated table, and equals an evaluation from a freshly built copy bit for bit."""
    from quadraturefields_amd.optim import Adam
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceField
    from quadraturefields_amd import synthetic
    f, _ = _field(device)
    f.compute_dtype = "fp16"
    x, dirs = helpers.random_points(3001, seed=14, outside_frac=0.0)
    xd = x.to(device)
    before = f(xd, return_grad=False)[0]
    assert f._half_cache is not None
    opt = Adam(f.parameters(), lr=1e-2, eps=1e-15)
    g = torch.Generator(device="cpu").manual_seed(5)
    for p in f.parameters():
        p.grad = torch.randn(p.shape, generator=g).to(device)
    v0 = f.xyz_encoder.params._version
    opt.step()
    assert f.xyz_encoder.params._version > v0
    after = f(xd, return_grad=False)[0]
    assert not torch.equal(after, before)
    frac, mx = _stats(after, ref16d.deform_field_f16(x, helpers.oracle_deform_weights(f)))
    assert frac >= FRAC_MIN and mx <= MAX_TOL, (frac, mx)
    f._half_cache = None
    assert torch.equal(f(xd, return_grad=False)[0], after)
    # the NGP field's fp16 copies (same cache key)
    torch.manual_seed(0)
    ngp = NGPRadianceField(aabb=[-1.5] * 3 + [1.5] * 3, log2_hashmap_size=12)
    ngp.load_state_dict(synthetic.seeded_ngp_state(12, ngp.mlp_base.grid.n_rows, seed=42), strict=False)
    ngp = ngp.to(device)
    ngp.compute_dtype = "fp16"
    dd = dirs.to(device)
    rgb0, den0 = ngp(xd, dd)
    opt = Adam(ngp.parameters(), lr=1e-2, eps=1e-15)
    for p in ngp.parameters():
        p.grad = torch.randn(p.shape, generator=g).to(device)
    opt.step()
    rgb1, den1 = ngp(xd, dd)
    assert not torch.equal(rgb1, rgb0) and not torch.equal(den1, den0)
    ngp._half_cache = None
    rgb2, den2 = ngp(xd, dd)
    assert torch.equal(rgb1, rgb2) and torch.equal(den1, den2)


def test_deform_fp16_leaves_training_fp32(device):
    """With autograd recording the field trains in fp32 whatever compute_dtype says.  Bit-identical between the two
    modes: the forward output of a small deformation loss (fused backward), the encoding saved for its backward, and the
    field gradient of ``forward(return_grad=True)``.  The parameter gradients are summed with fp32 atomics (table
    scatter, MLP weight tiles), whose order -- and so whose last bits -- is not reproducible from one launch to the next
    even in fp32.  So two fp32 runs are compared too.  Measured on MI355X: two fp32 runs differ by 7.1e-7 of the largest
    entry, the fp16 setting from fp32 by 5.5e-7, i.e. at the fp32 noise.  Both must stay within 1e-5 (about 14x the
    measured noise); an fp16 forward would move the gradients by ~1e-4, and the saved encoding above is already
    required to be the fp32 one bit for bit."""
    x, _ = helpers.random_points(4099, seed=13, outside_frac=0.0)
    res = {}
    for run, dt in (("fp32", "fp32"), ("fp32 again", "fp32"), ("fp16", "fp16")):
        f, _ = _field(device)
        f.compute_dtype = dt
        with torch.enable_grad():
            out = f.density(x.to(device))
            enc = out.grad_fn.saved_tensors[-1]                          # _DeformTrainFn's encoding [n,32]
            loss = (torch.tanh(out) * 0.13).pow(2).mean()
            loss.backward()
            xg = x.to(device).requires_grad_(True)
            field, grad = f(xg, return_grad=True)
        assert getattr(f, "_half_cache", None) is None                   # no fp16 copy was made
        res[run] = ([out.detach(), enc.detach(), field.detach(), grad.detach()],
                    [p.grad.clone() for p in f.parameters()])
    assert enc.shape == (4099, 32) and not torch.equal(enc, enc.half().float())   # the fp32 features
    for a, b in zip(res["fp32"][0], res["fp16"][0]):
        assert torch.equal(a, b)
    assert len(res["fp32"][1]) == len(res["fp16"][1]) == 7

    def rel(other):
        return max(float((a - b).abs().max()) / float(a.abs().max()) for a, b in zip(res["fp32"][1], res[other][1]))

    noise, d16 = rel("fp32 again"), rel("fp16")
    print(f"parameter gradients, max |diff| / max |g|: fp32 vs fp32 {noise:.2e}, fp16 setting vs fp32 {d16:.2e}")
    assert noise <= 1e-5 and d16 <= 1e-5


def _deformed_scene(device):
    from quadraturefields_amd import synthetic
    from quadraturefields_amd.field import Field
    from quadraturefields_amd.mesh_utils import MeshIntersection
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceField
    mesh = synthetic.shell_mesh(n_shells=4, subdivisions=3)
    mi = MeshIntersection(mesh, simplify_mesh=False, scale=1.0, num_intersections=25)
    field = NGPRadianceField(aabb=[-1.5] * 3 + [1.5] * 3, log2_hashmap_size=14)
    field.load_state_dict(synthetic.seeded_ngp_state(14, field.mlp_base.grid.n_rows), strict=False)
    net = Field(scale=1.5, precision=16, log2_T=14, L=16, max_res=512, min_res=16, output_dim=1, hidden_size=32,
                num_features=2, back_prop=False, nl="relu")
    net.load_state_dict(synthetic.seeded_deform_state(net.xyz_encoder.grid.n_params), strict=False)
    return mi, field.to(device), net.to(device)


def test_deformed_frames_at_fp16_on_every_route(device):
    """Both fields at compute_dtype = "fp16", scalings 0.0434 (the scripts'), 0.13 and 1.5: FrameRenderer.render with a
    camera, FrameRenderer.render_async (device-side sample count) and render_image_finetune_with_occgrid on the
    ray-major samples give bit-identical pixels, and they differ from the same frame with an fp32 deformation field --
    each route took the fp16 deformation."""
    from quadraturefields_amd import synthetic, utils
    from quadraturefields_amd.datasets.utils import Rays
    from quadraturefields_amd.mesh_utils import make_camera
    from quadraturefields_amd.render import FrameRenderer
    mi, field, net = _deformed_scene(device)
    field.compute_dtype = "fp16"
    w = h = 64
    c2w = synthetic.orbit_cameras(1, seed=2)[0]
    focal = synthetic.lego_focal(800) * w / 800.0
    o, d = synthetic.camera_rays(c2w, focal, w, h)
    od, dd = o.to(device), d.to(device)
    cam = make_camera(c2w, focal, w, h)
    fr = FrameRenderer(mi, field, field_net=net)
    for sc in (0.0434, 0.0434 * 3, 1.5):
        frames = {}
        for dt in ("fp32", "fp16"):
            net.compute_dtype = dt
            data = mi.sampling_raytrace_device(d, o)
            ref = utils.render_image_finetune_with_occgrid(field, net, None, Rays(origins=o, viewdirs=d), data,
                                                           render_step_size=5e-3, mesh_intersect=mi, scaling=sc)
            rgb_f, alpha_f, depth_f, n_f = fr.render(od, dd, scaling=sc, camera=cam)
            rgb_a, alpha_a, depth_a, _ = fr.render_async(od, dd, cam, scaling=sc)
            assert n_f == ref[3]
            assert torch.equal(rgb_f, ref[0].reshape(-1, 3)) and torch.equal(alpha_f, ref[1].reshape(-1, 1))
            assert torch.equal(depth_f, ref[2].reshape(-1, 1))
            assert torch.equal(rgb_a, rgb_f) and torch.equal(alpha_a, alpha_f) and torch.equal(depth_a, depth_f)
            frames[dt] = (rgb_f, depth_f)
        assert not torch.equal(frames["fp16"][1], frames["fp32"][1]), sc
    net.compute_dtype = "fp32"


def test_fp16_deformation_quality_against_the_fp32_oracle(device):
    """What the reference's precision costs: the 64 x 64 deformed frame (host quadrature points, scaling 0.13) with the
    deformation field at fp16 against the fp32 oracle frame (oracle.meshpath.render_image_finetune), with the radiance
    field at fp32 and at fp16, and the largest difference of the displacement tanh(f) * scaling over the frame's
    samples.  Measured on MI355X: all fp32 116.8 dB, fp16 deformation 72.1 dB, both fields fp16 72.2 dB; displacement
    difference at most 6.6e-5 (scene units; the scene is 3 across).  Floors: 68 dB and 1.5e-4."""
    from oracle import meshpath as om
    from quadraturefields_amd import synthetic, utils
    from quadraturefields_amd.datasets.utils import Rays
    from quadraturefields_amd.render import psnr
    mi, field, net = _deformed_scene(device)
    ngp_w, def_w = helpers.oracle_ngp_weights(field), helpers.oracle_deform_weights(net)
    w = h = 64
    o, d = synthetic.camera_rays(synthetic.orbit_cameras(1, seed=2)[0], synthetic.lego_focal(800) * w / 800.0, w, h)
    data = om.to_loader_tensors(mi.sampling_raytrace_numpy(d.numpy(), o.numpy(), 0))
    sc = 0.0434 * 3
    rgb_o = om.render_image_finetune(ngp_w, def_w, data, w * h, scaling=sc)[0]
    out = {}
    for ngp_dt, def_dt in (("fp32", "fp32"), ("fp32", "fp16"), ("fp16", "fp16")):
        field.compute_dtype, net.compute_dtype = ngp_dt, def_dt
        out[(ngp_dt, def_dt)] = utils.render_image_finetune_with_occgrid(
            field, net, None, Rays(origins=o, viewdirs=d), data, render_step_size=5e-3, mesh_intersect=mi,
            scaling=sc)[0].cpu()
    p = {k: psnr(v.reshape(-1, 3), rgb_o.reshape(-1, 3)) for k, v in out.items()}
    net.compute_dtype = "fp16"
    disp16 = torch.tanh(net(data[0].to(device), return_grad=False)[0].cpu()) * sc
    disp_o = torch.tanh(ofields.deform_field(data[0], def_w)) * sc
    dmax = float((disp16 - disp_o).abs().max())
    net.compute_dtype = field.compute_dtype = "fp32"
    print(f"PSNR against the fp32 oracle: all fp32 {p[('fp32', 'fp32')]:.1f} dB, fp16 deformation "
          f"{p[('fp32', 'fp16')]:.1f} dB, both fp16 {p[('fp16', 'fp16')]:.1f} dB; max displacement difference {dmax:.3e}")
    assert not torch.equal(out[("fp32", "fp16")], out[("fp32", "fp32")])
    assert p[("fp32", "fp32")] >= 100.0
    assert p[("fp32", "fp16")] >= 68.0
    assert p[("fp16", "fp16")] >= 68.0
    assert dmax <= 1.5e-4
