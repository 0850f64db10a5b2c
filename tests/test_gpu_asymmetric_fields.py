"""GPU: the fused field kernels, their fused backward and one frame on a box that is not a centred cube
(``tests/asymmetric_inputs.BOX``: extents 3.0 / 1.75 / 2.75, centre off the origin on every axis).

Every other field test builds its module on ``[-1.5]*3 + [1.5]*3``, where a kernel that reads another axis's extent, takes
``lo`` for ``-hi`` or scales a position gradient by another axis computes the same numbers;
``tests/test_asymmetric_inputs_host.py`` shows that these inputs do tell.  Same seeded states, same oracles and the SAME
BOUNDS as the tests mirrored here: ``test_gpu_fields.py`` (fp32: 2e-5 + 2e-5 |b| on rgb and geo features, 1e-7 + 5e-5 |b|
on densities, 5e-5 on SG rgb / features; bf16: 2e-3 and 1e-6 + 1e-2 |b|), ``test_gpu_fp16.py`` (2.5e-4 and 1.25e-3
relative), ``test_gpu_train.py`` (gradients: 3e-4 of the largest reference entry for the NGP head, 5e-4 for the SG head),
``test_gpu_render.py`` (pixels: 2e-4).
"""
import numpy as np
import pytest
import torch

from oracle import fields as ofields
from oracle import meshpath as om
from tests import asymmetric_inputs as asym
from tests import fp16_reference as ref16
from tests import helpers

pytestmark = pytest.mark.gpu

UNIT_BOX = [0.0, 0.0, 0.0, 1.0, 1.0, 1.0]


def _make(cls, device, aabb=asym.BOX, log2_T=12, seed=42, **kw):
    from quadraturefields_amd import synthetic
    torch.manual_seed(0)
    f = cls(aabb=list(aabb), log2_hashmap_size=log2_T, **kw)
    st = synthetic.seeded_ngp_state(log2_T, f.mlp_base.grid.n_rows, seed=seed, sg_lobes=kw.get("num_g_lobes", 0))
    missing = f.load_state_dict(st, strict=False)
    assert not missing.unexpected_keys
    assert f.aabb.tolist() == list(aabb)                  # (the state dict carries no box of its own)
    return f.to(device)


def _ratio(a, b, atol, rtol):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float(((a - b).abs() / (atol + rtol * b.abs())).max()) if a.numel() else 0.0


def _close(a, b, atol, rtol, what=""):
    r = _ratio(a, b, atol, rtol)
    print(f"{what}: worst ratio against the bound {r:.3f}")
    assert r <= 1.0, f"{what}: worst ratio {r:.2f}"


def _selector(x, w):
    sel = ofields.normalize_to_aabb(x, w.aabb)[0]
    n_fixed = min(x.shape[0], asym.FIXED_ROWS)
    want = asym.fixed_rows()[1][asym.FIXED_ROWS - n_fixed:]
    assert torch.equal(sel[x.shape[0] - n_fixed:], want)          # faces out, the cube witnesses as named, the centre in
    return sel, n_fixed


def _assert_selector(den, sel, n_fixed):
    den = den.detach().cpu().reshape(-1)
    assert bool((den[~sel] == 0).all()), "a point the oracle's selector rejects has a density"
    assert bool((den[sel] != 0).all()), "a point the oracle's selector accepts has none"
    fixed = slice(den.shape[0] - n_fixed, den.shape[0])
    assert torch.equal(den[fixed] != 0, sel[fixed])


@pytest.mark.parametrize("n", [1, 17, 4101])
def test_ngp_forward_on_the_box(device, n):
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceField
    f = _make(NGPRadianceField, device)
    x, d = asym.box_points(n, seed=n)
    w = helpers.oracle_ngp_weights(f)
    assert w.aabb.tolist() == asym.BOX
    sel, n_fixed = _selector(x, w)
    rgb_o, den_o = ofields.ngp_forward(x, d, w)
    rgb, den = f(x.to(device), d.to(device))
    assert rgb.shape == (n, 3) and den.shape == (n, 1)
    _close(rgb, rgb_o, 2e-5, 2e-5, f"n={n} rgb")
    _close(den, den_o, 1e-7, 5e-5, f"n={n} density")
    _assert_selector(den, sel, n_fixed)
    if n > 100:
        assert 0.02 < float((~sel).float().mean()) < 0.2


def test_query_density_and_feat_on_the_box(device):
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceField
    f = _make(NGPRadianceField, device)
    x, _ = asym.box_points(2048, seed=3)
    w = helpers.oracle_ngp_weights(f)
    sel, n_fixed = _selector(x, w)
    den_o, feat_o = ofields.query_density(x, w, return_feat=True)
    den, feat = f.query_density(x.to(device), return_feat=True)
    assert feat.shape == (2048, 15)
    _close(den, den_o, 1e-7, 5e-5, "density")
    _close(feat, feat_o, 2e-5, 2e-5, "geo features")
    _assert_selector(den, sel, n_fixed)
    den2 = f.query_density(x.to(device).reshape(32, 64, 3))
    assert den2.shape == (32, 64, 1) and torch.equal(den2.reshape(-1), den.reshape(-1))
    # the module's own normalize (torch, on the device) agrees with the oracle's on every point, bit for bit
    sel_d, x01 = f.normalize(x.to(device))
    sel_o, x01_o = ofields.normalize_to_aabb(x, w.aabb)
    assert torch.equal(sel_d.cpu(), sel_o) and torch.equal(x01.cpu(), x01_o)
    _close(f.mlp_base(x01)[:, 1:], feat_o, 2e-5, 2e-5, "tcnn duck type")


@pytest.mark.parametrize("lobes", [1, 8])
def test_sg_forward_and_features_on_the_box(device, lobes):
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceFieldSGNew
    f = _make(NGPRadianceFieldSGNew, device, use_viewdirs=False, num_g_lobes=lobes)
    x, d = asym.box_points(1000 + lobes, seed=lobes)
    w = helpers.oracle_ngp_weights(f)
    sel, n_fixed = _selector(x, w)
    rgb_o, den_o = ofields.sg_forward(x, d, w)
    feats_o = ofields.sg_features(x, w)
    rgb, den = f(x.to(device), d.to(device))
    feats = f.features(x.to(device))
    assert feats.shape == (x.shape[0], 3 + 7 * lobes + 1)
    _close(den, den_o, 1e-7, 5e-5, "density")
    _close(feats[:, :-1], feats_o[:, :-1], 5e-5, 5e-5, "features")
    _close(feats[:, -1], feats_o[:, -1], 1e-7, 5e-5, "features' density")
    _close(rgb, rgb_o, 5e-5, 5e-5, "rgb")
    _assert_selector(den, sel, n_fixed)
    _assert_selector(feats[:, -1], sel, n_fixed)


@pytest.mark.parametrize("n", [17, 5000])
def test_fp16_ngp_on_the_box(device, n):
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceField
    f = _make(NGPRadianceField, device, log2_T=14)
    f.compute_dtype = "fp16"
    x, d = asym.box_points(n, seed=n + 100)
    w = helpers.oracle_ngp_weights(f)
    sel, n_fixed = _selector(x, w)
    rgb_o, den_o = ref16.ngp_forward_f16(x, d, w)
    rgb, den = f(x.to(device), d.to(device))
    _close(rgb, rgb_o, 2.5e-4, 2.5e-4, f"fp16 n={n} rgb")
    _close(den, den_o, 1e-7, 1.25e-3, f"fp16 n={n} density")
    _assert_selector(den, sel, n_fixed)
    den2, feat = f.query_density(x.to(device), return_feat=True)
    _close(feat, ref16.query_density_f16(x, w)[1], 2.5e-4, 2.5e-4, f"fp16 n={n} geo features")
    assert torch.equal(den2, den)
    if n > 100:                                           # "fp16" is not quietly evaluated in fp32 (as the mirrored test)
        f.compute_dtype = "fp32"
        rgb32, _ = f(x.to(device), d.to(device))
        m16, m32 = float((rgb.cpu() - rgb_o).abs().mean()), float((rgb32.cpu() - rgb_o).abs().mean())
        e16, e32 = float((rgb.cpu() - rgb_o).abs().max()), float((rgb32.cpu() - rgb_o).abs().max())
        print(f"max |fp16 - ref16| = {e16:.3e}, max |fp32 - ref16| = {e32:.3e}; means {m16:.3e} / {m32:.3e}")
        assert m16 <= 0.25 * m32
        assert e16 < e32


@pytest.mark.parametrize("n", [17, 5000])
def test_bf16_ngp_on_the_box(device, n):
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceField
    f = _make(NGPRadianceField, device, log2_T=14)
    f.compute_dtype = "bf16"
    x, d = asym.box_points(n, seed=n + 100)
    w = helpers.oracle_ngp_weights(f)
    sel, n_fixed = _selector(x, w)
    rgb_o, den_o = ofields.ngp_forward_bf16(x, d, w)
    rgb, den = f(x.to(device), d.to(device))
    _close(rgb, rgb_o, 2e-3, 2e-3, f"bf16 n={n} rgb")
    _close(den, den_o, 1e-6, 1e-2, f"bf16 n={n} density")
    _assert_selector(den, sel, n_fixed)
    den2, feat = f.query_density(x.to(device), return_feat=True)
    _close(feat, ofields.query_density_bf16(x, w)[1], 2e-3, 2e-3, f"bf16 n={n} geo features")
    assert torch.equal(den2, den)
    f.compute_dtype = "fp32"                              # close to, but not, the fp32 evaluation (as the mirrored test)
    rgb32, _ = f(x.to(device), d.to(device))
    assert float((rgb32 - rgb).abs().max()) < 0.08
    if n > 100:
        assert float((rgb32 - rgb).abs().max()) > 1e-5


@pytest.mark.parametrize("dtype", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("head", ["ngp", "sg"])
def test_box_module_equals_the_unit_box_module_at_x01(device, head, dtype):
    """No oracle: the module on BOX at x against a module on [0,1]^3, same parameters, at x01 = (x - lo) / (hi - lo)
    computed on the host in fp32 -- the kernels' own expression, and on the unit box (x01 - 0) / (1 - 0) is x01 exactly.
    Densities and colours are equal bit for bit wherever the selector is true."""
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceField, NGPRadianceFieldSGNew
    kw = dict(use_viewdirs=False, num_g_lobes=3) if head == "sg" else {}
    cls = NGPRadianceFieldSGNew if head == "sg" else NGPRadianceField
    on_box, on_unit = _make(cls, device, **kw), _make(cls, device, aabb=UNIT_BOX, **kw)
    for (ka, a), (kb, b) in zip(on_box.state_dict().items(), on_unit.state_dict().items()):
        assert ka == kb and (ka == "aabb" or torch.equal(a, b))
    on_box.compute_dtype = on_unit.compute_dtype = dtype
    x, d = asym.box_points(4101, seed=7)
    lo, hi = torch.tensor(asym.BOX_LO, dtype=torch.float32), torch.tensor(asym.BOX_HI, dtype=torch.float32)
    x01 = (x - lo) / (hi - lo)
    sel = ((x01 > 0.0) & (x01 < 1.0)).all(dim=-1)
    assert torch.equal(sel, ofields.normalize_to_aabb(x, torch.tensor(asym.BOX))[0]) and 0.02 < float((~sel).float().mean()) < 0.2
    rgb_a, den_a = on_box(x.to(device), d.to(device))
    rgb_b, den_b = on_unit(x01.to(device), d.to(device))
    sel_d = sel.to(device)
    assert torch.equal(den_a, den_b)                      # (outside both are zero)
    assert bool((den_a[sel_d] != 0).all()) and bool((den_a[~sel_d] == 0).all())
    assert torch.equal(rgb_a[sel_d], rgb_b[sel_d])
    assert float(rgb_a[sel_d].std()) > 0.01


def _leaf(t):
    return t.detach().clone().requires_grad_(True)


def _oracle_leaves(wts):
    wts.table = _leaf(wts.table)
    wts.base = [_leaf(w) for w in wts.base]
    if wts.head_tcnn is not None:
        wts.head_tcnn = [_leaf(w) for w in wts.head_tcnn]
    if getattr(wts, "head_layers", None):
        wts.head_layers = [(_leaf(w), _leaf(b)) for w, b in wts.head_layers]
    return wts


def _grad_close(got, want, rtol):
    """test_gpu_train._close: max |got - want| <= rtol * max |want|."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    err, ref = float((got - want).abs().max()), float(want.abs().max())
    return err <= rtol * ref, err, ref


@pytest.mark.parametrize("n", [17, 1000])
@pytest.mark.parametrize("head,rtol", [("ngp", 3e-4), ("sg", 5e-4)])
def test_position_gradients_through_the_fused_backward_on_the_box(device, head, rtol, n):
    """d loss / d position of the fused training route (``g_pos = g_x01 / (hi - lo)``, radiance_fields/ngp.py) against
    autograd through the oracle, axis by axis, with the bound test_gpu_train.py holds the parameter gradients to; the
    parameter gradients ride along.  At n = 1000 the three axes' mean |gradient| stand in the inverse ratio of the
    extents (the encoding is isotropic in x01), so a gradient scaled by another axis's extent cannot pass."""
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceField, NGPRadianceFieldSGNew
    if head == "ngp":
        field = _make(NGPRadianceField, device, log2_T=14)
    else:
        field = _make(NGPRadianceFieldSGNew, device, log2_T=13, use_viewdirs=False, num_g_lobes=3)
    assert field.fused_backward
    wts = _oracle_leaves(helpers.oracle_ngp_weights(field))
    x, d = asym.box_points(n, seed=n + 5)
    g = torch.Generator().manual_seed(9)
    t_rgb, t_sig = torch.rand(n, 3, generator=g), torch.rand(n, 1, generator=g)

    def loss_fn(rgb, sigma, t_rgb, t_sig):
        return ((rgb - t_rgb) ** 2).mean() + 1e-2 * ((torch.log1p(sigma) - t_sig) ** 2).mean()

    with torch.enable_grad():
        xd, xo = _leaf(x.to(device)), _leaf(x)
        rgb_t, sig_t = field(xd, d.to(device))
        assert rgb_t.requires_grad and sig_t.requires_grad
        loss_fn(rgb_t, sig_t, t_rgb.to(device), t_sig.to(device)).backward()
        rgb_o, sig_o = (ofields.ngp_forward if head == "ngp" else ofields.sg_forward)(xo, d, wts)
        loss_fn(rgb_o, sig_o, t_rgb, t_sig).backward()
    assert xd.grad is not None and xd.grad.shape == (n, 3)
    sel = ofields.normalize_to_aabb(x, wts.aabb)[0]
    for k in range(3):                                    # (every point: the colour's gradient does not stop at the faces)
        ok, err, ref = _grad_close(xd.grad[:, k], xo.grad[:, k], rtol)
        print(f"{head} n={n} axis {k}: max |d - oracle| = {err:.3e}, {err / (rtol * ref):.3f} of the bound; max |oracle| = {ref:.3e}")
        assert ok and ref > 0, (k, err, ref)
    n_net = field.mlp_base.n_network_params
    gb = field.mlp_base.params.grad
    for name, got, want in (("table", gb[n_net:], wts.table.grad.reshape(-1)),
                            ("base mlp", gb[:n_net], torch.cat([w.grad.reshape(-1) for w in wts.base]))):
        ok, err, ref = _grad_close(got, want, rtol)
        assert ok and ref > 0, (name, err, ref)
    if n >= 1000:
        ext = np.array(asym.BOX_HI) - np.array(asym.BOX_LO)
        for grad in (xo.grad.double(), xd.grad.cpu().double()):
            mean = grad[sel].abs().mean(dim=0).numpy()
            scaled = mean * ext                            # mean |g_x01|: the same on every axis, up to sampling noise
            print(f"mean |g| per axis {mean}, times the extent {scaled}")
            assert scaled.max() / scaled.min() < 1.25      # every pair of axes within 25 % of its extent ratio ...
            assert mean[1] / mean[0] > 1.25 and mean[1] / mean[2] > 1.25      # ... which are 1.71 and 1.57 for y : x and y : z


def test_one_frame_with_the_box_field(device):
    """FrameRenderer, 4 shells of 5120 triangles in all, 40 x 24, K = 25, the field on BOX (which cuts through the shells):
    the one-call frame equals the separately bound launches bit for bit (as in test_gpu_render.py), and the oracle's
    pixels within that file's 2e-4.  The frame has samples on both sides of the box's faces."""
    from quadraturefields_amd import synthetic
    from quadraturefields_amd.mesh_utils import MeshIntersection, make_camera
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceField
    from quadraturefields_amd.render import FrameRenderer
    mesh = synthetic.shell_mesh(n_shells=4, subdivisions=3)
    mi = MeshIntersection(mesh, simplify_mesh=False, scale=1.0, num_intersections=25)
    field = _make(NGPRadianceField, device, log2_T=14)
    fr = FrameRenderer(mi, field)
    ri = mi.rayintersector
    w, h = 40, 24
    focal = synthetic.lego_focal(800) * w / 800.0
    c2w = synthetic.orbit_cameras(2, seed=5)[1]
    o, d = synthetic.camera_rays(c2w, focal, w, h)
    cam = make_camera(c2w, focal, w, h)
    od, dd = o.to(device), d.to(device)
    assert ri.fused_frame_ready(cam, mi.num_intersections)
    one = fr.render_async(od, dd, cam)
    n_one = ri.frame_samples()
    ready = ri.fused_frame_ready
    ri.fused_frame_ready = lambda *a, **k: False
    try:
        sep = fr.render_async(od, dd, cam)
    finally:
        ri.fused_frame_ready = ready
    n_sep = ri.frame_samples()
    assert n_one == n_sep > 500
    for a, b in zip(one[:3], sep[:3]):
        assert (a is None and b is None) or torch.equal(a, b)
    assert torch.equal(one[3].hit_count, sep[3].hit_count) and torch.equal(one[3].tile_base, sep[3].tile_base)
    total = int(one[3].total_dev.item())
    assert torch.equal(one[3].depth_c[:total], sep[3].depth_c[:total])
    assert ri.camera_mismatch_frames == 0                 # the camera-coherent pass answered, not the BVH
    data = om.to_loader_tensors(om.sampling_raytrace_numpy(om.BruteForceIntersector(mesh.vertices, mesh.faces),
                                                           d.numpy(), o.numpy(), 25))
    wts = helpers.oracle_ngp_weights(field)
    sel = ofields.normalize_to_aabb(data[0], wts.aabb)[0]
    assert n_one == data[0].shape[0]
    print(f"{n_one} samples, {int(sel.sum())} inside the box")
    assert int(sel.sum()) > 100 and int((~sel).sum()) > 100
    rgb_o = om.render_image_finetune(wts, None, data, w * h)[0]
    ref = fr.render(od, dd, camera=cam)
    assert ref[3] == n_one and torch.equal(ref[0], one[0])
    err = float((one[0].cpu() - rgb_o).abs().max())
    print(f"max |rgb - oracle| = {err:.3e}")
    assert err <= 2e-4, err
