"""GPU: qf_frame_score / qf_frame_images_u8 through ``quadraturefields_amd.metrics`` against the fp64 references of
``tests/frame_metrics_reference.py``.

Where the bars come from (none is taken from what the kernels give):

* Down-sample.  The kernel adds the f^2 values of a block in fp32 (f^2 - 1 additions, each off by at most half an ulp,
  2^-24 relative, of a partial sum that is no larger than sum|x|), multiplies by fl(1/f^2) (one more 2^-24 for the constant,
  one for the product; both exact at f = 2) -- to first order |err| <= (f^2 + 1) 2^-24 mean|block|, plus 2^-149 for a
  subnormal result.  At f = 1 the value is copied: bitwise equal.
* MSE.  Every down-sampled value is within delta = f^2 2^-24 max|x| of the fp64 one, so by Cauchy-Schwarz
  |mse - mse64| <= 2 sqrt(mse64) delta + delta^2; PSNR = -10 log10 of a value in that interval.
* SSIM.  The reference is ``ssim_torchmetrics`` in fp64 ON THE DOWN-SAMPLED IMAGE THE KERNEL RETURNED (the down-sample has
  its own bar above); the yardstick is the same function in fp32, what a user of torchmetrics gets.  A window may be off
  by twice the yardstick's largest window error on that input, the frame value by twice the largest frame error the
  yardstick makes on any input of this file.
"""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import frame_metrics_reference as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTORS = (1, 2, 3)
KEYS = [(name, f) for name in ref.CASES for f in FACTORS]


class Scored:
    pass


@pytest.fixture(scope="module")
def scored(device):
    """Every case at every factor: scored once on the device, referenced once on the CPU."""
    from quadraturefields_amd.metrics import FrameScorer
    out = {}
    for name, f, render, truth, depth in ref.cases(FACTORS):
        h, w = truth.shape[:2]
        scorer = FrameScorer(h, w, up_sample=f, capacity=4, device=device)
        slot = scorer.score(torch.from_numpy(render).to(device), torch.from_numpy(truth).to(device),
                            depth=torch.from_numpy(depth).to(device), images=True, ssim_map=True)
        s = Scored()
        s.render, s.truth, s.depth, s.f = render, truth, depth, f
        s.rgb_small, s.depth_small = (t.cpu() for t in scorer.last_small())
        s.map = scorer.last_ssim_map().cpu()
        s.images = tuple(t.cpu() for t in scorer.last_images())
        s.record = scorer.record(slot).cpu()
        res = scorer.results()
        assert res["frames"] == 1
        s.mse, s.psnr, s.ssim, s.depth_max = (float(res[k][0]) for k in ("mse", "psnr", "ssim", "depth_max"))
        assert [s.mse, s.psnr, s.ssim, s.depth_max] == s.record.tolist()
        s.map64, s.ssim64 = ref.ssim_torchmetrics(s.rgb_small, truth, torch.float64)
        map32, ssim32 = ref.ssim_torchmetrics(s.rgb_small, truth, torch.float32)
        s.yard_map = float((map32.double() - s.map64).abs().max())
        s.yard_mean = abs(ssim32 - s.ssim64)
        out[(name, f)] = s
    return out


@pytest.fixture(scope="module")
def mean_bar(scored):
    """2 x the largest frame error of the yardstick over all inputs of this file (one input's error can be small by luck
    of cancellation; the largest cannot hide that)."""
    worst = max(s.yard_mean for s in scored.values())
    print(f"yardstick (fp32 torchmetrics) frame errors: " + ", ".join(f"{k[0]}/f{k[1]} {s.yard_mean:.2e}" for k, s in scored.items()))
    assert worst > 0
    return 2.0 * worst


@pytest.mark.parametrize("name,f", KEYS)
def test_downsample(scored, name, f):
    s = scored[(name, f)]
    for got, full in ((s.rgb_small, s.render), (s.depth_small, s.depth)):
        if f == 1:
            assert torch.equal(got, torch.from_numpy(full)), "f = 1 copies"
            assert np.array_equal(got.numpy().view(np.uint32), full.view(np.uint32))
            continue
        err = np.abs(got.double().numpy() - ref.box_downsample64(full, f))
        bar = (f * f + 1) * 2.0 ** -24 * ref.box_mean_abs64(full, f) + 2.0 ** -149
        worst = float((err / bar).max())
        print(f"{name} f={f}: max |err| {err.max():.3e}, max err/bar {worst:.3f}")
        assert worst <= 1.0
    assert s.depth_max == float(s.depth_small.max())


def _mse_bounds(s):
    mse64 = ref.mse64(ref.box_downsample64(s.render, s.f), s.truth)
    delta = s.f ** 2 * 2.0 ** -24 * float(np.abs(s.render).max())
    return mse64, 2.0 * math.sqrt(mse64) * delta + delta * delta


@pytest.mark.parametrize("name,f", KEYS)
def test_mse_and_psnr(scored, name, f):
    s = scored[(name, f)]
    mse64, bar = _mse_bounds(s)
    print(f"{name} f={f}: mse {s.mse:.17g} mse64 {mse64:.17g} |diff| {abs(s.mse - mse64):.3e} bar {bar:.3e} psnr {s.psnr:.12g}")
    assert abs(s.mse - mse64) <= bar
    lo = -10.0 * math.log10(mse64 + bar)
    hi = math.inf if mse64 - bar <= 0 else -10.0 * math.log10(mse64 - bar)
    assert lo - 1e-12 <= s.psnr <= hi + 1e-12
    assert s.psnr == (math.inf if s.mse == 0 else -10.0 * math.log10(s.mse)) or abs(s.psnr + 10.0 * math.log10(s.mse)) <= 1e-12
    if name == "identical" and f in (1, 2):          # the box average of 1 or 4 equal values is exact
        assert s.mse == 0.0 and s.psnr == math.inf


@pytest.mark.parametrize("name,f", KEYS)
def test_ssim_map(scored, name, f):
    s = scored[(name, f)]
    err = float((s.map.double() - s.map64).abs().max())
    print(f"{name} f={f}: ssim map max error {err:.3e}, yardstick {s.yard_map:.3e}")
    assert s.map.shape == (s.truth.shape[0] - 10, s.truth.shape[1] - 10, 3)
    assert err <= 2.0 * s.yard_map


@pytest.mark.parametrize("name,f", KEYS)
def test_ssim_mean(scored, mean_bar, name, f):
    s = scored[(name, f)]
    print(f"{name} f={f}: ssim {s.ssim:.15f} ssim64 {s.ssim64:.15f} |diff| {abs(s.ssim - s.ssim64):.3e} bar {mean_bar:.3e}")
    assert abs(s.ssim - s.ssim64) <= mean_bar
    assert abs(s.ssim - float(s.map.double().mean())) <= 1e-12       # fp64, ordered reduction of the returned values
    if name == "identical" and f in (1, 2):
        assert abs(s.ssim - 1.0) <= mean_bar
    if name == "constant":
        a, b = ref.CONSTANT_A, ref.CONSTANT_B
        assert abs(s.ssim - (2 * a * b + ref.C1) / (a * a + b * b + ref.C1)) <= mean_bar


@pytest.mark.parametrize("name,f", KEYS)
def test_images(scored, name, f):
    """Byte for byte the scripts' expressions (train_finetune.py:639-646) on the kernel's own down-sampled frame."""
    s = scored[(name, f)]
    rgb8, err8, depth8 = s.images
    clamped = s.rgb_small.clamp(0, 1)
    assert torch.equal(rgb8, (clamped * 255).to(torch.uint8))
    assert torch.equal(err8, ((clamped - torch.from_numpy(s.truth)).abs().clamp(0, 1) * 255).to(torch.uint8))
    depth_max = torch.tensor(s.depth_max, dtype=torch.float64).to(torch.float32)
    assert float(depth_max) == s.depth_max and s.depth_max > 0
    assert torch.equal(depth8, (s.depth_small / depth_max * 255).to(torch.uint8))
    assert int(depth8.max()) == 255


def test_all_miss_frame(device):
    """No hit: white render, zero depth.  The reference divides by zero here; the kernel writes a zero depth image."""
    from quadraturefields_amd.metrics import FrameScorer
    h, w, f = 40, 50, 2
    scorer = FrameScorer(h, w, up_sample=f, device=device)
    truth = torch.from_numpy(ref.case("block400", 1)[1][90:90 + h, 120:120 + w].copy()).to(device)   # a corner of the block
    slot = scorer.score(torch.ones(h * f * w * f, 3, device=device), truth, depth=torch.zeros(h * f * w * f, 1, device=device),
                        images=True)
    rgb8, err8, depth8 = scorer.last_images()
    assert int(depth8.max()) == 0 and int(rgb8.min()) == 255
    rec = scorer.record(slot).cpu()
    assert bool(torch.isfinite(rec).all()) and rec[3] == 0
    # without depth there is no depth image and depth_max is 0
    scorer.score(torch.ones(h * f, w * f, 3, device=device), truth, images=True)
    assert scorer.last_images()[2] is None and scorer.last_small()[1] is None
    assert scorer.results()["depth_max"].tolist() == [0.0, 0.0]


def test_argument_checks_on_the_device(device):
    from quadraturefields_amd.metrics import FrameScorer
    scorer = FrameScorer(32, 48, up_sample=2, capacity=1, device=device)
    good, truth = torch.zeros(64, 96, 3, device=device), torch.zeros(32, 48, 3, device=device)
    with pytest.raises(ValueError):
        scorer.score(torch.zeros(32, 48, 3, device=device), truth)
    with pytest.raises(ValueError):
        scorer.score(good, torch.zeros(48, 32, 3, device=device))
    with pytest.raises(ValueError):
        scorer.score(good, truth, depth=torch.zeros(32, 48, device=device))
    with pytest.raises(TypeError):
        scorer.score(good.double(), truth)
    with pytest.raises(ValueError):
        scorer.score(torch.zeros(64, 96, 6, device=device)[:, :, ::2], truth)
    assert len(scorer) == 0
    scorer.score(good, truth)
    with pytest.raises(RuntimeError, match="full"):
        scorer.score(good, truth)
    scorer.reset()
    assert scorer.score(good.reshape(-1, 3), truth.reshape(-1, 3), depth=torch.zeros(64 * 96, device=device)) == 0


def test_determinism(device):
    """The same frame in two slots, and again after 50 other frames: bit-identical records."""
    from quadraturefields_amd.metrics import FrameScorer
    render, truth, depth = (torch.from_numpy(a).to(device) for a in ref.case("odd133x77", 2))
    scorer = FrameScorer(133, 77, up_sample=2, capacity=64, device=device)
    g = torch.Generator(device=device).manual_seed(3)
    a = scorer.score(render, truth, depth=depth)
    b = scorer.score(render, truth, depth=depth)
    for _ in range(50):
        scorer.score(torch.rand(render.shape, generator=g, device=device), truth, depth=depth)
    c = scorer.score(render, truth, depth=depth)
    table = scorer.results()
    rec = np.stack([table[k] for k in ("mse", "psnr", "ssim", "depth_max")], axis=1)
    assert table["frames"] == 53
    assert rec[a].tobytes() == rec[b].tobytes() == rec[c].tobytes()
    assert len({r.tobytes() for r in rec}) == 51


def test_no_allocation_per_frame_and_batched_results(device):
    from quadraturefields_amd import metrics
    h, w, f = 96, 120, 2
    g = torch.Generator(device=device).manual_seed(5)
    truth = torch.rand(h, w, 3, generator=g, device=device)
    frames = [(torch.rand(h * f, w * f, 3, generator=g, device=device) * 0.2 + 0.4,
               torch.rand(h * f, w * f, generator=g, device=device)) for _ in range(32)]
    scorer = metrics.FrameScorer(h, w, up_sample=f, capacity=32, device=device)
    scorer.score(frames[0][0], truth, depth=frames[0][1], images=True)
    scorer.reset()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for rgb, depth in frames:
        scorer.score(rgb, truth, depth=depth, images=True)
    assert torch.cuda.memory_allocated() == before
    res = scorer.results()
    assert res["frames"] == 32 and res["psnr"].dtype == np.float64 and res["psnr"].shape == (32,)
    single = metrics.FrameScorer(h, w, up_sample=f, capacity=1, device=device)
    for i, (rgb, depth) in enumerate(frames):
        single.reset()
        single.score(rgb, truth, depth=depth)
        one = single.results()
        for k in ("mse", "psnr", "ssim", "depth_max"):
            assert one[k][0] == res[k][i], (k, i)
        small = single.last_small()[0]
        assert float(metrics.ssim(small, truth)) == res["ssim"][i] and float(metrics.psnr(small, truth)) == res["psnr"][i]
    assert res["psnr_avg"] == sum(res["psnr"].tolist()) / 32 and res["ssim_avg"] == sum(res["ssim"].tolist()) / 32


def test_real_frame(device, scored, mean_bar):
    """The 800x800 synthetic bench frame at up_sample 2 against the up_sample 1 frame of a perturbed field."""
    from quadraturefields_amd import metrics, synthetic
    from quadraturefields_amd.mesh_utils import MeshIntersection, make_camera
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceField
    from quadraturefields_amd.render import FrameRenderer, area_downsample, psnr
    size, f, log2_t = 800, 2, 19
    mesh = synthetic.shell_mesh(n_shells=12, subdivisions=6, seed=42)
    mi = MeshIntersection(mesh, simplify_mesh=False, scale=1.0, num_intersections=25, render_step_size=5e-3, device=device)

    def field_of(perturbed):
        field = NGPRadianceField(aabb=[-1.5] * 3 + [1.5] * 3, log2_hashmap_size=log2_t)
        n_rows = field.mlp_base.grid.n_rows
        state = synthetic.seeded_ngp_state(log2_t, n_rows, seed=42)
        field.load_state_dict(synthetic.perturbed_ngp_state(state, n_rows) if perturbed else state, strict=False)
        return field.to(device)

    c2w, focal = synthetic.orbit_cameras(1, seed=42)[0], synthetic.lego_focal(size)
    o, d = synthetic.camera_rays(c2w, focal, size, size, device=device)
    pixels = FrameRenderer(mi, field_of(True)).render(o, d, camera=make_camera(c2w, focal, size, size))[0]
    o, d = synthetic.camera_rays(c2w, focal * f, size * f, size * f, device=device)
    rgb, _, depth, n = FrameRenderer(mi, field_of(False)).render(o, d, camera=make_camera(c2w, focal * f, size * f, size * f))
    assert n > 0
    scorer = metrics.FrameScorer(size, size, up_sample=2.0, device=device)
    scorer.score(rgb, pixels, depth=depth, images=True)
    res = scorer.results()
    small = scorer.last_small()[0]
    # PSNR: render.psnr (fp64 on the fp32 images) of render.area_downsample's output
    down = area_downsample(rgb.reshape(size * f, size * f, 3), f)
    s = Scored()
    s.render, s.truth, s.f = rgb.reshape(size * f, size * f, 3).cpu().numpy(), pixels.reshape(size, size, 3).cpu().numpy(), f
    mse64, bar = _mse_bounds(s)
    mse_torch = float(torch.mean((down.double() - pixels.reshape(size, size, 3).double()) ** 2))
    print(f"real frame: psnr {res['psnr'][0]:.9f} render.psnr {psnr(down, pixels.reshape(size, size, 3)):.9f} "
          f"mse {res['mse'][0]:.12g} mse64 {mse64:.12g} bar {bar:.3e}")
    assert 10.0 < res["psnr"][0] < 60.0
    assert abs(res["mse"][0] - mse_torch) <= 2 * bar          # both sides within `bar` of the fp64 value
    lo, hi = -10.0 * math.log10(mse_torch + 2 * bar), -10.0 * math.log10(mse_torch - 2 * bar)
    assert lo <= res["psnr"][0] <= hi and lo <= psnr(down, pixels.reshape(size, size, 3)) <= hi
    # SSIM: the fp64 reference on the downloaded frames
    _, ssim64 = ref.ssim_torchmetrics(small.cpu(), s.truth, torch.float64)
    print(f"real frame: ssim {res['ssim'][0]:.12f} ssim64 {ssim64:.12f} bar {mean_bar:.3e}")
    assert 0.0 < res["ssim"][0] < 1.0 and abs(res["ssim"][0] - ssim64) <= mean_bar
    # ... and the class the scripts use, called as train_finetune.py:460, 633-635 call it
    test_ssim = metrics.StructuralSimilarityIndexMeasure(data_range=1).cuda()
    test_ssim(small.permute(2, 0, 1).unsqueeze(0), pixels.reshape(size, size, 3).permute(2, 0, 1).unsqueeze(0))
    value = test_ssim.compute()
    test_ssim.reset()
    assert value.item() == res["ssim"][0]
    rgb8, err8, depth8 = scorer.last_images()
    assert int(depth8.max()) == 255 and int(err8.max()) > 0 and rgb8.shape == (size, size, 3)


def test_evaluate_synthetic_example(device, tmp_path):
    from PIL import Image
    out = str(tmp_path / "eval")
    env = dict(os.environ, PYTHONPATH=ROOT)
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "evaluate_synthetic.py"), out, "--size", "200",
                           "--views", "3", "--shells", "4", "--subdivisions", "4", "--log2_hashmap_size", "15"],
                          env=env, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-2000:]
    res = json.load(open(os.path.join(out, "results.json")))
    assert "lpips" not in res and len(res["psnrs"]) == 3
    assert math.isfinite(res["psnr"]) and 0.0 < res["ssim"] < 1.0
    for i in range(3):
        for name, mode in (("rgb_test_after", "RGB"), ("rgb_error_after", "RGB"), ("depth_after", "L")):
            im = Image.open(os.path.join(out, f"{name}_{i}.png"))
            assert im.size == (200, 200) and im.mode == mode
