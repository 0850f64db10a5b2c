"""CPU: the SSIM definition the frame-metrics kernels are tested against, stated twice, and the argument checks of
``quadraturefields_amd.metrics`` that need no device."""
import numpy as np
import pytest
import torch

from tests import frame_metrics_reference as ref


@pytest.fixture(scope="module")
def f1_cases():
    return [(name,) + ref.case(name, 1)[:2] for name in ref.CASES]


def test_conv_and_scipy_statements_agree(f1_cases):
    """Two independent fp64 statements of one definition: torchmetrics' padded depthwise conv2d with the crop, and two
    1-D correlations on the valid region.  The frame values agree to 1e-12.  A single window may differ by more: the two
    statements add a window's 121 products in different orders, so a moment of size <= 1.5 (the render is not clamped)
    differs by at most 120 * 2^-53 * 1.5, and SSIM turns an error of a sigma term into at most 2 / c2 times as much
    (its denominator holds sigma_p^2 + sigma_t^2 + c2 >= c2)."""
    window_bar = 2.0 / ref.C2 * 120 * 2.0 ** -53 * 1.5
    for name, p, t in f1_cases:
        m_conv, s_conv = ref.ssim_torchmetrics(p, t, torch.float64)
        m_sp, s_sp = ref.ssim_scipy(p, t)
        assert m_conv.shape == (p.shape[0] - 10, p.shape[1] - 10, 3), name
        assert np.abs(m_conv.numpy() - m_sp).max() <= window_bar, name
        assert abs(s_conv - s_sp) <= 1e-12, name


def test_reflect_padding_never_reaches_a_kept_value(f1_cases):
    """torchmetrics pads by 5 and crops by 5: the kept windows lie inside the image, so the padding mode is dead."""
    for name, p, t in f1_cases:
        m_reflect, _ = ref.ssim_torchmetrics(p, t, torch.float64, padding="reflect")
        m_zero, _ = ref.ssim_torchmetrics(p, t, torch.float64, padding="constant")
        assert torch.equal(m_reflect, m_zero), name


def test_identical_and_constant_images():
    p, t, _ = ref.case("identical", 1)
    m, s = ref.ssim_torchmetrics(p, t, torch.float64)
    assert s == 1.0 and bool((m == 1.0).all())
    p, t, _ = ref.case("constant", 1)
    a, b = float(p[0, 0, 0]), float(t[0, 0, 0])
    closed = (2 * a * b + ref.C1) / (a * a + b * b + ref.C1)
    m, s = ref.ssim_torchmetrics(p, t, torch.float64)
    assert abs(s - closed) <= 1e-12 and np.abs(m.numpy() - closed).max() <= 1e-12
    assert abs(ref.ssim_scipy(p, t)[1] - closed) <= 1e-12


def test_upsampled_cases_average_back():
    """The f = 2, 3 inputs are the f = 1 case plus sub-pixel detail of zero block mean."""
    for name in ("odd133x77", "identical"):
        base = ref.case(name, 1)
        for f in (2, 3):
            up = ref.case(name, f)
            assert up[0].shape == (base[0].shape[0] * f, base[0].shape[1] * f, 3) and up[2].shape == up[0].shape[:2]
            assert np.abs(ref.box_downsample64(up[0], f) - base[0]).max() <= 1e-6
            assert np.array_equal(up[1], base[1])


@pytest.mark.parametrize("up_sample", [1.5, 0, 5, -1, "2", None, 2.0000001])
def test_scorer_refuses_a_bad_factor_before_allocating(up_sample):
    """No device here: a constructor that allocated first would fail with another error."""
    from quadraturefields_amd.metrics import FrameScorer
    with pytest.raises(ValueError):
        FrameScorer(64, 64, up_sample=up_sample)


@pytest.mark.parametrize("size", [(10, 64), (64, 10), (0, 0), (64.5, 64)])
def test_scorer_refuses_a_bad_size_before_allocating(size):
    from quadraturefields_amd.metrics import FrameScorer
    with pytest.raises(ValueError):
        FrameScorer(*size, up_sample=2.0)


def test_metrics_refuse_host_tensors():
    """Like every entry of the package: host tensors stop at ``_C.ptr``, nothing is computed on the CPU."""
    from quadraturefields_amd import metrics
    a, b = torch.rand(32, 32, 3), torch.rand(32, 32, 3)
    with pytest.raises(RuntimeError):
        metrics.ssim(a, b)
    with pytest.raises(RuntimeError):
        metrics.psnr(a, b)
    m = metrics.StructuralSimilarityIndexMeasure(data_range=1).cuda()
    with pytest.raises(RuntimeError):
        m(a.permute(2, 0, 1).unsqueeze(0), b.permute(2, 0, 1).unsqueeze(0))


def test_ssim_class_names_what_it_supports():
    from quadraturefields_amd.metrics import StructuralSimilarityIndexMeasure
    with pytest.raises(NotImplementedError, match="data_range=1"):
        StructuralSimilarityIndexMeasure(data_range=255.0)
    with pytest.raises(NotImplementedError, match="data_range=1"):
        StructuralSimilarityIndexMeasure(data_range=1.0, kernel_size=7)
    m = StructuralSimilarityIndexMeasure(data_range=1.0)
    with pytest.raises(NotImplementedError, match=r"\[1, 3, H, W\]"):
        m(torch.zeros(2, 3, 32, 32), torch.zeros(2, 3, 32, 32))
    with pytest.raises(NotImplementedError, match="float32"):
        m(torch.zeros(1, 3, 32, 32, dtype=torch.float64), torch.zeros(1, 3, 32, 32, dtype=torch.float64))


def test_entry_points_refuse_bad_arguments_before_any_launch(lib):
    """qf_frame_score validates sizes on the host: no device is needed to be refused."""
    import ctypes
    assert lib.qf_frame_score_scratch_bytes(10, 64) == -1 and lib.qf_frame_score_scratch_bytes(64, 10) == -1
    # one partial record (3 doubles) per 32x16 tile of windows and channel
    assert lib.qf_frame_score_scratch_bytes(800, 800) == 25 * 50 * 3 * 3 * 8
    assert lib.qf_frame_score_scratch_bytes(11, 11) == 3 * 3 * 8
    p = ctypes.c_void_p(256)            # never dereferenced: every call below fails validation
    n = lib.qf_frame_score_scratch_bytes(64, 64)
    ok = dict(rgb=p, rh=128, rw=128, depth=None, pixels=p, h=64, w=64, f=2, small=None, dsmall=None, smap=None, table=p,
              slot=0, cap=1, scratch=p, sbytes=n, stream=None)
    bad = [dict(f=0), dict(f=5), dict(rh=127), dict(rw=192), dict(h=10, rh=20), dict(slot=1), dict(slot=-1),
           dict(sbytes=n - 1), dict(rgb=None), dict(pixels=None), dict(table=None), dict(dsmall=p)]
    for change in bad:
        a = dict(ok, **change)
        assert lib.qf_frame_score(*a.values()) == -1, change
    assert lib.qf_frame_images_u8(None, p, None, p, 64, 64, p, p, None, None) == -1
    assert lib.qf_frame_images_u8(p, p, None, p, 64, 64, p, p, p, None) == -1
