"""Frame scores on the device: the tail of the reference's evaluation loops (train_finetune.py:620-667) -- INTER_AREA
down-sample, PSNR, SSIM as torchmetrics' ``StructuralSimilarityIndexMeasure(data_range=1)`` computes it, and the three
``uint8`` images the scripts write -- through ``qf_frame_score`` / ``qf_frame_images_u8`` (csrc/frame_metrics.hip).

``FrameScorer`` scores a run of frames without a host wait per frame: every ``score`` lands in one slot of a device
table and ``results()`` is the one synchronisation.  LPIPS is not here (it needs VGG weights).
"""
from typing import Optional

import numpy as np
import torch

from . import _C

_RECORD = 4            # fp64 values per slot: mse, psnr, ssim, depth_max
_WINDOW = 11           # torchmetrics' default kernel_size; an image edge must hold one window


def _factor(up_sample) -> int:
    if isinstance(up_sample, bool) or not isinstance(up_sample, (int, float, np.integer, np.floating)):
        raise ValueError(f"up_sample must be an integer in 1..4, got {up_sample!r}")
    if float(up_sample) != int(up_sample):
        raise ValueError(f"up_sample must be integral (the box average of INTER_AREA), got {up_sample!r}")
    f = int(up_sample)
    if not 1 <= f <= 4:
        raise ValueError(f"up_sample must be in 1..4, got {f}")
    return f


def _check_size(height, width):
    if int(height) != height or int(width) != width or height < _WINDOW or width < _WINDOW:
        raise ValueError(f"height and width must be integers >= {_WINDOW} (one 11x11 SSIM window), got {height}x{width}")
    return int(height), int(width)


def _image(t: torch.Tensor, height: int, width: int, channels: int, what: str) -> torch.Tensor:
    """``t`` as [height, width(, 3)] without a copy: [N, C], [N] and [H, W, C] inputs are views of the same memory."""
    _C.ptr(t, torch.float32)                         # host tensors, other dtypes and strided views are refused here
    n = height * width
    if channels == 3:
        ok = tuple(t.shape) in ((n, 3), (height, width, 3))
    else:
        ok = tuple(t.shape) in ((n,), (n, 1), (height, width), (height, width, 1))
    if not ok:
        raise ValueError(f"{what}: shape {tuple(t.shape)} is not a {height}x{width} image")
    return t


class FrameScorer:
    """Scores rendered frames against ground truth on the device.

    ``height, width``: the GROUND-TRUTH size; the render is ``up_sample`` times larger each way (an int or an integral
    float in 1..4, as the scripts' ``--up_sample 2.0``).  Owns the results table (``capacity`` frames), the partial-sum
    scratch and the output buffers: nothing is allocated per frame.
    """

    def __init__(self, height: int, width: int, up_sample=1, capacity: int = 256, device="cuda"):
        self.factor = _factor(up_sample)
        self.height, self.width = _check_size(height, width)
        if int(capacity) != capacity or capacity < 1:
            raise ValueError(f"capacity must be a positive integer, got {capacity!r}")
        self.capacity = int(capacity)
        self.device = _C.resolve_device(device)
        if self.device.type != "cuda":
            raise RuntimeError("FrameScorer needs the HIP device (no CPU fallback)")
        scratch_bytes = int(_C.lib().qf_frame_score_scratch_bytes(self.height, self.width))
        if scratch_bytes < 0:
            raise ValueError(f"unsupported frame size {self.height}x{self.width}")
        h, w, dev = self.height, self.width, self.device
        self._table = torch.zeros((self.capacity, _RECORD), dtype=torch.float64, device=dev)
        self._scratch = torch.empty((scratch_bytes,), dtype=torch.uint8, device=dev)
        self._rgb_small = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
        self._depth_small = torch.empty((h, w), dtype=torch.float32, device=dev)
        self._ssim_map = None            # [h-10, w-10, 3]; allocated by the first score(..., ssim_map=True)
        self._images = None              # rgb8, err8, depth8; allocated by the first score(..., images=True)
        self._count = 0
        self._last = {"depth": False, "images": False, "ssim_map": False}

    def __len__(self) -> int:
        return self._count

    def reset(self) -> None:
        """Forget the scored frames (the buffers stay)."""
        self._count = 0
        self._last = {"depth": False, "images": False, "ssim_map": False}

    @torch.no_grad()
    def score(self, rgb: torch.Tensor, pixels: torch.Tensor, depth: Optional[torch.Tensor] = None, images: bool = False,
              ssim_map: bool = False) -> int:
        """Enqueue one frame on the current stream and return its slot; never waits for the device.

        ``rgb``: fp32 [N, 3] or [H*f, W*f, 3], the render as the renderers return it, unclamped; ``pixels``: fp32 [N, 3]
        or [H, W, 3]; ``depth``: fp32 [N], [N, 1] or [H*f, W*f].  ``images``: also write the three uint8 images
        (``last_images``); ``ssim_map``: also keep the per-window SSIM values (``last_ssim_map``)."""
        if self._count >= self.capacity:
            raise RuntimeError(f"FrameScorer is full ({self.capacity} frames): call results() and reset(), or raise capacity")
        h, w, f = self.height, self.width, self.factor
        rgb = _image(rgb, h * f, w * f, 3, "rgb")
        pixels = _image(pixels, h, w, 3, "pixels")
        if depth is not None:
            depth = _image(depth, h * f, w * f, 1, "depth")
        for t in (rgb, pixels, depth):
            if t is not None and t.device != self.device:
                raise ValueError(f"tensor on {t.device}, scorer on {self.device}")
        if ssim_map and self._ssim_map is None:
            self._ssim_map = torch.empty((h - 10, w - 10, 3), dtype=torch.float32, device=self.device)
        if images and self._images is None:
            self._images = (torch.empty((h, w, 3), dtype=torch.uint8, device=self.device),
                            torch.empty((h, w, 3), dtype=torch.uint8, device=self.device),
                            torch.zeros((h, w), dtype=torch.uint8, device=self.device))
        slot = self._count
        lib, stream = _C.lib(), _C.stream()
        _C.check(lib.qf_frame_score(_C.ptr(rgb), h * f, w * f, _C.ptr(depth), _C.ptr(pixels), h, w, f, _C.ptr(self._rgb_small),
                                    _C.ptr(self._depth_small) if depth is not None else None,
                                    _C.ptr(self._ssim_map) if ssim_map else None, _C.ptr(self._table), slot, self.capacity,
                                    _C.ptr(self._scratch), self._scratch.numel(), stream), "qf_frame_score")
        if images:
            rgb8, err8, depth8 = self._images
            _C.check(lib.qf_frame_images_u8(_C.ptr(self._rgb_small), _C.ptr(pixels),
                                            _C.ptr(self._depth_small) if depth is not None else None,
                                            _C.ptr(self._table[slot]), h, w, _C.ptr(rgb8), _C.ptr(err8),
                                            _C.ptr(depth8) if depth is not None else None, stream), "qf_frame_images_u8")
        self._count = slot + 1
        self._last = {"depth": depth is not None, "images": images, "ssim_map": ssim_map}
        return slot

    def last_small(self):
        """(rgb_small [H, W, 3], depth_small [H, W] or None) of the most recent ``score``: views of reused buffers, valid
        until the next ``score``."""
        if self._count == 0:
            raise RuntimeError("no frame has been scored")
        return self._rgb_small, (self._depth_small if self._last["depth"] else None)

    def last_images(self):
        """(rgb8 [H, W, 3], err8 [H, W, 3], depth8 [H, W] or None), uint8 on the device, of the most recent
        ``score(..., images=True)``: views of reused buffers, valid until the next ``score``."""
        if not self._last["images"]:
            raise RuntimeError("the most recent score() was not called with images=True")
        rgb8, err8, depth8 = self._images
        return rgb8, err8, (depth8 if self._last["depth"] else None)

    def last_ssim_map(self) -> torch.Tensor:
        """fp32 [H-10, W-10, 3] SSIM of every 11x11 window of the most recent ``score(..., ssim_map=True)``: a view of a
        reused buffer, valid until the next ``score``."""
        if not self._last["ssim_map"]:
            raise RuntimeError("the most recent score() was not called with ssim_map=True")
        return self._ssim_map

    def record(self, slot: int) -> torch.Tensor:
        """The slot's (mse, psnr, ssim, depth_max) as an fp64 [4] device tensor (a view of the table; no wait)."""
        if not 0 <= slot < self._count:
            raise IndexError(f"slot {slot} of {self._count} scored frames")
        return self._table[slot]

    def results(self) -> dict:
        """The one synchronisation: per-frame ``mse``, ``psnr``, ``ssim``, ``depth_max`` as numpy fp64 arrays, and
        ``psnr_avg`` / ``ssim_avg`` as the scripts compute them (``sum(psnrs) / len(psnrs)``)."""
        table = self._table[:self._count].cpu().numpy()
        out = {"frames": self._count, "mse": table[:, 0].copy(), "psnr": table[:, 1].copy(), "ssim": table[:, 2].copy(),
               "depth_max": table[:, 3].copy()}
        n = self._count
        out["psnr_avg"] = sum(out["psnr"].tolist()) / n if n else float("nan")
        out["ssim_avg"] = sum(out["ssim"].tolist()) / n if n else float("nan")
        return out


def _score_pair(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """fp64 [4] device record of one pair of [H, W, 3] fp32 images at factor 1."""
    _C.ptr(a, torch.float32)
    _C.ptr(b, torch.float32)
    if a.dim() != 3 or a.shape[2] != 3 or a.shape != b.shape:
        raise ValueError(f"expected two [H, W, 3] images of one size, got {tuple(a.shape)} and {tuple(b.shape)}")
    h, w = _check_size(a.shape[0], a.shape[1])
    if a.device != b.device:
        raise ValueError("the two images are on different devices")
    scratch_bytes = int(_C.lib().qf_frame_score_scratch_bytes(h, w))
    if scratch_bytes < 0:
        raise ValueError(f"unsupported image size {h}x{w}")
    with torch.cuda.device(a.device):
        table = torch.empty((_RECORD,), dtype=torch.float64, device=a.device)
        scratch = torch.empty((scratch_bytes,), dtype=torch.uint8, device=a.device)
        _C.check(_C.lib().qf_frame_score(_C.ptr(a), h, w, None, _C.ptr(b), h, w, 1, None, None, None, _C.ptr(table), 0, 1,
                                         _C.ptr(scratch), scratch_bytes, _C.stream()), "qf_frame_score")
    return table


def ssim(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """SSIM (torchmetrics' definition, data_range 1) of two fp32 [H, W, 3] device images: a 0-dim fp64 device tensor."""
    return _score_pair(a, b)[2]


def psnr(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """-10 log10(mse) of two fp32 [H, W, 3] device images: a 0-dim fp64 device tensor (no host wait)."""
    return _score_pair(a, b)[1]


class StructuralSimilarityIndexMeasure:
    """The part of torchmetrics' class the reference's scripts use (train_finetune.py:460, 633-635):
    ``StructuralSimilarityIndexMeasure(data_range=1).cuda()``, ``metric(preds, target)`` on fp32 [1, 3, H, W] device
    tensors, ``compute()``, ``reset()``.  Defaults only: Gaussian 11x11 windows, sigma 1.5, k1 0.01, k2 0.03, mean."""

    def __init__(self, data_range=1.0, **kwargs):
        if kwargs:
            raise NotImplementedError(f"StructuralSimilarityIndexMeasure: only data_range=1 with torchmetrics' defaults is "
                                      f"supported, got {sorted(kwargs)}")
        if data_range is None or isinstance(data_range, (tuple, list)) or float(data_range) != 1.0:
            raise NotImplementedError(f"StructuralSimilarityIndexMeasure: only data_range=1 is supported, got {data_range!r}")
        self._sum = None
        self._total = 0

    def to(self, *args, **kwargs):
        return self

    def cuda(self, device=None):
        return self

    def update(self, preds: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        for name, t in (("preds", preds), ("target", target)):
            if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.shape[0] != 1 or t.shape[1] != 3:
                raise NotImplementedError(f"StructuralSimilarityIndexMeasure: {name} must be [1, 3, H, W] (one RGB image), "
                                          f"got {tuple(getattr(t, 'shape', ()))}")
            if t.dtype != torch.float32:
                raise NotImplementedError(f"StructuralSimilarityIndexMeasure: {name} must be float32, got {t.dtype}")
        # [1, 3, H, W] -> [H, W, 3]: free for the scripts' permuted views of channel-last images
        value = ssim(preds[0].permute(1, 2, 0).contiguous(), target[0].permute(1, 2, 0).contiguous())
        self._sum = value if self._sum is None else self._sum + value
        self._total += 1
        return value

    __call__ = update
    forward = update

    def compute(self) -> torch.Tensor:
        if self._total == 0:
            raise RuntimeError("StructuralSimilarityIndexMeasure.compute() before any update")
        return self._sum / self._total

    def reset(self) -> None:
        self._sum = None
        self._total = 0
