"""Training regularisers of the stage-1 script: the distortion loss on the gfx950 kernel and the closed-form ones.

``flatten_eff_distloss`` / ``eff_distloss`` / ``eff_distloss_native`` restate the ``torch_efficient_distloss`` package
(imported at ``examples/train_finetune.py:33`` and ``examples/train_ngp_nerf_sg_occ.py:27``) from its published
algorithm; ``regulariser`` is the ``--reg_type`` chain of ``examples/train_ngp_nerf_sg_occ.py:315-334``.

The distortion loss is the ORDERED sum over the samples of a ray in their stored order,

    L_ray = sum_i sum_{j<i} 2 w_i w_j (m_i - m_j) + (1/3) sum_i w_i^2 interval_i,     loss = sum_rays L_ray / n_rays,

which is the Mip-NeRF-360 definition (``|m_i - m_j|``) exactly when ``m`` is nondecreasing along every ray.  One launch of
``qf_distortion_loss`` computes the loss and ``dloss/dw``; the backward is ``grad_out * saved``.  Gradients flow to ``w``
only.  There is no host wait and no CPU fallback.
"""
from typing import Optional, Union

import torch
from torch import Tensor
from torch.autograd.function import once_differentiable

from . import _C

_workspaces = {}


def _workspace(device: torch.device) -> Tensor:
    """The kernel's ticket + partials, zeroed once per (device, stream): launches of one stream run in order and each
    leaves the ticket at 0, so the block is reused without a memset launch."""
    key = (device.index, _C.raw_stream())
    ws = _workspaces.get(key)
    if ws is None:
        ws = _workspaces[key] = torch.zeros((_C.DISTORTION_WORKSPACE_BYTES,), dtype=torch.uint8, device=device)
    return ws


def _typed(t, name: str, dtype) -> Tensor:
    if not isinstance(t, Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    return t


def _arguments(w, m, interval, ray_id=None):
    """Every type, then every shape, then devices and strides, so that a wrong argument is named for what is wrong with
    it wherever the tensors live; returns (w, m, interval tensor or None, interval constant, ray_id)."""
    w, m = _typed(w, "w", torch.float32), _typed(m, "m", torch.float32).detach()
    named = [("w", w), ("m", m)]
    interval_t, interval_c = None, 0.0
    if isinstance(interval, Tensor):
        interval_t = _typed(interval, "interval", torch.float32).detach()
        named.append(("interval", interval_t))
    elif isinstance(interval, (int, float)):
        interval_c = float(interval)
    else:
        raise TypeError(f"interval must be a tensor or a float, got {type(interval).__name__}")
    if ray_id is not None:
        named.append(("ray_id", _typed(ray_id, "ray_id", torch.int64)))
    for name, t in named:
        if t.shape != w.shape:
            raise ValueError(f"{name} must have the shape of w {tuple(w.shape)}, got {tuple(t.shape)}")
    for name, t in named:
        if not t.is_cuda:
            raise RuntimeError(f"{name} is a host tensor: quadraturefields_amd kernels need tensors on the HIP device "
                               "(no CPU fallback)")
        if t.device != w.device:
            raise ValueError(f"{name} is on {t.device}, w on {w.device}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous (a strided view would be copied on every step: pass "
                             ".contiguous())")
    return w, m, interval_t, interval_c, ray_id


def _launch(w: Tensor, m: Tensor, interval_t: Optional[Tensor], interval_c: float, ray_id: Optional[Tensor], count: int,
            n_rays: int, want_grad: bool):
    n = w.numel()
    loss = torch.empty((), dtype=torch.float32, device=w.device)
    grad = torch.empty_like(w) if want_grad else None
    with torch.cuda.device(w.device):
        _C.check(_C.lib().qf_distortion_loss(
            _C.ptr(w), _C.ptr(m), _C.ptr(interval_t), interval_c, _C.ptr(ray_id), count, n, n_rays, _C.ptr(loss),
            _C.ptr(grad), _C.ptr(_workspace(w.device)), _C.stream()), "qf_distortion_loss")
    return loss, grad


class _DistortionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, w, m, interval_t, interval_c, ray_id, count, n_rays, want_grad):
        loss, grad = _launch(w, m, interval_t, interval_c, ray_id, count, n_rays, want_grad)
        if want_grad:
            ctx.save_for_backward(grad)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        (grad,) = ctx.saved_tensors
        return grad_out * grad, None, None, None, None, None, None, None


def _wants_grad(w: Tensor) -> bool:
    """Whether autograd records this call.  (``ctx.needs_input_grad`` inside the Function is no substitute: it follows
    ``w.requires_grad`` under ``no_grad`` too.)  When it does not, the kernel gets no gradient buffer and skips the stores."""
    return torch.is_grad_enabled() and w.requires_grad


def flatten_eff_distloss(w: Tensor, m: Tensor, interval: Union[Tensor, float], ray_id: Tensor,
                         n_rays: Optional[int] = None) -> Tensor:
    """Distortion loss of packed samples: ``w``, ``m`` [n] float32, ``interval`` [n] float32 or a float, ``ray_id`` [n]
    int64, nondecreasing and >= 0.  ``n_rays`` (extension): the number of rays the sum is divided by; by default
    ``ray_id[-1] + 1``, read on the device.  Rays without samples count.  Returns a 0-d tensor, differentiable in ``w``."""
    w, m, interval_t, interval_c, ray_id = _arguments(w, m, interval, ray_id)
    if w.dim() != 1:
        raise ValueError(f"w must be flattened (n,), got {tuple(w.shape)}")
    if n_rays is None:
        n_rays = 0
    elif int(n_rays) <= 0:
        raise ValueError(f"n_rays must be positive, got {n_rays}")
    return _DistortionFn.apply(w, m, interval_t, interval_c, ray_id, 0, int(n_rays), _wants_grad(w))


def eff_distloss(w: Tensor, m: Tensor, interval: Union[Tensor, float]) -> Tensor:
    """Distortion loss of batched rays ``[..., N]``: per-ray sums, mean over the rays (the same kernel, told the uniform
    sample count instead of ray ids)."""
    w, m, interval_t, interval_c, _ = _arguments(w, m, interval)
    if w.dim() < 1:
        raise ValueError("w must have shape [..., N]")
    count = w.shape[-1]
    n_rays = w.numel() // count if count else 0
    return _DistortionFn.apply(w, m, interval_t, interval_c, None, count, n_rays, _wants_grad(w))


eff_distloss_native = eff_distloss


def ray_distortion(weights: Tensor, t_starts: Tensor, t_ends: Tensor, ray_indices: Tensor,
                   n_rays: Optional[int] = None) -> Tensor:
    """The distortion loss of marched samples with their true midpoints and lengths: ``m = (t_starts + t_ends) / 2``,
    ``interval = t_ends - t_starts``.  The midpoints ascend along a ray by construction, so this is the Mip-NeRF-360
    loss; new code should call this form."""
    t_starts, t_ends = t_starts.detach().reshape(-1), t_ends.detach().reshape(-1)
    return flatten_eff_distloss(weights.reshape(-1), (t_starts + t_ends) / 2.0, t_ends - t_starts, ray_indices.reshape(-1),
                                n_rays)


# ------------------------------------------------------------------------------------------- stage-1 regularisers
class _ExclusiveSumFn(torch.autograd.Function):
    """Per-ray exclusive prefix sum with its adjoint, the exclusive SUFFIX sum of the incoming gradient
    (ray total - exclusive prefix - own entry): both directions on the scan and accumulate kernels."""

    @staticmethod
    def forward(ctx, x, info, ray_indices):
        from .field_rendering import exclusive_sum
        ctx.save_for_backward(info, ray_indices)
        return exclusive_sum(x, info)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        from .field_rendering import _accumulate, exclusive_sum
        info, ray_indices = ctx.saved_tensors
        g = _C.f32c(g)
        total = _accumulate(g, None, info, info.shape[0])[:, 0]
        return total[ray_indices] - exclusive_sum(g, info) - g, None, None


def differentiable_weights(extras, n_rays: int) -> Tensor:
    """The compositing weights of ``render_image_with_occgrid``'s ``extras`` as a function of ``extras["sigmas"]``.
    The differentiable route of ``rendering`` returns its weights detached (the finetune step only reads them); the
    stage-1 regularisers on the weights (entropy, lol, distortion) need their gradient, so they are rebuilt here:
    ``w = exp(-excl_sum(sigma dt)) (1 - exp(-sigma dt))``."""
    from .field_rendering import pack_info
    w, sigmas = extras["weights"].reshape(-1), extras["sigmas"].reshape(-1)
    if w.requires_grad or not (torch.is_grad_enabled() and sigmas.requires_grad):
        return w
    ray_indices = _C.i64c(extras["ray_indices"].reshape(-1))
    tau = sigmas * (extras["t_ends"] - extras["t_starts"]).detach().reshape(-1)
    excl = _ExclusiveSumFn.apply(_C.f32c(tau), pack_info(ray_indices, int(n_rays)), ray_indices)
    return torch.exp(-excl) * (1.0 - torch.exp(-tau))


REG_TYPES = ("occ", "entropy", "cauchy", "both", "lol", "none", "distortion")


def regulariser(reg_type: str, *, acc: Tensor, extras, rays, o_lambda: float, c_lambda: float,
                render_step_size: float) -> Tensor:
    """``loss_reg`` of ``examples/train_ngp_nerf_sg_occ.py:315-334`` for ``--reg_type``: ``acc`` and ``extras`` as
    ``render_image_with_occgrid`` returns them, ``rays`` the rays it rendered.  The formulas are the reference's, the
    ``1e-10`` / ``1e-7`` guards included; ``distortion`` takes ``m = |p . d|`` at the sample midpoints with the constant
    interval ``render_step_size`` (the ordered sum: ``|p . d|`` is V-shaped for a camera that looks past the origin)."""
    if reg_type not in REG_TYPES:
        raise ValueError(f"unknown reg_type {reg_type!r}; one of {REG_TYPES}")
    acc = acc.squeeze()
    occ = lambda: (o_lambda * (-acc * torch.log(acc + 1e-10))).mean()
    cauchy = lambda: c_lambda * (torch.log(1 + extras["sigmas"] ** 2)).mean()
    if reg_type == "occ":
        return occ()
    if reg_type == "cauchy":
        return cauchy()
    if reg_type == "both":
        return occ() + cauchy()
    if reg_type == "none":
        return torch.zeros(1, device=acc.device).mean()
    viewdirs = rays.viewdirs.reshape(-1, 3)
    weights = differentiable_weights(extras, viewdirs.shape[0])
    if reg_type == "entropy":
        return (o_lambda * (-weights * torch.log(weights + 1e-7))).mean()
    if reg_type == "lol":
        return (o_lambda * (torch.log(torch.exp(-weights) + torch.exp(-torch.abs(1 - weights))))).mean()
    index_ray = extras["ray_indices"].reshape(-1)
    dirs = viewdirs.to(weights.device)[index_ray]
    mids = (extras["t_starts"] + extras["t_ends"]).reshape(-1)[..., None] / 2.0
    positions = extras["t_origins"][index_ray] + dirs * mids
    m = torch.abs((positions * dirs).sum(1)).detach()
    return o_lambda * flatten_eff_distloss(weights.contiguous(), _C.f32c(m), float(render_step_size), _C.i64c(index_ray))
