"""Image-level renderers of the mesh-quadrature path on the gfx950 kernels.

Mirrors the hot-path functions of ``examples/utils.py`` of the reference with the same names, arguments and
return tuples: ``derive_properties`` (:863-898), ``render_image_finetune_with_occgrid`` (:465-607),
``render_image_fit_sg_with_occgrid`` (:610-730), ``render_image_bake_texture_images_with_occgrid`` (:998-1095),
``render_image_with_occgrid`` (:65-172), ``render_image_with_occgrid_test`` (:176-350),
``render_image_field_with_occgrid`` (:353-462), ``compress_sigma`` /
``inverse_of_compressed_sigma`` (:54-63), plus ``generate_splits`` (``examples/train_finetune.py:419-439``).
Every tensor stays on the device; the reference's 160 000-sample Python batch loops, its
``torch.cuda.empty_cache()`` calls and its host round trips (np.lexsort, trimesh barycentrics) are gone,
the results do not depend on any chunk size.
"""
import math
import random
from typing import Optional

import numpy as np
import torch

from . import _C
from .baking import QuantisedVertexFeatures, VertexBakedFeatures
from .datasets.utils import Rays, namedtuple_map
from .field import Field as _Field
from .mesh_utils import SampleSet, SampleWindow

NERF_SYNTHETIC_SCENES = ["chair", "drums", "ficus", "hotdog", "lego", "materials", "mic", "ship"]
# imported by both harness scripts (train_finetune.py:18, test_baking_texture_images.py:23) and only used to pick the
# unbounded-scene loader / aabb (train_finetune.py:248), which is out of scope here: the names exist, the branch does not
MIPNERF360_UNBOUNDED_SCENES = ["garden", "bicycle", "bonsai", "counter", "kitchen", "room", "stump"]


def set_random_seed(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


def compress_sigma(sigma):
    alpha = 1 - torch.exp(-sigma * 0.005)
    return torch.clip(alpha * 255, 0, 255).to(torch.uint8)


def inverse_of_compressed_sigma(alpha):
    alpha = alpha.to(torch.float32) / 255.0
    return -torch.log(1 - alpha) / 0.005


def generate_splits(data, num_rays, chunk_size=160000):
    """Windows of ``chunk_size`` rays over the packed samples (train_finetune.py:419-439).

    The reference masks every array once per window (on the CPU tensors of its DataLoader worker).  Device arrays
    whose ray ids ascend -- what every loader of the path produces (mesh_utils.py:373-381: lexsort by (depth, ray)) --
    are cut with ONE searchsorted and one host read instead: a window's samples are a contiguous slice, the splits are
    views (same values as the masked copies).  Anything else takes the masks."""
    xyzs, dirs, index_ray, ts, index_tri, origins = data
    chunks = []
    n = int(index_ray.shape[0])
    if (isinstance(data, SampleSet) and int(chunk_size) == data.window_rays and int(num_rays) == data.num_rays
            and data.cuts[-1] == n):
        # a loader item cut for exactly these windows (SubjectLoader -> sampling_raytrace_device(window_rays=)): the
        # windows' boundaries came back with the frame's own readback and the frame-wide coherent layout restarts at every
        # window -- views only, no launch, no host wait; empty windows are skipped as the reference does (:427-428)
        for a, b in zip(data.cuts[:-1], data.cuts[1:]):
            if b > a:
                chunks.append(SampleWindow(tuple(t[a:b] for t in (xyzs, dirs, index_ray, ts, index_tri, origins)),
                                           base=a, inverse=data.inverse[a:b],
                                           order=None if data.order is None else data.order[a:b],
                                           xyz_c=data.xyz_c[a:b], dirs_c=data.dirs_c[a:b], num_rays=data.num_rays))
        return chunks
    if n > 0 and index_ray.is_cuda and index_ray.dim() == 1 and index_ray.dtype == torch.int64:
        edges = torch.arange(0, int(num_rays) + int(chunk_size), int(chunk_size), dtype=torch.int64, device=index_ray.device)
        cuts = torch.searchsorted(index_ray, edges)
        ascending = (index_ray[1:] >= index_ray[:-1]).all().reshape(1).to(torch.int64)
        host = torch.cat([cuts, ascending]).tolist()
        if host[-1]:
            for a, b in zip(host[:-2], host[1:-1]):
                if b > a:
                    chunks.append(tuple(t[a:b] for t in (xyzs, dirs, index_ray, ts, index_tri, origins)))
            return chunks
    for i in range(0, num_rays, chunk_size):
        mask = (index_ray < i + chunk_size) & (index_ray >= i)
        if mask.sum() == 0:
            continue
        chunks.append(tuple(t[mask].contiguous() for t in (xyzs, dirs, index_ray, ts, index_tri, origins)))
    return chunks


_BG = {"white": _C.BG_WHITE, "black": _C.BG_BLACK}

#: SURVEY.md B-14: the reference draws ``torch.rand((S, 3))`` on the device for EVERY split it renders, evaluation included
#: (examples/utils.py:543-546: the random barycentric points of the regulariser, which evaluation then discards).  The
#: pixels do not depend on it, so the evaluation route here does not draw -- but a seeded run that interleaves training
#: and evaluation (train_finetune.py evaluates every ``eval_every`` steps) then sees a different random stream after its
#: first ``test()`` than the reference would.  True: ``render_image_finetune_with_occgrid`` draws (and drops) the same
#: tensor at evaluation, one small launch per split, and the device generator advances exactly as in the reference.
REPRODUCE_EVAL_RNG_ADVANCE = False


class _DerivePropertiesFn(torch.autograd.Function):
    """Differentiable compositing: forward = qf_derive_properties, backward = qf_derive_properties_backward
    (gradients w.r.t. per-sample colour, density and depth; the returned weights are not differentiated, the
    reference only uses them detached -- examples/field.py:246-252).

    Domain: densities in [0, +inf] with ``delta > 0`` wherever the density is infinite (``inf * 0`` is NaN in the
    forward already); ``delta = 0`` with a finite density is a sample of no weight.  The gradients are finite on all
    of it: an opaque sample has gradient 0 w.r.t. its own density, everything behind it has weight and gradients 0."""

    @staticmethod
    def forward(ctx, color, density, depths, deltas_t, delta_c, index_ray, N, mode, bk, sample_index=None):
        n = depths.shape[0]
        dev = color.device
        rgb = torch.empty((N, 3), dtype=torch.float32, device=dev)
        alpha = torch.empty((N, 1), dtype=torch.float32, device=dev)
        depth_out = torch.empty((N, 1), dtype=torch.float32, device=dev)
        weights = torch.empty((n, 1), dtype=torch.float32, device=dev)
        _C.check(_C.lib().qf_derive_properties(
            _C.ptr(color), _C.ptr(density), _C.ptr(depths), _C.ptr(deltas_t), delta_c, _C.ptr(index_ray), n, N, mode,
            _C.ptr(bk), _C.ptr(sample_index, torch.int32), _C.ptr(rgb), _C.ptr(alpha), _C.ptr(depth_out), _C.ptr(weights),
            _C.stream()), "qf_derive_properties")
        if sample_index is not None:
            ctx.mark_non_differentiable(rgb, alpha, depth_out, weights)     # the indexed form is inference only
            return rgb, alpha, depth_out, weights
        ctx.save_for_backward(color, density, depths, deltas_t, index_ray, bk)
        ctx.delta_c, ctx.mode, ctx.n_rays = delta_c, mode, N
        ctx.mark_non_differentiable(weights)
        return rgb, alpha, depth_out, weights

    @staticmethod
    def backward(ctx, g_rgb, g_alpha, g_depth, _g_weights):
        color, density, depths, deltas_t, index_ray, bk = ctx.saved_tensors
        n = color.shape[0]
        g_color = torch.empty_like(color)
        g_sigma = torch.empty_like(density)
        g_t = torch.empty_like(depths) if ctx.needs_input_grad[2] else None
        if n:
            _C.check(_C.lib().qf_derive_properties_backward(
                _C.ptr(color), _C.ptr(density), _C.ptr(depths), _C.ptr(deltas_t), ctx.delta_c, _C.ptr(index_ray), n,
                ctx.n_rays, ctx.mode, _C.ptr(bk), _C.ptr(_C.f32c(g_rgb)), _C.ptr(_C.f32c(g_alpha)), _C.ptr(_C.f32c(g_depth)),
                _C.ptr(g_color), _C.ptr(g_sigma), _C.ptr(g_t), _C.stream()), "qf_derive_properties_backward")
        return g_color, g_sigma, g_t, None, None, None, None, None, None, None


def derive_properties(color, density, depths, deltas, boundary, index_ray, render_bkgd=None, bg_color="white", N=0,
                      sample_index=None):
    """Per-ray colour / alpha / depth buffers from packed samples sorted by (ray, depth): one fused launch
    (the reference runs three kaolin scans + three scatters, utils.py:863-898).

    Returns (rgb [N,3], alpha [N,1], index_ray[boundary], Depth [N,1], weights [S,1]).  Background handling
    follows the reference, quirks included: white (or any non-"black" name) fills untouched rays with 1 and
    blends ``(1-a) + a*sum(w c)``; "black" uses ``a*sum(w c)``; other names blend with ``render_bkgd``.
    Differentiable w.r.t. colour, density and depths when autograd is recording (training).
    ``sample_index`` (extension, inference only): int32 [S]; sample i's colour and density are
    ``color[sample_index[i]]`` / ``density[sample_index[i]]`` -- they were evaluated in the field kernel's coherent
    order (``RayIntersector.coherent_layout``); depths, deltas and index_ray stay indexed by i."""
    color = _C.f32c(color.reshape(-1, 3))
    dev = color.device
    density = _C.f32c(density.reshape(-1))
    depths = _C.f32c(depths.reshape(-1))
    index_ray = _C.i64c(index_ray.reshape(-1))
    N = int(N)
    if N <= 0 and depths.shape[0] > 0:
        # the reference's default N=0 fails there too (index N-sized buffers by ray id: IndexError)
        raise IndexError(f"derive_properties: {depths.shape[0]} samples but N={N} rays; pass the number of rays")
    deltas_t, delta_c = None, 0.0
    if isinstance(deltas, torch.Tensor):
        deltas_t = _C.f32c(deltas.detach().reshape(-1))
    else:
        delta_c = float(deltas)
    mode = _BG.get(bg_color, _C.BG_CUSTOM)
    bk = None
    if mode == _C.BG_CUSTOM:
        bk = _C.f32c(render_bkgd.detach().reshape(3).to(dev))
    if sample_index is not None and (torch.is_grad_enabled() and (color.requires_grad or density.requires_grad)):
        raise ValueError("sample_index is an inference-only path")
    rgb, alpha, depth_out, weights = _DerivePropertiesFn.apply(color, density, depths, deltas_t, delta_c, index_ray,
                                                               N, mode, bk, sample_index)
    hit_rays = index_ray[boundary] if boundary is not None else None
    return rgb, alpha, hit_rays, depth_out, weights


@torch.no_grad()
def composite_frame(color_c, density_c, frame, render_step_size: float, render_bkgd=None, bg_color="white",
                    want_weights: bool = False, packed: bool = False):
    """``derive_properties`` for a whole frame whose colours / densities come straight from the field kernel, i.e. in the
    intersector's coherent order: ``frame`` = ``RayIntersector.last_frame`` (depths in that order, per-pixel sample
    counts, tile bases, image size).  One launch (``qf_composite_tiles``), every load a contiguous run; the same
    values as ``derive_properties(..., sample_index=inverse)`` bit for bit.  Returns (rgb [N,3], alpha [N,1],
    depth [N,1], weights in the coherent order [S,1] or None).  ``packed``: ONE [N,5] array (rgb | alpha | depth per
    pixel, what a row band of a sharded frame sends) comes back in place of the three: (packed, None, None, weights).
    Inference only."""
    color_c = _C.f32c(color_c.reshape(-1, 3))
    density_c = _C.f32c(density_c.reshape(-1))
    dev = color_c.device
    n = frame.depth_c.shape[0]
    if getattr(frame, "band_rows", 0):
        raise ValueError("composite_frame: this frame's layout is cut into row bands (a loader item for generate_splits); "
                         "composite it with derive_properties(sample_index=inverse)")
    if color_c.shape[0] != n or density_c.shape[0] != n:
        raise ValueError(f"composite_frame: {n} samples in the frame, {color_c.shape[0]} colours, {density_c.shape[0]} densities")
    n_rays = frame.width * frame.height
    mode = _BG.get(bg_color, _C.BG_CUSTOM)
    bk = _C.f32c(render_bkgd.detach().reshape(3).to(dev)) if mode == _C.BG_CUSTOM else None
    rgb = alpha = depth = out5 = None
    if packed:
        out5 = torch.empty((n_rays, 5), dtype=torch.float32, device=dev)
    else:
        rgb = torch.empty((n_rays, 3), dtype=torch.float32, device=dev)
        alpha = torch.empty((n_rays, 1), dtype=torch.float32, device=dev)
        depth = torch.empty((n_rays, 1), dtype=torch.float32, device=dev)
    weights = torch.empty((n, 1), dtype=torch.float32, device=dev) if want_weights else None
    _C.check(_C.lib().qf_composite_tiles(
        _C.ptr(color_c), _C.ptr(density_c), _C.ptr(frame.depth_c), float(render_step_size), _C.ptr(frame.hit_count),
        frame.max_hits, _C.ptr(frame.tile_base), frame.width, frame.height, mode, _C.ptr(bk), _C.ptr(rgb), _C.ptr(alpha),
        _C.ptr(depth), _C.ptr(weights), _C.ptr(out5), _C.stream()), "qf_composite_tiles")
    if packed:
        return out5, None, None, weights
    return rgb, alpha, depth, weights


@torch.no_grad()
def deform_frame(f_c, scaling: float, xyz_c, dirs_c, frame, total_device=None):
    """The "before" evaluation's displacement + re-sort (utils.py:555-572, mesh_utils.py:389-403) on a frame in the
    intersector's coherent order: ``f_c`` = the deformation field's output at ``xyz_c``; returns (xyz, depth) in the
    same order, every ray's samples displaced by ``tanh(f) * scaling`` along the ray and back in depth order
    (``qf_deform_resort_tiles``).  Inference only."""
    f_c = _C.f32c(f_c.detach().reshape(-1))
    n = frame.total                    # slots of the arrays (their capacity when the count stays on the device)
    if f_c.shape[0] != n or xyz_c.shape[0] != n:
        raise ValueError(f"deform_frame: {n} slots in the frame, {f_c.shape[0]} field outputs, {xyz_c.shape[0]} positions")
    xyz_out = torch.empty_like(xyz_c)
    depth_out = torch.empty_like(frame.depth_c)
    _C.check(_C.lib().qf_deform_resort_tiles(
        _C.ptr(f_c), float(scaling), _C.ptr(_C.f32c(xyz_c)), _C.ptr(_C.f32c(dirs_c)), _C.ptr(frame.depth_c),
        _C.ptr(frame.hit_count), frame.max_hits, _C.ptr(frame.tile_base), n, _C.ptr(total_device, torch.int64),
        frame.width, frame.height, _C.ptr(xyz_out), _C.ptr(depth_out), _C.stream()), "qf_deform_resort_tiles")
    return xyz_out, depth_out


def _flatten_rays(rays: Rays):
    rays_shape = rays.origins.shape
    if len(rays_shape) == 3:
        height, width, _ = rays_shape
        num_rays = height * width
        rays = namedtuple_map(lambda r: r.reshape([num_rays] + list(r.shape[2:])), rays)
    else:
        num_rays, _ = rays_shape
    return rays, rays_shape, num_rays


def _to_device(data, device):
    xyzs, dirs, index_ray, ts, index_tri, origins = data
    return (xyzs.to(device), dirs.to(device), index_ray.to(device).long(), ts.to(device),
            index_tri.to(device).long(), origins.to(device))


def _module_trains(module) -> bool:
    return module is not None and torch.is_grad_enabled() and any(p.requires_grad for p in module.parameters())


def _faces_on_device(mesh_intersect) -> torch.Tensor:
    cache = getattr(mesh_intersect, "_faces_dev", None)
    if cache is None or cache[0] is not mesh_intersect.mesh.faces:
        faces = torch.from_numpy(np.ascontiguousarray(mesh_intersect.mesh.faces, dtype=np.int64)).to(mesh_intersect.device)
        mesh_intersect._faces_dev = cache = (mesh_intersect.mesh.faces, faces)
    return cache[1]


def render_image_finetune_with_occgrid(
    radiance_field: torch.nn.Module, field_net: Optional[torch.nn.Module], estimator, rays: Rays, data,
    near_plane: float = 0.0, far_plane: float = 1e10, render_step_size: float = 1e-3,
    render_bkgd: Optional[torch.Tensor] = None, cone_angle: float = 0.0, alpha_thre: float = 0.0,
    test_chunk_size: int = 8192, timestamps: Optional[torch.Tensor] = None, mesh_intersect=None,
    mesh_finetune=None, scaling=1 / 128, bg_color="white", order=None, order_inverse=None,
):
    """Render the samples of one split through the (deformed) quadrature points -- utils.py:465-607.
    ``order`` (extension, optional): coherent processing order (``RayIntersector.last_order``, or the first member
    of ``RayIntersector.coherent_layout``);
    ``order_inverse``: its inverse map if the caller has it (``RayIntersector.last_layout[0]``).

    Returns the reference's 9-tuple (colors, opacities, depths, n_samples, weights, positions, index_ray,
    loss, index_tri).

    Inference (``torch.no_grad()``, as the reference's eval loop runs it): fused kernels throughout; ``loss`` is
    returned as zeros (the regulariser needs the random barycentric samples of :543-546, which only matter for
    training, and the ``torch.rand`` call of :545 is not made).
    Training (autograd recording and ``field_net`` / ``radiance_field`` have trainable parameters): the
    deformation, the re-sort gather, the field and the compositing stay in the autograd graph and ``loss`` is the
    regulariser of :583, ``mean(dv^2) + mean((dv_vertex - dv.detach())^2)``."""
    rays, rays_shape, num_rays = _flatten_rays(rays)
    device = mesh_intersect.device
    xyzs, dirs, index_ray, ts, index_tri, origins = _to_device(data, device)
    dh = None
    loss = torch.zeros(1, device=device)
    inference = not (torch.is_grad_enabled() and (xyzs.requires_grad or ts.requires_grad or _module_trains(radiance_field)
                                                  or _module_trains(field_net)))
    if REPRODUCE_EVAL_RNG_ADVANCE and not _module_trains(field_net) and xyzs.shape[0] > 0:
        torch.rand((xyzs.shape[0], 3), device=device)          # utils.py:545, drawn and dropped: only the stream moves
    auto_inverse = None
    window = data if (isinstance(data, SampleWindow) and inference and order is None and xyzs.shape[0] > 0
                      and data.num_rays == num_rays and data.inverse.device == device) else None
    if window is not None:
        # a window of a loader item that came with its frame-wide coherent layout (generate_splits): positions relative
        # to the window's first sample -- one subtraction instead of the four launches of qf_split_layout
        deforms = field_net is not None and scaling != 0
        auto_inverse = window.inverse - window.base
        if deforms and isinstance(field_net, _Field) and window.order is not None:
            order = window.order - window.base
        if not deforms:
            # no deformation: the samples ARE sorted by (ray, depth), the re-sort of sampling_indexing is the identity
            # (what FrameRenderer.render relies on too) and the loader's pack has already written the streamed copies:
            # field on the window's slice of them, compositing through the inverse map -- no resort launch at all
            rgbs, sigmas = radiance_field(window.xyz_c, window.dirs_c)
            rgb, opacity, _, depth_img, weights = derive_properties(
                rgbs, sigmas.reshape(-1), ts, float(mesh_intersect.render_step_size), None, index_ray, bg_color=bg_color,
                render_bkgd=render_bkgd, N=num_rays, sample_index=auto_inverse)
            if mesh_finetune is not None:
                mesh_finetune.update_d(None, weights[:, 0].detach(), index_tri)
            return (rgb.view((*rays_shape[:-1], -1)), opacity.view((*rays_shape[:-1], -1)),
                    depth_img.view((*rays_shape[:-1], -1)), xyzs.shape[0], weights, xyzs, index_ray, loss, index_tri)
    elif order is None and inference and xyzs.shape[0] > 0:
        # the reference's eval loop hands over a window of a frame and no processing order: derive the coherent order
        # from the window's own ray ids (qf_split_layout) when the intersector knows the frame's width, and let the
        # re-sort launch write the streamed copies -- locality only, same pixels
        shape = getattr(getattr(mesh_intersect, "rayintersector", None), "last_image_shape", None)
        if shape is not None and shape[0] * shape[1] == num_rays:
            deforms = field_net is not None and scaling != 0 and isinstance(field_net, _Field)
            order, auto_inverse, _ = mesh_intersect.rayintersector.split_layout(index_ray, shape[0], shape[1],
                                                                               want_order=deforms)
    if _module_trains(field_net):
        tri_v = mesh_intersect.vertices[_faces_on_device(mesh_intersect)[index_tri]][:, :, 0:3]        # [S,3,3]
        w = torch.rand((xyzs.shape[0], 3), device=device)[..., None]
        verts = torch.sum(tri_v * w, dim=1) / (torch.sum(w, dim=1) + 1e-6)
        # the reference evaluates the deformation field twice (utils.py:547,556: at the random triangle points and at
        # the samples); one call on both point sets is the same per-point arithmetic with one forward, one MLP backward
        # and one table scatter instead of two
        n_v = verts.shape[0]
        both = torch.tanh(field_net(torch.cat([verts, xyzs], dim=0), return_grad=False)[0]) * scaling
        del_vector_v = both[:n_v].expand(-1, 3)
        del_vector = both[n_v:].expand(-1, 3)                                                      # [S,1] -> 3 (B-15)
        del_delta = (del_vector * dirs).sum(-1, keepdim=True)
        dh = del_delta * dirs
        xyzs = xyzs + dh
        ts = ts + del_delta.view(-1)
        loss = ((del_vector ** 2).mean() + ((del_vector_v - del_vector.detach()) ** 2).mean()).reshape(1)
    elif field_net is not None and scaling != 0:
        xyzs, ts = _C.f32c(xyzs), _C.f32c(ts)
        # the samples arrive sorted by (ray, depth), which is the layout ``order`` was built for
        f = (field_net(xyzs, return_grad=False, order=order) if isinstance(field_net, _Field)
             else field_net(xyzs, return_grad=False))[0].detach().reshape(-1).contiguous()
        moved, ts_moved = torch.empty_like(xyzs), torch.empty_like(ts)      # out of place: the inputs are the caller's
        dh = torch.empty_like(xyzs) if mesh_finetune is not None else None  # the reference's dh = del_delta * dirs
        _C.check(_C.lib().qf_apply_deformation(_C.ptr(f), float(scaling), _C.ptr(_C.f32c(dirs)), _C.ptr(xyzs), _C.ptr(ts),
                                               xyzs.shape[0], _C.ptr(moved), _C.ptr(ts_moved), _C.ptr(dh), _C.stream()),
                 "qf_apply_deformation")
        xyzs, ts = moved, ts_moved
    # scaling == 0 multiplies the displacement by zero in the reference (utils.py:566-571): skipping is exact.
    if auto_inverse is not None:
        points, deltas, boundary, dirs, index_ray, depth, index_tri_s, _ = mesh_intersect.sampling_indexing(
            xyzs, origins, dirs, index_ray, ts, index_tri, layout_inverse=auto_inverse, lean=True)
    else:
        points, deltas, boundary, dirs, index_ray, depth, index_tri_s, _ = mesh_intersect.sampling_indexing(
            xyzs, origins, dirs, index_ray, ts, index_tri)
    sample_index = None
    if auto_inverse is not None:
        points_c, dirs_c = mesh_intersect.last_resort_layout
        rgbs, sigmas = radiance_field(points_c, dirs_c)
        sample_index = auto_inverse
    elif order is not None and order.shape[0] == points.shape[0]:
        # coherent processing order: locality only
        if torch.is_grad_enabled() and (points.requires_grad or _module_trains(radiance_field)):
            rgbs, sigmas = radiance_field(points, dirs, order=order)
        else:
            # inference: lay the (deformed, re-sorted) points out IN that order so that the field kernel streams, and
            # let compositing pick colour / density up through the inverse map (same bits, see qf_pack_samples)
            o64 = order.long()
            rgbs, sigmas = radiance_field(points[o64], dirs[o64])
            if order_inverse is not None and order_inverse.shape[0] == points.shape[0]:
                sample_index = order_inverse
            else:
                sample_index = torch.empty_like(order)
                sample_index[o64] = torch.arange(order.shape[0], dtype=order.dtype, device=order.device)
    else:
        rgbs, sigmas = radiance_field(points, dirs)
    # (boundary=None: the third return value, index_ray[boundary], is discarded here as in the reference -- utils.py:585
    #  -- and computing it would cost a boolean-mask gather with a host wait per split)
    rgb, opacity, _, depth_img, weights = derive_properties(
        rgbs, sigmas.reshape(-1), depth, deltas, None, index_ray, bg_color=bg_color, render_bkgd=render_bkgd,
        N=num_rays, sample_index=sample_index)
    if mesh_finetune is not None:
        # dh None: the displacement is identically zero, cache_d += 0 * w is a no-op (update_d skips it)
        mesh_finetune.update_d(None if dh is None else dh.detach(), weights[:, 0].detach(), index_tri)
    return (rgb.view((*rays_shape[:-1], -1)), opacity.view((*rays_shape[:-1], -1)),
            depth_img.view((*rays_shape[:-1], -1)), xyzs.shape[0], weights, points, index_ray, loss, index_tri)


@torch.no_grad()
def render_image_bake_texture_images_with_occgrid(
    radiance_field: torch.nn.Module, rays: Rays, data, texture=None, uv=None, near_plane: float = 0.0,
    far_plane: float = 1e10, render_step_size: float = 1e-3, render_bkgd: Optional[torch.Tensor] = None,
    cone_angle: float = 0.0, alpha_thre: float = 0.0, test_chunk_size: int = 8192,
    timestamps: Optional[torch.Tensor] = None, mesh_intersect=None, mesh_finetune=None, scaling=1 / 128,
    discretize=False, compressor=None, bg_color="white",
):
    """Render from the baked SG textures -- utils.py:998-1095.  Returns the reference's 8-tuple
    (colors, opacities, depths, n_samples, weights, positions, rays, 0).  ``uv`` is the per-vertex UV array
    already scaled by the texture size (test_baking_texture_images.py:325-328)."""
    rays, rays_shape, num_rays = _flatten_rays(rays)
    device = mesh_intersect.device
    xyzs, dirs, index_ray, ts, index_tri, origins = _to_device(data, device)
    if isinstance(data, (SampleSet, SampleWindow)):
        # the device loader's own pack: sorted by (ray, depth) by construction and nothing has displaced the samples
        # since (this renderer has no deformation), so the re-sort of sampling_indexing (mesh_utils.py:389-412) is the
        # identity and the constant step needs no boundaries -- one launch and one boolean-mask gather less per frame
        points, depth, deltas, boundary = xyzs, ts, float(mesh_intersect.render_step_size), None
    else:
        points, deltas, boundary, dirs, index_ray, depth, index_tri, _ = mesh_intersect.sampling_indexing(
            xyzs, origins, dirs, index_ray, ts, index_tri)
    texel = texel_indices(mesh_intersect, uv, points, index_tri, compressor.texture_size)
    if discretize:
        feats = compressor.get_features_from_texture_map(texel)
        sigmas = inverse_of_compressed_sigma(compress_sigma(feats[:, -1]))
        rgbs = radiance_field.features_to_rgb(feats[:, :-1].contiguous(), dirs)
    else:
        rgbs, sigmas = compressor.shade(texel, dirs)
    rgb, opacity, _, depth_img, weights = derive_properties(
        rgbs, sigmas, depth, deltas, boundary, index_ray, bg_color=bg_color, render_bkgd=None, N=num_rays)
    return (rgb.view((*rays_shape[:-1], -1)), opacity.view((*rays_shape[:-1], -1)),
            depth_img.view((*rays_shape[:-1], -1)), xyzs.shape[0], weights, points, rays, 0)


def render_image_fit_sg_with_occgrid(
    radiance_field: torch.nn.Module, radiance_field_sg: torch.nn.Module, estimator, rays: Rays, data,
    near_plane: float = 0.0, far_plane: float = 1e10, render_step_size: float = 1e-3,
    render_bkgd: Optional[torch.Tensor] = None, cone_angle: float = 0.0, alpha_thre: float = 0.0,
    test_chunk_size: int = 8192, timestamps: Optional[torch.Tensor] = None, mesh_intersect=None,
    mesh_finetune=None, scaling=1 / 128, bg_color="white",
):
    """The renderer of the spherical-Gaussian fitting stage -- utils.py:610-730 (train_fit_sg.py:439-452,513-528):
    colour from ``radiance_field_sg`` (trained), density from ``radiance_field`` (frozen, evaluated without gradient
    as the reference does), the samples as given (no deformation, no re-sort), ``derive_properties``.  Returns the
    reference's 8-tuple (colors, opacities, depths, n_samples, weights, xyzs, index_ray, index_tri).  The 32 768-sample
    Python batches of the reference are gone; nothing depends on them."""
    if timestamps is not None:
        raise NotImplementedError("dynamic (D-NeRF) fields are out of scope")
    rays, rays_shape, num_rays = _flatten_rays(rays)
    device = mesh_intersect.device if mesh_intersect is not None else rays.origins.device
    xyzs, dirs, index_ray, ts, index_tri, origins = _to_device(data, device)
    t_dirs = _C.f32c(rays.viewdirs.to(device))[index_ray]
    rgbs, _ = radiance_field_sg(xyzs, t_dirs)
    with torch.no_grad():
        sigmas = radiance_field.query_density(xyzs).reshape(-1)
    rgb, opacity, _, depth, weights = derive_properties(
        rgbs, sigmas, ts, float(render_step_size), None, index_ray, bg_color=bg_color, render_bkgd=render_bkgd,
        N=num_rays)
    return (rgb.view((*rays_shape[:-1], -1)), opacity.view((*rays_shape[:-1], -1)), depth.view((*rays_shape[:-1], -1)),
            xyzs.shape[0], weights, xyzs, index_ray, index_tri)


def _triangle_records(mesh_intersect, uv):
    """The per-(mesh, uv) table of 128-byte triangle records of ``qf_texel_records_pack`` on the device, built on first
    use and rebuilt when the mesh's vertices or the uv tensor change."""
    cache = getattr(mesh_intersect, "_texel_cache", None)
    if cache is None or cache[0] is not mesh_intersect.mesh.vertices:
        v64 = torch.from_numpy(np.ascontiguousarray(mesh_intersect.mesh.vertices, dtype=np.float64)).to(mesh_intersect.device)
        faces = torch.from_numpy(np.ascontiguousarray(mesh_intersect.mesh.faces, dtype=np.int64)).to(mesh_intersect.device)
        cache = mesh_intersect._texel_cache = [mesh_intersect.mesh.vertices, v64, faces, None, None]
    _, v64, faces = cache[:3]
    uv = _C.f32c(torch.as_tensor(uv).to(mesh_intersect.device))
    key = (uv.data_ptr(), uv._version, tuple(uv.shape))
    if cache[3] != key:
        records = torch.empty((faces.shape[0], _C.QF_TEXEL_TRIANGLE_RECORD_BYTES), dtype=torch.uint8, device=uv.device)
        _C.check(_C.lib().qf_texel_records_pack(_C.ptr(v64), _C.ptr(faces), _C.ptr(uv), faces.shape[0], _C.ptr(records),
                                                _C.stream()), "qf_texel_records_pack")
        # the uv tensor stays referenced: its address is the key
        cache[3], cache[4] = key, _C.StreamCached(key, (records, uv), [records])
    return cache[4].get()[0]                 # ordered for a consumer on another stream than the one that packed them


def texel_indices(mesh_intersect, uv, points, index_tri, texture_size: int) -> torch.Tensor:
    """Nearest-texel lookup of utils.py:1055-1063 on the device (float64 barycentrics, fp32 UV blend) from the
    per-(mesh, uv) table of 128-byte triangle records."""
    records = _triangle_records(mesh_intersect, uv)
    points = _C.f32c(points)
    index_tri = _C.i64c(index_tri)
    n = points.shape[0]
    texel = torch.empty((n, 2), dtype=torch.int64, device=points.device)
    _C.check(_C.lib().qf_texel_indices_packed(_C.ptr(records), _C.ptr(points), _C.ptr(index_tri), n, int(texture_size),
                                              _C.ptr(texel), _C.stream()), "qf_texel_indices_packed")
    return texel


@torch.no_grad()
def shade_baked_points(mesh_intersect, uv, compressor, points, index_tri, dirs, n_device=None):
    """(rgb [n,3], sigma [n]) of samples given by position and triangle: ``texel_indices`` + ``compressor.shade`` in one
    launch (``qf_texture_shade_points``: the texel is looked up inside the shading kernel, no index array in between).
    Same values as the two calls."""
    records = _triangle_records(mesh_intersect, uv)
    points, dirs = _C.f32c(points), _C.f32c(dirs)
    # int32 ids (what the tile pack writes) go to the kernel as they are; anything else as the reference's int64
    tri32 = index_tri.contiguous() if index_tri.dtype == torch.int32 else None
    tri64 = None if tri32 is not None else _C.i64c(index_tri)
    n = points.shape[0]
    rgb = torch.empty((n, 3), dtype=torch.float32, device=points.device)
    sigma = torch.empty((n,), dtype=torch.float32, device=points.device)
    _C.check(_C.lib().qf_texture_shade_points(
        _C.ptr(compressor.records()), int(compressor.alpha.shape[0]), compressor.num_lobes,
        1 if compressor.compression_type == "sigma" else 0, float(compressor.lambda_thres), _C.ptr(records), _C.ptr(points),
        _C.ptr(tri64), _C.ptr(tri32), _C.ptr(dirs), n, _C.ptr(n_device, torch.int64), _C.ptr(rgb), _C.ptr(sigma), _C.stream()),
        "qf_texture_shade_points")
    return rgb, sigma


def early_stop_tau(early_stop_eps) -> float:
    """The optical depth behind which a front-to-back frame's pixel stops (a baked frame stops shading, a field frame
    stops being evaluated), from the transmittance threshold ``early_stop_eps`` in [0, 1): ``float32(-log(eps))``, computed once on the host; ``+inf`` (never stop) for 0.
    Anything else, NaN included, raises ValueError."""
    eps = float(early_stop_eps)
    if not (0.0 <= eps < 1.0):
        raise ValueError(f"early_stop_eps must lie in [0, 1), got {early_stop_eps!r}")
    return float("inf") if eps == 0.0 else float(np.float32(-math.log(eps)))


#: The default rank-window schedule of the front-to-back field frame before its ends >= K are collapsed into one final K
#: (``front_rank_windows``): the fastest of the four candidates of ``tools/field_front_bench.py`` on its opaque scene
#: (DESIGN.md section 3.5c has the numbers).
FRONT_RANK_WINDOWS = (1, 3, 7, 15)


def front_rank_windows(rank_windows, max_hits: int) -> tuple:
    """The rank-window schedule of a front-to-back field frame as the library takes it: strictly increasing ints,
    1 <= len <= 8, first >= 1, last >= ``max_hits``.  ``None``: the default, ``FRONT_RANK_WINDOWS`` followed by K with every
    end >= K collapsed into the final K ((1, 3, 7, 15, 25) at K = 25, (1, 3, 5) at K = 5, (1,) at K = 1).  Anything else raises
    ValueError."""
    k = int(max_hits)
    if rank_windows is None:
        return tuple(b for b in FRONT_RANK_WINDOWS if b < k) + (k,)
    w = tuple(int(b) for b in rank_windows)
    if tuple(rank_windows) != w or not 1 <= len(w) <= _C.QF_FRONT_MAX_WINDOWS or w[0] < 1 or w[-1] < k \
            or any(b <= a for a, b in zip(w, w[1:])):
        raise ValueError(f"rank_windows must be 1..{_C.QF_FRONT_MAX_WINDOWS} strictly increasing integers, the first >= 1 and "
                         f"the last >= max_hits = {k}, got {rank_windows!r}")
    return w


def front_scratch(n_rays: int, n_tiles: int, capacity: int, device):
    """The ``qf_front_scratch`` of a front-to-back field frame: (struct, tensors it points at -- keep them referenced until
    the frame's launches ran)."""
    state = torch.empty((n_rays, 8), dtype=torch.float32, device=device)
    win_count = torch.empty((n_tiles + (n_tiles + 15) // 16,), dtype=torch.int32, device=device)   # per tile | per 16 tiles
    win_total = torch.empty((1,), dtype=torch.int64, device=device)
    win_order = torch.empty((capacity,), dtype=torch.int32, device=device)
    s = _C.FrontScratch()
    s.state, s.win_count, s.win_total = state.data_ptr(), win_count.data_ptr(), win_total.data_ptr()
    s.win_order = win_order.data_ptr()
    return s, (state, win_count, win_total, win_order)


@torch.no_grad()
def render_field_front(radiance_field, xyz_c, dirs_c, frame, render_step_size: float, stop_tau: float, rank_windows,
                       render_bkgd=None, bg_color="white", packed: bool = False):
    """The field + ``composite_frame`` of a frame in the intersector's tile order, front to back in rank windows with
    early ray termination, as separately bound launches: per window ``qf_front_select``
    (composite the previous window, select the pixels that still see something, list their samples) and the field's
    fused kernel over that list (``forward_into``: ``order`` = the list, ``n_device`` = its length), then
    ``qf_front_finish``.  No host wait.  ``stop_tau`` from ``early_stop_tau`` (``inf`` never stops and gives the field +
    ``composite_frame`` pixels bit for bit), ``rank_windows`` from ``front_rank_windows``.  Returns (rgb [N,3],
    alpha [N,1], depth [N,1], shaded_count [N] int32, evaluated_count [N] int32) -- with ``packed`` ([N,5], None, None,
    shaded_count, evaluated_count).  What ``qf_frame_render_front`` composes into one call."""
    if getattr(frame, "band_rows", 0):
        raise ValueError("render_field_front: an unbanded frame is required")
    windows = front_rank_windows(rank_windows, frame.max_hits)
    xyz_c, dirs_c = _C.f32c(xyz_c), _C.f32c(dirs_c)
    dev = xyz_c.device
    n = frame.depth_c.shape[0]
    if xyz_c.shape[0] != n or dirs_c.shape[0] != n:
        raise ValueError(f"render_field_front: {n} slots in the frame, {xyz_c.shape[0]} positions, {dirs_c.shape[0]} directions")
    n_rays = frame.width * frame.height
    mode = _BG.get(bg_color, _C.BG_CUSTOM)
    bk = _C.f32c(render_bkgd.detach().reshape(3).to(dev)) if (mode == _C.BG_CUSTOM and render_bkgd is not None) else None
    rgb = alpha = depth = out5 = None
    if packed:
        out5 = torch.empty((n_rays, 5), dtype=torch.float32, device=dev)
    else:
        rgb = torch.empty((n_rays, 3), dtype=torch.float32, device=dev)
        alpha = torch.empty((n_rays, 1), dtype=torch.float32, device=dev)
        depth = torch.empty((n_rays, 1), dtype=torch.float32, device=dev)
    shaded = torch.empty((n_rays,), dtype=torch.int32, device=dev)
    evaluated = torch.empty((n_rays,), dtype=torch.int32, device=dev)
    rgbs = torch.empty((n, 3), dtype=torch.float32, device=dev)
    sigmas = torch.empty((n,), dtype=torch.float32, device=dev)
    _, (state, win_count, win_total, win_order) = front_scratch(n_rays, frame.tile_base.shape[0], n, dev)
    lib = _C.lib()
    common = (_C.ptr(rgbs), _C.ptr(sigmas), _C.ptr(frame.depth_c), float(render_step_size), _C.ptr(frame.hit_count),
              frame.max_hits, _C.ptr(frame.tile_base), frame.width, frame.height, float(stop_tau))
    lo = mid = 0
    for hi in windows:
        _C.check(lib.qf_front_select(*common, lo, mid, hi, _C.ptr(state), _C.ptr(win_count), _C.ptr(win_total),
                                     _C.ptr(win_order), n, _C.stream()), "qf_front_select")
        radiance_field.forward_into(xyz_c, dirs_c, rgbs, sigmas, order=win_order, n_device=win_total)
        lo, mid = mid, hi
    _C.check(lib.qf_front_finish(*common, lo, mid, _C.ptr(state), mode, _C.ptr(bk), _C.ptr(rgb), _C.ptr(alpha), _C.ptr(depth),
                                 _C.ptr(out5), _C.ptr(shaded), _C.ptr(evaluated), _C.stream()), "qf_front_finish")
    if packed:
        return out5, None, None, shaded, evaluated
    return rgb, alpha, depth, shaded, evaluated


def baked_shading(mesh_intersect, uv, compressor):
    """The ``qf_baked_shading`` of a (mesh, uv, texture set): (struct, tensors it points at -- keep them referenced until
    the launch that reads them ran)."""
    tri_records = _triangle_records(mesh_intersect, uv)
    records = compressor.records()
    s = _C.BakedShading()
    s.records, s.triangle_records = records.data_ptr(), tri_records.data_ptr()
    s.texture_size, s.n_lobes = int(compressor.alpha.shape[0]), int(compressor.num_lobes)
    s.sigmoid_codec = 1 if compressor.compression_type == "sigma" else 0
    s.lambda_thres = float(compressor.lambda_thres)
    return s, (records, tri_records)


@torch.no_grad()
def shade_composite_baked_frame(mesh_intersect, uv, compressor, xyz_c, dirs_c, frame, render_step_size: float,
                                stop_tau: float, render_bkgd=None, bg_color="white", packed: bool = False):
    """``shade_baked_points`` + ``composite_frame`` of a baked frame in the intersector's tile order as ONE launch that
    walks every pixel front to back (``qf_texture_composite_tiles``): no colour / density arrays, and a pixel stops
    fetching texels once the optical depth in front of its next sample exceeds ``stop_tau`` (``early_stop_tau``; ``inf``
    never stops and gives the two calls' pixels bit for bit).  ``frame`` must carry the samples' triangle ids
    (``want_tri``).  Returns (rgb [N,3], alpha [N,1], depth [N,1], shaded_count [N] int32: the samples of each pixel
    that contributed) -- with ``packed`` ([N,5], None, None, shaded_count)."""
    if getattr(frame, "band_rows", 0) or frame.tri_c is None:
        raise ValueError("shade_composite_baked_frame: an unbanded frame with triangle ids (want_tri) is required")
    shading, keep = baked_shading(mesh_intersect, uv, compressor)
    xyz_c, dirs_c = _C.f32c(xyz_c), _C.f32c(dirs_c)
    dev = xyz_c.device
    n = frame.depth_c.shape[0]
    if xyz_c.shape[0] != n or dirs_c.shape[0] != n or frame.tri_c.shape[0] != n:
        raise ValueError(f"shade_composite_baked_frame: {n} slots in the frame, {xyz_c.shape[0]} positions, "
                         f"{dirs_c.shape[0]} directions, {frame.tri_c.shape[0]} triangle ids")
    n_rays = frame.width * frame.height
    mode = _BG.get(bg_color, _C.BG_CUSTOM)
    bk = _C.f32c(render_bkgd.detach().reshape(3).to(dev)) if (mode == _C.BG_CUSTOM and render_bkgd is not None) else None
    rgb = alpha = depth = out5 = None
    if packed:
        out5 = torch.empty((n_rays, 5), dtype=torch.float32, device=dev)
    else:
        rgb = torch.empty((n_rays, 3), dtype=torch.float32, device=dev)
        alpha = torch.empty((n_rays, 1), dtype=torch.float32, device=dev)
        depth = torch.empty((n_rays, 1), dtype=torch.float32, device=dev)
    shaded = torch.empty((n_rays,), dtype=torch.int32, device=dev)
    _C.check(_C.lib().qf_texture_composite_tiles(
        shading.records, shading.texture_size, shading.n_lobes, shading.sigmoid_codec, shading.lambda_thres,
        shading.triangle_records, _C.ptr(xyz_c), _C.ptr(dirs_c), _C.ptr(frame.depth_c), _C.ptr(frame.tri_c, torch.int32),
        _C.ptr(frame.hit_count), frame.max_hits, _C.ptr(frame.tile_base), frame.width, frame.height, float(render_step_size),
        mode, _C.ptr(bk), float(stop_tau), _C.ptr(rgb), _C.ptr(alpha), _C.ptr(depth), _C.ptr(out5), _C.ptr(shaded),
        _C.stream()), "qf_texture_composite_tiles")
    if packed:
        return out5, None, None, shaded
    return rgb, alpha, depth, shaded


def _vertex_lobes(width: int) -> int:
    lobes, rest = divmod(int(width) - 4, 7)
    if rest or not 1 <= lobes <= _C.QF_MAX_LOBES:
        raise ValueError(f"vertex features must have 3 + 7 L + 1 columns with 1 <= L <= {_C.QF_MAX_LOBES}, got {width}")
    return lobes


def _vertex_features_lobes(vertex_features) -> int:
    if isinstance(vertex_features, (VertexBakedFeatures, QuantisedVertexFeatures)):
        return vertex_features.n_lobes
    return _vertex_lobes(vertex_features.shape[1])


def _vertex_records(mesh_intersect):
    """The mesh's cache of the vertex-baked route, built on first use: [vertex array, records, table key, table]."""
    cache = getattr(mesh_intersect, "_vertex_baked_cache", None)
    if cache is None or cache[0] is not mesh_intersect.mesh.vertices:
        dev = mesh_intersect.device
        v64 = torch.from_numpy(np.ascontiguousarray(mesh_intersect.mesh.vertices, dtype=np.float64)).to(dev)
        faces = torch.from_numpy(np.ascontiguousarray(mesh_intersect.mesh.faces, dtype=np.int64)).to(dev)
        records = torch.empty((faces.shape[0], _C.QF_VERTEX_TRIANGLE_RECORD_BYTES), dtype=torch.uint8, device=dev)
        _C.check(_C.lib().qf_vertex_records_pack(_C.ptr(v64), v64.shape[0], _C.ptr(faces), faces.shape[0], _C.ptr(records),
                                                 _C.stream()), "qf_vertex_records_pack")
        # v64 and faces stay referenced: the pack may still be reading them on its stream
        cache = mesh_intersect._vertex_baked_cache = [mesh_intersect.mesh.vertices,
                                                      _C.StreamCached(None, (records, v64, faces), [records]), None, None]
    return cache


def vertex_baked_shading(mesh_intersect, vertex_features):
    """What the vertex-baked kernels read, on the device: (table, records).  ``table``: float32
    [V, stride], ``vertex_features`` ([V, 3 + 7L + 1], ``baking.bake_vertex_features``) with every row zero-padded to
    ``_C.vertex_row_stride(L)`` floats (64-byte lines).  ``records``: the 128-byte vertex-triangle records of
    ``qf_vertex_records_pack`` from the mesh's float64 vertices.  Both are built on first use and cached the way
    ``_triangle_records`` caches its table: the records per vertex array of the mesh, the padded table per (address,
    version, shape) of the feature tensor, each ordered for a consumer on another stream than the one that built it.
    A ``baking.VertexBakedFeatures`` is taken as it is: ``table`` is its parameter's own memory (detached), nothing is
    copied or cached, and ordering it across streams is the caller's, as for any tensor they own."""
    cache = _vertex_records(mesh_intersect)
    if isinstance(vertex_features, VertexBakedFeatures):
        vertex_features.check_rows(mesh_intersect.mesh.vertices.shape[0])
        table = vertex_features.table.detach()
        if table.device != _C.resolve_device(mesh_intersect.device) or not table.is_contiguous() or table.data_ptr() % 64:
            raise ValueError(f"the VertexBakedFeatures table must be contiguous, 64-byte aligned and on "
                             f"{mesh_intersect.device}, it is on {table.device}")
        return table, cache[1].get()[0]
    feats = torch.as_tensor(vertex_features)
    if feats.dim() != 2 or feats.shape[0] != mesh_intersect.mesh.vertices.shape[0]:
        raise ValueError(f"vertex_features must be [V, 3 + 7L + 1] with V = {mesh_intersect.mesh.vertices.shape[0]} rows, "
                         f"got {tuple(feats.shape)}")
    lobes = _vertex_lobes(feats.shape[1])
    key = (feats.data_ptr(), feats._version, tuple(feats.shape), feats.dtype, feats.device)
    if cache[2] != key:
        table = torch.zeros((feats.shape[0], _C.vertex_row_stride(lobes)), dtype=torch.float32, device=mesh_intersect.device)
        table[:, :feats.shape[1]] = feats.detach().to(mesh_intersect.device)
        # the feature tensor stays referenced: its address is the key
        cache[2], cache[3] = key, _C.StreamCached(key, (table, feats), [table])
    return cache[3].get()[0], cache[1].get()[0]


def vertex_baked_shading_struct(mesh_intersect, vertex_features):
    """The ``qf_vertex_baked_shading`` of a (mesh, feature tensor or ``VertexBakedFeatures``): (struct, tensors it points
    at -- keep them referenced until the launch that reads them ran)."""
    table, records = vertex_baked_shading(mesh_intersect, vertex_features)
    s = _C.VertexBakedShading()
    s.table, s.records = table.data_ptr(), records.data_ptr()
    s.n_vertices, s.stride, s.n_lobes = int(table.shape[0]), int(table.shape[1]), _vertex_features_lobes(vertex_features)
    return s, (table, records)


def vertex_quant_shading(mesh_intersect, quantised):
    """What the quantised vertex kernels read, on the device: (records, tri_records).
    ``records``: the [T*T, 64] uint8 vertex records of a ``baking.QuantisedVertexFeatures`` (its texture set's texel
    records, cached there and ordered across streams); ``tri_records``: the mesh's 128-byte vertex-triangle records, the
    fp32 route's own cache."""
    quantised.check_rows(mesh_intersect.mesh.vertices.shape[0])
    records = quantised.records()
    if records.device != _C.resolve_device(mesh_intersect.device) or records.data_ptr() % 16:
        raise ValueError(f"the QuantisedVertexFeatures records must be 16-byte aligned and on {mesh_intersect.device}, "
                         f"they are on {records.device}")
    return records, _vertex_records(mesh_intersect)[1].get()[0]


def vertex_quant_shading_struct(mesh_intersect, quantised):
    """The ``qf_vertex_quant_shading`` of a (mesh, ``QuantisedVertexFeatures``): (struct, tensors it points at -- keep them
    referenced until the launch that reads them ran)."""
    records, tri_records = vertex_quant_shading(mesh_intersect, quantised)
    s = _C.VertexQuantShading()
    s.records, s.tri_records = records.data_ptr(), tri_records.data_ptr()
    s.n_vertices, s.n_lobes = quantised.n_vertices, quantised.n_lobes
    s.sigmoid_codec, s.lambda_thres = quantised.sigmoid_codec, float(quantised.compressor.lambda_thres)
    return s, (records, tri_records)


def check_vertex_features(mesh_intersect, vertex_features) -> None:
    """Raises for a table that does not fit the mesh (either kind), before anything is sampled."""
    if isinstance(vertex_features, QuantisedVertexFeatures):
        vertex_quant_shading(mesh_intersect, vertex_features)
    else:
        vertex_baked_shading(mesh_intersect, vertex_features)


class _VertexShadeFn(torch.autograd.Function):
    """Differentiable vertex shading: forward = ``qf_vertex_shade_points`` on the padded table,
    backward = ``qf_vertex_shade_points_backward`` into a zero-filled [V, stride] gradient.  Only inputs are saved: the
    backward recomputes the blend.  ``train_density`` False: the density is frozen -- sigma carries no graph and the
    kernel gets no ``d_sigma``.  The ids come as exactly one of ``tri64`` / ``tri32``."""

    @staticmethod
    def forward(ctx, table, records, points, tri64, tri32, dirs, lobes, n_device, train_density):
        n = points.shape[0]
        rgb = torch.empty((n, 3), dtype=torch.float32, device=points.device)
        sigma = torch.empty((n,), dtype=torch.float32, device=points.device)
        _C.check(_C.lib().qf_vertex_shade_points(
            _C.ptr(table), int(table.shape[1]), lobes, _C.ptr(records), _C.ptr(points), _C.ptr(tri64), _C.ptr(tri32),
            _C.ptr(dirs), n, _C.ptr(n_device, torch.int64), None, _C.ptr(rgb), _C.ptr(sigma), _C.stream()),
            "qf_vertex_shade_points")
        ctx.save_for_backward(table, records, points, tri64, tri32, dirs, n_device)
        ctx.lobes, ctx.train_density = lobes, train_density
        if not train_density:
            ctx.mark_non_differentiable(sigma)
        return rgb, sigma

    @staticmethod
    def backward(ctx, g_rgb, g_sigma):
        table, records, points, tri64, tri32, dirs, n_device = ctx.saved_tensors
        grad = torch.zeros_like(table)
        g_rgb = _C.f32c(g_rgb)
        g_sigma = _C.f32c(g_sigma) if ctx.train_density else None
        _C.check(_C.lib().qf_vertex_shade_points_backward(
            _C.ptr(table), int(table.shape[1]), ctx.lobes, _C.ptr(records), int(table.shape[0]), _C.ptr(points),
            _C.ptr(tri64), _C.ptr(tri32), _C.ptr(dirs), points.shape[0], _C.ptr(n_device, torch.int64), _C.ptr(g_rgb),
            _C.ptr(g_sigma), _C.ptr(grad), _C.stream()), "qf_vertex_shade_points_backward")
        return grad, None, None, None, None, None, None, None, None


def _vertex_table_trains(vertex_features) -> bool:
    """The differentiable route is taken exactly when a ``VertexBakedFeatures`` whose table requires a gradient is passed
    while autograd is recording."""
    return (isinstance(vertex_features, VertexBakedFeatures) and torch.is_grad_enabled()
            and vertex_features.table.requires_grad)


@torch.no_grad()
def _shade_vertex_quant_points(mesh_intersect, quantised, points, index_tri, dirs, n_device, want_features):
    records, tri_records = vertex_quant_shading(mesh_intersect, quantised)
    lobes = quantised.n_lobes
    points, dirs = _C.f32c(points), _C.f32c(dirs)
    tri32 = index_tri.contiguous() if index_tri.dtype == torch.int32 else None
    tri64 = None if tri32 is not None else _C.i64c(index_tri)
    n = points.shape[0]
    rgb = torch.empty((n, 3), dtype=torch.float32, device=points.device)
    sigma = torch.empty((n,), dtype=torch.float32, device=points.device)
    feats = torch.empty((n, 3 + 7 * lobes + 1), dtype=torch.float32, device=points.device) if want_features else None
    _C.check(_C.lib().qf_vertex_quant_shade_points(
        _C.ptr(records), quantised.n_vertices, lobes, quantised.sigmoid_codec, float(quantised.compressor.lambda_thres),
        _C.ptr(tri_records), _C.ptr(points), _C.ptr(tri64), _C.ptr(tri32), _C.ptr(dirs), n, _C.ptr(n_device, torch.int64),
        _C.ptr(feats), _C.ptr(rgb), _C.ptr(sigma), _C.stream()), "qf_vertex_quant_shade_points")
    if want_features:
        return rgb, sigma, feats
    return rgb, sigma


def shade_vertex_baked_points(mesh_intersect, vertex_features, points, index_tri, dirs, n_device=None,
                              want_features: bool = False):
    """(rgb [n,3], sigma [n]) of samples given by position and triangle from the vertex-baked features: the unclamped
    fp32 barycentrics of the sample in its triangle, the blend of the triangle's three vertex rows, SG shading of the
    blend -- utils.py:822-840 in one launch (``qf_vertex_shade_points``).  ``want_features``: the blend itself comes
    back as a third value, [n, 3 + 7L + 1].  ``n_device``: see ``shade_baked_points``.
    ``vertex_features``: a [V, 3 + 7L + 1] tensor (inference only: detached, padded once, cached) or a
    ``baking.VertexBakedFeatures``, whose table is read in place.  With such a module whose table requires a gradient,
    while autograd is recording, rgb and sigma carry a graph to the table (``_VertexShadeFn``; ``want_features`` is then
    not offered); every other call runs without one, as before.  A ``baking.QuantisedVertexFeatures`` is shaded from its
    64-byte records (``qf_vertex_quant_shade_points``): the values of this function on its ``dequantise()`` table, bit for
    bit."""
    if isinstance(vertex_features, QuantisedVertexFeatures):
        return _shade_vertex_quant_points(mesh_intersect, vertex_features, points, index_tri, dirs, n_device, want_features)
    if _vertex_table_trains(vertex_features):
        if want_features:
            raise ValueError("want_features is an inference-only output")
        with torch.no_grad():
            _, records = vertex_baked_shading(mesh_intersect, vertex_features)
            points, dirs = _C.f32c(points.detach()), _C.f32c(dirs.detach())
            tri32 = index_tri.contiguous() if index_tri.dtype == torch.int32 else None
            tri64 = None if tri32 is not None else _C.i64c(index_tri)
        return _VertexShadeFn.apply(vertex_features.table, records, points, tri64, tri32, dirs, vertex_features.n_lobes,
                                    n_device, vertex_features.train_density)
    with torch.no_grad():
        table, records = vertex_baked_shading(mesh_intersect, vertex_features)
        lobes = _vertex_features_lobes(vertex_features)
        points, dirs = _C.f32c(points), _C.f32c(dirs)
        # int32 ids (what the tile pack writes) go to the kernel as they are; anything else as the reference's int64
        tri32 = index_tri.contiguous() if index_tri.dtype == torch.int32 else None
        tri64 = None if tri32 is not None else _C.i64c(index_tri)
        n = points.shape[0]
        rgb = torch.empty((n, 3), dtype=torch.float32, device=points.device)
        sigma = torch.empty((n,), dtype=torch.float32, device=points.device)
        feats = torch.empty((n, 3 + 7 * lobes + 1), dtype=torch.float32, device=points.device) if want_features else None
        _C.check(_C.lib().qf_vertex_shade_points(
            _C.ptr(table), int(table.shape[1]), lobes, _C.ptr(records), _C.ptr(points), _C.ptr(tri64), _C.ptr(tri32),
            _C.ptr(dirs), n, _C.ptr(n_device, torch.int64), _C.ptr(feats), _C.ptr(rgb), _C.ptr(sigma), _C.stream()),
            "qf_vertex_shade_points")
    if want_features:
        return rgb, sigma, feats
    return rgb, sigma


@torch.no_grad()
def shade_composite_vertex_baked_frame(mesh_intersect, vertex_features, xyz_c, dirs_c, frame, render_step_size: float,
                                       stop_tau: float, render_bkgd=None, bg_color="white", packed: bool = False):
    """``shade_vertex_baked_points`` + ``composite_frame`` of a frame in the intersector's tile order as ONE launch that
    walks every pixel front to back (``qf_vertex_composite_tiles``) and stops reading vertex rows once the optical depth
    in front of a pixel's next sample exceeds ``stop_tau`` (``early_stop_tau``; ``inf`` never stops and gives the two
    calls' pixels bit for bit).  Arguments and returns as ``shade_composite_baked_frame``; ``vertex_features`` a tensor or a
    ``baking.VertexBakedFeatures`` (inference either way: the tile-order frame has no backward), or a
    ``baking.QuantisedVertexFeatures`` (``qf_vertex_quant_composite_tiles``)."""
    if getattr(frame, "band_rows", 0) or frame.tri_c is None:
        raise ValueError("shade_composite_vertex_baked_frame: an unbanded frame with triangle ids (want_tri) is required")
    quant = isinstance(vertex_features, QuantisedVertexFeatures)          # qf_vertex_quant_composite_tiles: same pixels as
    if quant:                                                             # on its dequantise() table
        shading, keep = vertex_quant_shading_struct(mesh_intersect, vertex_features)
    else:
        shading, keep = vertex_baked_shading_struct(mesh_intersect, vertex_features)
    xyz_c, dirs_c = _C.f32c(xyz_c), _C.f32c(dirs_c)
    dev = xyz_c.device
    n = frame.depth_c.shape[0]
    if xyz_c.shape[0] != n or dirs_c.shape[0] != n or frame.tri_c.shape[0] != n:
        raise ValueError(f"shade_composite_vertex_baked_frame: {n} slots in the frame, {xyz_c.shape[0]} positions, "
                         f"{dirs_c.shape[0]} directions, {frame.tri_c.shape[0]} triangle ids")
    n_rays = frame.width * frame.height
    mode = _BG.get(bg_color, _C.BG_CUSTOM)
    bk = _C.f32c(render_bkgd.detach().reshape(3).to(dev)) if (mode == _C.BG_CUSTOM and render_bkgd is not None) else None
    rgb = alpha = depth = out5 = None
    if packed:
        out5 = torch.empty((n_rays, 5), dtype=torch.float32, device=dev)
    else:
        rgb = torch.empty((n_rays, 3), dtype=torch.float32, device=dev)
        alpha = torch.empty((n_rays, 1), dtype=torch.float32, device=dev)
        depth = torch.empty((n_rays, 1), dtype=torch.float32, device=dev)
    shaded = torch.empty((n_rays,), dtype=torch.int32, device=dev)
    if quant:
        _C.check(_C.lib().qf_vertex_quant_composite_tiles(
            shading.records, shading.n_vertices, shading.n_lobes, shading.sigmoid_codec, shading.lambda_thres,
            shading.tri_records, _C.ptr(xyz_c), _C.ptr(dirs_c), _C.ptr(frame.depth_c), _C.ptr(frame.tri_c, torch.int32),
            _C.ptr(frame.hit_count), frame.max_hits, _C.ptr(frame.tile_base), frame.width, frame.height,
            float(render_step_size), mode, _C.ptr(bk), float(stop_tau), _C.ptr(rgb), _C.ptr(alpha), _C.ptr(depth), _C.ptr(out5),
            _C.ptr(shaded), _C.stream()), "qf_vertex_quant_composite_tiles")
        if packed:
            return out5, None, None, shaded
        return rgb, alpha, depth, shaded
    _C.check(_C.lib().qf_vertex_composite_tiles(
        shading.table, shading.stride, shading.n_lobes, shading.records, _C.ptr(xyz_c), _C.ptr(dirs_c), _C.ptr(frame.depth_c),
        _C.ptr(frame.tri_c, torch.int32), _C.ptr(frame.hit_count), frame.max_hits, _C.ptr(frame.tile_base), frame.width,
        frame.height, float(render_step_size), mode, _C.ptr(bk), float(stop_tau), _C.ptr(rgb), _C.ptr(alpha), _C.ptr(depth),
        _C.ptr(out5), _C.ptr(shaded), _C.stream()), "qf_vertex_composite_tiles")
    if packed:
        return out5, None, None, shaded
    return rgb, alpha, depth, shaded


def render_image_finetune_baking_with_occgrid(
    radiance_field: torch.nn.Module, estimator, rays: Rays, data, near_plane: float = 0.0, far_plane: float = 1e10,
    render_step_size: float = 1e-3, render_bkgd: Optional[torch.Tensor] = None, cone_angle: float = 0.0,
    alpha_thre: float = 0.0, test_chunk_size: int = 8192, timestamps: Optional[torch.Tensor] = None, mesh_intersect=None,
    mesh_finetune=None, scaling=1 / 128, vertex_features=None, bg_color="white",
):
    """Render from SG features kept at the mesh vertices -- utils.py:733-861.  Returns the reference's 8-tuple (colors,
    opacities, depths, n_samples, weights, positions, rays, 0); ``positions`` is, as there, the three corner positions of
    every sample's triangle, [3n, 3].  The reference evaluates ``radiance_field.features`` at those 3n corners on every
    call; here the field is evaluated once per VERTEX (``baking.bake_vertex_features``: the same values, the field being a
    function of the position) and the samples gather: ``vertex_features`` (extension) takes that table from the caller,
    ``None`` bakes it once per call.  ``bg_color`` (extension): the reference composites on white.
    The view direction of a sample is the loader's ``dirs`` (``d / (|d| + 1e-7)``, what every other renderer here and the
    tile pack use) where the reference indexes ``rays.viewdirs`` (:840): one ulp apart, and the camera frame of
    ``FrameRenderer.render_vertex_baked`` then equals this function bit for bit.
    ``vertex_features`` may also be a ``baking.VertexBakedFeatures``, whose table is read in place.  With such a module
    whose table requires a gradient, while autograd is recording, colors, opacities and depths carry a graph to the table
    (``_VertexShadeFn`` followed by the differentiable ``derive_properties``); every other call
    runs under ``torch.no_grad()`` and returns tensors without a graph, as before.  A ``baking.QuantisedVertexFeatures``
    (inference only) is shaded from its uint8 records: the values of its ``dequantise()`` table, bit for bit."""
    with torch.set_grad_enabled(_vertex_table_trains(vertex_features)):
        return _render_vertex_baked_ray_major(radiance_field, rays, data, timestamps, mesh_intersect, vertex_features, bg_color)


def _render_vertex_baked_ray_major(radiance_field, rays, data, timestamps, mesh_intersect, vertex_features, bg_color):
    if timestamps is not None:
        raise NotImplementedError("dynamic (D-NeRF) fields are out of scope")
    rays, rays_shape, num_rays = _flatten_rays(rays)
    device = mesh_intersect.device
    if vertex_features is None:
        from .baking import bake_vertex_features
        vertex_features = bake_vertex_features(radiance_field, mesh_intersect)
    xyzs, dirs, index_ray, ts, index_tri, origins = _to_device(data, device)
    if isinstance(data, (SampleSet, SampleWindow)):
        # the device loader's own pack: sorted by (ray, depth) and not displaced since (no deformation here), so the
        # re-sort of sampling_indexing is the identity and the constant step needs no boundaries
        points, depth, deltas, boundary = xyzs, ts, float(mesh_intersect.render_step_size), None
    else:
        points, deltas, boundary, dirs, index_ray, depth, index_tri, _ = mesh_intersect.sampling_indexing(
            xyzs, origins, dirs, index_ray, ts, index_tri)
    rgbs, sigmas = shade_vertex_baked_points(mesh_intersect, vertex_features, points, index_tri, dirs)
    rgb, opacity, _, depth_img, weights = derive_properties(
        rgbs, sigmas, depth, deltas, boundary, index_ray, bg_color=bg_color, render_bkgd=None, N=num_rays)
    corners = mesh_intersect.vertices[_faces_on_device(mesh_intersect)[index_tri]].reshape(-1, 3)
    return (rgb.view((*rays_shape[:-1], -1)), opacity.view((*rays_shape[:-1], -1)),
            depth_img.view((*rays_shape[:-1], -1)), xyzs.shape[0], weights, corners, rays, 0)


def render_image_with_occgrid(
    radiance_field: torch.nn.Module, estimator, rays: Rays, near_plane: float = 0.0, far_plane: float = 1e10,
    render_step_size: float = 1e-3, render_bkgd: Optional[torch.Tensor] = None, cone_angle: float = 0.0,
    alpha_thre: float = 0.0, test_chunk_size: int = 8192, timestamps: Optional[torch.Tensor] = None,
    use_eps_loss: bool = False,
):
    """Occupancy-grid ray marching + nerfacc ``rendering`` -- utils.py:65-172 of the reference (the stage-1/2 renderer
    and the ``rgb_full`` branch of finetuning).  Returns (colors, opacities, depths, n_samples, extras) with the
    image shape of ``rays``.  The reference splits evaluation into ``test_chunk_size`` ray chunks to bound memory;
    one chunk of any size gives the same result here, so the whole image is marched at once.
    Under ``torch.no_grad()`` everything is a fused kernel; when autograd is recording and the field trains (the
    ``rgb_full`` term of train_finetune.py:513-523) the sampling stays non-differentiable, as in nerfacc, and the
    field + ``rendering`` take their differentiable routes."""
    from .field_rendering import rendering
    if timestamps is not None:
        raise NotImplementedError("dynamic (D-NeRF) fields are out of scope")
    rays, rays_shape, num_rays = _flatten_rays(rays)
    device = estimator.aabbs.device
    origins = _C.f32c(rays.origins.to(device))
    viewdirs = _C.f32c(rays.viewdirs.to(device))

    def positions_of(t_starts, t_ends, ray_indices):
        return origins[ray_indices] + viewdirs[ray_indices] * (t_starts + t_ends)[:, None] / 2.0

    def sigma_fn(t_starts, t_ends, ray_indices):
        return radiance_field.query_density(positions_of(t_starts, t_ends, ray_indices)).squeeze(-1)

    def rgb_sigma_fn(t_starts, t_ends, ray_indices):
        rgbs, sigmas = radiance_field(positions_of(t_starts, t_ends, ray_indices), viewdirs[ray_indices])
        return rgbs, sigmas.squeeze(-1)

    ray_indices, t_starts, t_ends = estimator.sampling(
        origins, viewdirs, sigma_fn=sigma_fn, near_plane=near_plane, far_plane=far_plane,
        render_step_size=render_step_size, stratified=radiance_field.training, cone_angle=cone_angle,
        alpha_thre=alpha_thre)
    rgb, opacity, depth, extras = rendering(t_starts, t_ends, ray_indices, n_rays=num_rays, rgb_sigma_fn=rgb_sigma_fn,
                                            render_bkgd=render_bkgd)
    extras["t_starts"], extras["t_ends"], extras["ray_indices"] = t_starts, t_ends, ray_indices
    extras["t_origins"] = origins
    return (rgb.view((*rays_shape[:-1], -1)), opacity.view((*rays_shape[:-1], -1)), depth.view((*rays_shape[:-1], -1)),
            int(t_starts.shape[0]), extras)


@torch.no_grad()
def render_image_with_occgrid_test(
    max_samples: int, radiance_field: torch.nn.Module, estimator, rays: Rays, near_plane: float = 0.0,
    far_plane: float = 1e10, render_step_size: float = 1e-3, render_bkgd: Optional[torch.Tensor] = None,
    cone_angle: float = 0.0, alpha_thre: float = 0.0, early_stop_eps: float = 1e-4,
    timestamps: Optional[torch.Tensor] = None, trace: Optional[list] = None,
):
    """The test-time volumetric renderer with early ray termination -- utils.py:176-350 of the reference (the NeRF frame
    of the paper's speed comparison; ``mc_utils.grid_transmittance_synthetic`` builds its mask from the positions).
    Returns (colors, opacities, depths, total_samples, positions): the first three in the image shape of ``rays``,
    ``depths`` NOT divided by the opacity (the reference has that line commented out), ``total_samples`` the samples left
    by the alpha filter, ``positions`` every marched sample, round by round, within a round by ray and depth.

    The frame is rendered in rounds: the alive rays march ``max(min(num_rays // n_alive, 64), 1)``
    kept samples on from their near planes (``qf_grid_march_round_count`` / ``_write``), the field shades exactly those,
    ``qf_volumetric_accumulate`` composites them and retires every ray whose opacity has passed ``1 - early_stop_eps`` or
    that left the box.  Round buffers are ``num_rays`` rows, allocated once.  The host reads one pinned block per round
    (the alive count the round started with and its sample count), where the reference calls ``.item()``; the sample
    quota itself never leaves the device.  ``NGPRadianceField`` / ``NGPRadianceFieldSGNew`` take their fused kernels with
    the round's sample count read from device memory; any other module is called as ``radiance_field(positions, dirs)``
    on the round's rows.  ``trace`` (extension): a list that receives one dict per round -- ``n_alive``, ``n_samples``,
    ``ray_indices``, ``t_starts``, ``t_ends``, and the ``alive`` mask and ``near`` planes after the round."""
    from .radiance_fields.ngp import NGPRadianceField, NGPRadianceFieldSGNew
    if timestamps is not None:
        raise NotImplementedError("dynamic (D-NeRF) fields are out of scope")
    if cone_angle != 0.0:
        raise NotImplementedError("cone_angle > 0 (unbounded scenes) is out of scope")
    if int(max_samples) <= 0:
        raise ValueError(f"max_samples must be positive, got {max_samples}")
    if not (rays.origins.is_cuda and rays.viewdirs.is_cuda and estimator.binaries.is_cuda):
        raise ValueError("render_image_with_occgrid_test needs device tensors (quadraturefields_amd has no CPU fallback)")
    rays, rays_shape, num_rays = _flatten_rays(rays)
    device = rays.origins.device
    origins, viewdirs = _C.f32c(rays.origins), _C.f32c(rays.viewdirs)
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=device)
    rgb = torch.zeros((num_rays, 3), device=device)
    opacity = torch.zeros((num_rays, 1), device=device)
    depth = torch.zeros((num_rays, 1), device=device)
    positions_all = []
    total_samples = 0
    if num_rays:
        near = torch.full((num_rays,), float(near_plane), dtype=torch.float32, device=device)
        alive = torch.ones((num_rays,), dtype=torch.uint8, device=device)
        state = torch.zeros((_C.VOLUMETRIC_STATE_WORDS,), dtype=torch.int64, device=device)
        state[0] = num_rays
        host = torch.empty((_C.VOLUMETRIC_STATE_WORDS,), dtype=torch.int64).pin_memory()
        count, term = new((num_rays,), torch.int32), new((num_rays,), torch.float32)
        csum = new((num_rays,), torch.int64)
        t_starts, t_ends = new((num_rays,), torch.float32), new((num_rays,), torch.float32)
        ray_indices = new((num_rays,), torch.int64)
        xyz, dirs = new((num_rays, 3), torch.float32), new((num_rays, 3), torch.float32)
        n_round = state[_C.VOLUMETRIC_ROUND_SAMPLES:_C.VOLUMETRIC_ROUND_SAMPLES + 1]
        fused = isinstance(radiance_field, (NGPRadianceField, NGPRadianceFieldSGNew))
        aabb, res = estimator._host_geometry()
        binaries = estimator.binaries[0].contiguous()
        lib = _C.lib()
        march = (aabb, res, _C.ptr(binaries), _C.ptr(origins), _C.ptr(viewdirs), _C.ptr(near), _C.ptr(alive), num_rays,
                 float(near_plane), float(far_plane), float(render_step_size), _C.ptr(state))
        iter_samples, parity = 0, 0
        while iter_samples < max_samples:
            # the round is marched before the host knows whether a ray is still alive: with none the launches write nothing
            _C.check(lib.qf_grid_march_round_count(*march, parity, _C.ptr(count), _C.ptr(term), _C.stream()),
                     "qf_grid_march_round_count")
            torch.cumsum(count, dim=0, out=csum)
            _C.check(lib.qf_grid_march_round_write(*march, parity, _C.ptr(count), _C.ptr(csum), num_rays, _C.ptr(t_starts),
                                                   _C.ptr(t_ends), _C.ptr(ray_indices), _C.ptr(xyz), _C.ptr(dirs),
                                                   _C.stream()), "qf_grid_march_round_write")
            host.copy_(state, non_blocking=True)
            torch.cuda.current_stream(device).synchronize()          # the round's one read-back
            n_alive, n_marched = int(host[parity]), int(host[_C.VOLUMETRIC_ROUND_SAMPLES])
            if n_alive == 0:
                break
            n_samples = max(min(num_rays // n_alive, 64), 1)
            iter_samples += n_samples
            if fused:
                rgbs, sigmas = radiance_field(xyz, dirs, n_device=n_round)
            elif n_marched:
                rgbs, sigmas = radiance_field(xyz[:n_marched], dirs[:n_marched])
            else:
                rgbs, sigmas = xyz, term                             # no sample to shade: nothing reads them
            rgbs, sigmas = _C.f32c(rgbs.reshape(-1, 3)), _C.f32c(sigmas.reshape(-1))
            if rgbs.shape[0] != sigmas.shape[0] or (n_marched and rgbs.shape[0] < n_marched):
                raise ValueError(f"the field returned {rgbs.shape[0]} colours and {sigmas.shape[0]} densities for "
                                 f"{n_marched} samples")
            _C.check(lib.qf_volumetric_accumulate(
                _C.ptr(t_starts), _C.ptr(t_ends), _C.ptr(sigmas), _C.ptr(rgbs), _C.ptr(count), _C.ptr(csum), _C.ptr(term),
                num_rays, max(min(num_rays, rgbs.shape[0]), 1), float(alpha_thre), float(early_stop_eps), _C.ptr(state),
                parity, _C.ptr(rgb), _C.ptr(opacity), _C.ptr(depth), _C.ptr(near), _C.ptr(alive), _C.stream()),
                "qf_volumetric_accumulate")
            positions_all.append(xyz[:n_marched].clone())
            if trace is not None:
                trace.append({"n_alive": n_alive, "n_samples": n_samples, "ray_indices": ray_indices[:n_marched].clone(),
                              "t_starts": t_starts[:n_marched].clone(), "t_ends": t_ends[:n_marched].clone(),
                              "alive": alive.bool(), "near": near.clone()})
            parity ^= 1
        total_samples = int(state[_C.VOLUMETRIC_TOTAL_SAMPLES].item())
    if render_bkgd is not None:
        rgb = rgb + render_bkgd.to(device) * (1.0 - opacity)
    positions = torch.cat(positions_all, dim=0) if positions_all else torch.zeros((0, 3), device=device)
    return (rgb.view((*rays_shape[:-1], -1)), opacity.view((*rays_shape[:-1], -1)), depth.view((*rays_shape[:-1], -1)),
            total_samples, positions)


def render_image_field_with_occgrid(
    radiance_field: torch.nn.Module, estimator, rays: Rays, near_plane: float = 0.0, far_plane: float = 1e10,
    render_step_size: float = 1e-3, render_bkgd: Optional[torch.Tensor] = None, cone_angle: float = 0.0,
    alpha_thre: float = 0.0, test_chunk_size: int = 8192, timestamps: Optional[torch.Tensor] = None,
):
    """Occupancy-grid ray marching + ``rendering_field`` -- utils.py:353-462 of the reference (imported by
    train_finetune.py:21 and test_baking_texture_images.py:26, called by train_field.py:330): the renderer that also
    returns the weights of the reversed rays.  Returns the reference's 8-tuple (colors, opacities, depths, n_samples,
    weights, weights_rev, positions, dirs).  The chunk loop of the reference is kept (``test_chunk_size`` rays per
    chunk at eval, one chunk in training): colours / opacities / depths / weights do not depend on it, but
    ``weights_rev`` does -- ``rendering_field`` applies the chunk's ascending pack layout to the flipped samples
    (field_rendering.py:575-733), so a chunk's reversed weights depend on which rays share the chunk.  Sampling uses
    ``early_stop_eps=1e-4`` as the reference passes it (utils.py:437)."""
    from .field_rendering import rendering_field
    if timestamps is not None:
        raise NotImplementedError("dynamic (D-NeRF) fields are out of scope")
    rays, rays_shape, num_rays = _flatten_rays(rays)
    device = estimator.aabbs.device
    origins = _C.f32c(rays.origins.to(device))
    viewdirs = _C.f32c(rays.viewdirs.to(device))
    results = []
    chunk = torch.iinfo(torch.int32).max if radiance_field.training else int(test_chunk_size)
    for i in range(0, num_rays, chunk):
        c_origins, c_dirs = origins[i:i + chunk], viewdirs[i:i + chunk]

        def positions_of(t_starts, t_ends, ray_indices):
            return c_origins[ray_indices] + c_dirs[ray_indices] * (t_starts + t_ends)[:, None] / 2.0

        def sigma_fn(t_starts, t_ends, ray_indices):
            return radiance_field.query_density(positions_of(t_starts, t_ends, ray_indices)).squeeze(-1)

        def rgb_sigma_fn(t_starts, t_ends, ray_indices):
            rgbs, sigmas = radiance_field(positions_of(t_starts, t_ends, ray_indices), c_dirs[ray_indices])
            return rgbs, sigmas.squeeze(-1)

        ray_indices, t_starts, t_ends = estimator.sampling(
            c_origins, c_dirs, sigma_fn=sigma_fn, near_plane=near_plane, far_plane=far_plane,
            render_step_size=render_step_size, stratified=radiance_field.training, cone_angle=cone_angle,
            alpha_thre=alpha_thre, early_stop_eps=1e-4)
        n_chunk = c_origins.shape[0]
        if t_starts.shape[0] == 0:
            # the reference's rendering_field takes torch.max of an empty tensor here and raises; a chunk of pure
            # background is ordinary at eval (8192 rays of an image corner), so it renders as background instead
            colors = torch.zeros((n_chunk, 3), device=device)
            if render_bkgd is not None:
                colors = colors + render_bkgd.to(device)
            empty = torch.zeros((0,), device=device)
            results.append([colors, torch.zeros((n_chunk, 1), device=device), torch.zeros((n_chunk, 1), device=device),
                            0, empty, empty, torch.zeros((0, 3), device=device), torch.zeros((0, 3), device=device)])
            continue
        rgb, opacity, depth, weights, weights_rev = rendering_field(
            t_starts, t_ends, ray_indices, n_rays=n_chunk, rgb_sigma_fn=rgb_sigma_fn, render_bkgd=render_bkgd)
        results.append([rgb, opacity, depth, int(t_starts.shape[0]), weights, weights_rev,
                        positions_of(t_starts, t_ends, ray_indices), c_dirs[ray_indices]])
    colors, opacities, depths, n_rendering_samples, weights, weights_rev, positions, dirs = [
        torch.cat(r, dim=0) if isinstance(r[0], torch.Tensor) else r for r in zip(*results)]
    return (colors.view((*rays_shape[:-1], -1)), opacities.view((*rays_shape[:-1], -1)),
            depths.view((*rays_shape[:-1], -1)), sum(n_rendering_samples), weights, weights_rev, positions, dirs)
