"""Stage 2's grid extraction on the device: ``extract_grid`` / ``extract_density_grid`` of examples/field_utils.py.

``extract_grid`` (field_utils.py:276-318) samples the quadrature ``Field`` on a (2N)^3 lattice, takes the field and the
norm of its spatial gradient, clips the norm to [0, 65504] and average-pools both 2x2x2 on the CPU; ``grids_valid.npy``
(fp32) and ``grads_valid.npy`` (fp16) are stage 3's inputs (``examples/extract_mesh.py``).  ``extract_density_grid``
(:321-341) does the same for the radiance field's ``query_density`` (fp16 ``density_grids_valid.npy``).

Coordinates: the lattice is ``torch.linspace(-1, 1, 2N) * scale`` in fp32 on every axis and output [a, b, c] pools
lattice indices {2a, 2a+1} x {2b, 2b+1} x {2c, 2c+1} -- the reference's ``meshgrid`` ("ij") order.  Pooling equals torch's
CPU ``AvgPool3d`` bit for bit: the eight values summed from 0, first lattice index outermost, then divided by 8
(DESIGN.md §3.10).  Both grids are produced in x-slabs ``[x_begin, x_begin + x_count)`` of whole x-rows, each one
contiguous range of the C-order array, so the ``extract_*`` writers stream them into a host memmap.
"""
import numpy as np
import torch

from . import _C
from .field import Field

FP16_MAX = 65504.0


def lattice_axis(grid_size: int, scale: float, device=None) -> torch.Tensor:
    """The reference's lattice coordinates, ``torch.linspace(-1, 1, 2 grid_size) * scale`` (fp32, computed where the
    reference computes them: on the CPU), on ``device``."""
    axis = torch.linspace(-1, 1, 2 * grid_size) * scale
    return axis if device is None else axis.to(device)


def plan_slabs(grid_size: int, x_slab=None):
    """[(x_begin, x_count)] covering [0, grid_size) once, in order; ``x_slab`` rows per slab (None: the whole grid)."""
    if grid_size < 1:
        raise ValueError(f"grid_size must be >= 1, got {grid_size}")
    step = grid_size if x_slab is None else int(x_slab)
    if step < 1:
        raise ValueError(f"x_slab must be >= 1, got {x_slab}")
    return [(b, min(step, grid_size - b)) for b in range(0, grid_size, step)]


def pool2(t: torch.Tensor) -> torch.Tensor:
    """[2X, 2Y, 2Z] -> [X, Y, Z]: torch's CPU ``AvgPool3d(2, stride=2)`` bit for bit, on the tensor's own device (the
    eight terms added one by one from 0, first index outermost, then / 8; each fp32 add is correctly rounded)."""
    X, Y, Z = t.shape[0] // 2, t.shape[1] // 2, t.shape[2] // 2
    v = t.reshape(X, 2, Y, 2, Z, 2)
    s = torch.zeros((X, Y, Z), dtype=t.dtype, device=t.device)
    for dx in range(2):
        for dy in range(2):
            for dz in range(2):
                s.add_(v[:, dx, :, dy, :, dz])
    return s.div_(8.0)


def _device_of(module) -> torch.device:
    """The module's device (its first parameter or buffer); a plain callable runs on the current HIP device."""
    dev = None
    if isinstance(module, torch.nn.Module):
        dev = next((p.device for p in module.parameters()), None)
        if dev is None:
            dev = next((b.device for b in module.buffers()), None)
    elif torch.cuda.is_available():
        dev = torch.device("cuda", torch.cuda.current_device())
    if dev is None or dev.type != "cuda":
        raise RuntimeError("quadraturefields_amd kernels need tensors on the HIP device (no CPU fallback)")
    return dev


def fused_route(field) -> bool:
    """True when ``field_grids`` takes qf_field_grid_extract for ``field``: a ``Field`` with ``back_prop`` off (the
    kernel does not carry the gradient through the hash grid)."""
    return isinstance(field, Field) and not field.back_prop


def _fused_slab(field: Field, axis, grid_size, x_begin, x_count, value, grad, pool=2):
    name, table = field.extract_entry()
    _C.check(getattr(_C.lib(), name)(
        field.xyz_encoder.grid.desc, _C.ptr(table), float(field.scale), field.hidden_size, field.activation_code,
        *[_C.ptr(t) for t in field.decoder_arrays()], _C.ptr(axis, torch.float32), grid_size, x_begin, x_count, pool,
        None, 0, None, _C.ptr(value, torch.float32), _C.ptr(grad, torch.float16), _C.stream()), name)


def _field_value_grad(field, x):
    """(value [M], d value / dx [M,3]) through autograd, ``create_graph=False``."""
    x = x.detach().requires_grad_(True)
    if isinstance(field, Field):
        f = field.field(x)
        g = field.field_grad(x, f, create_graph=False)
    else:
        f, g = field(x)
    return f.detach().reshape(-1), g.detach()


def _autograd_slab(field, axis, grid_size, x_begin, x_count, value, grad, batch=1 << 20):
    """The reference-shaped route for any ``field(x) -> (f, grad)``: lattice points of one x-row pair at a time through
    autograd in batches, |grad| clipped, then ``pool2``."""
    L = 2 * grid_size
    yz = torch.stack(torch.meshgrid(axis, axis, indexing="ij"), -1).reshape(-1, 2)
    with torch.enable_grad():
        for a in range(x_begin, x_begin + x_count):
            vals, gns = [], []
            for X in (2 * a, 2 * a + 1):
                pts = torch.cat([axis[X].expand(yz.shape[0], 1), yz], 1)
                for b in range(0, pts.shape[0], batch):
                    f, g = _field_value_grad(field, pts[b:b + batch])
                    vals.append(f)
                    gns.append(torch.clip(torch.linalg.norm(g, dim=-1), 0, FP16_MAX))
            r = a - x_begin
            value[r] = pool2(torch.cat(vals).reshape(2, L, L))[0]
            grad[r] = pool2(torch.cat(gns).reshape(2, L, L))[0].to(torch.float16)


def _grid_slab(field, axis, grid_size, x_begin, x_count, value, grad):
    if fused_route(field):
        _fused_slab(field, axis, grid_size, x_begin, x_count, value, grad)
    else:
        _autograd_slab(field, axis, grid_size, x_begin, x_count, value, grad)


def field_grids(field, grid_size: int = 1024, scale=None, x_slab=None):
    """The two grids of ``extract_grid`` on the device: (value fp32 [N,N,N], |grad| fp16 [N,N,N]).  ``field``: a
    ``Field`` (qf_field_grid_extract unless ``back_prop``) or any callable ``field(x) -> (f, grad)`` (the
    reference-shaped autograd route); ``scale`` defaults to ``field.scale``."""
    if scale is None:
        scale = field.scale
    dev = _device_of(field)
    axis = lattice_axis(grid_size, scale, dev)
    value = torch.empty((grid_size,) * 3, dtype=torch.float32, device=dev)
    grad = torch.empty((grid_size,) * 3, dtype=torch.float16, device=dev)
    with torch.no_grad():
        for xb, xc in plan_slabs(grid_size, x_slab):
            _grid_slab(field, axis, grid_size, xb, xc, value[xb:xb + xc], grad[xb:xb + xc])
    return value, grad


def _slab_rows(grid_size: int, bytes_per_voxel: int, budget: int = 1 << 30) -> int:
    return max(1, min(grid_size, budget // (bytes_per_voxel * grid_size * grid_size)))


def extract_grid(field_grid, prefix, scale, grid_size: int = 1024):
    """field_utils.py:276-318: ``{prefix}/grids_valid.npy`` (float32) and ``{prefix}/grads_valid.npy`` (float16),
    [N,N,N] each, streamed slab by slab (host memory stays at the output size)."""
    dev = _device_of(field_grid)
    axis = lattice_axis(grid_size, scale, dev)
    shape = (grid_size,) * 3
    grids = np.lib.format.open_memmap("{}/grids_valid.npy".format(prefix), mode="w+", dtype=np.float32, shape=shape)
    grads = np.lib.format.open_memmap("{}/grads_valid.npy".format(prefix), mode="w+", dtype=np.float16, shape=shape)
    rows = _slab_rows(grid_size, 6)
    value = torch.empty((rows, grid_size, grid_size), dtype=torch.float32, device=dev)
    grad = torch.empty((rows, grid_size, grid_size), dtype=torch.float16, device=dev)
    with torch.no_grad():
        for xb, xc in plan_slabs(grid_size, rows):
            _grid_slab(field_grid, axis, grid_size, xb, xc, value[:xc], grad[:xc])
            grids[xb:xb + xc] = value[:xc].cpu().numpy()
            grads[xb:xb + xc] = grad[:xc].cpu().numpy()
    grids.flush()
    grads.flush()
    del grids, grads


def _density_slab(model, axis, grid_size, x_begin, x_count, out):
    """Lattice points of x-rows [x_begin, x_begin + x_count) built on the device, the model's fused ``query_density``,
    clip to [0, 65504], ``pool2``, fp16."""
    L = 2 * grid_size
    xs = axis[2 * x_begin:2 * (x_begin + x_count)]
    pts = torch.stack(torch.meshgrid(xs, axis, axis, indexing="ij"), -1).reshape(-1, 3)
    sigma = model.query_density(pts).reshape(2 * x_count, L, L)
    out.copy_(pool2(torch.clip(sigma, 0, FP16_MAX)).to(torch.float16))


def density_grid(model, scale, grid_size: int = 1024, x_slab=None):
    """The grid of ``extract_density_grid`` on the device: fp16 [N,N,N]."""
    dev = _device_of(model)
    axis = lattice_axis(grid_size, scale, dev)
    out = torch.empty((grid_size,) * 3, dtype=torch.float16, device=dev)
    rows = _slab_rows(grid_size, 8 * 4 * 5) if x_slab is None else x_slab
    with torch.no_grad():
        for xb, xc in plan_slabs(grid_size, rows):
            _density_slab(model, axis, grid_size, xb, xc, out[xb:xb + xc])
    return out


def extract_density_grid(model, scale, prefix, grid_size: int = 512):
    """field_utils.py:321-341: ``prefix + "density_grids_valid.npy"`` (float16 [N,N,N]), streamed slab by slab."""
    dev = _device_of(model)
    axis = lattice_axis(grid_size, scale, dev)
    grids = np.lib.format.open_memmap(prefix + "density_grids_valid.npy", mode="w+", dtype=np.float16,
                                      shape=(grid_size,) * 3)
    rows = _slab_rows(grid_size, 8 * 4 * 5)
    out = torch.empty((rows, grid_size, grid_size), dtype=torch.float16, device=dev)
    with torch.no_grad():
        for xb, xc in plan_slabs(grid_size, rows):
            _density_slab(model, axis, grid_size, xb, xc, out[:xc])
            grids[xb:xb + xc] = out[:xc].cpu().numpy()
    grids.flush()
    del grids
