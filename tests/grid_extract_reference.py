"""fp64 restatement of the reference's grid extraction (examples/field_utils.py:276-341), for the tests.

``extract_grid``: the stage-2 ``Field`` (field.py:130-238, ``back_prop=False``) at every lattice point -- the hash
encoding by ``oracle.fields.hash_encode`` (the tcnn rule, fp32), the decoder and its gradient with respect to the three
x01 columns in fp64 through autograd, d/dx = d/dx01 / (2 scale) -- then |grad| clipped to [0, 65504] and both grids
2x2x2-averaged.  ``extract_density_grid``: ``oracle.fields.query_density`` on the lattice, clipped and averaged.  With
``round16`` the table and the 32 encoding outputs are rounded to fp16 where the reference's fp16 tcnn ``Encoding`` rounds
them (tests/fp16_deform_reference.py).
"""
import torch
import torch.nn.functional as F

from oracle import fields as ofields
from tests.fp16_reference import half_round

FP16_MAX = 65504.0


def lattice_axis(grid_size: int, scale: float) -> torch.Tensor:
    """field_utils.py:278,289-291: torch.linspace(-1, 1, 2N) (CPU), the lattice's coordinates times ``scale``."""
    return torch.linspace(-1, 1, 2 * grid_size) * scale


def lattice_points(axis: torch.Tensor, xs=None) -> torch.Tensor:
    """[(len(xs) or len(axis)) * len(axis)^2, 3] fp32, meshgrid "ij" order (x outermost)."""
    xs = axis if xs is None else xs
    return torch.stack(torch.meshgrid(xs, axis, axis, indexing="ij"), -1).reshape(-1, 3)


def field_value_grad(x: torch.Tensor, wts: ofields.DeformWeights, nl: str, round16: bool = False):
    """(value [M] fp64, |d value / dx| [M] fp64, unclipped) of Field.density at fp32 points x [M,3]."""
    x01 = ((x + wts.scale) / (wts.scale + wts.scale)).float()
    table = half_round(wts.table) if round16 else wts.table
    h = ofields.hash_encode(x01, table, wts.levels)
    if round16:
        h = half_round(h)
    act = F.elu if nl == "elu" else F.relu
    with torch.enable_grad():
        xd = x01.double().requires_grad_(True)
        z = torch.cat([xd, h.double()], 1)
        for w, b in wts.layers[:-1]:
            z = act(F.linear(z, w.double(), b.double()))
        w, b = wts.layers[-1]
        out = F.linear(z, w.double(), b.double())[:, 0]
        g, = torch.autograd.grad(out.sum(), [xd])
    g = g / (2.0 * wts.scale)
    return out.detach(), g.norm(dim=-1)


def pool(t: torch.Tensor) -> torch.Tensor:
    """[2X, 2Y, 2Z] -> [X, Y, Z] mean (fp64)."""
    return F.avg_pool3d(t[None, None].double(), 2, 2)[0, 0]


def extract_grid(wts: ofields.DeformWeights, nl: str, grid_size: int, scale: float, round16: bool = False):
    """(value [N,N,N], clipped |grad| [N,N,N]) in fp64: pooled but not rounded to the file dtypes."""
    axis = lattice_axis(grid_size, scale)
    L = 2 * grid_size
    v, g = field_value_grad(lattice_points(axis), wts, nl, round16)
    return pool(v.reshape(L, L, L)), pool(g.clamp(0, FP16_MAX).reshape(L, L, L))


def extract_grid_voxels(wts, nl, grid_size: int, scale: float, idx: torch.Tensor, round16: bool = False):
    """The voxels idx [K,3] (int64) of ``extract_grid`` only: (value [K], clipped |grad| [K]) in fp64."""
    axis = lattice_axis(grid_size, scale)
    e = torch.tensor([[dx, dy, dz] for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)])
    lat = (2 * idx[:, None, :] + e[None]).reshape(-1, 3)
    v, g = field_value_grad(axis[lat], wts, nl, round16)
    return v.reshape(-1, 8).mean(1), g.clamp(0, FP16_MAX).reshape(-1, 8).mean(1)


def extract_density_grid(wts: ofields.NGPWeights, grid_size: int, scale: float):
    """fp64 pooled density, clipped to [0, 65504] (query_density in the oracle's own precision)."""
    axis = lattice_axis(grid_size, scale)
    L = 2 * grid_size
    sigma = ofields.query_density(lattice_points(axis), wts)[:, 0].double()
    return pool(sigma.clamp(0, FP16_MAX).reshape(L, L, L))
