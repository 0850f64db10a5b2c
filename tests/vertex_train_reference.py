"""The gradient of the vertex-baked shading with respect to the vertex table in float64, on the
CPU: the fp32 barycentrics of ``vertex_baked_reference.barycentrics`` promoted, the blend in the stated order, the SG
mixture and the sigmoid in float64 torch, ``autograd.grad`` with respect to the table.  A sample whose barycentrics are
not finite (a degenerate face, a face with an id out of range) contributes nothing, which is the kernel's rule.  Also the
float64 chain of the whole ray-major renderer (``oracle.volrend.derive_properties`` promoted) and the per-column
comparison the GPU tests use.  No tests in here, no device."""
import numpy as np
import torch

from oracle import meshpath as om
from oracle import volrend
from tests import vertex_baked_reference as R

# The bar the project holds its SG gradients to: no measured tolerance may exceed it.
TOL_CEILING = 3e-4


def sg_rgb(blend: torch.Tensor, dirs: torch.Tensor, n_lobes: int) -> torch.Tensor:
    """sigmoid(diffuse + sum over lobes of colour * exp(|lambda| (axis / |axis| . dir - 1))) in the dtype of ``blend``."""
    pre = blend[:, :3]
    for l in range(n_lobes):
        o = 3 + 7 * l
        axis = blend[:, o:o + 3]
        axis = axis / axis.norm(dim=1, keepdim=True)
        e = torch.exp(blend[:, o + 3].abs() * ((axis * dirs).sum(dim=1) - 1.0))
        pre = pre + blend[:, o + 4:o + 7] * e[:, None]
    return torch.sigmoid(pre)


def shade64(table64: torch.Tensor, faces_v: np.ndarray, b32: np.ndarray, dirs, n_lobes: int):
    """(rgb [n,3], sigma [n]) in float64 from a float64 table [V, W], the samples' vertex ids [n,3] and their fp32
    barycentrics [n,3]; differentiable with respect to ``table64``."""
    b = torch.from_numpy(np.asarray(b32, dtype=np.float32)).double()
    f = torch.from_numpy(np.asarray(faces_v, dtype=np.int64))
    blend = (table64[f[:, 0]] * b[:, 0:1] + table64[f[:, 1]] * b[:, 1:2]) + table64[f[:, 2]] * b[:, 2:3]
    d = torch.as_tensor(dirs).double()
    return sg_rgb(blend, d, n_lobes), blend[:, -1]


def table_gradient(features, vertices64, faces, points, index_tri, dirs, d_rgb, d_sigma, n_lobes) -> np.ndarray:
    """float64 [V, W]: d(sum d_rgb . rgb + sum d_sigma sigma) / d table; ``features`` [V, W] fp32 (unpadded), ``d_sigma``
    None = the density column gets no gradient.  Samples with non-finite barycentrics are left out."""
    faces = np.array(faces, dtype=np.int64)
    bad = ((faces < 0) | (faces >= np.asarray(vertices64).shape[0])).any(axis=1)
    faces[bad] = 0                                           # qf_vertex_records_pack's rule
    index_tri = np.asarray(index_tri)
    b = R.barycentrics(vertices64, faces, np.asarray(points), index_tri)
    keep = np.isfinite(b).all(axis=1)
    table = torch.from_numpy(np.asarray(features, dtype=np.float32)).double().requires_grad_(True)
    if not keep.any():
        return np.zeros(tuple(table.shape))
    with torch.enable_grad():
        rgb, sigma = shade64(table, faces[index_tri[keep]], b[keep], torch.as_tensor(dirs)[torch.from_numpy(keep)], n_lobes)
        loss = (rgb * torch.as_tensor(d_rgb).double()[torch.from_numpy(keep)]).sum()
        if d_sigma is not None:
            loss = loss + (sigma * torch.as_tensor(d_sigma).double()[torch.from_numpy(keep)]).sum()
        return torch.autograd.grad(loss, table)[0].numpy()


def render_gradient(features, vertices64, faces, data, n_rays, n_lobes, A, B, bg_color="white", render_step_size=R.DELTA):
    """float64 [V, W]: d(sum(rgb . A) + sum(alpha . B)) / d table through ``vertex_baked_reference.render``'s chain --
    sampling_indexing, the fp32 barycentrics promoted, the blend, the SG mixture, ``oracle.volrend.derive_properties`` on
    float64 colours and densities.  Also returns the chain's (rgb, alpha) in float32, as the oracle stores them."""
    xyzs, dirs, index_ray, ts, index_tri, origins = data
    points, deltas, boundary, dirs, index_ray, depth, index_tri, _ = om.sampling_indexing(
        xyzs, origins, dirs, index_ray, ts, index_tri, render_step_size)
    faces = np.asarray(faces, dtype=np.int64)
    b = R.barycentrics(vertices64, faces, points.numpy(), index_tri.numpy())
    table = torch.from_numpy(np.asarray(features, dtype=np.float32)).double().requires_grad_(True)
    with torch.enable_grad():
        rgbs, sigmas = shade64(table, faces[index_tri.numpy()], b, dirs, n_lobes)
        rgb, alpha, _, _, _ = volrend.derive_properties(rgbs, sigmas, depth.double(), torch.as_tensor(deltas).double(), boundary,
                                                        index_ray, bg_color=bg_color, render_bkgd=None, N=n_rays)
        loss = (rgb.double() * torch.as_tensor(A).double()).sum() + (alpha.double() * torch.as_tensor(B).double()).sum()
        return torch.autograd.grad(loss, table)[0].numpy(), rgb.detach(), alpha.detach()


def column_ratio(got, want) -> float:
    """max over the columns c of max|got[:, c] - want[:, c]| / max|want[:, c]|: the per-column error the tolerance bounds.
    A column whose reference is all zero must be exactly zero in ``got`` (ratio 0, inf otherwise)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    scale = np.abs(want).max(axis=0)
    err = np.abs(got - want).max(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(scale > 0, err / scale, np.where(err > 0, np.inf, 0.0))
    return float(ratio.max())


def random_table(n_vertices: int, n_lobes: int, seed: int) -> np.ndarray:
    """The seeded random table of the kernel tests, float32 [V, W]: columns ~N(0,1), lambda columns x4, density |N| * 10."""
    g = np.random.default_rng(seed)
    w = R.row_width(n_lobes)
    t = g.normal(size=(n_vertices, w))
    for l in range(n_lobes):
        t[:, 3 + 7 * l + 3] *= 4.0
    t[:, -1] = np.abs(t[:, -1]) * 10.0
    return t.astype(np.float32)


def contributions(n_vertices: int, faces, index_tri) -> np.ndarray:
    """int64 [V]: the number of samples that add to each vertex's row."""
    f = np.asarray(faces)[np.asarray(index_tri)]
    return np.bincount(f.reshape(-1), minlength=n_vertices)
