"""Mesh extraction of the reference's ``examples/marching_cubes.py`` on the device.

The reference smooths and normalises its saved grids on the GPU, copies the 1024^3 volume to the host and runs
scikit-image's marching cubes there, twice: over ``sin(omega * q)`` for the nested quadrature surfaces and over the NeRF
density.  Here the marching cubes is the HIP kernel of ``csrc/marching_cubes.hip`` (``qf_marching_cubes_count`` /
``qf_marching_cubes_emit``, rules in DESIGN.md section 3.8); the steps around it stay torch ops on the device.
``transmittance_mask`` is the device form of ``grid_transmittance_synthetic`` (examples/mc_utils.py:462-570).
``compact_mesh_device`` / ``compact_mesh`` clean a mesh (keep mask, degenerate and duplicate faces, small islands,
unreferenced vertices; ``csrc/mesh_compact.hip``, rules in DESIGN.md section 3.9b), and ``prunning_mesh_train_visibility``
/ ``prunning_mesh_train_visibility_complement`` are the reference's visibility pruning (examples/mc_utils.py:272-345) on
top of them.
``mesh_edges_device`` / ``subdivide_mesh_device`` / ``subdivide_mesh`` number a mesh's edges and split its faces at the
midpoints of any marked subset of them, conformingly (``csrc/mesh_subdivide.hip``, rules in DESIGN.md section 3.9c).
"""
import ctypes
import math
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from . import _C
from ._mesh_args import (counts_buffer, mask_u8, mesh_inputs, raise_invalid_faces, read_counts, to_numpy, trimesh_tensors,
                         workspace, zero_counts)
from .mesh_io import TriMesh
from .parameterization_utils import concatenate_meshes


def marching_cubes(volume: torch.Tensor, level: float):
    """``(verts, faces)``: device fp32 [V,3] in array-index coordinates (``verts[:,0]`` is the axis-0 index) and int32
    [F,3], faces wound from inside (``volume > level``) to outside.  ``volume`` is a device fp32 or fp16 [n0,n1,n2]
    tensor (fp16 is widened exactly).  Raises ValueError for a host tensor, a shape that is not 3-D with every
    dimension >= 2 (or is too large), a non-finite level, a non-finite sample, or totals that do not fit int32."""
    if not isinstance(volume, torch.Tensor):
        raise TypeError("volume must be a torch.Tensor")
    if not volume.is_cuda:
        raise ValueError("marching_cubes needs a device tensor (quadraturefields_amd has no CPU fallback)")
    if volume.ndim != 3 or min(volume.shape) < 2:
        raise ValueError(f"volume must be 3-D with every dimension >= 2, got shape {tuple(volume.shape)}")
    if volume.dtype not in (torch.float32, torch.float16):
        raise TypeError(f"volume must be float32 or float16, got {volume.dtype}")
    level32 = float(np.float32(level))
    if not math.isfinite(level32):
        raise ValueError(f"level must be finite in fp32, got {level}")
    vol = volume.to(torch.float32).contiguous()
    n0, n1, n2 = vol.shape
    lib = _C.lib()
    ws_bytes = int(lib.qf_marching_cubes_workspace_bytes(n0, n1, n2))
    if ws_bytes < 0:
        raise ValueError(f"volume shape {tuple(vol.shape)} is refused (each dimension <= 2^24, n0 n1 n2 < 2^31)")
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=vol.device)
    counts = torch.empty((3,), dtype=torch.int64, device=vol.device)
    with torch.cuda.device(vol.device):
        _C.check(lib.qf_marching_cubes_count(_C.ptr(vol), n0, n1, n2, level32, _C.ptr(ws), ws_bytes, _C.ptr(counts),
                                             _C.stream()), "qf_marching_cubes_count")
        n_verts, n_faces, n_bad = counts.tolist()
        if n_bad:
            raise ValueError(f"volume has {n_bad} samples whose difference from the level is not finite")
        if n_verts >= 2 ** 31 or n_faces >= 2 ** 31:
            raise ValueError(f"the mesh has {n_verts} vertices and {n_faces} faces; both must be < 2^31")
        verts = torch.empty((n_verts, 3), dtype=torch.float32, device=vol.device)
        faces = torch.empty((n_faces, 3), dtype=torch.int32, device=vol.device)
        _C.check(lib.qf_marching_cubes_emit(_C.ptr(vol), n0, n1, n2, level32, _C.ptr(ws), ws_bytes, _C.ptr(verts),
                                            n_verts, _C.ptr(faces), n_faces, _C.stream()), "qf_marching_cubes_emit")
    return verts, faces


def _to_device(x, device) -> torch.Tensor:
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x))
    return t.to(device=device, dtype=torch.float32)


def gaussian_kernel_1d(sigma: float, size: int = 5) -> torch.Tensor:
    """The normalised 1-D factor of ``field_utils.GaussianSmoothing``'s product kernel (fp32, as it is built there):
    the normalised 3-D kernel is the product of three of these."""
    x = torch.arange(size, dtype=torch.float32)
    g = 1 / (sigma * math.sqrt(2 * math.pi)) * torch.exp(-((x - (size - 1) / 2) / sigma) ** 2 / 2)
    return g / g.sum()


def smooth(grid: torch.Tensor, sigma: float) -> torch.Tensor:
    """``GaussianSmoothing(1, 5, sigma, dim=3)`` with ``padding="same"`` (zero padding) as three 1-D passes."""
    w = gaussian_kernel_1d(sigma).tolist()
    x = grid
    for axis in range(3):
        n = x.shape[axis]
        out = torch.zeros_like(x)
        for k, wk in enumerate(w):
            off = k - 2                                        # out[i] += w[k] * x[i + off]
            m = n - abs(off)
            if m <= 0:
                continue
            out.narrow(axis, max(-off, 0), m).add_(x.narrow(axis, max(off, 0), m), alpha=wk)
        x = out
    return x


def quadrature_quantity(grid, grads, binaries, *, sigma=100.0, include_grad=True, grad_thres=0.01,
                        device="cuda") -> torch.Tensor:
    """The masked, normalised field ``q`` whose ``sin(omega * q)`` is meshed (marching_cubes.py:30-58), on the device:
    smoothing, the occupancy ``binaries[0]`` upsampled trilinearly (align_corners) to the grid's shape, min / max
    normalisation to [-1, 1] over ``grid * d``, and the mask ``grads > grad_thres``."""
    dev = _C.resolve_device(device)
    g = _to_device(grid, dev)
    if g.ndim != 3:
        raise ValueError(f"grid must be 3-D, got shape {tuple(g.shape)}")
    g = smooth(g, sigma)
    b = _to_device(binaries[0], dev)
    d = F.interpolate(b[None, None], size=tuple(g.shape), mode="trilinear", align_corners=True)[0, 0]
    mn = (g * d).min()
    g.sub_(mn)
    mx = (g * d).max()
    g.div_(mx + 1e-6)
    g.sub_(0.5).mul_(2)
    q = g * d
    del g, d
    if include_grad:
        q = q * (_to_device(grads, dev) > grad_thres)
    return q


def normalise_vertices(verts: torch.Tensor, n: int) -> torch.Tensor:
    """``v / (N - 1)`` then ``(v - 0.5) * 2``, in float64 as the reference's trimesh vertices are (on verts' device)."""
    v = verts.to(torch.float64) / (n - 1)
    return (v - 0.5) * 2


def _normalised_mesh(verts: torch.Tensor, faces: torch.Tensor, n: int) -> TriMesh:
    return TriMesh(*to_numpy(normalise_vertices(verts, n), faces))


def quadrature_surface_mesh(grid, grads, binaries, *, sigma=100.0, include_grad=True, omega=100.0, thres=0.0,
                            grad_thres=0.01, device="cuda") -> TriMesh:
    """The nested quadrature surfaces: marching cubes of ``sin(omega * q)`` at ``thres`` (marching_cubes.py:30-82)."""
    q = quadrature_quantity(grid, grads, binaries, sigma=sigma, include_grad=include_grad, grad_thres=grad_thres,
                            device=device)
    n = q.shape[0]
    vol = torch.sin(omega * q)
    del q
    verts, faces = marching_cubes(vol, thres)
    return _normalised_mesh(verts, faces, n)


def density_surface_mesh(density_grid, density_thres=10.0, device="cuda") -> TriMesh:
    """The ``mesh_nerf.ply`` half: marching cubes of the NeRF density grid at ``density_thres``, normalised by the
    density grid's own ``N - 1`` (marching_cubes.py:61-69).  fp16 grids (as the reference saves them) are widened."""
    dev = _C.resolve_device(device)
    d = density_grid if isinstance(density_grid, torch.Tensor) else torch.from_numpy(np.asarray(density_grid))
    if d.dtype not in (torch.float16, torch.float32):
        d = d.to(torch.float32)
    d = d.to(dev)
    verts, faces = marching_cubes(d, density_thres)
    return _normalised_mesh(verts, faces, d.shape[0])


def combined_mesh(quadrature: TriMesh, density: TriMesh) -> TriMesh:
    """``mesh.ply``: the quadrature surfaces, then the density mesh (the reference's concatenation order)."""
    return concatenate_meshes([quadrature, density])


CONTRACTIONS = {"average": 0, "quadric": 1}


def simplify_vertex_clustering(vertices: torch.Tensor, faces: torch.Tensor, voxel_size: float,
                               contraction: str = "quadric", return_fallbacks: bool = False):
    """open3d's ``simplify_vertex_clustering(voxel_size, contraction)`` on the device, under the rules of DESIGN.md
    section 3.9: ``(vertices, faces)`` as device fp64 [cells,3] and int64 [F',3].  ``vertices`` is a device float
    tensor [V,3] (fp32 is widened exactly), ``faces`` a device int64 or int32 tensor [F,3].  With
    ``return_fallbacks=True`` the number of quadric cells whose vertex fell back to the mean is returned third.
    Raises ValueError for host tensors, a voxel size that is not positive and finite, non-finite vertices, face indices
    outside [0, V), V or F of 2^31 or more, or more than 2^21 cells along an axis."""
    if contraction not in CONTRACTIONS:
        raise ValueError(f"contraction must be one of {sorted(CONTRACTIONS)}, got {contraction!r}")
    s = float(voxel_size)
    if not (math.isfinite(s) and s > 0):
        raise ValueError(f"voxel_size must be positive and finite, got {voxel_size}")
    v, f, dev, n_v, n_f = mesh_inputs(vertices, faces, "simplify_vertex_clustering", limit="F")
    if n_v == 0:
        if n_f:
            raise_invalid_faces(n_f, 0)
        out = (torch.empty((0, 3), dtype=torch.float64, device=dev), torch.empty((0, 3), dtype=torch.int64, device=dev))
        return out + (0,) if return_fallbacks else out
    lib = _C.lib()
    with torch.cuda.device(dev):
        ws, ws_bytes = workspace("qf_vertex_clustering_workspace_bytes", dev, V=n_v, F=n_f)
        counts = torch.empty((5,), dtype=torch.int64, device=dev)
        _C.check(lib.qf_vertex_clustering_count(_C.ptr(v), n_v, _C.ptr(f), n_f, s, _C.ptr(ws), ws_bytes,
                                                _C.ptr(counts), _C.stream()), "qf_vertex_clustering_count")
        n_cells, n_out, bad_v, bad_f, axis_cells = counts.tolist()
        if bad_v or bad_f:
            raise ValueError(f"{bad_v} vertices are not finite and {bad_f} faces have an index outside [0, {n_v})")
        if axis_cells > 2 ** 21:
            raise ValueError(f"voxel size {s} needs {axis_cells} cells along an axis; at most 2^21 are allowed")
        out_v = torch.empty((n_cells, 3), dtype=torch.float64, device=dev)
        out_f = torch.empty((n_out, 3), dtype=torch.int64, device=dev)
        fallbacks = torch.zeros((1,), dtype=torch.int64, device=dev)
        _C.check(lib.qf_vertex_clustering_emit(_C.ptr(v), n_v, _C.ptr(f), n_f, s, CONTRACTIONS[contraction],
                                               _C.ptr(ws), ws_bytes, _C.ptr(out_v), n_cells, _C.ptr(out_f), n_out,
                                               _C.ptr(fallbacks), _C.stream()), "qf_vertex_clustering_emit")
    if return_fallbacks:
        return out_v, out_f, int(fallbacks.item())
    return out_v, out_f


def downsample_mesh(mesh: TriMesh, vx=0, device="cuda", merge_tolerance=None) -> TriMesh:
    """The reference's ``mc_utils.downsample_mesh(mesh, vx)``: with ``vx > 0`` the mesh clustered with quadric
    contraction at voxel size ``1 / vx`` (on the device), else ``mesh`` unchanged.  With a ``merge_tolerance`` the
    clustered mesh is then welded at that tolerance (``weld_vertices``): the stand-in for the
    tolerance merge the reference gets from ``trimesh.Trimesh(..., process=True)``, under this project's own rule
    (parity with trimesh is unpinned; degenerate faces stay).  ``None`` keeps the clustered mesh as it is."""
    if not vx > 0:
        return mesh
    dev = _C.resolve_device(device)
    v, f = simplify_vertex_clustering(*trimesh_tensors(mesh, dev), 1 / vx, "quadric")
    if merge_tolerance is not None:
        welded = weld_vertices_device(v, f, merge_tolerance)
        v, f = welded.vertices, welded.faces
    return TriMesh(*to_numpy(v, f))


def mark_visited_cells(positions01: torch.Tensor, mask: torch.Tensor, out_of_range: torch.Tensor = None) -> None:
    """``mask[floor(p * (M - 1))] = mask[ceil(p * (M - 1))] = True`` for every row ``p`` of ``positions01`` (device fp32
    [n,3], already normalised to [0,1]^3), in place in the device ``mask`` [M,M,M] (uint8 or bool): the loop body of the
    reference's ``grid_transmittance_synthetic`` (mc_utils.py:555-560) as one launch, no index tensors.  A row with a
    component outside [0,1] writes nothing and adds one to ``out_of_range`` (device int64 [1], optional)."""
    if not isinstance(positions01, torch.Tensor) or not isinstance(mask, torch.Tensor):
        raise TypeError("positions01 and mask must be torch.Tensors")
    if not positions01.is_cuda or not mask.is_cuda:
        raise ValueError("mark_visited_cells needs device tensors (quadraturefields_amd has no CPU fallback)")
    if mask.ndim != 3 or not (mask.shape[0] == mask.shape[1] == mask.shape[2]) or not mask.is_contiguous():
        raise ValueError(f"mask must be a contiguous cube [M,M,M], got shape {tuple(mask.shape)}")
    if mask.dtype not in (torch.uint8, torch.bool):
        raise TypeError(f"mask must be uint8 or bool, got {mask.dtype}")
    if positions01.ndim != 2 or positions01.shape[1] != 3:
        raise ValueError(f"positions01 must be [n,3], got shape {tuple(positions01.shape)}")
    if out_of_range is not None and (out_of_range.dtype != torch.int64 or out_of_range.numel() != 1
                                     or out_of_range.device != mask.device):
        raise ValueError("out_of_range must be one int64 on the mask's device")
    p = _C.f32c(positions01)
    with torch.cuda.device(mask.device):
        _C.check(_C.lib().qf_mark_visited_cells(_C.ptr(p), p.shape[0], mask.shape[0], _C.ptr(mask.view(torch.uint8)),
                                                _C.ptr(out_of_range), _C.stream()), "qf_mark_visited_cells")


@torch.no_grad()
def transmittance_mask(radiance_field, estimator, views, *, max_samples=1024, chunk_size=256, size=1024, **render_kwargs):
    """The reference's ``grid_transmittance_synthetic`` (mc_utils.py:462-570) on the device: the cells that light reaches.
    Every view is rendered by ``utils.render_image_with_occgrid_test`` (early ray termination, ``max_samples`` per ray),
    the cells of a ``chunk_size``^3 grid that hold a marched position -- ``radiance_field.normalize(positions)``, floor
    and ceil -- are marked, and the grid is upsampled trilinearly (``align_corners=False``) to ``size``^3 and thresholded
    at 0.5.  ``views``: an iterable of ``Rays`` or of loader items (dicts with ``"rays"`` and optionally ``"color_bkgd"``,
    which is the view's background unless ``render_bkgd`` is given).  ``render_kwargs`` go to the renderer
    (``render_step_size``, ``near_plane``, ``alpha_thre``, ``early_stop_eps``, ...).  Returns the bool mask [size]^3 on
    the device; naming and saving it is the caller's business."""
    from .utils import render_image_with_occgrid_test
    device = estimator.binaries.device
    mask = torch.zeros((int(chunk_size),) * 3, dtype=torch.uint8, device=device)
    for view in views:
        kwargs = dict(render_kwargs)
        rays = view
        if isinstance(view, dict):
            rays = view["rays"]
            if "color_bkgd" in view:
                kwargs.setdefault("render_bkgd", view["color_bkgd"])
        positions = render_image_with_occgrid_test(max_samples, radiance_field, estimator, rays, **kwargs)[4]
        mark_visited_cells(radiance_field.normalize(positions)[1], mask)
    up = F.interpolate(mask[None, None].to(torch.float32), size=(int(size),) * 3, mode="trilinear", align_corners=False)
    return up[0, 0] > 0.5


# ---- mesh clean-up (include/qf_mesh_compact.h) ---------------------------------------------------

CompactedMesh = namedtuple("CompactedMesh", ["vertices", "faces", "face_map", "vertex_map", "stats"])


def _compact_count(lib, dev, v, f, keep, flags: int, min_component_faces: int):
    """Enqueue ``qf_mesh_compact_count``: ``(job, counts)``, the call's leading arguments with the workspace they point
    into (for ``_compact_emit``) and the device counts, still unread."""
    n_v, n_f = v.shape[0], f.shape[0]
    ws, ws_bytes = workspace("qf_mesh_compact_workspace_bytes", dev, V=n_v, F=n_f)
    counts = counts_buffer(_C.MESH_COMPACT_COUNTS, dev)
    args = (_C.ptr(v), n_v, _C.ptr(f), n_f, _C.ptr(keep), flags, min_component_faces, _C.ptr(ws), ws_bytes)
    _C.check(lib.qf_mesh_compact_count(*args, _C.ptr(counts), _C.stream()), "qf_mesh_compact_count")
    return (args, ws), counts


def _compact_emit(lib, dev, job, n_vertices: int, n_faces: int):
    """``(vertices, faces, face_map, vertex_map)`` of the counted job, whose counts gave the two sizes."""
    out_v = torch.empty((n_vertices, 3), dtype=torch.float64, device=dev)
    out_f = torch.empty((n_faces, 3), dtype=torch.int64, device=dev)
    face_map = torch.empty((n_faces,), dtype=torch.int64, device=dev)
    vertex_map = torch.empty((n_vertices,), dtype=torch.int64, device=dev)
    _C.check(lib.qf_mesh_compact_emit(*job[0], _C.ptr(out_v), n_vertices, _C.ptr(out_f), n_faces, _C.ptr(face_map),
                                      _C.ptr(vertex_map), _C.stream()), "qf_mesh_compact_emit")
    return out_v, out_f, face_map, vertex_map


def compact_mesh_device(vertices: torch.Tensor, faces: torch.Tensor, keep=None, *, remove_degenerate: bool = False,
                        remove_duplicates: bool = False, min_component_faces: int = 0,
                        remove_unreferenced: bool = True) -> CompactedMesh:
    """Clean a mesh on the device under the rules of DESIGN.md section 3.9b, in this order: faces with ``keep[f] == 0``
    dropped; faces with two equal indices dropped (``remove_degenerate``); faces whose sorted index triple an earlier
    surviving face has dropped (``remove_duplicates``); faces of vertex-connected components with fewer than
    ``min_component_faces`` faces dropped (when >= 2); vertices no surviving face uses removed and the faces remapped
    (``remove_unreferenced``).  ``vertices``: device float [V,3] (fp32 is widened exactly), ``faces``: device int64 or
    int32 [F,3], ``keep``: bool / integer [F] or None.  Returns ``CompactedMesh(vertices fp64 [V',3], faces int64
    [F',3], face_map int64 [F'], vertex_map int64 [V'], stats)``: the maps name the source face / vertex of every output
    row, ``stats`` is a dict of the eight counts (``_C.MESH_COMPACT_COUNTS``).  One host wait, for the counts.  Raises
    ValueError for host tensors, bad shapes and, with their number, faces that index outside [0, V)."""
    m = int(min_component_faces)
    if m != min_component_faces or m < 0 or m >= 2 ** 31:
        raise ValueError(f"min_component_faces must be an integer in [0, 2^31), got {min_component_faces}")
    v, f, dev, n_v, n_f = mesh_inputs(vertices, faces, "compact_mesh_device", limit="F")
    k = mask_u8(keep, n_f, dev, "keep flags")
    flags = ((_C.MESH_REMOVE_DEGENERATE if remove_degenerate else 0) | (_C.MESH_REMOVE_DUPLICATES if remove_duplicates else 0)
             | (_C.MESH_REMOVE_UNREFERENCED if remove_unreferenced else 0))
    if n_v == 0:
        if n_f:
            raise_invalid_faces(n_f, 0)
        empty = torch.empty((0,), dtype=torch.int64, device=dev)
        return CompactedMesh(v.clone(), empty.reshape(0, 3), empty, empty.clone(), zero_counts(_C.MESH_COMPACT_COUNTS))
    lib = _C.lib()
    with torch.cuda.device(dev):
        job, counts = _compact_count(lib, dev, v, f, k, flags, m)
        stats = read_counts(_C.MESH_COMPACT_COUNTS, counts)
        if stats["invalid_faces"]:
            raise_invalid_faces(stats["invalid_faces"], n_v)
        return CompactedMesh(*_compact_emit(lib, dev, job, stats["vertices"], stats["faces"]), stats)


def compact_mesh(mesh: TriMesh, keep=None, device="cuda", return_stats: bool = False, **options):
    """``compact_mesh_device`` on a ``TriMesh``: ``(TriMesh, face_map, vertex_map)`` with numpy int64 maps (and the
    stats dict fourth with ``return_stats``).  Per-vertex ``visual.uv`` is carried through ``vertex_map``.  ``keep`` may
    be a device tensor: it then makes no round trip."""
    dev = keep.device if isinstance(keep, torch.Tensor) and keep.is_cuda else _C.resolve_device(device)
    out = compact_mesh_device(*trimesh_tensors(mesh, dev), keep, **options)
    vertices, faces, face_map, vertex_map = to_numpy(*out[:4])
    uv = None if mesh.visual.uv is None else np.asarray(mesh.visual.uv)[vertex_map]
    res = (TriMesh(vertices, faces, uv), face_map, vertex_map)
    return res + (out.stats,) if return_stats else res


def mark_hit_faces(hit_tri: torch.Tensor, hit_count, mask: torch.Tensor, out_of_range: torch.Tensor = None) -> None:
    """``mask[id] = 1`` for the triangle ids of an intersector's lists (``qf_mark_hit_faces``), in place, one launch, no
    host wait: ``hit_tri`` device int32 [n_rays, max_hits] (-1 padded), ``hit_count`` device int32 [n_rays] (slots
    ``k < min(hit_count[r], max_hits)`` are considered) or None (every slot with an id >= 0 is), ``mask`` device uint8
    or bool [n_faces].  An id outside [0, n_faces) writes nothing and adds one to ``out_of_range`` (device int64 [1],
    optional).  Only ever sets bytes: views accumulate into one mask."""
    if not isinstance(hit_tri, torch.Tensor) or not isinstance(mask, torch.Tensor):
        raise TypeError("hit_tri and mask must be torch.Tensors")
    if not hit_tri.is_cuda or not mask.is_cuda:
        raise ValueError("mark_hit_faces needs device tensors (quadraturefields_amd has no CPU fallback)")
    if hit_tri.ndim != 2 or hit_tri.shape[1] < 1:
        raise ValueError(f"hit_tri must be [n_rays, max_hits >= 1], got shape {tuple(hit_tri.shape)}")
    if mask.ndim != 1 or not mask.is_contiguous() or mask.dtype not in (torch.uint8, torch.bool):
        raise ValueError(f"mask must be a contiguous uint8 or bool vector, got {mask.dtype} {tuple(mask.shape)}")
    n_rays, k = hit_tri.shape
    if hit_count is not None and (hit_count.dtype != torch.int32 or hit_count.numel() != n_rays
                                  or hit_count.device != hit_tri.device):
        raise ValueError("hit_count must be int32 [n_rays] on hit_tri's device")
    if out_of_range is not None and (out_of_range.dtype != torch.int64 or out_of_range.numel() != 1
                                     or out_of_range.device != mask.device):
        raise ValueError("out_of_range must be one int64 on the mask's device")
    with torch.cuda.device(mask.device):
        _C.check(_C.lib().qf_mark_hit_faces(_C.ptr(hit_tri.contiguous(), torch.int32),
                                            _C.ptr(hit_count.contiguous()) if hit_count is not None else None, n_rays, k,
                                            mask.shape[0], _C.ptr(mask.view(torch.uint8)), _C.ptr(out_of_range),
                                            _C.stream()), "qf_mark_hit_faces")


@torch.no_grad()
def train_visibility_mask(mesh, train_dataset, max_hits: int = 5, bvh_builder: str = "host", device="cuda"):
    """``(mesh, mask)``: the ``TriMesh`` and the device uint8 [F] mask of the faces some training ray hits among its
    first ``max_hits`` hits -- the loop of the reference's ``prunning_mesh_train_visibility`` (examples/mc_utils.py:
    309-339).  ``mesh``: a ``TriMesh`` (an intersector is built for it, ``bvh_builder`` as ``RayIntersector``'s) or a
    ``MeshIntersection`` (its intersector is used).  Per item of ``train_dataset`` (the first ``len(images)`` when it has
    ``images``) the rays ``item["rays"].origins / .viewdirs`` go through the intersector's id lists (``hits``) and
    ``qf_mark_hit_faces``; nothing waits on the host per view.  Raises IndexError when an id fell outside the mesh."""
    from .mesh_utils import MeshIntersection, RayIntersector
    if isinstance(mesh, MeshIntersection):
        ri, tri_mesh = mesh.rayintersector, mesh.mesh
    elif isinstance(mesh, TriMesh):
        ri, tri_mesh = RayIntersector(mesh, max_hits=int(max_hits), device=device, builder=bvh_builder), mesh
    else:
        raise TypeError("mesh must be a TriMesh or a MeshIntersection")
    n_faces = int(tri_mesh.faces.shape[0])
    mask = torch.zeros((n_faces,), dtype=torch.uint8, device=ri.device)
    bad = torch.zeros((1,), dtype=torch.int64, device=ri.device)
    n_views = len(train_dataset.images) if hasattr(train_dataset, "images") else None
    for j, data in enumerate(train_dataset):
        if n_views is not None and j == n_views:
            break
        rays = data["rays"]
        hit_tri, _, hit_count, _, _ = ri.hits(rays.origins.reshape(-1, 3), rays.viewdirs.reshape(-1, 3), int(max_hits))
        mark_hit_faces(hit_tri, hit_count, mask, bad)
    n_bad = int(bad.item())
    if n_bad:
        raise IndexError(f"{n_bad} hit(s) carried a triangle id outside [0, {n_faces})")
    return tri_mesh, mask


def prunning_mesh_train_visibility(mesh, train_dataset, max_hits=5, bvh_builder="host", device="cuda"):
    """The reference's ``prunning_mesh_train_visibility`` (examples/mc_utils.py:309-345) on the device: ``(mesh, mask)``,
    the mesh without the faces no training ray hits among its first ``max_hits`` hits, duplicate faces and unreferenced
    vertices removed (``compact_mesh``), and the numpy bool [F] visibility mask over the input's faces."""
    tri_mesh, mask = train_visibility_mask(mesh, train_dataset, max_hits, bvh_builder, device)
    cleaned = compact_mesh(tri_mesh, mask, remove_duplicates=True, remove_unreferenced=True)[0]
    return cleaned, mask.cpu().numpy().astype(bool)


def prunning_mesh_train_visibility_complement(mesh, train_dataset, max_hits=5, bvh_builder="host", device="cuda"):
    """The reference's ``prunning_mesh_train_visibility_complement`` (examples/mc_utils.py:272-306): ``(mesh, mesh_c,
    mask)``, the visible and the invisible half of the faces, both with every vertex kept and nothing else cleaned, as
    the reference's ``update_faces`` leaves them."""
    tri_mesh, mask = train_visibility_mask(mesh, train_dataset, max_hits, bvh_builder, device)
    m = mask.cpu().numpy().astype(bool)
    uv = tri_mesh.visual.uv
    return (TriMesh(tri_mesh.vertices.copy(), tri_mesh.faces[m], uv), TriMesh(tri_mesh.vertices.copy(), tri_mesh.faces[~m], uv),
            m)


# ---- mesh refinement (include/qf_mesh_subdivide.h) -----------------------------------------------

MeshEdges = namedtuple("MeshEdges", ["edges", "face_edges", "stats"])
SubdividedMesh = namedtuple("SubdividedMesh", ["vertices", "faces", "face_map", "vertex_parents", "stats"])


def mesh_edges_device(faces: torch.Tensor, n_vertices: int) -> MeshEdges:
    """The undirected edges of a mesh, numbered on the device in the order of their first appearance (stage A of DESIGN.md
    section 3.9c).  ``faces``: device int64 or int32 [F,3] over ``n_vertices`` vertices.  Returns ``MeshEdges(edges int64
    [E,2] as (min, max), face_edges int64 [F,3], stats)``: ``face_edges[f, k]`` is the edge between corners k and k + 1 of
    face f, -1 on a degenerate face (two equal indices), which contributes no edge; ``stats`` is a dict of the four
    counts (``_C.MESH_EDGES_COUNTS``).  One host wait, for the counts.  Raises ValueError for host tensors, bad shapes
    and, with their number, faces that index outside [0, n_vertices)."""
    _, f, dev, n_v, n_f = mesh_inputs(None, faces, "mesh_edges_device", limit="3F", n_vertices=n_vertices)
    if n_v == 0:
        if n_f:
            raise_invalid_faces(n_f, 0)
        return MeshEdges(torch.empty((0, 2), dtype=torch.int64, device=dev), torch.empty((0, 3), dtype=torch.int64, device=dev),
                         zero_counts(_C.MESH_EDGES_COUNTS))
    lib = _C.lib()
    with torch.cuda.device(dev):
        ws, ws_bytes = workspace("qf_mesh_edges_workspace_bytes", dev, V=n_v, F=n_f)
        counts = counts_buffer(_C.MESH_EDGES_COUNTS, dev)
        _C.check(lib.qf_mesh_edges_count(_C.ptr(f), n_f, n_v, _C.ptr(ws), ws_bytes, _C.ptr(counts), _C.stream()),
                 "qf_mesh_edges_count")
        stats = read_counts(_C.MESH_EDGES_COUNTS, counts)
        if stats["invalid_faces"]:
            raise_invalid_faces(stats["invalid_faces"], n_v)
        edges = torch.empty((stats["edges"], 2), dtype=torch.int64, device=dev)
        face_edges = torch.empty((n_f, 3), dtype=torch.int64, device=dev)
        _C.check(lib.qf_mesh_edges_emit(_C.ptr(f), n_f, n_v, _C.ptr(ws), ws_bytes, _C.ptr(edges), edges.shape[0],
                                        _C.ptr(face_edges), _C.stream()), "qf_mesh_edges_emit")
    return MeshEdges(edges, face_edges, stats)


def subdivide_mesh_device(vertices: torch.Tensor, faces: torch.Tensor, edge_mark=None, edges: torch.Tensor = None,
                          face_edges: torch.Tensor = None) -> SubdividedMesh:
    """Split the faces of a mesh at the midpoints of its marked edges, on the device, under the rules of DESIGN.md section
    3.9c: a marked edge ``e`` gets vertex ``V + (marked edges with a smaller id)`` at ``0.5 * (p[min] + p[max])`` in fp64;
    a face becomes 1, 2, 3 or 4 children by its number of marked edges, consecutive, with the parent's winding; every
    face that uses a marked edge is split at the same vertex, so the result has no T-junction whatever the marks are.
    ``vertices``: device float [V,3] (fp32 is widened exactly), ``faces``: device int64 or int32 [F,3], ``edge_mark``:
    bool / integer [E] over the edges of ``mesh_edges_device`` (None marks every edge), ``edges`` / ``face_edges``: that
    function's result when the caller already has it (both or neither).  Returns ``SubdividedMesh(vertices fp64 [V',3],
    faces int64 [F',3], face_map int64 [F'], vertex_parents int64 [V',2], stats)``: ``face_map`` names every child's
    parent, ``vertex_parents`` is (min, max) of the split edge for a new vertex and (v, v) for an old one, and the first
    V rows of the vertices are the input's, bit for bit; ``stats`` is a dict of the seven counts
    (``_C.MESH_SUBDIVIDE_COUNTS``).  One host wait per stage, for the counts."""
    v, f, dev, n_v, n_f = mesh_inputs(vertices, faces, "subdivide_mesh_device", limit="subdivide")
    if (edges is None) != (face_edges is None):
        raise ValueError("pass both edges and face_edges (mesh_edges_device's) or neither")
    if edges is None:
        edges, face_edges, _ = mesh_edges_device(f, n_v)
    else:
        if edges.ndim != 2 or edges.shape[1] != 2 or tuple(face_edges.shape) != (n_f, 3):
            raise ValueError(f"edges must be [E,2] and face_edges [F,3], got {tuple(edges.shape)} and {tuple(face_edges.shape)}")
        if edges.device != dev or face_edges.device != dev or face_edges.dtype != torch.int64:
            raise ValueError("edges and face_edges must be mesh_edges_device's int64 tensors on the vertices' device")
        face_edges = face_edges.contiguous()
    n_e = edges.shape[0]
    mark = mask_u8(edge_mark, n_e, dev, "edge marks", none_is=1)
    if n_v + n_e >= 2 ** 31:
        raise ValueError(f"the mesh has {n_v} vertices and {n_e} edges; V + E must be < 2^31")
    if n_v == 0:
        empty = torch.empty((0,), dtype=torch.int64, device=dev)
        return SubdividedMesh(v, empty.reshape(0, 3), empty, empty.reshape(0, 2), zero_counts(_C.MESH_SUBDIVIDE_COUNTS))
    lib = _C.lib()
    with torch.cuda.device(dev):
        ws, ws_bytes = workspace("qf_mesh_subdivide_workspace_bytes", dev, V=n_v, F=n_f, E=n_e)
        counts = counts_buffer(_C.MESH_SUBDIVIDE_COUNTS, dev)
        args = (_C.ptr(f), n_f, n_v, _C.ptr(face_edges), n_e, _C.ptr(mark), _C.ptr(ws), ws_bytes)
        _C.check(lib.qf_mesh_subdivide_count(*args, _C.ptr(counts), _C.stream()), "qf_mesh_subdivide_count")
        stats = read_counts(_C.MESH_SUBDIVIDE_COUNTS, counts)
        if stats["invalid_faces"]:
            raise ValueError(f"{stats['invalid_faces']} faces have a vertex index outside [0, {n_v}) or an edge id outside "
                             f"[0, {n_e})")
        out_v = torch.empty((stats["vertices"], 3), dtype=torch.float64, device=dev)
        out_f = torch.empty((stats["faces"], 3), dtype=torch.int64, device=dev)
        face_map = torch.empty((stats["faces"],), dtype=torch.int64, device=dev)
        parents = torch.empty((stats["vertices"], 2), dtype=torch.int64, device=dev)
        _C.check(lib.qf_mesh_subdivide_emit(_C.ptr(v), *args, _C.ptr(out_v), out_v.shape[0], _C.ptr(out_f), out_f.shape[0],
                                            _C.ptr(face_map), _C.ptr(parents), _C.stream()), "qf_mesh_subdivide_emit")
    return SubdividedMesh(out_v, out_f, face_map, parents, stats)


def chain_vertex_parents(before: torch.Tensor, level: torch.Tensor) -> torch.Tensor:
    """``vertex_parents`` over several levels: a level's rows name vertices of its own input, whose indices the levels
    before it left as they were, so the rows each level adds are appended.  Row v then names two vertices of smaller index,
    or (v, v) for a vertex of the first input."""
    return torch.cat([before, level[before.shape[0]:]])


def subdivide_mesh(mesh: TriMesh, edge_mark=None, levels: int = 1, device="cuda"):
    """``subdivide_mesh_device`` on a ``TriMesh``, ``levels`` times: ``(TriMesh, face_map, vertex_parents)`` with numpy
    int64 maps composed over the levels -- ``face_map[child]`` is the face of the INPUT mesh the child lies in, and
    ``vertex_parents[v]`` names two vertices of smaller index (the ends of the edge v split, at the level that made it), or
    (v, v) for a vertex of the input, so every chain ends at input vertices.  ``edge_mark`` (over the edges of
    ``mesh_edges_device``, None = every edge) applies to the first level; further levels split every edge.  Per-vertex
    ``visual.uv`` is carried along by the same midpoint rule."""
    levels = int(levels)
    if levels < 1:
        raise ValueError(f"levels must be >= 1, got {levels}")
    dev = edge_mark.device if isinstance(edge_mark, torch.Tensor) and edge_mark.is_cuda else _C.resolve_device(device)
    v, f = trimesh_tensors(mesh, dev)
    uv = None if mesh.visual.uv is None else np.asarray(mesh.visual.uv, np.float64)
    face_map, parents = None, None
    for level in range(levels):
        out = subdivide_mesh_device(v, f, edge_mark if level == 0 else None)
        if uv is not None:
            added = out.vertex_parents[v.shape[0]:].cpu().numpy()
            uv = np.concatenate([uv, 0.5 * (uv[added[:, 0]] + uv[added[:, 1]])])
        v, f = out.vertices, out.faces
        face_map = out.face_map if face_map is None else face_map[out.face_map]
        parents = out.vertex_parents if parents is None else chain_vertex_parents(parents, out.vertex_parents)
    return (TriMesh(*to_numpy(v, f), uv), *to_numpy(face_map, parents))


def mark_edges_longer_than(vertices: torch.Tensor, edges: torch.Tensor, length: float) -> torch.Tensor:
    """uint8 [E]: 1 where the edge ``(a, b)`` of ``edges`` (int64 [E,2]) is longer than ``length`` in the vertices'
    precision; torch ops on the tensors' device."""
    if vertices.ndim != 2 or vertices.shape[1] != 3 or edges.ndim != 2 or edges.shape[1] != 2:
        raise ValueError(f"vertices must be [V,3] and edges [E,2], got {tuple(vertices.shape)} and {tuple(edges.shape)}")
    d = vertices[edges[:, 0]] - vertices[edges[:, 1]]
    return ((d * d).sum(dim=1) > float(length) ** 2).to(torch.uint8)


# ---- mesh decimation (include/qf_mesh_decimate.h) -----------------------------------------------

DecimatedMesh = namedtuple("DecimatedMesh", ["vertices", "faces", "face_map", "vertex_target", "stats"])
DECIMATE_STOP_TARGET, DECIMATE_STOP_NO_EDGE, DECIMATE_STOP_MAX_ROUNDS = ("target reached", "no edge taken",
                                                                          "max_rounds reached")


DECIMATE_BOUNDARY_MODES = ("lock", "collapse")


def _boundary_options(boundary, boundary_weight):
    if boundary not in DECIMATE_BOUNDARY_MODES:
        raise ValueError(f"boundary must be one of {DECIMATE_BOUNDARY_MODES}, got {boundary!r}")
    weight = float(boundary_weight)
    if not (weight >= 0.0 and math.isfinite(weight)):
        raise ValueError(f"boundary_weight must be finite and >= 0, got {boundary_weight}")
    return boundary == "collapse", weight


def decimate_mesh_device(vertices: torch.Tensor, faces: torch.Tensor, target_faces: int, *, max_cost=None,
                         vertex_lock=None, max_rounds: int = 128, return_stats: bool = False, boundary: str = "lock",
                         boundary_weight: float = 1.0) -> DecimatedMesh:
    """Bring a mesh down to ``target_faces`` faces on the device by rounds of independent quadric edge collapses, under
    the rules of DESIGN.md section 3.9d (this project's own; parity with the reference's ``fast_simplification`` is
    unpinned).  Per round: the edges are numbered, every edge whose ends are neither locked nor on a boundary or
    non-manifold edge gets the point that minimises the summed quadrics of its ends and that point's cost, candidates that
    would break the surface's topology or flip a face are dropped, an independent set of the rest is selected through
    hashed power-of-two cost buckets, the cheapest of it are collapsed up to the face budget, and the mesh is compacted.
    ``vertices``: device float [V,3] (fp32 is widened exactly), all finite; ``faces``: device int64 or int32 [F,3];
    ``max_cost``: candidates that cost more are dropped (None: no limit); ``vertex_lock``: bool / integer [V], vertices
    that neither move nor disappear.  Returns ``DecimatedMesh(vertices fp64 [V',3], faces int64 [F',3], face_map int64
    [F'], vertex_target int64 [V], stats)``: output faces keep their winding and relative order, ``face_map`` names the
    source face of each, ``vertex_target[v]`` is the output vertex that input vertex v ended in (-1 if it was dropped as
    unreferenced).  With ``return_stats`` ``stats`` is a dict: ``rounds``, the per-round lists ``faces`` (after the round),
    ``candidates``, ``legal``, ``selected``, ``taken``, and ``stop`` (one of the ``DECIMATE_STOP_*`` strings); else None.
    ``target_faces >= F`` returns copies of the input, bit for bit.  Two host waits per round, for the edge count and for
    the compaction's counts (the round's own counts come with the latter).  Raises ValueError for host tensors, bad
    shapes and, with their number, faces that index outside [0, V) and vertices that are not finite.

    ``boundary="lock"`` (the default) keeps every vertex on a boundary or non-manifold edge.  ``boundary="collapse"``
    (include/qf_mesh_decimate_open.h) lets an open mesh reach its target: every boundary edge adds a plane through itself,
    perpendicular to its face, to the quadrics of its ends with weight ``boundary_weight`` (finite, >= 0; 1.0 counts a
    boundary edge like one face), boundary edges collapse along the border, interior vertices collapse onto border
    vertices, and the budget counts the one face a boundary collapse removes.  Bow-tie and non-manifold vertices stay
    locked.  The stats then gain the per-round list ``boundary_taken``; on a closed mesh the result is ``"lock"``'s, bit
    for bit."""
    collapse_mode, weight = _boundary_options(boundary, boundary_weight)
    target, max_rounds = int(target_faces), int(max_rounds)
    if target != target_faces or target < 0 or max_rounds < 0:
        raise ValueError(f"target_faces and max_rounds must be integers >= 0, got {target_faces} and {max_rounds}")
    cost_cap = math.inf if max_cost is None else float(max_cost)
    if not cost_cap >= 0.0:
        raise ValueError(f"max_cost must be >= 0, got {max_cost}")
    v, f, dev, n_v0, n_f0 = mesh_inputs(vertices, faces, "decimate_mesh_device", limit="3F")
    lock = mask_u8(vertex_lock, n_v0, dev, "vertex locks")
    v, f = v.clone(), f.clone()
    face_map = torch.arange(n_f0, dtype=torch.int64, device=dev)
    vertex_target = torch.arange(n_v0, dtype=torch.int64, device=dev)
    stats = {"rounds": 0, "faces": [], "candidates": [], "legal": [], "selected": [], "taken": [], "stop": None}
    count_names = _C.MESH_COLLAPSE_OPEN_COUNTS if collapse_mode else _C.MESH_COLLAPSE_COUNTS
    stat_names = ("candidates", "legal", "selected", "taken")
    if collapse_mode:
        stats["boundary_taken"] = []
        stat_names += ("boundary_taken",)
    lib = _C.lib()
    flags = _C.MESH_REMOVE_DEGENERATE | _C.MESH_REMOVE_UNREFERENCED
    quadrics = None
    ws_name = "qf_mesh_decimate_open_workspace_bytes" if collapse_mode else "qf_mesh_decimate_workspace_bytes"
    with torch.cuda.device(dev):
        while True:
            n_v, n_f = v.shape[0], f.shape[0]
            if n_f <= target:
                stats["stop"] = DECIMATE_STOP_TARGET
                break
            if stats["rounds"] >= max_rounds:
                stats["stop"] = DECIMATE_STOP_MAX_ROUNDS
                break
            if n_v == 0:
                raise_invalid_faces(n_f, 0)
            if quadrics is None:
                quadrics = torch.empty((n_v, 10), dtype=torch.float64, device=dev)
                quadric_counts = counts_buffer(_C.MESH_QUADRIC_COUNTS, dev)
                ws, ws_bytes = workspace(ws_name, dev, V=n_v, F=n_f, E=0)
                _C.check(lib.qf_mesh_vertex_quadrics(_C.ptr(v), n_v, _C.ptr(f), n_f, _C.ptr(quadrics), _C.ptr(ws), ws_bytes,
                                                     _C.ptr(quadric_counts), _C.stream()), "qf_mesh_vertex_quadrics")
                edges, face_edges, _ = mesh_edges_device(f, n_v)          # raises for faces out of range
                n_bad = quadric_counts.tolist()[0]                        # the stream has drained: no further wait
                if n_bad:
                    raise ValueError(f"{n_bad} vertices are not finite")
                if collapse_mode:
                    ws, ws_bytes = workspace(ws_name, dev, V=n_v, F=n_f, E=edges.shape[0])
                    boundary_counts = counts_buffer(_C.MESH_BOUNDARY_COUNTS, dev)
                    _C.check(lib.qf_mesh_boundary_quadrics(_C.ptr(v), n_v, _C.ptr(f), n_f, _C.ptr(edges), edges.shape[0],
                                                           _C.ptr(face_edges), _C.ptr(quadrics), weight, _C.ptr(ws),
                                                           ws_bytes, _C.ptr(boundary_counts), _C.stream()),
                             "qf_mesh_boundary_quadrics")
            else:
                edges, face_edges, _ = mesh_edges_device(f, n_v)
            n_e = edges.shape[0]
            max_take = (n_f - target + 1) // 2
            ws, ws_bytes = workspace(ws_name, dev, V=n_v, F=n_f, E=n_e)
            counts = counts_buffer(count_names, dev)
            if collapse_mode:
                _C.check(lib.qf_mesh_collapse_select_open(_C.ptr(v), n_v, _C.ptr(f), n_f, _C.ptr(edges), n_e,
                                                          _C.ptr(face_edges), _C.ptr(quadrics), _C.ptr(lock), cost_cap,
                                                          stats["rounds"], n_f - target, _C.ptr(ws), ws_bytes,
                                                          _C.ptr(counts), _C.stream()), "qf_mesh_collapse_select_open")
                _C.check(lib.qf_mesh_collapse_apply_open(_C.ptr(v), n_v, _C.ptr(f), n_f, _C.ptr(edges), n_e,
                                                         _C.ptr(quadrics), n_f - target, _C.ptr(vertex_target), n_v0,
                                                         _C.ptr(ws), ws_bytes, _C.stream()), "qf_mesh_collapse_apply_open")
            else:
                _C.check(lib.qf_mesh_collapse_select(_C.ptr(v), n_v, _C.ptr(f), n_f, _C.ptr(edges), n_e, _C.ptr(face_edges),
                                                     _C.ptr(quadrics), _C.ptr(lock), cost_cap, stats["rounds"], max_take,
                                                     _C.ptr(ws), ws_bytes, _C.ptr(counts), _C.stream()),
                         "qf_mesh_collapse_select")
                _C.check(lib.qf_mesh_collapse_apply(_C.ptr(v), n_v, _C.ptr(f), n_f, _C.ptr(edges), n_e, _C.ptr(quadrics),
                                                    max_take, _C.ptr(vertex_target), n_v0, _C.ptr(ws), ws_bytes,
                                                    _C.stream()), "qf_mesh_collapse_apply")
            job, c_counts = _compact_count(lib, dev, v, f, None, flags, 0)
            both = torch.cat([c_counts, counts]).tolist()                 # the round's second host wait
            compacted = dict(zip(_C.MESH_COMPACT_COUNTS, both))
            collapse = dict(zip(count_names, both[len(_C.MESH_COMPACT_COUNTS):]))
            stats["rounds"] += 1
            for name in stat_names:
                stats[name].append(collapse[name])
            if collapse["taken"] == 0:
                stats["faces"].append(n_f)
                stats["stop"] = DECIMATE_STOP_NO_EDGE
                break
            m_v, m_f = compacted["vertices"], compacted["faces"]
            out_v, out_f, c_face_map, c_vertex_map = _compact_emit(lib, dev, job, m_v, m_f)
            out_q = torch.empty((m_v, 10), dtype=torch.float64, device=dev)
            out_lock = None if lock is None else torch.empty((m_v,), dtype=torch.uint8, device=dev)
            out_face_map = torch.empty((m_f,), dtype=torch.int64, device=dev)
            _C.check(lib.qf_mesh_collapse_gather(_C.ptr(quadrics), _C.ptr(lock), _C.ptr(face_map), n_v, n_f,
                                                 _C.ptr(c_vertex_map), m_v, _C.ptr(c_face_map), m_f, _C.ptr(out_q),
                                                 _C.ptr(out_lock), _C.ptr(out_face_map), _C.ptr(vertex_target), n_v0,
                                                 _C.ptr(ws), ws_bytes, _C.stream()), "qf_mesh_collapse_gather")
            v, f, quadrics, lock, face_map = out_v, out_f, out_q, out_lock, out_face_map
            stats["faces"].append(m_f)
    return DecimatedMesh(v, f, face_map, vertex_target, stats if return_stats else None)


def decimate_mesh(mesh: TriMesh, target_faces: int, *, max_cost=None, vertex_lock=None, max_rounds: int = 128,
                  return_stats: bool = False, device="cuda", boundary: str = "lock", boundary_weight: float = 1.0):
    """``decimate_mesh_device`` on a ``TriMesh``: ``(TriMesh, face_map, vertex_target)`` with numpy int64 maps (and the
    stats dict fourth with ``return_stats``).  An output vertex takes the per-vertex ``visual.uv`` of the input vertex
    with the lowest index among those that ended in it: the end a collapse keeps.  ``boundary`` and ``boundary_weight`` are
    ``decimate_mesh_device``'s."""
    _boundary_options(boundary, boundary_weight)
    dev = _C.resolve_device(device)
    out = decimate_mesh_device(*trimesh_tensors(mesh, dev), target_faces, max_cost=max_cost, vertex_lock=vertex_lock,
                               max_rounds=max_rounds, return_stats=True, boundary=boundary, boundary_weight=boundary_weight)
    vertices, faces, face_map, vertex_target = to_numpy(*out[:4])
    uv = None
    if mesh.visual.uv is not None:
        ends, first = np.unique(vertex_target, return_index=True)
        uv = np.zeros((out.vertices.shape[0], 2), dtype=np.asarray(mesh.visual.uv).dtype)
        uv[ends[ends >= 0]] = np.asarray(mesh.visual.uv)[first[ends >= 0]]
    res = (TriMesh(vertices, faces, uv), face_map, vertex_target)
    return res + (out.stats,) if return_stats else res


# ---- manifold repair (include/qf_mesh_manifold.h) --------------------------------------------------

ManifoldMesh = namedtuple("ManifoldMesh", ["vertices", "faces", "vertex_map", "stats"])


def make_manifold_device(vertices: torch.Tensor, faces: torch.Tensor, *, return_stats: bool = False) -> ManifoldMesh:
    """Make a mesh a manifold with boundary on the device, losslessly, under the rule of DESIGN.md section 3.9e (this
    project's own; it is not open3d's ``remove_non_manifold_edges``, which drops faces): the mesh is cut along every edge
    with three or more faces and every vertex is split into one copy per fan of faces.  No face is dropped, none moves
    and no coordinate changes: ``out.vertices[out.faces]`` equals ``vertices[faces]`` bit for bit, so every rendered frame
    is unchanged, while every edge of the result has at most two faces and every vertex one fan -- the meshes
    ``decimate_mesh_device(boundary="collapse")`` gets through.  ``vertices``: device float [V,3] (fp32 is widened
    exactly), ``faces``: device int64 or int32 [F,3].  Returns ``ManifoldMesh(vertices fp64 [V',3], faces int64 [F,3],
    vertex_map int64 [V'], stats)``: the first V rows are the input's, ``vertex_map`` names the source vertex of every
    row (``baking.remap_vertex_features(table, vertex_map)`` carries a vertex-baked table along, with repeated rows; a
    quantised table is refused there as ever).  With ``return_stats`` ``stats`` is a dict of the eight counts
    (``_C.MESH_MANIFOLD_COUNTS``), else None.  A mesh that is already manifold comes back as itself.  Duplicate faces
    put three or more faces on their edges and get cut apart from their neighbours: run ``compact_mesh_device`` with
    ``remove_duplicates`` first.  Two host waits: the edge count of ``mesh_edges_device``, then V'.  Raises ValueError for
    host tensors, bad shapes and, with their number, faces that index outside [0, V)."""
    v, f, dev, n_v, n_f = mesh_inputs(vertices, faces, "make_manifold_device", limit="3F")
    if n_v == 0:
        if n_f:
            raise_invalid_faces(n_f, 0)
        stats = zero_counts(_C.MESH_MANIFOLD_COUNTS) if return_stats else None
        return ManifoldMesh(v.clone(), f.clone(), torch.empty((0,), dtype=torch.int64, device=dev), stats)
    numbered = mesh_edges_device(f, n_v)                                  # raises for faces out of range
    face_edges, n_e = numbered.face_edges, numbered.stats["edges"]
    lib = _C.lib()
    with torch.cuda.device(dev):
        ws, ws_bytes = workspace("qf_mesh_manifold_workspace_bytes", dev, V=n_v, F=n_f, E=n_e)
        counts = counts_buffer(_C.MESH_MANIFOLD_COUNTS, dev)
        _C.check(lib.qf_mesh_manifold_count(_C.ptr(f), n_f, n_v, _C.ptr(face_edges), n_e, _C.ptr(ws), ws_bytes,
                                            _C.ptr(counts), _C.stream()), "qf_mesh_manifold_count")
        stats = read_counts(_C.MESH_MANIFOLD_COUNTS, counts)
        if stats["invalid_faces"]:
            raise_invalid_faces(stats["invalid_faces"], n_v)
        out_v = torch.empty((stats["vertices"], 3), dtype=torch.float64, device=dev)
        out_f = torch.empty((n_f, 3), dtype=torch.int64, device=dev)
        vertex_map = torch.empty((stats["vertices"],), dtype=torch.int64, device=dev)
        _C.check(lib.qf_mesh_manifold_emit(_C.ptr(v), _C.ptr(f), n_f, n_v, _C.ptr(ws), ws_bytes, _C.ptr(out_v),
                                           out_v.shape[0], _C.ptr(out_f), _C.ptr(vertex_map), _C.stream()),
                 "qf_mesh_manifold_emit")
    return ManifoldMesh(out_v, out_f, vertex_map, stats if return_stats else None)


def make_manifold(mesh: TriMesh, device="cuda", return_stats: bool = False):
    """``make_manifold_device`` on a ``TriMesh``: ``(TriMesh, vertex_map)`` with a numpy int64 map (and the stats dict
    third with ``return_stats``).  Per-vertex ``visual.uv`` is carried through ``vertex_map``."""
    dev = _C.resolve_device(device)
    out = make_manifold_device(*trimesh_tensors(mesh, dev), return_stats=True)
    vertices, faces, vertex_map = to_numpy(*out[:3])
    uv = None if mesh.visual.uv is None else np.asarray(mesh.visual.uv)[vertex_map]
    res = (TriMesh(vertices, faces, uv), vertex_map)
    return res + (out.stats,) if return_stats else res


# ---- welding vertices by position (include/qf_mesh_weld.h) -----------------------------------------

WeldedMesh = namedtuple("WeldedMesh", ["vertices", "faces", "vertex_map", "vertex_class", "stats"])


def weld_vertices_device(vertices: torch.Tensor, faces: torch.Tensor = None, tolerance: float = 0.0, *,
                         return_stats: bool = False) -> WeldedMesh:
    """Weld the vertices of a mesh by position on the device, under the rule of DESIGN.md section 3.9g (this project's
    own; parity with trimesh's ``merge_vertices`` is unpinned).  With ``tolerance == 0`` two finite vertices are one iff
    their coordinates compare equal (-0.0 equals +0.0); with ``tolerance = h > 0`` iff ``((dx*dx + dy*dy) + dz*dz) <= h*h``
    in fp64, a closed ball, and transitively: a chain of points each within ``h`` of the next is one vertex (single
    linkage).  A class keeps the row of its lowest vertex, its root, bit for bit -- no coordinate is computed, so with
    ``h > 0`` a vertex may move by up to its class's diameter.  Vertices with a non-finite coordinate merge with nothing.
    No face is dropped: faces that become degenerate stay and are counted (``compact_mesh_device(remove_degenerate=True)``
    drops them).  ``vertices``: device float [V,3] (fp32 is widened exactly), ``faces``: device int64 or int32 [F,3] or
    None.  Returns ``WeldedMesh(vertices fp64 [V',3], faces int64 [F,3], vertex_map int64 [V'], vertex_class int64 [V],
    stats)``: ``vertex_map`` names the root of every output row, ``vertex_class`` the output row of every input vertex
    (``baking.weld_vertex_features(table, vertex_class, V')`` carries a vertex-baked table along).  With ``return_stats``
    ``stats`` is a dict of the eight counts (``_C.MESH_WELD_COUNTS``), else None.  The link pass costs the square of a
    search cell's population (``stats["largest_cell"]``, cells of edge ``2 h``).  One host wait, for V'.  Raises
    ValueError for host tensors, bad shapes, a negative or non-finite tolerance and, with their number, faces that index
    outside [0, V) and vertices whose search cell is out of range (``|x| / (2 h) >= 2^51``)."""
    h = float(tolerance)
    if not (h >= 0.0 and math.isfinite(h)):
        raise ValueError(f"tolerance must be finite and >= 0, got {tolerance}")
    v, f, dev, n_v, n_f = mesh_inputs(vertices, faces, "weld_vertices_device", limit="F", faces_optional=True)
    if n_v == 0:
        if n_f:
            raise_invalid_faces(n_f, 0)
        empty = torch.empty((0,), dtype=torch.int64, device=dev)
        stats = zero_counts(_C.MESH_WELD_COUNTS) if return_stats else None
        return WeldedMesh(v.clone(), f.clone(), empty, empty.clone(), stats)
    lib = _C.lib()
    with torch.cuda.device(dev):
        ws, ws_bytes = workspace("qf_mesh_weld_workspace_bytes", dev, V=n_v, F=n_f)
        counts = counts_buffer(_C.MESH_WELD_COUNTS, dev)
        _C.check(lib.qf_mesh_weld_count(_C.ptr(v), n_v, _C.ptr(f) if n_f else None, n_f, h, _C.ptr(ws), ws_bytes,
                                        _C.ptr(counts), _C.stream()), "qf_mesh_weld_count")
        stats = read_counts(_C.MESH_WELD_COUNTS, counts)
        if stats["invalid_faces"]:
            raise_invalid_faces(stats["invalid_faces"], n_v)
        if stats["out_of_range_vertices"]:
            raise ValueError(f"{stats['out_of_range_vertices']} vertices have a search cell out of range at tolerance {h} "
                             "(a coordinate over twice the tolerance must stay below 2^51)")
        out_v = torch.empty((stats["vertices"], 3), dtype=torch.float64, device=dev)
        out_f = torch.empty((n_f, 3), dtype=torch.int64, device=dev)
        vertex_map = torch.empty((stats["vertices"],), dtype=torch.int64, device=dev)
        vertex_class = torch.empty((n_v,), dtype=torch.int64, device=dev)
        _C.check(lib.qf_mesh_weld_emit(_C.ptr(v), n_v, _C.ptr(f) if n_f else None, n_f, _C.ptr(ws), ws_bytes, _C.ptr(out_v),
                                       out_v.shape[0], _C.ptr(out_f) if n_f else None, _C.ptr(vertex_map),
                                       _C.ptr(vertex_class), _C.stream()), "qf_mesh_weld_emit")
    return WeldedMesh(out_v, out_f, vertex_map, vertex_class, stats if return_stats else None)


def weld_vertices(mesh: TriMesh, tolerance: float = 0.0, device="cuda", return_stats: bool = False, compact: bool = False):
    """``weld_vertices_device`` on a ``TriMesh``: ``(TriMesh, vertex_map, vertex_class)`` with numpy int64 maps (and the
    stats dict last with ``return_stats``).  Per-vertex ``visual.uv`` follows the root, so **welding an atlas mesh
    discards the atlas**: the per-triangle atlas gives every corner its own uv, and of the corners welded into one
    vertex only the root's survives.  With ``compact=True`` the welded mesh then goes through ``compact_mesh`` with
    degenerate and duplicate faces and unreferenced vertices removed, and the result is ``(TriMesh, face_map, vertex_map,
    vertex_class)``: ``face_map`` is that step's (the input face of every output face, since the weld moves none),
    ``vertex_map`` the input root of every output vertex, and ``vertex_class`` the output vertex of every input vertex,
    -1 for those whose class no surviving face uses."""
    dev = _C.resolve_device(device)
    out = weld_vertices_device(*trimesh_tensors(mesh, dev), tolerance, return_stats=True)
    vertices, faces, vertex_map, vertex_class = to_numpy(*out[:4])
    uv = None if mesh.visual.uv is None else np.asarray(mesh.visual.uv)[vertex_map]
    welded = TriMesh(vertices, faces, uv)
    if not compact:
        res = (welded, vertex_map, vertex_class)
        return res + (out.stats,) if return_stats else res
    cleaned, face_map, kept = compact_mesh(welded, device=dev, remove_degenerate=True, remove_duplicates=True,
                                           remove_unreferenced=True)
    rank = np.full((vertex_map.shape[0],), -1, dtype=np.int64)
    rank[kept] = np.arange(kept.shape[0], dtype=np.int64)
    res = (cleaned, face_map, vertex_map[kept], rank[vertex_class])
    return res + (out.stats,) if return_stats else res


# ---- points drawn by area from a mesh's surface (include/qf_mesh_sample.h) ------------------------

SurfaceSamples = namedtuple("SurfaceSamples", ["points", "face", "bary"])


def sample_surface_device(vertices: torch.Tensor, faces: torch.Tensor, n_samples: int, seed: int = 0,
                          face_weight: torch.Tensor = None, return_stats: bool = False):
    """``n_samples`` points drawn from the surface of a mesh on the device, uniformly by area, under the rule of DESIGN.md
    section 3.9h (this project's own).  The faces are laid end to end by measure -- area, times ``face_weight[f]`` when
    weights are given, quantised to 2^-32 of the largest face -- and sample ``i`` falls in the ``i``-th of ``n_samples``
    equal strata of that line, so the number of samples on a face is within 2 of its share, and face ids come out
    non-decreasing; inside its face a sample is uniform.  The same ``seed`` gives the same bytes, from run to run and
    whatever the launch shape.  ``vertices``: device float [V,3] (fp32 is widened exactly), ``faces``: device int64 or
    int32 [F,3], ``face_weight``: device float [F], non-negative and finite, or None; ``seed`` in [0, 2^64).  Faces below
    2^-32 of the largest measure (degenerate ones, zero weights) are never sampled.  Returns ``SurfaceSamples(points fp64
    [N,3], face int64 [N], bary fp64 [N,3])``, and with ``return_stats`` a dict of the six counts
    (``_C.MESH_SAMPLE_COUNTS``) second.  One host wait, for the counts, after both calls are enqueued.  Raises ValueError
    for host tensors, bad shapes and, naming the counts, a mesh with non-finite vertices, faces that index outside
    [0, V), bad weights, non-finite measures, or no measure at all."""
    n, seed = int(n_samples), int(seed)
    if not 0 <= n < 2 ** 31:
        raise ValueError(f"n_samples must be in [0, 2^31), got {n_samples}")
    if not 0 <= seed < 2 ** 64:
        raise ValueError(f"seed must be in [0, 2^64), got {seed}")
    v, f, dev, n_v, n_f = mesh_inputs(vertices, faces, "sample_surface_device", limit="3F")
    if n_v < 1 or n_f < 1:
        raise ValueError(f"the mesh has {n_v} vertices and {n_f} faces; it needs 1 <= V and 1 <= F")
    w = None
    if face_weight is not None:
        if not isinstance(face_weight, torch.Tensor) or not face_weight.is_floating_point():
            raise TypeError("face_weight must be a floating-point torch.Tensor")
        if face_weight.shape != (n_f,):
            raise ValueError(f"face_weight must be [{n_f}], got {tuple(face_weight.shape)}")
        if face_weight.device != dev:
            raise ValueError(f"vertices on {dev} and face_weight on {face_weight.device}")
        w = face_weight.to(torch.float64).contiguous()
    lib = _C.lib()
    with torch.cuda.device(dev):
        ws, ws_bytes = workspace("qf_mesh_sample_workspace_bytes", dev, V=n_v, F=n_f)
        counts = counts_buffer(_C.MESH_SAMPLE_COUNTS, dev)
        points = torch.empty((n, 3), dtype=torch.float64, device=dev)
        face = torch.empty((n,), dtype=torch.int64, device=dev)
        bary = torch.empty((n, 3), dtype=torch.float64, device=dev)
        _C.check(lib.qf_mesh_sample_prepare(_C.ptr(v), n_v, _C.ptr(f), n_f, None if w is None else _C.ptr(w), _C.ptr(ws),
                                            ws_bytes, _C.ptr(counts), _C.stream()), "qf_mesh_sample_prepare")
        _C.check(lib.qf_mesh_sample_emit(_C.ptr(v), n_v, _C.ptr(f), n_f, _C.ptr(ws), ws_bytes, n, seed,
                                         _C.ptr(points) if n else None, _C.ptr(face) if n else None,
                                         _C.ptr(bary) if n else None, _C.stream()), "qf_mesh_sample_emit")
        stats = read_counts(_C.MESH_SAMPLE_COUNTS, counts)              # the host wait
    if any(stats[k] for k in _C.MESH_SAMPLE_COUNTS[:4]) or stats["no_measure"]:
        raise ValueError("sample_surface_device: the mesh cannot be sampled: "
                         + ", ".join(f"{k}={stats[k]}" for k in _C.MESH_SAMPLE_COUNTS))
    out = SurfaceSamples(points, face, bary)
    return (out, stats) if return_stats else out


def sample_surface(mesh: TriMesh, n_samples: int, seed: int = 0, face_weight=None, device="cuda", return_stats: bool = False):
    """``sample_surface_device`` on a ``TriMesh``: ``SurfaceSamples`` of numpy arrays (and the stats dict second with
    ``return_stats``).  ``face_weight``: array-like [F] or None."""
    dev = _C.resolve_device(device)
    w = None if face_weight is None else torch.from_numpy(np.ascontiguousarray(face_weight, dtype=np.float64)).to(dev)
    out, stats = sample_surface_device(*trimesh_tensors(mesh, dev), n_samples, seed, face_weight=w, return_stats=True)
    res = SurfaceSamples(*to_numpy(*out))
    return (res, stats) if return_stats else res


# ---- mesh-to-mesh distance (include/qf_closest_point.h) ----------------------------------------------

MeshDistance = namedtuple("MeshDistance", ["a_to_b_mean", "a_to_b_rms", "a_to_b_max", "b_to_a_mean", "b_to_a_rms",
                                           "b_to_a_max", "symmetric_max"])


def _distance_mesh(vertices, faces, what: str):
    v, f, _, n_v, n_f = mesh_inputs(vertices, faces, "mesh_distance_device", limit="3F", label=what)
    if n_f < 1 or n_v < 1:
        raise ValueError(f"{what}: a mesh needs at least one vertex and one face")
    if int(f.min()) < 0 or int(f.max()) >= n_v:
        raise ValueError(f"{what}: faces index outside [0, {n_v})")
    return v, f


def _one_sided_distance(samples: torch.Tensor, vertices: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
    """Distance fp64 [N] from every sample to the mesh, through a tree built on the device for this one query."""
    lib, dev = _C.lib(), vertices.device
    tri = vertices.to(torch.float32)[faces].reshape(-1, 9).contiguous()
    n = samples.shape[0]
    handle = ctypes.c_void_p()
    with torch.cuda.device(dev):
        _C.check(lib.qf_bvh_create_device(_C.ptr(tri, torch.float32), tri.shape[0], _C.stream(), ctypes.byref(handle)),
                 "qf_bvh_create_device")
        try:
            out_tri = torch.empty((n,), dtype=torch.int32, device=dev)
            bary = torch.empty((n, 3), dtype=torch.float64, device=dev)
            dist2 = torch.empty((n,), dtype=torch.float64, device=dev)
            counts = torch.empty((len(_C.CLOSEST_POINT_COUNTS),), dtype=torch.int64, device=dev)
            _C.check(lib.qf_bvh_closest_points(handle, _C.ptr(samples), n, math.inf, _C.ptr(out_tri), _C.ptr(bary),
                                               _C.ptr(dist2), _C.ptr(counts), _C.stream()), "qf_bvh_closest_points")
            nonfinite, missed = counts.tolist()          # the host wait: the tree is no longer in use when it is destroyed
        finally:
            lib.qf_bvh_destroy(handle)
    if nonfinite or missed:
        raise ValueError(f"mesh_distance_device: {nonfinite} samples are not finite and {missed} found no triangle")
    return dist2.sqrt()


def mesh_distance_device(vertices_a: torch.Tensor, faces_a: torch.Tensor, vertices_b: torch.Tensor,
                         faces_b: torch.Tensor, samples: int = None, seed: int = 0) -> MeshDistance:
    """The distance between two meshes, measured: each mesh is sampled at its vertices and its face centroids (fp64), and
    every sample is taken to its closest point on the OTHER mesh (``qf_bvh_closest_points``, DESIGN.md section 3.9f, over
    a tree built on the device from that mesh's vertices rounded to fp32).  Returns ``MeshDistance``: mean, root mean
    square and maximum of the one-sided distances a -> b and b -> a, and ``symmetric_max``, the larger maximum (a sampled
    Hausdorff distance: a lower bound of the true one).  Device tensors: vertices float [V,3], faces int64 or int32
    [F,3], at least one face each; raises ValueError for host tensors, bad shapes, faces out of range and vertices that
    are not finite.  Two device BVH builds and two queries; one host wait each.

    The default samples follow the tessellation, so its mean and RMS are averages over vertices and centroids, not over
    the surface: they move when a mesh is re-tessellated without moving.  With ``samples=N`` each mesh is sampled instead
    at ``N`` points drawn uniformly by area (``sample_surface_device`` with ``seed``): mean and
    RMS then estimate the surface integrals, whatever the tessellation, and the maximum is taken over those points.  The
    Hausdorff figure is still a lower bound of the true one: a finite sample can miss the farthest point (and unlike
    the default it need not contain the vertices).  ``samples=None`` is bit for bit the function without the argument."""
    va, fa = _distance_mesh(vertices_a, faces_a, "mesh a")
    vb, fb = _distance_mesh(vertices_b, faces_b, "mesh b")
    if va.device != vb.device:
        raise ValueError(f"mesh a on {va.device} and mesh b on {vb.device}")
    if samples is not None and int(samples) < 1:
        raise ValueError(f"samples must be None or at least 1, got {samples}")
    stats = []
    for (v, f), (ov, of) in (((va, fa), (vb, fb)), ((vb, fb), (va, fa))):
        if samples is None:
            corners = v[f]
            centroids = ((corners[:, 0] + corners[:, 1]) + corners[:, 2]) / 3.0
            queries = torch.cat([v, centroids]).contiguous()
        else:
            queries = sample_surface_device(v, f, int(samples), seed).points
        d = _one_sided_distance(queries, ov, of)
        stats += [float(d.mean()), float((d * d).mean().sqrt()), float(d.max())]
    return MeshDistance(*stats, max(stats[2], stats[5]))


def mesh_distance(mesh_a: TriMesh, mesh_b: TriMesh, device="cuda", samples: int = None, seed: int = 0) -> MeshDistance:
    """``mesh_distance_device`` on two ``TriMesh``."""
    dev = _C.resolve_device(device)
    return mesh_distance_device(*trimesh_tensors(mesh_a, dev), *trimesh_tensors(mesh_b, dev), samples=samples, seed=seed)


def down_sample_quadraic(mesh: TriMesh, agg=None, verbose: bool = False, device="cuda", boundary: str = "lock") -> TriMesh:
    """The reference's ``down_sample_quadraic`` (examples/mc_utils.py:214-219) on the device: the mesh decimated to
    ``F // 10`` faces by ``decimate_mesh``.  The reference calls ``fast_simplification.simplify``; this is the project's
    own rule and parity with it is unpinned.  ``agg``, fast_simplification's aggressiveness, has
    no counterpart and is unused.  ``boundary="collapse"`` lets an open mesh get there (``decimate_mesh_device``)."""
    out, _, _, stats = decimate_mesh(mesh, mesh.faces.shape[0] // 10, return_stats=True, device=device, boundary=boundary)
    if verbose:
        print(f"decimated {mesh.faces.shape[0]} -> {out.faces.shape[0]} faces in {stats['rounds']} rounds ({stats['stop']})")
    return out


def clean_mesh(mesh: TriMesh, agg=None, remove_duplicate_faces: bool = False, remove_non_manifold_edges: bool = False,
               verbose: bool = False, device="cuda", boundary: str = "lock") -> TriMesh:
    """The reference's ``clean_mesh`` (examples/mc_utils.py:222-242) on the device.  ``remove_duplicate_faces`` goes
    through ``compact_mesh`` (every vertex kept, as trimesh's call leaves them); decimation to ``F // 10`` runs iff
    ``agg > 0`` (``agg=None`` skips it; the reference would raise) -- ``agg``'s value is otherwise unused, since
    fast_simplification's aggressiveness has no counterpart in DESIGN.md section 3.9d's rule, and parity with
    fast_simplification is unpinned.  ``remove_non_manifold_edges=True`` (open3d's removal) is not built and raises
    NotImplementedError, before any work: open3d's rule drops faces; ``make_manifold`` is the
    lossless repair this project has instead, a step of its own.  ``boundary`` is ``down_sample_quadraic``'s."""
    _boundary_options(boundary, 1.0)
    if remove_non_manifold_edges:
        raise NotImplementedError("remove_non_manifold_edges (open3d's removal, which drops faces) is not built: DESIGN.md "
                                  "section 3.9d; mc_utils.make_manifold cuts and splits instead and drops nothing "
                                  "(section 3.9e)")
    if remove_duplicate_faces:
        mesh = compact_mesh(mesh, device=device, remove_duplicates=True, remove_unreferenced=False)[0]
        if verbose:
            print(f"after removing duplicate faces: {mesh.faces.shape[0]} faces")
    if agg is not None and agg > 0:
        mesh = down_sample_quadraic(mesh, agg, verbose=verbose, device=device, boundary=boundary)
    return mesh
