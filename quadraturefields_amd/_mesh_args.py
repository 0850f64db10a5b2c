"""The one input contract of the mesh wrappers (``mc_utils``, ``baking``, ``uv_atlas``): what they check about a mesh
before the first ABI call, in one order and one wording, and the small steps around every call -- the workspace, the
counts, the ``TriMesh`` conversions.  Plain functions; imports nothing of the package but ``_C``.

Order of the checks: a wrapper first refuses its own scalar options, then ``mesh_inputs``
checks tensor types, shapes, dtypes, device, same device and sizes, then the wrapper checks its masks and other tensors."""
import numpy as np
import torch

from . import _C

# The size rules, which are the kernels': every stage needs V < 2^31; the ones that sort or scan the 3 F corners need
# 3 F < 2^31, subdivide (four children a face) F < 2^29, the rest F < 2^31.
LIMITS = {"F": (2 ** 31, "V and F must be < 2^31"), "3F": ((2 ** 31 + 2) // 3, "V and 3 F must be < 2^31"),
          "subdivide": (2 ** 29, "V must be < 2^31 and F < 2^29")}


def mesh_inputs(vertices, faces, what: str, *, limit: str, n_vertices=None, faces_optional: bool = False, label: str = ""):
    """``(v fp64 contiguous [V,3], f int64 contiguous [F,3], device, V, F)`` of a wrapper's mesh, or the refusal.
    ``what`` names the wrapper, ``limit`` its size rule (a key of ``LIMITS``), ``label`` goes in front of every message
    (a wrapper of two meshes).  A wrapper that takes the faces and only the number of vertices passes ``vertices=None``
    and ``n_vertices``; ``v`` is then None.  With ``faces_optional`` ``faces=None`` stands for no faces."""
    pre = f"{label}: " if label else ""
    only_faces = n_vertices is not None
    if faces is None and faces_optional and isinstance(vertices, torch.Tensor):
        faces = torch.empty((0, 3), dtype=torch.int64, device=vertices.device)
    if not isinstance(faces, torch.Tensor) or not (only_faces or isinstance(vertices, torch.Tensor)):
        raise TypeError(pre + ("faces must be a torch.Tensor" if only_faces else "vertices and faces must be torch.Tensors"))
    if not only_faces and (vertices.ndim != 2 or vertices.shape[1] != 3):
        raise ValueError(f"{pre}vertices must be [V,3], got {tuple(vertices.shape)}")
    if faces.ndim != 2 or faces.shape[1] != 3:
        raise ValueError(f"{pre}faces must be [F,3], got {tuple(faces.shape)}")
    if not only_faces and not vertices.is_floating_point():
        raise TypeError(f"{pre}vertices must be floating point, got {vertices.dtype}")
    if faces.dtype not in (torch.int64, torch.int32):
        raise TypeError(f"{pre}faces must be int64 or int32, got {faces.dtype}")
    if not faces.is_cuda or not (only_faces or vertices.is_cuda):
        raise ValueError(f"{pre}{what} needs device tensors (quadraturefields_amd has no CPU fallback)")
    if not only_faces and vertices.device != faces.device:
        raise ValueError(f"{pre}vertices on {vertices.device} and faces on {faces.device}")
    n_v, n_f = (n_vertices if only_faces else vertices.shape[0]), faces.shape[0]
    f_limit, rule = LIMITS[limit]
    if n_v != int(n_v) or not 0 <= n_v < 2 ** 31 or n_f >= f_limit:
        raise ValueError(f"{pre}the mesh has {n_v} vertices and {n_f} faces; {rule}")
    v = None if only_faces else vertices.to(torch.float64).contiguous()
    return v, faces.to(torch.int64).contiguous(), faces.device, int(n_v), n_f


def mask_u8(mask, n: int, device, noun: str, *, none_is=None):
    """A mask (tensor or array, bool or integer) as a contiguous device uint8 [n].  ``None`` stays None, or with
    ``none_is=1`` becomes all ones.  ``noun`` names the entries in the refusals ("keep flags", "edge marks")."""
    if mask is None:
        return None if none_is is None else torch.full((n,), none_is, dtype=torch.uint8, device=device)
    k = mask if isinstance(mask, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(mask))
    k = k.reshape(-1)
    if k.shape[0] != n:
        raise ValueError(f"{k.shape[0]} {noun} where {n} are needed")
    if k.is_floating_point() or k.is_complex():
        raise TypeError(f"{noun} must be a bool or integer mask, got {k.dtype}")
    k = k.to(device)
    return (k if k.dtype == torch.uint8 else (k != 0).to(torch.uint8)).contiguous()


def workspace(name: str, dev, error=RuntimeError, **sizes):
    """``(uint8 tensor, n_bytes)`` for the ABI's ``name(*sizes.values())``; a negative answer raises ``error`` with the
    sizes by their names (``V=..., F=...``)."""
    n = int(getattr(_C.lib(), name)(*sizes.values()))
    if n < 0:
        raise error(f"{name} refused " + ", ".join(f"{k}={v}" for k, v in sizes.items()))
    return torch.empty((n,), dtype=torch.uint8, device=dev), n


def counts_buffer(names, dev) -> torch.Tensor:
    return torch.empty((len(names),), dtype=torch.int64, device=dev)


def read_counts(names, counts: torch.Tensor) -> dict:
    """The counts by name: one ``.tolist()``, which is the host wait."""
    return dict(zip(names, counts.tolist()))


def zero_counts(names) -> dict:
    return dict.fromkeys(names, 0)


def raise_invalid_faces(n: int, n_v: int):
    raise ValueError(f"{n} faces have an index outside [0, {n_v})")


def trimesh_tensors(mesh, dev):
    """fp64 vertices and int64 faces of a ``TriMesh`` (or anything with ``vertices`` and ``faces``, arrays or tensors) on
    ``dev``."""
    v, f = mesh.vertices, mesh.faces
    v = v if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v, np.float64))
    f = f if isinstance(f, torch.Tensor) else torch.from_numpy(np.asarray(f, np.int64))
    return v.to(device=dev, dtype=torch.float64), f.to(device=dev, dtype=torch.int64)


def to_numpy(*tensors):
    """The tensors as numpy arrays on the host, one copy each."""
    return tuple(t.cpu().numpy() for t in tensors)
