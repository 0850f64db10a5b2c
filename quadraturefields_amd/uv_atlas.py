"""UV atlas of an extracted mesh, on the device (``csrc/uv_atlas.hip``, rules in DESIGN.md section 3.12).

The reference builds its atlas with the ScanNet ``segmentator`` binary and ``xatlas``
(``examples/generate_uv_xatlas_old.py``); neither is available here.  The baked path looks its textures up by nearest
texel, so chart seams cost nothing, and every face can have a chart of its own: a staircase of ``(k+1)(k+2)/2``
texels whose leg ``k`` follows the face's area, two staircases to a block, blocks on shelves, taller classes first.
The rule set is this project's own; parity with xatlas is unpinned.
"""
import math
from types import SimpleNamespace

import numpy as np
import torch

from . import _C
from ._mesh_args import workspace
from .mesh_io import TriMesh

MAX_TEXTURE_SIDE = 16384
MAX_LEG = 63
BISECTIONS = 40


def atlas_capacity(texture_size: int) -> int:
    """Faces a ``texture_size``^2 atlas holds at most: all of class 0, two to each 1 x 2 block, the last row and
    column left empty."""
    return 2 * ((texture_size - 1) // 2) * (texture_size - 1)


def _is_int(n) -> bool:
    return isinstance(n, (int, np.integer)) and not isinstance(n, bool)


@torch.no_grad()
def per_triangle_atlas(mesh: TriMesh, texture_size: int, texels_per_unit=None, max_leg: int = MAX_LEG, device="cuda"):
    """``(mesh_uv, info)``: ``mesh`` with its vertices unshared (vertex ``3f+i`` is input vertex ``faces[f,i]``,
    ``faces = arange(3F).reshape(-1,3)``: face f is still face f) and ``visual.uv`` [3F,2] float64 in [0,1), ``uv[:,0]``
    the row -- what ``baking.texel_positions`` and the baked renderer take.  Any UVs ``mesh`` carries are ignored.

    Face f is class ``k = min(max_leg, floor(rho * sqrt(|(b-a) x (c-a)|)))`` and owns ``(k+1)(k+2)/2`` texels.  ``rho``
    is ``texels_per_unit`` if given (ValueError if that does not fit), else the largest density a doubling and
    40 bisection steps find to fit (each probe is one small device-to-host read).

    ``info``: ``rho``, ``class_counts`` (numpy int64 [max_leg+1]), ``face_class`` (device int32 [F]), ``face_origin``
    (device int32 [F,2], top-left row and column of the face's block), ``face_half`` (device uint8 [F]), ``rows_used``,
    ``texels_used``.

    Raises ValueError for non-finite vertices, face indices outside [0, V), F = 0 or 3F >= 2^31, V = 0 or V >= 2^31,
    ``max_leg`` outside [0, 63], ``texture_size`` outside [max_leg + 3, 16384], a ``texels_per_unit`` that is not
    positive and finite, and a mesh with more faces than the atlas has room for."""
    if not _is_int(max_leg) or not 0 <= max_leg <= MAX_LEG:
        raise ValueError(f"max_leg must be an integer in [0, {MAX_LEG}], got {max_leg!r}")
    if not _is_int(texture_size) or not max_leg + 3 <= texture_size <= MAX_TEXTURE_SIDE:
        raise ValueError(f"texture_size must be an integer in [max_leg + 3, {MAX_TEXTURE_SIDE}] = "
                         f"[{max_leg + 3}, {MAX_TEXTURE_SIDE}], got {texture_size!r}")
    if texels_per_unit is not None:
        texels_per_unit = float(texels_per_unit)
        if not (math.isfinite(texels_per_unit) and texels_per_unit > 0):
            raise ValueError(f"texels_per_unit must be positive and finite, got {texels_per_unit}")
    S, N = int(texture_size), int(max_leg)
    n_v, n_f = np.size(mesh.vertices) // 3, np.size(mesh.faces) // 3        # before any copy: a refused mesh may be huge
    if n_f < 1 or 3 * n_f >= 2 ** 31:
        raise ValueError(f"the mesh has {n_f} faces; per_triangle_atlas needs 1 <= F and 3 F < 2^31")
    if n_v < 1 or n_v >= 2 ** 31:
        raise ValueError(f"the mesh has {n_v} vertices; per_triangle_atlas needs 1 <= V < 2^31")
    vertices = np.ascontiguousarray(mesh.vertices, dtype=np.float64).reshape(-1, 3)
    faces = np.ascontiguousarray(mesh.faces, dtype=np.int64).reshape(-1, 3)
    dev = _C.resolve_device(device)
    lib = _C.lib()
    with torch.cuda.device(dev):
        ws, ws_bytes = workspace("qf_uv_atlas_workspace_bytes", dev, F=n_f)
        v_d = torch.from_numpy(vertices).to(dev)
        f_d = torch.from_numpy(faces).to(dev)
        counts = torch.empty((3,), dtype=torch.int64, device=dev)
        _C.check(lib.qf_uv_atlas_measure(_C.ptr(v_d), n_v, _C.ptr(f_d), n_f, _C.ptr(ws), ws_bytes, _C.ptr(counts),
                                         _C.stream()), "qf_uv_atlas_measure")
        bad_v, bad_f, n_positive = counts.tolist()
        if bad_v or bad_f:
            raise ValueError(f"{bad_v} vertices are not finite and {bad_f} faces have an index outside [0, {n_v})")
        result = torch.empty((4,), dtype=torch.int64, device=dev)

        def probe(rho):
            """(fits, saturated, rows_used) at density rho; saturated: every face that can reach class N is there (the
            faces of positive l, and with N = 0 every face)."""
            _C.check(lib.qf_uv_atlas_probe(n_f, rho, N, S, _C.ptr(ws), ws_bytes, _C.ptr(result), _C.stream()),
                     "qf_uv_atlas_probe")
            rows_used, _, n_top, fits = result.tolist()
            return bool(fits), n_top >= n_positive, rows_used

        if texels_per_unit is not None:
            rho = texels_per_unit
            fits, _, rows_used = probe(rho)
            if not fits:
                raise ValueError(f"texels_per_unit = {rho} does not fit a {S} x {S} atlas: rows_used = {rows_used}, "
                                 f"at most {S - 1} are allowed")
        else:
            rho = _search(probe, n_f, S)
        # vertices and UVs share one buffer so that they come back with one copy
        packed = torch.empty((15 * n_f,), dtype=torch.float64, device=dev)
        out_v, out_uv = packed[:9 * n_f], packed[9 * n_f:]
        face_class = torch.empty((n_f,), dtype=torch.int32, device=dev)
        face_origin = torch.empty((n_f, 2), dtype=torch.int32, device=dev)
        face_half = torch.empty((n_f,), dtype=torch.uint8, device=dev)
        tail = torch.empty((N + 1 + 4,), dtype=torch.int64, device=dev)      # class_counts, then result
        class_counts, result = tail[:N + 1], tail[N + 1:]
        _C.check(lib.qf_uv_atlas_emit(_C.ptr(v_d), n_v, _C.ptr(f_d), n_f, rho, N, S, _C.ptr(ws), ws_bytes, _C.ptr(out_v),
                                      _C.ptr(out_uv), _C.ptr(face_class), _C.ptr(face_origin), _C.ptr(face_half),
                                      _C.ptr(class_counts), _C.ptr(result), _C.stream()), "qf_uv_atlas_emit")
        tail_h = tail.cpu().numpy()
        rows_used, texels_used, _, fits = tail_h[N + 1:].tolist()
        if not fits:
            raise RuntimeError(f"qf_uv_atlas_emit: rho = {rho} passed its probe but not the emit (rows_used = {rows_used})")
        packed_h = packed.cpu().numpy()
    mesh_uv = TriMesh(packed_h[:9 * n_f].reshape(-1, 3), np.arange(3 * n_f, dtype=np.int64).reshape(-1, 3),
                      packed_h[9 * n_f:].reshape(-1, 2))
    info = SimpleNamespace(rho=float(rho), class_counts=tail_h[:N + 1].copy(), face_class=face_class,
                           face_origin=face_origin, face_half=face_half, rows_used=int(rows_used),
                           texels_used=int(texels_used))
    return mesh_uv, info


def _search(probe, n_faces: int, S: int) -> float:
    """Rule 6 of DESIGN.md section 3.12: rho = 0 must fit; hi doubles from 1 until it does not fit or the class
    histogram is saturated (then rho = hi); 40 bisection steps; rho = lo."""
    if not probe(0.0)[0]:
        raise ValueError(f"{n_faces} faces do not fit: a {S} x {S} atlas holds at most {atlas_capacity(S)} faces")
    lo, hi = 0.0, 1.0
    while True:
        fits, saturated, _ = probe(hi)
        if not fits:
            break
        if saturated:
            return hi
        lo, hi = hi, hi * 2.0
    for _ in range(BISECTIONS):
        mid = (lo + hi) / 2.0
        if probe(mid)[0]:
            lo = mid
        else:
            hi = mid
    return lo
