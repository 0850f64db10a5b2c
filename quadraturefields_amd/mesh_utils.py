"""Ray / mesh quadrature points on the gfx950 BVH kernels.

Mirrors the live part of ``examples/mesh_utils.py`` of the reference: ``RayIntersector`` (the duck type
of the trimesh / OptiX intersectors, :75-109), ``MeshIntersection`` (:180-412: ``sampling_raytrace_numpy``,
``sampling_indexing``, ``find_deltas``) and ``MeshFinetune`` (:112-156).  The K-iteration Embree loop, the
numpy argsort / lexsort and the device->host->device round trip of ``sampling_indexing`` are replaced by
one traversal launch that emits every ray's hits already ordered front to back, plus a per-ray device
re-sort after deformation.
"""
import ctypes
import math
import os
from collections import namedtuple
from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch

from . import _C, spc_render
from .mesh_io import TriMesh, load_mesh


def _as_device_f32(x, device) -> torch.Tensor:
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return x.to(device=device, dtype=torch.float32).contiguous()


def make_camera(c2w, focal: float, width: int, height: int) -> _C.Camera:
    """Pinhole camera in the reference's convention (nerf_synthetic.py:219-226,341-358): K = [[f,0,W/2],[0,f,H/2]],
    pixel centres at +0.5, OpenGL axes.  ``c2w``: [3,4] or [4,4] (tensor / array)."""
    m = np.asarray(c2w.detach().cpu() if isinstance(c2w, torch.Tensor) else c2w, dtype=np.float32)[:3, :4]
    cam = _C.Camera()
    for i, v in enumerate(m.reshape(-1).tolist()):
        cam.c2w[i] = v
    cam.fx = cam.fy = float(focal)
    cam.cx, cam.cy = width / 2.0, height / 2.0
    cam.width, cam.height = int(width), int(height)
    return cam


def _on_device(fn):
    """Run a method with the intersector's device current: its kernels launch on that device's stream (a caller whose
    current device is another GPU would otherwise launch on the wrong one with this device's pointers)."""
    import functools

    @functools.wraps(fn)
    def wrapped(self, *args, **kwargs):
        if torch._C._cuda_getDevice() == self.device.index:      # already current: skip the context manager (~5 us a call)
            return fn(self, *args, **kwargs)
        with torch.cuda.device(self.device):
            return fn(self, *args, **kwargs)
    return wrapped


def mesh_depth_complexity(vertices, faces) -> float:
    """Mean number of surface crossings of a random line through the mesh's bounding box: 2 * area(mesh) / area(box)
    (Cauchy-Crofton).  0 for an empty or flat mesh."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces).reshape(-1, 3)
    if v.shape[0] == 0 or f.shape[0] == 0:
        return 0.0
    area = 0.5 * np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1).sum()
    e = v.max(axis=0) - v.min(axis=0)
    box = 2.0 * (e[0] * e[1] + e[1] * e[2] + e[0] * e[2])
    return float(2.0 * area / box) if box > 0 else 0.0


def trimesh_ray_offset(vertices) -> float:
    """The distance trimesh 3.23.5 re-originates a ray past each hit in ``RayMeshIntersector.intersects_id``
    (``ray_pyembree.py``: ``clip(_ray_offset_factor * self._scale, _ray_offset_floor, inf)`` with
    ``_ray_offset_factor = 1e-4``, ``_ray_offset_floor = 1e-8`` and ``_scale = 100 / mesh.scale``, ``mesh.scale`` = the
    length of the bounding-box diagonal).  Hits closer than this to the previously returned hit are skipped by the
    reference.  Restated from memory -- trimesh is not in the container: parity unpinned."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    if v.shape[0] == 0:
        return 1e-8
    diag = float(np.sqrt(((v.max(axis=0) - v.min(axis=0)) ** 2).sum()))
    if not diag > 0:
        return 1e-8
    return float(np.clip(1e-4 * (100.0 / diag), 1e-8, np.inf))


_resolve_device = _C.resolve_device

#: What ``RayIntersector.closest_points`` returns, all on the device: ``tri`` int64 [N] (-1: none), ``bary`` fp64 [N,3],
#: ``dist2`` fp64 [N] (+inf: none), ``counts`` int64 [2] in the order of ``_C.CLOSEST_POINT_COUNTS``.
ClosestPoints = namedtuple("ClosestPoints", ["tri", "bary", "dist2", "counts"])


class _PermuteRowsFn(torch.autograd.Function):
    """``x[perm]`` for a PERMUTATION ``perm``: the backward is a plain scatter (``grad_in[perm] = grad_out``).  torch's
    own indexing backward has to assume repeated indices and sorts them first (a segmented sort + merge: 20 launches,
    ~0.3 ms per finetune step for the four re-sorted sample arrays)."""

    @staticmethod
    def forward(ctx, x, perm):
        ctx.save_for_backward(perm)
        return x[perm]

    @staticmethod
    def backward(ctx, grad):
        (perm,) = ctx.saved_tensors
        out = torch.empty_like(grad)
        out[perm] = grad
        return out, None


def _permute_rows(x, perm):
    return _PermuteRowsFn.apply(x, perm) if x.requires_grad else x[perm]


class SampleSet(tuple):
    """The six sample tensors of a frame -- ``(xyzs, dirs, index_ray, ts, index_tri, origins)``, what the reference's
    loader hands to the renderers (nerf_synthetic.py:256-257); this IS that tuple -- plus, as attributes, one frame-wide
    coherent layout cut at the windows of ``generate_splits``: ``cuts`` (first sample of every window, and the total),
    ``window_rays``, ``num_rays``, ``inverse`` / ``order`` (sample <-> position, int32) and the streamed copies
    ``xyz_c`` / ``dirs_c``.  A window's samples are ``[cuts[w], cuts[w+1])`` in the ray-major arrays AND in the copies."""

    def __new__(cls, arrays, **meta):
        obj = super().__new__(cls, arrays)
        obj.__dict__.update(meta)
        return obj


class SampleWindow(tuple):
    """One window of a ``SampleSet`` (``generate_splits``): the reference's 6-tuple of the window's samples (views), plus
    ``base`` = the window's first sample and the same range of the frame's layout (``inverse`` / ``order`` hold FRAME
    positions: subtract ``base``)."""

    def __new__(cls, arrays, **meta):
        obj = super().__new__(cls, arrays)
        obj.__dict__.update(meta)
        return obj


class _InterView:
    """``RayIntersector.inter``: the native module's two methods, bound to the adapter's BVH."""

    def __init__(self, owner):
        self._owner = owner

    def find_intersections(self, rays):
        return self._owner.find_intersections(rays)

    def update_vertices(self, vertices):
        self._owner.update_intersector(vertices)


class RayIntersector:
    """Multi-hit ray/mesh intersector.  Duck-types trimesh's ``RayMeshIntersector`` and the reference's OptiX
    adapter (``intersects_id``, ``update_intersector``; mesh_utils.py:75-109).

    Ray directions: the re-origin distance is compared with the ray PARAMETER ``t``, which is a world-space distance only
    for unit directions -- what every loader of the path hands over (``viewdirs`` are normalised, nerf_synthetic.py:366;
    trimesh unitises the directions itself before it offsets).  A caller with non-unit ``vectors`` gets a threshold that
    is off by ``|d|``; normalise first.
    ``min_separation``: the reference's multi-hit rule (``qf_bvh_set_min_separation``): ``"trimesh"`` (default) =
    ``trimesh_ray_offset(mesh.vertices)``, a float = that distance, ``0`` / ``None`` = every hit counts."""

    def __init__(self, mesh: TriMesh, max_hits: int = 10, device="cuda:0", sah_depth: int = 32,
                 min_separation="trimesh", builder: str = "host"):
        if max_hits < 1 or max_hits > _C.QF_BVH_MAX_HITS:
            raise ValueError(f"max_hits must be in 1..{_C.QF_BVH_MAX_HITS}")
        if builder not in ("host", "device"):
            raise ValueError("builder: 'host' (binned SAH, the default) or 'device' (linear BVH built on the GPU)")
        self.builder = builder
        self.mesh = mesh
        self.max_hits = int(max_hits)
        self.device = _resolve_device(device)
        # "trimesh": the separation follows the mesh -- trimesh derives it from the CURRENT mesh's extent, so it is
        # recomputed whenever the vertices are updated (update_intersector)
        self._min_separation_auto = isinstance(min_separation, str)
        if min_separation is None:
            min_separation = 0.0
        elif isinstance(min_separation, str):
            if min_separation != "trimesh":
                raise ValueError("min_separation: 'trimesh', a distance, 0 or None")
            min_separation = trimesh_ray_offset(mesh.vertices)
        self.min_separation = max(float(min_separation), 0.0)
        self.last_order = None           # coherent processing order of the most recent image-shaped sample_device()
        self.last_route = None           # the ABI call that answered the most recent intersection: "bvh", "plain", "plain+cull",
                                         # "bins", "wide", "wide+cull", "slabs", "frame" or "frame+cull" (recorded, never read)
        self._raster_backoff = 0         # frames left to skip the camera-coherent intersector after an overflow
        self.repaired_frames = 0         # frames on which some pixels overflowed K and were repaired through the BVH
        self.camera_mismatch_frames = 0  # frames whose rays were not their camera's pixel grid (see camera_mismatch)
        self._warned_mismatch = False
        self._raster_streak = 0          # consecutive camera-coherent attempts that overflowed (see want_raster)
        self._raster_trying = False
        self.scratch_slot = 0            # see _frame_scratch
        self._rule_upfront = 0           # frames left that decide the re-origin rule up front (see _hits_raster_frame)
        self._rule_pending = None        # the frame whose optimistic pack has not been checked yet (rule_violated)
        self.rule_redone_frames = 0      # frames packed twice because the optimistic check failed
        self.raster_wide = 0             # > 0: the camera-coherent pass keeps this many candidates per ray (dense scenes)
        # The overflow policy's STARTING point, from the mesh alone (the first frame of a dense-shell
        # scene ran the plain pass into ~30 ms of overflow atomics and whole-image repair before the policy switched).
        # Cauchy-Crofton: a random line through a convex body K crosses a surface of area S inside it 2 S / area(dK)
        # times on average; with K = the mesh's bounding box this is the mean depth complexity of a ray that meets the
        # box (5.5 for the 12-shell Lego stand-in, 16.7 for configs[2]'s 36 shells).  At half of K or more most object
        # rays overflow K: start with the wide / depth-slab lists (``_seed_policy``).  Only the start: the per-frame
        # overflow counts keep steering afterwards, and the state survives ``update_intersector`` / a replaced ``inter``.
        self.depth_complexity = mesh_depth_complexity(mesh.vertices, mesh.faces)
        self._policy_seeded = False
        self.raster_slabs = int(os.environ.get("QF_RASTER_SLABS", self.RASTER_SLABS))      # (env: experiments)
        self._wide_scratch = {}
        self._scratch = {}               # per-ray-count frame scratch, see _frame_scratch
        self.last_layout = None          # (inverse, xyz, dirs) of the most recent image-shaped pack, in the coherent order
        self.last_frame = None           # what utils.composite_frame needs of that pack (depths in the coherent order, ...)
        self.last_image_shape = None     # (width, height) of the most recent image-shaped batch (see split_layout)
        self._deferred_policy = None     # (event, pinned block, n_rays, k) of a frame packed without a host wait
        self._fused_pending = []         # the same records of one-call frames (fused_frame_job), oldest first
        self._fused_parity = 0           # which of the scratch block's two events the last one-call frame recorded
        self._split_scratch = {}
        self._handle = ctypes.c_void_p()
        tri = np.ascontiguousarray(mesh.vertices.astype(np.float32)[mesh.faces].reshape(-1, 9))
        with torch.cuda.device(self.device):
            if builder == "device":
                self._handle = self._device_build(torch.from_numpy(tri).to(self.device))
            else:
                _C.check(_C.lib().qf_bvh_create_ex(tri.ctypes.data_as(ctypes.c_void_p), tri.shape[0], int(sah_depth),
                                                   ctypes.byref(self._handle)), "qf_bvh_create_ex")
            _C.check(_C.lib().qf_bvh_set_min_separation(self._handle, self.min_separation), "qf_bvh_set_min_separation")

    def _device_build(self, tri: torch.Tensor) -> ctypes.c_void_p:
        """A fresh handle from device triangles [F, 9] fp32 (``qf_bvh_create_device``), on the current stream."""
        handle = ctypes.c_void_p()
        _C.check(_C.lib().qf_bvh_create_device(_C.ptr(tri, torch.float32), tri.shape[0], _C.stream(), ctypes.byref(handle)),
                 "qf_bvh_create_device")
        return handle

    def _triangle_soup(self, vertices) -> torch.Tensor:
        """``vertices`` ([V,3], or the flattened [F*9] soup; tensor or array) -> device triangles [F, 9] fp32."""
        n_tri = self.mesh.faces.shape[0]
        v = vertices.detach() if isinstance(vertices, torch.Tensor) else torch.from_numpy(
            np.ascontiguousarray(np.asarray(vertices, dtype=np.float32)))
        v = v.to(device=self.device, dtype=torch.float32)
        if v.numel() == n_tri * 9 and tuple(v.shape) != tuple(self.mesh.vertices.shape):
            return v.reshape(-1, 9).contiguous()
        if getattr(self, "_faces_dev", None) is None:
            self._faces_dev = torch.from_numpy(np.ascontiguousarray(self.mesh.faces, dtype=np.int64)).to(self.device)
        return v.reshape(-1, 3)[self._faces_dev].reshape(-1, 9).contiguous()

    def _vertex_extent(self, vertices) -> np.ndarray:
        """[2,3] fp64 bounds of ``vertices``: two small reductions for a device tensor."""
        if isinstance(vertices, torch.Tensor):
            vv = vertices.detach().reshape(-1, 3)
            return torch.stack([vv.min(dim=0).values, vv.max(dim=0).values]).double().cpu().numpy()
        vv = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
        return np.stack([vv.min(axis=0), vv.max(axis=0)])

    @_on_device
    def rebuild(self, vertices) -> None:
        """New vertex positions, same faces, NEW topology: a fresh tree is built on the device
        (``qf_bvh_create_device``) and swapped in the way the ``inter`` setter does it -- the old handle is destroyed,
        the separation follows the mesh if it is ``"trimesh"``, the policy state is kept.  ``vertices``: the shapes
        ``update_intersector`` accepts, device tensor or host array.  A refit (``update_intersector``) keeps the
        topology of the build, whose boxes loosen as the mesh moves; this replaces it."""
        new = self._device_build(self._triangle_soup(vertices))
        old, self._handle = self._handle, new
        if old is not None and old.value:
            _C.lib().qf_bvh_destroy(old)
        self._apply_min_separation(trimesh_ray_offset(self._vertex_extent(vertices)) if self._min_separation_auto
                                   else self.min_separation)

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h is not None and h.value:
            try:
                _C.lib().qf_bvh_destroy(h)
            except Exception:
                pass
            self._handle = ctypes.c_void_p()

    @property
    def num_nodes(self) -> int:
        return int(_C.lib().qf_bvh_num_nodes(self._handle))

    @property
    def max_depth(self) -> int:
        return int(_C.lib().qf_bvh_max_depth(self._handle))

    @property
    def num_wide_nodes(self) -> int:
        return int(_C.lib().qf_bvh_num_wide_nodes(self._handle))

    @property
    def max_stack(self) -> int:
        return int(_C.lib().qf_bvh_max_stack(self._handle))

    @property
    def inter(self):
        """The reference's adapter keeps the native module's object in ``.inter`` and the finetune loop REPLACES it
        after a vertex update (``rayintersector.inter = intersector.Intersector(vertices[faces].flatten(), K, 0)``,
        train_finetune.py:716-718).  Reading gives a view with that object's methods; assigning an
        ``intersector.Intersector`` of the same triangle count adopts its freshly built BVH."""
        return _InterView(self)

    @inter.setter
    def inter(self, new) -> None:
        core = getattr(new, "core", None)
        if not isinstance(core, RayIntersector):
            raise TypeError("inter: expected a quadraturefields_amd.intersector.Intersector")
        if core.mesh.faces.shape[0] != self.mesh.faces.shape[0] or core.device != self.device:
            raise ValueError("inter: the new intersector must hold the same triangles on the same device")
        self._handle, core._handle = core._handle, self._handle       # ours is destroyed with ``new``
        if self._min_separation_auto:
            self._apply_min_separation(trimesh_ray_offset(core.mesh.vertices))     # follows the adopted mesh's extent
        else:
            self._apply_min_separation(self.min_separation)

    def set_min_separation(self, min_separation: float) -> None:
        """A fixed distance (or 0): from now on the separation no longer follows the mesh's extent."""
        self._min_separation_auto = False
        self._apply_min_separation(min_separation)

    def _apply_min_separation(self, min_separation: float) -> None:
        self.min_separation = max(float(min_separation or 0.0), 0.0)
        _C.check(_C.lib().qf_bvh_set_min_separation(self._handle, self.min_separation), "qf_bvh_set_min_separation")

    def update_intersector(self, vertices) -> None:
        """New vertex positions, same faces (Intersector.update_vertices; train_finetune.py:716-718).
        ``vertices``: [V,3] vertex array, or the flattened [F*9] triangle soup the OptiX module took.  A tensor on this
        intersector's device is refitted ON the device, stream-ordered (``qf_bvh_refit_device``: no D2H / host refit /
        H2D round trip in the training loop); host arrays take the host refit."""
        n_tri = self.mesh.faces.shape[0]
        if self._min_separation_auto:
            # trimesh's re-origin distance is 1e-4 * 100 / (bounding-box diagonal of the mesh it intersects): it moves
            # with the vertices.  Only the extent is needed: two small reductions for a device tensor.
            self._apply_min_separation(trimesh_ray_offset(self._vertex_extent(vertices)))
        if isinstance(vertices, torch.Tensor) and vertices.is_cuda:
            tri = self._triangle_soup(vertices)
            with torch.cuda.device(self.device):
                _C.check(_C.lib().qf_bvh_refit_device(self._handle, _C.ptr(tri), n_tri, _C.stream()), "qf_bvh_refit_device")
            return
        v = np.asarray(vertices.detach().cpu() if isinstance(vertices, torch.Tensor) else vertices, dtype=np.float32)
        if v.size == n_tri * 9 and v.shape != tuple(self.mesh.vertices.shape):
            tri = np.ascontiguousarray(v.reshape(-1, 9))
        else:
            tri = np.ascontiguousarray(v.reshape(-1, 3)[self.mesh.faces].reshape(-1, 9))
        with torch.cuda.device(self.device):
            _C.check(_C.lib().qf_bvh_refit(self._handle, tri.ctypes.data_as(ctypes.c_void_p), tri.shape[0]), "qf_bvh_refit")

    def closest_points(self, points, max_distance: float = math.inf) -> ClosestPoints:
        """The closest point of the mesh for every query point, under the rule of DESIGN.md section 3.9f
        (include/qf_closest_point.h; this project's own, restated in numpy in tests/closest_point_reference.py): the
        nearest triangle (ties to the lower face id), its barycentric coordinates there and the squared distance, fp64
        arithmetic on the fp32 vertices the tree holds NOW -- after ``update_intersector`` or ``rebuild`` the answer is for
        the new vertices.  ``points``: device float [N,3] (fp32 is widened exactly); ``max_distance`` >= 0: triangles
        farther away do not count (``inf``: no limit).  Returns ``ClosestPoints(tri int64 [N], bary fp64 [N,3], dist2 fp64
        [N], counts int64 [2])`` on the device: a query with a NaN or infinite coordinate, or with no triangle in reach,
        gets ``tri`` -1, zero ``bary`` and ``dist2`` +inf, and ``counts`` holds the number of each (``_C.CLOSEST_POINT_COUNTS``).
        One launch on the current stream, no host wait: ``counts`` stays on the device until the caller reads it.  Raises
        TypeError / ValueError for host tensors, integer dtypes, bad shapes and a ``max_distance`` that is negative or NaN."""
        if not isinstance(points, torch.Tensor):
            raise TypeError("points must be a torch.Tensor")
        if not points.is_floating_point():
            raise TypeError(f"points must be floating point, got {points.dtype}")
        if points.ndim != 2 or points.shape[1] != 3:
            raise ValueError(f"points must be [N,3], got {tuple(points.shape)}")
        if not points.is_cuda:
            raise ValueError("closest_points needs device tensors (quadraturefields_amd has no CPU fallback)")
        if points.device != self.device:
            raise ValueError(f"points on {points.device} and the intersector on {self.device}")
        reach = float(max_distance)
        if not reach >= 0.0:
            raise ValueError(f"max_distance must be >= 0, got {max_distance}")
        pts = points.detach().to(torch.float64).contiguous()
        n = pts.shape[0]
        tri = torch.empty((n,), dtype=torch.int32, device=self.device)
        bary = torch.empty((n, 3), dtype=torch.float64, device=self.device)
        dist2 = torch.empty((n,), dtype=torch.float64, device=self.device)
        counts = torch.empty((len(_C.CLOSEST_POINT_COUNTS),), dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            _C.check(_C.lib().qf_bvh_closest_points(self._handle, _C.ptr(pts), n, reach, _C.ptr(tri), _C.ptr(bary),
                                                    _C.ptr(dist2), _C.ptr(counts), _C.stream()), "qf_bvh_closest_points")
        return ClosestPoints(tri.to(torch.int64), bary, dist2, counts)

    #: After a frame on which some pixel collected more than K candidates (the camera-coherent pass is then wasted and
    #: the BVH answers) the next frames go straight to the BVH: 1 frame after an isolated overflow, doubling while the
    #: overflows keep coming (dense-shell scenes overflow on every frame), up to this many; a clean pass halves it.
    RASTER_BACKOFF_MAX = 64

    def want_raster(self, camera) -> bool:
        if camera is None:
            return False
        if self._raster_backoff > 0:
            self._raster_backoff -= 1
            return False
        if self._raster_trying:             # the previous attempt was not reported as an overflow: a clean pass
            self._raster_streak = 0
        self._raster_trying = True
        return True

    def camera_mismatch(self) -> None:
        """A frame's rays were NOT the pixel grid of the camera that came with them (the pass's device-side check,
        ``qf_raster_intersect`` ray_flag: origin, direction within 0.02 px of the own pixel, unit length).  That frame was
        answered exactly by the BVH inside its repair launch; the next frames go straight to the BVH traversal (same
        back-off as an overflowing scene: 1 frame, doubling while it keeps happening), and the caller is told once."""
        self.camera_mismatch_frames += 1
        if not self._warned_mismatch:
            import warnings
            self._warned_mismatch = True
            warnings.warn("RayIntersector: the rays passed with camera= are not that camera's pixel grid (origin, direction "
                          "within 0.02 px of the own pixel centre, unit length -- e.g. jittered directions, a stale "
                          "make_camera, another up_sample or ray order); the frame was intersected exactly through the BVH "
                          "instead of the camera-coherent pass (about 5x slower).  Pass camera=None for such rays.",
                          stacklevel=3)
        self.raster_overflowed()

    def raster_overflowed(self) -> None:
        self._raster_trying = False
        self._raster_streak += 1
        self._raster_backoff = min(self.RASTER_BACKOFF_MAX, 1 << min(self._raster_streak - 1, 30))

    #: Dense scenes: when more than 5 % of a frame's candidates are beyond K, the following frames run the
    #: camera-coherent pass with this many slots per ray (times K, at most RASTER_WIDE_MAX) and select the K nearest on
    #: the device (qf_raster_intersect_wide) instead of leaving most of the image to the BVH.
    RASTER_WIDE_FACTOR = 4
    RASTER_WIDE_MAX = 128
    #: Dense mode, round 3: instead of collecting every crossing (4K slots per ray), rasterise the triangle chunks in this
    #: many depth slabs, nearest first; a pixel stops accepting candidates once it holds K (+ 8 with the re-origin rule)
    #: + 1 when a slab's pass starts (qf_raster_intersect_slabs).  SLAB_ROOM: list slots beyond that for the crossings of
    #: the slab in which a pixel fills up.  0 slabs = the round-2 wide lists.  Measured on configs[2] (intersection stage,
    #: ms): 0 slabs 3.23 | 2: 3.09 | 3: 2.87 | 4: 2.97 | 6: 3.22 | 8: 3.46 | 12: 3.80 -- every pass pays its launch, a copy
    #: of the counts and a tail, and a chunk that straddles a slab edge is rasterised twice.
    RASTER_SLABS = 3
    SLAB_ROOM = 32

    def _alloc_hits(self, n, k):
        return (torch.empty((n, k), dtype=torch.int32, device=self.device),
                torch.empty((n, k), dtype=torch.float32, device=self.device),
                torch.empty((n,), dtype=torch.int32, device=self.device))

    @_on_device
    def _hits_bvh(self, o, d, k, image_width):
        n = o.shape[0]
        hit_tri, hit_t, hit_count = self._alloc_hits(n, k)
        self.last_route = "bvh"
        _C.check(_C.lib().qf_bvh_intersect(self._handle, _C.ptr(o), _C.ptr(d), n, k, int(image_width),
                                           _C.ptr(hit_tri), _C.ptr(hit_t), _C.ptr(hit_count), _C.stream()),
                 "qf_bvh_intersect")
        return hit_tri, hit_t, hit_count

    @_on_device
    def _hits_raster(self, o, d, k, camera, sort_lists=True):
        """Camera-coherent path; returns the lists plus the device overflow counter (unchecked).
        sort_lists=False leaves the lists in arrival order for qf_pack_samples (which sorts while packing)."""
        n = o.shape[0]
        hit_tri, hit_t, _ = self._alloc_hits(n, k)
        # counts | overflow counter | origin flag, zeroed by one fill (qf_raster_intersect's layout convention)
        counts = torch.empty((n + 2,), dtype=torch.int32, device=self.device)
        hit_count, overflow = counts[:n], counts[n:n + 1]
        self._raster_words = counts[n:]                       # (overflow counter, ray flag): ``hits`` reads both at once
        self.last_route = "plain"
        _C.check(_C.lib().qf_raster_intersect(self._handle, ctypes.byref(camera), _C.ptr(o), _C.ptr(d), n, k,
                                              _C.ptr(hit_tri), _C.ptr(hit_t), _C.ptr(hit_count), _C.ptr(overflow),
                                              1 if sort_lists else 0, 0, _C.ptr(counts[n + 1:]), _C.stream()),
                 "qf_raster_intersect")
        return hit_tri, hit_t, hit_count, overflow

    @_on_device
    def hits(self, origins, vectors, max_hits: Optional[int] = None, image_width: int = 0, camera=None):
        """Device result: (hit_tri [R,K] int32 (-1 pad), hit_t [R,K] fp32 (+inf pad), hit_count [R] int32, o, d),
        each ray's hits ascending in (t, triangle id).  ``camera`` (see ``make_camera``) selects the
        camera-coherent intersector for rays that are that camera's pixel grid; results are identical."""
        k = self.max_hits if max_hits is None else int(max_hits)
        o = _as_device_f32(origins, self.device).reshape(-1, 3)
        d = _as_device_f32(vectors, self.device).reshape(-1, 3)
        if o.shape != d.shape:
            raise ValueError("origins and vectors must have the same shape")
        if camera is not None:
            image_width = camera.width
        if self.want_raster(camera):
            hit_tri, hit_t, hit_count, overflow = self._hits_raster(o, d, k, camera)
            ovf, bad_rays = self._raster_words.tolist()
            if ovf == 0 and bad_rays == 0:
                return hit_tri, hit_t, hit_count, o, d
            if bad_rays:                        # not this camera's pixel grid (the pass wrote nothing): the BVH answers
                self.camera_mismatch()
            else:
                self.raster_overflowed()        # some ray has more than K candidates: exact K-nearest via the BVH
        hit_tri, hit_t, hit_count = self._hits_bvh(o, d, k, image_width)
        return hit_tri, hit_t, hit_count, o, d

    def find_intersections(self, rays) -> np.ndarray:
        """OptiX-module shape: rays float[R*6] (origin, direction) -> int[R*max_hits] triangle ids, -1 padded."""
        r = np.asarray(rays, dtype=np.float32).reshape(-1, 6)
        hit_tri, _, _, _, _ = self.hits(r[:, :3], r[:, 3:])
        return hit_tri.reshape(-1).cpu().numpy()

    def _frame_scratch(self, n):
        """Frame scratch reused across frames: [n+3] int64 = sample offsets | total | raster overflow counter |
        hits dropped by the tile pack's re-origin rule,
        the scan's temp storage, a pinned (device-writable) host block [total, overflow, close-pair flag or dropped hits, -] that the
        kernels write directly, and the two events that guard it (after the offsets; after the pack).
        One entry per (stream, slot), sized for the LARGEST ray count seen there: the band-sharded renderer moves its
        cuts every frame, and keying by n would allocate -- and pin -- a fresh block for every new band height; the
        pinned block and the events are never replaced, only the device buffers grow."""
        # frames in flight on different streams, or two consecutive frames of a front / back pipeline (``scratch_slot``
        # alternates: the next frame's offsets kernel must not overwrite the pinned block the host has not read yet),
        # do not share it
        key = (_C.raw_stream(), self.scratch_slot)
        s = self._scratch.get(key)
        if s is None:
            host = torch.zeros((4,), dtype=torch.int64).pin_memory()
            # the tile pack's dropped-hit counter: its own fixed word (the kernel that publishes it leaves it at zero
            # for the next frame, so it must not move with n)
            dropped = torch.zeros((1,), dtype=torch.int32, device=self.device)
            # s[6]: how many frames have used this block (``frame_samples`` refuses a frame whose counts a later frame
            # has overwritten: the pinned block, ``dropped`` and the total word are shared per (stream, slot))
            s = self._scratch[key] = [0, None, None, host, (torch.cuda.Event(), torch.cuda.Event()), dropped, 0]
        if n > s[0]:
            cap = max(n, 2 * s[0]) if s[0] else n
            nbytes = int(_C.lib().qf_frame_offsets_temp_bytes(cap))
            if nbytes < 0:
                raise _C.QFError("qf_frame_offsets_temp_bytes failed")
            # stream-ordered allocator: the previous buffers are only reused after the kernels queued on them ran
            s[1] = torch.zeros((cap + 3,), dtype=torch.int64, device=self.device)
            s[2] = torch.empty((nbytes,), dtype=torch.uint8, device=self.device)
            s[0] = cap
        s[6] += 1
        self._scratch_stamp = (s, s[6])             # the frame being set up takes this stamp (``_stamp``)
        return s[1][:n + 3], s[2], s[3], s[4], s[5]

    def _stamp(self, frame):
        """Tie ``frame`` to the scratch block it was packed through and that block's use count at the time."""
        frame._scratch, frame._seq = self._scratch_stamp
        return frame

    #: render-only frames on the plain pass bin their hits per 8x8 tile (``qf_raster_intersect_tiles``); False keeps
    #: them on the per-ray lists (the two routes give the same frame bit for bit)
    hit_bins = True

    def _hit_bins_ready(self, k, camera) -> bool:
        """Is this frame's pass the plain one (no wide lists, no culling, rule not decided up front) at a K and a triangle
        count the hit bins' records hold?"""
        self._seed_policy(k)
        return (self.hit_bins and int(self.raster_wide) <= k and k <= 32 and not getattr(camera, "cull", False)
                and int(self.mesh.faces.shape[0]) < (1 << 26) and not (self.min_separation > 0 and self._rule_upfront > 0))

    def _bin_scratch(self, camera, k):
        """(tile cursors, tile masks, bins) of a frame on the hit-bin route: one set per (stream, scratch slot), like the
        frame scratch -- two frames in flight never share bins -- grown to the largest frame seen there."""
        key = (_C.raw_stream(), self.scratch_slot)
        n_tiles = ((int(camera.width) + 7) // 8) * ((int(camera.height) + 7) // 8)
        nbytes = int(_C.lib().qf_hit_bins_bytes(int(camera.width), int(camera.height), k))
        if nbytes < 0:
            raise _C.QFError("qf_hit_bins_bytes failed")
        s = self.__dict__.setdefault("_bin_scratch_sets", {}).get(key)
        if s is None or s[0].numel() < n_tiles or s[2].numel() < nbytes // 8:
            s = self._bin_scratch_sets[key] = (torch.empty((n_tiles,), dtype=torch.int32, device=self.device),
                                               torch.empty((n_tiles,), dtype=torch.int64, device=self.device),
                                               torch.empty((nbytes // 8,), dtype=torch.int64, device=self.device))
        return s

    @_on_device
    def _hits_raster_frame(self, o, d, k, camera, bins=False):
        """Camera-coherent pass whose overflow counter lives next to the frame's sample total (one readback).
        ``bins`` (``_hit_bins_ready``): the hits go to per-tile bins; only the overflowed pixels' per-ray rows are
        written (by the repair), and ``hit_count._qf_bins`` carries the bins to the tile pack."""
        n = o.shape[0]
        hit_tri, hit_t, _ = self._alloc_hits(n, k)
        # the overflow counter rides right behind the counts (qf_raster_intersect then zeroes both with one fill); the
        # offsets scan copies it to the frame's pinned block together with the sample total (one readback)
        # (... and the origin flag behind that: qf_raster_intersect's layout convention)
        counts = torch.empty((n + 2,), dtype=torch.int32, device=self.device)
        # overflow: 2 words -- the overflow counter and the pass's ray flag (raised: the rays are not this camera's pixel
        # grid; the passes then write nothing and the repair launch below traverses every ray)
        hit_count, overflow, origin_flag = counts[:n], counts[n:], counts[n + 1:]
        self._seed_policy(k)
        wide = max(int(self.raster_wide), 0)
        # a camera that sees part of the scene (parallel.band_camera sets .cull): cull the triangles in chunks first
        cull = 1 if getattr(camera, "cull", False) else 0
        if bins:
            cursor, mask, records = self._bin_scratch(camera, k)
            self.last_route = "bins"
            _C.check(_C.lib().qf_raster_intersect_tiles(self._handle, ctypes.byref(camera), _C.ptr(o), _C.ptr(d), n, k,
                                                        _C.ptr(cursor), _C.ptr(mask), _C.ptr(records), records.numel() * 8,
                                                        _C.ptr(hit_count), _C.ptr(overflow), _C.ptr(origin_flag),
                                                        _C.stream()), "qf_raster_intersect_tiles")
            self._repair(o, d, k, int(camera.width), hit_tri, hit_t, hit_count, with_mask=False, all_flag=origin_flag)
            hit_count._qf_bins = (cursor, mask, records, origin_flag)
            return hit_tri, hit_t, hit_count, overflow
        if wide > k and self.raster_slabs >= 2:
            sel_cap = k + 8 if self.min_separation > 0 else k            # select_capacity() of the kernels
            wide_s = min(sel_cap + 1 + self.SLAB_ROOM, 4096)
            key = (n, -wide_s, _C.raw_stream())
            keys = self._wide_scratch.get(key)
            if keys is None:
                self._wide_scratch.clear()
                keys = self._wide_scratch[key] = torch.empty((wide_s, n), dtype=torch.int64, device=self.device)
            self.last_route = "slabs"
            _C.check(_C.lib().qf_raster_intersect_slabs(self._handle, ctypes.byref(camera), _C.ptr(o), _C.ptr(d), n, k, wide_s,
                                                        int(self.raster_slabs), _C.ptr(keys), _C.ptr(hit_tri), _C.ptr(hit_t),
                                                        _C.ptr(hit_count), _C.ptr(overflow), _C.ptr(origin_flag), _C.stream()),
                     "qf_raster_intersect_slabs")
        elif wide > k:
            key = (n, wide, _C.raw_stream())
            lists = self._wide_scratch.get(key)
            if lists is None:
                self._wide_scratch.clear()
                lists = self._wide_scratch[key] = (torch.empty((wide, n), dtype=torch.int32, device=self.device),
                                                   torch.empty((wide, n), dtype=torch.float32, device=self.device))
            self.last_route = "wide+cull" if cull else "wide"
            _C.check(_C.lib().qf_raster_intersect_wide(self._handle, ctypes.byref(camera), _C.ptr(o), _C.ptr(d), n, k, wide,
                                                       _C.ptr(lists[0]), _C.ptr(lists[1]), _C.ptr(hit_tri), _C.ptr(hit_t),
                                                       _C.ptr(hit_count), _C.ptr(overflow), cull, _C.ptr(origin_flag),
                                                       _C.stream()),
                     "qf_raster_intersect_wide")
        else:
            self.last_route = "plain+cull" if cull else "plain"
            _C.check(_C.lib().qf_raster_intersect(self._handle, ctypes.byref(camera), _C.ptr(o), _C.ptr(d), n, k,
                                                  _C.ptr(hit_tri), _C.ptr(hit_t), _C.ptr(hit_count), _C.ptr(overflow),
                                                  0, cull, _C.ptr(origin_flag), _C.stream()), "qf_raster_intersect")
        # pixels that collected more than K candidates: exact K nearest through the BVH, those rays only, no host
        # round trip (afterwards every count is <= K).  With the reference's re-origin rule on, the same launch decides
        # it for every other ray as a keep-mask over its sorted list (the lists are not rewritten); the mask rides on
        # the count tensor to qf_pack_samples.
        # The rule for the OTHER rays (complete lists): a render-only frame's tile pack applies it on its own sorted
        # lists (qf_pack_tiles).  The ray-major pack applies it optimistically: pack_hits packs as if it dropped
        # nothing and verifies that exactly on the sorted lists (qf_pack_samples close_flag); only after such a frame
        # did have a close pair (duplicated / near-coincident faces) the following RULE_UPFRONT_FRAMES frames decide it
        # up front, per ray, in the repair launch (keep mask; ~0.03 ms per 800x800 frame).
        upfront = self.min_separation > 0 and self._rule_upfront > 0
        if upfront:
            self._rule_upfront -= 1
        self._repair(o, d, k, int(camera.width), hit_tri, hit_t, hit_count, with_mask=upfront, all_flag=origin_flag)
        return hit_tri, hit_t, hit_count, overflow

    #: frames that decide the re-origin rule up front after one frame's optimistic pack found a close pair
    RULE_UPFRONT_FRAMES = 64

    def _repair(self, o, d, k, width, hit_tri, hit_t, hit_count, with_mask, all_flag=None):
        n = o.shape[0]
        mask = raw = None
        if with_mask:
            mask = torch.empty((n,), dtype=torch.int64, device=self.device)
            raw = torch.empty((n,), dtype=torch.int32, device=self.device)
        _C.check(_C.lib().qf_bvh_repair_overflow(self._handle, _C.ptr(o), _C.ptr(d), n, k, int(width),
                                                 _C.ptr(hit_tri), _C.ptr(hit_t), _C.ptr(hit_count), _C.ptr(mask), _C.ptr(raw),
                                                 _C.ptr(all_flag), _C.stream()), "qf_bvh_repair_overflow")
        hit_count._qf_keep = (mask, raw) if mask is not None else None

    def pack_hits(self, o, d, k, hit_tri, hit_t, hit_count, overflow, width, lean=False, layout=True,
                  defer_rule_check=False, want_tri=False, band_rows=0):
        """Per-ray hit lists -> ([xyzs, dirs, index_ray, ts, index_tri, origins] or None, coherent order or None).

        The output size is data dependent.  Instead of stalling on it, the offsets are scanned on the device, the
        (total, raster overflow) pair starts its way to pinned host memory, and the pack and ordering kernels run
        into buffers sized for the worst case (n_rays * K samples -- 60 B each, ~1 GB for an 800x800 frame, nothing
        against 288 GB) while the host waits for those 16 bytes; the results are views of the first ``total`` rows.
        ``overflow`` (from ``_hits_raster_frame``) counts candidates beyond K; those rays were already repaired on the
        device, the count only steers the intersector policy.  ``pack_hits_begin`` / ``pack_hits_end`` are the two halves, for callers
        that keep several frames in flight on different streams."""
        return self.pack_hits_end(self.pack_hits_begin(o, d, k, hit_tri, hit_t, hit_count, overflow, width, lean, layout,
                                                       want_tri, band_rows=band_rows), defer_rule_check)

    @_on_device
    def pack_hits_begin(self, o, d, k, hit_tri, hit_t, hit_count, overflow, width, lean=False, layout=True,
                        want_tri=False, publish=True, band_rows=0):
        """Enqueue scan, readback, pack and ordering on the current stream; no host wait.  ``lean`` (image-shaped
        batches only): a caller that only renders reads the streamed copies in ``last_layout`` / ``last_frame``, so the
        tile kernel (``qf_pack_tiles``) writes just those and the six ray-major arrays come back as None.
        ``want_tri`` (lean frames): also the samples' triangle ids in that order (``last_frame.tri_c``; the baked-texture
        render looks its texels up by triangle).  ``layout=False``: no processing order at all.  ``publish=False`` (lean
        frames packed by ``pack_hits_device``): the tile pack's dropped-hit count stays in device memory -- no
        publishing launch; ``frame_samples()`` copies it when asked.
        ``band_rows`` (ray-major packs of an image only): the coherent layout's tile grid restarts every ``band_rows`` rows
        (``qf_frame_offsets`` band_rows), so that the samples of each band of rows -- a window of the reference's eval loop
        -- are one contiguous run of the coherent copies, at the same positions they have ray-major; the bands' sample
        boundaries come back with the frame's 16-byte readback (``last_band_cuts``)."""
        n = o.shape[0]
        dev = self.device
        buf, temp, host, (ev, ev_flag), dropped = self._frame_scratch(n)
        cap = n * k
        image = bool(layout) and width > 0 and n % width == 0
        self.last_image_shape = (int(width), n // int(width)) if width > 0 and n % width == 0 else None
        # sample offsets (+ total) and, for an image, the tile bases of the coherent order: three small launches
        tile_base = None
        band_rows = int(band_rows) if (image and not lean and band_rows and band_rows > 0) else 0
        tile_band = band_rows if (band_rows and band_rows < n // width) else 0      # one band = the plain tile grid
        self.last_band_cuts = None
        if image:
            height = n // width
            n_tiles = ((width + 7) // 8) * ((height + 7) // 8) if not tile_band else \
                int(_C.lib().qf_banded_tile_count(int(width), height, tile_band))
            tile_base = torch.empty((n_tiles,), dtype=torch.int64, device=dev)
        # the camera-coherent pass's ray flag rides behind its overflow counter (``_hits_raster_frame``): to host[3]
        ray_flag = overflow[1:] if (overflow is not None and overflow.numel() >= 2) else None
        if bool(lean) and image:              # render-only frame: tile bases + total, no per-ray offsets
            _C.check(_C.lib().qf_tile_offsets(_C.ptr(hit_count), k, int(width), n // int(width), _C.ptr(tile_base),
                                              _C.ptr(buf[n:]), _C.ptr(overflow), _C.ptr(ray_flag),
                                              ctypes.c_void_p(host.data_ptr()), _C.ptr(dropped), _C.stream()),
                     "qf_tile_offsets")       # (zeroes ``dropped``)
        else:
            _C.check(_C.lib().qf_frame_offsets(_C.ptr(hit_count), n, k, int(width) if image else 0, n // width if image else 0,
                                               _C.ptr(buf), _C.ptr(tile_base), _C.ptr(temp), temp.numel(), _C.ptr(overflow),
                                               _C.ptr(ray_flag), ctypes.c_void_p(host.data_ptr()), tile_band, _C.stream()),
                     "qf_frame_offsets")
            if band_rows:
                # the bands' first samples = the ray offsets at the bands' first rays: a handful of int64 that ride to
                # pinned memory beside the total, so that generate_splits needs neither a search nor a host wait
                edges = self._band_edges(n, int(width), band_rows)
                cuts_host = self._band_cut_buffer(edges.shape[0])
                cuts_host.copy_(buf.index_select(0, edges), non_blocking=True)
                self.last_band_cuts = (cuts_host, band_rows * int(width))
        ev.record()                           # (total, overflow) are in pinned memory once this event has passed
        lean = bool(lean) and image
        want_layout = layout
        keep = getattr(hit_count, "_qf_keep", None) or (None, None)      # from _repair (re-origin rule decided up front)
        optimistic = keep[0] is None and self.min_separation > 0
        flag = None
        if optimistic:                        # the pack kernel verifies "nothing dropped" and raises host[2] otherwise
            host[2] = 0
            flag = ctypes.c_void_p(host.data_ptr() + 16)
        min_sep = float(self.min_separation) if optimistic else 0.0
        xyz = dirs = org = index_ray = index_tri = depth = None
        order = inverse = xyz_c = dirs_c = depth_c = layout = frame = None    # (from here on ``layout`` is the result tuple)
        if image:                             # streamed copies in the coherent order (+ what composite_frame needs)
            xyz_c = torch.empty((cap, 3), dtype=torch.float32, device=dev)
            dirs_c = torch.empty((cap, 3), dtype=torch.float32, device=dev)
            depth_c = torch.empty((cap,), dtype=torch.float32, device=dev)
            frame = SimpleNamespace(depth_c=depth_c, hit_count=hit_count, max_hits=int(k), tile_base=tile_base,
                                    width=int(width), height=n // int(width), total=0, tri_c=None,
                                    total_dev=buf[n:n + 1])      # the slot count, on the device (int64)
            self._stamp(frame)
        if lean:
            # render-only frame: the tile kernel writes the coherent copies directly; no ray-major arrays, no order,
            # no inverse map exist for it (the six sample arrays come back as None).  It also applies the re-origin
            # rule itself, on the sorted lists (unless _repair already decided it): nothing optimistic about such a
            # frame, it is never packed twice; host[2] receives the number of hits the rule dropped.
            layout = (None, xyz_c, dirs_c)
            optimistic = False
            final_count = torch.empty((n,), dtype=torch.int32, device=dev)
            frame.tri_c = torch.empty((cap,), dtype=torch.int32, device=dev) if want_tri else None
            bins = getattr(hit_count, "_qf_bins", None)
            if bins is not None:              # the hit-bin route (``_hits_raster_frame``): lists from the tiles' bins
                _C.check(_C.lib().qf_pack_tiles_bins(_C.ptr(o), _C.ptr(d), int(width), n // int(width), k, _C.ptr(hit_tri),
                                                     _C.ptr(hit_t), _C.ptr(hit_count), _C.ptr(tile_base), _C.ptr(buf[n:]),
                                                     _C.ptr(xyz_c), _C.ptr(dirs_c), _C.ptr(depth_c), _C.ptr(frame.tri_c),
                                                     float(self.min_separation), _C.ptr(final_count), _C.ptr(dropped),
                                                     ctypes.c_void_p(host.data_ptr()) if publish else None, 1,
                                                     _C.ptr(bins[0]), _C.ptr(bins[1]), _C.ptr(bins[2]), _C.ptr(bins[3]),
                                                     _C.stream()), "qf_pack_tiles_bins")
            else:
                _C.check(_C.lib().qf_pack_tiles(_C.ptr(o), _C.ptr(d), int(width), n // int(width), k, _C.ptr(hit_tri),
                                                _C.ptr(hit_t), _C.ptr(hit_count), _C.ptr(tile_base), _C.ptr(buf[n:]),
                                                _C.ptr(xyz_c), _C.ptr(dirs_c), _C.ptr(depth_c), _C.ptr(frame.tri_c),
                                                _C.ptr(keep[0]), _C.ptr(keep[1]),
                                                float(self.min_separation) if keep[0] is None else 0.0,
                                                _C.ptr(final_count), _C.ptr(dropped),
                                                ctypes.c_void_p(host.data_ptr()) if publish else None, 1, _C.stream()),
                         "qf_pack_tiles")
            frame.hit_count = final_count
            frame.dropped_dev = None if publish else dropped
            ev_flag.record()
        else:
            xyz = torch.empty((cap, 3), dtype=torch.float32, device=dev)
            dirs = torch.empty((cap, 3), dtype=torch.float32, device=dev)
            org = torch.empty((cap, 3), dtype=torch.float32, device=dev)
            index_ray = torch.empty((cap,), dtype=torch.int64, device=dev)
            index_tri = torch.empty((cap,), dtype=torch.int64, device=dev)
            depth = torch.empty((cap,), dtype=torch.float32, device=dev)
            if image:                         # the coherent order and its inverse
                order, inverse = self.coherent_layout(hit_count, buf, cap, width, tile_base, want_order=True,
                                                      band_rows=tile_band)
                layout = (inverse, xyz_c, dirs_c)
                if tile_band:                 # a banded tile grid: not the geometry qf_composite_tiles walks
                    frame.band_rows = tile_band
            _C.check(_C.lib().qf_pack_samples(_C.ptr(o), _C.ptr(d), n, k, _C.ptr(hit_tri), _C.ptr(hit_t),
                                              _C.ptr(hit_count), _C.ptr(buf), _C.ptr(xyz), _C.ptr(dirs),
                                              _C.ptr(index_ray), _C.ptr(depth), _C.ptr(index_tri), _C.ptr(org),
                                              _C.ptr(inverse), _C.ptr(xyz_c), _C.ptr(dirs_c), _C.ptr(depth_c),
                                              _C.ptr(keep[0]), _C.ptr(keep[1]), min_sep, flag, _C.stream()),
                     "qf_pack_samples")
        if optimistic:
            ev_flag.record()
        return (o, d, k, width, (lean, want_layout, band_rows), host, (ev, ev_flag if (optimistic or lean) else None),
                [xyz, dirs, index_ray, depth, index_tri, org], order, layout,
                (hit_tri, hit_t, hit_count, keep),    # the lists stay referenced until the kernels reading them ran
                frame)

    @_on_device
    def pack_hits_end(self, pending, defer_rule_check=False):
        """Wait for the 16-byte readback of ``pack_hits_begin`` and slice the results (same stream as ``begin``).
        When the re-origin rule was applied optimistically the pack kernel's verdict arrives a little later (after the
        pack): by default it is waited for here and, if some ray did have a close pair, the frame is packed again with
        the rule decided per ray -- the caller always gets exact samples.  ``defer_rule_check=True`` returns at once
        instead; the caller launches its field / compositing kernels and THEN asks ``rule_violated()`` (by which time
        the verdict is long there); on True it must discard its results and sample again."""
        o, d, k, width, lean, host, (ev, ev_flag), arrays, order, layout, _lists, frame = pending
        ev.synchronize()
        total, ovf = int(host[0]), int(host[1])
        if int(host[3]):
            self.camera_mismatch()
        self._rule_pending = None
        if ev_flag is not None and not lean[0]:
            if defer_rule_check:
                self._rule_pending = (ev_flag, host)
            else:
                ev_flag.synchronize()
                if int(host[2]) != 0:
                    return self._repack_exact(pending)
        self._overflow_policy(ovf, o.shape[0], k)
        self.last_layout = self.last_frame = None
        if total == 0:
            return None, None
        if layout is not None:      # (inverse or None, xyz, dirs) in the coherent order: see coherent_layout
            self.last_layout = tuple(None if t is None else t[:total] for t in layout)
            frame.depth_c = frame.depth_c[:total]
            if frame.tri_c is not None:
                frame.tri_c = frame.tri_c[:total]
            frame.total = total               # slots of the coherent arrays (what the field kernel streams)
            # a render-only frame's tile pack applied the re-origin rule itself: its samples are the slots minus the
            # hits that dropped (host[2], there once ev_flag has passed -- read on demand by frame_samples())
            frame.samples = None if lean[0] else total
            frame.dropped_src = (ev_flag, host) if lean[0] else None
            self.last_frame = frame
        return [None if t is None else t[:total] for t in arrays], (order[:total] if order is not None else None)

    #: ``depth_complexity / K`` from which the first frame already uses the wide / depth-slab candidate lists
    SEED_WIDE_AT = 0.5

    def _seed_policy(self, k: int) -> None:
        """Before the first camera-coherent frame: dense scenes (mean depth complexity >= half of K) start in the dense
        mode instead of learning it from a frame's overflow count (see ``depth_complexity``)."""
        if self._policy_seeded:
            return
        self._policy_seeded = True
        wide = min(self.RASTER_WIDE_FACTOR * k, self.RASTER_WIDE_MAX)
        if self.raster_wide == 0 and wide > k and self.depth_complexity >= self.SEED_WIDE_AT * k:
            self.raster_wide = wide

    def _overflow_policy(self, ovf: int, n_rays: int, k: int) -> None:
        """``ovf`` candidates beyond K in the camera-coherent pass of a frame (those rays were already repaired on the
        device, qf_bvh_repair_overflow): steer the next frames' intersector."""
        if ovf:
            self.repaired_frames += 1
            if ovf > 0.05 * n_rays:            # much of the image overflows (dense shells)
                wide = min(self.RASTER_WIDE_FACTOR * k, self.RASTER_WIDE_MAX)
                if self.raster_wide < wide and wide > k:
                    self.raster_wide = wide    # from the next frame on: wide candidate lists + K-nearest selection
                else:
                    self.raster_overflowed()   # even the wide lists overflow: the camera-coherent pass is wasted

    def _settle_deferred_policy(self) -> None:
        """A frame packed by ``pack_hits_device`` never made the host wait for its 16-byte block; the overflow count in it
        only steers policy, so it is read here, when the NEXT frame is about to be sampled (the event has long passed:
        the block is written by the second launch of the frame it belongs to)."""
        pend, self._deferred_policy = self._deferred_policy, None
        if pend is not None:
            ev, host, n_rays, k = pend
            ev.synchronize()
            if int(host[3]):
                self.camera_mismatch()
            self._overflow_policy(int(host[1]), n_rays, k)
        while self._fused_pending:
            self._settle_fused_policy(0)

    def _settle_fused_policy(self, keep: int = 1) -> None:
        """One-call frames (``fused_frame_job``) record their event after their LAST launch; waiting for the previous
        frame's would let the host enqueue a frame only once the GPU has finished the one before -- host and GPU taking
        turns.  They alternate between the scratch block's two events instead, and a frame settles the policy of the
        frame BEFORE the previous one (``keep`` = frames left pending), which has long finished.  The pinned block
        holds the overflow count of the latest frame that got that far: recent enough for a policy."""
        while len(self._fused_pending) > keep:
            ev, host, n_rays, k = self._fused_pending.pop(0)
            ev.synchronize()
            if int(host[3]):
                self.camera_mismatch()
            self._overflow_policy(int(host[1]), n_rays, k)

    def pack_hits_device(self, pending):
        """Second half of a RENDER-ONLY frame (``pack_hits_begin(..., lean=True)``) WITHOUT the host wait: the sample
        count stays on the device (``frame.total_dev``; every consumer takes it as ``n_device``), the coherent arrays
        are handed on at their worst-case capacity (``n_rays * K`` slots) and the frame is a fixed sequence of launches
        -- nothing between the rays and the pixels returns to the host.  Returns ``last_frame`` (``last_layout`` holds
        the capacity-sized position / direction arrays).  ``frame_samples()`` still answers, by waiting then."""
        o, d, k, width, lean, host, (ev, ev_flag), arrays, order, layout, _lists, frame = pending
        if not lean[0] or frame is None or layout is None:
            raise ValueError("pack_hits_device: a lean image-shaped pack is required")
        self._rule_pending = None
        self._deferred_policy = (ev, host, o.shape[0], k)
        self.last_layout = layout                       # (None, xyz_c, dirs_c) at capacity
        frame.total = int(frame.depth_c.shape[0])       # slots of the arrays = capacity; the live count is total_dev
        frame.samples = None
        frame.total_src = (ev, host)
        frame.dropped_src = (ev_flag, host)
        frame._keep = _lists                            # the hit lists stay referenced until their readers ran
        self.last_frame = frame
        return frame

    def frame_samples(self, frame=None) -> int:
        """Quadrature points of the most recent image-shaped pack (``last_frame``), or of ``frame`` (what
        ``render_async`` / ``sample_frame_device`` returned): for a render-only frame the slots of the coherent arrays
        minus the hits its re-origin rule dropped.  A frame packed WITHOUT a host wait keeps its counts in words that the
        next frame on the same stream reuses (the pinned block, the dropped-hit counter, the total): ask before that
        frame is sampled -- afterwards this raises instead of handing out another frame's count."""
        f = self.last_frame if frame is None else frame
        if f is None:
            return 0
        if f.samples is None:
            sc = getattr(f, "_scratch", None)
            if sc is not None and sc[6] != f._seq:
                raise RuntimeError("frame_samples: this render-only frame's counts have not been read yet and a later frame "
                                   "has since reused the words they live in (same stream and scratch slot); ask for a "
                                   "frame's sample count before the next frame is sampled")
            total = f.total
            src = getattr(f, "total_src", None)
            if src is not None:                 # packed without a host wait: the count is read now
                src[0].synchronize()
                total = int(src[1][0])
                f.total_src = None
            if getattr(f, "dropped_dev", None) is not None:
                # packed without the publishing launch: the counter is still the frame's until the next frame's tile
                # offsets zero it, so this must be asked before the next frame is sampled on this stream
                f.samples = total - int(f.dropped_dev.item())
                f.dropped_dev = None
            else:
                ev_flag, host = f.dropped_src
                ev_flag.synchronize()
                f.samples = total - int(host[2])
            f.dropped_src = None
        return f.samples

    def rule_violated(self) -> bool:
        """After ``pack_hits_end(..., defer_rule_check=True)``: did the optimistic pack of that frame find a ray whose
        hits the re-origin rule would thin out?  True -> the samples (and everything computed from them) are not the
        reference's; sample again (the following frames decide the rule up front, so the retry is exact)."""
        pend, self._rule_pending = self._rule_pending, None
        if pend is None:
            return False
        ev_flag, host = pend
        ev_flag.synchronize()
        if int(host[2]) == 0:
            return False
        self._rule_violation()
        return True

    def _rule_violation(self):
        """A frame's optimistic pack was refuted: decide the rule up front for the next frames -- 64 after the first
        time, doubling (up to 4096) each time the optimistic retry at the end of such a window fails again."""
        self._rule_window = min(4096, 2 * getattr(self, "_rule_window", self.RULE_UPFRONT_FRAMES // 2))
        self._rule_upfront = self._rule_window
        self.rule_redone_frames += 1

    def _repack_exact(self, pending):
        """The optimistic pack of ``pending`` failed its check: decide the rule per ray (keep masks over the same
        lists) and pack again."""
        o, d, k, width, (lean, want_layout, band_rows), _host, _evs, _arrays, _order, _layout, (hit_tri, hit_t, hit_count, _keep), _frame = pending
        self._rule_violation()
        self._repair(o, d, k, width, hit_tri, hit_t, hit_count, with_mask=True)
        return self.pack_hits_end(self.pack_hits_begin(o, d, k, hit_tri, hit_t, hit_count, None, width, lean, want_layout,
                                                       band_rows=band_rows))

    @_on_device
    def sample_device(self, origins, vectors, max_hits: Optional[int] = None, image_width: int = 0, camera=None,
                      lean: bool = False, layout: bool = True, defer_rule_check: bool = False, want_tri: bool = False,
                      band_rows: int = 0):
        """Packed, sorted samples on the device: [xyzs, dirs, index_ray, ts, index_tri, origins] -- the six
        tensors the reference's DataLoader hands to the renderers (nerf_synthetic.py:256-257) -- or None
        when no ray hits anything.  ``lean`` with a camera: a render-only frame -- six Nones; the samples are in
        ``last_layout`` / ``last_frame`` (see ``pack_hits_begin``)."""
        k = self.max_hits if max_hits is None else int(max_hits)
        o = _as_device_f32(origins, self.device).reshape(-1, 3)
        d = _as_device_f32(vectors, self.device).reshape(-1, 3)
        n = o.shape[0]
        if n == 0:
            return None
        if camera is not None:
            image_width = camera.width
        self._settle_deferred_policy()
        if self.want_raster(camera):
            hit_tri, hit_t, hit_count, overflow = self._hits_raster_frame(o, d, k, camera)
        else:
            hit_tri, hit_t, hit_count = self._hits_bvh(o, d, k, image_width)
            overflow = None
        data, self.last_order = self.pack_hits(o, d, k, hit_tri, hit_t, hit_count, overflow, int(image_width), lean,
                                               layout, defer_rule_check, want_tri, band_rows)
        return data

    @_on_device
    def sample_frame_device(self, origins, vectors, max_hits: Optional[int] = None, camera=None, want_tri: bool = False):
        """A render-only camera frame with NO host wait: intersection, tile offsets and tile pack are enqueued and the
        frame comes back at once -- ``last_frame`` (``total_dev`` = the slot count on the device) and ``last_layout`` =
        (None, xyz_c, dirs_c) at worst-case capacity.  See ``pack_hits_device``."""
        if camera is None:
            raise ValueError("sample_frame_device: the rays must be a camera's pixel grid")
        k = self.max_hits if max_hits is None else int(max_hits)
        o = _as_device_f32(origins, self.device).reshape(-1, 3)
        d = _as_device_f32(vectors, self.device).reshape(-1, 3)
        if o.shape[0] != camera.width * camera.height:
            raise ValueError("sample_frame_device: origins / vectors must be the camera's full pixel grid")
        self._settle_deferred_policy()
        if self.want_raster(camera):
            hit_tri, hit_t, hit_count, overflow = self._hits_raster_frame(o, d, k, camera,
                                                                          bins=self._hit_bins_ready(k, camera))
        else:
            hit_tri, hit_t, hit_count = self._hits_bvh(o, d, k, camera.width)
            overflow = None
        self.last_order = None
        return self.pack_hits_device(self.pack_hits_begin(o, d, k, hit_tri, hit_t, hit_count, overflow, int(camera.width),
                                                          lean=True, layout=True, want_tri=want_tri, publish=False))

    def fused_frame_ready(self, camera, max_hits: Optional[int] = None) -> bool:
        """Does ``sample_frame_device`` reduce to the fixed sequence ``qf_frame_render`` composes -- the plain
        camera-coherent pass (no wide candidate lists, no back-off to the BVH path) with the re-origin rule left to the
        tile pack?  No side effects (beyond seeding the policy from the mesh the first time anyone asks)."""
        k = self.max_hits if max_hits is None else int(max_hits)
        self._seed_policy(k)
        return (camera is not None and self._raster_backoff <= 0 and int(self.raster_wide) <= k
                and not (self.min_separation > 0 and self._rule_upfront > 0))

    @_on_device
    def fused_frame_job(self, origins, vectors, max_hits: Optional[int] = None, camera=None, want_tri: bool = False):
        """The sampling half of a ``qf_frame_job`` for a camera frame (``fused_frame_ready`` must hold): every buffer
        ``sample_frame_device`` would allocate, and the frame record it would return -- with nothing enqueued yet.
        Returns (job, frame, token) -- or None when settling an earlier frame's overflow count has just moved the policy
        away from the plain pass (take ``sample_frame_device``); the caller adds the field / image pointers, calls
        ``qf_frame_render`` and hands ``token`` to ``fused_frame_done``."""
        k = self.max_hits if max_hits is None else int(max_hits)
        o = _as_device_f32(origins, self.device).reshape(-1, 3)
        d = _as_device_f32(vectors, self.device).reshape(-1, 3)
        n = o.shape[0]
        w, h = int(camera.width), int(camera.height)
        if n != w * h:
            raise ValueError("fused_frame_job: origins / vectors must be the camera's full pixel grid")
        if self._deferred_policy is not None:
            self._settle_deferred_policy()
        self._settle_fused_policy(1)
        if not self.fused_frame_ready(camera, k) or not self.want_raster(camera):      # (the policy may just have moved)
            return None
        dev = self.device
        cap = n * k
        hit_tri, hit_t, _ = self._alloc_hits(n, k)
        counts = torch.empty((n + 2,), dtype=torch.int32, device=dev)         # counts | overflow | ray flag
        final_count = torch.empty((n,), dtype=torch.int32, device=dev)
        tile_base = torch.empty((((w + 7) // 8) * ((h + 7) // 8),), dtype=torch.int64, device=dev)
        xyz_c = torch.empty((cap, 3), dtype=torch.float32, device=dev)
        dirs_c = torch.empty((cap, 3), dtype=torch.float32, device=dev)
        depth_c = torch.empty((cap,), dtype=torch.float32, device=dev)
        tri_c = torch.empty((cap,), dtype=torch.int32, device=dev) if want_tri else None
        buf, _temp, host, events, dropped = self._frame_scratch(n)
        self._fused_parity ^= 1
        ev, ev_flag = events[self._fused_parity], events[self._fused_parity ^ 1]
        job = _C.FrameJob()
        job.camera = ctypes.addressof(camera)
        job.rays_o, job.rays_d, job.n_rays, job.max_hits = o.data_ptr(), d.data_ptr(), n, k
        job.cull_chunks = (1 if getattr(camera, "cull", False) else 0) | (0 if self.hit_bins else 2)   # QF_FRAME_PER_RAY_LISTS
        job.min_separation = float(self.min_separation)
        job.hit_tri, job.hit_t, job.hit_count = hit_tri.data_ptr(), hit_t.data_ptr(), counts.data_ptr()
        job.final_count, job.tile_base = final_count.data_ptr(), tile_base.data_ptr()
        job.total, job.host_block, job.dropped = buf.data_ptr() + 8 * n, host.data_ptr(), dropped.data_ptr()
        job.xyz_c, job.dirs_c, job.depth_c = xyz_c.data_ptr(), dirs_c.data_ptr(), depth_c.data_ptr()
        job.tri_c = tri_c.data_ptr() if want_tri else None
        frame = SimpleNamespace(depth_c=depth_c, hit_count=final_count, max_hits=k, tile_base=tile_base, width=w, height=h,
                                total=cap, tri_c=tri_c, total_dev=buf[n:n + 1], samples=None, total_src=(ev, host),
                                dropped_src=(ev_flag, host), dropped_dev=dropped,
                                _keep=(hit_tri, hit_t, counts, o, d, camera))
        self._stamp(frame)
        return job, frame, (ev, host, n, k, xyz_c, dirs_c)

    def fused_frame_done(self, frame, token) -> None:
        """After ``qf_frame_render`` was enqueued: the state ``sample_frame_device`` leaves behind."""
        ev, host, n, k, xyz_c, dirs_c = token
        ev.record()                           # (total, overflow) are in the pinned block once this event has passed
        self._rule_pending = None
        self._fused_pending.append((ev, host, n, k))
        self.last_order = None
        self.last_image_shape = (frame.width, frame.height)
        self.last_layout = (None, xyz_c, dirs_c)
        self.last_frame = frame

    @_on_device
    def _band_edges(self, n_rays: int, width: int, band_rows: int) -> torch.Tensor:
        """First ray of every band of ``band_rows`` rows, and ``n_rays``: int64 on the device, cached."""
        key = (n_rays, width, band_rows)
        cache = self.__dict__.setdefault("_band_edge_cache", {})
        e = cache.get(key)
        if e is None:
            if len(cache) > 8:
                cache.clear()
            step = band_rows * width
            e = cache[key] = torch.tensor(list(range(0, n_rays, step)) + [n_rays], dtype=torch.int64, device=self.device)
        return e

    def _band_cut_buffer(self, m: int) -> torch.Tensor:
        """Pinned int64 [m], two alternating per size (the previous frame's cuts may not have been read yet)."""
        ring = self.__dict__.setdefault("_band_cut_ring", {})
        r = ring.get(m)
        if r is None:
            r = ring[m] = [[torch.empty((m,), dtype=torch.int64).pin_memory() for _ in range(4)], 0]
        r[1] += 1
        return r[0][r[1] % len(r[0])]

    def coherent_layout(self, hit_count, ray_offset, total: int, width: int, tile_base=None, want_order=True,
                        band_rows: int = 0):
        """(order, inverse): the int32 permutation of the ``total`` packed samples of a row-major ``width``-wide image,
        ordered (8x8 tile, hit rank, pixel), and its inverse map (``inverse[sample] = position``).  Handing ``order`` to
        ``radiance_field(points, dirs, order=...)`` makes the points of one wave pass neighbours on the same surface
        patch (cache locality only; results are unchanged); ``want_order=False`` returns None for it.  Given the inverse,
        ``qf_pack_samples`` also writes ``xyz[order]`` / ``dirs[order]``, so ``field(xyz_c, dirs_c)`` reads and writes
        sequentially (the indirection through ``order`` costs it 10 %), and
        ``derive_properties(..., sample_index=inverse)`` picks colour and density back up per ray.  ``tile_base``: the
        exclusive scan of the tile totals when ``qf_frame_offsets`` already produced it."""
        height = hit_count.shape[0] // width
        tiles = ((width + 7) // 8) * ((height + 7) // 8)
        dev = hit_count.device
        if tile_base is None:
            totals = torch.empty((tiles,), dtype=torch.int64, device=dev)
            _C.check(_C.lib().qf_tile_totals(_C.ptr(hit_count), width, height, _C.ptr(totals), _C.stream()), "qf_tile_totals")
            tile_base = (torch.cumsum(totals, dim=0) - totals).contiguous()
        # a lean (render-only) frame streams the coherent copies and never reads the forward permutation: skip it
        order = torch.empty((total,), dtype=torch.int32, device=dev) if want_order else None
        inverse = torch.empty((total,), dtype=torch.int32, device=dev)
        _C.check(_C.lib().qf_coherent_layout(_C.ptr(hit_count), _C.ptr(ray_offset), _C.ptr(tile_base), width, height,
                                             _C.ptr(order), _C.ptr(inverse), int(band_rows), _C.stream()),
                 "qf_coherent_layout")
        return order, inverse

    @_on_device
    def split_layout(self, index_ray: torch.Tensor, width: int, height: int, want_order: bool = True):
        """(order or None, inverse, invalid flag) -- the coherent processing order of ``coherent_layout`` for the samples
        of one SPLIT of a ``width x height`` frame, from its ascending ray ids alone (``qf_split_layout``: four launches,
        no host wait).  This is what lets ``render_image_finetune_with_occgrid`` stream the field kernel when the
        caller -- the reference's eval loop -- hands it a 160 000-ray window and no order.  Ids that are not ascending
        or lie outside the frame give the identity (flag set on the device, not read here)."""
        index_ray = _C.i64c(index_ray)
        n = index_ray.shape[0]
        n_rays = int(width) * int(height)
        if n == 0:
            empty = torch.empty((0,), dtype=torch.int32, device=self.device)
            return (empty if want_order else None), empty.clone(), torch.zeros((1,), dtype=torch.int32, device=self.device)
        key = (n_rays, int(width), _C.raw_stream())
        sc = self._split_scratch.get(key)
        if sc is None:
            if len(self._split_scratch) > 4:
                self._split_scratch.clear()
            tiles = ((width + 7) // 8) * ((height + 7) // 8)
            sc = self._split_scratch[key] = (torch.empty((n_rays,), dtype=torch.int32, device=self.device),
                                             torch.empty((n_rays + 1,), dtype=torch.int64, device=self.device),
                                             torch.empty((tiles,), dtype=torch.int64, device=self.device),
                                             torch.zeros((1,), dtype=torch.int32, device=self.device))
        hit_count, ray_offset, tile_base, invalid = sc
        order = torch.empty((n,), dtype=torch.int32, device=self.device) if want_order else None
        inverse = torch.empty((n,), dtype=torch.int32, device=self.device)
        _C.check(_C.lib().qf_split_layout(_C.ptr(index_ray), n, int(width), int(height), _C.ptr(hit_count),
                                          _C.ptr(ray_offset), _C.ptr(tile_base), _C.ptr(invalid), _C.ptr(order),
                                          _C.ptr(inverse), _C.stream()), "qf_split_layout")
        return order, inverse, invalid

    @torch.no_grad()
    def _warn_if_not_unit(self, vectors) -> None:
        """The re-origin rule compares the ray parameter t with a WORLD distance (``min_separation``), i.e. it assumes unit
        directions -- what every caller of the reference passes (nerf_synthetic.py:341-358 normalises its rays) and what
        trimesh enforces itself (it unitises the directions it is given).  Host arrays are cheap to check: warn once."""
        if self.min_separation <= 0 or getattr(self, "_warned_unit", False) or not isinstance(vectors, np.ndarray):
            return
        if vectors.size == 0:
            return
        nrm = np.linalg.norm(np.asarray(vectors, dtype=np.float64).reshape(-1, 3), axis=1)
        if float(np.abs(nrm - 1.0).max()) > 1e-3:
            import warnings
            self._warned_unit = True
            warnings.warn("RayIntersector: ray directions are not unit vectors; the multi-hit rule's separation "
                          f"({self.min_separation:.3g}) is applied to the ray parameter t, i.e. scaled by 1/|d| -- normalise "
                          "the directions (as trimesh does) or set min_separation for your parametrisation", stacklevel=3)

    def intersects_id(self, origins, vectors, multiple_hits=True, return_locations=True, max_hits=10):
        """numpy (index_tri[S], index_ray[S], locations[S,3]) like trimesh / mesh_utils.py:86-109.  Rows come
        grouped by ray, front to back (a valid ordering: the reference's callers sort anyway)."""
        k = int(max_hits) if multiple_hits else 1
        self._warn_if_not_unit(vectors)
        out = self.sample_device(origins, vectors, k)
        if out is None:
            return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 3), np.float64)
        xyz, _, index_ray, _, index_tri, _ = out
        return index_tri.cpu().numpy(), index_ray.cpu().numpy(), xyz.cpu().numpy().astype(np.float64)


class MeshFinetune:
    """Per-triangle accumulation of weighted displacements and the vertex update (mesh_utils.py:112-156).
    scatter_add / scatter_mean run as torch index_add_ on the device (not on the render hot path)."""

    def __init__(self, vertices, faces, scaling, device="cuda:0") -> None:
        self.vertices = np.array(vertices).astype(np.float32)
        self.device = _resolve_device(device)
        self.faces = torch.from_numpy(np.asarray(faces)).to(self.device).long()
        # one 16-byte row per triangle (sum d w | sum w): qf_mesh_update_d's four atomics of a sample are one request
        self._cache = torch.zeros((self.faces.shape[0], 4), device=self.device)
        self.cache_d = self._cache[:, :3]                 # the reference's two attributes, as views
        self.cache_w = self._cache[:, 3]
        self.cache_w[:] = 1e-8
        self.scaling = scaling
        # samples whose triangle id was outside [0, n_faces): counted on the device by update_d, raised by check_ids()
        self._skipped = torch.zeros((1,), dtype=torch.int32, device=self.device)

    @torch.no_grad()
    def update_d(self, d, w, index_tri):
        """cache_d[tri] += d * w, cache_w[tri] += w (mesh_utils.py:126-131) in one launch (``qf_mesh_update_d``).
        ``d`` may be None: a displacement that is identically zero (``scaling == 0``) leaves cache_d as it is.
        The reference's ``scatter_add`` raises at once on a triangle id outside the mesh; here such samples are skipped
        and counted on the device (no host wait per split), and ``check_ids`` -- called by ``update_faces``, which
        synchronises anyway -- raises ``IndexError``."""
        n = int(w.shape[0])
        if n == 0:
            return
        with torch.cuda.device(self.device):
            _C.check(_C.lib().qf_mesh_update_d(
                _C.ptr(_C.f32c(d.reshape(-1, 3))) if d is not None else None, _C.ptr(_C.f32c(w.reshape(-1))),
                _C.ptr(_C.i64c(index_tri.reshape(-1))), n, int(self.faces.shape[0]), _C.ptr(self._cache),
                _C.ptr(self._skipped), _C.stream()), "qf_mesh_update_d")

    def check_ids(self) -> None:
        """Raises if any ``update_d`` since the last check saw a triangle id outside ``[0, n_faces)`` (host wait)."""
        bad = int(self._skipped.item())
        if bad:
            self._skipped.zero_()
            raise IndexError(f"MeshFinetune.update_d: {bad} sample(s) carried a triangle id outside [0, "
                             f"{int(self.faces.shape[0])}) and were skipped (stale samples after a mesh swap?)")

    @torch.no_grad()
    def update_faces(self):
        self.check_ids()
        deformation = torch.clip(self.cache_d / self.cache_w.unsqueeze(1), -self.scaling, self.scaling)
        df_vertices = torch.repeat_interleave(deformation, dim=0, repeats=3)
        flat = self.faces.flatten()
        n_v = self.vertices.shape[0]
        dv = torch.zeros((n_v, 3), device=self.device).index_add_(0, flat, df_vertices)
        cnt = torch.zeros(n_v, device=self.device).index_add_(0, flat, torch.ones_like(flat, dtype=torch.float32))
        self.vertices += (dv / cnt.clamp_min(1.0)[:, None]).cpu().numpy()

    @torch.no_grad()
    def reset_d(self):
        self.cache_d[:] = 0
        self.cache_w[:] = 1e-8


class MeshIntersection:
    """Quadrature-point generator of the mesh path (mesh_utils.py:180-412).  ``mesh_path`` may also be a
    ``TriMesh``.  ``optix`` is accepted and ignored: there is one intersector, the gfx950 BVH."""

    def __init__(self, mesh_path, simplify_mesh=True, scale=1.0, num_repeat=16, optix=False, voxel_size=512,
                 num_intersections=20, render_step_size=0.005, device="cuda:0", min_hit_separation="trimesh",
                 bvh_builder="host"):
        if isinstance(mesh_path, TriMesh):
            self.mesh = TriMesh(mesh_path.vertices.copy(), mesh_path.faces.copy(), mesh_path.visual.uv)
        else:
            self.mesh = load_mesh(mesh_path)
        if simplify_mesh:
            # The reference's default (mesh_utils.py:181).  It does not run THERE either: the open3d branch is disabled by
            # an `import nonsense` (:186), every mesh is a trimesh.Trimesh, and `simplify_vertex_clustering` (:199) is an
            # open3d method -- AttributeError.  Every script of the reference passes simplify_mesh=False.
            raise NotImplementedError("simplify_mesh=True: vertex-clustering simplification is offline mesh tooling (out "
                                      "of scope) -- and the reference's own default path raises AttributeError (its open3d "
                                      "branch is disabled, mesh_utils.py:186,199); its scripts pass simplify_mesh=False")
        self.num_repeat = num_repeat
        self.num_intersections = num_intersections
        self.render_step_size = render_step_size
        self.device = _resolve_device(device)
        self.mesh.vertices *= scale
        self.vertices = torch.from_numpy(self.mesh.vertices.astype(np.float32)).to(self.device)
        # min_hit_separation: the re-origin distance of the reference's trimesh intersector (default), a distance in
        # world units, or 0 / None to count every hit (``RayIntersector``)
        # bvh_builder: "host" (binned SAH) or "device" (linear BVH built on the GPU: far faster to build, slower to traverse)
        self.rayintersector = RayIntersector(self.mesh, max_hits=self.num_intersections, device=self.device,
                                             min_separation=min_hit_separation, builder=bvh_builder)

    def closest_points(self, points, max_distance: float = math.inf) -> ClosestPoints:
        """``RayIntersector.closest_points`` of this mesh's intersector."""
        return self.rayintersector.closest_points(points, max_distance)

    def find_deltas(self, boundary, depth):
        """Constant step for every sample (mesh_utils.py:225-231; B-4)."""
        return torch.full((depth.shape[0],), self.render_step_size, dtype=torch.float32, device=self.device)

    def sampling_raytrace_device(self, vectors, origins, image_width: int = 0, camera=None, layout: bool = True,
                                 window_rays: int = 0):
        """Fast path of ``sampling_raytrace_numpy``: same six arrays, on the device, no host round trip.
        ``camera`` (``make_camera``): the rays are that camera's full pixel grid -> camera-coherent intersector.
        ``window_rays`` (with a camera or an image width, and ``layout``): the caller will cut the frame into windows of
        this many rays (``generate_splits``, 160 000 in the reference's eval loop).  When that is a whole number of rows the
        result is a ``SampleSet``: the same six tensors (it IS a tuple of them) that also carries ONE frame-wide coherent
        layout whose tile grid restarts at every window, so that ``generate_splits`` hands out windows without a search or
        a host wait and ``render_image_finetune_with_occgrid`` streams each of them without deriving a layout."""
        ri = self.rayintersector
        width = int(camera.width) if camera is not None else int(image_width)
        band_rows = 0
        if layout and window_rays and width > 0 and window_rays % width == 0:
            band_rows = int(window_rays) // width
        data = ri.sample_device(origins, vectors, self.num_intersections, image_width, camera, layout=layout,
                                band_rows=band_rows)
        if data is None or not band_rows or ri.last_band_cuts is None or ri.last_layout is None:
            return data
        cuts_host, band_rays = ri.last_band_cuts
        inverse, xyz_c, dirs_c = ri.last_layout
        n_rays = int(vectors.shape[0]) if hasattr(vectors, "shape") else int(len(vectors))
        return SampleSet(data, cuts=cuts_host.tolist(), window_rays=band_rays, num_rays=n_rays, inverse=inverse,
                         order=ri.last_order, xyz_c=xyz_c, dirs_c=dirs_c, width=width)

    def sampling_raytrace_numpy(self, vectors, origins, random=0):
        """numpy 7-tuple (points, dirs, index_ray, depth, index_tri, 0, origins) sorted by (ray, depth), or None
        when nothing is hit -- mesh_utils.py:343-387.  (The reference returns float64 arrays that the loader
        casts to float32, nerf_synthetic.py:256-257; these are the float32 values directly.)"""
        self.rayintersector._warn_if_not_unit(vectors)
        out = self.sampling_raytrace_device(vectors, origins)
        if out is None:
            return None
        xyz, dirs, index_ray, depth, index_tri, org = [t.cpu().numpy() for t in out]
        return xyz, dirs, index_ray, depth, index_tri, 0, org

    def sampling_indexing(self, points, origins, vectors, index_ray, depth, index_tri, random=0, layout_inverse=None,
                          lean=False):
        """Re-sort by (ray, depth) after deformation, boundaries, deltas -- mesh_utils.py:389-412, without
        leaving the device.  Inference: ONE launch (``qf_resort_samples``: sort, gathers and boundaries fused).
        When autograd is recording on the inputs (training) the permutation is applied with differentiable
        indexing instead.
        ``layout_inverse`` (extension, inference only; from ``RayIntersector.split_layout`` on the same ``index_ray``):
        the launch also writes the re-sorted positions / directions in the coherent order; they are left in
        ``self.last_resort_layout = (points_c, vectors_c)`` (the return value keeps the reference's 8-tuple).
        ``lean`` (extension, inference only): the caller reads neither the re-sorted origins nor the re-sorted triangle ids
        (``render_image_finetune_with_occgrid`` discards both, utils.py:574-577): they are not produced (None in the tuple)."""
        self.last_resort_layout = None
        index_ray = _C.i64c(index_ray)
        n = depth.shape[0]
        dev = depth.device
        if torch.is_grad_enabled() and any(t.requires_grad for t in (points, depth, origins, vectors)):
            depth_c = _C.f32c(depth.detach())
            perm = torch.empty((n,), dtype=torch.int64, device=dev)
            _C.check(_C.lib().qf_resort_by_depth(_C.ptr(index_ray), _C.ptr(depth_c), n, _C.ptr(perm), _C.stream()),
                     "qf_resort_by_depth")
            index_tri, index_ray = index_tri[perm], index_ray[perm]
            points, depth, origins, vectors = (_permute_rows(t, perm) for t in (points, depth, origins, vectors))
            boundary = spc_render.mark_pack_boundaries(index_ray)
            return points, self.find_deltas(boundary, depth), boundary, vectors, index_ray, depth, index_tri, origins
        points, depth, vectors = (_C.f32c(t.detach()) for t in (points, depth, vectors))
        if lean:
            origins = index_tri = o_origins = o_tri = None
        else:
            origins, index_tri = _C.f32c(origins.detach()), _C.i64c(index_tri)
            o_origins, o_tri = torch.empty_like(origins), torch.empty_like(index_tri)
        o_points, o_vectors = torch.empty_like(points), torch.empty_like(vectors)
        o_depth = torch.empty_like(depth)
        boundary = torch.empty((n,), dtype=torch.bool, device=dev)
        points_c = vectors_c = None
        if layout_inverse is not None:
            if layout_inverse.shape[0] != n:
                raise ValueError(f"layout_inverse has {layout_inverse.shape[0]} entries for {n} samples")
            points_c, vectors_c = torch.empty_like(points), torch.empty_like(vectors)
        _C.check(_C.lib().qf_resort_samples(
            _C.ptr(index_ray), _C.ptr(depth), n, _C.ptr(points), _C.ptr(origins), _C.ptr(vectors), _C.ptr(index_tri),
            None, _C.ptr(o_points), _C.ptr(o_depth), _C.ptr(o_origins), _C.ptr(o_vectors), _C.ptr(o_tri),
            _C.ptr(boundary), _C.ptr(layout_inverse, torch.int32), _C.ptr(points_c), _C.ptr(vectors_c), _C.stream()),
            "qf_resort_samples")
        if layout_inverse is not None:
            self.last_resort_layout = (points_c, vectors_c)
        return o_points, self.find_deltas(boundary, o_depth), boundary, o_vectors, index_ray, o_depth, o_tri, o_origins
