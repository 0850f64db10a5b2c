"""Stage 6a of the baking pipeline: prune the finetuned mesh (``examples/prune_mesh_after_finetuning.py:323-373``).

The reference renders every training view (at ``up_sample`` 2, ``scaling`` 0), scatter-maxes the view's compositing
weights over the samples' triangles, keeps the running maximum over the views, drops the faces whose maximum is not above
1e-3 and writes ``triangle_weights.npy``, ``mesh_updated.ply``, ``num_samples.npy`` and ``num_valid_samples.npy`` next to
the mesh.  ``MeshPruner`` is that loop on the device: a camera view is ONE bound call (``qf_frame_prune``: the frame's
launch sequence with the tile compositor folding its weights into ``triangle_weights``), no weight
array, no host wait per view; the per-view counts live in a device table that ``sample_counts()`` reads once.
"""
import ctypes
import os
from typing import Optional

import numpy as np
import torch

from . import _C, baking
from .mesh_io import TriMesh
from .radiance_fields.ngp import NGPRadianceField, NGPRadianceFieldSGNew
from .render import FrameRenderer

FILES = ("triangle_weights.npy", "mesh_updated.ply", "num_samples.npy", "num_valid_samples.npy")
MAP_FILES = ("face_map.npy", "vertex_map.npy")           # written beside FILES with ``compact``


def write_pruning_files(out_dir: str, mesh: TriMesh, triangle_weights, num_samples, num_valid_samples,
                        threshold: float = 1e-3, compact: bool = False, min_component_faces: int = 0) -> TriMesh:
    """The stage's four files (``FILES``) in ``out_dir``: the float32 maxima [F], the pruned mesh (vertices kept), the
    per-view int64 counts [n_views].  With ``compact`` the mesh written is the cleaned one (``baking.prune_faces``) and
    ``MAP_FILES`` are written beside the four: the source face / vertex of its rows; the three per-face and per-view
    arrays still describe the original mesh.  Returns the pruned mesh."""
    tw = triangle_weights.detach().cpu().numpy() if isinstance(triangle_weights, torch.Tensor) else np.asarray(triangle_weights)
    tw = np.ascontiguousarray(tw, dtype=np.float32).reshape(-1)
    if tw.shape[0] != mesh.faces.shape[0]:
        raise ValueError(f"{tw.shape[0]} triangle weights for {mesh.faces.shape[0]} faces")
    if compact:
        pruned, face_map, vertex_map = baking.prune_faces(mesh, tw, threshold, compact=True,
                                                          min_component_faces=min_component_faces, return_maps=True)
    else:
        pruned = baking.prune_faces(mesh, tw, threshold)
    os.makedirs(out_dir, exist_ok=True)
    if compact:
        np.save(os.path.join(out_dir, MAP_FILES[0]), face_map)
        np.save(os.path.join(out_dir, MAP_FILES[1]), vertex_map)
    np.save(os.path.join(out_dir, FILES[0]), tw)
    pruned.export(os.path.join(out_dir, FILES[1]))
    np.save(os.path.join(out_dir, FILES[2]), np.asarray(num_samples, dtype=np.int64).reshape(-1))
    np.save(os.path.join(out_dir, FILES[3]), np.asarray(num_valid_samples, dtype=np.int64).reshape(-1))
    return pruned


class MeshPruner:
    """Per-triangle maximum compositing weight over views, and the mesh without the faces nobody sees.

    ``triangle_weights``: device float32 [F], the running maximum.  ``threshold``: faces with a maximum <= it are dropped
    (strict comparison, :363); ``valid_threshold``: what ``num_valid_samples`` counts above (:353).  ``render_step_size``
    as ``FrameRenderer`` (the mesh intersector's)."""

    def __init__(self, mesh_intersect, radiance_field, render_step_size: Optional[float] = None, threshold: float = 1e-3,
                 valid_threshold: float = 1e-3):
        self._renderer = FrameRenderer(mesh_intersect, radiance_field, None, render_step_size)
        self.mesh_intersect = mesh_intersect
        self.radiance_field = radiance_field
        self.threshold = float(threshold)
        self.valid_threshold = float(valid_threshold)
        self.device = mesh_intersect.device
        self.n_faces = int(mesh_intersect.mesh.faces.shape[0])
        self.triangle_weights = torch.zeros((self.n_faces,), dtype=torch.float32, device=self.device)
        self.n_views = 0
        self._counts = torch.zeros((16, 2), dtype=torch.int64, device=self.device)
        self._bad_ids = torch.zeros((1,), dtype=torch.int32, device=self.device)

    def _next_counts(self) -> torch.Tensor:
        """Row ``n_views`` of the device count table (zeros), which grows geometrically -- a device copy, no host wait."""
        if self.n_views == self._counts.shape[0]:
            grown = torch.zeros((2 * self.n_views, 2), dtype=torch.int64, device=self.device)
            grown[:self.n_views] = self._counts
            self._counts = grown
        row = self._counts[self.n_views]
        self.n_views += 1
        return row

    @torch.no_grad()
    def add_view(self, origins: torch.Tensor, viewdirs: torch.Tensor, camera):
        """One training view: ``origins`` / ``viewdirs`` [W*H,3] are the pixel grid of ``camera`` (``make_camera``).  The
        whole view is enqueued on the current stream without a host wait.  As ``FrameRenderer.render_async``: on the plain
        camera-coherent pass with an fp32 / fp16 NGP or SG field it is one ``qf_frame_prune``; otherwise (the
        intersector's policy is in its dense mode or backing off, another field) the stages are enqueued one by one and
        the tile compositor still folds the weights.  Rays that are not the camera's (the pass's device-side check) or
        pixels with more than K candidates are repaired inside the sequence.  Returns the frame record."""
        fr, rf = self._renderer, self.radiance_field
        ri = self.mesh_intersect.rayintersector
        k = self.mesh_intersect.num_intersections
        with torch.cuda.device(ri.device):
            counts = self._next_counts()
            one_call = (getattr(rf, "discretize", False) is False and type(rf) in (NGPRadianceField, NGPRadianceFieldSGNew)
                        and rf.compute_dtype in ("fp32", "fp16") and ri.fused_frame_ready(camera, k))
            prepared = fr._one_call_job(origins, viewdirs, camera, k, None, False, want_tri=True, image=False) if one_call else None
            if prepared is not None:
                job, frame, token, keep, _ = prepared
                ri.last_route = "frame+cull" if job.cull_chunks & 1 else "frame"
                _C.check(_C.lib().qf_frame_prune(ri._handle, ctypes.byref(job), _C.ptr(self.triangle_weights), self.n_faces,
                                                 self.valid_threshold, _C.ptr(counts), _C.ptr(self._bad_ids), _C.stream()),
                         "qf_frame_prune")
                ri.fused_frame_done(frame, token)
                frame._keep = frame._keep + keep
                return frame
            if getattr(rf, "discretize", False) is False:
                frame = ri.sample_frame_device(origins, viewdirs, k, camera, want_tri=True)
                _, xyz_c, dirs_c = ri.last_layout
                rgbs, sigmas = rf(xyz_c, dirs_c, n_device=frame.total_dev)
            else:               # tensor-op field (uint8 round trips): it needs the sample count on the host
                if ri.sample_device(origins, viewdirs, k, camera.width, camera, lean=True, want_tri=True) is None:
                    return None
                frame = ri.last_frame
                _, xyz_c, dirs_c = ri.last_layout
                rgbs, sigmas = rf(xyz_c, dirs_c)
            self._fold_frame(rgbs, sigmas, frame, counts)
            return frame

    def _fold_frame(self, rgbs, sigmas, frame, counts) -> None:
        """``qf_composite_tiles_trimax`` without an image on a frame in the intersector's coherent order."""
        rgbs, sigmas = _C.f32c(rgbs.reshape(-1, 3)), _C.f32c(sigmas.reshape(-1))
        n = frame.depth_c.shape[0]
        if rgbs.shape[0] != n or sigmas.shape[0] != n or frame.tri_c is None:
            raise ValueError(f"MeshPruner: {n} slots in the frame, {rgbs.shape[0]} colours, {sigmas.shape[0]} densities")
        _C.check(_C.lib().qf_composite_tiles_trimax(
            _C.ptr(rgbs), _C.ptr(sigmas), _C.ptr(frame.depth_c), float(self._renderer.render_step_size),
            _C.ptr(frame.hit_count), frame.max_hits, _C.ptr(frame.tile_base), frame.width, frame.height, _C.BG_WHITE, None,
            None, None, None, None, _C.ptr(frame.tri_c, torch.int32), _C.ptr(self.triangle_weights), self.n_faces,
            self.valid_threshold, _C.ptr(counts), _C.ptr(self._bad_ids), _C.stream()), "qf_composite_tiles_trimax")

    @torch.no_grad()
    def add_samples(self, weights: torch.Tensor, index_tri: torch.Tensor) -> None:
        """One view given as its samples' weights [S] or [S,1] and triangle ids [S] -- what
        ``render_image_finetune_with_occgrid`` returns, for callers that render with a non-zero ``scaling`` -- through
        ``qf_scatter_max``.  Same ``triangle_weights``, same counters."""
        w = _C.f32c(weights.detach().reshape(-1)).to(self.device)
        idx = _C.i64c(index_tri.reshape(-1)).to(self.device)
        if w.shape[0] != idx.shape[0]:
            raise ValueError(f"add_samples: {w.shape[0]} weights for {idx.shape[0]} triangle ids")
        with torch.cuda.device(self.device):
            counts = self._next_counts()
            counts[0] = w.shape[0]
            counts[1] = (w > self.valid_threshold).sum()
            self._bad_ids += ((idx < 0) | (idx >= self.n_faces)).sum().to(torch.int32)
            baking.triangle_max_weights(w, idx, self.triangle_weights)

    def sample_counts(self):
        """(num_samples, num_valid_samples): numpy int64 [n_views] -- the one host wait.  Raises ``IndexError`` when a
        view carried triangle ids outside the mesh (they were skipped)."""
        bad = int(self._bad_ids.item())
        if bad:
            raise IndexError(f"MeshPruner: {bad} sample(s) carried a triangle id outside [0, {self.n_faces}) and were "
                             "skipped (samples of another mesh?)")
        c = self._counts[:self.n_views].cpu().numpy()
        return c[:, 0].copy(), c[:, 1].copy()

    def keep_mask(self) -> torch.Tensor:
        """Device bool [F]: ``triangle_weights > threshold``."""
        return self.triangle_weights > self.threshold

    def pruned_mesh(self, compact: bool = False, min_component_faces: int = 0) -> TriMesh:
        """The mesh with the masked-out faces removed, face order preserved; vertices (and per-vertex UVs) kept as they
        are, as ``trimesh.update_faces`` leaves them.  ``compact``: the vertices no kept face uses are removed too, and
        with ``min_component_faces`` >= 2 the small islands (``baking.prune_faces``)."""
        return baking.prune_faces(self.mesh_intersect.mesh, self.keep_mask(), compact=compact,
                                  min_component_faces=min_component_faces)

    def save(self, out_dir: str, compact: bool = False, min_component_faces: int = 0) -> TriMesh:
        """Write the reference's four files into ``out_dir`` (with ``compact`` the cleaned mesh and its two maps,
        ``write_pruning_files``); returns the pruned mesh."""
        num_samples, num_valid = self.sample_counts()
        return write_pruning_files(out_dir, self.mesh_intersect.mesh, self.triangle_weights, num_samples, num_valid,
                                   self.threshold, compact=compact, min_component_faces=min_component_faces)
