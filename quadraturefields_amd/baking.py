"""Producer side of the baked-texture format and triangle pruning.

* ``bake_texture_images``: ``examples/bake_texture_images_shelly.py:270-294`` -- evaluate the SG field's features
  and the density field at every valid texel of ``V`` (texel -> 3-D point, all-zero rows are empty), quantise with
  the reference's codecs and scatter into the uint8 texture set.
* ``bake_texture_set``: the same stage as a fixed launch sequence per band of rows of a device ``V`` -- compact the
  valid texels, the two field launches bounded by the device count, one encode launch into the planes -- without a
  host wait (``qf_bake_compact_texels`` / ``qf_bake_encode_texels``).
* ``texel_positions``: the texel-position map ``V`` itself from a UV-mapped mesh -- the fill of the reference's UV stage
  (``examples/parameterization_utils.py:97-153``), one HIP call (``qf_texel_positions``).
* ``bake_vertex_features``: the vertex-baked asset of ``render_image_finetune_baking_with_occgrid`` -- the SG field's
  features once per mesh vertex.
* ``VertexBakedFeatures`` / ``finetune_vertex_features``: that table as a trainable module, and the loop that fits it to
  images through the differentiable vertex shading.
* ``quantise_vertex_features`` / ``QuantisedVertexFeatures``: that table as 64-byte uint8 records in the reference's
  texture format, shaded in place by the ``qf_vertex_quant_*`` kernels and stored as the uint8 PNG set (DESIGN.md section
  3.5f).
* ``triangle_max_weights`` / ``prune_faces``: ``examples/prune_mesh_after_finetuning.py:323-373`` -- per-triangle
  maximum compositing weight over the training views, faces below 1e-3 dropped.
* ``subdivide_vertex_features`` / ``vertex_edge_error`` / ``refine_vertex_baked``: the vertex table carried through a
  midpoint split of the mesh, the per-edge error of the table against the field, and the loop that splits the mesh where
  that error is above a tolerance.
"""
import ctypes
import math
from collections import namedtuple

import numpy as np
import torch

from . import _C
from ._mesh_args import counts_buffer, mesh_inputs, read_counts, to_numpy, trimesh_tensors, workspace
from .mesh_io import TriMesh


UNTOUCHED_MODES = {"last_face": _C.UNTOUCHED_LAST_FACE, "zero": _C.UNTOUCHED_ZERO}
MAX_TEXTURE_SIDE = 16384


@torch.no_grad()
def texel_positions(mesh: TriMesh, height: int, width: int = None, untouched: str = "last_face", device=None):
    """Texel-position map of a UV-mapped mesh: ``(V, tri_size)`` with V a device float32 tensor [height, width, 3] (the
    3-D point each texel stands for, what the reference saves as ``V_{size}.npy``) and tri_size a device int64 tensor
    [F] (texels in each face's cover).  ``uv[:,0]`` selects the row.  ``untouched``: what a texel no face covers and no
    edge touches gets -- "last_face" (the reference: the centroid of face F-1) or "zero" (left empty, so that
    ``bake_texture_images`` skips it).  The host only validates and uploads; the map is computed on the device."""
    width = height if width is None else width
    uv = getattr(getattr(mesh, "visual", None), "uv", None)
    if uv is None:
        raise ValueError("texel_positions needs a mesh with per-vertex UVs (mesh.visual.uv)")
    if untouched not in UNTOUCHED_MODES:
        raise ValueError(f"untouched must be one of {sorted(UNTOUCHED_MODES)}, got {untouched!r}")
    for name, n in (("height", height), ("width", width)):
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= n <= MAX_TEXTURE_SIDE:
            raise ValueError(f"{name} must be an integer in [1, {MAX_TEXTURE_SIDE}], got {n!r}")
    height, width = int(height), int(width)
    if height * width >= 1 << 31:
        raise ValueError(f"height * width must be below 2^31, got {height} x {width}")
    vertices = np.ascontiguousarray(mesh.vertices, dtype=np.float64).reshape(-1, 3)
    faces = np.ascontiguousarray(mesh.faces, dtype=np.int64).reshape(-1, 3)
    uv = np.ascontiguousarray(uv, dtype=np.float64)
    if uv.shape != (vertices.shape[0], 2):
        raise ValueError(f"uv must be [V, 2] = [{vertices.shape[0]}, 2], got {list(uv.shape)}")
    if faces.shape[0] < 1:
        raise ValueError("texel_positions needs at least one face")
    if faces.min() < 0 or faces.max() >= vertices.shape[0]:           # the C entry cannot check device indices
        raise ValueError(f"face indices must lie in [0, {vertices.shape[0]})")
    if not np.isfinite(uv).all():
        raise ValueError("uv must be finite")
    dev = _C.resolve_device(device if device is not None else "cuda")
    n_faces = faces.shape[0]
    ws_bytes = int(_C.lib().qf_texel_positions_workspace_bytes(n_faces, height, width))
    v_d = torch.from_numpy(vertices).to(dev)
    f_d = torch.from_numpy(faces).to(dev)
    uv_d = torch.from_numpy(uv).to(dev)
    out = torch.empty((height, width, 3), dtype=torch.float32, device=dev)
    tri_size = torch.empty((n_faces,), dtype=torch.int64, device=dev)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _C.check(_C.lib().qf_texel_positions(_C.ptr(v_d), vertices.shape[0], _C.ptr(f_d), n_faces, _C.ptr(uv_d),
                                             height, width, UNTOUCHED_MODES[untouched], _C.ptr(out), _C.ptr(tri_size),
                                             _C.ptr(ws), ws_bytes, _C.stream()), "qf_texel_positions")
    return out, tri_size


@torch.no_grad()
def bake_texture_images(radiance_field_sg, radiance_field, V, compressor, batch_size: int = 100000):
    """Fill ``compressor``'s texture maps in place; returns the boolean texel mask (V.sum(-1) != 0).  ``V`` is a numpy
    array (or anything ``np.asarray`` takes) or a device tensor -- ``texel_positions``' output -- which then stays on
    the device: the mask comes back as a device tensor."""
    if isinstance(V, torch.Tensor) and V.is_cuda:
        return _bake_device(radiance_field_sg, radiance_field, V, compressor, batch_size)
    V = np.asarray(V, dtype=np.float32)
    mask = ~(V.sum(-1) == 0)
    ind = np.argwhere(mask)
    dev = compressor.device
    for b in range(0, ind.shape[0], batch_size):
        rows = ind[b:b + batch_size]
        pts = torch.from_numpy(V[rows[:, 0], rows[:, 1]]).to(dev)
        features = radiance_field_sg.features(pts)
        density = radiance_field.query_density(pts)
        features[..., -1] = density.flatten()
        compressor.load_features_into_maps(features, torch.from_numpy(rows).to(dev))
    return mask


def _bake_device(radiance_field_sg, radiance_field, V, compressor, batch_size):
    V = V.to(compressor.device, torch.float32)
    mask = ((V[..., 0] + V[..., 1]) + V[..., 2]) != 0                  # numpy's float32 sum order
    ind = torch.nonzero(mask)                                           # row-major, as np.argwhere
    for b in range(0, ind.shape[0], batch_size):
        rows = ind[b:b + batch_size]
        pts = V[rows[:, 0], rows[:, 1]].contiguous()
        features = radiance_field_sg.features(pts)
        density = radiance_field.query_density(pts)
        features[..., -1] = density.flatten()
        compressor.load_features_into_maps(features, rows)
    return mask


def bake_chunk_rows(texture_size: int, num_lobes: int, workspace_bytes: int = 256 << 20) -> int:
    """Rows of a ``[T, T, 3]`` map that ``bake_texture_set`` takes per band so that the band's buffers -- per texel an
    int32 index, a position (3 floats), a feature row (3 + 7L + 1 floats) and a density -- fit in ``workspace_bytes``;
    at least 1, at most T.  ValueError when a single row does not fit."""
    t, lobes = int(texture_size), int(num_lobes)
    if t < 1 or lobes < 1:
        raise ValueError(f"texture_size and num_lobes must be positive, got {texture_size!r}, {num_lobes!r}")
    row_bytes = t * (4 + 12 + 4 * (3 + 7 * lobes + 1) + 4)
    rows = int(workspace_bytes) // row_bytes
    if rows < 1:
        raise ValueError(f"one row of a {t} x {t} map with {lobes} lobes needs {row_bytes} bytes, "
                         f"workspace_bytes is {workspace_bytes}")
    return min(rows, t)


@torch.no_grad()
def bake_texture_set(radiance_field_sg, radiance_field, V, compressor, rows_per_chunk: int = None):
    """Fill ``compressor``'s texture maps in place from a device texel-position map ``V`` [T, T, 3] (fp32): returns
    ``(mask, count)``, the device bool [T, T] texel mask ((x + y) + z != 0 in fp32) and a device int64 with the number of
    valid texels.  The map is taken in ``ceil(T / rows_per_chunk)`` bands of rows (default: ``bake_chunk_rows``), each a
    fixed sequence of launches -- compact the band's valid texels, the SG field's features and the other field's
    density on them (both bounded by the count in device memory), encode into the planes -- so nothing here waits for
    the device and the sequence depends only on T and ``rows_per_chunk``, never on how many texels are valid."""
    if not isinstance(V, torch.Tensor) or V.dim() != 3 or V.shape[0] != V.shape[1] or V.shape[2] != 3:
        raise ValueError(f"V must be a [T, T, 3] tensor, got {list(getattr(V, 'shape', []))}")
    t = int(V.shape[0])
    if t != compressor.texture_size:
        raise ValueError(f"V is {t} x {t}, the texture set is {compressor.texture_size} x {compressor.texture_size}")
    lobes = int(radiance_field_sg.num_g_lobes)
    if lobes != compressor.num_lobes:
        raise ValueError(f"the field has {lobes} lobes, the texture set {compressor.num_lobes}")
    if rows_per_chunk is None:
        rows_per_chunk = bake_chunk_rows(t, lobes)
    if isinstance(rows_per_chunk, bool) or not isinstance(rows_per_chunk, (int, np.integer)) or rows_per_chunk < 1:
        raise ValueError(f"rows_per_chunk must be an integer >= 1, got {rows_per_chunk!r}")
    if t > MAX_TEXTURE_SIDE:
        raise ValueError(f"texture size must be at most {MAX_TEXTURE_SIDE}, got {t}")
    if not V.is_cuda or V.dtype != torch.float32:
        raise ValueError("V must be a float32 tensor on the device (texel_positions' output)")
    if V.device != compressor.device:
        raise ValueError(f"V is on {V.device}, the texture set on {compressor.device}")
    rows_per_chunk = min(int(rows_per_chunk), t)
    dev = V.device
    V = V.contiguous()
    lib = _C.lib()
    cap = rows_per_chunk * t
    ws_bytes = int(lib.qf_bake_compact_workspace_bytes(cap))
    texel = torch.empty((cap,), dtype=torch.int32, device=dev)
    points = torch.empty((cap, 3), dtype=torch.float32, device=dev)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    counts = torch.empty((-(-t // rows_per_chunk),), dtype=torch.int64, device=dev)
    mask = torch.empty((t, t), dtype=torch.bool, device=dev)
    width = 3 + 7 * lobes + 1
    with torch.cuda.device(dev):
        tex = compressor.texture_set()
        for band, row in enumerate(range(0, t, rows_per_chunk)):
            rows = min(rows_per_chunk, t - row)
            n_dev = counts[band:band + 1]
            _C.check(lib.qf_bake_compact_texels(_C.ptr(V), t, row, rows, _C.ptr(texel), _C.ptr(points), _C.ptr(n_dev),
                                                _C.ptr(mask), _C.ptr(ws), ws_bytes, _C.stream()), "qf_bake_compact_texels")
            pts = points[:rows * t]
            features = radiance_field_sg.features(pts, n_device=n_dev)
            density = radiance_field.query_density(pts, n_device=n_dev)
            _C.check(lib.qf_bake_encode_texels(ctypes.byref(tex), _C.ptr(features), width, _C.ptr(density.reshape(-1)),
                                               _C.ptr(texel), rows * t, _C.ptr(n_dev), _C.stream()),
                     "qf_bake_encode_texels")
    compressor.invalidate_records()       # the planes changed behind torch's version counters: rebuild on next use
    return mask, counts.sum()


@torch.no_grad()
def bake_vertex_features(radiance_field, mesh_intersect, batch_size: int = 1000000) -> torch.Tensor:
    """The vertex-baked asset of ``render_image_finetune_baking_with_occgrid`` (utils.py:819-836): the SG field's feature
    vector ``radiance_field.features`` -- [diffuse3 | (axis3, lambda, colour3) * L | sigma] -- at every vertex of the mesh,
    float32 [V, 3 + 7L + 1] on the device.  The reference evaluates it at the three corners of every sample's triangle,
    every frame; the field depends on the position alone, so once per vertex gives the same values
    (``utils.vertex_baked_shading`` pads the rows for the kernels).  Chunks of ``batch_size`` vertices as the reference's
    loop (:831-833); the values do not depend on it."""
    from .radiance_fields.ngp import NGPRadianceFieldSGNew
    if not isinstance(radiance_field, NGPRadianceFieldSGNew):
        raise NotImplementedError("bake_vertex_features takes an NGPRadianceFieldSGNew: the table holds its SG features")
    vertices = _C.f32c(mesh_intersect.vertices)
    n = vertices.shape[0]
    out = torch.empty((n, 3 + 7 * radiance_field.num_g_lobes + 1), dtype=torch.float32, device=vertices.device)
    for b in range(0, n, int(batch_size)):
        out[b:b + batch_size] = radiance_field.features(vertices[b:b + batch_size])
    return out


class VertexBakedFeatures(torch.nn.Module):
    """The vertex-baked asset as something that trains: ONE parameter ``table``, float32
    [V, ``_C.vertex_row_stride(L)``] -- the rows of ``bake_vertex_features`` zero-padded to 64-byte lines, which is the
    layout the kernels read, so they read the parameter in place and no padded copy is rebuilt after an optimiser step.
    Every function that takes ``vertex_features`` takes this module too and then uses its table directly; the pixels
    equal those of ``features()`` passed as a plain tensor.  The type decides, not the shape: 32 columns is both the
    stride of 2 lobes and the width of 4.

    ``features``: a [V, 3 + 7L + 1] tensor (any device; the table lives on ``device``, default the tensor's).
    ``train_density``: whether the differentiable route hands the density column a gradient (``finetune_vertex_features``
    sets it per run; stage 5's rule is colours over fixed densities)."""

    def __init__(self, features, device=None, train_density: bool = True):
        super().__init__()
        feats = torch.as_tensor(features)
        if feats.dim() != 2 or feats.shape[0] < 1:
            raise ValueError(f"vertex features must be [V, 3 + 7L + 1] with V >= 1, got {tuple(feats.shape)}")
        lobes, rest = divmod(int(feats.shape[1]) - 4, 7)
        if rest or not 1 <= lobes <= _C.QF_MAX_LOBES:
            raise ValueError(f"vertex features must have 3 + 7 L + 1 columns with 1 <= L <= {_C.QF_MAX_LOBES}, "
                             f"got {feats.shape[1]}")
        self.n_lobes = lobes
        self.train_density = bool(train_density)
        table = torch.zeros((feats.shape[0], _C.vertex_row_stride(lobes)), dtype=torch.float32,
                            device=feats.device if device is None else device)
        table[:, :feats.shape[1]] = feats.detach().to(table.device, torch.float32)
        if table.data_ptr() % 64:
            raise RuntimeError("the allocator returned a vertex table that is not 64-byte aligned")
        self.table = torch.nn.Parameter(table)

    @classmethod
    def from_field(cls, radiance_field, mesh_intersect, batch_size: int = 1000000):
        """The table of ``bake_vertex_features(radiance_field, mesh_intersect)``."""
        return cls(bake_vertex_features(radiance_field, mesh_intersect, batch_size))

    @property
    def width(self) -> int:
        return 3 + 7 * self.n_lobes + 1

    def features(self) -> torch.Tensor:
        """The detached [V, 3 + 7L + 1] view of the table: what ``vertex_features.npy`` holds."""
        return self.table.detach()[:, :self.width]

    def check_rows(self, n_vertices: int) -> None:
        if self.table.shape[0] != n_vertices:
            raise ValueError(f"vertex_features must have V = {n_vertices} rows, got {tuple(self.table.shape)}")


def vertex_texture_size(n_vertices: int) -> int:
    """Side T = ceil(sqrt(V)) of the "vertex texture" that holds a V-row quantised vertex table: vertex v lives at texel
    (v // T, v % T)."""
    n = int(n_vertices)
    if n < 1:
        raise ValueError(f"n_vertices must be >= 1, got {n_vertices!r}")
    return math.isqrt(n - 1) + 1


class QuantisedVertexFeatures:
    """The vertex-baked asset quantised to the reference's texture format: a
    ``FeatureCompression`` of side ``vertex_texture_size(V)`` whose texel (v // T, v % T) holds vertex v and whose texels
    ``>= V`` are zero, so that ``compressor.records()`` is the [T*T, 64] uint8 vertex record table (row v = vertex v) the
    ``qf_vertex_quant_*`` kernels read, and ``compressor.save_to_file`` its on-disk form (the uint8 PNG set).  Inference
    only, no ``nn.Module``: every function that takes ``vertex_features`` takes this and dispatches on the type; where a
    gradient is wanted (``finetune_vertex_features``) it is refused with ``TypeError`` -- ``dequantise()`` gives the fp32
    table a ``VertexBakedFeatures`` can go on fitting.  Built by ``quantise_vertex_features`` or ``load``."""

    def __init__(self, compressor, n_vertices: int):
        n_vertices = int(n_vertices)
        t = vertex_texture_size(n_vertices)
        if tuple(compressor.alpha.shape) != (t, t):
            raise ValueError(f"a vertex texture of {n_vertices} vertices is {t} x {t}, the texture set is "
                             f"{tuple(compressor.alpha.shape)}")
        self.compressor = compressor
        self.n_vertices = n_vertices
        self.n_lobes = int(compressor.num_lobes)

    @property
    def width(self) -> int:
        return 3 + 7 * self.n_lobes + 1

    @property
    def device(self):
        return self.compressor.alpha.device

    @property
    def sigmoid_codec(self) -> int:
        return 1 if self.compressor.compression_type == "sigma" else 0     # the reference's string test (B-7)

    def records(self) -> torch.Tensor:
        """[T*T, 64] uint8 on the device: row v is vertex v's record (``FeatureCompression.records``, cached)."""
        return self.compressor.records()

    def check_rows(self, n_vertices: int) -> None:
        if self.n_vertices != n_vertices:
            raise ValueError(f"vertex_features must have V = {n_vertices} rows, got {self.n_vertices}")

    def save(self, path_prefix: str) -> None:
        """The PNG set of ``FeatureCompression.save_to_file``: 2 + 2L files ``path_prefix + name``."""
        self.compressor.save_to_file(path_prefix)

    @classmethod
    def load(cls, path_prefix: str, n_vertices: int, num_lobes: int, compression_type: str = "linear",
             lambda_thres: float = 7.5, device="cuda:0"):
        from .texture_utils import FeatureCompression
        comp = FeatureCompression(num_lobes, path=path_prefix, compression_type=compression_type, lambda_thres=lambda_thres,
                                  device=device)
        return cls(comp, n_vertices)

    @torch.no_grad()
    def dequantise(self, padded: bool = False) -> torch.Tensor:
        """The decoded table, float32 [V, 3 + 7L + 1] (``padded``: [V, ``_C.vertex_row_stride(L)``], the kernels' layout):
        row v is what ``get_features_from_texture_map`` returns for vertex v's texel, bit for bit
        (``qf_vertex_quant_decode``).  The shading of this object equals the fp32 route's on this table bit for bit."""
        records = self.records()
        stride = _C.vertex_row_stride(self.n_lobes) if padded else self.width
        out = torch.empty((self.n_vertices, stride), dtype=torch.float32, device=records.device)
        with torch.cuda.device(records.device):
            _C.check(_C.lib().qf_vertex_quant_decode(_C.ptr(records), self.n_vertices, self.n_lobes, self.sigmoid_codec,
                                                     float(self.compressor.lambda_thres), _C.ptr(out), stride, _C.stream()),
                     "qf_vertex_quant_decode")
        return out


@torch.no_grad()
def quantise_vertex_features(vertex_features, compression_type: str = "linear", lambda_thres: float = 7.5,
                             device=None) -> QuantisedVertexFeatures:
    """Quantise a vertex table -- a [V, 3 + 7L + 1] tensor or a ``VertexBakedFeatures``, e.g. one that
    ``finetune_vertex_features`` fitted -- with the codecs of the texture bake: ONE ``qf_bake_encode_texels`` launch on a
    zeroed T x T set with ``texel = arange(V)`` and the density taken from the last column, so the codes are exactly what
    ``bake_texture_set`` would write for those rows.  ``device``: where the asset lives (default: the table's)."""
    from .texture_utils import FeatureCompression
    feats = vertex_features.features() if isinstance(vertex_features, VertexBakedFeatures) else torch.as_tensor(vertex_features)
    if feats.dim() != 2 or feats.shape[0] < 1:
        raise ValueError(f"vertex features must be [V, 3 + 7L + 1] with V >= 1, got {tuple(feats.shape)}")
    lobes, rest = divmod(int(feats.shape[1]) - 4, 7)
    if rest or not 1 <= lobes <= _C.QF_MAX_LOBES:
        raise ValueError(f"vertex features must have 3 + 7 L + 1 columns with 1 <= L <= {_C.QF_MAX_LOBES}, got {feats.shape[1]}")
    n = int(feats.shape[0])
    t = vertex_texture_size(n)
    if t > MAX_TEXTURE_SIDE:
        raise ValueError(f"{n} vertices need a {t} x {t} vertex texture, the limit is {MAX_TEXTURE_SIDE}")
    dev = _C.resolve_device(feats.device if device is None else device)
    feats = _C.f32c(feats.detach().to(dev))
    comp = FeatureCompression(lobes, initialize=True, texture_size=t, compression_type=compression_type,
                              lambda_thres=lambda_thres, device=dev)
    with torch.cuda.device(dev):
        density = feats[:, -1].contiguous()
        texel = torch.arange(n, dtype=torch.int32, device=dev)
        n_dev = torch.full((1,), n, dtype=torch.int64, device=dev)
        tex = comp.texture_set()
        _C.check(_C.lib().qf_bake_encode_texels(ctypes.byref(tex), _C.ptr(feats), int(feats.shape[1]), _C.ptr(density),
                                                _C.ptr(texel), n, _C.ptr(n_dev), _C.stream()), "qf_bake_encode_texels")
        comp.invalidate_records()             # the planes changed behind torch's version counters
        comp.records()                        # packed here, on the encoding stream: ordered for any later consumer
    return QuantisedVertexFeatures(comp, n)


def finetune_vertex_features(module, mesh_intersect, next_batch, steps: int, lr: float = 1e-2, train_density: bool = False,
                             bg_color="white", render_step_size=None):
    """Fit a ``VertexBakedFeatures`` to images: ``steps`` times ``next_batch() -> (Rays,
    pixels [n, 3])`` (random training rays, as train_fit_sg.py's loop draws them) -> ray-major intersection
    (``sampling_raytrace_device(..., layout=False)``) -> ``utils.render_image_finetune_baking_with_occgrid`` on the module
    under autograd -> ``smooth_l1_loss`` -> ``optim.Adam`` (eps 1e-15), whose update of a zero gradient from zero moments
    is zero: the pad columns stay exactly zero.  ``train_density`` False (stage 5's rule: colours train over fixed
    densities) leaves the density column bit for bit; True trains it too and clamps it at >= 0 after every step, which
    keeps the compositor inside its documented domain.  A batch none of whose rays hits the mesh is skipped (its loss is
    recorded from the background alone).  Returns the loss history, a list of floats read back once at the end."""
    from . import utils
    from .optim import Adam
    if not isinstance(module, VertexBakedFeatures):
        raise TypeError("finetune_vertex_features takes a VertexBakedFeatures (a QuantisedVertexFeatures is inference only: "
                        "fit VertexBakedFeatures(q.dequantise()) and quantise the result)")
    # the renderer composites with the mesh's step (the loader's pack carries no deltas): a value given here replaces it
    # for the run
    was_step = mesh_intersect.render_step_size
    step_size = float(was_step if render_step_size is None else render_step_size)
    mesh_intersect.render_step_size = step_size
    optimizer = Adam([module.table], lr=lr, eps=1e-15)
    was_density, was_grad = module.train_density, module.table.requires_grad
    module.train_density = bool(train_density)
    module.table.requires_grad_(True)
    sigma_col = module.width - 1
    losses = []
    try:
        for _ in range(int(steps)):
            rays, pixels = next_batch()
            origins, viewdirs = rays.origins.reshape(-1, 3), rays.viewdirs.reshape(-1, 3)
            pixels = pixels.reshape(-1, 3).to(module.table.device, torch.float32)
            data = mesh_intersect.sampling_raytrace_device(viewdirs, origins, layout=False)
            if data is None:
                bg = torch.zeros_like(pixels) if bg_color == "black" else torch.ones_like(pixels)
                losses.append(torch.nn.functional.smooth_l1_loss(bg, pixels).detach())
                continue
            rgb = utils.render_image_finetune_baking_with_occgrid(
                None, None, type(rays)(origins=origins, viewdirs=viewdirs), data, render_step_size=step_size,
                mesh_intersect=mesh_intersect, vertex_features=module, bg_color=bg_color)[0]
            loss = torch.nn.functional.smooth_l1_loss(rgb, pixels)
            optimizer.zero_grad(set_to_none=True)
            loss.backward()
            optimizer.step()
            if train_density:
                with torch.no_grad():
                    module.table[:, sigma_col].clamp_(min=0.0)
            losses.append(loss.detach())
    finally:
        module.train_density = was_density
        module.table.requires_grad_(was_grad)
        mesh_intersect.render_step_size = was_step
    return [float(v) for v in torch.stack(losses).cpu()] if losses else []


def triangle_max_weights(weights: torch.Tensor, index_tri: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out[f] = max(out[f], max of ``weights`` over the samples on triangle f) -- scatter_max, in place."""
    w = _C.f32c(weights.reshape(-1))
    idx = _C.i64c(index_tri.reshape(-1))
    if not (out.is_contiguous() and out.dtype == torch.float32):
        raise ValueError("out must be a contiguous float32 tensor")
    _C.check(_C.lib().qf_scatter_max(_C.ptr(w), _C.ptr(idx), w.shape[0], out.shape[0], _C.ptr(out), _C.stream()),
             "qf_scatter_max")
    return out


def prune_faces(mesh: TriMesh, triangle_weights, threshold: float = 1e-3, compact: bool = False,
                min_component_faces: int = 0, return_maps: bool = False):
    """Mesh with the faces whose maximum weight is <= threshold removed (vertices kept, as ``update_faces``).
    ``triangle_weights`` may also be a boolean keep mask, and either may be a device tensor: the faces are then selected
    on the device (the weights / mask make no round trip; only the kept faces come back for the ``TriMesh``).
    ``compact``: the unreferenced vertices are removed as well and the faces remapped, and with ``min_component_faces``
    >= 2 the vertex-connected components of fewer faces are dropped (``mc_utils.compact_mesh``, DESIGN.md section 3.9b,
    on the device); ``return_maps`` then returns ``(mesh, face_map, vertex_map)``, the source face / vertex of every
    output row.  The defaults give the uncompacted mesh, where the maps are the kept faces and every vertex."""
    if not compact and min_component_faces:
        raise ValueError("min_component_faces needs compact=True")
    if compact:
        from . import mc_utils
        if isinstance(triangle_weights, torch.Tensor):
            t = triangle_weights.detach().reshape(-1)
            keep = t if t.dtype == torch.bool else t > threshold
        else:
            tw = np.asarray(triangle_weights).reshape(-1)
            keep = tw if tw.dtype == np.bool_ else tw > threshold
        if keep.shape[0] != mesh.faces.shape[0]:
            raise ValueError(f"{keep.shape[0]} weights for {mesh.faces.shape[0]} faces")
        out = mc_utils.compact_mesh(mesh, keep, min_component_faces=min_component_faces, remove_unreferenced=True)
        return out if return_maps else out[0]
    if isinstance(triangle_weights, torch.Tensor) and triangle_weights.is_cuda:
        t = triangle_weights.detach().reshape(-1)
        keep = t if t.dtype == torch.bool else t > threshold
        if keep.shape[0] != mesh.faces.shape[0]:
            raise ValueError(f"{keep.shape[0]} weights for {mesh.faces.shape[0]} faces")
        faces = torch.from_numpy(np.ascontiguousarray(mesh.faces)).to(t.device)[keep]
        pruned = TriMesh(mesh.vertices.copy(), faces.cpu().numpy(), mesh.visual.uv)
        keep = keep.cpu().numpy()
    else:
        tw = triangle_weights.detach().cpu().numpy() if isinstance(triangle_weights, torch.Tensor) else np.asarray(triangle_weights)
        keep = tw.reshape(-1) if tw.dtype == np.bool_ else tw.reshape(-1) > threshold
        pruned = TriMesh(mesh.vertices.copy(), mesh.faces[keep], mesh.visual.uv)
    if return_maps:
        return pruned, np.nonzero(keep)[0].astype(np.int64), np.arange(mesh.vertices.shape[0], dtype=np.int64)
    return pruned


def remap_vertex_features(vertex_features, vertex_map):
    """The per-vertex table of a compacted mesh: rows ``vertex_map`` (``mc_utils.compact_mesh``'s, int64 [V'], array or
    tensor) of ``vertex_features``.  A tensor [V, W] comes back as a tensor, a ``VertexBakedFeatures`` as a new module
    (same lobes, same ``train_density``, on the same device) whose table holds the selected rows bit for bit.  A
    ``QuantisedVertexFeatures`` is refused with ``TypeError``: its records sit in a vertex texture laid out by V, so
    quantise after compaction (``quantise_vertex_features`` of the remapped fp32 table)."""
    if isinstance(vertex_features, QuantisedVertexFeatures):
        raise TypeError("remap_vertex_features: a QuantisedVertexFeatures cannot be remapped (its vertex texture is laid "
                        "out by V); compact the mesh first, remap the fp32 table and quantise after compaction")
    table = vertex_features.table.detach() if isinstance(vertex_features, VertexBakedFeatures) else vertex_features
    if not isinstance(table, torch.Tensor) or table.dim() != 2:
        raise TypeError("vertex_features must be a [V, W] tensor or a VertexBakedFeatures")
    idx = torch.as_tensor(np.asarray(vertex_map) if not isinstance(vertex_map, torch.Tensor) else vertex_map)
    if idx.dim() != 1 or idx.dtype not in (torch.int64, torch.int32):
        raise ValueError(f"vertex_map must be an int64 vector, got {idx.dtype} {tuple(idx.shape)}")
    idx = idx.to(device=table.device, dtype=torch.int64)
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= table.shape[0]):
        raise IndexError(f"vertex_map reaches outside the table's {table.shape[0]} rows")
    if isinstance(vertex_features, VertexBakedFeatures):
        return VertexBakedFeatures(vertex_features.features()[idx], train_density=vertex_features.train_density)
    return table[idx]


def weld_vertex_features(vertex_features, vertex_class, n_out: int, reduce: str = "first"):
    """The per-vertex table of a welded mesh (``mc_utils.weld_vertices_device``):
    ``vertex_class`` (int64 [V], array or tensor) is the output row of every input vertex, ``n_out`` the number of output
    rows.  ``reduce="first"`` gives every class the row of its root, its lowest vertex, bit for bit -- the same rows as
    ``remap_vertex_features(table, vertex_map)``.  ``reduce="mean"`` gives, per class, the fp64 sum of its members' rows
    taken in increasing vertex index, divided by the member count and rounded once to fp32 (a stable sort by class and a
    sequential segmented sum: the order is the stated one and two runs give the same bits).  A tensor [V, W] comes back
    as a tensor [n_out, W], a ``VertexBakedFeatures`` as a new module (same lobes, same ``train_density``).  Every output
    row needs at least one member, and every class must lie in [0, n_out).  A ``QuantisedVertexFeatures`` is refused with
    ``TypeError``: its records sit in a vertex texture laid out by V, so weld the fp32 table and quantise after."""
    if isinstance(vertex_features, QuantisedVertexFeatures):
        raise TypeError("weld_vertex_features: a QuantisedVertexFeatures cannot be welded (its vertex texture is laid "
                        "out by V); weld the fp32 table and quantise after")
    if reduce not in ("first", "mean"):
        raise ValueError(f"reduce must be 'first' or 'mean', got {reduce!r}")
    baked = isinstance(vertex_features, VertexBakedFeatures)
    table = (vertex_features.features() if baked else vertex_features)
    if not isinstance(table, torch.Tensor) or table.dim() != 2:
        raise TypeError("vertex_features must be a [V, W] tensor or a VertexBakedFeatures")
    table = table.detach()
    cls = torch.as_tensor(np.asarray(vertex_class) if not isinstance(vertex_class, torch.Tensor) else vertex_class)
    if cls.dim() != 1 or cls.dtype not in (torch.int64, torch.int32) or cls.shape[0] != table.shape[0]:
        raise ValueError(f"vertex_class must be an int64 vector of the table's {table.shape[0]} rows, got {cls.dtype} "
                         f"{tuple(cls.shape)}")
    n_out = int(n_out)
    cls = cls.to(device=table.device, dtype=torch.int64)
    if cls.numel() and (int(cls.min()) < 0 or int(cls.max()) >= n_out):
        raise IndexError(f"vertex_class reaches outside the {n_out} output rows")
    order = torch.sort(cls, stable=True).indices                  # by class, members in increasing vertex index
    members = torch.bincount(cls, minlength=n_out)
    if n_out and int(members.min()) == 0:
        raise ValueError("vertex_class leaves an output row without a member")
    start = torch.cumsum(members, 0) - members
    if reduce == "first":
        out = table[order[start]]
    else:
        rows = table[order].to(torch.float64)
        total = rows[start]                                       # the sum starts as the root's row (a -0.0 stays one)
        for k in range(1, int(members.max()) if n_out else 0):    # member k of every class that has one: a gather and an
            has = members > k                                     # add on distinct rows, so the order is the stated one
            total[has] = total[has] + rows[start[has] + k]
        out = (total / members.to(torch.float64)[:, None]).to(table.dtype)
    if baked:
        return VertexBakedFeatures(out, train_density=vertex_features.train_density)
    return out


@torch.no_grad()
def transfer_vertex_features(src_mesh_intersect, vertex_features, dst_vertices, max_distance: float = math.inf):
    """The per-vertex table of ANOTHER mesh of the same surface (a decimated, clustered or re-extracted one): row i is the
    source table blended at the closest point of the source mesh to ``dst_vertices[i]``, ``b0 row[f0] + b1 row[f1] + b2
    row[f2]`` over the closest source triangle f -- the function the vertex-baked renderer draws there.  The query is
    ``closest_points`` of ``src_mesh_intersect`` (a ``MeshIntersection`` or ``RayIntersector`` of the source mesh; DESIGN.md
    section 3.9f); the blend is fp32, left to right, from the barycentrics rounded once to fp32.  ``dst_vertices``: device
    float [V',3].  A tensor [V, W] comes back as a tensor [V', W], a ``VertexBakedFeatures`` as a new module (same lobes,
    same ``train_density``).  Destination vertices that are the source's own get their rows back bit for bit.  A
    ``QuantisedVertexFeatures`` is refused with ``TypeError``: its records sit in a vertex texture laid out by V, so
    transfer the fp32 table and quantise after.  Raises ValueError, with their number, for destination vertices that are
    not finite or have no source triangle within ``max_distance`` (one host wait, for those counts)."""
    if isinstance(vertex_features, QuantisedVertexFeatures):
        raise TypeError("transfer_vertex_features: a QuantisedVertexFeatures cannot be transferred (its vertex texture is "
                        "laid out by V); transfer the fp32 table and quantise after")
    table = vertex_features.features() if isinstance(vertex_features, VertexBakedFeatures) else vertex_features
    if not isinstance(table, torch.Tensor) or table.dim() != 2:
        raise TypeError("vertex_features must be a [V, W] tensor or a VertexBakedFeatures")
    inter = getattr(src_mesh_intersect, "rayintersector", src_mesh_intersect)
    faces = np.asarray(inter.mesh.faces, dtype=np.int64)
    if table.shape[0] != inter.mesh.vertices.shape[0]:
        raise ValueError(f"vertex_features must have V = {inter.mesh.vertices.shape[0]} rows, got {tuple(table.shape)}")
    found = inter.closest_points(dst_vertices, max_distance)
    nonfinite, missed = found.counts.tolist()
    if nonfinite or missed:
        raise ValueError(f"transfer_vertex_features: {nonfinite} destination vertices are not finite and {missed} have no "
                         f"source triangle within {max_distance}")
    table = table.detach().to(device=inter.device, dtype=torch.float32)
    corners = torch.from_numpy(faces).to(inter.device)[found.tri]
    b = found.bary.to(torch.float32)
    out = b[:, 0:1] * table[corners[:, 0]] + b[:, 1:2] * table[corners[:, 1]] + b[:, 2:3] * table[corners[:, 2]]
    if isinstance(vertex_features, VertexBakedFeatures):
        return VertexBakedFeatures(out, train_density=vertex_features.train_density)
    return out


# ---- the vertex table fitted to the field over the surface (include/qf_vertex_fit.h) --------------

AXIS_DIRECTIONS = ((1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, -1.0))


def _clamp_mask(clamp_columns, n_columns: int) -> int:
    if clamp_columns is None:
        return 0
    if isinstance(clamp_columns, str):
        if clamp_columns != "all":
            raise ValueError(f"clamp_columns must be a sequence of column indices, None or 'all', got {clamp_columns!r}")
        return (1 << n_columns) - 1
    mask = 0
    for c in clamp_columns:
        c = int(c)
        if not -n_columns <= c < n_columns:
            raise IndexError(f"clamp column {c} is outside the table's {n_columns} columns")
        mask |= 1 << (c % n_columns)
    return mask


def _fit_table_of(prior, what: str):
    if isinstance(prior, QuantisedVertexFeatures):
        raise TypeError(f"{what}: a QuantisedVertexFeatures cannot be fitted (its records are uint8 codes in a vertex "
                        "texture); fit the fp32 table and quantise after")
    table = prior.table.detach() if isinstance(prior, VertexBakedFeatures) else prior
    if not isinstance(table, torch.Tensor) or table.dim() != 2:
        raise TypeError("the prior must be a [V, C] float32 tensor or a VertexBakedFeatures")
    if table.dtype != torch.float32:
        raise TypeError(f"the prior must be float32, got {table.dtype}")
    return table, (prior.width if isinstance(prior, VertexBakedFeatures) else int(table.shape[1]))


@torch.no_grad()
def fit_vertex_table_device(faces, n_vertices: int, sample_face, sample_bary, targets, prior, prior_weight: float = 1.0 / 64,
                            iterations: int = 32, clamp_columns=(-1,), return_stats: bool = False):
    """The vertex table that the renderer's piecewise-linear blend fits best, in the least-squares sense, to ``targets``
    given at surface samples, regularised towards ``prior`` (the rule is stated in
    ``include/qf_vertex_fit.h`` and restated in ``tests/vertex_fit_reference.py``).  With ``b_s`` the barycentrics of
    sample s in its face ``(f0, f1, f2)`` it minimises ``sum_s |y_s - (b_s0 X[f0] + b_s1 X[f1] + b_s2 X[f2])|^2 +
    prior_weight * sum_v d_v |X[v] - prior[v]|^2`` (``d_v``: the barycentric mass the samples give vertex v) by exactly
    ``iterations`` steps of Jacobi-preconditioned conjugate gradients in fp64 with fixed-order sums, every column on its
    own: the same bytes from run to run.  The eigenvalues of the preconditioned operator lie in
    ``[prior_weight, 1 + prior_weight]`` whatever the mesh, so the step count does not grow with it: at the default
    weight 32 steps cut the energy-norm error to 7e-4 of the start's at worst; measured relative residuals are 1e-13 on
    an icosphere and 4e-7 on the 983 040-face bench mesh (``return_stats`` hands back both norms per column).

    ``faces``: device int64 / int32 [F,3] over ``n_vertices`` vertices.  ``sample_face`` int64 [N] non-decreasing and
    ``sample_bary`` fp64 [N,3]: what ``mc_utils.sample_surface_device`` returns.  ``targets``: device float32 [N, C],
    1 <= C <= 64.  ``prior``: device float32 [V, C] (rows may be strided) or a ``VertexBakedFeatures``, whose table is
    read in place.  ``clamp_columns``: the columns (negative indices count from the end; ``None`` for none, ``"all"``)
    whose fitted entries are clamped to the range of the prior entry and the targets of the samples in the faces around
    the vertex; the default is the last column, the activated density, which ``alpha = 1 - exp(-sigma * step)`` must not
    see negative -- a least-squares fit overshoots where the field has a sharp edge.  Clamping every column gives back
    part of the gain.

    A vertex without a sample in any of its faces keeps its prior row bit for bit.  Faces with an index out of range or
    a repeated index take no part, and neither do their samples.  With fewer samples than faces the fit follows its
    samples too closely and is worse than the prior on fresh samples; 4 to 16 samples per face is the working range.  A
    vertex with hundreds of faces and a face with thousands of samples stay correct but are walked by one lane each.

    A tensor prior comes back as a float32 [V, C] tensor, a ``VertexBakedFeatures`` as a new module (same lobes, same
    ``train_density``).  With ``return_stats`` a dict comes second: the eight counts (``_C.VERTEX_FIT_COUNTS``) and, per
    column, ``rhs_norm`` and ``residual_norm`` (lists of C floats).  One host wait, for the counts.  Raises ValueError,
    naming the counts, when sample faces are out of range or decrease, or when a barycentric, target or prior entry is
    not finite; then nothing was solved."""
    table, n_c = _fit_table_of(prior, "fit_vertex_table_device")
    lam, steps = float(prior_weight), int(iterations)
    if not (lam >= 0.0 and math.isfinite(lam)):
        raise ValueError(f"prior_weight must be finite and >= 0, got {prior_weight!r}")
    if steps < 0:
        raise ValueError(f"iterations must be >= 0, got {iterations!r}")
    _, f, dev, n_v, n_f = mesh_inputs(None, faces, "fit_vertex_table_device", limit="3F", n_vertices=n_vertices)
    for name, t in (("sample_face", sample_face), ("sample_bary", sample_bary), ("targets", targets), ("prior", table)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
        if t.device != dev:
            raise ValueError(f"faces on {dev} and {name} on {t.device}")
    if sample_face.dim() != 1 or sample_face.dtype != torch.int64:
        raise ValueError(f"sample_face must be int64 [N], got {sample_face.dtype} {tuple(sample_face.shape)}")
    n = sample_face.shape[0]
    if tuple(sample_bary.shape) != (n, 3) or sample_bary.dtype != torch.float64:
        raise ValueError(f"sample_bary must be float64 [{n},3], got {sample_bary.dtype} {tuple(sample_bary.shape)}")
    if not 1 <= n_c <= _C.VERTEX_FIT_MAX_COLUMNS:
        raise ValueError(f"the table must have 1 to {_C.VERTEX_FIT_MAX_COLUMNS} columns, got {n_c}")
    if targets.dim() != 2 or tuple(targets.shape) != (n, n_c) or targets.dtype != torch.float32:
        raise ValueError(f"targets must be float32 [{n},{n_c}], got {targets.dtype} {tuple(targets.shape)}")
    if table.shape[0] != n_v or n_v < 1:
        raise ValueError(f"the prior must have V = {n_v} >= 1 rows, got {tuple(table.shape)}")
    if table.stride(1) != 1 or table.stride(0) < n_c:
        table = table.contiguous()
    mask = _clamp_mask(clamp_columns, n_c)
    sf, sb, y = sample_face.contiguous(), sample_bary.contiguous(), targets.contiguous()
    lib = _C.lib()
    with torch.cuda.device(dev):
        ws, ws_bytes = workspace("qf_vertex_fit_workspace_bytes", dev, ValueError, V=n_v, F=n_f, N=n, C=n_c)
        gram = torch.empty((n_f, 9), dtype=torch.float64, device=dev)
        mass = torch.empty((n_v,), dtype=torch.float64, device=dev)
        rhs = torch.empty((n_v, n_c), dtype=torch.float64, device=dev)
        counts = counts_buffer(_C.VERTEX_FIT_COUNTS, dev)
        norms = torch.empty((n_c, 2), dtype=torch.float64, device=dev)
        out = torch.empty((n_v, n_c), dtype=torch.float32, device=dev)
        x0 = ctypes.c_void_p(table.data_ptr())
        _C.check(lib.qf_vertex_fit_assemble(_C.ptr(f) if n_f else None, n_f, n_v, _C.ptr(sf) if n else None,
                                            _C.ptr(sb) if n else None, n, _C.ptr(y) if n else None, n_c, x0, table.stride(0),
                                            n_c, lam, _C.ptr(gram) if n_f else None, _C.ptr(mass), _C.ptr(rhs), _C.ptr(ws),
                                            ws_bytes, _C.ptr(counts), _C.stream()), "qf_vertex_fit_assemble")
        _C.check(lib.qf_vertex_fit_solve(_C.ptr(f) if n_f else None, n_f, n_v, x0, table.stride(0), n_c,
                                         _C.ptr(gram) if n_f else None, _C.ptr(mass), _C.ptr(rhs), steps, mask, _C.ptr(ws),
                                         ws_bytes, _C.ptr(out), n_c, _C.ptr(norms), _C.ptr(counts), _C.stream()),
                 "qf_vertex_fit_solve")
        stats = read_counts(_C.VERTEX_FIT_COUNTS, counts)                # the host wait
    if stats["refused"]:
        raise ValueError("fit_vertex_table_device: the input cannot be fitted: "
                         + ", ".join(f"{k}={stats[k]}" for k in _C.VERTEX_FIT_COUNTS[:3]))
    result = VertexBakedFeatures(out, train_density=prior.train_density) if isinstance(prior, VertexBakedFeatures) else out
    if return_stats:
        host = norms.tolist()
        stats["rhs_norm"] = [r[0] for r in host]
        stats["residual_norm"] = [r[1] for r in host]
        return result, stats
    return result


def _mesh_tensors(mesh, device):
    """fp64 vertices and int64 faces of a ``TriMesh`` (or anything with ``vertices`` and ``faces``) on ``device``."""
    return trimesh_tensors(getattr(mesh, "mesh", mesh), device)


@torch.no_grad()
def fit_vertex_features(radiance_field, mesh, samples_per_face: int = 8, n_samples: int = None, seed: int = 0,
                        face_weight=None, prior=None, prior_weight: float = 1.0 / 64, iterations: int = 32,
                        clamp_columns=(-1,), device="cuda", return_stats: bool = False):
    """The vertex-baked table fitted to the SG field over the surface of ``mesh`` instead of sampled at its vertices
    (DESIGN.md section 3.9i): ``n_samples`` (default ``samples_per_face * F``) area-stratified surface samples from
    ``mc_utils.sample_surface_device`` (``seed``, ``face_weight`` as there), the field's feature rows at their float32
    positions as targets, and ``fit_vertex_table_device`` with the remaining arguments.  ``prior``: a float32 [V, 3 + 7L +
    1] tensor or a ``VertexBakedFeatures`` (a fine-tuned or transferred table, say); by default the point bake, the
    field's features at the float32 vertices, which is also what a vertex no sample reaches keeps.  ``mesh``: a
    ``TriMesh`` or anything with ``vertices`` and ``faces``.  A tensor or no prior comes back as a tensor, a
    ``VertexBakedFeatures`` as a new module; a ``QuantisedVertexFeatures`` is refused with ``TypeError``.  Keep at least
    a few samples per face: with fewer samples than faces the fit is worse on fresh samples than the point bake."""
    from . import mc_utils
    if isinstance(prior, QuantisedVertexFeatures):
        _fit_table_of(prior, "fit_vertex_features")
    dev = _C.resolve_device(device) if prior is None else \
        (prior.table.device if isinstance(prior, VertexBakedFeatures) else prior.device)
    v, f = _mesh_tensors(mesh, dev)
    n = int(samples_per_face) * f.shape[0] if n_samples is None else int(n_samples)
    if n < 0:
        raise ValueError(f"the number of samples must be >= 0, got {n}")
    w = None if face_weight is None else torch.as_tensor(np.asarray(face_weight, dtype=np.float64)
                                                        if not isinstance(face_weight, torch.Tensor) else face_weight).to(dev)
    samples = mc_utils.sample_surface_device(v, f, n, seed, face_weight=w)
    targets = _field_features(radiance_field, samples.points.to(torch.float32))
    if prior is None:
        prior = _field_features(radiance_field, v.to(torch.float32))
    return fit_vertex_table_device(f, v.shape[0], samples.face, samples.bary, targets, prior, prior_weight, iterations,
                                   clamp_columns, return_stats)


@torch.no_grad()
def vertex_surface_error(radiance_field, mesh, table, n_samples: int, seed: int = 0, render_step_size: float = 0.005,
                         dirs=None, device="cuda"):
    """How far a vertex table is from the field over the whole surface, not only at edge midpoints: at ``n_samples``
    area-stratified surface samples (``mc_utils.sample_surface_device`` with ``seed``) the field's features ``f_m`` at the
    float32 point against the blend ``f_i = b0 row[f0] + b1 row[f1] + b2 row[f2]`` the renderer draws there, scored by
    ``vertex_edge_error``'s ``e`` (composited-pixel units; ``dirs`` and ``render_step_size`` as there).  Returns a dict:
    ``mean``, ``rms`` and ``max`` of ``e`` and ``feature_rms``, the RMS of ``f_i - f_m`` per column (a list).  Torch
    operations: the field evaluation dominates.  One host wait."""
    from . import mc_utils
    t = table.features() if isinstance(table, VertexBakedFeatures) else table
    if isinstance(table, QuantisedVertexFeatures) or not isinstance(t, torch.Tensor) or t.dim() != 2:
        raise TypeError("table must be a [V, W] tensor or a VertexBakedFeatures")
    dev = t.device
    v, f = _mesh_tensors(mesh, dev)
    if t.shape[0] != v.shape[0]:
        raise ValueError(f"the table has {t.shape[0]} rows for {v.shape[0]} vertices")
    samples = mc_utils.sample_surface_device(v, f, int(n_samples), seed)
    f_m = _field_features(radiance_field, samples.points.to(torch.float32))
    tri, b = f[samples.face], samples.bary.to(torch.float32)
    t = t.detach().to(torch.float32)
    f_i = b[:, 0:1] * t[tri[:, 0]] + b[:, 1:2] * t[tri[:, 1]] + b[:, 2:3] * t[tri[:, 2]]
    step = float(render_step_size)
    alpha_m = 1.0 - torch.exp(-f_m[:, -1] * step)
    alpha_i = 1.0 - torch.exp(-f_i[:, -1] * step)
    d_all = torch.tensor(AXIS_DIRECTIONS, dtype=torch.float32, device=dev) if dirs is None else _C.f32c(torch.as_tensor(dirs)).to(dev)
    if d_all.dim() != 2 or d_all.shape[1] != 3 or d_all.shape[0] < 1:
        raise ValueError(f"dirs must be [D,3] with D >= 1, got {tuple(d_all.shape)}")
    colour = torch.zeros_like(alpha_m)
    for d in d_all:
        dd = d.expand(f_m.shape[0], 3).contiguous()
        diff = (radiance_field.features_to_rgb(f_m, dd) - radiance_field.features_to_rgb(f_i, dd)).abs().max(dim=1).values
        colour = torch.maximum(colour, diff)
    e = torch.maximum((alpha_m - alpha_i).abs(), torch.maximum(alpha_m, alpha_i) * colour).to(torch.float64)
    feat = ((f_i - f_m).to(torch.float64) ** 2).mean(dim=0).sqrt()
    return {"mean": float(e.mean()), "rms": float((e * e).mean().sqrt()), "max": float(e.max()),
            "feature_rms": feat.tolist()}


# ---- refining the vertex-baked asset -------------------------------------------------------------

RefinedVertexBaked = namedtuple("RefinedVertexBaked", ["mesh", "table", "face_map", "vertex_parents", "levels"])


@torch.no_grad()
def _field_features(radiance_field, positions: torch.Tensor, batch_size: int = 1000000) -> torch.Tensor:
    """``radiance_field.features`` at float32 positions, in the chunks of ``bake_vertex_features``."""
    from .radiance_fields.ngp import NGPRadianceFieldSGNew
    if not isinstance(radiance_field, NGPRadianceFieldSGNew):
        raise NotImplementedError("the vertex table holds the SG features of an NGPRadianceFieldSGNew")
    x = _C.f32c(positions)
    out = torch.empty((x.shape[0], 3 + 7 * radiance_field.num_g_lobes + 1), dtype=torch.float32, device=x.device)
    for b in range(0, x.shape[0], int(batch_size)):
        out[b:b + batch_size] = radiance_field.features(x[b:b + batch_size])
    return out


@torch.no_grad()
def subdivide_vertex_features(vertex_features, vertex_parents, radiance_field=None, vertices=None):
    """The per-vertex table of a refined mesh (``mc_utils.subdivide_mesh_device`` / ``subdivide_mesh``): the old rows
    copied bit for bit, one new row per row ``vertex_parents`` (int64 [V',2], array or tensor) adds.  Without a field a
    new row is ``(row[a] + row[b]) * 0.5`` in fp32 over its two parents -- the function the renderer interpolates is then
    what it was, which is how a fine-tuned ``VertexBakedFeatures`` is carried along; parents that are themselves new rows
    (maps chained over several levels) are resolved level by level.  With ``radiance_field`` a new row is the field's own
    ``features`` at the new vertex, float32 of ``vertices`` (the refined mesh's, [V',3], required then).  A tensor [V, W]
    comes back as a tensor [V', W], a ``VertexBakedFeatures`` as a new module (same lobes, same ``train_density``, same
    device).  Device-agnostic without a field.  A ``QuantisedVertexFeatures`` is refused with ``TypeError``: its records
    sit in a vertex texture laid out by V, so quantise after refining."""
    if isinstance(vertex_features, QuantisedVertexFeatures):
        raise TypeError("subdivide_vertex_features: a QuantisedVertexFeatures cannot be refined (its vertex texture is laid "
                        "out by V); refine the fp32 table and quantise after refining")
    module = vertex_features if isinstance(vertex_features, VertexBakedFeatures) else None
    table = module.features() if module is not None else vertex_features
    if not isinstance(table, torch.Tensor) or table.dim() != 2 or not table.is_floating_point():
        raise TypeError("vertex_features must be a floating-point [V, W] tensor or a VertexBakedFeatures")
    par = torch.as_tensor(np.asarray(vertex_parents) if not isinstance(vertex_parents, torch.Tensor) else vertex_parents)
    if par.dim() != 2 or par.shape[1] != 2 or par.dtype not in (torch.int64, torch.int32):
        raise ValueError(f"vertex_parents must be an int64 [V',2] array, got {par.dtype} {tuple(par.shape)}")
    par = par.to(device=table.device, dtype=torch.int64)
    n_old, n_new = table.shape[0], par.shape[0]
    if n_new < n_old:
        raise ValueError(f"vertex_parents has {n_new} rows for a table of {n_old}")
    own = torch.arange(n_old, device=table.device)
    if not bool(((par[:n_old, 0] == own) & (par[:n_old, 1] == own)).all()):
        raise ValueError(f"the first {n_old} rows of vertex_parents must be (v, v): the vertices the table already has")
    if n_new > n_old and (int(par[n_old:].min()) < 0 or int(par[n_old:].max()) >= n_new):
        raise IndexError(f"vertex_parents reaches outside its own {n_new} rows")
    out = torch.empty((n_new, table.shape[1]), dtype=table.dtype, device=table.device)
    out[:n_old] = table
    if radiance_field is not None:
        if vertices is None or tuple(vertices.shape) != (n_new, 3):
            raise ValueError(f"with a field, vertices must be the refined mesh's [{n_new}, 3] positions")
        if table.dtype != torch.float32:
            raise TypeError(f"with a field the table must be float32, got {table.dtype}")
        pos = torch.as_tensor(vertices)[n_old:].to(device=table.device, dtype=torch.float32)
        feats = _field_features(radiance_field, pos)
        if feats.shape[1] != table.shape[1]:
            raise ValueError(f"the field has {feats.shape[1]} features per point, the table {table.shape[1]} columns")
        out[n_old:] = feats
    else:
        start = n_old
        while start < n_new:                    # one level per pass: its rows' parents all lie below `start`
            ready = (par[start:].max(dim=1).values < start).to(torch.int64)
            n_level = int(torch.cumprod(ready, dim=0).sum())
            if n_level == 0:
                raise ValueError(f"vertex_parents row {start} names a vertex that is not above it: not a chain of levels")
            a, b = par[start:start + n_level, 0], par[start:start + n_level, 1]
            out[start:start + n_level] = (out[a] + out[b]) * 0.5
            start += n_level
    if module is not None:
        return VertexBakedFeatures(out, train_density=module.train_density)
    return out


@torch.no_grad()
def vertex_edge_error(radiance_field, vertices, edges, table, render_step_size: float, dirs=None,
                      return_midpoint_features: bool = False):
    """How far the vertex table is from the field at the midpoint of every edge, in the units of a composited pixel:
    float32 [E] on the device.  With ``f_m`` the field's features at the midpoint ``0.5 * (p[a] + p[b])`` (in the
    vertices' precision, then float32: the position a split would create) and ``f_i = (table[a] + table[b]) * 0.5`` (what
    the renderer interpolates there), ``alpha(f) = 1 - exp(-sigma(f) * render_step_size)`` and

        e = max(|alpha(f_m) - alpha(f_i)|,  max(alpha(f_m), alpha(f_i)) * max_d max_c |rgb(f_m, d) - rgb(f_i, d)|_c),

    ``d`` over ``dirs`` ([D,3] unit vectors; the six axis directions by default).  Built from ``radiance_field.features``
    and ``features_to_rgb``.  ``return_midpoint_features``: also ``f_m`` [E, W], which is the new row of every edge a
    refinement splits."""
    v = torch.as_tensor(vertices)
    e = torch.as_tensor(edges)
    if v.dim() != 2 or v.shape[1] != 3 or e.dim() != 2 or e.shape[1] != 2:
        raise ValueError(f"vertices must be [V,3] and edges [E,2], got {tuple(v.shape)} and {tuple(e.shape)}")
    t = table.features() if isinstance(table, VertexBakedFeatures) else table
    if t.shape[0] != v.shape[0]:
        raise ValueError(f"the table has {t.shape[0]} rows for {v.shape[0]} vertices")
    dev = t.device
    v, e = v.to(dev), e.to(device=dev, dtype=torch.int64)
    a, b = e[:, 0], e[:, 1]
    mid = (0.5 * (v[a] + v[b])).to(torch.float32)
    f_m = _field_features(radiance_field, mid)
    f_i = ((t[a] + t[b]) * 0.5).to(torch.float32)
    step = float(render_step_size)
    alpha_m = 1.0 - torch.exp(-f_m[:, -1] * step)
    alpha_i = 1.0 - torch.exp(-f_i[:, -1] * step)
    d_all = torch.tensor(AXIS_DIRECTIONS, dtype=torch.float32, device=dev) if dirs is None else _C.f32c(torch.as_tensor(dirs)).to(dev)
    if d_all.dim() != 2 or d_all.shape[1] != 3 or d_all.shape[0] < 1:
        raise ValueError(f"dirs must be [D,3] with D >= 1, got {tuple(d_all.shape)}")
    colour = torch.zeros_like(alpha_m)
    for d in d_all:
        dd = d.expand(e.shape[0], 3).contiguous()
        diff = (radiance_field.features_to_rgb(f_m, dd) - radiance_field.features_to_rgb(f_i, dd)).abs().max(dim=1).values
        colour = torch.maximum(colour, diff)
    err = torch.maximum((alpha_m - alpha_i).abs(), torch.maximum(alpha_m, alpha_i) * colour)
    return (err, f_m) if return_midpoint_features else err


@torch.no_grad()
def refine_vertex_baked(mesh: TriMesh, radiance_field, tol: float, max_levels: int = 3, max_vertices: int = None,
                        render_step_size: float = 0.005, device="cuda", uniform: bool = False,
                        keep_level_arrays: bool = False) -> RefinedVertexBaked:
    """Refine a mesh where its vertex-baked table is too coarse for the field.  Per level: the edges of the current mesh
    (``mc_utils.mesh_edges_device``), ``vertex_edge_error`` of the current table, the edges with ``e > tol`` marked, the
    conforming split (``mc_utils.subdivide_mesh_device``).  The table is baked once, on the input mesh; afterwards the
    field is evaluated at edge midpoints only, and the row of a new vertex is the midpoint's features the error pass
    already has (the same float32 position, so the same bits as ``bake_vertex_features`` of the refined mesh).  With
    ``max_vertices`` a level marks at most ``max_vertices - V`` edges, the largest errors first (ties: the lower edge id).
    Stops after ``max_levels`` levels or at the first level that marks nothing.  ``uniform``: every edge is marked,
    whatever its error (``tol`` is still reported against).

    Returns ``RefinedVertexBaked(mesh, table, face_map, vertex_parents, levels)``: the refined ``TriMesh`` (fp64
    vertices; a midpoint split does not move the surface), the float32 [V', W] device table, numpy maps composed over the
    levels as ``mc_utils.subdivide_mesh`` composes them, and one dict per level (vertices, faces and edges before the
    split, marked edges, edges above ``tol``, the largest and the mean error; with ``keep_level_arrays`` also the device
    tensors ``edges``, ``errors`` and ``marks``)."""
    from . import mc_utils
    dev = _C.resolve_device(device)
    v, f = trimesh_tensors(mesh, dev)
    if max_vertices is not None and int(max_vertices) < v.shape[0]:
        raise ValueError(f"max_vertices = {max_vertices} is below the mesh's {v.shape[0]} vertices")
    table = _field_features(radiance_field, v.to(torch.float32))
    n_f0 = f.shape[0]
    face_map = torch.arange(n_f0, dtype=torch.int64, device=dev)
    parents = torch.arange(v.shape[0], dtype=torch.int64, device=dev)[:, None].repeat(1, 2)
    levels = []
    for level in range(int(max_levels)):
        edges, face_edges, _ = mc_utils.mesh_edges_device(f, v.shape[0])
        err, f_m = vertex_edge_error(radiance_field, v, edges, table, render_step_size, return_midpoint_features=True)
        above = err > float(tol)
        mark = torch.ones_like(above) if uniform else above
        if max_vertices is not None and int(mark.sum()) > int(max_vertices) - v.shape[0]:
            room = int(max_vertices) - v.shape[0]
            order = torch.sort(torch.where(mark, err, torch.full_like(err, -1.0)), descending=True, stable=True).indices
            mark = torch.zeros_like(mark)
            mark[order[:room]] = True
        n_mark = int(mark.sum())
        record = dict(level=level, vertices=v.shape[0], faces=f.shape[0], edges=edges.shape[0], marked=n_mark,
                      above_tol=int(above.sum()), max_error=float(err.max()) if err.numel() else 0.0,
                      mean_error=float(err.mean()) if err.numel() else 0.0)
        if keep_level_arrays:
            record.update(edges_tensor=edges, errors=err, marks=mark)
        levels.append(record)
        if n_mark == 0:
            break
        out = mc_utils.subdivide_mesh_device(v, f, mark, edges, face_edges)
        table = torch.cat([table, f_m[mark]])
        v, f = out.vertices, out.faces
        face_map = face_map[out.face_map]
        parents = mc_utils.chain_vertex_parents(parents, out.vertex_parents)
    return RefinedVertexBaked(TriMesh(*to_numpy(v, f), None), table, *to_numpy(face_map, parents), levels)
