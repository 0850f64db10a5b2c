"""The reference's ``examples/parameterization_utils.py`` names over the device path.

Only the fill of the UV stage is in scope: ``fill_triangles_fill_boundary`` turns a UV-mapped mesh into the texel-position
map ``V`` that ``bake_texture_images`` consumes, computed on the device by ``baking.texel_positions``.  The chart
generation before it (xatlas) stays offline tooling.  ``fill_triangles`` and ``sample_points_on_triangle`` exist so that
``bake_texture_images_shelly.py``'s imports resolve; no in-scope stage calls them, and they raise.
"""
import numpy as np

from .baking import texel_positions
from .mesh_io import TriMesh


def fill_triangles_fill_boundary(mesh, HEIGHT, WIDTH):
    """``(V, tri_size)``: V numpy float32 [HEIGHT, WIDTH, 3], tri_size a list of per-face texel counts -- the reference's
    return values, computed on the device (``baking.texel_positions`` with untouched="last_face")."""
    V, tri_size = texel_positions(mesh, HEIGHT, WIDTH, untouched="last_face")
    return V.cpu().numpy(), tri_size.cpu().tolist()


def concatenate_meshes(meshes):
    """One ``TriMesh`` of ``meshes`` (vertices stacked, faces offset, per-vertex UVs stacked)."""
    vertices, faces, uvs, base = [], [], [], 0
    for m in meshes:
        vertices.append(np.asarray(m.vertices, dtype=np.float64))
        faces.append(np.asarray(m.faces, dtype=np.int64) + base)
        uvs.append(m.visual.uv)
        base += len(m.vertices)
    uv = None if any(u is None for u in uvs) else np.concatenate(uvs)
    return TriMesh(np.concatenate(vertices), np.concatenate(faces), uv)


def fill_triangles(mesh, SIZE=8192):
    raise NotImplementedError("fill_triangles (the fill without edge pixels) is not part of the device path: no in-scope "
                              "stage calls it; use fill_triangles_fill_boundary")


def sample_points_on_triangle(indices, mesh, n, uv):
    raise NotImplementedError("sample_points_on_triangle is not part of the device path: no in-scope stage calls it "
                              "(bake_texture_images_shelly.py imports it and leaves it unused)")
