"""``from parameterization_utils import sample_points_on_triangle, fill_triangles`` (bake_texture_images_shelly.py:33-34),
``fill_triangles_fill_boundary`` (generate_uv_xatlas_old.py:133)."""
from quadraturefields_amd.parameterization_utils import (concatenate_meshes, fill_triangles,  # noqa: F401
                                                         fill_triangles_fill_boundary, sample_points_on_triangle)
