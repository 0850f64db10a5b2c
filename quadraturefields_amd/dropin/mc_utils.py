"""``from mc_utils import prunning_mesh_train_visibility`` (examples/mc_utils.py): the helpers that have a device
counterpart.  ``clean_mesh`` and ``down_sample_quadraic`` decimate under this project's own rules (DESIGN.md section
3.9d; parity with fast_simplification is unpinned); open3d's non-manifold-edge removal in ``clean_mesh`` has none."""
from quadraturefields_amd.mc_utils import (clean_mesh, compact_mesh, down_sample_quadraic, downsample_mesh,  # noqa: F401
                                           prunning_mesh_train_visibility, prunning_mesh_train_visibility_complement)
