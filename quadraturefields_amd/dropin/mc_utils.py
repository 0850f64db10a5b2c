"""``from mc_utils import prunning_mesh_train_visibility`` (examples/mc_utils.py): the helpers that have a device
counterpart; the reference's ``clean_mesh`` (fast_simplification, open3d) has none."""
from quadraturefields_amd.mc_utils import (compact_mesh, downsample_mesh, prunning_mesh_train_visibility,  # noqa: F401
                                           prunning_mesh_train_visibility_complement)
