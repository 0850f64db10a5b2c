"""The mesh simplification step of the reference (examples/downsample_mesh.py) with its two positional arguments:

    python examples/downsample_mesh.py MESH_PATH VOXEL_SIZE

It reads MESH_PATH (.ply or .obj), clusters its vertices on the device with quadric contraction at voxel size
1 / VOXEL_SIZE (quadraturefields_amd.mc_utils.downsample_mesh), prints the shapes before and
after, and writes ``smp_{name}.ply`` next to the input.  VOXEL_SIZE is an integer, as in the reference (150, or 300 for
the shelly scenes).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np


def main(argv):
    if len(argv) != 2:
        sys.exit(__doc__)
    mesh_path, voxel_size = argv[0], int(argv[1])
    from quadraturefields_amd import mc_utils
    from quadraturefields_amd.mesh_io import load_mesh

    name = os.path.splitext(os.path.basename(mesh_path))[0]
    mesh = load_mesh(mesh_path)
    print("Before mesh simplification: ", np.shape(mesh.vertices), np.shape(mesh.faces))
    mesh = mc_utils.downsample_mesh(mesh, voxel_size)
    print("After mesh simplification: ", np.shape(mesh.vertices), np.shape(mesh.faces))
    mesh.export(os.path.join(os.path.dirname(os.path.abspath(mesh_path)), f"smp_{name}.ply"))


if __name__ == "__main__":
    main(sys.argv[1:])
