"""The mesh extraction stage of the reference (examples/marching_cubes.py) with its nine positional arguments:

    python examples/extract_mesh.py ROOT SIGMA INCLUDE_GRAD OMEGA THRES AXIS COMBINE GRAD_THRES DENSITY_THRES

It reads what the field training saved under ROOT (``grids_valid.npy``, ``grads_valid.npy``, ``binaries.npy`` and, with
COMBINE=True, ``density_grids_valid.npy``) and writes ``mesh_nerf.ply`` (COMBINE=True) and ``mesh.ply``: the quadrature
surfaces of ``sin(OMEGA * q)`` at THRES followed by the density mesh at DENSITY_THRES.  AXIS is accepted and unused, as
in the reference.  With COMBINE=False, ``mesh.ply`` holds the quadrature surfaces alone (the reference would load a
``mesh_nerf.ply`` left by an earlier run).  Marching cubes runs on the device (quadraturefields_amd.mc_utils).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np


def main(argv):
    if len(argv) != 9:
        sys.exit(__doc__)
    root, sigma, include_grad, omega, thres, _axis, combine, grad_thres, density_thres = argv
    from quadraturefields_amd import mc_utils

    grid = np.load(root + "grids_valid.npy")
    grads = np.load(root + "grads_valid.npy")
    binaries = np.load(root + "binaries.npy")
    mesh = mc_utils.quadrature_surface_mesh(grid, grads, binaries, sigma=float(sigma), include_grad=include_grad == "True",
                                            omega=float(omega), thres=float(thres), grad_thres=float(grad_thres))
    del grid, grads, binaries
    print("Quadrature mesh: Faces", mesh.faces.shape, "Vertices:", mesh.vertices.shape)
    if combine == "True":
        nerf = mc_utils.density_surface_mesh(np.load(root + "density_grids_valid.npy"), float(density_thres))
        print("Density mesh: Faces", nerf.faces.shape, "Vertices:", nerf.vertices.shape)
        nerf.export(os.path.join(root, "mesh_nerf.ply"))
        mesh = mc_utils.combined_mesh(mesh, nerf)
    mesh.export(os.path.join(root, "mesh.ply"))
    print("Combined mesh: Faces", mesh.faces.shape, "Vertices:", mesh.vertices.shape)


if __name__ == "__main__":
    main(sys.argv[1:])
