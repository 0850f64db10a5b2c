"""The UV stage of the reference (examples/generate_uv_xatlas_old.py) with its five positional arguments:

    python examples/generate_uv_atlas.py ROOT MESH_NAME LABELS_NAME TEXTURE_SIZE CONTRACTION

It reads ROOT/MESH_NAME (.ply or .obj), gives every face its own chart of a TEXTURE_SIZE^2 atlas on the device
(quadraturefields_amd.uv_atlas.per_triangle_atlas) and writes, into ROOT/<mesh stem>/,
``mesh_segmentation_{TEXTURE_SIZE}.obj`` (the unshared mesh with its UVs) and ``V_{TEXTURE_SIZE}.npy`` (the
texel-position map of baking.texel_positions; float16 above 8192, as the reference saves it).

The reference segments the mesh with the ScanNet segmentator and charts the segments with xatlas; here there is no
segmentation step, so LABELS_NAME is accepted and unused.  CONTRACTION=True (unbounded scenes) is out of scope.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np


def str2bool(v):
    return v.lower() in ("yes", "true", "t", "1")


def main(argv):
    if len(argv) != 5:
        sys.exit(__doc__)
    root_path, mesh_name, _labels_name, texture_size, contraction = argv[0], argv[1], argv[2], int(argv[3]), str2bool(argv[4])
    if contraction:
        sys.exit("generate_uv_atlas.py: CONTRACTION=True (the contracted space of unbounded scenes) is not supported")
    from quadraturefields_amd import baking, uv_atlas
    from quadraturefields_amd.mesh_io import load_mesh

    mesh = load_mesh(os.path.join(root_path, mesh_name))
    print("mesh:", np.shape(mesh.vertices), np.shape(mesh.faces))
    mesh_uv, info = uv_atlas.per_triangle_atlas(mesh, texture_size)
    print(f"atlas: {info.rho:.6g} texels per unit, {info.rows_used} of {texture_size - 1} rows, "
          f"{info.texels_used} texels ({info.texels_used / texture_size ** 2:.1%} of the atlas)")
    out_dir = os.path.join(root_path, os.path.splitext(mesh_name)[0])
    os.makedirs(out_dir, exist_ok=True)
    mesh_uv.export_obj(os.path.join(out_dir, f"mesh_segmentation_{texture_size}.obj"))
    V, _ = baking.texel_positions(mesh_uv, texture_size)
    V = V.cpu().numpy()
    np.save(os.path.join(out_dir, f"V_{texture_size}.npy"), V.astype(np.float16 if texture_size > 8192 else np.float32))


if __name__ == "__main__":
    main(sys.argv[1:])
