"""Weld the vertices of a mesh by position on the GPU (a rule of this project's own, parity with
trimesh's ``merge_vertices`` is unpinned).

    python examples/weld_mesh.py IN.{ply,obj} OUT.{ply,obj} [--tolerance H] [--compact]

With ``--tolerance 0`` (the default) vertices whose coordinates compare equal become one vertex: an unshared mesh such as
``mesh_segmentation_*.obj`` becomes an indexed one again and every triangle stays where it is.  With ``H > 0`` vertices
within ``H`` of one another do, transitively; a class keeps the position of its lowest vertex, so the surface moves by at
most a class's diameter.  No face is dropped: faces that become degenerate stay and are counted, unless ``--compact``
then removes degenerate and duplicate faces and the vertices nothing uses.  Per-vertex UVs
follow the lowest vertex of a class: welding an atlas mesh discards the atlas.

Writes OUT and, beside it, ``weld_vertex_map.npy`` (the input vertex every output vertex is) and
``weld_vertex_class.npy`` (the output vertex of every input vertex; -1 after ``--compact`` where nothing uses it), with
``--compact`` also ``weld_face_map.npy`` (the input face of every output face), and prints the counts as one JSON
line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("mesh_in")
    ap.add_argument("mesh_out")
    ap.add_argument("--tolerance", type=float, default=0.0, metavar="H")
    ap.add_argument("--compact", action="store_true",
                    help="then drop degenerate and duplicate faces and unreferenced vertices (writes weld_face_map.npy)")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    from quadraturefields_amd import mc_utils
    from quadraturefields_amd.mesh_io import load_mesh
    if not (args.tolerance >= 0.0 and np.isfinite(args.tolerance)):
        ap.error("--tolerance must be finite and >= 0")
    mesh = load_mesh(args.mesh_in)
    res = mc_utils.weld_vertices(mesh, args.tolerance, device=args.device, return_stats=True, compact=args.compact)
    out, stats = res[0], res[-1]
    vertex_map, vertex_class = res[-3], res[-2]
    if args.mesh_out.lower().endswith(".obj"):
        out.export_obj(args.mesh_out)
    else:
        out.export(args.mesh_out)
    folder = os.path.dirname(os.path.abspath(args.mesh_out))
    np.save(os.path.join(folder, "weld_vertex_map.npy"), vertex_map)
    np.save(os.path.join(folder, "weld_vertex_class.npy"), vertex_class)
    if args.compact:
        np.save(os.path.join(folder, "weld_face_map.npy"), res[1])
    print(json.dumps(dict(stats, tolerance=args.tolerance, compact=args.compact, vertices_in=int(mesh.vertices.shape[0]),
                          faces_in=int(mesh.faces.shape[0]), vertices_out=int(out.vertices.shape[0]),
                          faces_out=int(out.faces.shape[0]))))


if __name__ == "__main__":
    main()
