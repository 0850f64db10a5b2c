"""Draw points uniformly by area from the surface of a mesh on the GPU (a rule of this project's
own; the reference's ``sample_points_on_triangle`` is a stub).

    python examples/sample_surface.py MESH.{ply,obj} OUT.npz [--n N] [--seed S] [--face_weights W.npy]

Writes OUT.npz with ``points`` fp64 [N,3], ``face`` int64 [N] (non-decreasing) and ``bary`` fp64 [N,3], and prints the
counts as one JSON line.  The faces are laid end to end by area and sample ``i`` falls in the ``i``-th of ``N`` equal
strata, so every face gets its share of the samples to within 2; the same seed gives the same bytes.  With
``--face_weights`` (fp [F], non-negative: ``MeshPruner``'s per-triangle render weights, for one) a face's share is its
area times its weight; a weight of zero keeps a face from being sampled."""
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
    ap.add_argument("out_npz")
    ap.add_argument("--n", type=int, default=65536, metavar="N")
    ap.add_argument("--seed", type=int, default=0, metavar="S")
    ap.add_argument("--face_weights", default=None, metavar="W.npy", help="per-face weights [F] (.npy)")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    from quadraturefields_amd import mc_utils
    from quadraturefields_amd.mesh_io import load_mesh
    mesh = load_mesh(args.mesh_in)
    weights = None if args.face_weights is None else np.load(args.face_weights)
    out, stats = mc_utils.sample_surface(mesh, args.n, seed=args.seed, face_weight=weights, device=args.device,
                                         return_stats=True)
    np.savez(args.out_npz, points=out.points, face=out.face, bary=out.bary)
    print(json.dumps(dict(stats, samples=int(out.face.shape[0]), seed=args.seed, weighted=weights is not None,
                          vertices_in=int(mesh.vertices.shape[0]), faces_in=int(mesh.faces.shape[0]),
                          faces_sampled=int(np.unique(out.face).shape[0]))))


if __name__ == "__main__":
    main()
