"""Decimate a mesh to a face count on the GPU (rounds of independent quadric edge collapses; the
rules are this project's own, parity with the reference's fast_simplification is unpinned).

    python examples/decimate_mesh.py IN.ply OUT.ply (--target_faces N | --ratio R) [--max_cost C] [--max_rounds K]
                                                [--boundary {lock,collapse}] [--boundary_weight W] [--make_manifold] [--weld H]
                                                [--vertex_features IN.npy --out_vertex_features OUT.npy]
                                                [--distance_samples N]

Writes OUT.ply and, beside it, ``face_map.npy`` (the source face of every output face) and ``vertex_target.npy`` (the
output vertex every input vertex ended in, -1 if it was dropped), and prints the stats as one JSON line.  With the default
``--boundary lock`` boundary and non-manifold edges are never collapsed, so an open mesh keeps its border and the fine
triangles along it; ``--boundary collapse`` adds boundary quadrics (weight ``--boundary_weight``) and collapses along the
border too, so an open mesh reaches its target.  Non-manifold edges are never collapsed, and bow-tie vertices never move:
``--make_manifold`` first cuts the mesh along its non-manifold edges and splits every vertex into one copy per fan
(no face is dropped, no coordinate changes), decimates the cut mesh and also writes
``cut_vertex_map.npy`` (the input vertex of every vertex of the cut mesh); ``vertex_target.npy`` then refers to the cut
mesh's vertices, and the JSON line gains ``cut_vertices_added``, ``cut_split_vertices`` and ``cut_complex_edges``.

``--vertex_features IN.npy --out_vertex_features OUT.npy`` carries a vertex-baked table [V, W] of the input mesh to the
output mesh (``baking.transfer_vertex_features``, DESIGN.md section 3.9f: every output vertex takes the input table
blended at its closest point on the INPUT surface -- the uncut input, also with ``--make_manifold``, so no
``cut_vertex_map`` is needed).  With these flags the JSON line gains the measured surface
distances ``distance_out_to_in_mean`` / ``_max`` and ``distance_in_to_out_mean`` / ``_max`` (``mc_utils.mesh_distance``).
Without them the files and the line are what they were.

``--weld H`` welds the decimated mesh last (vertices at the same place, or with ``H > 0`` within
``H`` of one another, become the lowest of them; no face is dropped).  ``--weld 0`` re-joins exactly the copies
``--make_manifold`` made that did not move apart since: all of them after ``--boundary lock``, while copies that
``--boundary collapse`` moved stay apart unless ``H`` reaches them, at the cost of moving the surface by up to a class's
diameter.  It also writes ``weld_vertex_map.npy`` (the vertex of the decimated mesh every output vertex is) and
``weld_vertex_class.npy`` (the output vertex of every vertex of the decimated mesh; ``vertex_target.npy`` still refers to
the decimated mesh before the weld), the JSON line gains ``weld_tolerance``, ``weld_vertices_removed``,
``weld_merged_classes``, ``weld_largest_class`` and ``weld_collapsed_faces``, and a transferred table goes through
``baking.weld_vertex_features(..., "first")``.  Without the flag nothing changes.

``--distance_samples N`` measures the distance between the output and the input mesh at ``N`` points drawn uniformly by
area from each (``mc_utils.mesh_distance(..., samples=N)``, DESIGN.md section 3.9h: mean and RMS over the surface, not
over the tessellation) and adds ``distance_samples``, ``distance_sampled_out_to_in_mean`` / ``_rms`` / ``_max`` and
``distance_sampled_in_to_out_mean`` / ``_rms`` / ``_max`` to the JSON line.  Without the flag nothing changes."""
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
    goal = ap.add_mutually_exclusive_group(required=True)
    goal.add_argument("--target_faces", type=int)
    goal.add_argument("--ratio", type=float, help="target = floor(ratio * F)")
    ap.add_argument("--max_cost", type=float, default=None)
    ap.add_argument("--max_rounds", type=int, default=128)
    ap.add_argument("--boundary", choices=("lock", "collapse"), default="lock")
    ap.add_argument("--boundary_weight", type=float, default=1.0,
                    help="weight of a boundary edge's plane in the quadrics of its ends (collapse mode)")
    ap.add_argument("--make_manifold", action="store_true",
                    help="cut non-manifold edges and split bow-tie vertices first (writes cut_vertex_map.npy)")
    ap.add_argument("--weld", type=float, default=None, metavar="H",
                    help="weld the decimated mesh at this tolerance last (writes weld_vertex_map.npy, weld_vertex_class.npy)")
    ap.add_argument("--vertex_features", default=None, help="vertex-baked table [V, W] (.npy) of the input mesh")
    ap.add_argument("--out_vertex_features", default=None, help="where the table transferred to the output mesh goes")
    ap.add_argument("--distance_samples", type=int, default=None, metavar="N",
                    help="also measure the output-to-input distance at N area-weighted surface samples per mesh")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    from quadraturefields_amd import mc_utils
    from quadraturefields_amd.mesh_io import load_mesh
    if (args.vertex_features is None) != (args.out_vertex_features is None):
        ap.error("--vertex_features and --out_vertex_features go together")
    mesh = load_mesh(args.mesh_in)
    source = mesh
    n_f = mesh.faces.shape[0]
    if args.ratio is not None and not 0.0 <= args.ratio <= 1.0:
        ap.error("--ratio must lie in [0, 1]")
    target = args.target_faces if args.target_faces is not None else int(args.ratio * n_f)
    n_v, cut = int(mesh.vertices.shape[0]), {}
    if args.make_manifold:
        mesh, cut_vertex_map, cut_stats = mc_utils.make_manifold(mesh, device=args.device, return_stats=True)
        cut = dict(cut_vertices_added=cut_stats["vertices"] - n_v, cut_split_vertices=cut_stats["split_vertices"],
                   cut_complex_edges=cut_stats["complex_edges"])
    out, face_map, vertex_target, stats = mc_utils.decimate_mesh(mesh, target, max_cost=args.max_cost,
                                                                 max_rounds=args.max_rounds, return_stats=True,
                                                                 device=args.device, boundary=args.boundary,
                                                                 boundary_weight=args.boundary_weight)
    decimated = out
    if args.weld is not None:
        out, weld_vertex_map, weld_vertex_class, weld_stats = mc_utils.weld_vertices(out, args.weld, device=args.device,
                                                                                     return_stats=True)
        cut = dict(cut, weld_tolerance=args.weld, weld_vertices_removed=int(decimated.vertices.shape[0]) - weld_stats["vertices"],
                   weld_merged_classes=weld_stats["merged_classes"], weld_largest_class=weld_stats["largest_class"],
                   weld_collapsed_faces=weld_stats["collapsed_faces"])
    out.export(args.mesh_out)
    folder = os.path.dirname(os.path.abspath(args.mesh_out))
    np.save(os.path.join(folder, "face_map.npy"), face_map)
    np.save(os.path.join(folder, "vertex_target.npy"), vertex_target)
    if args.make_manifold:
        np.save(os.path.join(folder, "cut_vertex_map.npy"), cut_vertex_map)
    if args.weld is not None:
        np.save(os.path.join(folder, "weld_vertex_map.npy"), weld_vertex_map)
        np.save(os.path.join(folder, "weld_vertex_class.npy"), weld_vertex_class)
    if args.vertex_features is not None:
        import torch
        from quadraturefields_amd import baking
        from quadraturefields_amd.mesh_utils import RayIntersector
        table = np.load(args.vertex_features)
        inter = RayIntersector(source, device=args.device, builder="device")
        moved = baking.transfer_vertex_features(inter, torch.from_numpy(np.ascontiguousarray(table, np.float32)).to(inter.device),
                                                torch.from_numpy(np.asarray(decimated.vertices, np.float64)).to(inter.device))
        if args.weld is not None:
            moved = baking.weld_vertex_features(moved, weld_vertex_class, out.vertices.shape[0], "first")
        np.save(args.out_vertex_features, moved.cpu().numpy())
        d = mc_utils.mesh_distance(out, source, device=args.device)
        cut = dict(cut, distance_out_to_in_mean=d.a_to_b_mean, distance_out_to_in_max=d.a_to_b_max,
                   distance_in_to_out_mean=d.b_to_a_mean, distance_in_to_out_max=d.b_to_a_max)
    if args.distance_samples is not None:
        d = mc_utils.mesh_distance(out, source, device=args.device, samples=args.distance_samples)
        cut = dict(cut, distance_samples=args.distance_samples, distance_sampled_out_to_in_mean=d.a_to_b_mean,
                   distance_sampled_out_to_in_rms=d.a_to_b_rms, distance_sampled_out_to_in_max=d.a_to_b_max,
                   distance_sampled_in_to_out_mean=d.b_to_a_mean, distance_sampled_in_to_out_rms=d.b_to_a_rms,
                   distance_sampled_in_to_out_max=d.b_to_a_max)
    print(json.dumps(dict(stats, boundary=args.boundary, boundary_weight=args.boundary_weight, faces_in=n_f, vertices_in=n_v, target_faces=target,
                          faces_out=int(out.faces.shape[0]), vertices_out=int(out.vertices.shape[0]), **cut)))


if __name__ == "__main__":
    main()
