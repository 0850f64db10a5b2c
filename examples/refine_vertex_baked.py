"""Refine the mesh where the vertex-baked table is too coarse for the SG field, and score every level: the conforming
midpoint split of DESIGN.md section 3.9c on the synthetic scene.

    python examples/refine_vertex_baked.py --synthetic --root ROOT --num_lobes 6 --log2_hashmap_size 19
                                           --ckpt_path ROOT/fit_sg.pth [--mesh_path MESH] [--size 200] [--views 4]
                                           [--shells 2] [--subdivisions 3] [--tol 0.01] [--max_levels 3]
                                           [--max_vertices N] [--uniform]

The mesh, the field and the cameras are those of ``examples/evaluate_vertex_baked.py`` (same arguments).  Per level,
``baking.refine_vertex_baked`` evaluates ``baking.vertex_edge_error`` on every edge -- how far the table's interpolation is
from the field at the edge's midpoint, in the units of a composited pixel --, marks the edges above ``--tol`` (every edge
with ``--uniform``; at most ``--max_vertices`` vertices in all, the largest errors first) and splits them
(``mc_utils.subdivide_mesh_device``).  A midpoint split does not move the surface: the samples and their depths stay, only
the table gains rows.  Per level the script prints V, F, the bytes of the fp32 table and of its 64-byte quantised records,
and the PSNR of the vertex-baked frames against the SG field's own frames of the INPUT mesh.  It writes the refined mesh
(``ROOT/mesh_refined.ply``), ``ROOT/vertex_features_refined.npy``, ``ROOT/face_map.npy`` (the input face every refined
face lies in) and ``ROOT/vertex_parents.npy`` (the two vertices a new vertex lies between), and prints one JSON line.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch


def parse(argv):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--synthetic", action="store_true", help="orbit cameras; ground truth rendered from the SG field")
    ap.add_argument("--root", type=str, default="./")
    ap.add_argument("--mesh_path", type=str, default="")
    ap.add_argument("--ckpt_path", type=str, default="")
    ap.add_argument("--num_lobes", type=int, default=6)
    ap.add_argument("--log2_hashmap_size", type=int, default=19)
    ap.add_argument("--scale", type=float, default=1.5)
    ap.add_argument("--max_hits", type=int, default=25)
    ap.add_argument("--size", type=int, default=200, help="frame width and height")
    ap.add_argument("--views", type=int, default=4, help="orbit cameras")
    ap.add_argument("--shells", type=int, default=2)
    ap.add_argument("--subdivisions", type=int, default=3)
    ap.add_argument("--tol", type=float, default=0.01, help="edges whose error is above this are split")
    ap.add_argument("--max_levels", type=int, default=3)
    ap.add_argument("--max_vertices", type=int, default=None, help="vertex budget: the largest errors are split first")
    ap.add_argument("--uniform", action="store_true", help="split every edge at every level, whatever its error")
    return ap.parse_args(argv)


def main(argv=None):
    args = parse(argv)
    if not args.synthetic:
        sys.exit("refine_vertex_baked.py: only --synthetic is implemented (orbit cameras, the SG field as ground truth)")
    from quadraturefields_amd import baking, synthetic
    from quadraturefields_amd.mesh_io import load_mesh
    from quadraturefields_amd.mesh_utils import MeshIntersection, make_camera
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceFieldSGNew
    from quadraturefields_amd.render import FrameRenderer, psnr

    device = torch.device("cuda:0")
    step = 5e-3
    mesh = load_mesh(args.mesh_path) if args.mesh_path else synthetic.shell_mesh(n_shells=args.shells,
                                                                                 subdivisions=args.subdivisions)
    log2_t = args.log2_hashmap_size
    sg = NGPRadianceFieldSGNew(aabb=[-args.scale] * 3 + [args.scale] * 3, use_viewdirs=False, num_g_lobes=args.num_lobes,
                               num_layers=2, log2_hashmap_size=log2_t)
    if args.ckpt_path and os.path.exists(args.ckpt_path):
        sg.load_state_dict(torch.load(args.ckpt_path, map_location="cpu")["radiance_field"])
        print("loaded", args.ckpt_path)
    else:
        sg.load_state_dict(synthetic.seeded_ngp_state(log2_t, sg.mlp_base.grid.n_rows, sg_lobes=args.num_lobes), strict=False)
        print("no checkpoint at", repr(args.ckpt_path), "-- the seeded SG state")
    sg = sg.to(device).eval()
    os.makedirs(args.root, exist_ok=True)
    size = args.size
    focal = synthetic.lego_focal(size)
    kw = dict(simplify_mesh=False, scale=1.0, num_intersections=args.max_hits, render_step_size=step, device=device)
    views = []
    with torch.no_grad():
        truth_renderer = FrameRenderer(MeshIntersection(mesh, **kw), sg, render_step_size=step)
        for c2w in synthetic.orbit_cameras(args.views):
            o, d = synthetic.camera_rays(c2w, focal, size, size, device=device)
            cam = make_camera(c2w, focal, size, size)
            views.append((o, d, cam, truth_renderer.render(o, d, camera=cam)[0].clone()))     # the field's own frame
        rows, result = [], None
        for n_levels in range(args.max_levels + 1):
            # the levels are deterministic: a run with one level more repeats the levels before it
            result = baking.refine_vertex_baked(mesh, sg, args.tol, max_levels=n_levels, max_vertices=args.max_vertices,
                                                render_step_size=step, device=device, uniform=args.uniform)
            split = [r for r in result.levels if r["marked"]]
            if len(split) < n_levels:
                break
            renderer = FrameRenderer(MeshIntersection(result.mesh, **kw), sg, render_step_size=step)
            scores = [float(psnr(renderer.render_vertex_baked(o, d, result.table, camera=cam)[0], truth))
                      for o, d, cam, truth in views]
            n_v, n_f = int(result.table.shape[0]), int(result.mesh.faces.shape[0])
            side = baking.vertex_texture_size(n_v)
            row = {"level": n_levels, "vertices": n_v, "faces": n_f, "table_bytes": n_v * 4 * int(result.table.shape[1]),
                   "quantised_bytes": side * side * 64, "psnr": float(np.mean(scores)), "psnrs": scores}
            if split:
                last = split[-1]
                row.update(marked=last["marked"], edges=last["edges"], above_tol=last["above_tol"],
                           max_error=last["max_error"], mean_error=last["mean_error"])
            rows.append(row)
            print(f"level {n_levels}: V = {n_v}, F = {n_f}, table {row['table_bytes']} bytes, quantised {row['quantised_bytes']} "
                  f"bytes, psnr vs the field's frames {row['psnr']:.2f} dB"
                  + (f" (split {row['marked']} of {row['edges']} edges, {row['above_tol']} above tol {args.tol}, largest error "
                     f"{row['max_error']:.4f})" if split else ""), flush=True)
    final = baking.refine_vertex_baked(mesh, sg, args.tol, max_levels=len(rows) - 1, max_vertices=args.max_vertices,
                                       render_step_size=step, device=device, uniform=args.uniform)
    final.mesh.export(os.path.join(args.root, "mesh_refined.ply"))
    np.save(os.path.join(args.root, "vertex_features_refined.npy"), final.table.cpu().numpy())
    np.save(os.path.join(args.root, "face_map.npy"), final.face_map)
    np.save(os.path.join(args.root, "vertex_parents.npy"), final.vertex_parents)
    print("wrote mesh_refined.ply, vertex_features_refined.npy, face_map.npy and vertex_parents.npy under", args.root)
    out = {"tol": args.tol, "uniform": bool(args.uniform), "max_vertices": args.max_vertices, "levels": rows}
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
