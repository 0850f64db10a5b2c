"""A level of detail for the vertex-baked asset: bake the table, decimate the mesh, carry the table over to the decimated
mesh at the closest points of the full one (``baking.transfer_vertex_features``) and render the
held-out views with both assets.

    python examples/lod_vertex_baked.py --synthetic --root ROOT --num_lobes 6 --log2_hashmap_size 19
                                        --ckpt_path ROOT/fit_sg.pth --ratio 0.25 [--mesh_path MESH] [--features PATH]
                                        [--size 200] [--views 4] [--shells 2] [--subdivisions 3] [--boundary {lock,collapse}]
                                        [--fit_samples_per_face N]

The mesh is ``--mesh_path`` or the shell mesh ``examples/fit_sg_synthetic.py`` fits on; the field is ``--ckpt_path``'s
``radiance_field`` or, if the file does not exist, the seeded SG state.  The table is ``--features PATH`` (what
``examples/finetune_vertex_baked.py`` wrote: the case this is for, a table fitted to images that a re-bake would throw
away) or ``baking.bake_vertex_features`` of the field.  The mesh is decimated to ``ratio * F`` faces
(``mc_utils.decimate_mesh``), the table is transferred, and every orbit view is rendered three times by
``FrameRenderer.render_vertex_baked``: the full asset, the decimated mesh with the transferred table, and the decimated
mesh with a table baked again from the field at its vertices.  Each is scored by ``metrics.FrameScorer`` against the SG
field's own render of the view on the full mesh.  Prints faces, vertices, table bytes and PSNR / SSIM of each, the
measured surface distance between the two meshes, and one JSON line; writes ``ROOT/lod_mesh.ply`` and
``ROOT/lod_vertex_features.npy``.

With ``--fit_samples_per_face N`` two more assets are rendered and scored beside those three: the full and the decimated
mesh, each with a table fitted to the field over its surface (``baking.fit_vertex_features`` with N samples per face,
DESIGN.md section 3.9i) in place of the point bake.  Without the flag nothing else changes."""
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
    ap.add_argument("--ratio", type=float, default=0.25, help="faces of the decimated mesh = floor(ratio * F)")
    ap.add_argument("--boundary", choices=("lock", "collapse"), default="lock")
    ap.add_argument("--size", type=int, default=200)
    ap.add_argument("--views", type=int, default=4, help="orbit cameras")
    ap.add_argument("--shells", type=int, default=2)
    ap.add_argument("--subdivisions", type=int, default=3)
    ap.add_argument("--features", type=str, default="", help="load this vertex table (.npy) instead of baking one")
    ap.add_argument("--fit_samples_per_face", type=int, default=0,
                    help="also score tables fitted to the field over the surface, with this many samples per face")
    return ap.parse_args(argv)


def main(argv=None):
    args = parse(argv)
    if not args.synthetic:
        sys.exit("lod_vertex_baked.py: only --synthetic is implemented (orbit cameras, the SG field as ground truth)")
    if not 0.0 < args.ratio <= 1.0:
        sys.exit("lod_vertex_baked.py: --ratio must lie in (0, 1]")
    from quadraturefields_amd import baking, mc_utils, synthetic
    from quadraturefields_amd.mesh_io import load_mesh
    from quadraturefields_amd.mesh_utils import MeshIntersection, make_camera
    from quadraturefields_amd.metrics import FrameScorer
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceFieldSGNew
    from quadraturefields_amd.render import FrameRenderer

    device = torch.device("cuda:0")
    mesh = load_mesh(args.mesh_path) if args.mesh_path else synthetic.shell_mesh(n_shells=args.shells,
                                                                                 subdivisions=args.subdivisions)

    def intersection(m):
        return MeshIntersection(m, simplify_mesh=False, scale=1.0, num_intersections=args.max_hits, render_step_size=5e-3,
                                device=device)
    full = intersection(mesh)
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
    with torch.no_grad():
        if args.features:
            table = torch.from_numpy(np.load(args.features).astype(np.float32)).to(device)
        else:
            table = baking.bake_vertex_features(sg, full)
        target = int(args.ratio * mesh.faces.shape[0])
        small_mesh = mc_utils.decimate_mesh(mesh, target, device=device, boundary=args.boundary)[0]
        small = intersection(small_mesh)
        moved = baking.transfer_vertex_features(full, table, small.vertices)
        rebaked = baking.bake_vertex_features(sg, small)
        distance = mc_utils.mesh_distance(small_mesh, mesh, device=device)
        small_mesh.export(os.path.join(args.root, "lod_mesh.ply"))
        np.save(os.path.join(args.root, "lod_vertex_features.npy"), moved.cpu().numpy())

        assets = {"full": (full, table), "transferred": (small, moved), "rebaked": (small, rebaked)}
        if args.fit_samples_per_face > 0:
            assets["fitted"] = (full, baking.fit_vertex_features(sg, mesh, args.fit_samples_per_face, device=device))
            assets["fitted_decimated"] = (small, baking.fit_vertex_features(sg, small_mesh, args.fit_samples_per_face,
                                                                            device=device))
        size, focal = args.size, synthetic.lego_focal(args.size)
        scorers = {k: FrameScorer(size, size, up_sample=1, capacity=max(args.views, 1), device=device) for k in assets}
        renderers = {k: FrameRenderer(mi, sg, render_step_size=5e-3) for k, (mi, _) in assets.items()}
        for c2w in synthetic.orbit_cameras(args.views):
            o, d = synthetic.camera_rays(c2w, focal, size, size, device=device)
            camera = make_camera(c2w, focal, size, size)
            pixels = renderers["full"].render(o, d, camera=camera)[0]                  # the field's own frame
            for k, (_, feats) in assets.items():
                scorers[k].score(renderers[k].render_vertex_baked(o, d, feats, camera=camera)[0], pixels)
    out = {"ratio": args.ratio, "distance_out_to_in_mean": distance.a_to_b_mean, "distance_out_to_in_max": distance.a_to_b_max,
           "distance_in_to_out_mean": distance.b_to_a_mean, "distance_in_to_out_max": distance.b_to_a_max}
    for k, (mi, feats) in assets.items():
        res = scorers[k].results()
        out[k] = {"faces": int(mi.mesh.faces.shape[0]), "vertices": int(feats.shape[0]), "table_bytes": int(feats.numel() * 4),
                  "psnr": res["psnr_avg"], "ssim": res["ssim_avg"]}
        print(f"{k:{max(12, *map(len, assets))}s} {out[k]['faces']:8d} faces {out[k]['vertices']:8d} vertices {out[k]['table_bytes'] / 1e6:8.2f} MB   "
              f"psnr {out[k]['psnr']:.2f}  ssim {out[k]['ssim']:.4f}")
    print(f"surface distance: decimated -> full mean {distance.a_to_b_mean:.3e} max {distance.a_to_b_max:.3e}, "
          f"full -> decimated mean {distance.b_to_a_mean:.3e} max {distance.b_to_a_max:.3e}")
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
