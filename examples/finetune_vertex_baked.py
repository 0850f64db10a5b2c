"""Fit the vertex-baked table to images: bake the SG field's features at the mesh vertices, then keep optimising the table
against training views through the differentiable vertex shading -- what is lost by baking once
per vertex is the linear interpolation inside a triangle, and the table can be fitted to make up for it.

    python examples/finetune_vertex_baked.py --synthetic --root ROOT --num_lobes 6 --log2_hashmap_size 19
                                             --ckpt_path ROOT/fit_sg.pth [--mesh_path MESH] [--size 200] [--views 4]
                                             [--train_views 16] [--steps 300] [--batch_rays 16384] [--lr 5e-3]
                                             [--train_density] [--shells 2] [--subdivisions 3]

Scene arguments as ``examples/evaluate_vertex_baked.py``.  The targets are the SG field's own frames of ``--train_views``
orbit cameras (``FrameRenderer.render`` on the same mesh); ``baking.finetune_vertex_features`` draws ``--batch_rays``
random rays of them per step.  ``--views`` held-out orbit cameras, drawn with another seed, are rendered by
``FrameRenderer.render_vertex_baked`` and scored by ``metrics.FrameScorer`` before and after.  Prints both PSNR / SSIM
pairs and one JSON line, writes ``ROOT/vertex_features_finetuned.npy`` (``evaluate_vertex_baked.py --features`` renders
it) and exits non-zero if the held-out PSNR did not rise.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

TRAIN_SEED, HELD_OUT_SEED = 0, 1234


def parse(argv):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--synthetic", action="store_true", help="orbit cameras; targets rendered from the SG field")
    ap.add_argument("--root", type=str, default="./")
    ap.add_argument("--mesh_path", type=str, default="")
    ap.add_argument("--ckpt_path", type=str, default="")
    ap.add_argument("--num_lobes", type=int, default=6)
    ap.add_argument("--log2_hashmap_size", type=int, default=19)
    ap.add_argument("--scale", type=float, default=1.5)
    ap.add_argument("--max_hits", type=int, default=25)
    ap.add_argument("--size", type=int, default=200, help="width and height of the training and the held-out frames")
    ap.add_argument("--views", type=int, default=4, help="held-out orbit cameras")
    ap.add_argument("--train_views", type=int, default=16, help="training orbit cameras")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--batch_rays", type=int, default=16384)
    ap.add_argument("--lr", type=float, default=5e-3)
    ap.add_argument("--train_density", action="store_true", help="also train the density column (clamped at >= 0)")
    ap.add_argument("--shells", type=int, default=2)
    ap.add_argument("--subdivisions", type=int, default=3)
    return ap.parse_args(argv)


def main(argv=None):
    args = parse(argv)
    if not args.synthetic:
        sys.exit("finetune_vertex_baked.py: only --synthetic is implemented (orbit cameras, the SG field as ground truth)")
    from quadraturefields_amd import baking, synthetic
    from quadraturefields_amd.datasets.utils import Rays
    from quadraturefields_amd.mesh_io import load_mesh
    from quadraturefields_amd.mesh_utils import MeshIntersection, make_camera
    from quadraturefields_amd.metrics import FrameScorer
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceFieldSGNew
    from quadraturefields_amd.render import FrameRenderer

    device = torch.device("cuda:0")
    mesh = load_mesh(args.mesh_path) if args.mesh_path else synthetic.shell_mesh(n_shells=args.shells,
                                                                                 subdivisions=args.subdivisions)
    mesh_intersect = MeshIntersection(mesh, simplify_mesh=False, scale=1.0, num_intersections=args.max_hits,
                                      render_step_size=5e-3, device=device)
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
    renderer = FrameRenderer(mesh_intersect, sg, render_step_size=5e-3)
    size = args.size
    focal = synthetic.lego_focal(size)

    def views(n, seed):
        out = []
        with torch.no_grad():
            for c2w in synthetic.orbit_cameras(n, seed=seed):
                o, d = synthetic.camera_rays(c2w, focal, size, size, device=device)
                cam = make_camera(c2w, focal, size, size)
                out.append((o, d, cam, renderer.render(o, d, camera=cam)[0]))      # the field's own frame
        return out

    def score(module):
        scorer = FrameScorer(size, size, up_sample=1, capacity=max(args.views, 1), device=device)
        with torch.no_grad():
            for o, d, cam, pixels in held_out:
                scorer.score(renderer.render_vertex_baked(o, d, module, camera=cam)[0], pixels)
        res = scorer.results()
        return float(res["psnr_avg"]), float(res["ssim_avg"])

    train, held_out = views(args.train_views, TRAIN_SEED), views(args.views, HELD_OUT_SEED)
    module = baking.VertexBakedFeatures.from_field(sg, mesh_intersect)
    print(f"baked {module.table.shape[0]} vertices x {module.width} columns; {args.train_views} training views, "
          f"{args.views} held-out views at {size}x{size}")
    before = score(module)
    all_o = torch.cat([v[0] for v in train])
    all_d = torch.cat([v[1] for v in train])
    all_rgb = torch.cat([v[3].reshape(-1, 3) for v in train])
    gen = torch.Generator(device=device).manual_seed(TRAIN_SEED)

    def next_batch():
        pick = torch.randint(0, all_o.shape[0], (args.batch_rays,), generator=gen, device=device)
        return Rays(origins=all_o[pick], viewdirs=all_d[pick]), all_rgb[pick]

    losses = baking.finetune_vertex_features(module, mesh_intersect, next_batch, args.steps, lr=args.lr,
                                             train_density=args.train_density)
    after = score(module)
    path = os.path.join(args.root, "vertex_features_finetuned.npy")
    np.save(path, module.features().cpu().numpy())
    head, tail = float(np.mean(losses[:5])), float(np.mean(losses[-5:]))
    print(f"loss: first five {head:.3e}, last five {tail:.3e} over {args.steps} steps")
    print(f"held-out psnr: {before[0]:.3f} -> {after[0]:.3f}")
    print(f"held-out ssim: {before[1]:.5f} -> {after[1]:.5f}")
    print("wrote", path)
    out = {"psnr_before": before[0], "psnr_after": after[0], "ssim_before": before[1], "ssim_after": after[1],
           "loss_first": head, "loss_last": tail, "steps": args.steps, "train_views": args.train_views,
           "vertices": int(module.table.shape[0]), "columns": module.width}
    print(json.dumps(out))
    if not after[0] > before[0]:
        sys.exit("finetune_vertex_baked.py: the held-out PSNR did not rise")
    return out


if __name__ == "__main__":
    main()
