"""Bake the SG field's features at the mesh VERTICES and render the test views from them: the vertex-baked renderer
(``render_image_finetune_baking_with_occgrid`` of the reference) on the synthetic scene.

    python examples/evaluate_vertex_baked.py --synthetic --root ROOT --num_lobes 6 --log2_hashmap_size 19
                                             --ckpt_path ROOT/fit_sg.pth [--early_stop_eps E] [--mesh_path MESH]
                                             [--size 200] [--views 4] [--up_sample 1] [--shells 2] [--subdivisions 3]
                                             [--features PATH] [--quantise {linear,sigma}] [--save_quantised PREFIX]
                                             [--load_quantised PREFIX] [--fit_samples_per_face N]

The mesh is ``--mesh_path`` or, without it, the shell mesh ``examples/fit_sg_synthetic.py`` fits on (``--shells``,
``--subdivisions``); the field is ``--ckpt_path``'s ``radiance_field`` (what ``fit_sg_synthetic.py --out`` wrote) or, if
the file does not exist, the seeded SG state.  ``baking.bake_vertex_features`` evaluates the field once per vertex and the
table goes to ``ROOT/vertex_features.npy``; every orbit view is rendered by ``FrameRenderer.render_vertex_baked`` and
scored by ``metrics.FrameScorer`` against the SG field's own render of the view on the same mesh at ``up_sample`` 1, as
``examples/evaluate_baked_textures.py --synthetic`` scores a texture set -- the score is what interpolating the features
inside a triangle costs.  Prints PSNR / SSIM (and one JSON line); with ``--early_stop_eps`` the frame is rendered front to
back with early ray termination and the share of the samples that were shaded is printed too.  ``--features PATH`` loads
a [V, 3 + 7L + 1] table (``vertex_features.npy``, or what ``examples/finetune_vertex_baked.py`` wrote) instead of baking
one; nothing is written then.  ``--quantise {linear,sigma}`` quantises the baked or loaded table to 64-byte uint8 records
with that colour codec (``baking.quantise_vertex_features``) and renders from the records;
``--save_quantised PREFIX`` writes its uint8 PNG set (``PREFIX + alpha.png`` ...), ``--load_quantised PREFIX`` reads one
(written with the codec ``--quantise`` names, default linear) instead of quantising.  The PSNR against the fp32 vertex
frame is then printed too.  ``--fit_samples_per_face N`` also fits the fp32 table to the field over the surface
(``baking.fit_vertex_features`` with the baked or loaded table as the prior), renders the same
views from the fitted table and prints its PSNR / SSIM and both tables' ``baking.vertex_surface_error`` beside the
others; without the flag nothing else changes.
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
    ap.add_argument("--up_sample", type=float, default=1.0)
    ap.add_argument("--early_stop_eps", type=float, default=None,
                    help="render front to back in one launch and stop a pixel once its transmittance has fallen below this "
                         "threshold, in [0, 1); not given: every sample is shaded, as in the reference")
    ap.add_argument("--size", type=int, default=200, help="ground-truth width and height")
    ap.add_argument("--views", type=int, default=4, help="orbit cameras")
    ap.add_argument("--shells", type=int, default=2)
    ap.add_argument("--subdivisions", type=int, default=3)
    ap.add_argument("--features", type=str, default="", help="load this vertex table (.npy) instead of baking one")
    ap.add_argument("--quantise", choices=("linear", "sigma"), default=None,
                    help="quantise the vertex table to uint8 records with this colour codec before rendering")
    ap.add_argument("--save_quantised", type=str, default="", help="write the quantised table's PNG set under this prefix")
    ap.add_argument("--load_quantised", type=str, default="", help="read the quantised table's PNG set from this prefix")
    ap.add_argument("--fit_samples_per_face", type=int, default=0,
                    help="also score the table fitted to the field over the surface, with this many samples per face")
    return ap.parse_args(argv)


def main(argv=None):
    args = parse(argv)
    if not args.synthetic:
        sys.exit("evaluate_vertex_baked.py: only --synthetic is implemented (orbit cameras, the SG field as ground truth)")
    from quadraturefields_amd import baking, synthetic
    from quadraturefields_amd.mesh_io import load_mesh
    from quadraturefields_amd.mesh_utils import MeshIntersection, make_camera
    from quadraturefields_amd.metrics import FrameScorer, _factor
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceFieldSGNew
    from quadraturefields_amd.render import FrameRenderer

    device = torch.device("cuda:0")
    factor = _factor(args.up_sample)
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
    with torch.no_grad():
        if args.features:
            features = torch.from_numpy(np.load(args.features).astype(np.float32)).to(device)
            print(f"loaded {features.shape[0]} vertices x {features.shape[1]} columns from {args.features}")
        else:
            features = baking.bake_vertex_features(sg, mesh_intersect)
            path = os.path.join(args.root, "vertex_features.npy")
            np.save(path, features.cpu().numpy())
            print(f"baked {features.shape[0]} vertices x {features.shape[1]} columns ({features.numel() * 4 / 1e6:.2f} MB) -> {path}")
        asset = features
        if args.load_quantised:
            asset = baking.QuantisedVertexFeatures.load(args.load_quantised, features.shape[0], args.num_lobes,
                                                        compression_type=args.quantise or "linear", device=device)
            print(f"loaded the quantised table of {asset.n_vertices} vertices from {args.load_quantised}*.png")
        elif args.quantise or args.save_quantised:
            asset = baking.quantise_vertex_features(features, compression_type=args.quantise or "linear")
            print(f"quantised {asset.n_vertices} vertices to {asset.records().shape[0]} records of 64 bytes "
                  f"({asset.records().numel() / 1e6:.2f} MB)")
        if args.save_quantised and asset is not features:
            os.makedirs(os.path.dirname(args.save_quantised) or ".", exist_ok=True)
            asset.save(args.save_quantised)
            print(f"wrote {args.save_quantised}*.png")
        sq_err, n_px = torch.zeros((), dtype=torch.float64, device=device), 0
        renderer = FrameRenderer(mesh_intersect, sg, render_step_size=5e-3)
        size = args.size
        focal = synthetic.lego_focal(size)
        scorer = FrameScorer(size, size, up_sample=factor, capacity=max(args.views, 1), device=device)
        shaded = samples = 0
        fitted = fit_scorer = None
        if args.fit_samples_per_face > 0:
            fitted = baking.fit_vertex_features(sg, mesh, args.fit_samples_per_face, prior=features, device=device)
            fit_scorer = FrameScorer(size, size, up_sample=factor, capacity=max(args.views, 1), device=device)
        for c2w in synthetic.orbit_cameras(args.views):
            o, d = synthetic.camera_rays(c2w, focal, size, size, device=device)
            pixels = renderer.render(o, d, camera=make_camera(c2w, focal, size, size))[0]        # the field's own frame
            o, d = synthetic.camera_rays(c2w, focal * factor, size * factor, size * factor, device=device)
            camera = make_camera(c2w, focal * factor, size * factor, size * factor)
            rgb, _, depth, n_samples = renderer.render_vertex_baked(o, d, asset, camera=camera,
                                                                    early_stop_eps=args.early_stop_eps)
            if args.early_stop_eps is not None and n_samples:
                shaded += int(mesh_intersect.rayintersector.last_frame.shaded_count.sum())
                samples += n_samples
            if asset is not features:                   # the same frame from the fp32 table: what the codes cost
                rgb32 = renderer.render_vertex_baked(o, d, features, camera=camera, early_stop_eps=args.early_stop_eps)[0]
                sq_err += ((rgb.double() - rgb32.double()) ** 2).sum()
                n_px += rgb.numel()
            scorer.score(rgb, pixels)
            if fitted is not None:
                fit_scorer.score(renderer.render_vertex_baked(o, d, fitted, camera=camera,
                                                              early_stop_eps=args.early_stop_eps)[0], pixels)
        res = scorer.results()
    out = {"psnr": res["psnr_avg"], "ssim": res["ssim_avg"], "psnrs": res["psnr"].tolist(), "ssims": res["ssim"].tolist(),
           "vertices": int(features.shape[0]), "columns": int(features.shape[1])}
    print("psnr: ", out["psnr"])
    print("ssim: ", out["ssim"])
    if args.early_stop_eps is not None:
        out["shaded_share"] = shaded / max(samples, 1)
        print(f"samples shaded (early_stop_eps {args.early_stop_eps}): {shaded} of {samples} = {out['shaded_share']:.4f}")
    if asset is not features:
        mse = float(sq_err) / max(n_px, 1)
        out["psnr_vs_fp32_vertex"] = -10.0 * float(np.log10(mse)) if mse > 0 else float("inf")
        print("psnr vs fp32 vertex frame: ", out["psnr_vs_fp32_vertex"])
    if fitted is not None:
        fit_res = fit_scorer.results()
        n_fresh = args.fit_samples_per_face * int(mesh.faces.shape[0])
        errors = {k: baking.vertex_surface_error(sg, mesh, t, n_fresh, seed=1) for k, t in (("", features), ("fit_", fitted))}
        out.update({"fit_samples_per_face": args.fit_samples_per_face, "fit_psnr": fit_res["psnr_avg"],
                    "fit_ssim": fit_res["ssim_avg"], "surface_error_rms": errors[""]["rms"],
                    "fit_surface_error_rms": errors["fit_"]["rms"]})
        print(f"fitted table ({args.fit_samples_per_face} samples per face): psnr {out['fit_psnr']}  ssim {out['fit_ssim']}")
        print(f"surface error (rms, pixel units, fresh samples): {out['surface_error_rms']:.3e} as loaded or baked, "
              f"{out['fit_surface_error_rms']:.3e} fitted")
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
