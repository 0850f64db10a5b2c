"""The reference's evaluation loop (``test()`` of examples/train_finetune.py:575-694) on the synthetic scene, scored on
the device:

    python examples/evaluate_synthetic.py OUT_DIR [--size 800] [--up_sample 2] [--views 4] [--shells 12] [--subdivisions 6]
                                                  [--log2_hashmap_size 19] [--early_stop_eps EPS] [--render_step_size 5e-3]

Every view is rendered at ``up_sample`` times the ground-truth size, as the scripts do (run_nerfsynthetic_finetune.sh:9),
and scored by ``metrics.FrameScorer``: INTER_AREA down-sample, PSNR, SSIM, the rgb / error / depth images, with no host
wait per frame; ``results()`` after the last view is the loop's one synchronisation for the scores.  There is no data
set to load, so the ground truth of a view is the same scene rendered at ``up_sample 1`` by a field whose hash table is
perturbed.  Writes ``results.json`` with the scripts' key names (``psnr``, ``ssim``; LPIPS is not computed) and
``rgb_test_after_{i}.png``, ``rgb_error_after_{i}.png``, ``depth_after_{i}.png``.

``--early_stop_eps EPS`` renders the scored views front to back in rank windows with early ray termination
(``FrameRenderer.render(..., early_stop_eps=EPS)``) and prints, per view, the share of the frame's
samples the field evaluated; the ground truth stays on the default route.  The seeded field is thin: at the default
``--render_step_size`` no ray ever stops, 0.5 makes the shells opaque.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out_dir")
    ap.add_argument("--size", type=int, default=800, help="ground-truth width and height")
    ap.add_argument("--up_sample", type=float, default=2.0)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--shells", type=int, default=12)
    ap.add_argument("--subdivisions", type=int, default=6)
    ap.add_argument("--log2_hashmap_size", type=int, default=19)
    ap.add_argument("--bvh_builder", choices=("host", "device"), default="host",
                    help="where the ray-mesh BVH is built: host (binned SAH) or device (linear BVH on the GPU: faster build, slower traversal)")
    ap.add_argument("--early_stop_eps", type=float, default=None,
                    help="transmittance threshold in [0, 1): render the scored views front to back with early ray termination")
    ap.add_argument("--render_step_size", type=float, default=5e-3, help="the compositing step (optical depth = density * step)")
    args = ap.parse_args(argv)

    from quadraturefields_amd import synthetic
    from quadraturefields_amd.mesh_utils import MeshIntersection, make_camera
    from quadraturefields_amd.metrics import FrameScorer
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceField
    from quadraturefields_amd.render import FrameRenderer
    from quadraturefields_amd.texture_utils import _write_png

    device = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    size, log2_t = args.size, args.log2_hashmap_size
    scorer = FrameScorer(size, size, up_sample=args.up_sample, capacity=args.views, device=device)
    f = scorer.factor
    mesh = synthetic.shell_mesh(n_shells=args.shells, subdivisions=args.subdivisions)
    mi = MeshIntersection(mesh, simplify_mesh=False, scale=1.0, num_intersections=25, render_step_size=args.render_step_size, device=device,
                          bvh_builder=args.bvh_builder)

    def field_of(perturbed):
        field = NGPRadianceField(aabb=[-1.5] * 3 + [1.5] * 3, log2_hashmap_size=log2_t)
        n_rows = field.mlp_base.grid.n_rows
        state = synthetic.seeded_ngp_state(log2_t, n_rows)
        field.load_state_dict(synthetic.perturbed_ngp_state(state, n_rows) if perturbed else state, strict=False)
        return field.to(device)

    renderer = FrameRenderer(mi, field_of(False))
    truth_renderer = FrameRenderer(mi, field_of(True))

    os.makedirs(args.out_dir, exist_ok=True)
    focal = synthetic.lego_focal(size)
    for i, c2w in enumerate(synthetic.orbit_cameras(args.views)):
        o, d = synthetic.camera_rays(c2w, focal, size, size, device=device)
        pixels = truth_renderer.render(o, d, camera=make_camera(c2w, focal, size, size))[0]
        o, d = synthetic.camera_rays(c2w, focal * f, size * f, size * f, device=device)
        rgb, _, depth, n_samples = renderer.render(o, d, camera=make_camera(c2w, focal * f, size * f, size * f),
                                                   early_stop_eps=args.early_stop_eps)
        if args.early_stop_eps is not None:
            frame = mi.rayintersector.last_frame
            evaluated, shaded = int(frame.evaluated_count.sum()), int(frame.shaded_count.sum())
            print(f"view {i}: {evaluated} of {n_samples} samples evaluated ({evaluated / max(n_samples, 1):.1%}), "
                  f"{shaded} contribute")
        scorer.score(rgb, pixels, depth=depth, images=True)
        # the images live in reused buffers: they are copied out before the next frame is scored
        names = ("rgb_test_after_{}.png", "rgb_error_after_{}.png", "depth_after_{}.png")
        for name, image in zip(names, scorer.last_images()):
            _write_png(os.path.join(args.out_dir, name.format(i)), image.cpu().numpy())
    res = scorer.results()
    out = {"psnr": res["psnr_avg"], "ssim": res["ssim_avg"], "psnrs": res["psnr"].tolist(), "ssims": res["ssim"].tolist(),
           "up_sample": f, "views": args.views, "width": size, "height": size}
    with open(os.path.join(args.out_dir, "results.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    print(f"PSNR: {out['psnr']}, SSIM: {out['ssim']}")


if __name__ == "__main__":
    main()
