"""The volumetric NeRF frame of the reference's evaluation (``render_image_with_occgrid_test``, examples/utils.py:176-350)
and the transmittance mask built from it (``grid_transmittance_synthetic``, examples/mc_utils.py:462-570) on the
synthetic scene:

    python examples/evaluate_volumetric.py OUT_DIR [--size 800] [--views 4] [--max_samples 1024] [--step 5e-3]
                                                   [--log2_hashmap_size 19] [--mask_size 256]

Every view is marched in rounds with early ray termination (``early_stop_eps`` 1e-4) through a 128^3 occupancy grid
filled from the field's density, and scored on the device by ``metrics.FrameScorer`` against the same view rendered by a
field whose hash table is perturbed (there is no data set to load).  Writes ``results.json`` (``psnr``, ``ssim``, the
samples shaded per view), ``rgb_volumetric_{i}.png``, ``depth_volumetric_{i}.png`` and ``binaries_transmittance.pth``,
the bool mask of the cells that light reaches, ``mask_size`` cubed (the reference's is 1024).
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
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--max_samples", type=int, default=1024)
    ap.add_argument("--step", type=float, default=5e-3)
    ap.add_argument("--log2_hashmap_size", type=int, default=19)
    ap.add_argument("--occ_threshold", type=float, default=5.0)
    ap.add_argument("--mask_size", type=int, default=256)
    args = ap.parse_args(argv)

    from quadraturefields_amd import mc_utils, synthetic, utils
    from quadraturefields_amd.datasets.utils import Rays
    from quadraturefields_amd.estimators import OccGridEstimator
    from quadraturefields_amd.metrics import FrameScorer
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceField
    from quadraturefields_amd.texture_utils import _write_png

    device = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    size, log2_t = args.size, args.log2_hashmap_size
    aabb = [-1.5] * 3 + [1.5] * 3

    def field_of(perturbed):
        field = NGPRadianceField(aabb=aabb, log2_hashmap_size=log2_t)
        n_rows = field.mlp_base.grid.n_rows
        state = synthetic.seeded_ngp_state(log2_t, n_rows)
        field.load_state_dict(synthetic.perturbed_ngp_state(state, n_rows) if perturbed else state, strict=False)
        return field.to(device).eval()

    field, truth = field_of(False), field_of(True)
    estimator = OccGridEstimator(roi_aabb=aabb, resolution=128, levels=1).to(device).eval()
    estimator.set_occupancy_from_density(lambda p: field.query_density(p), threshold=args.occ_threshold)
    scorer = FrameScorer(size, size, up_sample=1, capacity=args.views, device=device)
    bkgd = torch.ones(3, device=device)
    kwargs = dict(render_step_size=args.step, render_bkgd=bkgd, early_stop_eps=1e-4)

    os.makedirs(args.out_dir, exist_ok=True)
    focal = synthetic.lego_focal(size)
    views, samples = [], []
    for i, c2w in enumerate(synthetic.orbit_cameras(args.views)):
        o, d = synthetic.camera_rays(c2w, focal, size, size, device=device)
        rays = Rays(origins=o.reshape(size, size, 3), viewdirs=d.reshape(size, size, 3))
        views.append(rays)
        pixels = utils.render_image_with_occgrid_test(args.max_samples, truth, estimator, rays, **kwargs)[0]
        rgb, _, depth, n, _ = utils.render_image_with_occgrid_test(args.max_samples, field, estimator, rays, **kwargs)
        samples.append(n)
        scorer.score(rgb.reshape(-1, 3), pixels.reshape(-1, 3), depth=depth.reshape(-1, 1), images=True)
        rgb_u8, _, depth_u8 = scorer.last_images()
        _write_png(os.path.join(args.out_dir, f"rgb_volumetric_{i}.png"), rgb_u8.cpu().numpy())
        _write_png(os.path.join(args.out_dir, f"depth_volumetric_{i}.png"), depth_u8.cpu().numpy())
    mask = mc_utils.transmittance_mask(field, estimator, views, max_samples=args.max_samples, size=args.mask_size, **kwargs)
    torch.save(mask.cpu(), os.path.join(args.out_dir, "binaries_transmittance.pth"))
    res = scorer.results()
    out = {"psnr": res["psnr_avg"], "ssim": res["ssim_avg"], "psnrs": res["psnr"].tolist(), "ssims": res["ssim"].tolist(),
           "samples": samples, "views": args.views, "width": size, "height": size,
           "transmittance_mask_fill": float(mask.float().mean())}
    with open(os.path.join(args.out_dir, "results.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    print(f"PSNR: {out['psnr']}, SSIM: {out['ssim']}, samples per view: {samples}")


if __name__ == "__main__":
    main()
