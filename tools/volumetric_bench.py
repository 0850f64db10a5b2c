"""Volumetric frames: frame time of ``utils.render_image_with_occgrid_test`` (rounds with early
ray termination) against ``utils.render_image_with_occgrid`` (march everything, density pass, compaction, field pass),
both under ``no_grad``.

    python tools/volumetric_bench.py [--size 800] [--views 4] [--repeats 3] [--out profiles/volumetric/volumetric_bench.json]

Bench scene: the seeded NGP field (T = 2^19, aabb +-1.5), a 128^3 occupancy grid filled from its density
(``--occ_threshold``), orbit views at ``--size`` squared, step 5e-3, ``early_stop_eps`` 1e-4, ``max_samples`` 1024, white
background.  The two renderers alternate view by view after a warm-up on other views; a frame is timed by a host clock
around a call that ends in a device synchronise (both renderers wait for the device themselves: the baseline for its
sample count, the new one once per round).  Reported per renderer: the median frame time over views and repeats, the
spread of the per-repeat medians, the samples it shaded, and for the new renderer the number of rounds; also the largest
and the mean pixel difference between the two images and the number of pixels that differ by more than 1e-3 (they are
different estimators: the baseline drops samples with T < 1e-4 one by one, the rounds stop a ray at a round's end, and a
round restarts the step lattice at its near plane, so a sample whose midpoint sits on a cell face can fall either way).  No ratio is promised: the file holds what was measured.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--step", type=float, default=5e-3)
    ap.add_argument("--max_samples", type=int, default=1024)
    ap.add_argument("--early_stop_eps", type=float, default=1e-4)
    ap.add_argument("--occ_threshold", type=float, default=5.0)
    ap.add_argument("--log2_hashmap_size", type=int, default=19)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "volumetric", "volumetric_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("volumetric_bench.py: no HIP device (timings are only taken on the GPU)")
    torch.set_grad_enabled(False)
    from quadraturefields_amd import synthetic, utils
    from quadraturefields_amd.datasets.utils import Rays
    from quadraturefields_amd.estimators import OccGridEstimator
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceField

    dev = torch.device("cuda:0")
    aabb = [-1.5] * 3 + [1.5] * 3
    field = NGPRadianceField(aabb=aabb, log2_hashmap_size=args.log2_hashmap_size)
    field.load_state_dict(synthetic.seeded_ngp_state(args.log2_hashmap_size, field.mlp_base.grid.n_rows), strict=False)
    field = field.to(dev).eval()
    est = OccGridEstimator(roi_aabb=aabb, resolution=128, levels=1).to(dev).eval()
    est.set_occupancy_from_density(lambda p: field.query_density(p), threshold=args.occ_threshold)
    size = args.size
    focal = synthetic.lego_focal(size)
    bk = torch.ones(3, device=dev)
    views = []
    for c2w in synthetic.orbit_cameras(args.views + args.warmup, seed=17):
        o, d = synthetic.camera_rays(c2w, focal, size, size, device=dev)
        views.append(Rays(origins=o.reshape(size, size, 3), viewdirs=d.reshape(size, size, 3)))
    common = dict(render_step_size=args.step, render_bkgd=bk)

    def baseline(rays):
        rgb, _, _, n, _ = utils.render_image_with_occgrid(field, est, rays, **common)
        return rgb, n, None

    def rounds(rays):
        trace = []
        rgb, _, _, n, pos = utils.render_image_with_occgrid_test(args.max_samples, field, est, rays, trace=trace,
                                                                 early_stop_eps=args.early_stop_eps, **common)
        return rgb, n, (len(trace), pos.shape[0])

    def timed(fn, rays):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn(rays)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, out

    for rays in views[:args.warmup]:
        baseline(rays), rounds(rays)
    modes = {"render_image_with_occgrid": baseline, "render_image_with_occgrid_test": rounds}
    times = {k: [[] for _ in range(args.repeats)] for k in modes}
    samples = {k: [] for k in modes}
    n_rounds, marched, max_diff, mean_diff, differing = [], [], 0.0, [], []
    for rep in range(args.repeats):
        for rays in views[args.warmup:]:
            images = {}
            for name, fn in modes.items():
                ms, (rgb, n, extra) = timed(fn, rays)
                times[name][rep].append(ms)
                images[name] = rgb
                if rep == 0:
                    samples[name].append(int(n))
                    if extra:
                        n_rounds.append(extra[0])
                        marched.append(extra[1])
            if rep == 0:
                a, b = images.values()
                diff = (a - b).abs()
                max_diff = max(max_diff, float(diff.max()))
                mean_diff.append(float(diff.mean()))
                differing.append(int((diff.reshape(-1, 3).max(dim=1).values > 1e-3).sum()))
    result = {"size": size, "views": args.views, "repeats": args.repeats, "step": args.step, "max_samples": args.max_samples,
              "early_stop_eps": args.early_stop_eps, "occupancy": float(est.binaries.float().mean()),
              "device": torch.cuda.get_device_name(0), "max_pixel_difference": max_diff,
              "mean_pixel_difference": mean_diff, "pixels_differing_by_1e-3": differing,
              "rounds_per_frame": n_rounds, "marched_samples_per_frame": marched}
    for name in modes:
        per_rep = [statistics.median(t) for t in times[name]]
        result[name] = {"frame_ms_median": statistics.median([x for t in times[name] for x in t]),
                        "frame_ms_repeat_medians": per_rep, "frame_ms_spread": max(per_rep) - min(per_rep),
                        "samples_per_frame": samples[name]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
