"""The baked-texture frame front to back against the two-launch route, on bench.py's configs[4]
scene: 4096^2 uint8 texture set, 6 lobes, 800 x 800 orbit frames of the bench mesh, both UV sets of the bench line (the
mesh's own charts and random per-triangle charts).

    python tools/baked_frame_bench.py [--frames 8] [--warmup 3] [--repeats 5] [--out profiles/baked_frame/baked_frame_bench.json]

  a  FrameRenderer.render_baked_async as it is without the keyword (shade every sample, write rgb / sigma, composite)
  b  early_stop_eps = 0      (one launch, never stops: the same pixels as a, bit for bit)
  c  early_stop_eps = 1e-3
  d  early_stop_eps = 1e-2
All four run in ONE process; a repeat times every case once over the same frames, in an order that rotates from repeat to
repeat, with device events around the case's frames (no host wait inside).  Reported per case: the median over the
repeats of the time per frame, the spread (min, max) over the repeats, and the share of the frames' samples that were
shaded.  Two texture sets: ``synthetic.random_textures`` (alpha uniform in 1..255: translucent, the rule fires late) and
an "opaque" set -- the same planes with every alpha code raised into 200..255 -- which STANDS IN for a trained scene:
there is no trained checkpoint to bake in this repository, so what a real asset gains lies between the two.
"""
import argparse
import json
import os
import statistics
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import bench

CASES = [("a", None), ("b", 0.0), ("c", 1e-3), ("d", 1e-2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--texture-size", type=int, default=4096)
    ap.add_argument("--lobes", type=int, default=6)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("baked_frame_bench.py: no HIP device (timings are only taken on the GPU)")
    torch.set_grad_enabled(False)
    warnings.simplefilter("ignore")
    from quadraturefields_amd import synthetic
    from quadraturefields_amd.mesh_utils import MeshIntersection, make_camera
    from quadraturefields_amd.render import FrameRenderer
    from quadraturefields_amd.texture_utils import FeatureCompression

    dev = torch.device("cuda:0")
    size, lobes = args.texture_size, args.lobes
    mesh, mi, _field = bench.build_scene(dev)
    mesh_r, uv_r = synthetic.per_triangle_charts(mesh, size, seed=42)
    mi_r = MeshIntersection(mesh_r, simplify_mesh=False, scale=1.0, num_intersections=bench.MAX_HITS,
                            render_step_size=bench.STEP, device=dev)
    uv_sets = {"charted": (mi, torch.from_numpy(synthetic.scaled_uv(mesh, size)).to(dev)),
               "per_triangle_random": (mi_r, torch.from_numpy(uv_r).to(dev))}
    tex = synthetic.random_textures(size, lobes, seed=42)
    opaque_alpha = (200 + tex["alpha"] % 56).astype(tex["alpha"].dtype)           # every code in 200..255, charts or not
    assert int(opaque_alpha.min()) >= 200
    comps = {}
    for name, alpha in (("random", tex["alpha"]), ("opaque", opaque_alpha)):
        comps[name] = FeatureCompression.from_arrays(alpha, tex["diffuse"], tex["colors"], tex["lambdas"],
                                                     compression_type="sigmoid", lambda_thres=7.5, device=dev)
        comps[name].records()
    del tex
    n_frames = args.frames + args.warmup
    cams = synthetic.orbit_cameras(n_frames, seed=42)
    focal = synthetic.lego_focal(bench.W)
    frames = [synthetic.camera_rays(c, focal, bench.W, bench.H, device=dev) + (make_camera(c, focal, bench.W, bench.H),)
              for c in cams]
    warm, timed = frames[:args.warmup], frames[args.warmup:]

    result = {"workload": f"configs[4] scene: baked SG textures {size}^2, L={lobes}, {bench.W}x{bench.H}, K={bench.MAX_HITS}, "
                          f"{args.frames} orbit frames per case and repeat, {args.repeats} repeats in rotating order",
              "cases": {"a": "render_baked_async (two launches)", "b": "front to back, eps 0", "c": "front to back, eps 1e-3",
                        "d": "front to back, eps 1e-2"},
              "opaque_set": "random_textures with every alpha code raised into 200..255: a stand-in for a trained scene "
                            "(no checkpoint exists to bake)",
              "runs": {}}
    for tex_name, comp in comps.items():
        for uv_name, (mi_u, uv) in uv_sets.items():
            fr = FrameRenderer(mi_u, None, render_step_size=bench.STEP)
            ri = mi_u.rayintersector

            def run(eps, views):
                out = None
                for o, d, cam in views:
                    out = fr.render_baked_async(o, d, uv, comp, cam) if eps is None else \
                        fr.render_baked_async(o, d, uv, comp, cam, early_stop_eps=eps)
                return out

            # untimed: the pixels of b equal a, the bound of c / d, the share of samples shaded
            share, max_change = {}, {}
            for case, eps in CASES:
                shaded = total = 0
                worst = 0.0
                for view in timed:
                    rgb, _, _, frame = run(eps, [view])
                    ref = run(None, [view])[0] if eps is not None else rgb
                    worst = max(worst, float((rgb - ref).abs().max()))
                    total += int(frame.hit_count.sum())
                    shaded += int(frame.shaded_count.sum()) if eps is not None else int(frame.hit_count.sum())
                share[case], max_change[case] = shaded / max(total, 1), worst
                if eps is not None and worst > 3 * eps:
                    sys.exit(f"baked_frame_bench.py: case {case} moved a pixel by {worst} > 3 eps")
            for case, eps in CASES:
                run(eps, warm)
            torch.cuda.synchronize()
            times = {case: [] for case, _ in CASES}
            for r in range(args.repeats):
                order = CASES[r % len(CASES):] + CASES[:r % len(CASES)]
                for case, eps in order:
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    run(eps, timed)
                    b.record()
                    b.synchronize()
                    times[case].append(a.elapsed_time(b) / len(timed))
            ri._settle_fused_policy(0)
            result["runs"][f"{tex_name}/{uv_name}"] = {
                "route": ri.last_route,
                "cases": {case: {"median_ms_per_frame": statistics.median(times[case]), "min_ms": min(times[case]),
                                 "max_ms": max(times[case]), "repeats_ms": times[case], "shaded_share": share[case],
                                 "max_pixel_change_vs_a": max_change[case]} for case, _ in CASES}}
            print(f"{tex_name}/{uv_name}: " + ", ".join(
                f"{case} {statistics.median(times[case]):.3f} ms [{min(times[case]):.3f}, {max(times[case]):.3f}] "
                f"shaded {share[case]:.3f}" for case, _ in CASES), flush=True)
    text = json.dumps(result, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
