"""The field-evaluated frame front to back in rank windows against the default route of the same
build, on bench.py's scene: the 983 040-triangle shell mesh, 800 x 800, K = 25, T = 2^19, the seeded field, fp32.

    python tools/field_front_bench.py [--views 4] [--warmup 2] [--repeats 3] [--passes 10]
                                      [--out profiles/field_front/field_front_bench.json]
    python tools/field_front_bench.py --trace-only      # a few frames of each route, for a kernel trace of their launches

Two scenes, the same mesh, views and field:
  a  render_step_size 5e-3 (bench.py's): the seeded field is thin, no ray ever stops -- the new route's overhead;
  b  render_step_size 0.5: the shells are opaque, the way the tests make them -- what termination saves.
Cases: the default ``render_async`` and the new route with eps = 1e-3 on every candidate schedule, all in ONE process.  A
repeat times every case once, in an order that rotates from repeat to repeat; a timing is the host clock around one pass
over the views (every frame enqueued, then one device synchronise), divided by the views; a repeat's figure is the median
over its passes.  Reported per case: the median of the repeat medians and their spread (max - min), the share of hit rays
that stop early and the share of the frame's samples that the field evaluated.  Untimed, first: eps = 0 gives the default
route's pixels bit for bit, and eps = 1e-3 stays within 3 eps of them.

The window list reaches the field kernel through its ``order`` argument (outputs land in place); the alternative of the
issue, streamed copies of the positions and directions per window, is not built, so it is not timed here.
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import bench

EPS = 1e-3
K = bench.MAX_HITS
SCHEDULES = {"(K)": (K,), "(4,K)": (4, K), "(2,6,K)": (2, 6, K), "(1,3,7,15,K)": (1, 3, 7, 15, K)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("field_front_bench.py: no HIP device (timings are only taken on the GPU)")
    torch.set_grad_enabled(False)
    warnings.simplefilter("ignore")
    from quadraturefields_amd import synthetic
    from quadraturefields_amd.mesh_utils import make_camera
    from quadraturefields_amd.render import FrameRenderer

    dev = torch.device("cuda:0")
    _mesh, mi, field = bench.build_scene(dev)
    ri = mi.rayintersector
    cams = synthetic.orbit_cameras(args.views + args.warmup, seed=42)
    focal = synthetic.lego_focal(bench.W)
    frames = [synthetic.camera_rays(c, focal, bench.W, bench.H, device=dev) + (make_camera(c, focal, bench.W, bench.H),)
              for c in cams]
    warm, timed = frames[:args.warmup], frames[args.warmup:]
    cases = [("default", None)] + [(name, w) for name, w in SCHEDULES.items()]

    def run(fr, windows, views, eps=EPS):
        out = None
        for o, d, cam in views:
            out = fr.render_async(o, d, cam) if windows is None else \
                fr.render_async(o, d, cam, early_stop_eps=eps, rank_windows=windows)
        return out

    if args.trace_only:
        for step in (bench.STEP, 0.5):
            mi.render_step_size = step
            fr = FrameRenderer(mi, field)
            for _name, windows in cases:
                run(fr, windows, frames)
        torch.cuda.synchronize()
        ri._settle_fused_policy(0)
        return

    result = {"workload": f"bench scene: {bench.W}x{bench.H}, K={K}, fp32 field, {args.views} orbit views after {args.warmup} "
                          f"warm-up views, {args.repeats} repeats of {args.passes} passes per case in rotating order; host "
                          "clock around a pass that ends in a device synchronise, per frame",
              "eps": EPS, "field_feed": "order list (qf_field_forward's order / n_device); streamed copies not built",
              "scenes": {}}
    for scene, step in (("a_step_5e-3", bench.STEP), ("b_step_0.5", 0.5)):
        mi.render_step_size = step
        fr = FrameRenderer(mi, field)
        # untimed: eps = 0 is the default route bit for bit; eps = 1e-3 stays within 3 eps; the shares
        share = {}
        for name, windows in cases[1:]:
            stop = hit = evaluated = total = 0
            worst = 0.0
            for view in timed:
                ref = run(fr, None, [view])
                zero = run(fr, windows, [view], eps=0.0)
                for a, b in zip(zero[:3], ref[:3]):
                    if not torch.equal(a, b):
                        sys.exit(f"field_front_bench.py: scene {scene} schedule {name}: eps 0 is not the default route's frame")
                rgb, _, _, frame = run(fr, windows, [view])
                worst = max(worst, float((rgb - ref[0]).abs().max()))
                hit += int((frame.hit_count > 0).sum())
                stop += int((frame.shaded_count < frame.hit_count).sum())
                total += int(frame.hit_count.sum())
                evaluated += int(frame.evaluated_count.sum())
            if worst > 3 * EPS:
                sys.exit(f"field_front_bench.py: scene {scene} schedule {name} moved a pixel by {worst} > 3 eps")
            share[name] = {"rays_stopping_share": stop / max(hit, 1), "evaluated_share": evaluated / max(total, 1),
                           "max_pixel_change_vs_default": worst}
        for _name, windows in cases:
            run(fr, windows, warm)
            run(fr, windows, timed)
        torch.cuda.synchronize()
        medians = {name: [] for name, _ in cases}
        for r in range(args.repeats):
            order = cases[r % len(cases):] + cases[:r % len(cases)]
            for name, windows in order:
                per_pass = []
                for _ in range(args.passes):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    run(fr, windows, timed)
                    torch.cuda.synchronize()
                    per_pass.append((time.perf_counter() - t0) * 1e3 / len(timed))
                medians[name].append(statistics.median(per_pass))
        ri._settle_fused_policy(0)
        rows = {}
        for name, _ in cases:
            m = medians[name]
            rows[name] = {"median_ms_per_frame": statistics.median(m), "spread_ms": max(m) - min(m), "repeat_medians_ms": m}
            rows[name].update(share.get(name, {}))
        base = rows["default"]
        best = min((n for n, _ in cases[1:]), key=lambda n: rows[n]["median_ms_per_frame"])
        gain = base["median_ms_per_frame"] - rows[best]["median_ms_per_frame"]
        spread = max(base["spread_ms"], rows[best]["spread_ms"])
        result["scenes"][scene] = {"render_step_size": step, "route": ri.last_route, "cases": rows, "fastest_schedule": best,
                                   "gain_ms_vs_default": gain, "spread_ms": spread,
                                   "accepted": bool(gain > 2 * spread) if scene.startswith("b") else None}
        print(f"{scene}: " + ", ".join(f"{n} {rows[n]['median_ms_per_frame']:.3f} ms (spread {rows[n]['spread_ms']:.3f})"
                                       + (f" evaluated {rows[n]['evaluated_share']:.3f}" if n in share else "")
                                       for n, _ in cases), flush=True)
    text = json.dumps(result, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
