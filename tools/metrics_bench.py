"""What scoring an evaluation frame costs: ``metrics.FrameScorer`` against what a user does today, in ONE process.

    python tools/metrics_bench.py [--frames 300] [--repeats 5] [--loop-frames 8] [--out profiles/r5/frame_metrics.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/metrics_bench.py --profile-run      # kernel times, separately

At 800x800 ground truth, up_sample 1 and 2, after warm-up of every shape, the routes alternating inside every repeat,
synchronised host timing per block of ``--frames`` frames (median, min and max over the repeats are reported):

1. ``scorer``: ``FrameScorer.score(rgb, pixels, depth, images=True)`` back to back, one ``results()`` at the end.
2. ``today``: ``render.area_downsample`` + ``F.mse_loss`` + the fp32 ``conv2d`` SSIM of tests/frame_metrics_reference.py on
   the device + clamp / error / depth images, with three ``.item()`` per frame (PSNR, SSIM and, standing in for LPIPS'
   wait, the depth maximum); ``today_roundtrip``: the same with the device -> host -> device trip of the full-resolution
   frame that ``cv2.resize`` forces (the host resize is torch's mean here: cv2 is not a dependency).
3. ``loop``: the reference-shaped evaluation loop of bench.py's ``reference_route`` (loader item -> ``generate_splits``
   windows -> ``render_image_finetune_with_occgrid`` per window -> assembly), restated: bare, with the scorer, and with
   route 2 after every frame.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch
import torch.nn.functional as F

H = W = 800
HBM_PEAK_GBS = 8000.0            # HBM3E spec rate of the MI355X


def today(rgb_full, depth_full, pixels, f, roundtrip, ref):
    """train_finetune.py:620-646 with torch ops; returns what the scripts keep."""
    from quadraturefields_amd.render import area_downsample
    if roundtrip:
        rgb = area_downsample(rgb_full.cpu(), f).cuda()
        depth = area_downsample(depth_full.cpu(), f).cuda()
    else:
        rgb, depth = area_downsample(rgb_full, f), area_downsample(depth_full, f)
    mse = F.mse_loss(rgb, pixels)
    psnr = -10.0 * torch.log(mse) / np.log(10.0)
    ssim = ref.ssim_windows(rgb.permute(2, 0, 1).unsqueeze(0), pixels.permute(2, 0, 1).unsqueeze(0)).mean()
    out = (psnr.item(), ssim.item())
    rgb = torch.clamp(rgb, 0, 1)
    error = torch.clamp(torch.abs(rgb - pixels), 0, 1)
    dmax = depth.max()
    depth = depth / dmax
    images = ((rgb * 255).to(torch.uint8), (error * 255).to(torch.uint8), (depth * 255).to(torch.uint8))
    return out + (dmax.item(),), images


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "runs": ms}


def timed(fn, frames):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(frames):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / frames * 1e3


def standalone(device, ref, frames, repeats):
    from quadraturefields_amd.metrics import FrameScorer
    g = torch.Generator(device=device).manual_seed(0)
    out = {}
    for f in (1, 2):
        pixels = torch.rand(H, W, 3, generator=g, device=device)
        inputs = []
        for _ in range(4):
            small = (pixels + 0.05 * torch.randn(H, W, 3, generator=g, device=device))
            rgb = small.repeat_interleave(f, 0).repeat_interleave(f, 1).contiguous()
            inputs.append((rgb, torch.rand(H * f, W * f, generator=g, device=device) * 4.0))
        scorer = FrameScorer(H, W, up_sample=f, capacity=frames, device=device)

        def run_scorer(i):
            if i == 0:
                scorer.reset()
            scorer.score(inputs[i % 4][0], pixels, depth=inputs[i % 4][1], images=True)
            if i == frames - 1:
                scorer.results()

        routes = {"scorer": run_scorer,
                  "today": lambda i: today(inputs[i % 4][0], inputs[i % 4][1], pixels, f, False, ref),
                  "today_roundtrip": lambda i: today(inputs[i % 4][0], inputs[i % 4][1], pixels, f, True, ref)}
        for fn in routes.values():                      # warm-up of every shape
            timed(fn, frames if fn is run_scorer else 5)
        ms = {k: [] for k in routes}
        for _ in range(repeats):
            for k, fn in routes.items():
                ms[k].append(timed(fn, frames))
        res = {k: summary(v) for k, v in ms.items()}
        # the same frame by both routes: the numbers that are being paid for
        scorer.reset()
        scorer.score(inputs[0][0], pixels, depth=inputs[0][1], images=True)
        r = scorer.results()
        t = today(inputs[0][0], inputs[0][1], pixels, f, False, ref)[0]
        res["same_frame"] = {"scorer": {"psnr": r["psnr"][0], "ssim": r["ssim"][0]}, "today": {"psnr": t[0], "ssim": t[1]}}
        res["tile_kernel_bytes"] = 4 * 3 * H * W * (f * f + 1) + 4 * H * W * f * f + 4 * 3 * H * W + 4 * H * W
        out[f"up_sample_{f}"] = res
    return out


def eval_loop(device, ref, loop_frames, repeats):
    """bench.py's reference_route finetune loop (scaling 0), restated, at up_sample 1 and 2."""
    import bench
    from quadraturefields_amd import synthetic, utils
    from quadraturefields_amd.datasets.nerf_synthetic import SubjectLoader
    from quadraturefields_amd.field import Field
    from quadraturefields_amd.mesh_utils import MeshFinetune
    from quadraturefields_amd.metrics import FrameScorer
    scene = bench.build_scene(device)
    mesh, mi, field = scene
    n = 6
    cams = np.stack([np.asarray(c, dtype=np.float32) for c in synthetic.orbit_cameras(n, seed=42)])
    images = np.zeros((n, H, W, 4), dtype=np.uint8)
    field_net = Field(scale=1.5, precision=16, log2_T=24, L=16, max_res=512, min_res=16, output_dim=1, hidden_size=32,
                      num_features=2, back_prop=False, nl="relu").to(device)
    mesh_finetune = MeshFinetune(mi.mesh.vertices, mi.mesh.faces, 0.0434, device=device)
    out = {}
    for f in (1, 2):
        ds = SubjectLoader.from_arrays(images, cams, synthetic.lego_focal(W), split="test", mesh_intersect=mi, device=device,
                                       upsample=f)
        pixels = torch.rand(H, W, 3, device=device)
        scorer = FrameScorer(H, W, up_sample=f, capacity=loop_frames, device=device)

        def frame(i):
            item = ds[i % n]
            rays = item["rays"]
            n_rays = rays.origins.shape[0]
            rgb = torch.ones((n_rays, 3), device=device)
            depth = torch.zeros((n_rays,), device=device)
            for split in utils.generate_splits(item["data"], n_rays):
                color, _, d, *_ = utils.render_image_finetune_with_occgrid(
                    field, field_net, None, rays, split, near_plane=0.0, render_step_size=bench.STEP,
                    render_bkgd=item["color_bkgd"], cone_angle=0.0, alpha_thre=0.0, mesh_intersect=mi,
                    mesh_finetune=mesh_finetune, scaling=0.0)
                rgb[split[2]] = color[split[2]]
                depth[split[2]] = d.squeeze()[split[2]]
            return rgb, depth

        def with_scorer(i):
            if i == 0:
                scorer.reset()
            rgb, depth = frame(i)
            scorer.score(rgb, pixels, depth=depth, images=True)
            if i == loop_frames - 1:
                scorer.results()

        def with_today(i):
            rgb, depth = frame(i)
            today(rgb.reshape(H * f, W * f, 3), depth.reshape(H * f, W * f), pixels, f, False, ref)

        def with_today_roundtrip(i):
            rgb, depth = frame(i)
            today(rgb.reshape(H * f, W * f, 3), depth.reshape(H * f, W * f), pixels, f, True, ref)

        routes = {"bare": frame, "with_scorer": with_scorer, "with_today": with_today,
                  "with_today_roundtrip": with_today_roundtrip}
        for fn in routes.values():
            timed(fn, loop_frames if fn is with_scorer else 2)
        ms = {k: [] for k in routes}
        for _ in range(repeats):
            for k, fn in routes.items():
                ms[k].append(timed(fn, loop_frames))
        res = {k: summary(v) for k, v in ms.items()}
        bare = res["bare"]["median_ms"]
        res["added_ms"] = {k: res[k]["median_ms"] - bare for k in routes if k != "bare"}
        out[f"up_sample_{f}"] = res
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loop-frames", type=int, default=8, help="frames per timed block of the evaluation loop (0: skip it)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-run", action="store_true", help="only 50 scored frames per factor, for a kernel trace")
    args = ap.parse_args(argv)
    from tests import frame_metrics_reference as ref
    device = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    if args.profile_run:
        standalone_profile(device)
        return
    result = {"what": "tools/metrics_bench.py: ms per frame, 800x800 ground truth; median / min / max over the repeats of "
                      "synchronised host timing per block of frames, routes alternating in one process",
              "frames_per_block": args.frames, "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
              "standalone": standalone(device, ref, args.frames, args.repeats)}
    if args.loop_frames > 0:
        result["eval_loop"] = dict(eval_loop(device, ref, args.loop_frames, max(3, args.repeats // 2)),
                                   frames_per_block=args.loop_frames)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


def standalone_profile(device):
    from quadraturefields_amd.metrics import FrameScorer
    for f in (1, 2):
        pixels = torch.rand(H, W, 3, device=device)
        rgb, depth = torch.rand(H * f, W * f, 3, device=device), torch.rand(H * f, W * f, device=device)
        scorer = FrameScorer(H, W, up_sample=f, capacity=64, device=device)
        for _ in range(50):
            scorer.score(rgb, pixels, depth=depth, images=True)
        scorer.results()


if __name__ == "__main__":
    main()
