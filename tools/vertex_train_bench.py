"""The backward of the vertex shading on bench.py's scene: 983 040 triangles, 491 544 vertices,
K = 25, a seeded 6-lobe SG field baked at the vertices.

    python tools/vertex_train_bench.py [--repeats 7] [--warmup 2] [--out profiles/vertex_train/vertex_train_bench.json]

Two sample sets: ``batch`` = the ray-major samples of 2^17 random rays drawn from four 800 x 800 orbit frames (a training
batch), ``frame`` = the ray-major samples of one whole 800 x 800 frame.  On each, in ONE process, repeats in rotating
order, device events around every call, median [min, max]:

  fused     qf_vertex_shade_points_backward on the 6-lobe table (the zero fill of the gradient is timed apart)
  fused1/8  the same kernel on random 1- and 8-lobe tables (64-byte and 240-byte row segments)
  torch     the same gradient from what exists without the kernel: three row gathers, the blend,
            NGPRadianceFieldSGNew.features_to_rgb's differentiable route (qf_sg_features_to_rgb and its backward), three
            index_add_ calls over [n, W] products -- forward and backward timed apart
Reported with the fused times: the added bytes (3 W 4 per sample) per second beside the ~1.3 TB/s the memory side takes
float atomics at, and the largest difference between the two gradients relative to each column's largest entry.  Then
one fine-tuning step on ``batch`` end to end, split into intersection, forward, backward and Adam.
"""
import argparse
import json
import os
import statistics
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench

ATOMIC_RATE_TBS = 1.3


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def _stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "repeats_ms": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch-rays", type=int, default=1 << 17)
    ap.add_argument("--shells", type=int, default=None, help="default: the bench scene's")
    ap.add_argument("--subdivisions", type=int, default=None)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("vertex_train_bench.py: no HIP device (timings are only taken on the GPU)")
    warnings.simplefilter("ignore")
    from quadraturefields_amd import _C, baking, synthetic, utils
    from quadraturefields_amd.datasets.utils import Rays
    from quadraturefields_amd.mesh_utils import make_camera
    from quadraturefields_amd.optim import Adam
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceFieldSGNew

    dev = torch.device("cuda:0")
    lobes = 6
    mesh, mi, _ngp = bench.build_scene(dev, n_shells=args.shells, subdiv=args.subdivisions)
    del _ngp
    sg = NGPRadianceFieldSGNew(aabb=[-1.5] * 3 + [1.5] * 3, use_viewdirs=False, num_g_lobes=lobes, log2_hashmap_size=bench.LOG2_T)
    sg.load_state_dict(synthetic.seeded_ngp_state(bench.LOG2_T, sg.mlp_base.grid.n_rows, sg_lobes=lobes), strict=False)
    sg = sg.to(dev).eval()
    n_vertices = int(mesh.vertices.shape[0])
    gen = torch.Generator().manual_seed(7)
    with torch.no_grad():
        modules = {lobes: baking.VertexBakedFeatures.from_field(sg, mi)}
        for l in (1, 8):
            t = torch.randn(n_vertices, 3 + 7 * l + 1, generator=gen)
            t[:, -1] = t[:, -1].abs() * 10.0
            modules[l] = baking.VertexBakedFeatures(t, device=dev)
        faces = utils._faces_on_device(mi)
        v64 = torch.from_numpy(np.ascontiguousarray(mesh.vertices, dtype=np.float64)).to(dev)
        focal = synthetic.lego_focal(bench.W)
        views = [synthetic.camera_rays(c, focal, bench.W, bench.H, device=dev) + (make_camera(c, focal, bench.W, bench.H),)
                 for c in synthetic.orbit_cameras(4, seed=42)]
        all_o, all_d = torch.cat([v[0] for v in views]), torch.cat([v[1] for v in views])
        pick = torch.randint(0, all_o.shape[0], (args.batch_rays,), generator=gen).to(dev)
        batch_o, batch_d = all_o[pick].contiguous(), all_d[pick].contiguous()
        sets = {"batch": mi.sampling_raytrace_device(batch_d, batch_o, layout=False),
                "frame": mi.sampling_raytrace_device(views[0][1], views[0][0], camera=views[0][2], layout=False)}

    result = {"device": torch.cuda.get_device_name(0),
              "workload": f"bench scene: {int(mesh.faces.shape[0])} triangles, {n_vertices} vertices, K={bench.MAX_HITS}, L={lobes}; "
                          f"batch = {args.batch_rays} random rays of four {bench.W}x{bench.H} orbit frames, frame = one whole frame, "
                          f"ray-major; {args.repeats} repeats in rotating order after {args.warmup} warm-up rounds, one process",
              "atomic_rate_reference_tbs": ATOMIC_RATE_TBS, "sets": {}}

    for name, data in sets.items():
        points, dirs, tri = _C.f32c(data[0]), _C.f32c(data[1]), _C.i64c(data[4])
        n = int(points.shape[0])
        d_rgb = torch.randn(n, 3, generator=gen).to(dev)
        d_sigma = torch.randn(n, generator=gen).to(dev)
        grads = {l: torch.empty_like(m.table) for l, m in modules.items()}

        def fused(l):
            m = modules[l]
            table, records = utils.vertex_baked_shading(mi, m)
            _C.check(_C.lib().qf_vertex_shade_points_backward(
                _C.ptr(table), table.shape[1], l, _C.ptr(records), table.shape[0], _C.ptr(points), _C.ptr(tri), None,
                _C.ptr(dirs), n, None, _C.ptr(d_rgb), _C.ptr(d_sigma), _C.ptr(grads[l]), _C.stream()),
                "qf_vertex_shade_points_backward")

        def fused_forward():
            with torch.no_grad():
                return utils.shade_vertex_baked_points(mi, modules[lobes], points, tri, dirs)

        # the torch composition: barycentrics once, outside the timing (fp64 Cramer, cast to fp32, as the reference)
        with torch.no_grad():
            corners = v64[faces[tri]]
            e0, e1, e2 = corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0], points.double() - corners[:, 0]
            d00, d01, d11 = (e0 * e0).sum(1), (e0 * e1).sum(1), (e1 * e1).sum(1)
            d20, d21 = (e2 * e0).sum(1), (e2 * e1).sum(1)
            inv = 1.0 / (d00 * d11 - d01 * d01)
            b1, b2 = (d11 * d20 - d01 * d21) * inv, (d00 * d21 - d01 * d20) * inv
            bary = torch.stack([1.0 - b1 - b2, b1, b2], dim=1).float()
            f0, f1, f2 = (faces[tri][:, k].contiguous() for k in range(3))
            del corners, e0, e1, e2
        feats = modules[lobes].features().contiguous()
        state = {}

        def torch_forward():
            with torch.no_grad():
                blend = (feats[f0] * bary[:, 0:1] + feats[f1] * bary[:, 1:2]) + feats[f2] * bary[:, 2:3]
            blend.requires_grad_(True)
            with torch.enable_grad():
                state["rgb"] = sg.features_to_rgb(blend, dirs)
            state["blend"] = blend
            return state["rgb"]

        def torch_backward():
            d_blend, = torch.autograd.grad(state["rgb"], state["blend"], d_rgb)
            with torch.no_grad():
                d_blend[:, -1] += d_sigma
                grad = torch.zeros_like(feats)
                grad.index_add_(0, f0, d_blend * bary[:, 0:1])
                grad.index_add_(0, f1, d_blend * bary[:, 1:2])
                grad.index_add_(0, f2, d_blend * bary[:, 2:3])
            return grad

        def zero():
            grads[lobes].zero_()

        def run(case):
            if case == "torch":
                fwd, _ = _timed(torch_forward)
                bwd, g = _timed(torch_backward)
                state.clear()
                return {"torch_forward": fwd, "torch_backward": bwd}, g
            if case == "fused":
                z, _ = _timed(zero)
                fwd, _ = _timed(fused_forward)
                bwd, _ = _timed(lambda: fused(lobes))
                return {"fused_zero_fill": z, "fused_forward": fwd, "fused": bwd}, None
            l = int(case[5:])
            grads[l].zero_()
            return {case: _timed(lambda: fused(l))[0]}, None

        cases = ["fused", "torch", "fused1", "fused8"]
        for _ in range(args.warmup):
            for c in cases:
                run(c)
        # the two gradients: largest difference relative to each column's largest entry
        zero()
        fused(lobes)
        _, g_torch = run("torch")
        w = feats.shape[1]
        scale = g_torch.abs().amax(dim=0)
        diff = float(((grads[lobes][:, :w] - g_torch).abs().amax(dim=0) / scale).max())
        del g_torch
        times = {}
        for r in range(args.repeats):
            order = cases[r % len(cases):] + cases[:r % len(cases)]
            for c in order:
                for k, ms in run(c)[0].items():
                    times.setdefault(k, []).append(ms)
        torch.cuda.synchronize()
        res = {k: _stats(v) for k, v in times.items()}
        for key, l in (("fused", lobes), ("fused1", 1), ("fused8", 8)):
            added = n * 3 * (3 + 7 * l + 1) * 4
            res[key]["added_bytes"] = added
            res[key]["row_segment_bytes"] = (3 + 7 * l + 1) * 4
            res[key]["added_tb_per_s"] = added / (res[key]["median_ms"] * 1e-3) / 1e12
        f, t = res["fused"], res["torch_backward"]
        spread = (f["max_ms"] - f["min_ms"]) + (t["max_ms"] - t["min_ms"])
        res["samples"] = n
        res["max_column_relative_difference"] = diff
        res["bar"] = {"gap_ms": t["median_ms"] - f["median_ms"], "combined_spread_ms": spread,
                      "fused_faster_by_more_than_the_spread": bool(t["median_ms"] - f["median_ms"] > spread)}
        result["sets"][name] = res
        print(f"{name}: {n} samples; fused {f['median_ms']:.3f} ms [{f['min_ms']:.3f}, {f['max_ms']:.3f}] = "
              f"{f['added_tb_per_s']:.3f} TB/s added; torch backward {t['median_ms']:.3f} ms [{t['min_ms']:.3f}, {t['max_ms']:.3f}] "
              f"(+ forward {res['torch_forward']['median_ms']:.3f}); 1 lobe {res['fused1']['median_ms']:.3f} ms = "
              f"{res['fused1']['added_tb_per_s']:.3f} TB/s, 8 lobes {res['fused8']['median_ms']:.3f} ms = "
              f"{res['fused8']['added_tb_per_s']:.3f} TB/s; gradients differ by {diff:.2e}", flush=True)

    # one fine-tuning step on the batch, end to end
    module = modules[lobes]
    module.table.requires_grad_(True)
    module.train_density = False
    optimizer = Adam([module.table], lr=1e-3, eps=1e-15)
    rays = Rays(origins=batch_o, viewdirs=batch_d)
    target = torch.rand(args.batch_rays, 3, generator=gen).to(dev)
    parts = {"intersection": [], "forward": [], "backward": [], "adam": []}
    for r in range(args.repeats + args.warmup):
        ms_i, data = _timed(lambda: mi.sampling_raytrace_device(batch_d, batch_o, layout=False))

        def forward():
            rgb = utils.render_image_finetune_baking_with_occgrid(None, None, rays, data, mesh_intersect=mi,
                                                                  vertex_features=module)[0]
            return torch.nn.functional.smooth_l1_loss(rgb, target)

        ms_f, loss = _timed(forward)
        optimizer.zero_grad(set_to_none=True)
        ms_b, _ = _timed(loss.backward)
        ms_a, _ = _timed(optimizer.step)
        if r >= args.warmup:
            for k, ms in zip(parts, (ms_i, ms_f, ms_b, ms_a)):
                parts[k].append(ms)
    step = {k: _stats(v) for k, v in parts.items()}
    step["total_median_ms"] = sum(s["median_ms"] for s in step.values())
    result["step"] = step
    print("step: " + ", ".join(f"{k} {v['median_ms']:.3f} ms" for k, v in step.items() if isinstance(v, dict))
          + f"; total {step['total_median_ms']:.3f} ms", flush=True)
    text = json.dumps(result, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
