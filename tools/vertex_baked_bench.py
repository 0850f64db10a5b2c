"""The vertex-baked frame against the baked-texture frame, on bench.py's scene: 800 x 800 orbit
frames of the bench mesh (983 040 triangles, 491 544 vertices), K = 25, a seeded 6-lobe SG field.

    python tools/vertex_baked_bench.py [--frames 6] [--warmup 2] [--repeats 5] [--texture-size 4096]
                                       [--out profiles/vertex_baked/vertex_baked_bench.json]

  v   FrameRenderer.render_vertex_baked(camera=)                      shade every sample, composite (two launches)
  v0  ... early_stop_eps = 0                                          one launch front to back, never stops: v's pixels
  v3  ... early_stop_eps = 1e-3
  t   FrameRenderer.render_baked(camera=) on the texture_size^2 set   the texture route (two launches)
The vertex table is ``baking.bake_vertex_features`` of the SG field; the texture set is ``baking.bake_texture_set`` of the
same field (colour features AND density) over ``uv_atlas.per_triangle_atlas`` of the same mesh, linear colour codec.  All
four cases run in ONE process; a repeat times every case once over the same frames, in an order that rotates from repeat
to repeat, with device events around the case's frames (every call ends in the renderer's one host wait for the sample
count, the same in all four).  Reported per case: the median over the repeats of the time per frame and the spread (min,
max); the share of the samples shaded; and the PSNR of the case's frames against the SG field's own frames
(``FrameRenderer.render`` on the same mesh), mean over the timed frames -- what each asset costs in quality.
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

CASES = ["v", "v0", "v3", "t"]
EPS = {"v": None, "v0": 0.0, "v3": 1e-3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--texture-size", type=int, default=4096)
    ap.add_argument("--lobes", type=int, default=6)
    ap.add_argument("--shells", type=int, default=None, help="default: the bench scene's")
    ap.add_argument("--subdivisions", type=int, default=None)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("vertex_baked_bench.py: no HIP device (timings are only taken on the GPU)")
    torch.set_grad_enabled(False)
    warnings.simplefilter("ignore")
    from quadraturefields_amd import baking, synthetic, uv_atlas
    from quadraturefields_amd.mesh_utils import MeshIntersection, make_camera
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceFieldSGNew
    from quadraturefields_amd.render import FrameRenderer, psnr
    from quadraturefields_amd.texture_utils import FeatureCompression

    dev = torch.device("cuda:0")
    size, lobes = args.texture_size, args.lobes
    mesh, mi, _ngp = bench.build_scene(dev, n_shells=args.shells, subdiv=args.subdivisions)
    del _ngp
    sg = NGPRadianceFieldSGNew(aabb=[-1.5] * 3 + [1.5] * 3, use_viewdirs=False, num_g_lobes=lobes, log2_hashmap_size=bench.LOG2_T)
    sg.load_state_dict(synthetic.seeded_ngp_state(bench.LOG2_T, sg.mlp_base.grid.n_rows, sg_lobes=lobes), strict=False)
    sg = sg.to(dev).eval()
    # the two assets of the same field
    features = baking.bake_vertex_features(sg, mi)
    mesh_uv, _ = uv_atlas.per_triangle_atlas(mesh, size)
    V, _ = baking.texel_positions(mesh_uv, size, untouched="last_face")
    comp = FeatureCompression(lobes, initialize=True, texture_size=size, compression_type="linear", device=dev)
    baking.bake_texture_set(sg, sg, V, comp)
    comp.records()
    del V
    mi_uv = MeshIntersection(mesh_uv, simplify_mesh=False, scale=1.0, num_intersections=bench.MAX_HITS,
                             render_step_size=bench.STEP, device=dev)
    uv = torch.from_numpy(synthetic.scaled_uv(mesh_uv, size)).to(dev)
    fr_v = FrameRenderer(mi, sg, render_step_size=bench.STEP)
    fr_t = FrameRenderer(mi_uv, None, render_step_size=bench.STEP)

    n_frames = args.frames + args.warmup
    cams = synthetic.orbit_cameras(n_frames, seed=42)
    focal = synthetic.lego_focal(bench.W)
    frames = [synthetic.camera_rays(c, focal, bench.W, bench.H, device=dev) + (make_camera(c, focal, bench.W, bench.H),)
              for c in cams]
    warm, timed = frames[:args.warmup], frames[args.warmup:]

    def render(case, view):
        o, d, cam = view
        if case == "t":
            return fr_t.render_baked(o, d, uv, comp, camera=cam)
        return fr_v.render_vertex_baked(o, d, features, camera=cam, early_stop_eps=EPS[case])

    # untimed: quality against the field's own frame, the share of samples shaded, v0 == v
    quality, share, samples = {c: [] for c in CASES}, {}, {}
    for case in CASES:
        shaded = total = 0
        for view in timed:
            truth = fr_v.render(view[0], view[1], camera=view[2])[0]
            rgb, _, _, n = render(case, view)
            quality[case].append(float(psnr(rgb, truth)))
            total += n
            if EPS.get(case) is not None:
                shaded += int(mi.rayintersector.last_frame.shaded_count.sum())
                if case == "v0" and not torch.equal(rgb, render("v", view)[0]):
                    sys.exit("vertex_baked_bench.py: eps 0 does not give the default route's pixels")
            else:
                shaded += n
        share[case], samples[case] = shaded / max(total, 1), total / len(timed)
    for case in CASES:
        for view in warm:
            render(case, view)
    torch.cuda.synchronize()
    times = {c: [] for c in CASES}
    for r in range(args.repeats):
        order = CASES[r % len(CASES):] + CASES[:r % len(CASES)]
        for case in order:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for view in timed:
                render(case, view)
            b.record()
            b.synchronize()
            times[case].append(a.elapsed_time(b) / len(timed))
    width = features.shape[1]
    result = {
        "device": torch.cuda.get_device_name(0),
        "workload": f"bench scene: {int(mesh.faces.shape[0])} triangles, {int(mesh.vertices.shape[0])} vertices, {bench.W}x{bench.H}, "
                    f"K={bench.MAX_HITS}, L={lobes}, {args.frames} orbit frames per case and repeat, {args.repeats} repeats in "
                    "rotating order, one process",
        "cases": {"v": "render_vertex_baked (two launches)", "v0": "vertex-baked front to back, eps 0",
                  "v3": "vertex-baked front to back, eps 1e-3", "t": f"render_baked on the {size}^2 texture set (two launches)"},
        "vertex_table_bytes": int(features.shape[0]) * 4 * (16 * ((width + 15) // 16)),
        "vertex_records_bytes": int(mesh.faces.shape[0]) * 128,
        "texture_records_bytes": size * size * 64, "texture_triangle_records_bytes": int(mesh_uv.faces.shape[0]) * 128,
        "psnr_reference": "FrameRenderer.render of the same SG field on the same mesh (fp32), mean over the timed frames",
        "results": {c: {"median_ms_per_frame": statistics.median(times[c]), "min_ms": min(times[c]), "max_ms": max(times[c]),
                        "repeats_ms": times[c], "samples_per_frame": samples[c], "shaded_share": share[c],
                        "psnr_vs_field_db": statistics.mean(quality[c]), "psnr_per_frame_db": quality[c]} for c in CASES}}
    for c in CASES:
        r = result["results"][c]
        print(f"{c}: {r['median_ms_per_frame']:.3f} ms [{r['min_ms']:.3f}, {r['max_ms']:.3f}]  shaded {r['shaded_share']:.3f}  "
              f"PSNR vs field {r['psnr_vs_field_db']:.2f} dB", flush=True)
    text = json.dumps(result, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
