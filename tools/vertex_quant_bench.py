"""The quantised vertex-baked frame against the fp32 vertex frame and the texture frame, on
bench.py's scene: 800 x 800 orbit frames of the bench mesh (983 040 triangles, 491 544 vertices), K = 25, a seeded 6-lobe
SG field.

    python tools/vertex_quant_bench.py [--frames 6] [--warmup 2] [--repeats 5] [--texture-size 4096]
                                       [--out profiles/vertex_quant/vertex_quant_bench.json]

  t   FrameRenderer.render_baked(camera=) on the texture_size^2 set   the texture route (two launches)
  v   FrameRenderer.render_vertex_baked(camera=), fp32 table          shade every sample, composite (two launches)
  v0  ... early_stop_eps = 0                                          one launch front to back, never stops: v's pixels
  v3  ... early_stop_eps = 1e-3
  q   render_vertex_baked(camera=) on the QuantisedVertexFeatures     64-byte uint8 records, two launches
  q0  ... early_stop_eps = 0                                          one launch front to back: q's pixels
  q3  ... early_stop_eps = 1e-3
t, v, v0 and v3 are ``tools/vertex_baked_bench.py``'s cases, unchanged: the baseline of the same run.  The quantised table
is ``baking.quantise_vertex_features`` of the fp32 table (linear colour codec).  All cases run in ONE process; a repeat
times every case once over the same frames, in an order that rotates from repeat to repeat, with device events around the
case's frames.  Reported per case: the median over the repeats of the time per frame and the spread (min, max); the share
of the samples shaded; the PSNR against the SG field's own frames and, for the q cases, against the v frames; the bytes
each asset keeps resident and takes on disk (the fp32 table as ``.npy``, the quantised one as its PNG set, written to a
temporary directory and measured).
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench

CASES = ["t", "v", "v0", "v3", "q", "q0", "q3"]
EPS = {"v": None, "v0": 0.0, "v3": 1e-3, "q": None, "q0": 0.0, "q3": 1e-3}


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
        sys.exit("vertex_quant_bench.py: no HIP device (timings are only taken on the GPU)")
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
    # the three assets of the same field
    features = baking.bake_vertex_features(sg, mi)
    quantised = baking.quantise_vertex_features(features, compression_type="linear")
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
    with tempfile.TemporaryDirectory() as tmp:
        np.save(os.path.join(tmp, "vertex_features.npy"), features.cpu().numpy())
        npy_bytes = os.path.getsize(os.path.join(tmp, "vertex_features.npy"))
        quantised.save(os.path.join(tmp, "vq_"))
        png_bytes = sum(os.path.getsize(os.path.join(tmp, f)) for f in os.listdir(tmp) if f.endswith(".png"))

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
        return fr_v.render_vertex_baked(o, d, quantised if case[0] == "q" else features, camera=cam, early_stop_eps=EPS[case])

    # untimed: quality against the field's own frame (and, for q, the v frame), the share of samples shaded, eps 0 == default
    quality, vs_v, share, samples = {c: [] for c in CASES}, {c: [] for c in CASES if c[0] == "q"}, {}, {}
    for case in CASES:
        shaded = total = 0
        for view in timed:
            truth = fr_v.render(view[0], view[1], camera=view[2])[0]
            rgb, _, _, n = render(case, view)
            quality[case].append(float(psnr(rgb, truth)))
            total += n
            if EPS.get(case) is not None:
                shaded += int(mi.rayintersector.last_frame.shaded_count.sum())
                if EPS[case] == 0.0 and not torch.equal(rgb, render(case[0], view)[0]):
                    sys.exit(f"vertex_quant_bench.py: {case}: eps 0 does not give the default route's pixels")
            else:
                shaded += n
            if case[0] == "q":
                vs_v[case].append(float(psnr(rgb, render("v" + case[1:], view)[0])))
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
    tri_bytes = int(mesh.faces.shape[0]) * 128
    resident = {"t": size * size * 64 + int(mesh_uv.faces.shape[0]) * 128,
                "v": int(features.shape[0]) * 4 * (16 * ((width + 15) // 16)) + tri_bytes,
                "q": int(quantised.records().numel()) + tri_bytes}
    disk = {"t": None, "v": npy_bytes, "q": png_bytes}
    result = {
        "device": torch.cuda.get_device_name(0),
        "workload": f"bench scene: {int(mesh.faces.shape[0])} triangles, {int(mesh.vertices.shape[0])} vertices, {bench.W}x{bench.H}, "
                    f"K={bench.MAX_HITS}, L={lobes}, {args.frames} orbit frames per case and repeat, {args.repeats} repeats in "
                    "rotating order, one process",
        "cases": {"t": f"render_baked on the {size}^2 texture set (two launches)", "v": "render_vertex_baked, fp32 table (two launches)",
                  "v0": "fp32 table front to back, eps 0", "v3": "fp32 table front to back, eps 1e-3",
                  "q": "render_vertex_baked, quantised table (two launches)", "q0": "quantised table front to back, eps 0",
                  "q3": "quantised table front to back, eps 1e-3"},
        "vertex_texture_size": int(quantised.compressor.texture_size),
        "bytes_resident": "the asset's table or records plus its 128-byte triangle records",
        "bytes_on_disk": "v: the [V, 3 + 7L + 1] fp32 .npy; q: the 2 + 2L uint8 PNGs; t: not written by this tool",
        "psnr_reference": "FrameRenderer.render of the same SG field on the same mesh (fp32), mean over the timed frames",
        "results": {c: {"median_ms_per_frame": statistics.median(times[c]), "min_ms": min(times[c]), "max_ms": max(times[c]),
                        "repeats_ms": times[c], "samples_per_frame": samples[c], "shaded_share": share[c],
                        "psnr_vs_field_db": statistics.mean(quality[c]), "psnr_per_frame_db": quality[c],
                        "psnr_vs_v_db": statistics.mean(vs_v[c]) if c in vs_v else None,
                        "bytes_resident": resident[c[0]], "bytes_on_disk": disk[c[0]]} for c in CASES}}
    for c in CASES:
        r = result["results"][c]
        extra = f"  PSNR vs v {r['psnr_vs_v_db']:.2f} dB" if r["psnr_vs_v_db"] is not None else ""
        print(f"{c}: {r['median_ms_per_frame']:.3f} ms [{r['min_ms']:.3f}, {r['max_ms']:.3f}]  shaded {r['shaded_share']:.3f}  "
              f"PSNR vs field {r['psnr_vs_field_db']:.2f} dB{extra}  resident {r['bytes_resident'] / 1e6:.1f} MB", flush=True)
    text = json.dumps(result, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
