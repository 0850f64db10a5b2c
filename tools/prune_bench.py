"""Pruning stage: time per training view of the four ways to get the per-triangle maxima.

    python tools/prune_bench.py [--size 1600] [--views 24] [--repeats 3] [--modes a,b,b_add_view,c,d] [--out FILE]

Bench scene (``synthetic.shell_mesh()``: 983 040 triangles; seeded NGP field, T = 2^19), K = 25, distinct orbit views.
  a           qf_frame_render alone (the frame the pruning rides on; job with triangle ids and an image)
  b           qf_frame_prune on the same job (image included, so that b - a is the cost of pruning on top of a frame)
  b_add_view  pruning.MeshPruner.add_view (qf_frame_prune without an image)
  c           the unfused device composition: qf_frame_render, a host read of the slot count, qf_composite_tiles with a
              weight array, an int64 copy of the ids, qf_scatter_max, the two counts
  d           the reference-shaped loop: sampling_raytrace_device -> render_image_finetune_with_occgrid(scaling=0) ->
              per-view host counts -> qf_scatter_max into zeros -> running torch.maximum
Every mode starts from zero maxima after a warm-up on other views (whose maxima are thrown away), so view 1 (nearly every
sample wins its atomic) and the steady state (the median of the views from ``--settle`` on: nearly every sample loses the
read-before-atomic comparison) are reported separately.  A view is timed with HIP events around its enqueue; the modes
are run ``--repeats`` times in alternation and the spread of a mode's steady state over the repeats is reported next to
it.  The maxima of b, b_add_view, c and d must be equal, bit for bit.  Kernel times: run the tool under
``rocprofv3 --kernel-trace --stats`` with ``--modes a,b --repeats 1``.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

K = 25
DELTA = 5e-3
VALID = 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1600)
    ap.add_argument("--views", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle", type=int, default=8, help="first view (1-based) of the steady-state window")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--modes", type=str, default="a,b,b_add_view,c,d")
    ap.add_argument("--log2_hashmap_size", type=int, default=19)
    ap.add_argument("--shells", type=int, default=12)
    ap.add_argument("--subdivisions", type=int, default=6)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("prune_bench.py: no HIP device (timings are only taken on the GPU)")
    torch.set_grad_enabled(False)
    warnings.simplefilter("ignore")
    from quadraturefields_amd import _C as C, baking, synthetic, utils
    from quadraturefields_amd.datasets.utils import Rays
    from quadraturefields_amd.mesh_utils import MeshIntersection, make_camera
    from quadraturefields_amd.pruning import MeshPruner
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceField
    from quadraturefields_amd.render import FrameRenderer

    dev = torch.device("cuda:0")
    size, log2_t = args.size, args.log2_hashmap_size
    mesh = synthetic.shell_mesh(n_shells=args.shells, subdivisions=args.subdivisions)
    n_tri = int(mesh.faces.shape[0])
    mi = MeshIntersection(mesh, simplify_mesh=False, scale=1.0, num_intersections=K, render_step_size=DELTA, device=dev)
    ri = mi.rayintersector
    field = NGPRadianceField(aabb=[-1.5] * 3 + [1.5] * 3, log2_hashmap_size=log2_t)
    field.load_state_dict(synthetic.seeded_ngp_state(log2_t, field.mlp_base.grid.n_rows), strict=False)
    field = field.to(dev)
    fr = FrameRenderer(mi, field)
    # the reference-shaped loop has an intersector of its own: its ray-major packs steer the re-origin policy their own way
    mi_d = MeshIntersection(mesh, simplify_mesh=False, scale=1.0, num_intersections=K, render_step_size=DELTA, device=dev)
    focal = synthetic.lego_focal(size)
    cams = synthetic.orbit_cameras(args.views + args.warmup, seed=17)
    views = []
    for c2w in cams:
        o, d = synthetic.camera_rays(c2w, focal, size, size, device=dev)
        views.append((o, d, make_camera(c2w, focal, size, size)))
    warm, timed_views = views[:args.warmup], views[args.warmup:]

    def job(view):
        o, d, cam = view
        prepared = fr._one_call_job(o, d, cam, K, None, False, want_tri=True)
        if prepared is None:
            sys.exit("prune_bench.py: the intersector left the plain camera-coherent pass on the bench scene: "
                     f"raster_wide {ri.raster_wide}, back-off {ri._raster_backoff}, rule up front {ri._rule_upfront}, "
                     f"repaired frames {ri.repaired_frames}, camera mismatches {ri.camera_mismatch_frames}")
        return prepared

    def mode_a(view, state):
        j, frame, token, keep, _ = job(view)
        C.check(C.lib().qf_frame_render(ri._handle, ctypes.byref(j), C.stream()), "qf_frame_render")
        ri.fused_frame_done(frame, token)
        frame._keep = frame._keep + keep
        return frame, keep

    def mode_b(view, state):
        j, frame, token, keep, _ = job(view)
        C.check(C.lib().qf_frame_prune(ri._handle, ctypes.byref(j), C.ptr(state["tw"]), n_tri, VALID,
                                       C.ptr(state["counts"][state["i"]]), C.ptr(state["bad"]), C.stream()), "qf_frame_prune")
        ri.fused_frame_done(frame, token)
        frame._keep = frame._keep + keep

    def mode_b_add_view(view, state):
        state["pruner"].add_view(*view)

    def mode_c(view, state):
        frame, keep = mode_a(view, state)
        rgbs, sigmas = keep[0], keep[1]
        n = int(frame.total_dev.item())                     # slots of the frame: the host wait of this route
        weights = torch.zeros((n,), dtype=torch.float32, device=dev)
        img = state["img"]
        C.check(C.lib().qf_composite_tiles(C.ptr(rgbs), C.ptr(sigmas), C.ptr(frame.depth_c), DELTA, C.ptr(frame.hit_count), K,
                                           C.ptr(frame.tile_base), size, size, C.BG_WHITE, None, C.ptr(img[0]), C.ptr(img[1]),
                                           C.ptr(img[2]), C.ptr(weights), None, C.stream()), "qf_composite_tiles")
        ids = frame.tri_c[:n].long()
        C.check(C.lib().qf_scatter_max(C.ptr(weights), C.ptr(ids), n, n_tri, C.ptr(state["tw"]), C.stream()), "qf_scatter_max")
        row = state["counts"][state["i"]]
        row[0] = frame.hit_count.sum()
        row[1] = (weights > VALID).sum()

    def mode_d(view, state):
        o, d, cam = view
        data = mi_d.sampling_raytrace_device(d, o, camera=cam)
        out = utils.render_image_finetune_with_occgrid(field, None, None, Rays(origins=o, viewdirs=d), data,
                                                       render_step_size=DELTA, mesh_intersect=mi_d, scaling=0.0)
        weights, index_tri = out[4], out[8]
        state["num"].append(len(weights))
        state["valid"].append(int(torch.sum(weights > 0.001).item()))
        tw_i = baking.triangle_max_weights(weights[:, 0], index_tri, torch.zeros_like(state["tw"]))
        state["tw"] = torch.maximum(state["tw"], tw_i)

    modes = {"a": mode_a, "b": mode_b, "b_add_view": mode_b_add_view, "c": mode_c, "d": mode_d}
    chosen = [m for m in args.modes.split(",") if m]

    def fresh_state():
        n = size * size
        st = {"tw": torch.zeros((n_tri,), dtype=torch.float32, device=dev),
              "counts": torch.zeros((len(views), 2), dtype=torch.int64, device=dev),
              "bad": torch.zeros((1,), dtype=torch.int32, device=dev), "i": 0, "num": [], "valid": [],
              "img": [torch.empty((n, c), dtype=torch.float32, device=dev) for c in (3, 1, 1)]}
        st["pruner"] = MeshPruner(mi, field)
        return st

    def run_mode(name):
        fn = modes[name]
        scratch = fresh_state()
        for v in warm:                                      # code objects, allocator, policy; maxima thrown away
            fn(v, scratch)
        ri._settle_fused_policy(0)
        ri._settle_deferred_policy()
        torch.cuda.synchronize()
        st = fresh_state()
        events = []
        t0 = time.perf_counter()
        for i, v in enumerate(timed_views):
            st["i"] = i
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(v, st)
            b.record()
            events.append((a, b))
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3 / len(timed_views)
        ms = [a.elapsed_time(b) for a, b in events]
        tw = st["pruner"].triangle_weights if name == "b_add_view" else st["tw"]
        return {"view1_ms": ms[0], "steady_ms": statistics.median(ms[args.settle - 1:]), "per_view_ms": ms,
                "wall_ms_per_view": wall}, tw.clone()

    results = {m: [] for m in chosen}
    maxima = {}
    for _ in range(args.repeats):
        for m in chosen:                                    # the modes alternate inside a repeat
            r, tw = run_mode(m)
            results[m].append(r)
            maxima[m] = tw
    out = {"scene": {"triangles": n_tri, "log2_hashmap_size": log2_t, "width": size, "height": size, "K": K,
                     "views": len(timed_views), "warmup_views": args.warmup, "steady_from_view": args.settle,
                     "repeats": args.repeats},
           "device": torch.cuda.get_device_name(0), "modes": {}}
    for m in chosen:
        steady = [r["steady_ms"] for r in results[m]]
        out["modes"][m] = {"view1_ms": [r["view1_ms"] for r in results[m]], "steady_ms": steady,
                           "steady_ms_median": statistics.median(steady), "steady_ms_spread": max(steady) - min(steady),
                           "wall_ms_per_view": [r["wall_ms_per_view"] for r in results[m]],
                           "per_view_ms_last_repeat": results[m][-1]["per_view_ms"]}
    with_tw = [m for m in chosen if m != "a"]
    out["maxima_equal"] = {f"{with_tw[0]}=={m}": bool(torch.equal(maxima[with_tw[0]], maxima[m])) for m in with_tw[1:]}
    if with_tw:
        tw = maxima[with_tw[0]]
        out["faces_kept"] = int((tw > 1e-3).sum().item())
    md = out["modes"]
    if "a" in md and "b" in md:
        out["prune_on_top_of_frame_ms"] = md["b"]["steady_ms_median"] - md["a"]["steady_ms_median"]
        out["prune_on_top_of_frame_view1_ms"] = statistics.median(md["b"]["view1_ms"]) - statistics.median(md["a"]["view1_ms"])
    if "b" in md and "c" in md:
        out["b_minus_c_ms"] = md["b"]["steady_ms_median"] - md["c"]["steady_ms_median"]
        out["session_spread_ms"] = max(md["b"]["steady_ms_spread"], md["c"]["steady_ms_spread"])
        out["b_not_slower_than_c"] = out["b_minus_c_ms"] <= out["session_spread_ms"]
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
