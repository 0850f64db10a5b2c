"""Per-triangle UV atlas (uv_atlas.per_triangle_atlas): time of the call and of its kernels.

    python tools/uv_atlas_bench.py [--sizes 4096 8192] [--iters 5]

Mesh: the bench mesh (``synthetic.shell_mesh()``, 983 040 faces) with its UVs ignored.  The whole call -- upload,
measure, the density search with its one small read-back per probe, emit, and the copy of vertices and UVs back to the
host -- is timed with HIP events (median of --iters); the same with ``texels_per_unit`` given (one probe instead of the
search); each kernel's time comes from the profiler's device timestamps of one further searched call.  One JSON line per
size.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

KERNELS = {"reduce_kernel": "measure", "finalize_kernel": "measure", "measure_kernel": "measure",
           "histogram_kernel": "probes", "layout_kernel": "probes", "key_kernel": "keys", "rank_kernel": "rank",
           "emit_kernel": "emit", "radix": "sort", "onesweep": "sort", "sort": "sort"}


def timed(fn, iters):
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times)


def run(mesh, size, iters):
    from quadraturefields_amd import uv_atlas
    from torch.profiler import ProfilerActivity, profile
    _, info = uv_atlas.per_triangle_atlas(mesh, size)                      # warm-up (and the lazy library load)
    torch.cuda.synchronize()
    searched = timed(lambda: uv_atlas.per_triangle_atlas(mesh, size), iters)
    fixed = timed(lambda: uv_atlas.per_triangle_atlas(mesh, size, texels_per_unit=info.rho), iters)
    groups, launches = {}, {}
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        uv_atlas.per_triangle_atlas(mesh, size)
        torch.cuda.synchronize()
    for ev in prof.events():
        if ev.device_type.name not in ("CUDA", "HIP"):
            continue
        for kname, group in KERNELS.items():
            if kname in ev.name:
                groups[group] = groups.get(group, 0.0) + ev.device_time_total / 1e3           # us -> ms
                launches[group] = launches.get(group, 0) + 1
                break
    return {"faces": len(mesh.faces), "size": size, "rho": info.rho, "rows_used": info.rows_used,
            "texels_used": info.texels_used, "utilisation": info.texels_used / size ** 2,
            "classes": [int(i) for i, c in enumerate(info.class_counts) if c],
            "call_ms_median": searched[0], "call_ms_min": searched[1], "fixed_rho_call_ms_median": fixed[0],
            "kernel_ms": groups, "launches": launches}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 8192])
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    from quadraturefields_amd import synthetic
    from quadraturefields_amd.mesh_io import TriMesh
    shell = synthetic.shell_mesh()
    mesh = TriMesh(shell.vertices, shell.faces)
    for size in args.sizes:
        print(json.dumps(run(mesh, size, args.iters)), flush=True)


if __name__ == "__main__":
    main()
