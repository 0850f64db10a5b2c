"""Vertex clustering (qf_vertex_clustering_count / qf_vertex_clustering_emit) per call, and the whole device pipeline.

    python tools/cluster_bench.py [--sizes 256 512 1024] [--vx 150 300] [--iters 5]

Inputs are the marching-cubes meshes of tools/mc_bench.py (a smooth sphere ``0.4 n - r`` in voxels and a shell-dense
``sin(100 r)``), normalised to [-1, 1] as ``mc_utils`` does.  count and emit (quadric contraction) are timed with HIP
events around their C calls, median of --iters after one warm-up.  The pipeline column times marching cubes ->
normalise -> ``simplify_vertex_clustering`` (count, read-back of the totals, allocation, emit) with HIP events around
the whole composition, median of --iters.  Prints one JSON line per (size, volume, vx).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

sys.path.insert(0, os.path.join(ROOT, "tools"))
from mc_bench import volumes  # noqa: E402


def _events(n):
    return [torch.cuda.Event(enable_timing=True) for _ in range(n)]


def time_calls(v, f, s, iters):
    from quadraturefields_amd import _C
    lib = _C.lib()
    n_v, n_f = v.shape[0], f.shape[0]
    ws_bytes = int(lib.qf_vertex_clustering_workspace_bytes(n_v, n_f))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device="cuda")
    counts = torch.empty((5,), dtype=torch.int64, device="cuda")
    fb = torch.zeros((1,), dtype=torch.int64, device="cuda")
    args = (_C.ptr(v), n_v, _C.ptr(f), n_f, s)
    _C.check(lib.qf_vertex_clustering_count(*args, _C.ptr(ws), ws_bytes, _C.ptr(counts), _C.stream()), "count")
    n_cells, n_out = counts.tolist()[:2]
    out_v = torch.empty((n_cells, 3), dtype=torch.float64, device="cuda")
    out_f = torch.empty((n_out, 3), dtype=torch.int64, device="cuda")
    t_count, t_emit = [], []
    for _ in range(iters + 1):
        e = _events(3)
        e[0].record()
        _C.check(lib.qf_vertex_clustering_count(*args, _C.ptr(ws), ws_bytes, _C.ptr(counts), _C.stream()), "count")
        e[1].record()
        _C.check(lib.qf_vertex_clustering_emit(*args, 1, _C.ptr(ws), ws_bytes, _C.ptr(out_v), n_cells, _C.ptr(out_f),
                                               n_out, _C.ptr(fb), _C.stream()), "emit")
        e[2].record()
        torch.cuda.synchronize()
        t_count.append(e[0].elapsed_time(e[1]))
        t_emit.append(e[1].elapsed_time(e[2]))
    return {"V_out": n_cells, "F_out": n_out, "fallback_cells": int(fb.item()), "workspace_bytes": ws_bytes,
            "count_ms": statistics.median(t_count[1:]), "emit_ms": statistics.median(t_emit[1:])}


def time_pipeline(vol, s, iters):
    from quadraturefields_amd import mc_utils
    n = vol.shape[0]
    times = []
    for _ in range(iters + 1):
        e = _events(2)
        e[0].record()
        verts, faces = mc_utils.marching_cubes(vol, 0.0)
        v = mc_utils.normalise_vertices(verts, n)
        del verts
        out = mc_utils.simplify_vertex_clustering(v, faces, s)
        e[1].record()
        torch.cuda.synchronize()
        times.append(e[0].elapsed_time(e[1]))
        del v, faces, out
    return statistics.median(times[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512, 1024])
    ap.add_argument("--vx", type=int, nargs="+", default=[150, 300])
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    from quadraturefields_amd import build, mc_utils
    build.build()
    for n in a.sizes:
        for name, vol in volumes(n):
            vol = vol.contiguous()
            verts, faces = mc_utils.marching_cubes(vol, 0.0)
            v = mc_utils.normalise_vertices(verts, n)
            f = faces.to(torch.int64)
            del verts, faces
            for vx in a.vx:
                row = {"n": n, "volume": name, "vx": vx, "V_in": v.shape[0], "F_in": f.shape[0],
                       **time_calls(v, f, 1 / vx, a.iters), "pipeline_ms": time_pipeline(vol, 1 / vx, a.iters)}
                print(json.dumps(row), flush=True)
                torch.cuda.empty_cache()
            del v, f, vol
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
