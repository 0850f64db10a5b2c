"""Marching cubes (qf_marching_cubes_count / qf_marching_cubes_emit) per pass, and the whole quadrature extraction.

    python tools/mc_bench.py [--sizes 256 512 1024] [--iters 5] [--pipeline 1024]

Volumes: a smooth sphere (``0.4 n - r`` in voxels) and a shell-dense ``sin(100 r)`` with r the radius in the
reference's [-1, 1] coordinates (tens of millions of triangles at 1024^3).  Each pass is timed with HIP events around
its C call (median of --iters); GB/s counts one read of the fp32 volume against the measured 6.29 TB/s copy rate.
The pipeline row is the wall time of ``mc_utils.quadrature_surface_mesh`` on a radial field grid (inputs already on
the host as numpy, as the reference loads them), including the host copy of the mesh.
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

COPY_BYTES_PER_S = 6.29e12


def volumes(n):
    ax = torch.arange(n, device="cuda", dtype=torch.float32) - (n - 1) / 2
    r = torch.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2)
    yield "sphere", 0.4 * n - r
    yield "shells", torch.sin(100.0 * (r * (2.0 / (n - 1))))


def time_passes(vol, iters):
    from quadraturefields_amd import _C
    lib = _C.lib()
    n0, n1, n2 = vol.shape
    ws_bytes = int(lib.qf_marching_cubes_workspace_bytes(n0, n1, n2))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device="cuda")
    counts = torch.empty((3,), dtype=torch.int64, device="cuda")
    args = (_C.ptr(vol), n0, n1, n2, 0.0, _C.ptr(ws), ws_bytes)
    _C.check(lib.qf_marching_cubes_count(*args, _C.ptr(counts), _C.stream()), "count")
    nv, nf, _ = counts.tolist()
    verts = torch.empty((nv, 3), dtype=torch.float32, device="cuda")
    faces = torch.empty((nf, 3), dtype=torch.int32, device="cuda")
    t_count, t_emit = [], []
    for _ in range(iters + 1):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        _C.check(lib.qf_marching_cubes_count(*args, _C.ptr(counts), _C.stream()), "count")
        e[1].record()
        _C.check(lib.qf_marching_cubes_emit(*args, _C.ptr(verts), nv, _C.ptr(faces), nf, _C.stream()), "emit")
        e[2].record()
        torch.cuda.synchronize()
        t_count.append(e[0].elapsed_time(e[1]) * 1e-3)
        t_emit.append(e[1].elapsed_time(e[2]) * 1e-3)
    tc, te = statistics.median(t_count[1:]), statistics.median(t_emit[1:])
    nbytes = 4 * vol.numel()
    return {"vertices": nv, "faces": nf, "workspace_bytes": ws_bytes, "count_ms": tc * 1e3, "emit_ms": te * 1e3,
            "count_GBps": nbytes / tc / 1e9, "emit_GBps": nbytes / te / 1e9,
            "count_frac_copy": nbytes / tc / COPY_BYTES_PER_S, "emit_frac_copy": nbytes / te / COPY_BYTES_PER_S}


def pipeline(n, iters):
    from quadraturefields_amd import mc_utils
    ax = np.arange(n, dtype=np.float32) - (n - 1) / 2
    grid = np.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2) / (n - 1)
    grads = np.ones((n, n, n), np.float32)
    binaries = np.ones((1, n // 4, n // 4, n // 4), np.float32)
    times, mesh = [], None
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mesh = mc_utils.quadrature_surface_mesh(grid, grads, binaries, sigma=100.0, omega=100.0)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        del mesh
        torch.cuda.empty_cache()
    return {"n": n, "wall_s": statistics.median(times), "all_s": times}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512, 1024])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--pipeline", type=int, default=1024, help="grid size of the whole-pipeline row (0 = skip)")
    ap.add_argument("--pipeline-iters", type=int, default=2)
    a = ap.parse_args()
    from quadraturefields_amd import build
    build.build()
    rows = []
    for n in a.sizes:
        for name, vol in volumes(n):
            row = {"n": n, "volume": name, **time_passes(vol.contiguous(), a.iters)}
            print(json.dumps(row), flush=True)
            rows.append(row)
            del vol
            torch.cuda.empty_cache()
    if a.pipeline:
        print(json.dumps({"pipeline": pipeline(a.pipeline, a.pipeline_iters)}), flush=True)


if __name__ == "__main__":
    main()
