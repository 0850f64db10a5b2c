"""Times the two BVH builders -- qf_bvh_create (host, binned SAH) and qf_bvh_create_device (GPU, linear BVH straight to the
8-wide tree) -- in one process on the bench mesh (983 040 triangles) and the configs[2] mesh, and the traversal of the two
trees they produce: the general traversal on an 800x800 camera frame and on 2^17 random rays, and the camera-coherent
pass.  Writes one JSON object.

    python tools/bvh_build_bench.py [--out profiles/bvh_build/bvh_build_bench.json] [--iters 10]
"""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import bench

PASSES = ("reduce", "keys", "sort", "gather", "levels", "boxes", "stack")
REPEATS = 5


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    ev = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        ev.append((a, b))
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def tree_shape(lib, handle):
    starts = np.zeros(128, dtype=np.int32)
    n = int(lib.qf_bvh_copy_level_starts(handle, starts.ctypes.data_as(ctypes.c_void_p), 128))
    return {"n_nodes8": int(lib.qf_bvh_num_wide_nodes(handle)), "levels": n - 1, "max_stack8": int(lib.qf_bvh_max_stack(handle))}


def build_times(lib, _C, tri, tri_dev):
    n = tri.shape[0]
    out = {}

    def host():
        h = ctypes.c_void_p()
        t0 = time.perf_counter()
        _C.check(lib.qf_bvh_create(tri.ctypes.data_as(ctypes.c_void_p), n, ctypes.byref(h)), "qf_bvh_create")
        dt = time.perf_counter() - t0
        shape = tree_shape(lib, h)
        lib.qf_bvh_destroy(h)
        return dt, shape

    def device(timed_passes=False):
        h = ctypes.c_void_p()
        ms = (ctypes.c_float * len(PASSES))()
        peak = ctypes.c_int64(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()           # everything the call does: allocations, launches, host waits, frees
        if timed_passes:
            _C.check(lib.qf_bvh_create_device_timed(_C.ptr(tri_dev), n, _C.stream(), ms, ctypes.byref(peak), ctypes.byref(h)),
                     "qf_bvh_create_device_timed")
        else:
            _C.check(lib.qf_bvh_create_device(_C.ptr(tri_dev), n, _C.stream(), ctypes.byref(h)), "qf_bvh_create_device")
        dt = time.perf_counter() - t0
        shape = tree_shape(lib, h)
        lib.qf_bvh_destroy(h)
        return dt, shape, list(ms), int(peak.value)

    device()                               # code-object load of the build's kernels: once per process
    runs = [host() for _ in range(REPEATS)]
    out["host_build_s"] = float(np.median([r[0] for r in runs]))
    out["host_build_runs_s"] = [r[0] for r in runs]
    out["host_tree"] = runs[0][1]
    runs = [device() for _ in range(REPEATS)]
    out["device_build_s"] = float(np.median([r[0] for r in runs]))
    out["device_build_runs_s"] = [r[0] for r in runs]
    out["device_tree"] = runs[0][1]
    runs = [device(True) for _ in range(REPEATS)]
    out["device_pass_ms"] = {p: float(np.median([r[2][i] for r in runs])) for i, p in enumerate(PASSES)}
    out["device_peak_bytes"] = runs[0][3]
    out["device_peak_bytes_per_triangle"] = runs[0][3] / n
    out["build_speedup"] = out["host_build_s"] / out["device_build_s"]
    return out


def traversal_times(mesh, dev, iters, rays_n):
    from quadraturefields_amd import synthetic
    from quadraturefields_amd.mesh_utils import RayIntersector, make_camera
    K, W, H = bench.MAX_HITS, bench.W, bench.H
    cams = synthetic.orbit_cameras(8, seed=1)
    focal = synthetic.lego_focal(W)
    rays = [synthetic.camera_rays(c, focal, W, H, device=dev) for c in cams]
    o, d = rays[0]
    cam = make_camera(cams[0], focal, W, H)
    pool_o, pool_d = torch.cat([r[0] for r in rays]), torch.cat([r[1] for r in rays])
    g = torch.Generator(device=dev).manual_seed(0)
    pick = torch.randint(0, pool_o.shape[0], (rays_n,), device=dev, generator=g)
    bo, bd = pool_o[pick].contiguous(), pool_d[pick].contiguous()
    out, hits = {}, {}
    for builder in ("host", "device"):
        ri = RayIntersector(mesh, max_hits=K, device=dev, builder=builder)
        r = {"frame_bvh_ms": timed(lambda: ri._hits_bvh(o, d, K, W), iters),
             "batch_random_ms": timed(lambda: ri._hits_bvh(bo, bd, K, 0), iters),
             "frame_camera_coherent_ms": timed(lambda: ri._hits_raster_frame(o, d, K, cam), iters),
             "camera_coherent_route": ri.last_route}
        hits[builder] = [x.clone() for x in ri._hits_bvh(bo, bd, K, 0)]
        out[builder] = r
        del ri
    out["batch_rays"] = rays_n
    out["hits_identical"] = all(torch.equal(a, b) for a, b in zip(hits["host"], hits["device"]))
    for key in ("frame_bvh_ms", "batch_random_ms", "frame_camera_coherent_ms"):
        out[key.replace("_ms", "_device_over_host")] = out["device"][key] / out["host"][key]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "bvh_build", "bvh_build_bench.json"))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rays", type=int, default=1 << 17)
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    from quadraturefields_amd import _C, synthetic
    lib = _C.lib()
    dev = torch.device("cuda:0")
    result = {"repeats": REPEATS, "meshes": {}}
    for name, shells in (("bench", bench.N_SHELLS), ("configs[2]", 36)):
        mesh = synthetic.shell_mesh(n_shells=shells, subdivisions=bench.SUBDIV)
        tri = np.ascontiguousarray(mesh.vertices.astype(np.float32)[mesh.faces].reshape(-1, 9))
        tri_dev = torch.from_numpy(tri).to(dev)
        r = {"triangles": int(tri.shape[0])}
        r.update(build_times(lib, _C, tri, tri_dev))
        r["traversal"] = traversal_times(mesh, dev, args.iters, args.rays)
        result["meshes"][name] = r
        print(name, json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    for name, r in result["meshes"].items():
        assert r["device_build_s"] < r["host_build_s"], f"{name}: the device build must beat the host build of the same run"


if __name__ == "__main__":
    main()
