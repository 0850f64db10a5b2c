"""The closest-point query (qf_bvh_closest_points) on the bench mesh, its baselines, and the
surface distances of decimation and vertex clustering that it makes measurable.

    python tools/closest_point_bench.py [--iters 7] [--vx 40] [--vx_sphere 8]
                                        [--out profiles/closest_point/closest_point_bench.json]

* ``bench``: the 983 040-triangle bench mesh (``shell_mesh(12, 6)``), a host-built (binned SAH) and a device-built
  (linear) tree, three query sets: the mesh's own 491 544 vertices, the vertices of its ``F // 10`` decimation, and 2^20
  uniform points in its bounding box.  One ``qf_bvh_closest_points`` call under HIP events, median / min / max of --iters
  runs after one warm-up, and queries per second from the median.
* ``morton``: the uniform points again on the device-built tree, as given and sorted by a 30-bit Morton code first (the
  sort itself is not timed): whether ordering the queries in the wrapper would pay.  The wrapper does not.
* ``torch_brute_force``: every pair of (query, triangle) in torch on the same GPU, fp64, dist2 only (the plane
  projection where it falls inside, else the three segments: ``closest_point_reference.plane_or_segments_dist2`` in
  torch), level-5 icosphere, the query count doubled until a run takes more than a second; the largest that fits is
  reported beside the device query on the same inputs.  Nothing else here computes this.
* ``restatement``: ``tests/closest_point_reference.closest_points`` (the plain numpy loop) on the level-5 icosphere with
  2 048 queries, one run, the device on the same inputs, and whether the bytes agree.
* ``surface_distance``: ``mc_utils.simplify_vertex_clustering`` (quadric contraction) at voxel size ``1 / vx`` (bench
  mesh) and ``1 / vx_sphere`` (level-5 sphere) against ``decimate_mesh_device`` to the face count clustering produced:
  ``mc_utils.mesh_distance_device`` of each output against the input (a = output, b = input), beside the
  nearest-input-vertex proxy of tools/mesh_decimate_bench.py.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch


def _stat(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


class Query:
    """Preallocated outputs around one qf_bvh_closest_points call on a handle."""

    def __init__(self, handle, points):
        self.handle, self.points = handle, points.to(torch.float64).contiguous()
        n = self.points.shape[0]
        self.tri = torch.empty((n,), dtype=torch.int32, device="cuda")
        self.bary = torch.empty((n, 3), dtype=torch.float64, device="cuda")
        self.dist2 = torch.empty((n,), dtype=torch.float64, device="cuda")
        self.counts = torch.empty((2,), dtype=torch.int64, device="cuda")

    def __call__(self):
        from quadraturefields_amd import _C
        _C.check(_C.lib().qf_bvh_closest_points(self.handle, _C.ptr(self.points), self.points.shape[0], math.inf, _C.ptr(self.tri),
                                                _C.ptr(self.bary), _C.ptr(self.dist2), _C.ptr(self.counts), _C.stream()),
                 "qf_bvh_closest_points")


def _events(fn, iters):
    ms = []
    for _ in range(iters + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return _stat(ms[1:])


def _timed_query(handle, points, iters):
    q = Query(handle, points)
    ms = _events(q, iters)
    return dict(queries=int(points.shape[0]), ms=ms, queries_per_second=points.shape[0] / (ms["median"] * 1e-3),
                mean_distance=float(q.dist2.sqrt().mean()), counts=q.counts.tolist()), q


def morton_order(points):
    lo, hi = points.min(dim=0).values, points.max(dim=0).values
    cell = ((points - lo) / (hi - lo).clamp_min(1e-30) * 1023.0).to(torch.int64).clamp_(0, 1023)

    def spread(x):
        x = (x | (x << 16)) & 0x030000FF
        x = (x | (x << 8)) & 0x0300F00F
        x = (x | (x << 4)) & 0x030C30C3
        return (x | (x << 2)) & 0x09249249
    return torch.argsort(spread(cell[:, 0]) | (spread(cell[:, 1]) << 1) | (spread(cell[:, 2]) << 2))


def torch_brute_force(q, t, chunk_pairs=1 << 24):
    """dist2 fp64 [N] of every query to the triangles t [T,3,3]: plane projection where inside, else the segments."""
    a, b, c = t[None, :, 0], t[None, :, 1], t[None, :, 2]
    n = torch.linalg.cross(b - a, c - a)
    n2 = (n * n).sum(-1)

    def seg(p, u, v):
        d = v - u
        l2 = (d * d).sum(-1).clamp_min(1e-300)
        s = (((p - u) * d).sum(-1) / l2).clamp(0.0, 1.0)
        e = p - (u + s[..., None] * d)
        return (e * e).sum(-1)
    out = []
    step = max(1, chunk_pairs // t.shape[0])
    for i in range(0, q.shape[0], step):
        p = q[i:i + step, None, :]
        h = ((p - a) * n).sum(-1)
        foot = p - (h / n2)[..., None] * n
        inside = torch.ones_like(h, dtype=torch.bool)
        for u, v in ((a, b), (b, c), (c, a)):
            inside &= (torch.linalg.cross((v - u).expand_as(foot), foot - u) * n).sum(-1) >= 0
        edges = torch.minimum(torch.minimum(seg(p, a, b), seg(p, a, c)), seg(p, b, c))
        out.append(torch.where(inside, h * h / n2, edges).min(dim=1).values)
    return torch.cat(out)


def nearest_vertex_mean(out_v, in_v, chunk=1024):
    a, b = out_v.to(torch.float32), in_v.to(torch.float32)
    total = 0.0
    for i in range(0, a.shape[0], chunk):
        total += float(torch.cdist(a[i:i + chunk], b).min(dim=1).values.double().sum())
    return total / max(a.shape[0], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--vx", type=float, default=40.0)
    ap.add_argument("--vx_sphere", type=float, default=8.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "closest_point", "closest_point_bench.json"))
    args = ap.parse_args()
    from quadraturefields_amd import mc_utils, synthetic
    from quadraturefields_amd.mesh_utils import RayIntersector
    from tests import closest_point_reference as cp
    from tests import mesh_decimate_reference as ref
    result = {"device": torch.cuda.get_device_name(0), "iters": args.iters}

    mesh = synthetic.shell_mesh(n_shells=12, subdivisions=6)
    v, f = torch.from_numpy(mesh.vertices).cuda(), torch.from_numpy(mesh.faces).cuda()
    small = mc_utils.decimate_mesh_device(v, f, f.shape[0] // 10)
    lo, hi = v.min(dim=0).values, v.max(dim=0).values
    gen = torch.Generator(device="cuda").manual_seed(0)
    uniform = lo + (hi - lo) * torch.rand((1 << 20, 3), dtype=torch.float64, device="cuda", generator=gen)
    sets = {"mesh_vertices": v, "decimated_vertices": small.vertices, "uniform_box": uniform}
    bench = {"vertices": int(v.shape[0]), "faces": int(f.shape[0]), "decimated_faces": int(small.faces.shape[0])}
    answers = {}
    for builder in ("host", "device"):
        t0 = time.perf_counter()
        inter = RayIntersector(mesh, device="cuda", builder=builder)
        torch.cuda.synchronize()
        bench[builder] = {"build_wall_ms": (time.perf_counter() - t0) * 1e3, "max_stack": inter.max_stack}
        for name, pts in sets.items():
            bench[builder][name], q = _timed_query(inter._handle, pts, args.iters)
            got = (q.tri.clone(), q.bary.clone(), q.dist2.clone())
            if name in answers:
                bench[builder][name]["same_bytes_as_host_tree"] = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8))
                                                                      for a, b in zip(got, answers[name]))
            answers.setdefault(name, got)
        if builder == "device":
            order = morton_order(uniform)
            result["morton"] = {"as_given": bench[builder]["uniform_box"]["ms"],
                                "sorted": _timed_query(inter._handle, uniform[order].contiguous(), args.iters)[0]["ms"]}
        del inter
    result["bench"] = bench
    print(json.dumps({k: {n: bench[k][n]["ms"]["median"] for n in sets} for k in ("host", "device")}), json.dumps(result["morton"]))

    sv, sf = ref.icosphere(5)
    sphere = RayIntersector(type(mesh)(sv, sf), device="cuda", builder="device")
    t64 = torch.from_numpy(cp.triangles_of(sv, sf).astype(np.float64)).cuda()
    n, fits = 1024, None
    while n <= (1 << 20):
        pts = torch.from_numpy(np.random.default_rng(n).uniform(-2, 2, (n, 3))).cuda()
        torch_brute_force(pts[:64], t64)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d2 = torch_brute_force(pts, t64)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        if ms > 1000.0:
            break
        dev, q = _timed_query(sphere._handle, pts, args.iters)
        rel = float(((q.dist2 - d2).abs() / d2).max())
        fits = {"queries": n, "triangles": int(sf.shape[0]), "pairs": n * int(sf.shape[0]), "torch_wall_ms": ms,
                "device_ms": dev["ms"], "max_relative_difference": rel}
        n *= 2
    result["torch_brute_force"] = fits
    print(json.dumps(fits))

    pts = np.random.default_rng(43).uniform(-2, 2, (2048, 3))
    t0 = time.perf_counter()
    want = cp.closest_points(cp.triangles_of(sv, sf), pts)
    numpy_ms = (time.perf_counter() - t0) * 1e3
    dev, q = _timed_query(sphere._handle, torch.from_numpy(pts).cuda(), args.iters)
    same = (q.tri.cpu().numpy().tobytes() == want[0].tobytes() and q.bary.cpu().numpy().tobytes() == want[1].tobytes()
            and q.dist2.cpu().numpy().tobytes() == want[2].tobytes() and q.counts.tolist() == want[3].tolist())
    result["restatement"] = {"mesh": "icosphere level 5", "faces": int(sf.shape[0]), "queries": 2048, "numpy_wall_ms": numpy_ms,
                             "device_ms": dev["ms"], "same_bytes": bool(same)}
    print(json.dumps(result["restatement"]))

    def compare(vin, fin, voxel):
        cv, cf = mc_utils.simplify_vertex_clustering(vin, fin, voxel, "quadric")
        d = mc_utils.decimate_mesh_device(vin, fin, cf.shape[0])
        out = {}
        for name, (ov, of) in (("clustering", (cv, cf)), ("decimation", (d.vertices, d.faces))):
            m = mc_utils.mesh_distance_device(ov, of, vin, fin)
            out[name] = {"faces": int(of.shape[0]), "vertices": int(ov.shape[0]), "out_to_in_mean": m.a_to_b_mean,
                         "out_to_in_rms": m.a_to_b_rms, "out_to_in_max": m.a_to_b_max, "in_to_out_mean": m.b_to_a_mean,
                         "in_to_out_rms": m.b_to_a_rms, "in_to_out_max": m.b_to_a_max, "symmetric_max": m.symmetric_max,
                         "mean_nearest_vertex": nearest_vertex_mean(ov, vin)}
        return out
    result["surface_distance"] = {"vx": args.vx, "vx_sphere": args.vx_sphere,
                                  "sphere": compare(torch.from_numpy(sv).cuda(), torch.from_numpy(sf).cuda(), 1.0 / args.vx_sphere),
                                  "bench": compare(v, f, 1.0 / args.vx)}
    print(json.dumps(result["surface_distance"]))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
