"""Mesh refinement (qf_mesh_edges_* / qf_mesh_subdivide_*) per call, against the same results
composed from torch ops on the same GPU, and what refining the bench scene's vertex-baked asset buys.

    python tools/mesh_subdivide_bench.py [--meshes bench configs2] [--iters 7] [--frames 6] [--tol 0.01]
                                         [--out profiles/mesh_subdivide/mesh_subdivide_bench.json]

Meshes: the 983 040-triangle bench mesh (``shell_mesh(12, 6)``) and the configs[2] mesh (``shell_mesh(36, 6)``), each with
every edge marked and with a seeded 10 % mark.

* ``edges_count_ms`` / ``edges_emit_ms`` / ``split_count_ms`` / ``split_emit_ms``: HIP events around the C calls.
  ``wrapper_ms``: ``mc_utils.mesh_edges_device`` and ``mc_utils.subdivide_mesh_device`` (count, the read-back of the
  counts, allocation, emit), a host clock around work that ends in a synchronise.
* ``torch_edges_ms`` / ``torch_split_ms``: the same results from torch ops -- ``torch.unique`` on the packed (min, max)
  pairs, ``searchsorted`` for every half-edge's pair, the lowest half-edge per pair by ``scatter_reduce``, an ``argsort`` of
  those for the first-appearance order; then cumulative sums for the output positions and indexed stores per split
  pattern -- with a synchronise at the end.  (The composition assumes a mesh without degenerate faces, which these are.)
* The composition's results are compared with the kernels' bytes before anything is timed.
Every time is the median of --iters runs after one warm-up, with the minimum and maximum beside it.

``frames``: on bench.py's scene (800 x 800 orbit frames, K = 25, the seeded 6-lobe SG field) the vertex-baked frame
(``FrameRenderer.render_vertex_baked``, two launches) of the input mesh, of one uniform level and of one
``baking.refine_vertex_baked`` level at ``--tol`` under a budget of twice the input's vertices: time per frame (median of
--iters passes over the frames after a warm-up pass, with the spread), PSNR against the SG field's own frames of the
input mesh, and the bytes of the table and of the mesh's 128-byte triangle records.
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch


def _stat(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def _timed(fn, iters):
    """Host clock around ``fn`` plus a synchronise: ms, median / min / max of ``iters`` after one warm-up."""
    out = []
    for _ in range(iters + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return _stat(out[1:])


def time_edges(f, n_v, iters):
    from quadraturefields_amd import _C
    lib = _C.lib()
    n_f = f.shape[0]
    ws_bytes = int(lib.qf_mesh_edges_workspace_bytes(n_v, n_f))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device="cuda")
    counts = torch.empty((4,), dtype=torch.int64, device="cuda")
    args = (_C.ptr(f), n_f, n_v, _C.ptr(ws), ws_bytes)
    _C.check(lib.qf_mesh_edges_count(*args, _C.ptr(counts), _C.stream()), "count")
    c = counts.tolist()
    edges = torch.empty((c[0], 2), dtype=torch.int64, device="cuda")
    face_edges = torch.empty((n_f, 3), dtype=torch.int64, device="cuda")
    t_count, t_emit = [], []
    for _ in range(iters + 1):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        _C.check(lib.qf_mesh_edges_count(*args, _C.ptr(counts), _C.stream()), "count")
        e[1].record()
        _C.check(lib.qf_mesh_edges_emit(*args, _C.ptr(edges), c[0], _C.ptr(face_edges), _C.stream()), "emit")
        e[2].record()
        torch.cuda.synchronize()
        t_count.append(e[0].elapsed_time(e[1]))
        t_emit.append(e[1].elapsed_time(e[2]))
    return dict(zip(_C.MESH_EDGES_COUNTS, c)), ws_bytes, _stat(t_count[1:]), _stat(t_emit[1:]), edges, face_edges


def time_split(v, f, face_edges, mark, iters):
    from quadraturefields_amd import _C
    lib = _C.lib()
    n_v, n_f, n_e = v.shape[0], f.shape[0], mark.shape[0]
    ws_bytes = int(lib.qf_mesh_subdivide_workspace_bytes(n_v, n_f, n_e))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device="cuda")
    counts = torch.empty((7,), dtype=torch.int64, device="cuda")
    args = (_C.ptr(f), n_f, n_v, _C.ptr(face_edges), n_e, _C.ptr(mark), _C.ptr(ws), ws_bytes)
    _C.check(lib.qf_mesh_subdivide_count(*args, _C.ptr(counts), _C.stream()), "count")
    c = counts.tolist()
    out_v = torch.empty((c[1], 3), dtype=torch.float64, device="cuda")
    out_f = torch.empty((c[0], 3), dtype=torch.int64, device="cuda")
    fm = torch.empty((c[0],), dtype=torch.int64, device="cuda")
    vp = torch.empty((c[1], 2), dtype=torch.int64, device="cuda")
    t_count, t_emit = [], []
    for _ in range(iters + 1):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        _C.check(lib.qf_mesh_subdivide_count(*args, _C.ptr(counts), _C.stream()), "count")
        e[1].record()
        _C.check(lib.qf_mesh_subdivide_emit(_C.ptr(v), *args, _C.ptr(out_v), c[1], _C.ptr(out_f), c[0], _C.ptr(fm), _C.ptr(vp),
                                            _C.stream()), "emit")
        e[2].record()
        torch.cuda.synchronize()
        t_count.append(e[0].elapsed_time(e[1]))
        t_emit.append(e[1].elapsed_time(e[2]))
    return dict(zip(_C.MESH_SUBDIVIDE_COUNTS, c)), ws_bytes, _stat(t_count[1:]), _stat(t_emit[1:]), (out_v, out_f, fm, vp)


def torch_edges(f, n_v):
    """(edges, face_edges) of a mesh without degenerate faces, from torch ops."""
    a, b = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)                      # half-edge 3 f + k joins a and b
    key = torch.minimum(a, b) * n_v + torch.maximum(a, b)
    uniq = torch.unique(key)
    where = torch.searchsorted(uniq, key)
    first = torch.full((uniq.shape[0],), key.shape[0], dtype=torch.int64, device=f.device)
    first.scatter_reduce_(0, where, torch.arange(key.shape[0], device=f.device), "amin")
    order = torch.argsort(first)                                           # pairs by their lowest half-edge
    rank = torch.empty_like(order)
    rank[order] = torch.arange(order.shape[0], device=f.device)
    pairs = uniq[order]
    return torch.stack([pairs // n_v, pairs % n_v], dim=1), rank[where].reshape(-1, 3)


def torch_split(v, f, edges, face_edges, mark):
    n_v, n_f = v.shape[0], f.shape[0]
    mk = mark != 0
    new_id = n_v + torch.cumsum(mk, 0) - mk.to(torch.int64)
    lo, hi = edges[mk, 0], edges[mk, 1]
    out_v = torch.cat([v, 0.5 * (v[lo] + v[hi])])
    parents = torch.cat([torch.arange(n_v, device=v.device)[:, None].repeat(1, 2), torch.stack([lo, hi], dim=1)])
    fm_k = mk[face_edges]
    n = fm_k.sum(dim=1)
    kids = n + 1
    pos = torch.cumsum(kids, 0) - kids
    out_f = torch.empty((int(kids.sum()), 3), dtype=torch.int64, device=f.device)
    face_map = torch.repeat_interleave(torch.arange(n_f, device=f.device), kids)
    m = new_id[face_edges]

    def put(rows, offset, a, b, c):
        out_f[pos[rows] + offset] = torch.stack([a, b, c], dim=1)

    rows = n == 0
    put(rows, 0, f[rows, 0], f[rows, 1], f[rows, 2])
    rows = n == 3
    v0, v1, v2, m0, m1, m2 = f[rows, 0], f[rows, 1], f[rows, 2], m[rows, 0], m[rows, 1], m[rows, 2]
    put(rows, 0, v0, m0, m2)
    put(rows, 1, m0, v1, m1)
    put(rows, 2, m2, m1, v2)
    put(rows, 3, m0, m1, m2)
    for k in range(3):
        rows = (n == 1) & fm_k[:, k]
        u0, u1, u2, mid = f[rows, k], f[rows, (k + 1) % 3], f[rows, (k + 2) % 3], m[rows, k]
        put(rows, 0, u0, mid, u2)
        put(rows, 1, mid, u1, u2)
        rows = (n == 2) & ~fm_k[:, k]                                      # edge k is the unmarked one
        u0, u1, u2 = f[rows, (k + 1) % 3], f[rows, (k + 2) % 3], f[rows, k]
        a, b = m[rows, (k + 1) % 3], m[rows, (k + 2) % 3]
        low = u0 < u2
        put(rows, 0, a, u1, b)
        put(rows, 1, u0, a, torch.where(low, b, u2))
        put(rows, 2, torch.where(low, u0, a), b, u2)
    return out_v, out_f, face_map, parents


def bench_mesh(name, shells, iters):
    from quadraturefields_amd import mc_utils, synthetic
    mesh = synthetic.shell_mesh(n_shells=shells, subdivisions=6)
    v, f = torch.from_numpy(mesh.vertices).cuda(), torch.from_numpy(mesh.faces).cuda()
    n_v = v.shape[0]
    stats, ws_bytes, t_count, t_emit, edges, face_edges = time_edges(f, n_v, iters)
    te, tfe = torch_edges(f, n_v)
    assert torch.equal(te, edges) and torch.equal(tfe, face_edges), "the torch composition of the edges disagrees with the kernels"
    row = {"mesh": name, "V": int(n_v), "F": int(f.shape[0]), "edges": {
        "counts": stats, "workspace_bytes": ws_bytes, "count_ms": t_count, "emit_ms": t_emit,
        "wrapper_ms": _timed(lambda: mc_utils.mesh_edges_device(f, n_v), iters),
        "torch_ms": _timed(lambda: torch_edges(f, n_v), iters)}, "split": []}
    rng = np.random.default_rng(42)
    for label, mark_np in (("all", np.ones(edges.shape[0], np.uint8)), ("10%", (rng.random(edges.shape[0]) < 0.1).astype(np.uint8))):
        mark = torch.from_numpy(mark_np).cuda()
        s, ws_b, tc, tm, outs = time_split(v, f, face_edges, mark, iters)
        want = torch_split(v, f, edges, face_edges, mark)
        for got, ref, what in zip(outs, want, ("vertices", "faces", "face_map", "vertex_parents")):
            assert got.shape == ref.shape and torch.equal(got.view(torch.int64), ref.view(torch.int64)), \
                f"the torch composition of the split disagrees with the kernels: {what}"
        row["split"].append({"marks": label, "counts": s, "workspace_bytes": ws_b, "count_ms": tc, "emit_ms": tm,
                             "wrapper_ms": _timed(lambda: mc_utils.subdivide_mesh_device(v, f, mark, edges, face_edges), iters),
                             "torch_ms": _timed(lambda: torch_split(v, f, edges, face_edges, mark), iters)})
        del outs, want
        torch.cuda.empty_cache()
    return row


def bench_frames(iters, n_frames, tol):
    import bench
    from quadraturefields_amd import baking, mc_utils, synthetic
    from quadraturefields_amd.mesh_io import TriMesh
    from quadraturefields_amd.mesh_utils import MeshIntersection, make_camera
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceFieldSGNew
    from quadraturefields_amd.render import FrameRenderer, psnr
    dev = torch.device("cuda:0")
    lobes = 6
    mesh, mi, _ngp = bench.build_scene(dev)
    del _ngp
    sg = NGPRadianceFieldSGNew(aabb=[-1.5] * 3 + [1.5] * 3, use_viewdirs=False, num_g_lobes=lobes, log2_hashmap_size=bench.LOG2_T)
    sg.load_state_dict(synthetic.seeded_ngp_state(bench.LOG2_T, sg.mlp_base.grid.n_rows, sg_lobes=lobes), strict=False)
    sg = sg.to(dev).eval()
    cams = synthetic.orbit_cameras(n_frames + 2, seed=42)[2:]      # tools/vertex_baked_bench.py's timed frames
    focal = synthetic.lego_focal(bench.W)
    frames = [synthetic.camera_rays(c, focal, bench.W, bench.H, device=dev) + (make_camera(c, focal, bench.W, bench.H),)
              for c in cams]
    truth = [FrameRenderer(mi, sg, render_step_size=bench.STEP).render(o, d, camera=cam)[0].clone() for o, d, cam in frames]
    n_v0 = int(mesh.vertices.shape[0])

    def measure(label, mesh_intersect, table, extra):
        fr = FrameRenderer(mesh_intersect, sg, render_step_size=bench.STEP)
        scores = [float(psnr(fr.render_vertex_baked(o, d, table, camera=cam)[0], t)) for (o, d, cam), t in zip(frames, truth)]
        times = []
        for _ in range(iters + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for o, d, cam in frames:
                fr.render_vertex_baked(o, d, table, camera=cam)
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b) / len(frames))
        n_v, n_f = int(table.shape[0]), int(mesh_intersect.mesh.faces.shape[0])
        stride = 16 * ((int(table.shape[1]) + 15) // 16)
        side = baking.vertex_texture_size(n_v)
        row = {"case": label, "vertices": n_v, "faces": n_f, "table_bytes": n_v * 4 * stride, "triangle_records_bytes": n_f * 128,
               "quantised_records_bytes": side * side * 64, "ms_per_frame": _stat(times[1:]),
               "psnr_vs_field_db": statistics.mean(scores), "psnr_per_frame_db": scores}
        row.update(extra)
        print(json.dumps(row), flush=True)
        return row

    kw = dict(simplify_mesh=False, scale=1.0, num_intersections=bench.MAX_HITS, render_step_size=bench.STEP, device=dev)
    rows = [measure("input mesh", mi, baking.bake_vertex_features(sg, mi), {})]
    del mi
    torch.cuda.empty_cache()
    t0 = time.perf_counter()
    uni = baking.refine_vertex_baked(mesh, sg, tol, max_levels=1, render_step_size=bench.STEP, device=dev, uniform=True)
    torch.cuda.synchronize()
    uni_ms = (time.perf_counter() - t0) * 1e3
    level = uni.levels[0]
    errors = {k: level[k] for k in ("edges", "above_tol", "max_error", "mean_error")}
    mi_u = MeshIntersection(uni.mesh, **kw)
    rows.append(measure("one uniform level", mi_u, uni.table, {"marked": level["marked"], "refine_ms_with_transfers": uni_ms}))
    del mi_u, uni
    torch.cuda.empty_cache()
    t0 = time.perf_counter()
    ada = baking.refine_vertex_baked(mesh, sg, tol, max_levels=1, max_vertices=2 * n_v0, render_step_size=bench.STEP, device=dev)
    torch.cuda.synchronize()
    ada_ms = (time.perf_counter() - t0) * 1e3
    mi_a = MeshIntersection(ada.mesh, **kw)
    rows.append(measure(f"one refine_vertex_baked level, tol {tol}, budget 2 V", mi_a, ada.table,
                        {"marked": ada.levels[0]["marked"], "refine_ms_with_transfers": ada_ms}))
    return {"scene": f"bench scene: {bench.W}x{bench.H}, K={bench.MAX_HITS}, L={lobes}, {n_frames} orbit frames",
            "tol": tol, "edge_errors_of_the_input_mesh": errors,
            "psnr_reference": "FrameRenderer.render of the same SG field on the input mesh (fp32), mean over the frames",
            "cases": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", nargs="*", default=["bench", "configs2"], choices=["bench", "configs2"])
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--frames", type=int, default=6, help="orbit frames of the bench scene; 0 skips the frame part")
    ap.add_argument("--tol", type=float, default=0.01)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "mesh_subdivide", "mesh_subdivide_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mesh_subdivide_bench.py needs the GPU: nothing here is measured on a CPU")
    torch.set_grad_enabled(False)
    warnings.simplefilter("ignore")
    from quadraturefields_amd import _C
    _C.lib()                                   # raises if the library has not been built
    result = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "meshes": [], "frames": None}
    for name in a.meshes:
        row = bench_mesh(name, 12 if name == "bench" else 36, a.iters)
        print(json.dumps(row), flush=True)
        result["meshes"].append(row)
        torch.cuda.empty_cache()
    if a.frames > 0:
        result["frames"] = bench_frames(a.iters, a.frames, a.tol)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
