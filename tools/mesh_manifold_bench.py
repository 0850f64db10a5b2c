"""The manifold repair (include/qf_mesh_manifold.h) on the bench mesh under the three masks of
tools/mesh_decimate_open_bench.py: the half (centroid z > 0), the seeded independent 50 % and the patches.

    python tools/mesh_manifold_bench.py [--iters 7] [--out profiles/mesh_manifold/mesh_manifold_bench.json]

Per mesh, medians of --iters runs after a warm-up, with minimum and maximum:
1. ``count_ms`` / ``emit_ms``: ``qf_mesh_manifold_count`` / ``_emit`` under HIP events; ``edges_wall_ms``: stage A
   (``mesh_edges_device``, one host wait); ``wrapper_wall_ms``: ``make_manifold_device`` with its two host waits (stage A
   included); ``torch_wall_ms``: the same result composed from torch ops on the same GPU, given stage A's ``face_edges``
   (sort, bincount, scatter-min label propagation with pointer jumping, cumsum) -- checked against the kernels, bit for
   bit, before anything is timed.
2. ``decimate``: ``decimate_mesh_device(boundary="collapse")`` to ``F // 10`` of the mesh as it is and of the cut mesh:
   faces reached, stop reason, rounds, wall.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch


def _stat(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def _wall(fn, iters):
    out = []
    for _ in range(iters + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return _stat(out[1:]), res


def torch_cut(v, f, face_edges, n_edges):
    """The rule of section 3.9e from torch ops: ``(out_vertices, out_faces, vertex_map)``.  Valid faces only."""
    n_v, n_f = v.shape[0], f.shape[0]
    ok = (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])
    corner_vertex = f.reshape(-1)
    corner_ok = ok.repeat_interleave(3)
    half = torch.nonzero(corner_ok).reshape(-1)
    e_of = face_edges.reshape(-1)[half]
    uses = torch.bincount(e_of, minlength=n_edges)
    by_edge = half[torch.sort(e_of, stable=True).indices]
    start = torch.cumsum(uses, 0) - uses
    pair = torch.nonzero(uses == 2).reshape(-1)
    h0, h1 = by_edge[start[pair]], by_edge[start[pair] + 1]

    def nxt(h):
        k = h % 3
        return h - k + (k + 1) % 3

    a0, a1, b0, b1 = h0, nxt(h0), h1, nxt(h1)
    same = (corner_vertex[a0] == corner_vertex[b0]) & (corner_vertex[a1] == corner_vertex[b1])
    opposite = (corner_vertex[a0] == corner_vertex[b1]) & (corner_vertex[a1] == corner_vertex[b0])
    a = torch.cat([a0[same], a1[same], a0[opposite], a1[opposite]])
    b = torch.cat([b0[same], b1[same], b1[opposite], b0[opposite]])
    corner = torch.arange(3 * n_f, dtype=torch.int64, device=f.device)
    lab = corner.clone()
    while True:                                                  # the lowest corner of every class
        m = torch.minimum(lab[a], lab[b])
        lab = lab.scatter_reduce(0, a, m, "amin").scatter_reduce(0, b, m, "amin")
        jumped = lab[lab]
        if torch.equal(jumped, lab) and torch.equal(jumped[a], jumped[b]):
            break
        lab = jumped
    is_root = corner_ok & (lab == corner)
    vmin = torch.full((n_v,), 3 * n_f, dtype=torch.int64, device=f.device)
    vmin = vmin.scatter_reduce(0, corner_vertex[is_root], corner[is_root], "amin")
    extra = is_root & (corner != vmin[corner_vertex])
    rank = torch.cumsum(extra, 0) - extra.to(torch.int64)
    index = torch.where(corner_ok & (lab != vmin[corner_vertex]), n_v + rank[lab], corner_vertex)
    vertex_map = torch.cat([torch.arange(n_v, dtype=torch.int64, device=f.device), corner_vertex[extra]])
    return v[vertex_map], index.reshape(n_f, 3), vertex_map


def staged(v, f, face_edges, n_e):
    """One count and one emit under events: ``(count ms, emit ms, out_vertices, out_faces, vertex_map, counts)``."""
    from quadraturefields_amd import _C
    lib = _C.lib()
    n_v, n_f = v.shape[0], f.shape[0]
    n_ws = int(lib.qf_mesh_manifold_workspace_bytes(n_v, n_f, n_e))
    ws = torch.empty((n_ws,), dtype=torch.uint8, device="cuda")
    counts = torch.empty((8,), dtype=torch.int64, device="cuda")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    ev[0].record()
    _C.check(lib.qf_mesh_manifold_count(_C.ptr(f), n_f, n_v, _C.ptr(face_edges), n_e, _C.ptr(ws), n_ws, _C.ptr(counts),
                                        _C.stream()), "count")
    ev[1].record()
    c = counts.tolist()
    out_v = torch.empty((c[0], 3), dtype=torch.float64, device="cuda")
    out_f = torch.empty((n_f, 3), dtype=torch.int64, device="cuda")
    vmap = torch.empty((c[0],), dtype=torch.int64, device="cuda")
    ev[2].record()
    _C.check(lib.qf_mesh_manifold_emit(_C.ptr(v), _C.ptr(f), n_f, n_v, _C.ptr(ws), n_ws, _C.ptr(out_v), c[0], _C.ptr(out_f),
                                       _C.ptr(vmap), _C.stream()), "emit")
    ev[3].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]), ev[2].elapsed_time(ev[3]), out_v, out_f, vmap, c, n_ws


def bits(t):
    return t.contiguous().view(torch.int64)


def measure(v, f, iters):
    from quadraturefields_amd import _C, mc_utils
    numbered = mc_utils.mesh_edges_device(f, v.shape[0])
    face_edges, n_e = numbered.face_edges, numbered.stats["edges"]
    _, _, out_v, out_f, vmap, counts, n_ws = staged(v, f, face_edges, n_e)
    t_v, t_f, t_map = torch_cut(v, f, face_edges, n_e)
    assert torch.equal(bits(t_v), bits(out_v)) and torch.equal(t_f, out_f) and torch.equal(t_map, vmap), "torch != kernels"
    wrapped = mc_utils.make_manifold_device(v, f, return_stats=True)
    assert torch.equal(bits(wrapped.vertices), bits(out_v)) and torch.equal(wrapped.faces, out_f)
    assert torch.equal(bits(out_v[out_f]), bits(v[f])), "the triangle soup changed"
    runs = [staged(v, f, face_edges, n_e) for _ in range(iters + 1)][1:]
    out = {"vertices": v.shape[0], "faces": f.shape[0], "edges": n_e, "workspace_bytes": n_ws,
           "counts": dict(zip(_C.MESH_MANIFOLD_COUNTS, counts)),
           "count_ms": _stat([r[0] for r in runs]), "emit_ms": _stat([r[1] for r in runs]),
           "edges_wall_ms": _wall(lambda: mc_utils.mesh_edges_device(f, v.shape[0]), iters)[0],
           "wrapper_wall_ms": _wall(lambda: mc_utils.make_manifold_device(v, f), iters)[0],
           "torch_wall_ms": _wall(lambda: torch_cut(v, f, face_edges, n_e), iters)[0]}
    print(json.dumps({k: out[k] for k in ("faces", "counts", "count_ms", "emit_ms", "wrapper_wall_ms", "torch_wall_ms")}), flush=True)
    target = f.shape[0] // 10
    out["decimate"] = {"target_faces": target}
    for name, (dv, df) in (("as_it_is", (v, f)), ("cut", (out_v, out_f))):
        wall, res = _wall(lambda: mc_utils.decimate_mesh_device(dv, df, target, return_stats=True, boundary="collapse"), iters)
        out["decimate"][name] = {"faces_out": res.faces.shape[0], "vertices_out": res.vertices.shape[0],
                                 "stop": res.stats["stop"], "rounds": res.stats["rounds"], "wall_ms": wall}
        print(json.dumps({name: out["decimate"][name]}), flush=True)
    return out


def drop_unreferenced(v, f):
    used = torch.zeros(v.shape[0], dtype=torch.bool, device=v.device)
    used[f.reshape(-1)] = True
    return v[used].contiguous(), (torch.cumsum(used, 0) - 1)[f].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_manifold", "mesh_manifold_bench.json"))
    args = ap.parse_args()
    from quadraturefields_amd import synthetic
    result = {"device": torch.cuda.get_device_name(0), "iters": args.iters}
    mesh = synthetic.shell_mesh(n_shells=12, subdivisions=6)
    v, f = torch.from_numpy(mesh.vertices).cuda(), torch.from_numpy(mesh.faces).cuda()
    c = v[f].mean(dim=1)
    result["half_bench"] = measure(*drop_unreferenced(v, f[c[:, 2] > 0.0]), args.iters)
    keep = torch.rand(f.shape[0], generator=torch.Generator().manual_seed(0)) < 0.5
    result["masked_bench"] = measure(*drop_unreferenced(v, f[keep.cuda()]), args.iters)
    keep = torch.sin(7.0 * c[:, 0] + 0.3) * torch.sin(7.0 * c[:, 1] + 1.1) * torch.sin(7.0 * c[:, 2] + 2.0) > 0.0
    result["patch_bench"] = measure(*drop_unreferenced(v, f[keep]), args.iters)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
