"""Mesh decimation (qf_mesh_vertex_quadrics / qf_mesh_collapse_*) on the bench mesh, per stage
and as a whole, the numpy restatement's time on a small sphere, and the geometric error beside vertex clustering's.

    python tools/mesh_decimate_bench.py [--iters 7] [--vx 40] [--vx_sphere 8]
                                        [--out profiles/mesh_decimate/mesh_decimate_bench.json]

* ``bench``: the 983 040-triangle bench mesh (``shell_mesh(12, 6)``) to ``F // 10``.  ``wall_ms``:
  ``mc_utils.decimate_mesh_device`` with its host waits, a host clock around work that ends in a synchronise, median /
  min / max of --iters runs after one warm-up.  ``stage_ms``: the same rounds issued from here with HIP events around the
  four stages of every round (edges: count, wait, emit; select; apply; compact: count, wait, emit, gather), summed over the
  rounds, median / min / max likewise; the waits fall inside the edges and compact intervals.  ``per_round`` has the counts
  of every round and ``selected_share`` = selected / legal candidates.
* ``restatement``: ``tests/mesh_decimate_reference.decimate`` on the level-5 icosphere (20 480 faces) to ``F // 10``, one
  run, and the device's wall time on the same mesh.  No other baseline exists here; nothing is claimed about
  fast_simplification.
* ``error``: ``mc_utils.simplify_vertex_clustering`` (quadric contraction) at voxel size ``1 / vx`` (bench mesh) and
  ``1 / vx_sphere`` (sphere: the voxel has to be larger than its triangles to remove any) against decimation to the face
  count that clustering produced.  Level-5 sphere: max and mean of ``| |v| - 1 |`` over the output vertices.  Bench
  mesh (not analytic): the mean distance from an output vertex to the nearest input vertex.
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

STAGES = ("edges", "select", "apply", "compact")


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


def staged_run(v0, f0, target):
    """The rounds of ``decimate_mesh_device`` (no lock, no cost limit) with events around the stages: ``(ms per stage
    summed over the rounds, quadrics ms, per-round counts, final face count)``."""
    from quadraturefields_amd import _C, mc_utils
    lib = _C.lib()
    v, f = v0.clone(), f0.clone()
    n_v0 = v.shape[0]
    face_map = torch.arange(f.shape[0], dtype=torch.int64, device="cuda")
    target_map = torch.arange(n_v0, dtype=torch.int64, device="cuda")
    flags = _C.MESH_REMOVE_DEGENERATE | _C.MESH_REMOVE_UNREFERENCED

    def workspace(*sizes):
        n = int(lib.qf_mesh_decimate_workspace_bytes(*sizes))
        return torch.empty((n,), dtype=torch.uint8, device="cuda"), n

    events, rounds = [], []
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    q = torch.empty((v.shape[0], 10), dtype=torch.float64, device="cuda")
    qc = torch.empty((2,), dtype=torch.int64, device="cuda")
    ws, n_ws = workspace(v.shape[0], f.shape[0], 0)
    ev[0].record()
    _C.check(lib.qf_mesh_vertex_quadrics(_C.ptr(v), v.shape[0], _C.ptr(f), f.shape[0], _C.ptr(q), _C.ptr(ws), n_ws, _C.ptr(qc),
                                         _C.stream()), "quadrics")
    ev[1].record()
    lock = None
    for rnd in range(128):
        n_v, n_f = v.shape[0], f.shape[0]
        if n_f <= target:
            break
        e = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        e[0].record()
        edges, face_edges, _ = mc_utils.mesh_edges_device(f, n_v)
        n_e = edges.shape[0]
        take = (n_f - target + 1) // 2
        ws, n_ws = workspace(n_v, n_f, n_e)
        counts = torch.empty((6,), dtype=torch.int64, device="cuda")
        e[1].record()
        _C.check(lib.qf_mesh_collapse_select(_C.ptr(v), n_v, _C.ptr(f), n_f, _C.ptr(edges), n_e, _C.ptr(face_edges), _C.ptr(q),
                                             None, float("inf"), rnd, take, _C.ptr(ws), n_ws, _C.ptr(counts), _C.stream()),
                 "select")
        e[2].record()
        _C.check(lib.qf_mesh_collapse_apply(_C.ptr(v), n_v, _C.ptr(f), n_f, _C.ptr(edges), n_e, _C.ptr(q), take,
                                            _C.ptr(target_map), n_v0, _C.ptr(ws), n_ws, _C.stream()), "apply")
        e[3].record()
        c_n = int(lib.qf_mesh_compact_workspace_bytes(n_v, n_f))
        c_ws = torch.empty((c_n,), dtype=torch.uint8, device="cuda")
        c_counts = torch.empty((8,), dtype=torch.int64, device="cuda")
        c_args = (_C.ptr(v), n_v, _C.ptr(f), n_f, None, flags, 0, _C.ptr(c_ws), c_n)
        _C.check(lib.qf_mesh_compact_count(*c_args, _C.ptr(c_counts), _C.stream()), "compact count")
        both = torch.cat([c_counts, counts]).tolist()
        m_f, m_v = both[0], both[1]
        rounds.append(dict(zip(_C.MESH_COLLAPSE_COUNTS, both[8:]), faces_before=n_f, edges=n_e, faces_after=m_f))
        if both[8 + 3] == 0:
            break
        out_v = torch.empty((m_v, 3), dtype=torch.float64, device="cuda")
        out_f = torch.empty((m_f, 3), dtype=torch.int64, device="cuda")
        c_fm = torch.empty((m_f,), dtype=torch.int64, device="cuda")
        c_vm = torch.empty((m_v,), dtype=torch.int64, device="cuda")
        _C.check(lib.qf_mesh_compact_emit(*c_args, _C.ptr(out_v), m_v, _C.ptr(out_f), m_f, _C.ptr(c_fm), _C.ptr(c_vm),
                                          _C.stream()), "compact emit")
        out_q = torch.empty((m_v, 10), dtype=torch.float64, device="cuda")
        out_fm = torch.empty((m_f,), dtype=torch.int64, device="cuda")
        _C.check(lib.qf_mesh_collapse_gather(_C.ptr(q), _C.ptr(lock), _C.ptr(face_map), n_v, n_f, _C.ptr(c_vm), m_v, _C.ptr(c_fm),
                                             m_f, _C.ptr(out_q), None, _C.ptr(out_fm), _C.ptr(target_map), n_v0, _C.ptr(ws), n_ws,
                                             _C.stream()), "gather")
        e[4].record()
        events.append(e)
        v, f, q, face_map = out_v, out_f, out_q, out_fm
    torch.cuda.synchronize()
    ms = {s: sum(e[i].elapsed_time(e[i + 1]) for e in events) for i, s in enumerate(STAGES)}
    return ms, ev[0].elapsed_time(ev[1]), rounds, f.shape[0]


def nearest_vertex_mean(out_v, in_v, chunk=1024):
    """Mean distance from each row of out_v to its nearest row of in_v (fp32 on the device, in chunks)."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_decimate", "mesh_decimate_bench.json"))
    args = ap.parse_args()
    from quadraturefields_amd import mc_utils, synthetic
    from tests import mesh_decimate_reference as ref
    result = {"device": torch.cuda.get_device_name(0), "iters": args.iters}

    mesh = synthetic.shell_mesh(n_shells=12, subdivisions=6)
    v, f = torch.from_numpy(mesh.vertices).cuda(), torch.from_numpy(mesh.faces).cuda()
    target = f.shape[0] // 10
    wall, out = _wall(lambda: mc_utils.decimate_mesh_device(v, f, target, return_stats=True), args.iters)
    runs = [staged_run(v, f, target) for _ in range(args.iters + 1)][1:]
    rounds = runs[0][2]
    for r in rounds:
        r["selected_share"] = r["selected"] / max(r["legal"], 1)
    result["bench"] = {
        "vertices": v.shape[0], "faces": f.shape[0], "target_faces": target, "faces_out": out.faces.shape[0],
        "vertices_out": out.vertices.shape[0], "rounds": out.stats["rounds"], "stop": out.stats["stop"], "wall_ms": wall,
        "quadrics_ms": _stat([r[1] for r in runs]),
        "stage_ms": {s: _stat([r[0][s] for r in runs]) for s in STAGES},
        "stage_ms_per_round": {s: _stat([r[0][s] / max(len(r[2]), 1) for r in runs]) for s in STAGES},
        "per_round": rounds,
        "selected_share": _stat([r["selected_share"] for r in rounds]),
    }
    print(json.dumps({k: result["bench"][k] for k in ("rounds", "faces_out", "wall_ms", "stage_ms", "selected_share")}))

    sv, sf = ref.icosphere(5)
    t0 = time.perf_counter()
    want = ref.decimate(sv, sf, sf.shape[0] // 10)
    numpy_ms = (time.perf_counter() - t0) * 1e3
    dsv, dsf = torch.from_numpy(sv).cuda(), torch.from_numpy(sf).cuda()
    s_wall, s_out = _wall(lambda: mc_utils.decimate_mesh_device(dsv, dsf, sf.shape[0] // 10, return_stats=True), args.iters)
    result["restatement"] = {"mesh": "icosphere level 5", "faces": int(sf.shape[0]), "target_faces": int(sf.shape[0] // 10),
                             "rounds": want[4]["rounds"], "numpy_wall_ms": numpy_ms, "device_wall_ms": s_wall,
                             "same_bytes": bool(s_out.vertices.cpu().numpy().tobytes() == want[0].tobytes()
                                                and np.array_equal(s_out.faces.cpu().numpy(), want[1]))}
    print(json.dumps(result["restatement"]))

    def radial(x):
        r = (x.norm(dim=1) - 1.0).abs()
        return {"max": float(r.max()), "mean": float(r.mean())}

    cv, cf = mc_utils.simplify_vertex_clustering(dsv, dsf, 1.0 / args.vx_sphere, "quadric")
    d = mc_utils.decimate_mesh_device(dsv, dsf, cf.shape[0])
    error = {"vx": args.vx, "vx_sphere": args.vx_sphere, "sphere": {"clustering": dict(radial(cv), faces=cf.shape[0], vertices=cv.shape[0]),
                                       "decimation": dict(radial(d.vertices), faces=d.faces.shape[0], vertices=d.vertices.shape[0])}}
    cv, cf = mc_utils.simplify_vertex_clustering(v, f, 1.0 / args.vx, "quadric")
    d = mc_utils.decimate_mesh_device(v, f, cf.shape[0], return_stats=True)
    error["bench"] = {"clustering": {"faces": cf.shape[0], "vertices": cv.shape[0], "mean_nearest_vertex": nearest_vertex_mean(cv, v)},
                      "decimation": {"faces": d.faces.shape[0], "vertices": d.vertices.shape[0], "rounds": d.stats["rounds"],
                                     "stop": d.stats["stop"], "mean_nearest_vertex": nearest_vertex_mean(d.vertices, v)}}
    result["error"] = error
    print(json.dumps(error))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
