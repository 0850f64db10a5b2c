"""Decimation of open meshes (boundary = "collapse", include/qf_mesh_decimate_open.h) beside the
default lock mode, on meshes with borders.

    python tools/mesh_decimate_open_bench.py [--iters 5] [--out profiles/mesh_decimate/mesh_decimate_open_bench.json]

* ``lock_closed``: lock mode on the closed bench mesh (``shell_mesh(12, 6)``) to ``F // 10``: wall and per-stage times as
  tools/mesh_decimate_bench.py measures them, for a comparison with that tool run on another build.
* ``open_bench``: the bench mesh without the faces whose centroid has z <= 0, to ``F // 10``, in both modes: faces
  reached, stop reason, rounds, wall time with its host waits (median / min / max of --iters runs after a warm-up),
  per-stage HIP-event times summed over the rounds (the one-off boundary planes are listed on their own), the border
  vertices before and after, and the counts of every round.
* ``masked_bench``: the bench mesh with a seeded 50 % face mask (faces dropped independently, which leaves many bow-tie
  and isolated pieces), the same comparison.
* ``patch_bench``: the bench mesh with the faces kept whose centroid c has ``sin(7 cx + 0.3) sin(7 cy + 1.1)
  sin(7 cz + 2.0) > 0``: about half of the faces, in patches of about 0.45 across with holes between them, the shape a
  visibility prune leaves; the same comparison.
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


def vertex_kinds(v, f):
    """``(border, complex)`` vertex counts of the mesh by step 2's classes, with torch ops."""
    from quadraturefields_amd import mc_utils
    if f.shape[0] == 0:
        return 0, 0
    edges, face_edges, _ = mc_utils.mesh_edges_device(f, v.shape[0])
    uses = torch.bincount(face_edges[face_edges >= 0].reshape(-1), minlength=edges.shape[0])
    nb = torch.bincount(edges[uses == 1].reshape(-1), minlength=v.shape[0])
    bad = torch.bincount(edges[(uses != 1) & (uses != 2)].reshape(-1), minlength=v.shape[0]) > 0
    border = (nb == 2) & ~bad
    return int(border.sum()), int(((nb != 0) & ~border | bad).sum())


def staged_run(v0, f0, target, collapse, weight=1.0):
    """The rounds of ``decimate_mesh_device`` with events around the stages: ``(ms per stage summed over the rounds,
    quadrics ms, boundary planes ms, per-round counts, final face count)``."""
    from quadraturefields_amd import _C, mc_utils
    lib = _C.lib()
    v, f = v0.clone(), f0.clone()
    n_v0 = v.shape[0]
    face_map = torch.arange(f.shape[0], dtype=torch.int64, device="cuda")
    target_map = torch.arange(n_v0, dtype=torch.int64, device="cuda")
    flags = _C.MESH_REMOVE_DEGENERATE | _C.MESH_REMOVE_UNREFERENCED
    names = _C.MESH_COLLAPSE_OPEN_COUNTS if collapse else _C.MESH_COLLAPSE_COUNTS
    size_fn = lib.qf_mesh_decimate_open_workspace_bytes if collapse else lib.qf_mesh_decimate_workspace_bytes

    def workspace(*sizes):
        n = int(size_fn(*sizes))
        return torch.empty((n,), dtype=torch.uint8, device="cuda"), n

    events, rounds = [], []
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    q = torch.empty((v.shape[0], 10), dtype=torch.float64, device="cuda")
    qc = torch.empty((2,), dtype=torch.int64, device="cuda")
    ws, n_ws = workspace(v.shape[0], f.shape[0], 0)
    ev[0].record()
    _C.check(lib.qf_mesh_vertex_quadrics(_C.ptr(v), v.shape[0], _C.ptr(f), f.shape[0], _C.ptr(q), _C.ptr(ws), n_ws, _C.ptr(qc),
                                         _C.stream()), "quadrics")
    ev[1].record()
    planes_ms = 0.0
    for rnd in range(128):
        n_v, n_f = v.shape[0], f.shape[0]
        if n_f <= target:
            break
        e = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        e[0].record()
        edges, face_edges, _ = mc_utils.mesh_edges_device(f, n_v)
        n_e = edges.shape[0]
        ws, n_ws = workspace(n_v, n_f, n_e)
        counts = torch.empty((len(names),), dtype=torch.int64, device="cuda")
        e[1].record()
        if collapse and rnd == 0:
            ev[2].record()
            _C.check(lib.qf_mesh_boundary_quadrics(_C.ptr(v), n_v, _C.ptr(f), n_f, _C.ptr(edges), n_e, _C.ptr(face_edges),
                                                   _C.ptr(q), weight, _C.ptr(ws), n_ws, _C.ptr(qc), _C.stream()), "planes")
            ev[3].record()
        e[5].record()                                           # select starts here: the planes are timed on their own
        if collapse:
            _C.check(lib.qf_mesh_collapse_select_open(_C.ptr(v), n_v, _C.ptr(f), n_f, _C.ptr(edges), n_e, _C.ptr(face_edges),
                                                      _C.ptr(q), None, float("inf"), rnd, n_f - target, _C.ptr(ws), n_ws,
                                                      _C.ptr(counts), _C.stream()), "select")
            e[2].record()
            _C.check(lib.qf_mesh_collapse_apply_open(_C.ptr(v), n_v, _C.ptr(f), n_f, _C.ptr(edges), n_e, _C.ptr(q),
                                                     n_f - target, _C.ptr(target_map), n_v0, _C.ptr(ws), n_ws, _C.stream()),
                     "apply")
        else:
            take = (n_f - target + 1) // 2
            _C.check(lib.qf_mesh_collapse_select(_C.ptr(v), n_v, _C.ptr(f), n_f, _C.ptr(edges), n_e, _C.ptr(face_edges),
                                                 _C.ptr(q), None, float("inf"), rnd, take, _C.ptr(ws), n_ws, _C.ptr(counts),
                                                 _C.stream()), "select")
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
        rounds.append(dict(zip(names, both[8:]), faces_before=n_f, edges=n_e, faces_after=m_f))
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
        _C.check(lib.qf_mesh_collapse_gather(_C.ptr(q), None, _C.ptr(face_map), n_v, n_f, _C.ptr(c_vm), m_v, _C.ptr(c_fm),
                                             m_f, _C.ptr(out_q), None, _C.ptr(out_fm), _C.ptr(target_map), n_v0, _C.ptr(ws), n_ws,
                                             _C.stream()), "gather")
        e[4].record()
        events.append(e)
        v, f, q, face_map = out_v, out_f, out_q, out_fm
    torch.cuda.synchronize()
    spans = {"edges": (0, 1), "select": (5, 2), "apply": (2, 3), "compact": (3, 4)}
    ms = {s: sum(e[a].elapsed_time(e[b]) for e in events) for s, (a, b) in spans.items()}
    if collapse and rounds:
        planes_ms = ev[2].elapsed_time(ev[3])
    return ms, ev[0].elapsed_time(ev[1]), planes_ms, rounds, f.shape[0]


def compare(v, f, target, iters, modes=("lock", "collapse")):
    from quadraturefields_amd import mc_utils
    border, cplx = vertex_kinds(v, f)
    out = {"vertices": v.shape[0], "faces": f.shape[0], "target_faces": target, "border_vertices": border,
           "complex_vertices": cplx}
    for mode in modes:
        wall, res = _wall(lambda: mc_utils.decimate_mesh_device(v, f, target, return_stats=True, boundary=mode), iters)
        runs = [staged_run(v, f, target, mode == "collapse") for _ in range(iters + 1)][1:]
        b_after, c_after = vertex_kinds(res.vertices, res.faces)
        assert runs[0][4] == res.faces.shape[0]
        out[mode] = {"faces_out": res.faces.shape[0], "vertices_out": res.vertices.shape[0], "stop": res.stats["stop"],
                     "rounds": res.stats["rounds"], "border_vertices_out": b_after, "complex_vertices_out": c_after,
                     "boundary_taken": sum(res.stats.get("boundary_taken", [])), "taken": sum(res.stats["taken"]),
                     "wall_ms": wall, "quadrics_ms": _stat([r[1] for r in runs]),
                     "boundary_planes_ms": _stat([r[2] for r in runs]),
                     "stage_ms": {s: _stat([r[0][s] for r in runs]) for s in STAGES}, "per_round": runs[0][3]}
        print(json.dumps({"mode": mode, **{k: out[mode][k] for k in ("faces_out", "stop", "rounds", "border_vertices_out",
                                                                     "wall_ms", "stage_ms")}}))
    return out


def drop_unreferenced(v, f):
    used = torch.zeros(v.shape[0], dtype=torch.bool, device=v.device)
    used[f.reshape(-1)] = True
    return v[used].contiguous(), (torch.cumsum(used, 0) - 1)[f].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_decimate", "mesh_decimate_open_bench.json"))
    args = ap.parse_args()
    from quadraturefields_amd import synthetic
    result = {"device": torch.cuda.get_device_name(0), "iters": args.iters}
    mesh = synthetic.shell_mesh(n_shells=12, subdivisions=6)
    v, f = torch.from_numpy(mesh.vertices).cuda(), torch.from_numpy(mesh.faces).cuda()

    result["lock_closed"] = compare(v, f, f.shape[0] // 10, args.iters, modes=("lock",))
    ov, of = drop_unreferenced(v, f[v[f].mean(dim=1)[:, 2] > 0.0])
    result["open_bench"] = compare(ov, of, of.shape[0] // 10, args.iters)
    keep = torch.rand(f.shape[0], generator=torch.Generator().manual_seed(0)) < 0.5
    mv, mf = drop_unreferenced(v, f[keep.cuda()])
    result["masked_bench"] = compare(mv, mf, mf.shape[0] // 10, args.iters)
    c = v[f].mean(dim=1)
    keep = torch.sin(7.0 * c[:, 0] + 0.3) * torch.sin(7.0 * c[:, 1] + 1.1) * torch.sin(7.0 * c[:, 2] + 2.0) > 0.0
    pv, pf = drop_unreferenced(v, f[keep])
    result["patch_bench"] = compare(pv, pf, pf.shape[0] // 10, args.iters)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
