"""Mesh clean-up (qf_mesh_compact_count / qf_mesh_compact_emit) and qf_mark_hit_faces per call, against the same results
composed from torch ops on the same GPU and from numpy on the host.

    python tools/mesh_compact_bench.py [--meshes bench configs2] [--iters 7] [--out profiles/mesh_compact/mesh_compact_bench.json]

Meshes: the 983 040-triangle bench mesh (``shell_mesh(12, 6)``) and the configs[2] mesh (``shell_mesh(36, 6)``), each under
a seeded 50 % keep mask, duplicates removed, islands below 16 faces dropped, unreferenced vertices removed.  The mask
frame is 800 x 800 rays of the bench camera at K = 25 through the intersector's id lists.

* ``count_ms`` / ``emit_ms``: HIP events around the C calls.  ``wrapper_ms``: ``mc_utils.compact_mesh_device`` (count, the
  read-back of the counts, allocation, emit), a host clock around work that ends in a synchronise.
* ``torch_ms``: the same mesh from torch ops -- boolean indexing, ``torch.unique(dim=0)`` on the sorted triples, components
  by min-label propagation with pointer jumping (``scatter_reduce`` until nothing changes), ``torch.unique`` on the
  indices -- with a synchronise at the end.  ``numpy_ms``: the same on the host (``np.unique``; components by scipy's
  ``connected_components`` where scipy imports, else the same propagation), inputs already on the host.
* The baselines' results are compared with the kernels' (faces and vertex map equal) before anything is timed.
Every time is the median of --iters runs after one warm-up, with the minimum and maximum beside it.
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

M = 16


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


def time_calls(v, f, keep, iters):
    from quadraturefields_amd import _C
    lib = _C.lib()
    n_v, n_f = v.shape[0], f.shape[0]
    ws_bytes = int(lib.qf_mesh_compact_workspace_bytes(n_v, n_f))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device="cuda")
    counts = torch.empty((8,), dtype=torch.int64, device="cuda")
    args = (_C.ptr(v), n_v, _C.ptr(f), n_f, _C.ptr(keep), 7, M, _C.ptr(ws), ws_bytes)
    _C.check(lib.qf_mesh_compact_count(*args, _C.ptr(counts), _C.stream()), "count")
    c = counts.tolist()
    out_v = torch.empty((c[1], 3), dtype=torch.float64, device="cuda")
    out_f = torch.empty((c[0], 3), dtype=torch.int64, device="cuda")
    fm = torch.empty((c[0],), dtype=torch.int64, device="cuda")
    vm = torch.empty((c[1],), dtype=torch.int64, device="cuda")
    t_count, t_emit = [], []
    for _ in range(iters + 1):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        _C.check(lib.qf_mesh_compact_count(*args, _C.ptr(counts), _C.stream()), "count")
        e[1].record()
        _C.check(lib.qf_mesh_compact_emit(*args, _C.ptr(out_v), c[1], _C.ptr(out_f), c[0], _C.ptr(fm), _C.ptr(vm),
                                          _C.stream()), "emit")
        e[2].record()
        torch.cuda.synchronize()
        t_count.append(e[0].elapsed_time(e[1]))
        t_emit.append(e[1].elapsed_time(e[2]))
    return dict(zip(_C.MESH_COMPACT_COUNTS, c)), ws_bytes, _stat(t_count[1:]), _stat(t_emit[1:]), (out_f, vm)


def _propagate(labels, faces, xp):
    """Min-label propagation over the faces with pointer jumping until nothing changes (torch or numpy)."""
    flat = faces.reshape(-1)
    while True:
        if xp is torch:
            m = labels[faces].amin(dim=1).repeat_interleave(3)
            new = labels.scatter_reduce(0, flat, m, "amin")
            new = new[new]
            if torch.equal(new, labels):
                return labels
        else:
            m = np.repeat(labels[faces].min(axis=1), 3)
            new = labels.copy()
            np.minimum.at(new, flat, m)
            new = new[new]
            if np.array_equal(new, labels):
                return labels
        labels = new


def torch_compose(v, f, keep):
    kept = torch.nonzero(keep).reshape(-1)
    fk = f[kept]
    tri = fk.sort(dim=1).values
    good = (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2])
    kept, fk, tri = kept[good], fk[good], tri[good]
    _, inverse = torch.unique(tri, dim=0, return_inverse=True)
    first = torch.full((int(inverse.max()) + 1 if inverse.numel() else 0,), fk.shape[0], dtype=torch.int64, device=f.device)
    first.scatter_reduce_(0, inverse, torch.arange(fk.shape[0], device=f.device), "amin")
    first = first.sort().values
    kept, fk = kept[first], fk[first]
    labels = _propagate(torch.arange(v.shape[0], device=f.device), fk, torch)
    face_label = labels[fk[:, 0]]
    size = torch.zeros(v.shape[0], dtype=torch.int64, device=f.device).index_add_(0, face_label, torch.ones_like(face_label))
    big = size[face_label] >= M
    kept, fk = kept[big], fk[big]
    vmap, inv = torch.unique(fk, return_inverse=True)
    return v[vmap], inv.reshape(-1, 3), kept, vmap


def numpy_compose(v, f, keep):
    kept = np.nonzero(keep)[0]
    fk = f[kept]
    tri = np.sort(fk, axis=1)
    good = (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2])
    kept, fk, tri = kept[good], fk[good], tri[good]
    _, first = np.unique(tri, axis=0, return_index=True)
    first.sort()
    kept, fk = kept[first], fk[first]
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        rows, cols = np.concatenate([fk[:, 0], fk[:, 1]]), np.concatenate([fk[:, 1], fk[:, 2]])
        n = v.shape[0]
        labels = connected_components(coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(n, n)), directed=False)[1]
    except ImportError:
        labels = _propagate(np.arange(v.shape[0]), fk, np)
    face_label = labels[fk[:, 0]]
    big = np.bincount(face_label, minlength=v.shape[0])[face_label] >= M
    kept, fk = kept[big], fk[big]
    vmap, inv = np.unique(fk, return_inverse=True)
    return v[vmap], inv.reshape(-1, 3), kept, vmap


def bench_mesh(name, shells, iters):
    from quadraturefields_amd import mc_utils, synthetic
    mesh = synthetic.shell_mesh(n_shells=shells, subdivisions=6)
    rng = np.random.default_rng(42)
    keep_np = (rng.random(mesh.faces.shape[0]) < 0.5).astype(np.uint8)
    v, f, keep = (torch.from_numpy(a).cuda() for a in (mesh.vertices, mesh.faces, keep_np))
    stats, ws_bytes, t_count, t_emit, (out_f, vm) = time_calls(v, f, keep, iters)
    tv, tf, tkept, tvm = torch_compose(v, f, keep)
    assert torch.equal(tf, out_f) and torch.equal(tvm, vm), "the torch composition disagrees with the kernels"
    nv, nf, nkept, nvm = numpy_compose(mesh.vertices, mesh.faces, keep_np)
    assert np.array_equal(nf, out_f.cpu().numpy()) and np.array_equal(nvm, vm.cpu().numpy()), "numpy disagrees"
    options = dict(remove_degenerate=True, remove_duplicates=True, min_component_faces=M, remove_unreferenced=True)
    row = {"mesh": name, "V": int(v.shape[0]), "F": int(f.shape[0]), "min_component_faces": M, "flags": "all", "counts": stats,
           "workspace_bytes": ws_bytes, "count_ms": t_count, "emit_ms": t_emit,
           "wrapper_ms": _timed(lambda: mc_utils.compact_mesh_device(v, f, keep, **options), iters),
           "torch_ms": _timed(lambda: torch_compose(v, f, keep), iters)}
    t = []
    for _ in range(max(iters // 2, 2) + 1):
        t0 = time.perf_counter()
        numpy_compose(mesh.vertices, mesh.faces, keep_np)
        t.append((time.perf_counter() - t0) * 1e3)
    row["numpy_ms"] = _stat(t[1:])
    return row, mesh


def bench_mark(mesh, iters):
    from quadraturefields_amd import mc_utils, synthetic
    from quadraturefields_amd.mesh_utils import RayIntersector
    w = h = 800
    k = 25
    c2w = synthetic.orbit_cameras(1)[0]
    o, d = synthetic.camera_rays(c2w, synthetic.lego_focal(w), w, h, device="cuda")
    ri = RayIntersector(mesh, max_hits=k, device="cuda:0")
    hit_tri, _, hit_count, _, _ = ri.hits(o, d, k)
    n_faces = mesh.faces.shape[0]
    mask = torch.zeros((n_faces,), dtype=torch.uint8, device="cuda")
    bad = torch.zeros((1,), dtype=torch.int64, device="cuda")
    t = []
    for _ in range(iters + 1):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        mask.zero_()
        e[0].record()
        mc_utils.mark_hit_faces(hit_tri, hit_count, mask, bad)
        e[1].record()
        torch.cuda.synchronize()
        t.append(e[0].elapsed_time(e[1]))

    def torch_mark():
        ok = torch.arange(k, device="cuda")[None, :] < hit_count.clamp(max=k)[:, None]
        m = torch.zeros((n_faces,), dtype=torch.uint8, device="cuda")
        m[torch.unique(hit_tri[ok].long())] = 1
        return m

    assert torch.equal(torch_mark(), mask) and int(bad.item()) == 0
    tri_np, count_np = hit_tri.cpu().numpy(), hit_count.cpu().numpy()

    def numpy_mark():
        ok = np.arange(k)[None, :] < np.minimum(count_np, k)[:, None]
        m = np.zeros(n_faces, np.uint8)
        m[np.unique(tri_np[ok])] = 1
        return m

    assert np.array_equal(numpy_mark(), mask.cpu().numpy())
    tn = []
    for _ in range(iters + 1):
        t0 = time.perf_counter()
        numpy_mark()
        tn.append((time.perf_counter() - t0) * 1e3)
    return {"frame": f"{w}x{h}", "max_hits": k, "F": int(n_faces), "hits": int(hit_count.clamp(max=k).sum()),
            "faces_marked": int(mask.sum()), "mark_hit_faces_ms": _stat(t[1:]), "torch_ms": _timed(torch_mark, iters),
            "numpy_ms": _stat(tn[1:])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", nargs="+", default=["bench", "configs2"], choices=["bench", "configs2"])
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "mesh_compact", "mesh_compact_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mesh_compact_bench.py needs the GPU: nothing here is measured on a CPU")
    from quadraturefields_amd import _C
    _C.lib()                                   # raises if the library has not been built
    result ={"device": torch.cuda.get_device_name(0), "iters": a.iters, "compact": [], "mark_hit_faces": None}
    for name in a.meshes:
        row, mesh = bench_mesh(name, 12 if name == "bench" else 36, a.iters)
        print(json.dumps(row), flush=True)
        result["compact"].append(row)
        if name == "bench":
            result["mark_hit_faces"] = bench_mark(mesh, a.iters)
            print(json.dumps(result["mark_hit_faces"]), flush=True)
        del mesh
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
