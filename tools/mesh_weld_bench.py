"""The vertex weld (include/qf_mesh_weld.h) on the bench mesh.

    python tools/mesh_weld_bench.py [--iters 7] [--out profiles/mesh_weld/mesh_weld_bench.json]

Inputs:
* ``soup_exact``: the atlas soup of the bench mesh (``shell_mesh(12, 6)`` unshared as ``uv_atlas.per_triangle_atlas``
  returns it: vertex 3 f + i is corner i of face f; 2 949 120 corners) at ``h == 0``;
* ``soup_tolerance``: the same soup at an ``h`` of one hundredth of the mesh's mean edge;
* ``cut_masked``: the bench mesh under the seeded independent 50 % face mask of tools/mesh_manifold_bench.py, cut by
  ``make_manifold_device``, at ``h == 0``.

Per input, medians of --iters runs after a warm-up, with minimum and maximum: ``count_ms`` / ``emit_ms``
(``qf_mesh_weld_count`` / ``_emit`` under HIP events), ``wrapper_wall_ms`` (``weld_vertices_device`` with its host wait,
wall time), the workspace bytes, the counts, and the baselines on the same input, wall time: for ``h == 0``
``torch_unique_wall_ms`` (``torch.unique(dim=0, return_inverse=True)`` on the same GPU, the input already there) and
``numpy_unique_wall_ms`` (``np.unique(axis=0, return_inverse=True)`` on the host, the input already there); for ``h > 0``
``scipy_wall_ms`` (``cKDTree.query_pairs`` plus ``connected_components`` on the host) if scipy imports, else the entry
``scipy`` says that it does not.  Every baseline's classes are checked equal to the kernels' after renumbering (the lowest
member of every class) before anything is timed."""
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


def _stat(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def _wall(fn, iters, sync=True):
    out = []
    for _ in range(iters + 1):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        if sync:
            torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return _stat(out[1:]), res


def staged(v, f, h):
    """One count and one emit under events: ``(count ms, emit ms, WeldedMesh-like tuple, counts, workspace bytes)``."""
    from quadraturefields_amd import _C
    lib = _C.lib()
    n_v, n_f = v.shape[0], f.shape[0]
    n_ws = int(lib.qf_mesh_weld_workspace_bytes(n_v, n_f))
    ws = torch.empty((n_ws,), dtype=torch.uint8, device="cuda")
    counts = torch.empty((8,), dtype=torch.int64, device="cuda")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    ev[0].record()
    _C.check(lib.qf_mesh_weld_count(_C.ptr(v), n_v, _C.ptr(f), n_f, h, _C.ptr(ws), n_ws, _C.ptr(counts), _C.stream()), "count")
    ev[1].record()
    c = counts.tolist()
    out_v = torch.empty((c[0], 3), dtype=torch.float64, device="cuda")
    out_f = torch.empty((n_f, 3), dtype=torch.int64, device="cuda")
    vmap = torch.empty((c[0],), dtype=torch.int64, device="cuda")
    vcls = torch.empty((n_v,), dtype=torch.int64, device="cuda")
    ev[2].record()
    _C.check(lib.qf_mesh_weld_emit(_C.ptr(v), n_v, _C.ptr(f), n_f, _C.ptr(ws), n_ws, _C.ptr(out_v), c[0], _C.ptr(out_f),
                                   _C.ptr(vmap), _C.ptr(vcls), _C.stream()), "emit")
    ev[3].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]), ev[2].elapsed_time(ev[3]), (out_v, out_f, vmap, vcls), c, n_ws


def torch_unique_labels(v):
    """A class label per vertex at h == 0 from ``torch.unique`` (+ 0.0 makes -0.0 a +0.0)."""
    inverse = torch.unique(v + 0.0, dim=0, return_inverse=True)[1]
    return inverse


def roots_of(labels):
    """Any class labelling renumbered: the lowest member of every vertex's class (torch, on the labels' device)."""
    n = labels.shape[0]
    low = torch.full((int(labels.max()) + 1,), n, dtype=torch.int64, device=labels.device)
    low = low.scatter_reduce(0, labels, torch.arange(n, dtype=torch.int64, device=labels.device), "amin")
    return low[labels]


def numpy_unique_labels(v):
    return np.unique(v + 0.0, axis=0, return_inverse=True)[1].reshape(-1)


def scipy_labels(v, h):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    pairs = cKDTree(v).query_pairs(h, output_type="ndarray")
    n = v.shape[0]
    graph = coo_matrix((np.ones(pairs.shape[0], dtype=np.int8), (pairs[:, 0], pairs[:, 1])), shape=(n, n))
    return connected_components(graph, directed=False)[1]


def measure(v, f, h, iters):
    from quadraturefields_amd import _C, mc_utils
    assert bool(torch.isfinite(v).all())
    _, _, (out_v, out_f, vmap, vcls), counts, n_ws = staged(v, f, h)
    roots = vmap[vcls]
    wrapped = mc_utils.weld_vertices_device(v, f, h, return_stats=True)
    assert torch.equal(wrapped.vertex_class, vcls) and torch.equal(wrapped.faces, out_f)
    assert torch.equal(wrapped.vertices.view(torch.int64), out_v.view(torch.int64))
    host_v = v.cpu().numpy()
    out = {"vertices": v.shape[0], "faces": f.shape[0], "tolerance": h, "workspace_bytes": n_ws,
           "counts": dict(zip(_C.MESH_WELD_COUNTS, counts))}
    if h == 0:
        assert torch.equal(out_v[out_f], v[f]), "the triangle soup changed"
        assert torch.equal(roots_of(torch_unique_labels(v)), roots), "torch.unique != kernels"
        assert np.array_equal(roots_of(torch.from_numpy(numpy_unique_labels(host_v))).numpy(), roots.cpu().numpy()), "np.unique != kernels"
    else:
        try:
            import scipy  # noqa: F401
            have_scipy = True
        except ImportError:
            have_scipy = False
            out["scipy"] = "scipy does not import on this machine: no host baseline for h > 0"
        if have_scipy:
            assert np.array_equal(roots_of(torch.from_numpy(scipy_labels(host_v, h).astype(np.int64))).numpy(),
                                  roots.cpu().numpy()), "scipy != kernels"
    runs = [staged(v, f, h) for _ in range(iters + 1)][1:]
    out["count_ms"] = _stat([r[0] for r in runs])
    out["emit_ms"] = _stat([r[1] for r in runs])
    out["wrapper_wall_ms"] = _wall(lambda: mc_utils.weld_vertices_device(v, f, h), iters)[0]
    print(json.dumps({k: out[k] for k in ("vertices", "tolerance", "counts", "count_ms", "emit_ms", "wrapper_wall_ms")}), flush=True)
    if h == 0:
        out["torch_unique_wall_ms"] = _wall(lambda: torch_unique_labels(v), iters)[0]
        print(json.dumps({"torch_unique_wall_ms": out["torch_unique_wall_ms"]}), flush=True)
        out["numpy_unique_wall_ms"] = _wall(lambda: numpy_unique_labels(host_v), iters, sync=False)[0]
        print(json.dumps({"numpy_unique_wall_ms": out["numpy_unique_wall_ms"]}), flush=True)
    elif "scipy" not in out:
        out["scipy_wall_ms"] = _wall(lambda: scipy_labels(host_v, h), iters, sync=False)[0]
        print(json.dumps({"scipy_wall_ms": out["scipy_wall_ms"]}), flush=True)
    return out


def drop_unreferenced(v, f):
    used = torch.zeros(v.shape[0], dtype=torch.bool, device=v.device)
    used[f.reshape(-1)] = True
    return v[used].contiguous(), (torch.cumsum(used, 0) - 1)[f].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_weld", "mesh_weld_bench.json"))
    args = ap.parse_args()
    from quadraturefields_amd import mc_utils, synthetic
    result = {"device": torch.cuda.get_device_name(0), "iters": args.iters}
    mesh = synthetic.shell_mesh(n_shells=12, subdivisions=6)
    v, f = torch.from_numpy(mesh.vertices).cuda(), torch.from_numpy(mesh.faces).cuda()
    soup_v = v[f].reshape(-1, 3).contiguous()
    soup_f = torch.arange(soup_v.shape[0], dtype=torch.int64, device="cuda").reshape(-1, 3)

    def save():                                                  # after every input, so that a cut-short run leaves what it has
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")

    result["soup_exact"] = measure(soup_v, soup_f, 0.0, args.iters)
    assert result["soup_exact"]["counts"]["vertices"] == v.shape[0], "the soup did not weld back to the mesh's vertices"
    save()
    tri = v[f]
    mean_edge = float(torch.stack([(tri[:, 0] - tri[:, 1]).norm(dim=1), (tri[:, 1] - tri[:, 2]).norm(dim=1),
                                   (tri[:, 2] - tri[:, 0]).norm(dim=1)]).mean())
    result["mean_edge"] = mean_edge
    result["soup_tolerance"] = measure(soup_v, soup_f, mean_edge / 100.0, args.iters)
    save()
    keep = torch.rand(f.shape[0], generator=torch.Generator().manual_seed(0)) < 0.5
    cut = mc_utils.make_manifold_device(*drop_unreferenced(v, f[keep.cuda()]))
    result["cut_masked"] = measure(cut.vertices, cut.faces, 0.0, args.iters)
    save()


if __name__ == "__main__":
    main()
