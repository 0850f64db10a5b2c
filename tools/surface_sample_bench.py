"""Surface sampling (include/qf_mesh_sample.h) on the bench mesh.

    python tools/surface_sample_bench.py [--iters 7] [--out profiles/surface_sample/surface_sample_bench.json]

On the 983 040-face bench mesh (``shell_mesh(12, 6)``), medians of --iters runs after a warm-up, with minimum and maximum:

* ``prepare_ms`` (``qf_mesh_sample_prepare`` under HIP events) and, for N = 2^17 and 2^20, ``emit_ms``
  (``qf_mesh_sample_emit`` under HIP events) and ``wrapper_wall_ms`` (``sample_surface_device`` with its allocations and
  its host wait, wall time);
* ``torch_wall_ms``: the only baseline, a torch composition on the same GPU in the same run -- areas from a cross product,
  ``cumsum``, ``rand``, ``searchsorted``, the square-root barycentrics, three gathers -- wall time, synchronised.  It
  draws plain (unstratified) uniform samples with torch's generator, so it computes something else; its bytes are not
  comparable;
* ``surface_distance``: section 3.9f's table again (``simplify_vertex_clustering`` against ``decimate_mesh_device`` to
  the face count clustering produced, each output against the input, on the level-5 sphere and the bench mesh) with
  ``samples=2^20`` beside the vertex-and-centroid figures, and the wall time of each ``mesh_distance_device`` call."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

SIZES = (2 ** 17, 2 ** 20)
DISTANCE_SAMPLES = 2 ** 20


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


class Staged:
    def __init__(self, v, f):
        from quadraturefields_amd import _C
        self.C, self.lib, self.v, self.f = _C, _C.lib(), v, f
        self.n_v, self.n_f = v.shape[0], f.shape[0]
        self.bytes = int(self.lib.qf_mesh_sample_workspace_bytes(self.n_v, self.n_f))
        self.ws = torch.empty((self.bytes,), dtype=torch.uint8, device="cuda")
        self.counts = torch.empty((6,), dtype=torch.int64, device="cuda")

    def prepare(self):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        self.C.check(self.lib.qf_mesh_sample_prepare(self.C.ptr(self.v), self.n_v, self.C.ptr(self.f), self.n_f, None,
                                                     self.C.ptr(self.ws), self.bytes, self.C.ptr(self.counts), self.C.stream()),
                     "prepare")
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    def emit(self, n, seed, out):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        self.C.check(self.lib.qf_mesh_sample_emit(self.C.ptr(self.v), self.n_v, self.C.ptr(self.f), self.n_f, self.C.ptr(self.ws),
                                                  self.bytes, n, seed, self.C.ptr(out[0]), self.C.ptr(out[1]), self.C.ptr(out[2]),
                                                  self.C.stream()), "emit")
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])


def torch_composition(v, f, n, generator):
    """Plain area-weighted sampling in torch: the baseline."""
    corners = v[f]
    a, b, c = corners[:, 0], corners[:, 1], corners[:, 2]
    cum = torch.linalg.cross(b - a, c - a).norm(dim=1).cumsum(0)
    r = torch.rand((n, 3), dtype=torch.float64, device=v.device, generator=generator)
    face = torch.searchsorted(cum, r[:, 0] * cum[-1], right=True).clamp_(max=f.shape[0] - 1)
    s = r[:, 1].sqrt()
    bary = torch.stack([1.0 - s, s * (1.0 - r[:, 2]), s * r[:, 2]], dim=1)
    points = (corners[face] * bary[:, :, None]).sum(dim=1)
    return points, face, bary


def nearest_is_on_the_face(v, f, out):
    """Every point is the barycentric blend of its face's corners, to rounding."""
    points, face, bary = out
    again = (v[f[face]] * bary[:, :, None]).sum(dim=1)
    return float((again - points).abs().max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--vx", type=float, default=40.0)
    ap.add_argument("--vx_sphere", type=float, default=8.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_sample", "surface_sample_bench.json"))
    args = ap.parse_args()
    from quadraturefields_amd import _C, mc_utils, synthetic
    from tests import mesh_sample_reference as ref
    result = {"device": torch.cuda.get_device_name(0), "iters": args.iters}

    def save():                                                  # after every part, so that a cut-short run leaves what it has
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")

    mesh = synthetic.shell_mesh(n_shells=12, subdivisions=6)
    v, f = torch.from_numpy(mesh.vertices).cuda(), torch.from_numpy(mesh.faces).cuda()
    st = Staged(v, f)
    result.update(vertices=st.n_v, faces=st.n_f, workspace_bytes=st.bytes)
    result["prepare_ms"] = _stat([st.prepare() for _ in range(args.iters + 1)][1:])
    result["counts"] = dict(zip(_C.MESH_SAMPLE_COUNTS, st.counts.tolist()))
    print(json.dumps({k: result[k] for k in ("faces", "workspace_bytes", "prepare_ms", "counts")}), flush=True)
    generator = torch.Generator(device="cuda").manual_seed(0)
    for n in SIZES:
        out = (torch.empty((n, 3), dtype=torch.float64, device="cuda"), torch.empty((n,), dtype=torch.int64, device="cuda"),
               torch.empty((n, 3), dtype=torch.float64, device="cuda"))
        entry = {"emit_ms": _stat([st.emit(n, 0, out) for _ in range(args.iters + 1)][1:])}
        wrapped = mc_utils.sample_surface_device(v, f, n, 0)
        assert all(torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(out, wrapped))
        entry["blend_max_abs_difference"] = nearest_is_on_the_face(v, f, out)
        entry["faces_sampled"] = int(torch.unique(out[1]).shape[0])
        entry["wrapper_wall_ms"] = _wall(lambda: mc_utils.sample_surface_device(v, f, n, 0), args.iters)[0]
        entry["torch_wall_ms"] = _wall(lambda: torch_composition(v, f, n, generator), args.iters)[0]
        result[f"n_{n}"] = entry
        print(json.dumps({f"n_{n}": entry}), flush=True)
        save()
    # the restatement on the bench mesh itself, once: the same bytes at N = 2^17
    n = SIZES[0]
    want = ref.sample(mesh.vertices, mesh.faces, n, 0)
    got = mc_utils.sample_surface_device(v, f, n, 0)
    result["restatement_same_bytes"] = bool(got.points.cpu().numpy().tobytes() == want[0].tobytes()
                                            and got.face.cpu().numpy().tobytes() == want[1].tobytes()
                                            and got.bary.cpu().numpy().tobytes() == want[2].tobytes())
    print(json.dumps({"restatement_same_bytes": result["restatement_same_bytes"]}), flush=True)
    save()

    def compare(vin, fin, voxel):
        cv, cf = mc_utils.simplify_vertex_clustering(vin, fin, voxel, "quadric")
        d = mc_utils.decimate_mesh_device(vin, fin, cf.shape[0])
        out = {}
        for name, (ov, of) in (("clustering", (cv, cf)), ("decimation", (d.vertices, d.faces))):
            entry = {"faces": int(of.shape[0]), "vertices": int(ov.shape[0])}
            for key, samples in (("vertices_and_centroids", None), ("sampled", DISTANCE_SAMPLES)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m = mc_utils.mesh_distance_device(ov, of, vin, fin, samples=samples)
                wall = (time.perf_counter() - t0) * 1e3
                entry[key] = {"out_to_in_mean": m.a_to_b_mean, "out_to_in_rms": m.a_to_b_rms, "out_to_in_max": m.a_to_b_max,
                              "in_to_out_mean": m.b_to_a_mean, "in_to_out_rms": m.b_to_a_rms, "in_to_out_max": m.b_to_a_max,
                              "symmetric_max": m.symmetric_max, "wall_ms": wall}
            # a second seed: how far the sampled means move with the sample
            m = mc_utils.mesh_distance_device(ov, of, vin, fin, samples=DISTANCE_SAMPLES, seed=1)
            entry["sampled_seed_1"] = {"out_to_in_mean": m.a_to_b_mean, "in_to_out_mean": m.b_to_a_mean,
                                       "out_to_in_rms": m.a_to_b_rms, "in_to_out_rms": m.b_to_a_rms,
                                       "symmetric_max": m.symmetric_max}
            out[name] = entry
        return out
    sv, sf = ref.icosphere(5)
    result["surface_distance"] = {"vx": args.vx, "vx_sphere": args.vx_sphere, "samples": DISTANCE_SAMPLES}
    result["surface_distance"]["sphere"] = compare(torch.from_numpy(sv).cuda(), torch.from_numpy(sf).cuda(), 1.0 / args.vx_sphere)
    save()
    result["surface_distance"]["bench"] = compare(v, f, 1.0 / args.vx)
    print(json.dumps(result["surface_distance"]), flush=True)
    save()


if __name__ == "__main__":
    main()
