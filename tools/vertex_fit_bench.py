"""The surface fit of the vertex table (include/qf_vertex_fit.h) on the bench mesh.

    python tools/vertex_fit_bench.py [--iters 7] [--frames 6] [--skip_lod] [--out profiles/vertex_fit/vertex_fit_bench.json]

On the 983 040-face bench mesh (``bench.build_scene``) with the seeded 6-lobe SG field, ``N = 8 F`` samples, ``C = 46``;
medians of --iters runs after a warm-up, with minimum and maximum:

* ``assemble_ms`` and ``solve_ms`` for K = 0, 1 and 32 steps (``qf_vertex_fit_assemble`` / ``qf_vertex_fit_solve`` under
  HIP events); ``step_ms`` = (K = 32 minus K = 0) / 32: one operator application, two dot products and two vector
  updates (the operator cannot be called on its own through the ABI);
* ``wrapper_wall_ms``: ``baking.fit_vertex_features`` with the sampling, both field evaluations, its allocations and
  its host wait, wall time;
* ``torch_*``: the only baseline, a torch composition on the same GPU in the same run -- the sparse ``[N, V]`` blend
  matrix ``W`` in fp64 CSR and its transpose, ``B = W'(y - W x0)``, the operator ``W'(W p) + lambda d p`` and the same
  Jacobi-preconditioned CG with torch's own reductions -- under HIP events;
* quality: the 800 x 800 bench frames' PSNR against the SG field's own frames for the point bake and for the fit
  (the frames of tools/vertex_baked_bench.py), ``baking.vertex_surface_error`` of both on a fresh seed, and the five
  figures of ``examples/lod_vertex_baked.py --fit_samples_per_face 8``."""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

PER_FACE = 8
LAMBDA = 1.0 / 64
STEPS = 32


def _stat(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def _events(fn, iters):
    out = []
    for _ in range(iters + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return _stat(out[1:]), res


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
    """Both entry points on preallocated buffers."""

    def __init__(self, f, n_v, face, bary, y, x0):
        from quadraturefields_amd import _C
        self.C, self.lib = _C, _C.lib()
        self.f, self.face, self.bary, self.y, self.x0 = f, face, bary, y, x0
        self.n_v, self.n_f, self.n, self.n_c = n_v, f.shape[0], face.shape[0], x0.shape[1]
        self.bytes = int(self.lib.qf_vertex_fit_workspace_bytes(self.n_v, self.n_f, self.n, self.n_c))
        dev = f.device
        self.ws = torch.empty((self.bytes,), dtype=torch.uint8, device=dev)
        self.gram = torch.empty((self.n_f, 9), dtype=torch.float64, device=dev)
        self.mass = torch.empty((self.n_v,), dtype=torch.float64, device=dev)
        self.rhs = torch.empty((self.n_v, self.n_c), dtype=torch.float64, device=dev)
        self.counts = torch.empty((8,), dtype=torch.int64, device=dev)
        self.stats = torch.empty((self.n_c, 2), dtype=torch.float64, device=dev)
        self.out = torch.empty((self.n_v, self.n_c), dtype=torch.float32, device=dev)

    def assemble(self):
        p = self.C.ptr
        self.C.check(self.lib.qf_vertex_fit_assemble(p(self.f), self.n_f, self.n_v, p(self.face), p(self.bary), self.n, p(self.y),
                                                     self.n_c, p(self.x0), self.n_c, self.n_c, LAMBDA, p(self.gram), p(self.mass),
                                                     p(self.rhs), p(self.ws), self.bytes, p(self.counts), self.C.stream()),
                     "assemble")

    def solve(self, steps):
        p = self.C.ptr
        self.C.check(self.lib.qf_vertex_fit_solve(p(self.f), self.n_f, self.n_v, p(self.x0), self.n_c, self.n_c, p(self.gram),
                                                  p(self.mass), p(self.rhs), steps, 1 << (self.n_c - 1), p(self.ws), self.bytes,
                                                  p(self.out), self.n_c, p(self.stats), p(self.counts), self.C.stream()), "solve")


class TorchFit:
    """The baseline: sparse matrices and torch's own reductions."""

    def __init__(self, f, n_v, face, bary, y, x0):
        self.f, self.n_v, self.face, self.bary, self.y, self.x0 = f, n_v, face, bary, y, x0

    def assemble(self):
        n = self.face.shape[0]
        rows = torch.arange(n, device=self.f.device).repeat_interleave(3)
        cols = self.f[self.face].reshape(-1)
        vals = self.bary.reshape(-1)
        self.W = torch.sparse_coo_tensor(torch.stack([rows, cols]), vals, (n, self.n_v)).coalesce().to_sparse_csr()
        self.Wt = torch.sparse_coo_tensor(torch.stack([cols, rows]), vals, (self.n_v, n)).coalesce().to_sparse_csr()
        x0 = self.x0.to(torch.float64)
        self.B = torch.sparse.mm(self.Wt, self.y.to(torch.float64) - torch.sparse.mm(self.W, x0))
        self.d = torch.zeros(self.n_v, dtype=torch.float64, device=self.f.device).index_add_(0, cols, vals)
        diag = torch.zeros(self.n_v, dtype=torch.float64, device=self.f.device).index_add_(0, cols, vals * vals)
        a = diag + LAMBDA * self.d
        self.inv = torch.where(a > 0, 1.0 / a, torch.zeros_like(a))[:, None]
        return self.B

    def apply(self, p):
        return torch.sparse.mm(self.Wt, torch.sparse.mm(self.W, p)) + (LAMBDA * self.d)[:, None] * p

    def solve(self, steps):
        Z, R = torch.zeros_like(self.B), self.B.clone()
        S = self.inv * R
        P, rho = S.clone(), (R * S).sum(0)
        for _ in range(steps):
            q = self.apply(P)
            pi = (P * q).sum(0)
            alpha = torch.where(pi > 0, rho / pi, torch.zeros_like(pi))
            Z += alpha * P
            R -= alpha * q
            S = self.inv * R
            rho_new = (R * S).sum(0)
            beta = torch.where(rho > 0, rho_new / rho, torch.zeros_like(rho))
            P = S + beta * P
            rho = rho_new
        return (self.x0.to(torch.float64) + Z).to(torch.float32), R


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--frames", type=int, default=6, help="orbit frames of the bench scene; 0 skips the frame part")
    ap.add_argument("--skip_lod", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vertex_fit", "vertex_fit_bench.json"))
    args = ap.parse_args()
    import bench
    from quadraturefields_amd import _C, baking, mc_utils, synthetic
    from quadraturefields_amd.mesh_utils import make_camera
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceFieldSGNew
    from quadraturefields_amd.render import FrameRenderer, psnr
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "samples_per_face": PER_FACE,
              "prior_weight": LAMBDA, "steps": STEPS}

    def save():                                                  # after every part, so that a cut-short run leaves what it has
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")

    lobes = 6
    mesh, mi, _ngp = bench.build_scene(dev)
    del _ngp
    sg = NGPRadianceFieldSGNew(aabb=[-1.5] * 3 + [1.5] * 3, use_viewdirs=False, num_g_lobes=lobes, log2_hashmap_size=bench.LOG2_T)
    sg.load_state_dict(synthetic.seeded_ngp_state(bench.LOG2_T, sg.mlp_base.grid.n_rows, sg_lobes=lobes), strict=False)
    sg = sg.to(dev).eval()
    v, f = baking._mesh_tensors(mesh, dev)
    n_v, n_f = v.shape[0], f.shape[0]
    samples = mc_utils.sample_surface_device(v, f, PER_FACE * n_f, 0)
    y = baking._field_features(sg, samples.points.to(torch.float32))
    bake = baking.bake_vertex_features(sg, mi)
    st = Staged(f, n_v, samples.face, samples.bary, y, bake)
    result.update(vertices=n_v, faces=n_f, samples=int(samples.face.shape[0]), columns=int(bake.shape[1]),
                  workspace_bytes=st.bytes)
    result["assemble_ms"] = _events(st.assemble, args.iters)[0]
    for steps in (0, 1, STEPS):
        result[f"solve_{steps}_ms"] = _events(lambda: st.solve(steps), args.iters)[0]
    result["step_ms"] = (result[f"solve_{STEPS}_ms"]["median"] - result["solve_0_ms"]["median"]) / STEPS
    result["counts"] = dict(zip(_C.VERTEX_FIT_COUNTS, st.counts.tolist()))
    norms = st.stats.cpu()
    result["largest_relative_residual"] = float((norms[:, 1] / norms[:, 0].clamp_min(1e-300)).max())
    result["wrapper_wall_ms"], fitted = _wall(lambda: baking.fit_vertex_features(sg, mesh, PER_FACE, device=dev), args.iters)
    result["wrapper_equals_staged_calls"] = bool(torch.equal(fitted.view(torch.int32), st.out.view(torch.int32)))
    print(json.dumps(result), flush=True)
    save()

    try:
        tf = TorchFit(f, n_v, samples.face, samples.bary, y, bake)
        result["torch_assemble_ms"] = _events(tf.assemble, args.iters)[0]
        probe = tf.inv * tf.B
        result["torch_operator_ms"] = _events(lambda: tf.apply(probe), args.iters)[0]
        result["torch_solve_ms"], (table, R) = _events(lambda: tf.solve(STEPS), args.iters)
        result["torch_max_abs_difference_unclamped_columns"] = float((table[:, :-1] - st.out[:, :-1]).abs().max())
        del tf, probe, table, R
    except Exception as exc:                                     # a sparse routine the build lacks: say so, go on
        result["torch_error"] = f"{type(exc).__name__}: {exc}"
    torch.cuda.empty_cache()
    print(json.dumps({k: result[k] for k in result if k.startswith("torch_")}), flush=True)
    save()

    fresh = PER_FACE * n_f
    result["surface_error_fresh_seed"] = {k: {m: e[m] for m in ("mean", "rms", "max")} | {"feature_rms_mean": statistics.mean(e["feature_rms"])}
                                          for k, e in (("point_bake", baking.vertex_surface_error(sg, mesh, bake, fresh, seed=1)),
                                                       ("fit", baking.vertex_surface_error(sg, mesh, fitted, fresh, seed=1)))}
    print(json.dumps(result["surface_error_fresh_seed"]), flush=True)
    save()
    del samples, y, st
    torch.cuda.empty_cache()

    if args.frames:
        cams = synthetic.orbit_cameras(args.frames + 2, seed=42)[2:]   # tools/vertex_baked_bench.py's timed frames
        focal = synthetic.lego_focal(bench.W)
        fr = FrameRenderer(mi, sg, render_step_size=bench.STEP)
        scores = {"point_bake": [], "fit": []}
        for c in cams:
            o, d = synthetic.camera_rays(c, focal, bench.W, bench.H, device=dev)
            cam = make_camera(c, focal, bench.W, bench.H)
            truth = fr.render(o, d, camera=cam)[0].clone()
            for k, table in (("point_bake", bake), ("fit", fitted)):
                scores[k].append(float(psnr(fr.render_vertex_baked(o, d, table, camera=cam)[0], truth)))
        result["bench_frames"] = {"scene": f"{bench.W}x{bench.H}, K={bench.MAX_HITS}, L={lobes}, {args.frames} orbit frames",
                                  **{k: {"psnr_vs_field_db": statistics.mean(s), "psnr_per_frame_db": s} for k, s in scores.items()}}
        print(json.dumps(result["bench_frames"]), flush=True)
        save()
    del mi
    torch.cuda.empty_cache()

    if not args.skip_lod:
        spec = importlib.util.spec_from_file_location("lod_example", os.path.join(ROOT, "examples", "lod_vertex_baked.py"))
        example = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(example)
        with tempfile.TemporaryDirectory() as tmp:
            out = example.main(["--synthetic", "--root", tmp, "--fit_samples_per_face", str(PER_FACE)])
        result["lod_vertex_baked"] = {k: {m: r[m] for m in ("faces", "vertices", "psnr", "ssim")} for k, r in out.items()
                                      if isinstance(r, dict)}
        save()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
