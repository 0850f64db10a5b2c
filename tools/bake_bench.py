"""Stage 6c: time of ``baking.bake_texture_set`` against ``baking.bake_texture_images`` on the same
device texel-position map.

    python tools/bake_bench.py [--cases 4096:6,8192:3] [--repeats 5] [--shells 12] [--subdivisions 6]
                               [--log2_hashmap_size 19] [--untouched last_face] [--out profiles/bake/bake_bench.json]

``V`` is ``baking.texel_positions`` of ``uv_atlas.per_triangle_atlas`` of ``synthetic.shell_mesh`` at each texture size
(``--untouched last_face`` is what ``examples/generate_uv_atlas.py`` writes: every texel no face covers stands for the
last face's centroid and is baked too; ``zero`` leaves those texels empty); the valid share is recorded.  Seeded SG and
NGP fields.  ``bake_texture_images`` runs at its default batch of 100 000 texels and is the code of the parent commit.
After one warm-up of each, the two routes alternate ``--repeats`` times; a run is timed with a host clock around a device
synchronise.  Medians, spreads (max - min) and the differing share per plane of the two texture sets are written.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=str, default="4096:6,8192:3", help="texture_size:lobes, comma separated")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shells", type=int, default=12)
    ap.add_argument("--subdivisions", type=int, default=6)
    ap.add_argument("--log2_hashmap_size", type=int, default=19)
    ap.add_argument("--untouched", type=str, default="last_face")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bake_bench.py: no HIP device (timings are only taken on the GPU)")
    torch.set_grad_enabled(False)
    from quadraturefields_amd import baking, synthetic, uv_atlas
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceField, NGPRadianceFieldSGNew
    from quadraturefields_amd.texture_utils import FeatureCompression

    dev = torch.device("cuda:0")
    log2_t = args.log2_hashmap_size
    aabb = [-1.5] * 3 + [1.5] * 3
    mesh = synthetic.shell_mesh(n_shells=args.shells, subdivisions=args.subdivisions)
    nf = NGPRadianceField(aabb=aabb, log2_hashmap_size=log2_t)
    nf.load_state_dict(synthetic.seeded_ngp_state(log2_t, nf.mlp_base.grid.n_rows, seed=7), strict=False)
    nf = nf.to(dev).eval()
    out = {"device": torch.cuda.get_device_name(0), "triangles": int(mesh.faces.shape[0]), "log2_hashmap_size": log2_t,
           "untouched": args.untouched, "repeats": args.repeats, "old_batch_size": 100000, "cases": []}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for case in args.cases.split(","):
        size, lobes = (int(x) for x in case.split(":"))
        sg = NGPRadianceFieldSGNew(aabb=aabb, use_viewdirs=False, num_g_lobes=lobes, log2_hashmap_size=log2_t)
        sg.load_state_dict(synthetic.seeded_ngp_state(log2_t, sg.mlp_base.grid.n_rows, sg_lobes=lobes), strict=False)
        sg = sg.to(dev).eval()
        mesh_uv, _ = uv_atlas.per_triangle_atlas(mesh, size)
        V, _ = baking.texel_positions(mesh_uv, size, untouched=args.untouched)
        new_set = FeatureCompression(lobes, initialize=True, texture_size=size, compression_type="linear", device=dev)
        old_set = FeatureCompression(lobes, initialize=True, texture_size=size, compression_type="linear", device=dev)
        rows = baking.bake_chunk_rows(size, lobes)
        state = {}

        def run_new():
            state["mask"], state["count"] = baking.bake_texture_set(sg, nf, V, new_set)

        def run_old():
            baking.bake_texture_images(sg, nf, V, old_set)

        timed(run_new)
        timed(run_old)
        new_ms, old_ms = [], []
        for _ in range(args.repeats):
            new_ms.append(timed(run_new))
            old_ms.append(timed(run_old))
        valid = int(state["count"])
        planes = [("alpha", new_set.alpha, old_set.alpha), ("diffuse", new_set.diffuse, old_set.diffuse)]
        for i in range(lobes):
            planes += [(f"color_{i}", new_set.sg_colors[i], old_set.sg_colors[i]),
                       (f"lambda_axis_{i}", new_set.lambdas[i], old_set.lambdas[i])]
        differing, max_step = {}, 0
        for name, a, b in planes:
            d = (a.to(torch.int16) - b.to(torch.int16)).abs()
            d = torch.minimum(d, 256 - d)                  # the azimuth wraps; no other code differs by more than 128
            max_step = max(max_step, int(d.max()))
            differing[name] = float((d.reshape(size * size, -1).amax(dim=-1) > 0).sum()) / max(valid, 1)
        spread = max(max(new_ms) - min(new_ms), max(old_ms) - min(old_ms))
        med_new, med_old = statistics.median(new_ms), statistics.median(old_ms)
        out["cases"].append({
            "texture_size": size, "lobes": lobes, "valid_texels": valid, "valid_share": valid / float(size * size),
            "rows_per_chunk": rows, "bands": -(-size // rows), "old_batches": -(-valid // 100000),
            "bake_texture_set_ms": new_ms, "bake_texture_images_ms": old_ms,
            "bake_texture_set_ms_median": med_new, "bake_texture_images_ms_median": med_old,
            "bake_texture_set_ms_spread": max(new_ms) - min(new_ms),
            "bake_texture_images_ms_spread": max(old_ms) - min(old_ms),
            "speedup": med_old / med_new, "not_slower_within_spread": bool(med_new - med_old <= spread),
            "max_code_step_between_routes": max_step, "differing_texel_share_per_plane": differing})
        print(json.dumps(out["cases"][-1]), flush=True)
        del V, new_set, old_set, sg, state
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
