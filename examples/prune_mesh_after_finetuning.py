"""Stage 6a of the baking pipeline, with the command line ``script/run_nerfsynthetic_baking.sh`` passes it:

    python examples/prune_mesh_after_finetuning.py --scene lego --data_root DATA --ckpt_path CKPT --mesh_path DIR/mesh.ply
                                                   --max_hits 25 --up_sample 2 --log2_hashmap_size 19 [--num_lobes N]
                                                   [--num_layers L] [--scale 1.5] [--compact] [--min_component_faces N]

Every view of the train split is rendered at ``up_sample`` through the finetuned field (``ckpt["radiance_field"]``) and
folded into each triangle's maximum compositing weight (``pruning.MeshPruner.add_view``: one bound call per view, no host
wait); the faces whose maximum is not above 1e-3 are dropped.  Next to the mesh it writes ``triangle_weights.npy``,
``mesh_updated.ply`` -- what ``examples/generate_uv_atlas.py ROOT mesh_updated.ply ...`` reads --, ``num_samples.npy`` and
``num_valid_samples.npy``.  The script's other flags are accepted and unused.  ``--compact`` also removes the vertices no
kept face uses (and, with ``--min_component_faces N``, the vertex-connected islands of fewer than N faces) on the device
(``mc_utils.compact_mesh``): ``mesh_updated.ply`` is then the cleaned mesh, ``face_map.npy`` and
``vertex_map.npy`` name the source face / vertex of its rows, and V, F, the clean-up counts and the bytes of a per-vertex
table (64-byte records) are printed before and after.

    python examples/prune_mesh_after_finetuning.py --synthetic OUT [--size 400] [--views 16] [--shells 6] [--subdivisions 4]

runs the stage end to end without a data set: the nested-shell mesh (written to ``OUT/mesh.ply``), a seeded field and
orbit cameras; the four files land in ``OUT``.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def parse(argv):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", type=str, default="lego")
    ap.add_argument("--data_root", type=str, default="data/nerf_synthetic")
    ap.add_argument("--ckpt_path", "--ckpt", dest="ckpt_path", type=str, default="")
    ap.add_argument("--mesh_path", type=str, default="")
    ap.add_argument("--max_hits", type=int, default=10)
    ap.add_argument("--bvh_builder", choices=("host", "device"), default="host",
                    help="where the ray-mesh BVH is built: host (binned SAH) or device (linear BVH on the GPU: faster build, slower traversal)")
    ap.add_argument("--up_sample", type=float, default=1.0)
    ap.add_argument("--log2_hashmap_size", type=int, default=19)
    ap.add_argument("--scale", type=float, default=1.5)
    ap.add_argument("--num_lobes", type=int, default=0)
    ap.add_argument("--num_layers", type=int, default=1)
    ap.add_argument("--compact", action="store_true", help="remove the unreferenced vertices too; writes face_map.npy and vertex_map.npy")
    ap.add_argument("--min_component_faces", type=int, default=0,
                    help="with --compact: drop vertex-connected components of fewer faces (0 or 1: none)")
    ap.add_argument("--synthetic", metavar="OUT", type=str, default=None, help="run on the synthetic scene, write into OUT")
    ap.add_argument("--size", type=int, default=400, help="--synthetic: image width and height before up_sample")
    ap.add_argument("--views", type=int, default=16, help="--synthetic: orbit cameras")
    ap.add_argument("--shells", type=int, default=6)
    ap.add_argument("--subdivisions", type=int, default=4)
    args, _unused = ap.parse_known_args(argv)          # --root, --exp_name, --scaling, --optix, --voxel_size, ...
    return args


def synthetic_views(args, device):
    """(mesh path, field, iterator of (origins, viewdirs, camera)) of the synthetic scene."""
    from quadraturefields_amd import synthetic
    from quadraturefields_amd.mesh_utils import make_camera
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceField
    os.makedirs(args.synthetic, exist_ok=True)
    mesh_path = os.path.join(args.synthetic, "mesh.ply")
    synthetic.shell_mesh(n_shells=args.shells, subdivisions=args.subdivisions).export(mesh_path)
    field = NGPRadianceField(aabb=[-1.5] * 3 + [1.5] * 3, log2_hashmap_size=args.log2_hashmap_size)
    field.load_state_dict(synthetic.seeded_ngp_state(args.log2_hashmap_size, field.mlp_base.grid.n_rows), strict=False)
    up = max(int(args.up_sample), 1)
    size = args.size * up
    focal = synthetic.lego_focal(size)

    def views():
        for c2w in synthetic.orbit_cameras(args.views):
            o, d = synthetic.camera_rays(c2w, focal, size, size, device=device)
            yield o, d, make_camera(c2w, focal, size, size)

    return mesh_path, field, views()


def dataset_views(args, device):
    from quadraturefields_amd.datasets.nerf_synthetic import SubjectLoader
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceField, NGPRadianceFieldSGNew
    scale = 2.0 if args.scene in ("horse", "woolly") else args.scale
    aabb = [-scale] * 3 + [scale] * 3
    if args.num_lobes > 0:
        field = NGPRadianceFieldSGNew(aabb=aabb, use_viewdirs=False, num_g_lobes=args.num_lobes, num_layers=args.num_layers,
                                      log2_hashmap_size=args.log2_hashmap_size)
    else:
        field = NGPRadianceField(aabb=aabb, num_layers=2, hidden_size=64, log2_hashmap_size=args.log2_hashmap_size)
    field.load_state_dict(torch.load(args.ckpt_path, map_location="cpu")["radiance_field"])
    dataset = SubjectLoader(subject_id=args.scene, root_fp=args.data_root, split="train", num_rays=None, device=device,
                            upsample=args.up_sample)

    def views():
        for i in range(len(dataset.images)):
            item = dataset.fetch_data(i)
            yield item["rays"].origins, item["rays"].viewdirs, item["camera"]

    return args.mesh_path, field, views()


def main(argv=None):
    args = parse(argv)
    from quadraturefields_amd.mesh_utils import MeshIntersection
    from quadraturefields_amd.pruning import MeshPruner
    device = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    if args.synthetic is not None:
        mesh_path, field, views = synthetic_views(args, device)
    else:
        if not args.mesh_path or not args.ckpt_path:
            sys.exit("prune_mesh_after_finetuning.py: --mesh_path and --ckpt_path are required (or --synthetic OUT)")
        mesh_path, field, views = dataset_views(args, device)
    mi = MeshIntersection(mesh_path, simplify_mesh=False, scale=1.0, num_intersections=args.max_hits,
                          render_step_size=5e-3, device=device, bvh_builder=args.bvh_builder)
    pruner = MeshPruner(mi, field.to(device).eval())
    for origins, viewdirs, camera in views:
        pruner.add_view(origins, viewdirs, camera)
    print("Number of faces before pruning: ", mi.mesh.faces.shape[0])
    if args.min_component_faces and not args.compact:
        sys.exit("prune_mesh_after_finetuning.py: --min_component_faces needs --compact")
    pruned = pruner.save(os.path.dirname(os.path.abspath(mesh_path)), compact=args.compact,
                         min_component_faces=args.min_component_faces)
    print("Number of faces after pruning: ", pruned.faces.shape[0])
    if args.compact:
        from quadraturefields_amd import mc_utils
        stats = mc_utils.compact_mesh(mi.mesh, pruner.keep_mask(), min_component_faces=args.min_component_faces,
                                      return_stats=True)[3]
        v0, f0, v1, f1 = mi.mesh.vertices.shape[0], mi.mesh.faces.shape[0], pruned.vertices.shape[0], pruned.faces.shape[0]
        print(f"before: V = {v0}, F = {f0}, vertex table {64 * v0} bytes")
        print(f"after:  V = {v1}, F = {f1}, vertex table {64 * v1} bytes")
        print("counts:", ", ".join(f"{k} = {v}" for k, v in stats.items()))


if __name__ == "__main__":
    main()
