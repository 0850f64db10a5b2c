"""Stage 6c of the baking pipeline (examples/bake_texture_images_shelly.py of the reference), with the command line
``script/run_nerfsynthetic_baking.sh`` passes it:

    python examples/bake_texture_images.py --mesh_path DIR/mesh_segmentation_4096.obj --texture_size 4096 --num_lobes 6
                                           --num_layers 2 --log2_hashmap_size 19 --scale 1.5 --compression_type linear
                                           --lambda_thres 7.5 --ckpt_path FINETUNE.pth --ckpt_path_sg FIT_SG.pth

Both checkpoints are read under the key ``radiance_field``: the finetuned field gives the density, the spherical-Gaussian
field the features.  ``V_{texture_size}.npy`` (what ``examples/generate_uv_atlas.py`` wrote next to the mesh; float16
above 8192, converted as the reference's ``.astype(np.float32)``) goes to the device once and
``baking.bake_texture_set`` fills the texture set band by band without a host wait.  Next to the mesh it writes
``texture_{texture_size}/`` (``alpha.png``, ``diffuse.png``, ``color_{i}.png``, ``lambda_axis_{i}.png``) -- what
``examples/evaluate_baked_textures.py`` reads -- and ``mask_V_{texture_size}.png`` (the valid texels, white), and prints the
valid share.  The script's other flags are accepted and unused.

    python examples/bake_texture_images.py --mesh_path DIR/mesh_segmentation_256.obj --texture_size 256 --num_lobes 3
                                           --log2_hashmap_size 12 --synthetic

needs no checkpoint: a checkpoint that is not given is replaced by the seeded state of ``synthetic.seeded_ngp_state``
(seed 42 for both fields, so that the two share their density network and the SG field rendered on the mesh is what the
baked textures approximate).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch


def parse(argv):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mesh_path", type=str, default="")
    ap.add_argument("--scene", type=str, default="lego")
    ap.add_argument("--texture_size", type=int, default=4096)
    ap.add_argument("--num_lobes", type=int, default=0)
    ap.add_argument("--num_layers", type=int, default=1)
    ap.add_argument("--log2_hashmap_size", type=int, default=19)
    ap.add_argument("--scale", type=float, default=1.5)
    ap.add_argument("--compression_type", type=str, default="linear")
    ap.add_argument("--lambda_thres", type=float, default=7.5)
    ap.add_argument("--ckpt_path", type=str, default="")
    ap.add_argument("--ckpt_path_sg", type=str, default="")
    ap.add_argument("--synthetic", action="store_true", help="seeded weights for every checkpoint that is not given")
    args, _unused = ap.parse_known_args(argv)          # --root, --data_root, --exp_name, --scaling, --max_hits, ...
    return args


def load_fields(args, device):
    """(SG field, density field) of the command line, on the device, in eval mode."""
    from quadraturefields_amd import synthetic
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceField, NGPRadianceFieldSGNew
    scale = 2.0 if args.scene in ("horse", "woolly") else args.scale
    aabb = [-scale] * 3 + [scale] * 3
    log2_t = args.log2_hashmap_size
    sg = NGPRadianceFieldSGNew(aabb=aabb, use_viewdirs=False, num_g_lobes=args.num_lobes, num_layers=args.num_layers,
                               log2_hashmap_size=log2_t)
    field = NGPRadianceField(aabb=aabb, num_layers=2, hidden_size=64, log2_hashmap_size=log2_t)
    if args.ckpt_path:
        field.load_state_dict(torch.load(args.ckpt_path, map_location="cpu")["radiance_field"])
    else:
        field.load_state_dict(synthetic.seeded_ngp_state(log2_t, field.mlp_base.grid.n_rows), strict=False)
    if args.ckpt_path_sg:
        sg.load_state_dict(torch.load(args.ckpt_path_sg, map_location="cpu")["radiance_field"])
    else:
        sg.load_state_dict(synthetic.seeded_ngp_state(log2_t, sg.mlp_base.grid.n_rows, sg_lobes=args.num_lobes), strict=False)
    return sg.to(device).eval(), field.to(device).eval()


def main(argv=None):
    args = parse(argv)
    if not args.mesh_path:
        sys.exit("bake_texture_images.py: --mesh_path is required")
    if not args.synthetic and not (args.ckpt_path and args.ckpt_path_sg):
        sys.exit("bake_texture_images.py: --ckpt_path and --ckpt_path_sg are required (or --synthetic)")
    if args.synthetic and args.num_layers == 1:
        args.num_layers = 2                                # the seeded head has the two layers of the scripts' SG field
    from quadraturefields_amd import baking
    from quadraturefields_amd.texture_utils import FeatureCompression, _write_png

    device = torch.device("cuda:0")
    size = args.texture_size
    root_path = os.path.dirname(os.path.abspath(args.mesh_path))
    sg, field = load_fields(args, device)
    V = np.load(os.path.join(root_path, f"V_{size}.npy")).astype(np.float32)
    compressor = FeatureCompression(args.num_lobes, initialize=True, texture_size=size, path=None,
                                    compression_type=args.compression_type, lambda_thres=args.lambda_thres, device=device)
    with torch.no_grad():
        mask, count = baking.bake_texture_set(sg, field, torch.from_numpy(V).to(device), compressor)
    texture_dir = os.path.join(root_path, f"texture_{size}")
    os.makedirs(texture_dir, exist_ok=True)
    compressor.save_to_file(texture_dir + os.sep)
    _write_png(os.path.join(root_path, f"mask_V_{size}.png"), mask.cpu().numpy().astype(np.uint8) * 255)
    count = int(count)
    print(f"Baked {count} of {size * size} texels ({count / (size * size):.1%} valid) into {texture_dir}")
    return compressor, mask


if __name__ == "__main__":
    main()
