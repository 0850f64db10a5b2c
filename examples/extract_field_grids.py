"""The end of the reference's field training (examples/train_field.py:262-273, 397-410) as a standalone step: from the
stage-1 checkpoint (``{"model", "estimator"}``: the NGP or SG radiance field) and the stage-2 checkpoint
(``{"estimator", "model"}``, ``model`` = the ``Field`` state dict, train_field.py:413-416) to the four files that
``examples/extract_mesh.py`` reads under ROOT:

    python examples/extract_field_grids.py STAGE1_CKPT STAGE2_CKPT ROOT [--num_lobes L] [--log2_hashmap_size T]
                                           [--scale S] [--grid_size N] [--compute_dtype fp32|fp16]
                                           [--log2_T 30] [--grid_resolution 128]

``binaries.npy`` (the estimator's occupancy grid), ``density_grids_valid.npy`` (field_utils.extract_density_grid),
``grids_valid.npy`` and ``grads_valid.npy`` (field_utils.extract_grid).  The models are built as train_field.py:217-252
builds them; ROOT is used as the reference's prefix (``args.root + "results/{scene}/{exp}/"``).  ``--log2_T`` and
``--grid_resolution`` are those of the run that wrote the checkpoints (``examples/train_field_synthetic.py``).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("stage1_ckpt")
    ap.add_argument("stage2_ckpt")
    ap.add_argument("root")
    ap.add_argument("--num_lobes", type=int, default=0)
    ap.add_argument("--num_layers", type=int, default=2)
    ap.add_argument("--log2_hashmap_size", type=int, default=19)
    ap.add_argument("--scale", type=float, default=1.5)
    ap.add_argument("--grid_size", type=int, default=1024)
    ap.add_argument("--compute_dtype", choices=("fp32", "fp16"), default="fp32",
                    help="precision of the Field's fused kernel (fp16 = the reference's tcnn precision)")
    ap.add_argument("--log2_T", type=int, default=30, help="the Field's table (30 = the reference's: every level dense)")
    ap.add_argument("--grid_resolution", type=int, default=128, help="the occupancy grid of the checkpoints")
    args = ap.parse_args(argv)

    from quadraturefields_amd import field_utils
    from quadraturefields_amd.estimators import OccGridEstimator
    from quadraturefields_amd.field import Field
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceField, NGPRadianceFieldSGNew

    device = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    aabb = torch.tensor([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]) * args.scale
    estimator = OccGridEstimator(roi_aabb=aabb, resolution=args.grid_resolution, levels=1).to(device)
    if args.num_lobes > 0:
        radiance_field = NGPRadianceFieldSGNew(aabb=estimator.aabbs[-1], use_viewdirs=False, num_g_lobes=args.num_lobes,
                                               log2_hashmap_size=args.log2_hashmap_size, num_layers=args.num_layers)
    else:
        radiance_field = NGPRadianceField(aabb=estimator.aabbs[-1], num_layers=2,
                                          log2_hashmap_size=args.log2_hashmap_size)
    radiance_field = radiance_field.to(device)
    field_net = Field(scale=0.5, precision=16, log2_T=args.log2_T, L=16, max_res=512, min_res=16, output_dim=1,
                      hidden_size=16, num_features=2, back_prop=False, nl="elu", bias=True, bias_last=True).to(device)
    field_net.compute_dtype = args.compute_dtype

    ckpt = torch.load(args.stage1_ckpt, map_location=device)
    radiance_field.load_state_dict(ckpt["model"])
    estimator.load_state_dict(ckpt["estimator"])
    del ckpt
    ckpt = torch.load(args.stage2_ckpt, map_location=device)
    field_net.load_state_dict(ckpt["model"])
    estimator.load_state_dict(ckpt["estimator"])
    del ckpt

    root = args.root
    os.makedirs(root, exist_ok=True)
    np.save(root + "binaries.npy", estimator.binaries.cpu().numpy())
    field_utils.extract_density_grid(radiance_field, scale=args.scale, prefix=root, grid_size=args.grid_size)
    print("wrote", root + "density_grids_valid.npy")
    field_utils.extract_grid(field_net, root, scale=0.5, grid_size=args.grid_size)
    print("wrote", "{}/grids_valid.npy".format(root), "and", "{}/grads_valid.npy".format(root))


if __name__ == "__main__":
    main()
