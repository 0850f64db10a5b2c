"""Stage 2 of the pipeline (``examples/train_field.py:217-372, 396-418`` of the reference) on the synthetic scene: fit the
quadrature ``Field`` so that |grad f . d| matches max(w, w_rev) at the samples of a volumetric render of the stage-1
field, and write the stage-2 checkpoint that ``examples/extract_field_grids.py`` reads.

    python examples/train_field_synthetic.py [--steps 400] [--out field.pth] [--log2_T 19] [--log2_hashmap_size 14]
                                             [--grid_resolution 128] [--size 64] [--views 8] [--rays 1024]
                                             [--target_samples 262144] [--step 5e-3] [--weight_decay 0.0]
                                             [--occ_threshold 5.0] [--stage1_out stage1.pth]

The stage-1 field is the seeded NGP field of the synthetic scene (there is no data set to load); its occupancy grid is
filled from its density.  The ``Field`` is built as the reference builds it (elu, hidden 16, 16 levels, ``back_prop``
off; the reference's ``log2_T = 30`` means "every level dense" -- the default here is a table that fits a quick run).
Every step draws a random batch of rays over the views, renders it with ``render_image_field_with_occgrid`` under
``no_grad``, moves the sample positions into the field's [-0.5, 0.5] cube and takes one Adam step on
``Field.field_loss`` (one fused launch forward, one backward).  The ray batch is resized to keep the sample count near
``--target_samples``; a batch without samples is skipped.  ``plot_field``, TensorBoard, LPIPS and the GradScaler of the
reference are out of scope.  Prints the loss of every step, then one JSON line with the first and last losses (means
over five steps) and ``falling``.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--out", default=None, help="stage-2 checkpoint {'estimator', 'model'} (train_field.py:413-418)")
    ap.add_argument("--stage1_out", default=None, help="also write the stage-1 checkpoint {'model', 'estimator'}")
    ap.add_argument("--log2_T", type=int, default=19)
    ap.add_argument("--log2_hashmap_size", type=int, default=14)
    ap.add_argument("--grid_resolution", type=int, default=128)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--rays", type=int, default=1024)
    ap.add_argument("--target_samples", type=int, default=1 << 18)
    ap.add_argument("--step", type=float, default=5e-3)
    ap.add_argument("--weight_decay", type=float, default=0.0)
    ap.add_argument("--occ_threshold", type=float, default=5.0)
    args = ap.parse_args(argv)

    from quadraturefields_amd import synthetic, utils
    from quadraturefields_amd.datasets.utils import Rays
    from quadraturefields_amd.estimators import OccGridEstimator
    from quadraturefields_amd.field import Field
    from quadraturefields_amd.optim import Adam
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceField

    device = torch.device("cuda:0")
    torch.manual_seed(0)
    aabb = [-1.5] * 3 + [1.5] * 3
    radiance_field = NGPRadianceField(aabb=aabb, num_layers=2, log2_hashmap_size=args.log2_hashmap_size)
    radiance_field.load_state_dict(
        synthetic.seeded_ngp_state(args.log2_hashmap_size, radiance_field.mlp_base.grid.n_rows), strict=False)
    radiance_field = radiance_field.to(device)
    estimator = OccGridEstimator(roi_aabb=aabb, resolution=args.grid_resolution, levels=1).to(device)
    with torch.no_grad():
        estimator.set_occupancy_from_density(lambda p: radiance_field.query_density(p), threshold=args.occ_threshold)
    if args.stage1_out:
        torch.save({"model": radiance_field.state_dict(), "estimator": estimator.state_dict()}, args.stage1_out)

    field_net = Field(scale=0.5, precision=16, log2_T=args.log2_T, L=16, max_res=512, min_res=16, output_dim=1,
                      hidden_size=16, num_features=2, back_prop=False, nl="elu", bias=True, bias_last=True).to(device)
    param_groups = [{"params": list(field_net.parameters()), "lr": 2e-2, "weight_decay": args.weight_decay}]
    optimizer = Adam(param_groups, lr=2e-3, eps=1e-15)
    max_steps = args.steps
    scheduler = torch.optim.lr_scheduler.ChainedScheduler([
        torch.optim.lr_scheduler.LinearLR(optimizer, start_factor=0.01, total_iters=100),
        torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=[max_steps // 2, max_steps * 3 // 4, max_steps * 9 // 10],
                                             gamma=0.33)])

    focal = synthetic.lego_focal(800) * args.size / 800.0
    origins, viewdirs = [], []
    for c2w in synthetic.orbit_cameras(args.views, seed=2):
        o, d = synthetic.camera_rays(c2w, focal, args.size, args.size, device=device)
        origins.append(o)
        viewdirs.append(d)
    origins, viewdirs = torch.cat(origins), torch.cat(viewdirs)
    bkgd = torch.ones(3, device=device)

    num_rays = args.rays
    history = []
    radiance_field.train()            # one chunk per batch, stratified marching (train_field.py:298)
    for step in range(max_steps):
        pick = torch.randint(0, origins.shape[0], (num_rays,), device=device)
        rays = Rays(origins=origins[pick], viewdirs=viewdirs[pick])
        with torch.no_grad():
            _, _, _, n_samples, weights, weights_rev, positions, dirs = utils.render_image_field_with_occgrid(
                radiance_field, estimator, rays, render_step_size=args.step, render_bkgd=bkgd)
            _, positions = radiance_field.normalize(positions)
        if n_samples == 0:
            continue
        positions = positions - 0.5
        with torch.enable_grad():
            loss = field_net.field_loss(positions, weights, weights_rev, dirs)
            optimizer.zero_grad()
            loss.backward()
        optimizer.step()
        scheduler.step()
        if args.target_samples > 0:   # keep the sample batch near the target (train_field.py:354-360)
            num_rays = max(1, int(num_rays * (args.target_samples / float(n_samples))))
        history.append(float(loss.detach()))
        print(f"step {step:4d}  field_loss {history[-1]:.6f}  samples {n_samples}  rays {pick.shape[0]}")

    if args.out:
        torch.save({"estimator": estimator.state_dict(), "model": field_net.state_dict()}, args.out)
        print("Saved checkpoints at", args.out)
    k = min(5, len(history))
    first, last = (sum(history[:k]) / k, sum(history[-k:]) / k) if k else (float("nan"), float("nan"))
    result = {"steps": len(history), "loss_first": first, "loss_last": last, "falling": bool(last < first)}
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    sys.exit(0 if main()["falling"] else 1)
