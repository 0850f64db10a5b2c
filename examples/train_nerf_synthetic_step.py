"""A few stage-1 training steps (``examples/train_ngp_nerf_sg_occ.py:270-341`` of the reference) on the synthetic scene,
with the regulariser of ``--reg_type`` added to the colour loss:

    python examples/train_nerf_synthetic_step.py [--reg_type distortion] [--steps 40] [--rays 1024] [--size 64] [--views 4]
                                                 [--o_lambda 1e-3] [--c_lambda 1e-4] [--step 1e-2] [--log2_hashmap_size 14]

The targets are views of the seeded NGP field; the field that trains starts from the perturbed hash table (there is no
data set to load).  Every step refreshes the occupancy grid (``update_every_n_steps``), marches a random batch of rays
(``render_image_with_occgrid``, stratified), adds ``losses.regulariser(reg_type, ...)`` to the smooth-L1 colour loss and
takes an Adam step.  Prints the loss, the regulariser and the sample count of every step, then one JSON line with the
first and last losses (means over five steps).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def main(argv=None):
    from quadraturefields_amd import losses
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reg_type", choices=losses.REG_TYPES, default="distortion")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rays", type=int, default=1024)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--o_lambda", type=float, default=1e-3)
    ap.add_argument("--c_lambda", type=float, default=1e-4)
    ap.add_argument("--step", type=float, default=1e-2)
    ap.add_argument("--lr", type=float, default=1e-2)
    ap.add_argument("--log2_hashmap_size", type=int, default=14)
    args = ap.parse_args(argv)

    from quadraturefields_amd import synthetic, utils
    from quadraturefields_amd.datasets.utils import Rays
    from quadraturefields_amd.estimators import OccGridEstimator
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceField

    device = torch.device("cuda:0")
    torch.manual_seed(0)
    size, log2_t = args.size, args.log2_hashmap_size
    aabb = [-1.5] * 3 + [1.5] * 3

    def field_of(perturbed):
        field = NGPRadianceField(aabb=aabb, log2_hashmap_size=log2_t)
        n_rows = field.mlp_base.grid.n_rows
        state = synthetic.seeded_ngp_state(log2_t, n_rows)
        field.load_state_dict(synthetic.perturbed_ngp_state(state, n_rows) if perturbed else state, strict=False)
        return field.to(device)

    truth, field = field_of(False).eval(), field_of(True)
    bkgd = torch.ones(3, device=device)
    focal = synthetic.lego_focal(800) * size / 800.0
    origins, viewdirs, pixels = [], [], []
    with torch.no_grad():
        full = OccGridEstimator(roi_aabb=aabb, resolution=32, levels=1).to(device)
        full.set_occupancy_from_density(lambda p: torch.ones(p.shape[0], device=device), threshold=0.5)
        for c2w in synthetic.orbit_cameras(args.views, seed=2):
            o, d = synthetic.camera_rays(c2w, focal, size, size, device=device)
            origins.append(o)
            viewdirs.append(d)
            pixels.append(utils.render_image_with_occgrid(truth, full, Rays(origins=o, viewdirs=d),
                                                          render_step_size=args.step, render_bkgd=bkgd)[0])
    origins, viewdirs, pixels = torch.cat(origins), torch.cat(viewdirs), torch.cat(pixels)

    estimator = OccGridEstimator(roi_aabb=aabb, resolution=32, levels=1).to(device)
    optimizer = torch.optim.Adam(field.parameters(), lr=args.lr, eps=1e-15)
    field.train()
    estimator.train()
    history = []
    for step in range(args.steps):
        estimator.update_every_n_steps(step=step, occ_eval_fn=lambda x: field.query_density(x) * args.step, occ_thre=1e-2,
                                       n=4)
        pick = torch.randint(0, origins.shape[0], (args.rays,), device=device)
        rays = Rays(origins=origins[pick], viewdirs=viewdirs[pick])
        rgb, acc, _, n_samples, extras = utils.render_image_with_occgrid(field, estimator, rays, render_step_size=args.step,
                                                                         render_bkgd=bkgd)
        if n_samples == 0:
            continue
        rgb_loss = torch.nn.functional.smooth_l1_loss(rgb, pixels[pick])
        loss_reg = losses.regulariser(args.reg_type, acc=acc, extras=extras, rays=rays, o_lambda=args.o_lambda,
                                      c_lambda=args.c_lambda, render_step_size=args.step)
        loss = rgb_loss + loss_reg
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        history.append(float(loss.detach()))
        print(f"step {step:3d}  loss {history[-1]:.6f}  rgb {float(rgb_loss.detach()):.6f}  "
              f"loss_reg[{args.reg_type}] {float(loss_reg.detach()):.3e}  samples {n_samples}")
    k = min(5, len(history))
    first, last = sum(history[:k]) / k, sum(history[-k:]) / k
    print(json.dumps({"reg_type": args.reg_type, "steps": len(history), "loss_first": first, "loss_last": last,
                      "falling": last < first}))
    return 0 if last < first else 1


if __name__ == "__main__":
    sys.exit(main())
