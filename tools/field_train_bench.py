"""One stage-2 training step: ``Field.field_loss`` forward + backward + Adam, timed on device
events, the fused route against the route of the parent commit.

    python tools/field_train_bench.py [--log2_samples 18 20] [--log2_T 30] [--iters 10] [--repeats 5]
                                      [--out profiles/field_train/field_train_bench.json]

The field is the reference's stage-2 ``Field`` (elu, hidden 16, ``log2_T = 30``: 16 dense levels, 317 MB fp32) under
``optim.Adam(lr=2e-2, eps=1e-15)``.  The points are drawn uniformly inside the occupied cells of the synthetic scene's
128^3 occupancy grid (filled from the seeded NGP density) and moved into the field's cube as the training loop does;
directions are random and unnormalised, weights random with 20 % empty samples.  Route ``fused`` is
``fused_backward = True`` (qf_field_quadrature_loss forward and backward, qf_grid_encode_backward_ws); route ``autograd``
is ``fused_backward = False``: the HIP grid encode, three ``F.linear`` + ELU, ``autograd.grad(create_graph=True)`` and
the double backward -- what the parent commit runs for this step.  Same field, same inputs, the two routes alternating
within every repeat; reported per size: the median step time of each route over ``--repeats`` windows of ``--iters``
steps, the spread (max - min), peak allocated memory of a step on each route, and the loss of both routes on the first
step.  No ratio is promised: the file holds what was measured.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch


def occupied_points(n, device, seed):
    """n points uniform inside the occupied cells of the synthetic scene, in the field's [-0.5, 0.5] cube."""
    from quadraturefields_amd import synthetic
    from quadraturefields_amd.estimators import OccGridEstimator
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceField
    aabb = [-1.5] * 3 + [1.5] * 3
    ngp = NGPRadianceField(aabb=aabb, num_layers=2, log2_hashmap_size=14)
    ngp.load_state_dict(synthetic.seeded_ngp_state(14, ngp.mlp_base.grid.n_rows), strict=False)
    ngp = ngp.to(device)
    est = OccGridEstimator(roi_aabb=aabb, resolution=128, levels=1).to(device)
    with torch.no_grad():
        est.set_occupancy_from_density(lambda p: ngp.query_density(p), threshold=5.0)
        cells = torch.nonzero(est.binaries[0])
        g = torch.Generator(device=device).manual_seed(seed)
        pick = cells[torch.randint(0, cells.shape[0], (n,), generator=g, device=device)]
        x = (pick.float() + torch.rand(n, 3, generator=g, device=device)) / 128.0 * 3.0 - 1.5
        _, x01 = ngp.normalize(x)
        dirs = torch.randn(n, 3, generator=g, device=device) * (0.25 + 3.0 * torch.rand(n, 1, generator=g, device=device))
        w = torch.rand(n, generator=g, device=device)
        w_rev = torch.rand(n, generator=g, device=device) * 0.7
        empty = torch.rand(n, generator=g, device=device) < 0.2
        w[empty] = 0.0
        w_rev[empty] = 0.0
    return (x01 - 0.5).contiguous(), dirs, w, w_rev, int(cells.shape[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2_samples", type=int, nargs="+", default=[18, 20])
    ap.add_argument("--log2_T", type=int, default=30)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "field_train", "field_train_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("field_train_bench.py: no HIP device (timings are only taken on the GPU)")
    from quadraturefields_amd.field import Field
    from quadraturefields_amd.optim import Adam
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    field = Field(scale=0.5, precision=16, log2_T=args.log2_T, L=16, max_res=512, min_res=16, output_dim=1, hidden_size=16,
                  num_features=2, back_prop=False, nl="elu", bias=True, bias_last=True).to(dev)
    opt = Adam([{"params": list(field.parameters()), "lr": 2e-2, "weight_decay": 0.0}], lr=2e-3, eps=1e-15)
    result = {"log2_T": args.log2_T, "table_bytes": int(field.xyz_encoder.params.numel()) * 4, "iters": args.iters,
              "repeats": args.repeats, "device": torch.cuda.get_device_name(0), "sizes": {}}

    for log2_n in args.log2_samples:
        n = 1 << log2_n
        pos, dirs, w, w_rev, n_cells = occupied_points(n, dev, seed=log2_n)

        def step(fused):
            field.fused_backward = fused
            opt.zero_grad(set_to_none=True)
            loss = field.field_loss(pos.detach(), w, w_rev, dirs)
            loss.backward()
            opt.step()
            return loss

        def timed(fused):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            for _ in range(args.iters):
                step(fused)
            stop.record()
            torch.cuda.synchronize()
            return start.elapsed_time(stop) * 1e3 / args.iters          # microseconds per step

        def forward_only():
            with torch.no_grad():
                field.fused_backward = True
                return field.field_loss(pos, w, w_rev, dirs)

        first = {}
        state = {k: v.detach().clone() for k, v in field.state_dict().items()}
        for fused in (True, False):                                      # the same first step on both routes
            field.load_state_dict(state)
            first[fused] = float(step(fused).detach())
        peak = {}
        for fused in (True, False):
            for _ in range(3):
                step(fused)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            step(fused)
            torch.cuda.synchronize()
            peak[fused] = int(torch.cuda.max_memory_allocated() - base)
        times = {True: [], False: [], "fwd": []}
        for _ in range(args.repeats):
            times[True].append(timed(True))
            times[False].append(timed(False))
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(args.iters):
                forward_only()
            stop.record()
            torch.cuda.synchronize()
            times["fwd"].append(start.elapsed_time(stop) * 1e3 / args.iters)
        med = {k: statistics.median(v) for k, v in times.items()}
        result["sizes"][str(n)] = {
            "occupied_cells": n_cells,
            "fused_step_us": med[True], "fused_step_us_spread": max(times[True]) - min(times[True]),
            "autograd_step_us": med[False], "autograd_step_us_spread": max(times[False]) - min(times[False]),
            "ratio_autograd_over_fused": med[False] / med[True],
            "fused_loss_forward_only_us": med["fwd"],
            "fused_peak_step_bytes": peak[True], "autograd_peak_step_bytes": peak[False],
            "first_step_loss_fused": first[True], "first_step_loss_autograd": first[False],
        }
        print(json.dumps({str(n): result["sizes"][str(n)]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
