"""Timing of stage 2's grid extraction at the reference's size, alone on the GPU:

    python tools/grid_extract_bench.py [--grid_size 1024] [--repeat 3] [--autograd_rows 2]

  * fused:     field_utils.field_grids on the stage-2 Field (elu, hidden 16, log2_T = 30), fp32 and fp16 tables;
  * density:   field_utils.density_grid on an NGP radiance field (log2_T = 19) through its fused query_density;
  * autograd:  the reference-shaped route (Field.forward with return_grad=True through autograd, 1 M-point batches) on
               a few x-rows, EXTRAPOLATED linearly to the full grid and labelled so.
Times are device events after one warm-up; points/s counts the (2N)^3 lattice points.  One JSON line per measurement.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def _time(fn, repeat):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / 1e3)
    return min(ts), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid_size", type=int, default=1024)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--autograd_rows", type=int, default=2)
    ap.add_argument("--skip", default="", help="comma list of fused,fp16,density,autograd to skip")
    args = ap.parse_args()
    from quadraturefields_amd import field_utils, synthetic
    from quadraturefields_amd.field import Field
    from quadraturefields_amd.radiance_fields.ngp import NGPRadianceField
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    n = args.grid_size
    pts = (2 * n) ** 3
    skip = set(args.skip.split(","))

    f = Field(scale=0.5, precision=16, log2_T=30, L=16, max_res=512, min_res=16, output_dim=1, hidden_size=16,
              num_features=2, back_prop=False, nl="elu")
    st = synthetic.seeded_deform_state(f.xyz_encoder.grid.n_params)
    st = {k: (v[:16, :35] if k == "decoder_field.layers.0.weight" else v[:16, :16] if k == "decoder_field.layers.1.weight"
              else v[:16] if k in ("decoder_field.layers.0.bias", "decoder_field.layers.1.bias")
              else v[:, :16] if k == "decoder_field.lout.weight" else v) for k, v in st.items()}
    f.load_state_dict(st, strict=False)
    f = f.to(dev)
    out = {}
    for mode in ("fp32", "fp16"):
        if (mode == "fp32" and "fused" in skip) or (mode == "fp16" and "fp16" in skip):
            continue
        f.compute_dtype = mode
        res = {}

        def run():
            res["vg"] = field_utils.field_grids(f, n)
        t, ts = _time(run, args.repeat)
        del res["vg"]
        out[f"fused_{mode}"] = dict(seconds=t, all=ts, points_per_s=pts / t)
        print(json.dumps({"what": f"field_grids {mode}", "grid_size": n, "seconds": t, "points_per_s": pts / t}),
              flush=True)
    f.compute_dtype = "fp32"
    if "autograd" not in skip:
        axis = field_utils.lattice_axis(n, 0.5, dev)
        rows = args.autograd_rows
        v = torch.empty((rows, n, n), dtype=torch.float32, device=dev)
        g = torch.empty((rows, n, n), dtype=torch.float16, device=dev)
        t, ts = _time(lambda: field_utils._autograd_slab(lambda x: f(x), axis, n, 0, rows, v, g), 1)
        full = t * n / rows
        print(json.dumps({"what": "autograd route", "grid_size": n, "rows_timed": rows, "seconds_rows": t,
                          "EXTRAPOLATED_seconds_full_grid": full, "points_per_s": 8 * rows * n * n / t}), flush=True)
        del v, g
    del f
    torch.cuda.empty_cache()
    if "density" not in skip:
        m = NGPRadianceField(aabb=[-1.5] * 3 + [1.5] * 3, log2_hashmap_size=19)
        m.load_state_dict(synthetic.seeded_ngp_state(19, m.mlp_base.grid.n_rows), strict=False)
        m = m.to(dev)
        res = {}

        def run_d():
            res["d"] = field_utils.density_grid(m, 1.5, n)
        t, ts = _time(run_d, args.repeat)
        print(json.dumps({"what": "density_grid", "grid_size": n, "seconds": t, "points_per_s": pts / t}), flush=True)


if __name__ == "__main__":
    main()
