"""Distortion loss: forward + gradient time of ``qf_distortion_loss`` at 2^20 packed samples
against a torch-op composition of the same formula.

    python tools/distloss_bench.py [--log2_samples 20] [--iters 50] [--repeats 5] [--out profiles/distloss/distloss_bench.json]

Two shapes: ``stage1`` -- ray lengths exponential with mean 64, clipped to 700 (an occupancy-grid training batch) -- and
``finetune`` -- 1..25 quadrature points per ray.  Weights come from random densities through exp, m from jittered steps of
5e-3 starting in [2, 6].  The kernel side is what ``losses.flatten_eff_distloss`` launches when autograd records: one
launch that writes the loss and dloss/dw.  The comparison partner (``composition`` below; the parent commit has nothing to
compare with) computes the same two outputs in fp32 from global ``cumsum``s minus per-ray bases; the index of every
sample's first and last ray sample is precomputed outside the timed region, in its favour.  Each side is timed by device
events around ``--iters`` back-to-back calls, after a warm-up; reported: the median over ``--repeats`` of the per-call
time, the spread, the ratio, and how far the fp32 composition's gradient is from the kernel's.  No ratio is promised: the
file holds what was measured.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch


def make_batch(kind, n, seed, dev):
    rng = np.random.default_rng(seed)
    lengths, total = [], 0
    while total < n:
        c = int(min(700, rng.exponential(64.0))) if kind == "stage1" else int(rng.integers(1, 26))
        c = min(c, n - total)
        lengths.append(c)
        total += c
    lengths = np.asarray(lengths, dtype=np.int64)
    ray_id = np.repeat(np.arange(len(lengths)), lengths)
    first = np.repeat(np.cumsum(lengths) - lengths, lengths)
    last = np.repeat(np.cumsum(lengths) - 1, lengths)
    step = 5e-3 * rng.uniform(0.5, 1.5, size=n)
    cs = np.cumsum(step)
    t = np.repeat(rng.uniform(2.0, 6.0, size=len(lengths)), lengths) + cs - (cs - step)[first]
    tau = rng.exponential(1.0, size=n) * step * 20.0
    ct = np.cumsum(tau) - tau
    w = np.exp(-(ct - ct[first])) * (1.0 - np.exp(-tau))
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    i = lambda a: torch.from_numpy(a).to(dev)
    return {"w": f(w), "m": f(t - 0.5 * step), "d": f(step), "ray_id": i(ray_id), "first": i(first), "last": i(last),
            "n_rays": len(lengths), "mean_length": float(lengths.mean()), "max_length": int(lengths.max())}


def composition(w, m, d, first, last, n_rays):
    """The same loss and gradient from torch ops, fp32: exclusive prefix sums as a global cumsum minus its value at the
    ray's first sample, suffix sums as ray total minus prefix."""
    wm = w * m
    pw, pwm = torch.cumsum(w, 0) - w, torch.cumsum(wm, 0) - wm        # global exclusive prefixes
    bw, bwm = pw[first], pwm[first]
    p, pm = pw - bw, pwm - bwm
    tw, twm = pw[last] + w[last] - bw, pwm[last] + wm[last] - bwm     # ray totals
    s, sm = tw - p - w, twm - pm - wm
    loss = ((2.0 * w * (m * p - pm)).sum() + (w * w * d).sum() / 3.0) / n_rays
    grad = (2.0 * (m * (p - s) + (sm - pm)) + (2.0 / 3.0) * w * d) / n_rays
    return loss, grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2_samples", type=int, default=20)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "distloss", "distloss_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("distloss_bench.py: no HIP device (timings are only taken on the GPU)")
    torch.set_grad_enabled(False)
    from quadraturefields_amd import losses
    dev = torch.device("cuda:0")
    n = 1 << args.log2_samples

    def timed(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(args.iters):
            fn()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) * 1e3 / args.iters             # microseconds per call

    result = {"samples": n, "iters": args.iters, "repeats": args.repeats, "device": torch.cuda.get_device_name(0)}
    for kind in ("stage1", "finetune"):
        b = make_batch(kind, n, 21, dev)
        kernel = lambda: losses._launch(b["w"], b["m"], b["d"], 0.0, b["ray_id"], 0, 0, True)
        torch_ops = lambda: composition(b["w"], b["m"], b["d"], b["first"], b["last"], b["n_rays"])
        (lk, gk), (lt, gt) = kernel(), torch_ops()
        for _ in range(3):
            kernel(), torch_ops()
        tk, tt = [], []
        for _ in range(args.repeats):
            tk.append(timed(kernel))
            tt.append(timed(torch_ops))
        result[kind] = {
            "n_rays": b["n_rays"], "mean_length": b["mean_length"], "max_length": b["max_length"],
            "kernel_us": statistics.median(tk), "kernel_us_spread": max(tk) - min(tk),
            "torch_composition_us": statistics.median(tt), "torch_composition_us_spread": max(tt) - min(tt),
            "ratio_torch_over_kernel": statistics.median(tt) / statistics.median(tk),
            "loss_kernel": float(lk), "loss_torch_composition": float(lt),
            "composition_grad_max_abs_diff_over_max_grad": float((gt - gk).abs().max() / gk.abs().max()),
        }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
