"""Texel-position map (qf_texel_positions) per pass: time, bytes, atomics, and their fraction of the roofline.

    python tools/texel_fill_bench.py [--sizes 4096 8192] [--iters 5] [--atomic-rate 1.0e10]

Meshes: the bench mesh (``synthetic.shell_mesh()``, 983 040 faces, per-shell (azimuth, elevation) cells) and the same
triangles on ``per_triangle_charts`` (a 4-texel chart per face at a random place).  The whole call is timed with HIP
events (median of --iters); each pass's kernel time comes from the profiler's device timestamps of one further call.
Rooflines: HBM at the nominal 8 TB/s for the byte-moving passes; for the atomic passes the calibrated rate of returning
device-scope integer atomics (tools/calib_atomic.hip, compiled and run here unless --atomic-rate is given).
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

HBM_BYTES_PER_S = 8.0e12
PASSES = {"face_setup_kernel": "setup", "scan_tiles_kernel": "scan", "scan_block_sums_kernel": "scan",
          "scan_add_kernel": "scan", "cover_kernel": "cover", "edges_kernel": "edges", "resolve_kernel": "resolve"}


def calibrated_atomic_rate():
    src = os.path.join(ROOT, "tools", "calib_atomic.hip")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "calib_atomic")
        subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", src, "-o", exe], check=True, capture_output=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120).stdout
    m = re.search(r"agent scope: .*= ([0-9.e+]+) /s", out)
    return float(m.group(1))


def edge_transitions(faces, uv, H, W, dev, chunk=1 << 16):
    """Texel changes along the 100 edge samples of every (face, edge): the texels the edge pass looks at."""
    w = torch.linspace(0, 1, 100, dtype=torch.float64, device=dev)
    w[-1] = 1.0
    s = torch.from_numpy(uv).to(dev) * torch.tensor([H, W], dtype=torch.float64, device=dev)
    s[:, 0].clamp_(0, H - 1)
    s[:, 1].clamp_(0, W - 1)
    f = torch.from_numpy(faces).to(dev)
    total = 0
    for b in range(0, f.shape[0], chunk):
        fc = f[b:b + chunk]
        for a, c in ((0, 1), (1, 2), (2, 0)):
            p = (s[fc[:, c]][:, None, :] * w[None, :, None] + s[fc[:, a]][:, None, :] * (1 - w[None, :, None])).long()
            lin = p[..., 0] * W + p[..., 1]
            total += int(lin.shape[0] + (lin[:, 1:] != lin[:, :-1]).sum())
    return total


def run(name, mesh, H, W, iters, atomic_rate, dev):
    from quadraturefields_amd import baking
    F = len(mesh.faces)
    V, ts = baking.texel_positions(mesh, H, W)                           # warm-up (and the lazy library load)
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        baking.texel_positions(mesh, H, W)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    per_pass = {}
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        baking.texel_positions(mesh, H, W)
        torch.cuda.synchronize()
    for ev in prof.events():
        for kname, pname in PASSES.items():
            if kname in ev.name and ev.device_type.name in ("CUDA", "HIP"):
                per_pass[pname] = per_pass.get(pname, 0.0) + ev.device_time_total / 1e3      # us -> ms
    uv = np.asarray(mesh.visual.uv, dtype=np.float64)
    qs = np.clip(uv * np.array([H, W]), 0, np.array([H - 1, W - 1])).astype(np.int64)[mesh.faces]
    area = (np.ptp(qs[:, :, 0], 1) + 1) * (np.ptp(qs[:, :, 1], 1) + 1)
    candidates = int(area.sum())
    covered = int(ts.sum())
    transitions = edge_transitions(np.asarray(mesh.faces), uv, H, W, dev)
    hw = H * W
    # bytes that must cross HBM (first touch), per pass
    bytes_ = {"setup": F * (24 + 3 * 16 + 3 * 24 + 64), "scan": 3 * 8 * F,
              "cover": candidates // 64 * 32 + 4 * covered, "edges": F * (24 + 3 * 16) + 4 * transitions,
              "resolve": 4 * hw + 4 * hw + 12 * hw}
    atomics = {"cover": covered + F, "edges": transitions}
    rows = {}
    for p in ("setup", "scan", "cover", "edges", "resolve"):
        ms = per_pass.get(p)
        row = {"ms": ms, "bytes": bytes_[p]}
        if ms:
            row["hbm_fraction"] = bytes_[p] / (ms * 1e-3) / HBM_BYTES_PER_S
            if p in atomics:
                row["atomics"] = atomics[p]
                if atomic_rate:
                    row["atomic_fraction"] = atomics[p] / (ms * 1e-3) / atomic_rate
        rows[p] = row
    return {"mesh": name, "H": H, "W": W, "faces": F, "candidates": candidates, "covered": covered,
            "texels": hw, "edge_transitions": transitions,
            "call_ms_median": statistics.median(times), "call_ms_min": min(times), "passes": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 8192])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--atomic-rate", type=float, default=None, help="atomics/s (default: run tools/calib_atomic.hip)")
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    from quadraturefields_amd import synthetic
    rate = args.atomic_rate
    if rate is None:
        try:
            rate = calibrated_atomic_rate()
        except (OSError, subprocess.SubprocessError, AttributeError) as e:
            print(f"# atomic calibration unavailable ({e}); atomic fractions omitted", file=sys.stderr)
    print(json.dumps({"atomic_rate_per_s": rate, "hbm_bytes_per_s": HBM_BYTES_PER_S}))
    shell = synthetic.shell_mesh()
    for size in args.sizes:
        charts, _ = synthetic.per_triangle_charts(shell, size)
        for name, mesh in (("shell_mesh", shell), ("per_triangle_charts", charts)):
            print(json.dumps(run(name, mesh, size, size, args.iters, rate, dev)), flush=True)


if __name__ == "__main__":
    main()
