#!/usr/bin/env python3
"""Per-lookup backward time of the on-demand correlation lookup under each
FLOWHIP_ALT_CORR_BWD mode (torch / direct / tiled), alternated in one
process: D=256, r=4, 4 levels, bf16 NHWC cotangent in the forward output's
own layout, smooth coordinates (grid + (2.375, -1.625) + jitter in +-0.5).
Next to each time it prints the float-atomic bytes the shape implies (an
upper bound: out-of-map and zero positions are skipped), i.e. the share of
the ~1.3 TB/s chip-wide atomic rate. One JSON line per (shape, mode).

    python tools/bench_alt_corr_bwd.py [--calls 20] [--coords smooth|rand]
"""

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, ".")

from flowhip import ops  # noqa: E402
from flowhip.utils import layout  # noqa: E402
from flowhip.utils.geometry import coords_grid  # noqa: E402

# (B, H, W): 128x256 training crops, 440x1024 at batch 3, 1088x1920 frames
SHAPES = [(2, 16, 32), (3, 56, 128), (1, 136, 240)]
D, R, L = 256, 4, 4
TORCH_MAX_P = 56 * 128      # the chunked recompute is O(P^2 D): skip above

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--coords", default="smooth", choices=["smooth", "rand"])
opt = ap.parse_args()

dev = torch.device("cuda:0")
layout.set_channels_last(True)
layout.set_corr_bf16(True)
K, KP, BOX = 2 * R + 1, 2 * R + 2, 2 * R + 2 + 4

for B, H, W in SHAPES:
    P = H * W
    torch.manual_seed(7)
    f1 = torch.randn(B, D, H, W, device=dev, requires_grad=True)
    f2 = torch.randn(B, D, H, W, device=dev, requires_grad=True)
    if opt.coords == "smooth":
        coords = (coords_grid(B, H, W, device=dev)
                  + torch.tensor([2.375, -1.625], device=dev).view(1, 2, 1, 1)
                  + torch.rand(B, 2, H, W, device=dev) - 0.5)
    else:
        coords = torch.rand(B, 2, H, W, device=dev) * torch.tensor(
            [W + 12.0, H + 12.0], device=dev).view(1, 2, 1, 1) - 6.0
    out = ops.alt_corr_lookup(f1, ops.alt_corr_pyramid(f2, L), coords, R,
                              fmap2=f2)
    assert out.dtype == torch.bfloat16
    # the cotangent in the output's own (padded NHWC) layout: no copy
    g = torch.empty_strided(out.shape, out.stride(), dtype=out.dtype,
                            device=dev)
    g.copy_(torch.randn(out.shape, device=dev))
    tiles = B * ((H + 3) // 4) * ((W + 3) // 4)
    atomic_mb = {"torch": 0.0,
                 "direct": B * P * L * KP * KP * D * 4 / 1e6,
                 "tiled": tiles * L * BOX * BOX * D * 4 / 1e6}
    modes = ["torch", "direct", "tiled"]
    if P > TORCH_MAX_P:
        modes.remove("torch")

    def backward(mode):
        os.environ["FLOWHIP_ALT_CORR_BWD"] = mode
        return torch.autograd.grad(out, (f1, f2), g, retain_graph=True)

    times = {m: [] for m in modes}
    for m in modes:
        for _ in range(opt.warmup):
            backward(m)
    torch.cuda.synchronize()
    for _ in range(opt.calls):
        for m in modes:                      # alternated: shared drift
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            backward(m)
            e1.record()
            e1.synchronize()
            times[m].append(e0.elapsed_time(e1))
    for m in modes:
        t = sorted(times[m])
        med = t[len(t) // 2]
        print(json.dumps({
            "probe": "alt_corr_bwd", "coords": opt.coords, "B": B, "H": H,
            "W": W, "D": D, "r": R, "mode": m, "calls": len(t),
            "ms_median": round(med, 4), "ms_min": round(t[0], 4),
            "ms_max": round(t[-1], 4),
            "atomic_mb": round(atomic_mb[m], 1),
            "atomic_floor_ms": round(atomic_mb[m] / 1.3e3, 4),
        }), flush=True)
os.environ.pop("FLOWHIP_ALT_CORR_BWD", None)
