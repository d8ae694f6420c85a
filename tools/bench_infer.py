#!/usr/bin/env python3
"""Inference benchmark — BASELINE config 4: RAFT-NCUP, KITTI shape 288x960,
24 refinement iterations, hipGraph-captured, 1 GPU. Prints eager vs graphed
pairs/sec as JSON lines.

    python tools/bench_infer.py [--iters 24] [--height 288] [--width 960]
                                [--alternate_corr] [--reps 20] [--no_eager]

Every line also carries `max_mem_mb` (torch.cuda.max_memory_allocated).
"""

import argparse
import json
import sys
import time

import torch

sys.path.insert(0, ".")

from flowhip.config.args import default_ncup_args
from flowhip.engine.graph import GraphedInference
from flowhip.models import build_model


def timeit(fn, warmup=3, iters=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=24)
    ap.add_argument("--height", type=int, default=288)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--model", default="raft_nc_dbl")
    ap.add_argument("--alternate_corr", action="store_true",
                    help="on-demand correlation lookup (no all-pairs volume)")
    ap.add_argument("--reps", type=int, default=20, help="timed repetitions")
    ap.add_argument("--no_eager", action="store_true",
                    help="time the hipGraph replay only (large frames)")
    args = ap.parse_args()

    dev = torch.device("cuda:0")
    margs = default_ncup_args(model=args.model, mixed_precision=True,
                              alternate_corr=args.alternate_corr)
    torch.manual_seed(1234)
    model = build_model(margs).to(dev).eval()

    shape = (args.batch, 3, args.height, args.width)
    img1 = torch.rand(shape, device=dev) * 255
    img2 = torch.rand(shape, device=dev) * 255

    def mem_mb():
        return torch.cuda.max_memory_allocated() / 2 ** 20

    tag = {"alternate_corr": args.alternate_corr, "iters": args.iters,
           "hw": [args.height, args.width], "batch": args.batch}
    t_eager = None
    if not args.no_eager:
        with torch.no_grad():
            t_eager = timeit(lambda: model(img1, img2, iters=args.iters,
                                           test_mode=True), iters=args.reps)
        print(json.dumps({"probe": "infer_eager", "ms": t_eager * 1e3,
                          "pairs_per_sec": args.batch / t_eager,
                          "max_mem_mb": mem_mb(), **tag}), flush=True)

    g = GraphedInference(model, shape, args.iters)
    with torch.no_grad():
        low_e, up_e = model(img1, img2, iters=args.iters, test_mode=True)
    low_g, up_g = g(img1, img2)
    err = (up_g - up_e).abs().max().item()
    t_graph = timeit(lambda: g(img1, img2), iters=args.reps)
    print(json.dumps({"probe": "infer_hipgraph", "ms": t_graph * 1e3,
                      "pairs_per_sec": args.batch / t_graph,
                      "speedup_vs_eager": (t_eager / t_graph
                                           if t_eager else None),
                      "max_abs_diff_vs_eager": err,
                      "max_mem_mb": mem_mb(), **tag}), flush=True)


if __name__ == "__main__":
    main()
