#!/usr/bin/env python3
"""Inference benchmark — BASELINE config 4: RAFT-NCUP, KITTI shape 288x960,
24 refinement iterations, hipGraph-captured, 1 GPU. Prints eager vs graphed
pairs/sec as JSON lines.

    python tools/bench_infer.py [--iters 24] [--height 288] [--width 960]
                                [--alternate_corr] [--reps 20] [--no_eager]
                                [--warm_start]

Every line also carries `max_mem_mb` (torch.cuda.max_memory_allocated).

--warm_start times sequence inference instead, each frame pair started from
the previous pair's splatted flow: ms per frame with the host scipy splat,
with the device splat run eagerly, and with the device splat inside the
replayed graph (plus `max_abs_diff_vs_eager` between the two device routes).
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


def bench_warm_start(model, args, tag):
    """Per-frame time of warm-started sequence inference, three ways: the
    host scipy splat (the reference's route), the device splat run eagerly,
    and the device splat inside the replayed hipGraph."""
    from flowhip.engine.stream import FlowStream
    from flowhip.utils.geometry import InputPadder, forward_interpolate

    dev = next(model.parameters()).device
    shape = (args.batch, 3, args.height, args.width)
    # padded to multiples of 8 as the evaluators do (436 -> 440 rows)
    padder = InputPadder(shape)
    g = torch.Generator().manual_seed(4321)
    frames = [padder.pad((torch.rand(shape, generator=g) * 255).to(dev))[0]
              for _ in range(5)]
    n = len(frames)
    shape = tuple(frames[0].shape)
    tag = dict(tag, padded_hw=list(shape[-2:]))

    def run(step, steps):
        """`steps` consecutive pairs; the last pair's upsampled flow."""
        up = None
        for i in range(steps):
            up = step(frames[i % n], frames[(i + 1) % n])[1]
        return up

    def timed(step):
        run(step, 3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(step, args.reps)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.reps * 1e3

    def report(probe, ms, **extra):
        print(json.dumps({"probe": probe, "ms_per_frame": ms, **extra,
                          "max_mem_mb": torch.cuda.max_memory_allocated()
                          / 2 ** 20, **tag}), flush=True)

    have_scipy = True
    try:
        import scipy  # noqa: F401
    except ImportError:
        have_scipy = False
    if have_scipy and args.batch == 1:
        state = {"prev": None}

        @torch.no_grad()
        def host_step(im1, im2):
            low, up = model(im1, im2, iters=args.iters,
                            flow_init=state["prev"], test_mode=True)
            state["prev"] = forward_interpolate(low[0])[None].to(dev)
            return low, up
        report("warm_start_host_scipy", timed(host_step))
    else:
        report("warm_start_host_scipy", None,
               note="scipy missing or batch > 1")

    eager = FlowStream(model, args.iters)
    report("warm_start_device_eager", timed(eager.step))

    graphed = FlowStream(model, args.iters, graphed=True, input_shape=shape)
    ms = timed(graphed.step)
    # same sequence from a cold start through both device routes
    eager.reset()
    graphed.reset()
    steps = 4
    err = (run(graphed.step, steps) - run(eager.step, steps)).abs().max()
    report("warm_start_device_hipgraph", ms,
           max_abs_diff_vs_eager=err.item())


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
    ap.add_argument("--warm_start", action="store_true",
                    help="time warm-started sequence inference per frame: "
                    "host scipy splat, eager device splat, splat in the graph")
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
    if args.warm_start:
        bench_warm_start(model, args, tag)
        return
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
