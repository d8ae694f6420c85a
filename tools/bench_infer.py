#!/usr/bin/env python3
"""Inference benchmark — BASELINE config 4: RAFT-NCUP, KITTI shape 288x960,
24 refinement iterations, hipGraph-captured, 1 GPU. Prints eager vs graphed
pairs/sec as JSON lines.

    python tools/bench_infer.py [--iters 24] [--height 288] [--width 960]
                                [--alternate_corr] [--reps 20] [--no_eager]
                                [--warm_start] [--bidirectional]

Every line also carries `max_mem_mb` (torch.cuda.max_memory_allocated).

--warm_start times sequence inference instead, each frame pair started from
the previous pair's splatted flow: ms per frame with the host scipy splat,
with the device splat run eagerly, and with the device splat inside the
replayed graph (plus `max_abs_diff_vs_eager` between the two device routes).

--bidirectional times both directions of one frame pair, each build in a
fresh peak-memory window: two graphed unidirectional replays, (a,b) then
(b,a); the graphed bidirectional replay (`ratio_vs_two_calls` against the
former); the same with the consistency check in the graph (`added_ms`); and
`ops.fb_consistency` alone on that `flow_up`, the HIP kernel against its
float64 torch twin.
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


def bench_bidirectional(model, args, tag):
    """Both directions of one pair: two unidirectional replays against one
    bidirectional replay, with and without the consistency check; then the
    check alone, kernel against twin."""
    from flowhip import ops
    from flowhip.ops import torch_ref

    dev = next(model.parameters()).device
    shape = (args.batch, 3, args.height, args.width)
    gen = torch.Generator().manual_seed(4321)
    a = (torch.rand(shape, generator=gen) * 255).to(dev)
    b = (torch.rand(shape, generator=gen) * 255).to(dev)

    def report(probe, **fields):
        print(json.dumps({"probe": probe, **fields,
                          "max_mem_mb": torch.cuda.max_memory_allocated()
                          / 2 ** 20, **tag}), flush=True)

    def fresh():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()

    fresh()
    g = GraphedInference(model, shape, args.iters)

    def two_calls():
        g(a, b)
        g(b, a)
    t_two = timeit(two_calls, iters=args.reps) * 1e3
    up_fw = g(a, b)[1].clone()
    up_bw = g(b, a)[1].clone()
    report("two_unidirectional_hipgraph", ms=t_two)
    del g

    fresh()
    g = GraphedInference(model, shape, args.iters, bidirectional=True)
    t_bi = timeit(lambda: g(a, b), iters=args.reps) * 1e3
    up = g(a, b)[1]
    sep = torch.cat([up_fw, up_bw])
    err = (up - sep).abs().max().item()
    report("bidirectional_hipgraph", ms=t_bi,
           ratio_vs_two_calls=t_bi / t_two, max_abs_diff_vs_two_calls=err,
           max_abs_flow=sep.abs().max().item())
    del g, up

    # the batch sensitivity the kernels have without this feature: the plain
    # forward on the stacked pairs (eager, once) against the same two calls
    fresh()
    with torch.no_grad():
        err0 = (model(torch.cat([a, b]), torch.cat([b, a]), iters=args.iters,
                      test_mode=True)[1] - sep).abs().max().item()
    report("stacked_unidirectional_eager", max_abs_diff_vs_two_calls=err0)
    del sep

    fresh()
    g = GraphedInference(model, shape, args.iters, bidirectional=True,
                         consistency=True)
    t_chk = timeit(lambda: g(a, b), iters=args.reps) * 1e3
    up = g(a, b)[1].clone()
    stats = g.consistency[4].clone()
    npix = args.height * args.width
    report("bidirectional_consistency_hipgraph", ms=t_chk,
           added_ms=t_chk - t_bi, ratio_vs_two_calls=t_chk / t_two,
           visible_share=(stats[..., 0] / npix).flatten().tolist())
    del g

    # the check alone on that flow_up: variants interleaved in one process
    fw, bw = up[:args.batch], up[args.batch:]
    variants = {
        "hip": lambda: ops.fb_consistency(fw, bw),
        "torch_twin": lambda: torch_ref.fb_consistency(fw, bw),
    }
    times = {k: [] for k in variants}
    for fn in variants.values():
        timeit(fn, warmup=2, iters=2)
    for _ in range(5):
        for k, fn in variants.items():
            times[k].append(timeit(fn, warmup=0, iters=10) * 1e3)
    got, ref = variants["hip"](), variants["torch_twin"]()
    fresh()
    report("fb_consistency_alone",
           **{k + "_ms_median": sorted(v)[len(v) // 2]
              for k, v in times.items()},
           **{k + "_ms_min": min(v) for k, v in times.items()},
           occ_mismatches=int((got[0] != ref[0]).sum()
                              + (got[1] != ref[1]).sum()),
           counts_equal=bool(torch.equal(got[4][..., :3], ref[4][..., :3])))


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
    ap.add_argument("--bidirectional", action="store_true",
                    help="time both directions of a pair: one bidirectional "
                    "replay (with and without the consistency check) against "
                    "two unidirectional replays; the check against its twin")
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
    if args.bidirectional:
        bench_bidirectional(model, args, tag)
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
