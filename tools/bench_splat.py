"""Forward-splat kernel alone (csrc/forward_splat.hip) at the low-res field
sizes of KITTI 288x960 (36x120), Sintel 436x1024 (55x128), 1080p (135x240)
and 4K (270x480) inference: the planned source chunk count G against a
forced single pass (G = 1), in one process, alternating rounds.

    python tools/bench_splat.py [--iters 20] [--rounds 5] [--sigma 4.0]

One JSON line per shape: median / min / max microseconds per call for both,
the brute force's pair count, whether the two paths agree bit for bit, and —
where scipy imports — the host time of the reference's route for the same
field (geometry.forward_interpolate, device-to-host copy included).
"""

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(36, 120), (55, 128), (135, 240), (270, 480)]


def _time(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / iters  # us per call


def _scipy_ms(flow, reps):
    try:
        import scipy  # noqa: F401
    except ImportError:
        return None
    from flowhip.utils.geometry import forward_interpolate
    forward_interpolate(flow[0])
    t0 = time.perf_counter()
    for _ in range(reps):
        forward_interpolate(flow[0])
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sigma", type=float, default=4.0,
                    help="std of the seeded gaussian flow, in cells")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_splat needs a GPU")
    import flowhip._C as C
    dev = torch.device("cuda:0")

    for (H, W) in SHAPES:
        g = torch.Generator().manual_seed(1000 * H + W)
        flow = (torch.randn(1, 2, H, W, generator=g) * args.sigma).to(dev)
        G = C.forward_splat_plan(H, W)
        # the 4K field is ~1.7e10 pair tests per call: fewer calls per round
        iters = args.iters if H * W < 50000 else max(2, args.iters // 5)

        variants = [("planned", 0), ("g1", 1)]
        outs = {k: C.forward_splat(flow, s) for k, s in variants}
        torch.cuda.synchronize()
        times = {k: [] for k, _ in variants}
        for k, s in variants:          # warm every variant
            _time(lambda: C.forward_splat(flow, s), 2)
        for _ in range(args.rounds):   # alternate the variants per round
            for k, s in variants:
                times[k].append(_time(lambda: C.forward_splat(flow, s), iters))
        scipy_ms = _scipy_ms(flow, 3 if H * W > 50000 else 10)
        rec = {
            "probe": "forward_splat", "H": H, "W": W, "sigma": args.sigma,
            "G": G, "pairs": (H * W) ** 2,
            "us": {k: round(statistics.median(v), 2)
                   for k, v in times.items()},
            "us_min": {k: round(min(v), 2) for k, v in times.items()},
            "us_max": {k: round(max(v), 2) for k, v in times.items()},
            "planned_equals_g1": torch.equal(outs["planned"], outs["g1"]),
            "host_scipy_ms": None if scipy_ms is None else round(scipy_ms, 3),
        }
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
