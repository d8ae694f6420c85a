"""Normalized-convolution backward A/B at the flagship NCUP shapes: the
split kernels with their torch glue (algo 0) against the fused kernel
(algo 1) of nconv_bwd_fused, in one process, alternating rounds.

    python tools/bench_nconv_bwd.py [--iters 30] [--rounds 5] [--strips 1,2,4,7]

One JSON line per layer: median microseconds per whole-layer backward
(everything NConv2dFn.backward launches) for each path, min and max over
the rounds, the speed-up, and the two paths' max-abs differences.
`--strips` additionally times the fused path at forced strip lengths (tile
rows per workgroup; 0 = its own choice). The strip rule in
flowhip_nconv_bwd_fused_plan follows this output.
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (name, N, H, W, Ci, Co, K, gcout given)
LAYERS = [
    ("nconv_in_1to2_5x5", 6, 448, 1024, 1, 2, 5, True),
    ("nconv_x2_2to2_5x5", 6, 448, 1024, 2, 2, 5, True),
    ("decoder0_4to2_3x3", 6, 448, 1024, 4, 2, 3, True),
    ("decoder0_folded_2to2_3x3", 6, 448, 1024, 2, 2, 3, True),
    ("nconv_out_2to1_1x1", 6, 448, 1024, 2, 1, 1, False),
]


def _time(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / iters  # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--strips", type=str, default="",
                    help="comma list of forced fused strip lengths to time")
    ap.add_argument("--only", type=str, default="",
                    help="substring filter on layer names")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_nconv_bwd needs a GPU")
    import flowhip._C as C
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    sweep = [int(v) for v in args.strips.split(",") if v != ""]

    for (name, N, H, W, Ci, Co, K, has_gcout) in LAYERS:
        if args.only and args.only not in name:
            continue
        data = torch.randn(N, Ci, H, W, device=dev)
        conf = 0.1 + 0.9 * torch.rand(N, Ci, H, W, device=dev)
        weight = torch.rand(Co, Ci, K, K, device=dev) + 0.05
        out, cout = C.nconv_fwd(data, conf, weight, None)
        gout = torch.randn_like(out)
        gcout = torch.randn_like(out) if has_gcout else None

        def call(algo, strip=0):
            return C.nconv_bwd_fused(gout, gcout, out, cout, data, conf,
                                     weight, None, 1e-20, algo, strip)

        rs = call(0)
        rf = call(1)
        torch.cuda.synchronize()
        diff = {k: (a - b).abs().max().item()
                for k, a, b in zip(("ddata", "dconf", "dweight"), rs, rf)}
        variants = [("split", 0, 0), ("fused", 1, 0)] + \
            [(f"fused_s{s}", 1, s) for s in sweep if s > 0]
        times = {k: [] for k, _, _ in variants}
        for k, a, s in variants:       # warm every variant
            _time(lambda: call(a, s), 3)
        for _ in range(args.rounds):   # alternate the variants per round
            for k, a, s in variants:
                times[k].append(_time(lambda: call(a, s), args.iters))
        med = {k: statistics.median(v) for k, v in times.items()}
        rec = {
            "layer": name, "N": N, "H": H, "W": W, "Ci": Ci, "Co": Co,
            "K": K, "gcout": has_gcout,
            "us": {k: round(v, 2) for k, v in med.items()},
            "us_min": {k: round(min(v), 2) for k, v in times.items()},
            "us_max": {k: round(max(v), 2) for k, v in times.items()},
            "speedup_fused": round(med["split"] / med["fused"], 3),
            "max_abs_diff": diff,
        }
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
