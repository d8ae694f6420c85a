"""Weight-gradient A/B at the flagship shape inventory: the generic per-tap
kernel (algo 0) against the halo-staged kernel (algo 1) of
conv_gemm_wrw, in one process, alternating rounds.

    python tools/bench_wrw.py [--iters 30] [--rounds 5] [--nchunks 0,16,64]

One JSON line per shape: median microseconds per call (partials kernel +
reduce) for each path, the speed-up, and both paths' max-abs difference.
`--nchunks` additionally times the halo path at forced split-M chunk
counts (0 = its own choice). The dispatch table in
flowhip_conv_gemm_wrw_plan follows this output.
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (name, B, H, W, C1, C2, Cout, KH, KW)
UPDATE = [(f"upd_{c1 + c2}to{o}_{kh}x{kw}", 3, 56, 128, c1, c2, o, kh, kw)
          for (c1, c2, o, kh, kw) in [
              (256, 0, 192, 3, 3), (128, 0, 64, 3, 3), (256, 0, 126, 3, 3),
              (128, 0, 256, 3, 3), (256, 0, 2, 3, 3),
              (128, 256, 256, 1, 5), (128, 256, 256, 5, 1),
              (128, 256, 128, 1, 5), (128, 256, 128, 5, 1)]]
ENCODER = [(f"enc_{c}to{c}_b{b}_{h}x{w}", b, h, w, c, 0, c, 3, 3)
           for (c, h, w) in [(64, 224, 512), (96, 112, 256), (128, 56, 128)]
           for b in (6, 3)]


def _cl(b, c, h, w, dev):
    t = (torch.randn(b, c, h, w, device=dev) / 4).to(torch.bfloat16)
    return t.contiguous(memory_format=torch.channels_last)


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
    ap.add_argument("--nchunks", type=str, default="",
                    help="comma list of forced halo chunk counts to time")
    ap.add_argument("--only", type=str, default="",
                    help="substring filter on shape names")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_wrw needs a GPU")
    import flowhip._C as C
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    sweep = [int(v) for v in args.nchunks.split(",") if v != ""]

    for (name, B, H, W, C1, C2, Cout, KH, KW) in UPDATE + ENCODER:
        if args.only and args.only not in name:
            continue
        x1 = _cl(B, C1, H, W, dev)
        x2 = _cl(B, C2, H, W, dev) if C2 else None
        op = Cout + (-Cout) % 8  # the autograd functions pad dy to %8
        dy = _cl(B, op, H, W, dev)
        if op != Cout:
            dy[:, Cout:] = 0

        def call(algo, nchunk=0):
            return C.conv_gemm_wrw(dy, x1, x2, KH, KW, 1, 1, True, algo,
                                   nchunk)

        dw_g, db_g = call(0)
        dw_h, db_h = call(1)
        torch.cuda.synchronize()
        diff = (dw_g - dw_h).abs().max().item()
        bdiff = (db_g - db_h).abs().max().item()
        variants = [("generic", 0, 0), ("halo", 1, 0)] + \
            [(f"halo_n{n}", 1, n) for n in sweep if n > 0]
        times = {k: [] for k, _, _ in variants}
        for k, a, n in variants:       # warm every variant
            _time(lambda: call(a, n), 3)
        for _ in range(args.rounds):   # alternate the variants per round
            for k, a, n in variants:
                times[k].append(_time(lambda: call(a, n), args.iters))
        med = {k: statistics.median(v) for k, v in times.items()}
        rec = {
            "shape": name, "B": B, "H": H, "W": W, "Cin": C1 + C2,
            "Cout": Cout, "K": f"{KH}x{KW}",
            "us": {k: round(v, 2) for k, v in med.items()},
            "us_min": {k: round(min(v), 2) for k, v in times.items()},
            "us_max": {k: round(max(v), 2) for k, v in times.items()},
            "speedup_halo": round(med["generic"] / med["halo"], 3),
            "max_abs_diff_dw": diff, "max_abs_diff_dbias": bdiff,
        }
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
