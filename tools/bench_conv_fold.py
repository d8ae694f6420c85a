"""Generic against tap-folded kernels (csrc/conv_fold.h) on the three
small-Cin 7x7 layers of the flagship step, forward and weight gradient
(partials + reduce), in one process, alternating rounds (the protocol of
tools/bench_wrw.py: median and min-max over --rounds, each of --iters calls).

    python tools/bench_conv_fold.py [--iters 30] [--rounds 5] [--nchunks 37,96]

One JSON line per shape: microseconds per call for the generic and folded
forward and for the weight gradient on the generic path and in both ky
forms of the folded kernel (form 0: ky in the grid, form 1: ky looped in
the workgroup), each form's planned chunk count, and the share of the byte
floor each variant reaches: the bytes every variant must move at least
(input padded to 8 channels + output, or input + dy) over --tbps.
`--nchunks` additionally times both folded forms at forced chunk counts.

    python tools/bench_conv_fold.py --accumulate [--calls 12]

times convf1's weight gradient per backward pass of --calls shared calls:
accumulating partials + one finish, on the generic path and in both
folded forms, and the folded one-shot partials with a finish into the
running dW. flowhip_conv_fold_wrw_plan and flowhip_conv_fold_accumulate_wins
follow this output.
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (name, B, H, W, real Cin, Cout, stride)
SHAPES = [("stem_fnet_b6", 6, 448, 1024, 3, 64, 2),
          ("stem_cnet_b3", 3, 448, 1024, 3, 64, 2),
          ("convf1_b3", 3, 56, 128, 2, 128, 1)]
K = 7


def _cl(t):
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


def _rounds(variants, args):
    times = {k: [] for k, _ in variants}
    for _, fn in variants:
        _time(fn, 3)
    for _ in range(args.rounds):
        for k, fn in variants:
            times[k].append(_time(fn, args.iters))
    return times


def _inputs(shape, dev):
    name, B, H, W, Cin, Cout, s = shape
    x = torch.zeros(B, 8, H, W, device=dev)
    x[:, :Cin] = torch.randn(B, Cin, H, W, device=dev) / 4
    x8 = _cl(x.to(torch.bfloat16))
    w8 = torch.zeros(Cout, 8, K, K, device=dev)
    w8[:, :Cin] = torch.randn(Cout, Cin, K, K, device=dev) / 8
    b = torch.randn(Cout, device=dev)
    OH, OW = (H - 1) // s + 1, (W - 1) // s + 1
    dy = _cl((torch.randn(B, Cout, OH, OW, device=dev) / 4).to(torch.bfloat16))
    return x8, w8, b, dy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--nchunks", type=str, default="")
    ap.add_argument("--only", type=str, default="")
    ap.add_argument("--accumulate", action="store_true")
    ap.add_argument("--calls", type=int, default=12)
    ap.add_argument("--tbps", type=float, default=6.3,
                    help="achievable HBM bandwidth for the byte floor")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_conv_fold needs a GPU")
    import flowhip._C as C
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    sweep = [int(v) for v in args.nchunks.split(",") if v != ""]

    for shape in SHAPES:
        name, B, H, W, Cin, Cout, s = shape
        if args.only and args.only not in name:
            continue
        if args.accumulate and s != 1:
            continue
        x8, w8, b, dy = _inputs(shape, dev)
        smode = 0 if s == 1 else 1

        def plan(algo, form):
            return C.conv_gemm_wrw_plan(dy, x8, None, K, K, s, s, True, algo,
                                        0, form)

        if args.accumulate:
            def passes(algo, form, accumulate):
                path, nchunk, numel, _ = plan(algo, form)

                def run():
                    buf = torch.empty(numel, dtype=torch.float32, device=dev)
                    dw = db = None
                    for i in range(args.calls):
                        C.conv_gemm_wrw_partials(
                            dy, x8, None, buf, K, K, s, s, True,
                            accumulate and i > 0, path, nchunk, form)
                        if not accumulate:
                            dw, db = C.conv_gemm_wrw_finish(
                                buf, Cout, 8, K, K, True, nchunk, dw, db,
                                path)
                    if accumulate:
                        dw, db = C.conv_gemm_wrw_finish(
                            buf, Cout, 8, K, K, True, nchunk, None, None,
                            path)
                    return dw
                return run, nchunk, numel

            specs = [("generic_accumulated", 0, -1, True),
                     ("fold0_accumulated", 2, 0, True),
                     ("fold1_accumulated", 2, 1, True),
                     ("fold0_finish_into", 2, 0, False)]
            built = [(k,) + passes(a, f, acc) for k, a, f, acc in specs]
            times = _rounds([(k, fn) for k, fn, _, _ in built], args)
            print(json.dumps({
                "shape": name, "calls": args.calls,
                "nchunk": {k: n for k, _, n, _ in built},
                "partials_MB": {k: round(m * 4 / 2 ** 20, 2)
                                for k, _, _, m in built},
                "us_per_pass": {k: round(statistics.median(v), 1)
                                for k, v in times.items()},
                "us_min": {k: round(min(v), 1) for k, v in times.items()},
                "us_max": {k: round(max(v), 1) for k, v in times.items()},
            }), flush=True)
            continue

        wg = C.conv_gemm_pack(w8, False, False)
        wf = C.conv_gemm_pack(w8, False, True)

        def fwd(wpk, fold):
            return C.conv_gemm_fwd2(x8, None, wpk, b, Cout, K, K, 0, 0, s, s,
                                    smode, 0, 0, fold)[0]

        def wrw(algo, form=-1, nchunk=0):
            return C.conv_gemm_wrw(dy, x8, None, K, K, s, s, True, algo,
                                   nchunk, form)

        fdiff = (fwd(wg, False).float() - fwd(wf, True).float()).abs().max()
        dw_g = wrw(0)[0]
        wdiff = max((dw_g - wrw(2, f)[0]).abs().max().item() for f in (0, 1))
        variants = [("fwd_generic", lambda: fwd(wg, False)),
                    ("fwd_folded", lambda: fwd(wf, True)),
                    ("wrw_generic", lambda: wrw(0)),
                    ("wrw_fold0", lambda: wrw(2, 0)),
                    ("wrw_fold1", lambda: wrw(2, 1))]
        for n in sweep:
            variants.append((f"wrw_fold0_n{n}", lambda n=n: wrw(2, 0, n)))
            variants.append((f"wrw_fold1_n{n}", lambda n=n: wrw(2, 1, n)))
        times = _rounds(variants, args)
        med = {k: statistics.median(v) for k, v in times.items()}
        # bytes no variant can avoid: the 8-channel input once, and the
        # output (forward) or dy (weight gradient) once
        floor_us = (x8.numel() + dy.numel()) * 2 / (args.tbps * 1e12) * 1e6
        print(json.dumps({
            "shape": name, "B": B, "H": H, "W": W, "Cin": Cin, "Cout": Cout,
            "stride": s,
            # planned: the rule's own form shows in its chunk count
            "nchunk": {"generic": plan(0, -1)[1], "fold0": plan(2, 0)[1],
                       "fold1": plan(2, 1)[1], "planned": plan(2, -1)[1]},
            "us": {k: round(v, 2) for k, v in med.items()},
            "us_min": {k: round(min(v), 2) for k, v in times.items()},
            "us_max": {k: round(max(v), 2) for k, v in times.items()},
            "floor_us": round(floor_us, 2),
            "floor_share": {k: round(floor_us / v, 3)
                            for k, v in med.items()},
            "max_abs_diff_fwd": fdiff.item(), "max_abs_diff_dw": wdiff,
        }), flush=True)


if __name__ == "__main__":
    main()
