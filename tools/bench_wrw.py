"""Weight-gradient A/B at the flagship shape inventory: the generic per-tap
kernel (algo 0) against the halo-staged kernel (algo 1) of
conv_gemm_wrw, in one process, alternating rounds.

    python tools/bench_wrw.py [--iters 30] [--rounds 5] [--nchunks 0,16,64]

One JSON line per shape: median microseconds per call (partials kernel +
reduce) for each path, the speed-up, and both paths' max-abs difference.
`--nchunks` additionally times the halo path at forced split-M chunk
counts (0 = its own choice). The dispatch table in
flowhip_conv_gemm_wrw_plan follows this output.

    python tools/bench_wrw.py --accumulate [--calls 12] [--rounds 5]

times what a conv shared by the refinement iterations costs per backward
pass on the planned (auto) path: `--calls` one-shot calls plus the
`--calls - 1` fp32 adds of dW and dbias that autograd does between them,
against `--calls` accumulating partials launches into one buffer plus one
finish, and against `--calls` one-shot partials whose finish adds to a
running dW (`finish_into`). Same protocol: alternating rounds, median and min-max per variant.
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
# the refinement loop's convs outside the halo envelope: (.., ld_extra)
# convc1 reads the 324-of-328 narrowed correlation view; convf1 sees the
# flow padded 2 -> 8 channels
LOOP_EXTRA = [("upd_324to256_1x1", 3, 56, 128, 324, 0, 256, 1, 1, 4),
              ("upd_8to128_7x7", 3, 56, 128, 8, 0, 128, 7, 7, 0)]


PATHS = {0: "generic", 1: "halo", 2: "folded"}


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


def accumulate_mode(args, C, dev):
    shapes = [c + (0,) for c in UPDATE] + LOOP_EXTRA
    for (name, B, H, W, C1, C2, Cout, KH, KW, ld_extra) in shapes:
        if args.only and args.only not in name:
            continue
        x1 = _cl(B, C1 + ld_extra, H, W, dev)
        if ld_extra:
            x1 = x1[:, :C1]
        x2 = _cl(B, C2, H, W, dev) if C2 else None
        op = Cout + (-Cout) % 8
        dy = _cl(B, op, H, W, dev)
        if op != Cout:
            dy[:, Cout:] = 0
        path, nchunk, numel, rule = C.conv_gemm_wrw_plan(dy, x1, x2, KH, KW,
                                                         1, 1, True)

        def one_shot():
            dw, db = C.conv_gemm_wrw(dy, x1, x2, KH, KW, 1, 1, True, path,
                                     nchunk)
            for _ in range(args.calls - 1):
                dw2, db2 = C.conv_gemm_wrw(dy, x1, x2, KH, KW, 1, 1, True,
                                           path, nchunk)
                dw.add_(dw2)
                db.add_(db2)
            return dw, db

        def accumulated():
            buf = torch.empty(numel, dtype=torch.float32, device=dev)
            for i in range(args.calls):
                C.conv_gemm_wrw_partials(dy, x1, x2, buf, KH, KW, 1, 1, True,
                                         i > 0, path, nchunk)
            return C.conv_gemm_wrw_finish(buf, op, C1 + C2, KH, KW, True,
                                          nchunk, None, None, path)

        def finish_into():
            buf = torch.empty(numel, dtype=torch.float32, device=dev)
            dw = db = None
            for i in range(args.calls):
                C.conv_gemm_wrw_partials(dy, x1, x2, buf, KH, KW, 1, 1, True,
                                         False, path, nchunk)
                dw, db = C.conv_gemm_wrw_finish(buf, op, C1 + C2, KH, KW,
                                                True, nchunk, dw, db, path)
            return dw, db

        dw_o, db_o = one_shot()
        dw_a, db_a = accumulated()
        dw_f, db_f = finish_into()
        torch.cuda.synchronize()
        assert torch.equal(dw_f, dw_o) and torch.equal(db_f, db_o)
        variants = [("one_shot", one_shot), ("accumulated", accumulated),
                    ("finish_into", finish_into)]
        times = {k: [] for k, _ in variants}
        for k, fn in variants:
            _time(fn, 2)
        for _ in range(args.rounds):
            for k, fn in variants:
                times[k].append(_time(fn, args.iters))
        med = {k: statistics.median(v) for k, v in times.items()}
        print(json.dumps({
            "shape": name, "B": B, "H": H, "W": W, "Cin": C1 + C2,
            "Cout": Cout, "K": f"{KH}x{KW}", "calls": args.calls,
            "path": PATHS[path], "nchunk": nchunk,
            "partials_MB": round(numel * 4 / 2 ** 20, 2),
            "us_per_pass": {k: round(v, 1) for k, v in med.items()},
            "us_min": {k: round(min(v), 1) for k, v in times.items()},
            "us_max": {k: round(max(v), 1) for k, v in times.items()},
            "saved_us": round(med["one_shot"] - med["accumulated"], 1),
            "saved_us_finish_into": round(
                med["one_shot"] - med["finish_into"], 1),
            "plan_accumulates": bool(rule),
            "max_abs_diff_dw": (dw_o - dw_a).abs().max().item(),
            "max_abs_diff_dbias": (db_o - db_a).abs().max().item(),
        }), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--nchunks", type=str, default="",
                    help="comma list of forced halo chunk counts to time")
    ap.add_argument("--only", type=str, default="",
                    help="substring filter on shape names")
    ap.add_argument("--accumulate", action="store_true",
                    help="one-shot calls + adds against accumulating calls "
                         "+ one finish, per backward pass")
    ap.add_argument("--calls", type=int, default=12,
                    help="uses of the weight per backward pass (--accumulate)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_wrw needs a GPU")
    import flowhip._C as C
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    if args.accumulate:
        return accumulate_mode(args, C, dev)
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
