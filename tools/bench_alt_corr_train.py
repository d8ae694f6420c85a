#!/usr/bin/env python3
"""Train-step time (forward + backward) of raft_nc_dbl at 128x256, batch 2,
12 iterations, mixed precision, with and without `alternate_corr` — the
cost of the on-demand mode's chunked backward (profiles/README.md). One
JSON line per mode.

    python tools/bench_alt_corr_train.py
"""

import json
import sys
import time

import torch

sys.path.insert(0, ".")

from flowhip import ops  # noqa: E402
from flowhip.config.args import default_ncup_args  # noqa: E402
from flowhip.models import build_model  # noqa: E402

dev = torch.device("cuda:0")
for flag in (False, True):
    torch.manual_seed(1234)
    args = default_ncup_args(model="raft_nc_dbl", mixed_precision=True,
                             alternate_corr=flag)
    model = build_model(args).to(dev).train()
    model.freeze_bn()
    h, w, b = 128, 256, 2
    i1 = torch.rand(b, 3, h, w, device=dev) * 255
    i2 = torch.rand(b, 3, h, w, device=dev) * 255
    gt = torch.randn(b, 2, h, w, device=dev)
    va = torch.ones(b, h, w, device=dev)

    def step():
        model.zero_grad(set_to_none=True)
        loss, _ = ops.sequence_loss(model(i1, i2, iters=12), gt, va, 0.85)
        loss.backward()
        return loss

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    n = 8
    for _ in range(n):
        loss = step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / n
    print(json.dumps({"probe": "train_step", "alternate_corr": flag,
                      "ms": dt * 1e3, "loss": loss.item(),
                      "max_mem_mb": torch.cuda.max_memory_allocated() / 2**20}),
          flush=True)
