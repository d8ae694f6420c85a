"""hipGraph-captured inference (BASELINE config 4).

Captures the fixed-shape iterative-refinement forward into one hipGraph
(torch.cuda.CUDAGraph is hipGraph on ROCm) and replays it per frame pair —
removing the per-iteration launch overhead of the 24-32 GRU iterations.

Capture-safety of the model forward is by construction: the corr-lookup
window offsets are device-resident compile-time constants (no host->device
delta transfer — SURVEY.md §2.9 quirk 8), coords grids are created on
device, and no host syncs occur in the loop.
"""

import torch

from .. import ops
from .stream import warm_init


class GraphedInference:
    """Wrap a model for fixed-shape graph-replayed test_mode inference.

    Usage:
        g = GraphedInference(model, (1, 3, 288, 960), iters=24)
        flow_low, flow_up = g(image1, image2)
    Inputs must match the capture shape; outputs are views of static buffers
    (clone them to retain across calls).

    warm_start=True captures the sequence form instead: the forward takes a
    static `flow_init` buffer (zeros = cold start; `coords + 0` is exact),
    and the same graph splats the resulting low-res flow into the static
    `next_init` (ops.forward_splat), ready to be the next frame's init:
        g = GraphedInference(model, shape, iters=32, warm_start=True)
        flow_low, flow_up = g(image1, image2)                # cold
        flow_low, flow_up = g(image2, image3, g.next_init)   # warm

    bidirectional=True captures the bidirectional forward: the outputs (and
    `flow_init` / `next_init`) have batch 2N, the 1->2 flow first. With
    consistency=True the same graph also runs `ops.fb_consistency` on the two
    halves of `flow_up`; its five results are the static buffers
    `self.consistency` (occ_fw, occ_bw, res_fw, res_bw, stats), valid after
    each call like the outputs. The check covers the captured shape: callers
    with padded frames unpad the flows and call the op themselves.
    """

    def __init__(self, model, input_shape, iters, warmup=3, warm_start=False,
                 bidirectional=False, consistency=False):
        assert torch.cuda.is_available(), "hipGraph capture requires a GPU"
        if consistency and not bidirectional:
            raise ValueError("consistency=True needs bidirectional=True")
        self.model = model.eval()
        self.iters = iters
        self.warm_start = warm_start
        self.bidirectional = bidirectional
        self.check = consistency
        self.consistency = None
        device = next(model.parameters()).device

        self.static_img1 = torch.zeros(input_shape, device=device)
        self.static_img2 = torch.zeros(input_shape, device=device)
        self.static_init = None
        self.next_init = None
        if warm_start:
            b, _, h, w = input_shape
            if bidirectional:
                b = 2 * b
            self.static_init = torch.zeros((b, 2, h // 8, w // 8),
                                           device=device)

        # warm up on a side stream (allocator + MIOpen autotune settle)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s), torch.no_grad():
            for _ in range(warmup):
                self._forward()
        torch.cuda.current_stream().wait_stream(s)

        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph), torch.no_grad():
            self.static_out = self._forward()

    def _forward(self):
        if self.bidirectional:
            return self._forward_bidirectional()
        out = self.model(self.static_img1, self.static_img2, iters=self.iters,
                         flow_init=self.static_init, test_mode=True)
        if self.warm_start:
            self.next_init = ops.forward_splat(out[0])
        return out

    def _forward_bidirectional(self):
        out = self.model(self.static_img1, self.static_img2, iters=self.iters,
                         flow_init=self.static_init, test_mode=True,
                         bidirectional=True)
        if self.warm_start:
            self.next_init = warm_init(out[0], bidirectional=True)
        if self.check:
            n = self.static_img1.shape[0]
            self.consistency = ops.fb_consistency(out[1][:n], out[1][n:])
        return out

    @torch.no_grad()
    def __call__(self, image1, image2, flow_init=None):
        self.static_img1.copy_(image1)
        self.static_img2.copy_(image2)
        if self.warm_start:
            # next_init is an output of the same graph: the copy below is
            # ordered before the replay that overwrites it
            if flow_init is None:
                self.static_init.zero_()
            else:
                self.static_init.copy_(flow_init)
        else:
            assert flow_init is None, \
                "flow_init needs GraphedInference(warm_start=True)"
        self.graph.replay()
        return self.static_out
