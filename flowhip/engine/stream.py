"""Streaming sequence inference with a device-side warm start.

Each frame pair starts from the previous pair's low-res flow, forward-warped
onto the grid by `ops.forward_splat` (the reference's Sintel submission
writer does this through scipy on the host — evaluate.py:23-57). The splat
stays on the model's device: no host round trip, and with `graphed=True` it
is part of the replayed hipGraph.
"""

import torch

from .. import ops


def warm_init(flow_low, bidirectional=False):
    """The next frame pair's `flow_init` from this pair's low-res flow.

    One direction: g = forward_splat(flow_low). Bidirectional (`flow_low` is
    the 2N batch, 1->2 first): the forward half is the same g, from the
    forward flow; the backward half is -forward_splat(g), the constant-
    velocity prediction — the point that lands on x + g(x) in the next frame
    came from x."""
    if not bidirectional:
        return ops.forward_splat(flow_low)
    g = ops.forward_splat(flow_low[:flow_low.shape[0] // 2])
    return torch.cat([g, -ops.forward_splat(g)], dim=0)


class FlowStream:
    """Warm-started test_mode inference over a frame sequence.

    Usage:
        stream = FlowStream(model, iters=32)
        for image1, image2 in pairs:
            flow_low, flow_up = stream.step(image1, image2)
        stream.reset()          # next sequence starts cold

    warm_start=False runs every pair cold. graphed=True replays a
    GraphedInference captured for `input_shape` (GPU only; outputs are then
    views of static buffers — clone them to retain across steps). On the CPU
    the splat runs through the float64 oracle.

    bidirectional=True estimates both directions of every pair: `step`
    returns the 2N-batch (flow_low, flow_up), 1->2 first, and the warm start
    carries an init for each half (`warm_init`).
    """

    def __init__(self, model, iters, warm_start=True, graphed=False,
                 input_shape=None, bidirectional=False):
        self.model = model.eval()
        self.iters = iters
        self.warm_start = warm_start
        self.bidirectional = bidirectional
        self.graph = None
        if graphed:
            assert input_shape is not None, \
                "FlowStream(graphed=True) needs the fixed input_shape"
            from .graph import GraphedInference
            self.graph = GraphedInference(model, input_shape, iters,
                                          warm_start=warm_start,
                                          bidirectional=bidirectional)
        self._init = None

    def reset(self):
        """Forget the previous frame: the next step is a cold start."""
        self._init = None

    @torch.no_grad()
    def step(self, image1, image2):
        if self.graph is not None:
            out = self.graph(image1, image2, self._init)
            if self.warm_start:
                self._init = self.graph.next_init
            return out
        if self.bidirectional:
            flow_low, flow_up = self.model(
                image1, image2, iters=self.iters, flow_init=self._init,
                test_mode=True, bidirectional=True)
        else:
            flow_low, flow_up = self.model(
                image1, image2, iters=self.iters, flow_init=self._init,
                test_mode=True)
        if self.warm_start:
            self._init = warm_init(flow_low, self.bidirectional)
        return flow_low, flow_up
