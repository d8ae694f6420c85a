"""Streaming sequence inference with a device-side warm start.

Each frame pair starts from the previous pair's low-res flow, forward-warped
onto the grid by `ops.forward_splat` (the reference's Sintel submission
writer does this through scipy on the host — evaluate.py:23-57). The splat
stays on the model's device: no host round trip, and with `graphed=True` it
is part of the replayed hipGraph.
"""

import torch

from .. import ops


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
    """

    def __init__(self, model, iters, warm_start=True, graphed=False,
                 input_shape=None):
        self.model = model.eval()
        self.iters = iters
        self.warm_start = warm_start
        self.graph = None
        if graphed:
            assert input_shape is not None, \
                "FlowStream(graphed=True) needs the fixed input_shape"
            from .graph import GraphedInference
            self.graph = GraphedInference(model, input_shape, iters,
                                          warm_start=warm_start)
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
        flow_low, flow_up = self.model(image1, image2, iters=self.iters,
                                       flow_init=self._init, test_mode=True)
        if self.warm_start:
            self._init = ops.forward_splat(flow_low)
        return flow_low, flow_up
