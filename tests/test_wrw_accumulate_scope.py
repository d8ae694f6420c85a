"""wrw_accumulate_scope / WrwSinkFn off-GPU: the scope is a no-op on the
torch reference path, and the sink node's backward runs once, after all of
its consumers, also when every gradient that reaches it is None."""

import pytest
import torch

from flowhip.config.args import default_ncup_args
from flowhip.models import build_model
from flowhip.ops import functional_conv as fc


def _model_grads(monkeypatch, flag):
    monkeypatch.setenv("FLOWHIP_WRW_ACCUM", flag)
    torch.manual_seed(3)
    model = build_model(default_ncup_args(model="raft_nc_dbl"))
    model.train()
    g = torch.Generator().manual_seed(4)
    # 128x128, not the GPU test's 64x96: off-GPU the 1x1 correlation level
    # of a smaller input hits the reference sampler's 2x/(W-1) singularity
    # (see tests/test_models.py) and every value compared would be NaN
    im1 = torch.rand(1, 3, 128, 128, generator=g) * 255
    im2 = torch.rand(1, 3, 128, 128, generator=g) * 255
    preds = model(im1, im2, iters=3)
    sum(p.abs().mean() for p in preds).backward()
    return ([p.detach() for p in preds],
            {k: p.grad for k, p in model.named_parameters()
             if p.grad is not None})


def test_scope_is_a_noop_on_cpu(monkeypatch):
    preds_on, g_on = _model_grads(monkeypatch, "1")
    preds_off, g_off = _model_grads(monkeypatch, "0")
    for a, b in zip(preds_on, preds_off):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    assert g_on.keys() == g_off.keys() and g_on
    for k in g_off:
        assert torch.equal(g_on[k], g_off[k]), k


def test_scope_switch_and_nesting(monkeypatch):
    monkeypatch.setenv("FLOWHIP_WRW_ACCUM", "0")
    with fc.wrw_accumulate_scope():
        assert getattr(fc._tls, "handles", None) is None
    monkeypatch.setenv("FLOWHIP_WRW_ACCUM", "1")
    with fc.wrw_accumulate_scope():
        outer = fc._tls.handles
        with fc.wrw_accumulate_scope():
            assert fc._tls.handles is not outer
        assert fc._tls.handles is outer
    assert fc._tls.handles is None


class _DepositFn(torch.autograd.Function):
    """Stand-in for a conv call with a handle: the weight gradient goes to
    the handle, the weight input gets None."""

    @staticmethod
    def forward(ctx, x, w, handle):
        ctx.save_for_backward(x, w)
        ctx.handle = handle
        return x * w

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        h = ctx.handle
        h.calls += 1
        h.dw = dy * x if h.dw is None else h.dw + dy * x
        return dy * w, None, None


class _Handle(fc._WrwHandle):
    __slots__ = ("calls",)

    def __init__(self):
        super().__init__()
        self.calls = 0


def _sink_chain(w, h, extra_use):
    wh, bh = fc.WrwSinkFn.apply(h, w, None)
    assert bh is None
    x = torch.full((3,), 2.0, requires_grad=True)
    y = x
    for _ in range(4):
        y = _DepositFn.apply(y, wh, h)
    loss = y.sum()
    if extra_use:                       # a gradient by an ordinary route
        loss = loss + (wh * 5.0).sum()
    return loss


def test_sink_backward_runs_after_all_uses_with_none_grads():
    for extra_use in (False, True):
        w = torch.tensor([1.0, 2.0, 3.0], requires_grad=True)
        h = _Handle()
        _sink_chain(w, h, extra_use).backward()
        assert h.calls == 4 and h.dw is None    # taken by the sink
        w2 = w.detach().clone().requires_grad_(True)
        x = torch.full((3,), 2.0)
        y = x
        for _ in range(4):
            y = y * w2
        loss = y.sum() + ((w2 * 5.0).sum() if extra_use else 0.0)
        loss.backward()
        torch.testing.assert_close(w.grad, w2.grad)


def test_sink_second_backward_starts_clean():
    w = torch.tensor([1.0, 2.0, 3.0], requires_grad=True)
    h = _Handle()
    loss = _sink_chain(w, h, False)
    loss.backward(retain_graph=True)
    g1 = w.grad.clone()
    loss.backward()
    assert h.calls == 8 and h.dw is None
    assert torch.equal(w.grad, 2 * g1)


class _SinkModule(torch.nn.Module):
    """A weight used four times behind a sink, as a conv in the scope."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor([1.0, 2.0, 3.0]))
        self.other = torch.nn.Linear(3, 3)

    def forward(self, x):
        h = _Handle()
        wh, _ = fc.WrwSinkFn.apply(h, self.w, None)
        y = self.other(x)
        for _ in range(4):
            y = _DepositFn.apply(y, wh, h)
        return y


def test_sink_under_ddp_static_graph(tmp_path):
    """DDP as engine/distributed.py wraps it (one bucket, bucket views,
    static_graph) sees each parameter's gradient once per step, from the
    sink: three steps give the gradients of the unwrapped module."""
    import torch.distributed as dist
    if dist.is_initialized():
        pytest.skip("process group already active")
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg",
                            rank=0, world_size=1)
    try:
        torch.manual_seed(0)
        plain = _SinkModule()
        wrapped = _SinkModule()
        wrapped.load_state_dict(plain.state_dict())
        ddp = torch.nn.parallel.DistributedDataParallel(
            wrapped, bucket_cap_mb=64, gradient_as_bucket_view=True,
            static_graph=True)
        for step in range(3):
            x = torch.full((2, 3), 1.0 + step)
            for m in (plain, ddp):
                m.zero_grad(set_to_none=True)
                m(x).sum().backward()
            for a, b in zip(plain.parameters(), wrapped.parameters()):
                torch.testing.assert_close(b.grad, a.grad)
    finally:
        dist.destroy_process_group()
