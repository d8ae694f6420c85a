"""CPU: the forward-backward consistency twin against a naive per-pixel
loop and closed forms, the bidirectional model forward against two separate
calls, and the bidirectional warm start of FlowStream."""

import functools

import numpy as np
import pytest
import torch

from flowhip import ops
from flowhip.config.args import default_ncup_args
from flowhip.engine.stream import FlowStream
from flowhip.models import build_model
from flowhip.ops import torch_ref

from fb_cases import (FB_INPUTS, POISON_B, POISON_F, TRANSLATION, bits_equal,
                      fb_input, naive_direction)

SHAPES = [(1, 5, 7), (2, 17, 23)]


# ---- ops.fb_consistency: the twin ------------------------------------------

@pytest.mark.parametrize("name", FB_INPUTS)
@pytest.mark.parametrize("N,H,W", SHAPES)
def test_twin_matches_naive_loop(N, H, W, name):
    f, b = fb_input(name, N, H, W)
    occ_fw, occ_bw, res_fw, res_bw, stats = ops.fb_consistency(f, b)
    assert occ_fw.dtype == torch.uint8 and occ_fw.shape == (N, 1, H, W)
    assert res_fw.dtype == torch.float32 and res_fw.shape == (N, 1, H, W)
    assert stats.dtype == torch.float64 and stats.shape == (N, 2, 4)
    assert not res_fw.requires_grad
    fn, bn = f.double().numpy(), b.double().numpy()
    for n in range(N):
        for d, (occ, res, p, q) in enumerate([(occ_fw, res_fw, fn, bn),
                                              (occ_bw, res_bw, bn, fn)]):
            want_occ, want_res, want_stats = naive_direction(p[n], q[n])
            assert np.array_equal(occ[n, 0].numpy(), want_occ)
            assert stats[n, d, :3].tolist() == want_stats[:3]
            assert sum(want_stats[:3]) == H * W
            # res is the fp32 rounding of a value within 1e-12 of the loop's
            lo = (want_res * (1 - 1e-12)).astype(np.float32)
            hi = (want_res * (1 + 1e-12)).astype(np.float32)
            got = res[n, 0].numpy()
            assert np.all((got >= lo) & (got <= hi))
            assert abs(stats[n, d, 3].item() - want_stats[3]) \
                <= 1e-12 * abs(want_stats[3])


@pytest.mark.parametrize("N,H,W", SHAPES + [(1, 8, 8), (1, 55, 128)])
def test_translation_closed_form(N, H, W):
    f, b = fb_input("translation", N, H, W)
    occ_fw, occ_bw, res_fw, res_bw, stats = ops.fb_consistency(f, b)
    tx, ty = TRANSLATION
    x = torch.arange(W)[None, :].expand(H, W)
    y = torch.arange(H)[:, None].expand(H, W)
    vis_fw = (x + tx <= W - 1) & (y + ty >= 0)
    vis_bw = (x - tx >= 0) & (y - ty <= H - 1)
    for occ, res, vis, d in [(occ_fw, res_fw, vis_fw, 0),
                             (occ_bw, res_bw, vis_bw, 1)]:
        assert torch.equal(occ[:, 0] == 0, vis.expand(N, H, W))
        assert torch.equal(res[:, 0] == 0, vis.expand(N, H, W))
        assert torch.isinf(res[:, 0][~vis.expand(N, H, W)]).all()
        assert stats[:, d].tolist() == [
            [int(vis.sum()), 0, H * W - int(vis.sum()), 0.0]] * N


def _touched(f, poison, H, W):
    """Pixels of one (2,H,W) clean flow whose four-tap sample footprint
    contains a poisoned pixel of the other flow."""
    hit = torch.zeros(H, W, dtype=torch.bool)
    for y in range(H):
        for x in range(W):
            px, py = x + f[0, y, x].item(), y + f[1, y, x].item()
            if not (0 <= px <= W - 1 and 0 <= py <= H - 1):
                continue
            x0, y0 = min(int(px // 1), W - 2), min(int(py // 1), H - 2)
            hit[y, x] = any((qy - y0) in (0, 1) and (qx - x0) in (0, 1)
                            for qy, qx, _, _ in poison)
    return hit


@pytest.mark.parametrize("N,H,W", SHAPES)
def test_nonfinite_stays_local(N, H, W):
    clean = fb_input("smooth", N, H, W)
    dirty = fb_input("nonfinite", N, H, W)
    want = ops.fb_consistency(*clean)
    got = ops.fb_consistency(*dirty)
    # (own poison, other flow's poison, occ index, res index, clean own flow)
    for own, other, io, ir, flow in [(POISON_F, POISON_B, 0, 2, clean[0]),
                                     (POISON_B, POISON_F, 1, 3, clean[1])]:
        own_mask = torch.zeros(H, W, dtype=torch.bool)
        for y, x, _, _ in own:
            own_mask[y, x] = True
            # a poisoned pixel of the checked flow: occluded, res = +inf
            assert (got[io][:, 0, y, x] == 1).all()
            assert (got[ir][:, 0, y, x] == float("inf")).all()
        for n in range(N):
            allowed = own_mask | _touched(flow[n], other, H, W)
            assert allowed.any() and not allowed.all()
            same_occ = got[io][n, 0] == want[io][n, 0]
            same_res = got[ir][n, 0] == want[ir][n, 0]
            assert (same_occ & same_res)[~allowed].all()
            # a NaN or infinite tap of the sampled flow: non-finite sample
            bad = _touched(flow[n], [p for p in other
                                     if not np.isfinite(p[3])], H, W)
            bad &= ~own_mask
            assert (got[io][n, 0][bad] == 1).all()
            assert torch.isinf(got[ir][n, 0][bad]).all()
    assert not torch.isnan(got[2]).any() and not torch.isnan(got[3]).any()
    assert torch.isfinite(got[4]).all()


def test_twin_rejects_bad_shapes():
    with pytest.raises(ValueError):
        ops.fb_consistency(torch.zeros(1, 2, 1, 8), torch.zeros(1, 2, 1, 8))
    with pytest.raises(ValueError):
        ops.fb_consistency(torch.zeros(1, 2, 4, 8), torch.zeros(1, 2, 4, 9))
    with pytest.raises(ValueError):
        ops.fb_consistency(torch.zeros(2, 4, 8), torch.zeros(2, 4, 8))


def test_margin_of_the_shared_inputs():
    """The inputs keep every decision clear of its threshold, so the GPU
    comparison of `occ` cannot hinge on fp64 rounding."""
    for name in FB_INPUTS:
        for N, H, W in SHAPES + [(1, 55, 128)]:
            margin = torch_ref.fb_consistency(
                *fb_input(name, N, H, W), return_margin=True)[5].item()
            print(f"{name} {(N, H, W)}: min |r2 - thr| = {margin:.3g}")
            assert margin >= 1e-9


# ---- models ----------------------------------------------------------------

MODELS = [("raft_nc_dbl", False), ("raft", False), ("raft", True)]


@functools.lru_cache(maxsize=None)
def _model(name, small, alternate_corr):
    torch.manual_seed(1234)
    args = default_ncup_args(model=name, small=small, mixed_precision=False,
                             alternate_corr=alternate_corr)
    return build_model(args).eval()


@functools.lru_cache(maxsize=None)
def _frames():
    g = torch.Generator().manual_seed(5)
    return (torch.rand(1, 3, 128, 128, generator=g) * 255,
            torch.rand(1, 3, 128, 128, generator=g) * 255)


@pytest.mark.parametrize("alternate_corr", [False, True])
@pytest.mark.parametrize("name,small", MODELS)
def test_bidirectional_equals_two_calls(name, small, alternate_corr):
    model = _model(name, small, alternate_corr)
    a, b = _frames()
    seen = []
    hook = model.fnet.register_forward_hook(
        lambda mod, inp, out: seen.append(
            sum(t.shape[0] for t in inp[0]) if isinstance(inp[0], (list, tuple))
            else inp[0].shape[0]))
    try:
        with torch.no_grad():
            low, up = model(a, b, iters=3, test_mode=True, bidirectional=True)
    finally:
        hook.remove()
    assert seen == [2]              # fnet: one call, 2N images, not 4N
    assert low.shape == (2, 2, 16, 16) and up.shape == (2, 2, 128, 128)
    with torch.no_grad():
        low_fw, up_fw = model(a, b, iters=3, test_mode=True)
        low_bw, up_bw = model(b, a, iters=3, test_mode=True)
    d_low = (low - torch.cat([low_fw, low_bw])).abs().max().item()
    d_up = (up - torch.cat([up_fw, up_bw])).abs().max().item()
    print(f"{name} small={small} alt={alternate_corr}: max|diff| low "
          f"{d_low:.3g} up {d_up:.3g}")
    assert d_low <= 1e-4 and d_up <= 1e-4
    assert not bits_equal(up_fw, up_bw)

    # a 2N flow_init equals the separate calls run with its halves
    g = torch.Generator().manual_seed(11)
    init = torch.randn(2, 2, 16, 16, generator=g)
    with torch.no_grad():
        low, up = model(a, b, iters=3, flow_init=init, test_mode=True,
                        bidirectional=True)
        low_fw, up_fw = model(a, b, iters=3, flow_init=init[:1],
                              test_mode=True)
        low_bw, up_bw = model(b, a, iters=3, flow_init=init[1:],
                              test_mode=True)
    d_low = (low - torch.cat([low_fw, low_bw])).abs().max().item()
    d_up = (up - torch.cat([up_fw, up_bw])).abs().max().item()
    print(f"  with flow_init: max|diff| low {d_low:.3g} up {d_up:.3g}")
    assert d_low <= 1e-4 and d_up <= 1e-4


@pytest.mark.parametrize("name,small", MODELS)
def test_bidirectional_argument_contract(name, small):
    model = _model(name, small, False)
    a, b = _frames()
    with pytest.raises(ValueError):
        model(a, b, iters=1, bidirectional=True)
    with torch.no_grad():
        want = model(a, b, iters=2, test_mode=True)
        got = model(a, b, iters=2, test_mode=True, bidirectional=False)
    assert bits_equal(got[0], want[0]) and bits_equal(got[1], want[1])


# ---- FlowStream -------------------------------------------------------------

class _Recorder(torch.nn.Module):
    """Wraps a model and keeps every `flow_init` it is called with."""

    def __init__(self, model):
        super().__init__()
        self.model = model
        self.inits = []

    def forward(self, *args, **kwargs):
        self.inits.append(kwargs.get("flow_init"))
        return self.model(*args, **kwargs)


def test_stream_bidirectional_warm_start():
    model = _Recorder(_model("raft_nc_dbl", False, False))
    g = torch.Generator().manual_seed(9)
    # 128x136: the CPU lookup needs >= 128 px for a finite flow (PARITY.md 7)
    frames = [torch.rand(1, 3, 128, 136, generator=g) * 255 for _ in range(3)]
    stream = FlowStream(model, iters=2, bidirectional=True)
    low0, up0 = stream.step(frames[0], frames[1])
    assert low0.shape == (2, 2, 16, 17) and up0.shape == (2, 2, 128, 136)
    assert torch.isfinite(up0).all()
    assert model.inits == [None]

    low1, up1 = stream.step(frames[1], frames[2])
    init = model.inits[1]
    fw = ops.forward_splat(low0[:1])
    assert init.shape == (2, 2, 16, 17)
    assert bits_equal(init[:1], fw)
    assert bits_equal(init[1:], -ops.forward_splat(fw))
    with torch.no_grad():
        cold1 = model.model(frames[1], frames[2], iters=2, test_mode=True,
                            bidirectional=True)
    assert not bits_equal(low1, cold1[0])     # the warm start is live

    stream.reset()
    low, up = stream.step(frames[1], frames[2])
    assert model.inits[-1] is None
    assert bits_equal(low, cold1[0]) and bits_equal(up, cold1[1])

    # one direction: unchanged
    plain = FlowStream(model, iters=2)
    low = plain.step(frames[0], frames[1])[0]
    plain.step(frames[1], frames[2])
    assert low.shape == (1, 2, 16, 17)
    assert bits_equal(model.inits[-1], ops.forward_splat(low))


# ---- demo.py ---------------------------------------------------------------

def test_demo_occlusion_png(tmp_path):
    from PIL import Image

    import demo

    f, b = fb_input("translation", 1, 17, 23)
    line = demo.write_occlusion(f, b, str(tmp_path / "occ_0000.png"))
    png = np.array(Image.open(tmp_path / "occ_0000.png"))
    assert png.dtype == np.uint8 and png.shape == (17, 23)
    occ = ops.fb_consistency(f, b)[0][0, 0].numpy()
    assert np.array_equal(png, occ * 255) and set(np.unique(png)) == {0, 255}
    vis = 100 * (1 - occ.mean())
    assert line.startswith("occ_0000.png: visible %.1f%% fw" % vis)
    assert "mean visible residual 0.000 px fw" in line
    args = demo.build_parser().parse_args(["--bidirectional"])
    assert args.bidirectional
    assert not demo.build_parser().parse_args([]).bidirectional
