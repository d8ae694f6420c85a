"""Forward splat (warm start) on the CPU: the float64 oracle against scipy,
its defined tie / no-source behaviour, FlowStream, and the device-splat route
of the Sintel submission writer."""

import pytest
import torch

from flowhip import ops
from flowhip.config.args import default_ncup_args
from flowhip.models import build_model
from flowhip.ops import torch_ref
from flowhip.utils.geometry import forward_interpolate

from splat_cases import RANDOM_FIELDS, bits_equal, random_flow, tie_field


def _scipy_splat(flow):
    pytest.importorskip("scipy")
    return forward_interpolate(flow)


@pytest.mark.parametrize("H,W,sigma", RANDOM_FIELDS)
def test_oracle_matches_scipy_outside_ties(H, W, sigma):
    flow = random_flow(1, H, W, sigma)[0]
    ref = _scipy_splat(flow)
    out, ties = torch_ref.forward_splat(flow, return_ties=True)
    assert out.shape == (2, H, W) and ties.shape == (H, W)
    n_ties = int(ties.sum())
    mism = (out.view(torch.int32) != ref.view(torch.int32)).any(0) & ~ties
    print(f"{H}x{W} sigma={sigma}: ties={n_ties} mismatches={int(mism.sum())}")
    assert n_ties <= 0.01 * H * W
    assert not mism.any()


def test_tie_field_lowest_index_wins():
    H, W = 9, 11
    flow = tie_field(1, H, W)[0]
    out, ties = torch_ref.forward_splat(flow, return_ties=True)
    print("tie targets:", int(ties.sum()))
    assert ties.all()  # every target sees its two nearest sources tie

    # brute force by hand: ascending sources, strict `<` keeps the lowest
    px = (torch.arange(W, dtype=torch.float64)[None] + flow[0].double())
    py = (torch.arange(H, dtype=torch.float64)[:, None] + flow[1].double())
    px, py = px.reshape(-1).tolist(), py.reshape(-1).tolist()
    fx, fy = flow[0].reshape(-1).tolist(), flow[1].reshape(-1).tolist()
    for ty in range(H):
        for tx in range(W):
            best, bi = float("inf"), -1
            for i in range(H * W):
                if not (0 < px[i] < W and 0 < py[i] < H):
                    continue
                d = (px[i] - tx) ** 2 + (py[i] - ty) ** 2
                if d < best:
                    best, bi = d, i
            assert out[0, ty, tx].item() == fx[bi], (ty, tx)
            assert out[1, ty, tx].item() == fy[bi], (ty, tx)

    ref = _scipy_splat(flow)
    mism = (out.view(torch.int32) != ref.view(torch.int32)).any(0) & ~ties
    assert not mism.any()


def test_tie_field_scipy_agrees_on_untied_targets():
    """A field with both tied and untied targets: scipy must agree wherever
    the minimum is unique."""
    H, W = 9, 11
    flow = tie_field(1, H, W)[0]
    flow[:, 4:] += random_flow(1, H, W, 0.3)[0][:, 4:]
    out, ties = torch_ref.forward_splat(flow, return_ties=True)
    assert ties.any() and not ties.all()
    ref = _scipy_splat(flow)
    mism = (out.view(torch.int32) != ref.view(torch.int32)).any(0) & ~ties
    assert not mism.any()


def test_all_invalid_sample_gives_zeros():
    flow = torch.full((1, 2, 6, 9), 1e6)
    out, ties = torch_ref.forward_splat(flow, return_ties=True)
    assert torch.equal(out, torch.zeros_like(flow))
    assert not ties.any()
    assert torch.equal(ops.forward_splat(flow), torch.zeros_like(flow))


def test_nan_entry_is_ignored():
    flow = random_flow(1, 7, 9, 1.0)
    poisoned = flow.clone()
    poisoned[0, 0, 3, 4] = float("nan")
    poisoned[0, 1, 5, 2] = float("nan")
    out = ops.forward_splat(poisoned)
    assert torch.isfinite(out).all()
    # same as the field with those two sources pushed out of the frame
    removed = flow.clone()
    removed[0, :, 3, 4] = 1e6
    removed[0, :, 5, 2] = 1e6
    assert bits_equal(out, ops.forward_splat(removed))


def test_batch_equals_per_sample():
    flow = random_flow(2, 17, 23, 3.0)
    flow[1] = tie_field(1, 17, 23)[0]
    out, ties = torch_ref.forward_splat(flow, return_ties=True)
    for b in range(2):
        o, t = torch_ref.forward_splat(flow[b:b + 1], return_ties=True)
        assert bits_equal(out[b:b + 1], o)
        assert torch.equal(ties[b:b + 1], t)


def test_3d_input_returns_3d():
    flow = random_flow(1, 5, 7, 1.5)
    out3 = ops.forward_splat(flow[0])
    assert out3.shape == (2, 5, 7)
    assert bits_equal(out3, ops.forward_splat(flow)[0])
    out3, ties = torch_ref.forward_splat(flow[0], return_ties=True)
    assert out3.shape == (2, 5, 7) and ties.shape == (5, 7)


def test_output_is_not_differentiable():
    flow = random_flow(1, 5, 7, 1.5).requires_grad_()
    out = ops.forward_splat(flow)
    assert not out.requires_grad


# ---- FlowStream ----------------------------------------------------------

def _small_model():
    torch.manual_seed(0)
    return build_model(default_ncup_args(model="raft_nc_dbl",
                                         small=True)).eval()


def _frames(n, h, w):
    g = torch.Generator().manual_seed(11)
    return [torch.rand(1, 3, h, w, generator=g) * 255 for _ in range(n)]


# 64x96 is below the CPU lookup's 128-px floor (PARITY.md 7: its 1-px pyramid
# level makes the flow NaN there), so that size checks the plumbing bit for
# bit and 128x136 checks it on finite flow.
@pytest.mark.parametrize("h,w", [(64, 96), (128, 136)])
def test_flow_stream_equals_hand_written_loop(h, w):
    from flowhip.engine.stream import FlowStream

    model = _small_model()
    frames = _frames(4, h, w)

    hand, init = [], None
    with torch.no_grad():
        for im1, im2 in zip(frames[:-1], frames[1:]):
            low, up = model(im1, im2, iters=2, flow_init=init, test_mode=True)
            init = ops.forward_splat(low)
            hand.append((low, up))

    stream = FlowStream(model, iters=2)
    got = [stream.step(im1, im2)
           for im1, im2 in zip(frames[:-1], frames[1:])]
    assert len(got) == 3
    for (low, up), (hlow, hup) in zip(got, hand):
        assert bits_equal(low, hlow) and bits_equal(up, hup)

    # reset(): the next step is a cold start
    stream.reset()
    low, up = stream.step(frames[1], frames[2])
    with torch.no_grad():
        clow, cup = model(frames[1], frames[2], iters=2, test_mode=True)
    assert bits_equal(low, clow) and bits_equal(up, cup)

    if (h, w) == (128, 136):
        assert all(torch.isfinite(low).all() and torch.isfinite(up).all()
                   for low, up in got)
        # the warm start is live: frame 2 differs from its cold start
        assert not bits_equal(got[1][0], clow)

    cold = FlowStream(model, iters=2, warm_start=False)
    cold.step(frames[0], frames[1])
    low, up = cold.step(frames[1], frames[2])
    assert bits_equal(low, clow) and bits_equal(up, cup)


def test_flow_stream_graphed_needs_gpu_and_shape():
    from flowhip.engine.stream import FlowStream

    model = _small_model()
    with pytest.raises(AssertionError):
        FlowStream(model, iters=2, graphed=True)
    if not torch.cuda.is_available():
        with pytest.raises(AssertionError):
            FlowStream(model, iters=2, graphed=True,
                       input_shape=(1, 3, 128, 136))


def test_sintel_submission_device_splat(tmp_path, monkeypatch):
    """The synthetic submission route of tests/test_engine.py with
    splat="device": same files as a hand-written device-splat sequence, and
    no call into the scipy path."""
    import numpy as np
    from PIL import Image

    from flowhip.data import frame_utils
    from flowhip.engine import evaluate as ev

    rng = np.random.RandomState(5)
    for dstype in ("clean", "final"):
        scene = tmp_path / "datasets" / "Sintel" / "test" / dstype / "seq_1"
        scene.mkdir(parents=True)
        for i in range(3):
            arr = (rng.rand(128, 136, 3) * 255).astype(np.uint8)
            Image.fromarray(arr).save(scene / f"frame_{i:04d}.png")

    monkeypatch.chdir(tmp_path)

    def no_scipy(flow):
        raise AssertionError("splat='device' must not take the scipy path")
    monkeypatch.setattr(ev, "forward_interpolate", no_scipy)

    model = _small_model()
    ev.create_sintel_submission(model, iters=2, warm_start=True,
                                output_path=str(tmp_path / "out"),
                                splat="device")

    seq = tmp_path / "datasets" / "Sintel" / "test" / "clean" / "seq_1"
    imgs = [torch.from_numpy(np.array(Image.open(seq / f"frame_{i:04d}.png")))
            .permute(2, 0, 1).float()[None] for i in range(3)]
    init = None
    for i in range(2):
        with torch.no_grad():
            low, up = model(imgs[i], imgs[i + 1], iters=2, flow_init=init,
                            test_mode=True)
        init = ops.forward_splat(low)
        flo = frame_utils.readFlow(
            str(tmp_path / "out" / "clean" / "seq_1" / f"frame{i + 1:04d}.flo"))
        assert flo.shape == (128, 136, 2)
        assert np.array_equal(flo, up[0].permute(1, 2, 0).numpy())
    assert (tmp_path / "out" / "final" / "seq_1" / "frame0002.flo").exists()

    with pytest.raises(AssertionError):
        ev.create_sintel_submission(model, iters=2, warm_start=True,
                                    output_path=str(tmp_path / "out2"),
                                    splat="host")
