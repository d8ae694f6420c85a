"""GPU tests (MI355X) for the on-demand correlation lookup
(`--alternate_corr`): the alt_corr HIP kernel against the fp32 all-pairs
volume formulation computed on the CPU, its autograd wrapper, the memory
bound, and the flag's path through the model and the hipGraph engine.

Feature maps stay >= 16 cells per side so every pyramid level is >= 2 px
(the torch sampler is singular at 1 px)."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(2, 256, 16, 24, 4), (2, 128, 17, 27, 3)]


def _dev():
    return torch.device("cuda:0")


@pytest.fixture
def fp32_corr():
    from flowhip.utils import layout
    old = layout.corr_bf16_enabled()
    layout.set_corr_bf16(False)
    yield
    layout.set_corr_bf16(old)


@pytest.fixture(params=[False, True], ids=["nchw", "nhwc"])
def channels_last(request):
    from flowhip.utils import layout
    old = layout.channels_last_enabled()
    layout.set_channels_last(request.param)
    yield request.param
    layout.set_channels_last(old)


def _volume_lookup(f1, f2, coords, r):
    """The oracle: lookup on the pyramid of the all-pairs volume (CPU fp32)."""
    from flowhip.ops import torch_ref
    pyr = torch_ref.corr_pyramid(torch_ref.corr_volume(f1, f2), 4)
    return torch_ref.corr_lookup(pyr, coords, r)


@functools.lru_cache(maxsize=None)
def _exact_case(B, D, H, W, r):
    """Integer features in {-1,0,1} and coordinates on the 1/8 grid over the
    map extended by ~6 px: pooled levels are exact in bf16 and the dot
    products exact in fp32, so indexing errors have no tolerance to hide
    behind. Returns CPU tensors (f1, f2, coords, ref); never modified."""
    g = torch.Generator().manual_seed(1000 + D + r)
    f1 = torch.randint(-1, 2, (B, D, H, W), generator=g).float()
    f2 = torch.randint(-1, 2, (B, D, H, W), generator=g).float()
    u = torch.rand(B, 2, H, W, generator=g)
    ext = torch.tensor([W + 12.0, H + 12.0]).view(1, 2, 1, 1)
    coords = torch.round((u * ext - 6.0) * 8) / 8
    coords[:, 0].clamp_(-6, W + 5)
    coords[:, 1].clamp_(-6, H + 5)
    return f1, f2, coords, _volume_lookup(f1, f2, coords, r)


@functools.lru_cache(maxsize=None)
def _random_case(B, D, H, W, r):
    g = torch.Generator().manual_seed(2000 + D + r)
    f1 = torch.randn(B, D, H, W, generator=g)
    f2 = torch.randn(B, D, H, W, generator=g)
    u = torch.rand(B, 2, H, W, generator=g)
    ext = torch.tensor([W + 12.0, H + 12.0]).view(1, 2, 1, 1)
    coords = u * ext - 6.0
    return f1, f2, coords, _volume_lookup(f1, f2, coords, r)


def _gpu_lookup(f1, f2, coords, r):
    from flowhip import ops
    from flowhip.ops.functional import AltOperandLevels
    levels = ops.alt_corr_pyramid(f2.to(_dev()), 4)
    assert isinstance(levels, AltOperandLevels)  # the HIP operand form
    return ops.alt_corr_lookup(f1.to(_dev()), levels, coords.to(_dev()), r)


def _padded_rows(out):
    """(B, H, W, C8) view of an NHWC lookup output's whole allocation."""
    B, C, H, W = out.shape
    c8 = (C + 7) // 8 * 8
    assert out.stride() == (H * W * c8, 1, W * c8, c8)
    return torch.as_strided(out, (B, H, W, c8), (H * W * c8, W * c8, c8, 1))


@pytest.mark.parametrize("B,D,H,W,r", SHAPES)
def test_exact_arithmetic(B, D, H, W, r, channels_last, fp32_corr):
    f1, f2, coords, ref = _exact_case(B, D, H, W, r)
    K2 = (2 * r + 1) ** 2
    for l in range(4):
        frac = (ref[:, l * K2:(l + 1) * K2] != 0).float().mean().item()
        assert frac >= 0.10, (l, frac)

    out = _gpu_lookup(f1, f2, coords, r)
    assert out.dtype == torch.float32 and out.shape == ref.shape
    if channels_last:
        rows = _padded_rows(out)
        assert rows.shape[-1] > 4 * K2          # both radii leave a pad tail
        assert (rows[..., 4 * K2:] == 0).all()
    else:
        assert out.is_contiguous()
    diff = (out.cpu() - ref).abs().max().item()
    print(f"exact D={D} r={r} nhwc={channels_last}: max|diff|={diff:.3g}")
    torch.testing.assert_close(out.cpu(), ref, atol=1e-5, rtol=0)


def test_asymmetric_probe(channels_last, fp32_corr):
    """One-hot f1 pixel, one-hot f2 position off the diagonal, one lookup
    centre: exactly one output channel is nonzero — an x/y or a/c swap
    moves it. f2's hot cell sits in the odd last row, which floor-mode
    pooling drops, so levels 1..3 stay zero."""
    B, D, H, W, r = 1, 128, 17, 27, 4
    K = 2 * r + 1
    py, px = 5, 9
    qy, qx = 16, 20
    da, dc = 3, -2                       # window offsets in x and in y
    f1 = torch.zeros(B, D, H, W)
    f2 = torch.zeros(B, D, H, W)
    f1[0, 7, py, px] = 1.0
    f2[0, 7, qy, qx] = 1.0
    from flowhip.utils.geometry import coords_grid
    coords = coords_grid(B, H, W)
    coords[0, :, py, px] = torch.tensor([qx - da, qy - dc], dtype=torch.float)

    out = _gpu_lookup(f1, f2, coords, r).cpu()
    want = torch.zeros(B, 4 * K * K, H, W)
    want[0, (da + r) * K + (dc + r), py, px] = 1.0 / (D ** 0.5)
    ref = _volume_lookup(f1, f2, coords, r)
    torch.testing.assert_close(ref, want, atol=1e-6, rtol=0)  # oracle agrees
    torch.testing.assert_close(out, want, atol=1e-6, rtol=0)
    assert out.nonzero().tolist() == [[0, (da + r) * K + (dc + r), py, px]]


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32res", "bf16res"])
@pytest.mark.parametrize("B,D,H,W,r", SHAPES)
def test_random_features_both_residency_modes(B, D, H, W, r, bf16):
    from flowhip.utils import layout
    f1, f2, coords, ref = _random_case(B, D, H, W, r)
    old = layout.corr_bf16_enabled()
    layout.set_corr_bf16(bf16)
    try:
        out = _gpu_lookup(f1, f2, coords, r)
    finally:
        layout.set_corr_bf16(old)
    assert out.dtype == (torch.bfloat16 if bf16 else torch.float32)
    diff = (out.float().cpu() - ref).abs().max().item()
    print(f"random D={D} r={r} bf16={bf16}: max|diff|={diff:.3g}")
    torch.testing.assert_close(out.float().cpu(), ref, atol=3e-2, rtol=3e-2)


def test_out_of_range_and_nan_coords(fp32_corr):
    B, D, H, W, r = SHAPES[0]
    f1, f2, coords, ref = _exact_case(B, D, H, W, r)
    far = [((0, 3, 5), (1e6, -1e6)), ((1, 8, 0), (-1e6, 1e6)),
           ((1, 15, 23), (1e6, 7.0))]
    nan = [((0, 9, 9), (float("nan"), 3.0)),
           ((1, 2, 17), (4.0, float("nan")))]
    coords = coords.clone()
    for (b, y, x), v in far + nan:
        coords[b, :, y, x] = torch.tensor(v)
    out = _gpu_lookup(f1, f2, coords, r)
    torch.cuda.synchronize()                 # the run ends clean
    out = out.cpu()
    keep = torch.ones(B, 1, H, W, dtype=torch.bool)
    for (b, y, x), _ in far:
        # the reference is zero there (checked once on the CPU oracle)
        assert (out[b, :, y, x] == 0).all()
        keep[b, 0, y, x] = False
    for (b, y, x), _ in nan:
        o = out[b, :, y, x]
        assert ((o == 0) | o.isnan()).all()
        keep[b, 0, y, x] = False
    far_only = _exact_case(B, D, H, W, r)[2].clone()
    for (b, y, x), v in far:
        far_only[b, :, y, x] = torch.tensor(v)
    ref_far = _volume_lookup(f1, f2, far_only, r)
    for (b, y, x), _ in far:
        assert (ref_far[b, :, y, x] == 0).all()
    # every other pixel is untouched by its neighbours' wild coordinates
    torch.testing.assert_close(torch.where(keep, out, ref), ref,
                               atol=1e-5, rtol=0)


def test_autograd_matches_chunked_oracle():
    from flowhip import ops
    from flowhip.ops import torch_ref
    B, D, H, W, r = 1, 128, 16, 24, 4
    f1, f2, coords, _ = _random_case(B, D, H, W, r)
    f1g = f1.to(_dev()).requires_grad_(True)
    f2g = f2.to(_dev()).requires_grad_(True)
    out = ops.alt_corr_lookup(f1g, ops.alt_corr_pyramid(f2g, 4),
                              coords.to(_dev()), r, fmap2=f2g)
    g = torch.randn(out.shape, generator=torch.Generator().manual_seed(9))
    d1, d2 = torch.autograd.grad(out, (f1g, f2g), g.to(_dev()).to(out.dtype))

    f1r = f1.clone().requires_grad_(True)
    f2r = f2.clone().requires_grad_(True)
    ref = torch_ref.alt_corr_lookup(
        f1r, torch_ref.alt_corr_pyramid(f2r, 4), coords, r, chunk=100)
    gr = g.to(out.dtype).float()            # the same rounded cotangent
    r1, r2 = torch.autograd.grad(ref, (f1r, f2r), gr)
    assert d1.shape == r1.shape and d2.shape == r2.shape
    for d, rr, n in ((d1, r1, "f1"), (d2, r2, "f2")):
        print(f"grad {n}: max|diff|={(d.cpu() - rr).abs().max().item():.3g}"
              f" max|ref|={rr.abs().max().item():.3g}")
        torch.testing.assert_close(d.cpu(), rr, atol=5e-2, rtol=5e-2)


def test_coords_must_be_detached():
    from flowhip import ops
    f1 = torch.randn(1, 128, 16, 24, device=_dev())
    f2 = torch.randn(1, 128, 16, 24, device=_dev())
    coords = torch.rand(1, 2, 16, 24, device=_dev(), requires_grad=True)
    with pytest.raises(AssertionError):
        ops.alt_corr_lookup(f1, ops.alt_corr_pyramid(f2, 4), coords, 4)


def test_memory_stays_below_a_quarter_of_the_volume():
    from flowhip.nn import AlternateCorrBlock
    B, D, H, W = 1, 256, 96, 160
    P = H * W
    torch.manual_seed(3)
    f1 = torch.randn(B, D, H, W, device=_dev())
    f2 = torch.randn(B, D, H, W, device=_dev())
    coords = torch.rand(B, 2, H, W, device=_dev()) * 90
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    with torch.no_grad():
        out = AlternateCorrBlock(f1, f2, num_levels=4, radius=4)(coords)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    print(f"on-demand lookup at P={P}: peak growth {grown / 1e6:.1f} MB")
    assert out.shape == (B, 4 * 81, H, W)
    assert torch.isfinite(out.float()).all()
    assert grown < P * P * 2 // 4, grown


def _ncup_model(**kw):
    from flowhip.config.args import default_ncup_args
    from flowhip.models import build_model
    args = default_ncup_args(model="raft_nc_dbl", mixed_precision=True, **kw)
    return build_model(args).to(_dev())


def test_model_deviation_from_volume_path_bounded():
    """raft_nc_dbl, mixed precision, 128x256, 6 iterations: flag on vs off
    under shared weights (setup and bound of
    test_model_bf16_corr_deviation_bounded)."""
    from flowhip.utils import layout
    torch.manual_seed(44)
    model = _ncup_model(dataset="sintel").eval()
    layout.apply_channels_last(model)
    img1 = torch.rand(1, 3, 128, 256, device=_dev()) * 255
    img2 = torch.rand(1, 3, 128, 256, device=_dev()) * 255
    outs = {}
    for flag in (False, True):
        model.args.alternate_corr = flag
        with torch.no_grad():
            _, flow = model(img1, img2, iters=6, test_mode=True)
        outs[flag] = flow.float()
    assert torch.isfinite(outs[True]).all()
    dev = (outs[True] - outs[False]).norm(dim=1).mean().item()
    print(f"alternate_corr vs volume path: mean EPE deviation {dev:.4g} px")
    assert dev < 0.1, dev


def test_train_step_with_flag():
    from flowhip import ops
    torch.manual_seed(1234)
    model = _ncup_model(alternate_corr=True)
    model.train()
    model.freeze_bn()
    h, w = 128, 256
    img1 = torch.rand(2, 3, h, w, device=_dev()) * 255
    img2 = torch.rand(2, 3, h, w, device=_dev()) * 255
    flow_gt = torch.randn(2, 2, h, w, device=_dev())
    valid = torch.ones(2, h, w, device=_dev())
    preds = model(img1, img2, iters=3)
    loss, _ = ops.sequence_loss(preds, flow_gt, valid, 0.85)
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss).item()
    for n, p in model.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and torch.isfinite(p.grad).all(), n


def test_graphed_inference_with_flag_replays_eager_bitwise():
    from flowhip.engine.graph import GraphedInference
    torch.manual_seed(1234)
    model = _ncup_model(alternate_corr=True).eval()
    shape = (1, 3, 128, 256)
    img1 = torch.rand(shape, device=_dev()) * 255
    img2 = torch.rand(shape, device=_dev()) * 255
    with torch.no_grad():
        low_e, up_e = model(img1, img2, iters=4, test_mode=True)
    g = GraphedInference(model, shape, iters=4)
    low_g, up_g = g(img1, img2)
    print("graph vs eager max|diff|:",
          (low_g - low_e).abs().max().item(), (up_g - up_e).abs().max().item())
    assert torch.equal(low_g, low_e)
    assert torch.equal(up_g, up_e)
