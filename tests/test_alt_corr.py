"""On-demand correlation lookup (`--alternate_corr`), CPU side: the chunked
torch formulation against the all-pairs-volume formulation, its gradients,
and the flag's path through models, parsers and evaluate.py."""

import argparse
import copy

import pytest
import torch

from flowhip import ops
from flowhip.config.args import (build_eval_parser, build_train_parser,
                                 default_ncup_args)
from flowhip.models import build_model
from flowhip.nn import AlternateCorrBlock, CorrBlock
from flowhip.ops import torch_ref


def _inputs(B, D, H, W, seed):
    """Features + coords uniform over the map extended by 6 px per side,
    with three planted pixels: far outside, the last cell, a corner-out."""
    g = torch.Generator().manual_seed(seed)
    f1 = torch.randn(B, D, H, W, generator=g)
    f2 = torch.randn(B, D, H, W, generator=g)
    u = torch.rand(B, 2, H, W, generator=g)
    ext = torch.tensor([W + 12.0, H + 12.0]).view(1, 2, 1, 1)
    coords = u * ext - 6.0
    coords[0, :, 0, 0] = torch.tensor([1e6, -1e6])
    coords[0, :, 1, 2] = torch.tensor([W - 1.0, H - 1.0])
    coords[0, :, 2, 1] = torch.tensor([-4.0, -4.0])
    return f1, f2, coords


def _volume_lookup(f1, f2, coords, radius, levels=4):
    pyr = torch_ref.corr_pyramid(torch_ref.corr_volume(f1, f2), levels)
    return torch_ref.corr_lookup(pyr, coords, radius)


SHAPES = [(2, 256, 16, 24, 4), (2, 128, 17, 27, 3)]


@pytest.mark.parametrize("B,D,H,W,r", SHAPES)
def test_chunked_lookup_matches_volume_formulation(B, D, H, W, r):
    f1, f2, coords = _inputs(B, D, H, W, seed=10 + r)
    ref = _volume_lookup(f1, f2, coords, r)
    levels = torch_ref.alt_corr_pyramid(f2, 4)
    assert [tuple(x.shape[-2:]) for x in levels] == [
        (H >> l, W >> l) for l in range(4)]
    P = H * W
    # chunk sizes that divide P, do not divide P, and exceed P
    for chunk in (P // 4 if P % 4 == 0 else P // 3, 100, 7, 2 * P):
        out = torch_ref.alt_corr_lookup(f1, levels, coords, r, chunk=chunk)
        assert out.shape == ref.shape and out.dtype == torch.float32
        torch.testing.assert_close(out, ref, atol=1e-4, rtol=1e-4)
    # the far-outside pixel sees nothing
    assert out[0, :, 0, 0].abs().max().item() == 0.0


def test_ops_dispatch_cpu_matches_volume_formulation():
    B, D, H, W, r = 2, 128, 17, 27, 3
    f1, f2, coords = _inputs(B, D, H, W, seed=3)
    out = ops.alt_corr_lookup(f1, ops.alt_corr_pyramid(f2, 4), coords, r)
    torch.testing.assert_close(out, _volume_lookup(f1, f2, coords, r),
                               atol=1e-4, rtol=1e-4)


def test_chunked_gradients_match_volume_formulation():
    B, D, H, W, r = 1, 128, 16, 24, 4
    f1, f2, coords = _inputs(B, D, H, W, seed=5)
    f1a = f1.clone().requires_grad_(True)
    f2a = f2.clone().requires_grad_(True)
    out = torch_ref.alt_corr_lookup(
        f1a, torch_ref.alt_corr_pyramid(f2a, 4), coords, r, chunk=100)
    g = torch.randn(out.shape, generator=torch.Generator().manual_seed(6))
    d1, d2 = torch.autograd.grad(out, (f1a, f2a), g)

    f1r = f1.clone().requires_grad_(True)
    f2r = f2.clone().requires_grad_(True)
    r1, r2 = torch.autograd.grad(_volume_lookup(f1r, f2r, coords, r),
                                 (f1r, f2r), g)
    torch.testing.assert_close(d1, r1, atol=1e-3, rtol=1e-3)
    torch.testing.assert_close(d2, r2, atol=1e-3, rtol=1e-3)


def test_block_matches_corr_block():
    f1, f2, coords = _inputs(1, 128, 16, 24, seed=8)
    a = AlternateCorrBlock(f1, f2, num_levels=4, radius=3)(coords)
    v = CorrBlock(f1, f2, num_levels=4, radius=3)(coords)
    torch.testing.assert_close(a, v, atol=1e-4, rtol=1e-4)


def _model_args(name, small):
    return default_ncup_args(model=name, small=small, dataset="sintel",
                             mixed_precision=False)


MODELS = [("raft", True), ("raft_nc_dbl", False)]


@pytest.mark.parametrize("name,small", MODELS)
def test_model_forward_agrees_with_volume_path(name, small):
    torch.manual_seed(0)
    vol = build_model(_model_args(name, small)).eval()
    args = _model_args(name, small)
    args.alternate_corr = True
    alt = build_model(args).eval()
    alt.load_state_dict(copy.deepcopy(vol.state_dict()))

    img1 = torch.rand(1, 3, 128, 128) * 255
    img2 = torch.rand(1, 3, 128, 128) * 255
    with torch.no_grad():
        lo_v, up_v = vol(img1, img2, iters=2, test_mode=True)
        lo_a, up_a = alt(img1, img2, iters=2, test_mode=True)
    torch.testing.assert_close(lo_a, lo_v, atol=1e-4, rtol=1e-4)
    torch.testing.assert_close(up_a, up_v, atol=1e-4, rtol=1e-4)


@pytest.mark.parametrize("name,small", MODELS)
def test_model_train_step_finite_grads(name, small):
    torch.manual_seed(1)
    args = _model_args(name, small)
    args.alternate_corr = True
    model = build_model(args).train()
    img1 = torch.rand(1, 3, 128, 128) * 255
    img2 = torch.rand(1, 3, 128, 128) * 255
    gt = torch.randn(1, 2, 128, 128)
    valid = torch.ones(1, 128, 128)
    preds = model(img1, img2, iters=2)
    loss, _ = ops.sequence_loss(preds, gt, valid, 0.85)
    loss.backward()
    assert torch.isfinite(loss).item()
    for n, p in model.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and torch.isfinite(p.grad).all(), n


def test_flag_selects_the_block(monkeypatch):
    """alternate_corr=True builds AlternateCorrBlock; a Namespace without
    the attribute (or with it False) builds the volume path."""
    from flowhip.models import raft as raft_mod
    built = []

    class SpyAlt(AlternateCorrBlock):
        def __init__(self, *a, **k):
            built.append("alt")
            super().__init__(*a, **k)

    class SpyVol(CorrBlock):
        def __init__(self, *a, **k):
            built.append("vol")
            super().__init__(*a, **k)

    monkeypatch.setattr(raft_mod, "AlternateCorrBlock", SpyAlt)
    monkeypatch.setattr(raft_mod, "CorrBlock", SpyVol)
    img = torch.rand(1, 3, 128, 128) * 255

    args = _model_args("raft", True)
    assert args.alternate_corr is False
    ns = argparse.Namespace(**{k: v for k, v in vars(args).items()
                               if k != "alternate_corr"})
    assert not hasattr(ns, "alternate_corr")
    on = _model_args("raft", True)
    on.alternate_corr = True
    for a, want in ((ns, "vol"), (args, "vol"), (on, "alt")):
        del built[:]
        torch.manual_seed(2)
        with torch.no_grad():
            build_model(a).eval()(img, img, iters=1, test_mode=True)
        assert built == [want]


def test_parsers_accept_flag():
    import demo
    argv = ["--alternate_corr"]
    assert build_train_parser(argv=argv).parse_args(argv).alternate_corr
    assert build_eval_parser(argv=argv).parse_args(argv).alternate_corr
    assert demo.build_parser().parse_args(argv).alternate_corr
    for p in (build_train_parser(argv=[]), build_eval_parser(argv=[]),
              demo.build_parser()):
        assert p.parse_args([]).alternate_corr is False


@pytest.mark.timeout(600)
def test_evaluate_cli_synthetic_alternate_corr(tmp_path):
    """evaluate.py end-to-end on the synthetic validator with the flag."""
    import subprocess
    import sys

    from flowhip.engine import checkpoints

    torch.manual_seed(0)
    args = default_ncup_args(model="raft_nc_dbl", small=True,
                             dataset="synthetic")
    ckpt = tmp_path / "m.pth"
    checkpoints.save_weights(build_model(args), str(ckpt))

    r = subprocess.run(
        [sys.executable, "evaluate.py", "--model", "raft_nc_dbl", "--small",
         "--restore_ckpt", str(ckpt), "--dataset", "synthetic",
         "--iters", "2", "--alternate_corr"],
        capture_output=True, text=True, timeout=500)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "synthetic" in r.stdout.lower()
