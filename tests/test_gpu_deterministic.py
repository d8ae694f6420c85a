"""GPU tests (MI355X) for deterministic mode: the atomics-free forms of the
column sums, the instance-norm partial reduction and the convex-upsample
flow gradient repeat bit for bit and stay inside their oracles' bounds, and
a whole training step (forward, loss, backward, clipped AdamW) of the
full-size `raft_nc_dbl` and `raft` repeats bit for bit with the mode on.
The switch itself is covered on the CPU in tests/test_deterministic_mode.py.

Nothing here asserts that the default path differs between runs: at these
sizes it often does not, and a test must not depend on a race."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

REPEATS = 3


def _dev():
    return torch.device("cuda:0")


def _ext():
    from flowhip.ops import _ext as loader
    return loader.ext()


@pytest.fixture
def det_mode():
    from flowhip import ops
    with ops.deterministic():
        yield


# ---------------------------------------------------------------------------
# column sums

COL_C = [8, 24, 64, 96]


@functools.lru_cache(maxsize=None)
def _col_case(C):
    """(1, C, 25, 31) channels-last bf16 pair: 775 rows are three whole
    256-row chunks and a 7-row tail. randn * 10^U(-2, 2) spreads the
    magnitudes over four decades, so the order of addition shows in the
    last bits. Returns the operands and, per sum, the float64 total and the
    first-order bound (M - 1) * 2^-24 * sum|term| that holds for any fp32
    summation order of exact terms (bf16 values and bf16 x bf16 products are
    exact in fp32)."""
    gen = torch.Generator().manual_seed(100 + C)

    def draw():
        v = torch.randn(1, C, 25, 31, generator=gen)
        v = v * 10 ** (torch.rand(1, C, 25, 31, generator=gen) * 4 - 2)
        return v.to(torch.bfloat16).contiguous(
            memory_format=torch.channels_last)

    g, x = draw(), draw()
    M = 25 * 31
    terms = {"g": g.double(), "gx": g.double() * x.double()}
    ref = {k: t.sum(dim=(0, 2, 3)) for k, t in terms.items()}
    bound = {k: (M - 1) * 2.0 ** -24 * t.abs().sum(dim=(0, 2, 3))
             for k, t in terms.items()}
    return g.to(_dev()), x.to(_dev()), ref, bound


def _within(out, ref, bound, what):
    err = (out.double().cpu() - ref).abs()
    worst = (err / bound).max().item()
    print(f"{what}: max err / bound = {worst:.3g}")
    assert (err <= bound).all(), (what, worst)


@pytest.mark.parametrize("C", COL_C)
def test_col_sum_repeats_and_is_bounded(C):
    g, _, ref, bound = _col_case(C)
    outs = [_ext().col_sum_bf16(g, deterministic=True) for _ in range(REPEATS)]
    assert outs[0].shape == (C,) and outs[0].dtype == torch.float32
    for o in outs[1:]:
        assert torch.equal(o, outs[0])
    for o in outs:
        _within(o, ref["g"], bound["g"], f"col_sum C={C}")


@pytest.mark.parametrize("C", COL_C)
def test_col_sum2_repeats_and_is_bounded(C):
    g, x, ref, bound = _col_case(C)
    outs = [_ext().col_sum2_bf16(g, x, deterministic=True)
            for _ in range(REPEATS)]
    assert outs[0].shape == (2, C) and outs[0].dtype == torch.float32
    for o in outs[1:]:
        assert torch.equal(o, outs[0])
    for o in outs:
        _within(o[0], ref["g"], bound["g"], f"col_sum2[0] C={C}")
        _within(o[1], ref["gx"], bound["gx"], f"col_sum2[1] C={C}")


def test_frozen_bn_backward_passes_the_mode(det_mode):
    """`_FrozenBNFn.backward` with the mode on returns the deterministic
    binding's sums: db is its first row bit for bit."""
    from flowhip.nn.norm import BatchNorm2d
    C = 24
    g, x, _, _ = _col_case(C)
    bn = BatchNorm2d(C).to(_dev()).eval()
    xin = x.clone().requires_grad_(True)
    bn(xin).backward(g)
    sums = _ext().col_sum2_bf16(g, x, deterministic=True)
    assert torch.equal(bn.bias.grad, sums[0])


# ---------------------------------------------------------------------------
# instance norm

IN_TOL = {torch.float32: dict(atol=1e-5, rtol=1e-5),
          torch.bfloat16: dict(atol=3e-2, rtol=3e-2)}


@functools.lru_cache(maxsize=None)
def _instnorm_case(C, dtype):
    """(2, C, 9, 130): P = 1170 is two 1024-pixel chunks, the second ragged.
    Returns x, dy and torch's own y and dx (fp32 math on the same values)."""
    gen = torch.Generator().manual_seed(200 + C)
    x = torch.randn(2, C, 9, 130, generator=gen).to(dtype)
    dy = torch.randn(2, C, 9, 130, generator=gen).to(dtype)
    xr = x.float().clone().requires_grad_(True)  # .float() may alias x
    yr = torch.nn.functional.instance_norm(xr, eps=1e-5)
    (dxr,) = torch.autograd.grad(yr, xr, dy.float())
    cl = dict(memory_format=torch.channels_last)
    return (x.to(_dev()).contiguous(**cl), dy.to(_dev()).contiguous(**cl),
            yr.detach(), dxr)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [8, 16, 24, 64])
def test_instnorm_repeats_and_matches_torch(C, dtype):
    x, dy, yr, dxr = _instnorm_case(C, dtype)
    runs = []
    for _ in range(REPEATS):
        y, mean, rstd = _ext().instnorm_cl_fwd(x, 1e-5, deterministic=True)
        dx = _ext().instnorm_cl_bwd(x, dy, mean, rstd, deterministic=True)
        runs.append((y, mean, rstd, dx))
    for run in runs[1:]:
        for name, a, b in zip(("y", "mean", "rstd", "dx"), run, runs[0]):
            assert torch.equal(a, b), name
    for y, _, _, dx in runs:
        torch.testing.assert_close(y.float().cpu(), yr, **IN_TOL[dtype])
        torch.testing.assert_close(dx.float().cpu(), dxr, **IN_TOL[dtype])


def test_instnorm_module_passes_the_mode(det_mode):
    """The module's forward and backward with the mode on are the
    deterministic bindings' results bit for bit."""
    from flowhip.nn.norm import InstanceNorm2d
    x, dy, _, _ = _instnorm_case(8, torch.float32)
    xin = x.clone().requires_grad_(True)
    y = InstanceNorm2d(8).to(_dev())(xin)
    y.backward(dy)
    y0, mean, rstd = _ext().instnorm_cl_fwd(x, 1e-5, deterministic=True)
    dx0 = _ext().instnorm_cl_bwd(x, dy, mean, rstd, deterministic=True)
    assert torch.equal(y.detach(), y0)
    assert torch.equal(xin.grad, dx0)


# ---------------------------------------------------------------------------
# convex upsample

@functools.lru_cache(maxsize=None)
def _convex_case():
    """N=2, H=5, W=7: corner, edge and interior coarse pixels all occur.
    Returns the operands and the float64 autograd of the torch reference."""
    from flowhip.ops import torch_ref
    gen = torch.Generator().manual_seed(300)
    flow = torch.randn(2, 2, 5, 7, generator=gen)
    mask = 3 * torch.randn(2, 576, 5, 7, generator=gen)
    gout = torch.randn(2, 2, 40, 56, generator=gen)
    fr = flow.double().requires_grad_(True)
    mr = mask.double().requires_grad_(True)
    ref = torch_ref.convex_upsample(fr, mr, 8)
    rf, rm = torch.autograd.grad(ref, (fr, mr), gout.double())
    return flow.to(_dev()), mask.to(_dev()), gout.to(_dev()), rf, rm


def test_convex_gflow_repeats_and_matches_fp64():
    flow, mask, gout, rf, rm = _convex_case()
    runs = [_ext().convex_up_bwd(gout, flow, mask, 8, deterministic=True)
            for _ in range(REPEATS)]
    for gflow, gmask in runs[1:]:
        assert torch.equal(gflow, runs[0][0])
        assert torch.equal(gmask, runs[0][1])
    for gflow, gmask in runs:
        torch.testing.assert_close(gflow.double().cpu(), rf,
                                   atol=1e-3, rtol=1e-3)
        torch.testing.assert_close(gmask.double().cpu(), rm,
                                   atol=1e-3, rtol=1e-3)


def test_convex_gmask_bits_do_not_change_with_the_mode():
    flow, mask, gout, _, _ = _convex_case()
    _, gmask_det = _ext().convex_up_bwd(gout, flow, mask, 8,
                                        deterministic=True)
    _, gmask_def = _ext().convex_up_bwd(gout, flow, mask, 8)
    assert torch.equal(gmask_det, gmask_def)


def test_convex_function_passes_the_mode(det_mode):
    from flowhip.ops.functional_upsample import ConvexUpsampleFn
    flow, mask, gout, _, _ = _convex_case()
    f = flow.clone().requires_grad_(True)
    m = mask.clone().requires_grad_(True)
    df, dm = torch.autograd.grad(ConvexUpsampleFn.apply(f, m, 8), (f, m),
                                 gout)
    gflow, gmask = _ext().convex_up_bwd(gout, flow, mask, 8,
                                        deterministic=True)
    assert torch.equal(df, gflow)
    assert torch.equal(dm, gmask)


# ---------------------------------------------------------------------------
# whole training step

H_IMG, W_IMG, BATCH, ITERS = 64, 96, 2, 3


def _batch():
    gen = torch.Generator().manual_seed(4321)
    img1 = (torch.rand(BATCH, 3, H_IMG, W_IMG, generator=gen) * 255)
    img2 = (torch.rand(BATCH, 3, H_IMG, W_IMG, generator=gen) * 255)
    flow_gt = torch.randn(BATCH, 2, H_IMG, W_IMG, generator=gen) * 4
    valid = torch.ones(BATCH, H_IMG, W_IMG)
    return [t.to(_dev()) for t in (img1, img2, flow_gt, valid)]


def _build(model_name, **kw):
    from flowhip.config.args import default_ncup_args
    from flowhip.models import build_model
    torch.manual_seed(1234)
    args = default_ncup_args(model=model_name, mixed_precision=True, **kw)
    model = build_model(args).to(_dev())
    model.train()
    model.freeze_bn()  # the frozen-BN backward (col_sum2) runs
    return model


def _train_run(model_name):
    """Seeded model, one forward + loss + backward (gradients recorded),
    then three clipped AdamW steps. Returns the recorded gradients and the
    final parameters, both by name."""
    from flowhip import ops
    model = _build(model_name)
    img1, img2, flow_gt, valid = _batch()
    opt = torch.optim.AdamW(model.parameters(), lr=1.25e-4,
                            weight_decay=1e-5, eps=1e-8)

    def fwd_bwd():
        opt.zero_grad(set_to_none=True)
        preds = model(img1, img2, iters=ITERS)
        loss, _ = ops.sequence_loss(preds, flow_gt, valid, 0.85)
        loss.backward()
        return loss

    loss = fwd_bwd()
    assert torch.isfinite(loss).item()
    grads = {n: p.grad.detach().clone()
             for n, p in model.named_parameters() if p.grad is not None}
    assert grads
    for step in range(3):
        if step:
            fwd_bwd()
        torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
        opt.step()
    params = {n: p.detach().clone() for n, p in model.named_parameters()}
    torch.cuda.synchronize()
    return grads, params


def _assert_step_repeats(model_name):
    g1, p1 = _train_run(model_name)
    g2, p2 = _train_run(model_name)
    assert g1.keys() == g2.keys()
    # reverse registration order is roughly backward order: the first name
    # reported is the op to look at
    diff = [n for n in reversed(list(g1)) if not torch.equal(g1[n], g2[n])]
    assert not diff, f"{len(diff)} of {len(g1)} gradients differ: {diff[:8]}"
    moved = [n for n in p1 if not torch.equal(p1[n], p2[n])]
    assert not moved, f"{len(moved)} parameters differ: {moved[:8]}"


def test_train_step_repeats_raft_nc_dbl(det_mode):
    _assert_step_repeats("raft_nc_dbl")


def test_train_step_repeats_raft(det_mode):
    """Exercises the convex-upsample backward, and the mask head's two torch
    nn.Conv2d modules: their weight gradient (aten::convolution_backward,
    MIOpen backward-weights) differed between runs until the mode also set
    torch.backends.cudnn.deterministic."""
    _assert_step_repeats("raft")


def test_alternate_corr_backward_refuses(det_mode):
    """The forward of the on-demand lookup runs; the backward, which would
    sum fmap2's gradient with float atomics, raises in Python before any
    kernel launch."""
    from flowhip import ops
    model = _build("raft", alternate_corr=True)
    img1, img2, flow_gt, valid = _batch()
    preds = model(img1, img2, iters=ITERS)
    loss, _ = ops.sequence_loss(preds, flow_gt, valid, 0.85)
    assert torch.isfinite(loss).item()
    with pytest.raises(RuntimeError, match="deterministic"):
        loss.backward()
