"""Accumulating weight-gradient partials (conv_gemm_wrw_plan / _partials /
_finish) against the one-shot call and an fp64 reference, then the autograd
plumbing that uses them (wrw_accumulate_scope, WrwSinkFn).

Accumulating K calls in one partials buffer and reducing once sums the same
fp32 per-chunk sums as K one-shot calls followed by K-1 fp32 adds, in a
different order. Per case both are measured against the fp64 sum of the K
gradients of the same rounded inputs; the accumulated error must be at most
twice the one-shot error (the project's reordering margin), and the
project's conv bound (atol=1e-1, rtol=5e-2) applies on top as a cap. Both
errors are printed.
"""

import contextlib
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

K = 3
CONV_BOUND = dict(atol=1e-1, rtol=5e-2)


def _dev():
    return torch.device("cuda:0")


# (id, B, H, W, C1, C2, Cout, KH, KW, ld_extra, stride, algos)
# The first eight are the shapes of tests/test_gpu_wrw_halo.py (tile tails,
# ragged Cin / Cout, Cout 2 -> 8 padding, two-source inputs, the 324-of-328
# narrowed view) on both paths; the last three are outside the halo
# envelope and run on the generic path only.
CASES = [
    ("floor_8to8_3x3", 1, 3, 5, 8, 0, 8, 3, 3, 0, 1, (0, 1)),
    ("tails_64to64_3x3", 2, 11, 37, 64, 0, 64, 3, 3, 0, 1, (0, 1)),
    ("ragged_72to126_3x3", 2, 11, 37, 72, 0, 126, 3, 3, 0, 1, (0, 1)),
    ("flowhead_256to2_3x3", 2, 11, 37, 256, 0, 2, 3, 3, 0, 1, (0, 1)),
    ("cat_64p40to64_1x5", 2, 11, 37, 64, 40, 64, 1, 5, 0, 1, (0, 1)),
    ("cat_64p40to64_5x1", 2, 11, 37, 64, 40, 64, 5, 1, 0, 1, (0, 1)),
    ("cat_128p256to128_5x1", 2, 9, 70, 128, 256, 128, 5, 1, 0, 1, (0, 1)),
    ("narrowed_324of328to64_3x3", 2, 11, 37, 324, 0, 64, 3, 3, 4, 1, (0, 1)),
    ("pointwise_72to64_1x1", 2, 11, 37, 72, 0, 64, 1, 1, 0, 1, (0,)),
    ("stride2_64to72_3x3", 2, 11, 37, 64, 0, 72, 3, 3, 0, 2, (0,)),
    ("convf1_8to16_7x7", 2, 11, 37, 8, 0, 16, 7, 7, 0, 1, (0,)),
]
COMBOS = [(c, a) for c in CASES for a in c[11]]
COMBO_IDS = [f"{c[0]}-algo{a}" for c, a in COMBOS]

_cache = {}


def _case(case):
    """K seeded (dy, x) pairs and the fp64 sum of their K gradients, built
    once per case and shared by every test of the case."""
    name, B, H, W, C1, C2, Cout, KH, KW, ld_extra, s, _ = case
    if name in _cache:
        return _cache[name]
    g = torch.Generator(device="cpu").manual_seed(2000 + len(name) + H * W)
    OH = (H + 2 * (KH // 2) - KH) // s + 1
    OW = (W + 2 * (KW // 2) - KW) // s + 1

    def cl(n, c, h, w):
        t = (torch.randn(n, c, h, w, generator=g) / 4).to(torch.bfloat16)
        return t.to(_dev()).contiguous(memory_format=torch.channels_last)

    pairs = []
    dw = torch.zeros(Cout, C1 + C2, KH, KW, dtype=torch.float64,
                     device=_dev())
    db = torch.zeros(Cout, dtype=torch.float64, device=_dev())
    for _ in range(K):
        x1 = cl(B, C1 + ld_extra, H, W)
        if ld_extra:
            x1 = x1[:, :C1]
        x2 = cl(B, C2, H, W) if C2 else None
        dy = cl(B, Cout, OH, OW)
        # the autograd functions pad dy's channels to a multiple of 8
        pad = (-Cout) % 8
        dyp = dy
        if pad:
            z = dy.new_zeros(B, pad, OH, OW).contiguous(
                memory_format=torch.channels_last)
            dyp = torch.cat([dy, z], dim=1).contiguous(
                memory_format=torch.channels_last)
        assert dyp.stride(1) == 1 and dyp.stride(3) == dyp.size(1)
        pairs.append((dyp, x1, x2))

        # fp64 gradient of the same rounded inputs, tap by tap
        xin = x1 if x2 is None else torch.cat([x1, x2], dim=1)
        xpad = torch.nn.functional.pad(
            xin.double(), (KW // 2, KW // 2, KH // 2, KH // 2))
        dy64 = dy.double()
        for ky in range(KH):
            for kx in range(KW):
                xs = xpad[:, :, ky:ky + s * (OH - 1) + 1:s,
                          kx:kx + s * (OW - 1) + 1:s]
                dw[:, :, ky, kx] += torch.einsum("noyx,ncyx->oc", dy64, xs)
        db += dy64.sum((0, 2, 3))
    _cache[name] = (pairs, dw, db)
    return _cache[name]


def _plan(C, case, algo, want_bias):
    _, _, _, _, _, _, _, KH, KW, _, s, _ = case
    dyp, x1, x2 = _case(case)[0][0]
    path, nchunk, numel, accumulate = C.conv_gemm_wrw_plan(
        dyp, x1, x2, KH, KW, s, s, want_bias, algo)
    assert path == algo and nchunk >= 1
    # the routing rule: shared calls sum their partials on the generic path
    assert accumulate == (1 if path == 0 else 0)
    return nchunk, numel


def _accumulate(C, case, algo, want_bias, k, fill=None):
    """k accumulating calls into one buffer (pre-filled with `fill`), then
    one finish -> (dw, dbias) over the padded Cout."""
    _, _, _, _, C1, C2, _, KH, KW, _, s, _ = case
    pairs = _case(case)[0]
    nchunk, numel = _plan(C, case, algo, want_bias)
    buf = torch.empty(numel, dtype=torch.float32, device=_dev())
    if fill is not None:
        buf.fill_(fill)
    for i in range(k):
        dyp, x1, x2 = pairs[i]
        C.conv_gemm_wrw_partials(dyp, x1, x2, buf, KH, KW, s, s, want_bias,
                                 i > 0, algo, nchunk)
    dw, db = C.conv_gemm_wrw_finish(buf, pairs[0][0].shape[1], C1 + C2, KH,
                                    KW, want_bias, nchunk)
    torch.cuda.synchronize()
    return dw, db


def _one_shot(C, case, algo, want_bias, i):
    _, _, _, _, _, _, _, KH, KW, _, s, _ = case
    dyp, x1, x2 = _case(case)[0][i]
    nchunk, _ = _plan(C, case, algo, want_bias)
    return C.conv_gemm_wrw(dyp, x1, x2, KH, KW, s, s, want_bias, algo, nchunk)


_bias = pytest.mark.parametrize("want_bias", [False, True],
                                ids=["nobias", "bias"])
_combo = pytest.mark.parametrize("combo", COMBOS, ids=COMBO_IDS)


@_bias
@_combo
def test_k3_accumulate_vs_one_shot_vs_fp64(combo, want_bias):
    import flowhip._C as C
    case, algo = combo
    name, Cout = case[0], case[6]
    _, dw_ref, db_ref = _case(case)

    dw_a, db_a = _accumulate(C, case, algo, want_bias, K)
    dw_s = db_s = None
    for i in range(K):
        dw, db = _one_shot(C, case, algo, want_bias, i)
        dw_s = dw if dw_s is None else dw_s + dw      # fp32 adds, as autograd
        if want_bias:
            db_s = db if db_s is None else db_s + db
    assert dw_a.shape == dw_s.shape

    err_a = (dw_a[:Cout].double() - dw_ref).abs().max().item()
    err_s = (dw_s[:Cout].double() - dw_ref).abs().max().item()
    print(f"[wrw_accum] {name} algo{algo} dW max-abs err: one-shot sum "
          f"{err_s:.3e} accumulated {err_a:.3e}")
    if want_bias:
        berr_a = (db_a[:Cout].double() - db_ref).abs().max().item()
        berr_s = (db_s[:Cout].double() - db_ref).abs().max().item()
        print(f"[wrw_accum] {name} algo{algo} dbias max-abs err: one-shot "
              f"sum {berr_s:.3e} accumulated {berr_a:.3e}")

    assert torch.isfinite(dw_a).all()
    assert err_a <= 2.0 * err_s, (err_a, err_s)
    torch.testing.assert_close(dw_a[:Cout].double(), dw_ref, **CONV_BOUND)
    if want_bias:
        assert berr_a <= 2.0 * berr_s, (berr_a, berr_s)
        torch.testing.assert_close(db_a[:Cout].double(), db_ref,
                                   **CONV_BOUND)


@_bias
@_combo
def test_k1_bit_identical_to_one_shot(combo, want_bias):
    import flowhip._C as C
    case, algo = combo
    dw_a, db_a = _accumulate(C, case, algo, want_bias, 1)
    dw_s, db_s = _one_shot(C, case, algo, want_bias, 0)
    assert torch.equal(dw_a, dw_s)
    if want_bias:
        assert torch.equal(db_a, db_s)


@_bias
@_combo
def test_first_call_overwrites_and_runs_are_deterministic(combo, want_bias):
    """A NaN-filled buffer gives the finite result of a zero-filled one
    (the first call overwrites every slot the reduce reads), and a second
    run of the same K-call sequence is bit-identical."""
    import flowhip._C as C
    case, algo = combo
    dw_n, db_n = _accumulate(C, case, algo, want_bias, K, fill=float("nan"))
    dw_z, db_z = _accumulate(C, case, algo, want_bias, K, fill=0.0)
    dw_r, db_r = _accumulate(C, case, algo, want_bias, K)
    assert torch.isfinite(dw_n).all()
    assert torch.equal(dw_n, dw_z) and torch.equal(dw_n, dw_r)
    if want_bias:
        assert torch.isfinite(db_n).all()
        assert torch.equal(db_n, db_z) and torch.equal(db_n, db_r)


@_bias
@_combo
def test_finish_into_equals_fp32_sum_of_one_shots(combo, want_bias):
    """One-shot partials whose finish adds to a running dW / dbias (the
    route of the shapes that do not accumulate partials) do the same fp32
    adds, in the same order, as summing K one-shot results: bit-identical."""
    import flowhip._C as C
    case, algo = combo
    _, _, _, _, C1, C2, _, KH, KW, _, s, _ = case
    pairs = _case(case)[0]
    nchunk, numel = _plan(C, case, algo, want_bias)
    buf = torch.full((numel,), float("nan"), dtype=torch.float32,
                     device=_dev())
    dw = db = dw_s = db_s = None
    for i, (dyp, x1, x2) in enumerate(pairs):
        C.conv_gemm_wrw_partials(dyp, x1, x2, buf, KH, KW, s, s, want_bias,
                                 False, algo, nchunk)
        dw, db = C.conv_gemm_wrw_finish(buf, dyp.shape[1], C1 + C2, KH, KW,
                                        want_bias, nchunk, dw,
                                        db if want_bias else None)
        dw1, db1 = _one_shot(C, case, algo, want_bias, i)
        dw_s = dw1 if dw_s is None else dw_s + dw1
        if want_bias:
            db_s = db1 if db_s is None else db_s + db1
    torch.cuda.synchronize()
    assert torch.equal(dw, dw_s)
    if want_bias:
        assert torch.equal(db, db_s)


def test_partials_rejects_a_pair_that_is_no_plan():
    """(algo, nchunk) other than a plan for the shapes would size the grid
    past the buffer: an error, nothing launched."""
    import flowhip._C as C
    case = CASES[1]
    dyp, x1, x2 = _case(case)[0][0]
    nchunk, numel = _plan(C, case, 1, False)
    buf = torch.empty(numel, dtype=torch.float32, device=_dev())
    with pytest.raises(RuntimeError):
        C.conv_gemm_wrw_partials(dyp, x1, x2, buf, 3, 3, 1, 1, False, False,
                                 1, nchunk + 100000)
    with pytest.raises(RuntimeError):
        C.conv_gemm_wrw_partials(dyp, x1, x2, buf[:-1], 3, 3, 1, 1, False,
                                 False, 1, nchunk)
    with pytest.raises(RuntimeError):   # dw_into of another shape
        C.conv_gemm_wrw_finish(buf, dyp.shape[1], 64, 3, 3, False, nchunk,
                               torch.zeros(8, 64, 3, 3, device=_dev()))


# ---------------------------------------------------------------------------
# Autograd level
# ---------------------------------------------------------------------------

def _scope(on):
    from flowhip.ops.functional_conv import wrw_accumulate_scope
    return wrw_accumulate_scope() if on else contextlib.nullcontext()


def _chain_setup():
    from flowhip.nn.update import FusedConv2d
    torch.manual_seed(7)
    conv = FusedConv2d(16, 16, 3, padding=1).to(_dev())
    g = torch.Generator(device="cpu").manual_seed(8)
    x0 = torch.randn(1, 16, 8, 16, generator=g).to(torch.bfloat16).to(
        _dev()).contiguous(memory_format=torch.channels_last)
    gs = [torch.randn(1, 16, 8, 16, generator=g).to(_dev())
          for _ in range(3)]
    return conv, x0, gs


def _chain_run(conv, x0, gs, scope, used=(0, 1, 2), backwards=1):
    from flowhip.ops import functional_conv as fc
    conv.zero_grad(set_to_none=True)
    x = x0.clone().requires_grad_(True)
    with _scope(scope):
        ys = [conv(x)]
        ys.append(conv(ys[0]))
        ys.append(conv(ys[1]))
        n_handles = len(fc._tls.handles) if scope else 0
    loss = sum((ys[i].float() * gs[i]).sum() for i in used)
    for b in range(backwards):
        loss.backward(retain_graph=b + 1 < backwards)
    torch.cuda.synchronize()
    return ([y.detach() for y in ys], x.grad, conv.weight.grad.clone(),
            conv.bias.grad.clone(), n_handles)


@pytest.mark.parametrize("used", [(0, 1, 2), (0, 1)], ids=["all", "unused3"])
def test_chained_conv_scope_on_vs_off(used):
    """A 16->16 3x3 FusedConv2d applied 3 times in a chain; `unused3`: the
    third output is not in the loss, so its backward never runs."""
    conv, x0, gs = _chain_setup()
    ys0, dx0, dw0, db0, _ = _chain_run(conv, x0, gs, False, used)
    ys1, dx1, dw1, db1, n = _chain_run(conv, x0, gs, True, used)
    assert n == 1                       # the scope made one shared handle
    for a, b in zip(ys0, ys1):
        assert torch.equal(a, b)
    assert torch.equal(dx0, dx1)
    torch.testing.assert_close(dw1, dw0, **CONV_BOUND)
    torch.testing.assert_close(db1, db0, **CONV_BOUND)
    assert dw1.abs().max() > 0


def test_chained_conv_backward_twice_doubles_grad():
    """The second backward(retain_graph=True) starts from a released
    buffer; both passes are deterministic, so .grad is exactly doubled."""
    conv, x0, gs = _chain_setup()
    _, _, dw1, db1, _ = _chain_run(conv, x0, gs, True)
    _, _, dw2, db2, _ = _chain_run(conv, x0, gs, True, backwards=2)
    assert torch.equal(dw2, 2 * dw1)
    assert torch.equal(db2, 2 * db1)


def test_scope_under_no_grad_makes_no_handle():
    from flowhip.ops import functional_conv as fc
    conv, x0, _ = _chain_setup()
    with torch.no_grad():
        y_off = conv(conv(x0))
        with fc.wrw_accumulate_scope():
            y_on = conv(conv(x0))
            assert len(fc._tls.handles) == 0
    assert torch.equal(y_on, y_off)
    assert not y_on.requires_grad


def test_sepconvgru_two_iterations_scope_on_vs_off():
    """Two SepConvGRU iterations (hidden 64, 8x16) through the packed z+r
    path: all six weights and six biases against the scope-off result."""
    from flowhip.nn.update import SepConvGRU
    from flowhip.ops import functional_conv as fc
    torch.manual_seed(11)
    gru = SepConvGRU(hidden_dim=64, input_dim=64).to(_dev())
    g = torch.Generator(device="cpu").manual_seed(12)

    def cl(c):
        return torch.randn(1, c, 8, 16, generator=g).to(torch.bfloat16).to(
            _dev()).contiguous(memory_format=torch.channels_last)

    h0, x, gy = cl(64), cl(64), cl(64).float()

    def run(scope):
        gru.zero_grad(set_to_none=True)
        with _scope(scope):
            h = gru(gru(h0, x), x)
            n = len(fc._tls.handles) if scope else 0
        (h.float() * gy).sum().backward()
        torch.cuda.synchronize()
        return h.detach(), {k: p.grad.clone()
                            for k, p in gru.named_parameters()}, n

    h_off, g_off, _ = run(False)
    h_on, g_on, n = run(True)
    assert n == 4                       # zr1, q1, zr2, q2
    assert torch.equal(h_on, h_off)
    assert len(g_on) == 12
    for k in g_off:
        torch.testing.assert_close(g_on[k], g_off[k], **CONV_BOUND)
        assert g_on[k].abs().max() > 0, k


# ---------------------------------------------------------------------------
# Model level: FLOWHIP_WRW_ACCUM=1 against 0, each in its own child process
# ---------------------------------------------------------------------------

_CHILD = """
import sys, torch
from flowhip.config.args import default_ncup_args
from flowhip.models import build_model
from flowhip import ops
dev = torch.device("cuda:0")
args = default_ncup_args(model="raft_nc_dbl", small=False,
                         mixed_precision=True, dataset="sintel")
torch.manual_seed(1234)
model = build_model(args).to(dev)
model.train()
g = torch.Generator(device="cpu").manual_seed(5)
h, w = 64, 96
im1 = (torch.rand(1, 3, h, w, generator=g) * 255).to(dev)
im2 = (torch.rand(1, 3, h, w, generator=g) * 255).to(dev)
gt = torch.randn(1, 2, h, w, generator=g).to(dev)
valid = torch.ones(1, h, w, device=dev)
preds = model(im1, im2, iters=3)
loss, _ = ops.sequence_loss(preds, gt, valid, 0.85)
loss.backward()
torch.cuda.synchronize()
torch.save({"preds": [p.detach().cpu() for p in preds],
            "grads": {k: p.grad.cpu() for k, p in model.named_parameters()
                      if p.grad is not None}}, sys.argv[1])
"""


def test_model_accum_on_vs_off(tmp_path):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = {}
    for flag in ("1", "0"):
        path = str(tmp_path / f"accum{flag}.pt")
        env = dict(os.environ, FLOWHIP_WRW_ACCUM=flag, PYTHONPATH=repo)
        subprocess.run([sys.executable, "-c", _CHILD, path], env=env,
                       cwd=repo, check=True, timeout=300)
        out[flag] = torch.load(path, weights_only=True)
    on, off = out["1"], out["0"]
    assert len(on["preds"]) == 3
    for a, b in zip(on["preds"], off["preds"]):
        assert torch.equal(a, b)
    assert on["grads"].keys() == off["grads"].keys() and on["grads"]
    worst = 0.0
    for k in off["grads"]:
        worst = max(worst, (on["grads"][k] - off["grads"][k]).abs().max()
                    .item())
        torch.testing.assert_close(on["grads"][k], off["grads"][k],
                                   **CONV_BOUND, msg=lambda m: f"{k}: {m}")
    print(f"[wrw_accum] model grads, accumulate on vs off: max-abs "
          f"{worst:.3e}")


def test_model_under_ddp_static_graph_world1():
    """The model as engine/distributed.py wraps it (one bucket, bucket
    views, static_graph) over single-rank nccl: with the scope on, every
    step's gradients match the unwrapped model's. static_graph takes effect
    from the second step, so three are run. Bound: the one
    tests/test_gpu_distributed.py uses for the same comparison (the
    backward of other kernels is not bit-reproducible)."""
    import torch.distributed as dist
    from flowhip import ops
    from flowhip.config.args import default_ncup_args
    from flowhip.engine import distributed
    from flowhip.models import build_model
    if dist.is_initialized():
        pytest.skip("process group already active")

    def make():
        torch.manual_seed(11)
        m = build_model(default_ncup_args(
            model="raft_nc_dbl", mixed_precision=True,
            dataset="sintel")).to(_dev())
        m.train()
        m.freeze_bn()
        return m

    g = torch.Generator().manual_seed(7)
    b, h, w = 1, 128, 128
    im1 = (torch.rand(b, 3, h, w, generator=g) * 255).to(_dev())
    im2 = (torch.rand(b, 3, h, w, generator=g) * 255).to(_dev())
    gt = torch.randn(b, 2, h, w, generator=g).to(_dev())
    valid = torch.ones(b, h, w, device=_dev())

    def grads(model, params):
        model.zero_grad(set_to_none=True)
        loss, _ = ops.sequence_loss(model(im1, im2, iters=2), gt, valid, 0.85)
        loss.backward()
        torch.cuda.synchronize()
        return {n: p.grad.float().clone() for n, p in params
                if p.grad is not None}

    plain = make()
    ref = grads(plain, list(plain.named_parameters()))
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29743")
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        inner = make()
        ddp = distributed.wrap_ddp(inner, _dev())
        assert ddp is not inner
        for _ in range(3):
            got = grads(ddp, list(inner.named_parameters()))
            assert set(got) == set(ref)
            bad = [n for n in ref if not torch.allclose(
                got[n], ref[n], atol=2e-2, rtol=2e-2)]
            assert not bad, bad[:8]
    finally:
        dist.destroy_process_group()
