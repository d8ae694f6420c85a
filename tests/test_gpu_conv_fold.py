"""Tap-folded small-Cin convolution path (csrc/conv_fold.h; the FOLD variant
of conv_gemm_fwd_kernel, conv_wrw_fold_kernel and its reduce).

Exact cases: inputs, weights, bias and cotangents are integers in
{-1, 0, 1}. A forward sum has at most 7*7*3 + 1 = 148 terms, so it stays
below 256 and is exact in bf16; a gradient sum has at most 2*161*161 terms,
below 2^24, exact in fp32. Forward, dW and dbias must equal the fp64 CPU
oracle bit for bit, in both ky forms: no tolerance hides an index error.

Random cases: max-abs error against the fp64 oracle on the same
bf16-rounded inputs, at most twice the error of the forced generic path
(algo 0, generic pack) on the same inputs. Both errors are printed.
"""

import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev():
    return torch.device("cuda:0")


# (id, B, H, W, Cin, Cout, KH, KW, stride)
CASES = [
    # every pixel near an edge; an m-tile spans two images; ragged Cout
    ("edges_2to16_7x7", 2, 11, 37, 2, 16, 7, 7, 1),
    ("stride2_3to64_7x7", 2, 30, 48, 3, 64, 7, 7, 2),
    ("stride2_odd_3to64_7x7", 2, 23, 37, 3, 64, 7, 7, 2),
    ("two_ntiles_2to128_7x7", 2, 24, 40, 2, 128, 7, 7, 1),
    # 406 BM=128 tiles: the other forward tile, with an M tail
    ("bm128_3to64_7x7", 2, 161, 161, 3, 64, 7, 7, 1),
    ("kh1_2to16_1x7", 2, 24, 40, 2, 16, 1, 7, 1),
    ("kw1_2to16_7x1", 2, 24, 40, 2, 16, 7, 1, 1),
    ("kw3_2to16_3x3", 2, 24, 40, 2, 16, 3, 3, 1),
]
IDS = [c[0] for c in CASES]

_cache = {}


def _cl(t):
    return t.to(_dev()).contiguous(memory_format=torch.channels_last)


def _case(case, exact):
    """Inputs as the kernels see them (8 channels, bf16, channels-last) and
    the fp64 CPU oracle with bias, built once and shared."""
    name, B, H, W, Cin, Cout, KH, KW, s = case
    k = (name, exact)
    if k in _cache:
        return _cache[k]
    g = torch.Generator(device="cpu").manual_seed(77 + len(name) + H * W)
    OH = (H + 2 * (KH // 2) - KH) // s + 1
    OW = (W + 2 * (KW // 2) - KW) // s + 1

    def draw(*shape):
        if exact:
            return torch.randint(-1, 2, shape, generator=g).float()
        return (torch.randn(*shape, generator=g) / 4).to(
            torch.bfloat16).float()

    x, w, b, dy = draw(B, Cin, H, W), draw(Cout, Cin, KH, KW), draw(Cout), \
        draw(B, Cout, OH, OW)
    w64 = w.double().requires_grad_()
    b64 = b.double().requires_grad_()
    pad = (KH // 2, KW // 2)
    out = F.conv2d(x.double(), w64, b64, stride=s, padding=pad)
    dw, db = torch.autograd.grad(out, (w64, b64), dy.double())
    out_nb = (out - b64.view(1, -1, 1, 1)).detach()
    x8 = _cl(F.pad(x, (0, 0, 0, 0, 0, 8 - Cin)).to(torch.bfloat16))
    w8 = F.pad(w, (0, 0, 0, 0, 0, 8 - Cin)).to(_dev()).contiguous()
    r = dict(x8=x8, w8=w8, b=b.to(_dev()), dy=_cl(dy.to(torch.bfloat16)),
             out=out.detach(), out_nb=out_nb, dw=dw, db=db)
    _cache[k] = r
    return r


def _fwd(C, case, r, fold, bias):
    _, B, H, W, Cin, Cout, KH, KW, s = case
    wpk = C.conv_gemm_pack(r["w8"], False, fold)
    assert tuple(wpk.shape) == ((KH, Cout, 64) if fold
                                else (KH * KW, Cout, 64))
    out = C.conv_gemm_fwd2(r["x8"], None, wpk, r["b"] if bias else None,
                           Cout, KH, KW, 0, 0, s, s, 0 if s == 1 else 1,
                           0, 0, fold)[0]
    torch.cuda.synchronize()
    return out.double().cpu()


def _wrw(C, case, r, bias, algo, form=-1, nchunk=0):
    _, B, H, W, Cin, Cout, KH, KW, s = case
    dw, db = C.conv_gemm_wrw(r["dy"], r["x8"], None, KH, KW, s, s, bias,
                             algo, nchunk, form)
    torch.cuda.synchronize()
    assert tuple(dw.shape) == (Cout, 8, KH, KW)
    assert not dw[:, Cin:].any()  # the pad channels are zero input
    return dw[:, :Cin].double().cpu(), (db.double().cpu() if bias else None)


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_exact(case, bias):
    import flowhip._C as C
    r = _case(case, True)
    out = _fwd(C, case, r, True, bias)
    assert torch.equal(out, r["out"] if bias else r["out_nb"])
    for form in (0, 1):
        dw, db = _wrw(C, case, r, bias, 2, form)
        assert torch.equal(dw, r["dw"]), form
        if bias:
            assert torch.equal(db, r["db"]), form


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_random_against_generic(case):
    import flowhip._C as C
    name = case[0]
    r = _case(case, False)
    e_g = (_fwd(C, case, r, False, True) - r["out"]).abs().max().item()
    e_f = (_fwd(C, case, r, True, True) - r["out"]).abs().max().item()
    print(f"[conv_fold] {name} fwd max-abs err: generic {e_g:.3e} "
          f"folded {e_f:.3e}")
    assert e_f <= 2.0 * e_g, (e_f, e_g)
    dw_g, db_g = _wrw(C, case, r, True, 0)
    ew_g = (dw_g - r["dw"]).abs().max().item()
    eb_g = (db_g - r["db"]).abs().max().item()
    for form in (0, 1):
        dw, db = _wrw(C, case, r, True, 2, form)
        ew = (dw - r["dw"]).abs().max().item()
        eb = (db - r["db"]).abs().max().item()
        print(f"[conv_fold] {name} form {form} dW max-abs err: generic "
              f"{ew_g:.3e} folded {ew:.3e}; dbias: generic {eb_g:.3e} "
              f"folded {eb:.3e}")
        assert ew <= 2.0 * ew_g, (form, ew, ew_g)
        assert eb <= 2.0 * eb_g, (form, eb, eb_g)


@pytest.mark.parametrize("shape", [(16, 2, 7, 7), (64, 3, 7, 7),
                                   (16, 8, 3, 8), (5, 8, 1, 1)],
                         ids=lambda s: "x".join(map(str, s)))
def test_pack_kernel_matches_torch_equivalent(shape):
    """wpk[ky][o][kx*8+c], zero where kx >= KW or c >= Cin: the kernel and
    the CPU branch of _pack_fwd against the definition."""
    import flowhip._C as C
    from flowhip.ops.functional_conv import _pack_fwd
    O, I, KH, KW = shape
    w = torch.randn(shape, generator=torch.Generator().manual_seed(3))
    want = torch.zeros(KH, O, 8, 8)
    want[:, :, :KW, :I] = w.permute(2, 0, 3, 1)
    want = want.reshape(KH, O, 64).to(torch.bfloat16)
    assert torch.equal(_pack_fwd(w, True), want)
    got = C.conv_gemm_pack(w.to(_dev()), False, True)
    assert torch.equal(got.cpu(), want)


# ---- weight-gradient contract ---------------------------------------------
CONTRACT = CASES[3]  # 2 -> 128 7x7: two N tiles, 30 m-tiles


def _triple():
    """Three (x8, dy) pairs of the contract shape and the fp64 sum of their
    gradients."""
    if "triple" in _cache:
        return _cache["triple"]
    _, B, H, W, Cin, Cout, KH, KW, s = CONTRACT
    g = torch.Generator(device="cpu").manual_seed(4242)
    pairs, dw_sum, db_sum = [], 0, 0
    for _ in range(3):
        x = (torch.randn(B, Cin, H, W, generator=g) / 4).to(torch.bfloat16)
        dy = (torch.randn(B, Cout, H, W, generator=g) / 4).to(torch.bfloat16)
        w64 = torch.zeros(Cout, Cin, KH, KW, dtype=torch.float64,
                          requires_grad=True)
        out = F.conv2d(x.double(), w64, None, padding=(KH // 2, KW // 2))
        dw_sum = dw_sum + torch.autograd.grad(out, w64, dy.double())[0]
        db_sum = db_sum + dy.double().sum((0, 2, 3))
        pairs.append((_cl(F.pad(x, (0, 0, 0, 0, 0, 8 - Cin))), _cl(dy)))
    _cache["triple"] = (pairs, dw_sum, db_sum)
    return _cache["triple"]


def _accumulated(C, form, fill=None, k=3, accumulate=True):
    _, B, H, W, Cin, Cout, KH, KW, s = CONTRACT
    pairs, _, _ = _triple()
    x8, dy = pairs[0]
    path, nchunk, numel, acc = C.conv_gemm_wrw_plan(dy, x8, None, KH, KW, 1,
                                                    1, True, 2, 0, form)
    assert path == 2 and acc == 1
    buf = torch.empty(numel, dtype=torch.float32, device=_dev())
    if fill is not None:
        buf.fill_(fill)
    for i in range(k):
        x8, dy = pairs[i]
        C.conv_gemm_wrw_partials(dy, x8, None, buf, KH, KW, 1, 1, True,
                                 accumulate and i > 0, 2, nchunk, form)
    dw, db = C.conv_gemm_wrw_finish(buf, Cout, 8, KH, KW, True, nchunk,
                                    None, None, 2)
    torch.cuda.synchronize()
    return dw[:, :Cin].double().cpu(), db.double().cpu()


@pytest.mark.parametrize("form", [0, 1])
def test_accumulating_calls_equal_sum_of_one_shots(form):
    import flowhip._C as C
    _, B, H, W, Cin, Cout, KH, KW, s = CONTRACT
    pairs, dw_ref, db_ref = _triple()
    dw_a, db_a = _accumulated(C, form)
    dw_s, db_s = 0, 0
    for x8, dy in pairs:
        dw, db = C.conv_gemm_wrw(dy, x8, None, KH, KW, 1, 1, True, 2, 0, form)
        dw_s, db_s = dw_s + dw[:, :Cin], db_s + db  # fp32, as autograd adds
    e_a = (dw_a - dw_ref).abs().max().item()
    e_s = (dw_s.double().cpu() - dw_ref).abs().max().item()
    b_a = (db_a - db_ref).abs().max().item()
    b_s = (db_s.double().cpu() - db_ref).abs().max().item()
    print(f"[conv_fold] form {form} dW err: one-shot sum {e_s:.3e} "
          f"accumulated {e_a:.3e}; dbias: {b_s:.3e} / {b_a:.3e}")
    assert e_a <= 2.0 * e_s and b_a <= 2.0 * b_s


@pytest.mark.parametrize("form", [0, 1])
def test_overwrite_ignores_buffer_contents(form):
    import flowhip._C as C
    dw_n, db_n = _accumulated(C, form, fill=float("nan"), k=1)
    dw_z, db_z = _accumulated(C, form, fill=0.0, k=1)
    assert torch.isfinite(dw_n).all() and torch.isfinite(db_n).all()
    assert torch.equal(dw_n, dw_z) and torch.equal(db_n, db_z)


def test_dw_into_adds_in_place():
    import flowhip._C as C
    _, B, H, W, Cin, Cout, KH, KW, s = CONTRACT
    (x8, dy), = _triple()[0][:1]
    path, nchunk, numel, _ = C.conv_gemm_wrw_plan(dy, x8, None, KH, KW, 1, 1,
                                                  True)
    assert path == 2  # auto, inside the envelope
    buf = torch.empty(numel, dtype=torch.float32, device=_dev())
    C.conv_gemm_wrw_partials(dy, x8, None, buf, KH, KW, 1, 1, True, False,
                             path, nchunk)
    dw, db = C.conv_gemm_wrw_finish(buf, Cout, 8, KH, KW, True, nchunk, None,
                                    None, path)
    run_w = torch.full_like(dw, 1.5)
    run_b = torch.full_like(db, -2.0)
    dw2, db2 = C.conv_gemm_wrw_finish(buf, Cout, 8, KH, KW, True, nchunk,
                                      run_w, run_b, path)
    assert dw2.data_ptr() == run_w.data_ptr()
    assert torch.equal(run_w, dw + 1.5) and torch.equal(run_b, db - 2.0)


@pytest.mark.parametrize("form", [0, 1])
def test_forced_chunk_counts(form):
    """One chunk, and a request above the m-tile count, which is clamped."""
    import flowhip._C as C
    _, B, H, W, Cin, Cout, KH, KW, s = CONTRACT
    r = _case(CONTRACT, True)
    mtiles = (B * H * W + 63) // 64
    plan = C.conv_gemm_wrw_plan(r["dy"], r["x8"], None, KH, KW, 1, 1, True,
                                2, 10 ** 6, form)
    assert plan[0] == 2 and plan[1] == mtiles
    for nchunk in (1, 10 ** 6):
        dw, db = _wrw(C, CONTRACT, r, True, 2, form, nchunk)
        assert torch.equal(dw, r["dw"]) and torch.equal(db, r["db"])


def test_wrong_plan_is_refused():
    import flowhip._C as C
    _, B, H, W, Cin, Cout, KH, KW, s = CONTRACT
    r = _case(CONTRACT, True)
    x8, dy = r["x8"], r["dy"]
    path, nchunk, numel, _ = C.conv_gemm_wrw_plan(dy, x8, None, KH, KW, 1, 1,
                                                  True, 2)
    buf = torch.empty(numel, dtype=torch.float32, device=_dev())
    mtiles = (B * H * W + 63) // 64
    with pytest.raises(RuntimeError):  # a chunk count the plan would clamp
        C.conv_gemm_wrw_partials(dy, x8, None, buf, KH, KW, 1, 1, True,
                                 False, 2, mtiles + 1)
    with pytest.raises(RuntimeError):  # the folded buffer on another path
        C.conv_gemm_wrw_partials(dy, x8, None, buf, KH, KW, 1, 1, True,
                                 False, 0, nchunk)
    with pytest.raises(RuntimeError):  # and in the generic reduce
        C.conv_gemm_wrw_finish(buf, Cout, 8, KH, KW, True, nchunk, None, None,
                               0)
    with pytest.raises(RuntimeError):  # short buffer
        C.conv_gemm_wrw_partials(dy, x8, None, buf[:-1], KH, KW, 1, 1, True,
                                 False, 2, nchunk)


def test_outside_the_envelope_raises():
    import flowhip._C as C
    g = torch.Generator(device="cpu").manual_seed(5)
    x16 = _cl(torch.randn(2, 16, 11, 37, generator=g).to(torch.bfloat16))
    x8 = _cl(torch.randn(2, 8, 11, 37, generator=g).to(torch.bfloat16))
    dy = _cl(torch.randn(2, 16, 11, 37, generator=g).to(torch.bfloat16))
    with pytest.raises(RuntimeError):  # Cin != 8
        C.conv_gemm_wrw(dy, x16, None, 7, 7, 1, 1, False, 2)
    with pytest.raises(RuntimeError):  # a second source
        C.conv_gemm_wrw(dy, x8, x8, 7, 7, 1, 1, False, 2)
    w16 = torch.zeros(16, 16, 7, 7, device=_dev())
    with pytest.raises(RuntimeError):  # no folded pack of 16 channels
        C.conv_gemm_pack(w16, False, True)
    w8 = torch.zeros(16, 8, 7, 7, device=_dev())
    wpk = C.conv_gemm_pack(w8, False, True)
    with pytest.raises(RuntimeError):  # a folded pack on 16 input channels
        C.conv_gemm_fwd2(x16, None, wpk, None, 16, 7, 7, 0, 0, 1, 1, 0, 0, 0,
                         True)
    with pytest.raises(RuntimeError):  # a folded pack not announced
        C.conv_gemm_fwd2(x8, None, wpk, None, 16, 7, 7, 0, 0)


# ---- public path ----------------------------------------------------------
PUBLIC = [
    # (id, B, H, W, Cin, Cout, stride): the stem and convf1 layers
    ("stem", 2, 30, 48, 3, 64, 2),
    ("convf1", 2, 24, 40, 2, 128, 1),
]


@pytest.mark.parametrize("pub", PUBLIC, ids=[p[0] for p in PUBLIC])
def test_fused_conv2d_takes_the_folded_kernels(pub):
    import flowhip._C as C
    from flowhip.ops.functional_conv import fused_conv2d
    name, B, H, W, Cin, Cout, s = pub
    g = torch.Generator(device="cpu").manual_seed(11)
    x = _cl((torch.randn(B, Cin, H, W, generator=g) / 4).to(torch.bfloat16))
    w = (torch.randn(Cout, Cin, 7, 7, generator=g) / 8).to(
        _dev()).requires_grad_()
    b = torch.randn(Cout, generator=g).to(_dev()).requires_grad_()
    cache = {}
    out = fused_conv2d(x, w, b, s, 3, 1, 1, cache)
    assert cache["fold"] is True and tuple(cache["fwd"].shape) == (7, Cout, 64)
    dy = _cl((torch.randn(out.shape, generator=g) / 4).to(torch.bfloat16))
    out.backward(dy)
    # the same kernels called directly, bit for bit (they are deterministic)
    x8 = _cl(F.pad(x, (0, 0, 0, 0, 0, 8 - Cin)))
    w8 = F.pad(w.detach(), (0, 0, 0, 0, 0, 8 - Cin)).contiguous()
    assert C.conv_gemm_wrw_plan(dy, x8, None, 7, 7, s, s, True)[0] == 2
    o2 = C.conv_gemm_fwd2(x8, None, C.conv_gemm_pack(w8, False, True),
                          b.detach(), Cout, 7, 7, 0, 0, s, s,
                          0 if s == 1 else 1, 0, 0, True)[0]
    dw2, db2 = C.conv_gemm_wrw(dy, x8, None, 7, 7, s, s, True, 2)
    assert torch.equal(out.detach(), o2)
    assert torch.equal(w.grad, dw2[:, :Cin]) and torch.equal(b.grad, db2)
    ref = F.conv2d(x.double(), w.detach().to(torch.bfloat16).double(),
                   b.detach().double(), stride=s, padding=3)
    torch.testing.assert_close(out.detach().double(), ref, atol=1e-1,
                               rtol=5e-2)


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import torch
import flowhip._C as C
from flowhip.ops.functional_conv import fused_conv2d
dev = torch.device("cuda:0")
x = torch.randn(2, 2, 24, 40, device=dev).to(torch.bfloat16).contiguous(
    memory_format=torch.channels_last)
w = torch.randn(16, 2, 7, 7, device=dev, requires_grad=True)
cache = {}
out = fused_conv2d(x, w, None, 1, 3, 1, 1, cache)
out.sum().backward()
x8 = torch.nn.functional.pad(x, (0, 0, 0, 0, 0, 6)).contiguous(
    memory_format=torch.channels_last)
dy = torch.ones_like(out)
path = C.conv_gemm_wrw_plan(dy, x8, None, 7, 7, 1, 1, False)[0]
torch.cuda.synchronize()
print("FOLD", cache["fold"], tuple(cache["fwd"].shape), path,
      bool(torch.isfinite(w.grad).all()))
"""


def test_switch_off_takes_todays_path():
    env = dict(os.environ, FLOWHIP_CONV_FOLD="0")
    run = subprocess.run([sys.executable, "-c", _CHILD, REPO], env=env,
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-3000:]
    assert "FOLD False (49, 16, 64) 0 True" in run.stdout, run.stdout


def test_accumulate_scope_matches_scope_off():
    from flowhip.ops.functional_conv import (fused_conv2d,
                                             wrw_accumulate_scope)
    _, B, H, W, Cin, Cout, KH, KW, s = CONTRACT
    pairs, dw_ref, db_ref = _triple()
    g = torch.Generator(device="cpu").manual_seed(12)
    w0 = (torch.randn(Cout, Cin, KH, KW, generator=g) / 8).to(_dev())
    b0 = torch.randn(Cout, generator=g).to(_dev())

    def grads(scope):
        w = w0.clone().requires_grad_()
        b = b0.clone().requires_grad_()
        cache = {}
        ctx = wrw_accumulate_scope() if scope else torch.enable_grad()
        with ctx:
            loss = 0
            for x8, dy in pairs:
                out = fused_conv2d(x8[:, :Cin].contiguous(
                    memory_format=torch.channels_last), w, b, 1, 3, 1, 1,
                    cache)
                assert cache["fold"] is True
                loss = loss + (out.float() * dy.float()).sum()
        loss.backward()
        torch.cuda.synchronize()
        return w.grad.double().cpu(), b.grad.double().cpu()

    dw_on, db_on = grads(True)
    dw_off, db_off = grads(False)
    e_on = (dw_on - dw_ref).abs().max().item()
    e_off = (dw_off - dw_ref).abs().max().item()
    b_on = (db_on - db_ref).abs().max().item()
    b_off = (db_off - db_ref).abs().max().item()
    print(f"[conv_fold] scope dW err: off {e_off:.3e} on {e_on:.3e}; "
          f"dbias: off {b_off:.3e} on {b_on:.3e}")
    assert e_on <= 2.0 * e_off and b_on <= 2.0 * b_off


def test_folded_forward_replays_in_a_graph():
    import flowhip._C as C
    case = CASES[1]
    _, B, H, W, Cin, Cout, KH, KW, s = case
    r = _case(case, False)
    wpk = C.conv_gemm_pack(r["w8"], False, True)

    def run():
        return C.conv_gemm_fwd2(r["x8"], None, wpk, r["b"], Cout, KH, KW, 0,
                                0, s, s, 1, 0, 0, True)[0]

    eager = run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
