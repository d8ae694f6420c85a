"""Fused normalized-convolution backward (csrc/nconv_bwd_fused.hip) against
the split kernels and an fp64 reference.

The reference is the fp64 autograd gradient of torch_ref.nconv2d on the
same inputs, computed on the CPU. Per case and per result (ddata, dconf,
dweight, dbias) the split path's (algo=0) max-abs error against it is
measured, and the fused path's (algo=1) error must be at most twice that:
the margin covers a different summation order only. The project's NConv
bound (TestNConv.test_backward_matches_ref: atol=1e-3, rtol=1e-3) applies
on top as an absolute cap. Both errors are printed.

Shapes (N=2): 5x8 is smaller than a tile and than the 5x5 halo reach, so
every staged chunk crosses an image edge; 19x68 has a 4-wide tile tail in x
and a 3-row tail in y; 37x132 has three tile columns and three tile rows
(forced strip lengths 1 and 2 give several strips with a ragged last one);
18x22 has W % 4 != 0 and must take the split kernels through algo=-1.
"""

import os

import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 1e-20


def _dev():
    return torch.device("cuda:0")


# (Ci, Co, K, bias)
LAYERS = [(1, 2, 5, False), (2, 2, 5, False), (4, 2, 3, False),
          (2, 2, 3, False), (2, 1, 1, False), (2, 2, 3, True)]
SHAPES = [(5, 8), (19, 68), (37, 132), (18, 22)]
# zero_inject at scale 4, offset 2: samples at rows / columns 2, 6, 10, ...
# Only shapes where every 5x5 window, edge windows included, holds a sample
# (at 18x22 the windows of rows 17 and column 21 hold none).
INJECT_SHAPES = [(5, 8), (19, 68), (37, 132)]

CASES = [(ci, co, k, b, h, w, False)
         for (ci, co, k, b) in LAYERS for (h, w) in SHAPES] + \
        [(1, 2, 5, False, h, w, True) for (h, w) in INJECT_SHAPES] + \
        [(4, 4, 5, False, 19, 68, False)]  # accumulators in 4 co groups


def _id(c):
    ci, co, k, b, h, w, inj = c
    return f"{ci}to{co}_k{k}{'_bias' if b else ''}_{h}x{w}{'_inject' if inj else ''}"


_cache = {}


def _case(case):
    """Inputs, the kernel's own forward outputs and the fp64 gradients with
    and without gcout, built once per case."""
    if case in _cache:
        return _cache[case]
    from flowhip.ops import torch_ref
    import flowhip._C as C
    ci, co, k, has_bias, H, W, inject = case
    N = 2
    g = torch.Generator(device="cpu").manual_seed(
        7000 + 131 * ci + 17 * co + 5 * k + H * W + int(has_bias) + 2 * int(inject))
    data = torch.randn(N, ci, H, W, generator=g)
    conf = 0.1 + 0.9 * torch.rand(N, ci, H, W, generator=g)
    if inject:
        m = torch.zeros(H, W)
        m[2::4, 2::4] = 1.0
        data = data * m
        conf = conf * m
    weight = torch.rand(co, ci, k, k, generator=g) + 0.05
    bias = torch.randn(co, generator=g) if has_bias else None
    gout = torch.randn(N, co, H, W, generator=g)
    gcout = torch.randn(N, co, H, W, generator=g)

    refs = {}
    for with_gcout in (True, False):
        leaves = [t.double().requires_grad_(True)
                  for t in (data, conf, weight)]
        b64 = bias.double().requires_grad_(True) if has_bias else None
        rout, rcout = torch_ref.nconv2d(leaves[0], leaves[1], leaves[2], b64,
                                        1, k // 2, 1, 1, EPS, True)
        assert (rcout > 0).all(), "a window without samples: no reference"
        outs, grads = [rout], [gout.double()]
        if with_gcout:
            outs.append(rcout)
            grads.append(gcout.double())
        wrt = leaves + ([b64] if has_bias else [])
        r = torch.autograd.grad(outs, wrt, grads)
        refs[with_gcout] = dict(ddata=r[0], dconf=r[1], dweight=r[2],
                                dbias=r[3] if has_bias else None)

    dv = _dev()
    t = dict(data=data.to(dv), conf=conf.to(dv), weight=weight.to(dv),
             bias=bias.to(dv) if has_bias else None, gout=gout.to(dv),
             gcout=gcout.to(dv))
    t["out"], t["cout"] = C.nconv_fwd(t["data"], t["conf"], t["weight"],
                                      t["bias"])
    _cache[case] = (t, refs)
    return _cache[case]


def _run(t, with_gcout, algo, strip=0, gout=True):
    import flowhip._C as C
    r = C.nconv_bwd_fused(t["gout"] if gout else None,
                          t["gcout"] if with_gcout else None, t["out"],
                          t["cout"], t["data"], t["conf"], t["weight"],
                          t["bias"], EPS, algo, strip)
    torch.cuda.synchronize()
    return dict(ddata=r[0], dconf=r[1], dweight=r[2],
                dbias=r[3] if t["bias"] is not None else None)


@pytest.mark.parametrize("with_gcout", [True, False], ids=["gcout", "nogcout"])
@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_fused_vs_split_vs_fp64(case, with_gcout):
    ci, co, k, has_bias, H, W, inject = case
    t, refs = _case(case)
    ref = refs[with_gcout]
    fusable = W % 4 == 0
    split = _run(t, with_gcout, 0)
    # outside the envelope the automatic rule must take the split kernels
    fused = _run(t, with_gcout, 1 if fusable else -1)
    for name in ("ddata", "dconf", "dweight", "dbias"):
        if ref[name] is None:
            continue
        r = ref[name]
        s = split[name].double().cpu()
        f = fused[name].double().cpu()
        err_s = (s - r).abs().max().item()
        err_f = (f - r).abs().max().item()
        print(f"[nconv_bwd_fused] {_id(case)} "
              f"{'gcout' if with_gcout else 'nogcout'} {name} max-abs err: "
              f"split {err_s:.3e} fused {err_f:.3e}")
        assert torch.isfinite(f).all()
        # Outside the envelope both runs are the same untiled kernels, whose
        # weight gradient sums with float atomics: its error differs from
        # run to run by more than 2x, so the ratio rule (a rule about the
        # fused kernel's summation order) is applied where that kernel runs.
        if fusable or name != "dweight":
            assert err_f <= 2.0 * err_s, (name, err_f, err_s)
        torch.testing.assert_close(f, r, atol=1e-3, rtol=1e-3)
    if not fusable:
        for name in ("ddata", "dconf"):  # the gathers repeat bit for bit
            assert torch.equal(fused[name], split[name])
        with pytest.raises(RuntimeError):
            _run(t, with_gcout, 1)


@pytest.mark.parametrize("strip", [1, 2, 3])
@pytest.mark.parametrize("layer", [(2, 2, 5, False), (2, 2, 3, True),
                                   (4, 2, 3, False)],
                         ids=["2to2_k5", "2to2_k3_bias", "4to2_k3"])
def test_forced_strip_lengths(layer, strip):
    """Every strip length (3 strips of 1 tile row, 2 ragged strips, 1 strip
    of all 3) gives the same results up to fp32 summation order, and the
    same ddata / dconf bit for bit."""
    case = layer + (37, 132, False)
    t, refs = _case(case)
    base = _run(t, True, 1, 0)
    got = _run(t, True, 1, strip)
    assert torch.equal(got["ddata"], base["ddata"])
    assert torch.equal(got["dconf"], base["dconf"])
    for name in ("dweight", "dbias"):
        if refs[True][name] is not None:
            torch.testing.assert_close(got[name].double().cpu(),
                                       refs[True][name], atol=1e-3, rtol=1e-3)


def test_gout_absent_is_zero_gout():
    """gout=None (only cout used downstream) equals an all-zero gout."""
    case = (2, 2, 3, True, 19, 68, False)
    t, _ = _case(case)
    got = _run(t, True, 1, gout=False)
    tz = dict(t, gout=torch.zeros_like(t["gout"]))
    want = _run(tz, True, 1)
    for name in ("ddata", "dconf", "dweight", "dbias"):
        assert torch.equal(got[name], want[name]), name
    split = _run(t, True, 0, gout=False)
    for name in ("ddata", "dconf", "dweight", "dbias"):
        torch.testing.assert_close(got[name], split[name], atol=1e-3,
                                   rtol=1e-3)


@pytest.mark.parametrize("layer", [(2, 2, 5, False), (2, 2, 3, True)],
                         ids=["2to2_k5", "2to2_k3_bias"])
def test_fused_is_deterministic(layer):
    case = layer + (37, 132, False)
    t, _ = _case(case)
    a = _run(t, True, 1)
    b = _run(t, True, 1)
    for name in a:
        if a[name] is not None:
            assert torch.equal(a[name], b[name]), name


@pytest.mark.parametrize("use_cout", [False, True], ids=["out", "out_cout"])
@pytest.mark.parametrize("nds", [1, 2])
def test_unet_hip_matches_ref_path(nds, use_cout):
    """Whole NConvUNet, shipped config (and num_downsampling=2, where the
    folded stage 0 sits next to a real 2x decoder stage), forward and
    backward: HIP path against FLOWHIP_FORCE_REF=1. With use_cout=False the
    net's cout is dropped, as in the NCUP head, and nconv_out's backward
    receives gcout=None."""
    from flowhip.nn.nconv import NConvUNet
    torch.manual_seed(10)
    net = NConvUNet(in_ch=1, channels_multiplier=2, num_downsampling=nds,
                    encoder_filter_sz=5, decoder_filter_sz=3,
                    out_filter_sz=1, use_bias=False,
                    data_pooling="conf_based", shared_encoder=True,
                    use_double_conv=False).to(_dev())
    data = torch.randn(4, 1, 64, 64, device=_dev())
    conf = torch.rand(4, 1, 64, 64, device=_dev())
    g1 = torch.randn(4, 1, 64, 64, device=_dev())
    g2 = torch.randn(4, 1, 64, 64, device=_dev())
    params = [p for p in net.parameters()]

    def run():
        d = data.clone().requires_grad_(True)
        c = conf.clone().requires_grad_(True)
        out, cout = net((d, c))
        outs, gs = [out], [g1]
        if use_cout:
            outs.append(cout)
            gs.append(g2)
        grads = torch.autograd.grad(outs, [d, c] + params, gs)
        return out.detach(), cout.detach(), grads

    out, cout, grads = run()
    os.environ["FLOWHIP_FORCE_REF"] = "1"
    try:
        rout, rcout, rgrads = run()
    finally:
        del os.environ["FLOWHIP_FORCE_REF"]
    torch.testing.assert_close(out, rout, atol=1e-4, rtol=1e-4)
    torch.testing.assert_close(cout, rcout, atol=1e-4, rtol=1e-4)
    for a, b in zip(grads, rgrads):
        torch.testing.assert_close(a, b, atol=1e-3, rtol=1e-3)
