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
18x22 has W % 4 != 0: the bindings refuse it, and run it zero-padded to
18x24 with zero upstream gradient in the pad columns, which is the same
problem in columns [0, 22) (asserted on the fp64 reference before anything
runs on the GPU).

Further down: NConv2dFn at unaligned widths (it pads and slices), an
off-table layer through ops.nconv2d (torch path, with a warning), and
FLOWHIP_NCONV_BWD=split.
"""

import os
import warnings

import pytest
import torch
import torch.nn.functional as F

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


def _ref64(data, conf, weight, bias, gout, gcout, k, need_samples=True):
    """fp64 outputs and gradients of torch_ref.nconv2d on the CPU, with and
    without gcout."""
    from flowhip.ops import torch_ref
    refs = {}
    for with_gcout in (True, False):
        leaves = [t.double().requires_grad_(True)
                  for t in (data, conf, weight)]
        b64 = bias.double().requires_grad_(True) if bias is not None else None
        rout, rcout = torch_ref.nconv2d(leaves[0], leaves[1], leaves[2], b64,
                                        1, k // 2, 1, 1, EPS, True)
        if need_samples:
            assert (rcout > 0).all(), "a window without samples: no reference"
        outs, grads = [rout], [gout.double()]
        if with_gcout:
            outs.append(rcout)
            grads.append(gcout.double())
        wrt = leaves + ([b64] if bias is not None else [])
        r = torch.autograd.grad(outs, wrt, grads)
        refs[with_gcout] = dict(out=rout.detach(), cout=rcout.detach(),
                                ddata=r[0], dconf=r[1], dweight=r[2],
                                dbias=r[3] if bias is not None else None)
    return refs


def _rpad(t, pad):
    """t with `pad` zero columns appended on the right."""
    return F.pad(t, (0, pad)) if pad else t


def _case(case):
    """Inputs (right-padded with zero columns to W % 4 == 0), the kernel's
    own forward outputs on them and the fp64 gradients of the unpadded
    problem with and without gcout, built once per case."""
    if case in _cache:
        return _cache[case]
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

    refs = _ref64(data, conf, weight, bias, gout, gcout, k)
    pad = -W % 4
    if pad:
        # on the CPU, before the GPU sees the padded problem: it is the
        # unpadded one in columns [0, W)
        data, conf, gout, gcout = (_rpad(t, pad)
                                   for t in (data, conf, gout, gcout))
        prefs = _ref64(data, conf, weight, bias, gout, gcout, k,
                       need_samples=False)
        for with_gcout in (True, False):
            for name, r in refs[with_gcout].items():
                if r is None:
                    continue
                pr = prefs[with_gcout][name]
                assert torch.isfinite(pr).all(), name
                if name not in ("dweight", "dbias"):
                    pr = pr[..., :W]
                assert (pr - r).abs().max().item() <= 1e-10, name

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
    split = _run(t, with_gcout, 0)
    fused = _run(t, with_gcout, 1)
    for name in ("ddata", "dconf", "dweight", "dbias"):
        if ref[name] is None:
            continue
        r = ref[name]
        s = split[name].double().cpu()
        f = fused[name].double().cpu()
        if name in ("ddata", "dconf"):  # the image's columns of a padded run
            s, f = s[..., :W], f[..., :W]
        err_s = (s - r).abs().max().item()
        err_f = (f - r).abs().max().item()
        print(f"[nconv_bwd_fused] {_id(case)} "
              f"{'gcout' if with_gcout else 'nogcout'} {name} max-abs err: "
              f"split {err_s:.3e} fused {err_f:.3e}")
        assert torch.isfinite(f).all()
        assert err_f <= 2.0 * err_s, (name, err_f, err_s)
        torch.testing.assert_close(f, r, atol=1e-3, rtol=1e-3)
    if W % 4:
        # the unpadded planes themselves are outside every binding's envelope
        import flowhip._C as C
        u = {n: (v[..., :W].contiguous()
                 if v is not None and v.dim() == 4 and n != "weight" else v)
             for n, v in t.items()}
        for algo in (-1, 0, 1):
            with pytest.raises(RuntimeError):
                _run(u, with_gcout, algo)
        with pytest.raises(RuntimeError):
            C.nconv_fwd(u["data"], u["conf"], u["weight"], u["bias"])


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


UNALIGNED_SIZES = [(7, 3), (5, 9), (18, 22), (6, 65)]
UNALIGNED_LAYERS = [(1, 2, 5, False), (2, 2, 3, True), (2, 1, 1, False)]


@pytest.mark.parametrize("use_cout", [True, False], ids=["out_cout", "out"])
@pytest.mark.parametrize("layer", UNALIGNED_LAYERS,
                         ids=["1to2_k5", "2to2_k3_bias", "2to1_k1"])
@pytest.mark.parametrize("size", UNALIGNED_SIZES,
                         ids=[f"{h}x{w}" for h, w in UNALIGNED_SIZES])
def test_function_pads_unaligned_widths(size, layer, use_cout):
    """NConv2dFn at W % 4 != 0 (W = 3 is narrower than one float4 chunk, 65
    pads into a second tile column): outputs and gradients are, bit for bit,
    the bindings' on the zero-padded planes, sliced; contiguous, of the
    unpadded shape, and within the NConv cap of fp64."""
    import flowhip._C as C
    from flowhip.ops.functional_nconv import NConv2dFn
    (H, W), (ci, co, k, has_bias) = size, layer
    N, pad, dv = 2, -W % 4, _dev()
    g = torch.Generator(device="cpu").manual_seed(9100 + 7 * H * W + 31 * ci + k)
    data = torch.randn(N, ci, H, W, generator=g)
    conf = 0.1 + 0.9 * torch.rand(N, ci, H, W, generator=g)
    weight = torch.rand(co, ci, k, k, generator=g) + 0.05
    bias = torch.randn(co, generator=g) if has_bias else None
    gout = torch.randn(N, co, H, W, generator=g)
    gcout = torch.randn(N, co, H, W, generator=g)
    ref = _ref64(data, conf, weight, bias, gout, gcout, k)[use_cout]

    leaves = [x.to(dv).requires_grad_(True) for x in (data, conf, weight)]
    if has_bias:
        leaves.append(bias.to(dv).requires_grad_(True))
    out, cout = NConv2dFn.apply(leaves[0], leaves[1], leaves[2],
                                leaves[3] if has_bias else None, k // 2, EPS,
                                True)
    outs, gs = [out], [gout.to(dv)]
    if use_cout:
        outs.append(cout)
        gs.append(gcout.to(dv))
    grads = torch.autograd.grad(outs, leaves, gs)
    got = dict(out=out.detach(), cout=cout.detach(), ddata=grads[0],
               dconf=grads[1], dweight=grads[2],
               dbias=grads[3] if has_bias else None)

    pd, pc = (_rpad(x, pad).to(dv) for x in (data, conf))
    wd = weight.to(dv)
    bd = bias.to(dv) if has_bias else None
    pout, pcout = C.nconv_fwd(pd, pc, wd, bd)
    r = C.nconv_bwd_fused(_rpad(gout, pad).to(dv),
                          _rpad(gcout, pad).to(dv) if use_cout else None,
                          pout, pcout, pd, pc, wd, bd, EPS, -1)
    want = dict(out=pout[..., :W], cout=pcout[..., :W], ddata=r[0][..., :W],
                dconf=r[1][..., :W], dweight=r[2],
                dbias=r[3] if has_bias else None)
    for name, w in want.items():
        if w is None:
            continue
        assert got[name].shape == ref[name].shape, name
        assert got[name].is_contiguous(), name
        assert torch.equal(got[name], w), name
        torch.testing.assert_close(got[name].double().cpu(), ref[name],
                                   atol=1e-3, rtol=1e-3)


def test_off_table_layer_takes_torch_path_with_warning():
    """(Ci, Co, K) = (3, 2, 3) is in no kernel table (its weight gradient
    used to abort): ops.nconv2d says so and runs torch_ref, forward and
    backward."""
    from flowhip import ops
    from flowhip.ops import torch_ref
    dv = _dev()
    g = torch.Generator(device="cpu").manual_seed(9300)
    data = torch.randn(2, 3, 12, 16, generator=g).to(dv).requires_grad_(True)
    conf = (0.1 + 0.9 * torch.rand(2, 3, 12, 16, generator=g)).to(
        dv).requires_grad_(True)
    weight = (torch.rand(2, 3, 3, 3, generator=g) + 0.05).to(
        dv).requires_grad_(True)
    g1 = torch.randn(2, 2, 12, 16, generator=g).to(dv)
    g2 = torch.randn(2, 2, 12, 16, generator=g).to(dv)
    assert not ops.nconv2d_uses_hip(data, conf, weight, 1, 1, 1, 1, EPS, True)
    # an in-table layer with the same arguments does, without a warning
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert ops.nconv2d_uses_hip(data[:, :2], conf[:, :2], weight[:, :2],
                                    1, 1, 1, 1, EPS, True)
    with pytest.warns(UserWarning, match=r"\(3, 2, 3\)"):
        out, cout = ops.nconv2d(data, conf, weight, None, 1, 1, 1, 1, EPS,
                                True)
    grads = torch.autograd.grad((out, cout), (data, conf, weight), (g1, g2))
    rl = [x.detach().clone().requires_grad_(True)
          for x in (data, conf, weight)]
    rout, rcout = torch_ref.nconv2d(rl[0], rl[1], rl[2], None, 1, 1, 1, 1,
                                    EPS, True)
    rgrads = torch.autograd.grad((rout, rcout), rl, (g1, g2))
    torch.testing.assert_close(out, rout, atol=1e-4, rtol=1e-4)
    torch.testing.assert_close(cout, rcout, atol=1e-4, rtol=1e-4)
    for a, b in zip(grads, rgrads):
        torch.testing.assert_close(a, b, atol=1e-3, rtol=1e-3)


def test_split_env_var_runs_the_binding_algo0():
    """FLOWHIP_NCONV_BWD=split makes NConv2dFn.backward run exactly
    nconv_bwd_fused(algo=0), the split path the tests above measure: all
    four gradients equal the binding's bit for bit. (The split path repeats
    bit for bit: its plane sums add in a fixed order.)"""
    from flowhip.ops.functional_nconv import NConv2dFn
    case = (2, 2, 3, True, 19, 68, False)
    t, _ = _case(case)
    want = _run(t, True, 0)
    leaves = [t[n].detach().clone().requires_grad_(True)
              for n in ("data", "conf", "weight", "bias")]
    out, cout = NConv2dFn.apply(leaves[0], leaves[1], leaves[2], leaves[3],
                                1, EPS, True)
    old = os.environ.get("FLOWHIP_NCONV_BWD")
    os.environ["FLOWHIP_NCONV_BWD"] = "split"
    try:
        grads = torch.autograd.grad((out, cout), leaves,
                                    (t["gout"], t["gcout"]))
    finally:
        if old is None:
            del os.environ["FLOWHIP_NCONV_BWD"]
        else:
            os.environ["FLOWHIP_NCONV_BWD"] = old
    names = ("ddata", "dconf", "dweight", "dbias")
    for got, name in zip(grads, names):
        d = (got.double() - want[name].double()).abs().max().item()
        print(f"[nconv_bwd_split_env] {name} max-abs diff to algo=0: {d:.3e}")
    for got, name in zip(grads, names):
        assert torch.equal(got, want[name]), name


def test_split_is_deterministic():
    """algo=0 with bias and gcout, so that both plane sums run (dbias and
    the sum(cout * gcout) term of dweight), ten block sums per channel."""
    t, _ = _case((2, 2, 3, True, 37, 132, False))
    a = _run(t, True, 0)
    for _ in range(5):
        b = _run(t, True, 0)
        for name in a:
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
