"""GPU: the forward-backward consistency HIP kernel against its float64
twin, the bidirectional forward against two separate calls on the device, and
the graphed bidirectional stream (consistency check inside the hipGraph)
against the eager one."""

import functools

import pytest
import torch

from flowhip import ops
from flowhip.config.args import default_ncup_args
from flowhip.models import build_model
from flowhip.ops import torch_ref

from fb_cases import FB_INPUTS, bits_equal, fb_input

pytestmark = pytest.mark.gpu

# one partly filled workgroup; two workgroups, rows that straddle them; many
# workgroups with a partly filled last one
SHAPES = [(1, 5, 7), (2, 17, 23), (1, 55, 128)]


def _dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _oracle(name, N, H, W):
    """CPU float64 twin and its decision margin, computed once per input and
    shared (read-only)."""
    return torch_ref.fb_consistency(*fb_input(name, N, H, W),
                                    return_margin=True)


def _check_against_oracle(got, want, N, H, W):
    occ_fw, occ_bw, res_fw, res_bw, stats = (t.cpu() for t in got)
    assert occ_fw.dtype == torch.uint8 and occ_fw.shape == (N, 1, H, W)
    assert res_fw.dtype == torch.float32 and res_fw.shape == (N, 1, H, W)
    assert stats.dtype == torch.float64 and stats.shape == (N, 2, 4)
    assert torch.equal(occ_fw, want[0]) and torch.equal(occ_bw, want[1])
    for res, ref in [(res_fw, want[2]), (res_bw, want[3])]:
        assert not torch.isnan(res).any() and not torch.isnan(ref).any()
        inf = torch.isinf(ref)
        assert torch.equal(torch.isinf(res), inf)
        assert (res[inf] == ref[inf]).all()              # all +inf
        ulps = (res.view(torch.int32)[~inf].long()
                - ref.view(torch.int32)[~inf].long()).abs()
        # every pixel is either compared as an infinity or in ulps
        assert int(inf.sum()) + ulps.numel() == N * H * W
        print(f"  res: {ulps.numel()} finite, max ulp diff "
              f"{int(ulps.max()) if ulps.numel() else 0}")
        assert (ulps <= 1).all()
    assert torch.equal(stats[..., :3], want[4][..., :3])
    assert (stats[..., :3].sum(-1) == H * W).all()
    err = (stats[..., 3] - want[4][..., 3]).abs()
    assert (err <= 1e-10 * want[4][..., 3].abs()).all()


@pytest.mark.parametrize("name", FB_INPUTS)
@pytest.mark.parametrize("N,H,W", SHAPES)
def test_kernel_matches_twin(N, H, W, name):
    want = _oracle(name, N, H, W)
    margin = want[5].item()
    print(f"{name} {(N, H, W)}: oracle min |r2 - thr| {margin:.3g}")
    assert margin >= 1e-9      # no decision within fp64 rounding of thr
    f, b = fb_input(name, N, H, W)
    got = ops.fb_consistency(f.to(_dev()), b.to(_dev()))
    assert all(t.is_cuda and not t.requires_grad for t in got)
    _check_against_oracle(got, want, N, H, W)


def test_thresholds_reach_the_kernel():
    f, b = fb_input("smooth", 2, 17, 23)
    want = torch_ref.fb_consistency(f, b, 0.05, 0.1, return_margin=True)
    assert want[5].item() >= 1e-9
    assert not torch.equal(want[0], _oracle("smooth", 2, 17, 23)[0])
    got = ops.fb_consistency(f.to(_dev()), b.to(_dev()), alpha1=0.05,
                             alpha2=0.1)
    _check_against_oracle(got, want, 2, 17, 23)


@pytest.mark.parametrize("N,H,W", [(2, 17, 23), (1, 55, 128)])
def test_non_contiguous_input(N, H, W):
    f, b = (t.to(_dev()) for t in fb_input("random", N, H, W))
    want = ops.fb_consistency(f, b)
    wide_f = torch.zeros(N, 2, H, W + 17, device=_dev())
    wide_b = torch.zeros(N, 2, H, W + 17, device=_dev())
    wide_f[..., 5:5 + W] = f
    wide_b[..., 5:5 + W] = b
    vf, vb = wide_f[..., 5:5 + W], wide_b[..., 5:5 + W]
    assert not vf.is_contiguous()
    got = ops.fb_consistency(vf, vb)
    assert all(bits_equal(x, y) for x, y in zip(got, want))
    # the halves of a stacked batch, as the engine passes them
    both = torch.cat([f, b])
    got = ops.fb_consistency(both[:N], both[N:])
    assert all(bits_equal(x, y) for x, y in zip(got, want))


def test_dispatch_and_checks():
    f, b = fb_input("random", 1, 5, 7)
    out = ops.fb_consistency(f.double().to(_dev()), b.double().to(_dev()))
    assert all(t.is_cuda for t in out)      # fp64 CUDA input: the twin
    _check_against_oracle(out, _oracle("random", 1, 5, 7), 1, 5, 7)
    from flowhip.ops import _ext
    with pytest.raises(RuntimeError):
        _ext.ext().fb_consistency(torch.zeros(1, 2, 1, 8, device=_dev()),
                                  torch.zeros(1, 2, 1, 8, device=_dev()))
    with pytest.raises(RuntimeError):
        _ext.ext().fb_consistency(torch.zeros(1, 2, 4, 8, device=_dev()),
                                  torch.zeros(1, 2, 4, 9, device=_dev()))


@pytest.mark.parametrize("name", ["random", "nonfinite"])
def test_reproducible(name):
    f, b = (t.to(_dev()) for t in fb_input(name, 1, 55, 128))
    first = ops.fb_consistency(f, b)
    second = ops.fb_consistency(f, b)
    assert all(bits_equal(x, y) for x, y in zip(first, second))


# ---- model on the device ---------------------------------------------------

def _model(alternate_corr=False, mixed_precision=True):
    torch.manual_seed(1234)
    args = default_ncup_args(model="raft_nc_dbl",
                             mixed_precision=mixed_precision,
                             alternate_corr=alternate_corr)
    return build_model(args).to(_dev()).eval()


@pytest.mark.parametrize("mixed_precision", [False, True])
def test_bidirectional_against_two_calls(mixed_precision):
    """d: the bidirectional forward against two separate calls; d0: the naive
    stacked call model(cat(a,b), cat(b,a)) against the same two calls, the
    batch sensitivity the kernels have without this feature. fp32 asserts
    d <= 2*d0 + 1e-4; bf16 refinement amplifies last-bit differences by an
    unmeasured factor, so that case only prints."""
    model = _model(mixed_precision=mixed_precision)
    g = torch.Generator().manual_seed(21)
    a = (torch.rand(1, 3, 64, 96, generator=g) * 255).to(_dev())
    b = (torch.rand(1, 3, 64, 96, generator=g) * 255).to(_dev())
    with torch.no_grad():
        low, up = model(a, b, iters=4, test_mode=True, bidirectional=True)
        low_fw, up_fw = model(a, b, iters=4, test_mode=True)
        low_bw, up_bw = model(b, a, iters=4, test_mode=True)
        low0, up0 = model(torch.cat([a, b]), torch.cat([b, a]), iters=4,
                          test_mode=True)
    assert low.shape == (2, 2, 8, 12) and up.shape == (2, 2, 64, 96)
    assert torch.isfinite(up).all() and torch.isfinite(low).all()
    sep_low, sep_up = torch.cat([low_fw, low_bw]), torch.cat([up_fw, up_bw])
    for what, got, naive, sep in [("low", low, low0, sep_low),
                                  ("up", up, up0, sep_up)]:
        d = (got - sep).abs().max().item()
        d0 = (naive - sep).abs().max().item()
        print(f"mixed_precision={mixed_precision} {what}: d {d:.3g} "
              f"d0 {d0:.3g}")
        if not mixed_precision:
            assert d <= 2 * d0 + 1e-4


# ---- hipGraph --------------------------------------------------------------

@pytest.mark.parametrize("alternate_corr", [False, True])
def test_graphed_bidirectional_equals_eager_stream(alternate_corr):
    from flowhip.engine.graph import GraphedInference
    from flowhip.engine.stream import FlowStream

    model = _model(alternate_corr)
    shape = (1, 3, 64, 96)
    g = torch.Generator().manual_seed(3)
    frames = [(torch.rand(shape, generator=g) * 255).to(_dev())
              for _ in range(4)]
    pairs = list(zip(frames[:-1], frames[1:]))

    eager = FlowStream(model, iters=4, bidirectional=True)
    want = []
    for a, b in pairs:
        low, up = (t.clone() for t in eager.step(a, b))
        assert low.shape == (2, 2, 8, 12) and up.shape == (2, 2, 64, 96)
        assert torch.isfinite(low).all() and torch.isfinite(up).all()
        cons = ops.fb_consistency(up[:1], up[1:])
        assert (cons[4][..., :3].sum(-1) == 64 * 96).all()
        want.append((low, up, cons))
    with torch.no_grad():
        cold1 = model(*pairs[1], iters=4, test_mode=True, bidirectional=True)
    assert not bits_equal(want[1][0][:1], cold1[0][:1])  # both warm starts
    assert not bits_equal(want[1][0][1:], cold1[0][1:])  # are live

    # the graph with the check inside, warm started by hand
    graph = GraphedInference(model, shape, 4, warm_start=True,
                             bidirectional=True, consistency=True)
    init = None
    for i, ((a, b), (wlow, wup, wcons)) in enumerate(zip(pairs, want)):
        low, up = graph(a, b, init)
        init = graph.next_init
        cons = graph.consistency
        print(f"frame {i}: max|diff| low "
              f"{(low - wlow).abs().max().item():.3g} up "
              f"{(up - wup).abs().max().item():.3g}; visible share "
              f"{(cons[4][..., 0] / (64 * 96)).flatten().tolist()}")
        assert bits_equal(low, wlow) and bits_equal(up, wup), i
        assert len(cons) == 5
        assert all(bits_equal(x, y) for x, y in zip(cons, wcons)), i

    # the graphed stream against the eager stream
    graphed = FlowStream(model, iters=4, graphed=True, input_shape=shape,
                         bidirectional=True)
    assert graphed.graph.consistency is None
    for i, ((a, b), (wlow, wup, _)) in enumerate(zip(pairs, want)):
        low, up = graphed.step(a, b)
        assert bits_equal(low, wlow) and bits_equal(up, wup), i

    # reset() mid-sequence equals a cold bidirectional forward
    graphed.reset()
    low, up = graphed.step(*pairs[1])
    assert bits_equal(low, cold1[0]) and bits_equal(up, cold1[1])


def test_capture_constructor_unchanged():
    from flowhip.engine.graph import GraphedInference

    model = _model()
    shape = (1, 3, 64, 96)
    g = torch.Generator().manual_seed(3)
    a = (torch.rand(shape, generator=g) * 255).to(_dev())
    b = (torch.rand(shape, generator=g) * 255).to(_dev())
    with torch.no_grad():
        want = model(a, b, iters=4, test_mode=True)
    plain = GraphedInference(model, shape, 4)
    assert plain.static_init is None and plain.next_init is None
    assert plain.consistency is None
    low, up = plain(a, b)
    assert low.shape == (1, 2, 8, 12) and up.shape == (1, 2, 64, 96)
    assert bits_equal(low, want[0]) and bits_equal(up, want[1])
    with pytest.raises(ValueError):
        GraphedInference(model, shape, 4, consistency=True)
