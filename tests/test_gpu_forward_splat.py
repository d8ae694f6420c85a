"""GPU: the forward-splat HIP kernel against the float64 oracle (bit-exact,
ties included), its reproducibility, and warm-started hipGraph inference
against the eager stream."""

import functools

import pytest
import torch

from flowhip import ops
from flowhip.config.args import default_ncup_args
from flowhip.models import build_model
from flowhip.ops import _ext, torch_ref

from splat_cases import KERNEL_INPUTS, bits_equal, kernel_input

pytestmark = pytest.mark.gpu

SHAPES = [(1, 5, 7), (2, 17, 23), (1, 55, 128)]


def _dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _oracle(name, B, H, W):
    """CPU float64 oracle, computed once per input and shared (read-only)."""
    return torch_ref.forward_splat(kernel_input(name, B, H, W))


def _ragged_splits(H, W):
    """Smallest forced chunk count >= 4 (above the planned 1 and 3 of the
    small shapes) whose last chunk is shorter."""
    HW = H * W
    for s in range(4, HW):
        chunk = -(-HW // s)
        if HW % chunk and -(-HW // chunk) == s:
            return s
    raise AssertionError("no ragged split")


@pytest.mark.parametrize("mode", ["planned", "single", "ragged"])
@pytest.mark.parametrize("name", KERNEL_INPUTS)
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_kernel_matches_oracle_bit_exact(B, H, W, name, mode):
    ext = _ext.ext()
    splits = {"planned": 0, "single": 1, "ragged": _ragged_splits(H, W)}[mode]
    G = ext.forward_splat_plan(H, W, splits)
    if mode == "single":
        assert G == 1
    if mode == "ragged":
        assert G == splits > 1 and (H * W) % (-(-(H * W) // G)) != 0

    flow = kernel_input(name, B, H, W)
    ref = _oracle(name, B, H, W)
    out = ops.forward_splat(flow.to(_dev()), splits=splits)
    assert not out.requires_grad
    bad = (out.cpu().view(torch.int32) != ref.view(torch.int32))
    print(f"{name} {tuple(flow.shape)} G={G}: mismatching values {int(bad.sum())}")
    assert bits_equal(out, ref)


def test_plan_reaches_both_paths():
    """The test shapes cover the single-pass and the partials+finish path at
    their planned G; the flagship field launches well over 256 workgroups."""
    ext = _ext.ext()
    assert ext.forward_splat_plan(5, 7) == 1
    assert ext.forward_splat_plan(17, 23) > 1
    G = ext.forward_splat_plan(55, 128)
    assert G * -(-(55 * 128) // 1024) > 256
    # forced chunk counts that would leave empty chunks are normalised
    assert ext.forward_splat_plan(5, 7, 1000) == 35
    assert ext.forward_splat_plan(5, 7, 4) == 4


def test_3d_input_and_dispatch():
    flow = kernel_input("random", 1, 5, 7)
    out = ops.forward_splat(flow[0].to(_dev()))
    assert out.shape == (2, 5, 7) and out.is_cuda
    assert bits_equal(out, _oracle("random", 1, 5, 7)[0])
    # non-fp32 CUDA input takes the oracle
    out64 = ops.forward_splat(flow.double().to(_dev()))
    assert out64.dtype == torch.float64
    assert torch.equal(out64.float().cpu(), _oracle("random", 1, 5, 7))


def test_non_contiguous_input():
    flow = kernel_input("random", 2, 17, 23).to(_dev())
    wide = torch.zeros(2, 2, 17, 40, device=_dev())
    wide[..., 5:28] = flow
    out = ops.forward_splat(wide[..., 5:28])
    assert bits_equal(out, _oracle("random", 2, 17, 23))


@pytest.mark.parametrize("splits", [0, 1])
def test_reproducible(splits):
    flow = kernel_input("random", 1, 55, 128).to(_dev())
    a = ops.forward_splat(flow, splits=splits)
    b = ops.forward_splat(flow, splits=splits)
    assert bits_equal(a, b)
    ties = kernel_input("ties", 1, 55, 128).to(_dev())
    assert bits_equal(ops.forward_splat(ties, splits=splits),
                      ops.forward_splat(ties, splits=splits))


# ---- warm-started hipGraph inference --------------------------------------

def _model(alternate_corr):
    torch.manual_seed(1234)
    args = default_ncup_args(model="raft_nc_dbl", mixed_precision=True,
                             alternate_corr=alternate_corr)
    return build_model(args).to(_dev()).eval()


@pytest.mark.parametrize("alternate_corr", [False, True])
def test_graphed_warm_start_equals_eager_stream(alternate_corr):
    from flowhip.engine.graph import GraphedInference
    from flowhip.engine.stream import FlowStream

    model = _model(alternate_corr)
    shape = (1, 3, 64, 96)
    g = torch.Generator().manual_seed(3)
    frames = [(torch.rand(shape, generator=g) * 255).to(_dev())
              for _ in range(4)]
    pairs = list(zip(frames[:-1], frames[1:]))

    eager = FlowStream(model, iters=4)
    want = [tuple(t.clone() for t in eager.step(a, b)) for a, b in pairs]
    for low, up in want:
        assert torch.isfinite(low).all() and torch.isfinite(up).all()
    with torch.no_grad():
        cold1 = model(*pairs[1], iters=4, test_mode=True)
    assert not bits_equal(want[1][0], cold1[0])  # the warm start is live

    graphed = FlowStream(model, iters=4, graphed=True, input_shape=shape)
    got = [tuple(t.clone() for t in graphed.step(a, b)) for a, b in pairs]
    for i, ((low, up), (wlow, wup)) in enumerate(zip(got, want)):
        print(f"frame {i}: max|diff| low "
              f"{(low - wlow).abs().max().item():.3g} up "
              f"{(up - wup).abs().max().item():.3g}")
        assert bits_equal(low, wlow) and bits_equal(up, wup), i

    # reset() mid-sequence equals a fresh stream
    graphed.reset()
    low, up = graphed.step(*pairs[1])
    assert bits_equal(low, cold1[0]) and bits_equal(up, cold1[1])
    low, up = graphed.step(*pairs[2])
    fresh = FlowStream(model, iters=4)
    fresh.step(*pairs[1])
    flow, fup = fresh.step(*pairs[2])
    assert bits_equal(low, flow) and bits_equal(up, fup)

    # warm_start=False: today's graph, unchanged output, no init input
    plain = GraphedInference(model, shape, iters=4)
    assert plain.static_init is None and plain.next_init is None
    low, up = plain(*pairs[1])
    assert bits_equal(low, cold1[0]) and bits_equal(up, cold1[1])
    with pytest.raises(AssertionError):
        plain(*pairs[1], flow_init=want[0][0])
