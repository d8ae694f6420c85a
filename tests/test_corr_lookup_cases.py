"""The lookup cases checked on the CPU: every case holds its coverage
conditions, the fp64 oracle agrees with the torch reference to that
reference's own fp32 error, and the probes' hand-built tensors are what the
oracle computes. tests/test_gpu_corr_lookup.py runs the kernel on them."""

import pytest
import torch

import corr_lookup_cases as cases
from flowhip.ops import torch_ref

RADII = [3, 4]
# torch_ref.corr_lookup in fp32 normalises coordinates for grid_sample;
# about 4e-5 from its own fp64 run at these sizes
REF_ATOL = 2e-4


@pytest.mark.parametrize("r", RADII)
def test_conditions_hold(r):
    case = cases.exact_case(r)
    assert case.coords.shape == (2, 2, 15, 23)
    assert (case.B * case.H * case.W) % 256 != 0
    assert case.shapes[0][0] % 2 == 1 and case.shapes[0][1] % 2 == 1
    for l, row in enumerate(cases.check_conditions(case)):
        print(f"r={r} level {l} {case.shapes[l]}: {row}")
    # on the 1/8 grid, inside the map extended by the margin
    assert torch.equal(case.coords * 8, (case.coords * 8).round())
    H0, W0 = case.shapes[0]
    assert case.coords[:, 0].min() >= -cases.MARGIN
    assert case.coords[:, 0].max() <= W0 + cases.MARGIN - 1
    assert case.coords[:, 1].min() >= -cases.MARGIN
    assert case.coords[:, 1].max() <= H0 + cases.MARGIN - 1
    for t in case.levels[:1] + case.chain_g:
        assert torch.equal(t, t.round()) and t.abs().max() <= 4


@pytest.mark.parametrize("r", RADII)
def test_chain_lookups_overlap_on_nonzero_cells(r):
    """The second and third accumulate of the chain must meet cells the
    earlier ones already made nonzero, at every level."""
    case = cases.exact_case(r)
    for l in range(cases.L):
        singles = [cases.oracle_backward(case.shapes, c, r, g)[l]
                   for c, g in zip(case.chain_coords, case.chain_g)]
        both = int(((singles[2] != 0) & (singles[1] != 0)).sum())
        three = int(((singles[2] != 0) & (singles[1] != 0)
                     & (singles[0] != 0)).sum())
        print(f"r={r} level {l}: cells hit twice {both}, three times {three}")
        assert both >= 100 and three >= 100


@pytest.mark.parametrize("r", RADII)
def test_oracle_agrees_with_torch_ref(r):
    case = cases.exact_case(r)
    leaves = [p.clone().requires_grad_(True) for p in case.levels]
    out = torch_ref.corr_lookup(leaves, case.coords, r)
    grads = torch.autograd.grad(out, leaves, case.g)
    d = (out.double() - case.ref).abs().max().item()
    print(f"r={r}: oracle vs torch_ref forward max|diff|={d:.3g}")
    torch.testing.assert_close(out.double(), case.ref, atol=REF_ATOL, rtol=0)
    for l, (a, b) in enumerate(zip(grads, case.grads)):
        d = (a.double() - b).abs().max().item()
        print(f"r={r}: backward level {l} max|diff|={d:.3g}")
        torch.testing.assert_close(a.double(), b, atol=REF_ATOL, rtol=0)


@pytest.mark.parametrize("r", RADII)
def test_far_coordinates_give_zero_rows(r):
    """What the GPU test asserts for far finite coordinates: the oracle and
    the torch reference both give exact zeros there and leave every other
    pixel alone."""
    case = cases.exact_case(r)
    coords, far, _ = cases.wild_coords(r, nonfinite=False)
    out = cases.oracle_lookup([p.double() for p in case.levels], coords, r)
    ref = torch_ref.corr_lookup(case.levels, coords, r)
    keep = torch.ones(case.B, 1, case.H, case.W, dtype=torch.bool)
    for b, y, x in far:
        assert (out[b, :, y, x] == 0).all()
        assert (ref[b, :, y, x] == 0).all()
        keep[b, 0, y, x] = False
    assert torch.equal(torch.where(keep, out, case.ref), case.ref)
    grads = cases.oracle_backward(case.shapes, coords, r, case.g)
    for b, y, x in far:
        for gl in grads:
            assert (gl[cases.pixel_index(b, y, x)] == 0).all()


@pytest.mark.parametrize("r", RADII)
def test_wild_pixels_have_an_interior_other_axis(r):
    """Each single-axis wild pixel would take the fast path at level 0 on
    its other axis alone: the combination that formed the wild address."""
    case = cases.exact_case(r)
    K = 2 * r + 1
    coords, _, _ = cases.wild_coords(r)
    x0, y0 = cases.origins(coords.nan_to_num(0, 0, 0), 0, r)
    H0, W0 = case.shapes[0]
    n = 0
    for (b, y, x), v in cases.WILD_FAR + cases.WILD_NONFINITE:
        p = cases.pixel_index(b, y, x)
        if v[0] is None:
            assert 0 <= x0[p] and x0[p] + K < W0
            n += 1
        if v[1] is None:
            assert 0 <= y0[p] and y0[p] + K < H0
            n += 1
    assert n >= 12


@pytest.mark.parametrize("r", RADII)
def test_ideal_bf16_accumulate_holds_the_chain_bound(r):
    """The premise of the GPU chain test: an accumulate that rounds once
    per read-modify-write stays inside (n+1) * 2^-9 * S on this seed."""
    case = cases.bf16_case(r)
    ratios = cases.worst_ratio(cases.ideal_bf16_chain(case), case)
    print(f"r={r}: ideal bf16 chain, worst ratio per level {ratios}")
    assert max(ratios) <= 1.0
    one = (case.ref.float().to(torch.bfloat16).double() - case.ref).abs()
    assert one.max() <= 2.0 ** -8 * case.ref.abs().max()


@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("path,lvl", cases.PROBES)
def test_probe_tensors_equal_the_oracle(path, lvl, r):
    p = cases.probe(path, r, lvl)
    out = cases.oracle_lookup([x.double() for x in p.levels], p.coords_fwd, r)
    assert torch.equal(out, p.want_out)
    assert out.nonzero().tolist() == p.want_index
    grads = cases.oracle_backward(p.shapes, p.coords_bwd, r, p.cot)
    for got, want in zip(grads, p.want_grads):
        assert torch.equal(got, want)
    assert grads[lvl].nonzero().tolist() == p.want_cells
    assert len(p.want_cells) == (4 if path == "interior" else 2)
    # the reference samples the same cells
    ref = torch_ref.corr_lookup(p.levels, p.coords_fwd, r)
    torch.testing.assert_close(ref.double(), p.want_out, atol=REF_ATOL,
                               rtol=0)
