"""GPU tests (MI355X) for the default correlation lookup
(csrc/corr_lookup.hip) against the fp64 oracle of tests/corr_lookup_cases.py:
both kernel paths at every level and the boundary between them, windows
over every map edge, batch > 1 with a partial last block, odd maps, both
output layouts, the fresh-buffer and the accumulating backward (fp32 exact,
bf16 within the per-accumulate rounding), and far / non-finite coordinates.

The exact cases have no rounding anywhere (see the case module), so their
tolerance is derived: atol=1e-6, rtol=0; the observed max|diff| should be 0.
"""

import functools

import pytest
import torch

import corr_lookup_cases as cases

pytestmark = pytest.mark.gpu

RADII = [3, 4]
ATOL = cases.EXACT_ATOL
GUARD = 8192            # elements of sentinel around every guarded level
SENTINEL = -1536.0      # no gradient of these cases comes near it


def _dev():
    return torch.device("cuda:0")


def _C():
    import flowhip._C as C
    return C


@pytest.fixture(params=[False, True], ids=["nchw", "nhwc"])
def channels_last(request):
    from flowhip.utils import layout
    old = layout.channels_last_enabled()
    layout.set_channels_last(request.param)
    yield request.param
    layout.set_channels_last(old)


@functools.lru_cache(maxsize=None)
def _dev_levels(kind, r):
    """The case's levels on the GPU, shared and never written."""
    case = cases.exact_case(r) if kind == "exact" else cases.bf16_case(r)
    return [p.to(_dev()) for p in case.levels]


def _shapes4(case):
    BP = case.B * case.H * case.W
    return [[BP, 1, h, w] for h, w in case.shapes]


def _cotangent(g, channels_last):
    g = g.to(_dev())
    if channels_last:
        return g.contiguous(memory_format=torch.channels_last)
    return g.contiguous()


def _poison_allocator(like):
    """Leave NaNs in the block the next same-sized torch::empty will reuse,
    so an unwritten output element or pad-tail entry cannot pass as zero."""
    B, C, H, W = like
    junk = torch.full((B * H * W * ((C + 7) // 8 * 8),), float("nan"),
                      device=_dev())
    del junk


def _check_layout(out, channels_last, K2):
    """NHWC: 8-aligned channel stride and a zeroed pad tail; NCHW: dense."""
    B, C, H, W = out.shape
    assert C == cases.L * K2
    if not channels_last:
        assert out.is_contiguous()
        return
    c8 = (C + 7) // 8 * 8
    assert c8 > C                            # both radii leave a pad tail
    assert out.stride() == (H * W * c8, 1, W * c8, c8)
    rows = torch.as_strided(out, (B, H, W, c8), (H * W * c8, W * c8, c8, 1))
    assert (rows[..., C:] == 0).all()


def _guarded(case, dtype, fill=None):
    """Level buffers carved out of one flat allocation with sentinel bands
    before, between and after them. Returns (levels, guards_untouched)."""
    BP = case.B * case.H * case.W
    sizes = [BP * h * w for h, w in case.shapes]
    flat = torch.full((sum(sizes) + (len(sizes) + 1) * GUARD,), SENTINEL,
                      dtype=dtype, device=_dev())
    is_guard = torch.ones(flat.shape, dtype=torch.bool, device=_dev())
    levels, off = [], GUARD
    for l, (n, (h, w)) in enumerate(zip(sizes, case.shapes)):
        lvl = flat.narrow(0, off, n).view(BP, 1, h, w)
        assert lvl.is_contiguous()
        if fill is None:
            lvl.zero_()
        else:
            lvl.copy_(fill[l])
        is_guard[off:off + n] = False
        levels.append(lvl)
        off += n + GUARD
    assert off == flat.numel()

    def untouched():
        return bool((flat[is_guard] == SENTINEL).all())

    assert untouched()
    return levels, untouched


def _max_diff(got, want):
    return (got.detach().cpu().double() - want).abs().max().item()


def _assert_exact(got, want, what):
    d = _max_diff(got, want)
    print(f"{what}: max|diff|={d:.3g}")
    torch.testing.assert_close(got.detach().cpu().double(), want, atol=ATOL,
                               rtol=0)


# ---------------------------------------------------------------------------
# exact forward
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("r", RADII)
def test_forward_exact(r, channels_last):
    from flowhip import ops
    from flowhip.ops.functional import CorrLookupFn
    case = cases.exact_case(r)
    K2 = (2 * r + 1) ** 2
    levels = _dev_levels("exact", r)
    coords = case.coords.to(_dev())
    for name, fn in (("ops.corr_lookup", ops.corr_lookup),
                     ("CorrLookupFn", lambda p, c, rr:
                      CorrLookupFn.apply(c, rr, *p)[0])):
        _poison_allocator(case.ref.shape)
        out = fn(levels, coords, r)
        assert out.dtype == torch.float32 and out.shape == case.ref.shape
        _check_layout(out, channels_last, K2)
        _assert_exact(out, case.ref,
                      f"forward {name} r={r} nhwc={channels_last}")


# ---------------------------------------------------------------------------
# exact backward through the binding: fresh buffer, zeros, nonzero buffer
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("r", RADII)
def test_backward_binding_exact(r, channels_last):
    case = cases.exact_case(r)
    coords = case.coords.to(_dev())
    g = _cotangent(case.g, channels_last)
    tag = f"r={r} nhwc={channels_last}"

    # acc=0: the binding zero-fills one flat buffer, the kernel stores
    fresh = _C().corr_lookup_bwd(g, coords, r, _shapes4(case), channels_last,
                                 False, None)
    for l, (got, want) in enumerate(zip(fresh, case.grads)):
        _assert_exact(got, want, f"backward fresh {tag} level {l}")

    # acc=1 onto zeros: the same bits, and nothing outside the levels
    zeros, untouched = _guarded(case, torch.float32)
    res = _C().corr_lookup_bwd(g, coords, r, _shapes4(case), channels_last,
                               False, zeros)
    assert untouched()
    for l, (a, b, z) in enumerate(zip(res, fresh, zeros)):
        assert a.data_ptr() == z.data_ptr()          # accumulated in place
        same = torch.equal(a.view(torch.int32), b.view(torch.int32))
        if not same:
            print(f"level {l}: {int((a != b).sum())} values differ, "
                  f"{int((a.view(torch.int32) != b.view(torch.int32)).sum())}"
                  " bit patterns differ")
        assert same, l

    # acc=1 onto nonzero integers: prev + oracle, exactly
    prev = cases.int_prev(r)
    bufs, untouched = _guarded(case, torch.float32, fill=prev)
    res = _C().corr_lookup_bwd(g, coords, r, _shapes4(case), channels_last,
                               False, bufs)
    assert untouched()
    for l, (got, p, want) in enumerate(zip(res, prev, case.grads)):
        _assert_exact(got, p.double() + want,
                      f"backward accumulate {tag} level {l}")


# ---------------------------------------------------------------------------
# the chain
# ---------------------------------------------------------------------------

def _run_chain(case, levels, r):
    """Three chained lookups on one pyramid, loss = sum_k <out_k, g_k>."""
    from flowhip import ops
    leaves = [p.detach().clone().requires_grad_(True) for p in levels]
    pyr, loss = leaves, 0.0
    for c, g in zip(case.chain_coords, case.chain_g):
        out, pyr = ops.corr_lookup_chained(pyr, c.to(_dev()), r)
        assert out.dtype == levels[0].dtype
        loss = loss + (out.float() * g.to(_dev()).float()).sum()
    return torch.autograd.grad(loss, leaves)


@pytest.mark.parametrize("r", RADII)
def test_chain_exact(r, channels_last):
    """The level gradients of three chained lookups (two of them
    read-modify-write onto nonzero cells) equal the fp64 sum of the three
    single-lookup gradients exactly."""
    case = cases.exact_case(r)
    grads = _run_chain(case, _dev_levels("exact", r), r)
    for l, (got, want) in enumerate(zip(grads, case.chain_grads)):
        assert got.dtype == torch.float32
        _assert_exact(got, want,
                      f"chain r={r} nhwc={channels_last} level {l}")


def test_dropped_passthrough_accumulates_onto_zeros(channels_last,
                                                    monkeypatch):
    """A lookup whose passthrough levels are dropped: autograd materialises
    their undefined gradients as zeros, so the backward runs the
    accumulating kernel onto zero buffers (never the fresh-buffer path),
    and returns those very buffers."""
    from flowhip.ops.functional import CorrLookupFn
    r = 4
    case = cases.exact_case(r)
    C = _C()
    real = C.corr_lookup_bwd
    seen = []

    def spy(gout, coords, radius, shapes, cl, bf16, prev):
        seen.append(None if prev is None
                    else [bool((p == 0).all()) for p in prev])
        ptrs = None if prev is None else [p.data_ptr() for p in prev]
        res = real(gout, coords, radius, shapes, cl, bf16, prev)
        if ptrs is not None:
            assert [t.data_ptr() for t in res] == ptrs
        return res

    monkeypatch.setattr(C, "corr_lookup_bwd", spy)
    leaves = [p.detach().clone().requires_grad_(True)
              for p in _dev_levels("exact", r)]
    out = CorrLookupFn.apply(case.coords.to(_dev()), r, *leaves)[0]
    grads = torch.autograd.grad(out, leaves, case.g.to(_dev()))
    assert seen == [[True] * cases.L]
    for l, (got, want) in enumerate(zip(grads, case.grads)):
        _assert_exact(got, want, f"dropped passthrough level {l}")


# ---------------------------------------------------------------------------
# asymmetric probes
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("path,lvl", cases.PROBES)
def test_probe_forward(path, lvl, r, channels_last):
    from flowhip import ops
    p = cases.probe(path, r, lvl)
    _poison_allocator(p.want_out.shape)
    out = ops.corr_lookup([x.to(_dev()) for x in p.levels],
                          p.coords_fwd.to(_dev()), r)
    assert out.nonzero().tolist() == p.want_index
    assert torch.equal(out.cpu().double(), p.want_out)


@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("path,lvl", cases.PROBES)
def test_probe_backward(path, lvl, r, channels_last):
    p = cases.probe(path, r, lvl)
    shapes4 = [list(x.shape) for x in p.levels]
    g = _cotangent(p.cot, channels_last)
    coords = p.coords_bwd.to(_dev())
    zeros = [torch.zeros(s, device=_dev()) for s in shapes4]
    for prev in (None, zeros):
        grads = _C().corr_lookup_bwd(g, coords, r, shapes4, channels_last,
                                     False, prev)
        for l, (got, want) in enumerate(zip(grads, p.want_grads)):
            assert torch.equal(got.cpu().double(), want), (l, prev is None)
        assert grads[lvl].nonzero().tolist() == p.want_cells


# ---------------------------------------------------------------------------
# bf16-resident levels
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("r", RADII)
def test_bf16_forward(r, channels_last):
    """One output rounding away from the oracle on the bf16-rounded maps."""
    from flowhip import ops
    case = cases.bf16_case(r)
    _poison_allocator(case.ref.shape)
    out = ops.corr_lookup(_dev_levels("bf16", r), case.coords.to(_dev()), r)
    assert out.dtype == torch.bfloat16 and out.shape == case.ref.shape
    _check_layout(out, channels_last, (2 * r + 1) ** 2)
    atol = 2.0 ** -8 * case.ref.abs().max().item()
    d = _max_diff(out, case.ref)
    print(f"bf16 forward r={r} nhwc={channels_last}: max|diff|={d:.3g} "
          f"atol={atol:.3g}")
    torch.testing.assert_close(out.cpu().double(), case.ref, atol=atol,
                               rtol=0)


@pytest.mark.parametrize("r", RADII)
def test_bf16_chain_within_rounding_bound(r, channels_last):
    """n=3 chained lookups on bf16 levels: every read-modify-write rounds
    once, so each element may be off by (n+1) * 2^-9 * S, S the sum of the
    absolute contributions to it (the oracle backward of |g|). The bound
    comes from the oracle alone; cells no lookup touches must stay 0."""
    case = cases.bf16_case(r)
    grads = _run_chain(case, _dev_levels("bf16", r), r)
    assert all(g.dtype == torch.bfloat16 for g in grads)
    ratios = cases.worst_ratio([g.cpu() for g in grads], case)
    print(f"bf16 chain r={r} nhwc={channels_last}: worst ratio to the bound "
          f"per level {[round(x, 4) for x in ratios]}")
    assert max(ratios) <= 1.0, ratios


# ---------------------------------------------------------------------------
# far and non-finite coordinates
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("r", RADII)
def test_wild_coordinates(r, channels_last):
    """+-1e6, +-3e9, +-inf and NaN in x and in y, next to an axis that is
    interior (a value >= 2^31 there used to select the unchecked fast
    path): the run ends clean, far rows are zero, non-finite rows zero or
    NaN, every other pixel and every guard band is untouched by them."""
    from flowhip import ops
    case = cases.exact_case(r)
    coords, far, bad = cases.wild_coords(r)
    coords = coords.to(_dev())
    out = ops.corr_lookup(_dev_levels("exact", r), coords, r)
    torch.cuda.synchronize()                 # the run ends clean
    out = out.cpu().double()
    keep = torch.ones(case.B, 1, case.H, case.W, dtype=torch.bool)
    for b, y, x in far:
        assert (out[b, :, y, x] == 0).all(), (b, y, x)
        keep[b, 0, y, x] = False
    for b, y, x in bad:
        o = out[b, :, y, x]
        assert ((o == 0) | o.isnan()).all(), (b, y, x)
        keep[b, 0, y, x] = False
    torch.testing.assert_close(torch.where(keep, out, case.ref), case.ref,
                               atol=ATOL, rtol=0)

    prev = cases.int_prev(r)
    bufs, untouched = _guarded(case, torch.float32, fill=prev)
    res = _C().corr_lookup_bwd(_cotangent(case.g, channels_last), coords, r,
                               _shapes4(case), channels_last, False, bufs)
    torch.cuda.synchronize()
    assert untouched()
    wild = [cases.pixel_index(*p) for p in far + bad]
    tame = torch.ones(case.B * case.H * case.W, dtype=torch.bool)
    tame[wild] = False
    for l, (got, p, want) in enumerate(zip(res, prev, case.grads)):
        got = got.cpu().double()
        w = got[wild]
        assert ((w == p[wild].double()) | w.isnan()).all(), l
        torch.testing.assert_close(got[tame], (p.double() + want)[tame],
                                   atol=ATOL, rtol=0)
