"""GPU tests (MI355X) for the HIP backward of the on-demand correlation
lookup (`alt_corr_lookup_bwd`, csrc/alt_corr_bwd.hip): both scatter forms
against `torch_ref.alt_corr_chunk` differentiated in fp64 on the CPU on the
same rounded operands, the cotangent layouts, `needs_input_grad`, wild
coordinates, the public autograd path under every FLOWHIP_ALT_CORR_BWD
value, and the memory bound of the backward.

Tolerance everywhere: the oracle is also evaluated in fp32 on the CPU; with
e32 its max deviation from the fp64 one, the kernel is allowed
max(8 * e32, 1e-5). On the integer inputs e32 <= 2e-6 at gradient
magnitudes 1-4, and an indexing error shows at 0.1 or more."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

# odd extents that floor pooling drops, extents that are no tile multiple,
# B*P % 4 != 0, and D = 200: a channel tail (D % 64 != 0)
SHAPES = [(2, 256, 16, 24, 4), (2, 64, 17, 27, 3), (1, 200, 17, 27, 3)]
COORDSETS = ["rand", "smooth", "mixed"]
ALGOS = ["direct", "tiled"]
L = 4


def _dev():
    return torch.device("cuda:0")


def _C():
    from flowhip.ops import _ext
    return _ext.ext()


def _coords(B, H, W, kind, gen, grid8):
    """-> (coords, thrown): `thrown` (B, H, W) bool marks pixels sent to
    wild coordinates (mixed set only)."""
    from flowhip.utils.geometry import coords_grid
    thrown = torch.zeros(B, H, W, dtype=torch.bool)
    if kind == "rand":
        # uniform over the map extended by 6 px: nearly everything spills
        u = torch.rand(B, 2, H, W, generator=gen)
        ext = torch.tensor([W + 12.0, H + 12.0]).view(1, 2, 1, 1)
        coords = u * ext - 6.0
    else:
        # smooth flow: the tiled kernel's box path
        jit = torch.rand(B, 2, H, W, generator=gen) - 0.5
        off = torch.tensor([2.375, -1.625]).view(1, 2, 1, 1)
        coords = coords_grid(B, H, W) + off + jit
    if grid8:
        coords = torch.round(coords * 8) / 8
    if kind == "mixed":
        # a few pixels of every 4x4 tile
        thrown = torch.rand(B, H, W, generator=gen) < 0.15
    return coords, thrown


def _throw(coords, thrown):
    """Wild coordinates at the thrown pixels: (1e6, -1e6) and NaN in turn."""
    out = coords.clone()
    idx = thrown.nonzero().tolist()
    for n, (b, y, x) in enumerate(idx):
        if n % 3 == 0:
            v = (1e6, -1e6)
        elif n % 3 == 1:
            v = (float("nan"), float("nan"))
        else:
            v = (float("-inf"), 3.0)
        out[b, :, y, x] = torch.tensor(v)
    return out


def _oracle(rows, levels, coords, g, r, dtype):
    """df1_rows (B, P, D) and df2 (B, D, H, W) of alt_corr_chunk in `dtype`
    on the CPU, with the rounded operands as leaves and the level gradients
    pushed through alt_corr_pyramid's autograd."""
    from flowhip.ops import torch_ref
    B, P, D = rows.shape
    H, W = coords.shape[-2:]
    rl = rows.to(dtype).requires_grad_(True)
    ll = [x.to(dtype).requires_grad_(True) for x in levels]
    xy = coords.to(dtype).reshape(B, 2, P).transpose(1, 2)
    outs = [torch_ref.alt_corr_chunk(
        rl[b], [x[b].permute(2, 0, 1) for x in ll], xy[b], r)
        for b in range(B)]
    cot = g.to(dtype).reshape(B, -1, P).transpose(1, 2)
    grads = torch.autograd.grad(outs, [rl] + ll, [cot[b] for b in range(B)])
    x = torch.zeros(B, D, H, W, dtype=dtype, requires_grad=True)
    pooled = torch_ref.alt_corr_pyramid(x, len(levels))
    (df2,) = torch.autograd.grad(
        pooled, x, [gl.permute(0, 3, 1, 2) for gl in grads[1:]])
    return grads[0], df2


@functools.lru_cache(maxsize=None)
def _case(B, D, H, W, r, kind, integer=True):
    """CPU tensors of one case, computed once and never modified:
    rounded operands (f1_rows, levels), coords as the kernel gets them,
    cotangent g (B, C, H, W) fp32, the thrown mask, the fp64 oracle
    (df1_rows, df2) and the tolerance. The oracle of the mixed set runs on
    the smooth coordinates with the thrown pixels' cotangent zeroed: a
    thrown pixel contributes nothing."""
    from flowhip.ops import torch_ref
    gen = torch.Generator().manual_seed(
        3000 + D + r + 17 * COORDSETS.index(kind) + (0 if integer else 7))
    C = L * (2 * r + 1) ** 2
    if integer:
        f1 = torch.randint(-1, 2, (B, D, H, W), generator=gen).float()
        f2 = torch.randint(-1, 2, (B, D, H, W), generator=gen).float()
        g = torch.randint(-1, 2, (B, C, H, W), generator=gen).float()
    else:
        f1 = torch.randn(B, D, H, W, generator=gen)
        f2 = torch.randn(B, D, H, W, generator=gen)
        g = torch.randn(B, C, H, W, generator=gen)
    rows = f1.permute(0, 2, 3, 1).reshape(B, H * W, D).to(
        torch.bfloat16).contiguous()
    levels = [x.permute(0, 2, 3, 1).to(torch.bfloat16).contiguous()
              for x in torch_ref.alt_corr_pyramid(f2, L)]
    sane, thrown = _coords(B, H, W, kind, gen, integer)
    coords = _throw(sane, thrown)
    g_eff = g * (~thrown).unsqueeze(1)
    ref64 = _oracle(rows, levels, sane, g_eff, r, torch.float64)
    ref32 = _oracle(rows, levels, sane, g_eff, r, torch.float32)
    e32 = max((a.double() - b).abs().max().item()
              for a, b in zip(ref32, ref64))
    tol = max(8 * e32, 1e-5)
    return dict(rows=rows, levels=levels, coords=coords, sane=sane, g=g,
                g_eff=g_eff, thrown=thrown, ref=ref64, e32=e32, tol=tol)


def _cotangent(g, form, tail=float("nan")):
    """g (B, C, H, W) fp32 on the CPU -> (GPU cotangent, channels_last) in
    one of the layouts the forward emits."""
    B, C, H, W = g.shape
    if form == "nchw_f32":
        return g.to(_dev()).contiguous(), False
    dt = torch.bfloat16 if form == "nhwc_bf16" else torch.float32
    c8 = (C + 7) // 8 * 8
    assert c8 > C
    full = torch.full((B, H, W, c8), tail, dtype=dt, device=_dev())
    full[..., :C] = g.permute(0, 2, 3, 1).to(_dev()).to(dt)
    return torch.as_strided(full, (B, C, H, W),
                            (H * W * c8, 1, W * c8, c8)), True


def _run(c, r, algo, g=None, form="nhwc_f32", need=(True, True), tail=float("nan"),
         coords=None):
    gg, cl = _cotangent(c["g"] if g is None else g, form, tail)
    d1, d2 = _C().alt_corr_lookup_bwd(
        gg, c["rows"].to(_dev()), [x.to(_dev()) for x in c["levels"]],
        (c["coords"] if coords is None else coords).to(_dev()), r, cl,
        need[0], need[1], algo)
    torch.cuda.synchronize()
    return (None if d1 is None else d1.cpu(),
            None if d2 is None else d2.cpu())


def _check(c, d1, d2, what):
    r1, r2 = c["ref"]
    if d1 is not None:
        assert d1.shape == r1.shape and d1.dtype == torch.float32
        e1 = (d1.double() - r1).abs().max().item()
    if d2 is not None:
        assert d2.shape == r2.shape and d2.dtype == torch.float32
        e2 = (d2.double() - r2).abs().max().item()
    print(f"{what}: e32={c['e32']:.3g} tol={c['tol']:.3g}"
          + (f" df1 err={e1:.3g} (max {r1.abs().max().item():.3g})"
             if d1 is not None else "")
          + (f" df2 err={e2:.3g} (max {r2.abs().max().item():.3g})"
             if d2 is not None else ""))
    if d1 is not None:
        assert torch.isfinite(d1).all()
        assert e1 <= c["tol"], (what, "df1", e1, c["tol"])
    if d2 is not None:
        assert torch.isfinite(d2).all()
        assert e2 <= c["tol"], (what, "df2", e2, c["tol"])


def test_binding_present():
    assert hasattr(_C(), "alt_corr_lookup_bwd")


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("kind", COORDSETS)
@pytest.mark.parametrize("B,D,H,W,r", SHAPES)
def test_binding_matches_fp64_oracle_integer(B, D, H, W, r, kind, algo):
    c = _case(B, D, H, W, r, kind)
    for ref in c["ref"]:
        if kind != "mixed":                      # thrown rows of df1 are zero
            assert (ref != 0).double().mean().item() > 0.99
        assert 0.5 <= ref.abs().max().item()
    d1, d2 = _run(c, r, algo)
    _check(c, d1, d2, f"int D={D} r={r} {kind} {algo}")


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("kind", COORDSETS)
@pytest.mark.parametrize("B,D,H,W,r", SHAPES)
def test_binding_matches_fp64_oracle_gaussian(B, D, H, W, r, kind, algo):
    c = _case(B, D, H, W, r, kind, integer=False)
    d1, d2 = _run(c, r, algo)
    _check(c, d1, d2, f"gauss D={D} r={r} {kind} {algo}")


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("form", ["nchw_f32", "nhwc_f32", "nhwc_bf16"])
def test_cotangent_forms(form, algo):
    """Integer cotangents are exact in bf16, so every form meets the same
    oracle; a NaN pad tail must change nothing (it is never read)."""
    B, D, H, W, r = SHAPES[1]
    c = _case(B, D, H, W, r, "smooth")
    d1, d2 = _run(c, r, algo, form=form, tail=float("nan"))
    _check(c, d1, d2, f"{form} {algo}")
    z1, z2 = _run(c, r, algo, form=form, tail=0.0)
    assert torch.equal(d1, z1)                   # df1 has no atomics
    assert (d2 - z2).abs().max().item() <= c["tol"]


@pytest.mark.parametrize("algo", ALGOS)
def test_needs_input_grad(algo):
    B, D, H, W, r = SHAPES[2]
    c = _case(B, D, H, W, r, "rand")
    d1, d2 = _run(c, r, algo)
    a1, a2 = _run(c, r, algo, need=(True, False))
    assert a2 is None and torch.equal(a1, d1)
    b1, b2 = _run(c, r, algo, need=(False, True))
    assert b1 is None
    _check(c, None, b2, f"f2 only {algo}")
    # atomic reordering only
    assert (b2 - d2).abs().max().item() <= c["tol"]


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("B,D,H,W,r", SHAPES[:2])
def test_wild_coordinates(B, D, H, W, r, algo):
    c = _case(B, D, H, W, r, "mixed")
    thrown = c["thrown"]
    n = int(thrown.sum())
    assert 0.05 * thrown.numel() < n < 0.3 * thrown.numel()
    assert not torch.isfinite(c["coords"]).all()
    d1, d2 = _run(c, r, algo)                    # ends clean (synchronised)
    rows = d1.reshape(B, H, W, D)
    assert (rows[thrown] == 0).all()
    # the others: the run on sane coordinates with the thrown pixels'
    # cotangent zeroed instead
    s1, _ = _run(c, r, algo, g=c["g_eff"], coords=c["sane"])
    assert torch.equal(rows[~thrown], s1.reshape(B, H, W, D)[~thrown])
    _check(c, d1, d2, f"mixed D={D} r={r} {algo}")


def _public_grads(c, f1, f2, coords, r, g):
    from flowhip import ops
    f1g = f1.to(_dev()).requires_grad_(True)
    f2g = f2.to(_dev()).requires_grad_(True)
    out = ops.alt_corr_lookup(f1g, ops.alt_corr_pyramid(f2g, L),
                              coords.to(_dev()), r, fmap2=f2g)
    # a contiguous NCHW cotangent: the op copies it into the output's layout
    d1, d2 = torch.autograd.grad(out, (f1g, f2g), g.to(_dev()).to(out.dtype))
    torch.cuda.synchronize()
    return d1.cpu(), d2.cpu()


def test_public_path_under_every_mode(monkeypatch):
    B, D, H, W, r = SHAPES[0]
    c = _case(B, D, H, W, r, "smooth")
    gen = torch.Generator().manual_seed(77)
    f1 = torch.randint(-1, 2, (B, D, H, W), generator=gen).float()
    f2 = torch.randint(-1, 2, (B, D, H, W), generator=gen).float()
    monkeypatch.setenv("FLOWHIP_ALT_CORR_BWD", "torch")
    t1, t2 = _public_grads(c, f1, f2, c["coords"], r, c["g"])
    assert t1.shape == f1.shape and t2.shape == f2.shape
    for mode in ("direct", "tiled", None):
        if mode is None:
            monkeypatch.delenv("FLOWHIP_ALT_CORR_BWD")
        else:
            monkeypatch.setenv("FLOWHIP_ALT_CORR_BWD", mode)
        d1, d2 = _public_grads(c, f1, f2, c["coords"], r, c["g"])
        e1 = (d1 - t1).abs().max().item()
        e2 = (d2 - t2).abs().max().item()
        print(f"public {mode}: df1 {e1:.3g} df2 {e2:.3g} tol {c['tol']:.3g}"
              f" (max {t1.abs().max().item():.3g} {t2.abs().max().item():.3g})")
        assert d1.shape == t1.shape and d2.shape == t2.shape
        assert e1 <= c["tol"] and e2 <= c["tol"], (mode, e1, e2)
    monkeypatch.setenv("FLOWHIP_ALT_CORR_BWD", "bogus")
    with pytest.raises(ValueError):
        _public_grads(c, f1, f2, c["coords"], r, c["g"])


def test_backward_memory_is_linear_in_pixels():
    """The chunked torch backward's slab alone is floor(2^24 / P) * P * 4 =
    67 MB here; the HIP backward needs df1, df2 and the level accumulators,
    about 3.33 * P * D * 4 bytes, plus the copy of a cotangent that is not
    in the output's layout."""
    from flowhip import ops
    B, D, H, W, r = 1, 128, 64, 96, 4
    P = H * W
    torch.manual_seed(5)
    f1g = torch.randn(B, D, H, W, device=_dev(), requires_grad=True)
    f2g = torch.randn(B, D, H, W, device=_dev(), requires_grad=True)
    from flowhip.utils.geometry import coords_grid
    coords = coords_grid(B, H, W, device=_dev()) + 1.3
    out = ops.alt_corr_lookup(f1g, ops.alt_corr_pyramid(f2g, L), coords, r,
                              fmap2=f2g)
    g = torch.ones_like(out)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    d1, d2 = torch.autograd.grad(out, (f1g, f2g), g)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    print(f"backward at P={P}, D={D}: peak growth {grown / 1e6:.1f} MB "
          f"(bound {8 * P * D * 4 / 1e6:.1f} MB)")
    assert torch.isfinite(d1).all() and torch.isfinite(d2).all()
    assert grown <= 8 * P * D * 4, grown
