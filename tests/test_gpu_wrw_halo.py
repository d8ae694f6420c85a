"""Halo-staged weight-gradient kernel (csrc/conv_wrw_halo.hip) against the
generic per-tap kernel and an fp64 reference.

Both kernels sum the same bf16 products in fp32, in different orders. Per
case the generic kernel's (algo=0) max-abs error against the fp64 gradient
of the same rounded inputs is measured, and the halo kernel's (algo=1)
error must be at most twice that: the margin covers the reordering only.
The project's conv bound (TestConvGemm: atol=1e-1, rtol=5e-2) applies on
top as an absolute cap. Both errors are printed.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


# (id, B, H, W, C1, C2, Cout, KH, KW, ld_extra)
# C2 > 0: two-source input cat([x1, x2]); ld_extra > 0: x is a
# channel-narrowed view of a (C1 + ld_extra)-channel allocation
CASES = [
    # single-tile floor; nchunk clamps to the tile count
    ("floor_8to8_3x3", 1, 3, 5, 8, 0, 8, 3, 3, 0),
    # tile tails in both axes; chunks crossing image boundaries
    ("tails_64to64_3x3", 2, 11, 37, 64, 0, 64, 3, 3, 0),
    # ragged Cin slab, ragged Cout
    ("ragged_72to126_3x3", 2, 11, 37, 72, 0, 126, 3, 3, 0),
    # Cout padded 2 -> 8, the flow-head output
    ("flowhead_256to2_3x3", 2, 11, 37, 256, 0, 2, 3, 3, 0),
    # two-source, x1 = 64 ch, x2 = 40 ch
    ("cat_64p40to64_1x5", 2, 11, 37, 64, 40, 64, 1, 5, 0),
    ("cat_64p40to64_5x1", 2, 11, 37, 64, 40, 64, 5, 1, 0),
    # two-source; second slab wholly from x2
    ("cat_128p256to128_5x1", 2, 9, 70, 128, 256, 128, 5, 1, 0),
    # narrowed-view input with padded ld_x (the 324-of-328 corr case)
    ("narrowed_324of328to64_3x3", 2, 11, 37, 324, 0, 64, 3, 3, 4),
]

_cache = {}


def _case(case):
    """Inputs and the fp64 reference, built once per case and shared by
    the bias / no-bias tests."""
    name, B, H, W, C1, C2, Cout, KH, KW, ld_extra = case
    if name in _cache:
        return _cache[name]
    g = torch.Generator(device="cpu").manual_seed(1000 + len(name) + H * W)

    def cl(n, c):
        t = (torch.randn(n, c, H, W, generator=g) / 4).to(torch.bfloat16)
        return t.to(_dev()).contiguous(memory_format=torch.channels_last)

    x1 = cl(B, C1 + ld_extra)
    if ld_extra:
        x1 = x1[:, :C1]
    x2 = cl(B, C2) if C2 else None
    dy = cl(B, Cout)
    # the autograd functions pad dy's channels to a multiple of 8
    pad = (-Cout) % 8
    dyp = dy
    if pad:
        z = dy.new_zeros(B, pad, H, W).contiguous(
            memory_format=torch.channels_last)
        dyp = torch.cat([dy, z], dim=1).contiguous(
            memory_format=torch.channels_last)
    assert dyp.stride(1) == 1 and dyp.stride(3) == dyp.size(1)

    # fp64 gradient of the same rounded inputs, tap by tap
    xin = x1 if x2 is None else torch.cat([x1, x2], dim=1)
    xpad = torch.nn.functional.pad(
        xin.double(), (KW // 2, KW // 2, KH // 2, KH // 2))
    dy64 = dy.double()
    dw = torch.empty(Cout, C1 + C2, KH, KW, dtype=torch.float64,
                     device=_dev())
    for ky in range(KH):
        for kx in range(KW):
            dw[:, :, ky, kx] = torch.einsum(
                "noyx,ncyx->oc", dy64, xpad[:, :, ky:ky + H, kx:kx + W])
    db = dy64.sum((0, 2, 3))
    _cache[name] = (x1, x2, dyp, dw, db)
    return _cache[name]


@pytest.mark.parametrize("want_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_halo_vs_generic_vs_fp64(case, want_bias):
    import flowhip._C as C
    name, B, H, W, C1, C2, Cout, KH, KW, _ = case
    x1, x2, dyp, dw_ref, db_ref = _case(case)

    def run(algo):
        dw, db = C.conv_gemm_wrw(dyp, x1, x2, KH, KW, 1, 1, want_bias, algo)
        torch.cuda.synchronize()
        assert dw.shape == (dyp.shape[1], C1 + C2, KH, KW)
        return dw[:Cout].double(), (db[:Cout].double() if want_bias else None)

    dw_g, db_g = run(0)
    dw_h, db_h = run(1)
    err_g = (dw_g - dw_ref).abs().max().item()
    err_h = (dw_h - dw_ref).abs().max().item()
    print(f"[wrw_halo] {name} dW  max-abs err: generic {err_g:.3e} "
          f"halo {err_h:.3e}")
    if want_bias:
        berr_g = (db_g - db_ref).abs().max().item()
        berr_h = (db_h - db_ref).abs().max().item()
        print(f"[wrw_halo] {name} dbias max-abs err: generic {berr_g:.3e} "
              f"halo {berr_h:.3e}")

    assert torch.isfinite(dw_h).all()
    assert err_h <= 2.0 * err_g, (err_h, err_g)
    torch.testing.assert_close(dw_h, dw_ref, atol=1e-1, rtol=5e-2)
    if want_bias:
        assert berr_h <= 2.0 * berr_g, (berr_h, berr_g)
        torch.testing.assert_close(db_h, db_ref, atol=1e-1, rtol=5e-2)

    # auto dispatch takes one of the two paths bit for bit (both are
    # deterministic: fixed split-M chunks, no float atomics)
    dw_a, _ = C.conv_gemm_wrw(dyp, x1, x2, KH, KW, 1, 1, want_bias)
    dw_a = dw_a[:Cout].double()
    assert torch.equal(dw_a, dw_h) or torch.equal(dw_a, dw_g)


def test_forced_chunk_counts_agree():
    """Every split-M chunk count gives the same sums up to fp32 order:
    one chunk per pixel tile, and one chunk in all (chunks crossing image
    boundaries either way)."""
    import flowhip._C as C
    case = CASES[1]
    x1, x2, dyp, dw_ref, _ = _case(case)
    outs = []
    for nchunk in (1, 5, 12):
        dw, _ = C.conv_gemm_wrw(dyp, x1, x2, 3, 3, 1, 1, False, 1, nchunk)
        outs.append(dw.double())
    for dw in outs:
        torch.testing.assert_close(dw, dw_ref, atol=1e-1, rtol=5e-2)


def test_halo_refuses_shapes_outside_envelope():
    """algo=1 on a 1x1 or strided conv is an error, not a quiet fall-back."""
    import flowhip._C as C
    x1, x2, dyp, _, _ = _case(CASES[1])
    with pytest.raises(RuntimeError):
        C.conv_gemm_wrw(dyp, x1, None, 1, 1, 1, 1, False, 1)
