"""Autograd bindings for the HIP kernels.

Each Function pairs a hand-written gfx950 forward kernel with an explicit
backward (HIP kernels where hot, torch/MIOpen composition where not). The
math contracts live in `torch_ref.py`; GPU unit tests compare both paths.

Layout conventions for the correlation stack (chosen for MFMA/LDS on CDNA4,
not inherited from the reference):
  - feature maps enter as (B, D, H, W) fp32 and are staged as k-contiguous
    bf16 (P, D) operands so both GEMM tiles are ds_read_b128-friendly;
  - the batched GEMM computes C = alpha * A @ B^T with A (M,K), B (N,K) both
    row-major bf16, C (M,N) fp32 — forward and both backward products all map
    onto this one kernel (see CorrVolumeFn docstring).
"""

import math
import os

import torch

from . import _ext
from .determinism import deterministic_enabled


def _pad_k(t):
    """Zero-pad the trailing (K) dim to a multiple of 64 (kernel tile depth).
    Zero columns contribute nothing to the dot products."""
    k = t.shape[-1]
    pad = (-k) % 64
    if pad == 0:
        return t
    return torch.nn.functional.pad(t, (0, pad))


def _bgemm_nt(a, b, alpha, out_bf16=False):
    """C[bat] = alpha * A[bat] @ B[bat]^T ; a (Bt,M,K) bf16, b (Bt,N,K) bf16
    -> fp32 (default) or bf16 (resident corr volume)."""
    return _ext.ext().bgemm_nt(_pad_k(a).contiguous(), _pad_k(b).contiguous(),
                               alpha, out_bf16)


class CorrVolumeFn(torch.autograd.Function):
    """All-pairs correlation C[b,i,j] = <f1[:,i], f2[:,j]>/sqrt(D).

    forward:  C (B,P,P) = 1/sqrt(D) * F1t (B,P,D) @ F2t (B,P,D)^T
    backward: dF1t = 1/sqrt(D) * dC @ F2  -> gemm_nt(dC, F2 (D,P) as (N=D,K=P)? )
    Both backward products reuse the same gemm_nt kernel:
      dF1t (P,D) = gemm_nt(dC  (P,P), F2 (D,P))   [B operand = f2 k-major over P]
      dF2t (P,D) = gemm_nt(dC^T(P,P), F1 (D,P))
    Reference math: core/corr.py:47-55. Inputs are cast to bf16 (fp32
    accumulate in MFMA) — documented deviation from the reference's fp32
    matmul; tolerance covered by tests/test_gpu_corr.py.
    """

    @staticmethod
    def forward(ctx, fmap1, fmap2):
        B, D, H, W = fmap1.shape
        P = H * W

        def as_pd(f):
            # channels_last (B,H,W,D) memory IS the (B,P,D) operand — no
            # transpose kernel, just the bf16 cast
            if f.is_contiguous(memory_format=torch.channels_last):
                return f.permute(0, 2, 3, 1).reshape(B, P, D).to(torch.bfloat16)
            return f.reshape(B, D, P).transpose(1, 2).contiguous().to(
                torch.bfloat16)

        from ..utils.layout import corr_bf16_enabled
        f1t = as_pd(fmap1)  # (B,P,D)
        f2t = as_pd(fmap2)
        # (B,P,P); bf16 residency halves HBM footprint + all pyramid/lookup
        # read traffic (fp32 accumulate inside the MFMA either way)
        corr = _bgemm_nt(f1t, f2t, 1.0 / math.sqrt(D),
                         out_bf16=corr_bf16_enabled())
        ctx.save_for_backward(f1t, f2t)
        ctx.shape = (B, D, H, W)
        ctx.cl = fmap1.is_contiguous(memory_format=torch.channels_last)
        return corr.reshape(B * P, 1, H, W)

    @staticmethod
    def backward(ctx, grad):
        f1t, f2t = ctx.saved_tensors
        B, D, H, W = ctx.shape
        P = H * W
        alpha = 1.0 / math.sqrt(D)
        g3 = grad.reshape(B, P, P).contiguous()
        dc = g3 if g3.dtype == torch.bfloat16 else g3.to(torch.bfloat16)
        # tiled transpose(+cast) kernel (eager transpose().to(bf16) is an
        # uncoalesced ~300us elementwise op at P=7168); accepts fp32 or bf16
        dct = _ext.ext().transpose_cast_bf16(g3)
        # dF1t[i,d] = sum_j dC[i,j] * F2t[j,d]: A = dC (M=P, K=P); the B
        # operand must be (N=D, K=P) row-major = f2 in (D, P) layout with P
        # contiguous.
        f2_kn = f2t.transpose(1, 2).contiguous()  # (B,D,P) bf16, P contiguous
        f1_kn = f1t.transpose(1, 2).contiguous()
        df1t = _bgemm_nt(dc, f2_kn, alpha)   # (B,P,D) fp32
        df2t = _bgemm_nt(dct, f1_kn, alpha)  # (B,P,D) fp32
        if ctx.cl:
            # (B,P,D) memory == channels_last (B,D,H,W): zero-copy view
            df1 = df1t.reshape(B, H, W, D).permute(0, 3, 1, 2)
            df2 = df2t.reshape(B, H, W, D).permute(0, 3, 1, 2)
        else:
            df1 = df1t.transpose(1, 2).reshape(B, D, H, W)
            df2 = df2t.transpose(1, 2).reshape(B, D, H, W)
        return df1, df2


class CorrLookupFn(torch.autograd.Function):
    """Fused 4-level (2r+1)^2-tap bilinear window lookup (core/corr.py:23-44).

    coords never require grad in the RAFT iteration loop (coords1 is detached
    right before every lookup — raft.py:122, raft_nc_dbl.py:149), so backward
    produces gradients for the pyramid levels only and asserts that contract.

    Returns (out, *levels): the pyramid is passed THROUGH so CorrBlock can
    thread it along the iteration loop — the autograd graph then forms a
    CHAIN over the 12 lookups instead of a 12-way fan-out, and each
    backward ACCUMULATES its patch contribution into the incoming level
    grads in-kernel (no per-iteration zero-fill, no autograd add_ fan-in).
    The incoming level grads are REUSED IN PLACE: backward writes into them
    and returns the same tensors — a performance contract of the chain
    (one buffer per level for the whole loop). That is safe because each
    passthrough output has exactly one consumer, the next lookup.

    Callers that drop the passthrough (tests, single lookups, the last
    iteration) still get correct fan-out semantics, by the same path:
    autograd materialises the undefined level grads as zeros (forward does
    not call `set_materialize_grads(False)`), so backward accumulates onto
    fresh zero buffers. The `prev=None` branch below, the binding's own
    zero-fill plus plain stores, is therefore not reached from autograd; it
    serves direct callers of `_C.corr_lookup_bwd`.
    tests/test_gpu_corr_lookup.py pins both down.
    """

    @staticmethod
    def forward(ctx, coords, radius, *pyramid):
        from ..utils.layout import channels_last_enabled
        B, _, H1, W1 = coords.shape
        assert not coords.requires_grad, (
            "corr_lookup: coords must be detached (reference contract)")
        coords_c = coords.contiguous()
        cl = channels_last_enabled()
        out = _ext.ext().corr_lookup_fwd(list(pyramid), coords_c, int(radius),
                                         cl)
        ctx.save_for_backward(coords_c)
        ctx.radius = int(radius)
        ctx.cl = cl
        ctx.level_shapes = [tuple(p.shape) for p in pyramid]
        ctx.levels_bf16 = pyramid[0].dtype == torch.bfloat16
        return (out, *pyramid)

    @staticmethod
    def backward(ctx, grad, *glevels):
        (coords,) = ctx.saved_tensors
        dt = torch.bfloat16 if ctx.levels_bf16 else torch.float32
        if grad.dtype != dt:
            grad = grad.to(dt)
        if ctx.cl:
            grad = grad.contiguous(memory_format=torch.channels_last)
        else:
            grad = grad.contiguous()
        have = [g is not None for g in glevels]
        prev = None
        if all(have):
            prev = [g.contiguous() for g in glevels]
        else:
            assert not any(have), "corr_lookup chain: partial level grads"
        grads = _ext.ext().corr_lookup_bwd(
            grad, coords, ctx.radius,
            [list(s) for s in ctx.level_shapes], ctx.cl, ctx.levels_bf16,
            prev)
        return (None, None, *grads)


class CorrPyramidFn(torch.autograd.Function):
    """Fused avg-pool pyramid (reference corr.py:19-21).

    forward: one LDS-staged kernel emits levels 1..n-1 (level 0 = input,
    passed through). backward: one gather kernel combines the per-level
    grads, dcorr[y,x] = g0 + g1[y/2,x/2]/4 + g2[..]/16 + g3[..]/64 —
    replacing the 3-deep avg_pool2d-backward chain.
    """

    @staticmethod
    def forward(ctx, corr, num_levels):
        corr = corr.contiguous()
        levels = _ext.ext().corr_pyramid_fwd(corr, int(num_levels))
        ctx.corr_shape = list(corr.shape)
        return (corr, *levels)

    @staticmethod
    def backward(ctx, *grads):
        gs = [g.contiguous() if g is not None else None for g in grads]
        dcorr = _ext.ext().corr_pyramid_bwd(gs, ctx.corr_shape)
        return dcorr, None


# budget of one recomputed correlation slab in the chunked backward
# (elements; fp32 -> 64 MiB for level 0, ~1/3 more for the coarser levels)
_ALT_BWD_SLAB = 1 << 24


def alt_f1_rows(fmap1):
    """(B, D, H, W) feature map -> (B, P, D) bf16 rows, rounded once: the
    `f1` operand of the on-demand lookup kernel. Channels-last memory already
    is this layout."""
    B, D, H, W = fmap1.shape
    with torch.no_grad():
        return fmap1.detach().permute(0, 2, 3, 1).reshape(B, H * W, D).to(
            torch.bfloat16).contiguous()


class AltOperandLevels(list):
    """List of pooled f2 levels in the lookup kernel's operand form
    ((B, Hl, Wl, D) bf16); the type tells `ops.alt_corr_lookup` apart from
    the torch path's (B, D, Hl, Wl) levels."""


def alt_f2_levels(fmap2, num_levels):
    """Pooled (B, Hl, Wl, D) bf16 channels-last levels of the second feature
    map: floor-mode 2x2 averaging in fp32, each level rounded to bf16 once.
    Built once per image pair, not on the hot path."""
    from . import torch_ref
    with torch.no_grad():
        lv = torch_ref.alt_corr_pyramid(fmap2.detach().float(), num_levels)
        return AltOperandLevels(
            x.permute(0, 2, 3, 1).to(torch.bfloat16).contiguous() for x in lv)


def _alt_grad_layout(grad, cl):
    """The cotangent in the layout `alt_corr_lookup_fwd` emits (what
    `alt_corr_lookup_bwd` reads): contiguous NCHW, or NHWC rows with the
    8-aligned channel stride. A cotangent that already has it passes through;
    any other is copied (the pad tail is never read, so it stays
    uninitialised)."""
    if grad.dtype not in (torch.float32, torch.bfloat16):
        grad = grad.float()
    if not cl:
        return grad.contiguous()
    B, C, H, W = grad.shape
    c8 = (C + 7) // 8 * 8
    want = (H * W * c8, 1, W * c8, c8)
    if all(grad.shape[d] == 1 or grad.stride(d) == want[d] for d in range(4)):
        return grad.as_strided(grad.shape, want)
    full = torch.empty((B, c8, H, W), device=grad.device, dtype=grad.dtype,
                       memory_format=torch.channels_last)
    g = full.narrow(1, 0, C)
    g.copy_(grad)
    return g


class AltCorrLookupFn(torch.autograd.Function):
    """On-demand correlation window lookup (`--alternate_corr`): what
    CorrLookupFn gathers out of the all-pairs pyramid, computed from the
    feature maps by `alt_corr_lookup_fwd` with nothing of size P^2 alive.

    forward(coords, radius, fmap1, fmap2, f1_rows, *levels): `f1_rows` and
    `levels` are the bf16 kernel operands (`alt_f1_rows`, `alt_f2_levels`),
    built once per pair; `fmap1` / `fmap2` (B, D, H, W) only carry the
    autograd graph and may be None when no gradient is wanted. coords must
    be detached, as for CorrLookupFn. Only coords, f1_rows and the levels
    are saved.

    backward returns gradients for fmap1 and fmap2 from `alt_corr_lookup_bwd`
    (csrc/alt_corr_bwd.hip): the transposed window blend per (pixel, level),
    df1 rows summed in registers, level gradients of f2 summed with float
    atomics into fp32 accumulators (so df2 is not bit-reproducible; in
    deterministic mode a backward that needs df2 raises) and
    gathered back through the pooling chain by one kernel. It allocates
    df1, df2 and the level accumulators, about 3.33 * P * D * 4 bytes, and
    nothing that grows with P^2. `needs_input_grad` selects what is
    computed; a cotangent in another layout than the forward's output is
    copied into it first.

    FLOWHIP_ALT_CORR_BWD=torch|direct|tiled forces a path: `torch` is the
    chunked recompute with torch matmuls (`_backward_torch`, up to
    `_ALT_BWD_SLAB` floats per slab), `direct` and `tiled` the two HIP
    scatter forms; unset, the binding's measured pick runs (table in
    profiles/README.md).
    """

    @staticmethod
    def forward(ctx, coords, radius, fmap1, fmap2, f1_rows, *levels):
        from ..utils.layout import channels_last_enabled, corr_bf16_enabled
        assert not coords.requires_grad, (
            "alt_corr_lookup: coords must be detached (reference contract)")
        coords_c = coords.contiguous()
        cl = channels_last_enabled()
        out = _ext.ext().alt_corr_lookup_fwd(
            f1_rows, list(levels), coords_c, int(radius), cl,
            corr_bf16_enabled())
        ctx.save_for_backward(coords_c, f1_rows, *levels)
        ctx.radius = int(radius)
        ctx.cl = cl
        ctx.fmap_shape = None if fmap1 is None else tuple(fmap1.shape)
        return out

    @staticmethod
    def backward(ctx, grad):
        coords, f1_rows, *levels = ctx.saved_tensors
        need1, need2 = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        if not (need1 or need2):
            return (None,) * (5 + len(levels))
        if need2 and deterministic_enabled():
            raise RuntimeError(
                "alt_corr_lookup backward: the on-demand lookup's df2 (the "
                "gradient of fmap2) does not have a deterministic "
                "implementation, but deterministic mode is on "
                "(flowhip.set_deterministic / FLOWHIP_DETERMINISTIC / "
                "--deterministic). Turn the mode off for this operation, or "
                "train without --alternate_corr.")
        mode = os.environ.get("FLOWHIP_ALT_CORR_BWD", "") or "auto"
        if mode not in ("auto", "torch", "direct", "tiled"):
            raise ValueError(
                f"FLOWHIP_ALT_CORR_BWD={mode!r}: expected torch, direct or "
                "tiled")
        if mode == "torch":
            df1, df2 = AltCorrLookupFn._backward_torch(
                ctx, grad, coords, f1_rows, levels, need1, need2)
        else:
            B, P, D = f1_rows.shape
            H, W = coords.shape[-2:]
            g = _alt_grad_layout(grad, ctx.cl)
            rows, df2 = _ext.ext().alt_corr_lookup_bwd(
                g, f1_rows, list(levels), coords, ctx.radius, ctx.cl,
                bool(need1), bool(need2), mode)
            # (B, P, D) memory == channels_last (B, D, H, W)
            df1 = (rows.reshape(B, H, W, D).permute(0, 3, 1, 2)
                   if need1 else None)
        return (None, None, df1, df2, None) + (None,) * len(levels)

    @staticmethod
    def _backward_torch(ctx, grad, coords, f1_rows, levels, need1, need2):
        """FLOWHIP_ALT_CORR_BWD=torch: the chunked recompute with torch
        matmuls (one (chunk, Hl, Wl) slab per level, at most
        `_ALT_BWD_SLAB` elements at level 0); baseline of the HIP backward
        in tests and tools/bench_alt_corr_bwd.py."""
        from . import torch_ref
        B, P, D = f1_rows.shape
        H, W = coords.shape[-2:]
        g = grad.float().reshape(B, -1, P).transpose(1, 2)      # (B, P, C)
        xy = coords.reshape(B, 2, P).transpose(1, 2)            # (B, P, 2)
        chunk = max(1, min(P, _ALT_BWD_SLAB // P))
        gf1 = torch.zeros(B, P, D, device=grad.device, dtype=torch.float32)
        glv = [torch.zeros(x.shape, device=grad.device, dtype=torch.float32)
               for x in levels]
        with torch.enable_grad():
            for b in range(B):
                # (D, Hl, Wl) fp32 views of the saved bf16 operands
                lv = [x[b].float().permute(2, 0, 1).requires_grad_(need2)
                      for x in levels]
                for s in range(0, P, chunk):
                    rows = f1_rows[b, s:s + chunk].float().requires_grad_(
                        need1)
                    o = torch_ref.alt_corr_chunk(rows, lv, xy[b, s:s + chunk],
                                                 ctx.radius)
                    wanted = ([rows] if need1 else []) + (lv if need2 else [])
                    gs = torch.autograd.grad(o, wanted, g[b, s:s + chunk])
                    if need1:
                        gf1[b, s:s + chunk] = gs[0]
                        gs = gs[1:]
                    if need2:
                        for acc, gl in zip(glv, gs):
                            acc[b] += gl.permute(1, 2, 0)
        df1 = df2 = None
        if need1:
            # (B, P, D) memory == channels_last (B, D, H, W)
            df1 = gf1.reshape(B, H, W, D).permute(0, 3, 1, 2)
        if need2:
            # transpose of the pooling chain: level grads -> fmap2 grad
            with torch.enable_grad():
                x = torch.zeros(B, D, H, W, device=grad.device,
                                dtype=torch.float32).requires_grad_(True)
                pooled = torch_ref.alt_corr_pyramid(x, len(levels))
                (df2,) = torch.autograd.grad(
                    pooled, x, [a.permute(0, 3, 1, 2) for a in glv])
        return df1, df2
