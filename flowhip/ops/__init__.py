"""flowhip.ops — the op layer: dispatch between hand-written
gfx950 HIP kernels (CUDA tensors, extension built) and the pure-PyTorch
reference path (CPU, or forced via FLOWHIP_FORCE_REF=1).

Public surface (mirrors the compute-heavy call sites of the reference —
SURVEY.md §2.2 kernel inventory):

  corr_volume(fmap1, fmap2)            kernel #1  (MFMA batched GEMM)
  corr_pyramid(corr, num_levels)       kernel #2  (avg-pool pyramid)
  corr_lookup(pyramid, coords, r)      kernel #3  (4-level 81-tap gather+lerp)
  alt_corr_pyramid(fmap2, num_levels)  pooled f2 levels for the on-demand mode
  alt_corr_lookup(f1, levels, coords, r)  on-demand window lookup, no volume
  nconv2d(...)                         kernel #6  (fused normalized conv)
  conf_pool(data, conf)                kernel #7  (confidence-based pooling)
  zero_inject(x, sh, sw)               kernel #8  (sparse injection scatter)
  convex_upsample(flow, mask)          kernel #11 (RAFT convex upsample)
  forward_splat(flow)                  warm-start nearest splat (no gradient)
  fb_consistency(flow_fw, flow_bw)     forward-backward occlusion check
  sequence_loss(preds, gt, valid, g)   kernel #12 (loss; torch for now)

  set_deterministic(flag) / deterministic_enabled() / deterministic(flag)
                                       bit-reproducible training step
                                       (ops/determinism.py)
"""

import torch

from . import _ext, torch_ref
from .determinism import (deterministic, deterministic_enabled,  # noqa: F401
                          set_deterministic)
from .torch_ref import MAX_FLOW  # re-export  # noqa: F401


def sequence_loss(flow_preds, flow_gt, valid, gamma=0.8, max_flow=MAX_FLOW):
    """gamma-weighted L1 over the prediction sequence + final-pred metrics
    (kernel #12; reference train.py:46-71).

    Degenerate-batch behavior: with ZERO valid pixels the fused
    kernel clamps the divisor to 1 and reports 0 loss/metrics, whereas the
    reference's `epe.mean()` over an empty selection yields NaN and poisons
    the step. 0 is the defined behavior here (a no-op step instead of a
    NaN-corrupted model); the torch_ref path mirrors it.
    """
    if (_ext.use_hip(flow_gt) and 1 <= len(flow_preds) <= 32
            and all(p.dtype == torch.float32 for p in flow_preds)):
        from .functional_loss import sequence_loss_fused
        return sequence_loss_fused(flow_preds, flow_gt, valid, gamma,
                                   max_flow)
    return torch_ref.sequence_loss(flow_preds, flow_gt, valid, gamma,
                                   max_flow)


def corr_volume(fmap1, fmap2):
    if _ext.use_hip(fmap1):
        from .functional import CorrVolumeFn
        return CorrVolumeFn.apply(fmap1, fmap2)
    return torch_ref.corr_volume(fmap1, fmap2)


def corr_pyramid(corr, num_levels=4):
    # fused single-pass build + single-kernel backward combine. The LDS
    # budget is dynamic (~31k fp32 / ~62k bf16 level-0 cells — covers every
    # BASELINE/eval shape incl. KITTI submission 47x156); larger maps fall
    # back to the torch avg_pool chain WITH a warning (round-1 fell back
    # silently — VERDICT r01).
    if _ext.use_hip(corr) and 2 <= num_levels <= 4:
        if _ext.ext().corr_pyramid_fits(corr.shape[-2], corr.shape[-1],
                                        corr.dtype == torch.bfloat16):
            from .functional import CorrPyramidFn
            return list(CorrPyramidFn.apply(corr, num_levels))
        import warnings
        warnings.warn(
            f"corr_pyramid: map {tuple(corr.shape[-2:])} exceeds the fused "
            "kernel's LDS budget; using the torch avg_pool chain")
    return torch_ref.corr_pyramid(corr, num_levels)


def corr_lookup(pyramid, coords, radius):
    # HIP kernel instantiates the RAFT radii (3 small / 4 basic)
    if radius in (3, 4) and _ext.use_hip(coords):
        from .functional import CorrLookupFn
        return CorrLookupFn.apply(coords, radius, *pyramid)[0]
    return torch_ref.corr_lookup(pyramid, coords, radius)


def corr_lookup_chained(pyramid, coords, radius):
    """Lookup + pyramid passthrough for the iteration loop (see
    CorrLookupFn): returns (out, new_pyramid) where new_pyramid must be
    fed to the NEXT iteration's lookup so level grads accumulate along
    the chain."""
    if radius in (3, 4) and _ext.use_hip(coords):
        from .functional import CorrLookupFn
        res = CorrLookupFn.apply(coords, radius, *pyramid)
        return res[0], list(res[1:])
    return torch_ref.corr_lookup(pyramid, coords, radius), pyramid


def alt_corr_pyramid(fmap2, num_levels=4):
    """Pooled second-feature-map pyramid for the on-demand lookup.

    HIP path: the kernel's operand form — (B, Hl, Wl, D) bf16 channels-last
    levels, detached (gradients reach fmap2 through `alt_corr_lookup`'s
    `fmap2` argument). Outside the kernel's envelope (D % 8, D <= 512,
    1..4 levels) and on CPU: the differentiable fp32 (B, D, Hl, Wl) levels
    of `torch_ref.alt_corr_pyramid`, which select the torch lookup."""
    if _ext.use_hip(fmap2):
        # the radius is checked at lookup time; 4 stands in for it here
        if _ext.ext().alt_corr_supported(fmap2.shape[1], 4, num_levels):
            from .functional import alt_f2_levels
            return alt_f2_levels(fmap2, num_levels)
        import warnings
        warnings.warn(
            f"alt_corr_pyramid: D={fmap2.shape[1]}, {num_levels} levels is "
            "outside the on-demand lookup kernel's envelope; using the "
            "chunked torch path")
    return torch_ref.alt_corr_pyramid(fmap2, num_levels)


def alt_corr_lookup(fmap1, fmap2_levels, coords, radius, fmap2=None,
                    f1_rows=None):
    """Correlation window lookup without the all-pairs volume; same output
    (values, dtype, layout) as `corr_lookup` on the pyramid of
    `corr_volume(fmap1, fmap2)`.

    `fmap2_levels` comes from `alt_corr_pyramid`. On the HIP path `fmap2`
    is the map the levels were built from — required only for its gradient;
    `f1_rows` optionally passes a cached `functional.alt_f1_rows(fmap1)`."""
    from .functional import AltOperandLevels
    if isinstance(fmap2_levels, AltOperandLevels):
        if radius in (3, 4) and _ext.use_hip(coords):
            from .functional import AltCorrLookupFn, alt_f1_rows
            if f1_rows is None:
                f1_rows = alt_f1_rows(fmap1)
            return AltCorrLookupFn.apply(coords, radius, fmap1, fmap2,
                                         f1_rows, *fmap2_levels)
        # other radii: torch path on the rounded operands
        fmap2_levels = [x.permute(0, 3, 1, 2).float() for x in fmap2_levels]
    return torch_ref.alt_corr_lookup(fmap1, fmap2_levels, coords, radius)


def nconv2d(data, conf, weight, bias=None, stride=1, padding=0, dilation=1,
            groups=1, eps=1e-20, prop_conf=True):
    if _ext.use_hip(data) and _can_fuse_nconv(
            data, conf, weight, stride, padding, dilation, groups, eps,
            prop_conf, warn=True):
        from .functional_nconv import NConv2dFn
        return NConv2dFn.apply(data, conf, weight, bias, padding, eps, prop_conf)
    return torch_ref.nconv2d(data, conf, weight, bias, stride, padding,
                             dilation, groups, eps, prop_conf)


def nconv2d_uses_hip(data, conf, weight, stride=1, padding=0, dilation=1,
                     groups=1, eps=1e-20, prop_conf=True):
    """True where nconv2d would run the HIP kernels for these arguments."""
    return _ext.use_hip(data) and _can_fuse_nconv(
        data, conf, weight, stride, padding, dilation, groups, eps, prop_conf)


def _can_fuse_nconv(data, conf, weight, stride, padding, dilation, groups,
                    eps, prop_conf, warn=False):
    """Everything the kernels hard-wire — stride 1, dilation 1, groups 1,
    square K, zero padding K//2, the forward's eps of 1e-20, propagated
    confidence, fp32 — and their (Ci, Co, K) table. `warn` reports a call
    that only the table keeps on the torch path."""
    from torch.nn.modules.utils import _pair
    if _pair(stride) != (1, 1) or _pair(dilation) != (1, 1) or groups != 1:
        return False
    o, i, kh, kw = weight.shape
    if (kh != kw or _pair(padding) != (kh // 2, kh // 2) or eps != 1e-20
            or not prop_conf
            or not data.dtype == conf.dtype == weight.dtype == torch.float32):
        return False
    if _ext.ext().nconv_supported(i, o, kh):
        return True
    if warn:
        import warnings
        warnings.warn(
            f"nconv2d: (Ci, Co, K) = ({i}, {o}, {kh}) is not in the "
            "normalized-convolution kernel table (csrc/nconv.h); using the "
            "torch path")
    return False


def conf_pool(data, conf, ds_factor=2, pooling_type="conf_based"):
    if (_ext.use_hip(data) and ds_factor == 2
            and pooling_type == "conf_based"
            and data.dtype == torch.float32):
        from .functional_nconv import ConfPoolFn
        return ConfPoolFn.apply(data, conf)
    return torch_ref.conf_pool(data, conf, ds_factor, pooling_type)


def area_resize(x, size):
    """F.interpolate(x, size, mode='area') with a fused kernel for the
    exact-2x-upsample case (the per-iteration guidance resize)."""
    import torch.nn.functional as F
    ih, iw = x.shape[-2:]
    if (_ext.use_hip(x) and x.dtype == torch.float32
            and size[0] == 2 * ih and size[1] == 2 * iw):
        from .functional_upsample import AreaUp2xFn
        return AreaUp2xFn.apply(x)
    return F.interpolate(x, size, mode="area")


def up2x_cat(low, skip):
    """cat([nearest_2x(low), skip], dim=1) in one kernel (NConvUNet decoder
    skip path). Exact-2x only; callers fall back otherwise."""
    import torch.nn.functional as F
    import torch as _t
    if (_ext.use_hip(low) and low.dtype == _t.float32
            and skip.shape[2] == 2 * low.shape[2]
            and skip.shape[3] == 2 * low.shape[3]):
        from .functional_upsample import Up2xCatFn
        return Up2xCatFn.apply(low, skip)
    up = F.interpolate(low, size=skip.shape[2:], mode="nearest")
    return _t.cat((up, skip), 1)


def zero_inject(inp, scale_h, scale_w, out_h=None, out_w=None):
    if _ext.use_hip(inp) and inp.dtype == torch.float32:
        from .functional_upsample import ZeroInjectFn
        oh = out_h if out_h is not None else inp.shape[2] * scale_h
        ow = out_w if out_w is not None else inp.shape[3] * scale_w
        return ZeroInjectFn.apply(inp, scale_h, scale_w, oh, ow)
    return torch_ref.zero_inject(inp, scale_h, scale_w, out_h, out_w)


def forward_splat(flow, splits=0):
    """Warm-start splat: forward-warp a flow field (B,2,H,W) or (2,H,W) onto
    the grid, each cell taking the flow of the nearest landed source
    (reference core/utils/utils.py:28-56, scipy griddata "nearest" there).

    Defined behaviour where scipy's is not: ties go to the lowest source
    index, and a sample with no source inside the frame yields zeros. Not
    differentiable. HIP for CUDA fp32 tensors (`splits` forces the kernel's
    source chunk count, 0 = planned); the float64 oracle otherwise."""
    if _ext.use_hip(flow) and flow.dtype == torch.float32:
        from .functional_upsample import ForwardSplatFn
        if flow.dim() == 3:
            return ForwardSplatFn.apply(flow[None], splits)[0]
        return ForwardSplatFn.apply(flow, splits)
    return torch_ref.forward_splat(flow)


def fb_consistency(flow_fw, flow_bw, alpha1=0.01, alpha2=0.5):
    """Forward-backward consistency check of a bidirectional flow pair:
    `flow_fw` (1->2, on frame 1's grid) and `flow_bw` (2->1, on frame 2's
    grid), both (N,2,H,W) with H, W >= 2.

    Returns (occ_fw, occ_bw, res_fw, res_bw, stats): uint8 occlusion masks
    (1 = occluded, out of frame or non-finite), fp32 residuals |f + b~| and
    fp64 (N,2,4) per-sample, per-direction counts and visible residual sum —
    the definition is `torch_ref.fb_consistency`'s. The defaults are the
    UnFlow thresholds. Not differentiable. HIP for CUDA fp32 tensors (any
    strides); the float64 twin otherwise."""
    if (_ext.use_hip(flow_fw) and flow_bw.is_cuda
            and flow_fw.dtype == flow_bw.dtype == torch.float32):
        return tuple(_ext.ext().fb_consistency(
            flow_fw.detach(), flow_bw.detach(), float(alpha1), float(alpha2)))
    return torch_ref.fb_consistency(flow_fw, flow_bw, alpha1, alpha2)


def convex_upsample(flow, mask, factor=8):
    if _ext.use_hip(flow):
        from .functional_upsample import ConvexUpsampleFn
        return ConvexUpsampleFn.apply(flow, mask, factor)
    return torch_ref.convex_upsample(flow, mask, factor)
