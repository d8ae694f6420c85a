"""Autograd binding for the fused normalized-convolution kernel.

Forward: one fused HIP kernel (csrc/nconv.hip) producing (nconv, cout).
Backward: one fused HIP kernel plus a small reduce
(csrc/nconv_bwd_fused.hip) producing ddata, dconf, dweight and dbias; shapes
outside its envelope, and FLOWHIP_NCONV_BWD=split, take the split kernels
(prep, bwd-data, weight-grad, plane sums) with their torch glue. denom is
reconstructed from the saved cout (denom = cout * sum(w)) so no extra
forward tensor is stored. (The original torch/MIOpen composition fell into
naive_conv wrw fallbacks at ~240 ms/call for these tiny-channel full-res
shapes — see profiles/.)

Math (d denotes upstream grads):
  nomin = (out − bias) · (denom + eps)
  dnomin = dout / (denom + eps)
  ddenom = −dout · nomin / (denom+eps)² + dcout / s
  ddata  = conf · convT(dnomin, w)
  dconf  = data · convT(dnomin, w) + convT(ddenom, w)
  dw     = ∇w[conv(data·conf) vs dnomin] + ∇w[conv(conf) vs ddenom]
           − Σ(cout·dcout)/s   (through s = Σw per out-channel)
  dbias  = Σ dout
Reference math: nconv_modules.py:164-199.
"""

import os

import torch

from . import _ext


class NConv2dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, data, conf, weight, bias, padding, eps, prop_conf):
        data = data.contiguous()
        conf = conf.contiguous()
        weight = weight.contiguous()
        b = bias.contiguous() if bias is not None else None
        out, cout = _ext.ext().nconv_fwd(data, conf, weight, b)
        if b is not None:
            ctx.save_for_backward(data, conf, weight, out, cout, b)
        else:
            ctx.save_for_backward(data, conf, weight, out, cout)
        ctx.has_bias = bias is not None
        ctx.padding = padding
        ctx.eps = eps
        # an unused output (the cout dropped after nconv_out) then arrives
        # in backward as None instead of a zero-filled plane
        ctx.set_materialize_grads(False)
        return out, cout

    @staticmethod
    def backward(ctx, gout, gcout):
        if gout is None and gcout is None:
            return None, None, None, None, None, None, None
        data, conf, weight, out, cout, *maybe_bias = ctx.saved_tensors
        bias = maybe_bias[0] if ctx.has_bias else None
        gout = gout.contiguous() if gout is not None else None
        gcout = gcout.contiguous() if gcout is not None else None

        if os.environ.get("FLOWHIP_NCONV_BWD", "") == "split":
            ddata, dconf, dweight, dbias = _backward_split(
                gout, gcout, out, cout, data, conf, weight, bias, ctx.eps)
        else:
            ddata, dconf, dweight, dbias = _ext.ext().nconv_bwd_fused(
                gout, gcout, out, cout, data, conf, weight, bias, ctx.eps, -1)
        if not ctx.needs_input_grad[2]:
            dweight = None
        if not ctx.has_bias:
            dbias = None
        return ddata, dconf, dweight, dbias, None, None, None


def _backward_split(gout, gcout, out, cout, data, conf, weight, bias, eps):
    """The pre-fusion backward: prep, bwd-data, weight-grad and plane-sum
    kernels with the glue between them in torch ops."""
    s = weight.sum(dim=(1, 2, 3)).contiguous()         # (Co)
    if gout is None:
        gout = torch.zeros_like(out)

    # fused elementwise preamble (one kernel): denom reconstructed from
    # cout; dnomin = gout/de, ddenom = -gout*(out-bias)/de + gcout/s
    dnomin, ddenom = _ext.ext().nconv_bwd_prep(
        gout, gcout, out, cout, s, bias, eps)

    ddata, dconf, dweight = _ext.ext().nconv_bwd(dnomin, ddenom, data,
                                                 conf, weight)
    if gcout is not None:
        # cout = denom/s depends on s = sum(w) per out channel; one
        # fused per-channel plane reduction instead of the full-res
        # mul + sum pair
        ds = -_ext.ext().plane_sum_nchw(cout, gcout) / s
        dweight = dweight + ds.view(-1, 1, 1, 1)

    dbias = _ext.ext().plane_sum_nchw(gout) if bias is not None else None
    return ddata, dconf, dweight, dbias


class ConfPoolFn(torch.autograd.Function):
    """Confidence-based 2x pooling (kernel #7; nconv_modules.py:94-104):
    one fused kernel each way, full-write backward (no scatter)."""

    @staticmethod
    def forward(ctx, data, conf):
        dds, cds, code = _ext.ext().conf_pool_fwd(data.contiguous(),
                                                  conf.contiguous())
        ctx.save_for_backward(code)
        ctx.in_shape = list(data.shape)
        return dds, cds

    @staticmethod
    def backward(ctx, gdds, gcds):
        (code,) = ctx.saved_tensors
        gdds = gdds.contiguous() if gdds is not None else None
        gcds = gcds.contiguous() if gcds is not None else None
        gdata, gconf = _ext.ext().conf_pool_bwd(gdds, gcds, code,
                                                ctx.in_shape)
        return gdata, gconf
