"""Autograd binding for the fused normalized-convolution kernels.

Forward: one fused HIP kernel (csrc/nconv.hip) producing (nconv, cout).
Backward: one fused HIP kernel plus a small reduce
(csrc/nconv_bwd_fused.hip) producing ddata, dconf, dweight and dbias;
FLOWHIP_NCONV_BWD=split (read per call) runs the split kernels (prep,
bwd-data, weight-grad, plane sums) through the same binding instead. denom
is reconstructed from the saved cout (denom = cout * sum(w)) so no extra
forward tensor is stored. (The original torch/MIOpen composition fell into
naive_conv wrw fallbacks at ~240 ms/call for these tiny-channel full-res
shapes — see profiles/.)

The kernels need whole float4 rows. At W % 4 != 0 the planes are
right-padded with zero columns to the next multiple of 4 and the results
sliced back: the convolution zero-pads outside the image anyway, and pad
columns with zero upstream gradient add nothing to dweight or dbias.

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
import torch.nn.functional as F

from . import _ext


class NConv2dFn(torch.autograd.Function):
    """padding, eps and prop_conf are what ops.nconv2d admitted: K // 2,
    1e-20 and True, the values the kernels hard-wire."""

    @staticmethod
    def forward(ctx, data, conf, weight, bias, padding, eps, prop_conf):
        W = data.shape[-1]
        pad = -W % 4
        if pad:
            data = F.pad(data, (0, pad))
            conf = F.pad(conf, (0, pad))
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
        ctx.eps = eps
        ctx.pad = pad
        # an unused output (the cout dropped after nconv_out) then arrives
        # in backward as None instead of a zero-filled plane
        ctx.set_materialize_grads(False)
        if pad:
            return out[..., :W].contiguous(), cout[..., :W].contiguous()
        return out, cout

    @staticmethod
    def backward(ctx, gout, gcout):
        if gout is None and gcout is None:
            return None, None, None, None, None, None, None
        data, conf, weight, out, cout, *maybe_bias = ctx.saved_tensors
        bias = maybe_bias[0] if ctx.has_bias else None
        if ctx.pad:
            gout = F.pad(gout, (0, ctx.pad)) if gout is not None else None
            gcout = F.pad(gcout, (0, ctx.pad)) if gcout is not None else None
        gout = gout.contiguous() if gout is not None else None
        gcout = gcout.contiguous() if gcout is not None else None

        algo = 0 if os.environ.get("FLOWHIP_NCONV_BWD", "") == "split" else -1
        ddata, dconf, dweight, dbias = _ext.ext().nconv_bwd_fused(
            gout, gcout, out, cout, data, conf, weight, bias, ctx.eps, algo)
        if ctx.pad:
            W = data.shape[-1] - ctx.pad
            ddata = ddata[..., :W].contiguous()
            dconf = dconf[..., :W].contiguous()
        if not ctx.needs_input_grad[2]:
            dweight = None
        if not ctx.has_bias:
            dbias = None
        return ddata, dconf, dweight, dbias, None, None, None


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
