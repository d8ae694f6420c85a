"""Implicit-GEMM conv (kernel #5) autograd binding for the update block.

Routes the stride-1 same-padding NHWC bf16 convolutions of the motion
encoder / SepConvGRU / flow head (reference update.py:6-146) onto the
hand-written MFMA kernel in csrc/conv_gemm.hip. The packed bf16 weights
([kyx][o][c_pad] for forward, flipped/transposed for backward-data) are
cached per weight version so they are rebuilt only after optimizer steps.

  forward:   out = conv(x, w) + b          (one kernel)
  bwd-data:  dx  = conv(dy, flipT(w))      (same kernel, swapped packing)
  bwd-wrw:   dW  = split-M MFMA partials + reduce (fp32)
  bwd-bias:  per-chunk column sums from the same partials kernel

Convs whose padded input has exactly 8 channels (the 7x7 encoder stems and
convf1) take the tap-folded kernels of csrc/conv_fold.h: the forward through
a folded pack chosen here (_fold_ok), the weight gradient through the
extension's plan (path 2). FLOWHIP_CONV_FOLD=0 switches both off.

Inside wrw_accumulate_scope() (the models open it around the refinement
loop) a conv that is called K times with the same weights sums its K weight
gradients natively and hands the parameter ONE gradient, from the backward
of a sink node placed between the parameter and its K uses (WrwSinkFn):
in one partials buffer reduced once where that measured faster, else by a
reduce that adds into the running dW (_wrw; the rule sits next to the plan
code in csrc/conv_gemm.h).
"""

import contextlib
import os
import threading

import torch
import torch.nn.functional as F
from torch.nn.modules.utils import _pair

from . import _ext


def _pad64(n):
    return (n + 63) // 64 * 64


def _pad_x8(x, pad):
    z = x.new_zeros(x.shape[0], pad, x.shape[2], x.shape[3]).contiguous(
        memory_format=torch.channels_last)
    return torch.cat([x, z], dim=1)


def _pad_c8(x, weight):
    """Channel-pad input AND weight to a multiple of 8 via differentiable
    cats. The staging kernel reads whole 16-B pieces; with Cin % 8 != 0 the
    tail piece of the last pixel would read past the tensor allocation
    (fault, allocator-layout dependent). Zero input channels x zero weight
    columns = identical math, all reads in-bounds."""
    O, I, KH, KW = weight.shape
    pad = (-I) % 8
    if pad == 0:
        return x, weight
    xp = _pad_x8(x, pad)
    wz = weight.new_zeros(O, pad, KH, KW)
    wp = torch.cat([weight, wz], dim=1)
    return xp, wp


def _dy_bf16_cl8(dy):
    """The backward prologue: dy as bf16, channels-last, channel-padded to
    a multiple of 8 -> (padded dy, real Cout). Same OOB-tail argument as
    _pad_c8; the packed-bwd weight k-columns beyond Cout are zero, so
    padded dy channels contribute nothing."""
    dy = dy.contiguous(memory_format=torch.channels_last)
    if dy.dtype != torch.bfloat16:
        dy = dy.to(torch.bfloat16)
    O = dy.shape[1]
    pad = (-O) % 8
    return (_pad_x8(dy, pad) if pad else dy), O


def _log_fallback(tag, x, describe):
    """FLOWHIP_LOG_FALLBACK=1 names every GPU conv that leaves the MFMA
    path for F.conv2d."""
    if x.is_cuda and os.environ.get("FLOWHIP_LOG_FALLBACK", "0") == "1":
        print(f"[{tag} fallback] {describe()}", flush=True)


def conv_fold_enabled():
    """FLOWHIP_CONV_FOLD=0 keeps the small-Cin convs off the tap-folded
    kernels (A/B switch; default on). The extension reads the variable, for
    its auto weight-gradient plan and for the pack choice here."""
    return _ext.ext().conv_fold_enabled()


def _fold_ok(x, weight):
    """The folded envelope (csrc/conv_fold.h) for a conv can_fuse_conv
    accepted: 8 input channels in whole 16-byte pixels, KW <= 8."""
    return (conv_fold_enabled() and weight.shape[1] == 8
            and weight.shape[3] <= 8 and x.stride(3) % 8 == 0)


def _pack_fwd(weight, fold=False):
    """(O, I, KH, KW) fp32 -> (KYX, O, pad64(I)) bf16 contiguous; folded:
    (KH, O, 64) with column kx * 8 + c."""
    w = weight.detach()
    if w.is_cuda and w.dtype == torch.float32:
        return _ext.ext().conv_gemm_pack(w.contiguous(), False, fold)
    O, I, KH, KW = w.shape
    if fold:
        w = w.to(torch.bfloat16).permute(2, 0, 3, 1)  # (KH, O, KW, I)
        w = F.pad(w, (0, 8 - I, 0, 8 - KW))
        return w.reshape(KH, O, 64).contiguous()
    w = w.to(torch.bfloat16).permute(2, 3, 0, 1).reshape(KH * KW, O, I)
    return F.pad(w, (0, _pad64(I) - I)).contiguous()


def _pack_bwd(weight):
    """flip + transpose: (O, I, KH, KW) -> (KYX, I, pad64(O)) bf16."""
    w = weight.detach()
    if w.is_cuda and w.dtype == torch.float32:
        return _ext.ext().conv_gemm_pack(w.contiguous(), True)
    O, I, KH, KW = w.shape
    w = w.to(torch.bfloat16).flip(2, 3).permute(2, 3, 1, 0)
    w = w.reshape(KH * KW, I, O)
    return F.pad(w, (0, _pad64(O) - O)).contiguous()


def _weight_key(*tensors):
    """Cache key of what is derived from these parameters: changes with an
    optimizer step (in place, _version) and with a rebound tensor."""
    return tuple(v for t in tensors for v in (t.data_ptr(), t._version))


def _packs(weight, cache, key=None, fold=False):
    if key is None:
        key = _weight_key(weight)
    if cache.get("k") != key or cache.get("fold", False) != fold:
        cache["k"] = key
        cache["fold"] = fold
        cache["fwd"] = _pack_fwd(weight, fold)
        cache["bwd"] = _pack_bwd(weight)
    return cache["fwd"], cache["bwd"]


# ---------------------------------------------------------------------------
# Shared weight gradients: one partials buffer per weight and backward pass
# ---------------------------------------------------------------------------
_tls = threading.local()


def wrw_accum_enabled():
    """FLOWHIP_WRW_ACCUM=0 keeps every conv on the one-shot weight-gradient
    path (A/B switch; default on)."""
    return os.environ.get("FLOWHIP_WRW_ACCUM", "1") != "0"


@contextlib.contextmanager
def wrw_accumulate_scope():
    """Convs called inside the scope with grad enabled share one weight
    handle per conv (created at its first call). A no-op off-GPU, under
    no_grad and for weights that need no gradient: no handle is made."""
    if not wrw_accum_enabled():
        yield
        return
    prev = getattr(_tls, "handles", None)
    _tls.handles = {}
    try:
        yield
    finally:
        _tls.handles = prev


class _WrwHandle:
    """State shared by the backward calls of one weight's uses."""

    __slots__ = ("buf", "live", "plan", "geom", "dw", "db")

    def __init__(self):
        self.buf = None    # partials buffer, kept until the sink runs
        self.live = False  # buf holds the summed partials of earlier calls
        self.plan = None   # (path, nchunk, numel, accumulate) buf is for;
        #                    path 2 (folded) has a buffer layout of its own
        self.geom = None   # (Cout padded to 8, Cin, KH, KW, has_bias)
        self.dw = None     # running sums of the calls already reduced,
        self.db = None     # over the padded Cout


class WrwSinkFn(torch.autograd.Function):
    """Identity on (weight, bias) whose backward finishes the handle.

    The convs in the scope take the sink's outputs, so by graph order the
    sink's backward runs after the backward of every use. Those leave
    their gradients in the handle (_wrw) and return None for weight and
    bias; here a live partials buffer is reduced, once, and everything is
    released. A gradient that reaches the outputs by an ordinary route is
    added."""

    @staticmethod
    def forward(ctx, handle, weight, bias):
        ctx.set_materialize_grads(False)
        ctx.handle = handle
        ctx.O = weight.shape[0]
        if bias is None:
            return weight.view_as(weight), None
        return weight.view_as(weight), bias.view_as(bias)

    @staticmethod
    def backward(ctx, gw, gb):
        h = ctx.handle
        dw, db = h.dw, h.db
        if h.live:
            dw, db = _finish_into_running(h)
        h.buf = h.dw = h.db = None
        h.live = False
        if dw is not None:
            dw = dw[:ctx.O]
            if db is not None:
                db = db[:ctx.O]
        if gw is not None:
            dw = gw if dw is None else dw + gw
        if gb is not None:
            db = gb if db is None else db + gb
        return None, dw, db


def _finish_into_running(h):
    """Reduce the handle's partials buffer and add the sums to its running
    (dw, db), made here on the first call -> the new (dw, db)."""
    Op, Cin, KH, KW, has_bias = h.geom
    dw, db = _ext.ext().conv_gemm_wrw_finish(
        h.buf, Op, Cin, KH, KW, has_bias, h.plan[1], h.dw,
        h.db if has_bias else None, h.plan[0])
    return dw, (db if has_bias else None)


def _scope_entry(cache, key, weight, bias, pad8=False):
    """(handle, weight view, bias view) of this conv in the open scope,
    made at the conv's first call; None outside a scope, under no_grad or
    when neither tensor needs a gradient. `weight` may be a callable that
    builds the tensor to differentiate (the packed z+r pair), run once."""
    handles = getattr(_tls, "handles", None)
    if handles is None or not torch.is_grad_enabled():
        return None
    k = (id(cache), key, pad8)
    ent = handles.get(k)
    if ent is None:
        if callable(weight):
            weight, bias = weight()
        if pad8:
            # the 8-padded weight is what the Function differentiates: the
            # zero-column cat and its backward run once per scope
            O, I, KH, KW = weight.shape
            weight = torch.cat(
                [weight, weight.new_zeros(O, (-I) % 8, KH, KW)], dim=1)
        if not (weight.requires_grad
                or (bias is not None and bias.requires_grad)):
            ent = False
        else:
            h = _WrwHandle()
            wh, bh = WrwSinkFn.apply(h, weight, bias)
            ent = (h, wh, bh)
        handles[k] = ent
    return ent or None


def _wrw(handle, dyp, x, x2, KH, KW, sH, sW, has_bias, O_real):
    """Weight / bias gradient of one conv call -> (dw, dbias). With a
    handle the gradient stays in the handle and both are None: the sink
    returns the sum over the calls. Where the plan says accumulation wins,
    the call's partials are summed into the handle's buffer and the sink
    reduces once; elsewhere the call's reduce adds to the running dW, which
    saves autograd's add launches only."""
    E = _ext.ext()
    if handle is None:
        dw, db = E.conv_gemm_wrw(dyp, x, x2, KH, KW, sH, sW, has_bias)
        if dw.shape[0] != O_real:
            dw = dw[:O_real].contiguous()
        return dw, (db[:O_real] if has_bias else None)
    h = handle
    plan = tuple(E.conv_gemm_wrw_plan(dyp, x, x2, KH, KW, sH, sW, has_bias))
    Cin = x.shape[1] + (x2.shape[1] if x2 is not None else 0)
    geom = (dyp.shape[1], Cin, KH, KW, has_bias)
    if h.buf is None:
        h.buf = torch.empty(plan[2], dtype=torch.float32, device=x.device)
        h.plan, h.geom = plan, geom
    if (plan, geom) != (h.plan, h.geom):
        # another resolution than the buffer was planned for: one-shot
        dw, db = E.conv_gemm_wrw(dyp, x, x2, KH, KW, sH, sW, has_bias)
        h.dw = dw if h.dw is None else h.dw + dw
        if has_bias:
            h.db = db if h.db is None else h.db + db
        return None, None
    path, nchunk, _, accumulate = plan
    E.conv_gemm_wrw_partials(dyp, x, x2, h.buf, KH, KW, sH, sW, has_bias,
                             h.live, path, nchunk)
    if accumulate:
        h.live = True
    else:
        h.dw, h.db = _finish_into_running(h)
    return None, None


class ConvGemmFn(torch.autograd.Function):
    """Same-padding conv on the MFMA kernel over x or, with x2 given, over
    the virtually-concatenated pair cat([x, x2], 1): no per-call cat
    materialization and no backward narrows (4 per GRU iteration); x's
    channel count must then be a multiple of 64. Stride 1, or strided
    (smode 1 fwd / smode 2 bwd-data) with a single source. fold: wpk_fwd
    is a folded pack (the forward only; the backward-data keeps the
    generic pack and the weight gradient plans its own path)."""

    @staticmethod
    def forward(ctx, x, x2, weight, bias, wpk_fwd, wpk_bwd, sH, sW,
                handle=None, fold=False):
        O, I, KH, KW = weight.shape
        b = bias.detach().float().contiguous() if bias is not None else None
        smode = 0 if (sH, sW) == (1, 1) else 1
        out = _ext.ext().conv_gemm_fwd2(x, x2, wpk_fwd, b, O, KH, KW, 0, 0,
                                        sH, sW, smode, 0, 0, fold)[0]
        ctx.save_for_backward(x, x2, wpk_bwd)
        ctx.meta = (I, KH, KW, bias is not None, sH, sW)
        ctx.handle = handle
        return out

    @staticmethod
    def backward(ctx, dy):
        x, x2, wpk_bwd = ctx.saved_tensors
        I, KH, KW, has_bias, sH, sW = ctx.meta
        dyp, O_real = _dy_bf16_cl8(dy)
        dx = dx2 = None
        if x2 is not None:
            dx, dx2 = _ext.ext().conv_gemm_fwd2(dyp, None, wpk_bwd, None, I,
                                                KH, KW, x.shape[1], 0)
        elif ctx.needs_input_grad[0]:  # leaf inputs (the stem images) skip dx
            smode = 0 if (sH, sW) == (1, 1) else 2
            dx = _ext.ext().conv_gemm_fwd2(dyp, None, wpk_bwd, None, I, KH,
                                           KW, 0, 0, sH, sW, smode,
                                           x.shape[2], x.shape[3])[0]
        dw = dbias = None
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
            dw, dbias = _wrw(ctx.handle, dyp, x, x2, KH, KW, sH, sW,
                             has_bias, O_real)
        return dx, dx2, dw, dbias, None, None, None, None, None, None


def can_fuse_conv(x, weight, stride, padding, dilation, groups):
    if not (x.is_cuda and x.dim() == 4 and x.dtype == torch.bfloat16):
        return False
    if x.stride(1) != 1:  # channels-last-like only
        return False
    if _ext.ext() is None or _ext.force_ref():
        return False
    if (_pair(stride) not in ((1, 1), (2, 2))
            or _pair(dilation) != (1, 1) or groups != 1):
        return False
    O, I, KH, KW = weight.shape
    if _pair(padding) != (KH // 2, KW // 2):
        return False
    if I != x.shape[1] or O > 512 or KH * KW > 49:
        return False
    if x.stride(3) < x.size(1):
        return False
    if I % 8 != 0 and x.stride(3) != x.size(1):
        # narrowed view with ragged Cin: the 16-B tail piece must stay
        # inside the row (the padded-allocation case has ld % 8 == 0)
        if x.stride(3) % 8 != 0 or x.stride(3) < I + ((-I) % 8):
            return False
    return True


def fused_conv2d(x, weight, bias, stride, padding, dilation, groups, cache,
                 key=None):
    """F.conv2d drop-in that routes supported shapes to the MFMA kernel."""
    # autocast does NOT auto-cast custom autograd Functions: an fp32 input
    # under an active bf16 autocast region (convc1's corr features, convf1's
    # flow) would silently fall back to MIOpen — do autocast's cast here
    if (x.is_cuda and x.dtype == torch.float32
            and torch.is_autocast_enabled("cuda")
            and torch.get_autocast_dtype("cuda") == torch.bfloat16):
        xc = x.to(torch.bfloat16)
        if xc.stride(1) != 1 or not xc.is_contiguous(
                memory_format=torch.channels_last):
            xc = xc.contiguous(memory_format=torch.channels_last)
        if can_fuse_conv(xc, weight, stride, padding, dilation, groups):
            x = xc
    if can_fuse_conv(x, weight, stride, padding, dilation, groups):
        if key is None:
            key = _weight_key(weight)
        # ragged Cin on a tight row: pad both (16-B staging tail).
        # A channel-narrowed view with padded ld (the corr-lookup
        # output) needs NO pad — its tail bytes are in-row and the
        # packed weight's zero columns null them (saves a full-tensor
        # cat copy per GRU iteration).
        pad8 = weight.shape[1] % 8 != 0 and x.stride(3) == x.size(1)
        ent = _scope_entry(cache, key, weight, bias, pad8)
        handle = None
        if ent is not None:
            handle, wh, bias = ent
            if pad8:
                x = _pad_x8(x, (-weight.shape[1]) % 8)
            weight = wh
        elif pad8:
            x, weight = _pad_c8(x, weight)
        fold = _fold_ok(x, weight)
        wf, wb = _packs(weight, cache, key, fold)
        sH, sW = _pair(stride)
        return ConvGemmFn.apply(x, None, weight, bias, wf, wb, sH, sW,
                                handle, fold)
    _log_fallback("conv", x, lambda: (
        f"w={tuple(weight.shape)} stride={stride} "
        f"pad={padding} dil={dilation} g={groups} x={tuple(x.shape)} "
        f"xs={x.stride()} dt={x.dtype}"))
    return F.conv2d(x, weight, bias, stride, padding, dilation, groups)


class ConvGemmCat2ZrFn(torch.autograd.Function):
    """Packed z+r gate convolution over the virtually-concatenated GRU
    input: ONE kernel computes conv(cat([h, x]), cat([wz, wr])) without
    materializing either cat. The packed weights/bias are cached per
    parameter version (rebuilt after optimizer steps only); gradients are
    routed back to the four separate parameters by slicing — replaces the
    per-call torch.cat of weights AND its CatBackward (4 cat launches per
    GRU pass)."""

    @staticmethod
    def forward(ctx, x1, x2, wz, wr, bz, br, bias_f, wpk_fwd, wpk_bwd):
        Oz, I, KH, KW = wz.shape
        O = Oz + wr.shape[0]
        out = _ext.ext().conv_gemm_fwd2(x1, x2, wpk_fwd, bias_f, O, KH, KW,
                                        0, 0)[0]
        ctx.save_for_backward(x1, x2, wpk_bwd)
        ctx.meta = (O, Oz, I, KH, KW, x1.shape[1])
        return out

    @staticmethod
    def backward(ctx, dy):
        x1, x2, wpk_bwd = ctx.saved_tensors
        O, Oz, I, KH, KW, C1 = ctx.meta
        dy, _ = _dy_bf16_cl8(dy)
        dx1, dx2 = _ext.ext().conv_gemm_fwd2(dy, None, wpk_bwd, None, I, KH,
                                             KW, C1, 0)
        if not any(ctx.needs_input_grad[2:6]):
            return dx1, dx2, None, None, None, None, None, None, None
        dw, db = _ext.ext().conv_gemm_wrw(dy, x1, x2, KH, KW, 1, 1, True)
        return (dx1, dx2, dw[:Oz], dw[Oz:O].contiguous(), db[:Oz],
                db[Oz:O].contiguous(), None, None, None)


def _can_fuse_cat2(x1, x2, KH, KW, padding):
    """Two bf16 channels-last sources on the GPU whose first fills whole
    64-channel slabs, same padding."""
    return (x1.is_cuda and x1.dtype == torch.bfloat16
            and x2.dtype == torch.bfloat16
            and x1.shape[1] % 64 == 0
            and (x1.shape[1] + x2.shape[1]) % 8 == 0  # 16-B staging tail
            and x1.stride(1) == 1 and x2.stride(1) == 1
            and _ext.ext() is not None and not _ext.force_ref()
            and _pair(padding) == (KH // 2, KW // 2))


def fused_gru_zr_conv(h, x, convz, convr, padding, cache):
    """conv2d(cat([h, x]), cat([wz, wr])) + cat([bz, br]) in one fused
    kernel with version-cached packing. Falls back to the eager
    composition off-GPU."""
    O1, I, KH, KW = convz.weight.shape
    if _can_fuse_cat2(h, x, KH, KW, padding):
        key = _weight_key(convz.weight, convr.weight, convz.bias, convr.bias)
        if cache.get("k") != key:
            with torch.no_grad():
                w = torch.cat([convz.weight, convr.weight])
                cache["k"] = key
                cache["fwd"] = _pack_fwd(w)
                cache["bwd"] = _pack_bwd(w)
                cache["bias"] = torch.cat([convz.bias, convr.bias]) \
                    .float().contiguous()
        ent = _scope_entry(cache, key, lambda: (
            torch.cat([convz.weight, convr.weight]),
            torch.cat([convz.bias, convr.bias])), None)
        if ent is not None:
            # the packed pair is what the Function differentiates: one
            # weight cat (and its backward slices) per scope, and the two
            # gates' gradients share one partials buffer
            handle, wh, bh = ent
            return ConvGemmFn.apply(h, x, wh, bh, cache["fwd"], cache["bwd"],
                                    1, 1, handle)
        return ConvGemmCat2ZrFn.apply(h, x, convz.weight, convr.weight,
                                      convz.bias, convr.bias, cache["bias"],
                                      cache["fwd"], cache["bwd"])
    _log_fallback("zr", h, lambda: (
        f"h={tuple(h.shape)} hd={h.dtype} "
        f"hs={h.stride()} x={tuple(x.shape)} xd={x.dtype} "
        f"xs={x.stride()} pad={padding} K=({KH},{KW})"))
    zr_w = torch.cat([convz.weight, convr.weight])
    zr_b = torch.cat([convz.bias, convr.bias])
    hx = torch.cat([h, x], dim=1)
    return F.conv2d(hx, zr_w, zr_b, padding=padding)


def fused_conv2d_cat2(x1, x2, weight, bias, padding, cache, key=None):
    """conv2d(cat([x1, x2], 1), weight) without materializing the cat.
    Falls back to the eager cat + F.conv2d outside the fused envelope."""
    O, I, KH, KW = weight.shape
    if _can_fuse_cat2(x1, x2, KH, KW, padding):
        if key is None:
            key = _weight_key(weight)
        wf, wb = _packs(weight, cache, key)
        ent = _scope_entry(cache, key, weight, bias)
        handle = None
        if ent is not None:
            handle, weight, bias = ent
        return ConvGemmFn.apply(x1, x2, weight, bias, wf, wb, 1, 1, handle)
    _log_fallback("cat2", x1, lambda: (
        f"x1={tuple(x1.shape)} d={x1.dtype} "
        f"s={x1.stride()} x2={tuple(x2.shape)} d2={x2.dtype} "
        f"s2={x2.stride()} w={tuple(weight.shape)} pad={padding}"))
    hx = torch.cat([x1, x2], dim=1)
    return F.conv2d(hx, weight, bias, padding=padding)
