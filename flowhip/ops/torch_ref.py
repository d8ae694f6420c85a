"""Pure-PyTorch reference implementations of every flowhip op.

These serve three roles:
  1. the CPU execution path (no GPU required — tests, plumbing, debugging);
  2. the numerical oracle that every HIP kernel is unit-tested against
     (SURVEY.md §4.2 item 2);
  3. the documentation of the exact math each kernel computes, with citations
     into the reference repo.

Every function here is differentiable through torch autograd, except
`forward_splat` (a nearest-source selection) and `fb_consistency` (a mask).
"""

import math

import torch
import torch.nn.functional as F

from ..utils.geometry import bilinear_sampler


# ---------------------------------------------------------------------------
# Correlation volume / pyramid / lookup  (reference core/corr.py)
# ---------------------------------------------------------------------------

def corr_volume(fmap1, fmap2):
    """All-pairs correlation: C[b, i, j] = <f1[b,:,i], f2[b,:,j]> / sqrt(D).

    In:  fmap1, fmap2 (B, D, H, W).
    Out: (B*H*W, 1, H, W) — the reference's post-reshape layout
         (core/corr.py:12-16, 47-55); scaling by 1/sqrt(D) per corr.py:55.
    """
    batch, dim, ht, wd = fmap1.shape
    f1 = fmap1.reshape(batch, dim, ht * wd)
    f2 = fmap2.reshape(batch, dim, ht * wd)
    corr = torch.matmul(f1.transpose(1, 2), f2) / math.sqrt(dim)
    return corr.reshape(batch * ht * wd, 1, ht, wd)


def corr_pyramid(corr, num_levels=4):
    """Build the average-pool pyramid over the *second* image's spatial dims.

    In:  corr (B*H*W, 1, H, W) from `corr_volume`.
    Out: list of `num_levels` tensors, level l at (H/2^l, W/2^l).
    Parity: core/corr.py:18-21.
    """
    pyramid = [corr]
    for _ in range(num_levels - 1):
        corr = F.avg_pool2d(corr, 2, stride=2)
        pyramid.append(corr)
    return pyramid


def corr_lookup(pyramid, coords, radius):
    """Window lookup: for each target pixel, bilinearly sample a
    (2r+1)^2 window around `coords / 2^l` at every pyramid level.

    In:  pyramid — list of L tensors (B*H1*W1, 1, Hl, Wl);
         coords (B, 2, H1, W1) pixel coordinates into level 0.
    Out: (B, L*(2r+1)^2, H1, W1); channel = l*(2r+1)^2 + dy_idx*(2r+1) + dx_idx.
    Parity: core/corr.py:23-44 (delta from meshgrid(dy, dx) 'ij'), sampling via
    bilinear_sampler (= grid_sample align_corners=True, zero padding).
    """
    r = radius
    coords = coords.permute(0, 2, 3, 1)  # (B, H1, W1, 2)
    batch, h1, w1, _ = coords.shape

    out_pyramid = []
    for i, corr in enumerate(pyramid):
        dx = torch.linspace(-r, r, 2 * r + 1, device=coords.device, dtype=coords.dtype)
        dy = torch.linspace(-r, r, 2 * r + 1, device=coords.device, dtype=coords.dtype)
        delta = torch.stack(torch.meshgrid(dy, dx, indexing="ij"), axis=-1)

        centroid_lvl = coords.reshape(batch * h1 * w1, 1, 1, 2) / 2 ** i
        delta_lvl = delta.view(1, 2 * r + 1, 2 * r + 1, 2)
        coords_lvl = centroid_lvl + delta_lvl

        sampled = bilinear_sampler(corr, coords_lvl)
        out_pyramid.append(sampled.view(batch, h1, w1, -1))

    out = torch.cat(out_pyramid, dim=-1)
    return out.permute(0, 3, 1, 2).contiguous().float()


# ---------------------------------------------------------------------------
# On-demand correlation lookup (upstream RAFT's --alternate_corr mode)
# ---------------------------------------------------------------------------

def alt_corr_pyramid(fmap2, num_levels=4):
    """Average-pool pyramid of the *second feature map*.

    Pooling and the dot product are both linear, so correlating against the
    pooled features equals pooling the correlation volume:
    `corr_pyramid(corr_volume(f1, f2))[l][i] == <f1[:, i], levels[l]>/sqrt(D)`
    with the same floor-mode 2x2 pooling.

    In:  fmap2 (B, D, H, W).
    Out: list of `num_levels` tensors (B, D, H/2^l, W/2^l); level 0 = input.
    """
    levels = [fmap2]
    for _ in range(num_levels - 1):
        fmap2 = F.avg_pool2d(fmap2, 2, stride=2)
        levels.append(fmap2)
    return levels


def alt_corr_chunk(f1_rows, fmap2_levels, coords_rows, radius):
    """Window lookup for one chunk of target pixels of ONE batch element.

    In:  f1_rows (n, D) feature rows of the chunk's target pixels;
         fmap2_levels — list of (D, Hl, Wl) pooled maps of that element;
         coords_rows (n, 2) level-0 (x, y) lookup centres.
    Out: (n, L*(2r+1)^2), channel order as `corr_lookup`.
    Per level the (n, Hl, Wl) correlation slab is one matmul; nothing else
    of that size exists.
    """
    r = radius
    n, dim = f1_rows.shape
    d = torch.linspace(-r, r, 2 * r + 1, device=coords_rows.device,
                       dtype=coords_rows.dtype)
    delta = torch.stack(torch.meshgrid(d, d, indexing="ij"), axis=-1)
    delta = delta.view(1, 2 * r + 1, 2 * r + 1, 2)
    out = []
    for lvl, f2 in enumerate(fmap2_levels):
        _, hl, wl = f2.shape
        slab = torch.matmul(f1_rows, f2.reshape(dim, hl * wl)) / math.sqrt(dim)
        centroid = coords_rows.reshape(n, 1, 1, 2) / 2 ** lvl
        sampled = bilinear_sampler(slab.view(n, 1, hl, wl), centroid + delta)
        out.append(sampled.view(n, -1))
    return torch.cat(out, dim=-1)


def alt_corr_lookup(fmap1, fmap2_levels, coords, radius, chunk=1024):
    """`corr_lookup(corr_pyramid(corr_volume(f1, f2), L), coords, r)` without
    the all-pairs volume: target pixels are processed `chunk` at a time, so
    no more than chunk*P correlation values exist at once (under autograd the
    slabs of all chunks are retained for the backward pass; callers that need
    a bounded backward run the chunks one by one — see AltCorrLookupFn).

    In:  fmap1 (B, D, H, W); fmap2_levels from `alt_corr_pyramid`;
         coords (B, 2, H, W).
    Out: (B, L*(2r+1)^2, H, W) fp32.
    """
    batch, dim, ht, wd = fmap1.shape
    npix = ht * wd
    f1 = fmap1.reshape(batch, dim, npix).transpose(1, 2)     # (B, P, D)
    xy = coords.reshape(batch, 2, npix).transpose(1, 2)      # (B, P, 2)
    rows = []
    for b in range(batch):
        lv = [f2[b] for f2 in fmap2_levels]
        parts = [alt_corr_chunk(f1[b, s:s + chunk], lv, xy[b, s:s + chunk],
                                radius)
                 for s in range(0, npix, chunk)]
        rows.append(torch.cat(parts, dim=0))
    out = torch.stack(rows, dim=0)                           # (B, P, C)
    return out.transpose(1, 2).reshape(batch, -1, ht, wd).contiguous().float()


# ---------------------------------------------------------------------------
# Normalized convolution  (reference core/nconv_modules.py:140-216)
# ---------------------------------------------------------------------------

def nconv2d(data, conf, weight, bias=None, stride=1, padding=0, dilation=1,
            groups=1, eps=1e-20, prop_conf=True):
    """Confidence-normalized convolution with confidence propagation.

    out  = conv(data*conf, w) / (conv(conf, w) + eps)  [+ bias]
    cout = conv(conf, w) / sum_per_outchannel(w)

    `weight` is the *effective* (non-negative) weight — the softplus
    reparameterization (EnforcePos, nconv_modules.py:218-265) is applied by
    the calling module, not here.
    Parity: nconv_modules.py:164-199.
    """
    denom = F.conv2d(conf, weight, None, stride, padding, dilation, groups)
    nomin = F.conv2d(data * conf, weight, None, stride, padding, dilation, groups)
    nconv = nomin / (denom + eps)

    if bias is not None:
        nconv = nconv + bias.view(1, -1, 1, 1)

    if prop_conf:
        s = weight.reshape(weight.shape[0], -1).sum(dim=-1).view(1, -1, 1, 1)
        cout = denom / s
    else:
        cout = None
    return nconv, cout


def conf_pool(data, conf, ds_factor=2, pooling_type="conf_based"):
    """Confidence-based 2x downsampling of a (data, conf) pair.

    conf is max-pooled (and divided by 4 — the Jacobian determinant of the
    scale change, nconv_modules.py:97); data keeps the values at the argmax-
    confidence positions (`conf_based`) or is max-pooled itself.
    Parity: nconv_modules.py:94-104 and retrieve_elements_from_indices :19-22.
    """
    conf_ds, idx = F.max_pool2d(conf, ds_factor, ds_factor, return_indices=True)
    conf_ds = conf_ds / 4
    if pooling_type == "conf_based":
        flat = data.flatten(start_dim=2)
        data_ds = flat.gather(dim=2, index=idx.flatten(start_dim=2)).view_as(idx)
    elif pooling_type == "max_pooling":
        data_ds = F.max_pool2d(data, ds_factor, ds_factor)
    else:
        raise NotImplementedError(
            "Choose pooling_type from [conf_based, max_pooling]!")
    return data_ds, conf_ds


# ---------------------------------------------------------------------------
# Sparse zero-injection upsample  (reference core/upsampler.py:179-210)
# ---------------------------------------------------------------------------

def zero_inject(inp, scale_h, scale_w, out_h=None, out_w=None):
    """Place low-res samples on a zero high-res grid at stride s, offset s//2.

    out[:, :, sH//2::sH, sW//2::sW] = inp   (upsampler.py:208)
    """
    b, c, ih, iw = inp.shape
    oh = out_h if out_h is not None else ih * scale_h
    ow = out_w if out_w is not None else iw * scale_w
    out = inp.new_zeros((b, c, oh, ow))
    out[:, :, scale_h // 2::scale_h, scale_w // 2::scale_w] = inp
    return out


# ---------------------------------------------------------------------------
# Warm-start forward splat  (reference core/utils/utils.py:28-56)
# ---------------------------------------------------------------------------

@torch.no_grad()
def forward_splat(flow, return_ties=False, max_pairs=1 << 22):
    """Forward-warp a flow field onto the grid: each cell takes the flow of
    the nearest landed source (the reference's scipy griddata "nearest").
    A selection, so not differentiable (the one such function here).

    Source i = y*W + x sits at (x + dx, y + dy), evaluated in float64 as
    numpy does; it is valid iff 0 < px < W and 0 < py < H (NaN fails). A
    target (tx, ty) copies the valid source with the smallest
    (px-tx)^2 + (py-ty)^2 (float64, each op rounded on its own). Ties go to
    the lowest source index; a sample without a valid source gives zeros
    (scipy: unspecified / raises).

    In:  (B, 2, H, W) or (2, H, W). Out: same shape and dtype, detached.
    return_ties: also return a bool (B, H, W) / (H, W) map of the targets
    whose minimum is attained by more than one source.
    Chunked float64 brute force, at most `max_pairs` pairs per sample at a
    time.
    """
    squeeze = flow.dim() == 3
    fl = flow.detach()[None] if squeeze else flow.detach()
    B, _, H, W = fl.shape
    HW = H * W
    dev = fl.device
    fl = fl.reshape(B, 2, HW)

    gy, gx = torch.meshgrid(
        torch.arange(H, device=dev, dtype=torch.float64),
        torch.arange(W, device=dev, dtype=torch.float64), indexing="ij")
    gx, gy = gx.reshape(-1), gy.reshape(-1)
    px = gx + fl[:, 0].double()
    py = gy + fl[:, 1].double()
    valid = (px > 0) & (px < W) & (py > 0) & (py < H)
    inf = float("inf")
    px = torch.where(valid, px, inf)[:, None, :]   # (B, 1, sources)
    py = torch.where(valid, py, inf)[:, None, :]
    src_idx = torch.arange(HW, device=dev)

    best = torch.empty(B, HW, dtype=torch.long, device=dev)
    found = torch.empty(B, HW, dtype=torch.bool, device=dev)
    ties = torch.empty(B, HW, dtype=torch.bool, device=dev)
    step = max(1, max_pairs // HW)
    for t0 in range(0, HW, step):
        ddx = px - gx[None, t0:t0 + step, None]    # (B, targets, sources)
        ddy = py - gy[None, t0:t0 + step, None]
        d = ddx * ddx + ddy * ddy
        dmin = d.min(dim=2, keepdim=True).values
        hit = (d == dmin) & (dmin < inf)
        # lowest index among the sources that attain the minimum
        best[:, t0:t0 + step] = torch.where(hit, src_idx, HW).min(dim=2).values
        found[:, t0:t0 + step] = dmin[..., 0] < inf
        ties[:, t0:t0 + step] = hit.sum(dim=2) > 1

    idx = best.clamp(max=HW - 1)[:, None, :].expand(B, 2, HW)
    out = torch.where(found[:, None, :], torch.gather(fl, 2, idx),
                      torch.zeros((), dtype=fl.dtype, device=dev))
    out = out.reshape(B, 2, H, W)
    ties = ties.reshape(B, H, W)
    if squeeze:
        out, ties = out[0], ties[0]
    return (out, ties) if return_ties else out


# ---------------------------------------------------------------------------
# Forward-backward consistency check (occlusion mask of a bidirectional pair)
# ---------------------------------------------------------------------------

def _fb_one_direction(f, b, alpha1, alpha2):
    """`f` (N,2,H,W) float64 checked against `b`; see fb_consistency."""
    N, _, H, W = f.shape
    HW = H * W
    dev = f.device
    gy, gx = torch.meshgrid(
        torch.arange(H, device=dev, dtype=torch.float64),
        torch.arange(W, device=dev, dtype=torch.float64), indexing="ij")
    fx, fy = f[:, 0], f[:, 1]
    px = gx + fx
    py = gy + fy
    inframe = (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)
    # out-of-frame lanes sample (0, 0): computed, then masked out below
    px = torch.where(inframe, px, 0.0)
    py = torch.where(inframe, py, 0.0)
    x0 = px.floor().clamp(max=W - 2)
    y0 = py.floor().clamp(max=H - 2)
    wx = px - x0
    wy = py - y0
    i00 = (y0 * W + x0).long().reshape(N, 1, HW).expand(N, 2, HW)
    bb = b.reshape(N, 2, HW)

    def tap(off):
        return torch.gather(bb, 2, i00 + off).reshape(N, 2, H, W)

    wx, wy = wx[:, None], wy[:, None]
    top = tap(0) * (1.0 - wx) + tap(1) * wx
    bot = tap(W) * (1.0 - wx) + tap(W + 1) * wx
    bs = top * (1.0 - wy) + bot * wy
    bx, by = bs[:, 0], bs[:, 1]

    sx = fx + bx
    sy = fy + by
    r2 = sx * sx + sy * sy
    thr = alpha1 * ((fx * fx + fy * fy) + (bx * bx + by * by)) + alpha2
    finite = inframe & torch.isfinite(r2) & torch.isfinite(thr)
    visible = finite & (r2 <= thr)
    r = torch.where(finite, r2, 0.0).sqrt()
    occ = (~visible).to(torch.uint8)[:, None]
    res = torch.where(finite, r, float("inf")).float()[:, None]
    stats = torch.stack([
        visible.sum(dim=(1, 2)).double(),
        (finite & ~visible).sum(dim=(1, 2)).double(),
        (~finite).sum(dim=(1, 2)).double(),
        torch.where(visible, r, 0.0).sum(dim=(1, 2))], dim=1)
    gap = torch.where(finite, (r2 - thr).abs(), float("inf"))
    return occ, res, stats, gap.min()


@torch.no_grad()
def fb_consistency(flow_fw, flow_bw, alpha1=0.01, alpha2=0.5,
                   return_margin=False):
    """Forward-backward consistency of a bidirectional flow pair (the UnFlow
    occlusion test). No gradient.

    `flow_fw` is the 1->2 flow on frame 1's grid, `flow_bw` the 2->1 flow on
    frame 2's grid, both (N, 2, H, W), channel 0 = x, H, W >= 2. One
    direction, `f` checked against `b`, in float64 on the inputs' values,
    every operation rounded on its own:

        p   = (x + f_x, y + f_y)
        in frame iff 0 <= p_x <= W-1 and 0 <= p_y <= H-1 (false for NaN)
        b~  = bilinear sample of b at p: x0 = min(floor(p_x), W-2),
              w_x = p_x - x0, same in y; all four taps are read, so a
              non-finite tap makes b~ non-finite even at weight 0
              top = b00*(1-w_x) + b01*w_x, bot likewise, b~ = top*(1-w_y) + bot*w_y
        r2  = (f_x + b~_x)^2 + (f_y + b~_y)^2
        thr = alpha1 * ((f_x^2 + f_y^2) + (b~_x^2 + b~_y^2)) + alpha2
        visible iff in frame, r2 and thr finite, r2 <= thr

    Returns (occ_fw, occ_bw, res_fw, res_bw, stats):
        occ   uint8 (N,1,H,W), 1 where not visible
        res   fp32 (N,1,H,W), sqrt(r2); +inf out of frame or non-finite
        stats fp64 (N,2,4), per sample and direction (0 = fw, 1 = bw):
              visible count, in-frame-but-inconsistent count,
              out-of-frame-or-non-finite count, sum of sqrt(r2) over visible
    return_margin: also return the smallest |r2 - thr| over the finite
    in-frame pixels of both directions (inf when there is none): how far the
    closest decision sits from its threshold.
    """
    if (flow_fw.dim() != 4 or flow_fw.shape[1] != 2
            or flow_fw.shape != flow_bw.shape
            or flow_fw.shape[2] < 2 or flow_fw.shape[3] < 2):
        raise ValueError(
            "fb_consistency: two (N,2,H,W) flows of one shape, H, W >= 2; got "
            f"{tuple(flow_fw.shape)} and {tuple(flow_bw.shape)}")
    f = flow_fw.detach().double()
    b = flow_bw.detach().double()
    occ_fw, res_fw, st_fw, gap_fw = _fb_one_direction(f, b, alpha1, alpha2)
    occ_bw, res_bw, st_bw, gap_bw = _fb_one_direction(b, f, alpha1, alpha2)
    out = (occ_fw, occ_bw, res_fw, res_bw, torch.stack([st_fw, st_bw], dim=1))
    if return_margin:
        return out + (torch.minimum(gap_fw, gap_bw),)
    return out


# ---------------------------------------------------------------------------
# Convex-combination upsample  (reference core/raft.py:73-84)
# ---------------------------------------------------------------------------

def convex_upsample(flow, mask, factor=8):
    """x`factor` upsample of flow as a learned convex combination of each
    coarse pixel's 3x3 neighborhood; mask holds 9 logits per output subpixel.

    In:  flow (N, 2, H, W); mask (N, 9*factor*factor, H, W).
    Out: (N, 2, factor*H, factor*W); flow values scaled by `factor`.
    Parity: raft.py:73-84 (softmax over the 9 taps, unfold 3x3 pad 1,
    permute to pixel-shuffle layout).
    """
    N, _, H, W = flow.shape
    mask = mask.view(N, 1, 9, factor, factor, H, W)
    mask = torch.softmax(mask, dim=2)

    up_flow = F.unfold(factor * flow, [3, 3], padding=1)
    up_flow = up_flow.view(N, 2, 9, 1, 1, H, W)

    up_flow = torch.sum(mask * up_flow, dim=2)
    up_flow = up_flow.permute(0, 1, 4, 2, 5, 3)
    return up_flow.reshape(N, 2, factor * H, factor * W)


# ---------------------------------------------------------------------------
# Sequence loss  (reference train.py:43-71)
# ---------------------------------------------------------------------------

MAX_FLOW = 400


def sequence_loss(flow_preds, flow_gt, valid, gamma=0.8, max_flow=MAX_FLOW):
    """Exponentially weighted L1 over the iteration sequence + EPE metrics.

    Weight of prediction i (of n) is gamma^(n-1-i) — later iterations weigh
    more. Pixels with valid < 0.5 or ||gt|| >= max_flow are excluded.
    Metrics are computed on the final prediction only.
    Parity: train.py:46-71.
    """
    n_predictions = len(flow_preds)
    flow_loss = 0.0

    mag = torch.sum(flow_gt ** 2, dim=1).sqrt()
    valid = (valid >= 0.5) & (mag < max_flow)

    for i in range(n_predictions):
        i_weight = gamma ** (n_predictions - i - 1)
        i_loss = (flow_preds[i] - flow_gt).abs()
        flow_loss += i_weight * (valid[:, None] * i_loss).mean()

    epe = torch.sum((flow_preds[-1] - flow_gt) ** 2, dim=1).sqrt()
    epe = epe.view(-1)[valid.view(-1)]

    metrics = {
        "epe": epe.mean().item(),
        "1px": (epe < 1).float().mean().item(),
        "3px": (epe < 3).float().mean().item(),
        "5px": (epe < 5).float().mean().item(),
    }
    return flow_loss, metrics
