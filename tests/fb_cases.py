"""Seeded inputs and a naive oracle for the forward-backward consistency
tests (CPU twin and GPU kernel)."""

import functools
import math

import numpy as np
import torch

FB_INPUTS = ["zeros", "translation", "smooth", "random", "nonfinite"]

TRANSLATION = (3.25, -2.5)

# (y, x, channel, value) written into every sample of `smooth`; all inside
# the smallest test shape (5, 7)
NAN, INF = float("nan"), float("inf")
POISON_F = [(1, 2, 0, NAN), (2, 4, 1, INF), (0, 0, 0, -INF),
            (3, 1, 0, 1e30), (4, 5, 1, -1e30), (2, 0, 1, 1e6)]
POISON_B = [(3, 3, 0, NAN), (1, 5, 1, INF), (4, 0, 0, -INF),
            (0, 3, 1, 1e30), (2, 2, 0, -1e30), (4, 6, 0, 1e6)]


def _smooth(N, H, W):
    y = torch.arange(H, dtype=torch.float64)[:, None].expand(H, W)
    x = torch.arange(W, dtype=torch.float64)[None, :].expand(H, W)
    f = torch.stack([2.375 + 1.5 * torch.sin(y / 7),
                     -1.625 + torch.cos(x / 9)]).float()
    f = f[None].repeat(N, 1, 1, 1)
    g = torch.Generator().manual_seed(100 * H + W)
    b = -f + 0.6 * torch.randn(N, 2, H, W, generator=g)
    return f, b


@functools.lru_cache(maxsize=None)
def fb_input(name, N, H, W):
    """(flow_fw, flow_bw) fp32 CPU tensors, built once per (name, shape) and
    shared (read-only)."""
    if name == "zeros":
        return torch.zeros(N, 2, H, W), torch.zeros(N, 2, H, W)
    if name == "translation":
        f = torch.empty(N, 2, H, W)
        f[:, 0] = TRANSLATION[0]
        f[:, 1] = TRANSLATION[1]
        return f, -f
    if name == "smooth":
        return _smooth(N, H, W)
    if name == "random":
        g = torch.Generator().manual_seed(7 * H + W)
        return (3 * torch.randn(N, 2, H, W, generator=g),
                3 * torch.randn(N, 2, H, W, generator=g))
    if name == "nonfinite":
        f, b = (t.clone() for t in _smooth(N, H, W))
        for y, x, c, v in POISON_F:
            f[:, c, y, x] = v
        for y, x, c, v in POISON_B:
            b[:, c, y, x] = v
        return f, b
    raise KeyError(name)


def naive_direction(f, b, alpha1=0.01, alpha2=0.5):
    """One direction of the check, one pixel at a time in Python floats
    (IEEE double, no fused operations). f, b: (2, H, W) arrays.
    Returns occ (H, W) uint8, res (H, W) float64, [vis, inc, out, sum]."""
    _, H, W = f.shape
    occ = np.ones((H, W), np.uint8)
    res = np.full((H, W), np.inf)
    counts = [0, 0, 0]
    total = []
    for y in range(H):
        for x in range(W):
            fx, fy = float(f[0, y, x]), float(f[1, y, x])
            px, py = x + fx, y + fy
            if not (0 <= px <= W - 1 and 0 <= py <= H - 1):
                counts[2] += 1
                continue
            x0 = min(int(math.floor(px)), W - 2)
            y0 = min(int(math.floor(py)), H - 2)
            wx, wy = px - x0, py - y0
            s = []
            for c in range(2):
                b00, b01 = float(b[c, y0, x0]), float(b[c, y0, x0 + 1])
                b10, b11 = float(b[c, y0 + 1, x0]), float(b[c, y0 + 1, x0 + 1])
                top = b00 * (1.0 - wx) + b01 * wx
                bot = b10 * (1.0 - wx) + b11 * wx
                s.append(top * (1.0 - wy) + bot * wy)
            sx, sy = fx + s[0], fy + s[1]
            r2 = sx * sx + sy * sy
            thr = alpha1 * ((fx * fx + fy * fy)
                            + (s[0] * s[0] + s[1] * s[1])) + alpha2
            if not (math.isfinite(r2) and math.isfinite(thr)):
                counts[2] += 1
                continue
            res[y, x] = math.sqrt(r2)
            if r2 <= thr:
                occ[y, x] = 0
                counts[0] += 1
                total.append(res[y, x])
            else:
                counts[1] += 1
    return occ, res, counts + [math.fsum(total)]


def bits_equal(a, b):
    """Bit-for-bit equality of two tensors of one dtype and shape."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    a, b = a.contiguous().cpu(), b.contiguous().cpu()
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    elif a.dtype == torch.float64:
        a, b = a.view(torch.int64), b.view(torch.int64)
    return torch.equal(a, b)
