"""Per-element reference of the spatial transformer (trainer/transformer.py:11-31 -> F.grid_sample(bilinear, border,
align_corners=True)) and its backward, for the tests of csrc/loss_stn.hip.

The sample COORDINATES are computed in float32, one rounded operation at a time in the order the reference program (and the
kernel's warp_coord) uses: the training starts from flows of ~1e-5, where the coordinates sit next to integers and d/dflow jumps
with the cell floor() picks -- a float64 oracle picks other cells (tests/test_stn_ref.py records that).  numpy float32 arithmetic
is IEEE, so these are the bits every correct float32 implementation produces.  Everything AFTER the coordinates -- floor, the
four weights, the gather, the d_flow formulas and the scatter into d_src -- is float64.
"""
import numpy as np
import torch


def _coord(g, f, size):
    """float32 numpy: pixel index g + flow f -> clipped source coordinate and the 0 / 1 multiplier of d(coord)/d(flow)."""
    sm1 = np.float32(size - 1)
    loc = (g + f).astype(np.float32)
    loc = (loc / sm1).astype(np.float32)
    loc = (loc - np.float32(0.5)).astype(np.float32)
    loc = (np.float32(2.0) * loc).astype(np.float32)
    u = (loc + np.float32(1.0)).astype(np.float32)
    u = (u / np.float32(2.0)).astype(np.float32)
    u = (u * sm1).astype(np.float32)
    mult = ((u > 0) & (u < sm1)).astype(np.float64)
    u = np.minimum(np.maximum(u, np.float32(0.0)), sm1)
    assert u.dtype == np.float32
    return torch.from_numpy(u.astype(np.float64)), torch.from_numpy(mult)


def warp_coords(flow):
    """flow (B, 2, H, W), any device / strides -> iy, my, ix, mx as float64 CPU tensors (B, H, W)."""
    f = flow.detach().to("cpu", torch.float32).contiguous().numpy()
    _, _, h, w = f.shape
    gy = np.arange(h, dtype=np.float32).reshape(1, h, 1)
    gx = np.arange(w, dtype=np.float32).reshape(1, 1, w)
    iy, my = _coord(gy, f[:, 0], h)
    ix, mx = _coord(gx, f[:, 1], w)
    return iy, my, ix, mx


def warp_ref(src, flow, gout):
    """src, gout (B, 1, H, W), flow (B, 2, H, W) -> out, d_src, d_flow, k, S (float64 CPU tensors).

    k[dest] counts the contributions scattered to a destination of d_src (those of weight 0 included: they are still added).
    S = {"out", "d_src", "d_flow"}: per element of each result, the sum of the |terms| that went into it.  The neighbour at
    x1 == W or y1 == H does not exist and is skipped (its weight is 0 there anyway)."""
    b, _, h, w = flow.shape
    iy, my, ix, mx = warp_coords(flow)
    s = src.detach().to("cpu", torch.float64).reshape(b, h * w)
    g = gout.detach().to("cpu", torch.float64).reshape(b, h, w)
    fy, fx = torch.floor(iy), torch.floor(ix)
    y0, x0 = fy.long(), fx.long()
    y1, x1 = y0 + 1, x0 + 1
    wx1, wx0, wy1, wy0 = ix - fx, (fx + 1.0) - ix, iy - fy, (fy + 1.0) - iy
    bx, by = x1 < w, y1 < h
    x1c, y1c = x1.clamp(max=w - 1), y1.clamp(max=h - 1)

    def gather(yy, xx, ok):
        v = torch.gather(s, 1, (yy * w + xx).reshape(b, h * w)).reshape(b, h, w)
        return torch.where(ok, v, torch.zeros_like(v))

    ok_nw = torch.ones_like(bx)
    corners = ((y0, x0, ok_nw, wx0 * wy0), (y0, x1c, bx, wx1 * wy0), (y1c, x0, by, wx0 * wy1), (y1c, x1c, bx & by, wx1 * wy1))
    vals = [gather(yy, xx, ok) for yy, xx, ok, _ in corners]
    vnw, vne, vsw, vse = vals
    out = sum(v * c[3] for v, c in zip(vals, corners))
    s_out = sum(v.abs() * c[3] for v, c in zip(vals, corners))

    n = b * h * w
    d_src, k, s_src = (torch.zeros(n, dtype=torch.float64) for _ in range(3))
    base = (torch.arange(b) * h * w).view(b, 1, 1)
    for yy, xx, ok, wt in corners:
        idx = (base + yy * w + xx).reshape(-1)          # (clamped coordinates: a skipped neighbour adds 0 to a valid place)
        okf = ok.reshape(-1).double()
        t = (wt * g).reshape(-1) * okf
        d_src += torch.bincount(idx, weights=t, minlength=n)
        s_src += torch.bincount(idx, weights=t.abs(), minlength=n)
        k += torch.bincount(idx, weights=okf, minlength=n)

    gix = (-vnw * wy0 + vne * wy0 - vsw * wy1 + vse * wy1) * g
    giy = (-vnw * wx0 - vne * wx1 + vsw * wx0 + vse * wx1) * g
    s_gix = (vnw.abs() * wy0 + vne.abs() * wy0 + vsw.abs() * wy1 + vse.abs() * wy1) * g.abs()
    s_giy = (vnw.abs() * wx0 + vne.abs() * wx1 + vsw.abs() * wx0 + vse.abs() * wx1) * g.abs()
    d_flow = torch.stack((my * giy, mx * gix), 1)
    s_flow = torch.stack((my * s_giy, mx * s_gix), 1)
    shape = (b, 1, h, w)
    S = {"out": s_out.reshape(shape), "d_src": s_src.reshape(shape), "d_flow": s_flow}
    return out.reshape(shape), d_src.reshape(shape), d_flow, k.reshape(shape), S
