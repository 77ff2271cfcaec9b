"""numpy restatement (test infrastructure only) of the shaded volume rendering along lines in any direction, csrc/render_lines.hip
(ctg_render_lines), written from the definition in include/ctagan_hip.h on top of reformat_np.counted / reformat_np.sample (where
a sample lies, whether it counts, its nearest or trilinear value), rotate_np.level (its class) and render_np.clamped (the table):

  gradient(vol, xi, yi, zi, zscale)                    (gx, gy, gz) int64 at voxels inside the volume: central differences of the
                                                       stored values with the edge replicated, gx, gy clamped to +-4095 and
                                                       gz = clamp((dz zscale + 128) >> 8, +-4095)
  shade(gx, gy, gz, light, ambient, gmin2)             0 .. 256: 256 where m = |g|^2 < gmin2, else ambient + (((256 - ambient) diff
                                                       + 128) >> 8) with diff = min((|g . l| // floor(sqrt(m))) >> 4, 256) and the
                                                       light clamped to +-4096
  render(vol, lines, U, T, lut, sampling, ...)         {"rgb": uint8 [..., U, 3], "opacity": uint8 [..., U], "depth": int16 [..., U],
                                                       "tr", "weight", "taken", "counted", "lit", "gated": int64 [..., U]} -- lit /
                                                       gated: the weight the ray gave to samples that were shaded / fell under
                                                       the gate (both 0 without a light)

A plain loop over k with `live` and counted masks: no lanes, no trips, no interval, no packed alphas.  int64 inside; the uint32 /
int32 ranges the kernel relies on are asserted.  The square root is a float64 seed corrected to the exact floor."""
import numpy as np

import reformat_np
import render_np
import rotate_np

ONE = 32768
GMAX, LMAX = 4095, 4096


def isqrt(m):
    m = np.asarray(m, dtype=np.int64)
    n = np.floor(np.sqrt(m.astype(np.float64))).astype(np.int64)
    n = np.where(n * n > m, n - 1, n)
    n = np.where((n + 1) * (n + 1) <= m, n + 1, n)
    assert ((n * n <= m) & ((n + 1) * (n + 1) > m)).all()
    return n


def gradient(vol, xi, yi, zi, zscale):
    n, h, w = vol.shape
    p = vol.astype(np.int64)
    assert 1 <= zscale <= 4096
    dx = p[zi, yi, np.minimum(xi + 1, w - 1)] - p[zi, yi, np.maximum(xi - 1, 0)]
    dy = p[zi, np.minimum(yi + 1, h - 1), xi] - p[zi, np.maximum(yi - 1, 0), xi]
    dz = p[np.minimum(zi + 1, n - 1), yi, xi] - p[np.maximum(zi - 1, 0), yi, xi]
    assert np.abs(dz * zscale).max(initial=0) < 2 ** 31 - 128
    return np.clip(dx, -GMAX, GMAX), np.clip(dy, -GMAX, GMAX), np.clip((dz * zscale + 128) >> 8, -GMAX, GMAX)


def shade(gx, gy, gz, light, ambient, gmin2):
    """light: int64 broadcastable to gx.shape + (3,)."""
    assert 0 <= ambient <= 256 and 1 <= gmin2 <= 1 << 26
    m = gx * gx + gy * gy + gz * gz
    assert m.max(initial=0) < 2 ** 26
    lv = np.clip(np.asarray(light).astype(np.int64), -LMAX, LMAX)
    dot = np.abs(gx * lv[..., 0] + gy * lv[..., 1] + gz * lv[..., 2])
    assert dot.max(initial=0) < 2 ** 26
    root = np.maximum(isqrt(m), 1)      # (1 only where the gate below takes over: m >= gmin2 >= 1 has a root >= 1)
    diff = np.minimum((dot // root) >> 4, 256)
    lit = ambient + (((256 - ambient) * diff + 128) >> 8)
    out = np.where(m < gmin2, 256, lit)
    assert out.min(initial=256) >= 0 and out.max(initial=0) <= 256
    return out, m >= gmin2


def render(vol, lines, U, T, lut, sampling="nearest", stop=128, surface=16384, bg=(0, 0, 0), wc=300.0, ww=1500.0, hu=False,
           light=None, zscale=256, ambient=77, gmin2=1600):
    vol = np.asarray(vol)
    lines = np.asarray(lines).astype(np.int64)
    assert vol.dtype == np.int16 and vol.ndim == 3 and lines.shape[-1] == 9 and sampling in reformat_np.SAMPLINGS
    assert 1 <= U <= 4096 and 1 <= T <= 4096
    assert 0 <= stop <= ONE - 1 and 1 <= surface <= ONE and len(bg) == 3 and all(0 <= int(b) <= 255 for b in bg)
    lead = lines.shape[:-1]
    c = lines.reshape(-1, 9)
    assert (np.abs(c[:, 0::3]) + np.abs(c[:, 1::3]) * (U - 1) + np.abs(c[:, 2::3]) * (T - 1)).max() < 2 ** 31
    if light is not None:
        light = np.asarray(light).astype(np.int64)
        assert light.shape == lead + (3,), (light.shape, lead)
        light = light.reshape(-1, 1, 3)
    col, alpha = render_np.clamped(lut)
    i = np.arange(U, dtype=np.int64)[None, :]
    shape = (len(c), U)
    tr = np.full(shape, ONE, dtype=np.int64)
    acc = np.zeros(shape + (3,), dtype=np.int64)
    weight, taken, counted, lit, gated = (np.zeros(shape, dtype=np.int64) for _ in range(5))
    depth = np.full(shape, -1, dtype=np.int64)
    live = np.ones(shape, dtype=bool)
    for k in range(T):
        X, Y, Z = (c[:, 3 * a, None] + c[:, 3 * a + 1, None] * i + c[:, 3 * a + 2, None] * k for a in range(3))
        ok = reformat_np.counted(vol.shape, X, Y, Z)
        v = reformat_np.sample(vol, X, Y, Z, sampling)
        cls = rotate_np.level(v, wc, ww, hu).astype(np.int64) & 255
        part = live & ok
        wgt = np.where(part, (tr * alpha[cls]) >> 15, 0)
        assert (wgt <= tr).all()
        cols = col[cls]
        if light is not None:
            xi, yi, zi = (np.where(ok, q >> 16, 0) for q in (X, Y, Z))
            sh, shaded = shade(*gradient(vol, xi, yi, zi, zscale), light, ambient, gmin2)
            cols = (cols * sh[..., None] + 128) >> 8
            assert cols.max() <= 255
            lit += np.where(shaded, wgt, 0)
            gated += np.where(shaded, 0, wgt)
        acc += wgt[..., None] * cols
        tr -= wgt
        weight += wgt
        taken += part
        counted += ok
        depth = np.where(part & (depth < 0) & (ONE - tr >= surface), k, depth)
        live &= ~(part & (tr <= stop))
    assert (weight == ONE - tr).all() and tr.min() >= 0 and acc.max() <= ONE * 255      # the weights telescope
    rgb = (acc + np.array([int(b) for b in bg], dtype=np.int64) * tr[..., None] + 16384) >> 15
    opacity = ((ONE - tr) * 255 + 16384) >> 15
    assert rgb.min() >= 0 and rgb.max() <= 255 and opacity.min() >= 0 and opacity.max() <= 255
    out = {"rgb": rgb.astype(np.uint8).reshape(lead + (U, 3)), "opacity": opacity.astype(np.uint8).reshape(lead + (U,)),
           "depth": depth.astype(np.int16).reshape(lead + (U,))}
    for name, plane in (("tr", tr), ("weight", weight), ("taken", taken), ("counted", counted), ("lit", lit), ("gated", gated)):
        out[name] = plane.reshape(lead + (U,))
    return out
