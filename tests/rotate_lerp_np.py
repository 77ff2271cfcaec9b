"""numpy restatement (test infrastructure only) of the bilinear rotating projections, csrc/project_rotate.hip
(ctg_project_rotate_bilinear), and of oversampled rays for both samplings:

  coefficients(angle, h, w, u, t, oversample)   the six 16.16 coefficients of rays of t voxels taken in t s steps of 1 / s voxel
                                                (s = oversample): ct = (t s - 1) / (2 s), c2 = r(-sin / s), c5 = r(cos / s), the
                                                rest as rotate_np.coefficients; s = 1 is rotate_np.coefficients itself
  rotate_modes(vol, coef, U, T, modes, fill)    the same for several modes at once, {mode: planes}
  rotate(vol, coef, U, T, mode, fill)           int16 [A][N][U]: max / min / mean over the counted samples of every ray, T = t s
                                                steps.  A sample counts exactly when rotate_np counts it (pixel (X >> 16, Y >> 16)
                                                in the slice); its value is the bilinear interpolation of the four pixels around
                                                the centre-based position (X - 32768, Y - 32768), fractions of 8 bits, the edge
                                                pixel replicated, rounded once: (top (256 - fy) + bot fy + 32768) >> 16
  level(values, wc, ww, hu)                     rotate_np.level

int64 inside; the int32 ranges the kernel relies on are asserted."""
import math

import numpy as np

import rotate_np
from rotate_np import count, detector, level  # noqa: F401  (counting and the level are those of nearest sampling)


def coefficients(angle, h, w, u=None, t=None, oversample=1):
    d = detector(h, w)
    u, t, s = d if u is None else u, d if t is None else t, int(oversample)
    assert s >= 1
    rad = math.radians(angle)
    cos, sin = math.cos(rad), math.sin(rad)
    cx, cy, cu, ct = (w - 1) / 2.0, (h - 1) / 2.0, (u - 1) / 2.0, (t * s - 1) / (2.0 * s)

    def r(v):
        return int(math.floor(v * 65536.0 + 0.5))

    return [r(cx - cu * cos + ct * sin + 0.5), r(cos), r(-sin / s), r(cy - cu * sin - ct * cos + 0.5), r(sin), r(cos / s)]


def samples(vol, c, U, T):
    """(v, ok): the interpolated values int64 [N][U][T] of one coefficient row (whatever lies at an uncounted sample) and the
    counted mask [U][T]."""
    n, h, w = vol.shape
    c = [int(x) for x in c]
    u = np.arange(U, dtype=np.int64)[:, None]
    t = np.arange(T, dtype=np.int64)[None, :]
    X, Y = c[0] + c[1] * u + c[2] * t, c[3] + c[4] * u + c[5] * t
    assert max(np.abs(X).max(), np.abs(Y).max()) < 2 ** 31 - 32768      # the kernel's int32 holds them, less the half too
    ok = rotate_np._samples(h, w, c, U, T)[2]
    Xc, Yc = X - 32768, Y - 32768
    x0, fx = Xc >> 16, (Xc >> 8) & 255
    y0, fy = Yc >> 16, (Yc >> 8) & 255
    assert x0[ok].size == 0 or (x0[ok].min() >= -1 and x0[ok].max() <= w - 1 and y0[ok].min() >= -1 and y0[ok].max() <= h - 1)
    xa, xb = np.clip(x0, 0, w - 1), np.clip(x0 + 1, 0, w - 1)
    ya, yb = np.clip(y0, 0, h - 1), np.clip(y0 + 1, 0, h - 1)
    p = vol.astype(np.int64)
    top = p[:, ya, xa] * (256 - fx) + p[:, ya, xb] * fx
    bot = p[:, yb, xa] * (256 - fx) + p[:, yb, xb] * fx
    acc = top * (256 - fy) + bot * fy + 32768
    assert acc.min() >= -2 ** 31 + 32768 and acc.max() <= 2 ** 31 - 32768      # int32 holds the accumulator, nothing to spare
    v = acc >> 16
    assert v.min() >= -32768 and v.max() <= 32767
    return v, ok


def rotate_modes(vol, coef, U, T, modes=("max", "min", "mean"), fill=0):
    """{mode: int16 [A][N][U]}: the samples of every angle are interpolated once and reduced in each of `modes`."""
    vol = np.asarray(vol)
    assert vol.dtype == np.int16 and vol.ndim == 3 and all(m in ("max", "min", "mean") for m in modes), (vol.dtype, vol.shape, modes)
    assert 1 <= T <= 4096
    planes = {m: [] for m in modes}
    for c in np.asarray(coef).reshape(-1, 6):
        v, ok = samples(vol, c, U, T)
        cnt = ok.sum(axis=1)[None, :]
        for m in modes:
            if m == "max":
                red = np.where(ok[None], v, -(2 ** 40)).max(axis=2)
            elif m == "min":
                red = np.where(ok[None], v, 2 ** 40).min(axis=2)
            else:
                s = np.where(ok[None], v, 0).sum(axis=2)
                assert np.abs(s).max() < 2 ** 31      # the kernel's int32 sum
                red = np.sign(s) * (np.abs(s) // np.maximum(cnt, 1))
            planes[m].append(np.where(cnt > 0, red, int(fill)))
    out = {m: np.stack(p) for m, p in planes.items()}
    assert all(o.min() >= -32768 and o.max() <= 32767 for o in out.values())
    return {m: o.astype(np.int16) for m, o in out.items()}


def rotate(vol, coef, U, T, mode, fill=0):
    return rotate_modes(vol, coef, U, T, (mode,), fill)[mode]
