"""numpy restatement (test infrastructure only) of the rotating projections, csrc/project_rotate.hip:

  detector(h, w)                            D = ceil(hypot(h, w)): the default detector width and ray length
  coefficients(angle, h, w, u, t)           the six 16.16 fixed-point coefficients of the view at `angle` degrees about the centre
                                            ((w-1)/2, (h-1)/2) of an h x w slice, detector of u columns, rays of t unit steps:
                                            float64, r(v) = floor(v * 65536 + 0.5)
  count(h, w, coef, U, T)                   [A][U] counted samples of every ray: sample (u, t) is pixel xi = (c0 + c1 u + c2 t) >> 16,
                                            yi = (c3 + c4 u + c5 t) >> 16 (arithmetic shift) and counts when it lies in the slice
  rotate(vol, coef, U, T, mode, fill)       int16 [A][N][U]: max / min / mean of slice n over the counted samples of ray u of angle
                                            a; the mean is the int64 sum divided toward zero by the ray's own count; `fill` where
                                            the count is 0
  level(values, wc, ww, hu)                 project_np.level: the 8-bit window level of those values

int64 inside."""
import math

import numpy as np

from project_np import level  # noqa: F401  (the level of a rotated value is the level of any projected value)


def detector(h, w):
    return int(math.ceil(math.hypot(h, w)))


def coefficients(angle, h, w, u=None, t=None):
    d = detector(h, w)
    u, t = d if u is None else u, d if t is None else t
    rad = math.radians(angle)
    cos, sin = math.cos(rad), math.sin(rad)
    cx, cy, cu, ct = (w - 1) / 2.0, (h - 1) / 2.0, (u - 1) / 2.0, (t - 1) / 2.0

    def r(v):
        return int(math.floor(v * 65536.0 + 0.5))

    return [r(cx - cu * cos + ct * sin + 0.5), r(cos), r(-sin), r(cy - cu * sin - ct * cos + 0.5), r(sin), r(cos)]


def _samples(h, w, c, U, T):
    """(xi, yi, ok), each [U][T], of one coefficient row."""
    c = [int(v) for v in c]
    u = np.arange(U, dtype=np.int64)[:, None]
    t = np.arange(T, dtype=np.int64)[None, :]
    fx, fy = c[0] + c[1] * u + c[2] * t, c[3] + c[4] * u + c[5] * t
    assert max(np.abs(fx).max(), np.abs(fy).max()) < 2 ** 31      # the kernel's int32 holds them
    xi, yi = fx >> 16, fy >> 16
    return xi, yi, (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)


def count(h, w, coef, U, T):
    return np.stack([_samples(h, w, c, U, T)[2].sum(axis=1) for c in np.asarray(coef).reshape(-1, 6)])


def rotate(vol, coef, U, T, mode, fill=0):
    vol = np.asarray(vol)
    assert vol.dtype == np.int16 and vol.ndim == 3 and mode in ("max", "min", "mean"), (vol.dtype, vol.shape, mode)
    n, h, w = vol.shape
    v64 = vol.astype(np.int64)
    planes = []
    for c in np.asarray(coef).reshape(-1, 6):
        xi, yi, ok = _samples(h, w, c, U, T)
        g = v64[:, np.where(ok, yi, 0), np.where(ok, xi, 0)]      # [N][U][T]
        cnt = ok.sum(axis=1)[None, :]
        if mode == "max":
            red = np.where(ok[None], g, -(2 ** 40)).max(axis=2)
        elif mode == "min":
            red = np.where(ok[None], g, 2 ** 40).min(axis=2)
        else:
            s = np.where(ok[None], g, 0).sum(axis=2)
            red = np.sign(s) * (np.abs(s) // np.maximum(cnt, 1))
        planes.append(np.where(cnt > 0, red, int(fill)))
    out = np.stack(planes)
    assert out.min() >= -32768 and out.max() <= 32767
    return out.astype(np.int16)
