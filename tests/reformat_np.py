"""numpy restatement (test infrastructure only) of the lines in any direction, csrc/reformat.hip (ctg_reformat_lines), written from
the definitions in include/ctagan_hip.h:

  reformat(vol, lines, U, T, mode, sampling, fill)   (values int16 [..., U], counted int64 [..., U]) for a table [..., 9] of rows
                                                     (x0, xu, xk, y0, yu, yk, z0, zu, zk): sample (l, i, k) lies at the 16.16
                                                     position X = x0 + xu i + xk k (Y, Z likewise) and counts exactly when voxel
                                                     (X >> 16, Y >> 16, Z >> 16) lies in the volume; max / min / mean over the
                                                     counted samples of the ray, the mean the sum over the ray's own count divided
                                                     toward zero, `fill` where the count is 0
  sample(vol, X, Y, Z, sampling)                     the value of samples at int64 positions of any shape: "nearest" the voxel
                                                     above (0 where it is not counted), "trilinear" about (X - 32768, ...):
                                                     v0, v1 = the bilinear value (top (256 - fy) + bot fy + 32768) >> 16 on
                                                     slices clamp(z0), clamp(z0 + 1) with clamped in-plane neighbours,
                                                     v = (v0 (256 - fz) + v1 fz + 128) >> 8
  level(values, wc, ww, hu)                          project_np.level

A plain loop over k with a counted mask: no lanes, no interval, no key.  int64 inside; the int32 ranges the kernel relies on are
asserted."""
import numpy as np

from project_np import level  # noqa: F401  (the level of a reformatted value is the level of any projected value)

MODES = ("max", "min", "mean")
SAMPLINGS = ("nearest", "trilinear")


def counted(shape, X, Y, Z):
    n, h, w = shape
    xi, yi, zi = X >> 16, Y >> 16, Z >> 16
    return (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h) & (zi >= 0) & (zi < n)


def sample(vol, X, Y, Z, sampling):
    n, h, w = vol.shape
    p = vol.astype(np.int64)
    if sampling == "nearest":
        ok = counted(vol.shape, X, Y, Z)
        return np.where(ok, p[np.where(ok, Z >> 16, 0), np.where(ok, Y >> 16, 0), np.where(ok, X >> 16, 0)], 0)
    assert sampling == "trilinear", sampling
    Xc, Yc, Zc = X - 32768, Y - 32768, Z - 32768
    x0, fx = Xc >> 16, (Xc >> 8) & 255
    y0, fy = Yc >> 16, (Yc >> 8) & 255
    z0, fz = Zc >> 16, (Zc >> 8) & 255
    xa, xb = np.clip(x0, 0, w - 1), np.clip(x0 + 1, 0, w - 1)
    ya, yb = np.clip(y0, 0, h - 1), np.clip(y0 + 1, 0, h - 1)
    planes = []
    for z in (np.clip(z0, 0, n - 1), np.clip(z0 + 1, 0, n - 1)):
        top = p[z, ya, xa] * (256 - fx) + p[z, ya, xb] * fx
        bot = p[z, yb, xa] * (256 - fx) + p[z, yb, xb] * fx
        acc = top * (256 - fy) + bot * fy + 32768
        assert acc.min() >= -2 ** 31 + 32768 and acc.max() <= 2 ** 31 - 32768      # int32 holds the accumulator
        planes.append(acc >> 16)
    v = (planes[0] * (256 - fz) + planes[1] * fz + 128) >> 8
    assert v.min() >= -32768 and v.max() <= 32767
    return v


def reformat(vol, lines, U, T, mode, sampling="nearest", fill=0):
    vol = np.asarray(vol)
    lines = np.asarray(lines).astype(np.int64)
    assert vol.dtype == np.int16 and vol.ndim == 3 and lines.shape[-1] == 9 and mode in MODES, (vol.dtype, vol.shape, lines.shape, mode)
    assert 1 <= U <= 4096 and 1 <= T <= 4096
    lead = lines.shape[:-1]
    c = lines.reshape(-1, 9)
    # the range ops.LineTable promises the kernel: no fixed-point sum leaves int32
    assert (np.abs(c[:, 0::3]) + np.abs(c[:, 1::3]) * (U - 1) + np.abs(c[:, 2::3]) * (T - 1)).max() < 2 ** 31
    i = np.arange(U, dtype=np.int64)[None, :]
    best = np.zeros((len(c), U), dtype=np.int64)
    total = np.zeros((len(c), U), dtype=np.int64)
    cnt = np.zeros((len(c), U), dtype=np.int64)
    for k in range(T):
        X, Y, Z = (c[:, 3 * a, None] + c[:, 3 * a + 1, None] * i + c[:, 3 * a + 2, None] * k for a in range(3))
        ok = counted(vol.shape, X, Y, Z)
        v = sample(vol, X, Y, Z, sampling)
        first = ok & (cnt == 0)
        if mode == "max":
            best = np.where(first, v, np.where(ok, np.maximum(best, v), best))
        elif mode == "min":
            best = np.where(first, v, np.where(ok, np.minimum(best, v), best))
        total += np.where(ok, v, 0)
        cnt += ok
    assert np.abs(total).max() < 2 ** 31      # the kernel's int32 sum
    if mode == "mean":
        best = np.sign(total) * (np.abs(total) // np.maximum(cnt, 1))
    out = np.where(cnt > 0, best, int(fill))
    assert out.min() >= -32768 and out.max() <= 32767
    return out.astype(np.int16).reshape(lead + (U,)), cnt.reshape(lead + (U,))
