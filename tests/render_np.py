"""numpy restatement (test infrastructure only) of the volume-rendered rotating views, csrc/project_render.hip
(ctg_project_render).  Written from the definition with the explicit sample tables of rotate_np._samples /
rotate_lerp_np.samples, classes from rotate_np.level and a plain loop over the steps t, vectorised over the rays with a `live`
mask for the rays that have ended: no lanes, no trips, no packed alphas, so the kernel's fold is checked independently.

  clamped(lut)                                    (col int64 [256][3], alpha int64 [256]): min(R, G, B, 255) and min(alpha, 32768)
  classes(vol, coef, U, T, sampling, wc, ww, hu)  (cls uint8 [A][N][U][T], ok bool [A][U][T]): the class of every sample (whatever
                                                  lies at an uncounted one) and the counted mask
  composite(cls, ok, lut, stop, surface, bg)      {"rgb": uint8 [A][N][U][3], "opacity": uint8, "depth": int16, "tr": the final
                                                  transparency, "weight": the sum of the weights, "taken": how many samples took
                                                  part, "counted": how many the ray has (broadcast), each int64 [A][N][U]}
  render(vol, coef, U, T, lut, ...)               classes + composite

A ray starts from Tr = 32768, C = 0 and takes its counted samples in ascending t:
    wgt = (Tr A) >> 15;  C += wgt col;  Tr -= wgt;  depth = t the first time 32768 - Tr >= surface;  Tr <= stop ends the ray
rgb = (C + bg Tr + 16384) >> 15, opacity = ((32768 - Tr) 255 + 16384) >> 15.  int64 inside; the uint32 ranges the kernel relies
on are asserted."""
import numpy as np

import rotate_lerp_np
import rotate_np

ONE = 32768


def clamped(lut):
    lut = np.asarray(lut)
    assert lut.shape == (256, 4) and lut.dtype.kind in "iu" and lut.min() >= 0 and lut.max() <= 65535
    lut = lut.astype(np.int64)
    return np.minimum(lut[:, :3], 255), np.minimum(lut[:, 3], ONE)


def classes(vol, coef, U, T, sampling="nearest", wc=300.0, ww=1500.0, hu=False):
    vol = np.asarray(vol)
    assert vol.dtype == np.int16 and vol.ndim == 3 and sampling in ("nearest", "bilinear") and 1 <= T <= 4096
    n, h, w = vol.shape
    v64 = vol.astype(np.int64)
    cls, oks = [], []
    for c in np.asarray(coef).reshape(-1, 6):
        if sampling == "nearest":
            xi, yi, ok = rotate_np._samples(h, w, c, U, T)
            g = v64[:, np.where(ok, yi, 0), np.where(ok, xi, 0)]      # [N][U][T]
        else:
            g, ok = rotate_lerp_np.samples(vol, c, U, T)
        cls.append(rotate_np.level(g, wc, ww, hu))
        oks.append(ok)
    return np.stack(cls), np.stack(oks)


def composite(cls, ok, lut, stop=128, surface=16384, bg=(0, 0, 0)):
    assert cls.dtype == np.uint8 and cls.ndim == 4 and ok.shape == (cls.shape[0],) + cls.shape[2:]
    assert 0 <= stop <= ONE - 1 and 1 <= surface <= ONE and len(bg) == 3 and all(0 <= int(b) <= 255 for b in bg)
    col, alpha = clamped(lut)
    a, n, u, steps = cls.shape
    tr = np.full((a, n, u), ONE, dtype=np.int64)
    acc = np.zeros((a, n, u, 3), dtype=np.int64)
    weight = np.zeros((a, n, u), dtype=np.int64)
    taken = np.zeros((a, n, u), dtype=np.int64)
    depth = np.full((a, n, u), -1, dtype=np.int64)
    live = np.ones((a, n, u), dtype=bool)
    for t in range(steps):
        part = live & ok[:, None, :, t]
        l = cls[..., t]
        wgt = np.where(part, (tr * alpha[l]) >> 15, 0)
        assert (wgt <= tr).all()      # Tr never goes negative
        acc += wgt[..., None] * col[l]
        tr -= wgt
        weight += wgt
        taken += part
        depth = np.where(part & (depth < 0) & (ONE - tr >= surface), t, depth)
        live &= ~(part & (tr <= stop))
    assert (weight == ONE - tr).all() and tr.min() >= 0 and acc.max() <= ONE * 255      # the weights telescope
    rgb = (acc + np.array([int(b) for b in bg], dtype=np.int64) * tr[..., None] + 16384) >> 15
    opacity = ((ONE - tr) * 255 + 16384) >> 15
    assert rgb.min() >= 0 and rgb.max() <= 255 and opacity.min() >= 0 and opacity.max() <= 255
    return {"rgb": rgb.astype(np.uint8), "opacity": opacity.astype(np.uint8), "depth": depth.astype(np.int16), "tr": tr,
            "weight": weight, "taken": taken, "counted": np.broadcast_to(ok.sum(axis=2)[:, None, :], taken.shape)}


def render(vol, coef, U, T, lut, sampling="nearest", stop=128, surface=16384, bg=(0, 0, 0), wc=300.0, ww=1500.0, hu=False):
    cls, ok = classes(vol, coef, U, T, sampling, wc, ww, hu)
    return composite(cls, ok, lut, stop, surface, bg)
