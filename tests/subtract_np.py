"""numpy restatement (test infrastructure only) of the subtraction volume, csrc/subtract.hip:

  subtract(cta, ct, hu, median, floor, ct_min, ct_max)   int16 [N, H, W]: per pixel, in int64,
                                a = max(ct + 1024, 0), b = cta + (1024 if hu else 0), d = b - a; median: the middle of the nine
                                values of the 3 x 3 in-plane neighbourhood, the edge pixel replicated outside the plane
                                (scipy.ndimage.median_filter(size=3, mode='nearest') of every plane); d = 0 where ct < ct_min,
                                ct > ct_max or d < floor (the centre pixel, after the median; None switches a test off);
                                clamped to int16
  level(values, wc, ww)         the 8-bit level of a HU difference in the window (wc, ww): project_np.level with hu=True"""
import numpy as np

import project_np


def median3x3(d):
    """[N, H, W] -> the 3 x 3 in-plane median, edges replicated: the sort of the nine edge-padded shifts, element [4]."""
    n, h, w = d.shape
    p = np.pad(d, ((0, 0), (1, 1), (1, 1)), mode="edge")
    nine = np.stack([p[:, dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)])
    return np.sort(nine, axis=0)[4]


def difference(cta, ct, hu=False):
    cta, ct = np.asarray(cta), np.asarray(ct)
    assert cta.dtype == np.int16 and ct.dtype == np.int16 and cta.shape == ct.shape and cta.ndim == 3
    return cta.astype(np.int64) + (1024 if hu else 0) - np.maximum(ct.astype(np.int64) + 1024, 0)


def subtract(cta, ct, hu=False, median=True, floor=0, ct_min=None, ct_max=None):
    d = difference(cta, ct, hu)
    if median:
        d = median3x3(d)
    c = np.asarray(ct).astype(np.int64)
    drop = np.zeros(d.shape, dtype=bool)
    if ct_min is not None:
        drop |= c < ct_min
    if ct_max is not None:
        drop |= c > ct_max
    if floor is not None:
        drop |= d < floor
    return np.clip(np.where(drop, 0, d), -32768, 32767).astype(np.int16)


def level(values, wc=150.0, ww=300.0):
    return project_np.level(values, wc, ww, True)
