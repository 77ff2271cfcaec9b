"""numpy restatement (test infrastructure only) of the series projections, csrc/project.hip:

  project(vol, mode, thick)     the three int16 projections of an int16 volume [N, H, W]: axial [S, H, W] in slabs of `thick`
                                slices that do not overlap (the last may be shorter), coronal [N, W] (over H), sagittal [N, H]
                                (over W); mode "max", "min" or "mean".  The mean is the int64 sum divided toward zero:
                                sign(s) * (|s| // div)
  level(values, wc, ww, hu)     the 8-bit window level of projected values: the tail of to_windowdata (trainer/HdTrainer.py:43-61)
                                on the stored value t = float32(v + (1024 if hu else 0)) -- t == 0 -> -2000; t - 1024;
                                t - win_min; trunc(t * dFactor); clamp to [0, 255] -- in np.float32, one operation at a time,
                                win_min and dFactor formed in float64 (python floats in the reference) and then rounded"""
import numpy as np

F = np.float32


def _reduce(v, mode, axis):
    v = v.astype(np.int64)
    if mode == "max":
        return v.max(axis=axis)
    if mode == "min":
        return v.min(axis=axis)
    assert mode == "mean", mode
    s = v.sum(axis=axis)
    return np.sign(s) * (np.abs(s) // v.shape[axis])


def project(vol, mode, thick=None):
    vol = np.asarray(vol)
    assert vol.dtype == np.int16 and vol.ndim == 3
    n = vol.shape[0]
    thick = n if thick is None else int(thick)
    axial = np.stack([_reduce(vol[s:s + thick], mode, 0) for s in range(0, n, thick)])
    coronal, sagittal = _reduce(vol, mode, 1), _reduce(vol, mode, 2)
    for a in (axial, coronal, sagittal):
        assert a.min() >= -32768 and a.max() <= 32767
    return axial.astype(np.int16), coronal.astype(np.int16), sagittal.astype(np.int16)


def win_params(wc, ww):
    wc, ww = float(wc), float(ww)
    win_min = (2 * wc - ww) / 2.0 + 0.5
    win_max = (2 * wc + ww) / 2.0 + 0.5
    return F(win_min), F(255.0 / (win_max - win_min))


def level(values, wc, ww, hu=False):
    wmin, dfac = win_params(wc, ww)
    t = (np.asarray(values).astype(np.int64) + (1024 if hu else 0)).astype(F)
    t = np.where(t == 0, F(-2000), t)
    t = t - F(1024)
    t = t - wmin
    t = np.trunc(t * dfac)
    assert t.dtype == F
    return np.clip(t, 0, 255).astype(np.uint8)
