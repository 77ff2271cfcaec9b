"""numpy restatement (test infrastructure only) of the depth of the maximum, csrc/project_rotate.hip (ctg_project_rotate_depth)
and csrc/project.hip (ctg_project_accumulate_depth, ctg_project_finish_depth).  Written with masked argmax / argmin (first
occurrence) over the explicit sample tables of rotate_np._samples / rotate_lerp_np.samples and over the volume's axes: no packed
key anywhere, so the kernels' formulation is checked independently.

  rotate_depth(vol, coef, U, T, mode, sampling, fill)   (values int16, depth int16), each [A][N][U]: the max / min of slice n over
                                                        the counted samples of ray u of angle a, and the smallest step t that
                                                        attains it; `fill` and depth -1 where no sample counts
  rotate_depth_modes(vol, coef, U, T, modes, ...)       the same for several modes at once, {mode: (values, depth)}
  project_depth(vol, mode, thick)                       {axis: (values int16, depth int16, start, length)}: axial [S, H, W] with
                                                        the global slice n, coronal [N, W] with the row y, sagittal [N, H] with
                                                        the column x; start / length (broadcastable to the plane): where the
                                                        rays of that plane begin along the axis and how long they are
  cue_weight(cue, d, length)                            w = 256 - (cue d) // length for d >= 0 (d < length), 256 for d < 0
  cued(level, cue, d, length)                           (level w + 128) >> 8, uint8

int64 inside."""
import numpy as np

import rotate_lerp_np
import rotate_np

MODES = ("max", "min")
FAR = 2 ** 40      # beyond every int16 value: what an uncounted sample holds before the argmax / argmin


def cue_weight(cue, d, length):
    cue = int(cue)
    assert 0 <= cue <= 256
    d, length = np.asarray(d, dtype=np.int64), np.asarray(length, dtype=np.int64)
    assert (length >= 1).all() and (d < length).all()
    w = np.where(d < 0, 256, 256 - cue * np.maximum(d, 0) // length)      # d >= 0: C division and floor division agree
    assert w.min() >= 1 and w.max() <= 256
    return w


def cued(level, cue, d, length):
    level = np.asarray(level)
    assert level.dtype == np.uint8
    out = (level.astype(np.int64) * cue_weight(cue, d, length) + 128) >> 8
    assert out.min() >= 0 and (out <= level).all()
    return out.astype(np.uint8)


def _first(v, ok, mode):
    """(value, index) along the last axis of v over the entries where ok: the extreme and its first occurrence."""
    assert mode in MODES, mode
    if mode == "max":
        m = np.where(ok, v, -FAR)
        i = m.argmax(axis=-1)
    else:
        m = np.where(ok, v, FAR)
        i = m.argmin(axis=-1)
    return np.take_along_axis(m, i[..., None], axis=-1)[..., 0], i


def rotate_depth_modes(vol, coef, U, T, modes=MODES, sampling="nearest", fill=0):
    """{mode: (values, depth)}: the samples of every angle are formed once and reduced in each of `modes`."""
    vol = np.asarray(vol)
    assert vol.dtype == np.int16 and vol.ndim == 3 and sampling in ("nearest", "bilinear") and 1 <= T <= 4096
    n, h, w = vol.shape
    v64 = vol.astype(np.int64)
    planes = {m: ([], []) for m in modes}
    for c in np.asarray(coef).reshape(-1, 6):
        if sampling == "nearest":
            xi, yi, ok = rotate_np._samples(h, w, c, U, T)
            g = v64[:, np.where(ok, yi, 0), np.where(ok, xi, 0)]      # [N][U][T]
        else:
            g, ok = rotate_lerp_np.samples(vol, c, U, T)
        seen = (ok.sum(axis=1) > 0)[None, :]
        for m in modes:
            val, idx = _first(g, ok[None], m)
            planes[m][0].append(np.where(seen, val, int(fill)))
            planes[m][1].append(np.where(seen, idx, -1))
    out = {}
    for m, (values, depth) in planes.items():
        values, depth = np.stack(values), np.stack(depth)
        assert values.min() >= -32768 and values.max() <= 32767 and depth.min() >= -1 and depth.max() < T
        out[m] = (values.astype(np.int16), depth.astype(np.int16))
    return out


def rotate_depth(vol, coef, U, T, mode, sampling="nearest", fill=0):
    return rotate_depth_modes(vol, coef, U, T, (mode,), sampling, fill)[mode]


def project_depth(vol, mode, thick=None):
    vol = np.asarray(vol)
    assert vol.dtype == np.int16 and vol.ndim == 3 and max(vol.shape) <= 32767
    n, h, w = vol.shape
    thick = n if thick is None else min(int(thick), n)
    v64 = vol.astype(np.int64)
    yes = np.ones((), dtype=bool)
    planes = []
    for s in range(0, n, thick):      # a slab's rays run along the slices, its own first slice nearest the viewer
        val, idx = _first(np.moveaxis(v64[s:s + thick], 0, -1), yes, mode)
        planes.append((val, idx + s, s, min(thick, n - s)))
    out = {"axial": (np.stack([p[0] for p in planes]).astype(np.int16), np.stack([p[1] for p in planes]).astype(np.int16),
                     np.array([p[2] for p in planes], dtype=np.int64)[:, None, None],
                     np.array([p[3] for p in planes], dtype=np.int64)[:, None, None])}
    val, idx = _first(np.moveaxis(v64, 1, -1), yes, mode)      # over the rows: [N][W]
    out["coronal"] = (val.astype(np.int16), idx.astype(np.int16), 0, h)
    val, idx = _first(v64, yes, mode)                          # over the columns: [N][H]
    out["sagittal"] = (val.astype(np.int16), idx.astype(np.int16), 0, w)
    return out
