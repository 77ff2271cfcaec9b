"""numpy restatement (test infrastructure only) of the sliding thin-slab projections, csrc/project_slabs.hip:

  windows(length, thick, step)           the explicit window list [(start, stop), ...] along an axis of `length` voxels: starts
                                         0, step, 2 step, ...; the list ends with the first window that reaches the end of the
                                         axis (brute enumeration, no closed form)
  slabs(vol, mode, thick, step, axis)    int16 [J, ...] of an int16 volume [N, H, W]: axis "axial" [J, H, W] (over the slices of
                                         each window), "coronal" [J, N, W] (over its rows), "sagittal" [J, N, H] (over its
                                         columns); mode "max", "min" or "mean" (project_np._reduce: the int64 sum divided toward
                                         zero by the window's own length)
Levels come from project_np.level."""
import numpy as np

import project_np

AXIS = {"axial": 0, "coronal": 1, "sagittal": 2}


def windows(length, thick, step):
    length, thick, step = int(length), int(thick), int(step)
    assert length >= 1 and 1 <= step <= thick
    out, start = [], 0
    while True:
        out.append((start, min(start + thick, length)))
        if start + thick >= length:
            return out
        start += step


def slabs(vol, mode, thick, step, axis):
    vol = np.asarray(vol)
    assert vol.dtype == np.int16 and vol.ndim == 3
    ax = AXIS[axis]
    planes = []
    for a, b in windows(vol.shape[ax], thick, step):
        index = [slice(None)] * 3
        index[ax] = slice(a, b)
        planes.append(project_np._reduce(vol[tuple(index)], mode, ax))
    out = np.stack(planes)
    assert out.min() >= -32768 and out.max() <= 32767
    return out.astype(np.int16)
