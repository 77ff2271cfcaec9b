"""Series inference: a raw HU volume in, the synthesized volume out in the scanner's pixel format.

The export half of the reference's test() loop (trainer/HdTrainer.py:539-552) without its DICOM container: int16 HU crosses
PCIe at 2 B/pixel, `ops.series_inputs` makes the generator's plane on the device, the generator runs without autograd, and
`ops.export_slices` turns its output into int16 pixels (+ the 8-bit window level) that cross back at 3 B/pixel.  Chunks of
`batch` slices go through two page-locked slots per direction; the H2D and the D2H copies run on streams of their own behind
events, so both hide behind the forward of the neighbouring chunks and the host only ever waits to get a slot back.

Projections (`SeriesProjector`, `project_volume`, `SeriesTranslator(project=...)`): the maximum- / minimum-intensity or mean
projection of the volume along the three body axes, and thin-slab axial ones, accumulated on the device chunk by chunk
(`ops.project_accumulate`) as the chunks leave `ops.export_slices`; only the finished projections and their 8-bit window
levels (`ops.project_finish`) cross PCIe, once, after the last chunk.

Rotating projections (`SeriesRotator`, `rotate_volume`, `SeriesTranslator(rotate=...)`): the same projection at any number of
view angles about the cranio-caudal axis, what an angiography volume is read as first.  A row of a rotated view depends on one
slice only, so every chunk finishes its own rows of every angle in one launch (`ops.project_rotate`): samples on a 16.16
fixed-point grid, integer arithmetic throughout.  The default is nearest sampling at unit steps, which visits about 82 % of the
voxels at 45 degrees (a ray of slope 1 skips pixels between its samples), so a one-pixel vessel can vanish at some angles.
`sampling="bilinear"` interpolates the four pixels around every sample (8-bit fractions, still exact integers) and
`oversample=s` takes s steps per voxel, with either sampling: bilinear sees a one-pixel maximum at every angle, nearest at two
steps per voxel at nearly every one.

Depth of the maximum (`depth=True` on `SeriesRotator`, `SeriesProjector`, `rotate_volume`, `project_volume`,
`SeriesTranslator`): a MIP throws the depth away, so front and back look the same in a rotating view and a pixel cannot be sent
back to its voxel.  With `depth=True` (mode "max" / "min") every projection also returns "depth", int16: how far along the ray
the value was found (the first sample from the viewer's end; -1 on a rotated ray that misses the slice), and "cued", the 8-bit
level attenuated by that depth (`cue` in 0 .. 256; 0 leaves the level as it is).  The (value, depth) pair is one 32-bit key, so
the kernels stay single-pass, order-free integer reductions (`ops.project_rotate_depth`, `ops.project_accumulate_depth`,
`ops.project_finish_depth`); `ray_voxel` maps a rotated pixel and its depth back to the voxel.  Sliding thin slabs have no
depth planes: a thin slab has little depth to show.

Subtraction (`subtract_volume`, `SeriesTranslator(subtract=True)`): the synthesized CTA minus the CT it was made from.  The
generator writes on its input's pixel grid, so the pair is registered by construction: the difference of the stored values is the
contrast-enhancement map and bone cancels without a segmentation.  One launch per chunk (`ops.subtract_slices`: 3 x 3 in-plane
median, a floor and a band on the input HU), from the two chunks that are on the device anyway; `project_source="sub"` hands
that chunk to the projector and the rotator instead of the synthesized one: the bone-free MIP and rotating MIP.

Sliding thin slabs (`SeriesSlabs`, `slab_volume`, `SeriesTranslator(slabs=...)`): the mode a CTA is read in.  A slab of T voxels
is projected and moved on by S <= T voxels (`slab_windows`), along the axial, the coronal or the sagittal axis, so a vessel that
runs obliquely stays connected from one slab to the next.  A coronal or sagittal slab row depends on one slice only, so every
chunk finishes its own rows of every slab plane in one launch per axis (`ops.project_slabs_inplane`); the axial slabs are int32
accumulators (`ops.project_accumulate_sliding`) finished by `ops.project_finish`.  S = 1 makes about one plane per voxel of the
axis: `SeriesSlabs.nbytes` says what that costs before anything runs.

Reformats (`VolumeReformatter`, `reformat_volume`, `SeriesTranslator(reformat=...)`): every display whose rows cross slices --
double-oblique planes and thin oblique slabs (`oblique_lines`), rotation about any axis (`orbit_lines`: the tumble), the
straightened curved reformat along a vessel's centreline (`curved_lines`), any parallel view (`view_lines`).  The source volume
stays on the device and one kernel samples it along lines given by a table of nine 16.16 integers per output line
(`ops.reformat_lines`): nearest or trilinear sampling in exact integers, max / min / mean along rays of T steps, anisotropic
voxels inside the table (`aspect`), one launch per table after the last chunk.

Shaded rendering along lines (`VolumeRenderer`, `render_lines_volume`, `SeriesTranslator(render3d=...)`): the volume-rendered view on
the same line tables -- rays in any direction, trilinear sampling, anisotropic voxels inside the geometry -- with every sample's
colour shaded by the local gradient (`ops.render_lines`: the compositing chain of `ops.project_render`, central differences at the
sample's voxel, a light per line from `headlight` or one fixed vector, all in exact integers).  It reads the volume on the device
as the reformats do; `line_voxel` maps a depth back to its voxel.

Connected components (`VolumeComponents`, `components_volume`, `SeriesTranslator(components=..., project_source="vessels")`): the
volume with only the wanted connected components of a threshold band left -- islands below a size dropped, the K largest kept, or
the component a seed voxel (`ray_voxel`, `line_voxel`) lies in -- labelled on the device after the last chunk (`ops.components_label`
/ `components_select` / `components_apply`: a block union-find whose labels are the smallest linear index of a component, so the
result does not depend on the order of the kernels' atomics).  `root_voxel` maps a root to its voxel.  The centreline
(`VolumeCentreline`, `centreline_volume`, `SeriesTranslator(centreline=...)`) is the cheapest path through such a band between clicks.

The resident volume.  The four `Volume*` views read the whole int16 volume on the device.  It is an object of its own,
`ResidentVolume`: a view makes one for itself, or reads the one it is given (`source=`), so `SeriesTranslator` keeps one per source
("cta", "sub", the cleaned "vessels") however many views read it and feeds it once per chunk; a volume that is already a contiguous
device tensor -- the cleaned one, the input of a `*_volume` function -- is adopted as it is, without a copy.

The view protocol.  The display classes above are views (`_SeriesView` holds what they share), and `SeriesTranslator` and
the `*_volume` functions drive every one of them the same way.  A view is made for one volume shape and has `.n`, `.h`, `.w` and
`.device`; `update(pix_chunk, n0)` takes a device chunk of slices n0 .. n0+K-1 on the current stream, in any order, every slice
once; `result()` returns a tree on the device -- a dict of tensors, Nones and nested dicts -- once they have all arrived;
`reset()` makes the view ready for the next volume of the same shape.  A view whose result has one plane per view angle keeps the
angles as the host list `.angles`.  Where the classes differ: `SeriesProjector.update` forwards an empty chunk to ops (the others
return early) and its `result` takes the window (the others take it at construction); the `Volume*` views also bound the sides by
`ops.REFORMAT_MAX_DIM`, check the chunk's dtype, resolve device=None at the first chunk only and, given a `source=`, take no chunks.
"""
from __future__ import annotations

import collections
import math
import time

import numpy as np
import torch

from . import ops

SLOTS = 2


def plan_chunks(n, batch):
    """[(start, stop, slot), ...]: `n` slices in chunks of at most `batch` (the last may be shorter), chunk i in slot i % 2."""
    n, batch = int(n), int(batch)
    if n < 0 or batch < 1:
        raise ValueError("plan_chunks: n >= 0 and batch >= 1 expected, got n=%d batch=%d" % (n, batch))
    return [(s, min(s + batch, n), i % SLOTS) for i, s in enumerate(range(0, n, batch))]


def _pair(size):
    return (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))


AXES = ("axial", "coronal", "sagittal")
PROJECTIONS = ("max", "min", "mean")


def slab_plan(n, thick):
    """(S, div_last): `n` slices in S = ceil(n / thick) slabs that do not overlap, the last of div_last <= thick slices."""
    n, thick = int(n), int(thick)
    if n < 1 or thick < 1:
        raise ValueError("slab_plan: n >= 1 and thick >= 1 expected, got n=%d thick=%d" % (n, thick))
    s = (n + thick - 1) // thick
    return s, n - (s - 1) * thick


def slab_windows(length, thick, step):
    """(J, thick_clipped, last_len): the sliding slabs along an axis of `length` voxels, `thick` >= 1 voxels each, moved on by
    `step` voxels, 1 <= step <= thick (checked against the thick given; thick is clipped to the axis afterwards, as
    `SeriesProjector` clips its slab).  Slab j covers [j step, min(j step + thick, length)); J = 1 if length <= thick, else
    ceil((length - thick) / step) + 1.  Only the last slab can be short: last_len <= thick_clipped voxels.  With step == thick
    this is `slab_plan`."""
    length, thick, step = int(length), int(thick), int(step)
    if length < 1 or thick < 1 or not 1 <= step <= thick:
        raise ValueError("slab_windows: length >= 1 and 1 <= step <= thick expected, got length=%d thick=%d step=%d"
                         % (length, thick, step))
    j = ops.slab_count(length, thick, step)
    thick = min(thick, length)
    return j, thick, min(thick, length - (j - 1) * step)


def aspect_rows(n, aspect):
    """Source row of every output row when the n rows of a coronal / sagittal projection are drawn at `aspect` = slice spacing /
    pixel spacing: round(n * aspect) rows by the index rule of the nearest Resize (trainer/utils.py:13-32; float32, as
    `ops.resize_nearest` computes it)."""
    rows = max(1, int(round(int(n) * float(aspect))))
    scale = np.float32(n) / np.float32(rows)
    return np.minimum(np.floor(np.arange(rows, dtype=np.float32) * scale).astype(np.int64), int(n) - 1)


def _one_of(who, name, value, choices):
    if value not in choices:
        raise ValueError("%s: %s %r is not one of %s" % (who, name, value, choices))


def _int_in(who, name, v, lo, hi=None):
    """-> int(v) of an option that must be an integer (no bool, no float) in lo .. hi, or >= lo without a hi."""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo or (hi is not None and v > hi):
        raise ValueError("%s: %s: an integer %s expected, got %r" % (who, name, ">= %d" % lo if hi is None else "in %d .. %d" % (lo, hi), v))
    return int(v)


def _band(who, threshold):
    """-> (lo, hi) of a threshold band: an integer lo (hi = 32767) or a pair of them, -32768 <= lo <= hi <= 32767."""
    band = tuple(threshold) if isinstance(threshold, (tuple, list)) else (threshold, 32767)
    if len(band) != 2 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in band):
        raise ValueError("%s: threshold: an integer lo or a pair (lo, hi) expected, got %r" % (who, threshold))
    if not -32768 <= band[0] <= band[1] <= 32767:
        raise ValueError("%s: threshold: -32768 <= lo <= hi <= 32767 expected, got %r" % (who, threshold))
    return int(band[0]), int(band[1])


def _voxel_indices(who, what, points, n, h, w, least=1, most=None):
    """-> int64 [P], the linear indices (z h + y) w + x of `least` .. `most` integer points (z, y, x) that lie in the volume."""
    pts = np.asarray(list(points))
    if pts.ndim != 2 or pts.shape[1] != 3 or pts.dtype.kind not in "iu" or len(pts) < least or (most is not None and len(pts) > most):
        raise ValueError("%s: %s: %s integer (z, y, x) expected, got %r"
                         % (who, what, "at least %d" % least if most is None else "%d .. %d" % (least, most), points))
    pts = pts.astype(np.int64)
    if (pts < 0).any() or (pts >= np.array([n, h, w])).any():
        raise ValueError("%s: %s: a point lies outside the volume (%d, %d, %d)" % (who, what, n, h, w))
    return (pts[:, 0] * h + pts[:, 1]) * w + pts[:, 2]


def _check_depth(who, depth, cue, mode):
    """-> (depth, cue) of the depth planes: cue an integer in 0 .. 256; a depth exists for "max" and "min" only."""
    cue = _int_in(who, "cue", cue, 0, 256)
    if depth and mode not in ("max", "min"):
        raise ValueError("%s: depth=True needs mode 'max' or 'min' (a mean has no depth), got %r" % (who, mode))
    if cue and not depth:
        raise ValueError("%s: cue=%d needs depth=True" % (who, cue))
    return bool(depth), int(cue)


def _tree_to(tree, conv):
    """A result tree -- a dict of tensors, Nones and nested dicts or lists -- with `conv` applied to every tensor."""
    if isinstance(tree, dict):
        return {k: _tree_to(v, conv) for k, v in tree.items()}
    if isinstance(tree, list):
        return [_tree_to(v, conv) for v in tree]
    return None if tree is None else conv(tree)


def _tree_leaves(tree, path=()):
    """[(path, tensor), ...]: the tensors of a result tree in its own order, each with the keys that lead to it."""
    if isinstance(tree, dict):
        return [leaf for k, v in tree.items() for leaf in _tree_leaves(v, path + (k,))]
    if isinstance(tree, list):
        return [leaf for k, v in enumerate(tree) for leaf in _tree_leaves(v, path + (k,))]
    return [] if tree is None else [(path, tree)]


def _view_of_volume(who, volume, batch, device, make, result=lambda view: view.result(), whole=False):
    """What the `*_volume` functions share: the view `make(n, h, w, device)` fed with a volume that already exists -- int16
    [N, H, W], a host array / CPU tensor in chunks of `batch` slices or a device tensor -- and its `result`, converted to the
    input's kind.  The device is the tensor's, else `device`, else the current one.  whole=True, for the views on the whole
    volume: host chunks go to `update` as they are (it copies them into the resident volume, the only time they cross PCIe), and
    a contiguous device tensor is adopted as the resident volume instead of being copied into a second one."""
    is_np = isinstance(volume, np.ndarray)
    vol = torch.from_numpy(np.ascontiguousarray(volume)) if is_np else volume
    if not torch.is_tensor(vol) or vol.dtype != torch.int16 or vol.dim() != 3:
        raise RuntimeError("%s: an int16 volume [N, H, W] expected" % who)
    if int(batch) < 1:
        raise ValueError("%s: batch >= 1 expected" % who)
    on_host = not vol.is_cuda
    n, h, w = vol.shape
    view = make(n, h, w, vol.device if vol.is_cuda else torch.device("cuda", torch.cuda.current_device()) if device is None else device)
    with torch.cuda.device(view.device):
        if whole and not on_host and vol.is_contiguous():
            view.source.adopt(vol)
        else:
            for s, e, _ in plan_chunks(n, batch):
                view.update(vol[s:e] if whole or not on_host else vol[s:e].to(view.device), s)
        out = result(view)
    if not on_host:
        return out
    return _tree_to(out, (lambda t: t.cpu().numpy()) if is_np else (lambda t: t.cpu()))


class _SeriesView:
    """What the views and `ResidentVolume` share: the volume check, the device check, the check that a chunk lies in the volume,
    and a `reset()` that does nothing.  A view takes `update(pix_chunk, n0)` for every chunk and gives `result()` once they have
    all arrived.  An error names the class, or `who` where one speaks for another."""

    def _volume(self, n, h, w):
        self.n, self.h, self.w = int(n), int(h), int(w)
        if min(self.n, self.h, self.w) < 1:
            raise ValueError("%s: a volume of at least one voxel expected" % type(self).__name__)

    def _gpu(self, device):
        """-> the torch.device of `device` (None: the current one); anything but a GPU is refused."""
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("%s: a GPU device is required (no CPU fallback)" % type(self).__name__)
        return device

    def _chunk(self, pix_chunk, n0, dtype=None, who=None):
        """-> K, the slices of a chunk that lies in the volume (and, where the view asks for it, is of `dtype`)."""
        k, n0 = pix_chunk.shape[0], int(n0)
        if tuple(pix_chunk.shape[1:]) != (self.h, self.w) or n0 < 0 or n0 + k > self.n or (dtype is not None and pix_chunk.dtype != dtype):
            raise RuntimeError("%s: %schunk %s at slice %d does not lie in the volume (%d, %d, %d)"
                               % (who or type(self).__name__, "" if dtype is None else "int16 ", tuple(pix_chunk.shape), n0, self.n,
                                  self.h, self.w))
        return k

    def _rays(self, n, h, w, angles, detector, sampling, oversample, device):
        """What the rotating views share: the volume, `.angles`, the detector `.u` x `.t` (None: `default_detector` for both), `.steps`
        = t * oversample, the device and the coefficient table of the angles on it."""
        _check_sampling(type(self).__name__, sampling, oversample)
        self.sampling, self.oversample = sampling, int(oversample)
        self._volume(n, h, w)
        self.angles = [float(a) for a in angles]
        if not 1 <= len(self.angles) <= ops.ROTATE_MAX_DIM:
            raise ValueError("%s: 1 .. %d view angles expected, got %d" % (type(self).__name__, ops.ROTATE_MAX_DIM, len(self.angles)))
        d = default_detector(self.h, self.w)
        self.u, self.t = (d, d) if detector is None else _pair(detector)
        self.steps = self.t * self.oversample
        self.device = self._gpu(device)
        self.table = ops.RotateTable([rotation_coefficients(a, self.h, self.w, self.u, self.t, self.oversample)
                                      for a in self.angles], self.device)

    def reset(self):
        """For the next volume of the same shape: nothing to refill unless the view keeps accumulators."""


class SeriesProjector(_SeriesView):
    """Running projections of an int16 volume [n, h, w] that arrives in chunks on the device.

    mode "max" (MIP), "min" (MinIP) or "mean" (ray sum / count, truncated toward zero); slab: slices per axial slab (None: the
    whole volume, one plane; slabs do not overlap, the last may be shorter); axes: which of "axial" [S, h, w], "coronal" [n, w]
    (the reduction over h) and "sagittal" [n, h] (over w) to keep.  `update(pix_chunk, n0)` in any order, every slice once;
    `result(wc, ww)` -> {axis: {"values": int16, "level": uint8 or None}} on the device; `reset()` for the next volume of the
    same shape.  Exact integer arithmetic on the current stream: equal to numpy bit for bit.
    depth=True (mode "max" / "min"; no axis above 32767 voxels): the accumulators hold (value, depth) keys and every axis of the
    result gains "depth" int16 -- the slice n (axial; global, also with slabs), the row y (coronal) or the column x (sagittal)
    of the first voxel along the axis that attains the value, np.argmax / np.argmin -- and, when the level is wanted, "cued" uint8:
    the level attenuated by the depth inside the ray, (level w + 128) >> 8 with w = 256 - (cue d) / E, `cue` in 0 .. 256."""

    def __init__(self, n, h, w, mode="max", slab=None, axes=AXES, device=None, depth=False, cue=0):
        _one_of("SeriesProjector", "mode", mode, PROJECTIONS)
        self.depth, self.cue = _check_depth("SeriesProjector", depth, cue, mode)
        axes = tuple(axes)
        if not axes or any(a not in AXES for a in axes):
            raise ValueError("SeriesProjector: axes %r, a non-empty choice of %s expected" % (axes, AXES))
        self._volume(n, h, w)
        self.mode, self.axes = mode, tuple(a for a in AXES if a in axes)
        self.code = ops.PROJECT_MODES[mode]
        self.thick = self.n if slab is None else int(slab)
        self.slabs, self.div_last = slab_plan(self.n, self.thick)
        self.thick = min(self.thick, self.n)
        if self.depth and max(self.n, self.h, self.w) > 32767:
            raise ValueError("SeriesProjector: depth=True: no axis above %d voxels (a depth is an int16), got (%d, %d, %d)"
                             % (32767, self.n, self.h, self.w))
        self.device = self._gpu(device)
        shapes = {"axial": (self.slabs, self.h, self.w), "coronal": (self.n, self.w), "sagittal": (self.n, self.h)}
        self.acc = {a: torch.empty(shapes[a], dtype=torch.int32, device=self.device) for a in self.axes}
        self.reset()

    def reset(self):
        identity = ops.PROJECT_DEPTH_IDENTITY[self.code] if self.depth else ops.PROJECT_IDENTITY[self.code]
        for t in self.acc.values():
            t.fill_(identity)

    def update(self, pix_chunk, n0):
        self._chunk(pix_chunk, n0)      # (an empty chunk goes on to ops, which returns early)
        if self.depth:
            ops.project_accumulate_depth(pix_chunk, int(n0), self.thick, self.code, **self.acc)
        else:
            ops.project_accumulate(pix_chunk, int(n0), self.thick, self.code, **self.acc)

    def result(self, wc=50.0, ww=400.0, hu=False, level=True):
        if self.depth:
            extent = {"axial": (self.thick, self.n), "coronal": (self.h, self.h), "sagittal": (self.w, self.w)}
            out = {}
            for a, acc in self.acc.items():
                values, lvl, depth, cued = ops.project_finish_depth(acc, self.code, extent[a][0], extent[a][1], cue=self.cue, wc=wc,
                                                                    ww=ww, hu=hu, want_level=level, want_cued=level)
                out[a] = {"values": values, "level": lvl, "depth": depth}
                if level:
                    out[a]["cued"] = cued
            return out
        div = {"axial": (self.thick, self.div_last), "coronal": (self.h, self.h), "sagittal": (self.w, self.w)}
        out = {}
        for a, acc in self.acc.items():
            values, lvl = ops.project_finish(acc, self.code, div[a][0], div[a][1], wc=wc, ww=ww, hu=hu, want_level=level)
            out[a] = {"values": values, "level": lvl}
        return out


def project_volume(volume, mode="max", slab=None, wc=50.0, ww=400.0, hu=False, batch=64, axes=AXES, level=True, device=None,
                   depth=False, cue=0):
    """The projections of a volume that already exists (the input CT, the real CTA for a side-by-side view): int16 [N, H, W],
    a host array / CPU tensor (chunks of `batch` slices cross PCIe one after another) or a device tensor; depth and cue as
    `SeriesProjector`.  Returns what `SeriesProjector.result` returns, of the input's kind (numpy arrays, CPU tensors or device
    tensors)."""
    return _view_of_volume("project_volume", volume, batch, device,
                           lambda n, h, w, dev: SeriesProjector(n, h, w, mode=mode, slab=slab, axes=axes, device=dev, depth=depth, cue=cue),
                           result=lambda proj: proj.result(wc, ww, hu=hu, level=level))


def _per_axis(value, axes, what):
    """`thick` / `step` of SeriesSlabs: one int for every axis, or {axis: int} with an entry for each axis kept."""
    if isinstance(value, dict):
        if any(a not in value for a in axes):
            raise ValueError("SeriesSlabs: %s %r has no entry for every axis of %s" % (what, value, axes))
        return {a: int(value[a]) for a in axes}
    return {a: int(value) for a in axes}


class SeriesSlabs(_SeriesView):
    """Sliding thin-slab projections (STS-MIP / MinIP / mean) of an int16 volume [n, h, w] that arrives in chunks on the device:
    slabs of `thick` voxels moved on by `step` voxels (`slab_windows`; step=None: thick, slabs that do not overlap) along "axial"
    [J_a, h, w] (over slices), "coronal" [J_c, n, w] (over the rows of the slab) and "sagittal" [J_s, n, h] (over its columns).
    thick / step: an int for every axis or {axis: int} -- slice spacing and pixel spacing differ, so the axes want different
    counts.  mode "max", "min" or "mean" (the exact sum divided toward zero by the slab's own length); level=False skips the
    8-bit planes of the window (wc, ww, hu).  `update(pix_chunk, n0)` in any order, every slice once: a chunk finishes its own
    rows of every coronal and sagittal plane (`ops.project_slabs_inplane`) and is combined into the int32 axial accumulators
    (`ops.project_accumulate_sliding`); `result()` -> {axis: {"values": int16, "level": uint8 or None}} on the device finishes
    the axial ones (`ops.project_finish`); `reset()` refills only those.  `nbytes`: the device bytes of the outputs and the axial
    accumulators, known before the first chunk -- step = 1 makes J about the axis' length, so every axis then costs about a
    whole volume (and the axial one its int32 accumulators on top).  Exact integer arithmetic on the current stream: equal to
    numpy bit for bit."""

    def __init__(self, n, h, w, thick, step=None, mode="max", axes=AXES, wc=50.0, ww=400.0, hu=False, level=True, device=None):
        _one_of("SeriesSlabs", "mode", mode, PROJECTIONS)
        axes = tuple(axes)
        if not axes or any(a not in AXES for a in axes):
            raise ValueError("SeriesSlabs: axes %r, a non-empty choice of %s expected" % (axes, AXES))
        self._volume(n, h, w)
        self.mode, self.axes = mode, tuple(a for a in AXES if a in axes)
        self.code = ops.PROJECT_MODES[mode]
        self.given = _per_axis(thick, self.axes, "thick")      # what the kernels validate `step` against
        self.step = dict(self.given) if step is None else _per_axis(step, self.axes, "step")
        extent = {"axial": self.n, "coronal": self.h, "sagittal": self.w}
        self.slabs, self.thick, self.last_len = {}, {}, {}
        for a in self.axes:
            self.slabs[a], self.thick[a], self.last_len[a] = slab_windows(extent[a], self.given[a], self.step[a])
        self.hu, self.window, self.want_level = bool(hu), (float(wc), float(ww)), bool(level)
        self.device = self._gpu(device)
        shapes = {"coronal": (self.n, self.w), "sagittal": (self.n, self.h)}
        self.values = {a: torch.empty((self.slabs[a],) + shapes[a], dtype=torch.int16, device=self.device)
                       for a in self.axes if a != "axial"}
        self.level = {a: torch.empty(t.shape, dtype=torch.uint8, device=self.device) if self.want_level else None
                      for a, t in self.values.items()}
        self.acc = None
        if "axial" in self.axes:
            self.acc = torch.empty((self.slabs["axial"], self.h, self.w), dtype=torch.int32, device=self.device)
        per_item = 2 + (1 if self.want_level else 0)
        self.nbytes = sum(t.numel() * per_item for t in self.values.values())
        if self.acc is not None:
            self.nbytes += self.acc.numel() * (4 + per_item)
        self.reset()

    def reset(self):
        """For the next volume of the same shape: only the axial accumulators are refilled (every update writes whole rows of
        the coronal and sagittal planes)."""
        if self.acc is not None:
            self.acc.fill_(ops.PROJECT_IDENTITY[self.code])

    def update(self, pix_chunk, n0):
        k = self._chunk(pix_chunk, n0)
        if k < 1:
            return
        for a in self.values:
            ops.project_slabs_inplane(pix_chunk, int(n0), a, self.given[a], self.step[a], self.code, values=self.values[a],
                                      level=self.level[a], wc=self.window[0], ww=self.window[1], hu=self.hu)
        if self.acc is not None:
            ops.project_accumulate_sliding(pix_chunk, int(n0), self.n, self.given["axial"], self.step["axial"], self.code, self.acc)

    def result(self):
        out = {}
        for a in self.axes:
            if a == "axial":
                values, lvl = ops.project_finish(self.acc, self.code, self.thick[a], self.last_len[a], wc=self.window[0],
                                                 ww=self.window[1], hu=self.hu, want_level=self.want_level)
                out[a] = {"values": values, "level": lvl}
            else:
                out[a] = {"values": self.values[a], "level": self.level[a]}
        return out


def slab_volume(volume, thick, step=None, mode="max", axes=AXES, wc=50.0, ww=400.0, hu=False, level=True, batch=64, device=None):
    """The sliding thin-slab projections of a volume that already exists, the twin of `project_volume`: int16 [N, H, W], a host
    array / CPU tensor (chunks of `batch` slices cross PCIe one after another) or a device tensor.  Arguments as `SeriesSlabs`.
    Returns what `SeriesSlabs.result` returns, of the input's kind (numpy arrays, CPU tensors or device tensors)."""
    return _view_of_volume("slab_volume", volume, batch, device,
                           lambda n, h, w, dev: SeriesSlabs(n, h, w, thick, step=step, mode=mode, axes=axes, wc=wc, ww=ww, hu=hu,
                                                            level=level, device=dev))


def default_detector(h, w):
    """D = ceil(hypot(h, w)): a detector of D columns and rays of D unit steps see the whole h x w slice at every angle."""
    return int(math.ceil(math.hypot(int(h), int(w))))


def view_angles(count, span=360.0, start=0.0):
    """`count` view angles in degrees, start + i * span / count."""
    count = int(count)
    if count < 1:
        raise ValueError("view_angles: at least one angle expected, got %d" % count)
    return [float(start) + i * float(span) / count for i in range(count)]


def rotation_coefficients(angle, h, w, u=None, t=None, oversample=1):
    """The six 16.16 fixed-point coefficients (c0 .. c5) of the view at `angle` degrees about the axis through the centre
    ((w-1)/2, (h-1)/2) of an h x w slice, for a detector of u columns and rays of t voxels (default: `default_detector`) taken
    in t s steps of 1 / s voxel, s = `oversample`: sample (i, j) of the view is pixel x = (c0 + c1 i + c2 j) >> 16,
    y = (c3 + c4 i + c5 j) >> 16, the nearest pixel to
        x = cx + (i - cu) cos - (j/s - ct) sin,   y = cy + (i - cu) sin + (j/s - ct) cos,   cu = (u-1)/2, ct = (t s - 1)/(2 s).
    0 degrees is the coronal view (rays along y, the detector along x), 90 the sagittal one.  float64, rounded by
    floor(v * 65536 + 0.5); s = 1 divides by exactly 1, so its six integers are those of unit steps.  The kernels are called
    with T = t s steps."""
    h, w, s = int(h), int(w), int(oversample)
    d = default_detector(h, w)
    u, t = d if u is None else int(u), d if t is None else int(t)
    if min(h, w, u, t) < 1 or max(h, w, u, t) > ops.ROTATE_MAX_DIM:
        raise ValueError("rotation_coefficients: h, w, u, t in 1 .. %d expected, got %d %d %d %d" % (ops.ROTATE_MAX_DIM, h, w, u, t))
    if s < 1 or t * s > ops.ROTATE_MAX_DIM:
        raise ValueError("rotation_coefficients: oversample >= 1 and t * oversample <= %d steps expected, got t = %d, "
                         "oversample = %d: %d steps" % (ops.ROTATE_MAX_DIM, t, s, t * s))
    rad = math.radians(float(angle))
    cos, sin = math.cos(rad), math.sin(rad)
    cx, cy, cu, ct = (w - 1) / 2.0, (h - 1) / 2.0, (u - 1) / 2.0, (t * s - 1) / (2.0 * s)

    def r(v):
        return int(math.floor(v * 65536.0 + 0.5))

    return (r(cx - cu * cos + ct * sin + 0.5), r(cos), r(-sin / s), r(cy - cu * sin - ct * cos + 0.5), r(sin), r(cos / s))


def ray_voxel(coef_row, u, t):
    """(x, y): the pixel of the slice that sample (u, t) of a rotated view falls in, by the kernel's nearest rule
    x = (c0 + c1 u + c2 t) >> 16, y = (c3 + c4 u + c5 t) >> 16 (arithmetic shift) for the view's coefficient row (c0 .. c5)
    (`rotation_coefficients`, a row of `SeriesRotator.table.host`).  With t = the "depth" of detector column u in row n of the
    view, (n, y, x) is the voxel the projected value came from (nearest sampling; with bilinear sampling, the pixel the sample
    counts by).  A pure host function; u and t may be integers or integer arrays, a missed ray (depth -1) has no voxel."""
    c = [int(v) for v in coef_row]
    if len(c) != 6:
        raise ValueError("ray_voxel: a coefficient row of six integers expected, got %d" % len(c))
    u, t = np.asarray(u, dtype=np.int64), np.asarray(t, dtype=np.int64)
    x, y = (c[0] + c[1] * u + c[2] * t) >> 16, (c[3] + c[4] * u + c[5] * t) >> 16
    return (int(x), int(y)) if x.ndim == 0 else (x, y)


def _check_sampling(who, sampling, oversample):
    _one_of(who, "sampling", sampling, tuple(ops.ROTATE_SAMPLINGS))
    _int_in(who, "oversample", oversample, 1)


class SeriesRotator(_SeriesView):
    """Rotating projections of an int16 volume [n, h, w] that arrives in chunks on the device: one plane [n, U] per view angle
    (degrees about the cranio-caudal axis; 0 = coronal, 90 = sagittal), mode "max", "min" or "mean" along rays of T voxels.
    detector: None (U = T = `default_detector`), an int or (U, T).  sampling: "nearest" or "bilinear"; oversample = s >= 1: a ray
    takes `.steps` = T s steps of 1 / s voxel (`.t` stays T).  A ray that misses the slice gets `fill` (default: air, 0 or
    -1024 with `hu`); level=False skips the 8-bit planes of the window (wc, ww).  `update(pix_chunk, n0)` in any order, every
    slice once: a chunk finishes its own rows of every angle; `result()` -> {"values": int16 [A, n, U], "level": uint8 or None,
    "angles": float64 [A]} on the device.  Exact integer arithmetic on the current stream: equal to numpy bit for bit.
    depth=True (mode "max" / "min"): the result gains "depth" int16 [A, n, U] -- the step 0 .. `.steps`-1, counted from the
    viewer's end of the ray, of the first counted sample that attains the value; -1 where the ray misses the slice (`ray_voxel`
    maps it back to the pixel) -- and, with level, "cued" uint8: the level attenuated by the depth, (level w + 128) >> 8 with
    w = 256 - (cue depth) / steps, `cue` in 0 .. 256.  One launch per chunk either way: the depth entry replaces the plain one."""

    def __init__(self, n, h, w, angles, mode="max", detector=None, fill=None, wc=50.0, ww=400.0, hu=False, level=True, device=None,
                 sampling="nearest", oversample=1, depth=False, cue=0):
        _one_of("SeriesRotator", "mode", mode, PROJECTIONS)
        self.depth, self.cue = _check_depth("SeriesRotator", depth, cue, mode)
        self.mode, self.code = mode, ops.PROJECT_MODES[mode]
        self.hu, self.window = bool(hu), (float(wc), float(ww))
        self.fill = (-1024 if self.hu else 0) if fill is None else int(fill)
        self._rays(n, h, w, angles, detector, sampling, oversample, device)
        shape = (len(self.angles), self.n, self.u)
        self.values = torch.empty(shape, dtype=torch.int16, device=self.device)
        self.level = torch.empty(shape, dtype=torch.uint8, device=self.device) if level else None
        self.depth_plane = torch.empty(shape, dtype=torch.int16, device=self.device) if self.depth else None
        self.cued = torch.empty(shape, dtype=torch.uint8, device=self.device) if self.depth and level else None
        self._angles = torch.tensor(self.angles, dtype=torch.float64, device=self.device)

    def update(self, pix_chunk, n0):
        k = self._chunk(pix_chunk, n0)
        if k < 1:
            return
        if self.depth:
            ops.project_rotate_depth(pix_chunk, int(n0), self.table, self.steps, self.code, values=self.values, level=self.level,
                                     depth=self.depth_plane, cued=self.cued, cue=self.cue, fill=self.fill, wc=self.window[0],
                                     ww=self.window[1], hu=self.hu, sampling=self.sampling)
            return
        ops.project_rotate(pix_chunk, int(n0), self.table, self.steps, self.code, values=self.values, level=self.level,
                           fill=self.fill, wc=self.window[0], ww=self.window[1], hu=self.hu, sampling=self.sampling)

    def result(self):
        out = {"values": self.values, "level": self.level, "angles": self._angles}
        if self.depth:
            out["depth"] = self.depth_plane
            if self.cued is not None:
                out["cued"] = self.cued
        return out


def rotate_volume(volume, angles, mode="max", detector=None, fill=None, wc=50.0, ww=400.0, hu=False, level=True, batch=64,
                  device=None, sampling="nearest", oversample=1, depth=False, cue=0):
    """The rotating projections of a volume that already exists, the counterpart of `project_volume`: int16 [N, H, W], a host
    array / CPU tensor (chunks of `batch` slices cross PCIe one after another) or a device tensor; angles: degrees, or an int
    count of views around the full circle (`view_angles`); sampling, oversample, depth and cue as `SeriesRotator`.  Returns what
    `SeriesRotator.result` returns, of the input's kind."""
    return _view_of_volume("rotate_volume", volume, batch, device,
                           lambda n, h, w, dev: SeriesRotator(n, h, w, _angle_list(angles), mode=mode, detector=detector, fill=fill,
                                                              wc=wc, ww=ww, hu=hu, level=level, device=dev, sampling=sampling,
                                                              oversample=oversample, depth=depth, cue=cue))


def transfer_function(points, oversample=1):
    """The transfer table of `SeriesRenderer` / `ops.project_render` from control points: a sequence of (level, r, g, b, opacity)
    with levels strictly ascending in 0 .. 255, colours in 0 .. 255 and opacity in 0.0 .. 1.0.  Every channel is interpolated
    linearly over the classes 0 .. 255 in float64 (np.interp: the first and last point extend to the ends); colours round by
    floor(x + 0.5).  oversample = s: a ray that takes s steps per voxel meets s samples where it met one, so the opacity is
    corrected per step, a_s = 1 - (1 - a) ** (1 / s) (s = 1 changes nothing), and alpha = floor(a_s * 32768 + 0.5), 32768 = opaque.
    Returns uint16 [256, 4]: R, G, B, alpha."""
    _int_in("transfer_function", "oversample", oversample, 1)
    try:
        pts = np.array([[float(v) for v in p] for p in points], dtype=np.float64)
    except (TypeError, ValueError):
        pts = np.zeros((0, 5))
    if pts.ndim != 2 or pts.shape[0] < 1 or pts.shape[1] != 5 or not np.isfinite(pts).all():
        raise ValueError("transfer_function: a sequence of (level, r, g, b, opacity) points expected, got %r" % (points,))
    lv = pts[:, 0]
    if (lv != np.floor(lv)).any() or lv.min() < 0 or lv.max() > 255 or (np.diff(lv) <= 0).any():
        raise ValueError("transfer_function: whole levels in 0 .. 255, strictly ascending, expected, got %s" % lv.tolist())
    if pts[:, 1:4].min() < 0 or pts[:, 1:4].max() > 255 or pts[:, 4].min() < 0 or pts[:, 4].max() > 1:
        raise ValueError("transfer_function: colours in 0 .. 255 and opacities in 0.0 .. 1.0 expected")
    classes = np.arange(256, dtype=np.float64)
    lut = np.empty((256, 4), dtype=np.uint16)
    for c in range(3):
        lut[:, c] = np.floor(np.interp(classes, lv, pts[:, 1 + c]) + 0.5).astype(np.uint16)
    a = np.interp(classes, lv, pts[:, 4])
    if int(oversample) > 1:
        a = 1.0 - (1.0 - a) ** (1.0 / int(oversample))
    lut[:, 3] = np.floor(a * 32768.0 + 0.5).astype(np.uint16)
    return lut


# Named control points of `transfer_function`, for classes of the default transfer window (wc 300, ww 1500: about 5.9 HU per class,
# class 0 at -450 HU).  They are data: their look cannot be judged without a display and none was at hand, so they are a first
# guess by HU range, not tuned.
TRANSFER_PRESETS = {
    # R = G = B = the class, opacity a ramp
    "grey": [(0, 0, 0, 0, 0.0), (255, 255, 255, 255, 1.0)],
    # soft tissue (below about 110 HU) transparent, contrast-filled lumen red and near-opaque, bone pale and opaque
    "vessels": [(0, 0, 0, 0, 0.0), (95, 150, 60, 50, 0.0), (115, 210, 40, 30, 0.6), (150, 235, 50, 35, 0.9), (185, 240, 230, 200, 1.0),
                (255, 255, 255, 240, 1.0)],
    # everything below about 400 HU transparent, bone pale and opaque
    "bone": [(0, 0, 0, 0, 0.0), (145, 150, 120, 90, 0.0), (185, 230, 215, 180, 0.8), (255, 255, 255, 245, 1.0)],
}


def _transfer_table(who, transfer, oversample):
    """`transfer` of SeriesRenderer -> uint16 [256, 4]: a preset name, a point list (both through `transfer_function` with the
    renderer's oversample) or a ready table (taken as it is: whoever made it corrected it)."""
    if isinstance(transfer, str):
        _one_of(who, "transfer", transfer, tuple(TRANSFER_PRESETS))
        return transfer_function(TRANSFER_PRESETS[transfer], oversample)
    table = transfer.cpu().numpy() if torch.is_tensor(transfer) else transfer
    if isinstance(table, np.ndarray) and table.shape == (256, 4):
        return table
    return transfer_function(transfer, oversample)


class SeriesRenderer(_SeriesView):
    """Volume-rendered rotating views of an int16 volume [n, h, w] that arrives in chunks on the device: the rays, angles,
    detector, sampling and oversample of `SeriesRotator`, composited front to back instead of reduced to a maximum, so that what
    lies in front hides what lies behind.  A sample's class is its 8-bit level in the transfer window (wc, ww) (with `hu` as
    everywhere); `transfer` -- a name of TRANSFER_PRESETS, a point list for `transfer_function` (both corrected for `oversample`)
    or a ready [256, 4] table -- gives every class its colour and alpha.  A ray ends once its transparency is down to `stop`
    (of 32768); `surface` (1 .. 32768) is the accumulated opacity whose first step the depth plane records.  `update(pix_chunk,
    n0)` in any order, every slice once: a chunk finishes its own rows of every angle in one launch (`ops.project_render`);
    `result()` -> {"rgb": uint8 [A, n, U, 3], "opacity": uint8 [A, n, U], "depth": int16 [A, n, U] (absent with depth=False; -1
    where the ray never reaches `surface`; `ray_voxel` maps a hit back to the pixel), "angles": float64 [A]} on the device.  Exact
    integer arithmetic on the current stream: equal to numpy bit for bit."""

    def __init__(self, n, h, w, angles, transfer="vessels", detector=None, wc=300.0, ww=1500.0, hu=False, sampling="nearest",
                 oversample=1, background=(0, 0, 0), stop=128, surface=16384, depth=True, device=None):
        _check_sampling("SeriesRenderer", sampling, oversample)
        self.background, self.stop, self.surface = _check_compositing("SeriesRenderer", background, stop, surface)
        self.hu, self.window = bool(hu), (float(wc), float(ww))
        lut = _transfer_table("SeriesRenderer", transfer, int(oversample))
        self._rays(n, h, w, angles, detector, sampling, oversample, device)
        self.lut = ops.TransferTable(lut, self.device)
        shape = (len(self.angles), self.n, self.u)
        self.rgb = torch.empty(shape + (3,), dtype=torch.uint8, device=self.device)
        self.opacity = torch.empty(shape, dtype=torch.uint8, device=self.device)
        self.depth_plane = torch.empty(shape, dtype=torch.int16, device=self.device) if depth else None
        self._angles = torch.tensor(self.angles, dtype=torch.float64, device=self.device)

    def update(self, pix_chunk, n0):
        k = self._chunk(pix_chunk, n0)
        if k < 1:
            return
        ops.project_render(pix_chunk, int(n0), self.table, self.steps, self.lut, rgb=self.rgb, opacity=self.opacity,
                           depth=self.depth_plane, background=self.background, stop=self.stop, surface=self.surface,
                           wc=self.window[0], ww=self.window[1], hu=self.hu, sampling=self.sampling)

    def result(self):
        out = {"rgb": self.rgb, "opacity": self.opacity, "angles": self._angles}
        if self.depth_plane is not None:
            out["depth"] = self.depth_plane
        return out


def render_volume(volume, angles, batch=64, device=None, **options):
    """The volume-rendered views of a volume that already exists, the counterpart of `rotate_volume`: int16 [N, H, W], a host
    array / CPU tensor (chunks of `batch` slices cross PCIe one after another) or a device tensor; angles: degrees, or an int
    count of views around the full circle (`view_angles`); options: the keyword arguments of `SeriesRenderer` (transfer,
    detector, wc, ww, hu, sampling, oversample, background, stop, surface, depth).  Returns what `SeriesRenderer.result`
    returns, of the input's kind."""
    return _view_of_volume("render_volume", volume, batch, device,
                           lambda n, h, w, dev: SeriesRenderer(n, h, w, _angle_list(angles), device=dev, **options))


# ------------------------------------------------------------------------------------------------ lines in any direction
# Coordinates are (x, y, z) = (column, row, slice).  In "pixel units" the in-plane pitch is 1 and the slice pitch is `aspect`
# (slice spacing / pixel spacing): a point q is voxel (qx, qy, qz / aspect) and the volume's centre is ((w-1)/2, (h-1)/2,
# (n-1) aspect / 2).  The anisotropy is in the table, so the output is isotropic and no row is repeated on the host.
REFORMAT_SAMPLINGS = tuple(ops.REFORMAT_SAMPLINGS)
AXIS_VECTORS = {"x": (1.0, 0.0, 0.0), "y": (0.0, 1.0, 0.0), "z": (0.0, 0.0, 1.0)}


class LineSet(tuple):
    """What the geometry functions return: the pair (table, T) -- an int64 line table [..., rows, 9] for `ops.reformat_lines`
    and the steps per ray -- that also remembers `.cols`, the samples per line the table was made for."""

    def __new__(cls, table, steps, cols):
        self = super().__new__(cls, (table, int(steps)))
        self.cols = int(cols)
        return self


def _r16(v):
    return np.floor(np.asarray(v, dtype=np.float64) * 65536.0 + 0.5).astype(np.int64)


def _vec3(who, name, v):
    v = AXIS_VECTORS.get(v, v) if isinstance(v, str) else v
    try:
        a = np.array([float(c) for c in v], dtype=np.float64)
    except (TypeError, ValueError):
        a = np.zeros(0)
    if a.shape != (3,) or not np.isfinite(a).all():
        raise ValueError("%s: %s: three finite numbers (x, y, z)%s expected, got %r"
                         % (who, name, " or one of 'x', 'y', 'z'" if name == "axis" else "", v))
    return a


def _unit(who, name, v):
    a = _vec3(who, name, v)
    length = math.sqrt(float(a @ a))
    if length < 1e-12:
        raise ValueError("%s: %s has no direction: %r" % (who, name, v))
    return a / length


def _line_geometry(who, n, h, w, rows, cols, depth, oversample, aspect):
    n, h, w, rows, cols, depth = int(n), int(h), int(w), int(rows), int(cols), int(depth)
    _int_in(who, "oversample", oversample, 1)
    s, aspect = int(oversample), float(aspect)
    if min(n, h, w) < 1 or max(n, h, w) > ops.REFORMAT_MAX_DIM:
        raise ValueError("%s: n, h, w in 1 .. %d expected, got %d %d %d" % (who, ops.REFORMAT_MAX_DIM, n, h, w))
    if rows < 1 or not 1 <= cols <= ops.REFORMAT_MAX_DIM or depth < 1 or depth * s > ops.REFORMAT_MAX_DIM:
        raise ValueError("%s: rows >= 1, cols in 1 .. %d and depth * oversample in 1 .. %d steps expected, got rows = %d, cols = %d, "
                         "depth = %d, oversample = %d" % (who, ops.REFORMAT_MAX_DIM, ops.REFORMAT_MAX_DIM, rows, cols, depth, s))
    if not (aspect > 0 and math.isfinite(aspect)):
        raise ValueError("%s: aspect: a positive ratio expected, got %r" % (who, aspect))
    return n, h, w, rows, cols, depth, s, aspect


def volume_centre(n, h, w, aspect=1.0):
    """The centre of an n x h x w volume in pixel units, (x, y, z)."""
    return np.array([(int(w) - 1) / 2.0, (int(h) - 1) / 2.0, (int(n) - 1) * float(aspect) / 2.0])


def _table(start, right, forward, s, aspect):
    """int64 [R, 9]: lines that start (sample 0, step 0) at start [R, 3], move by right [R, 3] per sample and by forward [R, 3] / s
    per step, all in pixel units; every coefficient is rounded on its own, the start with the + 0.5 of the nearest rule."""
    scale = np.array([1.0, 1.0, aspect])
    out = np.empty((start.shape[0], 9), dtype=np.int64)
    out[:, 0::3] = _r16(start / scale + 0.5)
    out[:, 1::3] = _r16(right / scale)
    out[:, 2::3] = _r16(forward / s / scale)
    return out


def view_lines(n, h, w, right, down, forward, rows, cols, depth=1, offset=0.0, oversample=1, aspect=1.0, centre=None):
    """A parallel view of an n x h x w volume as a line table: -> `LineSet` (table int64 [rows, 9], T = depth * oversample).
    (right, down, forward): an orthonormal basis in pixel units (anything else is refused); sample (r, i, k) lies at
        q = centre + (i - cu) right + (r - cr) down + (offset + k/s - ct) forward,
        cu = (cols-1)/2, cr = (rows-1)/2, ct = (depth s - 1)/(2 s), s = oversample
    (`rotation_coefficients` has the same cu and ct), centre: (x, y, z) in pixel units, default `volume_centre`.  A ray is `depth`
    voxels long in depth * s steps and centred `offset` in front of the plane through the centre.  float64, every coefficient
    rounded by floor(v * 65536 + 0.5)."""
    who = "view_lines"
    n, h, w, rows, cols, depth, s, aspect = _line_geometry(who, n, h, w, rows, cols, depth, oversample, aspect)
    basis = np.stack([_vec3(who, "right", right), _vec3(who, "down", down), _vec3(who, "forward", forward)])
    if np.abs(basis @ basis.T - np.eye(3)).max() > 1e-6:
        raise ValueError("%s: (right, down, forward) is not an orthonormal basis: %r %r %r" % (who, right, down, forward))
    c = volume_centre(n, h, w, aspect) if centre is None else _vec3(who, "centre", centre)
    cu, cr, ct = (cols - 1) / 2.0, (rows - 1) / 2.0, (depth * s - 1) / (2.0 * s)
    r = np.arange(rows, dtype=np.float64)[:, None]
    start = c[None, :] + (-cu) * basis[0][None, :] + (r - cr) * basis[1][None, :] + (float(offset) - ct) * basis[2][None, :]
    ones = np.ones((rows, 1))
    return LineSet(_table(start, ones * basis[0][None, :], ones * basis[2][None, :], s, aspect), depth * s, cols)


def _rotate_about(v, axis, degrees):
    """v turned by `degrees` about the unit vector `axis` (Rodrigues; exact where the components are 0 and 1)."""
    rad = math.radians(float(degrees))
    cos, sin = math.cos(rad), math.sin(rad)
    return v * cos + np.cross(axis, v) * sin + axis * (float(axis @ v) * (1.0 - cos))


def _cover(n, h, w, aspect):
    """ceil of the volume's diagonal in pixel units: a view of that many rows, columns and voxels of depth sees all of it."""
    return int(math.ceil(math.sqrt(float(w) ** 2 + float(h) ** 2 + (float(n) * aspect) ** 2)))


def orbit_lines(n, h, w, angles, axis="z", rows=None, cols=None, depth=None, offset=0.0, oversample=1, aspect=1.0, centre=None):
    """The views of an orbit: -> `LineSet` (table int64 [A, rows, 9], T).  The coronal view -- right = +x, down = +z,
    forward = +y -- turned by each of `angles` (degrees) about `axis` through the centre: "z" is the spin of `SeriesRotator`,
    "x" the tumble, "y", or any 3-vector (x, y, z).  Defaults that let every angle see the whole volume: about z, rows =
    ceil(n aspect) and cols = depth = `default_detector`; about any other axis all three are the ceil of the volume's diagonal.
    With axis "z", aspect 1, rows = n and cols = depth = `default_detector`, the x and y columns of every row are the six integers
    of `rotation_coefficients` and z0 = (r << 16) + 32768, zu = zk = 0."""
    who = "orbit_lines"
    a = _unit(who, "axis", axis)
    angles = [float(v) for v in angles]
    if not angles:
        raise ValueError("%s: at least one angle expected" % who)
    spin = isinstance(axis, str) and axis == "z"
    d = default_detector(h, w) if spin else _cover(n, h, w, float(aspect))
    rows = (max(1, int(math.ceil(int(n) * float(aspect) - 1e-9))) if spin else d) if rows is None else rows
    cols, depth = d if cols is None else cols, d if depth is None else depth
    right, down, forward = (np.array(AXIS_VECTORS[k]) for k in "xzy")
    sets = [view_lines(n, h, w, _rotate_about(right, a, v), _rotate_about(down, a, v), _rotate_about(forward, a, v), rows, cols,
                       depth, offset, oversample, aspect, centre) for v in angles]
    return LineSet(np.stack([t for t, _ in sets]), sets[0][1], sets[0].cols)


def oblique_lines(n, h, w, normal, up=None, count=1, pitch=1.0, thick=1, rows=None, cols=None, oversample=1, aspect=1.0, centre=None):
    """Parallel oblique planes: -> `LineSet` (table int64 [count, rows, 9], T = thick * oversample).  `count` planes with the
    normal `normal` (x, y, z; pixel units), `pitch` apart along it and centred on the centre, each `thick` voxels deep along the
    normal (mode picks the slab's projection).  In the plane, `down` is the +z axis projected into it (the +y axis where the
    normal is within 1e-6 of z), or the opposite of `up` projected into it when `up` is given; `right` completes the basis and
    points toward +x (toward +y where it has no x component).  Defaults: rows and cols cover the volume's extent along down and
    right.  So, with aspect 1 and pitch 1: normal +z, count n returns the slices as stored; normal +y, count h returns
    vol[:, y, :]; normal +x, count w returns vol[:, :, x]."""
    who = "oblique_lines"
    forward = _unit(who, "normal", normal)
    count = int(count)
    if count < 1 or not (float(pitch) > 0 and math.isfinite(float(pitch))):
        raise ValueError("%s: count >= 1 and pitch > 0 expected, got %r %r" % (who, count, pitch))
    if up is not None:
        ref = -_unit(who, "up", up)
    else:
        ref = np.array(AXIS_VECTORS["y" if abs(forward[2]) > 1.0 - 1e-6 else "z"])
    down = ref - float(ref @ forward) * forward
    if math.sqrt(float(down @ down)) < 1e-6:
        raise ValueError("%s: up %r runs along the normal %r" % (who, up, normal))
    down = down / math.sqrt(float(down @ down))
    right = np.cross(down, forward)
    lead = right[0] if abs(right[0]) > 1e-9 else (right[1] if abs(right[1]) > 1e-9 else right[2])
    if lead < 0:
        right = -right
    size = np.array([float(w), float(h), float(n) * float(aspect)])
    rows = max(1, int(math.ceil(float(np.abs(down) @ size) - 1e-9))) if rows is None else rows
    cols = max(1, int(math.ceil(float(np.abs(right) @ size) - 1e-9))) if cols is None else cols
    sets = [view_lines(n, h, w, right, down, forward, rows, cols, thick, (p - (count - 1) / 2.0) * float(pitch), oversample, aspect,
                       centre) for p in range(count)]
    return LineSet(np.stack([t for t, _ in sets]), sets[0][1], sets[0].cols)


def _centreline_frames(who, centreline, pitch, aspect):
    """What `curved_lines` and `lumen_lines` share: a centreline float [M >= 2, 3] in (z, y, x) voxel order -> (q [R, 3], the points
    at arc length r pitch in (x, y, z) pixel units, R = floor(length / pitch) + 1; f1, f2 [R, 3], the parallel-transported frame
    across the line at each; at [R], the arc lengths).  The tangents are central differences of the resampled points (one-sided at
    the ends); e1 is re-projected orthogonal to each new tangent and normalised, e2 = tangent x e1; e1 starts from the x axis, or
    from the y axis where the first tangent is within 1e-6 of x."""
    pts = np.asarray(centreline, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[1] != 3 or pts.shape[0] < 2 or not np.isfinite(pts).all():
        raise ValueError("%s: a centreline of M >= 2 finite points (z, y, x) expected, got an array of shape %s" % (who, pts.shape))
    if not (float(pitch) > 0 and math.isfinite(float(pitch))):
        raise ValueError("%s: pitch > 0 expected, got %r" % (who, pitch))
    p = pts[:, ::-1] * np.array([1.0, 1.0, aspect])      # (x, y, z) in pixel units
    seg = np.sqrt(((p[1:] - p[:-1]) ** 2).sum(axis=1))
    arc = np.concatenate([[0.0], np.cumsum(seg)])
    if arc[-1] <= 0 or (seg <= 0).any():
        raise ValueError("%s: the centreline repeats a point" % who)
    at = np.arange(int(math.floor(arc[-1] / float(pitch) + 1e-9)) + 1, dtype=np.float64) * float(pitch)
    q = np.stack([np.interp(at, arc, p[:, j]) for j in range(3)], axis=1)      # [R, 3]
    if len(q) > 1:
        tan = np.empty_like(q)
        tan[1:-1], tan[0], tan[-1] = q[2:] - q[:-2], q[1] - q[0], q[-1] - q[-2]
    else:
        tan = (p[-1] - p[0])[None, :]
    tan = tan / np.sqrt((tan ** 2).sum(axis=1))[:, None]
    e1 = np.array(AXIS_VECTORS["y" if abs(tan[0][0]) > 1.0 - 1e-6 else "x"])
    f1, f2 = np.empty_like(q), np.empty_like(q)
    for r in range(len(q)):
        e1 = e1 - float(e1 @ tan[r]) * tan[r]
        e1 = e1 / math.sqrt(float(e1 @ e1))      # (a turn of 90 degrees between two rows would leave nothing: pitch too coarse)
        f1[r], f2[r] = e1, np.cross(tan[r], e1)
    return q, f1, f2, at


def curved_lines(n, h, w, centreline, angles=(0.0,), cols=65, depth=1, pitch=1.0, oversample=1, aspect=1.0):
    """The straightened curved reformat along a centreline: -> `LineSet` (table int64 [A, R, 9], T = depth * oversample).
    centreline: float [M >= 2, 3] in (z, y, x) voxel order.  It is resampled linearly at arc-length `pitch` (pixel units): R =
    floor(length / pitch) + 1 rows p_r; the tangents are central differences of the resampled points (one-sided at the ends);
    the frame (e1, e2) is carried along by parallel transport -- e1 is re-projected orthogonal to each new tangent and normalised,
    e2 = tangent x e1 -- and starts from the x axis, or from the y axis where the first tangent is within 1e-6 of x.  Row r at
    angle phi (degrees) samples p_r + (i - cu) (cos phi e1 + sin phi e2), cu = (cols-1)/2, and its slab of `depth` voxels runs
    along -sin phi e1 + cos phi e2, centred on the line.  For a straight centreline along z through (y0, x0) with aspect 1, angle
    0 reads vol[r, y0, x0 + i - cu]."""
    who = "curved_lines"
    angles = [float(v) for v in angles]
    if not angles:
        raise ValueError("%s: at least one angle expected" % who)
    n, h, w, _, cols, depth, s, aspect = _line_geometry(who, n, h, w, 1, cols, depth, oversample, aspect)
    q, f1, f2, _ = _centreline_frames(who, centreline, pitch, aspect)
    cu, ct = (cols - 1) / 2.0, (depth * s - 1) / (2.0 * s)
    tables = []
    for phi in angles:
        rad = math.radians(phi)
        cos, sin = math.cos(rad), math.sin(rad)
        right, forward = cos * f1 + sin * f2, (-sin) * f1 + cos * f2
        tables.append(_table(q + (-cu) * right + (-ct) * forward, right, forward, s, aspect))
    return LineSet(np.stack(tables), depth * s, cols)


class LumenSet(tuple):
    """What `lumen_lines` returns: the pair (table, T) like a `LineSet` -- an int64 table [R, rays, 9] for `ops.lumen_sections` and
    the steps per ray -- that also remembers `.rays`, `.steps` (= T), `.oversample` and `.arc`, float64 [R]: the arc length of
    every section along the centreline in pixel units.  `.cols` = rays: the table passes wherever a `LineSet` does."""

    def __new__(cls, table, steps, rays, oversample, arc):
        self = super().__new__(cls, (table, int(steps)))
        self.rays = self.cols = int(rays)
        self.steps, self.oversample = int(steps), int(oversample)
        self.arc = np.asarray(arc, dtype=np.float64)
        return self


def lumen_lines(n, h, w, centreline, rays=32, reach=16.0, pitch=1.0, oversample=2, aspect=1.0):
    """The ray fans that measure the lumen along a centreline: -> `LumenSet` (table int64 [R, rays, 9], T = floor(reach * oversample)
    + 1).  The centreline, its resampling at arc length `pitch` and the frame (e1, e2) across it are those of `curved_lines`.
    Section r has `rays` = 8, 16, 32 or 64 rays from the point p_r: ray j runs along cos(2 pi j / rays) e1 + sin(2 pi j / rays) e2
    in steps of 1 / oversample pixel, k = 0 at the centre, out to `reach` pixels; 2 <= T <= 256.  Every row holds the centre as its
    start, the ray's step in the k columns and 0 in the sample columns; `aspect` is inside the table like everywhere."""
    who = "lumen_lines"
    if isinstance(rays, bool) or rays not in ops.LUMEN_RAYS:
        raise ValueError("%s: rays %r is not one of %s" % (who, rays, ops.LUMEN_RAYS))
    n, h, w, _, _, _, s, aspect = _line_geometry(who, n, h, w, 1, 1, 1, oversample, aspect)
    reach = float(reach)
    steps = int(math.floor(reach * s + 1e-9)) + 1 if math.isfinite(reach) and reach > 0 else 0
    if not 2 <= steps <= ops.LUMEN_MAX_STEPS:
        raise ValueError("%s: floor(reach * oversample) + 1 = %d steps, 2 .. %d expected (reach %r, oversample %d)"
                         % (who, steps, ops.LUMEN_MAX_STEPS, reach, s))
    q, f1, f2, at = _centreline_frames(who, centreline, pitch, aspect)
    table = np.empty((len(q), int(rays), 9), dtype=np.int64)
    zero = np.zeros_like(q)
    for j in range(int(rays)):
        phi = 2.0 * math.pi * j / int(rays)
        table[:, j] = _table(q, zero, math.cos(phi) * f1 + math.sin(phi) * f2, s, aspect)
    return LumenSet(table, steps, rays, s, at)


def lumen_profile(result, pixel_mm=1.0, oversample=None, arc=None):
    """The measurements of a lumen result on the host, float64: result = {"radii", "cross", "sections", "centres"} (arrays or
    tensors, as `VolumeLumen.result` returns them, which also carries "oversample" and "arc"; either may be given here instead)
    -> {"area" [R] in mm^2: the polygon through the boundary points, sin(2 pi / K) / 2 * cross; "equivalent": 2 sqrt(area / pi);
    "dmin", "dmax": the least and greatest chord through the centre; "mean": twice the mean radius; "arc": the position along the line
    -- all in mm, a pixel being `pixel_mm` --; "valid" bool [R]: no open ray and the centre inside the band (a branch, a gap in the
    contrast or the edge of the volume leaves rays open: the numbers of such a section are there but mean little)}."""
    def host(v):
        return np.asarray(v.cpu() if torch.is_tensor(v) else v)
    radii, cross, sections = host(result["radii"]), host(result["cross"]), host(result["sections"])
    if radii.ndim != 2 or radii.shape[1] not in ops.LUMEN_RAYS or cross.shape != radii.shape[:1] or sections.shape != (len(radii), 8):
        raise ValueError("lumen_profile: radii [R, K], cross [R] and sections [R, 8] expected, got %s %s %s"
                         % (radii.shape, cross.shape, sections.shape))
    s = result.get("oversample") if oversample is None else oversample
    at = result.get("arc") if arc is None else arc
    s = int(host(s).reshape(-1)[0]) if s is not None else 0
    pixel_mm = float(pixel_mm)
    if s < 1 or not (pixel_mm > 0 and math.isfinite(pixel_mm)):
        raise ValueError("lumen_profile: oversample >= 1 (in the result or given) and pixel_mm > 0 expected, got %r %r" % (s, pixel_mm))
    k = radii.shape[1]
    unit = pixel_mm / (256.0 * s)      # one unit of rho in mm
    area = 0.5 * math.sin(2.0 * math.pi / k) * cross.astype(np.float64) * unit * unit
    at = np.arange(len(radii), dtype=np.float64) if at is None else host(at).astype(np.float64)
    if at.shape != (len(radii),):
        raise ValueError("lumen_profile: arc [%d] expected, got %s" % (len(radii), at.shape))
    return {"area": area, "equivalent": 2.0 * np.sqrt(area / math.pi), "dmin": sections[:, 1] * unit, "dmax": sections[:, 2] * unit,
            "mean": sections[:, 0] * (2.0 * unit / k), "arc": at * pixel_mm,
            "valid": (sections[:, 5] == 0) & (sections[:, 6] == 0)}


def lumen_stenosis(profile, margin=5, reference=10, gap=5):
    """The stenosis grade of a `lumen_profile`: the valid section of least equivalent diameter at least `margin` sections from
    either end; the reference diameter and area are the mean of two medians, over the valid sections among the `reference` sections
    that lie more than `gap` sections proximal of it and among those distal of it (the windows are cut at the ends of the line).
    -> {"index", "diameter", "area": of the narrowest section; "reference_diameter", "reference_area"; "percent_diameter" = 100 (1 -
    d / d_ref), "percent_area" likewise; "proximal", "distal": the indices of the valid sections used}.  ValueError when no valid
    section lies inside the margins or a window holds no valid section.  The defaults are a first guess, not tuned on patient data."""
    who = "lumen_stenosis"
    margin, reference, gap = _int_in(who, "margin", margin, 0), _int_in(who, "reference", reference, 1), _int_in(who, "gap", gap, 0)
    eq, area, valid = (np.asarray(profile[k]) for k in ("equivalent", "area", "valid"))
    r = len(eq)
    inner = np.zeros(r, dtype=bool)
    inner[margin:r - margin if margin else r] = True
    cand = np.flatnonzero(valid & inner)
    if not len(cand):
        raise ValueError("%s: no valid section lies %d or more sections from the ends" % (who, margin))
    i = int(cand[np.argmin(eq[cand])])      # (the first on a tie)
    index = np.arange(r)
    prox = np.flatnonzero(valid & (index < i - gap) & (index >= i - gap - reference))
    dist = np.flatnonzero(valid & (index > i + gap) & (index <= i + gap + reference))
    if not len(prox) or not len(dist):
        raise ValueError("%s: the %s reference window of section %d holds no valid section" % (who, "distal" if len(prox) else "proximal", i))
    dref = 0.5 * (float(np.median(eq[prox])) + float(np.median(eq[dist])))
    aref = 0.5 * (float(np.median(area[prox])) + float(np.median(area[dist])))
    return {"index": i, "diameter": float(eq[i]), "area": float(area[i]), "reference_diameter": dref, "reference_area": aref,
            "percent_diameter": 100.0 * (1.0 - float(eq[i]) / dref), "percent_area": 100.0 * (1.0 - float(area[i]) / aref),
            "proximal": prox, "distal": dist}


class ResidentVolume(_SeriesView):
    """An int16 volume [n, h, w] kept on the device for the views that read all of it (`VolumeReformatter`, `VolumeRenderer`,
    `VolumeComponents`, `VolumeCentreline`, `VolumeLumen`): any number of them read one `ResidentVolume` (their `source=`).  `.volume`: the
    tensor, None until the first chunk; `.device`: None means the current device at the first chunk; `.seen`: how often every slice
    has arrived; `.nbytes` = 2 n h w.  `update(pix_chunk, n0)` copies a chunk in, in any order; `whole(who)` raises unless every
    slice has arrived exactly once since the last `reset()`, which forgets the arrivals and keeps the memory.  `adopt(tensor)`
    takes a finished volume -- a contiguous int16 [n, h, w] tensor on the device -- as it is, without a copy: every slice has then
    arrived once, and `reset()` lets go of it."""

    def __init__(self, n, h, w, device=None):
        self._volume(n, h, w)
        self.device = None if device is None else self._gpu(device)
        self.seen = np.zeros(self.n, dtype=np.int64)
        self.volume, self._adopted = None, False      # on the device from the first chunk on
        self.nbytes = 2 * self.n * self.h * self.w

    def reset(self):
        self.seen[:] = 0
        if self._adopted:
            self.volume, self._adopted = None, False

    def update(self, pix_chunk, n0, who=None):
        k, n0 = self._chunk(pix_chunk, n0, dtype=torch.int16, who=who), int(n0)      # (the copy below would convert another dtype)
        if k < 1:
            return
        if self.volume is None or self._adopted:      # (an adopted tensor is somebody's result: never written to)
            self.device = self._gpu(None) if self.device is None else self.device
            self.volume, self._adopted = torch.empty((self.n, self.h, self.w), dtype=torch.int16, device=self.device), False
        self.volume[n0:n0 + k].copy_(pix_chunk, non_blocking=True)
        self.seen[n0:n0 + k] += 1

    def adopt(self, tensor):
        if (not torch.is_tensor(tensor) or tensor.dtype != torch.int16 or tuple(tensor.shape) != (self.n, self.h, self.w)
                or not tensor.is_cuda or not tensor.is_contiguous() or self.device not in (None, torch.device("cuda"), tensor.device)):
            got = (tensor.dtype, tuple(tensor.shape), tensor.device, tensor.is_contiguous()) if torch.is_tensor(tensor) else tensor
            raise RuntimeError("ResidentVolume: adopt: a contiguous int16 tensor (%d, %d, %d) on %s expected, got %r"
                               % (self.n, self.h, self.w, self.device or "a GPU", got))
        self.volume, self.device, self._adopted = tensor, tensor.device, True
        self.seen[:] = 1

    def whole(self, who):
        if (self.seen != 1).any():
            missing, twice = int((self.seen == 0).sum()), int((self.seen > 1).sum())
            raise RuntimeError("%s: every slice must have arrived exactly once: %d of %d missing, %d more than once"
                               % (who, missing, self.n, twice))


class _VolumeView(_SeriesView):
    """What the views on the whole volume share: they read a `ResidentVolume`, `.source`.  source=None: the view makes its own
    and `update` feeds it; source= a `ResidentVolume` of the same (n, h, w): the view reads that one, whoever owns it feeds it,
    and `nbytes` leaves the volume out.  `.volume` and `.device` are the source's.  A subclass checks its sides with `_sides`, ends
    its constructor with `_reads`, uploads its tables in `_upload` (run once on `self.device`: at the first chunk of its own
    volume, else before the first launch) and calls `_whole` before it launches."""

    volume = property(lambda self: self.source.volume)
    device = property(lambda self: self.source.device)

    def _sides(self, who, n, h, w, linear=False):
        self._volume(n, h, w)
        if max(self.n, self.h, self.w) > ops.REFORMAT_MAX_DIM:      # the line tables address the sides in 16.16 fixed point
            raise ValueError("%s: n, h, w in 1 .. %d expected, got %d %d %d" % (who, ops.REFORMAT_MAX_DIM, self.n, self.h, self.w))
        if linear and self.n * self.h * self.w > 2 ** 31 - 1:      # the kernels address a voxel by an int32 linear index
            raise ValueError("%s: at most 2^31 - 1 voxels expected, got %d x %d x %d" % (who, self.n, self.h, self.w))

    def _shown(self, wc, ww, hu, level, fill):
        """The window of the 8-bit level, whether it is wanted, and what lies outside the volume: air by default, 0 or -1024 with `hu`."""
        self.hu, self.window, self.want_level = bool(hu), (float(wc), float(ww)), bool(level)
        self.fill = (-1024 if self.hu else 0) if fill is None else int(fill)

    def _reads(self, device, source):
        """The last step of a constructor (`self.nbytes` counts a volume of the view's own by then)."""
        self.owns, self._uploaded = source is None, False
        if self.owns:
            source = ResidentVolume(self.n, self.h, self.w, None if device is None else self._gpu(device))
        elif not isinstance(source, ResidentVolume) or (source.n, source.h, source.w) != (self.n, self.h, self.w):
            raise ValueError("%s: source: a ResidentVolume of (%d, %d, %d) expected, got %r"
                             % (type(self).__name__, self.n, self.h, self.w,
                                (source.n, source.h, source.w) if isinstance(source, ResidentVolume) else source))
        else:
            self.nbytes -= source.nbytes
        self.source = source

    def _line_tables(self, who, tables, cols):
        """`tables` of the constructor -> {name: (host table, U, T)}, checked on the host."""
        if not isinstance(tables, dict) or not tables:
            raise ValueError("%s: tables: a dict {name: (table, T)} with at least one entry expected" % who)
        lines = {}
        for name, entry in tables.items():
            entry = entry(self.n, self.h, self.w) if callable(entry) else entry
            u = getattr(entry, "cols", cols)
            if not isinstance(entry, tuple) or len(entry) != 2 or u is None:
                raise ValueError("%s: table %r: a LineSet, or a pair (table, T) together with cols, expected" % (who, name))
            lines[name] = (ops.line_table_host(entry[0], u, entry[1]), int(u), int(entry[1]))
        return lines

    def _upload(self):
        """The view's tables onto `self.device`."""

    def _uploaded_once(self):
        if not self._uploaded and self.device is not None:
            self._upload()
            self._uploaded = True

    def reset(self):
        if self.owns:
            self.source.reset()

    def update(self, pix_chunk, n0):
        if not self.owns:
            raise RuntimeError("%s: update: the volume is fed through its source" % type(self).__name__)
        self.source.update(pix_chunk, n0, who=type(self).__name__)
        self._uploaded_once()

    def _whole(self):
        self.source.whole(type(self).__name__)
        self._uploaded_once()

    def _reformat(self, table, mode, sampling):
        """One `ops.reformat_lines` launch on the volume, in the view's window."""
        values, level = ops.reformat_lines(self.volume, table, table.u, table.t, mode, fill=self.fill, wc=self.window[0], ww=self.window[1],
                                           hu=self.hu, sampling=sampling, want_level=self.want_level)
        return {"values": values, "level": level}

    def _lumen_options(self, who, band, options, aspect):
        """The lumen options of a constructor -> the dict with every default filled in, checked on the host as far as they can be
        before a line exists: the band, the launch's options, and the geometry on a stand-in line."""
        opts = {**LUMEN_DEFAULTS, **options}
        opts["lo"], opts["hi"] = band
        try:
            steps = lumen_lines(self.n, self.h, self.w, np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 1.0]]), aspect=aspect,
                                **{k: opts[k] for k in LUMEN_GEOMETRY}).steps
            ops.lumen_options(who, opts["rays"], steps, opts["lo"], opts["hi"], opts["sampling"], opts["edge"], opts["base"],
                              opts["recentre"])
        except RuntimeError as err:
            raise ValueError(str(err)) from None
        return opts

    def _lumen(self, lines, opts, table=None):
        """One `ops.lumen_sections` launch on the volume along the `LumenSet` lines -> the result tree of `VolumeLumen`."""
        table = ops.LineTable(lines[0], lines.rays, lines.steps, self.device) if table is None else table
        radii, cross, sections, centres = ops.lumen_sections(self.volume, table, lines.rays, lines.steps, opts["lo"], opts["hi"],
                                                             sampling=opts["sampling"], edge=opts["edge"], base=opts["base"],
                                                             recentre=opts["recentre"])
        return {"radii": radii, "cross": cross, "sections": sections, "centres": centres,
                "arc": torch.from_numpy(lines.arc).to(self.device),
                "oversample": torch.tensor([lines.oversample], dtype=torch.int32, device=self.device)}


class VolumeReformatter(_VolumeView):
    """Reformats of an int16 volume [n, h, w] that arrives in chunks and stays on the device: oblique planes, tumbling views, curved
    reformats -- every display whose rows cross slices (`ops.reformat_lines`, csrc/reformat.hip).  tables: {name: a `LineSet`, a
    pair (table [..., 9], T) with `cols` given here, or a callable (n, h, w) -> either}; mode "max" / "min" / "mean" along the rays
    of T steps, sampling "trilinear" or "nearest", `fill` where a ray misses the volume (default: air, 0 or -1024 with `hu`),
    level=False skips the 8-bit planes of the window (wc, ww).  The volume, `source=`, `update` and `reset` as `_VolumeView` has
    them; `result()` makes one launch per table -> {name: {"values": int16 [..., U], "level": uint8 or None}} on the
    device.  `.nbytes`: the device memory held (the volume, unless it is a source's, and the tables) plus that of one result, known
    before the first chunk.  Exact integer arithmetic on the current stream: equal to numpy bit for bit."""

    def __init__(self, n, h, w, tables, mode="max", sampling="trilinear", fill=None, wc=50.0, ww=400.0, hu=False, level=True,
                 device=None, cols=None, source=None):
        who = "VolumeReformatter"
        _one_of(who, "mode", mode, PROJECTIONS)
        _one_of(who, "sampling", sampling, REFORMAT_SAMPLINGS)
        self._sides(who, n, h, w)
        self.lines = self._line_tables(who, tables, cols)      # name -> (host table, U, T), checked
        self.mode, self.sampling = mode, sampling
        self._shown(wc, ww, hu, level, fill)
        per = 2 + (1 if self.want_level else 0)
        self.nbytes = 2 * self.n * self.h * self.w + sum(t.nbytes + per * (t.size // 9) * u for t, u, _ in self.lines.values())
        self.tables = None      # on the device from `_upload` on
        self._reads(device, source)

    def _upload(self):
        self.tables = {name: ops.LineTable(t, u, steps, self.device) for name, (t, u, steps) in self.lines.items()}

    def result(self):
        self._whole()
        return {name: self._reformat(table, self.mode, self.sampling) for name, table in self.tables.items()}


def reformat_volume(volume, tables, mode="max", sampling="trilinear", fill=None, wc=50.0, ww=400.0, hu=False, level=True, batch=64,
                    device=None, cols=None):
    """The reformats of a volume that already exists, the twin of `rotate_volume`: int16 [N, H, W], a host array / CPU tensor
    (chunks of `batch` slices cross PCIe one after another) or a device tensor (read where it is when it is contiguous); tables and
    the options as `VolumeReformatter`.  Returns what `VolumeReformatter.result` returns, of the input's kind."""
    return _view_of_volume("reformat_volume", volume, batch, device, whole=True,
                           make=lambda n, h, w, dev: VolumeReformatter(n, h, w, tables, mode=mode, sampling=sampling, fill=fill, wc=wc,
                                                                       ww=ww, hu=hu, level=level, device=dev, cols=cols))


def _ray_table(who, lines):
    """A `LineSet` / pair (table, T) or a bare table -> (int64 table [..., 9], T or None)."""
    steps = None
    if isinstance(lines, tuple):
        if len(lines) != 2:
            raise ValueError("%s: a LineSet, a pair (table, T) or a table [..., 9] expected" % who)
        lines, steps = lines[0], int(lines[1])
    table = np.asarray(lines.cpu() if torch.is_tensor(lines) else lines)
    if table.ndim < 1 or table.shape[-1] != 9 or table.dtype.kind not in "iu":
        raise ValueError("%s: a line table of [..., 9] integers expected, got %s %s" % (who, table.dtype, tuple(table.shape)))
    return table.astype(np.int64), steps


def headlight(lines, aspect=1.0):
    """The light that shines along the rays of a line table, for `ops.render_lines` / `ops.LightTable`: int64 [..., 3], for every
    line the unit vector of its ray -- (xk, yk, zk aspect), the step of the table in pixel units -- times 4096, rounded by
    floor(v + 0.5).  The length of the step drops out, so every oversample of one view gets the same light (within the rounding
    of the table's own coefficients).  lines: a `LineSet`, a pair (table, T) or a table [..., 9]; a table of T = 1 has no ray, and
    a line whose step is (0, 0, 0) no direction: both are refused.  The shading is two-sided, so the sign does not matter."""
    who = "headlight"
    table, steps = _ray_table(who, lines)
    aspect = float(aspect)
    if not (aspect > 0 and math.isfinite(aspect)):
        raise ValueError("%s: aspect: a positive ratio expected, got %r" % (who, aspect))
    if steps is not None and steps < 2:
        raise ValueError("%s: a table of T = %d has no ray: give the light as a vector" % (who, steps))
    ray = table[..., 2::3].astype(np.float64) * np.array([1.0, 1.0, aspect])
    length = np.sqrt((ray ** 2).sum(axis=-1, keepdims=True))
    if (length <= 0).any():
        raise ValueError("%s: %d of %d lines have no ray direction" % (who, int((length <= 0).sum()), length.size))
    return np.floor(ray / length * float(ops.LIGHT_UNIT) + 0.5).astype(np.int64)


def line_voxel(row, i, k):
    """(z, y, x): the voxel that sample (i, k) of a line falls in, by the kernel's nearest rule x = (x0 + xu i + xk k) >> 16
    (y, z likewise; arithmetic shift) for the line's row (x0, xu, xk, y0, yu, yk, z0, zu, zk) -- the `ray_voxel` of a line table.
    With k = the "depth" of sample i of a rendered line it is the voxel at which the ray's opacity reached `surface` (with
    trilinear sampling, the voxel the sample counts and is shaded by).  A pure host function; i and k may be integers or integer
    arrays, a ray that never got there (depth -1) has no voxel."""
    c = [int(v) for v in row]
    if len(c) != 9:
        raise ValueError("line_voxel: a row of nine integers expected, got %d" % len(c))
    i, k = np.asarray(i, dtype=np.int64), np.asarray(k, dtype=np.int64)
    x, y, z = ((c[3 * a] + c[3 * a + 1] * i + c[3 * a + 2] * k) >> 16 for a in range(3))
    return (int(z), int(y), int(x)) if x.ndim == 0 else (z, y, x)


SHADING_OPTIONS = ("ambient", "gmin", "light")
SHADING_DEFAULTS = {"ambient": 0.3, "gmin": 40.0, "light": "head"}      # a first guess, like the presets: not tuned


def _check_compositing(who, background, stop, surface):
    """-> ((r, g, b), stop, surface) of a compositing view, checked."""
    bg = tuple(background)
    if len(bg) != 3 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v <= 255 for v in bg):
        raise ValueError("%s: background: three integers in 0 .. 255 expected, got %r" % (who, background))
    return (tuple(int(v) for v in bg), _int_in(who, "stop", stop, 0, ops.RENDER_OPAQUE - 1),
            _int_in(who, "surface", surface, 1, ops.RENDER_OPAQUE))


class VolumeRenderer(_VolumeView):
    """Shaded volume-rendered views of an int16 volume [n, h, w] that arrives in chunks and stays on the device, along rays in any
    direction (`ops.render_lines`, csrc/render_lines.hip): the compositing of `SeriesRenderer` on the line tables of
    `VolumeReformatter` -- tumbling and oblique views, trilinear sampling, anisotropic voxels inside the geometry -- with every
    sample's colour shaded by the local gradient.  tables: {name: a `LineSet`, a pair (table, T) with `cols` given here, or a
    callable (n, h, w) -> either}; transfer, (wc, ww), hu, background, stop, surface and depth as `SeriesRenderer` (a preset name or
    a point list is made for one step per voxel: for oversampled tables pass `transfer_function(points, oversample)`); sampling
    "trilinear" or "nearest".  shading: None (flat class colours) or a dict with any of "ambient" (0 .. 1, default 0.3: the share of
    the colour a wall edge-on to the light keeps), "gmin" (default 40, in stored units per two voxels: a sample whose gradient is
    shorter keeps its colour, so that noise in soft tissue is not shaded) and "light" ("head", default: along every line's own ray,
    `headlight`; or one vector (x, y, z) in pixel units for all).  aspect (slice spacing / pixel spacing, the one the tables were
    made with) scales the gradient's z component, zscale = floor(256 / aspect + 0.5) in 1 .. 4096, and the headlight.  The volume,
    `source=`, `update` and `reset` as `_VolumeView` has them; `result()` makes one launch per table -> {name: {"rgb": uint8 [...,
    U, 3], "opacity": uint8 [..., U], "depth": int16 [..., U] or None (-1 where the ray never reaches `surface`; `line_voxel` maps a
    hit back to the voxel)}} on the device.  `.nbytes`: the device memory held (the volume, unless it is a source's, and the tables)
    plus that of one result, known before the first chunk.  Exact integer arithmetic on the current stream: equal to numpy bit for
    bit."""

    def __init__(self, n, h, w, tables, transfer="vessels", wc=300.0, ww=1500.0, hu=False, sampling="trilinear", shading=None,
                 aspect=1.0, background=(0, 0, 0), stop=128, surface=16384, depth=True, device=None, cols=None, source=None):
        who = "VolumeRenderer"
        _one_of(who, "sampling", sampling, REFORMAT_SAMPLINGS)
        self._sides(who, n, h, w)
        self.lines = self._line_tables(who, tables, cols)      # name -> (host table, U, T), checked
        self.sampling, self.hu, self.window, self.want_depth = sampling, bool(hu), (float(wc), float(ww)), bool(depth)
        self.background, self.stop, self.surface = _check_compositing(who, background, stop, surface)
        self.aspect = float(aspect)
        if not (self.aspect > 0 and math.isfinite(self.aspect)) or not 1 <= math.floor(256.0 / self.aspect + 0.5) <= ops.RENDER_ZSCALE_MAX:
            raise ValueError("%s: aspect: a ratio with floor(256 / aspect + 0.5) in 1 .. %d expected, got %r"
                             % (who, ops.RENDER_ZSCALE_MAX, aspect))
        self.zscale = int(math.floor(256.0 / self.aspect + 0.5))
        self.lights = None      # name -> host light table [L, 3], or None: no shading
        self.ambient, self.gmin2 = 256, 1
        if shading is not None:
            if not isinstance(shading, dict) or set(shading) - set(SHADING_OPTIONS):
                raise ValueError("%s: shading %r: None or a dict with any of %s expected" % (who, shading, SHADING_OPTIONS))
            opts = {**SHADING_DEFAULTS, **shading}
            ambient, gmin = float(opts["ambient"]), float(opts["gmin"])
            if not 0.0 <= ambient <= 1.0:
                raise ValueError("%s: shading: ambient in 0 .. 1 expected, got %r" % (who, opts["ambient"]))
            if not (gmin >= 0.0 and gmin * gmin <= ops.RENDER_GMIN2_MAX):
                raise ValueError("%s: shading: gmin in 0 .. %d expected, got %r" % (who, math.isqrt(ops.RENDER_GMIN2_MAX), opts["gmin"]))
            self.ambient = int(math.floor(ambient * 256.0 + 0.5))
            self.gmin2 = max(1, int(math.floor(gmin * gmin + 0.5)))
            self.lights = {}
            for name, (t, u, steps) in self.lines.items():
                if isinstance(opts["light"], str) and opts["light"] == "head":
                    vec = headlight((t, steps), self.aspect)
                else:
                    unit = np.floor(_unit(who, "light", opts["light"]) * float(ops.LIGHT_UNIT) + 0.5).astype(np.int64)
                    vec = np.broadcast_to(unit, t.shape[:-1] + (3,))
                self.lights[name] = ops.light_table_host(vec, t.size // 9)
        self.lut_host = np.asarray(_transfer_table(who, transfer, 1))
        per = 3 + 1 + (2 if self.want_depth else 0)
        self.nbytes = 2 * self.n * self.h * self.w + 2 * 4 * 256 + sum(
            t.nbytes + (12 * (t.size // 9) if self.lights is not None else 0) + per * (t.size // 9) * u for t, u, _ in self.lines.values())
        self.tables = self.lamps = self.lut = None      # on the device from `_upload` on
        self._reads(device, source)

    def _upload(self):
        self.tables = {name: ops.LineTable(t, u, steps, self.device) for name, (t, u, steps) in self.lines.items()}
        self.lut = ops.TransferTable(self.lut_host, self.device)
        if self.lights is not None:
            self.lamps = {name: ops.LightTable(v, len(v), self.device) for name, v in self.lights.items()}

    def result(self):
        self._whole()
        out = {}
        for name, table in self.tables.items():
            rgb, opacity, depth = ops.render_lines(
                self.volume, table, table.u, table.t, self.lut, light=None if self.lamps is None else self.lamps[name],
                zscale=self.zscale, ambient=self.ambient, gmin2=self.gmin2, sampling=self.sampling, background=self.background,
                stop=self.stop, surface=self.surface, wc=self.window[0], ww=self.window[1], hu=self.hu, want_depth=self.want_depth)
            out[name] = {"rgb": rgb, "opacity": opacity, "depth": depth}
        return out


def render_lines_volume(volume, tables, batch=64, device=None, **options):
    """The shaded renderings of a volume that already exists, the twin of `reformat_volume`: int16 [N, H, W], a host array / CPU
    tensor (chunks of `batch` slices cross PCIe one after another) or a device tensor (read where it is when it is contiguous);
    tables and the options as `VolumeRenderer`.  Returns what `VolumeRenderer.result` returns, of the input's kind."""
    return _view_of_volume("render_lines_volume", volume, batch, device, whole=True,
                           make=lambda n, h, w, dev: VolumeRenderer(n, h, w, tables, device=dev, **options))


COMPONENTS_OPTIONS = ("threshold", "connectivity", "min_voxels", "largest", "seeds", "background", "fill", "wc", "ww", "hu", "level",
                      "labels", "top")


def root_voxel(root, h, w):
    """(z, y, x) of a component's root, the linear index (z h + y) w + x that `VolumeComponents` labels it with (the smallest in
    the component: its first voxel in slice, row, column order).  A pure host function; root may be an integer or an integer
    array, a row (-1, 0) of "top" has no voxel."""
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError("root_voxel: h, w >= 1 expected, got %d %d" % (h, w))
    r = np.asarray(root, dtype=np.int64)
    if (r < 0).any():
        raise ValueError("root_voxel: a root is a linear index >= 0 (a (-1, 0) row of `top` stands for no component)")
    z, y, x = r // (h * w), (r // w) % h, r % w
    return (int(z), int(y), int(x)) if r.ndim == 0 else (z, y, x)


class VolumeComponents(_VolumeView):
    """The connected components of an int16 volume [n, h, w] that arrives in chunks and stays on the device, and the volume with
    only the wanted ones left (`ops.components_label` / `components_select` / `components_apply`, csrc/components.hip): despeckle,
    the K largest vessels, the vessel tree a click lies in.  threshold: lo, or (lo, hi) with hi = 32767 by default -- a voxel is
    foreground when lo <= value <= hi (stored values: HU differences for the subtraction volume); connectivity 6 / 18 / 26 in index
    space.  Kept are the components of at least `min_voxels` voxels that, where `seeds` (a sequence of (z, y, x), e.g. from
    `ray_voxel` / `line_voxel`) is given, hold a seed; of those the `largest` = K biggest (0: all; ties: the smaller root first).
    background=False masks: everything but the kept components becomes `fill` (default: air, 0 or -1024 with `hu`); background=True
    despeckles: only the dropped components do.  The volume, `source=`, `update` and `reset` as `_VolumeView` has them; `result()`
    -> {"values": int16 [n, h, w], "level": uint8 in the window (wc, ww) or None, "labels": int32 [n, h, w] (-1 on background,
    otherwise the component's root: its smallest linear index, `root_voxel`) or None, "top": int32 [top, 2] = (root, size) of the
    biggest kept components in order, (-1, 0) beyond them, "stats": int32 [8] = foreground voxels, components, candidates, kept
    components, kept voxels, seeds that selected nothing, the internal-error flag (whoever reads stats on the host raises unless it
    is 0: `check_components_stats`), 0} on the device.  `.nbytes`: the device memory held (the volume, unless it is a source's,
    labels, sizes, marks: 2 + 9 bytes per voxel) plus that of one result (2, or 3 with level, per voxel), known before the first
    chunk.  It never writes to the volume: "values" is a fresh tensor per result.  Exact integer arithmetic on the current stream:
    equal to numpy bit for bit, whatever order the atomics land in."""

    def __init__(self, n, h, w, threshold, connectivity=26, min_voxels=1, largest=0, seeds=None, background=False, fill=None,
                 wc=50.0, ww=400.0, hu=False, level=True, labels=False, top=8, device=None, source=None):
        who = "VolumeComponents"
        self._sides(who, n, h, w, linear=True)
        self.lo, self.hi = _band(who, threshold)
        _one_of(who, "connectivity", connectivity, ops.COMPONENTS_CONNECTIVITY)
        self.connectivity = int(connectivity)
        self.min_voxels = _int_in(who, "min_voxels", min_voxels, 1, 2 ** 31 - 1)
        self.largest, self.top = (_int_in(who, name, v, 0, ops.COMPONENTS_MAX_TOP) for name, v in (("largest", largest), ("top", top)))
        self.seeds_host = None if seeds is None else _voxel_indices(who, "seeds", seeds, self.n, self.h, self.w).astype(np.int32)
        self._shown(wc, ww, hu, level, fill)
        self.background, self.want_labels = bool(background), bool(labels)
        if not -32768 <= self.fill <= 32767:
            raise ValueError("%s: fill %d is not an int16 value" % (who, self.fill))
        v = self.n * self.h * self.w
        self.nbytes = (2 + 4 + 4 + 1) * v + (2 + (1 if self.want_level else 0)) * v + 4 * (8 + 2 * self.top) + \
            (0 if self.seeds_host is None else self.seeds_host.nbytes)
        self.seeds = self._labels = self._sizes = self._keep = None      # on the device from `_upload` / the first result on
        self._reads(device, source)

    def _upload(self):
        if self.seeds_host is not None:
            self.seeds = torch.from_numpy(self.seeds_host).to(self.device)

    def result(self):
        self._whole()
        # the labels a caller asked for are theirs: a fresh array per result; otherwise the working arrays are kept between calls
        labels, stats = ops.components_label(self.volume, self.lo, self.hi, self.connectivity,
                                             labels=None if self.want_labels else self._labels)
        self._sizes, self._keep, top = ops.components_select(labels, stats, min_voxels=self.min_voxels, seeds=self.seeds,
                                                             largest=self.largest, ntop=self.top, sizes=self._sizes, keep=self._keep)
        if not self.want_labels:
            self._labels = labels
        values, level = ops.components_apply(self.volume, labels, self._keep, background=self.background, fill=self.fill,
                                             wc=self.window[0], ww=self.window[1], hu=self.hu, want_level=self.want_level)
        return {"values": values, "level": level, "labels": labels if self.want_labels else None, "top": top, "stats": stats}


def check_components_stats(stats):
    """Raise unless the internal-error flag of a `VolumeComponents` result's "stats", read on the host, is 0."""
    flag = int(np.asarray(stats.cpu() if torch.is_tensor(stats) else stats).reshape(-1)[6])
    if flag != 0:
        raise RuntimeError("VolumeComponents: the labelling met a value that cannot be a parent (stats[6] = %d): the result is not "
                           "to be trusted" % flag)


def components_volume(volume, threshold, batch=64, device=None, **options):
    """The components view of a volume that already exists, the twin of `reformat_volume`: int16 [N, H, W], a host array / CPU
    tensor (chunks of `batch` slices cross PCIe one after another) or a device tensor (read where it is when it is contiguous);
    threshold and the options as `VolumeComponents`.  Returns what `VolumeComponents.result` returns, of the input's kind; a
    result that comes back to the host has had its error flag checked."""
    out = _view_of_volume("components_volume", volume, batch, device, whole=True,
                          make=lambda n, h, w, dev: VolumeComponents(n, h, w, threshold, device=dev, **options))
    if not torch.is_tensor(out["stats"]) or not out["stats"].is_cuda:
        check_components_stats(out["stats"])
    return out


CENTRELINE_OPTIONS = ("threshold", "start", "ends", "radius", "aspect", "penalty", "max_points", "smooth", "cpr", "clearance",
                      "rounds_per_call", "max_rounds", "fill", "wc", "ww", "hu", "level", "lumen")
CPR_OPTIONS = ("angles", "cols", "depth", "pitch", "sampling", "mode")
LUMEN_GEOMETRY = ("rays", "reach", "pitch", "oversample")      # the options of `lumen_lines` a view passes on (aspect is its own)
LUMEN_OPTIONS = ("threshold",) + LUMEN_GEOMETRY + ("sampling", "edge", "base", "recentre")
LUMEN_DEFAULTS = {"rays": 32, "reach": 16.0, "pitch": 1.0, "oversample": 2, "sampling": "trilinear", "edge": "band", "base": None,
                  "recentre": 0}


def centreline_penalty(radius, far=1, near=64):
    """The penalty table of `VolumeCentreline`, uint16 [radius^2 + 1], indexed by the capped squared clearance c: floor(far + (near -
    far) (1 - sqrt(c) / radius)^2 + 0.5), so a voxel `radius` or more from the wall costs `far` per unit step and one at the wall
    close to `near`; entry 0 (background, never read) = near.  far and near are integers in 1 .. 4095.  The defaults are a first
    guess, as the transfer presets were: not tuned on patient data."""
    r = int(radius)
    if isinstance(radius, bool) or r != radius or not 1 <= r <= ops.CENTRELINE_MAX_RADIUS:
        raise ValueError("centreline_penalty: radius: an integer in 1 .. %d expected, got %r" % (ops.CENTRELINE_MAX_RADIUS, radius))
    far, near = _int_in("centreline_penalty", "far", far, 1, 4095), _int_in("centreline_penalty", "near", near, 1, 4095)
    c = np.arange(r * r + 1, dtype=np.float64)
    pen = np.floor(far + (near - far) * (1.0 - np.sqrt(c) / r) ** 2 + 0.5)
    pen[0] = near
    return np.clip(pen, 1, 4095).astype(np.uint16)


def _centreline_aspect(who, aspect):
    """-> (aspect, zq = floor(256 aspect^2 + 0.5), which must lie in 16 .. 65535)."""
    aspect = float(aspect)
    if not (aspect > 0 and math.isfinite(aspect)) or not 16 <= math.floor(256.0 * aspect * aspect + 0.5) <= 65535:
        raise ValueError("%s: aspect: a ratio with floor(256 aspect^2 + 0.5) in 16 .. 65535 expected, got %r" % (who, aspect))
    return aspect, int(math.floor(256.0 * aspect * aspect + 0.5))


def centreline_steps(aspect=1.0):
    """The five step lengths of a move to a 26-neighbour, floor(10 sqrt(k + aspect^2 dz^2) + 0.5) for k in-plane axes: in-plane
    face, in-plane edge, z alone, z + one in-plane, z + two in-plane -- (10, 14, 10, 14, 17) at aspect 1.  Each must fit 1 .. 255."""
    aspect, _ = _centreline_aspect("centreline_steps", aspect)
    steps = tuple(int(math.floor(10.0 * math.sqrt(k + aspect * aspect * dz) + 0.5)) for k, dz in ((1, 0), (2, 0), (0, 1), (1, 1), (2, 1)))
    if not all(1 <= s <= 255 for s in steps):
        raise ValueError("centreline_steps: aspect %r gives step lengths %r outside 1 .. 255" % (aspect, steps))
    return steps


def smooth_centreline(points, window=5):
    """A centred moving average over `window` (odd, >= 1) points of a path float [M, 3], the end points repeated beyond the ends;
    float64, on the host.  The voxel path of a trace is a staircase, and `curved_lines` takes its tangents by central differences."""
    pts = np.asarray(points, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[1] != 3 or pts.shape[0] < 1:
        raise ValueError("smooth_centreline: points [M >= 1, 3] expected, got an array of shape %s" % (pts.shape,))
    if isinstance(window, bool) or not isinstance(window, (int, np.integer)) or window < 1 or window % 2 != 1:
        raise ValueError("smooth_centreline: window: an odd integer >= 1 expected, got %r" % (window,))
    half = int(window) // 2
    padded = np.concatenate([np.repeat(pts[:1], half, axis=0), pts, np.repeat(pts[-1:], half, axis=0)])
    total = np.cumsum(np.concatenate([np.zeros((1, 3)), padded]), axis=0)
    return (total[int(window):] - total[:-int(window)]) / float(window)


class VolumeCentreline(_VolumeView):
    """The vessel centreline from a start voxel to each of up to 64 end voxels of an int16 volume [n, h, w] that arrives in chunks
    and stays on the device (`ops.centreline_clearance` / `centreline_field` / `centreline_trace`, csrc/centreline.hip): the
    cheapest 26-connected path through the foreground when a move into a voxel costs its length times a penalty that falls with the
    voxel's distance from the vessel wall -- the path `curved_lines` wants.  threshold: lo, or (lo, hi), as `VolumeComponents`;
    start and ends: (z, y, x) voxels, e.g. from `ray_voxel` / `line_voxel` (a click is not snapped to the vessel: it must lie on
    foreground); radius R in 1 .. 32 caps the clearance (in pixels); aspect = slice spacing / pixel spacing scales z in the
    clearance and the step lengths (`centreline_steps`); penalty: a uint16 table [R^2 + 1] (default `centreline_penalty(R)`);
    max_points: the longest path in voxels (default 4 (n + h + w)); smooth: the window of `smooth_centreline`.  cpr = a dict with
    any of angles, cols, depth, pitch (as `curved_lines`), sampling, mode (as `VolumeReformatter`) adds the curved reformat along
    every end's smoothed path, one `ops.reformat_lines` launch per end on the resident volume, in the window (wc, ww) / `hu`;
    lumen = a dict with any of threshold (default: the centreline's own band), rays, reach, pitch, oversample, sampling, edge, base,
    recentre (as `VolumeLumen`) measures the lumen along every end's smoothed path, one `ops.lumen_sections` launch per end, and
    adds "lumen": one result tree of `VolumeLumen` per end; without it nothing of that is allocated or launched.  The
    volume, `source=`, `update` and `reset` as `_VolumeView` has them; `result()` -> {"paths": int32 [E, max_points] (linear
    indices, end first, -1 beyond the count), "counts": int32 [E], "points": a list of float64 [M, 3] (z, y, x), start to end,
    smoothed, "clearance": uint16 [n, h, w] (clearance=True) or None, "stats": int32 [8] (`ops.CENTRELINE_STATS`), and with cpr
    "cpr": [{"values": int16 [A, rows, cols], "level": uint8 or None}]} on the device.  It reads the counts on the host (one
    synchronisation beyond those of the relaxation) and raises ValueError for a start on background, an end on background or in
    another component, or a path longer than max_points, and RuntimeError when the field saturated or the error flag is
    set.  `.nbytes`: the device memory held (the volume, unless it is a source's, the scratch and the clearance at 2 bytes per
    voxel, the field at 4, the tables) plus paths and counts, known before the first chunk; the cpr planes are not in it (their rows
    follow the length of the path).  Exact integer arithmetic on the current stream up to the path; the smoothing is float64 on the
    host."""

    def __init__(self, n, h, w, threshold, start, ends, radius=8, aspect=1.0, penalty=None, max_points=None, smooth=5, cpr=None,
                 clearance=False, rounds_per_call=16, max_rounds=4096, fill=None, wc=50.0, ww=400.0, hu=False, level=True, device=None,
                 source=None, lumen=None):
        who = "VolumeCentreline"
        self._sides(who, n, h, w, linear=True)
        v = self.n * self.h * self.w
        self.lo, self.hi = _band(who, threshold)
        index = _voxel_indices(who, "start and ends", [tuple(start)] + [tuple(e) for e in ends], self.n, self.h, self.w, 2,
                               1 + ops.CENTRELINE_MAX_ENDS)
        self.start, self.ends_host = int(index[0]), index[1:].astype(np.int32)
        self.radius = _int_in(who, "radius", radius, 1, ops.CENTRELINE_MAX_RADIUS)
        self.rounds_per_call = _int_in(who, "rounds_per_call", rounds_per_call, 1, ops.CENTRELINE_MAX_ROUNDS)
        self.max_rounds = _int_in(who, "max_rounds", max_rounds, 1, ops.CENTRELINE_MAX_ROUNDS)
        self.aspect, self.zq = _centreline_aspect(who, aspect)
        self.steps = centreline_steps(self.aspect)
        pen = centreline_penalty(self.radius) if penalty is None else np.asarray(penalty)
        if pen.shape != (self.radius ** 2 + 1,) or pen.dtype.kind not in "iu" or (pen[1:] < 1).any() or (pen[1:] > 4095).any():
            raise ValueError("%s: penalty: %d integers in 1 .. 4095 expected" % (who, self.radius ** 2 + 1))
        self.pen_host = np.clip(pen, 1, 4095).astype(np.uint16)
        max_points = min(v, 4 * (self.n + self.h + self.w), ops.CENTRELINE_MAX_POINTS) if max_points is None else max_points
        self.max_points = _int_in(who, "max_points", max_points, 1, ops.CENTRELINE_MAX_POINTS)
        smooth_centreline(np.zeros((1, 3)), smooth)
        self.smooth = int(smooth)
        self.cpr = None
        if cpr is not None:
            if not isinstance(cpr, dict) or set(cpr) - set(CPR_OPTIONS):
                raise ValueError("%s: cpr %r: a dict with any of %s expected" % (who, cpr, CPR_OPTIONS))
            self.cpr = {"angles": (0.0,), "cols": 65, "depth": 1, "pitch": 1.0, "sampling": "trilinear", "mode": "max", **cpr}
            if self.cpr["mode"] not in PROJECTIONS or self.cpr["sampling"] not in REFORMAT_SAMPLINGS:
                raise ValueError("%s: cpr: mode one of %s and sampling one of %s expected" % (who, PROJECTIONS, REFORMAT_SAMPLINGS))
            curved_lines(self.n, self.h, self.w, np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 1.0]]), aspect=self.aspect,
                         **{k: self.cpr[k] for k in ("angles", "cols", "depth", "pitch")})      # (the options, checked now)
        self.lumen = None
        if lumen is not None:
            if not isinstance(lumen, dict) or set(lumen) - set(LUMEN_OPTIONS):
                raise ValueError("%s: lumen %r: a dict with any of %s expected" % (who, lumen, LUMEN_OPTIONS))
            band = _band(who, lumen["threshold"]) if "threshold" in lumen else (self.lo, self.hi)
            self.lumen = self._lumen_options(who, band, {k: v for k, v in lumen.items() if k != "threshold"}, self.aspect)
        self.want_clearance = bool(clearance)
        self._shown(wc, ww, hu, level, fill)
        tz, ty, tx = ops.CENTRELINE_TILE
        tiles = -(-self.n // tz) * -(-self.h // ty) * -(-self.w // tx)
        e = len(self.ends_host)
        self.nbytes = (2 + 2 + 2 + 4) * v + self.pen_host.nbytes + 4 * e + 8 * tiles + 4 * self.max_rounds + 4 * e * (self.max_points + 1) + 32
        self.pen = self.ends = self._scratch = self._clear = self._dist = None      # on the device from `_upload` / the first result on
        self._reads(device, source)

    def _upload(self):
        self.pen = torch.from_numpy(self.pen_host.view(np.int16)).to(self.device).view(torch.uint16)
        self.ends = torch.from_numpy(self.ends_host).to(self.device)

    def result(self):
        who = "VolumeCentreline"
        self._whole()
        # a clearance the caller asked for is theirs: a fresh array per result; otherwise the working arrays are kept between calls
        if self._scratch is None:
            self._scratch = torch.empty((self.n, self.h, self.w), dtype=torch.uint16, device=self.device)
        clear = ops.centreline_clearance(self.volume, self.lo, self.hi, self.radius, self.zq, scratch=self._scratch,
                                         clear=None if self.want_clearance else self._clear)
        if not self.want_clearance:
            self._clear = clear
        self._dist, stats = ops.centreline_field(clear, self.pen, self.steps, self.start, self.radius, rounds_per_call=self.rounds_per_call,
                                                 max_rounds=self.max_rounds, dist=self._dist)
        paths, counts = ops.centreline_trace(clear, self.pen, self.steps, self._dist, self.ends, self.radius, self.max_points, stats=stats)
        found, flags = counts.cpu().numpy(), stats.cpu().numpy()      # (the synchronisation: the points are made on the host)
        if flags[0] != 0:
            raise ValueError("%s: the start lies on background (threshold %d .. %d): a click is not snapped to the vessel" % (who, self.lo, self.hi))
        if flags[3] != 0 or flags[6] != 0:
            raise RuntimeError("%s: the cost field %s: the paths are not to be trusted"
                               % (who, "saturated (stats[3])" if flags[3] != 0 else "does not explain itself (stats[6])"))
        if (found == 0).any():
            raise ValueError("%s: %d of %d ends lie on background or in another component than the start" % (who, int((found == 0).sum()), len(found)))
        if (found < 0).any():
            raise ValueError("%s: a path is longer than max_points = %d voxels" % (who, self.max_points))
        points = []
        for e, m in enumerate(found.tolist()):
            i = paths[e, :m].cpu().numpy()[::-1].astype(np.int64)
            points.append(smooth_centreline(np.stack([i // (self.h * self.w), (i // self.w) % self.h, i % self.w], axis=1), self.smooth))
        out = {"paths": paths, "counts": counts, "points": [torch.from_numpy(p).to(self.device) for p in points],
               "clearance": clear if self.want_clearance else None, "stats": stats}
        if self.cpr is not None:
            out["cpr"] = []
            for p in points:
                if len(p) < 2:
                    raise ValueError("%s: cpr: an end is the start itself: there is no line to reformat along" % who)
                lines = curved_lines(self.n, self.h, self.w, p, aspect=self.aspect, **{k: self.cpr[k] for k in ("angles", "cols", "depth", "pitch")})
                out["cpr"].append(self._reformat(ops.LineTable(lines[0], lines.cols, lines[1], self.device), self.cpr["mode"],
                                                 self.cpr["sampling"]))
        if self.lumen is not None:
            out["lumen"] = []
            for p in points:
                if len(p) < 2:
                    raise ValueError("%s: lumen: an end is the start itself: there is no line to measure along" % who)
                out["lumen"].append(self._lumen(lumen_lines(self.n, self.h, self.w, p, aspect=self.aspect,
                                                            **{k: self.lumen[k] for k in LUMEN_GEOMETRY}), self.lumen))
        return out


def centreline_volume(volume, threshold, start, ends, batch=64, device=None, **options):
    """The centreline view of a volume that already exists, the twin of `components_volume`: int16 [N, H, W], a host array / CPU
    tensor (chunks of `batch` slices cross PCIe one after another) or a device tensor (read where it is when it is contiguous);
    threshold, start, ends and the options as `VolumeCentreline`.  Returns what `VolumeCentreline.result` returns, of the input's
    kind."""
    return _view_of_volume("centreline_volume", volume, batch, device, whole=True,
                           make=lambda n, h, w, dev: VolumeCentreline(n, h, w, threshold, start, ends, device=dev, **options))


class VolumeLumen(_VolumeView):
    """The lumen profile along a centreline of an int16 volume [n, h, w] that arrives in chunks and stays on the device
    (`ops.lumen_sections`, csrc/lumen.hip): at every position of the line the lumen's radius along a fan of rays across it, from
    which `lumen_profile` takes area and diameters and `lumen_stenosis` the grade.  threshold: lo, or (lo, hi), the lumen's band of
    stored values as `VolumeComponents` has it; points: the centreline, float [M >= 2, 3] in (z, y, x) voxel order (a path of
    `VolumeCentreline`, smoothed); rays, reach, pitch, oversample, aspect as `lumen_lines`; sampling "trilinear" or "nearest";
    edge "band" (the wall is where the value leaves the band) or "half" with `base` <= lo (the wall is half-way between the
    section's own centre value and the background `base`, never below lo); recentre 0 .. 4: moves of every section's centre to the
    middle of its own boundary before the measurement that counts.  The volume, `source=`, `update` and `reset` as `_VolumeView` has
    them; `result()` makes one launch -> {"radii": int32 [R, rays] in 1 / (256 oversample) pixel, "cross": int64 [R], "sections":
    int32 [R, 8] (`ops.LUMEN_SECTIONS`), "centres": int32 [R, 3] = (x, y, z) in 16.16, "arc": float64 [R] in pixels, "oversample":
    int32 [1]} on the device: what `lumen_profile` takes.  A branch, a gap or the edge of the volume shows as open rays: such a section
    is not valid.  `.lines`: the `LumenSet`.  `.nbytes`: the device memory held (the volume, unless it is a source's, and the table)
    plus that of one result, known before the first chunk.  Exact integer arithmetic on the current stream: equal to numpy bit for
    bit."""

    def __init__(self, n, h, w, threshold, points, rays=32, reach=16.0, pitch=1.0, oversample=2, aspect=1.0, sampling="trilinear",
                 edge="band", base=None, recentre=0, device=None, source=None):
        who = "VolumeLumen"
        self._sides(who, n, h, w)
        self.options = self._lumen_options(who, _band(who, threshold), {"rays": rays, "reach": reach, "pitch": pitch,
                                                                         "oversample": oversample, "sampling": sampling, "edge": edge,
                                                                         "base": base, "recentre": recentre}, aspect)
        self.lines = lumen_lines(self.n, self.h, self.w, points, rays=rays, reach=reach, pitch=pitch, oversample=oversample, aspect=aspect)
        try:
            self.table_host = ops.lumen_table_host(self.lines[0], self.lines.rays, self.lines.steps, self.options["recentre"])
        except RuntimeError as err:
            raise ValueError("%s: %s" % (who, err)) from None
        sections = len(self.lines.arc)
        self.nbytes = 2 * self.n * self.h * self.w + self.table_host.nbytes + sections * (4 * self.lines.rays + 8 + 32 + 12 + 8) + 4
        self.table = None      # on the device from `_upload` on
        self._reads(device, source)

    def _upload(self):
        self.table = ops.LineTable(self.table_host, self.lines.rays, self.lines.steps, self.device)

    def result(self):
        self._whole()
        return self._lumen(self.lines, self.options, self.table)


def lumen_volume(volume, threshold, points, batch=64, device=None, **options):
    """The lumen view of a volume that already exists, the twin of `centreline_volume`: int16 [N, H, W], a host array / CPU tensor
    (chunks of `batch` slices cross PCIe one after another) or a device tensor (read where it is when it is contiguous); threshold,
    points and the options as `VolumeLumen`.  Returns what `VolumeLumen.result` returns, of the input's kind."""
    return _view_of_volume("lumen_volume", volume, batch, device, whole=True,
                           make=lambda n, h, w, dev: VolumeLumen(n, h, w, threshold, points, device=dev, **options))


def subtract_volume(cta, ct_hu, cta_is_hu=False, median=True, floor=0, ct_range=(None, None), wc=150.0, ww=300.0, level=True,
                    batch=64, device=None):
    """The subtraction of two volumes that already exist (a real CTA and its registered CT for a side-by-side view, or a
    synthesized volume written earlier): int16 [N, H, W] each, of one kind -- host arrays / CPU tensors (chunks of `batch`
    slices cross PCIe one after another) or device tensors.  Arguments as `ops.subtract_slices`.  Returns {"sub": int16
    [N, H, W], "level": uint8 or None} of the input's kind.  The median is in-plane, so chunking does not change a bit."""
    is_np = isinstance(cta, np.ndarray)
    if is_np != isinstance(ct_hu, np.ndarray):
        raise RuntimeError("subtract_volume: cta and ct_hu of one kind expected (both arrays or both tensors)")
    a = torch.from_numpy(np.ascontiguousarray(cta)) if is_np else cta
    c = torch.from_numpy(np.ascontiguousarray(ct_hu)) if is_np else ct_hu
    for t in (a, c):
        if not torch.is_tensor(t) or t.dtype != torch.int16 or t.dim() != 3:
            raise RuntimeError("subtract_volume: int16 volumes [N, H, W] expected")
    if a.shape != c.shape or a.is_cuda != c.is_cuda:
        raise RuntimeError("subtract_volume: cta %s and ct_hu %s differ in shape or place" % (tuple(a.shape), tuple(c.shape)))
    if int(batch) < 1:
        raise ValueError("subtract_volume: batch >= 1 expected")
    on_host = not a.is_cuda
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    dev = dev if on_host else a.device
    if dev.type != "cuda":
        raise RuntimeError("subtract_volume: a GPU device is required (no CPU fallback)")
    n = a.shape[0]
    sub = torch.empty(a.shape, dtype=torch.int16, device=dev)
    lvl = torch.empty(a.shape, dtype=torch.uint8, device=dev) if level else None
    with torch.cuda.device(dev):
        for s, e, _ in plan_chunks(n, batch):
            xa, xc = (a[s:e].to(dev), c[s:e].to(dev)) if on_host else (a[s:e].contiguous(), c[s:e].contiguous())
            ds, dl = ops.subtract_slices(xa, xc, cta_is_hu=cta_is_hu, median=median, floor=floor, ct_range=ct_range, wc=wc, ww=ww,
                                         want_level=level)
            sub[s:e].copy_(ds)
            if lvl is not None:
                lvl[s:e].copy_(dl)
    if not on_host:
        return {"sub": sub, "level": lvl}
    conv = (lambda t: t.cpu().numpy()) if is_np else (lambda t: t.cpu())
    return {"sub": conv(sub), "level": None if lvl is None else conv(lvl)}


PROJECT_SOURCES = ("cta", "sub", "vessels")
COMPONENTS_SOURCES = ("cta", "sub")
REFORMAT_OPTIONS = ("mode", "sampling", "fill", "cols")
RENDER_OPTIONS = ("transfer", "detector", "wc", "ww", "hu", "sampling", "oversample", "background", "stop", "surface", "depth")
RENDER3D_OPTIONS = ("transfer", "wc", "ww", "hu", "sampling", "shading", "aspect", "background", "stop", "surface", "depth", "cols")


def _option_dict(name, value, allowed, required=(), needs=None):
    """A dict option of `SeriesTranslator`, checked -> a copy of it ({} for None): every key of `required` and none outside
    `allowed`.  needs = (what the options go with, that thing, what it is made of): options without the thing are refused, and
    so is a thing with nothing in it."""
    opts = dict(value or {})
    if needs is not None and needs[1] is None:
        if opts:
            raise ValueError("SeriesTranslator: %s need %s" % (name, needs[0]))
    elif needs is not None and not needs[1]:
        raise ValueError("SeriesTranslator: %s needs at least one %s" % (needs[0], needs[2]))
    elif not set(required) <= set(opts) or set(opts) - set(allowed):
        raise ValueError("SeriesTranslator: %s %r: a dict with %sany of %s expected"
                         % (name, value, "".join("%r, " % key for key in required), tuple(allowed)))
    return opts


# What `SeriesTranslator` knows of a display that is on: make(n, h, w) -> its view; result(view) -> its tree; angles: the output
# gains the view's "angles"; reads: None for a view fed chunk by chunk, else the source ("cta", "sub", "vessels") whose
# `ResidentVolume` a view on the whole volume reads; first: its result is made before the others', and its "values" are the
# source "vessels" where a display reads that; check: what the finished tree is put through once it is on the host.
_Display = collections.namedtuple("_Display", "make result angles reads first check", defaults=(False, None, False, None))


def _angle_list(rotate):
    """`rotate` of SeriesTranslator / `angles` of rotate_volume: an int count of views around the full circle, or degrees."""
    if isinstance(rotate, (int, np.integer)) and not isinstance(rotate, bool):
        return view_angles(int(rotate))
    return [float(a) for a in rotate]


class SeriesTranslator:
    """`SeriesTranslator(generator)(volume)`: int16 HU volume [N, H, W] (numpy array or CPU tensor, SimpleITK convention) -> {"pix":
    int16 [N, H, W], "level": uint8 [N, H, W] or None}, of the input's kind.  project = "max" / "min" / "mean" (slab: slices per
    axial slab, None: the whole volume) adds "projections": {axis: {"values": int16, "level": uint8 or None}} of the synthesized
    volume (`SeriesProjector`), in the translator's own window and `hu` (their level whatever `level` says).
    rotate = an int count of views around the full circle, or a sequence of degrees (rotate_mode: "max" / "min" / "mean", default
    `project` or "max"; rotate_sampling "nearest" / "bilinear" and rotate_oversample = steps per voxel, as `SeriesRotator`) adds
    "rotation": {"values": int16 [A, N, D], "level": uint8, "angles": float64 [A]}.
    subtract=True adds "sub" (int16 [N, H, W]: synthesized minus input, `ops.subtract_slices` with sub_median, sub_floor,
    sub_ct_range) and "sub_level" (uint8 in sub_window = (wc, ww) of a HU difference, None with level=False).
    project_source="sub" (needs subtract=True) projects and rotates the subtraction volume instead of the synthesized one, its
    levels in sub_window with hu=True: the bone-free MIP.
    slabs = a dict of `SeriesSlabs` keyword arguments (thick, and any of step, mode, axes) adds "slabs": {axis: {"values": int16 [J,
    ...], "level": uint8}}, the sliding thin-slab projections of the same source in the same window, copied back once after the last
    chunk.
    depth=True (depth_cue: 0 .. 256) applies to whichever of `project` / `rotate` is on, with mode "max" / "min": their dicts gain
    "depth" (int16) and "cued" (uint8, the depth-cued level), as `SeriesProjector` / `SeriesRotator` give them, staged back with the
    other planes; the slabs have no depth planes.
    render = an int count of views around the full circle, or a sequence of degrees (render_options: a dict of `SeriesRenderer`
    keyword arguments -- transfer, detector, wc, ww, hu (default: that of the source), sampling, oversample, background, stop,
    surface, depth) adds "render": {"rgb": uint8 [A, N, D, 3], "opacity": uint8, "depth": int16 (unless depth=False), "angles":
    float64 [A]}, the volume-rendered views of the same source (`project_source`), copied back once after the last chunk.
    reformat = {name: a `LineSet`, a pair (table, T), or a callable (n, h, w) -> either} (reformat_options: a dict with any of mode,
    sampling, fill, cols, as `VolumeReformatter`) adds "reformat": {name: {"values": int16 [..., U], "level": uint8}}: oblique
    planes, tumbling views and curved reformats of the same source (`project_source`, so "sub" gives bone-free reformats in
    sub_window).  Their rows cross slices, so every table is one launch on the whole volume after the last chunk, and the planes are
    copied back once.
    render3d = tables as `reformat` (render3d_options: a dict of `VolumeRenderer` keyword arguments -- transfer, wc, ww, hu
    (default: that of the source), sampling, shading, aspect, background, stop, surface, depth, cols) adds "render3d": {name:
    {"rgb": uint8 [..., U, 3], "opacity": uint8, "depth": int16 or None}}: the shaded volume-rendered views of the same source
    (`project_source`) along rays in any direction, one launch per table after the last chunk, copied back once.
    components = a dict of `VolumeComponents` keyword arguments (threshold, and any of connectivity, min_voxels, largest, seeds,
    background, fill, wc, ww, hu, level, labels, top) adds "vessels": {"values": int16 [N, H, W], "level": uint8 or None, "labels":
    int32 or None, "top": int32 [top, 2], "stats": int32 [8]}, the volume of components_source ("cta" or "sub", which needs
    subtract=True; default: what `project_source` shows, "cta" for "vessels") with only the wanted connected components left, in
    that source's window and `hu`, labelled after the last chunk and copied back once; a stats[6] other than 0 raises.
    project_source="vessels" (needs components) makes every other display show that cleaned volume: the chunk loop then feeds only
    the components' source, and after the last chunk the views on the whole volume read the cleaned tensor where it is and the
    others get its slices in chunks of `batch`.
    centreline = a dict of `VolumeCentreline` keyword arguments (threshold, start, ends, and any of radius, aspect, penalty,
    max_points, smooth, cpr, clearance, rounds_per_call, max_rounds, fill, wc, ww, hu, level, lumen) adds "centreline": {"paths", "counts",
    "points": a list of float64 [M, 3], "clearance", "stats", with cpr "cpr": [{"values", "level"}], and with lumen "lumen": [the
    tree of `VolumeLumen` per end, for `lumen_profile` / `lumen_stenosis`]}, the vessel centreline from
    `start` to every end through the same source as the other displays (`project_source`), traced after the last chunk and copied
    back once; it waits for the relaxation on the host.
    reformat, render3d, components and centreline read the whole volume, which stays on the device: one `ResidentVolume` per source
    that any of them reads (2 N H W bytes, fed once per chunk), beside what each view holds itself (its `.nbytes`).
    A display that is off (None; depth=False, subtract=False) allocates and launches nothing.

    size: the side(s) the generator runs at (None: the volume's own); a volume of another size is resized (nearest) on the way
    in and comes back at its own size.  wc / ww: the window of the 8-bit level; hu: pixels minus 1024 (SimpleITK) instead of
    the reference's stored values; level=False skips the 8-bit plane.  Runs in whatever compute mode is set, on the current
    stream, outside any captured graph."""

    def __init__(self, generator, batch=16, size=None, wc=50.0, ww=400.0, hu=False, level=True, device=None, project=None,
                 slab=None, rotate=None, rotate_mode=None, subtract=False, sub_median=True, sub_floor=0, sub_ct_range=(None, None),
                 sub_window=(150.0, 300.0), project_source="cta", slabs=None, rotate_sampling="nearest", rotate_oversample=1,
                 depth=False, depth_cue=0, render=None, render_options=None, reformat=None, reformat_options=None, render3d=None,
                 render3d_options=None, components=None, components_source=None, centreline=None):
        if int(batch) < 1:
            raise ValueError("SeriesTranslator: batch >= 1 expected")
        self.centreline = centreline if centreline is None else _option_dict("centreline", centreline, CENTRELINE_OPTIONS,
                                                                             ("threshold", "start", "ends"))
        self.components = components if components is None else _option_dict("components", components, COMPONENTS_OPTIONS, ("threshold",))
        if self.components is None and components_source is not None:
            raise ValueError("SeriesTranslator: components_source needs components")
        if project_source == "vessels" and self.components is None:
            raise ValueError("SeriesTranslator: project_source 'vessels' needs components")
        if components_source is None:
            components_source = "cta" if project_source not in COMPONENTS_SOURCES else project_source
        if components_source not in COMPONENTS_SOURCES or (self.components is not None and components_source == "sub" and not subtract):
            raise ValueError("SeriesTranslator: components_source %r: one of %s expected, and 'sub' needs subtract=True"
                             % (components_source, COMPONENTS_SOURCES))
        self.components_source = components_source
        self.render3d = None if render3d is None else dict(render3d)
        self.render3d_options = _option_dict("render3d_options", render3d_options, RENDER3D_OPTIONS, needs=("render3d", self.render3d, "table"))
        self.reformat = None if reformat is None else dict(reformat)
        self.reformat_options = _option_dict("reformat_options", reformat_options, REFORMAT_OPTIONS, needs=("reformat", self.reformat, "table"))
        self.render = None if render is None else _angle_list(render)
        self.render_options = _option_dict("render_options", render_options, RENDER_OPTIONS, needs=("render", self.render, "angle"))
        if project_source not in PROJECT_SOURCES or (project_source == "sub" and not subtract):
            raise ValueError("SeriesTranslator: project_source %r: one of %s expected, and 'sub' needs subtract=True"
                             % (project_source, PROJECT_SOURCES))
        self.subtract, self.project_source = bool(subtract), project_source
        self.sub_median, self.sub_floor, self.sub_ct_range = bool(sub_median), sub_floor, tuple(sub_ct_range)
        self.sub_window = (float(sub_window[0]), float(sub_window[1]))
        if project is not None and project not in PROJECTIONS:
            raise ValueError("SeriesTranslator: project %r is not one of %s" % (project, PROJECTIONS))
        self.project, self.slab = project, slab
        self.rotate = None if rotate is None else _angle_list(rotate)
        self.rotate_mode = rotate_mode or project or "max"
        if self.rotate is not None and (self.rotate_mode not in PROJECTIONS or not self.rotate):
            raise ValueError("SeriesTranslator: rotate needs at least one angle and a rotate_mode of %s, got %r"
                             % (PROJECTIONS, self.rotate_mode))
        _check_sampling("SeriesTranslator", rotate_sampling, rotate_oversample)
        self.depth, self.depth_cue = _check_depth("SeriesTranslator", depth, depth_cue, "max")
        if self.depth and project is None and self.rotate is None:
            raise ValueError("SeriesTranslator: depth=True needs project or rotate")
        for mode in ([project] if project is not None else []) + ([self.rotate_mode] if self.rotate is not None else []):
            _check_depth("SeriesTranslator", self.depth, self.depth_cue, mode)
        self.rotate_sampling, self.rotate_oversample = rotate_sampling, int(rotate_oversample)
        self.slabs = slabs if slabs is None else _option_dict("slabs", slabs, ("thick", "step", "mode", "axes"), ("thick",))
        self.window = (float(wc), float(ww))
        self.generator = generator
        self.batch = int(batch)
        self.size = None if size is None else _pair(size)
        self.hu, self.level = bool(hu), bool(level)
        if device is None:
            p = next(generator.parameters(), None)
            device = p.device if p is not None and p.is_cuda else torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("SeriesTranslator: a GPU device is required (no CPU fallback)")
        self.wc = torch.full((self.batch,), float(wc), dtype=torch.float32, device=self.device)
        self.ww = torch.full((self.batch,), float(ww), dtype=torch.float32, device=self.device)
        self.h2d = torch.cuda.Stream(device=self.device)
        self.d2h = torch.cuda.Stream(device=self.device)
        self._hw = None
        self._in = self._out = None
        # the planes a chunk brings back, by output key: the dtype, or None for a plane that is off and keeps its key
        self._planes = {"pix": torch.int16, "level": torch.uint8 if self.level else None}
        if self.subtract:
            self._planes.update(sub=torch.int16, sub_level=torch.uint8 if self.level else None)
        # the displays that are on, by output key (`_Display`); a view on the whole volume reads the resident volume of its source
        dev, src, shown = self.device, self.project_source, self._shows(self.project_source)
        self._displays = {}
        if self.project is not None:
            self._displays["projections"] = _Display(
                lambda n, h, w: SeriesProjector(n, h, w, mode=self.project, slab=self.slab, device=dev, depth=self.depth, cue=self.depth_cue),
                lambda view: view.result(shown["wc"], shown["ww"], hu=shown["hu"]))
        if self.rotate is not None:
            self._displays["rotation"] = _Display(
                lambda n, h, w: SeriesRotator(n, h, w, self.rotate, mode=self.rotate_mode, **shown, device=dev, sampling=self.rotate_sampling,
                                              oversample=self.rotate_oversample, depth=self.depth, cue=self.depth_cue),
                SeriesRotator.result, angles=True)
        if self.slabs is not None:
            self._displays["slabs"] = _Display(lambda n, h, w: SeriesSlabs(n, h, w, **shown, device=dev, **self.slabs), SeriesSlabs.result)
        if self.render is not None:
            self._displays["render"] = _Display(
                lambda n, h, w: SeriesRenderer(n, h, w, self.render, device=dev, **{"hu": shown["hu"], **self.render_options}),
                SeriesRenderer.result, angles=True)
        if self.reformat is not None:
            self._displays["reformat"] = _Display(
                lambda n, h, w, **source: VolumeReformatter(n, h, w, self.reformat, **shown, **self.reformat_options, **source),
                VolumeReformatter.result, reads=src)
        if self.render3d is not None:
            self._displays["render3d"] = _Display(
                lambda n, h, w, **source: VolumeRenderer(n, h, w, self.render3d, **{"hu": shown["hu"], **self.render3d_options}, **source),
                VolumeRenderer.result, reads=src)
        if self.components is not None:      # (in the window of its own source, which is what the others show with "vessels")
            self._displays["vessels"] = _Display(
                lambda n, h, w, **source: VolumeComponents(n, h, w, **{**self._shows(self.components_source), **self.components}, **source),
                VolumeComponents.result, reads=self.components_source, first=True,
                check=lambda tree: check_components_stats(tree["stats"]))      # (on the host by then: no extra synchronisation)
        if self.centreline is not None:
            self._displays["centreline"] = _Display(
                lambda n, h, w, **source: VolumeCentreline(n, h, w, **{**shown, **self.centreline}, **source),
                VolumeCentreline.result, reads=src)
        # by output key: the view, the page-locked copy of its result; by source: the resident volume of the views that read it
        self._views, self._view_host, self._residents = {}, {}, {}
        # host seconds of the last call (scripts/export_bench.py): waiting to get a slot back, copying into the input slots,
        # copying out of the output slots, the whole call
        self.stats = {"wait": 0.0, "stage_in": 0.0, "stage_out": 0.0, "total": 0.0}

    def _stage(self, h, w):
        """The page-locked slots for planes of h x w (kept between calls on volumes of one size): one input plane and one dict
        of the output planes that are on per slot."""
        if self._hw != (h, w):
            shape = (self.batch, h, w)
            self._in = [torch.empty(shape, dtype=torch.int16, pin_memory=True) for _ in range(SLOTS)]
            self._out = [{key: torch.empty(shape, dtype=dtype, pin_memory=True) for key, dtype in self._planes.items() if dtype is not None}
                         for _ in range(SLOTS)]
            self._hw = (h, w)

    def __call__(self, volume):
        is_np = isinstance(volume, np.ndarray)
        vol = torch.from_numpy(np.ascontiguousarray(volume)) if is_np else volume
        if not torch.is_tensor(vol) or vol.is_cuda or vol.dtype != torch.int16 or vol.dim() != 3:
            raise RuntimeError("SeriesTranslator: an int16 volume [N, H, W] on the host (numpy array or CPU tensor) expected")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("SeriesTranslator: runs outside a captured graph (it waits on events from the host)")
        clock = time.perf_counter
        stats = self.stats = {"wait": 0.0, "stage_in": 0.0, "stage_out": 0.0, "total": 0.0}
        t_call = clock()
        vol = vol.contiguous()
        n, h, w = vol.shape
        gsize = self.size or (h, w)
        out = {key: None if dtype is None else torch.empty((n, h, w), dtype=dtype) for key, dtype in self._planes.items()}
        if n == 0:
            return _tree_to(out, (lambda t: t.numpy()) if is_np else (lambda t: t))
        self._stage(h, w)
        with torch.cuda.device(self.device):
            cur = torch.cuda.current_stream()
            residents = {d.reads: self._kept(self._residents, d.reads, n, h, w, lambda: ResidentVolume(n, h, w, self.device))
                         for d in self._displays.values() if d.reads is not None}
            views = {key: self._kept(self._views, key, n, h, w, lambda: d.make(
                n, h, w, **({} if d.reads is None else {"source": residents[d.reads]}))) for key, d in self._displays.items()}
            streaming = [view for key, view in views.items() if self._displays[key].reads is None]
            in_free = [None] * SLOTS       # event: the slot's H2D copy has drained, the host may rewrite it
            pending = [None] * SLOTS       # (event, start, stop): the slot's D2H copy, not yet moved into the result

            def drain(slot):
                if pending[slot] is None:
                    return
                ev, s, e = pending[slot]
                t0 = clock()
                ev.synchronize()
                t1 = clock()
                for key, buf in self._out[slot].items():
                    out[key][s:e].copy_(buf[:e - s])
                pending[slot] = None
                stats["wait"] += t1 - t0
                stats["stage_out"] += clock() - t1

            for s, e, slot in plan_chunks(n, self.batch):
                k = e - s
                t0 = clock()
                if in_free[slot] is not None:
                    in_free[slot].synchronize()      # two chunks ago: long finished in steady state
                t1 = clock()
                self._in[slot][:k].copy_(vol[s:e])
                stats["wait"] += t1 - t0
                stats["stage_in"] += clock() - t1
                arrived = torch.cuda.Event()
                with torch.cuda.stream(self.h2d):
                    dev_hu = self._in[slot][:k].to(self.device, non_blocking=True)
                    arrived.record()
                in_free[slot] = arrived
                cur.wait_event(arrived)
                dev_hu.record_stream(cur)            # allocated on the copy stream, consumed on this one
                with torch.no_grad():
                    x = ops.series_inputs(dev_hu, gsize).unsqueeze(1)
                    fake = self.generator(x)
                    planes = {}
                    planes["pix"], planes["level"] = ops.export_slices(fake, self.wc[:k], self.ww[:k], size=(h, w), hu=self.hu,
                                                                       want_level=self.level)
                    if self.subtract:
                        planes["sub"], planes["sub_level"] = ops.subtract_slices(
                            planes["pix"], dev_hu, cta_is_hu=self.hu, median=self.sub_median, floor=self.sub_floor,
                            ct_range=self.sub_ct_range, wc=self.sub_window[0], ww=self.sub_window[1], want_level=self.level)
                    # a source feeds its resident volume once, whatever number of views read it ("vessels" comes after the last chunk)
                    sources = {"cta": planes["pix"], "sub": planes.get("sub")}
                    for name, resident in residents.items():
                        if name in sources:
                            resident.update(sources[name], s)
                    if self.project_source in sources:
                        for view in streaming:
                            view.update(sources[self.project_source], s)
                computed = torch.cuda.Event()
                computed.record(cur)
                drain(slot)                          # the chunk that used this slot last: its D2H started two chunks ago
                done = torch.cuda.Event()
                with torch.cuda.stream(self.d2h):
                    self.d2h.wait_event(computed)
                    for key, buf in self._out[slot].items():
                        buf[:k].copy_(planes[key], non_blocking=True)
                        planes[key].record_stream(self.d2h)
                    done.record()
                pending[slot] = (done, s, e)
            # one copy back per display, after the last chunk: the finished planes are staged here, before the last slots are
            # drained, so that the copies run while the host drains (the reformats are one launch per table first: the whole
            # volume is on the device now).  An event per display: the host clones one display's planes while the next one's
            # are still being copied.
            staged = {}
            trees = {key: self._displays[key].result(view) for key, view in views.items() if self._displays[key].first}
            if self.project_source == "vessels":
                # the cleaned volume: the views on the whole volume read it where it is, the others get its slices in their chunks
                cleaned, = (tree["values"] for tree in trees.values())
                if "vessels" in residents:
                    residents["vessels"].adopt(cleaned)
                with torch.no_grad():
                    for s, e, _ in plan_chunks(n, self.batch):
                        for view in streaming:
                            view.update(cleaned[s:e], s)
            for key, view in views.items():
                tree = trees[key] if key in trees else self._displays[key].result(view)
                host, copied = self._stage_view(key, tree), torch.cuda.Event()
                copied.record(cur)
                staged[key] = (host, copied)
            for slot in sorted(range(SLOTS), key=lambda q: pending[q][1] if pending[q] else -1):
                drain(slot)
            shown = {}
            for key, (host, copied) in staged.items():
                t0 = clock()
                copied.synchronize()
                stats["wait"] += clock() - t0
                shown[key] = _tree_to(host, (lambda t: t.clone().numpy()) if is_np else (lambda t: t.clone()))
                if self._displays[key].check is not None:
                    self._displays[key].check(shown[key])
                if self._displays[key].angles:
                    angles = views[key].angles
                    shown[key]["angles"] = np.array(angles, dtype=np.float64) if is_np else torch.tensor(angles, dtype=torch.float64)
        # the forwards above ran fused conv + InstanceNorm launches: none may have given up (raises)
        ops.nie_check("series inference")
        stats["total"] = clock() - t_call
        out = _tree_to(out, (lambda t: t.numpy()) if is_np else (lambda t: t))
        out.update(shown)
        return out

    @staticmethod
    def _kept(kept, key, n, h, w, make):
        """`kept[key]`, a view or a resident volume, for an (n, h, w) volume: kept between calls on volumes of one shape (and reset
        for the next), else made anew."""
        item = kept.get(key)
        if item is None or (item.n, item.h, item.w) != (n, h, w):
            item = kept[key] = make()
        else:
            item.reset()
        return item

    def _stage_view(self, key, tree):
        """Start the copies of a view's finished result into page-locked buffers, one per tensor of the tree (kept between calls
        while every tensor's place, shape and dtype stay as they are).  A view's device "angles" are not staged: the output's are
        made from the view's host list."""
        if self._displays[key].angles:
            tree = {k: t for k, t in tree.items() if k != "angles"}
        dev, host = _tree_leaves(tree), self._view_host.get(key)
        if host is None or [(p, t.shape, t.dtype) for p, t in _tree_leaves(host)] != [(p, t.shape, t.dtype) for p, t in dev]:
            host = self._view_host[key] = _tree_to(tree, lambda t: torch.empty(t.shape, dtype=t.dtype, pin_memory=True))
        for (_, buf), (_, t) in zip(_tree_leaves(host), dev):
            buf.copy_(t, non_blocking=True)
        return host

    def _shows(self, source):
        """The window and `hu` of a display of `source`.  The subtraction has a window of its own, and its values are HU
        differences: 0 is the window's zero, whatever convention the synthesized pixels use.  The cleaned volume "vessels" is shown
        as the components' own source is."""
        source = self.components_source if source == "vessels" else source
        wc, ww = self.sub_window if source == "sub" else self.window
        return {"wc": wc, "ww": ww, "hu": True if source == "sub" else self.hu}
