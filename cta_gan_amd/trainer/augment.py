"""The training augmentation of the reference's loaders on the device (`noise_level`).

Every training loader of the reference applies, per image and before `Resize` (trainer/HdTrainer.py:130-142,641-653,
CycTrainer.py:91-99, p2pTrainer.py:81-89, RegTrainer.py:122-132; trainer/datasets.py:103-119,218-232):

    level = config['noise_level']
    RandomAffine(degrees=level, translate=[0.02*level, 0.02*level], scale=[1-0.02*level, 1+0.02*level], fillcolor=-1)

on a float ('F' mode) PIL image -- the misalignment the registration network exists to correct.  torchvision's PIL path ends
in `Image.transform(size, AFFINE, inverse matrix, NEAREST, fillcolor)`, and for a rotated float image PIL runs its 16.16
fixed-point loop: integer arithmetic on six coefficients.  The host part is here -- parameter draws, the inverse matrix in
float64, PIL's `FIX` rounding --, the gather is csrc/augment.hip (`ops.affine_nearest`, `ops.hu_affine_inputs`), which
reproduces PIL's pixels bit for bit (tests/golden/affine_*.npz hold PIL's own output).
"""
from __future__ import annotations

import math
import random

import torch

from .. import dp, ops

IMAGE_KEYS = ("A1", "A2", "B1", "B2", "A", "B")     # draw order inside one sample
HU_KEYS = {"hu_A": ("A1", "A2"), "hu_B": ("B1", "B2")}   # raw int16 HU planes -> (windowed, full-range) image keys
_SERIES = {"A2": "A1", "B2": "B1"}                 # shared_per_series: the second image of a slice reuses the first's draw


def inverse_matrix(center, angle, translate, scale):
    """torchvision's `_get_inverse_affine_matrix` without shear: the six float64 entries of the map output pixel -> source
    position that `Image.transform(AFFINE)` takes, for a rotation by `angle` degrees about `center` = (cx, cy), a scaling by
    `scale` and a translation by `translate` = (tx, ty)."""
    cx, cy = center
    tx, ty = translate
    r = math.radians(angle)
    c, s = math.cos(r) / scale, math.sin(r) / scale
    m = [c, s, 0.0, -s, c, 0.0]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty) + cx
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty) + cy
    return m


def _fix(v):
    return int(math.floor(v * 65536.0 + 0.5))


def fixed_coefficients(m, size=None):
    """PIL's 16.16 fixed-point coefficients (A0 .. A5) of the inverse matrix `m` (Geometry.c `affine_fixed`: FIX(v) =
    floor(v * 65536 + 0.5), the half-pixel centre folded into A2 / A5); source pixel of (y, x): ((A2 + A1 y + A0 x) >> 16,
    (A5 + A4 y + A3 x) >> 16).  With `size` = (H, W) of the image, raises where that sum can leave 32 bits: PIL's own `int`
    arithmetic is undefined there, so there is nothing to agree with."""
    a = [_fix(m[0]), _fix(m[1]), _fix(m[2] + m[0] * 0.5 + m[1] * 0.5),
         _fix(m[3]), _fix(m[4]), _fix(m[5] + m[3] * 0.5 + m[4] * 0.5)]
    h, w = (1, 1) if size is None else (int(size[0]), int(size[1]))
    for row in (a[0:3], a[3:6]):
        if abs(row[2]) + abs(row[1]) * (h - 1) + abs(row[0]) * (w - 1) >= 2 ** 31:
            raise OverflowError("affine coefficients %r leave 32-bit fixed point on a %d x %d image" % (row, h, w))
    return a


def _upload(table, device):
    """A list of 6-int rows -> int32 (n, 6) on `device` through a page-locked buffer, asynchronously on the current stream (the
    caching host allocator keeps the buffer alive until that copy has drained)."""
    host = torch.empty((len(table), 6), dtype=torch.int32, pin_memory=True)
    host.copy_(torch.tensor(table, dtype=torch.int32))
    return host.to(device, non_blocking=True)


class RandomAffine:
    """`transforms.RandomAffine` as the reference calls it, for device tensors: (H, W), (1, H, W) or (B, 1, H, W) fp32 on the
    GPU, every plane with a draw of its own.  Nearest resampling without shear only (`resample` / `shear` other than
    False / None / 0 raise NotImplementedError).

    The draws come from the instance's OWN `random.Random(seed)` -- Python's global `random`, which drives `ReplayBuffer`,
    is never touched -- in this order per plane: angle = uniform(-d, d), tx = round(uniform(-t0 W, t0 W)),
    ty = round(uniform(-t1 H, t1 H)), scale = uniform(s0, s1); `translate=None` / `scale=None` draw nothing and give 0 / 1.
    An angle of exactly 0 runs the same fixed-point gather, where PIL would switch to its axis-aligned scaling path; under
    a continuous draw that has probability zero."""

    def __init__(self, degrees, translate=None, scale=None, shear=None, resample=False, fillcolor=0, seed=None):
        if shear not in (None, 0, 0.0, (0, 0), [0, 0]):
            raise NotImplementedError("RandomAffine: shear is not part of this build")
        if resample not in (False, None, 0):
            raise NotImplementedError("RandomAffine: only nearest resampling (resample=False) is part of this build")
        if isinstance(degrees, (int, float)):
            if degrees < 0:
                raise ValueError("If degrees is a single number, it must be positive.")
            self.degrees = (-degrees, degrees)
        else:
            assert len(degrees) == 2, "degrees should be a list or tuple and it must be of length 2."
            self.degrees = tuple(degrees)
        if translate is not None:
            assert len(translate) == 2, "translate should be a list or tuple and it must be of length 2."
            for t in translate:
                if not 0.0 <= t <= 1.0:
                    raise ValueError("translation values should be between 0 and 1")
        self.translate = translate
        if scale is not None:
            assert len(scale) == 2, "scale should be a list or tuple and it must be of length 2."
            for s in scale:
                if s <= 0:
                    raise ValueError("scale values should be positive")
        self.scale = scale
        self.fillcolor = fillcolor
        self.rng = random.Random(seed)

    def get_params(self, img_w, img_h):
        """One draw: (angle, (tx, ty), scale) for an image of img_w x img_h pixels."""
        angle = self.rng.uniform(self.degrees[0], self.degrees[1])
        if self.translate is not None:
            max_dx, max_dy = self.translate[0] * img_w, self.translate[1] * img_h
            translations = (round(self.rng.uniform(-max_dx, max_dx)), round(self.rng.uniform(-max_dy, max_dy)))
        else:
            translations = (0, 0)
        scale = self.rng.uniform(self.scale[0], self.scale[1]) if self.scale is not None else 1.0
        return angle, translations, scale

    def coefficients(self, img_w, img_h, params=None):
        """The six fixed-point ints of one draw (`params`: a draw made earlier) for an img_w x img_h image."""
        angle, translations, scale = params if params is not None else self.get_params(img_w, img_h)
        m = inverse_matrix((img_w * 0.5, img_h * 0.5), angle, translations, scale)
        return fixed_coefficients(m, (img_h, img_w))

    def __call__(self, img):
        if not torch.is_tensor(img) or img.dim() not in (2, 3, 4) or (img.dim() > 2 and img.shape[-3] != 1):
            raise ValueError("RandomAffine: a (H, W), (1, H, W) or (B, 1, H, W) tensor expected")
        if not img.is_cuda:
            raise RuntimeError("RandomAffine: CPU tensors are not supported (no CPU fallback)")
        h, w = img.shape[-2:]
        table = [self.coefficients(w, h) for _ in range(img.numel() // (h * w))]
        return ops.affine_nearest(img, _upload(table, img.device), (h, w), self.fillcolor)


class NoiseAugmenter:
    """The reference's `noise_level` transform chain `[RandomAffine(level ...), Resize(size)]` on a dict batch of device tensors:
    every image key present (A1, A2, B1, B2, A, B; (B, 1, H, W) fp32) comes back as (B, 1, size, size) fp32, other entries pass
    through.  Raw batches carry `hu_A` / `hu_B` int16 HU planes instead and come back with A1, A2 / B1, B2 (`read_ori_w` fused
    into the same gather: `ops.hu_affine_inputs`).

    Draws: for each sample in batch order, one independent draw per image key in the order A1, A2, B1, B2, A, B -- as in
    trainer/datasets.py:218-232, where the windowed and the full-range image of one slice get different parameters.
    `shared_per_series=True` (an extension) gives A1 / A2 one draw and B1 / B2 one draw.  The generator is
    `random.Random(seed + dp.rank())`; Python's global `random` is not touched.

    Launches: one coefficient upload and one gather per distinct source size (all keys of that size stacked), on the current
    stream -- `DataPrefetcher(transform=...)` makes that the copy stream.  `level == 0` draws and launches nothing: the batch
    is returned as it came (resized where its size differs; raw HU converted).  An angle of exactly 0 at level > 0 has
    probability zero and runs the same kernel (see `RandomAffine`)."""

    def __init__(self, level, size, seed=0, shared_per_series=False):
        self.level = level or 0
        if self.level < 0:
            raise ValueError("noise_level must be >= 0")
        self.size = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
        self.shared_per_series = bool(shared_per_series)
        self.affine = None
        if self.level > 0:
            lv = self.level
            self.affine = RandomAffine(degrees=lv, translate=[0.02 * lv, 0.02 * lv], scale=[1 - 0.02 * lv, 1 + 0.02 * lv],
                                       fillcolor=-1, seed=seed + dp.rank())

    def sample(self, shapes):
        """Host only.  shapes: image key -> (B, H, W) of the planes to warp.  Returns key -> list of B coefficient rows, drawn
        in the documented order."""
        out = {k: [] for k in shapes}
        keys = [k for k in IMAGE_KEYS if k in shapes]
        for i in range(max((shapes[k][0] for k in keys), default=0)):
            drawn = {}
            for k in keys:
                b, h, w = shapes[k]
                if i >= b:
                    continue
                first = _SERIES.get(k)
                if self.shared_per_series and first in drawn:
                    params = drawn[first]
                else:
                    params = self.affine.get_params(w, h)
                drawn[k] = params
                out[k].append(self.affine.coefficients(w, h, params))
        return out

    def _plain(self, batch):
        """level 0: no draw; only what the loader's remaining transforms do (read_ori_w of raw planes, Resize)."""
        out = None
        for k, v in batch.items():
            if k in HU_KEYS:
                out = dict(batch) if out is None else out
                del out[k]
                for kk, img in zip(HU_KEYS[k], ops.hu_to_inputs(v.reshape(v.shape[0], 1, *v.shape[-2:]))):
                    out[kk] = img if tuple(img.shape[-2:]) == self.size else ops.resize_nearest(img, self.size)
            elif k in IMAGE_KEYS and torch.is_tensor(v) and tuple(v.shape[-2:]) != self.size:
                out = dict(batch) if out is None else out
                out[k] = ops.resize_nearest(v, self.size)
        return batch if out is None else out

    def __call__(self, batch):
        if self.level == 0:
            return self._plain(batch)
        shapes = {}
        for k, v in batch.items():
            if k in HU_KEYS:
                for kk in HU_KEYS[k]:
                    shapes[kk] = (v.shape[0], v.shape[-2], v.shape[-1])
            elif k in IMAGE_KEYS and torch.is_tensor(v):
                shapes[k] = (v.shape[0], v.shape[-2], v.shape[-1])
        coef = self.sample(shapes)
        out = {k: v for k, v in batch.items() if k not in HU_KEYS}
        fill = self.affine.fillcolor
        for hk, (k_win, k_full) in HU_KEYS.items():
            if hk not in batch:
                continue
            hu = batch[hk]
            b = hu.shape[0]
            table = [row for i in range(b) for row in (coef[k_win][i], coef[k_full][i])]
            win, full = ops.hu_affine_inputs(hu.reshape(b, 1, *hu.shape[-2:]), _upload(table, hu.device), self.size, fill=fill)
            out[k_win], out[k_full] = win, full
        groups = {}      # source size -> image keys, in draw order
        for k in IMAGE_KEYS:
            if k in batch and torch.is_tensor(batch[k]):
                groups.setdefault(tuple(batch[k].shape[-2:]), []).append(k)
        for (h, w), keys in groups.items():
            planes = [batch[k].reshape(-1, h, w) for k in keys]
            src = planes[0] if len(planes) == 1 else torch.cat(planes, 0)
            table = [row for k in keys for row in coef[k]]
            warped = ops.affine_nearest(src, _upload(table, src.device), self.size, fill)
            at = 0
            for k, p in zip(keys, planes):
                out[k] = warped[at:at + p.shape[0]].reshape(p.shape[0], 1, *self.size)
                at += p.shape[0]
        return out
