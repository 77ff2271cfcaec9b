"""Regenerate tests/golden/affine_*.npz: PIL's own output for the `noise_level` augmentation (trainer/augment.py).

    python scripts/make_golden_affine.py

Needs Pillow (and numpy); no GPU, no network, nothing of the reference.  Each case runs what torchvision's
RandomAffine(degrees=level, translate=[0.02*level]*2, scale=[1-0.02*level, 1+0.02*level], fillcolor=-1) runs on a float image:
`Image.fromarray(img, 'F').transform(size, AFFINE, inverse matrix, NEAREST, fillcolor=-1)`.  The parameter draw and the
inverse matrix are restated HERE, not imported from the package, so the fixtures check the package instead of echoing it;
the six fixed-point ints are stored beside PIL's pixels, which are the only judge of them.

  affine_<name>.npz      img (H, W) f32, params (angle, tx, ty, scale) f64, matrix (6) f64, coef (6) i64, out (H, W) f32
  affine_hu_<name>.npz   hu (H, W) i16 raw HU; params / matrix / coef with a leading axis 2 (windowed, full-range image);
                         win / full (H, W) f32 = PIL on oracle.ref_inputs.read_ori_w_arith(hu)
Image values are distinct multiples of 2^-13 above -1 (every pixel identifies its source; the files compress).
"""
import math
import os
import random
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FILL = -1.0

# name, (H, W), level, seed
CASES = [("5x7_l1", (5, 7), 1, 11), ("5x7_l5", (5, 7), 5, 12),
         ("37x53_l1", (37, 53), 1, 21), ("37x53_l2", (37, 53), 2, 22), ("37x53_l5", (37, 53), 5, 23),
         ("64x48_l1", (64, 48), 1, 31), ("64x48_l5", (64, 48), 5, 32),
         ("128x96_l5", (128, 96), 5, 41)]
HU_CASE = ("37x53_l2", (37, 53), 2, 51)


def draw(rng, level, h, w):
    angle = rng.uniform(-level, level)
    tx = round(rng.uniform(-0.02 * level * w, 0.02 * level * w))
    ty = round(rng.uniform(-0.02 * level * h, 0.02 * level * h))
    scale = rng.uniform(1 - 0.02 * level, 1 + 0.02 * level)
    return angle, tx, ty, scale


def matrix_of(angle, tx, ty, scale, h, w):
    cx, cy = w * 0.5, h * 0.5
    r = math.radians(angle)
    c, s = math.cos(r) / scale, math.sin(r) / scale
    m = [c, s, 0.0, -s, c, 0.0]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty) + cx
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty) + cy
    return m


def fixed_of(m):
    fix = lambda v: int(math.floor(v * 65536.0 + 0.5))      # noqa: E731  (Geometry.c: FIX)
    return [fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5)]


def pil_affine(img, m):
    h, w = img.shape
    out = Image.fromarray(img, "F").transform((w, h), Image.Transform.AFFINE, m, Image.Resampling.NEAREST, fillcolor=FILL)
    return np.asarray(out, dtype=np.float32).copy()


def image(h, w, seed):
    idx = np.random.RandomState(seed).permutation(h * w).reshape(h, w)
    return ((idx + 1 - 8192) / 8192.0).astype(np.float32)      # distinct, exact in float32, none equal to the fill


def main():
    total = 0
    for name, (h, w), level, seed in CASES:
        rng = random.Random(seed)
        p = draw(rng, level, h, w)
        m = matrix_of(*p, h, w)
        img = image(h, w, seed)
        path = os.path.join(GOLD, "affine_%s.npz" % name)
        np.savez_compressed(path, img=img, params=np.array(p, dtype=np.float64), matrix=np.array(m, dtype=np.float64),
                            coef=np.array(fixed_of(m), dtype=np.int64), out=pil_affine(img, m))
        total += os.path.getsize(path)
    sys.path.insert(0, ROOT)
    from oracle.ref_inputs import read_ori_w_arith
    name, (h, w), level, seed = HU_CASE
    rng = random.Random(seed)
    hu = np.random.RandomState(seed).randint(-1100, 1500, size=(h, w)).astype(np.int16)
    i1, i2 = read_ori_w_arith(hu.copy())
    ps = [draw(rng, level, h, w), draw(rng, level, h, w)]      # the windowed image's draw, then the full-range image's
    ms = [matrix_of(*p, h, w) for p in ps]
    path = os.path.join(GOLD, "affine_hu_%s.npz" % name)
    np.savez_compressed(path, hu=hu, params=np.array(ps, dtype=np.float64), matrix=np.array(ms, dtype=np.float64),
                        coef=np.array([fixed_of(m) for m in ms], dtype=np.int64),
                        win=pil_affine(i1.astype(np.float32), ms[0]), full=pil_affine(i2.astype(np.float32), ms[1]))
    total += os.path.getsize(path)
    print("wrote %d files, %d bytes" % (len(CASES) + 1, total))


if __name__ == "__main__":
    main()
