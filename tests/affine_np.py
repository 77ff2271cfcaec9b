"""numpy restatement (test infrastructure only) of the two formulas behind csrc/augment.hip:

  pil_affine_fixed   PIL's Image.transform(size, AFFINE, m, NEAREST, fillcolor) on a float image with a rotated matrix: the
                     16.16 fixed-point loop of Geometry.c, from its six ints
  resize_index       the source index of F.interpolate(mode='nearest') (trainer/utils.py:13-32), as resize_nearest_kernel
                     computes it in float32
Pinned against PIL itself by tests/golden/affine_*.npz (scripts/make_golden_affine.py)."""
import numpy as np


def source_index(coef, h, w):
    """(ys, xs, inside) int64 / bool arrays of shape (h, w): the source pixel PIL reads for every output pixel."""
    a0, a1, a2, a3, a4, a5 = (int(v) for v in coef)
    y = np.arange(h, dtype=np.int64)[:, None]
    x = np.arange(w, dtype=np.int64)[None, :]
    xs = (a2 + a1 * y + a0 * x) >> 16
    ys = (a5 + a4 * y + a3 * x) >> 16
    return ys, xs, (xs >= 0) & (xs < w) & (ys >= 0) & (ys < h)


def pil_affine_fixed(img, coef, fill):
    h, w = img.shape
    ys, xs, inside = source_index(coef, h, w)
    out = np.full((h, w), fill, dtype=img.dtype)
    out[inside] = img[ys[inside], xs[inside]]
    return out


def resize_index(n_out, n_in):
    scale = np.float32(n_in) / np.float32(n_out)
    i = np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64)
    return np.minimum(i, n_in - 1)


def resize_nearest(img, size):
    return img[resize_index(size[0], img.shape[0])[:, None], resize_index(size[1], img.shape[1])[None, :]]


def affine_resize(img, coef, fill, size):
    """What ops.affine_nearest(img, coef, size, fill) must return for one plane."""
    return resize_nearest(pil_affine_fixed(img, coef, fill), size)


def moved_share(coef, h, w):
    """Share of the output pixels that read a source pixel other than their own (outside pixels count as moved)."""
    ys, xs, inside = source_index(coef, h, w)
    same = inside & (ys == np.arange(h)[:, None]) & (xs == np.arange(w)[None, :])
    return 1.0 - same.mean()
