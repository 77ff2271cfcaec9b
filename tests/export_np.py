"""numpy restatement (test infrastructure only) of the per-pixel arithmetic behind csrc/export.hip and csrc/window_arith.h:

  pix_np      ((x + 1) * 0.5 * 4095).astype(int16) in float32, one rounding per operation, truncated toward zero
              (trainer/HdTrainer.py:539-543); hu: minus 1024
  level_np    the 8-bit window level to_windowdata (HdTrainer.py:41-61) holds before its rescale, `== 0 -> -2000` included
  window_np   level -> [-1, 1] (:62-63): to_windowdata's value
Pinned against the reference's own functions by tests/golden/export_*.npz (scripts/make_golden_export.py)."""
import numpy as np

F = np.float32


def stored_np(x):
    x = np.asarray(x, dtype=F)
    return ((x + F(1)) * F(0.5)) * F(4095)


def pix_np(x, hu=False):
    q = np.trunc(stored_np(x)).astype(np.int32)
    return (q - 1024 if hu else q).astype(np.int16)


def win_params_np(wc, ww):
    wc, ww = float(wc), float(ww)
    win_min = (2 * wc - ww) / 2.0 + 0.5
    win_max = (2 * wc + ww) / 2.0 + 0.5
    return F(win_min), F(255.0 / (win_max - win_min))


def level_np(x, wc, ww):
    wmin, dfac = win_params_np(wc, ww)
    t = stored_np(x)
    t = np.where(t == 0, F(-2000), t)
    t = t - F(1024)
    t = t - wmin
    t = np.trunc(t * dfac)
    assert t.dtype == F
    return np.clip(t, 0, 255).astype(np.uint8)


def window_np(level):
    t = level.astype(F) / F(255)
    return (t - F(0.5)) / F(0.5)
