"""Regenerate tests/golden/export_*.npz: what the reference's test() loop stores for a generator output (run where the
reference is available; the fixtures hold input and output arrays only).

    python scripts/make_golden_export.py

  pix    the int16 line of trainer/HdTrainer.py:539-543, stated here in numpy: ((x + 1) * 0.5 * 4095).astype(np.int16) on float32
  win    the reference's own to_windowdata(x, WC, WW) (:41-64), loaded by oracle.make_golden_metrics.load_reference_functions
  level  the 8-bit level behind `win`: rint((win + 1) / 2 * 255); the script asserts that (float32(level) / 255 - 0.5) / 0.5 in
         float32 gives `win` back bit for bit, so `level` IS the value to_windowdata held before its rescale

Random planes do not pin this arithmetic (a handful of pixels in 10^5 tell the correct operation order from a fused
multiply-add or a float64 evaluation), so the inputs are the boundary values themselves, each with its +-1 and +-2 ulp float32
neighbours, clipped to [-1, 1], plus -1, nextafter(-1, 0) and 1:
  pix    k / 2047.5 - 1, k = 0 .. 4095                                                   (where the truncation steps)
  level  (m / dFactor + win_min + 1024) / 2047.5 - 1, m = 0 .. 256, for each of WINDOWS    (where the level steps)
The script prints how many of them a float64 evaluation, a fused multiply-add and rounding instead of truncation would get wrong.

  export_87x87.npz   B = 3, odd H W (planes 1 and 2 start misaligned): every pix value + the first window's level values
  export_64x48.npz   B = 4, one window per slice: each plane holds its window's level values
  export_5x7.npz     B = 3, too small for a 16-byte store: a sample of all of them
Each file: x (B, H, W) f32, wc / ww (B) f32, pix (B, H, W) i16, win (B, H, W) f32, level (B, H, W) u8.  Values are shuffled
with a fixed seed; spare pixels repeat values of the same set.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
WINDOWS = [(50.0, 400.0), (40.0, 400.0), (60.0, 300.0), (300.0, 1500.0)]


def with_neighbours(x64):
    """float32(x) and its +-1, +-2 ulp neighbours, clipped to [-1, 1], + the three fixed points."""
    x = np.asarray(x64, dtype=np.float64).astype(np.float32)
    up1 = np.nextafter(x, np.float32(2)); up2 = np.nextafter(up1, np.float32(2))
    dn1 = np.nextafter(x, np.float32(-2)); dn2 = np.nextafter(dn1, np.float32(-2))
    v = np.clip(np.stack([dn2, dn1, x, up1, up2], 1).reshape(-1), np.float32(-1), np.float32(1))
    fixed = np.array([-1.0, np.nextafter(np.float32(-1), np.float32(0)), 1.0], dtype=np.float32)
    return np.concatenate([v, fixed]).astype(np.float32)


def pix_values():
    return with_neighbours(np.arange(4096, dtype=np.float64) / 2047.5 - 1.0)


def level_values(wc, ww):
    win_min = (2 * wc - ww) / 2.0 + 0.5
    win_max = (2 * wc + ww) / 2.0 + 0.5
    dfac = 255.0 / (win_max - win_min)
    m = np.arange(257, dtype=np.float64)
    return with_neighbours((m / dfac + win_min + 1024.0) / 2047.5 - 1.0)


def ref_pix(x):
    newimg = (x + 1) * 0.5 * 4095      # float32 array, python scalars: float32 arithmetic, one rounding per operation
    assert newimg.dtype == np.float32
    return newimg.astype(np.int16)


def planes(values, b, h, w, rng):
    """(b, h, w) float32 holding every value at least once, shuffled; spare pixels repeat values drawn from the set."""
    n = b * h * w
    assert values.size <= n, (values.size, n)
    v = np.concatenate([values, rng.choice(values, n - values.size)])
    return v[rng.permutation(n)].reshape(b, h, w).astype(np.float32)


def wrong_counts(x, wc, ww, pix, level):
    """How many of these inputs three plausible wrong implementations would miss (the fixtures' discriminating power)."""
    x64 = x.astype(np.float64)
    p64 = ((x64 + 1) * 0.5 * 4095)
    t32 = (x + np.float32(1)) * np.float32(0.5) * np.float32(4095)
    win_min = (2 * wc - ww) / 2.0 + 0.5
    dfac = 255.0 / ww

    def lvl(stored_minus_1024_f32, zero):
        t = np.where(zero, np.float32(-2000.0 - 1024.0), stored_minus_1024_f32).astype(np.float32)
        t = (t - np.float32(win_min)).astype(np.float32)
        return np.clip(np.trunc(t * np.float32(dfac)), 0, 255).astype(np.uint8)
    s64 = np.where(p64 == 0, -2000.0, p64) - 1024.0 - win_min
    l64 = np.clip(np.trunc(s64 * dfac), 0, 255).astype(np.uint8)
    # fused multiply-add: x * 4095 - 1024 with ONE rounding (the float64 product of two float32 numbers is exact)
    half = ((x + np.float32(1)) * np.float32(0.5)).astype(np.float32)
    fused = (half.astype(np.float64) * 4095.0 - 1024.0).astype(np.float32)
    lfma = lvl(fused, t32 == 0)
    # pix under a fused (x * 0.5 + 0.5) * 4095 is the same number (halving is exact); the fused form that can differ is the
    # float64-accumulated one above, and rounding instead of truncating
    return {"pix float64": int((np.trunc(p64).astype(np.int16) != pix).sum()),
            "pix round": int((np.rint(t32).astype(np.int16) != pix).sum()),
            "level float64": int((l64 != level).sum()), "level fma": int((lfma != level).sum())}


def main():
    sys.path.insert(0, ROOT)
    from oracle.make_golden_metrics import load_reference_functions
    to_windowdata = load_reference_functions()[0]
    rng = np.random.RandomState(20240539)
    pv = pix_values()
    lv = [level_values(*win) for win in WINDOWS]
    everything = np.concatenate([pv] + lv)
    cases = {
        "87x87": (planes(np.concatenate([pv, lv[0]]), 3, 87, 87, rng), [WINDOWS[0]] * 3),
        "64x48": (np.concatenate([planes(v, 1, 64, 48, rng) for v in lv]), WINDOWS),
        "5x7": (planes(rng.choice(everything, 105, replace=False), 3, 5, 7, rng), [WINDOWS[2], WINDOWS[0], WINDOWS[3]]),
    }
    total = 0
    for name, (x, wins) in cases.items():
        pix = ref_pix(x)
        win = np.stack([to_windowdata(x[i].copy(), wc, ww) for i, (wc, ww) in enumerate(wins)])
        assert win.dtype == np.float32
        lev64 = np.rint((win.astype(np.float64) + 1.0) / 2.0 * 255.0)
        assert lev64.min() >= 0 and lev64.max() <= 255
        level = lev64.astype(np.uint8)
        back = (level.astype(np.float32) / 255 - 0.5) / 0.5
        assert back.dtype == np.float32 and np.array_equal(back, win), name
        path = os.path.join(GOLD, "export_%s.npz" % name)
        np.savez_compressed(path, x=x, wc=np.array([w[0] for w in wins], dtype=np.float32),
                            ww=np.array([w[1] for w in wins], dtype=np.float32), pix=pix, win=win, level=level)
        total += os.path.getsize(path)
        print(name, x.shape, "levels reached:", np.unique(level).size, "pix range:", pix.min(), pix.max())
    # the discriminating power of the value sets themselves
    counts = wrong_counts(pv, *WINDOWS[0], ref_pix(pv), np.zeros(pv.size, np.uint8))
    print("pix values", pv.size, {k: v for k, v in counts.items() if k.startswith("pix")})
    for win_, v in zip(WINDOWS, lv):
        w = to_windowdata(v.copy(), *win_)
        level = np.rint((w.astype(np.float64) + 1.0) / 2.0 * 255.0).astype(np.uint8)
        counts = wrong_counts(v, *win_, ref_pix(v), level)
        print("level values", win_, v.size, "levels reached:", np.unique(level).size,
              {k: c for k, c in counts.items() if k.startswith("level")})
    print("wrote %d files, %d bytes" % (len(cases), total))


if __name__ == "__main__":
    main()
