"""Float64 / numpy helpers of tests/test_metrics_exact_gpu.py (csrc/metrics.hip, window_arith.h, input_arith.h).  No GPU.

oracle/ref_metrics.py and oracle/ref_inputs.py stay the definition of what the reference computes: everything here calls them.
What this file adds is (1) the inputs at which the kernels can go wrong -- level boundaries, special values, the 2^-4 grid --,
(2) the 20 sums of every block of ctg_window_metrics' `part` buffer in float64 from the oracle's masked images, with the sum of
the terms' magnitudes for the exactness argument, (3) the closed forms of window_metrics_final_kernel in float64 numpy, and
(4) two deliberately WRONG window evaluations that show what the boundary set is worth (tests/test_metrics_ref.py)."""
import collections
import math

import numpy as np

from oracle import ref_metrics

WINDOWS = ((50.0, 400.0), (40.0, 400.0), (60.0, 300.0), (300.0, 1500.0))      # (centre, width)
NSUM = 10                   # sums per pair: n_m, sum|d|_m, sum d^2_m, sum|d|, sum d^2, sx, sy, sxx, syy, sxy
U32 = 2.0 ** -24            # unit roundoff of fp32
GRANULE = 2.0 ** -8         # every term of the ten sums of a pair on the 2^-4 grid is a multiple of it


# ---------------------------------------------------------------------------- the oracle's images
class _Recorder:
    """`fns=` hook of the oracle's slice_metrics: its first mae call sees (c, b), the second (fake_m, real_m)."""

    def __init__(self):
        self.calls = []

    def mae(self, a, b):
        self.calls.append((a.copy(), b.copy()))
        with np.errstate(all="ignore"):
            return ref_metrics.mae(a, b)


def oracle_pairs(fake, real, wc, ww, aliased):
    """The four masked images of one slice as the oracle builds them, float32 [4, ...] in the plane order of ctg_window_pairs:
    [c, fake_m, b, real_m].  fake / real: 2-D float32 (any 2-D shape: the masks are elementwise)."""
    fake, real = np.asarray(fake, np.float32), np.asarray(real, np.float32)
    assert fake.ndim == 2 and fake.shape == real.shape
    rec = _Recorder()
    fn = ref_metrics.slice_metrics_cyc if aliased else ref_metrics.slice_metrics
    with np.errstate(all="ignore"):
        fn(fake.copy(), real.copy(), wc, ww, fns=(ref_metrics.to_windowdata, rec.mae, ref_metrics.psnr, ref_metrics.uqi))
    assert len(rec.calls) == 2
    (c, b), (fake_m, real_m) = rec.calls
    out = np.stack([c, fake_m, b, real_m])
    assert out.dtype == np.float32
    return out


def oracle_window(img, wc, ww):
    with np.errstate(invalid="ignore"):
        out = ref_metrics.to_windowdata(np.array(img, np.float32), wc, ww)
    assert out.dtype == np.float32
    return out


def oracle_metrics(fake, real, wc, ww, aliased):
    fn = ref_metrics.slice_metrics_cyc if aliased else ref_metrics.slice_metrics
    with np.errstate(all="ignore"):
        return fn(np.array(fake, np.float32), np.array(real, np.float32), wc, ww)


def levels_of(win):
    """The 8-bit level behind a windowed value (level / 255 - 0.5) / 0.5."""
    return np.rint((np.asarray(win, np.float64) * 0.5 + 0.5) * 255.0).astype(np.int64)


# ---------------------------------------------------------------------------- inputs
def boundary_set(wc, ww):
    """For every level L in 0 .. 256 the float32 value nearest to where the window's level steps to L, and its 4 float32
    neighbours on either side: 257 x 9 = 2313 values."""
    wmin = (2 * wc - ww) / 2.0 + 0.5
    dfac = 255.0 / ww
    L = np.arange(257, dtype=np.float64)
    v = (((L / dfac + wmin + 1024.0) / 4095.0) * 2.0 - 1.0).astype(np.float32)
    cols = [v]
    lo, hi = v.copy(), v.copy()
    for _ in range(4):
        lo = np.nextafter(lo, np.float32(-np.inf))
        hi = np.nextafter(hi, np.float32(np.inf))
        cols += [lo.copy(), hi.copy()]
    out = np.stack(cols, 1).reshape(-1).astype(np.float32)
    assert out.size == 2313
    return out


def grid_values():
    """The 33 values of the 2^-4 grid in [-1, 1]."""
    return (np.arange(-16, 17) / 16.0).astype(np.float32)


def special_values():
    one = np.float32(-1.0)
    return np.concatenate([np.array([-1.0, np.nextafter(one, np.float32(0)), 0.0, -0.0, 1.0, 1.5, -1.5, 3.0, -3.0], np.float32),
                           grid_values()])


def elementwise_set(wc, ww):
    """Boundary set of the window followed by the special values: 2355 values."""
    return np.concatenate([boundary_set(wc, ww), special_values()])


def elementwise_pair(wc, ww, n=None):
    """(fake, real) of the elementwise cases: `real` is the set (tiled to n values), `fake` the set read with a stride that is
    coprime to its length (2355 = 3 x 5 x 157), so foreground and background values of the one meet both of the other."""
    s = elementwise_set(wc, ww)
    fake = s[(np.arange(s.size) * 997) % s.size]
    if n is not None:
        idx = np.arange(n) % s.size
        s, fake = s[idx], fake[idx]
    return fake, s


def grid_images(seed, shape, lo=-16, hi=16):
    rng = np.random.default_rng(seed)
    return (rng.integers(lo, hi + 1, shape) / 16.0).astype(np.float32)


# ---------------------------------------------------------------------------- deliberately wrong evaluations
def window_fused(img, wc, ww):
    """WRONG on purpose: to_windowdata with `stored * 4095 - 1024` in ONE rounding (a contracted multiply-add), everything else
    float32 step by step as the reference.  What the kernel computed before csrc/window_arith.h."""
    f = np.float32
    h = ((np.asarray(img, f) + f(1)) * f(0.5)).astype(f)
    stored = h * f(4095)
    t = (h.astype(np.float64) * 4095.0 - 1024.0).astype(f)          # exact in float64, rounded once
    t = np.where(stored == 0, f(-2000.0 - 1024.0), t)
    wmin = f((2 * wc - ww) / 2.0 + 0.5)
    dfac = f(255.0 / (((2 * wc + ww) / 2.0 + 0.5) - ((2 * wc - ww) / 2.0 + 0.5)))
    t = np.trunc((t - wmin) * dfac)
    t = np.minimum(np.maximum(t, f(0)), f(255))
    t = t / f(255)
    return ((t - f(0.5)) / f(0.5)).astype(f)


def window_f64(img, wc, ww):
    """WRONG on purpose: the oracle itself, fed float64 (every step in double, the result cast to float32)."""
    return ref_metrics.to_windowdata(np.asarray(img, np.float32).astype(np.float64), wc, ww).astype(np.float32)


# ---------------------------------------------------------------------------- the reduction
def ops_nblk(hw):
    """The block count ops.window_metrics chooses (cta_gan_amd/ops.py: window_metrics_nblk), restated so that the CPU module can
    build the case without the library; the GPU module asserts that the two agree before it uses it."""
    return int(max(1, min(64, hw // 4096)))


def block_index(hw, nblk):
    """Block that owns pixel i: block b takes the 256-pixel chunks b, b + nblk, ..."""
    return (np.arange(hw) // 256) % nblk


def share_sizes(hw, nblk):
    return np.bincount(block_index(hw, nblk), minlength=nblk)


def pair_terms(x, y):
    """The ten terms per pixel of one pair (x = generated, y = reference side; background of y is exactly -1) in float64 from
    float32 images: [10, HW]."""
    x, y = np.asarray(x, np.float32).reshape(-1).astype(np.float64), np.asarray(y, np.float32).reshape(-1).astype(np.float64)
    d = x - y
    m = (y != -1.0).astype(np.float64)
    ad, d2 = np.abs(d), d * d
    # masked terms by selection, as the kernel does it (m ? ad : 0): a NaN outside the foreground stays outside
    return np.stack([m, np.where(m > 0, ad, 0.0), np.where(m > 0, d2, 0.0), ad, d2, x, y, x * x, y * y, x * y])


def part_ref(planes, nblk):
    """planes: the oracle's [c, fake_m, b, real_m] of one slice.  Returns (part [nblk, 20], S [nblk, 20], n [nblk]): the 20 sums
    of every block (windowed pair first, then the raw pair), the sums of the terms' magnitudes, the pixels per block.  The sums
    are math.fsum of the float64 terms: correctly rounded, so the reference itself is within half an ulp of the true sum."""
    planes = np.asarray(planes)
    hw = planes[0].size
    terms = np.concatenate([pair_terms(planes[0], planes[2]), pair_terms(planes[1], planes[3])])        # [20, HW]
    blk = block_index(hw, nblk)
    part = np.zeros((nblk, 2 * NSUM))
    S = np.zeros((nblk, 2 * NSUM))
    for b in np.unique(blk):
        sel = terms[:, blk == b]
        part[b] = [math.fsum(row) for row in sel.tolist()]
        S[b] = np.abs(sel).sum(1)
    return part, S, share_sizes(hw, nblk)


def gamma(n):
    """|fl32 sum - sum| <= gamma(n) * sum|terms| for n fp32 terms added in any order, each term carrying up to three roundings of
    its own (d = x - y, d * d): (n - 1) + 3 = n + 2 roundings."""
    n = np.asarray(n, np.float64)
    return (n + 2) * U32 / (1 - (n + 2) * U32)


U64 = 2.0 ** -53            # unit roundoff of double


def gamma64(n):
    """The same bound for what the kernel does: every term formed in double from two floats -- x, y, x * x, y * y, x * y and
    d = x - y are exact there, d * d is rounded once -- and n terms added in double in any order, against a correctly rounded
    reference (half a rounding): (n - 1) + 1 + 1 = n + 1 roundings of 2^-53."""
    n = np.asarray(n, np.float64)
    return (n + 1) * U64 / (1 - (n + 1) * U64)


def assert_exact_domain(S, granule=GRANULE):
    """As tests/conv_ref.py: S = the sum of the magnitudes of the terms of every accumulator.  Below 2^24 granules every fp32
    partial sum is exact, in any order; a block's share is a superset of any thread's or wave's."""
    m = float(np.max(S)) / granule
    assert m < 2 ** 24, "not an exact case: sum of |terms| = %g granules >= 2^24" % m
    return m


def final_ref(sums, hw):
    """The closed forms of window_metrics_final_kernel in float64 numpy: sums [2, 10] -> [2, 3] = {windowed, raw} x {MAE, PSNR,
    UQI}.  The same operations in the same order."""
    out = np.zeros((2, 3))
    N = np.float64(hw)
    with np.errstate(all="ignore"):
        for p in range(2):
            s = np.asarray(sums[p], np.float64)
            mae = (s[1] / s[0] if s[0] > 0.0 else s[3] / N + 1e-10) / 2.0
            mse = s[2] / (4.0 * s[0]) if s[0] > 0.0 else s[4] / (4.0 * N) + 1e-10
            psnr = 100.0 if mse < 1.0e-10 else 20.0 * np.log10(1.0 / (np.sqrt(mse) + 1e-10))
            mf, mr = s[5] / N, s[6] / N
            vf, vr = (s[7] - N * mf * mf) / (N - 1.0), (s[8] - N * mr * mr) / (N - 1.0)
            cov = (s[9] - N * mf * mr) / (N - 1.0)
            uqi = 4.0 * mf * mr * cov / ((mf * mf + mr * mr) * (vf + vr) + 1e-10)
            out[p] = (mae, psnr, uqi)
    return out


def uqi_two_pass_f64(x, y):
    """UQI (HdTrainer.py:1119-1125) of two images in float64, two passes: the yardstick of the ill-conditioned case."""
    with np.errstate(all="ignore"):
        return float(ref_metrics.uqi(np.asarray(x, np.float64).reshape(1, -1), np.asarray(y, np.float64).reshape(1, -1)))


# ---------------------------------------------------------------------------- reduction cases
# name, B, HW, nblk (None: what ops chooses)
Case = collections.namedtuple("Case", "name B HW nblk")
REDUCTION_CASES = (
    Case("hw2", 2, 2, 1),
    Case("hw255", 2, 255, 1),
    Case("hw256", 2, 256, 1),
    Case("hw257", 2, 257, 1),
    Case("hw12365_ops", 3, 4096 * 3 + 77, None),
    Case("hw1000_nblk4096", 2, 1000, 4096),
    Case("hw3841_nblk5", 2, 5 * 256 * 3 + 1, 5),
    Case("hw16384_nblk1", 2, 128 * 128, 1),
)
BATCH_CASES = (Case("b33", 33, 300, 2), Case("b70", 70, 300, 2))


def case_nblk(case):
    return case.nblk if case.nblk is not None else ops_nblk(case.HW)


def case_windows(B):
    wc = np.array([WINDOWS[i % 4][0] for i in range(B)], np.float32)
    ww = np.array([WINDOWS[i % 4][1] for i in range(B)], np.float32)
    return wc, ww


def case_inputs(case, seed=0):
    """fake, real [B, HW]: any values of the 2^-4 grid in [-1, 1], a different window per slice.  About two thirds of the grid are
    foreground under each window, so every slice is part foreground and cc is mixed too (tests/test_metrics_ref.py asserts it);
    pixel 0 is foreground and pixel 1 background in every slice, which is all of HW = 2."""
    rng = np.random.default_rng([seed, case.B, case.HW])
    fake = (rng.integers(-16, 17, (case.B, case.HW)) / 16.0).astype(np.float32)
    real = (rng.integers(-16, 17, (case.B, case.HW)) / 16.0).astype(np.float32)
    real[:, 0] = 0.75
    real[:, 1] = -1.0
    fake[:, 0] = 0.5
    wc, ww = case_windows(case.B)
    return fake, real, wc, ww


def case_reference(case, aliased, seed=0):
    """(fake, real, wc, ww, planes [B, 4, HW], part [B, nblk, 20], S [B, nblk, 20], n [nblk]) of a case."""
    fake, real, wc, ww = case_inputs(case, seed)
    nblk = case_nblk(case)
    planes = np.stack([oracle_pairs(fake[i][None], real[i][None], float(wc[i]), float(ww[i]), aliased)[:, 0] for i in range(case.B)])
    parts, Ss = [], []
    for i in range(case.B):
        p, S, n = part_ref(planes[i], nblk)
        parts.append(p)
        Ss.append(S)
    return fake, real, wc, ww, planes, np.stack(parts), np.stack(Ss), n


def exact_columns(aliased):
    """Which of the 20 sums are exact on grid inputs: the raw pair always; the windowed pair when it is binary (aliased); the
    count n_m of the windowed pair always."""
    e = np.zeros(2 * NSUM, bool)
    e[NSUM:] = True
    e[0] = True
    if aliased:
        e[:NSUM] = True
    return e


def ill_conditioned_slice(hw=128 * 128, seed=5, noise=0.0):
    """A nearly constant pair for UQI: -0.875 everywhere, a handful of pixels one grid step (2^-4) away; with `noise`, uniform
    noise of that amplitude on top (off the grid).  Window (-1000, 40): every value is foreground at level 255, so the raw pair
    is the pair itself.  hw is a power of two: the means and N * m^2 of the closed form are exact on the grid."""
    rng = np.random.default_rng(seed)
    fake = np.full(hw, -0.875, np.float32)
    real = np.full(hw, -0.875, np.float32)
    idx = rng.choice(hw, 12, replace=False)
    fake[idx[:8]] += np.float32(0.0625)           # eight pixels move together in both images, four in one of them only
    real[idx[:8]] += np.float32(0.0625)
    fake[idx[8:10]] -= np.float32(0.0625)
    real[idx[10:]] -= np.float32(0.0625)
    if noise:
        fake = (fake + rng.uniform(-noise, noise, hw)).astype(np.float32)
        real = (real + rng.uniform(-noise, noise, hw)).astype(np.float32)
    return fake, real, -1000.0, 40.0


def ill_conditioned_windowed_slice(hw=128 * 128, seed=7):
    """A nearly constant WINDOWED pair: under the window (50, 400) every pixel is foreground at level 200 (HU 165) but for a
    handful at level 201 (HU 166.6): c and b are 145 / 255 and 147 / 255, not dyadic, their variance about 5e-8 beside a mean square
    of 0.02.  The raw pair (the samples themselves, about -0.42) is as badly conditioned."""
    rng = np.random.default_rng(seed)
    v200 = np.float32((165.0 + 1024.0) / 4095.0 * 2.0 - 1.0)
    v201 = np.float32((166.6 + 1024.0) / 4095.0 * 2.0 - 1.0)
    fake = np.full(hw, v200, np.float32)
    real = np.full(hw, v200, np.float32)
    idx = rng.choice(hw, 12, replace=False)
    fake[idx[:10]] = v201                         # eight pixels step in both images, two in each of them alone
    real[idx[:8]] = v201
    real[idx[10:]] = v201
    return fake, real, 50.0, 400.0


def uqi_condition(sums, hw):
    """How much the closed form of UQI amplifies a relative error of its sums: the largest of (a + b) / |a - b| over the three
    moments s_xx - N mx^2, s_yy - N my^2, s_xy - N mx my.  sums: the ten sums of one pair."""
    s = np.asarray(sums, np.float64)
    N = float(hw)
    mf, mr = s[5] / N, s[6] / N
    k = 1.0
    for a, b in ((s[7], N * mf * mf), (s[8], N * mr * mr), (s[9], N * mf * mr)):
        if a != b:
            k = max(k, (abs(a) + abs(b)) / abs(a - b))
    return k


# ---------------------------------------------------------------------------- input pipeline
def hu_sweep():
    """The whole int16 domain followed by 77 repeated values (a ragged count)."""
    return np.concatenate([np.arange(-32768, 32768, dtype=np.int64), np.arange(77, dtype=np.int64) * 13 - 1100]).astype(np.int16)


def hu_reference(hu, wc, ww):
    """The oracle on the int16 array the reference's reader hands it (oracle/make_golden_inputs.py): `data1 + 1024` stays int16
    there and wraps above 31743."""
    from oracle import ref_inputs
    hu = np.asarray(hu)
    assert hu.dtype == np.int16
    i1, i2 = ref_inputs.read_ori_w_arith(hu.copy(), wc, ww)
    return i1.astype(np.float32), i2.astype(np.float32)


def first_diff(got, want):
    """Index and values of the first differing element (bits compared), for failure messages."""
    g, w = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).reshape(-1)
    assert g.dtype == w.dtype and g.size == w.size, (g.dtype, w.dtype, g.size, w.size)
    bits = {4: np.uint32, 8: np.uint64}[g.dtype.itemsize]
    bad = np.flatnonzero(g.view(bits) != w.view(bits))
    if bad.size == 0:
        return None
    i = int(bad[0])
    return "%d differ, first at %d: got %r want %r" % (bad.size, i, g[i], w[i])
