"""GPU: the metrics and input-pipeline kernels (csrc/metrics.hip, window_arith.h, input_arith.h) against the oracle
(oracle/ref_metrics.py, oracle/ref_inputs.py) through tests/metrics_ref.py -- bit for bit wherever the arithmetic allows it.

Exactness argument.  (1) Elementwise (ctg_to_windowdata, ctg_window_pairs, ctg_hu_to_inputs, ctg_resize_nearest): the kernels
restate the reference's float32 / float64 operations one rounding at a time, so every output has to equal the oracle's bit for
bit; the inputs are the ones where one rounding more or less shows -- for each window every level boundary with four float32
neighbours on either side (metrics_ref.boundary_set: a contracted `h * 4095 - 1024` differs from the oracle on 12 .. 87 of its
2313 values and on none of 2313 random ones, tests/test_metrics_ref.py), the special values and the 2^-4 grid; the whole int16
domain; every (n_in, n_out) up to 24.  NaN positions and the bits of everything else are compared separately.  (2) The reduction
(ctg_window_metrics): with fake and real on the 2^-4 grid the raw pair (fake_m, real_m) and the aliased windowed pair (+-1) are
dyadic, every term of their ten sums is a multiple of 2^-8 of magnitude <= 4, and while the sum of the terms' magnitudes of a
block's share stays below 2^24 granules (metrics_ref.assert_exact_domain, BEFORE anything is launched; the CPU module asserts it
for every case) the sum is exact in fp32 and in double in ANY order: those sums of `part` must equal the float64 sums of the
oracle's images over the pixels with (i // 256) % nblk == block, bit for bit -- a dropped, doubled or misplaced pixel is an exact
difference in a named (slice, block, sum).  The windowed pair that is not aliased holds level / 255 values, not dyadic.  The
kernel forms every term in double from two floats (x, y, x x, y y, x y and d = x - y are exact there, d d is rounded once) and
adds in double, so its nine sums are held to |got - want| <= gamma64 S, gamma64 = (n + 1) u / (1 - (n + 1) u), u = 2^-53, n the
pixels of the block's share, S the float64 sum of the terms' magnitudes: n - 1 additions in any order, the rounding of a term,
and the reference's own half rounding -- the reference sums are math.fsum, correctly rounded.  That is 2^29 times tighter than the
any-order fp32 bound gamma S with u = 2^-24 and (n + 2), which it implies (asserted); fp32 per-thread sums miss it by five orders
of magnitude (mutation 9).  `out` of BOTH pairs is compared with the closed forms of window_metrics_final_kernel evaluated in
float64 numpy (metrics_ref.final_ref) from the REFERENCE sums at 1e-12 relative (+ 1e-12, the float64 floor of
tests/test_metrics.py's SSIM checks): the kernel is not compared with itself anywhere.  Measured on the MI355X: every case met the closed forms with no difference above the 1e-12 floor (printed: 0), and the inexact sums used
at most 0.005 of gamma64 S, so
the device's log10 and sqrt needed no wider bound.  Only the two nearly constant level / 255 slices, whose UQI amplifies a
relative error of its sums by kappa = 2e7 and 1e9 (metrics_ref.uqi_condition), have a derived UQI bound instead:
1e-12 + 4 kappa (gamma64(n) + 4 u), see test_window_metrics_ill_conditioned_windowed_pair; measured there: UQI 1.5e-10 (windowed) and 7.2e-8 (raw) from the closed form of the reference sums, 3.0e-10 and
2.0e-8 from the float64 two-pass value, where the oracle's float32 two-pass UQI is 8.4e-8 and 1.3e-6 away.
The first four slices of every case are also held to the oracle's own float32 numbers at the suite's 1e-5 (+ 1e-9: `_close` of
tests/test_metrics.py).  (3) SSIM is float64 on
both sides in another order: the existing 1e-9 (+ 1e-12).

Every output buffer is filled with a sentinel (NaN for doubles, -12345 for floats) and allocated with a guard of 1024 elements
behind its end (64 per launch in the resize sweep); the guard, slot 1 of ctg_ssim's `part` in mode 0, and everything after a
refusal must keep the sentinel; every element a launch owns must have lost it.

Cases (B slices, per-slice windows out of (50, 400), (40, 400), (60, 300), (300, 1500) unless stated):
  to_windowdata, window_pairs x {plain, aliased}   B = 4 x 2355 (2355 % 256 = 51): boundary set + specials, `fake` = the set read with
                                                   stride 997 so all four mask combinations meet; B = 4 x (1024 * 256 + 300): second trip
  window_pairs / to_windowdata with NaN            a NaN in fake and in real, each under foreground and background of the other image
  window_metrics x {plain, aliased}, part + out    HW = 2 | 255, 256, 257 (nblk 1) | 12365 (nblk 3, what ops chooses; also through ops)
                                                   | 1000 (nblk 4096: 4092 blocks own no pixel and write 20 zeros) | 3841 (nblk 5: shares
                                                   769, 768 x 4) | 16384 (nblk 1: 64 trips per thread) | B = 33 and 70 x 300 (nblk 2)
  all background                                   both pairs (real = -1); the raw pair only (real = 0 under (300, 1500)); alone and as one
                                                   slice of three; against the oracle at 1e-5
  ill-conditioned UQI                              -0.875 with 12 pixels one grid step away, window (-1000, 40), 128 x 128, on the grid
                                                   (exact) and with uniform noise of 1e-3; levels 200 with 12 pixels at 201 under
                                                   (50, 400): a nearly constant, not dyadic windowed AND raw pair, nblk 4 (through ops too)
  NaN                                              one NaN pixel of fake in the foreground of one slice of three
  ssim mode 0                                      7x7, 7x200, 22x22, 23x22, 38x39, 21x134: grid and random inputs, data_range 2, 1, 255;
                                                   constant pairs (data_range 2, 0.5); B = 65 and 130 of 23x22 (two blocks per slice)
  ssim mode 1 x {plain, aliased}                   B = 33 of 23x22, per-slice windows
  hu_to_inputs, four windows                       -32768 .. 32767 + 77 values; 4096 * 256 + 300 values (second trip)
  resize_nearest                                   (n_in, n_out) in 1..24 x 1..24 along H, transposed along W, B = 2 (576 launches,
                                                   under 0.1 s: not halved); 3x5 -> 725x725 (second trip), 512 -> 256, 256 -> 512, n_out = 1
  refusals                                         null pointers, B = 0 and 65536 (four entries), HW = 1, nblk 0 / 4097, SSIM H / W = 6,
                                                   mode 2, mode 1 without windows, data_range 0 / NaN / < 0, ww <= 0, n = 0, zero dimensions

Not covered, and why:
  * a windowed pair that alone is all background: b != -1 exactly where the mask bb is 1, and bb = 0 everywhere makes the raw real_m
    all -1 too; the case that exists is the raw pair alone (real = 0 in the foreground);
  * `fake_m == 0 -> -1` through a ZERO SAMPLE under cc = 1 with the (50 | 40 | 60, ..) windows: the level of 0 is background there;
    (300, 1500) reaches it (level 250), the others reach the rule through the zero product under cc = 0;
  * infinite inputs; B = 65535 itself (a 65535-row grid of real launches is not a unit test); HW beyond 2^31;
  * which launch configuration ops picks for anything but ctg_window_metrics' nblk (the other grids are chosen inside the library);
  * the index clamp of nearest_src_index: floor(o * fl(n_in / n_out)) never reaches n_in for any pair of sizes below 600 (searched
    on the CPU), so no input shows it (mutation 6a).

Found by this module (fixed with it):
  * UQI lost every digit on nearly constant slices: the partial kernel accumulated in fp32 per thread and wave, and
    s_xx - N m^2 of such sums is a difference of nearly equal numbers.  Off-grid slice above, on the card: 6.4e-3 relative from the
    float64 two-pass UQI, where the oracle's float32 two-pass UQI is 1.4e-7 away; a slice whose windowed reference image is constant gave UQI -1.4e-9 for
    the oracle's 0.  The kernel now forms and adds every term in double: 6.4e-12 on the same slice.  (The header comment of
    csrc/metrics.hip had claimed fp64 all along.)
  * NaN samples: numpy's `m[m < 0.3] = 0; m[m >= 0.3] = 1` leaves a NaN mask NaN, so a NaN in real makes c, fake_m, b and real_m
    NaN; masked_pixel thresholded with `>= 0.3 ? 1 : 0` and gave c = fake_m = -1 (and, aliased, finite +-1 for b and c beside a NaN
    sample: the aliased windowed MAE / PSNR / UQI of a slice with a NaN pixel were finite).  Now threshold_mask keeps the NaN.
  * ctg_hu_to_inputs' full-range image above HU 31743: the reference adds 1024 to the reader's int16 array in int16, which wraps, and
    the clamp sends the negative result to -1; the kernel added in double (up to 15.5).  1024 of 65536 values; now wrapped as numpy does.
  * ctg_to_windowdata and ctg_window_metrics put B into gridDim.y without the B <= 65535 check of their neighbours.

Mutation checks.  Each was built once from csrc/metrics.hip and the mutated header into a library of its own outside the repository
(never committed; each stays inside its buffers), and this module and tests/test_metrics.py + tests/test_inputs.py were run
against it once on the card:
  1  partial kernel's loop stops at HW - HW % 256            -> the 16 ragged part_and_out cases (HW 2, 255, 257, 12365, 1000, 3841, 300 x 2) and
                                                               all_background (HW 300); 256 and 16384 pass.  The old modules PASS.
  2  final kernel's guard also `i >= 64`                     -> b33, b70 (both modes), nothing else.  The old modules PASS.
  3  red[3][k] left out of the block sum                     -> every part_and_out case but HW 2, all_background, ill-conditioned UQI.  Old modules: 3 fail.
  4a `>= 0.3f` becomes `> 0.3f`                              -> nothing, here or there: EQUIVALENT.  No level L / 255 rescales to 0.3f (165 -> 0.2941,
                                                               166 -> 0.3020), and the products by a 0 / 1 mask do not create it.
  4b `rm == 0 -> -1` dropped                                 -> the four window_pairs boundary cases (real_m, at the zero products), NaN pairs, every
                                                               part_and_out case, all_background, ssim mode 1.  Old modules: 4 fail.
  5  `fp contract(off)` removed from stored_level            -> nothing: EQUIVALENT with this compiler -- the kernel's code is the same instruction for
                                                               instruction, because the multiply of `x * 4095 - 1024` sits in stored_value under its own pragma.
  5b ... removed from stored_value and stored_level          -> both to_windowdata boundary cases, window_pairs boundary [plain] x 2 and the NaN pairs (their window check): the
                                                               compiler then contracts `x * 4095 - 1024` (one fused multiply-add more in the kernel).
                                                               The aliased pairs pass: no flipped level crosses the 0.3 mask.  The old modules PASS.
  6a nearest_src_index without the clamp to n - 1            -> nothing: the clamp never binds (see "Not covered").
  6b nearest_src_index with rintf                            -> both resize tests.  Old modules: 3 fail.
  7  hu_fullrange without the `< 0` clamp                    -> the four sweeps and the second trip (values below -1024).  Old modules: 1 fails (its
                                                               fixtures hold -2000).
  8  ssim_final_kernel reads `part` with stride npair        -> the six ssim_sizes cases and both mode-0 batches (all mode 0); mode 1 passes.  Old modules: 1 fails.
  9  PairAcc's sums float again (the first fault, both pairs)  -> the nine plain part_and_out cases from HW 255 on (the inexact sums), all_background[plain],
                                                               both ill-conditioned tests; the aliased cases and HW 2 pass (exact in fp32).  The old modules PASS.
  0  the library before the fixes above                      -> NaN pairs (2), all_background[plain], ill-conditioned UQI, NaN propagation[aliased], the
                                                               five HU cases.  The old modules PASS.
So of the first seven, 1, 2 and 5b (and 9, and the four faults found) were invisible to the old modules; 3, 4b, 6b and 7 were already caught there;
4a, 5 and 6a change nothing observable.

Wall time on the MI355X: 52 tests in 1.8 s (slowest: 0.27 s, the first launch; the 576-launch resize sweep under 0.1 s).
"""
import numpy as np
import pytest
import torch

import metrics_ref as R
from oracle import ref_metrics

pytestmark = pytest.mark.gpu

SENT = -12345.0          # float sentinel: no case produces it (windows: [-1, 1]; raw planes: the inputs, |v| <= 3; full range: [-1, 15.0]; resize: >= 0)
GUARD = 1024             # sentinel elements behind the end of every output buffer
EINVAL = 1


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cta_gan_amd import _lib
    return _lib.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _fbuf(n):
    return torch.full((n + GUARD,), SENT, dtype=torch.float32, device="cuda")


def _dbuf(n):
    return torch.full((n + GUARD,), float("nan"), dtype=torch.float64, device="cuda")


def _untouched_f(t, start=0):
    return bool((t[start:] == SENT).all())


def _untouched_d(t, start=0):
    return bool(torch.isnan(t[start:]).all())


def _same_bits(got, want, what):
    d = R.first_diff(np.asarray(got), np.asarray(want))
    assert d is None, "%s: %s" % (what, d)


def _same_bits_nan(got, want, what):
    """NaN positions first, then the bits of everything else."""
    got, want = np.asarray(got), np.asarray(want)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "%s: NaN at %s, the oracle at %s" % (what, np.flatnonzero(gn.reshape(-1))[:8], np.flatnonzero(wn.reshape(-1))[:8])
    _same_bits(np.where(gn, 0, got).astype(got.dtype), np.where(wn, 0, want).astype(want.dtype), what)


def _rel_close(got, want, rel, abs_):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool(np.all((np.abs(got - want) <= rel * np.abs(want) + abs_) | (np.isnan(got) & np.isnan(want))))


# ============================================================================ 1. elementwise arithmetic
def _elementwise_batch(n=None):
    """B = 4 slices, one per window: fake, real [4, n]."""
    pairs = [R.elementwise_pair(wc, ww, n) for wc, ww in R.WINDOWS]
    wc = np.array([w[0] for w in R.WINDOWS], np.float32)
    ww = np.array([w[1] for w in R.WINDOWS], np.float32)
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]), wc, ww


def _run_window(lib, img, wc, ww):
    b, hw = img.shape
    out = _fbuf(b * hw)
    d_img, d_wc, d_ww = _dev(img), _dev(wc), _dev(ww)              # named: they must outlive the launch
    st = lib.ctg_to_windowdata(d_img.data_ptr(), d_wc.data_ptr(), d_ww.data_ptr(), out.data_ptr(), b, hw, _st())
    assert st == 0, st
    assert _untouched_f(out, b * hw), "ctg_to_windowdata wrote behind its output"
    return out[:b * hw].cpu().numpy().reshape(b, hw)


def _run_pairs(lib, fake, real, wc, ww, aliased):
    b, hw = fake.shape
    out = _fbuf(4 * b * hw)
    d_f, d_r, d_wc, d_ww = _dev(fake), _dev(real), _dev(wc), _dev(ww)
    st = lib.ctg_window_pairs(d_f.data_ptr(), d_r.data_ptr(), d_wc.data_ptr(), d_ww.data_ptr(), b, hw, int(aliased), out.data_ptr(), _st())
    assert st == 0, st
    assert _untouched_f(out, 4 * b * hw), "ctg_window_pairs wrote behind its output"
    return out[:4 * b * hw].cpu().numpy().reshape(4, b, hw)


def _oracle_planes(fake, real, wc, ww, aliased):
    """[4, B, HW]"""
    return np.stack([R.oracle_pairs(fake[i][None], real[i][None], float(wc[i]), float(ww[i]), aliased)[:, 0]
                     for i in range(fake.shape[0])], 1)


@pytest.mark.parametrize("n", [None, 1024 * 256 + 300], ids=["set", "second_trip"])
def test_to_windowdata_on_the_boundary_set(lib, n):
    fake, real, wc, ww = _elementwise_batch(n)
    assert real.shape[1] % 256 != 0 and real.shape[1] == (n or 2355)
    got = _run_window(lib, real, wc, ww)
    for i in range(4):
        _same_bits(got[i], R.oracle_window(real[i], float(wc[i]), float(ww[i])), "window %s" % (R.WINDOWS[i],))


@pytest.mark.parametrize("aliased", [0, 1])
@pytest.mark.parametrize("n", [None, 1024 * 256 + 300], ids=["set", "second_trip"])
def test_window_pairs_on_the_boundary_set(lib, n, aliased):
    fake, real, wc, ww = _elementwise_batch(n)
    want = _oracle_planes(fake, real, wc, ww, aliased)
    for i in range(4):                                   # every (foreground, background) x (foreground, background) meets
        wf = R.oracle_window(fake[i], float(wc[i]), float(ww[i])) >= 0.3
        wr = R.oracle_window(real[i], float(wc[i]), float(ww[i])) >= 0.3
        assert all(((wf == a) & (wr == b)).any() for a in (False, True) for b in (False, True)), i
    got = _run_pairs(lib, fake, real, wc, ww, aliased)
    for plane, name in enumerate(("c", "fake_m", "b", "real_m")):
        for i in range(4):
            _same_bits(got[plane, i], want[plane, i], "%s, window %s" % (name, R.WINDOWS[i],))


@pytest.mark.parametrize("aliased", [0, 1])
def test_window_pairs_nan_is_the_oracles(lib, aliased):
    """A NaN in `fake` and a NaN in `real`, each under a foreground and under a background pixel of the other image: numpy's
    masked assignments leave a NaN mask NaN, so the pixel is NaN in every image the mask multiplies."""
    fake, real, wc, ww = _elementwise_batch()
    fake, real = fake.copy(), real.copy()
    for i in range(4):
        wf = R.oracle_window(fake[i], float(wc[i]), float(ww[i])) >= 0.3
        wr = R.oracle_window(real[i], float(wc[i]), float(ww[i])) >= 0.3
        fake[i, np.flatnonzero(wr)[3]] = np.nan
        fake[i, np.flatnonzero(~wr)[3]] = np.nan
        real[i, np.flatnonzero(wf & ~np.isnan(fake[i]))[5]] = np.nan
        real[i, np.flatnonzero(~wf & ~np.isnan(fake[i]))[5]] = np.nan
    want = _oracle_planes(fake, real, wc, ww, aliased)
    assert np.isnan(want).sum() >= 4 * 8
    got = _run_pairs(lib, fake, real, wc, ww, aliased)
    for plane, name in enumerate(("c", "fake_m", "b", "real_m")):
        _same_bits_nan(got[plane], want[plane], name)
    # ctg_to_windowdata: NaN stays NaN
    gw = _run_window(lib, real, wc, ww)
    _same_bits_nan(gw, np.stack([R.oracle_window(real[i], float(wc[i]), float(ww[i])) for i in range(4)]), "window")


# ============================================================================ 2. the reduction, through `part`
def _run_metrics(lib, fake, real, wc, ww, nblk, aliased):
    """-> part [B, nblk, 20], out [B, 2, 3]; both guards checked, and that the launch wrote every element of both."""
    b, hw = fake.shape
    part, out = _dbuf(b * nblk * 20), _dbuf(b * 6)
    d_f, d_r, d_wc, d_ww = _dev(fake), _dev(real), _dev(np.asarray(wc, np.float32)), _dev(np.asarray(ww, np.float32))
    st = lib.ctg_window_metrics(d_f.data_ptr(), d_r.data_ptr(), d_wc.data_ptr(), d_ww.data_ptr(), b, hw, nblk, int(aliased),
                                part.data_ptr(), out.data_ptr(), _st())
    assert st == 0, st
    assert _untouched_d(part, b * nblk * 20), "ctg_window_metrics wrote behind `part`"
    assert _untouched_d(out, b * 6), "ctg_window_metrics wrote behind `out` (elements past 6 B)"
    return part[:b * nblk * 20].cpu().numpy().reshape(b, nblk, 20), out[:b * 6].cpu().numpy().reshape(b, 2, 3)


def _seq_sum(part):
    """Block partials added in the final kernel's order: [B, nblk, 20] -> [B, 20]."""
    s = np.zeros((part.shape[0], part.shape[2]))
    for b in range(part.shape[1]):
        s = s + part[:, b]
    return s


def _check_part(part, want, S, n, e, name):
    """Every element of `part`: the exact sums (columns e) on their bits; the others within gamma64(n) S of the correctly
    rounded reference -- the bound for what the kernel does (double throughout), 2^29 times tighter than the fp32 any-order
    bound gamma(n) S, which it implies.  Returns the largest |got - want| / (gamma64 S)."""
    assert not np.isnan(part).any(), "%s: %d elements of `part` were not written" % (name, int(np.isnan(part).sum()))
    for i in range(part.shape[0]):
        for blk in range(part.shape[1]):
            d = R.first_diff(part[i, blk, e], want[i, blk, e])
            assert d is None, "%s: slice %d block %d (%d pixels), exact sums %s: %s" % (name, i, blk, n[blk], np.flatnonzero(e), d)
    if e.all():
        return 0.0
    bound = R.gamma64(n)[None, :, None] * S
    assert np.all(bound <= R.gamma(n)[None, :, None] * S)
    err = np.abs(part - want)
    bad = np.argwhere((err > bound) & ~e[None, None, :])
    assert bad.size == 0, "%s: (slice, block, sum) %s: |got - want| = %g > gamma64 S = %g" % (
        name, bad[0], err[tuple(bad[0])], bound[tuple(bad[0])])
    return float((err[:, :, ~e] / np.maximum(bound[:, :, ~e], 1e-300)).max())


def _check_reduction(lib, fake, real, wc, ww, nblk, aliased, planes, want, S, n, name):
    e = R.exact_columns(aliased)
    R.assert_exact_domain(S[:, :, e])                                   # before anything is launched
    part, out = _run_metrics(lib, fake, real, wc, ww, nblk, aliased)
    worst = _check_part(part, want, S, n, e, name)
    # out: the closed forms in float64 numpy from the REFERENCE sums, both pairs
    sums_ref = _seq_sum(want)
    worst_out = 0.0
    for i in range(fake.shape[0]):
        cf = R.final_ref(sums_ref[i].reshape(2, 10), fake.shape[1])
        rel = np.abs(out[i] - cf) / np.maximum(np.abs(cf), 1e-300)
        worst_out = max(worst_out, float(np.where(np.abs(out[i] - cf) <= 1e-12, 0.0, rel).max()))
        assert _rel_close(out[i], cf, 1e-12, 1e-12), "%s: slice %d out %s closed form of the reference sums %s" % (name, i, out[i], cf)
    print("%s aliased=%d: inexact sums at most %.3f of gamma64 S; out off the closed forms of the reference sums by at most %.2e relative"
          % (name, aliased, worst, worst_out))
    return part, out


@pytest.mark.parametrize("aliased", [0, 1])
@pytest.mark.parametrize("case", R.REDUCTION_CASES + R.BATCH_CASES, ids=lambda c: c.name)
def test_window_metrics_part_and_out(lib, case, aliased):
    fake, real, wc, ww, planes, want, S, n = R.case_reference(case, aliased)
    nblk = R.case_nblk(case)
    if case.nblk is None:
        from cta_gan_amd import ops
        assert nblk == ops.window_metrics_nblk(case.HW) and nblk > 1, nblk
    _, out = _check_reduction(lib, fake, real, wc, ww, nblk, aliased, planes, want, S, n, case.name)
    if case.nblk is None:                                               # the launch ops chooses: the same numbers
        from cta_gan_amd import ops
        got = ops.window_metrics(_dev(fake), _dev(real), wc.tolist(), ww.tolist(), aliased=bool(aliased)).cpu().numpy()
        _same_bits(got, out, "ops.window_metrics")
    for i in range(min(case.B, 4)):                                     # and the oracle's own float32 numbers at the suite's 1e-5
        o = R.oracle_metrics(fake[i][None], real[i][None], float(wc[i]), float(ww[i]), aliased)
        assert _rel_close(out[i], o, 1e-5, 1e-9), (case.name, i, out[i], o)


def _allbg_batch():
    """Slices of 300 pixels.  0: both pairs all background (real = -1).  1: the raw pair only -- real = 0 is foreground under the
    window (300, 1500) and the raw rule `real_m == 0 -> -1` makes it background.  (The windowed pair alone cannot be all
    background: b != -1 exactly where bb = 1, and bb = 0 makes real_m -1 as well.)  2: an ordinary slice."""
    hw = 300
    fake = R.grid_images(21, (3, hw))
    real = R.grid_images(22, (3, hw))
    real[0] = -1.0
    real[1] = 0.0
    real[2, :40] = 0.75
    wc = np.array([50.0, 300.0, 40.0], np.float32)
    ww = np.array([400.0, 1500.0, 400.0], np.float32)
    return fake, real, wc, ww


@pytest.mark.parametrize("aliased", [0, 1])
def test_window_metrics_all_background(lib, aliased):
    fake, real, wc, ww = _allbg_batch()
    planes = _oracle_planes(fake, real, wc, ww, aliased)                # [4, B, HW]
    ref = [R.part_ref(planes[:, i], 2) for i in range(3)]
    want, S, n = np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref]), ref[0][2]
    nm = want[:, :, (0, 10)].sum(1)
    assert nm[0, 0] == 0 and nm[0, 1] == 0 and nm[1, 0] > 0 and nm[1, 1] == 0 and nm[2, 0] > 0 and nm[2, 1] > 0, nm
    part, out = _run_metrics(lib, fake, real, wc, ww, 2, aliased)
    e = R.exact_columns(aliased)
    R.assert_exact_domain(S[:, :, e])
    _check_part(part, want, S, n, e, "all background")
    for sub in ([0], [1], [0, 1, 2]):                                   # alone and as one slice of a batch
        _, o = _run_metrics(lib, fake[sub], real[sub], wc[sub], ww[sub], 2, aliased)
        _same_bits(o, out[sub], "slices %s alone" % sub)
    for i in range(3):
        o = R.oracle_metrics(fake[i][None], real[i][None], float(wc[i]), float(ww[i]), aliased)
        assert _rel_close(out[i], o, 1e-5, 1e-9), (i, out[i], o)


def test_window_metrics_ill_conditioned_uqi(lib):
    """UQI's s_xx - N m^2 on a nearly constant slice.  On the grid the sums are exact: the closed form at 1e-12, the oracle's
    two-pass float32 UQI at 1e-5.  Off the grid (uniform noise of 1e-3): against a float64 two-pass UQI at the suite's 1e-5, with
    the oracle's own distance printed beside it."""
    from cta_gan_amd import ops
    fake, real, wc, ww = R.ill_conditioned_slice()
    fake6, real6 = R.ill_conditioned_slice(seed=6)[:2]
    f2, r2 = np.stack([fake, fake6]), np.stack([real, real6])
    wcv, wwv = np.full(2, wc, np.float32), np.full(2, ww, np.float32)
    nblk = R.ops_nblk(fake.size)
    planes = _oracle_planes(f2, r2, wcv, wwv, 0)
    assert np.array_equal(planes[1], f2) and np.array_equal(planes[3], r2)
    ref = [R.part_ref(planes[:, i], nblk) for i in range(2)]
    want, S, n = np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref]), ref[0][2]
    R.assert_exact_domain(S)                                            # the windowed pair is all ones: everything is exact
    part, out = _run_metrics(lib, f2, r2, wcv, wwv, nblk, 0)
    _same_bits(part, want, "part")
    for i in range(2):
        cf = R.final_ref(_seq_sum(want)[i].reshape(2, 10), fake.size)
        assert _rel_close(out[i], cf, 1e-12, 1e-12), (i, out[i], cf)
        o32 = float(ref_metrics.uqi(f2[i].reshape(128, 128), r2[i].reshape(128, 128)))
        t64 = R.uqi_two_pass_f64(f2[i], r2[i])
        assert _rel_close(out[i, 1, 2], o32, 1e-5, 1e-9) and _rel_close(out[i, 1, 2], t64, 1e-12, 1e-12), (out[i, 1, 2], o32, t64)
        assert 0.5 < out[i, 1, 2] < 0.95 and out[i, 0, 2] == 0.0
    fake, real, wc, ww = R.ill_conditioned_slice(noise=1e-3)
    got = ops.window_metrics(_dev(fake[None]), _dev(real[None]), wc, ww).cpu().numpy()[0, 1, 2]
    t64 = R.uqi_two_pass_f64(fake, real)
    o32 = float(ref_metrics.uqi(fake.reshape(128, 128), real.reshape(128, 128)))
    print("off-grid UQI: float64 two-pass %.12f; kernel off by %.3e, the oracle's float32 two-pass by %.3e (relative)"
          % (t64, abs(got - t64) / abs(t64), abs(o32 - t64) / abs(t64)))
    assert abs(got - t64) <= 1e-5 * abs(t64), (got, t64, o32)


def test_window_metrics_ill_conditioned_windowed_pair(lib):
    """A nearly constant windowed pair of level / 255 values (levels 200 and 201): sums that are not exact, and a UQI that
    amplifies their relative error by kappa = 2e7 (windowed) and 1e9 (raw; metrics_ref.uqi_condition).  `part` within
    gamma64 S of the correctly rounded reference (fp32 per-thread sums are 1e-7 S away: 2e5 times the bound); UQI of both pairs
    against the float64 two-pass value at the suite's 1e-5; `out` against the closed forms of the reference sums: MAE and PSNR
    at 1e-12, UQI at 1e-12 + 4 kappa (gamma64(n) + 4 u) -- each of the three moments is a difference of two numbers that carry
    the relative error gamma64(n) of a sum and the roundings of the closed form itself (the device may contract N m m into
    the subtraction, numpy does not), amplified by kappa, and UQI holds two of them."""
    from cta_gan_amd import ops
    fake, real, wc, ww = R.ill_conditioned_windowed_slice()
    fake7, real7 = R.ill_conditioned_windowed_slice(seed=8)[:2]
    f2, r2 = np.stack([fake, fake7]), np.stack([real, real7])
    wcv, wwv = np.full(2, wc, np.float32), np.full(2, ww, np.float32)
    nblk = ops.window_metrics_nblk(fake.size)
    assert nblk == R.ops_nblk(fake.size) == 4
    planes = _oracle_planes(f2, r2, wcv, wwv, 0)
    assert set(np.unique(R.levels_of(planes[0]))) == {200, 201} and set(np.unique(R.levels_of(planes[2]))) == {200, 201}
    assert np.array_equal(planes[1], f2) and np.array_equal(planes[3], r2)
    ref = [R.part_ref(planes[:, i], nblk) for i in range(2)]
    want, S, n = np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref]), ref[0][2]
    part, out = _run_metrics(lib, f2, r2, wcv, wwv, nblk, 0)
    e = np.zeros(20, bool)
    e[[0, 10]] = True                                                   # only the counts are exact here
    worst = _check_part(part, want, S, n, e, "ill-conditioned windowed")
    _same_bits(ops.window_metrics(_dev(f2), _dev(r2), wc, ww).cpu().numpy(), out, "ops.window_metrics")
    sums = _seq_sum(want)
    for i in range(2):
        cf = R.final_ref(sums[i].reshape(2, 10), fake.size)
        for p, (x, y) in enumerate(((planes[0, i], planes[2, i]), (planes[1, i], planes[3, i]))):
            kappa = R.uqi_condition(sums[i].reshape(2, 10)[p], fake.size)
            bound = 1e-12 + 4 * kappa * (float(R.gamma64(n.max())) + 4 * R.U64)
            t64 = R.uqi_two_pass_f64(x, y)
            o32 = float(ref_metrics.uqi(x.reshape(128, 128), y.reshape(128, 128)))
            print("slice %d pair %d: kappa %.2e; UQI off the closed form of the reference sums by %.2e (bound %.2e), off the float64 "
                  "two-pass value by %.2e (the oracle's float32: %.2e); sums at most %.3f of gamma64 S"
                  % (i, p, kappa, abs(out[i, p, 2] - cf[p, 2]) / abs(cf[p, 2]), bound, abs(out[i, p, 2] - t64) / abs(t64),
                     abs(o32 - t64) / abs(t64), worst))
            assert kappa > 1e7 and 0.3 < t64 < 0.95
            assert _rel_close(out[i, p, :2], cf[p, :2], 1e-12, 1e-12), (i, p, out[i, p], cf[p])
            assert abs(out[i, p, 2] - cf[p, 2]) <= bound * abs(cf[p, 2]), (i, p, out[i, p, 2], cf[p, 2], bound)
            assert abs(out[i, p, 2] - t64) <= 1e-5 * abs(t64), (i, p, out[i, p, 2], t64)


@pytest.mark.parametrize("aliased", [0, 1])
def test_window_metrics_nan_propagates(lib, aliased):
    """One NaN pixel of `fake` inside the foreground.  PSNR and UQI are NaN as in the oracle; MAE is NaN where the oracle's
    nanmean is finite -- deliberate: a diverged generator must not report a finite MAE.  The other slices
    of the batch are untouched by it."""
    case = R.Case("nan", 3, 300, 2)
    fake, real, wc, ww, planes, want, S, n = R.case_reference(case, aliased)
    _, clean = _run_metrics(lib, fake, real, wc, ww, 2, aliased)
    fake = fake.copy()
    fake[1, 0] = np.nan                                                 # real[:, 0] = 0.75: foreground under every window
    part, out = _run_metrics(lib, fake, real, wc, ww, 2, aliased)
    o = R.oracle_metrics(fake[1][None], real[1][None], float(wc[1]), float(ww[1]), aliased)
    assert np.isfinite(o[:, 0]).all() and np.isnan(o[:, 1:]).all(), o
    assert np.isnan(out[1]).all(), out[1]
    _same_bits(out[[0, 2]], clean[[0, 2]], "the slices beside the NaN slice")
    assert np.isnan(part[1, 0]).sum() > 0 and not np.isnan(part[1, 1]).any() and not np.isnan(part[[0, 2]]).any()   # pixel 0 is block 0's


# ============================================================================ 3. SSIM
SSIM_SIZES = ((7, 7), (7, 200), (22, 22), (23, 22), (38, 39), (21, 134))


def _ssim_nblk(h, w):
    return ((h - 6 + 15) // 16) * ((w - 6 + 15) // 16)


def _run_ssim(lib, fake, real, wc, ww, mode, aliased, data_range=2.0):
    """fake, real [B, H, W] -> out [B, npair]; part slot 1 in mode 0 and both guards keep the sentinel."""
    b, h, w = fake.shape
    nblk, npair = _ssim_nblk(h, w), 2 if mode else 1
    part, out = _dbuf(b * nblk * 2), _dbuf(b * npair)
    wcp = None if wc is None else _dev(np.asarray(wc, np.float32))
    wwp = None if ww is None else _dev(np.asarray(ww, np.float32))
    d_f, d_r = _dev(fake), _dev(real)
    st = lib.ctg_ssim(d_f.data_ptr(), d_r.data_ptr(), None if wcp is None else wcp.data_ptr(),
                      None if wwp is None else wwp.data_ptr(), b, h, w, mode, int(aliased), float(data_range), part.data_ptr(),
                      out.data_ptr(), _st())
    assert st == 0, st
    assert _untouched_d(part, b * nblk * 2) and _untouched_d(out, b * npair), "ctg_ssim wrote behind a buffer"
    p = part[:b * nblk * 2].cpu().numpy().reshape(b, nblk, 2)
    assert not np.isnan(p[:, :, :npair]).any(), "unwritten block partials"
    if not mode:
        assert np.isnan(p[:, :, 1]).all(), "mode 0 wrote slot 1 of `part`"
    o = out[:b * npair].cpu().numpy().reshape(b, npair)
    # consistency of the launch's two outputs only (no coverage of ssim_final_kernel: the oracle comparisons of the callers are):
    # the block partials add up to out * count
    assert np.allclose(p[:, :, :npair].sum(1), o * ((h - 6) * (w - 6)), rtol=1e-12, atol=1e-12)
    return o


@pytest.mark.parametrize("size", SSIM_SIZES, ids=lambda s: "%dx%d" % s)
def test_ssim_sizes(lib, size):
    from cta_gan_amd import ops
    h, w = size
    rng = np.random.default_rng([h, w])
    x = np.stack([R.grid_images([h, w, 1], (h, w)), rng.uniform(-1, 1, (h, w)).astype(np.float32)])
    y = np.stack([R.grid_images([h, w, 2], (h, w)), (x[1] + 0.2 * rng.standard_normal((h, w))).astype(np.float32)])
    for dr in (2.0, 1.0, 255.0):
        got = _run_ssim(lib, x, y, None, None, 0, 0, dr)
        for i in range(2):
            assert got[i, 0] == pytest.approx(ref_metrics.ssim(x[i], y[i], data_range=dr), rel=1e-9, abs=1e-12), (size, dr, i)
            assert got[i, 0] == pytest.approx(ref_metrics.ssim_bruteforce(x[i], y[i], data_range=dr), rel=1e-9, abs=1e-12), (size, dr, i)
        _same_bits(ops.ssim(_dev(x), _dev(y), data_range=dr).cpu().numpy(), got[:, 0], "ops.ssim")
    # constant pairs: (2ab + C1) / (a^2 + b^2 + C1), identical pairs: 1
    a, b = np.full((2, h, w), 0.25, np.float32), np.full((2, h, w), -0.5, np.float32)
    b[1] = 0.25
    for dr in (2.0, 0.5):
        c1 = (0.01 * dr) ** 2
        got = _run_ssim(lib, a, b, None, None, 0, 0, dr)
        assert got[0, 0] == pytest.approx((2 * 0.25 * -0.5 + c1) / (0.25 ** 2 + 0.5 ** 2 + c1), rel=1e-9)
        assert got[1, 0] == pytest.approx(1.0, abs=1e-12)


@pytest.mark.parametrize("B", [65, 130])
def test_ssim_mode0_batches(lib, B):
    rng = np.random.default_rng(B)
    x = rng.uniform(-1, 1, (B, 23, 22)).astype(np.float32)
    y = (x + rng.uniform(0.05, 0.5, (B, 1, 1)) * rng.standard_normal(x.shape)).astype(np.float32)
    got = _run_ssim(lib, x, y, None, None, 0, 0)
    want = np.array([ref_metrics.ssim(x[i], y[i]) for i in range(B)])
    assert np.unique(np.round(want, 6)).size == B                       # every row is its own number
    for i in range(B):
        assert got[i, 0] == pytest.approx(want[i], rel=1e-9, abs=1e-12), i


@pytest.mark.parametrize("aliased", [0, 1])
def test_ssim_mode1_batch(lib, aliased):
    from cta_gan_amd import ops
    B = 33
    rng = np.random.default_rng(33)
    real = rng.uniform(-1, 1, (B, 23, 22)).astype(np.float32)
    fake = np.clip(real + rng.uniform(0.02, 0.3, (B, 1, 1)) * rng.standard_normal(real.shape), -1, 1).astype(np.float32)
    real[:, :5] = -1
    wc, ww = R.case_windows(B)
    got = _run_ssim(lib, fake, real, wc, ww, 1, aliased)
    for i in range(B):
        want = ref_metrics.slice_ssim(fake[i].copy(), real[i].copy(), float(wc[i]), float(ww[i]), aliased=bool(aliased))
        assert np.allclose(got[i], want, rtol=1e-9, atol=1e-12), (i, got[i], want)
    _same_bits(ops.window_ssim(_dev(fake), _dev(real), wc.tolist(), ww.tolist(), aliased=bool(aliased)).cpu().numpy(), got, "ops.window_ssim")


# ============================================================================ 4. input pipeline
def _run_hu(lib, hu, wc, ww):
    n = hu.size
    win, full = _fbuf(n), _fbuf(n)
    d_hu = _dev(hu)
    st = lib.ctg_hu_to_inputs(d_hu.data_ptr(), float(wc), float(ww), win.data_ptr(), full.data_ptr(), n, _st())
    assert st == 0, st
    assert _untouched_f(win, n) and _untouched_f(full, n), "ctg_hu_to_inputs wrote behind an output"
    return win[:n].cpu().numpy(), full[:n].cpu().numpy()


@pytest.mark.parametrize("win", R.WINDOWS, ids=lambda w: "%g_%g" % w)
def test_hu_to_inputs_whole_int16_domain(lib, win):
    hu = R.hu_sweep()
    i1, i2 = R.hu_reference(hu, *win)
    g1, g2 = _run_hu(lib, hu, *win)
    _same_bits(g1, i1, "windowed image (hu = index - 32768 below 65536)")
    _same_bits(g2, i2, "full-range image (hu = index - 32768 below 65536)")


def test_hu_to_inputs_second_trip(lib):
    hu = R.hu_sweep()
    wc, ww = R.WINDOWS[0]
    i1, i2 = R.hu_reference(hu, wc, ww)
    n = 4096 * 256 + 300
    idx = np.arange(n) % hu.size
    g1, g2 = _run_hu(lib, hu[idx], wc, ww)
    _same_bits(g1, i1[idx], "windowed image")
    _same_bits(g2, i2[idx], "full-range image")


RGUARD = 64


def _resize_cases(lib, shapes, B=2):
    """shapes: (Hi, Wi, Ho, Wo).  All launches go out first, on arange planes; one copy back; every destination is followed by
    RGUARD sentinel elements.  Reference: F.interpolate(mode='nearest') on the CPU."""
    import torch.nn.functional as F
    srcs, offs, so, do = [], [], 0, 0
    for hi, wi, ho, wo in shapes:
        src = (np.arange(B * hi * wi, dtype=np.float32)).reshape(B, hi, wi)
        srcs.append(src)
        offs.append((so, do))
        so += src.size
        do += B * ho * wo + RGUARD
    dsrc = _dev(np.concatenate([s.reshape(-1) for s in srcs]))
    dst = torch.full((do,), SENT, dtype=torch.float32, device="cuda")
    for (hi, wi, ho, wo), (s0, d0) in zip(shapes, offs):
        st = lib.ctg_resize_nearest(dsrc.data_ptr() + 4 * s0, B, hi, wi, dst.data_ptr() + 4 * d0, ho, wo, _st())
        assert st == 0, (st, hi, wi, ho, wo)
    got = dst.cpu().numpy()
    for (hi, wi, ho, wo), (s0, d0), src in zip(shapes, offs, srcs):
        want = F.interpolate(torch.from_numpy(src)[None], size=[ho, wo]).squeeze(0).numpy()
        g = got[d0:d0 + B * ho * wo].reshape(B, ho, wo)
        if not np.array_equal(g, want):
            bad = np.argwhere(g != want)[0]
            raise AssertionError("resize %dx%d -> %dx%d: plane %d output (%d, %d) reads source element %g, F.interpolate %g"
                                 % (hi, wi, ho, wo, bad[0], bad[1], bad[2], g[tuple(bad)], want[tuple(bad)]))
        assert np.all(got[d0 + B * ho * wo:d0 + B * ho * wo + RGUARD] == SENT), "resize %dx%d -> %dx%d wrote behind its output" % (hi, wi, ho, wo)


def test_resize_nearest_every_pair_up_to_24(lib):
    """(n_in, n_out) along H and the same pair transposed along W in one launch: 576 launches of B = 2 planes."""
    _resize_cases(lib, [(a, b, b, a) for a in range(1, 25) for b in range(1, 25)])


def test_resize_nearest_large_and_single(lib):
    _resize_cases(lib, [(3, 5, 725, 725), (512, 512, 256, 256), (256, 256, 512, 512), (7, 9, 1, 1), (5, 5, 1, 8), (6, 4, 9, 1)])
    assert 725 * 725 > 2048 * 256


# ============================================================================ 5. refusals
def test_refusals_leave_the_outputs_alone(lib):
    st = _st()
    f32 = torch.zeros(4096, dtype=torch.float32, device="cuda")
    i16 = torch.zeros(4096, dtype=torch.int16, device="cuda")
    win = torch.full((8,), 40.0, dtype=torch.float32, device="cuda")
    wid = torch.full((8,), 400.0, dtype=torch.float32, device="cuda")
    outf, outf2, part, outd = _fbuf(4096), _fbuf(4096), _dbuf(4096), _dbuf(64)
    F, W1, W2, OF, OF2, P, OD, HU = (t.data_ptr() for t in (f32, win, wid, outf, outf2, part, outd, i16))
    nan = float("nan")
    calls = {
        "to_windowdata": (lib.ctg_to_windowdata, [F, W1, W2, OF, 2, 64, st], (0, 1, 2, 3),
                          [{4: 0}, {4: 65536}, {5: 0}]),
        "window_metrics": (lib.ctg_window_metrics, [F, F, W1, W2, 2, 64, 1, 0, P, OD, st], (0, 1, 2, 3, 8, 9),
                           [{4: 0}, {4: 65536}, {5: 1}, {6: 0}, {6: 4097}]),
        "window_pairs": (lib.ctg_window_pairs, [F, F, W1, W2, 2, 64, 0, OF, st], (0, 1, 2, 3, 7),
                         [{4: 0}, {4: 65536}, {5: 0}]),
        "ssim mode 0": (lib.ctg_ssim, [F, F, None, None, 2, 8, 8, 0, 0, 2.0, P, OD, st], (0, 1, 10, 11),
                        [{4: 0}, {4: 65536}, {5: 6}, {6: 6}, {7: 2}, {7: -1}, {9: 0.0}, {9: nan}, {9: -2.0}]),
        "ssim mode 1": (lib.ctg_ssim, [F, F, W1, W2, 2, 8, 8, 1, 0, 2.0, P, OD, st], (0, 1, 2, 3, 10, 11),
                        [{2: None, 3: None}, {4: 65536}, {5: 6}, {9: nan}]),
        "hu_to_inputs": (lib.ctg_hu_to_inputs, [HU, 50.0, 400.0, OF, OF2, 64, st], (0, 3, 4),
                         [{2: 0.0}, {2: -1.0}, {5: 0}]),
        "resize_nearest": (lib.ctg_resize_nearest, [F, 2, 4, 4, OF, 4, 4, st], (0, 4),
                           [{1: 0}, {2: 0}, {3: 0}, {5: 0}, {6: 0}]),
    }
    count = 0
    for name, (fn, good, ptrs, bad) in calls.items():
        for k in ptrs:
            bad = bad + [{k: None}]
        for change in bad:
            args = list(good)
            for k, v in change.items():
                args[k] = v
            assert fn(*args) == EINVAL, (name, change)
            count += 1
        assert fn(*good) == 0, name                        # the unchanged call is a valid one: each refusal is due to its change
        torch.cuda.synchronize()
        for t in (outf, outf2):
            t.fill_(SENT)
        for t in (part, outd):
            t.fill_(nan)
    # every refusal once more on clean buffers: nothing was written
    for name, (fn, good, ptrs, bad) in calls.items():
        for change in bad + [{k: None} for k in ptrs]:
            args = list(good)
            for k, v in change.items():
                args[k] = v
            assert fn(*args) == EINVAL, (name, change)
    torch.cuda.synchronize()
    assert _untouched_f(outf) and _untouched_f(outf2) and _untouched_d(part) and _untouched_d(outd)
    assert count >= 60
