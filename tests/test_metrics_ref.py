"""CPU: the helpers and case lists of tests/metrics_ref.py, which tests/test_metrics_exact_gpu.py compares the kernels of
csrc/metrics.hip with.  A case of the GPU module that is broken (outside the exact domain, a mask that is all one kind, a level that
never occurs) fails HERE, without a card."""
import numpy as np
import pytest

import metrics_ref as R
from oracle import ref_metrics


@pytest.mark.parametrize("win", R.WINDOWS, ids=lambda w: "%g_%g" % w)
def test_boundary_set_tells_a_fused_and_a_float64_window_from_the_oracle(win):
    """What the level-boundary set is worth: a window evaluation with `h * 4095 - 1024` contracted into one rounding and one in
    float64 must both differ from the oracle on it; uniformly random values of the same count do not show the contraction."""
    wc, ww = win
    s = R.boundary_set(wc, ww)
    assert s.size == 2313 and s.dtype == np.float32
    want = R.oracle_window(s, wc, ww)
    fused = int((R.window_fused(s, wc, ww) != want).sum())
    f64 = int((R.window_f64(s, wc, ww) != want).sum())
    rnd = np.random.default_rng(1).uniform(-1, 1, s.size).astype(np.float32)
    fused_rnd = int((R.window_fused(rnd, wc, ww) != R.oracle_window(rnd, wc, ww)).sum())
    print("window %s: fused differs on %d, float64 on %d of 2313 boundary values; fused on %d of 2313 random values"
          % (win, fused, f64, fused_rnd))
    assert 12 <= fused <= 87, fused           # measured here: 87, 84, 12, 82 for the four windows
    assert f64 > 1200, f64
    assert fused_rnd == 0
    assert set(R.levels_of(want).tolist()) == set(range(256))


@pytest.mark.parametrize("aliased", [False, True])
@pytest.mark.parametrize("win", R.WINDOWS, ids=lambda w: "%g_%g" % w)
def test_elementwise_pair_meets_every_mask_combination(win, aliased):
    """The (fake, real) pair of the elementwise GPU cases: every combination of (foreground, background) of W(real) with
    (foreground, background) of W(fake) occurs, and so does every rule of masked_pixel: c == 0 -> -1 under a foreground bb,
    fake_m == 0 -> -1 (a zero sample under cc = 1 needs a window whose level at 0 is foreground: none of the four; the rule is
    met by the zero PRODUCT under cc = 0), real_m of -0.0."""
    wc, ww = win
    fake, real = R.elementwise_pair(wc, ww)
    assert fake.size == real.size == 2355
    wf, wr = R.oracle_window(fake, wc, ww) >= 0.3, R.oracle_window(real, wc, ww) >= 0.3
    for a in (False, True):
        for b in (False, True):
            assert int(((wf == a) & (wr == b)).sum()) >= 20, (a, b)
    c, fake_m, b, real_m = R.oracle_pairs(fake[None], real[None], wc, ww, aliased)[:, 0]
    assert (b == -1).any() and (b != -1).any() and (c == -1).any() and (c != -1).any()
    assert ((c == -1) & (b != -1)).any()               # cc = 0 under bb = 1
    assert ((fake_m == -1) & (fake != -1)).any() and ((real_m == -1) & (real != -1)).any()
    if aliased:
        assert set(np.unique(c)) == {-1.0, 1.0} and set(np.unique(b)) == {-1.0, 1.0}


def test_special_values():
    s = R.special_values()
    assert s.size == 42 and np.signbit(s[3]) and s[3] == 0 and s[1] > -1 and s[1] == np.nextafter(np.float32(-1), np.float32(0))
    g = R.grid_values()
    assert g.size == 33 and g[0] == -1 and g[-1] == 1 and np.all(np.diff(g) == 2.0 ** -4)


def test_block_shares():
    for hw, nblk in ((2, 1), (255, 1), (257, 1), (1000, 4096), (3841, 5), (12365, 3), (300, 2)):
        n = R.share_sizes(hw, nblk)
        want = np.zeros(nblk, int)
        for i in range(hw):
            want[(i // 256) % nblk] += 1
        assert np.array_equal(n, want) and n.sum() == hw
    assert R.share_sizes(1000, 4096)[4:].sum() == 0 and list(R.share_sizes(3841, 5)) == [769, 768, 768, 768, 768]
    assert R.ops_nblk(4096 * 3 + 77) == 3 and R.ops_nblk(100) == 1 and R.ops_nblk(512 * 512) == 64


@pytest.mark.parametrize("aliased", [False, True])
@pytest.mark.parametrize("case", R.REDUCTION_CASES + R.BATCH_CASES, ids=lambda c: c.name)
def test_reduction_cases_are_exact_and_mixed(case, aliased):
    """Every case of the GPU module: the exact sums lie in the exact domain of fp32 (so the argument holds for any accumulation
    width), are multiples of the granule, every slice is part foreground, B >= 2 with more than one window."""
    fake, real, wc, ww, planes, part, S, n = R.case_reference(case, aliased)
    assert case.B >= 2 and len({(a, b) for a, b in zip(wc.tolist(), ww.tolist())}) >= 2
    e = R.exact_columns(aliased)
    R.assert_exact_domain(S[:, :, e])
    assert np.array_equal(part[:, :, e] / R.GRANULE, np.rint(part[:, :, e] / R.GRANULE))
    nm = part[:, :, (0, 10)].sum(1)                           # foreground pixels per slice and pair
    assert np.all(nm > 0) and np.all(nm < case.HW), nm
    assert n.sum() == case.HW and part.shape == (case.B, R.case_nblk(case), 20)
    assert np.all(part[:, n == 0] == 0)
    if not aliased and case.HW >= 255:
        assert not np.array_equal(part[:, :, 1:10] / R.GRANULE, np.rint(part[:, :, 1:10] / R.GRANULE))     # the inexact sums are inexact


def test_part_ref_and_final_ref_reproduce_the_oracles_metrics():
    """Blocks add up to the slice; the closed forms on the float64 sums give the oracle's slice_metrics (float32 numpy) at the
    suite's 1e-5, both aliasing variants -- random off-grid images, so this pins the term definitions, not the exact domain."""
    rng = np.random.default_rng(11)
    hw = 37 * 41
    real = rng.uniform(-1, 1, (37, 41)).astype(np.float32)
    fake = np.clip(real + 0.1 * rng.standard_normal(real.shape), -1, 1).astype(np.float32)
    real[:5] = -1
    for aliased in (False, True):
        planes = R.oracle_pairs(fake, real, 40.0, 400.0, aliased).reshape(4, -1)
        p1, S1, _ = R.part_ref(planes, 1)
        p7, S7, n7 = R.part_ref(planes, 7)
        assert np.all(np.abs(p7.sum(0) - p1[0]) <= 1e-13 * S1[0]) and np.allclose(S7.sum(0), S1[0], rtol=1e-13) and n7.sum() == hw
        assert np.all(S1 * (1 + 1e-12) >= np.abs(p1))             # (S is a numpy sum, the sums are correctly rounded)
        got = R.final_ref(p1[0].reshape(2, 10), hw)
        want = R.oracle_metrics(fake, real, 40.0, 400.0, aliased)
        assert np.all(np.abs(got - want) <= 1e-5 * np.abs(want) + 1e-9), (got, want)


def test_final_ref_all_background_and_nan():
    real = np.full((4, 5), -1.0, np.float32)
    fake = R.grid_images(2, (4, 5))
    planes = R.oracle_pairs(fake, real, 50.0, 400.0, False).reshape(4, -1)
    p, _, _ = R.part_ref(planes, 1)
    assert p[0, 0] == 0 and p[0, 10] == 0
    got, want = R.final_ref(p[0].reshape(2, 10), 20), R.oracle_metrics(fake, real, 50.0, 400.0, False)
    assert np.all(np.abs(got - want) <= 1e-5 * np.abs(want) + 1e-9), (got, want)
    # one NaN pixel in the foreground: the oracle's nanmean MAE is finite, the closed forms (plain sums) give NaN -- the
    # deliberate difference
    real = np.full((4, 5), 0.75, np.float32)
    fake = np.full((4, 5), 0.5, np.float32)
    fake[1, 2] = np.nan
    planes = R.oracle_pairs(fake, real, 50.0, 400.0, False).reshape(4, -1)
    p, _, _ = R.part_ref(planes, 1)
    got, want = R.final_ref(p[0].reshape(2, 10), 20), R.oracle_metrics(fake, real, 50.0, 400.0, False)
    assert np.isfinite(want[1, 0]) and np.isnan(want[1, 1:]).all()
    assert np.isnan(got[1]).all()


def test_gamma_and_exact_domain():
    assert R.gamma(256) == pytest.approx(258 * 2.0 ** -24, rel=1e-4)
    R.assert_exact_domain(np.array([2.0 ** 16 - 2.0 ** -8]))
    with pytest.raises(AssertionError):
        R.assert_exact_domain(np.array([2.0 ** 16]))
    # the bound is a bound: fp32 sums of fp32 terms in two orders, against float64
    rng = np.random.default_rng(4)
    t = rng.uniform(-1, 1, 5000).astype(np.float32)
    exact, S = t.astype(np.float64).sum(), np.abs(t.astype(np.float64)).sum()
    fwd = np.float32(0)
    for v in t:
        fwd = np.float32(fwd + v)
    assert abs(float(fwd) - exact) <= R.gamma(t.size) * S and abs(float(t.sum(dtype=np.float32)) - exact) <= R.gamma(t.size) * S


def test_gamma64_and_the_windowed_ill_conditioned_slice():
    """gamma64 is a bound for double sums against the correctly rounded reference and far below the fp32 bound; the nearly
    constant windowed pair has levels 200 / 201 only, no background, is badly conditioned, and its closed form on the reference
    sums is the float64 two-pass UQI within 4 kappa (gamma64 + 4 u) -- while fp32 per-thread sums would miss `part`'s bound."""
    assert R.gamma64(4096) == pytest.approx(4097 * 2.0 ** -53, rel=1e-9) and R.gamma64(4096) * 2 ** 28 < R.gamma(4096)
    fake, real, wc, ww = R.ill_conditioned_windowed_slice()
    planes = R.oracle_pairs(fake[None], real[None], wc, ww, False)[:, 0]
    assert set(np.unique(R.levels_of(planes[0]))) == {200, 201} and set(np.unique(R.levels_of(planes[2]))) == {200, 201}
    assert np.array_equal(planes[1], fake) and np.array_equal(planes[3], real)
    assert 0 < (fake != fake[0]).sum() <= 12 and (planes[2] != -1).all()
    part, S, n = R.part_ref(planes, R.ops_nblk(fake.size))
    assert part.shape == (4, 20) and np.all(n == 4096)
    # a float64 numpy sum in another order is inside the bound; a float32 accumulation of the same terms is far outside
    terms = np.concatenate([R.pair_terms(planes[0], planes[2]), R.pair_terms(planes[1], planes[3])])
    blk = R.block_index(fake.size, 4)
    for b in range(4):
        sel = terms[:, blk == b]
        assert np.all(np.abs(sel[:, ::-1].sum(1) - part[b]) <= R.gamma64(4096) * S[b])
        f32 = sel.astype(np.float32).cumsum(1, dtype=np.float32)[:, -1].astype(np.float64)
        assert (np.abs(f32 - part[b]) > R.gamma64(4096) * S[b])[[5, 6, 7, 8, 9, 15, 16, 17, 18, 19]].all()
    sums = part.sum(0).reshape(2, 10)
    cf = R.final_ref(sums, fake.size)
    for p, (x, y) in enumerate(((planes[0], planes[2]), (planes[1], planes[3]))):
        kappa = R.uqi_condition(sums[p], fake.size)
        t64 = R.uqi_two_pass_f64(x, y)
        assert kappa > 1e7 and 0.3 < t64 < 0.95
        assert abs(cf[p, 2] - t64) <= (1e-12 + 4 * kappa * (R.gamma64(4096) + 4 * R.U64)) * abs(t64) and abs(cf[p, 2] - t64) <= 1e-5 * abs(t64)
    fake, real, wc, ww, planes, part, S, n = R.case_reference(R.REDUCTION_CASES[4], False)          # an ordinary case: well conditioned
    assert R.uqi_condition(part[0].sum(0)[:10], fake.shape[1]) < 100


def test_ill_conditioned_slice():
    """On the grid: the raw pair is the pair (the window makes everything foreground), the closed form on exact sums is the
    float64 two-pass UQI at 1e-12 and the oracle's float32 two-pass UQI at 1e-5.  Off the grid the numbers the GPU module's
    docstring quotes: the oracle's own distance from the float64 value."""
    fake, real, wc, ww = R.ill_conditioned_slice()
    planes = R.oracle_pairs(fake[None], real[None], wc, ww, False)[:, 0]
    assert np.array_equal(planes[1], fake) and np.array_equal(planes[3], real) and np.all(planes[0] == 1) and np.all(planes[2] == 1)
    assert abs(float(fake.mean()) + 0.9) < 0.03 and 0 < (fake != -0.875).sum() <= 12
    p, S, _ = R.part_ref(planes, R.ops_nblk(fake.size))
    R.assert_exact_domain(S)
    got = R.final_ref(p.sum(0).reshape(2, 10), fake.size)[1, 2]
    t64 = R.uqi_two_pass_f64(fake, real)
    o32 = float(ref_metrics.uqi(fake.reshape(128, 128), real.reshape(128, 128)))
    assert got == pytest.approx(t64, rel=1e-12) and got == pytest.approx(o32, rel=1e-5) and 0.5 < got < 0.9
    fake, real, wc, ww = R.ill_conditioned_slice(noise=1e-3)
    t64 = R.uqi_two_pass_f64(fake, real)
    o32 = float(ref_metrics.uqi(fake.reshape(128, 128), real.reshape(128, 128)))
    print("off-grid: float64 two-pass UQI %.12f, oracle (float32 two-pass) off by %.2e relative" % (t64, abs(o32 - t64) / abs(t64)))
    assert abs(o32 - t64) <= 1e-5 * abs(t64)


@pytest.mark.parametrize("win", R.WINDOWS, ids=lambda w: "%g_%g" % w)
def test_hu_sweep_reference(win):
    hu = R.hu_sweep()
    assert hu.dtype == np.int16 and hu.size == 65536 + 77 and hu.size % 256 != 0
    assert np.array_equal(hu[:65536], np.arange(-32768, 32768))
    i1, i2 = R.hu_reference(hu, *win)
    assert set(R.levels_of(i1).tolist()) == set(range(256))
    # 0 .. 32767 stored values: everything below -1024 is 0, and so is everything above 31743 (the reference's int16 `+ 1024` wraps)
    assert np.unique(i2).size == 32768
    assert np.all(i2[hu < -1024] == -1) and np.all(i2[hu > 31743] == -1) and i2.max() == i2[hu == 31743][0]


def test_first_diff():
    a = np.array([0.0, 1.0, np.nan, -0.0], np.float32)
    assert R.first_diff(a, a.copy()) is None
    b = a.copy()
    b[3] = 0.0
    assert "first at 3" in R.first_diff(a, b)
