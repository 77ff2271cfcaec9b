"""GPU: the seven sliding-window ("strip") conv kernels, bit for bit, against tests/conv_ref.py on integer-grid operands.

Exactness argument (as in tests/test_conv_exact_gpu.py).  Operands are small integers (bf16 kernels: |x|, |w| <= 4 for the 32 -> 32
kernel, <= 3 for the others, <= 2 for the weights of the 128 -> 256 kernel; split pair: integers of magnitude 1 .. 2 plus
{-1, 0, 1} 2^-10), biases multiples of 1/8.  Every product and partial sum is a multiple of the granule (1, resp. 2^-10); while
S = the sum of the terms' magnitudes stays below 2^24 granules, fp32 accumulation is exact in ANY order, so the kernel has to
reproduce the float64 reference bit for bit, on every sample, band and strip: a dropped, duplicated or misplaced tap, a row
read before its DMA has landed, a mis-reflected column is an integer difference at a known element.  The bound
max|x| max|w| taps Cin >= S goes through assert_exact_domain BEFORE anything is launched, and so does every slab's sum of
squares before the bf16 moments are compared (they are sums of non-negative integers: their value is their S).  The dense
operand ranges above keep the squares in the domain at the longest bands of the default plan (largest slab: 1.2e7 of 1.7e7), so
one launch serves outputs and moments; every tap and input channel carries non-zero weights into every 16-channel output tile
(asserted), and about 1 % (32 -> 32), 0.05 % (transposed), 0.3 % (stride 2) of the outputs are no bf16 values, so the store's
rounding is exercised.  bias + ReLU / LeakyReLU is one fp32 add and one fp32 multiply by 0.2f: exact against conv_ref.epilogue.

The reference is float64 torch conv2d / conv_transpose2d on the CPU over explicitly padded input (conv_ref.conv3x3_f64,
convT3x3_f64, pair_f64; tests/test_conv_ref.py shows them equal to conv_taps_ref / conv_classes_ref / conv_pair_ref), computed
once per test and shared by its launches.  The thresholds (B H W >= 2^20, 2^18, 2^17) are met with many small samples, so the
edges sit at the smallest maps the launchers accept.

What every case does.  (1) The band plan of the launcher is mirrored in Python (conv_ref.band_plan / strip_plan with the
card's CU count) and the case ASSERTS that the plan is the edge it is named for before anything is launched -- a miss is a
failure that prints the CU count, never a skip.  (2) A launch without bias / activation and want_stats=True: the slab count must
be nbands x nstrips (2 x for the split-pair transposed kernel) -- a count the halo and gather kernels do not give, hence the
evidence that the strip kernel ran AND that its plan is the mirror's -- and within ops.moments_slabs.  (3) The output is the
channel slice of a sentinel buffer with 4096 guard elements behind the last sample; the WHOLE buffer is compared on its bits
(torch int16 views) with store_bf16 / store_pair of the reference: every sample, and everything the launch must not write.
(4) bf16 moments: every partial, slab by slab, exact, against the moments of that slab's pixels (conv_ref.band_slabs: slab =
band * nstrips + strip; a transposed slab holds the four parity classes of its input pixels) -- this shows the band and strip a
pixel was counted in and that the masked columns of a ragged strip count as zero.  Split-pair moments have squares that are
multiples of 2^-20, not exact in fp32: slab count, then ops.in_finalize against float64 mean / rstd of the exact pre-rounding
result at rtol 1e-5, atol 1e-6.  (5) A second launch: without moments (the same bits), or -- the 32 -> 32 kernel's epilogue
configurations -- with bias and activation and want_stats=True, which must return no moments.  Failure messages name sample,
band, row of the band, strip, column of the strip, parity class, 16-channel tile, plane, or "OUTSIDE the output slice" / guard.

Cases and the plan each reached on the MI355X (256 CUs), band_rows x nbands (rows of the last band), strips (columns of the last):
  conv_strip32_kernel        1024 x 32 x 32     32 x 1,        2 (16)   smallest map, two full strips
    (each in 4 configurations: 64 x 65 x 255    32 x 3 (1),   16 (15)   last band of ONE row (nin = 3), ragged strip of 15 columns
     forward + reflect,        64 x 70 x 255    32 x 3 (6),   16 (15)   last band shorter than the 9-row ring; x, y channel slices (pitches 48, 56)
     flipped + zero,           61 x 67 x 257    34 x 2 (33),  17 (1)    one-column strip whose reflection reads its neighbour; 2074 waves (% 4 == 2)
     forward + zero + bias + LeakyReLU, flipped + reflect + bias + ReLU)
                               8 x 3972 x 33    32 x 125 (4),  3 (1)    125 bands per strip; reference sample by sample
  conv_strip32p_kernel       1024 x 32 x 32     32 x 1,        2 (16)
    (the same 4)               64 x 65 x 255    33 x 2 (32),  16 (15)   channel slices (pitches 80, 80)
                               61 x 67 x 257    67 x 1,       17 (1)    1037 waves (% 4 == 1)
  conv_stript_128_64_kernel  1024 x 16 x 16     16 x 1,        1 (16)   smallest; the fast path of a full strip
                             908 x 17 x 17      17 x 1,        2 (1)    odd rows; one-column strip (slow path, no 17th pixel)
                             8 x 133 x 250      34 x 4 (31),  16 (10)   several bands, ragged band and strip; channel slices (160, 96)
  conv_striptp_128_64_kernel the same three     16 x 1 / 17 x 1 / 67 x 2 (66); 2 / 4 / 64 slabs; channel slices (288, 160)
  conv_strips2_64_128_kernel 2048 x 8 x 16       8 x 1,        1 (16)   smallest (output grid; the input is twice the size)
                             1821 x 9 x 16       9 x 1,        1 (16)   odd rows
                             8 x 131 x 256      33 x 4 (32),  16 (16)   several bands (pair -1 above a band is fetched); channel slices (72, 160)
  conv_strips2p_64_128_kernel 2048 x 8 x 16      8 x 1;  8 x 131 x 256: 66 x 2 (65); channel slices (160, 288)
  conv_strips2_128_256_kernel 1024 x 8 x 16      8 x 1;  911 x 9 x 16: 9 x 1;  8 x 129 x 128: 65 x 2 (64), 8 strips: both channel
                                                 halves x bands; channel slices (136, 272)
  one sample below each threshold: 1023 x 32 x 32 (both 32 -> 32 kernels: 4 slabs, not 2), 1023 x 16 x 16 (transposed: 8, not 1 / 2),
    1820 x 9 x 16 and 910 x 9 x 16 (stride 2: 2, not 1) -- the same exact bits, exact moment sums, another slab count.  (At
    2047 x 8 x 16 the gather kernel's count is 1 as well, which would show nothing: hence 9 rows.)

Not reachable under the default plan, or through the ABI, and therefore not covered:
  * an output pitch with y_ld % 8 == 4 for the 32 -> 32 kernel (launch_strip32 accepts y_ld & 3 == 0): ctg_conv_igemm itself
    answers CTG_EINVAL unless y_ld % 8 == 0 and y is 16-byte aligned, so the entry point never hands the launcher such a pitch.
    The slice case uses y_ld = 56 (y_ld % 16 == 8) at an 8-channel offset;
  * bands shorter than 32 rows for any kernel but the 32 -> 32 bf16 one: B H W >= 2^18 (2^17) with slots <= 2 CU means
    rows x strips >= 16 384, so ceil(rows / (slots / strips)) >= 32 > min_band -- min_band (16, 8) never binds, a one-row or
    shorter-than-the-ring last band exists only for conv_strip32_kernel (its split-pair form: rows x strips <= 65 536 = the
    threshold, so bands of exactly 32 rows need rows % 32 == 0), and the mirror's min_band is pinned by that kernel's cases only;
  * band_env overrides (CTG_* knobs are read once per process; the default plan is the one under test);
  * per-slab exact moments of the split-pair kernels (see above), and which of the two class groups of
    conv_striptp_128_64_kernel wrote which of its two slabs (only their sum is observable through in_finalize);
  * WHICH kernel served the bias + activation launches of the 32 -> 32 kernel.  They return no slab count (ops.conv_igemm
    allocates no moments buffer when a bias or an activation is set, so the library is never asked; the `epi && stats` refusal
    inside launch_strip32 is not reachable from ops, and the "no moments" assertion of those launches pins the Python gate), and
    since the -0 fix below the strip kernel and the halo kernel store the same bits for them.  The evidence is indirect: the
    plain twin launch of the same test (same shape, operands and dispatch conditions but bias / act, which launch_strip32 accepts
    up to LeakyReLU) shows the strip kernel's slab count, and before the fix the ReLU launches of every shape differed from
    the reference exactly by the strip kernel's -0 (mutation 0).  A quiet fallback of ONLY the epilogue launches would pass;
  * NaN / infinite pre-activations (the operands are finite integers): see the comment at strip_act in csrc/conv_strip.h.

Found by this module (both in csrc/conv_strip.h, fixed with it):
  * conv_strip32_kernel read the first three rows of its LDS ring before their DMA had landed whenever a band was shorter than
    the ring.  The prologue retired rows 0 .. 2 with s_waitcnt vmcnt(2 (R - 3)), which counts on R = 9 rows in flight; a band
    of nrows < 7 rows has only nrows + 2, so the count let rows 0 .. 2 pass unretired.  On the card: 64 x 65 x 255 (last band of
    one row) had 520 213 of that band's 522 240 elements wrong in every configuration, 64 x 70 x 255 (6 rows) 192 .. 3059 wrong
    elements in three of four configurations, 8 x 3972 x 33 (4 rows) 96 .. 6497 -- always from row 0 of the last band.  Any map
    with rows % band_rows in 1 .. 6 was affected; the workload's 512 x 512 is not.  Now vmcnt(0) when fewer than R rows are in
    flight.  The split-pair kernel counts per step and was right.
  * its bias + ReLU epilogue (both forms) stored -0 for a negative pre-activation (v * 0.f) where act_apply (csrc/common.h), and
    with it the halo kernel that serves the same layer below the threshold, stores +0: equal values, other bits.  Now the product
    is fma(v, slope, +0): only the sign of that zero changes, NaN and infinities propagate as before (comment at strip_act).

Mutation checks.  Each mutation was built once into a copy of the library outside the repository (never committed; each stays
inside the tensors and removes no wait), the module run against it once on the card; every one fails the cases named:
  1 strip32: reflected column offsets off by one at the right edge          -> all 10 reflect cases of test_strip32 (first diff: last valid column of the last strip)
  2 strip32: col_ok dropped from the masked moments branch                  -> the forward cases of the four ragged shapes (slab moments of the last strip; 1024 x 32 x 32 passes)
  3 strip32: FLIP not applied to tap 0                                      -> all 10 flipped cases of test_strip32
  4 stript: taps w3 and w5 of class (0,1) exchanged                         -> all three stript cases (first diff: parity class (0, 1))
  5 strips2: slab index band * nstrips + strip transposed                   -> strips2_8x131x256 (slab moments; one-band cases are unchanged by construction)
  6 strips2w: the two channel halves' moment destinations swapped           -> all three strips2w cases (slab moments)
  7 striptp: y_lo applied to the hi store (planes exchanged)                -> all three striptp cases
  8 band_plan mirror: min_band ignored                                      -> the plan assertions of 64 x 65 x 255 (22 x 3) and 64 x 70 x 255 (24 x 3), before any launch
  0 the library before the fixes above                                      -> the 16 cases listed under "Found by this module"

Wall time on the MI355X machine (16 CPU threads for the float64 references): 53 tests in 105 s; the slowest case 3.7 s
(split-pair stride-2, two reference passes), the bf16 cases 1.0 .. 2.1 s.  Tensors stay below 170 MB (split-pair 32 -> 32
channel slices: 2^20 pixels x 80 channels is the smallest pitch above the dense 64 that the ABI's % 16 rule allows, and the
threshold allows no fewer pixels; everything else below 150 MB).
"""
import collections

import numpy as np
import pytest
import torch

from conv_ref import (ACT_LRELU, ACT_NONE, ACT_RELU, PAD_REFLECT, PAD_ZERO, PAIR_GRANULE, assert_exact_domain, band_slabs, bias_grid,
                      conv3x3_f64, convT3x3_f64, convT_classes, epilogue, first_diff, int_grid, moments_ref, pack_tap, pair_f64,
                      pair_grid, slab_moments_ref, store_bf16, store_pair, strip_plan)

pytestmark = pytest.mark.gpu

SENT = -24576.0          # a bf16 value no case produces (|accumulator| <= 6912 everywhere)
GUARD = 4096             # sentinel elements behind the last sample of every output buffer
Plan = collections.namedtuple("Plan", "band_rows nbands last_rows nstrips last_cols")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cta_gan_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture
def pair_mode():
    from cta_gan_amd import ops
    ops.set_pair_mode(True)
    yield
    ops.set_pair_mode(False)


# ---------------------------------------------------------------------------- helpers
FWD = [pack_tap(ky - 1, kx - 1, ky * 3 + kx) for ky in range(3) for kx in range(3)]
FLIP = [pack_tap(1 - ky, 1 - kx, ky * 3 + kx) for ky in range(3) for kx in range(3)]


def _cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _plan(kernel, b, rows, cols, edge, what):
    """The plan the launcher makes on this card (the mirror), and the assertion that it IS the edge the case is named for --
    before anything is launched.  A case that misses its edge is a broken case: a failure, never a skip."""
    p = Plan(*strip_plan(kernel, _cu(), b, rows, cols))
    assert edge(p, b), "%s: the plan %r on %d compute units is not the edge this case is named for" % (what, tuple(p), _cu())
    return p


class _Out:
    """An output of C channels as the slice [off, off + C) of a [B, H, W, ld] sentinel buffer with GUARD sentinel elements behind
    the last sample; split pair: the lo plane lies ld / 2 behind the hi plane.  `check` compares the WHOLE buffer -- slice,
    the channels around it and the guard -- with the stored reference bit for bit and locates the first difference."""

    def __init__(self, dev, b, h, w, c, pair, ld=None, off=0):
        self.shape, self.c, self.pair, self.off = (b, h, w), c, pair, off
        self.ld = ld or (2 * c if pair else c)
        self.n = b * h * w * self.ld
        self.flat = torch.full((self.n + GUARD,), SENT, dtype=torch.bfloat16, device=dev)
        self.y = self.flat[:self.n].view(b, h, w, self.ld)[..., off:off + c]

    def check(self, hi, lo, what, plan, os_=1):
        b, h, w = self.shape
        want = torch.full((self.n + GUARD,), SENT, dtype=torch.bfloat16)
        full = want[:self.n].view(b, h, w, self.ld)
        full[..., self.off:self.off + self.c] = hi
        if self.pair:
            full[..., self.off + self.ld // 2:self.off + self.ld // 2 + self.c] = lo
        got = self.flat.cpu()
        ne = got.view(torch.int16) != want.view(torch.int16)
        if not bool(ne.any()):
            return
        k = int(torch.argmax(ne.to(torch.uint8)))
        raise AssertionError("%s: %d elements differ, first at flat index %d [%s]: got %r, want %r"
                             % (what, int(ne.sum()), k, self.where(k, plan, os_), float(got[k]), float(want[k])))

    def where(self, k, plan, os_):
        b, h, w = self.shape
        if k >= self.n:
            return "GUARD region, %d elements behind the last sample" % (k - self.n)
        n, r, c, ch = k // (h * w * self.ld), k // (w * self.ld) % h, k // self.ld % w, k % self.ld
        j, i = r // os_, c // os_
        loc = "sample %d, band %d, row %d of the band, strip %d, column %d of the strip" % (
            n, j // plan.band_rows, j % plan.band_rows, i // 16, i % 16)
        if os_ == 2:
            loc += ", parity class (%d, %d)" % (r & 1, c & 1)
        lo_off = self.off + self.ld // 2
        if self.off <= ch < self.off + self.c:
            return loc + ", channel %d (16-channel tile %d)%s" % (ch - self.off, (ch - self.off) // 16, ", hi plane" if self.pair else "")
        if self.pair and lo_off <= ch < lo_off + self.c:
            return loc + ", channel %d (16-channel tile %d), lo plane" % (ch - lo_off, (ch - lo_off) // 16)
        return loc + ", buffer channel %d: OUTSIDE the output slice" % ch


def _in_bf16(dev, x, ld=None, off=0):
    """x [B, H, W, C] (integers) as bf16 on the device: dense, or the channel slice [off, off + C) of a buffer of pitch ld whose
    other channels hold 9."""
    if ld is None:
        return x.to(torch.bfloat16).to(dev)
    b, h, w, c = x.shape
    full = torch.full((b, h, w, ld), 9.0, dtype=torch.bfloat16)
    full[..., off:off + c] = x.to(torch.bfloat16)
    return full.to(dev)[..., off:off + c]


def _in_pair(dev, xh, xl, ld=None, off=0):
    """Split-pair handle of the planes (xh, xl): hi plane at [off, off + C) of a [B, H, W, ld] buffer, lo plane ld / 2 behind; the
    other channels hold 9 (dense: ld = 2 C, as ops.empty_act lays a pair out)."""
    b, h, w, c = xh.shape
    ld = ld or 2 * c
    full = torch.full((b, h, w, ld), 9.0, dtype=torch.bfloat16)
    full[..., off:off + c] = xh.to(torch.bfloat16)
    full[..., off + ld // 2:off + ld // 2 + c] = xl.to(torch.bfloat16)
    return full.to(dev)[..., off:off + c]


def _pair_parts(v):
    """(hi, lo) of pair_grid values: hi = the integer, lo = the 2^-10 term (tests/test_conv_ref.py: equal to pair_split)."""
    hi = torch.round(v)
    return hi, v - hi


def _operands(rng, xshape, wshape, pair, xr, wr):
    """x, w and the bound on S (max|x| max|w| terms >= S; split pair: the three products' bounds, in granules of 2^-10), checked
    by assert_exact_domain BEFORE anything is launched.  Every tap and every input channel carries a non-zero weight into every
    16-channel output tile."""
    terms = wshape[0] * wshape[2]
    if pair:
        x, w = pair_grid(rng, xshape), pair_grid(rng, wshape)
        xh, xl = _pair_parts(x)
        wh, wl = _pair_parts(w)
        s = float(xh.abs().max() * (wh.abs().max() + wl.abs().max()) + xl.abs().max() * wh.abs().max()) * terms
        assert_exact_domain(torch.tensor(s), PAIR_GRANULE)
        return x, w, (xh, xl)
    x, w = int_grid(rng, xshape, -xr, xr), int_grid(rng, wshape, -wr, wr)
    assert_exact_domain(torch.tensor(float(x.abs().max() * w.abs().max()) * terms))
    assert bool((w != 0).view(wshape[0], wshape[1] // 16, 16, wshape[2]).any(2).all())
    return x, w, None


def _check_moments(ops, part, ns, acc, plan, pair, below, os_, what):
    """bf16: the partials [B, ns, C, 2] slab by slab, exact, against the moments of each slab's pixels (below the dispatch
    threshold, where another kernel with another slab layout runs: their sum over the slabs, exact).  Split pair: the squares are
    multiples of 2^-20 and not exact in fp32 -- ops.in_finalize of the partials against float64 mean / rstd of the exact
    pre-rounding result at rtol 1e-5, atol 1e-6."""
    b, h, w, c = acc.shape
    assert tuple(part.shape) == (b, ns, c, 2), (what, tuple(part.shape))
    if pair:
        mean, rstd = ops.in_finalize(part.contiguous(), ns, h * w)
        mu = acc.mean((1, 2))
        var = (acc * acc).mean((1, 2)) - mu * mu
        assert torch.allclose(mean.double().cpu(), mu, rtol=1e-5, atol=1e-6), (what, "mean")
        assert torch.allclose(rstd.double().cpu(), torch.rsqrt(var + 1e-5), rtol=1e-5, atol=1e-6), (what, "rstd")
        return
    got = part.double().cpu()
    if below:
        want = moments_ref(acc)
        assert_exact_domain(want[..., 1])
        assert torch.equal(got.sum(1), want), (what, first_diff(got.sum(1), want))
        return
    rows, cols = h // os_, w // os_
    want = slab_moments_ref(acc, band_slabs(rows, cols, plan.band_rows, os_))
    assert_exact_domain(want[..., 1])
    d = first_diff(got, want)
    if d is not None:
        (n, z, ch, q), g, wv, cnt = d
        raise AssertionError("%s: %d slab moments differ, first: sample %d, slab %d (band %d, strip %d), channel %d (16-channel tile %d), %s: "
                             "got %r, want %r" % (what, cnt, n, z, z // plan.nstrips, z % plan.nstrips, ch, ch // 16,
                                                  "sum of squares" if q else "sum", g, wv))


def _evidence(ops, ns, plan, pair_t, rows, cols, below, what):
    """Slab count = the strip kernel's (the evidence that it ran, and that its band plan is the mirror's), within the
    buffer-sizing rule; below the threshold: any other count."""
    strip_ns = plan.nbands * plan.nstrips * (2 if pair_t else 1)
    print(what, "plan", tuple(plan), "CUs", _cu(), "nslabs", ns)
    if below:
        assert ns != strip_ns, (what, "slab count %d IS the strip kernel's one pixel below its threshold" % ns)
        return
    assert ns == strip_ns, (what, "slab count %d, the strip kernel's is %d: not the intended kernel, or another band plan" % (ns, strip_ns))
    assert plan.nbands * plan.nstrips <= ops.moments_slabs(rows, cols), (what, "more slabs per class than the moments buffer is sized for")


# ---------------------------------------------------------------------------- conv_strip32_kernel / conv_strip32p_kernel
CONFIGS = {      # taps, padding, epilogue
    "forward_reflect": (False, PAD_REFLECT, ACT_NONE),
    "flipped_zero": (True, PAD_ZERO, ACT_NONE),
    "forward_zero_bias_lrelu": (False, PAD_ZERO, ACT_LRELU),
    "flipped_reflect_bias_relu": (True, PAD_REFLECT, ACT_RELU),
}


def _strip32(dev, *, b, h, w, cfg, pair, seed, edge=None, slices=False, chunk=16):
    """One shape and configuration of the 32 -> 32 channel kernel.  Launch 1: no bias / activation, want_stats=True -- output bits,
    slab count, moments.  Launch 2: a plain configuration again WITHOUT moments (the same bits); an epilogue configuration with its
    bias and activation, asked for moments (must return none: ops.conv_igemm hands the library no moments buffer then).  Both compare
    the whole sentinel buffer with the one float64 reference.  edge=None: one sample below the threshold."""
    from cta_gan_amd import ops
    kernel = "strip32p" if pair else "strip32"
    flipped, pad_mode, act = CONFIGS[cfg]
    what = "%s %dx%dx%d %s" % (kernel, b, h, w, cfg)
    below = edge is None
    plan = Plan(*strip_plan(kernel, _cu(), b, h, w)) if below else _plan(kernel, b, h, w, edge, what)
    rng = np.random.default_rng(seed)
    x, wt, parts = _operands(rng, (b, h, w, 32), (9, 32, 32), pair, 4, 4)
    bs = bias_grid(rng, 32)
    kw = dict(flipped=flipped, pad_mode=pad_mode, chunk=chunk)
    acc = pair_f64(conv3x3_f64, x, wt, parts=parts, **kw) if pair else conv3x3_f64(x, wt, **kw)
    taps = FLIP if flipped else FWD
    if pair:
        xd = _in_pair(dev, *parts, **(dict(ld=80, off=8) if slices else {}))
        wd = wt.float().to(dev)
        ygeo = dict(ld=80, off=8) if slices else {}
    else:
        xd = _in_bf16(dev, x, **(dict(ld=48, off=8) if slices else {}))
        wd = wt.to(torch.bfloat16).to(dev)
        ygeo = dict(ld=56, off=8) if slices else {}      # (y_ld % 16 == 8: every other pixel starts in the middle of a 32-byte sector)

    def stored(v):
        return store_pair(v) if pair else (store_bf16(v), None)

    def launch(bias, act_, want_stats):
        out = _Out(dev, b, h, w, 32, pair, **ygeo)
        r = ops.conv_igemm(xd, wd, 32, out.y, bias, 32, h, w, 0, 0, 1, 1, pad_mode, act_, taps, want_stats=want_stats)
        torch.cuda.synchronize()
        return out, r

    out, (part, ns) = launch(None, ACT_NONE, True)
    out.check(*stored(epilogue(acc)), what + " (with moments)", plan)
    _evidence(ops, ns, plan, False, h, w, below, what)
    _check_moments(ops, part, ns, acc, plan, pair, below, 1, what)
    del out
    if act == ACT_NONE:
        out, (part, ns) = launch(None, ACT_NONE, False)
        assert part is None and ns == 0
        out.check(*stored(epilogue(acc)), what + " (without moments)", plan)
    else:
        out, (part, ns) = launch(bs.float().to(dev), act, True)
        assert part is None and ns == 0, what + ": moments from a launch with an epilogue"
        out.check(*stored(epilogue(acc, bs, act)), what + " (bias + activation)", plan)


def _e_smallest(p, b):
    return p.nbands == 1 and p.band_rows == p.last_rows == 32 and p.nstrips == 2 and p.last_cols == 16


STRIP32 = {
    "1024x32x32_smallest": dict(b=1024, h=32, w=32, edge=_e_smallest),
    "64x65x255_one_row_band": dict(b=64, h=65, w=255, edge=lambda p, b: p.nbands >= 2 and p.last_rows == 1 and p.last_cols == 15),
    "64x70x255_band_shorter_than_ring_slices": dict(b=64, h=70, w=255, slices=True,
                                                    edge=lambda p, b: p.nbands >= 2 and 1 < p.last_rows < 9 and p.last_cols == 15),
    "61x67x257_one_column_strip": dict(b=61, h=67, w=257,
                                       edge=lambda p, b: p.nbands >= 2 and p.last_cols == 1 and (b * p.nbands * p.nstrips) % 4 == 2),
    "8x3972x33_many_bands": dict(b=8, h=3972, w=33, chunk=1, edge=lambda p, b: p.nbands >= 100 and p.last_rows < 9 and p.last_cols == 1),
}
STRIP32P = {
    "1024x32x32_smallest": dict(b=1024, h=32, w=32, edge=_e_smallest),
    "64x65x255_two_bands_slices": dict(b=64, h=65, w=255, slices=True,
                                       edge=lambda p, b: p.nbands == 2 and p.last_rows < p.band_rows and p.last_cols == 15),
    "61x67x257_one_column_strip": dict(b=61, h=67, w=257, edge=lambda p, b: p.last_cols == 1 and (b * p.nbands * p.nstrips) % 4 != 0),
}


@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("name", list(STRIP32))
def test_strip32(name, cfg, dev):
    _strip32(dev, cfg=cfg, pair=False, seed=1000 + 10 * sorted(STRIP32).index(name) + sorted(CONFIGS).index(cfg), **STRIP32[name])


@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("name", list(STRIP32P))
def test_strip32_split_pair(name, cfg, dev, pair_mode):
    _strip32(dev, cfg=cfg, pair=True, seed=1100 + 10 * sorted(STRIP32P).index(name) + sorted(CONFIGS).index(cfg), **STRIP32P[name])


@pytest.mark.parametrize("kind", ["bf16", "pair"])
def test_strip32_one_sample_below_the_threshold(kind, dev, request):
    """B = 1023 at 32 x 32 (2^20 - 1024 pixels): the same exact bits, moments whose slab sum is exact, and a slab count that is
    not the strip kernel's."""
    if kind == "pair":
        request.getfixturevalue("pair_mode")
    _strip32(dev, b=1023, h=32, w=32, cfg="forward_reflect", pair=kind == "pair", seed=1200)


# ---------------------------------------------------------------------------- the stride-2 and transposed kernels
# kernel -> (Cin, Cout, transposed, pair, |x| range, |w| range, (x_ld, x_off), (y_ld, y_off) of the slice cases)
KERNELS = {
    "stript": (128, 64, True, False, 3, 3, (160, 16), (96, 8)),
    "striptp": (128, 64, True, True, 0, 0, (288, 16), (160, 16)),
    "strips2": (64, 128, False, False, 3, 3, (72, 8), (160, 16)),
    "strips2p": (64, 128, False, True, 0, 0, (160, 16), (288, 16)),
    "strips2w": (128, 256, False, False, 3, 2, (136, 8), (272, 8)),
}


def _strided(dev, *, kernel, b, rows, cols, seed, edge=None, slices=False, chunk=16):
    """One shape of a stride-2 (rows x cols = the OUTPUT grid) or transposed (rows x cols = the INPUT grid) kernel: zero padding,
    no epilogue (what the launchers accept), with and without moments -- both launches compare the whole sentinel buffer with
    the one float64 reference.  edge=None: below the threshold."""
    from cta_gan_amd import ops
    cin, cout, transposed, pair, xr, wr, xgeo, ygeo = KERNELS[kernel]
    what = "%s %dx%dx%d" % (kernel, b, rows, cols)
    below = edge is None
    plan = Plan(*strip_plan(kernel, _cu(), b, rows, cols)) if below else _plan(kernel, b, rows, cols, edge, what)
    rng = np.random.default_rng(seed)
    hi_, wi_ = (rows, cols) if transposed else (2 * rows, 2 * cols)
    ho, wo = (2 * rows, 2 * cols) if transposed else (rows, cols)
    x, wt, parts = _operands(rng, (b, hi_, wi_, cin), (9, cout, cin), pair, xr, wr)
    conv, kw = (convT3x3_f64, dict(chunk=chunk)) if transposed else (conv3x3_f64, dict(stride=2, chunk=chunk))
    acc = pair_f64(conv, x, wt, parts=parts, **kw) if pair else conv(x, wt, **kw)
    xg = dict(ld=xgeo[0], off=xgeo[1]) if slices else {}
    yg = dict(ld=ygeo[0], off=ygeo[1]) if slices else {}
    xd = _in_pair(dev, *parts, **xg) if pair else _in_bf16(dev, x, **xg)
    wd = wt.float().to(dev) if pair else wt.to(torch.bfloat16).to(dev)
    want = store_pair(epilogue(acc)) if pair else (store_bf16(epilogue(acc)), None)
    classes = convT_classes(3, 1)
    os_ = 2 if transposed else 1
    for want_stats in (True, False):
        out = _Out(dev, b, ho, wo, cout, pair, **yg)
        if transposed:
            r = ops.conv_igemm_classes(xd, wd, cout, out.y, None, cout, rows, cols, classes, PAD_ZERO, ACT_NONE, want_stats=want_stats)
            assert r is not None, what + ": not served by the merged launch"
        else:
            r = ops.conv_igemm(xd, wd, cout, out.y, None, cout, rows, cols, 0, 0, 1, 2, PAD_ZERO, ACT_NONE, FWD, want_stats=want_stats)
        torch.cuda.synchronize()
        part, ns = r
        out.check(want[0], want[1], what + (" (with moments)" if want_stats else " (without moments)"), plan, os_)
        del out
        if want_stats:
            _evidence(ops, ns, plan, kernel == "striptp", rows, cols, below, what)
            if kernel == "striptp" and not below:
                assert ns <= 4 * ops.moments_slabs(rows, cols)
            if ns:
                _check_moments(ops, part, ns, acc, plan, pair, below, os_, what)
        else:
            assert part is None and ns == 0


def _e_one_band(rows, nstrips, last_cols):
    return lambda p, b: p.nbands == 1 and p.band_rows == p.last_rows == rows and p.nstrips == nstrips and p.last_cols == last_cols


def _e_bands(last_cols):
    return lambda p, b: p.nbands >= 2 and p.last_rows < p.band_rows and p.nstrips >= 2 and p.last_cols == last_cols


STRIDED = {
    "stript_1024x16x16_smallest": dict(kernel="stript", b=1024, rows=16, cols=16, edge=_e_one_band(16, 1, 16)),
    "stript_908x17x17_odd_one_column_strip": dict(kernel="stript", b=908, rows=17, cols=17, edge=_e_one_band(17, 2, 1)),
    "stript_8x133x250_bands_ragged_slices": dict(kernel="stript", b=8, rows=133, cols=250, slices=True, chunk=2, edge=_e_bands(10)),
    "strips2_2048x8x16_smallest": dict(kernel="strips2", b=2048, rows=8, cols=16, chunk=256, edge=_e_one_band(8, 1, 16)),
    "strips2_1821x9x16_odd": dict(kernel="strips2", b=1821, rows=9, cols=16, chunk=256, edge=_e_one_band(9, 1, 16)),
    "strips2_8x131x256_bands_slices": dict(kernel="strips2", b=8, rows=131, cols=256, slices=True, chunk=2, edge=_e_bands(16)),
    "strips2w_1024x8x16_smallest": dict(kernel="strips2w", b=1024, rows=8, cols=16, chunk=256, edge=_e_one_band(8, 1, 16)),
    "strips2w_911x9x16_odd": dict(kernel="strips2w", b=911, rows=9, cols=16, chunk=256, edge=_e_one_band(9, 1, 16)),
    "strips2w_8x129x128_bands_slices": dict(kernel="strips2w", b=8, rows=129, cols=128, slices=True, chunk=2, edge=_e_bands(16)),
}
STRIDED_PAIR = {
    "striptp_1024x16x16_smallest": dict(kernel="striptp", b=1024, rows=16, cols=16, edge=_e_one_band(16, 1, 16)),
    "striptp_908x17x17_odd_one_column_strip": dict(kernel="striptp", b=908, rows=17, cols=17, edge=_e_one_band(17, 2, 1)),
    "striptp_8x133x250_bands_ragged_slices": dict(kernel="striptp", b=8, rows=133, cols=250, slices=True, chunk=2, edge=_e_bands(10)),
    "strips2p_2048x8x16_smallest": dict(kernel="strips2p", b=2048, rows=8, cols=16, chunk=256, edge=_e_one_band(8, 1, 16)),
    "strips2p_8x131x256_bands_slices": dict(kernel="strips2p", b=8, rows=131, cols=256, slices=True, chunk=2, edge=_e_bands(16)),
}
# one sample below each threshold, at grids where the kernel that runs instead has another slab count than one band x one strip
BELOW = {
    "stript_1023x16x16": dict(kernel="stript", b=1023, rows=16, cols=16),
    "striptp_1023x16x16": dict(kernel="striptp", b=1023, rows=16, cols=16),
    "strips2_1820x9x16": dict(kernel="strips2", b=1820, rows=9, cols=16, chunk=256),
    "strips2p_1820x9x16": dict(kernel="strips2p", b=1820, rows=9, cols=16, chunk=256),
    "strips2w_910x9x16": dict(kernel="strips2w", b=910, rows=9, cols=16, chunk=256),
}


@pytest.mark.parametrize("name", list(STRIDED))
def test_stride2_and_transposed_strips(name, dev):
    _strided(dev, seed=2000 + sorted(STRIDED).index(name), **STRIDED[name])


@pytest.mark.parametrize("name", list(STRIDED_PAIR))
def test_stride2_and_transposed_strips_split_pair(name, dev, pair_mode):
    _strided(dev, seed=2100 + sorted(STRIDED_PAIR).index(name), **STRIDED_PAIR[name])


@pytest.mark.parametrize("name", list(BELOW))
def test_stride2_and_transposed_one_sample_below_the_threshold(name, dev, request):
    if KERNELS[BELOW[name]["kernel"]][3]:
        request.getfixturevalue("pair_mode")
    _strided(dev, seed=2200 + sorted(BELOW).index(name), **BELOW[name])
