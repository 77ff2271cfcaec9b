"""GPU: the convolution kernel family, bit for bit, against tests/conv_ref.py on integer-grid operands.

Exactness argument.  Operands are small integers (split-pair mode: integers of magnitude <= 2 plus {-1, 0, 1} 2^-10), biases
multiples of 1/8.  Every product and partial sum of an accumulator is then a multiple of the granule (1, resp. 2^-10), and while
S = sum of the terms' magnitudes is below 2^24 granules, fp32 accumulation is exact in ANY order, on the matrix cores or the
vector ALUs: the kernel has to reproduce the float64 reference bit for bit, and a dropped, duplicated, misplaced or mis-padded
term is a non-zero integer difference at a known element.  Three conditions were checked on the CPU (tests/test_conv_ref.py):
(1) the reference equals torch's float64 conv2d / conv_transpose2d / autograd / conv2d_weight on such inputs, (2) S of every
case here is below 2^24 granules -- `assert_exact_domain` runs on the reference's S BEFORE anything is launched, and on the sum
of squares where moments are emitted; a case that fails it is a broken case, never a skip --, (3) the bf16 and split-pair store
helpers equal tensor.bfloat16(), and 84 % of the integers in +-5000 are no bf16 values, so the output rounding is exercised.
Every comparison is torch.equal on the stored bits, outputs are pre-filled with a sentinel that everything the launch must not
write has to keep.  Allowances: tanh outputs against float64 tanh of the exact pre-activation within 2e-4 (the fp32 forward
bound of test_kernels_gpu.py; the same case runs with ACT_NONE and must be exact), and ops.in_finalize of exact partials
against float64 mean / rstd at rtol 1e-5, atol 1e-6.  LeakyReLU is one fp32 multiply by 0.2f in the kernels and in numpy: exact.

Path evidence.  Nothing in the ABI names the kernel that ran; what is observable is the slab count `nslabs` of the moments a
twin launch without bias / activation returns, and the partial count Z (and the status the library answers) of a weight gradient.

  case                      dispatch condition (csrc)                            instantiation reached             evidence
  gather 9x11, 13x15, 4x4   Hs or Ws < 16 (conv_igemm.hip: halo needs >= 16)      conv_igemm_kernel BM 128          nslabs = ceil(Hs Ws / 128)
  gather out_f32 / Cout<=16 Hs < 16                                               BN 16, fp32 store, scalar tail    none (no moments for Cout <= 16)
  gather stride-2 input     is == 2, Hs < 16 (no s2d, no strip kernel)            BM 128, BN 128                    nslabs = ceil(Hs Ws / 128)
  gather one class, os 2    Hs < 16                                               BM 128, BN 64                     none (moments need os == 1)
  gather frame              frame != 0 (halo and moments exclude it)              BM 128, BN 64 (frame64), 3-ring   none; ring-only write
  gather big tile           is 2, 3x3 (s2d serves 16 taps only), 4355 px >= 4096  BM 256, BN 128, 8 waves, 3-ring   nslabs = ceil(4355 / 256) = 18
  halo 64->64, 33x17        stride 1, full window, >= 16: launch_halo_t           BN 64, TH 8, KWC 3                nslabs = ceil(Hs/8) ceil(Ws/16)
  halo 128->256, 23x19      < 384 workgroups: halo_th8                            BN 128, TH 8                      nslabs = ceil(Hs/8) ceil(Ws/16)
  halo 128->256, 3x128x128  >= 384 workgroups                                     BN 128, TH 16                     nslabs = ceil(Hs/16) ceil(Ws/16)
  halo 32->32, 96->32       Cout <= 32 / Cin % 64 != 0                            BN 32, KCH 4, TH 16               nslabs (16-row tiles)
  halo 4x4                  kw == 4: run-time window                              KWC 0                             nslabs
  halo fp32                 dtype 0                                               launch_halo_t<float>, TH 16       nslabs (16-row tiles)
  halo res / fold           epi->res / fold                                       FUSE                              served only by the halo kernel (CTG_EINVAL otherwise)
  halo s2d                  is 2, 16 taps, Cout > 32, >= 16                       S2D, TH 16, 4 phases              nslabs = ceil(Hs/16) ceil(Ws/16)
  merged classes            ctg_conv_igemm_classes, >= 16                         MC, TH 8 (Cout 64) / 16 (128)     nslabs = 4 x halo count; not None
  wgrad per-tap             Hs < 8 / Ws < 16 / fp32                               conv_wgrad_kernel                 the two slabs='linear' cases: per-slab partials
                                                                                                                    in runs of `slab` row-major pixels
  wgrad halo                bf16, stride 1, row-major window, Hs >= 8, Ws >= 16   conv_wgrad_halo_kernel            the slabs='tile' case: per-slab partials in
                                                                                                                    runs of 8 x 16 tiles
  wgrad stride 2            is 2, zero padding                                    s2m (64-multiples) / 4 launches   not observable (see below)
  wgrad split pair          dtype 2                                               three sweeps / phase_split        status 0 / 3, Z = B sps / 3 B sps
  strip kernels             B Hs Ws >= 2^20 / 2^18 / 2^17 (csrc/conv_strip*.h)    not reached (every grid here is     covered by tests/test_strip_exact_gpu.py
                                                                                  smaller): "no strip kernel" above

What Z does NOT show: Z = B sps with status 0 is what the per-tap kernel, the halo-resident kernel, the merged stride-2 kernel
(s2m) and its four-launch form all answer, so for the weight-gradient cases without a per-slab comparison it only shows that
one partial per slab was written (against 3 B sps of the split forms), not which kernel wrote it.  There the instantiation
follows from the dispatch conditions of ctg_conv_wgrad alone (read from the source, restated in the table), and the only
run-time evidence is mutation 5 (confined to conv_wgrad_halo_kernel: the 17 x 33 halo cases fail, no per-tap case does) and
mutation 6 (confined to conv_wgrad_s2m_kernel: exactly the s2m cases fail, the four-launch case does not) -- runs that are
not part of the committed suite.

Cases reduced on purpose: none of the issue's cross products -- both s2d channel configurations and both merged stride-2
weight gradients run on the even and on the odd input size, and the four halo weight-gradient tiles run on both grids with
both paddings.

Not reachable through the ops-level entry points and therefore not covered: `wgs` ABOVE the tile count of ctg_corr_smallcin
(ops.corr_smallcin sizes it as min(tiles, ceil(512 / B)); `wgs` below the tile count -- several tiles per workgroup, uneven
shares -- is covered with B = 171 and B = 64); a first layer with two planes and a 4x4 stride-2 window (ops.smallcin_ok
refuses it).  Split-pair launches emit moments whose squares are multiples of 2^-20: their sums are not exact in fp32 and
only the slab count is asserted there (those moments are neither compared nor domain-checked).

Found by this module: nothing -- every case passed bit for bit on its first run on the MI355X, with the slab counts, partial
counts and statuses the table names.

Mutation checks.  Each mutation was built once into a copy of the library outside the repository (never committed; each
stays in bounds) and the module run against it; every one fails the cases named:
  1 far-edge row reflection of the halo loader (3x3 pre-computed offsets) off by one -> test_halo_kernel[64to64_reflect_33x17*], test_split_pair_forward[halo_64to64_33x17]
  2 last K chunk of the halo kernel skipped when Cin % 64 == 32 (Cin 96)             -> test_halo_kernel[96to32_32x32]
  3 top-edge pad slots of the frame launch pointing at pixel (1, Ws - 2)             -> all test_gather_kernel_frame_launch cases, test_split_pair_forward[frame_64to64_18x18]
  4 c_oy0 / c_ox0 of classes 1 and 2 swapped in ctg_conv_igemm_classes               -> all test_merged_parity_classes cases, test_split_pair_merged_parity_classes
  5 G-tile pixel mask of conv_wgrad_halo_kernel widened by one row (row Hs - 1 read twice) -> the 17x33 cases of test_weight_gradient_halo_kernel (as run: zero padding; the reflect ones were added later), the 4x4 stride-2 and the phase_split case
  6 tap slots 1 and 2 exchanged in conv_wgrad_s2m_kernel's partial store             -> the s2m and roles-swapped cases of test_weight_gradient_stride2_polyphase, the split-pair s2m case
  7 scalar tail loop of wgrad_reduce_multi_kernel removed                            -> test_wgrad_reduce_multi_25_jobs and 16 weight-gradient cases (their Z is no multiple of 4)
  8 `res` added before the bf16 rounding of the conv result instead of after it      -> every `res` and `res_fold` case of test_halo_kernel_residual_and_fold_epilogue
"""
import numpy as np
import pytest
import torch

from conv_ref import (ACT_LRELU, ACT_NONE, ACT_RELU, ACT_TANH, PAD_REFLECT, PAD_ZERO, PAIR_GRANULE, assert_exact_domain,
                      bias_grid, conv_classes_ref, conv_pair_ref, conv_pair_s, conv_taps_ref, convT_classes, epilogue, first_diff,
                      frame_mask, fused_store_bf16, int_grid, linear_slabs, moments_ref, pack_tap, pair_grid, place,
                      store_bf16, store_f32, store_pair, tanh_ref, tile_slabs, wgrad_pair_ref, wgrad_taps_ref)

pytestmark = pytest.mark.gpu

SENT = -24576.0          # a bf16 value no case produces
BF16, F32, PAIR = "bf16", "f32", "pair"


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
def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _where_nhwc(shape, os_=1):
    """Locates an element of an NHWC output [B, H, W, C]: the spatial tiles of the halo kernels (16 columns x 16 or 8 rows of
    the launch's own grid), the 128-pixel M tile (= moments slab) of the gather kernel, and the 64-channel tile."""
    def where(idx):
        j, i = idx[1] // os_, idx[2] // os_
        return "grid pixel (%d, %d): 16x16 tile (%d, %d), 8-row tile %d, gather M tile %d; channel tile %d" % (
            j, i, j // 16, i // 16, j // 8, (j * _ceil(shape[2], os_) + i) // 128, idx[3] // 64)
    return where


def _where_wgrad(taps):
    """Locates an element of a weight gradient stored [m][c][t]: its tap and the 64-wide channel tiles."""
    def where(idx):
        t = idx[2]
        return "tap %d (dy %d, dx %d); channel tiles m %d, c %d" % (t, (taps[t] & 0xff) - 64, ((taps[t] >> 8) & 0xff) - 64,
                                                                   idx[0] // 64, idx[1] // 64)
    return where


def _assert_bits(got, want, what, where=None):
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not torch.equal(_bits(got), _bits(want)):
        idx, g, w, n = first_diff(got.float(), want.float()) or ((), 0.0, 0.0, 0)
        if where is None and len(idx) == 4:
            where = _where_nhwc(got.shape)
        loc = " [%s]" % where(idx) if (where is not None and idx) else ""
        raise AssertionError("%s: %d elements differ, first at %s%s: got %r, want %r" % (what, n, idx, loc, g, w))


def _bn(cout):
    return 128 if cout > 64 else 64 if cout > 32 else 32 if cout > 16 else 16


def _ceil(a, b):
    return (a + b - 1) // b


def fwd_taps(k, pad):
    return [pack_tap(ky - pad, kx - pad, ky * k + kx) for ky in range(k) for kx in range(k)]


def flip_taps(k, p):
    """backward-data order: tap (ky, kx) reads g[j + p - ky, i + p - kx]"""
    return [pack_tap(p - ky, p - kx, ky * k + kx) for ky in range(k) for kx in range(k)]


def _slice_of(t, extra, off, fill):
    """`t` [B, H, W, C] as a channel slice at `off` of a buffer with `extra` more channels filled with `fill`."""
    if not extra:
        return t.contiguous(), None
    b, h, w, c = t.shape
    full = torch.full((b, h, w, c + extra), fill, dtype=t.dtype, device=t.device)
    full[..., off:off + c] = t
    return full[..., off:off + c], full


def _pack_w(w, npad, fill=5.0):
    """[slices, Cout, Cin] -> [slices, npad, Cin]; the rows of the N tile beyond Cout hold `fill` (computed, never stored)."""
    out = torch.full((w.shape[0], npad, w.shape[2]), fill, dtype=torch.float64)
    out[:, :w.shape[1]] = w
    return out


def _check_moments(ops, part, nslabs, acc, hw, what):
    """The partials [B, nslabs, C, 2] are exact integers: their float64 sum equals the exact moments; ops.in_finalize of them
    gives mean / rstd of the accumulators."""
    want = moments_ref(acc)
    assert_exact_domain(want[..., 1])
    got = part.double().sum(1).cpu()
    assert torch.equal(got, want), (what, first_diff(got, want))
    mean, rstd = ops.in_finalize(part.contiguous(), nslabs, hw)
    mu = want[..., 0] / hw
    var = want[..., 1] / hw - mu * mu
    assert torch.allclose(mean.double().cpu(), mu, rtol=1e-5, atol=1e-6), what
    assert torch.allclose(rstd.double().cpu(), torch.rsqrt(var + 1e-5), rtol=1e-5, atol=1e-6), what


# ---------------------------------------------------------------------------- ops.conv_igemm
def _fwd(dev, *, cin, cout, taps, B, Hi, Wi, Hs, Ws, seed, is_=1, os_=1, oy0=0, ox0=0, Ho=None, Wo=None, pad_mode=PAD_ZERO,
         kind=BF16, out_f32=False, bias=False, act=ACT_NONE, frame=False, xs=0, ys=0, res=False, fold=False, lo=-3, hi=3,
         nslabs=None, moments=True, wdens=1.0):
    """One ops.conv_igemm case.  nslabs: the slab count the intended kernel returns from the twin launch without bias /
    activation (None: the launch cannot emit moments -- frame, Cout <= 16, os == 2 on the gather kernel).  wdens: share of
    non-zero weights (tanh cases: pre-activations of a few units, so that the allowance tests the tanh evaluation)."""
    from cta_gan_amd import ops
    rng = np.random.default_rng(seed)
    Ho, Wo = Ho or Hs, Wo or Ws
    nsl = max(t >> 16 for t in taps) + 1
    pair = kind == PAIR
    x = pair_grid(rng, (B, Hi, Wi, cin)) if pair else int_grid(rng, (B, Hi, Wi, cin), lo, hi)
    w = pair_grid(rng, (nsl, cout, cin)) if pair else int_grid(rng, (nsl, cout, cin), lo, hi)
    if wdens < 1.0:
        w = w * torch.from_numpy((rng.random(tuple(w.shape)) < wdens).astype(np.float64))
    bs = bias_grid(rng, cout) if bias else None
    if pair:
        acc = conv_pair_ref(x, w, taps, Hs, Ws, is_, pad_mode)
        assert_exact_domain(conv_pair_s(x, w, taps, Hs, Ws, is_, pad_mode), PAIR_GRANULE)
    else:
        acc = conv_taps_ref(x, w, taps, Hs, Ws, is_, pad_mode)
        _domain(x, w, taps, Hs, Ws, is_, pad_mode)
    if nslabs and moments and not pair:
        assert_exact_domain(moments_ref(acc)[..., 1])
    rs = int_grid(rng, (B, Hs, Ws, cout), lo, hi) if res else None
    fd = int_grid(rng, (B, Hs + 2, Ws + 2, cout), lo, hi) if fold else None
    tanh = act == ACT_TANH
    if tanh:
        unsat = int((tanh_ref(acc, bs).abs() < 0.995).sum())
        assert unsat >= 100, "tanh case is saturated: only %d pre-activations below 3" % unsat
    v = epilogue(acc, bs, ACT_NONE if tanh else act)
    ydt = torch.float32 if (out_f32 or kind == F32) else torch.bfloat16
    if res or fold:
        assert kind == BF16 and not out_f32
        stored = fused_store_bf16(v, rs, fd)
    elif pair and not out_f32:
        stored = store_pair(v)
    else:
        stored = store_f32(v) if (out_f32 or kind == F32) else store_bf16(v)

    def full_of(st):
        full = torch.full((B, Ho, Wo, cout), SENT, dtype=ydt)
        sub = st
        if frame:
            sub = torch.where(frame_mask(Hs, Ws)[None, :, :, None], st, torch.full_like(st, SENT))
        return place(full, sub, os_, oy0, ox0)
    # ---- device operands
    cdt = torch.float32 if kind == F32 else torch.bfloat16
    npad = _ceil(cout, _bn(cout)) * _bn(cout)
    wp = _pack_w(w, npad).to(dev)
    if pair:
        xd = ops.to_pair(x.float().to(dev))
        wd = wp.float().contiguous()
    else:
        xd, _ = _slice_of(x.to(dev).to(cdt), xs, 8 if xs else 0, 9.0)
        wd = wp.to(cdt).contiguous()
    bd = bs.float().to(dev) if bias else None
    kw = {}
    if res:
        kw["res"] = rs.to(dev).to(ydt)
    if fold:
        kw["fold"] = fd.to(dev).to(ydt)

    yoff = 0 if not ys else 8 if ydt == torch.bfloat16 else min(4, ys // 2)

    def new_y():
        if pair and not out_f32:
            y = ops.empty_act((B, Ho, Wo, cout), torch.bfloat16, dev)
            y.fill_(SENT)
            ops.pair_lo(y).fill_(SENT)
            return y, None
        yfull = torch.full((B, Ho, Wo, cout + ys), SENT, dtype=ydt, device=dev)
        return yfull[..., yoff:yoff + cout], yfull

    y, yfull = new_y()
    plain = not bias and act == ACT_NONE and not res and not fold
    part, ns = ops.conv_igemm(xd, wd, npad, y, bd, cout, Hs, Ws, oy0, ox0, os_, is_, pad_mode, act, taps,
                              want_stats=plain and not frame, frame=frame, **kw)
    torch.cuda.synchronize()
    what = "conv %d->%d %dtaps %s @%dx%d" % (cin, cout, len(taps), kind, Hs, Ws)
    if tanh:
        want = tanh_ref(acc, bs)
        err = float((y.double().cpu() - want).abs().max())
        print(what, "tanh max err %.3g" % err)
        assert err <= 2e-4, (what, err)
    elif pair and not out_f32:
        _assert_bits(y, full_of(stored[0]), what + " hi plane", _where_nhwc(y.shape, os_))
        _assert_bits(ops.pair_lo(y), full_of(stored[1]), what + " lo plane", _where_nhwc(y.shape, os_))
    else:
        _assert_bits(y, full_of(stored), what, _where_nhwc(y.shape, os_))
    if yfull is not None and ys:
        mask = torch.ones(cout + ys, dtype=torch.bool)
        mask[yoff:yoff + cout] = False
        assert bool((yfull.cpu()[..., mask].float() == SENT).all()), what + ": wrote outside its channel slice"
    # ---- path evidence: the twin launch without bias / activation
    if not plain and not (res or fold) and not frame:
        y2, _ = new_y()
        part, ns = ops.conv_igemm(xd, wd, npad, y2, None, cout, Hs, Ws, oy0, ox0, os_, is_, pad_mode, ACT_NONE, taps,
                                  want_stats=True)
        torch.cuda.synchronize()
    if res or fold or frame:
        assert nslabs is None
        return
    print(what, "nslabs", ns)
    assert ns == (nslabs or 0), (what, "slab count %d: not the intended kernel (%r)" % (ns, nslabs))
    if ns and moments and not pair:      # (split pair: the squares are multiples of 2^-20, their sums are not exact in fp32)
        _check_moments(ops, part, ns, acc, Hs * Ws, what)


def _domain(x, w, taps, hs, ws, is_, pad_mode):
    """assert_exact_domain on S; the bound max|x| max|w| Cin taps >= S spares the second reference pass where it suffices."""
    bound = float(x.abs().max() * w.abs().max()) * x.shape[3] * len(taps)
    if bound < 2 ** 24:
        return assert_exact_domain(torch.tensor(bound))
    return assert_exact_domain(conv_taps_ref(x.abs(), w.abs(), taps, hs, ws, is_, pad_mode))


def _halo(hs, ws, th):
    return _ceil(hs, th) * _ceil(ws, 16)


GATHER = {
    "64to128_reflect_9x11": dict(cin=64, cout=128, taps=fwd_taps(3, 1), B=2, Hi=9, Wi=11, Hs=9, Ws=11, pad_mode=PAD_REFLECT, nslabs=1, lo=-2, hi=2),
    "128to64_flipped_zero_9x11": dict(cin=128, cout=64, taps=flip_taps(3, 1), B=2, Hi=9, Wi=11, Hs=9, Ws=11, nslabs=1),
    "32to32_lrelu_13x15": dict(cin=32, cout=32, taps=fwd_taps(3, 1), B=1, Hi=13, Wi=15, Hs=13, Ws=15, bias=True, act=ACT_LRELU, nslabs=2),
    "96to32_lrelu_13x15": dict(cin=96, cout=32, taps=fwd_taps(3, 1), B=1, Hi=13, Wi=15, Hs=13, Ws=15, bias=True, act=ACT_LRELU, nslabs=2),
    "64to64_1x1_4x4": dict(cin=64, cout=64, taps=fwd_taps(1, 0), B=2, Hi=4, Wi=4, Hs=4, Ws=4, nslabs=1),
    "32to2_f32out_7x7": dict(cin=32, cout=2, taps=fwd_taps(3, 1), B=2, Hi=7, Wi=7, Hs=7, Ws=7, out_f32=True, bias=True, ys=2),
    "512to1_4x4_f32out_7x7": dict(cin=512, cout=1, taps=fwd_taps(4, 1), B=2, Hi=7, Wi=7, Hs=6, Ws=6, out_f32=True, bias=True),
    "fp32_64to64_reflect_9x11": dict(cin=64, cout=64, taps=fwd_taps(3, 1), B=2, Hi=9, Wi=11, Hs=9, Ws=11, pad_mode=PAD_REFLECT, kind=F32, nslabs=1),
    "fp32_16to2_9x11": dict(cin=16, cout=2, taps=fwd_taps(3, 1), B=2, Hi=9, Wi=11, Hs=9, Ws=11, kind=F32, bias=True),
    "s2_64to128_3x3_15x13": dict(cin=64, cout=128, taps=fwd_taps(3, 1), B=2, Hi=15, Wi=13, Hs=8, Ws=7, is_=2, nslabs=1),
    "s2_64to128_4x4_10x14": dict(cin=64, cout=128, taps=fwd_taps(4, 1), B=2, Hi=10, Wi=14, Hs=5, Ws=7, is_=2, nslabs=1),
    "xslice_yslice_64to64_9x11": dict(cin=64, cout=64, taps=fwd_taps(3, 1), B=2, Hi=9, Wi=11, Hs=9, Ws=11, xs=16, ys=24, nslabs=1),
}


@pytest.mark.parametrize("name", list(GATHER))
def test_gather_kernel(name, dev):
    _fwd(dev, seed=sorted(GATHER).index(name) + 1, **GATHER[name])


@pytest.mark.parametrize("q", range(4))
def test_gather_kernel_one_parity_class_leaves_the_others(q, dev):
    """The four classes of convT 128 -> 64 from 7 x 9, one launch each into its (oy0, ox0) of the 14 x 18 output: the other three
    classes' pixels keep the sentinel."""
    py, px, taps = convT_classes(3, 1)[q]
    _fwd(dev, seed=40 + q, cin=128, cout=64, taps=taps, B=2, Hi=7, Wi=9, Hs=7, Ws=9, os_=2, oy0=py, ox0=px, Ho=14, Wo=18)


@pytest.mark.parametrize("grid", [(5, 4), (18, 18), (18, 130)], ids=["5x4", "18x18", "18x130"])
@pytest.mark.parametrize("ch", [64, 256])
def test_gather_kernel_frame_launch(ch, grid, dev):
    """frame=True: flipped 3x3, zero padding, on the padded grid -- only the 1-pixel ring is written (18 x 130: an edge longer
    than one 128-slot tile, the second tile's pad slots repeat the edge's last pixel)."""
    hs, ws = grid
    _fwd(dev, seed=50 + ch + ws, cin=ch, cout=ch, taps=flip_taps(3, 0), B=2, Hi=hs - 2, Wi=ws - 2, Hs=hs, Ws=ws, frame=True)


def test_gather_kernel_big_tile(dev):
    """128 -> 256 3x3 stride 2 from 130 x 134: 65 x 67 = 4355 pixels >= 4096, the 256 x 128 tile with the 3-stage ring."""
    _fwd(dev, seed=60, cin=128, cout=256, taps=fwd_taps(3, 1), B=1, Hi=130, Wi=134, Hs=65, Ws=67, is_=2, nslabs=_ceil(65 * 67, 256),
         lo=-1, hi=1)


HALO = {
    "64to64_reflect_33x17": dict(cin=64, cout=64, taps=fwd_taps(3, 1), B=1, Hi=33, Wi=17, Hs=33, Ws=17, pad_mode=PAD_REFLECT, nslabs=_halo(33, 17, 8)),
    "64to64_reflect_33x17_slices": dict(cin=64, cout=64, taps=fwd_taps(3, 1), B=1, Hi=33, Wi=17, Hs=33, Ws=17, pad_mode=PAD_REFLECT, xs=16, ys=24, nslabs=_halo(33, 17, 8)),
    "128to256_zero_23x19": dict(cin=128, cout=256, taps=fwd_taps(3, 1), B=1, Hi=23, Wi=19, Hs=23, Ws=19, nslabs=_halo(23, 19, 8), lo=-2, hi=2),
    "64to256_3x128x128_th16": dict(cin=64, cout=256, taps=fwd_taps(3, 1), B=3, Hi=128, Wi=128, Hs=128, Ws=128, nslabs=_halo(128, 128, 16), lo=-1, hi=1),
    "32to32_lrelu_40x24": dict(cin=32, cout=32, taps=fwd_taps(3, 1), B=2, Hi=40, Wi=24, Hs=40, Ws=24, bias=True, act=ACT_LRELU, nslabs=_halo(40, 24, 16)),
    "96to32_32x32": dict(cin=96, cout=32, taps=fwd_taps(3, 1), B=1, Hi=32, Wi=32, Hs=32, Ws=32, bias=True, act=ACT_RELU, nslabs=_halo(32, 32, 16), lo=-2, hi=2),
    "256to512_4x4_20x20": dict(cin=256, cout=512, taps=fwd_taps(4, 1), B=1, Hi=20, Wi=20, Hs=19, Ws=19, nslabs=_halo(19, 19, 8), lo=-1, hi=1),
    "64to1_7x7_reflect_f32out_32x48": dict(cin=64, cout=1, taps=fwd_taps(7, 3), B=2, Hi=32, Wi=48, Hs=32, Ws=48, pad_mode=PAD_REFLECT, out_f32=True, bias=True),
    "64to1_7x7_reflect_tanh_32x48": dict(cin=64, cout=1, taps=fwd_taps(7, 3), B=2, Hi=32, Wi=48, Hs=32, Ws=48, pad_mode=PAD_REFLECT, out_f32=True, bias=True, act=ACT_TANH, wdens=0.004),
    "32to2_f32out_32x16": dict(cin=32, cout=2, taps=fwd_taps(3, 1), B=2, Hi=32, Wi=16, Hs=32, Ws=16, out_f32=True, bias=True),
    "fp32_64to64_reflect_33x17": dict(cin=64, cout=64, taps=fwd_taps(3, 1), B=1, Hi=33, Wi=17, Hs=33, Ws=17, pad_mode=PAD_REFLECT, kind=F32, nslabs=_halo(33, 17, 16)),
    "s2d_64to128_4x4_70x66": dict(cin=64, cout=128, taps=fwd_taps(4, 1), B=2, Hi=70, Wi=66, Hs=35, Ws=33, is_=2, nslabs=_halo(35, 33, 16), lo=-2, hi=2),
    "s2d_64to128_4x4_37x51": dict(cin=64, cout=128, taps=fwd_taps(4, 1), B=2, Hi=37, Wi=51, Hs=18, Ws=25, is_=2, nslabs=_halo(18, 25, 16), lo=-2, hi=2),
    "s2d_128to256_4x4_70x66": dict(cin=128, cout=256, taps=fwd_taps(4, 1), B=1, Hi=70, Wi=66, Hs=35, Ws=33, is_=2, nslabs=_halo(35, 33, 16), lo=-1, hi=1),
    "s2d_128to256_4x4_37x51": dict(cin=128, cout=256, taps=fwd_taps(4, 1), B=1, Hi=37, Wi=51, Hs=18, Ws=25, is_=2, nslabs=_halo(18, 25, 16), lo=-2, hi=2),
}


@pytest.mark.parametrize("name", list(HALO))
def test_halo_kernel(name, dev):
    _fwd(dev, seed=100 + sorted(HALO).index(name), **HALO[name])


@pytest.mark.parametrize("epi", ["res", "fold", "res_fold"])
@pytest.mark.parametrize("grid", [(32, 48), (33, 17)], ids=["32x48", "33x17"])
@pytest.mark.parametrize("ch", [64, 256])
def test_halo_kernel_residual_and_fold_epilogue(ch, grid, epi, dev):
    """The FUSE instantiation: flipped 3x3; `res` is added to the ROUNDED conv result, the frame of `fold` (a padded-grid
    gradient whose interior holds non-zero values that must not be read) is folded in, and the sum is rounded again."""
    h, w = grid
    _fwd(dev, seed=200 + ch + h, cin=ch, cout=ch, taps=flip_taps(3, 1), B=2 if ch == 64 else 1, Hi=h, Wi=w, Hs=h, Ws=w,
         res="res" in epi, fold="fold" in epi)


def _classes(dev, *, cin, cout, k, B, Hs, Ws, seed, nslabs, kind=BF16, lo=-3, hi=3):
    from cta_gan_amd import ops
    rng = np.random.default_rng(seed)
    classes = convT_classes(k, 1)
    pair = kind == PAIR
    x = pair_grid(rng, (B, Hs, Ws, cin)) if pair else int_grid(rng, (B, Hs, Ws, cin), lo, hi)
    w = pair_grid(rng, (k * k, cout, cin)) if pair else int_grid(rng, (k * k, cout, cin), lo, hi)
    acc = torch.zeros(B, 2 * Hs, 2 * Ws, cout, dtype=torch.float64)
    for py, px, taps in classes:
        if pair:
            a = conv_pair_ref(x, w, taps, Hs, Ws, 1, PAD_ZERO)
            assert_exact_domain(conv_pair_s(x, w, taps, Hs, Ws, 1, PAD_ZERO), PAIR_GRANULE)
        else:
            a = conv_taps_ref(x, w, taps, Hs, Ws, 1, PAD_ZERO)
            assert_exact_domain(conv_taps_ref(x.abs(), w.abs(), taps, Hs, Ws, 1, PAD_ZERO))
        place(acc, a, 2, py, px)
    if not pair:
        assert torch.equal(acc, conv_classes_ref(x, w, classes, Hs, Ws, PAD_ZERO))
    v = epilogue(acc)
    if not pair:
        assert_exact_domain(moments_ref(acc)[..., 1])
    npad = _ceil(cout, _bn(cout)) * _bn(cout)
    wp = _pack_w(w, npad).to(dev)
    what = "merged classes %d->%d k%d %s @%dx%d" % (cin, cout, k, kind, Hs, Ws)
    if pair:
        xd, wd = ops.to_pair(x.float().to(dev)), wp.float().contiguous()
        y = ops.empty_act((B, 2 * Hs, 2 * Ws, cout), torch.bfloat16, dev)
        y.fill_(SENT)
        ops.pair_lo(y).fill_(SENT)
    else:
        xd, wd = x.to(dev).bfloat16(), wp.to(torch.bfloat16).contiguous()
        y = torch.full((B, 2 * Hs, 2 * Ws, cout), SENT, dtype=torch.bfloat16, device=dev)
    r = ops.conv_igemm_classes(xd, wd, npad, y, None, cout, Hs, Ws, classes, PAD_ZERO, ACT_NONE, want_stats=True)
    torch.cuda.synchronize()
    assert r is not None, what + ": not served by the merged launch"
    if pair:
        hi_, lo_ = store_pair(v)
        _assert_bits(y, hi_, what + " hi plane", _where_nhwc(y.shape, 2))
        _assert_bits(ops.pair_lo(y), lo_, what + " lo plane", _where_nhwc(y.shape, 2))
    else:
        _assert_bits(y, store_bf16(v), what, _where_nhwc(y.shape, 2))
    print(what, "nslabs", r[1])
    assert r[1] == nslabs, (what, r[1], nslabs)
    if not pair:
        _check_moments(ops, r[0], r[1], acc, 4 * Hs * Ws, what)


@pytest.mark.parametrize("case", [dict(cin=128, cout=64, k=3, B=2, Hs=24, Ws=20, nslabs=4 * _halo(24, 20, 8)),
                                  dict(cin=256, cout=128, k=3, B=1, Hs=16, Ws=16, nslabs=4 * _halo(16, 16, 16), lo=-2, hi=2),
                                  dict(cin=128, cout=64, k=4, B=2, Hs=24, Ws=20, nslabs=4 * _halo(24, 20, 8), lo=-2, hi=2)],
                         ids=["convT_128to64_24x20", "convT_256to128_16x16", "s2_4x4_bwd_data_128to64"])
def test_merged_parity_classes(case, dev):
    _classes(dev, seed=300 + case["cin"] + case["k"], **case)


# ---- split pair
PAIR_FWD = {
    "halo_64to64_33x17": dict(cin=64, cout=64, taps=fwd_taps(3, 1), B=1, Hi=33, Wi=17, Hs=33, Ws=17, pad_mode=PAD_REFLECT, nslabs=_halo(33, 17, 8)),
    "halo_64to128_23x19": dict(cin=64, cout=128, taps=fwd_taps(3, 1), B=2, Hi=23, Wi=19, Hs=23, Ws=19, nslabs=_halo(23, 19, 16)),
    "gather_s2_64to128_15x13": dict(cin=64, cout=128, taps=fwd_taps(3, 1), B=2, Hi=15, Wi=13, Hs=8, Ws=7, is_=2, nslabs=1),
    "frame_64to64_18x18": dict(cin=64, cout=64, taps=flip_taps(3, 0), B=2, Hi=16, Wi=16, Hs=18, Ws=18, frame=True),
    "f32out_32to2_32x16": dict(cin=32, cout=2, taps=fwd_taps(3, 1), B=2, Hi=32, Wi=16, Hs=32, Ws=16, out_f32=True, bias=True),
}


@pytest.mark.parametrize("name", list(PAIR_FWD))
def test_split_pair_forward(name, dev, pair_mode):
    """x_hi.w_hi + x_hi.w_lo + x_lo.w_hi (x_lo.w_lo dropped, as the ABI states), compared through the pair store."""
    _fwd(dev, seed=400 + sorted(PAIR_FWD).index(name), kind=PAIR, **PAIR_FWD[name])


def test_split_pair_merged_parity_classes(dev, pair_mode):
    _classes(dev, seed=450, cin=128, cout=64, k=3, B=2, Hs=24, Ws=20, nslabs=4 * _halo(24, 20, 8), kind=PAIR)


# ---------------------------------------------------------------------------- ops.conv_wgrad + reduce
class _Spy:
    """Records the slab size ops.conv_wgrad hands to ctg_conv_wgrad and the status the library answers."""

    def __init__(self, fn):
        self.fn, self.calls = fn, []

    def __call__(self, *a):
        rc = self.fn(*a)
        self.calls.append((a[0], a[15], rc))
        return rc


def _wgrad(dev, monkeypatch, *, mc, nc, taps, B, Hs, Ws, Hi, Wi, seed, is_=1, pad_mode=PAD_ZERO, kind=BF16, zfac=1, status=0,
           slabs=None, target_blocks=768, lo=-3, hi=3, crop=(0, 0), min_sps=1, swap_ok=True):
    """One ops.conv_wgrad case through defer=[] and ops.wgrad_reduce_multi, then once more through ctg_wgrad_reduce.
    zfac / status: the evidence (Z = zfac B sps; what ctg_conv_wgrad answered).  slabs: 'linear' | 'tile' compares `part`
    slab by slab."""
    from cta_gan_amd import _lib, ops
    rng = np.random.default_rng(seed)
    pair = kind == PAIR
    nt = len(taps)
    g = pair_grid(rng, (B, Hs, Ws, mc)) if pair else int_grid(rng, (B, Hs, Ws, mc), lo, hi)
    x = pair_grid(rng, (B, Hi, Wi, nc)) if pair else int_grid(rng, (B, Hi, Wi, nc), lo, hi)
    if pair:
        dw, s = wgrad_pair_ref(g, x, taps, is_, pad_mode)
        assert_exact_domain(s, PAIR_GRANULE)
    else:
        dw = wgrad_taps_ref(g, x, taps, is_, pad_mode)
        assert_exact_domain(wgrad_taps_ref(g.abs(), x.abs(), taps, is_, pad_mode))
    lib = _lib.load()
    spy = _Spy(lib.ctg_conv_wgrad)
    monkeypatch.setattr(lib, "ctg_conv_wgrad", spy)
    cdt = torch.float32 if kind == F32 else torch.bfloat16
    if pair:
        gd, xd = ops.to_pair(g.float().to(dev)), ops.to_pair(x.float().to(dev))
    else:
        gd, _ = _slice_of(g.to(dev).to(cdt), 16, 8, 9.0)
        xd, _ = _slice_of(x.to(dev).to(cdt), 8, 0, 9.0)
    mreal, nreal = mc - crop[0], nc - crop[1]
    want = dw[:, :mreal, :nreal].permute(1, 2, 0).contiguous().float()         # dst layout [m][c][t]
    n = mreal * nreal * nt
    what = "wgrad %dx%d %dtaps is%d %s @%dx%d" % (mc, nc, nt, is_, kind, Hs, Ws)
    for use_multi in (True, False):
        dst = torch.full((n + 64,), SENT, dtype=torch.float32, device=dev)
        jobs = [] if use_multi else None
        ops.conv_wgrad(gd, xd, taps, is_, pad_mode, dst, mreal, nreal, nreal * nt, nt, 1, target_blocks=target_blocks, defer=jobs)
        if use_multi:
            part, z = jobs[0][0], jobs[0][2]
            dtype_arg, slab, rc = spy.calls[0]
            sps = _ceil(Hs * Ws, slab)
            print(what, "Z", z, "B*sps", B * sps, "slab", slab, "status", rc)
            assert rc == status and z == zfac * B * sps and sps >= min_sps, (what, rc, z, B, sps)
            assert dtype_arg == (2 if pair else 0 if kind == F32 else 1)
            if slabs is not None:
                ids = linear_slabs(Hs, Ws, slab) if slabs == "linear" else tile_slabs(Hs, Ws, slab)
                assert ids[1] == sps
                _, pref = wgrad_taps_ref(g, x, taps, is_, pad_mode, slabs=ids)
                torch.cuda.synchronize()
                got = part[:z].cpu()
                for zz in range(z):
                    assert torch.equal(got[zz].double(), pref[zz]), \
                        (what, "slab %d (sample %d, slab %d of %d); index = (tap, m, c)" % (zz, zz // sps, zz % sps, sps),
                         first_diff(got[zz].double(), pref[zz]))
            ops.wgrad_reduce_multi(jobs)
        torch.cuda.synchronize()
        d = dst.cpu()
        _assert_bits(d[:n].view(mreal, nreal, nt), want, what + (" (reduce_multi)" if use_multi else " (reduce)"), _where_wgrad(taps))
        assert bool((d[n:] == SENT).all()), what + ": wrote behind the destination"


T3 = fwd_taps(3, 1)

WG_TAP = {
    "bf16_64x64_9taps_6x20": dict(mc=64, nc=64, taps=T3, B=2, Hs=6, Ws=20, Hi=6, Wi=20, target_blocks=96, min_sps=2, slabs="linear"),
    "bf16_reflect_32x32_7x18": dict(mc=32, nc=32, taps=T3, B=2, Hs=7, Ws=18, Hi=7, Wi=18, pad_mode=PAD_REFLECT, target_blocks=6, min_sps=2),
    "bf16_reflect_64x32_7x18": dict(mc=64, nc=32, taps=T3, B=2, Hs=7, Ws=18, Hi=7, Wi=18, pad_mode=PAD_REFLECT, target_blocks=6, min_sps=2),
    "bf16_reflect_32x64_7x18": dict(mc=32, nc=64, taps=T3, B=2, Hs=7, Ws=18, Hi=7, Wi=18, pad_mode=PAD_REFLECT, target_blocks=6, min_sps=2),
    "fp32_64x64_9x11": dict(mc=64, nc=64, taps=T3, B=2, Hs=9, Ws=11, Hi=9, Wi=11, kind=F32, target_blocks=64, min_sps=2),
    "fp32_128x32_9x11": dict(mc=128, nc=32, taps=T3, B=2, Hs=9, Ws=11, Hi=9, Wi=11, kind=F32, pad_mode=PAD_REFLECT, target_blocks=64, min_sps=2),
    "bf16_49taps_32x64_7x18": dict(mc=32, nc=64, taps=fwd_taps(7, 3), B=2, Hs=7, Ws=18, Hi=7, Wi=18, target_blocks=28, min_sps=2),
    "bf16_ragged_last_slab_sps3_13x15": dict(mc=64, nc=64, taps=T3, B=2, Hs=13, Ws=15, Hi=13, Wi=15, pad_mode=PAD_REFLECT, target_blocks=72,
                                             min_sps=3, slabs="linear", crop=(3, 5)),
}


@pytest.mark.parametrize("name", list(WG_TAP))
def test_weight_gradient_per_tap_kernel(name, dev, monkeypatch):
    _wgrad(dev, monkeypatch, seed=500 + sorted(WG_TAP).index(name), **WG_TAP[name])


WG_HALO = {}
for _m, _n in ((64, 64), (64, 32), (32, 64), (32, 32)):
    for _p, _pn in ((PAD_ZERO, "zero"), (PAD_REFLECT, "reflect")):
        WG_HALO["%dx%d_%s_17x33" % (_m, _n, _pn)] = dict(mc=_m, nc=_n, taps=T3, B=2, Hs=17, Ws=33, Hi=17, Wi=33, pad_mode=_p, min_sps=2)
        WG_HALO["%dx%d_%s_8x16" % (_m, _n, _pn)] = dict(mc=_m, nc=_n, taps=T3, B=1, Hs=8, Ws=16, Hi=8, Wi=16, pad_mode=_p)
WG_HALO["64x64_reflect_17x33_slabs"] = dict(mc=64, nc=64, taps=T3, B=2, Hs=17, Ws=33, Hi=17, Wi=33, pad_mode=PAD_REFLECT, min_sps=2,
                                            slabs="tile", crop=(3, 5))
WG_HALO["64x64_1tap_17x33"] = dict(mc=64, nc=64, taps=fwd_taps(1, 0), B=2, Hs=17, Ws=33, Hi=17, Wi=33)
WG_HALO["64x64_4x4_16taps_17x33"] = dict(mc=64, nc=64, taps=fwd_taps(4, 1), B=2, Hs=17, Ws=33, Hi=18, Wi=34)
WG_HALO["16x64_7x7_all_taps_17x33"] = dict(mc=16, nc=64, taps=fwd_taps(7, 3), B=2, Hs=17, Ws=33, Hi=17, Wi=33, pad_mode=PAD_REFLECT)
WG_HALO["32x64_7x7_row_groups_17x33"] = dict(mc=32, nc=64, taps=fwd_taps(7, 3), B=2, Hs=17, Ws=33, Hi=17, Wi=33, pad_mode=PAD_REFLECT)
WG_HALO["256x256_16x16"] = dict(mc=256, nc=256, taps=T3, B=1, Hs=16, Ws=16, Hi=16, Wi=16, pad_mode=PAD_REFLECT)


@pytest.mark.parametrize("name", list(WG_HALO))
def test_weight_gradient_halo_kernel(name, dev, monkeypatch):
    _wgrad(dev, monkeypatch, seed=600 + sorted(WG_HALO).index(name), **WG_HALO[name])


WG_S2 = {
    # G = the conv's output gradient on the small grid, X = its input: Mc = Cout, Nc = Cin
    "s2m_128x64_33x47": dict(mc=128, nc=64, taps=T3, B=2, Hs=17, Ws=24, Hi=33, Wi=47, is_=2, min_sps=2),
    "s2m_256x128_32x64": dict(mc=256, nc=128, taps=T3, B=1, Hs=16, Ws=32, Hi=32, Wi=64, is_=2, min_sps=2, lo=-2, hi=2),
    "s2m_128x64_32x64": dict(mc=128, nc=64, taps=T3, B=2, Hs=16, Ws=32, Hi=32, Wi=64, is_=2, min_sps=2),
    "s2m_256x128_33x47": dict(mc=256, nc=128, taps=T3, B=1, Hs=17, Ws=24, Hi=33, Wi=47, is_=2, min_sps=2, lo=-2, hi=2),
    "four_launches_mc32_33x47": dict(mc=32, nc=64, taps=T3, B=2, Hs=17, Ws=24, Hi=33, Wi=47, is_=2),
    "4x4_s2_128x64_34x38": dict(mc=128, nc=64, taps=fwd_taps(4, 1), B=2, Hs=17, Ws=19, Hi=34, Wi=38, is_=2),
    # transposed conv 128 -> 64 from 17 x 21: roles swapped, G = the layer's input (128 ch) on the small grid, X = dY (64 ch)
    "convT_roles_swapped_128x64_17x21": dict(mc=128, nc=64, taps=T3, B=2, Hs=17, Ws=21, Hi=34, Wi=42, is_=2),
}


@pytest.mark.parametrize("name", list(WG_S2))
def test_weight_gradient_stride2_polyphase(name, dev, monkeypatch):
    _wgrad(dev, monkeypatch, seed=700 + sorted(WG_S2).index(name), **WG_S2[name])


WG_PAIR = {
    # >= 384 workgroups: three sweeps in one launch, one partial per slab (status 0)
    "three_sweeps_256x256_24x32": dict(mc=256, nc=256, taps=T3, B=2, Hs=24, Ws=32, Hi=24, Wi=32, pad_mode=PAD_REFLECT, target_blocks=1024,
                                       status=0, zfac=1),
    # < 384 workgroups: phase_split, three partials per slab (status 3)
    "phase_split_64x64_17x33": dict(mc=64, nc=64, taps=T3, B=2, Hs=17, Ws=33, Hi=17, Wi=33, status=3, zfac=3),
    "s2m_pair_256x128_65x95": dict(mc=256, nc=128, taps=T3, B=2, Hs=33, Ws=48, Hi=65, Wi=95, is_=2, status=0, zfac=1),
}


@pytest.mark.parametrize("name", list(WG_PAIR))
def test_weight_gradient_split_pair(name, dev, monkeypatch, pair_mode):
    _wgrad(dev, monkeypatch, seed=800 + sorted(WG_PAIR).index(name), kind=PAIR, **WG_PAIR[name])


@pytest.mark.parametrize("shape", [(9, 32, 32), (4, 64, 64), (9, 64, 32), (16, 64, 64), (9, 96, 96)],
                         ids=["E9216", "E16384", "E18432", "E65536", "E82944"])
def test_wgrad_reduce_integer_partials(shape, dev):
    """ctg_wgrad_reduce on integer partials, exact: every loop remainder of the three kernels (Z in 1 .. 130), E on both sides of
    the 16 384 and 65 536 thresholds, Mreal < Mc / Nreal < Nc (cropped elements keep the sentinel), accumulate on an integer
    destination."""
    from cta_gan_amd import _lib
    lib = _lib.load()
    nt, mc, nc = shape
    rng = np.random.default_rng(nt * mc)
    zmax = 130
    part = int_grid(rng, (zmax, nt, mc, nc), -3, 3).float()
    pd = part.to(dev)
    st = torch.cuda.current_stream().cuda_stream
    for z in (1, 3, 4, 5, 63, 64, 67, 130):
        tot = part[:z].double().sum(0)                                  # [t][m][c]
        for mreal, nreal in ((mc, nc), (mc - 3, nc - 5)):
            # destination [Mc][Nc][nt] whatever the crop: the cropped rows / columns must keep the sentinel
            dst = torch.full((mc, nc, nt), SENT, dtype=torch.float32, device=dev)
            want = torch.full((mc, nc, nt), SENT, dtype=torch.float64)
            want[:mreal, :nreal] = tot[:, :mreal, :nreal].permute(1, 2, 0)
            assert lib.ctg_wgrad_reduce(pd.data_ptr(), z, nt, mc, nc, dst.data_ptr(), mreal, nreal, nc * nt, nt, 1, 0, st) == 0
            torch.cuda.synchronize()
            _assert_bits(dst, want.float(), "reduce Z=%d %s" % (z, shape))
            pre = int_grid(rng, (mc, nc, nt), -50, 50)
            dst.copy_(torch.where(want == SENT, want, pre).float())
            assert lib.ctg_wgrad_reduce(pd.data_ptr(), z, nt, mc, nc, dst.data_ptr(), mreal, nreal, nc * nt, nt, 1, 1, st) == 0
            torch.cuda.synchronize()
            _assert_bits(dst, torch.where(want == SENT, want, want + pre).float(), "reduce accumulate Z=%d %s" % (z, shape))


def test_wgrad_reduce_multi_25_jobs(dev):
    """25 reductions in one ops.wgrad_reduce_multi call = two launches (24 + 1): mixed lane-sharing shifts (0, 4, 5), element counts
    that are no multiple of a block's share (a job ends inside a block), crops, accumulate, the scalar tail of the slab loop."""
    from cta_gan_amd import ops
    rng = np.random.default_rng(77)
    shapes = [(9, 32, 32), (4, 64, 64), (9, 64, 32), (16, 64, 64), (9, 96, 96), (3, 5, 7), (1, 16, 512), (1, 33, 17)]
    zs = [1, 3, 4, 5, 63, 64, 67, 130]
    jobs, wants, dsts = [], [], []
    for i in range(25):
        nt, mc, nc = shapes[(i * 3) % len(shapes)]
        z = zs[(i * 5 + i // 8) % len(zs)]
        part = int_grid(rng, (z, nt, mc, nc), -3, 3).float()
        mreal, nreal = (mc, nc) if i % 2 else (mc - 2, nc - 3)
        acc = int(i % 3 == 0)
        pre = int_grid(rng, (mc, nc, nt), -50, 50)
        want = torch.full((mc, nc, nt), SENT, dtype=torch.float64)
        want[:mreal, :nreal] = part.double().sum(0)[:, :mreal, :nreal].permute(1, 2, 0) + (pre[:mreal, :nreal] if acc else 0)
        dst = torch.where(want == SENT, want, pre if acc else torch.full_like(pre, 123.0)).float().to(dev)
        jobs.append((part.to(dev), dst.data_ptr(), z, nt, mc, nc, mreal, nreal, nc * nt, nt, 1, acc, dst))
        wants.append(want.float())
        dsts.append(dst)
    ops.wgrad_reduce_multi(jobs)
    torch.cuda.synchronize()
    for i, (d, w) in enumerate(zip(dsts, wants)):
        _assert_bits(d, w, "reduce_multi job %d (Z=%d, %s)" % (i, jobs[i][2], jobs[i][3:6]))


# ---------------------------------------------------------------------------- first- and last-layer kernels
def _planes(rng, b, h, w, cin, lo=-3, hi=3):
    return [int_grid(rng, (b, h, w), lo, hi) for _ in range(cin)]


@pytest.mark.parametrize("size", [(4, 4), (16, 16), (17, 33), (40, 56)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("conf", [(1, 7, 1, 3, PAD_REFLECT, 64, True), (1, 7, 1, 3, PAD_REFLECT, 64, False), (1, 4, 2, 1, PAD_ZERO, 64, False),
                                  (2, 3, 1, 1, PAD_ZERO, 32, False), (2, 5, 1, 2, PAD_REFLECT, 64, False), (1, 5, 1, 2, PAD_ZERO, 48, True)],
                         ids=["cin1_7x7_reflect_kxw", "cin1_7x7_reflect", "cin1_4x4_s2", "cin2_3x3", "cin2_5x5_reflect", "cin1_5x5_kxw_48"])
def test_first_layer_conv_smallcin(conf, size, dev):
    """ops.conv_smallcin from integer image planes: plain (moments, exact) and bias + LeakyReLU."""
    from cta_gan_amd import ops
    cin, k, stride, pad, pad_mode, cout, kxw = conf
    h, w = size
    rng = np.random.default_rng(cin * 100 + k * 10 + h)
    b = 2
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    planes = _planes(rng, b, h, w, cin)
    x = torch.stack(planes, dim=-1)                                     # [B, H, W, cin]
    wt = int_grid(rng, (cout, cin, k, k), -3, 3)
    wtaps = wt.permute(2, 3, 0, 1).reshape(k * k, cout, cin)
    taps = fwd_taps(k, pad)
    acc = conv_taps_ref(x, wtaps, taps, ho, wo, stride, pad_mode)
    assert_exact_domain(conv_taps_ref(x.abs(), wtaps.abs(), taps, ho, wo, stride, pad_mode))
    assert_exact_domain(moments_ref(acc)[..., 1])
    bs = bias_grid(rng, cout)
    npad = _ceil(cout, 32) * 32
    w2d = wt.reshape(cout, cin * k * k).float().to(dev)
    if kxw:
        assert ops.kxw_ok(cin, cout, k, stride, torch.bfloat16)
        wp = ops.kxw_pack(w2d, k, npad, torch.bfloat16)
    else:
        wp = ops.weight_pack(w2d.contiguous(), torch.bfloat16, 1, cout, cin * k * k, npad, 64 if cin * k * k > 32 else 32, cin * k * k, 1, 0)
    s = [p.float().to(dev).contiguous() for p in planes]
    what = "smallcin cin%d k%d s%d %dx%d kxw=%d" % (cin, k, stride, h, w, kxw)
    for bias, act in ((None, ACT_NONE), (bs, ACT_LRELU)):
        yfull = torch.full((b, ho, wo, cout + 16), SENT, dtype=torch.bfloat16, device=dev)
        y = yfull[..., 8:8 + cout]
        part, ns = ops.conv_smallcin(s[0], s[1] if cin == 2 else None, k, stride, pad, pad_mode, wp, npad,
                                     None if bias is None else bias.float().to(dev), act, y, cout, want_stats=True, kxw=kxw)
        torch.cuda.synchronize()
        want = torch.full((b, ho, wo, cout + 16), SENT, dtype=torch.bfloat16)
        want[..., 8:8 + cout] = store_bf16(epilogue(acc, bias, act))
        _assert_bits(yfull, want, what + " act %d" % act)
        if bias is None:
            assert ns == _ceil(ho, 16) * _ceil(wo, 16), (what, ns)
            _check_moments(ops, part, ns, acc, ho * wo, what)


@pytest.mark.parametrize("size", [(4, 4), (20, 32), (21, 33), (50, 70)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", [BF16, F32])
def test_last_layer_conv_tail7(kind, size, dev):
    """ops.conv_tail7 (64 -> 1, 7x7, reflection padding 3): ACT_NONE exact, tanh within the fp32 forward bound."""
    from cta_gan_amd import ops
    h, w = size
    rng = np.random.default_rng(h * 7 + w)
    b = 2
    x = int_grid(rng, (b, h, w, 64), -3, 3)
    wt = int_grid(rng, (1, 64, 7, 7), -3, 3)
    wtaps = wt.permute(2, 3, 0, 1).reshape(49, 1, 64)
    taps = fwd_taps(7, 3)
    acc = conv_taps_ref(x, wtaps, taps, h, w, 1, PAD_REFLECT)
    assert_exact_domain(conv_taps_ref(x.abs(), wtaps.abs(), taps, h, w, 1, PAD_REFLECT))
    bs = bias_grid(rng, 1)
    cdt = torch.float32 if kind == F32 else torch.bfloat16
    xd, _ = _slice_of(x.to(dev).to(cdt), 16, 8, 9.0)
    wp = ops.tail7_pack(wt.float().to(dev), cdt)
    bd = bs.float().to(dev)
    y = torch.full((b, h, w), SENT, dtype=torch.float32, device=dev)
    ops.conv_tail7(xd, wp, bd, y, ACT_NONE)
    torch.cuda.synchronize()
    _assert_bits(y, store_f32(epilogue(acc, bs))[..., 0], "tail7 %s %dx%d" % (kind, h, w))
    # tanh on sparse weights (pre-activations of a few units: not saturated)
    wt2 = wt * torch.from_numpy((rng.random((1, 64, 7, 7)) < 0.004).astype(np.float64))
    acc2 = conv_taps_ref(x, wt2.permute(2, 3, 0, 1).reshape(49, 1, 64), taps, h, w, 1, PAD_REFLECT)
    unsat = int((tanh_ref(acc2, bs).abs() < 0.995).sum())
    assert unsat >= 4, "tanh case is saturated: only %d pre-activations below 3" % unsat
    ops.conv_tail7(xd, ops.tail7_pack(wt2.float().to(dev), cdt), bd, y, ACT_TANH)
    torch.cuda.synchronize()
    err = float((y.double().cpu() - tanh_ref(acc2, bs)[..., 0]).abs().max())
    print("tail7 tanh", kind, size, "max err %.3g" % err, "unsaturated", unsat)
    assert err <= 2e-4, ("tail7 tanh", kind, size, err)


@pytest.mark.parametrize("size", [(4, 4), (5, 7), (17, 33), (19, 19)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("pad", [0, 1, 2])
def test_patchgan_last_layer_cout1(pad, size, dev):
    """ops.conv_cout1_fwd / _bwd / _wgrad (512 -> 1, 4x4, fp32 vector-ALU kernels, fp32 master weights): values in [-3, 3] so
    that the 8192-term sums exceed 2^10."""
    from cta_gan_amd import ops
    hi_, wi_ = size
    ho, wo = hi_ + 2 * pad - 3, wi_ + 2 * pad - 3
    rng = np.random.default_rng(pad * 100 + hi_ + wi_)
    b = 2
    x = int_grid(rng, (b, hi_, wi_, 512), -3, 3)
    wt = int_grid(rng, (1, 512, 4, 4), -3, 3)
    g = int_grid(rng, (b, ho, wo, 1), -3, 3)
    wtaps = wt.permute(2, 3, 0, 1).reshape(16, 1, 512)
    taps = fwd_taps(4, pad)
    acc = conv_taps_ref(x, wtaps, taps, ho, wo, 1, PAD_ZERO)
    assert_exact_domain(conv_taps_ref(x.abs(), wtaps.abs(), taps, ho, wo, 1, PAD_ZERO))
    # dx[q][ci] = sum_taps g[q + pad - k] w[k][ci]: N = Cin, K = 1
    wb = wt.permute(2, 3, 1, 0).reshape(16, 512, 1)
    dxr = conv_taps_ref(g, wb, flip_taps(4, pad), hi_, wi_, 1, PAD_ZERO)
    dwr = wgrad_taps_ref(g, x, taps, 1, PAD_ZERO)                       # [16][1][512]
    assert_exact_domain(wgrad_taps_ref(g.abs(), x.abs(), taps, 1, PAD_ZERO))
    bs = bias_grid(rng, 1)
    xd, _ = _slice_of(x.to(dev).bfloat16(), 16, 8, 9.0)
    w16 = ops.cout1_pack(wt.float().to(dev))
    what = "cout1 pad %d %dx%d" % (pad, hi_, wi_)
    for act in (ACT_NONE, ACT_LRELU):
        y = torch.full((b, ho, wo), SENT, dtype=torch.float32, device=dev)
        ops.conv_cout1_fwd(xd, w16, bs.float().to(dev), y, act, pad)
        torch.cuda.synchronize()
        _assert_bits(y, store_f32(epilogue(acc, bs, act))[..., 0], what + " fwd act %d" % act)
    gd = g[..., 0].float().to(dev).contiguous()
    dxfull = torch.full((b, hi_, wi_, 512 + 16), SENT, dtype=torch.bfloat16, device=dev)
    ops.conv_cout1_bwd(gd, w16, dxfull[..., 8:520], pad)
    torch.cuda.synchronize()
    want = torch.full((b, hi_, wi_, 528), SENT, dtype=torch.bfloat16)
    want[..., 8:520] = store_bf16(epilogue(dxr))
    _assert_bits(dxfull, want, what + " bwd")
    dw = torch.full((1, 512, 4, 4), SENT, dtype=torch.float32, device=dev)
    ops.conv_cout1_wgrad(gd, xd, dw, pad)
    torch.cuda.synchronize()
    _assert_bits(dw, dwr[:, 0, :].t().reshape(1, 512, 4, 4).float(), what + " wgrad")


@pytest.mark.parametrize("size", [(4, 4), (16, 16), (17, 33), (40, 56)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("conf", [(1, 7, 3, PAD_REFLECT, 64), (2, 3, 1, PAD_ZERO, 32), (2, 5, 2, PAD_REFLECT, 64), (1, 5, 2, PAD_ZERO, 32)],
                         ids=["cin1_7x7_reflect_mc64", "cin2_3x3_mc32", "cin2_5x5_reflect_mc64", "cin1_5x5_mc32"])
def test_first_layer_weight_gradient_corr_smallcin(conf, size, dev):
    """ops.corr_smallcin: dW[m][(c, ky, kx)] = sum_q g[q][m] image_c[pad(q + k - pad)] of a stride-1 first layer.  The wrapper
    sizes `wgs` itself, min(tiles, ceil(512 / B)): with B = 2 every workgroup has exactly one tile here (1 .. 12 tiles); the
    test below has several tiles per workgroup."""
    from cta_gan_amd import ops
    cin, k, pad, pad_mode, mc = conf
    h, w = size
    rng = np.random.default_rng(cin * 50 + k + h + mc)
    b = 2
    planes = _planes(rng, b, h, w, cin)
    x = torch.stack(planes, dim=-1)
    g = int_grid(rng, (b, h, w, mc), -3, 3)
    taps = fwd_taps(k, pad)
    dwr = wgrad_taps_ref(g, x, taps, 1, pad_mode)                       # [kk][mc][cin]
    assert_exact_domain(wgrad_taps_ref(g.abs(), x.abs(), taps, 1, pad_mode))
    gd, _ = _slice_of(g.to(dev).bfloat16(), 16, 8, 9.0)
    s = [p.float().to(dev).contiguous() for p in planes]
    kk = cin * k * k
    dst = torch.full((mc * kk + 64,), SENT, dtype=torch.float32, device=dev)
    ops.corr_smallcin(gd, 0, PAD_ZERO, s[0], s[1] if cin == 2 else None, k, pad, pad_mode, h, w, dst, 0, mc, kk, kk, 1)
    torch.cuda.synchronize()
    want = dwr.permute(1, 2, 0).reshape(mc, kk).float()                 # [m][(c, ky kx)]
    d = dst.cpu()
    _assert_bits(d[:mc * kk].view(mc, kk), want, "corr_smallcin cin%d k%d mc%d %dx%d" % (cin, k, mc, h, w))
    assert bool((d[mc * kk:] == SENT).all())


@pytest.mark.parametrize("grid", [(171, 17, 64), (64, 40, 56)], ids=["B171_17x64_q2_rem2", "B64_40x56_q1_rem4"])
@pytest.mark.parametrize("conf", [(1, 7, 3, PAD_REFLECT, 64), (2, 3, 1, PAD_ZERO, 32)], ids=["cin1_7x7_reflect_mc64", "cin2_3x3_mc32"])
def test_first_layer_weight_gradient_corr_smallcin_several_tiles_per_workgroup(conf, grid, dev):
    """ops.corr_smallcin with fewer workgroups than tiles (wgs = ceil(512 / B) < tiles): a workgroup walks q or q + 1 tiles
    (csrc/corr_small.hip: the G prefetch across tiles and the uneven `rem` split).  B = 171: 3 workgroups for the 2 x 4 = 8 tiles
    of 17 x 64 (q 2, rem 2: shares 3, 3, 2; ragged rows); B = 64: 8 workgroups for the 3 x 4 = 12 tiles of 40 x 56 (q 1, rem 4)."""
    from cta_gan_amd import ops
    cin, k, pad, pad_mode, mc = conf
    b, h, w = grid
    ntiles, wgs = _ceil(h, 16) * _ceil(w, 16), _ceil(512, b)
    assert wgs < ntiles and ntiles % wgs != 0
    rng = np.random.default_rng(b + cin * 50 + k + mc)
    planes = _planes(rng, b, h, w, cin)
    x = torch.stack(planes, dim=-1)
    g = int_grid(rng, (b, h, w, mc), -3, 3)
    taps = fwd_taps(k, pad)
    dwr = wgrad_taps_ref(g, x, taps, 1, pad_mode)
    assert_exact_domain(torch.tensor(9.0 * b * h * w))                  # >= S: |g| |x| <= 9 per pixel
    gd, _ = _slice_of(g.to(dev).bfloat16(), 16, 8, 9.0)
    s = [p.float().to(dev).contiguous() for p in planes]
    kk = cin * k * k
    dst = torch.full((mc * kk + 64,), SENT, dtype=torch.float32, device=dev)
    ops.corr_smallcin(gd, 0, PAD_ZERO, s[0], s[1] if cin == 2 else None, k, pad, pad_mode, h, w, dst, 0, mc, kk, kk, 1)
    torch.cuda.synchronize()
    d = dst.cpu()
    _assert_bits(d[:mc * kk].view(mc, kk), dwr.permute(1, 2, 0).reshape(mc, kk).float(),
                 "corr_smallcin cin%d k%d mc%d B%d %dx%d (%d tiles, %d workgroups)" % (cin, k, mc, b, h, w, ntiles, wgs))
    assert bool((d[mc * kk:] == SENT).all())
