"""GPU: the InstanceNorm core of csrc/norm_act.hip -- statistics pass, the two finalizers, the four elementwise kernels --
element by element against tests/instnorm_ref.py (float64, CPU; checked against stock torch by tests/test_instnorm_ref.py).

Exact grid.  x and res are integers in [-8, 8], gradients integers in [-4, 4]; mean (an integer in [-2, 2]), rstd (1/4, 1/2, 1
or 2), s1 (a multiple of 1/4, |s1| <= 2) and s2 (a multiple of 1/4, |s2| <= 1) are SUPPLIED by the test and differ per (sample,
channel).  Then xhat is a multiple of 1/4 below 20, every forward value fits bf16, dx is a multiple of 1/64 (|dx| <= 52 without
a fold, <= 116 with nine folded sources) and the partial sums are integers / multiples of 1/4 far below 2^24: for ACT_NONE and
ACT_RELU nothing rounds in fp32 in ANY summation order, with or without FMA contraction, and the stored bits have to equal the
float64 reference rounded once to the storage type (`_assert_stored`: torch.equal on the bit patterns of every plane; it first
asserts that the reference IS an fp32 value).  A dropped pixel, a skipped trip, a missing fold term or a wrong channel's
parameter is a difference at a named element.

LeakyReLU (0.2f v rounds).
  pinned kernels (in_apply_kernel, in_bwd_apply_kernel: fp contract off, one explicit FMA): bit for bit against the op-for-op
      reference (forward_ops / backward_ops).
  fused *_part kernels, forward: no contract pragma.  With a residual each element has to be fl(fl(a) + r) or the one-FMA form
      fl(a + r), a = the activation's last product, rounded to storage (`_assert_one_of`); without a residual the result is exact.
      (Their mean / rstd come out of the kernel's own prologue and are no grid values, so the same two forms are what ANY
      activation with a residual may give there: for ACT_NONE / ACT_RELU a = d rstd, d = fl(x - mean).)
  fused *_part kernels, backward: per element |got - want| <= r (|want| + S), S = rstd (|g m| + |s1| + |xhat s2|), r = R[kind] of
      test_spatial_glue_gpu.py (a few fp32 roundings / one bf16 rounding / the pair's storage precision).
  partial sums: per entry |got - want| <= n 2^-24 sum|term|, n = the slab's pixel count (the worst case of sequential fp32
      summation; one dropped pixel is a whole term).
ops.in_finalize / the prologues: mean and both mode-1 outputs bit-exact (exactly summable partials: <= 1024 fp32 values whose
sum fits 53 bits; sum x invHW is exact in double, then ONE rounding to fp32); rstd within 1 fp32 ulp of the float64 formula (the
compiler may fuse b invHW - m^2, sqrt and the divide are library calls).  The cases keep |mean| <= 8 so that a fused / unfused
b invHW - m^2 differs by < 1e-14 absolute, 1e-9 of var + eps: far inside one fp32 ulp.

Which case pins which path
  moments_partial_kernel MODE 0   test_statistics_mode0: one slab (1,2,2); ragged slabs (3,9,15), (17,20,20); empty last slab
                                  (2,82,100); 35 pixels in one slab, fewer than the 64 / 256 pixel lanes (2,5,7); C = one chunk,
                                  8 chunks, 64 chunks per pixel (the LDS reduction over 256, 32, 4 pixel lanes)
  moments_partial_kernel MODE 1   test_statistics_mode1: the same, x no activation / ReLU / LeakyReLU x pad 0, 1, 3, plus
                                  H = pad + 1 and W = pad + 1 (interior rows with three folded sources); DT_MIX; xhat == 0 on
                                  1 / 17 of the elements (strict mask)
  moments_finalize_wave_kernel    test_in_finalize: nslabs 1, 63, 64, 65, 128, 129, 200, 1024 (the BatchNorm reshape), both
                                  modes, HW 4096 and 16510, tail slabs that drive E[x^2] - m^2 below 0
  wg_finalize + in_apply_part     test_fused_forward: partials of ops.in_partial (every slab arrangement above) and integer
                                  partials with nslabs 1, 7, 128; C = half a channel group, one group, four groups; published
                                  mean / rstd of EVERY group; 129 slabs refused
  wg_finalize + in_bwd_apply_part test_fused_backward: the same for the backward, pads 0, 1, 3, DT_MIX; 129 slabs take
                                  in_finalize + in_bwd_apply (bit for bit the pinned kernel's result)
  in_apply_kernel                 test_in_apply_lane_trips (less than a batch / exactly one / one or half / one for all lanes),
                                  test_large_bf16 (per 4: a batch of 4 or three single trips), test_large_fp32 (per 8: two
                                  batches, or one batch and three single trips); every activation x residual; in place
  in_bwd_apply_kernel             test_in_bwd_apply_lane_trips, the two large cases (pad 0, batched loop), test_in_bwd_padded
                                  (pads 1, 2, 3 incl. H = pad + 1: the one-pixel-per-trip fold loop; ops.in_bwd end to end);
                                  batch-wide s1 / s2 expanded over B and zeros (BatchNorm training / eval)
  refusals                        test_refusals
Every output (and every input) is a channel slice of a wider SENT-filled buffer; `outside_unchanged` is asserted for each.

Not covered here: the partial moments a conv epilogue emits (tests/test_conv_exact_gpu.py owns them: their slabs are tiles, not
runs of row-major pixels); nslabs values the wrappers cannot request for the statistics kernels (ops._nslabs yields
1 .. 128 by its own rule: other counts, and slab counts that are no result of it for a given shape, never reach
moments_partial_kernel -- ops.in_finalize and the fused kernels do get arbitrary counts here, from synthetic partials); ACT_TANH
/ ACT_SIGMOID after an InstanceNorm (the ACT_RT instantiation: no network has one); the CTG_NO_SMALLB grid rule.

Ill-conditioned statistics (test_ill_conditioned_statistics) leave the grid: random channels with |mean| / sigma = 0, 8, 64
against float64, rel(rstd) <= n 2^-24 (1 + (mean / sigma)^2), n = trips per lane + pixel lanes (the adds behind one partial):
the cancellation of the single-pass E[x^2] - m^2.

Largest measured error as a fraction of each derived bound (printed by the tests as "maxerr ..."; MI355X):
  bound                                      fp32    bf16    pair    mix
  partial sums, LeakyReLU (n 2^-24 sum|t|)   0.371   0.53    0.53    0.53
  in_bwd_stats fused (r (|want| + S))        0.254   0.498   0.488   0.498 (bf16 output)
  in_stats rstd, |mean| / sigma = 0          0.031   0.034   0.039
  in_stats rstd, |mean| / sigma = 8          0.028   0.006   0.020
  in_stats rstd, |mean| / sigma = 64         0.021   0.006   0.030
(a bf16 or pair result that is one value rounded once sits at half its bound by construction.)  The single-pass E[x^2] - m^2
stays a factor 25 inside its derived bound: no shifted partials are needed.

Found by this module: nothing in the kernels.

Mutation checks.  Each mutation was built once into a copy of csrc/norm_act.hip outside the repository (never committed; each
stays in bounds) and the module run once against it; every one fails the cases named, and no others:
  a each slab's last pixel dropped (pend - 1)                     -> all of test_statistics_mode0 and test_statistics_mode1,
                                                                     test_in_bwd_padded (ops.in_bwd), test_ill_conditioned_statistics
  b MODE 1 mask >= instead of >                                   -> all of test_statistics_mode1, test_in_bwd_padded (ops.in_bwd)
  c fold_srcs y <= p -> y < p                                     -> test_statistics_mode1[pad1-*, pad3-*], test_in_bwd_padded,
                                                                     test_fused_backward[*-1, *-3]
  d ragged-tail loop of in_apply_loop stopping one trip early     -> test_in_apply_lane_trips (all but one_batch_all, whose lanes
                                                                     have no tail), test_large_bf16_*, test_large_fp32_*
  e wg_finalize skipping its first stripe pass                    -> all of test_fused_forward and test_fused_backward
  f moments_finalize_wave_kernel reading only the first 64 slabs  -> test_in_finalize[65, 128, 129, 200, 1024], test_fused_forward
                                                                     (its ops.in_finalize twin), test_fused_backward (129 slabs)
  g a1 / a2 swapped in in_bwd_px                                  -> all of test_in_bwd_apply_lane_trips and test_in_bwd_padded,
                                                                     test_fused_backward (129 slabs), the two large cases
  h in_apply_part_kernel publishing mean / rstd for group 0 only  -> all of test_fused_forward (the four-group channel counts)
"""
import pytest
import torch

import instnorm_ref as ref
from test_spatial_glue_gpu import (BIAS_SHAPES, SENT, _Buf, _bits, _check_slab_arrangement, _close, _mode, _note,  # noqa: F401
                                   _stored_equal, dev)

pytestmark = pytest.mark.gpu

ACTS = (ref.ACT_NONE, ref.ACT_RELU, ref.ACT_LRELU)
FWD_KINDS = ("fp32", "bf16", "pair")
BWD_KINDS = ("fp32", "bf16", "pair", "mix")          # "mix": pair-typed saved x, bf16 gradients in and out (DT_MIX)
STAT_SHAPES = dict(BIAS_SHAPES, fewer_pixels_than_lanes=(2, 5, 7))
LANE_SHAPES = {"lt_batch_1chunk": (2, 5, 7, 8), "one_batch_32chunks": (1, 3, 3, 256), "one_or_half_batch": (3, 33, 17, 64),
               "one_batch_all": (1, 128, 64, 32)}


def _xg(kind):
    """(kind of the saved activation, kind of the gradients and of dx)."""
    return ("pair", "bf16") if kind == "mix" else (kind, kind)


def _epc(kind):
    return 4 if kind == "fp32" else 8


def _c(kind, c):
    """The channel count with the same chunks per pixel: fp32 chunks hold 4 channels, the bf16 types 8."""
    return c // 2 if kind == "fp32" else c


def _ints(shape, lo, hi, seed, device="cpu"):
    gen = torch.Generator(device=device).manual_seed(seed)
    return torch.randint(lo, hi + 1, tuple(shape), generator=gen, device=device).float()


class _Stats:
    """Grid statistics per (sample, channel): fp32 on the device for the kernels, float64 on `rdev` for the reference."""

    def __init__(self, b, c, seed, dev, rdev="cpu"):
        v = dict(mean=_ints((b, c), -2, 2, seed), rstd=2.0 ** _ints((b, c), -2, 1, seed + 1),
                 s1=_ints((b, c), -8, 8, seed + 2) / 4, s2=_ints((b, c), -4, 4, seed + 3) / 4)
        for k, t in v.items():
            setattr(self, k, t.to(dev))
            setattr(self, k + "64", t.double().to(rdev))


def _first_bad(bad):
    return tuple(int(v) for v in bad.nonzero()[0])


def _assert_stored(ops, kind, buf, want, what):
    """`buf` holds the float64 reference `want` rounded ONCE to its storage type, bit for bit, and nothing outside its slice
    changed.  The reference has to be an fp32 value (the exactness argument of the module docstring, re-asserted)."""
    assert torch.equal(ref.f32(want), want), (what, "the reference is no fp32 value: the case is off the exact domain")
    if not _stored_equal(ops, kind, buf.t, want.float().to(buf.raw.device)):
        got, exp = buf.get(), ref.stored_value(kind, want.cpu())
        bad = got != exp
        if not bool(bad.any()):
            raise AssertionError("%s %s: the stored planes differ from the reference only in the sign of zeros or in how the "
                                 "pair splits" % (what, kind))
        i = _first_bad(bad)
        raise AssertionError("%s %s: %d of %d elements differ, first at (n, y, x, c) = %s: got %r want %r" % (
            what, kind, int(bad.sum()), bad.numel(), i, float(got[i]), float(exp[i])))
    assert buf.outside_unchanged(), (what, "wrote outside its channel slice")


def _planes(buf):
    p = [buf.t.double().cpu()]
    return p + [buf.lo().double().cpu()] if buf.kind == "pair" else p


def _assert_one_of(kind, buf, cands, what):
    """Every element of `buf` is one of the candidate fp32 results rounded to storage (all planes of that candidate)."""
    got = _planes(buf)
    ok = torch.zeros(got[0].shape, dtype=torch.bool)
    for cand in cands:
        assert torch.equal(ref.f32(cand), cand)
        m = torch.ones_like(ok)
        for g, w in zip(got, ref.store(kind, cand)):
            m &= g == w
        ok |= m
    if not bool(ok.all()):
        i = _first_bad(~ok)
        raise AssertionError("%s %s: %d of %d elements are neither candidate, first at %s: got %r, candidates %r" % (
            what, kind, int((~ok).sum()), ok.numel(), i, float(sum(got)[i]), [float(c[i]) for c in cands]))
    assert buf.outside_unchanged(), (what, "wrote outside its channel slice")


def _ulps(got, want64):
    """Distance in fp32 units in the last place between fp32 `got` and the float64 `want64` rounded to fp32 (positive values)."""
    a = got.detach().cpu().contiguous().view(torch.int32).long()
    b = want64.float().contiguous().view(torch.int32).long()
    return (a - b).abs()


def _assert_sums(name, kind, got, want, mag, count, exact, what):
    """Partial sums [B, ns, C, 2]: bit-exact, or per entry within n 2^-24 sum|term| (n = the slab's pixel count)."""
    got = got.double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if exact:
        assert torch.equal(ref.f32(want), want), (what, "the reference sums are no fp32 values")
        bad = got != want
    else:
        bound = count.double()[None, :, None, None] * 2.0 ** -24 * mag
        err = (got - want).abs()
        _note(name, kind, float((err / bound.clamp_min(1e-300))[bound > 0].max()) if bool((bound > 0).any()) else 0.0)
        bad = err > bound
    if bool(bad.any()):
        i = _first_bad(bad)
        raise AssertionError("%s %s: %d of %d partial sums wrong, first at (n, slab, c, which) = %s: got %r want %r" % (
            what, kind, int(bad.sum()), bad.numel(), i, float(got[i]), float(want[i])))


def _sliced(kind, shape, dev, c0, extra):
    return _Buf(kind, shape, dev, c0=c0, extra=extra)


# ------------------------------------------------------------------------------------------------------------------ 1 statistics
def _stat_channels(kind):
    return (4, 32, 256) if kind == "fp32" else (8, 64, 512)


@pytest.mark.parametrize("name", list(STAT_SHAPES))
@pytest.mark.parametrize("kind", FWD_KINDS)
def test_statistics_mode0(kind, name, dev):
    """ops.in_partial: the whole [B, ns, C, 2] tensor of (sum x, sum x^2), bit for bit."""
    with _mode(kind) as ops:
        b, h, w = STAT_SHAPES[name]
        if name in BIAS_SHAPES:
            _check_slab_arrangement(ops, name, b, h * w)
        else:
            assert ops._nslabs(b, h * w) == 1 and h * w < 256 // 4        # fewer pixels than the fewest pixel lanes but C = 512's
        for n, c in enumerate(_stat_channels(kind)):
            x = _sliced(kind, (b, h, w, c), dev, 8, 8).put(_ints((b, h, w, c), -8, 8, 10 + n)).watch()
            part, ns = ops.in_partial(x.t)
            assert ns == ops._nslabs(b, h * w) and tuple(part.shape) == (b, ns, c, 2)
            want, mag, count = ref.partials(x.get(), ns)
            assert float(mag.max()) < 2.0 ** 24
            _assert_sums("in_partial", kind, part, want, mag, count, True, ("mode 0", name, c))
            assert x.outside_unchanged()


def _mode1_cases():
    out = []
    for pad in (0, 1, 3):
        for name, (b, h, w) in STAT_SHAPES.items():
            if pad < min(h, w):
                out.append((pad, name))
        if pad:
            out += [(pad, "h_w_pad_plus_1"), (pad, "h_pad_plus_1"), (pad, "w_pad_plus_1")]
    return out


def _mode1_shape(pad, name):
    return {"h_w_pad_plus_1": (2, pad + 1, pad + 1), "h_pad_plus_1": (2, pad + 1, 9), "w_pad_plus_1": (2, 9, pad + 1)}.get(
        name) or STAT_SHAPES[name]


@pytest.mark.parametrize("pad,name", _mode1_cases(), ids=["pad%d-%s" % c for c in _mode1_cases()])
@pytest.mark.parametrize("kind", BWD_KINDS)
def test_statistics_mode1(kind, pad, name, dev):
    """ops.in_bwd_partial: (sum g m, sum g m xhat) per slab with g = fold(dout).  No activation and ReLU: bit for bit;
    LeakyReLU: the summation bound."""
    with _mode(kind) as ops:
        xk, gk = _xg(kind)
        b, h, w = _mode1_shape(pad, name)
        if name in BIAS_SHAPES:
            _check_slab_arrangement(ops, name, b, h * w)
        ns = ops._nslabs(b, h * w)
        for n, c in enumerate(_stat_channels(kind)):
            seed = 100 + 10 * pad + n
            x = _sliced(xk, (b, h, w, c), dev, 8, 8).put(_ints((b, h, w, c), -8, 8, seed))
            d = _sliced(gk, (b, h + 2 * pad, w + 2 * pad, c), dev, 16, 8).put(_ints((b, h + 2 * pad, w + 2 * pad, c), -4, 4, seed + 1))
            st = _Stats(b, c, seed + 2, dev)
            x64, g64 = x.get(), ref.fold(d.get(), pad)
            if x64.numel() >= 2000:      # x == mean on 1 / 17 of the grid: the strict mask is exercised
                assert float((ref.xhat(x64, st.mean64, st.rstd64) == 0).double().mean()) > 0.04
            for act in ACTS:
                part = ops.in_bwd_partial(x.t, d.t, pad, st.mean, st.rstd, act)
                assert tuple(part.shape) == (b, ns, c, 2)
                want, mag, count = ref.partials(x64, ns, 1, g64, st.mean64, st.rstd64, act)
                assert float(mag.max()) < 2.0 ** 20
                _assert_sums("in_bwd_partial lrelu", kind, part, want, mag, count, act != ref.ACT_LRELU,
                             ("mode 1", name, pad, c, act))


# ------------------------------------------------------------------------------------------------------------------ 2 finalize
def _int_partials(b, ns, c, hw, seed, clamp_every=4):
    """Integer partials [B, ns, C, 2] (fp32, CPU) with |sum of the firsts| <= 4 HW (|mean| <= 4) and seconds in [0, 16 k];
    every `clamp_every`-th channel's last slab is negative enough for a total of -5: var < 0 without the clamp."""
    k = max(1, 4 * hw // ns)
    p = torch.stack((_ints((b, ns, c), -k, k, seed), _ints((b, ns, c), 0, 16 * k, seed + 1)), -1)
    if clamp_every:
        sel = torch.arange(c) % clamp_every == clamp_every - 1
        rest = p[:, :-1, :, 1].sum(1)
        p[:, -1, sel, 1] = (-rest - 5.0)[:, sel]
    assert float(p.abs().sum(1).max()) < 2.0 ** 24 and torch.equal(p, p.round())
    return p


def _check_finalized(got_a, got_b, part64, hw, mode, what):
    """(mean, rstd) / the two means a kernel finalized from `part64` against the float64 formula."""
    wa, wb = ref.finalize(part64, hw, mode)
    assert torch.equal(got_a.double().cpu(), ref.f32(wa)), (what, "first output (mean) not bit-exact",
                                                           _first_bad(got_a.double().cpu() != ref.f32(wa)))
    if mode == 1:
        assert torch.equal(got_b.double().cpu(), ref.f32(wb)), (what, "second mean not bit-exact")
    else:
        u = _ulps(got_b, wb)
        assert int(u.max()) <= 1, (what, "rstd %d ulps off at %s" % (int(u.max()), _first_bad(u > 1)))
        assert bool(torch.isfinite(got_b).all())


@pytest.mark.parametrize("nslabs", [1, 63, 64, 65, 128, 129, 200, 1024])
def test_in_finalize(nslabs, dev):
    with _mode("fp32") as ops:
        for hw in (4096, 16510):
            b, c = (1, 24) if nslabs == 1024 else (3, 8)          # 1024: engine.bnorm_forward's [1, b nsl, C, 2]
            p = _int_partials(b, nslabs, c, hw, 1000 + nslabs)
            a = p.double().sum(1)
            var = a[..., 1] * ref.inv_hw(hw) - (a[..., 0] * ref.inv_hw(hw)) ** 2
            assert bool((var < 0).any()) and bool((var > 1).any()) and float((a[..., 0] / hw).abs().max()) <= 4
            pd = p.to(dev)
            for mode in (0, 1):
                ga, gb = ops.in_finalize(pd, nslabs, hw, mode)
                _check_finalized(ga, gb, p.double(), hw, mode, ("in_finalize", nslabs, hw, mode))


def test_moments_slabs_counts_are_what_in_finalize_serves(dev):
    """ops.moments_slabs (the conv epilogues' slab count: one per 8 x 16 pixels) at the BatchNorm layers' sizes: b x that many
    slabs go through ops.in_finalize as one [1, b nsl, C, 2] tensor."""
    with _mode("fp32") as ops:
        assert [ops.moments_slabs(h, w) for h, w in ((1, 1), (8, 16), (9, 16), (8, 17), (128, 128))] == [1, 1, 2, 2, 128]
        b, hs, ws, c = 5, 20, 33, 8
        nsl = ops.moments_slabs(hs, ws)
        assert nsl == 9
        p = _int_partials(b, nsl, c, hs * ws, 77, clamp_every=0)
        ga, gb = ops.in_finalize(p.reshape(1, b * nsl, c, 2).to(dev), b * nsl, b * hs * ws)
        _check_finalized(ga, gb, p.reshape(1, b * nsl, c, 2).double(), b * hs * ws, 0, "batch-wide finalize")


# ------------------------------------------------------------------------------------------------------------------ 3 fused finalize
def _group_channels(kind):
    """Half a channel group (cpp < 8), exactly one group of 8 chunks, four groups."""
    return (4, 32, 128) if kind == "fp32" else (8, 64, 256)


def _fused_part_sources(ops, x, b, h, w, c, dev, seed):
    """[(label, partials on the device)]: ops.in_partial's for this x, and synthetic integer partials."""
    part, ns = ops.in_partial(x.t)
    out = [("in_partial ns %d" % ns, part)]
    for ns in (1, 7, 128):
        out.append(("synthetic ns %d" % ns, _int_partials(b, ns, c, h * w, seed + ns).to(dev)))
    return out


@pytest.mark.parametrize("name", list(STAT_SHAPES))
@pytest.mark.parametrize("kind", FWD_KINDS)
def test_fused_forward(kind, name, dev):
    """ops.in_apply_part: wg_finalize<0> + the elementwise pass.  The published mean / rstd of every channel group against the
    float64 formula (and ops.in_finalize), the output by the exact rules from the kernel's OWN published mean / rstd."""
    with _mode(kind) as ops:
        b, h, w = STAT_SHAPES[name]
        for n, c in enumerate(_group_channels(kind)):
            seed = 300 + n
            shape = (b, h, w, c)
            x = _sliced(kind, shape, dev, 8, 16).put(_ints(shape, -8, 8, seed))
            r = _sliced(kind, shape, dev, 16, 8).put(_ints(shape, -8, 8, seed + 1))
            x64, r64 = x.get(), r.get()
            sources = _fused_part_sources(ops, x, b, h, w, c, dev, seed)
            for label, part in sources:
                out = _sliced(kind, shape, dev, 24, 8).watch()
                for act in ACTS:
                    for res in (None, r):
                        what = ("in_apply_part", name, c, label, act, res is not None)
                        mean, rstd = ops.in_apply_part(x.t, part, act, None if res is None else res.t, out.t)
                        _check_finalized(mean, rstd, part.double().cpu(), h * w, 0, what)
                        fm, _ = ops.in_finalize(part, part.shape[1], h * w)
                        assert torch.equal(mean, fm), (what, "published mean differs from ops.in_finalize's")
                        m64, r64s = mean.double().cpu(), rstd.double().cpu()
                        if res is None:
                            _assert_stored(ops, kind, out, ref.forward_ops(x64, m64, r64s, act), what)
                        else:
                            _assert_one_of(kind, out, (ref.forward_ops(x64, m64, r64s, act, r64),
                                                       ref.forward_contracted(x64, m64, r64s, act, r64)), what)
        # 129 slabs: refused, by the wrapper and by the library, nothing written
        part = torch.zeros((b, 129, c, 2), device=dev)
        out = _sliced(kind, shape, dev, 24, 8).watch()
        with pytest.raises(AssertionError):
            ops.in_apply_part(x.t, part, ref.ACT_NONE, None, out.t)
        _refused(ops, out, lambda lib, st: lib.ctg_in_apply_part(
            ops.dtc(x.t), ops._p(x.t), ops._nhwc(x.t)[4], ops._p(part), 129, ops._p(st.mean), ops._p(st.rstd), 0, None, 0,
            ops._p(out.t), ops._nhwc(out.t)[4], b, h, w, c, ops._stream()), _Stats(b, c, 1, dev))


def _refused(ops, out, call, st=None):
    """`call(lib, st)` answers CTG_EINVAL through _lib.check and leaves `out` (both planes, the whole buffer) untouched."""
    from cta_gan_amd import _lib
    with pytest.raises(RuntimeError, match="CTG_EINVAL"):
        _lib.check(call(_lib.load(), st), "refusal")
    torch.cuda.synchronize()
    assert torch.equal(out.raw, out.snap), "a refused launch wrote to its output"


def _bwd_cases(pad):
    return [(2, pad + 1, pad + 1), (2, pad + 1, 9), (3, 9, 15), (2, 33, 17)] if pad else [(2, 5, 7), (3, 9, 15), (2, 33, 17)]


@pytest.mark.parametrize("pad", [0, 1, 3])
@pytest.mark.parametrize("kind", BWD_KINDS)
def test_fused_backward(kind, pad, dev, monkeypatch):
    """ops.in_bwd_stats with the fused finalize on: wg_finalize<1> + the elementwise pass from ops.in_bwd_partial's partials and
    from integer partials; per-element bound.  129 slabs take in_finalize + in_bwd_apply_kernel: bit for bit the op-for-op result."""
    with _mode(kind) as ops:
        monkeypatch.setattr(ops, "_FIN_FUSE", True)
        xk, gk = _xg(kind)
        for b, h, w in _bwd_cases(pad) + ([STAT_SHAPES["empty_last_slab"]] if pad == 1 else []):
            for n, c in enumerate(_group_channels(kind)):
                if h * w > 1000 and n != 1:
                    continue                               # the 128-slab real partials once, at exactly one channel group
                seed = 400 + 10 * pad + n
                shape, pshape = (b, h, w, c), (b, h + 2 * pad, w + 2 * pad, c)
                x = _sliced(xk, shape, dev, 8, 16).put(_ints(shape, -8, 8, seed))
                d = _sliced(gk, pshape, dev, 16, 8).put(_ints(pshape, -4, 4, seed + 1))
                st = _Stats(b, c, seed + 2, dev)
                x64, g64 = x.get(), ref.fold(d.get(), pad)
                dx = _sliced(gk, shape, dev, 24, 8).watch()
                last = (x, d, st, dx, shape)
                for act in ACTS:
                    sources = [("in_bwd_partial", ops.in_bwd_partial(x.t, d.t, pad, st.mean, st.rstd, act))]
                    # (the prologue knows no activation: the fusable synthetic counts once; 129 slabs -- the pinned kernel with
                    # s1 / s2 off the grid -- under every activation)
                    sources += [("synthetic ns %d" % ns, _int_partials(b, ns, c, h * w, seed + ns, 0).to(dev))
                                for ns in ((1, 7, 128, 129) if act == ref.ACT_LRELU else (129,))]
                    for label, part in sources:
                        what = ("in_bwd_stats", (b, h, w, c), pad, label, act)
                        ns = part.shape[1]
                        assert ops.fin_fusable(ns) == (ns <= 128)
                        ops.in_bwd_stats(x.t, d.t, st.mean, st.rstd, act, dx.t, part, pad=pad)
                        s1, s2 = (ref.f32(v) for v in ref.finalize(part.double().cpu(), h * w, 1))
                        if ns <= 128:
                            want, s = ref.backward(x64, g64, st.mean64, st.rstd64, s1, s2, act)
                            _close("in_bwd_stats fused", gk, dx.get(), want, s)
                            assert dx.outside_unchanged(), what
                        else:
                            f1, f2 = ops.in_finalize(part, ns, h * w, 1)
                            assert torch.equal(f1.double().cpu(), s1) and torch.equal(f2.double().cpu(), s2), what
                            _assert_stored(ops, gk, dx, ref.backward_ops(x64, g64, st.mean64, st.rstd64, s1, s2, act), what)
        x, d, st, dx, (b, h, w, c) = last
        part = torch.zeros((b, 129, c, 2), device=dev)
        dx.watch()
        _refused(ops, dx, lambda lib, _: lib.ctg_in_bwd_stats(
            ops.dtc_saved(x.t), ops._p(x.t), ops._nhwc(x.t)[4], ops._p(d.t), ops._nhwc(d.t)[4], pad, ops._p(st.mean),
            ops._p(st.rstd), 0, ops._p(dx.t), ops._nhwc(dx.t)[4], b, h, w, c, 129, ops._p(part), ops._stream()))


# ------------------------------------------------------------------------------------------------------------------ 4 elementwise
def pix_grid(kind, b, hw, c):
    """csrc/norm_act.hip: pix_grid (default knobs) -> (pixels per lane, pixel blocks, pixel lanes per workgroup)."""
    pl = 256 // (c // _epc(kind))
    per = 16
    while per > 2 and -(-hw // (pl * per)) * b < 2048:
        per >>= 1
    return per, max(1, min(4096, -(-hw // (pl * per)))), pl


def lane_trips(kind, b, hw, c):
    """The set of trip counts the lanes of a launch make: a lane starts at p0 < bx PL and strides by bx PL."""
    per, bx, pl = pix_grid(kind, b, hw, c)
    return sorted({-(-(hw - p0) // (bx * pl)) for p0 in range(min(bx * pl, hw))})


def _fwd_want(act, x64, st, r64):
    """Plain float64 for no activation / ReLU (exact on the grid), op for op for LeakyReLU."""
    if act == ref.ACT_LRELU:
        return ref.forward_ops(x64, st.mean64, st.rstd64, act, r64)
    return ref.forward(x64, st.mean64, st.rstd64, act, r64)


def _bwd_want(act, x64, g64, st, s1, s2):
    if act == ref.ACT_LRELU:
        return ref.backward_ops(x64, g64, st.mean64, st.rstd64, s1, s2, act)
    return ref.backward(x64, g64, st.mean64, st.rstd64, s1, s2, act)[0]


def _forward_case(ops, kind, shape, dev, seed, rdev="cpu", acts_res=None):
    b, h, w, c = shape
    x = _sliced(kind, shape, dev, 8, 16).put(_ints(shape, -8, 8, seed, rdev))
    r = _sliced(kind, shape, dev, 16, 8).put(_ints(shape, -8, 8, seed + 1, rdev))
    st = _Stats(b, c, seed + 2, dev, rdev)
    big = rdev != "cpu"
    x64, r64 = (x.t.double(), r.t.double()) if big else (x.get(), r.get())         # integers: the hi plane is the value
    out = _sliced(kind, shape, dev, 24, 8).watch()
    for act, with_res in acts_res or [(a, wr) for a in ACTS for wr in (False, True)]:
        what = ("in_apply", shape, act, with_res)
        ops.in_apply(x.t, st.mean, st.rstd, act, r.t if with_res else None, out.t)
        want = _fwd_want(act, x64, st, r64 if with_res else None)
        if big:
            assert torch.equal(ref.f32(want), want) and _stored_equal(ops, kind, out.t, want.float()), what
            assert out.outside_unchanged(), what
        else:
            _assert_stored(ops, kind, out, want, what)
        # in place (out == x): bit for bit the out-of-place result, the rest of x's buffer untouched
        xi = _sliced(kind, shape, dev, 8, 16)
        xi.raw.copy_(x.raw)
        xi.watch()
        ops.in_apply(xi.t, st.mean, st.rstd, act, r.t if with_res else None, xi.t)
        assert torch.equal(_bits(xi.t), _bits(out.t)) and (kind != "pair" or torch.equal(_bits(xi.lo()), _bits(out.lo()))), what
        assert xi.outside_unchanged(), what


def _backward_case(ops, kind, shape, pad, dev, seed, rdev="cpu", acts=ACTS, forms=("grid", "batch", "zero")):
    """ops.in_bwd_apply with s1 / s2 per (sample, channel) on the grid, batch-wide terms expanded over B (BatchNorm in
    training) and zeros (BatchNorm with running statistics)."""
    b, h, w, c = shape
    xk, gk = _xg(kind)
    pshape = (b, h + 2 * pad, w + 2 * pad, c)
    x = _sliced(xk, shape, dev, 8, 16).put(_ints(shape, -8, 8, seed, rdev))
    d = _sliced(gk, pshape, dev, 16, 8).put(_ints(pshape, -4, 4, seed + 1, rdev))
    st = _Stats(b, c, seed + 2, dev, rdev)
    big = rdev != "cpu"
    x64 = x.t.double() if big else x.get()
    g64 = d.t.double() if big else ref.fold(d.get(), pad)
    assert not (big and pad)
    dx = _sliced(gk, shape, dev, 24, 8).watch()
    for form in forms:
        if form == "grid":
            s1, s2 = st.s1, st.s2
        elif form == "batch":
            s1, s2 = st.s1[:1].expand(b, c).contiguous(), st.s2[:1].expand(b, c).contiguous()
        else:
            s1 = s2 = torch.zeros_like(st.s1)
        for act in acts:
            what = ("in_bwd_apply", kind, shape, pad, form, act)
            ops.in_bwd_apply(x.t, d.t, pad, st.mean, st.rstd, s1, s2, act, dx.t)
            want = _bwd_want(act, x64, g64, st, s1.double().to(rdev), s2.double().to(rdev))
            if big:
                assert torch.equal(ref.f32(want), want) and _stored_equal(ops, gk, dx.t, want.float()), what
                assert dx.outside_unchanged(), what
            else:
                _assert_stored(ops, gk, dx, want, what)
    return x, d, st, x64, g64, dx


@pytest.mark.parametrize("name", list(LANE_SHAPES))
@pytest.mark.parametrize("kind", FWD_KINDS)
def test_in_apply_lane_trips(kind, name, dev):
    with _mode(kind) as ops:
        b, h, w, c = LANE_SHAPES[name]
        c = _c(kind, c)
        want = {"lt_batch_1chunk": [1], "one_batch_32chunks": [1, 2], "one_or_half_batch": [1, 2], "one_batch_all": [2]}[name]
        assert lane_trips(kind, b, h * w, c) == want and pix_grid(kind, b, h * w, c)[0] == 2
        _forward_case(ops, kind, (b, h, w, c), dev, 500)


@pytest.mark.parametrize("name", list(LANE_SHAPES))
@pytest.mark.parametrize("kind", BWD_KINDS)
def test_in_bwd_apply_lane_trips(kind, name, dev):
    with _mode(kind) as ops:
        b, h, w, c = LANE_SHAPES[name]
        _backward_case(ops, kind, (b, h, w, _c(kind, c)), 0, dev, 600)


@pytest.mark.parametrize("pad", [1, 2, 3])
@pytest.mark.parametrize("kind", BWD_KINDS)
def test_in_bwd_padded(kind, pad, dev):
    """The gradient on the reflection-padded grid (fold_load, one pixel per trip): ops.in_bwd_apply on the grid, then ops.in_bwd
    end to end (statistics pass + in_finalize + in_bwd_apply_kernel): for no activation / ReLU the partials are exact, so s1 / s2
    are known to the bit; for LeakyReLU they are finalized from the kernel's own (deterministic) partial sums.  dx is bit for bit
    the op-for-op result under every activation."""
    with _mode(kind) as ops:
        gk = _xg(kind)[1]
        for n, (b, h, w) in enumerate(_bwd_cases(pad)):
            shape = (b, h, w, _c(kind, 64 if n % 2 else 8))
            x, d, st, x64, g64, dx = _backward_case(ops, kind, shape, pad, dev, 700 + 10 * pad + n, forms=("grid",))
            for act in ACTS:
                what = ("in_bwd", kind, shape, pad, act)
                ops.in_bwd(x.t, d.t, pad, st.mean, st.rstd, act, dx.t)
                if act == ref.ACT_LRELU:
                    # the partial sums round (test_statistics_mode1 bounds them), but the launches are deterministic: s1 / s2 are
                    # what ops.in_finalize makes of ops.in_bwd_partial's sums -- the two launches ops.in_bwd itself makes
                    pg = ops.in_bwd_partial(x.t, d.t, pad, st.mean, st.rstd, act)
                    f1, f2 = ops.in_finalize(pg, pg.shape[1], h * w, 1)
                    s1, s2 = (ref.f32(v) for v in ref.finalize(pg.double().cpu(), h * w, 1))
                    assert torch.equal(f1.double().cpu(), s1) and torch.equal(f2.double().cpu(), s2), what
                else:
                    part, _, _ = ref.partials(x64, ops._nslabs(b, h * w), 1, g64, st.mean64, st.rstd64, act)
                    s1, s2 = (ref.f32(v) for v in ref.finalize(part, h * w, 1))
                _assert_stored(ops, gk, dx, ref.backward_ops(x64, g64, st.mean64, st.rstd64, s1, s2, act), what)


def test_large_bf16_one_batch_of_four_or_three_single_trips(dev):
    """(4, 130, 127, 256) bf16: 4 pixels per lane, 516 pixel blocks of 8 lanes; a lane makes 4 trips (one batch of 4) or, from
    p0 = 4126, three single trips.  The float64 reference is evaluated with stock torch on the device."""
    with _mode("bf16") as ops:
        shape = (4, 130, 127, 256)
        assert pix_grid("bf16", 4, 130 * 127, 256) == (4, 516, 8) and lane_trips("bf16", 4, 130 * 127, 256) == [3, 4]
        _forward_case(ops, "bf16", shape, dev, 800, rdev=dev)
        _backward_case(ops, "bf16", shape, 0, dev, 810, rdev=dev, forms=("grid",))


def test_large_fp32_two_batches_or_one_batch_and_three_single_trips(dev):
    """(8, 130, 127, 128) fp32: 8 pixels per lane, 258 pixel blocks of 8 lanes; 8 trips (two batches of 4) or, from p0 = 2062, 7
    (one batch and three single trips)."""
    with _mode("fp32") as ops:
        shape = (8, 130, 127, 128)
        assert pix_grid("fp32", 8, 130 * 127, 128) == (8, 258, 8) and lane_trips("fp32", 8, 130 * 127, 128) == [7, 8]
        _forward_case(ops, "fp32", shape, dev, 820, rdev=dev)
        _backward_case(ops, "fp32", shape, 0, dev, 830, rdev=dev, forms=("grid",))


# ------------------------------------------------------------------------------------------------------------------ 5 conditioning
@pytest.mark.parametrize("kind", FWD_KINDS)
def test_ill_conditioned_statistics(kind, dev):
    """ops.in_stats on random data: channel c has |mean| / sigma = (0, 8, 64)[c % 4], channel 3 (mod 4) is the constant 1000.
    rel(rstd) <= n 2^-24 (1 + (mean / sigma)^2): the error of a sum of n fp32 adds is n 2^-24 of E[x^2] = sigma^2 + mean^2,
    and it lands on var = sigma^2 (rstd takes half of var's relative error: a factor 2 of slack)."""
    with _mode(kind) as ops:
        worst = {}
        for b, h, w, c in ((2, 33, 17, _c(kind, 8)), (3, 40, 40, _c(kind, 64))):
            gen = torch.Generator().manual_seed(h)
            ratio = torch.tensor([0.0, 8.0, 64.0, 0.0])[torch.arange(c) % 4]
            v = torch.randn((b, h, w, c), generator=gen) + ratio
            v[..., 3::4] = 1000.0
            x = _sliced(kind, (b, h, w, c), dev, 8, 8).put(v)
            x64 = x.get()
            mean, rstd = ops.in_stats(x.t)
            m64 = x64.mean((1, 2))
            var64 = x64.var((1, 2), unbiased=False)
            r64 = 1.0 / torch.sqrt(var64 + ref.EPS)
            ns = ops._nslabs(b, h * w)
            pl = 256 // (c // _epc(kind))
            n = -(-(-(-h * w // ns)) // pl) + pl                       # trips per lane + pixel lanes
            live = torch.arange(c) % 4 != 3
            true_ratio2 = (m64 * m64 / var64.clamp_min(1e-30))[:, live]
            bound = n * 2.0 ** -24 * (1.0 + true_ratio2)
            rel = ((rstd.double().cpu() - r64) / r64).abs()[:, live]
            for k, rt in enumerate((0.0, 8.0, 64.0)):
                worst[rt] = max(worst.get(rt, 0.0), float((rel / bound)[:, k::3].max()))
            print("in_stats %s %s n %d: worst fraction of the bound by ratio %s" % (kind, (b, h, w, c), n, worst))
            assert bool((rel <= bound).all()), (kind, (b, h, w, c), float((rel / bound).max()))
            assert bool(((mean.double().cpu() - m64).abs() <= n * 2.0 ** -24 * x64.abs().mean((1, 2)) + 2.0 ** -23 * m64.abs()).all())
            # the constant channel: finite, and never above 1 / sqrt(eps) (+ 1 ulp)
            top = torch.tensor(1.0 / ref.EPS ** 0.5, dtype=torch.float64)
            rc = rstd[:, 3::4].cpu()
            assert bool(torch.isfinite(rc).all()) and bool((rc > 0).all())
            assert bool((rc.double() <= float(top.float()) * (1 + 2.0 ** -23)).all())
            out = _sliced(kind, (b, h, w, c), dev, 8, 8).watch()
            ops.in_apply(x.t, mean, rstd, ref.ACT_NONE, None, out.t)
            assert bool(torch.isfinite(out.get()).all()) and out.outside_unchanged()
        for rt, f in worst.items():
            _note("in_stats rstd ratio %g" % rt, kind, f)


# ------------------------------------------------------------------------------------------------------------------ 6 refusals
@pytest.mark.parametrize("kind", FWD_KINDS)
def test_refusals(kind, dev):
    """A channel count that is no power-of-two number of chunks, 0 and 129 slabs for the statistics entries, pad >= H and
    pad >= W: CTG_EINVAL from _lib.check, the output buffer untouched.  Every buffer has the size the refused call names."""
    with _mode(kind) as ops:
        p, ld = ops._p, lambda buf: ops._nhwc(buf.t)[4]

        def raises(fn, *watched):
            with pytest.raises(RuntimeError, match="CTG_EINVAL"):
                fn()
            torch.cuda.synchronize()
            for buf in watched:
                assert torch.equal(buf.raw, buf.snap), "a refused launch wrote to its output"

        # 3 chunks per pixel
        b, h, w, c = 2, 4, 5, 24 if kind != "fp32" else 12
        x = _sliced(kind, (b, h, w, c), dev, 8, 8).put(_ints((b, h, w, c), -8, 8, 900))
        st = _Stats(b, c, 901, dev)
        out = _sliced(kind, (b, h, w, c), dev, 8, 8).watch()
        part = torch.zeros((b, 1, c, 2), device=dev)
        raises(lambda: ops.in_partial(x.t))
        raises(lambda: ops.in_stats(x.t))
        raises(lambda: ops.in_apply(x.t, st.mean, st.rstd, 0, None, out.t), out)
        raises(lambda: ops.in_apply_part(x.t, part, 0, None, out.t), out)
        raises(lambda: ops.in_bwd_partial(x.t, x.t, 0, st.mean, st.rstd, 0))
        raises(lambda: ops.in_bwd_apply(x.t, x.t, 0, st.mean, st.rstd, st.s1, st.s2, 0, out.t), out)
        raises(lambda: ops.in_bwd(x.t, x.t, 0, st.mean, st.rstd, 0, out.t), out)
        # 0 and 129 slabs for the statistics entries (the wrappers never ask for them: the C entries directly)
        c = _c(kind, 16)
        x = _sliced(kind, (b, h, w, c), dev, 8, 8).put(_ints((b, h, w, c), -8, 8, 902))
        st = _Stats(b, c, 903, dev)
        sums = _Buf("fp32", (b, 129, c, 2), dev).watch()
        mr = _Buf("fp32", (1, 1, 2 * b, c), dev).watch()
        dt = ops.dtc(x.t)
        for ns in (0, 129):
            _refused(ops, sums, lambda lib, _: lib.ctg_in_stats(dt, p(x.t), ld(x), b, h, w, c, ns, p(sums.raw), p(mr.raw),
                                                                p(mr.raw[0, 0, b:]), ops._stream()))
            assert torch.equal(mr.raw, mr.snap)
            _refused(ops, sums, lambda lib, _: lib.ctg_in_bwd_partial(dt, p(x.t), ld(x), p(x.t), ld(x), 0, p(st.mean), p(st.rstd), 0,
                                                                      b, h, w, c, ns, p(sums.raw), ops._stream()))
        # pad >= H, pad >= W, both
        for h, w, pad in ((3, 8, 3), (8, 3, 3), (2, 2, 2), (4, 5, 5)):
            shape, pshape = (b, h, w, c), (b, h + 2 * pad, w + 2 * pad, c)
            x = _sliced(kind, shape, dev, 8, 8).put(_ints(shape, -8, 8, 904))
            d = _sliced(kind, pshape, dev, 8, 8).put(_ints(pshape, -4, 4, 905))
            dx = _sliced(kind, shape, dev, 8, 8).watch()
            part = torch.zeros((b, 1, c, 2), device=dev)
            raises(lambda: ops.in_bwd_partial(x.t, d.t, pad, st.mean, st.rstd, 0))
            raises(lambda: ops.in_bwd_apply(x.t, d.t, pad, st.mean, st.rstd, st.s1, st.s2, 0, dx.t), dx)
            raises(lambda: ops.in_bwd_stats(x.t, d.t, st.mean, st.rstd, 0, dx.t, part, pad=pad), dx)
            raises(lambda: ops.in_bwd(x.t, d.t, pad, st.mean, st.rstd, 0, dx.t), dx)
            _refused(ops, dx, lambda lib, _: lib.ctg_in_bwd_stats(dt, p(x.t), ld(x), p(d.t), ld(d), pad, p(st.mean), p(st.rstd), 0,
                                                                  p(dx.t), ld(dx), b, h, w, c, 1, p(part), ops._stream()))
