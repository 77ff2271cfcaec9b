"""GPU: the compile-time tap walk of the halo kernel's 3x3 instantiations (csrc/conv_halo.h: walk3x3), bit for bit.

What is under test.  A launch whose taps are a FULL 3x3 window with tap t on weight slice t, in row-major or in flipped order
(csrc/conv_dispatch.h: taps_3x3_walk), runs the nine tap steps of a channel slice unrolled: window position, tile-row offset and
weight buffer of a step are constants of the step, the next weight tile is a running pointer, the weight buffers change roles at
every slice boundary (nine taps: the parity flips) and the halo refill is straight-line.  Any other tap list of a 3-wide window
(fewer rows, another order, other weight slices) keeps the generic loop of the same instantiation.

Exactness argument: that of tests/test_conv_exact_gpu.py (integer-grid operands, sums below 2^24 granules asserted before
anything is launched, torch.equal on the stored bits against the float64 reference of tests/conv_ref.py).  On top of it every
case asserts that EVERY tap carries non-zero weights from every channel slice into every 16-channel output tile, and the weights
are drawn independently per tap: a step that reads another tap's window position, another slice's halo or the other weight
buffer is a non-zero integer difference.

Shapes: the smallest at which the path can go wrong.  128 -> 128 channels = two channel slices (one refill, one change of buffer
roles), 256 -> 256 = four slices and two channel tiles; 32 x 32 = the smallest `conv_fusable` map cut into tiles, 33 x 47 = ragged
in both directions (waves without valid rows skip their MFMAs but keep loading); B = 2.

  case                               instantiation (evidence: slab count of the moments)            order
  forward bf16, 128 / 256 channels   BN 128, TH 8 (B tiles ntn < 384: halo_th8), KWC 3               row-major
  forward bf16 128 -> 256, 3x128x128 BN 128, TH 16 (384 workgroups): the training step's kernel      row-major, two slices
  flipped bf16 (plain backward-data) BN 128, TH 8                                                    flipped
  fused backward-data 32 x 32        FUSE, BN 128, TH 8: output, partial sums, slab count            flipped
  split pair 128 -> 128              PK, BN 128, TH 16, K steps of 32 channels = four slices: the    row-major and flipped
                                     split-pair instantiations keep the generic loop (register
                                     budget, LAB_NOTES section 26) and must not have changed
  2 x 3 window, 1 x 3 window,        KWC 3, generic loop (kh < 3)                                    -
  3x3 column-major, 3x3 with the
  weight slices reversed             KWC 3, generic loop (refused by taps_3x3_walk)                  -
  three-tap frame launch             gather kernel (frame != 0): ring-only write                     flipped, on the padded grid
"""
import zlib

import numpy as np
import pytest
import torch

from conv_ref import (ACT_LRELU, ACT_NONE, ACT_RELU, PAD_REFLECT, PAD_ZERO, PAIR_GRANULE, assert_exact_domain, bias_grid,
                      conv_pair_ref, conv_pair_s, conv_taps_ref, epilogue, int_grid, moments_ref, pack_tap, pair_grid, pair_split,
                      store_bf16, store_pair)
from test_conv_epilogue_exact_gpu import _fuse_case, fuse_reference
from test_conv_exact_gpu import SENT, _assert_bits, _check_moments, _fwd, flip_taps, fwd_taps

pytestmark = pytest.mark.gpu

B = 2
PADS = {"reflect": PAD_REFLECT, "zero": PAD_ZERO}
GRIDS = {"32x32": (32, 32), "33x47": (33, 47)}
ORDERS = {
    "fwd": fwd_taps(3, 1),
    "flip": flip_taps(3, 1),
    # refused by taps_3x3_walk: the same window walked column by column / tap t on weight slice 8 - t
    "colmajor": [pack_tap(ky - 1, kx - 1, ky * 3 + kx) for kx in range(3) for ky in range(3)],
    "wrev": [pack_tap(ky - 1, kx - 1, 8 - (ky * 3 + kx)) for ky in range(3) for kx in range(3)],
}


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


def _ceil(a, b):
    return (a + b - 1) // b


def assert_weights_everywhere(w, kslice):
    """w [taps, Cout, Cin]: every tap carries a non-zero weight from every K slice of `kslice` channels into every 16-channel
    output tile (split pair: in its hi plane, which all three products of a step but one use)."""
    t, co, ci = w.shape
    assert co % 16 == 0 and ci % kslice == 0
    nz = (w.reshape(t, co // 16, 16, ci // kslice, kslice) != 0).any(4).any(2)
    assert bool(nz.all()), "a (tap, output tile, slice) block of the weights is all zero: %s" % (nz == 0).nonzero()[:4].tolist()


_REF = {}


def _reference(cin, cout, b, h, w, pad, order, pair, lo):
    """Operands and exact accumulators of a case, computed once and left unchanged."""
    key = (cin, cout, b, h, w, pad, order, pair, lo)
    if key in _REF:
        return _REF[key]
    rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
    taps = ORDERS[order]
    if pair:
        x, wt = pair_grid(rng, (b, h, w, cin)), pair_grid(rng, (9, cout, cin))
        assert_weights_everywhere(pair_split(wt)[0], 32)
        acc = conv_pair_ref(x, wt, taps, h, w, 1, pad)
        assert_exact_domain(conv_pair_s(x, wt, taps, h, w, 1, pad), PAIR_GRANULE)
    else:
        x, wt = int_grid(rng, (b, h, w, cin), -lo, lo), int_grid(rng, (9, cout, cin), -lo, lo)
        assert_weights_everywhere(wt, 64)
        acc = conv_taps_ref(x, wt, taps, h, w, 1, pad)
        assert_exact_domain(torch.tensor(float(lo * lo * cin * 9)))      # >= the sum of the terms' magnitudes
        assert_exact_domain(moments_ref(acc)[..., 1])
    _REF[key] = (x, wt, acc)
    return _REF[key]


def _walk_case(dev, *, cin, cout, grid, pad, order, moments, pair=False, lo=2, b=B, th=8):
    from cta_gan_amd import ops
    h, w = grid
    pad_mode = PADS[pad]
    x, wt, acc = _reference(cin, cout, b, h, w, pad_mode, order, pair, lo)
    taps = ORDERS[order]
    npad = _ceil(cout, 128) * 128
    wp = torch.full((9, npad, cin), 5.0, dtype=torch.float64)
    wp[:, :cout] = wt
    what = "walk %d->%d %s %s %s @%dx%d%s" % (cin, cout, "pair" if pair else "bf16", order, pad, h, w, " +moments" if moments else "")
    if pair:
        xd, wd = ops.to_pair(x.float().to(dev)), wp.float().to(dev).contiguous()
        y = ops.empty_act((b, h, w, cout), torch.bfloat16, dev)
        y.fill_(SENT)
        ops.pair_lo(y).fill_(SENT)
    else:
        xd, wd = x.to(dev).bfloat16().contiguous(), wp.to(dev).bfloat16().contiguous()
        y = torch.full((b, h, w, cout), SENT, dtype=torch.bfloat16, device=dev)
    if moments:
        bs, act = None, ACT_NONE
    else:      # a launch that emits no moments: bias and activation in the epilogue
        bs, act = bias_grid(np.random.default_rng(cin + cout + h), cout), ACT_LRELU
    part, ns = ops.conv_igemm(xd, wd, npad, y, bs.float().to(dev) if bs is not None else None, cout, h, w, 0, 0, 1, 1, pad_mode, act,
                              taps, want_stats=moments)
    torch.cuda.synchronize()
    v = epilogue(acc, bs, act)
    if pair:
        hi_, lo_ = store_pair(v)
        _assert_bits(y, hi_, what + " hi plane")
        _assert_bits(ops.pair_lo(y), lo_, what + " lo plane")
    else:
        _assert_bits(y, store_bf16(v), what)
    if moments:
        want_ns = _ceil(h, th) * _ceil(w, 16)
        assert ns == want_ns, (what, "slab count %d: not the intended instantiation (%d)" % (ns, want_ns))
        if not pair:      # (split pair: the squares are multiples of 2^-20, their sums are not exact in fp32)
            _check_moments(ops, part, ns, acc, h * w, what)
    else:
        assert ns == 0, what


@pytest.mark.parametrize("moments", [True, False], ids=["moments", "plain"])
@pytest.mark.parametrize("pad", list(PADS))
@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("ch", [128, 256])
def test_forward_walk(ch, grid, pad, moments, dev):
    _walk_case(dev, cin=ch, cout=ch, grid=GRIDS[grid], pad=pad, order="fwd", moments=moments, lo=2 if ch == 128 else 1)


def test_forward_walk_16_row_tiles(dev):
    """128 -> 256 channels, 3 x 128 x 128: 384 workgroups, the BN 128 / TH 16 instantiation of the training step, two slices."""
    _walk_case(dev, cin=128, cout=256, grid=(128, 128), pad="reflect", order="fwd", moments=True, lo=1, b=3, th=16)


@pytest.mark.parametrize("case", [(128, "33x47", "zero"), (256, "32x32", "reflect")], ids=["128_33x47_zero", "256_32x32_reflect"])
def test_flipped_walk(case, dev):
    """The backward-data order without a fused epilogue: tap t at window position (2 - t / 3, 2 - t % 3)."""
    ch, grid, pad = case
    _walk_case(dev, cin=ch, cout=ch, grid=GRIDS[grid], pad=pad, order="flip", moments=True, lo=2 if ch == 128 else 1)


@pytest.mark.parametrize("act", [ACT_NONE, ACT_RELU], ids=["none", "relu"])
@pytest.mark.parametrize("ch", [128, 256])
def test_fused_backward_data_walk(ch, act, dev):
    """The fused backward-data launch of a residual block at 32 x 32 with `res`, `fold` and `in_bwd`: stored gradient, the
    per-tile InstanceNorm-backward sums and the slab count (8-row tiles), all exact."""
    lo = 2 if ch == 128 else 1
    ref = fuse_reference(ch, ch, B, 32, 32, 8, False, 7100 + ch, -lo, lo, epis=("res_fold",))
    assert_weights_everywhere(ref["w"], 64)
    _fuse_case(dev, ref, ch, ch, B, 32, 32, False, "res_fold", act, "fused bwd-data walk %d 32x32 act %d" % (ch, act))


@pytest.mark.parametrize("case", [("32x32", "reflect", "fwd"), ("33x47", "zero", "fwd"), ("33x47", "zero", "flip")],
                         ids=["32x32_reflect", "33x47_zero", "33x47_zero_flipped"])
def test_split_pair_walk(case, dev, pair_mode):
    """Split-pair operands, 128 -> 128: K steps of 32 channels (four slices, three refills), three MFMAs per pair of fragments.
    These instantiations are excluded from the walk: the same launches on the generic loop of the 3-wide kernel."""
    grid, pad, order = case
    _walk_case(dev, cin=128, cout=128, grid=GRIDS[grid], pad=pad, order=order, moments=True, pair=True, th=16)


# ---------------------------------------------------------------------------- what the walk refuses: the generic loop still serves it
@pytest.mark.parametrize("order", ["colmajor", "wrev"])
def test_refused_3x3_orders_take_the_generic_loop(order, dev):
    """A full 3x3 window in an order, or on weight slices, the walk does not hard-code: wrong results if it ran all the same."""
    _walk_case(dev, cin=128, cout=128, grid=GRIDS["33x47"], pad="reflect", order=order, moments=True)


WIN_2x3 = [pack_tap(ky - 1, kx - 1, ky * 3 + kx) for ky in range(2) for kx in range(3)]
WIN_1x3 = [pack_tap(0, kx - 1, kx) for kx in range(3)]


@pytest.mark.parametrize("taps", [WIN_2x3, WIN_1x3], ids=["2x3", "1x3"])
def test_narrower_windows_take_the_generic_loop(taps, dev):
    """kh < 3 on the 3-wide instantiation (KWC 3): six and three taps per slice, two slices."""
    _fwd(dev, seed=7200 + len(taps), cin=128, cout=128, taps=taps, B=B, Hi=33, Wi=47, Hs=33, Ws=47, pad_mode=PAD_REFLECT,
         nslabs=_ceil(33, 8) * _ceil(47, 16), lo=-2, hi=2)


def test_three_tap_frame_launch(dev):
    """The frame launch of the residual blocks' backward-data (flipped 3x3 on the padded grid, three live taps per edge): only the
    1-pixel ring is written, by the gather kernel."""
    _fwd(dev, seed=7300, cin=128, cout=128, taps=flip_taps(3, 0), B=B, Hi=32, Wi=32, Hs=34, Ws=34, frame=True, lo=-2, hi=2)
