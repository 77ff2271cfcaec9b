"""Tile paths of the halo-resident weight-gradient kernels (csrc/conv_wgrad.hip: conv_wgrad_halo_kernel, conv_wgrad_s2m_kernel).

Both kernels load a tile by one of two paths, chosen per tile by a workgroup-uniform test: a tile whose X halo and G tile lie wholly
inside the images takes sources of the form (scalar tile base + lane offset); a border or ragged tile reflects / zero-pads slot by
slot.  A workgroup walks a run of tiles with the tile origin carried from tile to tile, and with the prefetch double buffer live the
loads of tile t + 1 are issued while tile t is multiplied.  The cases of tests/test_conv_exact_gpu.py (8 x 16 and 17 x 33 images:
nine tiles, one of them interior) never run interior -> border -> interior inside one workgroup's run; the shapes here are the
smallest that do, for every window, channel tiling, stride and operand form the launcher dispatches.

Integer-grid operands (tests/conv_ref.py): every product and partial sum is exact in fp32 in any order, so the per-slab partials and
the reduced gradient must equal the float64 reference bit for bit.  The calls go through the C ABI directly (ctg_conv_wgrad with a
chosen slab size, ctg_wgrad_reduce), because the slab count -- how many tiles one workgroup walks -- is what the cases vary.
"""
import numpy as np
import pytest
import torch

from conv_ref import (PAD_REFLECT, PAD_ZERO, PAIR_GRANULE, assert_exact_domain, first_diff, int_grid, linear_slabs, pack_tap,
                      pair_grid, tile_slabs, wgrad_pair_ref, wgrad_taps_ref)

pytestmark = pytest.mark.gpu

SENT = -24576.0
BF16, PAIR = "bf16", "pair"


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


def fwd_taps(kh, kw, py, px):
    """Row-major kh x kw window with its origin at (-py, -px)."""
    return [pack_tap(ky - py, kx - px, ky * kw + kx) for ky in range(kh) for kx in range(kw)]


T3 = fwd_taps(3, 3, 1, 1)


def _ceil(a, b):
    return (a + b - 1) // b


def _slice_of(t, ld, off, fill=9.0):
    """`t` [B, H, W, C] as the channel slice at `off` of a buffer of `ld` channels filled with `fill`."""
    b, h, w, c = t.shape
    if ld == c:
        return t.contiguous()
    full = torch.full((b, h, w, ld), fill, dtype=t.dtype, device=t.device)
    full[..., off:off + c] = t
    return full[..., off:off + c]


# operands and references, computed once per (shape, seed) and shared by the cases that differ only in the slab count
_REF = {}


def _reference(seed, kind, mc, nc, taps, B, Hs, Ws, Hi, Wi, is_, pad_mode):
    key = (seed, kind, mc, nc, tuple(taps), B, Hs, Ws, Hi, Wi, is_, pad_mode)
    if key not in _REF:
        rng = np.random.default_rng(seed)
        if kind == PAIR:
            g, x = pair_grid(rng, (B, Hs, Ws, mc)), pair_grid(rng, (B, Hi, Wi, nc))
            dw, s = wgrad_pair_ref(g, x, taps, is_, pad_mode)
            assert_exact_domain(s, PAIR_GRANULE)
        else:
            g, x = int_grid(rng, (B, Hs, Ws, mc), -3, 3), int_grid(rng, (B, Hi, Wi, nc), -3, 3)
            dw = wgrad_taps_ref(g, x, taps, is_, pad_mode)
            assert_exact_domain(wgrad_taps_ref(g.abs(), x.abs(), taps, is_, pad_mode))
        _REF[key] = (g, x, dw)
    return _REF[key]


def _slab_partials(g, x, taps, is_, pad_mode, slabs):
    """Per-slab partials [B * count, T, M, C] in the kernels' order (sample-major): wgrad_taps_ref of one sample with G zeroed
    outside the slab (the same sums as its own `slabs=` form, without the one-hot contraction over every pixel)."""
    ids, cnt = slabs
    out = []
    for b in range(g.shape[0]):
        for s_ in range(cnt):
            mask = (ids == s_).to(g.dtype)[None, :, :, None]
            out.append(wgrad_taps_ref(g[b:b + 1] * mask, x[b:b + 1], taps, is_, pad_mode))
    return torch.stack(out)


def _run(dev, *, seed, mc, nc, taps, B, Hs, Ws, Hi=None, Wi=None, is_=1, pad_mode=PAD_ZERO, sps=1, kind=BF16, g_ld=None, g_off=0,
         x_ld=None, x_off=0, status=0, zfac=1, slabs="tile"):
    """One ctg_conv_wgrad call with `sps` slabs per sample: the status it answers, the per-slab partials (slabs: 'tile' = the
    halo-resident kernels' runs of 8 x 16 tiles, 'linear' = the per-tap kernel's runs of pixels, None = not compared) and the
    gradient ctg_wgrad_reduce makes of them, all bit for bit."""
    from cta_gan_amd import _lib, ops
    lib = _lib.load()
    Hi, Wi = Hi or Hs, Wi or Ws
    pair = kind == PAIR
    nt = len(taps)
    g, x, dw = _reference(seed, kind, mc, nc, taps, B, Hs, Ws, Hi, Wi, is_, pad_mode)
    if pair:
        gd, xd = ops.to_pair(g.float().to(dev)), ops.to_pair(x.float().to(dev))
    else:
        gd = _slice_of(g.to(dev).to(torch.bfloat16), g_ld or mc, g_off)
        xd = _slice_of(x.to(dev).to(torch.bfloat16), x_ld or nc, x_off)
    hw = Hs * Ws
    slab = _ceil(hw, sps)
    assert _ceil(hw, slab) == sps
    z1 = B * sps
    what = "wgrad %dx%d %dtaps is%d %s pad%d @%dx%d <- %dx%d, %d slabs" % (mc, nc, nt, is_, kind, pad_mode, Hs, Ws, Hi, Wi, sps)
    part = torch.full((3 * z1, nt, mc, nc), SENT, dtype=torch.float32, device=dev)
    rc = lib.ctg_conv_wgrad(2 if pair else ops.dt(torch.bfloat16), gd.data_ptr(), xd.data_ptr(), part.data_ptr(), B, Hs, Ws, mc,
                            ops._nhwc(gd)[4], Hi, Wi, nc, ops._nhwc(xd)[4], is_, pad_mode, slab, nt, ops._tap_array(taps),
                            ops._stream())
    assert rc == status, (what, "status", rc)
    z = zfac * z1
    torch.cuda.synchronize()
    got = part.cpu()
    assert bool((got[z:] == SENT).all()), what + ": wrote behind its partials"
    if slabs is not None:
        ids = tile_slabs(Hs, Ws, slab) if slabs == "tile" else linear_slabs(Hs, Ws, slab)
        assert ids[1] == sps
        pref = _slab_partials(g, x, taps, is_, pad_mode, ids)
        for zz in range(z):
            assert torch.equal(got[zz].double(), pref[zz]), \
                (what, "slab %d (sample %d, slab %d of %d); index = (tap, m, c)" % (zz, zz // sps, zz % sps, sps),
                 first_diff(got[zz].double(), pref[zz]))
    n = mc * nc * nt
    dst = torch.full((n + 64,), SENT, dtype=torch.float32, device=dev)
    assert lib.ctg_wgrad_reduce(part.data_ptr(), z, nt, mc, nc, dst.data_ptr(), mc, nc, nc * nt, nt, 1, 0, ops._stream()) == 0
    torch.cuda.synchronize()
    d = dst.cpu()
    want = dw.permute(1, 2, 0).contiguous().float()          # [m][c][t]
    have = d[:n].view(mc, nc, nt)
    assert torch.equal(have.view(torch.int32), want.view(torch.int32)), (what, "reduced; index = (m, c, tap)", first_diff(have, want))
    assert bool((d[n:] == SENT).all()), what + ": wrote behind the destination"


PADS = ((PAD_ZERO, "zero"), (PAD_REFLECT, "reflect"))

# ---------------------------------------------------------------------------- 3 x 3, 64 x 64 channels
# 40 x 80: 5 x 5 tiles, 9 interior.  One slab per sample walks all 25 tiles (border, interior and border again in every tile row);
# two slabs cut the run after tile 12, in the middle of a tile row.  41 x 83: 6 x 6 tiles, the last tile row (1 pixel row) and
# column (3 pixel columns) ragged, so the G tile's pixel mask sits beside interior tiles.
WALK = {}
for _p, _pn in PADS:
    for _h, _w in ((40, 80), (41, 83)):
        for _s in (1, 2):
            WALK["%s_%dx%d_sps%d" % (_pn, _h, _w, _s)] = dict(mc=64, nc=64, taps=T3, B=2, Hs=_h, Ws=_w, pad_mode=_p, sps=_s,
                                                              seed=1000 + 10 * _p + (_h == 41))


@pytest.mark.parametrize("name", list(WALK))
def test_tile_walk_3x3_64x64(name, dev):
    _run(dev, **WALK[name])


# ---------------------------------------------------------------------------- channel tilings, strided operands, other windows
# 24 x 48: 3 x 3 tiles, the middle one interior; two slabs (runs of 5 and 4 tiles) put it inside the first run
SHAPES = {}
for _m, _n in ((64, 32), (32, 64), (32, 32)):
    for _p, _pn in PADS:
        SHAPES["%dx%d_%s_24x48" % (_m, _n, _pn)] = dict(mc=_m, nc=_n, taps=T3, B=2, Hs=24, Ws=48, pad_mode=_p, sps=2, seed=1100 + _m + _n // 32 + _p)
# channel slices of wider buffers (the registration U-Net's concat buffers): the leading dimension, not the channel count, is the pixel pitch
for _p, _pn in PADS:
    SHAPES["strided_g128_x96_64x32_%s_24x48" % _pn] = dict(mc=64, nc=32, taps=T3, B=2, Hs=24, Ws=48, pad_mode=_p, sps=2, g_ld=128, g_off=64,
                                                          x_ld=96, x_off=32, seed=1200 + _p)
SHAPES["1tap_64x64_24x48"] = dict(mc=64, nc=64, taps=fwd_taps(1, 1, 0, 0), B=2, Hs=24, Ws=48, sps=2, seed=1300)
SHAPES["1tap_strided_32x32_24x48"] = dict(mc=32, nc=32, taps=fwd_taps(1, 1, 0, 0), B=2, Hs=24, Ws=48, sps=2, g_ld=128, g_off=64, x_ld=96,
                                          x_off=32, seed=1301)
SHAPES["4x4_zero_64x64_24x48"] = dict(mc=64, nc=64, taps=fwd_taps(4, 4, 1, 1), B=2, Hs=24, Ws=48, Hi=25, Wi=49, sps=2, seed=1302)
SHAPES["4x4_zero_32x64_24x48"] = dict(mc=32, nc=64, taps=fwd_taps(4, 4, 1, 1), B=2, Hs=24, Ws=48, Hi=25, Wi=49, sps=2, seed=1303)
SHAPES["7x7_reflect_row_groups_32x64_24x48"] = dict(mc=32, nc=64, taps=fwd_taps(7, 7, 3, 3), B=2, Hs=24, Ws=48, pad_mode=PAD_REFLECT, sps=2,
                                                    seed=1304)
SHAPES["7x7_reflect_row_groups_32x32_24x48"] = dict(mc=32, nc=32, taps=fwd_taps(7, 7, 3, 3), B=2, Hs=24, Ws=48, pad_mode=PAD_REFLECT, sps=2,
                                                    seed=1305)
SHAPES["7x7_reflect_all_taps_16x64_24x48"] = dict(mc=16, nc=64, taps=fwd_taps(7, 7, 3, 3), B=2, Hs=24, Ws=48, pad_mode=PAD_REFLECT, sps=2,
                                                  seed=1306)


@pytest.mark.parametrize("name", list(SHAPES))
def test_channel_tiles_strides_windows(name, dev):
    _run(dev, **SHAPES[name])


# ---------------------------------------------------------------------------- stride 2
# G on the 24 x 48 grid (3 x 3 tiles), X at twice the size: even (48 x 96) and odd (47 x 95, the last window row / column padded)
S2 = {}
for _hi, _wi in ((48, 96), (47, 95)):
    S2["s2m_128x64_%dx%d" % (_hi, _wi)] = dict(mc=128, nc=64, taps=T3, B=2, Hs=24, Ws=48, Hi=_hi, Wi=_wi, is_=2, sps=2, seed=1400 + _hi)
    S2["s2m_128x64_%dx%d_one_slab" % (_hi, _wi)] = dict(mc=128, nc=64, taps=T3, B=2, Hs=24, Ws=48, Hi=_hi, Wi=_wi, is_=2, sps=1, seed=1400 + _hi)
    S2["four_launches_32x64_%dx%d" % (_hi, _wi)] = dict(mc=32, nc=64, taps=T3, B=2, Hs=24, Ws=48, Hi=_hi, Wi=_wi, is_=2, sps=2, seed=1410 + _hi)
# transposed conv 64 -> 128 from 24 x 48: the roles swap, G = the layer's input on the small grid, X = dY on the large one
S2["convT_roles_swapped_64x128_24x48"] = dict(mc=64, nc=128, taps=T3, B=2, Hs=24, Ws=48, Hi=48, Wi=96, is_=2, sps=2, seed=1420)
S2["4x4_s2_four_launches_64x64_24x48"] = dict(mc=64, nc=64, taps=fwd_taps(4, 4, 1, 1), B=2, Hs=24, Ws=48, Hi=48, Wi=96, is_=2, sps=2, seed=1421)


@pytest.mark.parametrize("name", list(S2))
def test_stride2(name, dev):
    _run(dev, **S2[name])


# ---------------------------------------------------------------------------- split pair
def test_split_pair_three_sweeps_in_one_workgroup(dev, pair_mode):
    """256 x 256 channels at 40 x 48 (5 x 3 tiles, the middle column's tiles 4, 7, 10 interior), 12 slabs per sample at B = 2:
    16 x 2 x 12 = 384 workgroups, the smallest grid that keeps the three sweeps in one workgroup (status 0).  A workgroup walks
    two tiles -- (4, 5), (6, 7), (10, 11): an interior and a border one -- with the four plane buffers of the reuse schedule;
    slabs 8 .. 11 of a sample are empty.  g_hi x_hi + g_hi x_lo + g_lo x_hi of wgrad_pair_ref."""
    _run(dev, seed=1500, mc=256, nc=256, taps=T3, B=2, Hs=40, Ws=48, pad_mode=PAD_REFLECT, sps=12, kind=PAIR, status=0, zfac=1, slabs=None)


def test_split_pair_phase_split(dev, pair_mode):
    """64 x 64 channels at 24 x 48, B = 2: 4 workgroups < 384, so every sweep is a workgroup of its own with its own partial
    (status 3, three partials per slab); each of them walks border, interior and border tiles."""
    _run(dev, seed=1501, mc=64, nc=64, taps=T3, B=2, Hs=24, Ws=48, pad_mode=PAD_REFLECT, sps=2, kind=PAIR, status=3, zfac=3, slabs=None)


def test_split_pair_s2m(dev, pair_mode):
    """The merged stride-2 kernel's twelve-step split-pair schedule on the same 384-workgroup grid: runs of two tiles of the
    40 x 48 grid, X at 79 x 95."""
    _run(dev, seed=1502, mc=256, nc=256, taps=T3, B=2, Hs=40, Ws=48, Hi=79, Wi=95, is_=2, sps=12, kind=PAIR, status=0, zfac=1, slabs=None)


# ---------------------------------------------------------------------------- launcher
@pytest.mark.parametrize("pad_mode", [PAD_ZERO, PAD_REFLECT], ids=["zero", "reflect"])
def test_window_without_a_halo_geometry_falls_through(pad_mode, dev):
    """A row-major 2 x 3 window: the launcher would hand the 3-wide kernels khb = 2 rows per workgroup, and their halo height is
    compile-time (3 rows: 9 taps).  No instantiation serves it, so the call falls through to the per-tap kernel -- whose partials
    are runs of PIXELS, not of tiles, which is what shows that it ran -- and the gradient is right."""
    _run(dev, seed=1600 + pad_mode, mc=64, nc=64, taps=fwd_taps(2, 3, 1, 1), B=2, Hs=24, Ws=48, pad_mode=pad_mode, sps=2, slabs="linear")
