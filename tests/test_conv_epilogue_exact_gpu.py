"""GPU: the epilogues of the conv kernels (csrc/conv_halo.h, csrc/conv_igemm.hip), bit for bit, on integer-grid operands.

What is new against tests/test_conv_exact_gpu.py: every activation through every store form of both kernels (the activation is
decided once per staging loop: act_switch, one straight-line copy of the loop per activation and one run-time copy for tanh /
sigmoid), and the FUSE launch with the InstanceNorm-backward sums (GradMask: the branch-free mask; the frame-column chunk is
requested one trip ahead; every global address of the store loop is a base plus a per-trip step).  Exactness argument, helpers
and the sentinel convention are those of tests/conv_ref.py and tests/test_conv_exact_gpu.py: `assert_exact_domain` runs on the
reference BEFORE anything is launched, comparisons are torch.equal on the stored bits.

Activation x store form.  3x3, reflection padding, with bias; one output channel has zero weights and a zero bias, so that every
case holds pre-activations that are exactly zero beside negative and positive ones (asserted on the reference).  None / ReLU /
LeakyReLU: bit for bit (LeakyReLU is one fp32 multiply by 0.2f in the kernels and in numpy).  tanh / sigmoid: against the float64
function of the exact pre-activation; the kernels' fp32 evaluation is allowed the 2e-4 of tests/test_conv_exact_gpu.py, and the
STORE adds what the format cannot hold: nothing for fp32, the unit roundoff of an 8-bit significand (half a unit in the last
place <= 2^-8 |value|) for a bf16 result and 2^-16 |value| for a split pair (hi = bf16(v), lo = bf16(v - hi): |v - hi| <= 2^-8 |v|,
rounded to 8 bits once more).  Those cases use sparse weights (pre-activations of a few units), and at least 100 results must be
unsaturated.

  case                     dispatch condition (csrc)                                      instantiation               evidence
  halo 64->64 33x17        stride 1, full window, Hs, Ws >= 16, Cout > 32: launch_halo_t   BN 64, TH 8, KWC 3          nslabs 10 = ceil(33/8) x 2
  halo 128->256 33x17      Cout > 64, 24 workgroups < 384: halo_th8                        BN 128, TH 8, KWC 3         nslabs 10
    ... pair / fp32 out    out_f32 >= 2 (split-pair input), Cout > 64                      BN 128, TH 16, PK           nslabs 6 = ceil(33/16) x 2
    ... pair 64->64        Cout > 32, Hs >= 16                                             BN 64, TH 8, PK             nslabs 10
  gather 32->32 13x15      Hs, Ws < 16: no halo kernel                                     conv_igemm_kernel BM 128    nslabs 2 = ceil(195/128)
  store forms              y bf16 / y a split pair / y fp32 from split-pair input          staged bf16 / staged fp32 rounds / direct fp32
The slab count comes from a twin launch without bias and activation (bf16 and pair results; an fp32 result from split-pair input
emits no moments: there the instantiation follows from the dispatch conditions alone).

FUSE with InstanceNorm-backward sums.  A flipped 3x3 conv with zero padding through ops.conv_igemm(..., res=, fold=,
in_bwd=(z, mean, rstd, act)): `epi->res / fold` route the launch to the FUSE instantiation of the halo kernel (CTG_EINVAL on any
other kernel).  z is on the integer grid, mean an integer and rstd a power of two per (sample, channel): xhat is exact.  The
stored gradient must equal fused_store_bf16 bit for bit; the per-tile partials (sum g m, sum g m xhat) are taken from the stored,
rounded gradient: for no activation / ReLU every term is a multiple of the granule and the sums are exact (domain asserted), so
they must match bit for bit; for LeakyReLU m g = 0.2f g rounds, and the sums stay within n 2^-24 sum |term| (n = the tile's pixel
count: the bound tests/test_instnorm_exact_gpu.py uses for its MODE 1 sums).  The fold's interior holds non-zero values that must
not be read, and all four frame corners are non-zero (asserted).

  grid 48x48               9 tiles of 16 columns: corner, edge and interior tiles          64: BN 64 TH 8; 256: BN 128 TH 8 (36 wgs)   nslabs 18
  grid 33x17               row Hs - 2 = 31 in the ragged last tile row, column Ws - 2 = 15 and column 1 in the same tile;
                           the second tile column holds one pixel column                                                           nslabs 10
  256 ch, 3 x 128x128      384 workgroups: not below th8_wgs                               BN 128, TH 16, KWC 3 (the step's kernel)     nslabs 64
  split pair 64 ch 48x48   dtype 2 (split-pair planes), Cout > 32                          BN 64, TH 8, PK, FUSE                        nslabs 18
The slab count the launch returns is the tile count of the instantiation named.  In the split-pair case the terms are multiples
of 2^-10 (x its rstd): sparse weights keep the sums inside the exact domain, which is asserted like everywhere else.
"""
import numpy as np
import pytest
import torch

from conv_ref import (ACT_LRELU, ACT_NONE, ACT_RELU, ACT_TANH, PAD_REFLECT, PAD_ZERO, PAIR_GRANULE, assert_exact_domain, bias_grid,
                      conv_pair_ref, conv_pair_s, conv_taps_ref, epilogue, first_diff, fold_frame, fused_store_bf16, int_grid,
                      pack_tap, pair_grid, store_bf16, store_f32, store_pair)

pytestmark = pytest.mark.gpu

ACT_SIGMOID = 4
SENT = -24576.0          # a bf16 value no case produces
BF16, PAIR, F32 = "bf16", "pair", "f32"
ACT_NAMES = {ACT_NONE: "none", ACT_RELU: "relu", ACT_LRELU: "lrelu", ACT_TANH: "tanh", ACT_SIGMOID: "sigmoid"}


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


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _assert_bits(got, want, what):
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not torch.equal(_bits(got), _bits(want)):
        idx, g, w, n = first_diff(got.float(), want.float()) or ((), 0.0, 0.0, 0)
        raise AssertionError("%s: %d elements differ, first at (n, y, x, c) = %s (16-column tile %s, row tile of 8: %s): got %r, want %r" % (
            what, n, idx, idx[2] // 16 if idx else "", idx[1] // 8 if idx else "", g, w))


def _ceil(a, b):
    return (a + b - 1) // b


def _bn(cout):
    return 128 if cout > 64 else 64 if cout > 32 else 32 if cout > 16 else 16


def fwd_taps():
    return [pack_tap(ky - 1, kx - 1, ky * 3 + kx) for ky in range(3) for kx in range(3)]


def flip_taps():
    return [pack_tap(1 - ky, 1 - kx, ky * 3 + kx) for ky in range(3) for kx in range(3)]


def _pack_w(w, npad, fill=5.0):
    out = torch.full((w.shape[0], npad, w.shape[2]), fill, dtype=torch.float64)
    out[:, :w.shape[1]] = w
    return out


# ---------------------------------------------------------------------------- activation x store form
ACT_SHAPES = {
    "halo_64to64_33x17": dict(cin=64, cout=64, H=33, W=17, B=2, nslabs={BF16: 10, PAIR: 10}),
    "halo_128to256_33x17": dict(cin=128, cout=256, H=33, W=17, B=2, nslabs={BF16: 10, PAIR: 6}),
    "gather_32to32_13x15": dict(cin=32, cout=32, H=13, W=15, B=2, nslabs={BF16: 2, PAIR: 2}),
}
_ACT_REF = {}


def _act_reference(name, form, smooth):
    """Operands and exact pre-activation of a case, computed once per (shape, operand kind, weight density) and left unchanged."""
    key = (name, form != BF16, smooth)
    if key in _ACT_REF:
        return _ACT_REF[key]
    c = ACT_SHAPES[name]
    rng = np.random.default_rng(1000 + 7 * sorted(ACT_SHAPES).index(name) + 2 * (form != BF16) + smooth)
    pair = form != BF16
    taps = fwd_taps()
    shape_x, shape_w = (c["B"], c["H"], c["W"], c["cin"]), (9, c["cout"], c["cin"])
    x = pair_grid(rng, shape_x) if pair else int_grid(rng, shape_x, -3, 3)
    w = pair_grid(rng, shape_w) if pair else int_grid(rng, shape_w, -3, 3)
    if smooth:      # tanh / sigmoid: about three non-zero terms per output, pre-activations of a few units
        w = w * torch.from_numpy((rng.random(shape_w) < 3.0 / (9 * c["cin"])).astype(np.float64))
    bs = bias_grid(rng, c["cout"])
    w[:, 3, :] = 0.0      # channel 3: pre-activation exactly zero everywhere
    bs[3] = 0.0
    if pair:
        acc = conv_pair_ref(x, w, taps, c["H"], c["W"], 1, PAD_REFLECT)
        assert_exact_domain(conv_pair_s(x, w, taps, c["H"], c["W"], 1, PAD_REFLECT), PAIR_GRANULE)
    else:
        acc = conv_taps_ref(x, w, taps, c["H"], c["W"], 1, PAD_REFLECT)
        assert_exact_domain(conv_taps_ref(x.abs(), w.abs(), taps, c["H"], c["W"], 1, PAD_REFLECT))
    pre = acc + bs
    assert bool((pre < 0).any()) and bool((pre == 0).any()) and bool((pre > 0).any()), "pre-activations of one sign only"
    _ACT_REF[key] = (x, w, bs, acc, pre)
    return _ACT_REF[key]


def _smooth_ref(pre, act):
    return torch.tanh(pre) if act == ACT_TANH else torch.sigmoid(pre)


def _act_case(dev, name, form, act):
    from cta_gan_amd import ops
    c = ACT_SHAPES[name]
    smooth = act in (ACT_TANH, ACT_SIGMOID)
    x, w, bs, acc, pre = _act_reference(name, form, smooth)
    B, H, W, cin, cout = c["B"], c["H"], c["W"], c["cin"], c["cout"]
    pair = form != BF16
    npad = _ceil(cout, _bn(cout)) * _bn(cout)
    wp = _pack_w(w, npad).to(dev)
    if pair:
        xd, wd = ops.to_pair(x.float().to(dev)), wp.float().contiguous()
    else:
        xd, wd = x.to(dev).bfloat16().contiguous(), wp.bfloat16().contiguous()
    bd = bs.float().to(dev)

    def new_y():
        if form == PAIR:
            y = ops.empty_act((B, H, W, cout), torch.bfloat16, dev)
            y.fill_(SENT)
            ops.pair_lo(y).fill_(SENT)
            return y
        return torch.full((B, H, W, cout), SENT, dtype=torch.float32 if form == F32 else torch.bfloat16, device=dev)

    y = new_y()
    taps = fwd_taps()
    ops.conv_igemm(xd, wd, npad, y, bd, cout, H, W, 0, 0, 1, 1, PAD_REFLECT, act, taps)
    torch.cuda.synchronize()
    what = "%s %s %s" % (name, form, ACT_NAMES[act])
    if smooth:
        want = _smooth_ref(pre, act)
        unsat = int(((want.abs() < 0.995) & (want.abs() > 0.005)).sum())
        assert unsat >= 100, (what, "saturated: only %d results away from the asymptotes" % unsat)
        got = (y.double() + ops.pair_lo(y).double()).cpu() if form == PAIR else y.double().cpu()
        store = {F32: 0.0, BF16: 2.0 ** -8, PAIR: 2.0 ** -16}[form]
        bound = 2e-4 + store * (want.abs() + 2e-4)
        err = (got - want).abs()
        print(what, "max err %.3g, worst fraction of the bound %.3g" % (float(err.max()), float((err / bound).max())))
        assert bool((err <= bound).all()), (what, float(err.max()), float((err / bound).max()))
    else:
        v = epilogue(acc, bs, act)
        if form == PAIR:
            hi, lo = store_pair(v)
            _assert_bits(y, hi, what + " hi plane")
            _assert_bits(ops.pair_lo(y), lo, what + " lo plane")
        else:
            _assert_bits(y, store_f32(v) if form == F32 else store_bf16(v), what)
    if form != F32 and act == ACT_NONE:      # path evidence: the twin launch without bias / activation
        y2 = new_y()
        _, ns = ops.conv_igemm(xd, wd, npad, y2, None, cout, H, W, 0, 0, 1, 1, PAD_REFLECT, ACT_NONE, taps, want_stats=True)
        torch.cuda.synchronize()
        print(what, "nslabs", ns)
        assert ns == c["nslabs"][form], (what, "slab count %d: not the intended kernel (%d)" % (ns, c["nslabs"][form]))


ACTS5 = [ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH, ACT_SIGMOID]


@pytest.mark.parametrize("act", ACTS5, ids=[ACT_NAMES[a] for a in ACTS5])
@pytest.mark.parametrize("name", list(ACT_SHAPES))
def test_activation_bf16_store(name, act, dev):
    _act_case(dev, name, BF16, act)


@pytest.mark.parametrize("act", ACTS5, ids=[ACT_NAMES[a] for a in ACTS5])
@pytest.mark.parametrize("name", list(ACT_SHAPES))
def test_activation_split_pair_store(name, act, dev, pair_mode):
    _act_case(dev, name, PAIR, act)


@pytest.mark.parametrize("act", ACTS5, ids=[ACT_NAMES[a] for a in ACTS5])
@pytest.mark.parametrize("name", list(ACT_SHAPES))
def test_activation_fp32_store(name, act, dev, pair_mode):
    _act_case(dev, name, F32, act)


# ---------------------------------------------------------------------------- FUSE with InstanceNorm-backward sums
def _tile_ids(h, w, th):
    return (torch.arange(h)[:, None] // th) * _ceil(w, 16) + torch.arange(w)[None, :] // 16, _ceil(h, th) * _ceil(w, 16)


def _tile_sums(t, ids, cnt):
    """[B, H, W, C] float64 -> per-tile sums [B, cnt, C]."""
    b, h, w, c = t.shape
    out = torch.zeros(b, cnt, c, dtype=torch.float64)
    out.index_add_(1, ids.reshape(-1), t.reshape(b, h * w, c))
    return out


_FUSE_REF = {}


def fuse_reference(cin, ch, B, H, W, th, pair, seed, lo=-3, hi=3, wdens=1.0, epis=("res", "fold", "res_fold")):
    """Operands, the three stored gradients (res / fold / both) and, per activation, the exact per-tile sums of a FUSE case -- on
    the CPU, once per shape.  Every exact-domain condition is asserted here, before anything is launched."""
    key = (cin, ch, B, H, W, th, pair, seed)
    if key in _FUSE_REF:
        return _FUSE_REF[key]
    rng = np.random.default_rng(seed)
    taps = flip_taps()
    if pair:
        x, w = pair_grid(rng, (B, H, W, cin)), pair_grid(rng, (9, ch, cin))
    else:
        x, w = int_grid(rng, (B, H, W, cin), lo, hi), int_grid(rng, (9, ch, cin), lo, hi)
    if wdens < 1.0:
        w = w * torch.from_numpy((rng.random(tuple(w.shape)) < wdens).astype(np.float64))
    if pair:
        acc = conv_pair_ref(x, w, taps, H, W, 1, PAD_ZERO)
        assert_exact_domain(conv_pair_s(x, w, taps, H, W, 1, PAD_ZERO), PAIR_GRANULE)
    else:
        acc = conv_taps_ref(x, w, taps, H, W, 1, PAD_ZERO)
        assert_exact_domain(torch.tensor(float(x.abs().max() * w.abs().max()) * cin * 9))      # >= the sum of the terms' magnitudes
    res = pair_grid(rng, (B, H, W, ch)) if pair else int_grid(rng, (B, H, W, ch), -3, 3)
    fold = int_grid(rng, (B, H + 2, W + 2, ch), -3, 3)
    for ey in (0, H + 1):
        for ex in (0, W + 1):
            fold[:, ey, ex] = torch.where(fold[:, ey, ex] == 0, torch.ones_like(fold[:, ey, ex]), fold[:, ey, ex])
    assert bool((fold[:, 1:-1, 1:-1] != 0).any()), "the fold's interior must hold values that a stray read would show"
    assert all(bool((fold[:, ey, ex] != 0).all()) for ey in (0, H + 1) for ex in (0, W + 1)), "frame corners"
    z = int_grid(rng, (B, H, W, ch), -3, 3)
    mean = int_grid(rng, (B, ch), -2, 2)
    rstd = torch.from_numpy(rng.choice(np.array([1.0, 2.0]) if pair else np.array([0.25, 0.5, 1.0, 2.0]), size=(B, ch)))
    xh = (z - mean[:, None, None, :]) * rstd[:, None, None, :]
    assert float((xh == 0).double().mean()) > 0.04, "xhat == 0 must occur: the mask is strict"
    granule = (PAIR_GRANULE if pair else 1.0) * float(rstd.min())
    v = epilogue(acc)
    ids, cnt = _tile_ids(H, W, th)
    npx = _tile_sums(torch.ones(1, H, W, 1, dtype=torch.float64), ids, cnt)[0, :, 0]
    stored, sums = {}, {}
    for epi in epis:
        r, f = (res if "res" in epi else None), (fold if "fold" in epi else None)
        if pair:
            tot = acc + (r if r is not None else 0.0) + (fold_frame(f) if f is not None else 0.0)
            tot32 = tot.numpy().astype(np.float32)
            assert np.array_equal(tot32.astype(np.float64), tot.numpy()), "the fp32 sum of the pair epilogue is not exact"
            assert_exact_domain(acc.abs() + (r.abs() if r is not None else 0.0) + (fold_frame(f.abs()) if f is not None else 0.0), PAIR_GRANULE)
            st = store_pair(tot32)
            g = st[0].double() + st[1].double()
        else:
            st = fused_store_bf16(v, r, f)
            g = st.double()
        stored[epi] = st
        for act in (ACT_NONE, ACT_RELU, ACT_LRELU):
            if act == ACT_NONE:
                gm = g
            elif act == ACT_RELU:
                gm = torch.where(xh > 0, g, torch.zeros_like(g))
            else:
                g02 = torch.from_numpy((np.float32(0.2) * g.numpy().astype(np.float32)).astype(np.float32)).double()
                gm = torch.where(xh > 0, g, g02)
            want = torch.stack([_tile_sums(gm, ids, cnt), _tile_sums(gm * xh, ids, cnt)], dim=-1)
            mag = torch.stack([_tile_sums(gm.abs(), ids, cnt), _tile_sums((gm * xh).abs(), ids, cnt)], dim=-1)
            if act != ACT_LRELU:
                assert_exact_domain(mag, granule)
            sums[(epi, act)] = (want, mag)
    _FUSE_REF[key] = dict(x=x, w=w, res=res, fold=fold, z=z, mean=mean, rstd=rstd, stored=stored, sums=sums, npx=npx, cnt=cnt)
    return _FUSE_REF[key]


def _fuse_case(dev, ref, cin, ch, B, H, W, pair, epi, act, what):
    from cta_gan_amd import ops
    npad = _ceil(ch, _bn(ch)) * _bn(ch)
    wp = _pack_w(ref["w"], npad).to(dev)
    if pair:
        cv = lambda t: ops.to_pair(t.float().to(dev))
        xd, wd = cv(ref["x"]), wp.float().contiguous()
        y = ops.empty_act((B, H, W, ch), torch.bfloat16, dev)
        y.fill_(SENT)
        ops.pair_lo(y).fill_(SENT)
    else:
        cv = lambda t: t.to(dev).bfloat16().contiguous()
        xd, wd = cv(ref["x"]), wp.bfloat16().contiguous()
        y = torch.full((B, H, W, ch), SENT, dtype=torch.bfloat16, device=dev)
    kw = {}
    if "res" in epi:
        kw["res"] = cv(ref["res"])
    if "fold" in epi:
        kw["fold"] = cv(ref["fold"])
    part, ns = ops.conv_igemm(xd, wd, npad, y, None, ch, H, W, 0, 0, 1, 1, PAD_ZERO, ACT_NONE, flip_taps(),
                              in_bwd=(cv(ref["z"]), ref["mean"].float().to(dev), ref["rstd"].float().to(dev), act), **kw)
    torch.cuda.synchronize()
    st = ref["stored"][epi]
    if pair:
        _assert_bits(y, st[0], what + " hi plane")
        _assert_bits(ops.pair_lo(y), st[1], what + " lo plane")
    else:
        _assert_bits(y, st, what)
    assert ns == ref["cnt"], (what, "slab count %d: not the intended tile shape (%d)" % (ns, ref["cnt"]))
    want, mag = ref["sums"][(epi, act)]
    got = part.double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if act == ACT_LRELU:
        bound = ref["npx"][None, :, None, None] * 2.0 ** -24 * mag
        err = (got - want).abs()
        frac = float((err / bound.clamp_min(1e-300))[bound > 0].max())
        print(what, "lrelu sums: worst fraction of the bound %.3g" % frac)
        bad = err > bound
    else:
        bad = got != want
    if bool(bad.any()):
        i = tuple(int(k) for k in bad.nonzero()[0])
        raise AssertionError("%s: %d of %d partial sums wrong, first at (n, tile, c, which) = %s: got %r want %r" % (
            what, int(bad.sum()), bad.numel(), i, float(got[i]), float(want[i])))


ACTS3 = [ACT_NONE, ACT_RELU, ACT_LRELU]


@pytest.mark.parametrize("act", ACTS3, ids=[ACT_NAMES[a] for a in ACTS3])
@pytest.mark.parametrize("epi", ["res", "fold", "res_fold"])
@pytest.mark.parametrize("grid", [(48, 48), (33, 17)], ids=["48x48", "33x17"])
@pytest.mark.parametrize("ch", [64, 256])
def test_fuse_instnorm_backward_sums(ch, grid, epi, act, dev):
    h, w = grid
    lo = 3 if ch == 64 else 2
    ref = fuse_reference(ch, ch, 2, h, w, 8, False, 3000 + ch + h, -lo, lo)
    _fuse_case(dev, ref, ch, ch, 2, h, w, False, epi, act, "fuse %d %dx%d %s %s" % (ch, h, w, epi, ACT_NAMES[act]))


@pytest.mark.parametrize("act", [ACT_RELU, ACT_LRELU], ids=["relu", "lrelu"])
def test_fuse_instnorm_backward_sums_16_row_tiles(act, dev):
    """64 -> 256 channels, 3 x 128 x 128: 384 workgroups, the BN 128 / TH 16 instantiation the training step runs."""
    ref = fuse_reference(64, 256, 3, 128, 128, 16, False, 3500, -1, 1, epis=("res_fold",))
    _fuse_case(dev, ref, 64, 256, 3, 128, 128, False, "res_fold", act, "fuse th16 res_fold %s" % ACT_NAMES[act])


@pytest.mark.parametrize("act", ACTS3, ids=[ACT_NAMES[a] for a in ACTS3])
@pytest.mark.parametrize("epi", ["res", "fold", "res_fold"])
def test_fuse_instnorm_backward_sums_split_pair(epi, act, dev, pair_mode):
    ref = fuse_reference(64, 64, 2, 48, 48, 8, True, 3600, wdens=0.02)
    _fuse_case(dev, ref, 64, 64, 2, 48, 48, True, epi, act, "fuse pair 64 48x48 %s %s" % (epi, ACT_NAMES[act]))
