"""GPU: the small kernels between the convolutions -- csrc/spatial.hip (max pool, bilinear x2, channel copies, the tiny-channel
packers, weight / activation splitting) and the gradient glue at the end of csrc/norm_act.hip (grad_combine, the folds, the
activation backward, the bias gradients) -- each against stock torch on the CPU in float64, at the smallest shapes where they
can still go wrong: odd sizes, H = pad + 1, channel slices at a non-zero offset of a wider buffer, accumulate on and off, ties
in a pooling window, empty reduction slabs, and the second trip of the grid-stride loop.

The reference sees what the kernel reads: inputs are rounded to the storage type first (`_Buf.put` writes fp32 / bf16 / the two
bf16 planes hi = bf16(x), lo = bf16(x - hi) of a split pair with torch, `_Buf.get` reads them back as float64; the pair_convert
test shows that ops.to_pair / ops.from_pair produce and read exactly these planes).

Bounds.
  exact     copies, packers, max pool without accumulate, zero and sentinel regions: bit-identical to the reference rounded once
            to the storage type.
  elementwise arithmetic (bilinear, grad_combine, folds, max pool with accumulate, gout, act_bwd):
            |got - want| <= r |want| + r S per element, S = the sum of |terms| that went into the element (for results that
            pass through an activation derivative S is taken before it: |act'| <= 1 for every activation here and its own
            rounding error is absolute O(2^-24)).  r = 2^-22 for fp32 (a few fp32 roundings), 2^-8 for bf16 (one
            round-to-nearest with a factor 2 of slack), 2^-22 + 2^-17 for the split pair (the fp32 bound plus the pair's storage
            precision, as in test_in_elementwise_batched_gpu.py).
  bias sums `_db_err` of test_kernels_gpu.py (error relative to the per-channel L2 norm of the summed gradient) under its GTOL:
            4e-4 fp32 (and the split pair, whose sums are fp32 sums of fp32-grade values), 5e-3 bf16.
  pair round trip  |x - (hi + lo)| <= 2^-16 |x|: each of the two roundings leaves at most 2^-8 of what it rounds.

Largest measured error, as a fraction of the bound above (printed by every test as "maxerr ..."; MI355X):
  kernel                 fp32     bf16     pair
  act_bwd_f32            0.165    -        -
  bias_grad              0.00175  6.5e-05  0.0012
  bias_grad_act db       0.0221   0.00016  0.0371
  bias_grad_act gout     0.309    0.498    0.487
  bilinear_bwd           0.41     0.483    0.43
  bilinear_fwd           0.344    0.498    0.484
  fold_f32               0.233    -        -
  grad_combine           0.313    0.498    0.484
  maxpool2_bwd+acc       0.125    0.498    0.484
  pair round trip        -        -        0.471
(a bf16 or pair result that is one term rounded once sits at half its bound by construction: S = |want| there.)

Found by this module: ops._nhwc took the channel count as the pixel pitch of a single-pixel view (B = H = W = 1), so a
split-pair handle of one pixel -- the max pool of a (1, 2, 2, C) input -- had its lo plane written C / 2 elements behind the hi
plane instead of one buffer width; it now reads the pitch from the strides the view kept.
"""
import contextlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

KINDS = ("fp32", "bf16", "pair")
TD = {"fp32": torch.float32, "bf16": torch.bfloat16, "pair": torch.bfloat16}
R = {"fp32": 2.0 ** -22, "bf16": 2.0 ** -8, "pair": 2.0 ** -22 + 2.0 ** -17}
GTOL = {"fp32": 4e-4, "bf16": 5e-3, "pair": 4e-4}
SENT = 7.0                       # fills every buffer outside the slice a kernel may write
GRID_ITEMS = 8192 * 256          # ew_blocks: items one trip of the grid-stride loop covers


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cta_gan_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@contextlib.contextmanager
def _mode(kind):
    """The wrappers' storage mode for `kind`: plain for fp32 / bf16, split pair for "pair", and for "mix" the plain bf16 backward
    of a split-pair forward (DT_MIX launches), set up as test_in_elementwise_batched_gpu.py sets up its DT_MIX case."""
    from cta_gan_amd import ops
    prev = (ops._PAIR_MODE, ops.PAIR_BWD_PLAIN)
    ops.set_pair_mode(kind in ("pair", "mix"), bwd_plain=kind == "mix")
    try:
        if kind == "mix":
            with ops.plain_backward():
                yield ops
        else:
            yield ops
    finally:
        ops.set_pair_mode(*prev)


class _Buf:
    """An NHWC operand of `kind` with C channels at channel offset c0 of a buffer of c0 + C + extra channels (dense: c0 = extra
    = 0); a split pair keeps its lo plane one buffer width behind the hi plane.  Everything is SENT until written."""

    def __init__(self, kind, shape, dev, c0=0, extra=0):
        b, h, w, c = shape
        self.kind, self.c, self.c0, self.cbuf = kind, c, c0, c0 + c + extra
        self.raw = torch.full((b, h, w, (2 if kind == "pair" else 1) * self.cbuf), SENT, dtype=TD[kind], device=dev)
        self.t = self.raw[..., c0:c0 + c]
        self.snap = None

    def lo(self):
        return self.raw[..., self.cbuf + self.c0:self.cbuf + self.c0 + self.c]

    def put(self, x):
        x = x.to(self.raw.device, torch.float32)
        if self.kind == "pair":
            hi = x.bfloat16()
            self.t.copy_(hi)
            self.lo().copy_((x - hi.float()).bfloat16())
        else:
            self.t.copy_(x.to(TD[self.kind]))
        return self

    def get(self):
        """What the buffer holds, float64 on the CPU."""
        v = self.t.double().cpu()
        return v + self.lo().double().cpu() if self.kind == "pair" else v

    def watch(self):
        self.snap = self.raw.clone()
        return self

    def outside_unchanged(self):
        a, b = self.raw.clone(), self.snap.clone()
        for t in (a, b):
            t[..., self.c0:self.c0 + self.c] = 0
            if self.kind == "pair":
                t[..., self.cbuf + self.c0:self.cbuf + self.c0 + self.c] = 0
        return torch.equal(a, b)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _stored_equal(ops, kind, out, ref32):
    """`out` (a wrapper's result; the hi view of a split pair) holds `ref32` rounded once to the storage type, bit for bit."""
    if kind == "fp32":
        return torch.equal(_bits(out), _bits(ref32))
    hi = ref32.bfloat16()
    if kind == "bf16":
        return torch.equal(_bits(out), _bits(hi))
    return torch.equal(_bits(out), _bits(hi)) and torch.equal(_bits(ops.pair_lo(out)), _bits((ref32 - hi.float()).bfloat16()))


def _randn(shape, dev, seed, scale=1.0):
    gen = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(tuple(shape), generator=gen, device=dev) * scale


_WORST = {}


def _note(name, kind, frac):
    key = (name, kind)
    _WORST[key] = max(_WORST.get(key, 0.0), frac)
    print("maxerr %-22s %-5s %.3g of the bound" % (name, kind, _WORST[key]))


def _close(name, kind, got, want, s, r=None):
    """|got - want| <= r |want| + r S per element (float64 CPU tensors)."""
    r = R[kind] if r is None else r
    assert got.shape == want.shape == s.shape, (got.shape, want.shape, s.shape)
    err, bound = (got - want).abs(), r * (want.abs() + s)
    _note(name, kind, float((err / bound.clamp_min(1e-300)).max()) if bool((bound > 0).any()) else 0.0)
    bad = err > bound
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError("%s %s: %d of %d elements out of bound, first at %s: got %r want %r bound %.3g" % (
            name, kind, int(bad.sum()), bad.numel(), i, float(got[i]), float(want[i]), float(bound[i])))


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _fold_ref(g, pad):
    """(fold(g), fold(|g|)) of a float64 NHWC padded-grid gradient: the autograd transpose of F.pad(mode="reflect")."""
    if pad == 0:
        return g, g.abs()
    b, hp, wp, c = g.shape
    x = torch.zeros((b, c, hp - 2 * pad, wp - 2 * pad), dtype=torch.float64, requires_grad=True)
    y = F.pad(x, (pad,) * 4, mode="reflect")
    f, = torch.autograd.grad(y, x, _nchw(g).contiguous(), retain_graph=True)
    s, = torch.autograd.grad(y, x, _nchw(g).abs().contiguous())
    return _nhwc(f), _nhwc(s)


def _dact(ops, y, act):
    """act'(.) through the activation's saved OUTPUT y (float64)."""
    if act == ops.ACT_RELU:
        return (y > 0).double()
    if act == ops.ACT_LRELU:
        d = torch.full_like(y, 0.2)
        d[y > 0] = 1.0
        return d
    if act == ops.ACT_TANH:
        return 1.0 - y * y
    if act == ops.ACT_SIGMOID:
        return y * (1.0 - y)
    return torch.ones_like(y)


def _act_out(ops, pre, act):
    """A saved activation output made from the pre-activation `pre` (fp32, device); ReLU's has exact zeros."""
    if act == ops.ACT_RELU:
        return F.relu(pre)
    if act == ops.ACT_LRELU:
        return F.leaky_relu(pre, 0.2)
    if act == ops.ACT_TANH:
        return torch.tanh(pre)
    if act == ops.ACT_SIGMOID:
        return torch.sigmoid(pre)
    return pre


def _channels(kind, cs):
    return ((4,) if kind == "fp32" else ()) + tuple(cs)


def _slice(on, c0, extra):
    return dict(c0=c0, extra=extra) if on else {}


# ------------------------------------------------------------------------------------------------------------------ max pool
MP_SIZES = [(2, 2), (3, 5), (8, 12), (9, 6)]


def _maxpool_case(ops, kind, xval, sliced, seed, dev, forward=True):
    """Forward, then backward with accumulate 0 and 1, of one input `xval` (fp32 NHWC, device).  kind "mix": the saved input is a
    split pair, gradients in and out plain bf16 (no forward: the mode only exists in a backward)."""
    b, h, w, c = xval.shape
    ho, wo = h // 2, w // 2
    xk, gk = ("pair", "bf16") if kind == "mix" else (kind, kind)
    x = _Buf(xk, (b, h, w, c), dev, **_slice(sliced, 8, 16)).put(xval)
    xr = _nchw(x.get()).clone().requires_grad_(True)
    pr = F.max_pool2d(xr, 2)
    if forward:
        out = _Buf(kind, (b, ho, wo, c), dev, **_slice(sliced, 16, 8)).watch()
        ops.maxpool2_fwd(x.t, out.t)
        assert torch.equal(out.get(), _nhwc(pr.detach())), ("maxpool fwd", kind, tuple(xval.shape), sliced)
        assert out.outside_unchanged()
    g = _Buf(gk, (b, ho, wo, c), dev, **_slice(sliced, 24, 0)).put(_randn((b, ho, wo, c), dev, seed + 1))
    pr.backward(_nchw(g.get()))
    want = _nhwc(xr.grad)
    for acc in (0, 1):
        dx = _Buf(gk, (b, h, w, c), dev, **_slice(sliced, 8, 8)).put(_randn((b, h, w, c), dev, seed + 2)).watch()
        pre = dx.get()
        ops.maxpool2_bwd(x.t, g.t, dx.t, acc)
        got = dx.get()
        where = ("maxpool bwd", kind, tuple(xval.shape), sliced, acc)
        if acc:
            _close("maxpool2_bwd+acc", kind if kind != "mix" else "bf16", got, pre + want, pre.abs() + want.abs())
        else:
            assert torch.equal(got, want), where
        # the trailing row / column of an odd size belongs to no window: exactly 0, or exactly the previous content
        rest = pre if acc else torch.zeros_like(pre)
        assert torch.equal(got[:, 2 * ho:], rest[:, 2 * ho:]) and torch.equal(got[:, :, 2 * wo:], rest[:, :, 2 * wo:]), where
        assert dx.outside_unchanged(), where
    return want


@pytest.mark.parametrize("kind", KINDS)
def test_maxpool_forward_backward_odd_sizes_slices_accumulate(kind, dev):
    with _mode(kind) as ops:
        seed = 100
        for h, w in MP_SIZES:
            for b in (1, 3):
                for c in _channels(kind, (8, 32, 96)):
                    for sliced in (False, True):
                        seed += 3
                        _maxpool_case(ops, kind, _randn((b, h, w, c), dev, seed), sliced, seed, dev)


@pytest.mark.parametrize("kind", KINDS)
def test_maxpool_gradient_goes_to_the_first_maximum_of_a_tied_window(kind, dev):
    """Inputs of three distinct values: most windows hold a tie, some are all equal; F.max_pool2d's backward is the rule."""
    with _mode(kind) as ops:
        vals = torch.tensor([-1.5, 0.25, 2.0], device=dev)
        for n, (h, w) in enumerate(MP_SIZES):
            gen = torch.Generator(device=dev).manual_seed(40 + n)
            xval = vals[torch.randint(0, 3, (3, h, w, 32), generator=gen, device=dev)]
            win = xval[:, :h // 2 * 2, :w // 2 * 2].reshape(3, h // 2, 2, w // 2, 2, 32)
            if (h, w) == (8, 12):
                assert bool((win.amax((2, 4)) == win.amin((2, 4))).any()), "no all-equal window in the tie case"
            for sliced in (False, True):
                _maxpool_case(ops, kind, xval, sliced, 50 + n, dev)


def test_maxpool_backward_mixed_takes_the_argmax_of_hi_plus_lo(dev):
    """DT_MIX: the hi planes of a window tie while hi + lo does not -- the gradient goes where the forward (which pooled hi + lo)
    took its maximum, not to the first maximum of the hi plane."""
    with _mode("mix") as ops:
        base = torch.tensor([1.0, 2.0, -0.5, 0.75], device=dev)
        seed = 70
        for h, w in MP_SIZES:
            for b, c in ((1, 8), (3, 32)):
                seed += 3
                gen = torch.Generator(device=dev).manual_seed(seed)
                bv = base[torch.randint(0, 4, (b, h, w, c), generator=gen, device=dev)]
                k = torch.randint(-4, 5, (b, h, w, c), generator=gen, device=dev).float()
                xval = bv + k * 2.0 ** -12 * bv.abs()          # hi = bf16(xval) = bv, lo = the perturbation, both exact
                assert torch.equal(xval.bfloat16().float(), bv)
                probe = _Buf("pair", (b, h, w, c), dev).put(xval)
                assert ops.dtc_saved(probe.t) == ops.DT_MIX and ops.dtc(probe.t) == 1
                for sliced in (False, True):
                    want = _maxpool_case(ops, "mix", xval, sliced, seed, dev, forward=False)
                if (h, w) == (8, 12) and c == 32:
                    hr = _nchw(bv.double().cpu()).clone().requires_grad_(True)
                    F.max_pool2d(hr, 2).backward(torch.ones((b, c, h // 2, w // 2), dtype=torch.float64))
                    assert want.shape == xval.shape
                    wr =_nchw(xval.double().cpu()).clone().requires_grad_(True)
                    F.max_pool2d(wr, 2).backward(torch.ones((b, c, h // 2, w // 2), dtype=torch.float64))
                    assert not torch.equal(hr.grad, wr.grad), "the hi plane alone picks the same pixels: the case tests nothing"


# ------------------------------------------------------------------------------------------------------------------ bilinear
BL_SIZES = [(1, 1), (1, 7), (5, 1), (3, 4), (8, 12)]


def _bilinear_ref(x, size):
    """(F.interpolate(x), F.interpolate(|x|)) of a float64 NHWC tensor."""
    up = lambda t: _nhwc(F.interpolate(_nchw(t), size=size, mode="bilinear", align_corners=False))
    return up(x), up(x.abs())


def _bilinear_bwd_ref(g, size_in):
    b, ho, wo, c = g.shape
    x = torch.zeros((b, c) + tuple(size_in), dtype=torch.float64, requires_grad=True)
    y = F.interpolate(x, size=(ho, wo), mode="bilinear", align_corners=False)
    d, = torch.autograd.grad(y, x, _nchw(g).contiguous(), retain_graph=True)
    s, = torch.autograd.grad(y, x, _nchw(g).abs().contiguous())
    return _nhwc(d), _nhwc(s)


@pytest.mark.parametrize("kind", KINDS)
def test_bilinear_x2_forward_backward_through_concat_slices(kind, dev):
    with _mode(kind) as ops:
        seed = 200
        b = 2
        for hi, wi in BL_SIZES:
            for c in _channels(kind, (8, 32)):
                for c0 in (0, 8):       # the upsampled half of a concat buffer: at offset 0 or behind the skip tensor
                    seed += 2
                    x = _Buf(kind, (b, hi, wi, c), dev, **_slice(c0 > 0, 16, 8)).put(_randn((b, hi, wi, c), dev, seed))
                    out = _Buf(kind, (b, 2 * hi, 2 * wi, c), dev, c0=c0, extra=24).watch()
                    ops.bilinear_fwd(x.t, out.t)
                    want, s = _bilinear_ref(x.get(), (2 * hi, 2 * wi))
                    _close("bilinear_fwd", kind, out.get(), want, s)
                    assert out.outside_unchanged()
                    g = _Buf(kind, (b, 2 * hi, 2 * wi, c), dev, c0=c0, extra=24).put(_randn((b, 2 * hi, 2 * wi, c), dev, seed + 1))
                    dx = _Buf(kind, (b, hi, wi, c), dev, **_slice(c0 > 0, 8, 16)).watch()
                    ops.bilinear_bwd(g.t, dx.t)
                    want, s = _bilinear_bwd_ref(g.get(), (hi, wi))
                    _close("bilinear_bwd", kind, dx.get(), want, s)
                    assert dx.outside_unchanged()


@pytest.mark.parametrize("kind", KINDS)
def test_bilinear_forward_non_doubling_and_backward_refuses_it(kind, dev):
    """5x7 -> 8x16: neither axis doubles.  Power-of-two output sizes keep scale * (o + 0.5) - 0.5 exact in fp32, so the float64
    reference interpolates with the kernel's weights."""
    with _mode(kind) as ops:
        b, c = 2, 8
        x = _Buf(kind, (b, 5, 7, c), dev, c0=8, extra=8).put(_randn((b, 5, 7, c), dev, 31))
        out = _Buf(kind, (b, 8, 16, c), dev, c0=16, extra=8).watch()
        ops.bilinear_fwd(x.t, out.t)
        want, s = _bilinear_ref(x.get(), (8, 16))
        _close("bilinear_fwd", kind, out.get(), want, s)
        assert out.outside_unchanged()
        dx = _Buf(kind, (b, 5, 7, c), dev).watch()
        with pytest.raises(RuntimeError, match="CTG_EINVAL"):
            ops.bilinear_bwd(out.t, dx.t)
        torch.cuda.synchronize()
        assert torch.equal(dx.raw, dx.snap)


# ------------------------------------------------------------------------------------------------------------------ copies, packers
@pytest.mark.parametrize("kind", KINDS)
def test_copy_channels_between_slices_bit_for_bit(kind, dev):
    with _mode(kind) as ops:
        seed = 300
        for c in _channels(kind, (8, 32)):
            for s_sl, d_sl in ((True, False), (False, True), (True, True)):
                seed += 1
                shape = (2, 3, 5, c)
                src = _Buf(kind, shape, dev, **_slice(s_sl, 8, 16)).put(_randn(shape, dev, seed))
                dst = _Buf(kind, shape, dev, **_slice(d_sl, 24, 8)).watch()
                ops.copy_channels(src.t, dst.t)
                assert torch.equal(_bits(dst.t), _bits(src.t)), (kind, c, s_sl, d_sl)
                if kind == "pair":
                    assert torch.equal(_bits(dst.lo()), _bits(src.lo())), (kind, c, s_sl, d_sl)
                    assert bool((src.lo() != 0).any())
                assert dst.outside_unchanged()


@pytest.mark.parametrize("kind", KINDS)
def test_chan_pad_pads_with_exact_zeros(kind, dev):
    """P = 357 pixels: odd, and the second block of 256 is ragged.  Cs = 2 reads float2 from an 8-byte-aligned source and scalars
    from one that starts 4 bytes into its allocation."""
    with _mode(kind) as ops:
        b, h, w = 1, 3, 119
        for cs in (1, 2, 3, 4):
            for cpad in (8, 32):
                for off in ((0, 1) if cs == 2 else (0,)):
                    flat = _randn((b * h * w * cs + off,), dev, 400 + cs)
                    src = flat[off:].view(b, h, w, cs)
                    assert src.is_contiguous() and src.data_ptr() % 8 == 4 * off
                    out = ops.chan_pad(src, cs, TD[kind], cpad)
                    assert tuple(out.shape) == (b, h, w, cpad)
                    ref = torch.zeros((b, h, w, cpad), device=dev)
                    ref[..., :cs] = src
                    assert _stored_equal(ops, kind, out, ref), (kind, cs, cpad, off)
                    assert float(out[..., cs:].float().abs().max()) == 0.0
                    if kind == "pair":
                        assert float(ops.pair_lo(out)[..., cs:].float().abs().max()) == 0.0


IM2COL = [(7, 1, 3, True), (4, 2, 1, False), (3, 1, 1, False), (5, 1, 2, True)]


def _im2col_ref(planes, k, stride, pad, reflect, kpad):
    """[B, Ho, Wo, kpad] float32: columns in the order of weight.view(Cout, Cin * k * k), zeros beyond."""
    x = torch.stack(planes, 1).double().cpu()
    b, cin, h, w = x.shape
    xp = F.pad(x, (pad,) * 4, mode="reflect") if reflect else F.pad(x, (pad,) * 4)
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    cols = F.unfold(xp, k, stride=stride).view(b, cin * k * k, ho, wo)
    ref = torch.zeros((b, ho, wo, kpad), dtype=torch.float64)
    ref[..., :cin * k * k] = _nhwc(cols)
    return ref.float()


@pytest.mark.parametrize("kind", KINDS)
def test_im2col_pack_columns_in_weight_order(kind, dev):
    with _mode(kind) as ops:
        seed = 500
        for cin in (1, 2):
            for k, stride, pad, reflect in IM2COL:
                for h, w in ((4, 4), (7, 9), (17, 33)):
                    seed += 1
                    planes = [_randn((2, h, w), dev, seed * 2 + i) for i in range(cin)]
                    kpad = (cin * k * k + 31) // 32 * 32
                    out = ops.im2col_pack(planes[0], planes[1] if cin == 2 else None, k, stride, pad,
                                          ops.PAD_REFLECT if reflect else ops.PAD_ZERO, TD[kind], kpad)
                    ref = _im2col_ref(planes, k, stride, pad, reflect, kpad).to(dev)
                    assert tuple(out.shape) == tuple(ref.shape)
                    assert _stored_equal(ops, kind, out, ref), (kind, cin, k, stride, pad, reflect, h, w)


def test_im2col_pack_refuses_a_reflection_wider_than_the_image(dev):
    with _mode("fp32") as ops:
        img = _randn((1, 3, 8), dev, 1)
        with pytest.raises(RuntimeError, match="CTG_EINVAL"):
            ops.im2col_pack(img, None, 7, 1, 3, ops.PAD_REFLECT, torch.float32, 64)
        img = _randn((1, 8, 3), dev, 1)
        with pytest.raises(RuntimeError, match="CTG_EINVAL"):
            ops.im2col_pack(img, None, 7, 1, 3, ops.PAD_REFLECT, torch.float32, 64)
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ splitting
def _split_ref(w):
    """[P, C] fp32 -> [P, 2C] bf16, per 32 channels [hi 32 | lo 32] with hi = bf16(w), lo = bf16(w - hi)."""
    p, c = w.shape
    hi = w.bfloat16()
    lo = (w - hi.float()).bfloat16()
    return torch.stack((hi.view(p, c // 32, 32), lo.view(p, c // 32, 32)), 2).reshape(p, 2 * c)


def test_split_weights_multi_seventy_jobs_in_three_launches(dev):
    """70 jobs = launches of 32, 32 and 6 (SPLIT_MAX_T); rows of 32 / 64 / 256 channels, 1 to 47 rows, so jobs own one block or
    several with a ragged last one.  Every copy lies between guard elements."""
    from cta_gan_amd import _lib, ops
    lib = _lib.load()
    packs, guards, singles = [], [], []
    for j in range(70):
        c = (32, 64, 256)[(j * 7 + j // 5) % 3]
        p = 1 + (j * 11) % 47
        w = _randn((p, c), dev, 600 + j, scale=10.0 ** ((j % 7) - 3))
        big = torch.full((p * 2 * c + 64,), SENT, dtype=torch.bfloat16, device=dev)
        w._ctg_split3w_old = big[32:32 + p * 2 * c].view(p, 2 * c)
        assert w._ctg_split3w_old.data_ptr() % 16 == 0
        single = torch.empty((p, 2 * c), dtype=torch.bfloat16, device=dev)
        _lib.check(lib.ctg_split_weights(w.data_ptr(), c, single.data_ptr(), c, p, ops._stream()), "ctg_split_weights")
        packs.append(w)
        guards.append(big)
        singles.append(single)
    assert {w.shape[1] for w in packs} == {32, 64, 256}
    assert any(w.numel() // 8 > 256 and (w.numel() // 8) % 256 for w in packs)       # a job of several blocks, the last ragged
    ops.split_w_pair_refresh(packs)
    for j, (w, big, single) in enumerate(zip(packs, guards, singles)):
        got = w._ctg_split3w
        assert got.data_ptr() == big.data_ptr() + 64 and w._ctg_split3w_old is None
        assert torch.equal(_bits(got), _bits(single)), ("job %d differs from ctg_split_weights" % j, tuple(w.shape))
        assert torch.equal(_bits(got), _bits(_split_ref(w))), ("job %d differs from the definition" % j, tuple(w.shape))
        assert bool((big[:32] == SENT).all()) and bool((big[-32:] == SENT).all()), j


def test_pair_convert_with_pitched_rows_both_directions(dev):
    """fp32 rows of pitch > C -> pair rows of pitch > 2C and back; the planes are hi = bf16(x), lo = bf16(x - hi) -- the definition
    `_Buf` writes and reads by -- and ops.from_pair reads hi + lo."""
    from cta_gan_amd import _lib
    lib = _lib.load()
    with _mode("pair") as ops:
        for c in (8, 40):
            shape = (2, 3, 5, c)
            p = 2 * 3 * 5
            xval = _randn(shape, dev, 700 + c) * torch.logspace(-3, 3, c, device=dev)
            src = _Buf("fp32", shape, dev, c0=4, extra=4).put(xval)
            dst = _Buf("pair", shape, dev, c0=8, extra=8).watch()
            ops.to_pair(src.t, out=dst.t)
            want = _Buf("pair", shape, dev, c0=8, extra=8).put(xval)
            assert torch.equal(_bits(dst.t), _bits(want.t)) and torch.equal(_bits(dst.lo()), _bits(want.lo()))
            assert dst.outside_unchanged()
            back = _Buf("fp32", shape, dev, c0=4, extra=12).watch()
            _lib.check(lib.ctg_pair_convert(1, dst.t.data_ptr(), dst.t.stride(2), back.t.data_ptr(), back.t.stride(2), c, p,
                                            ops._stream()), "ctg_pair_convert")
            assert torch.equal(back.get(), dst.get()) and back.outside_unchanged()
            assert torch.equal(ops.from_pair(dst.t).double().cpu(), dst.get())
            x64 = xval.double().cpu()
            frac = float(((back.get() - x64).abs() / x64.abs()).max()) / 2.0 ** -16
            _note("pair round trip", "pair", frac)
            assert frac <= 1.0


# ------------------------------------------------------------------------------------------------------------------ gradient glue
def _glue_sizes(pad):
    return [(pad + 1, pad + 1), (pad + 1, 9), (5, 7), (16, 16)]


@pytest.mark.parametrize("pad", [0, 1, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_grad_combine_sum_fold_and_activation(kind, pad, dev):
    """out = a + fold(b), times act'(y): a only, b only and both; no activation, ReLU, LeakyReLU, Tanh; every operand a slice of a
    wider buffer.  At H = pad + 1 the interior rows 1 .. pad - 1 collect three source rows each."""
    with _mode(kind) as ops:
        seed = 800 + 10 * pad
        b = 2
        acts = (None, ops.ACT_RELU, ops.ACT_LRELU, ops.ACT_TANH)
        for h, w in _glue_sizes(pad):
            for c in (8, 32):
                seed += 5
                shape, pshape = (b, h, w, c), (b, h + 2 * pad, w + 2 * pad, c)
                a = _Buf(kind, shape, dev, c0=8, extra=0).put(_randn(shape, dev, seed))
                bb = _Buf(kind, pshape, dev, c0=16, extra=8).put(_randn(pshape, dev, seed + 1))
                ys = {act: _Buf(kind, shape, dev, c0=8, extra=8).put(_act_out(ops, _randn(shape, dev, seed + 2), act))
                      for act in acts if act is not None}
                out = _Buf(kind, shape, dev, c0=24, extra=8).watch()
                av, (fb, sb) = a.get(), _fold_ref(bb.get(), pad)
                for use_a, use_b in ((True, False), (False, True), (True, True)):
                    want = (av if use_a else 0) + (fb if use_b else 0)
                    s = (av.abs() if use_a else 0) + (sb if use_b else 0)
                    for act in acts:
                        y = ys.get(act)
                        ops.grad_combine(a.t if use_a else None, bb.t if use_b else None, pad, None if y is None else y.t,
                                         act or 0, out.t)
                        ref = want if y is None else want * _dact(ops, y.get(), act)
                        _close("grad_combine", kind, out.get(), ref, s)
                        assert out.outside_unchanged()


@pytest.mark.parametrize("pad", [1, 3])
def test_fold_f32_is_the_transpose_of_reflection_padding(pad, dev):
    with _mode("fp32") as ops:
        seed = 900 + pad
        for h, w in _glue_sizes(pad):
            for c in (1, 2, 3):
                seed += 1
                dp = _randn((2, h + 2 * pad, w + 2 * pad, c), dev, seed)
                out = ops.fold_f32(dp, pad)
                want, s = _fold_ref(dp.double().cpu(), pad)
                _close("fold_f32", "fp32", out.double().cpu(), want, s)


def test_act_bwd_f32_every_activation(dev):
    with _mode("fp32") as ops:
        for act in (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_LRELU, ops.ACT_TANH, ops.ACT_SIGMOID):
            for n in (1, 255, 257):
                g = _randn((n,), dev, 1000 + n)
                y = _act_out(ops, _randn((n,), dev, 1001 + n), act)
                out = ops.act_bwd_f32(g, y, act)
                g64 = g.double().cpu()
                _close("act_bwd_f32", "fp32", out.double().cpu(), g64 * _dact(ops, y.double().cpu(), act), g64.abs())


def _db_err(got, want, gout):
    """test_kernels_gpu.py's metric: max |diff| relative to the per-channel L2 norm of the summed gradient (NHWC here)."""
    scale = gout.pow(2).sum((0, 1, 2)).sqrt().clamp_min(1e-20)
    return float(((got - want).abs() / scale).max())


BIAS_SHAPES = {"one_slab": (1, 2, 2), "several_slabs_b3": (3, 9, 15), "several_slabs_b17": (17, 20, 20), "empty_last_slab": (2, 82, 100)}


def _check_slab_arrangement(ops, name, b, hw):
    """The slab arrangement a shape is here for, from the wrappers' own rule (moments_partial_kernel: per = ceil(HW / nslabs))."""
    ns = ops._nslabs(b, hw)
    per = (hw + ns - 1) // ns
    if name == "one_slab":
        assert ns == 1
    elif name == "empty_last_slab":
        assert ns > 2 and (ns - 1) * per >= hw, (ns, per)                        # the last slab starts behind the last pixel
        assert 0 < hw - (ns - 2) * per < per, (ns, per)                           # and the one before it is partly filled
    else:
        assert ns > 1 and (ns - 1) * per < hw, (ns, per)                          # several slabs, none empty
        assert per % 64, (ns, per)                                                # ragged against a wave of pixel lanes


@pytest.mark.parametrize("name", list(BIAS_SHAPES))
@pytest.mark.parametrize("kind", KINDS)
def test_bias_grad_and_bias_grad_act_over_slab_arrangements(kind, name, dev):
    """db (+)= per-channel sum of fold(g) [* act'(y)] over one slab, several, and a launch whose last slab is empty; only the
    first `creal` entries of db may change; gout = fold(g) * act'(y) elementwise."""
    with _mode(kind) as ops:
        b, h, w = BIAS_SHAPES[name]
        _check_slab_arrangement(ops, name, b, h * w)
        seed = 1100
        for c in (8, 64, 512):
            for pad in (0, 1, 3):
                if pad >= min(h, w):
                    continue                                    # reflection needs pad < H, W
                seed += 4
                shape, pshape = (b, h, w, c), (b, h + 2 * pad, w + 2 * pad, c)
                g = _Buf(kind, pshape, dev, c0=8, extra=8).put(_randn(pshape, dev, seed))
                fg, sg = _fold_ref(g.get(), pad)
                ys = {act: _Buf(kind, shape, dev, c0=16, extra=0).put(_act_out(ops, _randn(shape, dev, seed + 1), act))
                      for act in (ops.ACT_RELU, ops.ACT_LRELU)}
                gm = {act: fg * _dact(ops, y.get(), act) for act, y in ys.items()}
                gout = _Buf(kind, shape, dev, c0=8, extra=16).watch()
                first = True
                for creal in (c, c - 3, 1):
                    for acc in (0, 1):
                        pre = _randn((c,), dev, seed + 2 + acc)
                        db = pre.clone()
                        ops.bias_grad(g.t, pad, creal, db, accumulate=bool(acc))
                        want = fg.sum((0, 1, 2)) + (pre.double().cpu() if acc else 0)
                        got = db.double().cpu()
                        err = _db_err(got[:creal], want[:creal], fg[..., :creal])
                        _note("bias_grad", kind, err / GTOL[kind])
                        assert err < GTOL[kind], ("bias_grad", kind, name, c, pad, creal, acc, err)
                        assert torch.equal(db[creal:], pre[creal:]), ("bias_grad wrote beyond creal", c, pad, creal, acc)
                        for act in (ops.ACT_RELU, ops.ACT_LRELU) if creal == c else (ops.ACT_LRELU,):
                            db = pre.clone()
                            ops.bias_grad_act(g.t, pad, ys[act].t, act, gout.t, creal, db, accumulate=bool(acc))
                            want = gm[act].sum((0, 1, 2)) + (pre.double().cpu() if acc else 0)
                            got = db.double().cpu()
                            err = _db_err(got[:creal], want[:creal], gm[act][..., :creal])
                            _note("bias_grad_act db", kind, err / GTOL[kind])
                            assert err < GTOL[kind], ("bias_grad_act", kind, name, c, pad, creal, acc, act, err)
                            assert torch.equal(db[creal:], pre[creal:]), ("bias_grad_act wrote beyond creal", c, pad, creal, acc)
                            if first:       # (the pixel loop knows neither creal nor accumulate)
                                _close("bias_grad_act gout", kind, gout.get(), gm[act], sg)
                                assert gout.outside_unchanged()
                        first = False


def test_bias_grad_act_refuses_tanh(dev):
    with _mode("fp32") as ops:
        g = _randn((1, 4, 4, 8), dev, 1)
        y = torch.tanh(_randn((1, 4, 4, 8), dev, 2))
        gout = torch.full_like(g, SENT)
        db = torch.full((8,), SENT, device=dev)
        with pytest.raises(RuntimeError, match="CTG_EINVAL"):
            ops.bias_grad_act(g, 0, y, ops.ACT_TANH, gout, 8, db)
        torch.cuda.synchronize()
        assert bool((gout == SENT).all()) and bool((db == SENT).all())


# ------------------------------------------------------------------------------------------------------------------ grid-stride
# ew_blocks caps a launch at 8192 blocks of 256 threads: one case per kernel with a few more items than that (and no multiple
# of it), so the last items are reached only in a thread's second trip; the whole result is compared.  fp32 throughout.
def _second_trip(items):
    assert GRID_ITEMS < items < 2 * GRID_ITEMS and items % GRID_ITEMS, items


def test_grid_stride_maxpool_forward(dev):
    with _mode("fp32") as ops:
        b, h, w, c = 1, 2051, 2049, 8
        _second_trip(b * (h // 2) * (w // 2) * (c // 4))
        x = _randn((b, h, w, c), dev, 1201)
        out = torch.full((b, h // 2, w // 2, c), SENT, device=dev)
        ops.maxpool2_fwd(x, out)
        want = _nhwc(F.max_pool2d(_nchw(x.double().cpu()), 2))
        assert torch.equal(out.double().cpu(), want)


def test_grid_stride_maxpool_backward(dev):
    with _mode("fp32") as ops:
        b, h, w, c = 1, 1025, 1025, 8
        _second_trip(b * h * w * (c // 4))
        x = _randn((b, h, w, c), dev, 1202)
        g = _randn((b, h // 2, w // 2, c), dev, 1203)
        dx = torch.full((b, h, w, c), SENT, device=dev)
        ops.maxpool2_bwd(x, g, dx, False)
        xr = _nchw(x.double().cpu()).clone().requires_grad_(True)
        F.max_pool2d(xr, 2).backward(_nchw(g.double().cpu()))
        assert torch.equal(dx.double().cpu(), _nhwc(xr.grad))


def test_grid_stride_bilinear_forward(dev):
    with _mode("fp32") as ops:
        b, hi, wi, c = 1, 513, 512, 8
        _second_trip(b * 2 * hi * 2 * wi * (c // 4))
        x = _randn((b, hi, wi, c), dev, 1204)
        out = torch.full((b, 2 * hi, 2 * wi, c), SENT, device=dev)
        ops.bilinear_fwd(x, out)
        want, s = _bilinear_ref(x.double().cpu(), (2 * hi, 2 * wi))
        _close("bilinear_fwd", "fp32", out.double().cpu(), want, s)


def test_grid_stride_bilinear_backward(dev):
    with _mode("fp32") as ops:
        b, hi, wi, c = 1, 1025, 1025, 8
        _second_trip(b * hi * wi * (c // 4))
        g = _randn((b, 2 * hi, 2 * wi, c), dev, 1205)
        dx = torch.full((b, hi, wi, c), SENT, device=dev)
        ops.bilinear_bwd(g, dx)
        want, s = _bilinear_bwd_ref(g.double().cpu(), (hi, wi))
        _close("bilinear_bwd", "fp32", dx.double().cpu(), want, s)


def test_grid_stride_copy_channels(dev):
    with _mode("fp32") as ops:
        shape = (1, 1050, 1000, 8)
        _second_trip(1050 * 1000 * 2)
        src = _Buf("fp32", shape, dev, c0=4, extra=4).put(_randn(shape, dev, 1206))
        dst = _Buf("fp32", shape, dev, c0=8, extra=0).watch()
        ops.copy_channels(src.t, dst.t)
        assert torch.equal(_bits(dst.t), _bits(src.t)) and dst.outside_unchanged()


def test_grid_stride_chan_pad(dev):
    with _mode("fp32") as ops:
        b, h, w, cs, cpad = 1, 1031, 2035, 3, 8
        _second_trip(b * h * w)                                  # one pixel per thread
        src = _randn((b, h, w, cs), dev, 1207)
        out = ops.chan_pad(src, cs, torch.float32, cpad)
        ref = torch.zeros((b, h, w, cpad), device=dev)
        ref[..., :cs] = src
        assert torch.equal(_bits(out), _bits(ref))


def test_grid_stride_im2col_pack(dev):
    with _mode("fp32") as ops:
        b, h, w, k = 1, 513, 512, 3
        _second_trip(b * h * w * (32 // 4))
        img = _randn((b, h, w), dev, 1208)
        out = ops.im2col_pack(img, None, k, 1, 1, ops.PAD_ZERO, torch.float32, 32)
        assert torch.equal(_bits(out), _bits(_im2col_ref([img], k, 1, 1, False, 32).to(dev)))


def test_grid_stride_grad_combine(dev):
    with _mode("fp32") as ops:
        b, h, w, c, pad = 1, 513, 512, 32, 1
        _second_trip(b * h * w * (c // 4))
        a = _randn((b, h, w, c), dev, 1209)
        bb = _randn((b, h + 2 * pad, w + 2 * pad, c), dev, 1210)
        y = F.leaky_relu(_randn((b, h, w, c), dev, 1211), 0.2)
        out = torch.full((b, h, w, c), SENT, device=dev)
        ops.grad_combine(a, bb, pad, y, ops.ACT_LRELU, out)
        fb, sb = _fold_ref(bb.double().cpu(), pad)
        a64 = a.double().cpu()
        _close("grad_combine", "fp32", out.double().cpu(), (a64 + fb) * _dact(ops, y.double().cpu(), ops.ACT_LRELU), a64.abs() + sb)


def test_grid_stride_fold_f32(dev):
    with _mode("fp32") as ops:
        b, h, w, c, pad = 1, 700, 1000, 3, 3
        _second_trip(b * h * w * c)                              # one element per thread
        dp = _randn((b, h + 2 * pad, w + 2 * pad, c), dev, 1212)
        out = ops.fold_f32(dp, pad)
        want, s = _fold_ref(dp.double().cpu(), pad)
        _close("fold_f32", "fp32", out.double().cpu(), want, s)


def test_grid_stride_act_bwd_f32(dev):
    with _mode("fp32") as ops:
        n = GRID_ITEMS + 333
        _second_trip(n)
        g = _randn((n,), dev, 1213)
        y = torch.tanh(_randn((n,), dev, 1214))
        out = ops.act_bwd_f32(g, y, ops.ACT_TANH)
        g64 = g.double().cpu()
        _close("act_bwd_f32", "fp32", out.double().cpu(), g64 * _dact(ops, y.double().cpu(), ops.ACT_TANH), g64.abs())
