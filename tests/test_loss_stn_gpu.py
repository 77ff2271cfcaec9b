"""GPU: every kernel of csrc/loss_stn.hip -- the spatial transformer (warp forward, float-atomic and fixed-point backward), the
smoothness loss, L1 / masked L1, the global average pool, the fused LSGAN / BCE loss, sum_scalars, act_bwd_sum, weight_pack /
weight_pack_multi and the multi-tensor Adam -- per element against a plain float64 reference of the same operation on the CPU, at
the smallest shapes where they can still go wrong (2 x 2 images, odd sizes, one element, chunk and launch-list edges), at the
second trip of every grid-stride loop (ew_blocks caps at 4096 blocks: 1 048 576 items a trip), and at the planted edges the random
inputs never hit.

References.  The warp is compared with tests/stn_ref.py (float32 coordinates, float64 after them: test_stn_ref.py shows why not
torch in float64); the losses with the torch expressions of the reference program in float64 and their autograd gradients; the
packers with torch indexing; Adam with torch's update order in float64.  A reference sees what the kernel reads: the fp32 tensors
AND the fp32 scalars of the C ABI (loss weights, targets, lr, betas, eps are rounded to float32 first -- float32(0.999) is a
1.3e-8 perturbation of the hyper-parameter, not an error of the kernel).

Bounds.  u = 2^-24 (one fp32 rounding), r = 2^-22 (a few of them, the project's fp32 constant).  S = the sum of the |terms| that
went into an element, k = the number of contributions scattered to a destination.
  exact      packers, padding and sentinel regions, sum_scalars, the device Adam state and the device-state steps, zero gradients
             (a masked-out or overwritten pixel, gout = 0): bit-identical.
  r(|want| + S)   warp forward, d_flow, the smoothness gradient, per element.  (r |want| where there is one term: L1 / LSGAN / pool
             gradients, and r |g| for act_bwd_sum's out, |act'| <= 1.)
  (k + 3) u (|want| + S)   float-atomic d_src: three roundings in a term, k additions in arbitrary order.
  k q / 2 + r S + u |want|   fixed-point d_src: q = 2^(e - 38) the fixed-point unit, e = floor(log2 max|gout|) clamped to
             [-88, 88] as in det_scale; the rounding to integer per contribution, the float products before it, the final
             int64 -> float conversion.
  (t + 16) u sum|term|   block-partial sums (smooth_fwd, l1_fwd, avgpool, act_bwd_sum): every thread adds t =
             ceil(n / (blocks * 256)) terms in fp32, wave and block sums add at most 8 more roundings, the finalize is in double
             and rounds once more; an accumulated pre-set value counts as one more term.
  LSGAN / BCE loss   r sum|s_b term_b| + sum |s_b| max|term'| dp_b, dp_b the pooled bound above and max|term'| over
             [p - dp, p + dp] (term' is monotone, so at an end); dx against the derivative at the kernel's OWN pooled value.
             Planted constant 0.0 / 1.0 maps pool to exactly 0 / 1 (asserted), so dp = 0 there and the -100 clamp is met exactly.
  Adam       m: r(|m| b1 + |g| (1 - b1));  v: r |v_new|;  p: u |p_new| + r' |update| with update = (lr / bc1) m / denom, denom =
             sqrt(v) / sqrt(bc2) + eps, and r' = dm / |m_new| + 2.5 r: the m bound carried through the quotient, plus r / 2 (the v
             bound through the square root) + 4 u (sqrt, the division by the rounded sqrt(bc2), the addition of eps) for denom =
             1.5 r, plus 4 u = r for lr / bc1 with bc1 rounded, the quotient m / denom and the product.

Largest measured error, as a fraction of the bound above (printed by every test as "maxerr ..."; MI355X):
  warp_fwd                     0.355
  warp_bwd d_flow              0.509
  warp_bwd d_src (atomic)      0.326
  warp_bwd d_src (fixed)       0.997   (a destination with k = 1 whose one contribution rounds by almost q / 2: the bound is met
                                        by construction wherever q dominates, i.e. in the spike case)
  smooth_fwd / smooth_bwd      0.0662 / 0.51
  l1 fwd / bwd                 0.0823 / 0.248
  l1 masked fwd / bwd          0.0781 / 0.248
  avgpool_fwd / avgpool_bwd    0.0642 / 0.242
  lsgan pooled                 0.183
  lsgan loss / own pool / dx   0.104 / 0.237 / 0.74
  bce loss / own pool / dx     0.154 / 0.235 / 0.718
  act_bwd_sum out / sum        0.367 / 0.0175
  adam p / m / v               0.998 / 0.375 / 0.495   (p: the final rounding alone is u |p_new| just above a power of two)
  packers, sum_scalars, the device Adam state and the device-state steps, planted zero gradients: exact, nothing to tabulate.
The float32 coordinates of tests/stn_ref.py and the kernel's agree in every pixel of every case (one sample on another cell would
put d_flow out of bound by a neighbour difference of src): the claim above warp_coord holds on the card.

Found by this module: nothing -- every kernel and wrapper of the file met its bound as written.  What the module pins down that
was open before: the warp picks ATen's float32 cell at flows of 0 and 1e-5; both clamp ends of det_scale give finite, in-bound
gradients; the BCE mode meets torch's -100 and 1e-12 clamps exactly; the device-state Adam is bit-identical to the host-step one.
Each of these mutations of csrc/loss_stn.hip, built once on the side, makes the module fail:
floorf replaced by rintf in warp_coord's callers; the scatter's guard x1 < W tightened to x1 < W - 1 (the way that stays in
bounds); my and mx swapped in d_flow; the ab == 0 clause dropped from l1_term's dsign; the -100 clamps dropped from gan_term;
zero_f32_kernel without its grid-stride loop (the stale 7.0 shows in d_src); dev_bc[1] read for dev_bc[2] in adam_kernel; the
block base of weight_pack_multi_kernel off by one chunk.
"""
import contextlib
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from stn_ref import warp_ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
R = 2.0 ** -22
SENT = 7.0
GRID_ITEMS = 4096 * 256          # ew_blocks of loss_stn.hip: items one trip of a grid-stride loop covers


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cta_gan_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops(dev):
    from cta_gan_amd import ops as _ops
    return _ops


def f32(v):
    """A Python scalar as the C ABI receives it (float), back as a double."""
    return float(np.float32(v))


def c64(t):
    return t.detach().double().cpu()


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _randn(shape, dev, seed, scale=1.0):
    gen = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(tuple(shape), generator=gen, device=dev) * scale


def _cl(t):
    """The same values in channels-last memory (the layout Reg produces), logical shape unchanged."""
    out = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert out.stride() != t.contiguous().stride() or t.shape[1] == 1 or t.shape[2] * t.shape[3] == 1
    return out


def _trips(n):
    blocks = min(4096, max(1, (n + 255) // 256))
    return (n + blocks * 256 - 1) // (blocks * 256)


def _second_trip(items):
    assert GRID_ITEMS < items < 2 * GRID_ITEMS and items % GRID_ITEMS, items


_WORST = {}


def _note(name, frac):
    _WORST[name] = max(_WORST.get(name, 0.0), frac)
    print("maxerr %-26s %.3g of the bound" % (name, _WORST[name]))


def _close(name, got, want, bound, where=""):
    """|got - want| <= bound per element (float64 CPU tensors); a zero bound asks for the exact value."""
    got, want = got.reshape(want.shape), want
    bound = bound.expand_as(want) if torch.is_tensor(bound) else torch.full_like(want, bound)
    assert bool(torch.isfinite(got).all()), "%s %s: non-finite result" % (name, where)
    err = (got - want).abs()
    pos = bound > 0
    _note(name, float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0)
    bad = err > bound
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError("%s %s: %d of %d elements out of bound, first at %s: got %r want %r bound %.3g" % (
            name, where, int(bad.sum()), bad.numel(), i, float(got[i]), float(want[i]), float(bound[i])))


def _close_scalar(name, got, want, bound, where=""):
    _close(name, torch.tensor([float(got)], dtype=torch.float64), torch.tensor([float(want)], dtype=torch.float64),
           torch.tensor([float(bound)], dtype=torch.float64), where)


def _einval():
    return pytest.raises(RuntimeError, match="CTG_EINVAL")


# ------------------------------------------------------------------------------------------------------------------ warp
def _flows(b, h, w, dev, seed):
    """The flows of the issue, (B, 2, H, W) fp32 on the device; all finite."""
    ys = torch.arange(h, device=dev, dtype=torch.float32).view(1, h, 1).expand(b, h, w)
    xs = torch.arange(w, device=dev, dtype=torch.float32).view(1, 1, w).expand(b, h, w)
    fl = {"zero": torch.zeros((b, 2, h, w), device=dev),
          "tiny": _randn((b, 2, h, w), dev, seed, 1e-5),            # where the training starts: coordinates next to integers
          "big": _randn((b, 2, h, w), dev, seed + 1, 3.0)}
    out = _randn((b, 2, h, w), dev, seed + 2, 3.0)                   # rows and columns far outside on all four sides
    out[:, 0, 0, :], out[:, 0, -1, :], out[:, 1, :, 0], out[:, 1, :, -1] = -50.0, 50.0, -60.0, 70.0
    fl["outside"] = out
    # coordinates exactly on 0 and on s - 1 (g + f is an integer: every later operation is exact there)
    edge_y = torch.where(xs % 2 == 0, (h - 1) - ys, -ys)
    edge_x = torch.where(ys % 2 == 0, -xs, (w - 1) - xs)
    fl["edge"] = torch.stack((edge_y, edge_x), 1).contiguous()
    gen = torch.Generator(device=dev).manual_seed(seed + 3)
    fl["integer"] = torch.randint(-3, 4, (b, 2, h, w), generator=gen, device=dev).float()
    return fl


def _pileup_flow(b, h, w, dev, seed):
    """Every sample lands on the last row (k reaches H and beyond there), spread a little along x."""
    f = _randn((b, 2, h, w), dev, seed, 0.7)
    f[:, 0] = 1000.0
    return f


NEEDS = ((True, True), (True, False), (False, True))


def _check_warp(ops, src, flow, gout, ref, needs=NEEDS, forward=True, where=""):
    out_w, dsrc_w, dflow_w, k, S = ref
    if forward:
        out = ops.warp_fwd(src, flow)
        assert tuple(out.shape) == tuple(src.shape)
        _close("warp_fwd", c64(out), out_w, R * (out_w.abs() + S["out"]), where)
    for need_src, need_flow in needs:
        dsrc, dflow = ops.warp_bwd(src, flow, gout, need_src, need_flow)
        assert (dsrc is None) == (not need_src) and (dflow is None) == (not need_flow), where
        if need_src:
            _close("warp_bwd d_src (atomic)", c64(dsrc), dsrc_w, (k + 3.0) * U * (dsrc_w.abs() + S["d_src"]), where)
        if need_flow:
            assert dflow.stride() == flow.stride() and tuple(dflow.shape) == tuple(flow.shape), where
            _close("warp_bwd d_flow", c64(dflow), dflow_w, R * (dflow_w.abs() + S["d_flow"]), where)


WARP_SMALL = [(1, 2, 2), (2, 2, 3), (1, 33, 2), (2, 5, 7), (3, 37, 53)]


@pytest.mark.parametrize("shape", WARP_SMALL, ids=lambda s: "x".join(map(str, s)))
def test_warp_forward_backward_every_flow_layout_and_need(shape, ops, dev):
    b, h, w = shape
    seed = 1000 * h + 10 * w + b
    src = _randn((b, 1, h, w), dev, seed)
    gout = _randn((b, 1, h, w), dev, seed + 1)
    for name, flow in _flows(b, h, w, dev, seed + 2).items():
        ref = warp_ref(src, flow, gout)
        for layout, fl in (("contiguous", flow), ("channels-last", _cl(flow))):
            _check_warp(ops, src, fl, gout, ref, where="%s %s %s" % (shape, name, layout))


def test_warp_second_grid_stride_trip(ops, dev):
    b, h, w = 1, 1025, 1024
    _second_trip(b * h * w)
    src = _randn((b, 1, h, w), dev, 21)
    gout = _randn((b, 1, h, w), dev, 22)
    flow = _flows(b, h, w, dev, 23)["outside"]
    flow[:, :, 1:-1, 1:-1] *= 1e-5 / 3.0            # next to integers inside, far outside along the four borders
    ref = warp_ref(src, flow, gout)
    _check_warp(ops, src, flow, gout, ref, ((True, True),), where="second trip contiguous")
    _check_warp(ops, src, _cl(flow), gout, ref, ((True, True),), where="second trip channels-last")


def test_warp_backward_zero_fill_second_trip(ops, dev):
    """The zero fill before the scatter has its own grid (n / 4 + 1 items): above 4 194 304 pixels its threads take a second
    trip.  A same-sized block of 7.0 is freed just before the call, so that a d_src the fill skipped has something to show
    (best effort: nothing here depends on the allocator handing that block back)."""
    b, h, w = 4, 1025, 1024
    _second_trip(b * h * w // 4 + 1)
    src = _randn((b, 1, h, w), dev, 31)
    gout = _randn((b, 1, h, w), dev, 32)
    flow = _flows(b, h, w, dev, 33)["outside"]
    ref = warp_ref(src, flow, gout)
    junk = torch.full((b, 1, h, w), SENT, device=dev)
    torch.cuda.synchronize()
    del junk
    _check_warp(ops, src, flow, gout, ref, ((True, False),), forward=False, where="zero fill second trip")


def test_warp_refuses_a_single_row_or_column(ops, dev):
    for h, w in ((1, 5), (5, 1), (1, 1)):
        src = _randn((1, 1, h, w), dev, 1)
        flow = torch.zeros((1, 2, h, w), device=dev)
        with _einval():
            ops.warp_fwd(src, flow)
        for need in NEEDS:
            with _einval():
                ops.warp_bwd(src, flow, src, *need)
    torch.cuda.synchronize()


def test_warp_autograd_wiring(ops, dev):
    from cta_gan_amd import nets
    b, h, w = 2, 5, 7
    src, gout = _randn((b, 1, h, w), dev, 41), _randn((b, 1, h, w), dev, 42)
    flow = _cl(_flows(b, h, w, dev, 43)["big"])
    out_w, dsrc_w, dflow_w, k, S = warp_ref(src, flow, gout)
    sh, fh = src.clone().requires_grad_(True), flow.clone().requires_grad_(True)
    out = nets.warp(sh, fh)
    out.backward(gout)
    _close("warp_fwd", c64(out), out_w, R * (out_w.abs() + S["out"]), "nets.warp")
    _close("warp_bwd d_src (atomic)", c64(sh.grad), dsrc_w, (k + 3.0) * U * (dsrc_w.abs() + S["d_src"]), "nets.warp")
    _close("warp_bwd d_flow", c64(fh.grad), dflow_w, R * (dflow_w.abs() + S["d_flow"]), "nets.warp")
    # only the flow asks for a gradient (the registration step): the source gets none
    fh2 = flow.clone().requires_grad_(True)
    nets.warp(src, fh2).backward(gout)
    assert torch.equal(fh2.grad, fh.grad)


# ------------------------------------------------------------------------------------------------------------------ fixed point
@contextlib.contextmanager
def _deterministic(ops):
    prev = ops.DETERMINISTIC
    ops.DETERMINISTIC = True
    try:
        yield
    finally:
        ops.DETERMINISTIC = prev


def _det_gout(case, shape, dev, seed):
    g = _randn(shape, dev, seed)
    if case == "1e-5":
        return g * 1e-5
    if case == "one":
        return g
    if case == "spike":                      # one element 2^20 larger than the rest
        g.view(-1)[g.numel() // 3] = 2.0 ** 20
        return g
    if case == "zero":
        return torch.zeros_like(g)
    g = g / g.abs().max()                    # the largest element becomes exactly +-1
    return g * (2.0 ** -100 if case == "2^-100" else 2.0 ** 100)


DET_SHAPES = [(3, 37, 53), (1, 1025, 1024)]
DET_CASES = ["1e-5", "one", "spike", "zero", "2^-100", "2^100"]


@pytest.mark.parametrize("case", DET_CASES)
@pytest.mark.parametrize("shape", DET_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_warp_backward_fixed_point_scatter(shape, case, ops, dev):
    b, h, w = shape
    if h > 1000:
        _second_trip(b * h * w)
    src = _randn((b, 1, h, w), dev, 51)
    flow = _pileup_flow(b, h, w, dev, 52)
    gout = _det_gout(case, (b, 1, h, w), dev, 53)
    out_w, dsrc_w, dflow_w, k, S = warp_ref(src, flow, gout)
    assert float(k.max()) >= h
    gmax = float(gout.abs().max())
    if case == "zero":
        e = -88
    else:
        e = min(88, max(-88, math.floor(math.log2(gmax))))
        assert {"2^-100": e == -88 and gmax == 2.0 ** -100, "2^100": e == 88 and gmax == 2.0 ** 100}.get(case, abs(e) < 88)
    q = 2.0 ** (e - 38)
    bound = k * q / 2 + R * S["d_src"] + U * dsrc_w.abs()
    where = "%s gout %s" % (shape, case)
    _, dflow_plain = ops.warp_bwd(src, flow, gout, False, True)
    with _deterministic(ops):
        for fl in (flow, _cl(flow)):
            dsrc, dflow = ops.warp_bwd(src, fl, gout, True, True)
            dsrc2, none = ops.warp_bwd(src, fl, gout, True, False)
            assert none is None
            assert torch.equal(_bits(dsrc), _bits(dsrc2)), where + ": two runs differ"
            assert dflow.stride() == fl.stride() and torch.equal(_bits(dflow), _bits(dflow_plain)), where + ": d_flow differs"
            if case == "zero":
                assert float(dsrc.abs().max()) == 0.0 and float(dflow.abs().max()) == 0.0, where
            _close("warp_bwd d_src (fixed)", c64(dsrc), dsrc_w, bound, where)


# ------------------------------------------------------------------------------------------------------------------ smoothness
def _smooth_ref(f64, weight, gscale):
    """weight * (mean(dx^2) + mean(dy^2)), its gradient times gscale, and S of the gradient (float64 CPU)."""
    x = f64.clone().requires_grad_(True)
    dy = x[:, :, 1:, :] - x[:, :, :-1, :]
    dx = x[:, :, :, 1:] - x[:, :, :, :-1]
    loss = weight * (torch.mean(dx * dx) + torch.mean(dy * dy))
    grad, = torch.autograd.grad(loss, x)
    ax = F.pad(dx.detach().abs(), (1, 1)) * (2.0 * weight / dx.numel())
    ay = F.pad(dy.detach().abs(), (0, 0, 1, 1)) * (2.0 * weight / dy.numel())
    s = ax[..., 1:] + ax[..., :-1] + ay[:, :, 1:] + ay[:, :, :-1]
    return float(loss), grad * gscale, s * abs(gscale)


SMOOTH_SHAPES = [(1, 1, 2, 2), (2, 2, 2, 9), (2, 2, 9, 2), (1, 3, 5, 7), (2, 2, 37, 53), (1, 2, 725, 724)]


@pytest.mark.parametrize("shape", SMOOTH_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_smoothness_forward_backward(shape, ops, dev):
    n = shape[0] * shape[1] * shape[2] * shape[3]
    if n > GRID_ITEMS:
        _second_trip(n)
    f = _randn(shape, dev, 60 + shape[3], 2.5)
    for weight in (1.0, 10.0):
        gscale = torch.tensor(-1.75 if weight == 1.0 else 0.5, device=dev)
        loss_w, grad_w, s = _smooth_ref(c64(f), weight, float(gscale))
        for layout, fl in (("contiguous", f), ("channels-last", _cl(f))):
            where = "%s weight %g %s" % (shape, weight, layout)
            _close_scalar("smooth_fwd", ops.smooth_fwd(fl, weight), loss_w, (_trips(n) + 16) * U * abs(loss_w), where)
            df = ops.smooth_bwd(fl, gscale, weight)
            assert df.stride() == fl.stride(), where
            _close("smooth_bwd", c64(df), grad_w, R * (grad_w.abs() + s), where)


def test_smoothness_refuses_a_single_row_or_column(ops, dev):
    for shape in ((1, 2, 1, 5), (1, 2, 5, 1)):
        f = _randn(shape, dev, 1)
        with _einval():
            ops.smooth_fwd(f)
        with _einval():
            ops.smooth_bwd(f, torch.ones((), device=dev))
    torch.cuda.synchronize()


def test_smoothness_autograd_wiring(ops, dev):
    from cta_gan_amd import nets
    f = _cl(_randn((2, 2, 5, 7), dev, 71))
    fh = f.clone().requires_grad_(True)
    loss = nets.smoothing_loss(fh, weight=10.0)
    (3.0 * loss).backward()
    loss_w, grad_w, s = _smooth_ref(c64(f), 10.0, 3.0)
    _close_scalar("smooth_fwd", loss, loss_w, (1 + 16) * U * abs(loss_w), "nets.smoothing_loss")
    _close("smooth_bwd", c64(fh.grad), grad_w, R * (grad_w.abs() + s), "nets.smoothing_loss")


# ------------------------------------------------------------------------------------------------------------------ L1
L1_SIZES = [1, 255, 256, 257, GRID_ITEMS + 1]
M03 = np.float32(0.3)
MASK_EDGE = [float(np.nextafter(M03, np.float32(0))), float(M03), float(np.nextafter(M03, np.float32(1)))]


def _l1_inputs(n, dev, seed):
    """a, b, mask (fp32, device) with the planted edges where n has room for them, and the indices of the three mask edges."""
    a, b, m = _randn((n,), dev, seed), _randn((n,), dev, seed + 1), _randn((n,), dev, seed + 2, 0.5) + 0.3
    if n < 32:
        return a, b, m, None
    m[:16] = 1.0
    a[0] = 0.0                               # a == 0 under an open mask: overwritten with -1, gradient 0
    a[1] = -0.0
    a[2] = b[2]                              # a == b: sign(0) = 0
    b[3] = 0.0                               # b == 0: the target becomes -1
    a[4], m[4] = -1.0, 0.0                   # a == -1 with b masked out: |(-1) - (-1)| = 0, gradient 0
    a[5], b[5] = -1.0, 0.0                   # a == -1 against an overwritten target under an open mask: d = 0, sign 0
    a[6], b[6] = 0.0, 0.0
    m[7], a[7] = 0.0, 2.0                    # a * bb == 0 with a != 0
    m[8], b[8] = 0.0, -0.0
    m[9:12] = torch.tensor(MASK_EDGE, device=dev)          # below 0.3f, 0.3f, above: closed, open, open
    a[9:12], b[9:12] = 1.5, -0.5
    a[n - 1], m[n - 1] = 0.0, 1.0            # and one planted element in the last (ragged) block
    return a, b, m, (9, 10, 11)


def _l1_ref(a, b, m, weight, gscale):
    """The HdTrainer expression in float64 (the mask comparison on the float32 mask, as the reference program does it)."""
    x = c64(a).requires_grad_(True)
    b64 = c64(b)
    if m is None:
        terms = (x - b64).abs()
        loss = weight * F.l1_loss(x, b64)
    else:
        bb = m.detach().cpu().clone()
        bb[bb < 0.3] = 0
        bb[bb >= 0.3] = 1
        bb = bb.double()
        rb = b64 * bb
        rb[rb == 0] = -1
        wm = x * bb
        wm[wm == 0] = -1
        terms = (wm - rb).abs()
        loss = weight * F.l1_loss(wm, rb)
    grad, = torch.autograd.grad(loss, x)
    return float(loss), grad * gscale, float(terms.detach().sum()) * weight / x.numel()


@pytest.mark.parametrize("n", L1_SIZES)
def test_l1_and_masked_l1(n, ops, dev):
    a, b, m, edges = _l1_inputs(n, dev, 80 + n % 97)
    if edges is not None:
        bb = m.cpu().clone()
        bb[bb < 0.3] = 0
        bb[bb >= 0.3] = 1
        assert [float(bb[i]) for i in edges] == [0.0, 1.0, 1.0]
    for masked in (False, True):
        for weight in (1.0, 20.0):
            gscale = torch.tensor(1.0 if weight == 1.0 else -2.5, device=dev)
            mask = m if masked else None
            loss_w, grad_w, sabs = _l1_ref(a, b, mask, weight, float(gscale))
            where = "n %d masked %s weight %g" % (n, masked, weight)
            name = "l1 masked" if masked else "l1"
            _close_scalar(name + " fwd", ops.l1_fwd(a, b, mask, weight), loss_w, (_trips(n) + 16) * U * sabs, where)
            da = ops.l1_bwd(a, b, mask, gscale, weight)
            _close(name + " bwd", c64(da), grad_w, R * grad_w.abs(), where)
            if masked and edges is not None:
                zero = [0, 1, 2, 4, 5, 6, 7, 8]
                assert float(grad_w[zero].abs().max()) == 0.0 and float(da[zero].abs().max()) == 0.0, where
                assert float(da[3]) != 0.0, where
                assert float(da[9]) == 0.0 and float(da[10]) != 0.0 and float(da[11]) != 0.0, where


def test_l1_autograd_wiring(ops, dev):
    from cta_gan_amd import nets
    a, b, m, _ = _l1_inputs(257, dev, 90)
    shape = (1, 1, 257, 1)
    for masked in (False, True):
        ah = a.view(shape).clone().requires_grad_(True)
        if masked:
            loss = nets.masked_l1_loss(ah, b.view(shape), m.view(shape), weight=2.0)
        else:
            loss = nets.l1_loss(ah, b.view(shape), weight=2.0)
        (3.0 * loss).backward()
        loss_w, grad_w, sabs = _l1_ref(a, b, m if masked else None, 2.0, 3.0)
        name = "l1 masked" if masked else "l1"
        _close_scalar(name + " fwd", loss, loss_w, (1 + 16) * U * sabs, "nets")
        _close(name + " bwd", c64(ah.grad).view(-1), grad_w, R * grad_w.abs(), "nets")


# ------------------------------------------------------------------------------------------------------------------ pool, LSGAN, BCE
POOL_HW = [(1, 1), (7, 9), (8, 8), (5, 13), (1, 257), (30, 31)]
POOL_B = [1, 6, 257]


def _pooled_ref(x):
    x64 = c64(x).flatten(1)
    hw = x64.shape[1]
    p = x64.mean(1)
    dp = ((hw + 255) // 256 + 16) * U * x64.abs().sum(1) / hw
    return p, dp


def _gan_terms(p, t, mode):
    """term(p) and term'(p) in float64: squared error, or BCE with torch's clamps (logs at -100, EPSILON 1e-12)."""
    if mode == 0:
        return (p - t) ** 2, 2.0 * (p - t)
    term = F.binary_cross_entropy(p, t, reduction="none")
    return term, (p - t) / (p * (1.0 - p)).clamp_min(1e-12)


def _gan_targets(b, nb, t0, s0, t1, s1):
    first = torch.arange(b) < nb
    full = lambda v0, v1: torch.where(first, torch.full((b,), f32(v0), dtype=torch.float64), torch.full((b,), f32(v1), dtype=torch.float64))
    return full(t0, t1), full(s0, s1)


def _check_lsgan(ops, x, nb, t0, s0, t1, s1, mode, dev, where, exact_pool=False):
    b = x.shape[0]
    hw = x.numel() // b
    p_w, dp = _pooled_ref(x)
    loss, pooled = ops.lsgan_fwd(x, nb, t0, s0, t1, s1, mode)
    p_got = c64(pooled)
    if exact_pool:
        assert torch.equal(p_got, p_w), where
        dp = torch.zeros_like(dp)
    else:
        _close("lsgan pooled", p_got, p_w, dp, where)
    t, s = _gan_targets(b, nb, t0, s0, t1, s1)
    if mode == 0:
        want = float(F.mse_loss(p_w[:nb], t[:nb], reduction="sum") * f32(s0) + F.mse_loss(p_w[nb:], t[nb:], reduction="sum") * f32(s1))
    else:
        want = float(F.binary_cross_entropy(p_w[:nb], t[:nb], reduction="sum") * f32(s0)
                     + F.binary_cross_entropy(p_w[nb:], t[nb:], reduction="sum") * f32(s1))
    term, _ = _gan_terms(p_w, t, mode)
    clampp = (lambda v: v.clamp(0.0, 1.0)) if mode == 1 else (lambda v: v)
    slope = torch.maximum(_gan_terms(clampp(p_w - dp), t, mode)[1].abs(), _gan_terms(clampp(p_w + dp), t, mode)[1].abs())
    name = "lsgan" if mode == 0 else "bce"
    _close_scalar(name + " loss", loss, want, R * float((s * term).abs().sum()) + float((s.abs() * slope * dp).sum()), where)
    # the loss at the kernel's own pooled values: no propagated term
    term_own, slope_own = _gan_terms(p_got, t, mode)
    _close_scalar(name + " loss (own pool)", loss, float((s * term_own).sum()), R * float((s * term_own).abs().sum()), where)
    gscale = torch.tensor(-1.5, device=dev)
    dx = ops.lsgan_bwd(pooled, tuple(x.shape), nb, t0, s0, t1, s1, gscale, mode)
    assert tuple(dx.shape) == tuple(x.shape)
    dx_w = (-1.5 / hw * s * slope_own).view(b, 1).expand(b, hw)
    _close(name + " dx", c64(dx).view(b, hw), dx_w, R * dx_w.abs(), where)


@pytest.mark.parametrize("b", POOL_B)
def test_avgpool_lsgan_bce(b, ops, dev):
    for h, w in POOL_HW:
        hw = h * w
        x = _randn((b, 1, h, w), dev, 100 + hw + b, 1.5) + 0.25
        p_w, dp = _pooled_ref(x)
        pooled = ops.avgpool_fwd(x)
        assert tuple(pooled.shape) == (b, 1)
        _close("avgpool_fwd", c64(pooled).view(-1), p_w, dp, "B %d HW %d" % (b, hw))
        g = _randn((b, 1), dev, 101 + hw)
        dx = ops.avgpool_bwd(g, tuple(x.shape))
        dx_w = (c64(g) / hw).expand(b, hw)
        _close("avgpool_bwd", c64(dx).view(b, hw), dx_w, R * dx_w.abs(), "B %d HW %d" % (b, hw))
        sig = torch.sigmoid(x)
        for nb in sorted({0, 1, b - 1, b}):
            where = "B %d HW %d nb %d" % (b, hw, nb)
            _check_lsgan(ops, x, nb, 1.0, 0.7 / max(nb, 1), 0.0, 1.3 / max(b - nb, 1), 0, dev, where)
            _check_lsgan(ops, sig, nb, 1.0, 0.7 / max(nb, 1), 0.0, 1.3 / max(b - nb, 1), 1, dev, where)
        _check_lsgan(ops, sig, b // 2, 0.9, 0.5, 0.1, 0.25, 1, dev, "B %d HW %d smoothed labels" % (b, hw))


@pytest.mark.parametrize("const", [0.0, 1.0])
def test_bce_on_saturated_maps_meets_torchs_clamps(const, ops, dev):
    """A map of constant 0.0 or 1.0 pools to exactly 0 or 1: log(0) is clamped at -100 (the loss is 100 s where the target is
    the other end, 0 where it is this one) and the gradient is (p - t) / 1e-12."""
    for b, (h, w) in ((1, (1, 1)), (6, (30, 31)), (257, (5, 13))):
        x = torch.full((b, 1, h, w), const, device=dev)
        for nb in sorted({0, 1, b - 1, b}):
            _check_lsgan(ops, x, nb, 1.0, 0.7, 0.0, 1.3, 1, dev, "const %g B %d HW %d nb %d" % (const, b, h * w, nb), exact_pool=True)
        loss, pooled = ops.lsgan_fwd(x, b, 1.0 - const, 0.5, 0.0, 0.0, 1)
        assert float(loss) == float(np.float32(100.0 * 0.5 * b)), (const, b, float(loss))
        dx = ops.lsgan_bwd(pooled, tuple(x.shape), b, 1.0 - const, 0.5, 0.0, 0.0, torch.ones((), device=dev), 1)
        want = (2.0 * const - 1.0) / 1e-12 * 0.5 / (h * w)
        assert abs(float(dx.flatten()[-1]) - want) <= R * abs(want)


def test_lsgan_refuses_bad_arguments(ops, dev):
    x = _randn((3, 1, 4, 4), dev, 1)
    pooled = torch.zeros(3, device=dev)
    g = torch.ones((), device=dev)
    for nb, mode in ((4, 0), (-1, 0), (1, 2), (1, -1)):
        with _einval():
            ops.lsgan_fwd(x, nb, 1.0, 1.0, 0.0, 1.0, mode)
        with _einval():
            ops.lsgan_bwd(pooled, (3, 1, 4, 4), nb, 1.0, 1.0, 0.0, 1.0, g, mode)
    torch.cuda.synchronize()


@pytest.mark.parametrize("bce", [False, True])
def test_lsgan_autograd_wiring(bce, ops, dev):
    from cta_gan_amd import nets
    b, h, w = 6, 5, 13
    x = _randn((b, 1, h, w), dev, 120)
    x = torch.sigmoid(x) if bce else x
    name = "bce" if bce else "lsgan"
    for pair in (False, True):
        xh = x.clone().requires_grad_(True)
        loss = nets.lsgan_loss_pair(xh, 2, 0.0, 1.0, weight=0.5, bce=bce) if pair else nets.lsgan_loss(xh, 1.0, weight=5.4, bce=bce)
        (2.0 * loss).backward()
        # the reference at the pooled values the kernel itself works from (avgpool_fwd launches the same pooling kernel)
        p_got = c64(ops.avgpool_fwd(x)).view(-1)
        t = torch.where(torch.arange(b) < 2, 0.0, 1.0).double() if pair else torch.ones(b, dtype=torch.float64)
        s = torch.where(torch.arange(b) < 2, f32(0.5 / 2), f32(0.5 / 4)).double() if pair else torch.full((b,), f32(5.4 / b), dtype=torch.float64)
        term, slope = _gan_terms(p_got, t, int(bce))
        _close_scalar(name + " loss (own pool)", loss, float((s * term).sum()), R * float((s * term).abs().sum()), "nets pair %s" % pair)
        dx_w = (2.0 / (h * w) * s * slope).view(b, 1, 1, 1).expand(b, 1, h, w)
        _close(name + " dx", c64(xh.grad), dx_w, R * dx_w.abs(), "nets pair %s" % pair)
        # and against the stock torch expression end to end (F.mse_loss / F.binary_cross_entropy of the pooled map)
        xr = c64(x).requires_grad_(True)
        pr = F.avg_pool2d(xr, (h, w)).view(b, 1)
        crit = F.binary_cross_entropy if bce else F.mse_loss
        if pair:
            want = 0.5 * (crit(pr[:2], torch.zeros_like(pr[:2])) + crit(pr[2:], torch.ones_like(pr[2:])))
        else:
            want = 5.4 * crit(pr, torch.ones_like(pr))
        p_w, dp = _pooled_ref(x)
        lo, hi = _gan_terms(p_w - dp, t, int(bce))[1].abs(), _gan_terms(p_w + dp, t, int(bce))[1].abs()
        bound = (R + U) * float((s * term).abs().sum()) + float((s * torch.maximum(lo, hi) * dp).sum())   # (U: s = float32(weight / n))
        _close_scalar(name + " loss", loss, float(want), bound, "nets pair %s" % pair)


# ------------------------------------------------------------------------------------------------------------------ small sums
def test_sum_scalars_is_the_left_to_right_fp32_sum(ops, dev):
    from cta_gan_amd import _lib
    vals = _randn((9,), dev, 130) * torch.logspace(-4, 4, 9, device=dev)
    host = vals.cpu().numpy()
    for n in (1, 2, 8):
        got = ops.sum_scalars([vals[i] for i in range(n)])
        want = np.float32(0.0)
        for i in range(n):
            want = np.float32(want + host[i])
        assert np.float32(got.item()).view(np.int32) == want.view(np.int32), (n, float(got), float(want))
    out = torch.full((), SENT, device=dev)
    with pytest.raises((AssertionError, RuntimeError)):
        ops.sum_scalars([vals[i] for i in range(9)])
    import ctypes
    ptrs = (ctypes.c_void_p * 9)(*[vals[i].data_ptr() for i in range(9)])
    for n in (9, 0):
        with _einval():
            _lib.check(_lib.load().ctg_sum_scalars(n, ptrs, out.data_ptr(), ops._stream()), "ctg_sum_scalars")
    torch.cuda.synchronize()
    assert float(out) == SENT


def _dact(ops, y, act):
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
    fn = {ops.ACT_RELU: F.relu, ops.ACT_LRELU: lambda v: F.leaky_relu(v, 0.2), ops.ACT_TANH: torch.tanh, ops.ACT_SIGMOID: torch.sigmoid}
    return fn[act](pre) if act in fn else pre


@pytest.mark.parametrize("n", [1, 257, GRID_ITEMS + 1])
def test_act_bwd_sum_every_activation(n, ops, dev):
    for act in (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_LRELU, ops.ACT_TANH, ops.ACT_SIGMOID):
        g = _randn((n,), dev, 140 + act)
        y = _act_out(ops, _randn((n,), dev, 150 + act), act)
        g64 = c64(g)
        want = g64 * _dact(ops, c64(y), act)
        for pre, acc in ((SENT, False), (-3.25, True)):
            db = torch.full((1,), pre, device=dev)
            out = ops.act_bwd_sum_f32(g, y, act, db, accumulate=acc)
            where = "act %d n %d accumulate %s" % (act, n, acc)
            _close("act_bwd_sum out", c64(out), want, R * g64.abs(), where)
            total = float(want.sum()) + (pre if acc else 0.0)
            sabs = float(want.abs().sum()) + (abs(pre) if acc else 0.0)
            _close_scalar("act_bwd_sum sum", db, total, (_trips(n) + 16) * U * sabs, where)


# ------------------------------------------------------------------------------------------------------------------ weight pack
def _pack_job(dev, dtype, seed, ntaps, nreal, kreal, npad, kpad, transposed=False, guard=True):
    """(master, out, ntaps, nreal, kreal, npad, kpad, sn, sk, stp) for a conv weight (Cout, Cin, taps) or -- transposed -- a
    transposed-conv weight (Cin, Cout, taps) whose sn and sk swap roles; out lies between SENT guards."""
    master = _randn((max(1, nreal * kreal * ntaps),), dev, seed) * 10.0 ** ((seed % 7) - 3)
    sn, sk = (ntaps, nreal * ntaps) if transposed else (kreal * ntaps, ntaps)
    total = ntaps * npad * kpad
    big = torch.full((total + 64,), SENT, dtype=dtype, device=dev)
    out = big[32:32 + total].view(ntaps, npad, kpad)
    return (master, out, ntaps, nreal, kreal, npad, kpad, sn, sk, 1), big


def _pack_ref(job):
    master, out, ntaps, nreal, kreal, npad, kpad, sn, sk, stp = job
    ref = torch.zeros((ntaps, npad, kpad), dtype=torch.float32, device=master.device)
    if nreal and kreal:
        t = torch.arange(ntaps, device=master.device).view(-1, 1, 1)
        n = torch.arange(nreal, device=master.device).view(1, -1, 1)
        k = torch.arange(kreal, device=master.device).view(1, 1, -1)
        ref[:, :nreal, :kreal] = master[n * sn + k * sk + t * stp]
    return ref.to(out.dtype)


# (ntaps, nreal, kreal, npad, kpad, transposed): padding in both directions, nreal == 0, totals of 2047 / 2048 / 2049 elements
PACK_SPECS = [(9, 5, 3, 8, 8, False), (9, 5, 3, 8, 8, True), (1, 0, 4, 4, 8, False), (4, 3, 0, 3, 8, False), (1, 23, 89, 23, 89, False),
              (2, 30, 32, 32, 32, True), (3, 1, 680, 1, 683, False), (1, 1, 1, 1, 1, False), (49, 2, 1, 8, 8, False), (16, 40, 17, 48, 24, True)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_weight_pack_single(dtype, ops, dev):
    assert {s[0] * s[3] * s[4] for s in PACK_SPECS} >= {2047, 2048, 2049}
    for i, spec in enumerate(PACK_SPECS + [(9, 350, 349, 352, 352, False)]):
        job, _ = _pack_job(dev, dtype, 160 + i, *spec)
        if i == len(PACK_SPECS):
            _second_trip(spec[0] * spec[3] * spec[4])
        out = ops.weight_pack(job[0], dtype, *job[2:])
        ref = _pack_ref(job)
        assert torch.equal(_bits(out), _bits(ref)), spec
        assert float(out[:, spec[1]:].float().abs().max() if spec[1] < spec[3] else 0.0) == 0.0
        assert float(out[:, :, spec[2]:].float().abs().max() if spec[2] < spec[4] else 0.0) == 0.0
    master = _randn((64,), dev, 1)
    for nreal, kreal, npad, kpad, ntaps in ((5, 2, 4, 2, 1), (2, 5, 2, 4, 1), (2, 2, 2, 2, 0)):
        with _einval():
            ops.weight_pack(master, dtype, ntaps, nreal, kreal, npad, kpad, kreal, 1, 1)
    torch.cuda.synchronize()


@pytest.mark.parametrize("count", [1, 24, 25, 49])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_weight_pack_multi_lists_and_chunk_edges(dtype, count, ops, dev):
    """One launch per 24 jobs, 2048 elements per block: jobs of one element, of exactly one / just over one / several blocks, and
    empty masters, in an order that changes from launch to launch; every destination between guards."""
    jobs, guards = [], []
    for j in range(count):
        spec = PACK_SPECS[(j * 7 + j // 10 + count) % len(PACK_SPECS)]
        job, big = _pack_job(dev, dtype, 200 + 3 * j + count, *spec)
        jobs.append(job)
        guards.append(big)
    ops.weight_pack_multi(jobs)
    for j, (job, big) in enumerate(zip(jobs, guards)):
        assert torch.equal(_bits(job[1]), _bits(_pack_ref(job))), ("job %d of %d" % (j, count), job[2:])
        assert bool((big[:32] == SENT).all()) and bool((big[-32:] == SENT).all()), ("guards of job %d" % j, job[2:])
    bad, _ = _pack_job(dev, dtype, 5, 1, 5, 2, 4, 2)
    with _einval():
        ops.weight_pack_multi(jobs[:1] + [bad])
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ Adam
LR, B1, B2, EPS = 1e-4, 0.5, 0.999, 1e-8


def _guarded(values):
    big = torch.full((values.numel() + 16,), SENT, device=values.device)
    big[8:8 + values.numel()] = values
    return big[8:8 + values.numel()], big


def _adam_state(sizes, dev, seed, fresh=False):
    """p, g, m, v lists (device fp32; p, m, v between guards): gradients spanning 1e-6 .. 1e3, and planted g == 0 with v == 0."""
    ps, gs, ms, vs, bigs = [], [], [], [], []
    for j, n in enumerate(sizes):
        expo = torch.rand(n, generator=torch.Generator().manual_seed(seed + j)).to(dev) * 9.0 - 6.0
        g = _randn((n,), dev, seed + 100 + j) * 10.0 ** expo
        m = _randn((n,), dev, seed + 200 + j) * 10.0 ** expo
        v = (_randn((n,), dev, seed + 300 + j) * 10.0 ** expo) ** 2
        if fresh:
            m, v = torch.zeros_like(m), torch.zeros_like(v)
        g[0], v[0] = 0.0, 0.0                                    # the denominator is eps; the moment alone moves p
        if n > 2:
            g[n - 1], v[n - 1], m[n - 1] = 0.0, 0.0, 0.0         # nothing moves
        p, bp = _guarded(_randn((n,), dev, seed + 400 + j))
        m, bm = _guarded(m)
        v, bv = _guarded(v)
        ps.append(p); gs.append(g); ms.append(m); vs.append(v); bigs += [bp, bm, bv]
    return ps, gs, ms, vs, bigs


def _adam_ref(p, g, m, v, lr, b1, b2, eps, step):
    """torch.optim.Adam's update order in float64 and the bounds of the module docstring."""
    lr, b1, b2, eps = f32(lr), f32(b1), f32(b2), f32(eps)
    m_new = m + (g - m) * (1.0 - b1)
    v_new = v * b2 + (1.0 - b2) * g * g
    bc1, bc2s = 1.0 - b1 ** step, math.sqrt(1.0 - b2 ** step)
    denom = v_new.sqrt() / bc2s + eps
    upd = (lr / bc1) * m_new / denom
    p_new = p - upd
    dm = R * (m.abs() * b1 + g.abs() * (1.0 - b1))
    dv = R * v_new
    dp = U * p_new.abs() + (lr / bc1) * dm / denom + 2.5 * R * upd.abs()
    return (p_new, dp), (m_new, dm), (v_new, dv)


def _check_adam(ops, sizes, dev, seed, step, b1=B1, b2=B2, fresh=False):
    ps, gs, ms, vs, bigs = _adam_state(sizes, dev, seed, fresh)
    before = [(c64(p), c64(g), c64(m), c64(v)) for p, g, m, v in zip(ps, gs, ms, vs)]
    ops.adam_step(ps, gs, ms, vs, LR, b1, b2, EPS, step)
    for j, (p, m, v) in enumerate(zip(ps, ms, vs)):
        where = "tensor %d of %d (n %d) step %d" % (j, len(sizes), sizes[j], step)
        for name, got, (want, bound) in zip(("adam p", "adam m", "adam v"), (p, m, v), _adam_ref(*before[j], LR, b1, b2, EPS, step)):
            _close(name, c64(got), want, bound, where)
        n = sizes[j]
        if n > 2:
            assert float(p[n - 1]) == float(before[j][0][n - 1]) and float(m[n - 1]) == 0.0 and float(v[n - 1]) == 0.0, where
    for big in bigs:
        assert bool((big[:8] == SENT).all()) and bool((big[-8:] == SENT).all()), "an Adam launch wrote outside a tensor"


ADAM_SIZES = [1, 255, 4095, 4096, 4097, 8193]


@pytest.mark.parametrize("step", [1, 2, 3, 1000])
def test_adam_chunk_edges_and_steps(step, ops, dev):
    _check_adam(ops, ADAM_SIZES, dev, 500 + step, step)
    _check_adam(ops, ADAM_SIZES[::-1], dev, 600 + step, step, fresh=True)
    if step == 2:
        _check_adam(ops, ADAM_SIZES, dev, 700, step, b1=0.9, b2=0.99)


@pytest.mark.parametrize("count", [1, 24, 25, 49])
def test_adam_tensor_lists(count, ops, dev):
    """24 tensors a launch: the 25th and the 49th open another.  In the second list one tensor is far longer than the rest, so
    most blocks of the short ones leave at once."""
    _check_adam(ops, [1 + (j * 977 + count) % 5000 for j in range(count)], dev, 800 + count, 2)
    sizes = [1 + (j * 31) % 97 for j in range(count)]
    sizes[count // 2] = 300001
    _check_adam(ops, sizes, dev, 900 + count, 3)


def test_adam_device_state(ops, dev):
    b1, b2 = f32(B1), f32(B2)
    state = torch.zeros(3, device=dev)
    for k in range(1, 12):
        ops.adam_tick(state, B1, B2)
        want = np.array([k, 1.0 - b1 ** k, math.sqrt(1.0 - b2 ** k)], dtype=np.float64).astype(np.float32)
        assert np.array_equal(state.cpu().numpy().view(np.int32), want.view(np.int32)), (k, state.cpu().numpy(), want)
    # three steps by the device state == three steps by the host's step number, bit for bit
    sizes = [1, 4097, 255] + [33] * 23
    host = _adam_state(sizes, dev, 1000)
    devs = _adam_state(sizes, dev, 1000)
    state = torch.zeros(3, device=dev)
    for step in (1, 2, 3):
        for gh, gd in zip(host[1], devs[1]):
            gh.mul_(0.5 + step)
            gd.mul_(0.5 + step)
        ops.adam_step(*host[:4], LR, B1, B2, EPS, step)
        ops.adam_tick(state, B1, B2)
        ops.adam_step(*devs[:4], LR, B1, B2, EPS, 0, dev_state=state)
        for j in range(len(sizes)):
            for which in (0, 2, 3):
                assert torch.equal(_bits(host[which][j]), _bits(devs[which][j])), ("step %d tensor %d list %d" % (step, j, which))
    with _einval():
        ops.adam_step(*host[:4], LR, B1, B2, EPS, 0)
    with _einval():
        ops.adam_step(*host[:4], LR, B1, B2, EPS, -1)
    torch.cuda.synchronize()


def test_adam_optimizer_turns_capturable_at_step_three(ops, dev):
    from cta_gan_amd import optim
    shapes = [(5, 3), (4097,), (1,)] + [(7,)] * 24
    make = lambda: [torch.nn.Parameter(_randn(s, dev, 1100 + i)) for i, s in enumerate(shapes)]
    pa, pb = make(), make()
    oa = optim.Adam(pa, lr=LR, betas=(B1, B2))
    ob = optim.Adam(pb, lr=LR, betas=(B1, B2))
    for step in (1, 2, 3, 4):
        if step == 3:
            ob.capturable = True
        for i, (a, b) in enumerate(zip(pa, pb)):
            a.grad = _randn(a.shape, dev, 1200 + 50 * step + i, 10.0 ** (step - 2))
            b.grad = a.grad.clone()
        oa.step()
        ob.step()
        if step >= 3:
            assert float(ob._dev_state[0][0]) == float(step)
        for i, (a, b) in enumerate(zip(pa, pb)):
            assert torch.equal(_bits(a.detach()), _bits(b.detach())), ("step %d parameter %d" % (step, i))
            assert ob.state[b]["step"] == step
            assert torch.equal(_bits(oa.state[a]["exp_avg_sq"]), _bits(ob.state[b]["exp_avg_sq"]))
    # and the eager optimiser itself is the reference update: one more step of a fresh pair against float64
    p = torch.nn.Parameter(_randn((4097,), dev, 1300))
    p0 = c64(p)
    p.grad = _randn((4097,), dev, 1301)
    optim.Adam([p], lr=LR, betas=(B1, B2)).step()
    zero = torch.zeros_like(p0)
    (p_w, dp), _, _ = _adam_ref(p0, c64(p.grad), zero, zero, LR, B1, B2, EPS, 1)
    _close("adam p", c64(p), p_w, dp, "optim.Adam first step")
