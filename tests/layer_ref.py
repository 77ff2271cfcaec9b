"""Plain float64 reference of a conv LAYER as the networks use it -- padding, convolution, bias, activation, and the
gradients of all three operands by autograd -- and the case table of tests/test_layer_glue_exact_gpu.py.

The kernels are held by tests/test_conv_exact_gpu.py and its siblings, from tap lists the tests write themselves.  What is held
here is the code that WRITES the tap lists: engine.conv_forward, engine._conv_backward, _bwd_data_launch, add_grad and take_grad.
So the reference knows nothing of taps, packs, channel pads or padded grids: it is F.pad(mode="reflect"), F.conv2d,
F.conv_transpose2d(stride=2, padding=pad, output_padding=1) and the activation on float64 CPU tensors, differentiated by torch.

Operands are drawn on the integer grids of tests/conv_ref.py (x and w small integers, biases multiples of 1/8, output gradients
sparse in {-1, 0, 1}).  `check_case` asserts, on the reference alone, the conditions under which the engine has to reproduce the
reference bit for bit (module docstring of tests/test_layer_glue_exact_gpu.py); tests/test_layer_ref.py runs it for every case on
a machine without a GPU.

Tolerance cases (Tanh, Sigmoid, LeakyReLU) keep x on the integer grid and scale the sparse integer weights by a power of two, so
that the pre-activations are O(1) -- the activation is neither saturated nor linear -- while every operand is still a bf16 value:
what is left is the error of the activation, of its derivative and of the bf16 stores behind them.
"""
from dataclasses import dataclass, field
from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

import conv_ref as R

ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH, ACT_SIGMOID = 0, 1, 2, 3, 4
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


# ---------------------------------------------------------------------------- the table's records
@dataclass(frozen=True)
class Conv:
    """The fields of engine.ConvSpec as plain data (tests/test_layer_ref.py checks that the two agree field by field)."""
    cin: int
    cout: int
    k: int
    stride: int = 1
    pad: int = 0
    reflect: bool = False
    transposed: bool = False
    use_bias: bool = True
    act: int = ACT_NONE
    out_f32: bool = False


@dataclass(frozen=True)
class Case:
    """One layer (or, for the fan-out cases, two or three layers reading one activation) at one input size.

    owed       (x, weight, bias): which gradients are asked for; one not owed must come back as None
    exact      bitwise against the reference, or at TOL / GTOL of tests/test_kernels_gpu.py
    w_lo/w_hi, w_keep, w_shift: weights = integers of [w_lo, w_hi], kept with probability w_keep, times 2^-w_shift
    g_keep     density of the output gradient
    calls      {"fp32" | "bf16": {label: count}}: every launch the engine makes for the case (labels: `call_label`)
    order      {"fp32" | "bf16": [label, ...]}: the grad_combine launches in the order they must be made (fan-out cases)
    preds      {"fp32" | "bf16": set of predicate names that hold} (`predicates`); every other predicate must be False
    wgrad_g    bf16 only: (channels, pixel pitch) of the gradient operand handed to conv_wgrad
    paths      the numbers of the previously unreached paths (module docstring of the GPU test) the case is there for
    """
    name: str
    family: str
    convs: Tuple[Conv, ...]
    shape: Tuple[int, int, int, int]
    calls: Dict[str, Dict[str, int]]
    owed: Tuple[bool, bool, bool] = (True, True, True)
    exact: bool = True
    w_lo: int = -2
    w_hi: int = 2
    w_keep: float = 1.0
    w_shift: int = 0
    g_keep: float = 0.25
    order: Optional[Dict[str, Tuple[str, ...]]] = None
    preds: Dict[str, frozenset] = field(default_factory=lambda: {"fp32": frozenset(), "bf16": frozenset()})
    wgrad_g: Optional[Tuple[int, int]] = None
    paths: Tuple[int, ...] = ()


# ---------------------------------------------------------------------------- operands
def _seed(name):
    return int(np.frombuffer(name.encode(), dtype=np.uint8).astype(np.uint64).sum() * 7919 + len(name))


def out_hw(c: Conv, h, w):
    if c.transposed:
        return 2 * h, 2 * w
    return (h + 2 * c.pad - c.k) // c.stride + 1, (w + 2 * c.pad - c.k) // c.stride + 1


def operands(case: Case):
    """float64 CPU operands: x (B, C, H, W) in [-2, 2]; per conv w (torch layout: (Cout, Cin, k, k), transposed (Cin, Cout, k, k)),
    b (Cout,) and the output gradient g (B, Cout, Ho, Wo)."""
    rng = np.random.default_rng(_seed(case.name))
    b, c, h, w = case.shape
    x = R.int_grid(rng, (b, c, h, w), -2, 2)
    ws, bs, gs = [], [], []
    for cv in case.convs:
        wshape = (cv.cin, cv.cout, cv.k, cv.k) if cv.transposed else (cv.cout, cv.cin, cv.k, cv.k)
        wt = R.int_grid(rng, wshape, case.w_lo, case.w_hi)
        if case.w_keep < 1.0:
            wt = wt * torch.from_numpy((rng.random(wshape) < case.w_keep).astype(np.float64))
        ws.append(wt * 2.0 ** -case.w_shift)
        bs.append(R.bias_grid(rng, cv.cout))
        ho, wo = out_hw(cv, h, w)
        g = R.int_grid(rng, (b, cv.cout, ho, wo), 0, 1) * 2 - 1
        gs.append(g * torch.from_numpy((rng.random((b, cv.cout, ho, wo)) < case.g_keep).astype(np.float64)))
    return x, ws, bs, gs


# ---------------------------------------------------------------------------- the reference
def act_f64(v, act):
    if act == ACT_RELU:
        return F.relu(v)
    if act == ACT_LRELU:
        return F.leaky_relu(v, 0.2)
    if act == ACT_TANH:
        return torch.tanh(v)
    if act == ACT_SIGMOID:
        return torch.sigmoid(v)
    assert act == ACT_NONE
    return v


def layer(cv: Conv, x, w, b):
    """(y, xp): the layer on a (B, C, H, W) tensor of any float dtype, and the reflection-padded input (None without one) whose
    gradient is what the engine keeps on its padded grid."""
    bias = b if cv.use_bias else None
    if cv.transposed:
        assert cv.stride == 2
        return act_f64(F.conv_transpose2d(x, w, bias, stride=2, padding=cv.pad, output_padding=1), cv.act), None
    if cv.reflect:
        xp = F.pad(x, (cv.pad,) * 4, mode="reflect")
        return act_f64(F.conv2d(xp, w, bias, stride=cv.stride), cv.act), xp
    return act_f64(F.conv2d(x, w, bias, stride=cv.stride, padding=cv.pad), cv.act), None


@dataclass
class RefResult:
    y: list          # per conv (B, Cout, Ho, Wo)
    pre: list        # per conv: the pre-activation
    dx: torch.Tensor    # (B, C, H, W): the SUM over the convs
    dx_each: list    # per conv
    dxp: list        # per conv: gradient on the reflection-padded grid, or None
    dw: list
    db: list         # None where the bias is dead


def reference(case: Case, ops_=None, dtype=torch.float64):
    """The layer(s) of `case` forward and backward in `dtype` on the CPU.  ops_ = operands(case), or operands of one's own."""
    x, ws, bs, gs = ops_ if ops_ is not None else operands(case)
    x = x.to(dtype)
    ys, pres, dxe, dxps, dws, dbs = [], [], [], [], [], []
    for cv, w, b, g in zip(case.convs, ws, bs, gs):
        xl = x.clone().requires_grad_(True)
        wl, bl = w.to(dtype).clone().requires_grad_(True), b.to(dtype).clone().requires_grad_(True)
        lin = Conv(**{**cv.__dict__, "act": ACT_NONE})
        pre, xp = layer(lin, xl, wl, bl)
        if xp is not None:
            xp.retain_grad()
        y = act_f64(pre, cv.act)
        y.backward(g.to(dtype))
        ys.append(y.detach())
        pres.append(pre.detach())
        dxe.append(xl.grad)
        dxps.append(None if xp is None else xp.grad)
        dws.append(wl.grad)
        dbs.append(bl.grad if cv.use_bias else None)
    return RefResult(ys, pres, sum(dxe[1:], dxe[0].clone()), dxe, dxps, dws, dbs)


def magnitudes(case: Case, ops_=None):
    """S of every accumulator -- the sum of the magnitudes of its terms -- as the linear part of the layer run on abs() operands
    with abs() gradients (an activation derivative has magnitude <= 1): a RefResult whose tensors bound the sums."""
    x, ws, bs, gs = ops_ if ops_ is not None else operands(case)
    lin = Case(**{**case.__dict__, "convs": tuple(Conv(**{**c.__dict__, "act": ACT_NONE}) for c in case.convs)})
    return reference(lin, (x.abs(), [w.abs() for w in ws], [b.abs() for b in bs], [g.abs() for g in gs]))


def _is_int_le(t, bound):
    return bool((t == t.round()).all()) and float(t.abs().max()) <= bound


def check_case(case: Case):
    """The conditions of the exactness argument, on the reference alone.  Returns a small report (for printing)."""
    ops_ = operands(case)
    ref = reference(case, ops_)
    rep = {}
    # 6. no expected gradient is identically zero (and none is missing)
    for i, cv in enumerate(case.convs):
        assert float(ref.dw[i].abs().max()) > 0 and float(ref.dx_each[i].abs().max()) > 0, (case.name, "zero gradient")
        if cv.use_bias:
            assert float(ref.db[i].abs().max()) > 0, (case.name, "zero bias gradient")
        # 5. an activation with a mask has it on and off on at least 10 % of the elements each
        if cv.act in (ACT_RELU, ACT_LRELU):
            on = float((ref.pre[i] > 0).double().mean())
            rep["mask_on"] = on
            assert 0.1 <= on <= 0.9, (case.name, "mask on %.3f" % on)
        if cv.act in (ACT_TANH, ACT_SIGMOID):
            d = 1 - ref.y[i] ** 2 if cv.act == ACT_TANH else ref.y[i] * (1 - ref.y[i])
            live = float((d > 0.05 * float(d.max())).double().mean())      # neither saturated everywhere ...
            rep["act_live"] = live
            assert live >= 0.25 and float(ref.pre[i].abs().max()) > 1.0, (case.name, live)      # ... nor linear
    if not case.exact:
        return rep
    # 1. every accumulator stays below 2^24 granules: fp32 sums are exact in any order
    mag = magnitudes(case, ops_)
    gran = 2.0 ** -(3 + case.w_shift)      # biases are multiples of 1/8
    worst = max([R.assert_exact_domain(t, gran) for t in mag.y]
                + [R.assert_exact_domain(t, 2.0 ** -case.w_shift) for t in mag.dx_each + [mag.dx] + [t for t in mag.dxp if t is not None]]
                + [R.assert_exact_domain(t) for t in mag.dw] + [R.assert_exact_domain(t) for t in mag.db if t is not None])
    rep["S_max"] = worst
    # 2. gradients the engine keeps in bf16 (the input gradient of a wide layer, on the padded grid, folded, and accumulated over
    #    the consumers) are integers of magnitude <= 256: bf16 values, whichever of them the engine rounds
    assert case.w_shift == 0
    if case.shape[1] > 2:
        acc = None
        for i in range(len(case.convs) - 1, -1, -1):      # partial sums in the order the backward makes them
            acc = ref.dx_each[i] if acc is None else acc + ref.dx_each[i]
            for t in (ref.dx_each[i], acc, ref.dxp[i]):
                if t is not None:
                    assert _is_int_le(t, 256), (case.name, "input gradient off the bf16 integer grid", float(t.abs().max()))
        rep["dx_max"] = float(ref.dx.abs().max())
    # (the operands themselves, and the gradients after an exact activation, are bf16 values)
    for t in [ops_[0]] + ops_[1] + ops_[3]:
        assert torch.equal(t.bfloat16().double(), t)
    for cv in case.convs:
        assert cv.act in (ACT_NONE, ACT_RELU), (case.name, "only ReLU is exact")
    return rep


# ---------------------------------------------------------------------------- predicates and launch labels
def predicates(case: Case, dtype):
    """The pure-Python dispatch predicates of cta_gan_amd.ops for the (single) layer of `case`, by the role it has in the engine:
    head_* for a layer fed from image planes (Cin <= 2), tail_* for the one-channel reflect tail.  -> the set of those that hold."""
    from cta_gan_amd import ops
    cv = case.convs[0]
    _, _, h, w = case.shape
    odt = torch.float32 if cv.out_f32 else dtype
    p = {"cout1": ops.cout1_ok(cv.cin, cv.cout, cv.k, cv.stride, cv.reflect, cv.pad, cv.transposed, dtype),
         "tail7": cv.out_f32 and ops.conv_tail7_ok(cv.cin, cv.cout, cv.k, cv.stride, cv.reflect, cv.pad, dtype, h, w)}
    if cv.cin <= 2:
        p["head_smallcin"] = ops.smallcin_ok(cv.cin, cv.cout, cv.k, dtype, odt, cv.stride)
        p["head_kxw"] = ops.kxw_ok(cv.cin, cv.cout, cv.k, cv.stride, dtype)
        p["head_corr"] = ops.corr_smallcin_ok(cv.cin, cv.cout, cv.k, cv.stride, dtype)
    if cv.out_f32 and cv.cout == 1 and cv.reflect:
        p["tail_dx_small"] = ops.smallcin_ok(1, cv.cin, cv.k, dtype, dtype)
        p["tail_corr"] = ops.corr_smallcin_ok(1, cv.cin, cv.k, cv.stride, dtype)
        p["tail_kxw"] = ops.kxw_ok(1, cv.cin, cv.k, 1, dtype)
    return frozenset(k for k, v in p.items() if v)


TRACKED = ("conv_igemm", "conv_igemm_classes", "conv_smallcin", "conv_tail7", "conv_cout1_fwd", "conv_cout1_bwd",
           "conv_cout1_wgrad", "im2col_pack", "conv_wgrad", "corr_smallcin", "chan_pad", "bias_grad", "bias_grad_act",
           "grad_combine", "act_bwd_f32", "act_bwd_sum_f32", "fold_f32", "zero_act", "kxw_pack")


def call_label(name, args, kwargs, result):
    """The label a launch is counted under, or None for a call that launched nothing.
    conv_igemm: plain | :frame | :fold (folds a padded-grid frame in its epilogue) | :fold+res (and adds the waiting gradient);
    grad_combine: :act4 (activation backward on the (1, 1, n/4, 4) view) | :act | :fold (fold alone) | :add (two unpadded
    gradients) | :add+fold (one of the two on the padded grid); conv_igemm_classes: only when the library served the launch."""
    if name == "conv_igemm":
        if kwargs.get("frame"):
            return "conv_igemm:frame"
        if kwargs.get("fold") is not None:
            return "conv_igemm:fold+res" if kwargs.get("res") is not None else "conv_igemm:fold"
        assert kwargs.get("res") is None
        return name
    if name == "conv_igemm_classes":
        return name if result is not None else None
    if name == "grad_combine":
        a, b, pad, yact, act, out = args
        if yact is not None:
            assert b is None
            return "grad_combine:act4" if tuple(out.shape[:2]) == (1, 1) and out.shape[3] == 4 else "grad_combine:act"
        if a is None:
            assert pad > 0
            return "grad_combine:fold"
        return "grad_combine:add+fold" if pad else "grad_combine:add"
    return name


# ---------------------------------------------------------------------------- the case table
def _fs(*names):
    return frozenset(names)


def _both(d):
    return {"fp32": dict(d), "bf16": dict(d)}


def _tail(cout, act, **kw):
    return Conv(64, cout, 7, 1, 3, reflect=True, use_bias=True, act=act, out_f32=True, **kw)


_TAIL_PREDS_1 = {"fp32": _fs("tail7", "tail_dx_small"), "bf16": _fs("tail7", "tail_dx_small", "tail_corr", "tail_kxw")}
_NO_PREDS = {"fp32": _fs(), "bf16": _fs()}


def _tail_calls(step1):
    """Tail with 2..4 channels: forward on the gather kernel, the gradient zero-padded to 32 channels, the input gradient on the
    padded grid and folded when the network's input gradient is taken."""
    d = {"conv_igemm": 2, "chan_pad": 1, "bias_grad": 1, "conv_wgrad": 1, "grad_combine:fold": 1}
    d[step1] = 1
    return _both(d)


def _cases():
    cs = []
    # (a) multi-channel tails.  8x16: the smallest map whose weight gradient takes the [:16] channel slice (bf16); 12x20 ragged;
    # 7x16 and 8x12: the full 32-channel operand; 5x5, 3 channels, batch 1: 75 elements, the scalar activation backward
    for cout, act, shape, tag, wg, paths in (
            (2, ACT_RELU, (2, 64, 8, 16), "8x16", (16, 32), (2, 3)),
            (3, ACT_TANH, (1, 64, 8, 16), "8x16", (16, 32), (2, 3)),
            (4, ACT_RELU, (3, 64, 12, 20), "12x20", (16, 32), (2, 3)),
            (3, ACT_RELU, (2, 64, 7, 16), "7x16", (32, 32), (2, 3)),
            (2, ACT_TANH, (2, 64, 8, 12), "8x12", (32, 32), (2, 3)),
            (4, ACT_RELU, (1, 64, 8, 12), "8x12", (32, 32), (2, 3)),
            (3, ACT_RELU, (1, 64, 5, 5), "5x5", (32, 32), (1, 3)),
            (3, ACT_TANH, (1, 64, 5, 5), "5x5", (32, 32), (1, 3))):
        exact = act == ACT_RELU
        n = shape[0] * cout * shape[2] * shape[3]
        cs.append(Case("tail_64to%d_%s_%s" % (cout, "relu" if exact else "tanh", tag), "tail", (_tail(cout, act),), shape,
                       _tail_calls("act_bwd_f32" if n % 4 else "grad_combine:act4"), exact=exact,
                       w_keep=1.0 if exact else 0.25, w_shift=0 if exact else 6, w_lo=-2 if exact else -1, w_hi=2 if exact else 1,
                       preds=_NO_PREDS, wgrad_g=wg, paths=paths))
    # ... and the one-channel tail with its bias frozen: step 1 cannot take the fused activation + bias-sum pass
    cs.append(Case("tail_64to1_tanh_bias_frozen", "tail", (_tail(1, ACT_TANH),), (1, 64, 8, 16),
                   {"fp32": {"conv_tail7": 1, "grad_combine:act4": 1, "chan_pad": 1, "conv_wgrad": 1, "conv_igemm": 1,
                             "grad_combine:fold": 1},
                    "bf16": {"conv_tail7": 1, "grad_combine:act4": 1, "corr_smallcin": 1, "kxw_pack": 1, "conv_smallcin": 1,
                             "grad_combine:fold": 1}},
                   owed=(True, True, False), exact=False, w_keep=0.25, w_shift=6, w_lo=-1, w_hi=1, preds=_TAIL_PREDS_1,
                   paths=(2, 6)))
    cs.append(Case("tail_64to1_relu_bias_frozen", "tail", (_tail(1, ACT_RELU),), (2, 64, 8, 16),
                   {"fp32": {"conv_tail7": 1, "grad_combine:act4": 1, "chan_pad": 1, "conv_wgrad": 1, "conv_igemm": 1,
                             "grad_combine:fold": 1},
                    "bf16": {"conv_tail7": 1, "grad_combine:act4": 1, "corr_smallcin": 1, "kxw_pack": 1, "conv_smallcin": 1,
                             "grad_combine:fold": 1}},
                   owed=(True, True, False), preds=_TAIL_PREDS_1, paths=(2, 6)))
    # (b) the 7x7 head on two image planes: Cin k k = 98 > 64, so im2col_pack (Kpad 128) + a 1x1 gather
    for shape, tag in (((2, 2, 8, 8), "8x8"), ((1, 2, 17, 33), "17x33")):
        for use_bias in (True, False):
            for xreq in (True, False):
                d = {"im2col_pack": 1, "conv_igemm": 2 if xreq else 1, "conv_wgrad": 1}
                if use_bias:
                    d["bias_grad"] = 1
                if xreq:
                    d["fold_f32"] = 1
                cs.append(Case("head_2to64_%s_%s_%s" % (tag, "bias" if use_bias else "nobias", "dx" if xreq else "nodx"), "head",
                               (Conv(2, 64, 7, 1, 3, reflect=True, use_bias=use_bias),), shape, _both(d),
                               owed=(xreq, True, use_bias), g_keep=0.125, preds=_NO_PREDS, paths=(4,)))
    # (c) the PatchGAN's last layer with Sigmoid: vector-ALU kernels in bf16, zero-padded MFMA columns in fp32
    for shape, tag in (((2, 512, 5, 7), "5x7"), ((1, 512, 19, 19), "19x19")):
        cs.append(Case("dlast_512to1_sigmoid_%s" % tag, "dlast",
                       (Conv(512, 1, 4, 1, 1, use_bias=True, act=ACT_SIGMOID, out_f32=True),), shape,
                       {"fp32": {"conv_igemm": 2, "act_bwd_sum_f32": 1, "chan_pad": 1, "conv_wgrad": 1},
                        "bf16": {"conv_cout1_fwd": 1, "act_bwd_sum_f32": 1, "conv_cout1_wgrad": 1, "conv_cout1_bwd": 1}},
                       exact=False, w_keep=0.125, w_shift=6, w_lo=-1, w_hi=1, g_keep=0.5,
                       preds={"fp32": _fs(), "bf16": _fs("cout1")}, paths=(5,)))
    # (d) which parameter gradients are owed: a plain LeakyReLU layer and the one-channel Tanh tail
    plain = Conv(64, 64, 3, 1, 1, use_bias=True, act=ACT_LRELU)
    for owed, tag in (((True, True, True), "all"), ((True, True, False), "w_only"), ((True, False, True), "b_only"),
                      ((True, False, False), "dx_only")):
        d = {"conv_igemm": 2, ("bias_grad_act" if owed[2] else "grad_combine:act"): 1}
        if owed[1]:
            d["conv_wgrad"] = 1
        cs.append(Case("preq_plain_lrelu_%s" % tag, "preq", (plain,), (2, 64, 9, 11), _both(d), owed=owed, exact=False,
                       w_keep=0.25, w_shift=3, w_lo=-1, w_hi=1, preds=_NO_PREDS, paths=(6,) if tag != "all" else ()))
    for owed, tag in (((True, False, True), "b_only"), ((True, False, False), "dx_only")):
        f = {"conv_tail7": 1, "chan_pad": 1, "conv_igemm": 1, "grad_combine:fold": 1}
        h = {"conv_tail7": 1, "kxw_pack": 1, "conv_smallcin": 1, "grad_combine:fold": 1}
        for d in (f, h):
            d["act_bwd_sum_f32" if owed[2] else "grad_combine:act4"] = 1
        cs.append(Case("preq_tail_tanh_%s" % tag, "preq", (_tail(1, ACT_TANH),), (1, 64, 8, 16), {"fp32": f, "bf16": h},
                       owed=owed, exact=False, w_keep=0.25, w_shift=6, w_lo=-1, w_hi=1, preds=_TAIL_PREDS_1, paths=(6,)))
    # (e) one activation read by two or three convs (forward order as listed; the backward meets them in reverse).  9x11: every
    # gradient arrives on its own grid and add_grad combines them; 32x32: the reflect conv's backward-data is frame + tile-aligned
    # interior, and the interior launch takes a gradient already waiting at x as `res`
    refl, zpad, one = Conv(64, 64, 3, 1, 1, reflect=True), Conv(64, 64, 3, 1, 1), Conv(64, 64, 1, 1, 0)
    small, big = (2, 64, 9, 11), (1, 64, 32, 32)

    def fan(tag, convs, shape, extra, order, paths):
        n = len(convs)
        d = {"bias_grad": n, "conv_wgrad": n}
        d.update(extra)
        cs.append(Case("fanout_%s_%s" % (tag, "9x11" if shape is small else "32x32"), "fanout", convs, shape, _both(d),
                       g_keep=0.125, order=_both_t(order), preds=_NO_PREDS, paths=paths))

    fan("reflect_plain", (refl, zpad), small, {"conv_igemm": 4, "grad_combine:add+fold": 1}, ("grad_combine:add+fold",), ())
    fan("plain_reflect", (zpad, refl), small, {"conv_igemm": 4, "grad_combine:add+fold": 1}, ("grad_combine:add+fold",), ())
    fan("reflect_reflect", (refl, refl), small, {"conv_igemm": 4, "grad_combine:fold": 1, "grad_combine:add+fold": 1},
        ("grad_combine:fold", "grad_combine:add+fold"), (7,))
    fan("reflect_plain_1x1", (refl, zpad, one), small, {"conv_igemm": 6, "grad_combine:add": 1, "grad_combine:add+fold": 1},
        ("grad_combine:add", "grad_combine:add+fold"), (8,))
    fan("plain_1x1_reflect", (zpad, one, refl), small, {"conv_igemm": 6, "grad_combine:add": 1, "grad_combine:add+fold": 1},
        ("grad_combine:add+fold", "grad_combine:add"), (8,))
    fan("reflect_plain", (refl, zpad), big, {"conv_igemm": 3, "conv_igemm:frame": 1, "conv_igemm:fold+res": 1}, (), ())
    fan("plain_reflect", (zpad, refl), big, {"conv_igemm": 3, "conv_igemm:frame": 1, "conv_igemm:fold": 1, "grad_combine:add": 1},
        ("grad_combine:add",), ())
    fan("reflect_reflect", (refl, refl), big,
        {"conv_igemm": 2, "conv_igemm:frame": 2, "conv_igemm:fold": 1, "conv_igemm:fold+res": 1}, (), ())
    fan("reflect_plain_1x1", (refl, zpad, one), big,
        {"conv_igemm": 5, "conv_igemm:frame": 1, "conv_igemm:fold+res": 1, "grad_combine:add": 1}, ("grad_combine:add",), (8,))
    fan("plain_1x1_reflect", (zpad, one, refl), big,
        {"conv_igemm": 5, "conv_igemm:frame": 1, "conv_igemm:fold": 1, "grad_combine:add": 2},
        ("grad_combine:add", "grad_combine:add"), (8,))
    # (f) stride-2 backward-data: 9x13 walks the four parity classes one launch each, on grids of (hi - py + 1) // 2 rows; 16x24
    # is even but its class grids (8 x 12) are below the 16 x 16 the merged launch serves, so it walks the classes too; 32x40
    # is the smallest size here that takes the merged launch (bf16 only)
    s2 = Conv(64, 128, 3, 2, 1)
    loop = {"conv_igemm": 5, "bias_grad": 1, "conv_wgrad": 1}
    cs.append(Case("s2_64to128_9x13", "stride2", (s2,), (2, 64, 9, 13), _both(loop), g_keep=0.125, preds=_NO_PREDS))
    cs.append(Case("s2_64to128_16x24", "stride2", (s2,), (1, 64, 16, 24), _both(loop), g_keep=0.125, preds=_NO_PREDS))
    cs.append(Case("s2_64to128_32x40", "stride2", (s2,), (1, 64, 32, 40),
                   {"fp32": dict(loop), "bf16": {"conv_igemm": 1, "conv_igemm_classes": 1, "bias_grad": 1, "conv_wgrad": 1}},
                   g_keep=0.125, preds=_NO_PREDS))
    # (g) a transposed conv: forward by parity classes, weight gradient with the roles of input and gradient swapped
    cs.append(Case("convT_128to64_5x7", "transposed", (Conv(128, 64, 3, 2, 1, transposed=True),), (2, 128, 5, 7),
                   _both({"conv_igemm": 5, "bias_grad": 1, "conv_wgrad": 1}), g_keep=0.125, preds=_NO_PREDS))
    return cs


def _both_t(order):
    return {"fp32": tuple(order), "bf16": tuple(order)}


CASES = {c.name: c for c in _cases()}

# the paths no test reached before (module docstring of tests/test_layer_glue_exact_gpu.py): number -> the cases that hold it
PATH_CASES = {n: [c.name for c in CASES.values() if n in c.paths] for n in range(1, 9)}
