"""GPU: the conv LAYER glue of cta_gan_amd/engine.py -- conv_forward, _conv_backward, _bwd_data_launch, add_grad, take_grad --
against plain float64 autograd (tests/layer_ref.py), bit for bit, in the fp32 and the bf16 compute mode.

The kernels have exact tests of their own (tests/test_conv_exact_gpu.py and siblings), driven with tap lists the tests write.
This module holds the ~350 lines that write the tap lists for the networks: which kernel runs, with which taps, packs, channel
pads and channel slices, which gradients are computed at all, and how gradients from several consumers are accumulated.

Exactness argument
------------------
x and w are small integers, biases multiples of 1/8, output gradients sparse in {-1, 0, 1} (tests/conv_ref.py's grids).
  1. Every accumulator -- forward, backward-data, weight gradient, bias gradient -- has a sum of term magnitudes below 2^24
     granules, so its fp32 value is exact whatever the order of summation (layer_ref.check_case, conv_ref.assert_exact_domain).
  2. Every gradient the engine keeps in bf16 -- the input gradient of a wide layer, on the reflection-padded grid, folded, and
     summed over the consumers in the order the backward meets them -- is an integer of magnitude <= 256 in the reference: a
     bf16 value, so it does not matter where the engine rounds.  Operands and output gradients are bf16 values as well.
  3. A forward output kept in bf16 is compared with the reference rounded ONCE (.bfloat16()): pre-activation plus bias is exact
     in fp32 and ReLU is exact, so the store is the only rounding.
  4. ReLU (mask on and off on 10 % .. 90 % of the elements) and "no activation" cases are therefore compared with torch.equal;
     the multi-channel fp32 tails have a ReLU twin for this.
  5. Tanh, Sigmoid and LeakyReLU (whose backward multiplies by 0.2f) cases are compared at TOL / GTOL of
     tests/test_kernels_gpu.py against the unrounded float64 reference, bias gradients with its _db_err; their weights are
     sparse integers times a power of two, which keeps the operands bf16 values and the pre-activations O(1).
All of 1, 2, 4 and 5 are asserted on the CPU (tests/test_layer_ref.py) and again here before anything is launched.

Path table and evidence
-----------------------
Every case names the launches the engine must make for it, as {label: count} per compute mode (layer_ref.Case.calls; the labels
of layer_ref.call_label tell a frame launch from a fused one, and the five uses of grad_combine apart).  The test replaces the
entry points of cta_gan_amd.ops with counting wrappers and asserts the EXACT multiset, for the fan-out cases also the order of
the grad_combine launches, for the tails the (channels, pixel pitch) of the gradient operand conv_wgrad received, and wherever
an activation-backward pass also sums the bias gradient (act_bwd_sum_f32, bias_grad_act) that the buffer it wrote is the one
stored as the parameter's gradient.
The paths no test reached before, and the cases that hold them (layer_ref.PATH_CASES):
  1  _conv_backward step 1, act_bwd_f32 on a map of 75 elements          tail_64to3_{relu,tanh}_5x5
  2  step 1, grad_combine on the (1, 1, n/4, 4) view                     tail_64to{2,3,4}_*, tail_64to1_*_bias_frozen
  3  step 4, gm[..., :16] (16 channels at pitch 32) / full gm            tail_*_8x16, _12x20 / tail_*_7x16, _8x12, _5x5 (bf16)
  4  the 7x7 head on two planes: im2col_pack (Kpad 128), conv_wgrad      head_2to64_* (8 cases: bias x input gradient x size)
     from the packed matrix, input gradient on the padded grid + fold_f32
  5  PatchGAN last layer + Sigmoid, tail_db handed to the cout1 branch   dlast_512to1_sigmoid_* (bf16)
  6  partial preq: (w, not b), (b, not w), (neither, x.req)              preq_plain_lrelu_*, preq_tail_tanh_*, tail_64to1_*_frozen
  7  add_grad, both gradients padded (`p0 and pad`)                      fanout_reflect_reflect_9x11
  8  add_grad, three consumers, padded first / unpadded first            fanout_plain_1x1_reflect_* / fanout_reflect_plain_1x1_*
Also held: the odd-size class loop of the stride-2 backward-data (s2_64to128_9x13: grids of (hi - py + 1) // 2 rows), its merged
launch (s2_64to128_32x40, bf16), the roles-swapped weight gradient of a transposed conv (convT_128to64_5x7), and the 16-aligned
reflect backward-data that consumes the gradient waiting at x as `res` (fanout_*_32x32).

Not reachable, and not tested
-----------------------------
  * the split-pair modes (out of scope here; tests/test_bf16x3_gpu.py);
  * `_bwd_data_launch`'s zero_act branch: no stride-2 layer of the networks has a parity class without taps (k >= 3);
  * the 1-pixel-frame path without `conv_fusable` (ops._NO_HALO / _NO_EPI_FUSE are A/B switches read at import);
  * `in_bwd` sums in the fused backward-data launch: they need an InstanceNorm producer (tests/test_kernels_gpu.py holds them).

What the module found
---------------------
  * Nothing wrong in the engine: every case is bit-equal (or in tolerance), every call set as read from the code.
  * An even 16 x 24 input of a stride-2 layer does NOT take the merged four-class backward-data launch, whatever one might
    expect from `hi % 2 == 0 and wi % 2 == 0`: ops.conv_igemm_classes serves class grids of 16 x 16 and more only, so the
    smallest merged size is 32 x 32 (case s2_64to128_32x40 was added for it; 16x24 stays, as a class-loop case).
  * Kpad of the two-plane head is 128 whether Cin k k = 98 is rounded up to a multiple of 32 or of 64: mutation (vi) below is
    an equivalent mutant for every head the networks can build.

Mutation checks (each applied once to a scratch copy of engine.py, never committed; the cases that then FAILED)
-----------------------------------------------------------------------------------------------------------
  (i)   `gm[..., :16]` -> `[:8]`                      bf16: tail_64to2_relu_8x16, tail_64to3_tanh_8x16, tail_64to4_relu_12x20
                                                      (no launch: ops.conv_wgrad has no tile for 8 channels and stops in Python)
  (ii)  reflect backward-data taps (-ky, -kx)         48 cases, every reflect case that owes an input gradient: fp32 the 12 tails,
        -> (ky, kx), both lists                       the 4 head_*_dx, the 10 fan-outs; bf16 the same less the four one-channel
                                                      tails, whose input gradient is conv_smallcin's and has no such list
  (iii) add_grad without the fold of `p0 and pad`     fanout_reflect_reflect_9x11, both modes (input gradient)
  (iv)  sm and sn swapped, transposed conv_wgrad      convT_128to64_5x7, both modes (weight gradient, first differing tap named)
  (v)   tail_db not handed to the cout1 branch        bf16: dlast_512to1_sigmoid_5x7, _19x19 -- by the evidence that the stored bias
                                                      gradient is the buffer act_bwd_sum_f32 wrote; the VALUE is unchanged by
                                                      this mutation (the branch then sums the same masked gradient itself), so
                                                      before that evidence was added the mutant survived
  (vi)  Kpad of the head rounded to 64, not 32        none: equivalent mutant, 98 -> 128 either way (see above)
  (none: the unmutated copy through the same runner)  none
"""
import collections
import dataclasses

import pytest
import torch

import conv_ref as R
import layer_ref as L
from test_kernels_gpu import GTOL, TOL, _db_err, _rel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cta_gan_amd import _lib
    _lib.load()  # fail loudly if the HIP library is absent
    return torch.device("cuda:0")


def _make_probe(case):
    """A HipNet whose one activation (or image) is read by every conv of the case; one output per conv."""
    from cta_gan_amd import engine as E
    from cta_gan_amd import nets
    specs = [E.ConvSpec(**dataclasses.asdict(cv)) for cv in case.convs]

    class Probe(nets.HipNet):
        def __init__(self):
            super().__init__()
            self.slots = torch.nn.ModuleList(
                nets._Slot((s.cin, s.cout, s.k, s.k) if s.transposed else (s.cout, s.cin, s.k, s.k), (s.cout,)) for s in specs)

        def forward(self, x):
            return self._call(x)

        def _run(self, tape, inputs, need_in):
            (x,) = inputs
            dt = self.dtype_
            b, c, h, w = x.shape
            if c <= 2:
                xa = E.Act(torch.zeros(1, device=x.device).expand(b, h, w, c), req=need_in[0])
                srcs = (nets._img_plane(x, 0), nets._img_plane(x, 1) if c == 2 else None)
            else:
                xa, srcs = E.Act(nets._to_nhwc(x, dt), req=need_in[0]), None
            ys = [E.conv_forward(tape, self._cache, s, xa, sl.weight, sl.bias, dt, img_sources=srcs)
                  for s, sl in zip(specs, self.slots)]

            def finish(in_acts):
                g, _ = E.take_grad(in_acts[0])
                return [None if g is None else nets._to_nchw_view(g).float()]
            return ys, [xa], finish
    return Probe()


class _Calls:
    """Counting wrappers around the entry points of cta_gan_amd.ops the engine calls (through the module, so setattr is seen)."""

    SUM_OUT = {"act_bwd_sum_f32": 3, "bias_grad_act": 6}      # argument that receives the bias gradient of a fused pass

    def __init__(self, monkeypatch):
        from cta_gan_amd import engine, ops
        self.labels, self.wgrad_g, self.fused_db, self.stored = [], [], [], {}
        for name in L.TRACKED:
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name)))
        store = engine._store_param_grad

        def store_param_grad(param, grad):
            self.stored[id(param)] = grad.data_ptr()
            return store(param, grad)
        monkeypatch.setattr(engine, "_store_param_grad", store_param_grad)

    def _wrap(self, name, fn):
        def wrapper(*args, **kwargs):
            result = fn(*args, **kwargs)
            label = L.call_label(name, args, kwargs, result)
            if label is not None:
                self.labels.append(label)
            if name == "conv_wgrad":
                self.wgrad_g.append((int(args[0].shape[-1]), int(args[0].stride(-2))))
            if name in self.SUM_OUT:
                self.fused_db.append(args[self.SUM_OUT[name]].data_ptr())
            return result
        return wrapper


def _where(kind, idx, case, ci):
    """Tap or tile of a differing element, for the failure message."""
    cv = case.convs[ci]
    if kind == "dw":
        return "tap (ky %d, kx %d) = %d of conv %d" % (idx[2], idx[3], idx[2] * cv.k + idx[3], ci)
    if kind == "db":
        return "channel %d of conv %d" % (idx[0], ci)
    return "sample %d channel %d pixel (%d, %d): 16x16 tile (%d, %d), 8x16 tile (%d, %d)" % (
        idx[0], idx[1], idx[2], idx[3], idx[2] // 16, idx[3] // 16, idx[2] // 8, idx[3] // 16)


def _assert_equal(kind, got, want, case, ci, mode):
    got = got.detach().cpu()
    want = want.to(got.dtype) if got.dtype == torch.bfloat16 else want
    d = R.first_diff(got if got.dtype == torch.bfloat16 else got.double(), want)
    if d is not None:
        idx, g, w, n = d
        raise AssertionError("%s [%s] %s: %d elements differ; first at %s: got %r want %r -- %s"
                             % (case.name, mode, kind, n, idx, g, w, _where(kind, idx, case, ci)))


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(L.CASES))
def test_layer_glue(name, mode, dev, monkeypatch):
    case, dtype = L.CASES[name], L.DTYPES[mode]
    L.check_case(case)                                   # a case off the exact domain is a broken case, never a skip
    ops_ = L.operands(case)
    ref = L.reference(case, ops_)
    x, ws, bs, gs = ops_
    probe = _make_probe(case).to(dev)
    probe.compute_dtype = dtype
    xreq, wreq, breq = case.owed
    with torch.no_grad():
        for sl, w, b in zip(probe.slots, ws, bs):
            sl.weight.copy_(w.float())
            sl.bias.copy_(b.float())
    for sl in probe.slots:
        sl.weight.requires_grad_(wreq)
        sl.bias.requires_grad_(breq)
    xg = x.float().to(dev).requires_grad_(xreq)

    calls = _Calls(monkeypatch)
    ys = probe(xg)
    torch.autograd.backward(list(ys), [g.to(dev).to(y.dtype) for g, y in zip(gs, ys)])
    torch.cuda.synchronize()
    monkeypatch.undo()

    # --- path evidence
    got_calls = dict(collections.Counter(calls.labels))
    assert got_calls == case.calls[mode], (name, mode, got_calls, case.calls[mode])
    if case.order is not None:
        assert tuple(c for c in calls.labels if c.startswith("grad_combine")) == case.order[mode], (name, mode, calls.labels)
    if case.wgrad_g is not None:
        assert calls.wgrad_g == [case.wgrad_g if mode == "bf16" else (32, 32)], (name, mode, calls.wgrad_g)

    # a bias gradient summed by the activation-backward pass is the one that is stored: nothing sums it a second time
    assert sorted(calls.fused_db) == sorted(calls.stored.get(id(sl.bias)) for sl in probe.slots if calls.fused_db), (name, mode)

    # --- what is not owed is not computed
    if not xreq:
        assert xg.grad is None
    for sl, cv in zip(probe.slots, case.convs):
        assert (sl.weight.grad is None) == (not wreq), name
        assert (sl.bias.grad is None) == (not (breq and cv.use_bias)), name

    # --- values
    if case.exact:
        for i, (y, sl, cv) in enumerate(zip(ys, probe.slots, case.convs)):
            assert y.dtype == (torch.float32 if (cv.out_f32 or mode == "fp32") else torch.bfloat16)
            _assert_equal("y", y, ref.y[i], case, i, mode)
            if wreq:
                _assert_equal("dw", sl.weight.grad, ref.dw[i], case, i, mode)
            if breq and cv.use_bias:
                _assert_equal("db", sl.bias.grad, ref.db[i], case, i, mode)
        if xreq:
            _assert_equal("dx", xg.grad, ref.dx, case, 0, mode)
        return
    tol, gtol, l2 = TOL[dtype], GTOL[dtype], mode == "bf16"
    errs = {}
    for i, (y, sl, cv) in enumerate(zip(ys, probe.slots, case.convs)):
        errs["y%d" % i] = _rel(y, ref.y[i], l2)
        if wreq:
            errs["dw%d" % i] = _rel(sl.weight.grad, ref.dw[i], l2)
        if breq and cv.use_bias:
            errs["db%d" % i] = _db_err(sl.bias.grad, ref.db[i], gs[i])
    if xreq:
        errs["dx"] = _rel(xg.grad, ref.dx, l2)
    print(name, mode, {k: "%.2e" % v for k, v in errs.items()})
    assert all(v < (tol if k.startswith("y") else gtol) for k, v in errs.items()), (name, mode, errs)
