"""GPU: the split-bf16 ("bf16x3") compute mode -- split-pair storage ([hi | lo] bf16 planes per pixel row, ops.PAIR), every conv
contraction as hi.hi + hi.lo + lo.hi on the bf16 matrix cores straight from the planes.  It must meet the fp32 mode's parity bars (the reference computes in fp32:
Model/HdGan.py:20-23): the north_star's "generator output within 1e-3 rel-L2 of the CPU reference", the reference-generated
goldens at the fp32 tolerances of tests/test_parity_gpu.py, and per-layer agreement with stock torch at 5e-4 of the
tensor's max (forward) / 1e-3 (gradients) -- against 2e-4 / 4e-4 for exact-f32 MFMA and 5e-3 rel-L2 for plain bf16."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def x3_mode():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cta_gan_amd import _lib, nets
    _lib.load()
    nets.set_default_compute_dtype("bf16x3")
    assert nets.compute_mode() in ("bf16x3", "bf16x3f")      # (CTG_X3F=1 runs this file in the bf16-backward form of the mode)
    yield
    nets.set_default_compute_dtype(torch.float32)
    assert nets.compute_mode() == "fp32"


def rel_l2(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.sqrt(((got - want) ** 2).sum()) / max(np.sqrt((want ** 2).sum()), 1e-30))


def test_pair_storage_round_trip_and_views():
    """fp32 -> split pair -> fp32 to 2^-16 relative; planes are [hi C | lo C] per pixel; a channel slice of a pair buffer is a
    pair view (lo plane ld / 2 behind); an elementwise kernel (copy_channels) moves both planes."""
    from cta_gan_amd import ops
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(2, 5, 7, 64, generator=g) * torch.logspace(-3, 3, 64)).cuda()
    p = ops.to_pair(x)
    assert ops.is_pair(p) and tuple(p.shape) == (2, 5, 7, 64) and p.stride(2) == 128
    hi, lo = p.float(), ops.pair_lo(p).float()
    assert torch.equal(hi, x.bfloat16().float())
    assert float((((hi + lo) - x).abs() / x.abs().clamp_min(1e-30)).max()) < 2 ** -15
    back = ops.from_pair(p)
    assert torch.equal(back, hi + lo)
    sl = p[..., 32:]                                  # channel slice: still a pair (hi at +32, lo at +64+32)
    assert torch.equal(ops.from_pair(sl), back[..., 32:])
    dst = ops.empty_act((2, 5, 7, 96), torch.bfloat16, x.device)
    ops.zero_act(dst)
    ops.copy_channels(sl, dst[..., 64:])
    torch.cuda.synchronize()
    full = ops.from_pair(dst)
    assert torch.equal(full[..., 64:], back[..., 32:]) and float(full[..., :64].abs().max()) == 0.0


def test_weight_split_in_pair_k_step_order():
    """ctg_split_weights: per 32 channels [hi 32 | lo 32]."""
    from cta_gan_amd import ops
    g = torch.Generator().manual_seed(2)
    for cin in (128, 96, 32):
        w = torch.randn(9, 32, cin, generator=g).cuda()
        sw = ops.split_w_pair(w, cin).float()
        assert tuple(sw.shape) == (9, 32, 2 * cin)
        hi = w.bfloat16().float()
        lo = (w - hi).bfloat16().float()
        for j in range(cin // 32):
            assert torch.equal(sw[..., 64 * j:64 * j + 32], hi[..., 32 * j:32 * j + 32])
            assert torch.equal(sw[..., 64 * j + 32:64 * j + 64], lo[..., 32 * j:32 * j + 32])


@pytest.mark.parametrize("case", ["head_7x7_64ch", "reg_first_3x3_cin2_32ch", "tail_7x7_flipped", "ragged_4x4_cin1_64ch"])
def test_image_correlation_weight_gradient_one_launch_equals_three(case, monkeypatch):
    """Round 5: the split-pair image-correlation weight gradient (csrc/corr_small.hip, PAIR) sweeps g_hi.I_hi + g_hi.I_lo +
    g_lo.I_hi in ONE launch (each plane of g read once).  Same products and fp32 accumulation as rounds 3-4's three launches --
    only the order of the fp32 sums differs -- and within 1e-5 of an fp64 correlation of the fp32 operands."""
    from cta_gan_amd import ops
    from cta_gan_amd.ops import PAD_REFLECT, PAD_ZERO
    gen = torch.Generator().manual_seed(5)
    b, h, w, mc, cin, k, pad, reflect = {"head_7x7_64ch": (2, 40, 56, 64, 1, 7, 3, True),
                                          "reg_first_3x3_cin2_32ch": (2, 37, 45, 32, 2, 3, 1, False),
                                          "tail_7x7_flipped": (2, 33, 47, 64, 1, 7, 3, True),
                                          "ragged_4x4_cin1_64ch": (1, 19, 21, 64, 1, 4, 1, False)}[case]
    tail = case.startswith("tail")
    g32 = torch.randn(b, h, w, mc, generator=gen).cuda()
    gp = ops.to_pair(g32)
    if tail:
        # dW[ci][ky][kx] of Conv2d(64, 1, 7) behind ReflectionPad2d(3): the wide tensor is the layer INPUT, the "image" is dL/dy
        img = [torch.randn(b, h, w, generator=gen).cuda(), None]
        args = (pad, PAD_REFLECT, img[0], None, k, 2 * pad, PAD_ZERO, h + 2 * pad, w + 2 * pad)
        out_shape, tail_args = (1, mc, k, k), (k * k - 1, mc, k * k, k * k, -1)
    else:
        ih, iw = h + k - 1 - 2 * pad, w + k - 1 - 2 * pad
        img = [torch.randn(b, ih, iw, generator=gen).cuda() for _ in range(cin)] + [None]
        args = (0, PAD_ZERO, img[0], img[1], k, pad, PAD_REFLECT if reflect else PAD_ZERO, h, w)
        out_shape, tail_args = (mc, cin, k, k), (0, mc, cin * k * k, cin * k * k, 1)

    def run():
        dw = torch.zeros(out_shape, device="cuda")
        ops.corr_smallcin(gp, *args, dw, *tail_args)
        torch.cuda.synchronize()
        return dw.cpu()

    one = run()
    monkeypatch.setenv("CTG_CORR_3RUN", "1")
    three = run()
    monkeypatch.delenv("CTG_CORR_3RUN")
    # fp64 reference on the fp32 operands
    gd = g32.double().permute(0, 3, 1, 2).cpu()
    if tail:
        xpad = torch.nn.functional.pad(gd, (pad,) * 4, mode="reflect")
        gy = img[0].double().cpu()[:, None]
        ref = torch.nn.grad.conv2d_weight(xpad, (1, mc, k, k), gy)
    else:
        im = torch.stack([t.double().cpu() for t in img[:cin]], 1)
        im = torch.nn.functional.pad(im, (pad,) * 4, mode="reflect" if reflect else "constant")
        ref = torch.nn.grad.conv2d_weight(im, (mc, cin, k, k), gd)
    scale = float(ref.abs().max())
    e13 = float((one - three).abs().max()) / scale
    e1, e3 = float((one.double() - ref).abs().max()) / scale, float((three.double() - ref).abs().max()) / scale
    print(case, "one vs three %.2e, one vs fp64 %.2e, three vs fp64 %.2e" % (e13, e1, e3))
    assert e13 < 2e-6 and e1 < 1e-5 and e3 < 1e-5


X3_SPECS = ["res3x3_reflect_64", "res3x3_reflect_256", "down3x3_s2", "up_convT", "d_4x4_s2", "d_4x4_s1", "d_last_512to1",
            "g_tail_7x7_tanh", "reg_3x3_lrelu_32", "reg_up_96to32", "reg_1x1_64to128", "reg_out_32to2",
            "halo_reg_3x3_lrelu_32_ragged", "halo_reflect_64_ragged", "halo_d_4x4_s1_256to512", "halo_128to256",
            "halo_up_convT_classes", "halo_down_s2_bwd_classes", "frame_reflect_64", "frame_reflect_256", "frame_reflect_64_long_edges",
            "ring_res3x3_reflect_256", "ring_d_4x4_s2_tail", "s2d_d_4x4_64to128_in_lrelu", "s2d_d_4x4_128to256_odd",
            "s2d_down3x3_64to128", "s2d_down3x3_128to256_odd",
            # first layers fed by 1-/2-channel fp32 image planes: split-bf16 im2col tile (conv_small X3), image-correlation
            # weight gradient as one three-sweep launch on the gradient's planes (corr_small PAIR)
            "small_reg_first_cin2_in_lrelu", "small_d_first_cin1_s2", "small_head_cin2"]


@pytest.mark.parametrize("name", X3_SPECS)
def test_conv_family_x3(name):
    """Every conv kernel family of tests/test_kernels_gpu.py in the split-bf16 mode against stock fp32 torch."""
    import test_kernels_gpu as K
    spec, shape, norm_act = K._conv_specs()[name]
    dev = torch.device("cuda:0")
    probe = K._make_probe(spec, norm_act).to(dev)
    rng = np.random.default_rng(11)
    x = torch.from_numpy(rng.standard_normal(shape).astype(np.float32))
    xg = x.to(dev).requires_grad_(True)
    y = probe(xg)
    assert y.dtype == torch.float32
    gout = torch.from_numpy(rng.standard_normal(tuple(y.shape)).astype(np.float32))
    y.backward(gout.to(dev))
    w = probe.slot.weight.detach().cpu().clone().requires_grad_(True)
    b = probe.slot.bias.detach().cpu().clone().requires_grad_(True)
    xr = x.clone().requires_grad_(True)
    yr = K._ref_conv(spec, xr, w, b, spec.act, norm_act)
    yr.backward(gout)
    # behind an InstanceNorm + (Leaky)ReLU a forward difference of 1e-5 flips the mask of the few pre-activations that close to
    # zero (expected count ~ elements x 1e-5): each is an O(1) outlier in a max-norm and ~3e-3 in rel-L2 on a 1e5-element tensor
    # (observed: one flip, 2.9e-3) -- so gradients of the specs with an activation are held in rel-L2 (5e-3: the bf16 family's
    # bound, tests/test_kernels_gpu.py), the others in the max-norm (1e-3)
    l2 = norm_act is not None
    errs = {"fwd": K._rel(y, yr), "dx": K._rel(xg.grad, xr.grad, l2), "dw": K._rel(probe.slot.weight.grad, w.grad, l2)}
    print(name, {k: "%.2e" % v for k, v in errs.items()})
    gtol = 5e-3 if l2 else 1e-3
    assert errs["fwd"] < 5e-4 and errs["dx"] < gtol and errs["dw"] < gtol, errs


@pytest.mark.parametrize("shape", [(2, 64, 32, 48), (1, 256, 48, 32), (1, 32, 64, 32)], ids=["64", "256", "32"])
def test_residual_blocks_fused_epilogue_x3(shape):
    """Two chained residual blocks on 16-aligned maps >= 32 pixels in the split-bf16 mode: the backward-data pass of each
    reflect-padded conv folds its frame, adds the skip gradient and takes the InstanceNorm-backward sums in its (split-pair)
    epilogue -- against the blocks in stock fp32 torch, at the single-layer bars times the depth."""
    import test_kernels_gpu as K
    from cta_gan_amd import synth
    from cta_gan_amd.Model.HdGan import ResidualBlock
    dev = torch.device("cuda:0")
    c = shape[1]
    hip = [synth.fill_module(ResidualBlock(c), seed=60 + i).to(dev) for i in range(2)]
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.standard_normal(shape).astype(np.float32))
    xg = x.to(dev).requires_grad_(True)
    y = hip[1](hip[0](xg))
    gout = torch.from_numpy(rng.standard_normal(shape).astype(np.float32))
    y.float().backward(gout.to(dev))
    ws = [[dict(m.named_parameters())[k].detach().cpu().clone().requires_grad_(True)
           for k in ("conv_block.1.weight", "conv_block.5.weight")] for m in hip]
    xr = x.clone().requires_grad_(True)
    ident = lambda t: t      # noqa: E731
    yr = K._ref_resblock(K._ref_resblock(xr, ws[0][0], ws[0][1], ident), ws[1][0], ws[1][1], ident)
    yr.backward(gout)
    errs = {"fwd": K._rel(y, yr, True), "dx": K._rel(xg.grad, xr.grad, True)}
    for i in range(2):
        for j, k in enumerate(("conv_block.1.weight", "conv_block.5.weight")):
            errs["dw%d%d" % (i, j)] = K._rel(dict(hip[i].named_parameters())[k].grad, ws[i][j].grad, True)
    print(shape, {k: "%.2e" % v for k, v in errs.items()})
    # rel-L2: forward 1e-4; gradients 1e-2 (four InstanceNorm + ReLU layers deep: sqrt(e) of flipped masks per layer, see
    # test_goldens_x3)
    assert errs["fwd"] < 1e-4, errs
    assert all(v < 1e-2 for k, v in errs.items() if k != "fwd"), errs


@pytest.mark.parametrize("shape", [(4, 512, 512), (5, 500, 430), (9, 352, 344)], ids=["4x512x512", "5x500x430_ragged", "9x352x344"])
def test_sliding_window_conv32_split_pair(shape):
    """`conv_strip32p_kernel`: the 32 -> 32 channel 3x3 launches with >= 2^20 output pixels in the split-bf16 mode (split-pair in
    and out, both weight halves in registers, input-stationary row loop, counted vmcnt ring).  The same launch restricted to one
    sample runs the halo-resident kernel: the batched launch must agree with the per-sample launches to fp32 rounding (other
    summation order) -- reflect and zero padding, forward and flipped tap order, bias + LeakyReLU / ReLU epilogues, ragged
    strips and bands, InstanceNorm moments -- and with stock fp32 torch to the mode's 1e-5.
    Bit-exact per-sample, per-band and per-slab checks of this kernel against a float64 reference: tests/test_strip_exact_gpu.py."""
    import torch.nn.functional as F
    from cta_gan_amd import ops
    dev = torch.device("cuda:0")
    b, h, w = shape
    assert b * h * w >= (1 << 20) and h * w < (1 << 20)
    g = torch.Generator().manual_seed(h + w)
    x32 = torch.randn(b, h, w, 32, generator=g).to(dev)
    x = ops.to_pair(x32)
    wp = (torch.randn(9, 32, 32, generator=g) * 0.08).to(dev)
    bias = torch.randn(32, generator=g).to(dev)
    fwd = [ops.pack_tap(ky - 1, kx - 1, ky * 3 + kx) for ky in range(3) for kx in range(3)]
    flip = [ops.pack_tap(1 - ky, 1 - kx, ky * 3 + kx) for ky in range(3) for kx in range(3)]

    def run(xs, taps, pad_mode, bias_, act, want_stats):
        y = ops.empty_act((xs.shape[0], h, w, 32), torch.bfloat16, dev)
        part = ops.conv_igemm(xs, wp, 32, y, bias_, 32, h, w, 0, 0, 1, 1, pad_mode, act, taps, want_stats=want_stats)
        return ops.from_pair(y), part

    for taps, pad_mode, bias_, act, stats in ((fwd, ops.PAD_REFLECT, None, ops.ACT_NONE, True),
                                              (flip, ops.PAD_ZERO, None, ops.ACT_NONE, False),
                                              (fwd, ops.PAD_ZERO, bias, ops.ACT_LRELU, False),
                                              (flip, ops.PAD_REFLECT, bias, ops.ACT_RELU, False)):
        y_all, (p_all, n_all) = run(x, taps, pad_mode, bias_, act, stats)
        for i in sorted({0, b // 2, b - 1}):
            y_i, (p_i, n_i) = run(x[i:i + 1], taps, pad_mode, bias_, act, stats)
            err = float((y_all[i:i + 1] - y_i).abs().max() / y_i.abs().max())
            assert err < 2e-5, (i, pad_mode, act, err)
            if stats:
                assert n_all > 0 and n_i > 0 and n_all != n_i      # two kernels, two partial layouts
                m_all = ops.in_finalize(p_all[i:i + 1].contiguous(), n_all, h * w)
                m_i = ops.in_finalize(p_i, n_i, h * w)
                assert torch.allclose(m_all[0], m_i[0], rtol=1e-4, atol=1e-5) and torch.allclose(m_all[1], m_i[1], rtol=1e-4)
    xr = x32[:1].permute(0, 3, 1, 2)
    wr = wp.reshape(3, 3, 32, 32).permute(2, 3, 0, 1)
    ref = F.conv2d(F.pad(xr, (1, 1, 1, 1), mode="reflect"), wr)
    y_all, _ = run(x, fwd, ops.PAD_REFLECT, None, ops.ACT_NONE, False)
    assert rel_l2(y_all[:1].permute(0, 3, 1, 2).cpu().numpy(), ref.cpu().numpy()) < 2e-5


@pytest.mark.parametrize("shape", [(4, 256, 256), (5, 250, 230), (20, 120, 112)], ids=["4x256x256", "5x250x230_ragged", "20x120x112"])
def test_sliding_window_transposed_conv_split_pair_equals_the_class_kernels(shape):
    """`conv_striptp_128_64_kernel` (round 5: the 128 -> 64 channel stride-2 transposed 3x3 conv of the split-bf16 mode as a
    sliding window -- eight waves split the output channels and the parity classes so that the [w_hi | w_lo] weights stay in
    registers) serves `ctg_conv_igemm_classes` launches with >= 2^18 input pixels; the same launch restricted to one sample runs the
    merged parity classes on `conv_halo_kernel<PK, MC>`.  Per class both accumulate (32-channel slice, tap, [hi.w_hi, hi.w_lo,
    lo.w_hi]) in the same order with the same MFMA operand roles and split the fp32 result the same way: the batched launch must
    equal the per-sample launches BIT FOR BIT in both planes, ragged strips and bands included; the InstanceNorm moments (another
    partial layout) agree after finalisation; and the result matches F.conv_transpose2d in fp32 to the mode's 1e-5.
    Bit-exact per-sample, per-band and per-slab checks of this kernel against a float64 reference: tests/test_strip_exact_gpu.py."""
    import torch.nn.functional as F
    from cta_gan_amd import ops
    from cta_gan_amd.engine import _convT_classes
    dev = torch.device("cuda:0")
    b, h, w = shape
    assert b * h * w >= (1 << 18) and h * w < (1 << 18)
    g = torch.Generator().manual_seed(h * 3 + w)
    x32 = torch.randn(b, h, w, 128, generator=g).to(dev)
    x = ops.to_pair(x32)
    wp = (torch.randn(9, 64, 128, generator=g) * 0.05).to(dev)
    classes = _convT_classes(3, 1)

    def run(xs, want_stats):
        y = ops.empty_act((xs.shape[0], 2 * h, 2 * w, 64), torch.bfloat16, dev)
        ops.zero_act(y)
        r = ops.conv_igemm_classes(xs, wp, 64, y, None, 64, h, w, classes, ops.PAD_ZERO, ops.ACT_NONE, want_stats=want_stats)
        assert r is not None
        return y, r

    y_all, (p_all, n_all) = run(x, True)
    for i in sorted({0, b // 2, b - 1}):
        y_i, (p_i, n_i) = run(x[i:i + 1], True)
        assert torch.equal(y_all[i:i + 1], y_i), i                                        # hi planes
        assert torch.equal(ops.pair_lo(y_all)[i:i + 1], ops.pair_lo(y_i)), i              # lo planes
        assert n_all > 0 and n_i > 0 and n_all != n_i
        m_all = ops.in_finalize(p_all[i:i + 1].contiguous(), n_all, 4 * h * w)
        m_i = ops.in_finalize(p_i, n_i, 4 * h * w)
        assert torch.allclose(m_all[0], m_i[0], rtol=1e-5, atol=1e-6) and torch.allclose(m_all[1], m_i[1], rtol=1e-5)
    y_ns, _ = run(x, False)
    assert torch.equal(y_ns, y_all) and torch.equal(ops.pair_lo(y_ns), ops.pair_lo(y_all))
    # against stock torch: W_packed[t = ky*3+kx][co][ci] is ConvTranspose2d's weight[ci][co][ky][kx]
    wt = wp.reshape(3, 3, 64, 128).permute(3, 2, 0, 1).contiguous()
    ref = F.conv_transpose2d(ops.from_pair(x[:1]).permute(0, 3, 1, 2), wt, stride=2, padding=1, output_padding=1)
    assert rel_l2(ops.from_pair(y_all[:1]).permute(0, 3, 1, 2).cpu().numpy(), ref.cpu().numpy()) < 2e-5


@pytest.mark.parametrize("shape", [(4, 256, 256), (5, 250, 224), (20, 120, 112)], ids=["4x256x256", "5x250x224", "20x120x112"])
def test_sliding_window_stride2_conv_split_pair_equals_the_polyphase_kernel(shape):
    """`conv_strips2p_64_128_kernel` (round 5: the 64 -> 128 channel stride-2 3x3 conv of the split-bf16 mode as a sliding window over
    input row pairs, eight waves with one 16-channel tile of the [w_hi | w_lo] weights in registers each) serves `ctg_conv_igemm`
    launches with >= 2^18 output pixels; the same launch restricted to one sample runs the polyphase slices on
    `conv_halo_kernel<PK, S2D>`.  Both accumulate (phase, 32-channel slice, tap, [hi.w_hi, hi.w_lo, lo.w_hi]) in the same order with
    the same MFMA operand roles and split the fp32 result the same way: the batched launch must equal the per-sample launches BIT
    FOR BIT in both planes; the InstanceNorm moments (another partial layout) agree after finalisation; and the result matches
    F.conv2d in fp32 to the mode's 1e-5.
    Bit-exact per-sample, per-band and per-slab checks of this kernel against a float64 reference: tests/test_strip_exact_gpu.py."""
    import torch.nn.functional as F
    from cta_gan_amd import ops
    from cta_gan_amd.ops import pack_tap
    dev = torch.device("cuda:0")
    b, ho, wo = shape
    assert b * ho * wo >= (1 << 18) and ho * wo < (1 << 18)
    g = torch.Generator().manual_seed(ho * 3 + wo)
    x = ops.to_pair(torch.randn(b, 2 * ho, 2 * wo, 64, generator=g).to(dev))
    wp = (torch.randn(9, 128, 64, generator=g) * 0.05).to(dev)
    taps = [pack_tap(ky - 1, kx - 1, ky * 3 + kx) for ky in range(3) for kx in range(3)]

    def run(xs, want_stats):
        y = ops.empty_act((xs.shape[0], ho, wo, 128), torch.bfloat16, dev)
        ops.zero_act(y)
        r = ops.conv_igemm(xs, wp, 128, y, None, 128, ho, wo, 0, 0, 1, 2, ops.PAD_ZERO, ops.ACT_NONE, taps, want_stats=want_stats)
        return y, r

    y_all, (p_all, n_all) = run(x, True)
    for i in sorted({0, b // 2, b - 1}):
        y_i, (p_i, n_i) = run(x[i:i + 1], True)
        assert torch.equal(y_all[i:i + 1], y_i), i
        assert torch.equal(ops.pair_lo(y_all)[i:i + 1], ops.pair_lo(y_i)), i
        assert n_all > 0 and n_i > 0 and n_all != n_i
        m_all = ops.in_finalize(p_all[i:i + 1].contiguous(), n_all, ho * wo)
        m_i = ops.in_finalize(p_i, n_i, ho * wo)
        assert torch.allclose(m_all[0], m_i[0], rtol=1e-5, atol=1e-6) and torch.allclose(m_all[1], m_i[1], rtol=1e-5)
    y_ns, _ = run(x, False)
    assert torch.equal(y_ns, y_all) and torch.equal(ops.pair_lo(y_ns), ops.pair_lo(y_all))
    wr = wp.reshape(3, 3, 128, 64).permute(2, 3, 0, 1).contiguous()
    ref = F.conv2d(ops.from_pair(x[:1]).permute(0, 3, 1, 2), wr, stride=2, padding=1)
    assert rel_l2(ops.from_pair(y_all[:1]).permute(0, 3, 1, 2).cpu().numpy(), ref.cpu().numpy()) < 2e-5


def test_generator_x3_within_1e3_of_the_cpu_reference():
    """north_star: generator output within 1e-3 rel-L2 of the CPU reference -- at 256^2 against the oracle."""
    from cta_gan_amd import synth
    from cta_gan_amd.Model.HdGan import Generator
    from oracle import ref_models
    x = synth.synth_images("gen256", 2, 256)
    ref = synth.fill_module(ref_models.Generator(1, 1), seed=21)
    with torch.no_grad():
        want = ref(x).numpy()
    hip = synth.fill_module(Generator(1, 1), seed=21).cuda()
    with torch.no_grad():
        got = hip(x.cuda()).float().cpu().numpy()
    err = rel_l2(got, want)
    print("generator 256^2 rel-L2 in bf16x3 mode: %.3e" % err)
    assert err <= 1e-3


@pytest.mark.parametrize("name", ["generator_64", "resblock_256x12", "discriminator_64", "discriminator2_64",
                                  "discriminator_m1_64", "discriminator_m2_128", "nlayer_d_bn_64", "reg_256"])
def test_goldens_x3(name, golden_dir):
    import test_parity_gpu as P
    from hip_ns import hip_namespace
    from oracle import golden_cases
    want = np.load(os.path.join(golden_dir, name + ".npz"))
    got = golden_cases.CASES[name](hip_namespace())
    # outputs at the fp32 bound (1e-3; observed ~3e-5).  Gradients: a forward difference e flips the ReLU / LeakyReLU masks
    # of the pre-activations within e of 0 -- a fraction ~e of the elements, i.e. a rel-L2 gradient error ~sqrt(e) per
    # layer: sqrt(3e-5) = 5e-3 here against sqrt(4e-6) = 2e-3 for exact-f32 MFMA (whose bound is 5e-3) -> 2e-2
    # Reg's input gradient crosses ~45 (Leaky)ReLU / InstanceNorm layers, each adding its ~sqrt(e) of flipped masks (e = 3.4e-5
    # with split-pair storage, whose elementwise consumers also see the 2^-17 of the stored pair): observed 2.1e-2
    rep = P._compare(name, got, want, grad_tol=3e-2 if name == "reg_256" else 2e-2)
    print(name, {k: "%.2e" % v for k, v in rep.items()})


@pytest.mark.parametrize("name", ["hd_step_stage2_256", "cyc_step_128", "p2p_step_128"])
def test_step_goldens_x3(name, golden_dir):
    """One full optimiser step (oracle.ref_steps driving the HIP networks) vs the reference run, fp32 tolerances."""
    import test_parity_gpu as P
    from hip_ns import hip_namespace
    from oracle import golden_cases
    want = np.load(os.path.join(golden_dir, name + ".npz"))
    got = golden_cases.CASES[name](hip_namespace())
    for key in want.files:
        w, g = want[key], got[key]
        if np.ndim(w) == 0:
            assert abs(float(g) - float(w)) <= 2e-3 * max(abs(float(w)), 1e-6) + 1e-6, (name, key, float(g), float(w))
        elif "stats" in key:
            assert np.allclose(g, w, rtol=2e-2, atol=2e-3), (name, key, g, w)
        elif "delta" in key:
            assert np.allclose(g, w, rtol=5e-2, atol=1e-6), (name, key, g, w)
        else:
            # "after": the generator one Adam step later.  Adam's first step is lr * sign(g): what differs is the set of
            # parameters whose tiny gradient changed sign under the mode's gradient noise (5e-3 rel-L2: test_goldens_x3), not
            # a forward precision -- observed 2.8e-2 (the fp32-storage form of the mode, rounds 2-3: 1.9e-2)
            assert P.rel_l2(g, w) <= (4e-2 if "after" in key else 1e-3), (name, key, P.rel_l2(g, w))


def test_product_trainer_step_x3(golden_dir):
    """`Hd_Trainer_x2.train_step` (HIP Adam, side stream, batched D) in the split-bf16 mode vs the stage-2 step golden."""
    import test_step_parity_gpu as S
    want = np.load(os.path.join(golden_dir, "hd_step_stage2_256.npz"))
    tr = S.make_hd()
    losses = tr.train_step(S.hd_batch(), sync_losses=True)
    for k in S.HD_KEYS:
        w = float(want["loss_" + k])
        assert abs(losses[k] - w) <= 2e-3 * max(abs(w), 1e-6) + 1e-6, (k, losses[k], w)
    assert rel_l2(tr.last["fake_B"].cpu().numpy()[:, :, ::8, ::8], want["fake_after_sub"]) <= 4e-2     # (see test_step_goldens_x3)
