"""GPU: the batched InstanceNorm elementwise kernels (csrc/norm_act.hip: in_apply_kernel, in_bwd_apply_kernel).

A lane takes its next UNR pixel trips as one batch (all loads first, then compute and store) while it has UNR trips left and
makes the rest one at a time; UNR = min(4, pixels per lane of the launch's grid) for fp32 / bf16, 2 for the split-pair types.  Reference everywhere: stock torch in fp32 on the
same rounded inputs -- F.instance_norm + activation (+ residual), and autograd of that composite for ops.in_bwd.
Tolerances (rel-L2) are those of test_kernels_gpu.py::test_instance_norm_finalize_fused_into_elementwise_kernels:
forward 1e-5 (fp32) / 4e-3 (bf16), backward 2e-5 / 6e-3.  Split-pair tensors store a value to 2^-17 relative, so their bounds
are the fp32 ones plus 2^-17 (7.7e-6): 2e-5 forward, 3e-5 backward; the mixed form (pair-typed saved x, bf16 gradients)
writes bf16 and takes the bf16 bound.

Trip counts under pix_grid (PL = pixel lanes of a workgroup, bx = pixel blocks, a lane makes ceil((HW - p0) / (bx PL)) trips):
  (2, 5, 7, C=8 bf16 / 4 fp32)      PL 256, 2 px per lane, bx 1: 35 lanes make ONE trip -- less than the batch of 2
  (1, 3, 3, C=256 bf16 / 128 fp32)  PL 8, bx 1: lane 0 makes 2 trips (exactly one batch), lanes 1-7 one (single trip)
  (3, 33, 17, C=64 bf16 / 32 fp32)  PL 32, bx 9, stride 288 over 561 pixels: 2 trips below p0 = 273, 1 above
  (1, 128, 64, C=32 bf16 / 16 fp32) PL 64, bx 64: every lane makes exactly 2 trips = one batch of 2
  (4, 130, 127, C=128 fp32)         PL 8, 4 px per lane, bx 516, stride 4128 over 16510: 4 trips = one batch of 4; the lanes
                                    from p0 = 4126 make 3 (no batch, three single trips)
  (16, 130, 126, C=256 bf16)        PL 8, 16 px per lane, bx 128 (2048 workgroups), stride 1024 over 16380 pixels (no multiple
                                    of 8): 16 trips = 4 batches of 4; the lanes from p0 = 1020 make 15 (3 batches + 3 single trips)
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

FWD_TOL = {torch.float32: 1e-5, torch.bfloat16: 4e-3, "pair": 2e-5}
BWD_TOL = {torch.float32: 2e-5, torch.bfloat16: 6e-3, "pair": 3e-5}

SMALL = [(2, 5, 7, 8), (1, 3, 3, 256), (3, 33, 17, 64), (1, 128, 64, 32)]
BIG = (16, 130, 126, 256)
BIG_F32 = (4, 130, 127, 128)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cta_gan_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _rel_l2(got, want):
    got, want = got.detach().float(), want.detach().float()
    assert got.shape == want.shape, (got.shape, want.shape)
    return float((got - want).norm() / want.norm().clamp_min(1e-20))


def _act(t, act):
    from cta_gan_amd import ops
    return F.relu(t) if act == ops.ACT_RELU else F.leaky_relu(t, 0.2) if act == ops.ACT_LRELU else t


_CACHE = {}


def _data(shape, dtype, dev):
    """Inputs of one (shape, dtype), made once and never modified: x, residual r, gradient g (NHWC, rounded to dtype), the
    padded-grid gradient is made by its own test."""
    key = (shape, dtype)
    if key not in _CACHE:
        gen = torch.Generator(device=dev).manual_seed(sum(shape) + (0 if dtype == torch.float32 else 1))
        mk = lambda: torch.randn(shape, generator=gen, device=dev)
        x = (mk() * 1.7 + 0.3).to(dtype)
        _CACHE[key] = (x, mk().to(dtype), mk().to(dtype))
    return _CACHE[key]


def _shape_for(shape, dtype):
    b, h, w, c = shape
    return (b, h, w, c // 2) if dtype == torch.float32 else shape      # the same chunks per pixel in fp32 (4 elements per chunk)


def _check_forward(x, r, dtype, ops, acts_res):
    mean, rstd = ops.in_stats(x)
    xn = F.instance_norm(x.float().permute(0, 3, 1, 2), eps=1e-5)
    for act, with_res in acts_res:
        res = r if with_res else None
        out = torch.empty_like(x)
        ops.in_apply(x, mean, rstd, act, res, out)
        ref = _act(xn, act)
        if with_res:
            ref = ref + r.float().permute(0, 3, 1, 2)
        err = _rel_l2(out.permute(0, 3, 1, 2), ref)
        print("fwd", tuple(x.shape), dtype, "act", act, "res", with_res, "rel-L2 %.3g" % err)
        assert err < FWD_TOL[dtype], (act, with_res, err)


def _check_backward(x, g, dtype, ops, acts):
    mean, rstd = ops.in_stats(x)
    for act in acts:
        dx = torch.empty_like(x)
        ops.in_bwd(x, g, 0, mean, rstd, act, dx)
        xa = x.float().permute(0, 3, 1, 2).clone().requires_grad_(True)
        _act(F.instance_norm(xa, eps=1e-5), act).backward(g.float().permute(0, 3, 1, 2))
        err = _rel_l2(dx.permute(0, 3, 1, 2), xa.grad)
        print("bwd", tuple(x.shape), dtype, "act", act, "rel-L2 %.3g" % err)
        assert err < BWD_TOL[dtype], (act, err)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SMALL, ids=["lt_batch_1chunk", "one_batch_32chunks", "one_or_half_batch", "one_batch_all"])
def test_short_lanes_every_activation_with_and_without_residual(shape, dtype, dev):
    """Lanes that make less than one batch, exactly one batch, or a mix; channel extremes C = 8 / 256 (bf16) and 4 / 128 (fp32):
    one chunk per pixel with 256 pixel lanes, and 32 chunks per pixel with 8."""
    from cta_gan_amd import ops
    x, r, g = _data(_shape_for(shape, dtype), dtype, dev)
    acts = (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_LRELU)
    _check_forward(x, r, dtype, ops, [(a, wr) for a in acts for wr in (False, True)])
    _check_backward(x, g, dtype, ops, acts)


def test_several_batches_and_ragged_tail_bf16(dev):
    """The 16-pixels-per-lane grid (2048 workgroups): 4 batches of 4 per lane, the last one ragged for the lanes from p0 = 1020."""
    from cta_gan_amd import ops
    x, r, g = _data(BIG, torch.bfloat16, dev)
    acts = (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_LRELU)
    _check_forward(x, r, torch.bfloat16, ops, [(a, wr) for a in acts for wr in (False, True)])
    _check_backward(x, g, torch.bfloat16, ops, acts)


def test_one_batch_of_four_or_three_single_trips_fp32(dev):
    """fp32 at 4 pixels per lane: one batch of 4, or three single trips for the lanes from p0 = 4126."""
    from cta_gan_amd import ops
    x, r, g = _data(BIG_F32, torch.float32, dev)
    _check_forward(x, r, torch.float32, ops, [(ops.ACT_RELU, False), (ops.ACT_NONE, True), (ops.ACT_LRELU, True)])
    _check_backward(x, g, torch.float32, ops, (ops.ACT_RELU, ops.ACT_NONE))


@pytest.mark.parametrize("shape", [BIG, (3, 33, 17, 64)], ids=["several_batches", "small"])
def test_in_place_equals_out_of_place_bit_for_bit(shape, dev):
    """engine.inorm_forward normalises in place (out == x) when it keeps nothing: every load of a batch precedes its first store."""
    from cta_gan_amd import ops
    x, r, _ = _data(shape, torch.bfloat16, dev)
    mean, rstd = ops.in_stats(x)
    for act, res in ((ops.ACT_RELU, None), (ops.ACT_NONE, r), (ops.ACT_LRELU, None)):
        out = torch.empty_like(x)
        ops.in_apply(x, mean, rstd, act, res, out)
        xi = x.clone()
        ops.in_apply(xi, mean, rstd, act, res, xi)
        assert torch.equal(xi, out), act


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_output_into_a_channel_slice_leaves_the_rest_untouched(dtype, dev):
    """`out` is a channel slice of a wider buffer (o_ld > C, the U-Net concat case); x is one too (x_ld > C)."""
    from cta_gan_amd import ops
    shape = _shape_for((3, 33, 17, 64), dtype)
    x, r, _ = _data(shape, dtype, dev)
    b, h, w, c = shape
    mean, rstd = ops.in_stats(x)
    dense = torch.empty_like(x)
    ops.in_apply(x, mean, rstd, ops.ACT_LRELU, r, dense)
    wide = torch.full((b, h, w, c + 24), 7.0, dtype=dtype, device=dev)
    xw = torch.full((b, h, w, 2 * c), -3.0, dtype=dtype, device=dev)
    xw[..., c:] = x
    ops.in_apply(xw[..., c:], mean, rstd, ops.ACT_LRELU, r, wide[..., 8:8 + c])
    assert torch.equal(wide[..., 8:8 + c], dense)
    assert bool((wide[..., :8] == 7.0).all()) and bool((wide[..., 8 + c:] == 7.0).all())
    xn = F.instance_norm(x.float().permute(0, 3, 1, 2), eps=1e-5)
    ref = F.leaky_relu(xn, 0.2) + r.float().permute(0, 3, 1, 2)
    assert _rel_l2(dense.permute(0, 3, 1, 2), ref) < FWD_TOL[dtype]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_gradient_on_the_reflection_padded_grid(dtype, dev):
    """ops.in_bwd with pad = 1 (fold_load, one pixel per trip) against autograd through F.pad(mode="reflect"), whose backward
    is the fold."""
    from cta_gan_amd import ops
    b, h, w, c = _shape_for((2, 9, 4, 64), dtype)
    x, _, _ = _data((b, h, w, c), dtype, dev)
    gen = torch.Generator(device=dev).manual_seed(11)
    gp = torch.randn((b, h + 2, w + 2, c), generator=gen, device=dev).to(dtype)
    mean, rstd = ops.in_stats(x)
    for act in (ops.ACT_RELU, ops.ACT_NONE, ops.ACT_LRELU):
        dx = torch.empty_like(x)
        ops.in_bwd(x, gp, 1, mean, rstd, act, dx)
        xa = x.float().permute(0, 3, 1, 2).clone().requires_grad_(True)
        y = F.pad(_act(F.instance_norm(xa, eps=1e-5), act), (1, 1, 1, 1), mode="reflect")
        y.backward(gp.float().permute(0, 3, 1, 2))
        err = _rel_l2(dx.permute(0, 3, 1, 2), xa.grad)
        print("bwd pad1", dtype, "act", act, "rel-L2 %.3g" % err)
        assert err < BWD_TOL[dtype], (act, err)


@pytest.fixture()
def pair_mode():
    from cta_gan_amd import ops
    prev = (ops.PAIR, ops.PAIR_BWD_PLAIN)
    yield ops
    ops.set_pair_mode(*prev)


@pytest.mark.parametrize("shape", [(3, 33, 17, 64), (2, 130, 126, 256)], ids=["one_or_half_batch", "several_batches"])
def test_split_pair_forward_and_backward(shape, dev, pair_mode):
    """Activations in the split-pair form (two bf16 planes per tensor, batches of 2): (3, 33, 17, 64) as above;
    (2, 130, 126, 256) has PL 8, 2 px per lane, bx 1024, stride 8192 over 16380 pixels: 2 trips = one batch below p0 = 8188,
    one trip above."""
    ops = pair_mode
    x32, r32, g32 = _data(shape, torch.float32, dev)
    ops.set_pair_mode(True)
    x, r, g = ops.to_pair(x32), ops.to_pair(r32), ops.to_pair(g32)
    xv, rv, gv = ops.from_pair(x), ops.from_pair(r), ops.from_pair(g)      # what the kernels really see: hi + lo
    mean, rstd = ops.in_stats(x)
    xn = F.instance_norm(xv.permute(0, 3, 1, 2), eps=1e-5)
    for act, res in ((ops.ACT_RELU, None), (ops.ACT_NONE, r), (ops.ACT_LRELU, None)):
        out = ops.empty_like_act(x)
        ops.in_apply(x, mean, rstd, act, res, out)
        ref = _act(xn, act)
        if res is not None:
            ref = ref + rv.permute(0, 3, 1, 2)
        err = _rel_l2(ops.from_pair(out).permute(0, 3, 1, 2), ref)
        print("pair fwd", shape, "act", act, "rel-L2 %.3g" % err)
        assert err < FWD_TOL["pair"], (act, err)
        dx = ops.empty_like_act(x)
        ops.in_bwd(x, g, 0, mean, rstd, act, dx)
        xa = xv.permute(0, 3, 1, 2).clone().requires_grad_(True)
        _act(F.instance_norm(xa, eps=1e-5), act).backward(gv.permute(0, 3, 1, 2))
        err = _rel_l2(ops.from_pair(dx).permute(0, 3, 1, 2), xa.grad)
        print("pair bwd", shape, "act", act, "rel-L2 %.3g" % err)
        assert err < BWD_TOL["pair"], (act, err)


def test_mixed_backward_pair_saved_x_bf16_gradient(dev, pair_mode):
    """The bf16x3f arrangement: the saved forward activation is a split pair, the gradients in and out plain bf16 (a DT_MIX
    launch, reached through ops.set_pair_mode(True, bwd_plain=True) + ops.plain_backward())."""
    ops = pair_mode
    shape = (3, 33, 17, 64)
    x32, _, g32 = _data(shape, torch.float32, dev)
    ops.set_pair_mode(True, bwd_plain=True)
    x = ops.to_pair(x32)
    xv = ops.from_pair(x)
    mean, rstd = ops.in_stats(x)
    g = g32.bfloat16()
    with ops.plain_backward():
        assert ops.dtc_saved(x) == ops.DT_MIX and ops.dtc(g) == 1      # plain bf16
        for act in (ops.ACT_RELU, ops.ACT_NONE, ops.ACT_LRELU):
            dx = torch.empty_like(g)
            ops.in_bwd(x, g, 0, mean, rstd, act, dx)
            xa = xv.permute(0, 3, 1, 2).clone().requires_grad_(True)
            _act(F.instance_norm(xa, eps=1e-5), act).backward(g.float().permute(0, 3, 1, 2))
            err = _rel_l2(dx.permute(0, 3, 1, 2), xa.grad)
            print("mix bwd act", act, "rel-L2 %.3g" % err)
            assert err < BWD_TOL[torch.bfloat16], (act, err)
