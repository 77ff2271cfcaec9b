"""CPU: tests/instnorm_ref.py (the float64 reference of the InstanceNorm kernels) against stock torch in float64 --
F.instance_norm, autograd of act(IN(x)) [+ r] through F.pad(mode="reflect"), and the slab partition's edge cases.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import instnorm_ref as R

ACTS = (R.ACT_NONE, R.ACT_RELU, R.ACT_LRELU)
SIZES = [(1, 1), (2, 2), (3, 5), (5, 7), (9, 4)]


def _rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _torch_act(t, act):
    return F.relu(t) if act == R.ACT_RELU else F.leaky_relu(t, 0.2) if act == R.ACT_LRELU else t


def _stats(x):
    """(mean, rstd) of the reference from ONE slab of exact float64 partials, with the float64 1 / HW torch uses."""
    b, h, w, c = x.shape
    part, _, _ = R.partials(x, 1)
    m = part[:, 0, :, 0] / (h * w)
    var = (part[:, 0, :, 1] / (h * w) - m * m).clamp_min(0.0)
    return m, 1.0 / torch.sqrt(var + 1e-5)


# ------------------------------------------------------------------------------------------------------------------ slabs
@pytest.mark.parametrize("hw,ns,want", [
    (35, 1, [(0, 35)]),                                             # one slab
    (35, 4, [(0, 9), (9, 18), (18, 27), (27, 35)]),                 # several, the last ragged
    (10, 4, [(0, 3), (3, 6), (6, 9), (9, 10)]),
    (9, 4, [(0, 3), (3, 6), (6, 9), (9, 9)]),                       # an empty last slab
    (3, 5, [(0, 1), (1, 2), (2, 3), (3, 3), (3, 3)]),               # nslabs > HW
    (8200, 128, None),                                              # the wrappers' rule at (2, 82, 100): per 65, slab 127 empty
])
def test_slab_partition(hw, ns, want):
    got = R.slab_bounds(hw, ns)
    if want is not None:
        assert got == want
    per = -(-hw // ns)
    assert len(got) == ns and got[0][0] == 0 and max(e for _, e in got) == hw
    assert all(0 <= e - b <= per for b, e in got)
    assert all(got[i][1] == got[i + 1][0] for i in range(ns - 1))                   # contiguous: every pixel exactly once
    assert all(e - b == per for b, e in got if e < hw)                              # only the slab that reaches HW is short
    if (hw, ns) == (8200, 128):
        assert got[127] == (8200, 8200) and got[126] == (8190, 8200)


@pytest.mark.parametrize("ns", [1, 3, 4, 7, 40])
def test_partials_sum_to_the_whole_and_empty_slabs_are_zero(ns):
    x = _rand((2, 5, 7, 3), 1)
    part, mag, count = R.partials(x, ns)
    assert int(count.sum()) == 35 and part.shape == (2, ns, 3, 2)
    flat = x.reshape(2, 35, 3)
    torch.testing.assert_close(part.sum(1)[..., 0], flat.sum(1), rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(part.sum(1)[..., 1], (flat * flat).sum(1), rtol=1e-13, atol=1e-13)
    for s, (p0, p1) in enumerate(R.slab_bounds(35, ns)):
        assert torch.equal(part[:, s, :, 0], flat[:, p0:p1].sum(1))
        if p0 == p1:
            assert not bool(part[:, s].any()) and not bool(mag[:, s].any())
    assert bool((mag >= part.abs()).all())


def test_mode1_partials_use_a_strict_mask():
    """xhat == 0 exactly: ReLU drops the gradient there, LeakyReLU takes the slope."""
    x = torch.tensor([0.0, 1.0, 2.0, 1.0]).to(torch.float64).reshape(1, 2, 2, 1)
    g = torch.tensor([1.0, 2.0, 4.0, 8.0]).to(torch.float64).reshape(1, 2, 2, 1)
    mean, rstd = torch.ones((1, 1), dtype=torch.float64), torch.full((1, 1), 2.0, dtype=torch.float64)
    for act, s1, s2 in ((R.ACT_NONE, 15.0, -2.0 + 8.0), (R.ACT_RELU, 4.0, 8.0),
                        (R.ACT_LRELU, 4.0 + R.SLOPE * 11.0, 8.0 - 2.0 * R.SLOPE)):
        part, _, _ = R.partials(x, 1, 1, g, mean, rstd, act)
        assert float(part[0, 0, 0, 0]) == pytest.approx(s1, rel=1e-15), act
        assert float(part[0, 0, 0, 1]) == pytest.approx(s2, rel=1e-15), act


# ------------------------------------------------------------------------------------------------------------------ finalize
def test_finalize_equals_instance_norm_statistics():
    x = _rand((3, 9, 4, 5), 2, 1.7) + 0.3
    for ns in (1, 5, 36, 50):
        part, _, _ = R.partials(x, ns)
        mean, rstd = R.finalize(part, 36)
        want_m = x.mean((1, 2))
        want_r = 1.0 / torch.sqrt(x.var((1, 2), unbiased=False) + 1e-5)
        # invHW and eps are float32 values: 2^-24 relative on each
        torch.testing.assert_close(mean, want_m, rtol=2e-7, atol=1e-12)
        torch.testing.assert_close(rstd, want_r, rtol=2e-7, atol=0)
    a, b = R.finalize(part, 36, mode=1)
    torch.testing.assert_close(b, (x * x).mean((1, 2)), rtol=2e-7, atol=0)
    assert R.inv_hw(64) == 1.0 / 64 and R.inv_hw(35) != 1.0 / 35 and abs(R.inv_hw(35) * 35 - 1) < 2.0 ** -24


def test_finalize_clamps_a_negative_variance():
    part = torch.tensor([[[[8.0, 70.0]], [[0.0, -60.0]]]], dtype=torch.float64)      # [1, 2, 1, 2]: E[x^2] - m^2 = 2.5 - 4
    mean, rstd = R.finalize(part, 4)
    assert float(mean) == 2.0 and float(rstd) == 1.0 / (R.EPS ** 0.5)


# ------------------------------------------------------------------------------------------------------------------ fold
@pytest.mark.parametrize("pad", [1, 2, 3])
def test_fold_is_the_transpose_of_reflection_padding(pad):
    for h, w in [(pad + 1, pad + 1), (pad + 1, 9), (8, pad + 1), (5, 7), (4, 4)]:
        if pad >= min(h, w):
            continue
        g = _rand((2, h + 2 * pad, w + 2 * pad, 3), 10 * pad + h)
        x = torch.zeros((2, 3, h, w), dtype=torch.float64, requires_grad=True)
        want, = torch.autograd.grad(F.pad(x, (pad,) * 4, mode="reflect"), x, _nchw(g).contiguous())
        torch.testing.assert_close(R.fold(g, pad), _nhwc(want), rtol=1e-14, atol=1e-14)
    assert torch.equal(R.fold(g, 0), g)


# ------------------------------------------------------------------------------------------------------------------ forward / backward
@pytest.mark.parametrize("act", ACTS)
def test_forward_equals_instance_norm_activation_residual(act):
    for n, (h, w) in enumerate(SIZES[1:]):
        x, r = _rand((2, h, w, 3), 20 + n, 1.7) + 0.3, _rand((2, h, w, 3), 30 + n)
        mean, rstd = _stats(x)
        want = _torch_act(F.instance_norm(_nchw(x), eps=1e-5), act)
        torch.testing.assert_close(R.forward(x, mean, rstd, act, slope=0.2), _nhwc(want), rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(R.forward(x, mean, rstd, act, r, slope=0.2), _nhwc(want) + r, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("pad", [0, 1, 2, 3])
@pytest.mark.parametrize("act", ACTS)
def test_backward_equals_autograd_through_reflection_padding(act, pad):
    """partials (MODE 1) -> finalize (mode 1) -> backward, against autograd of F.pad(act(IN(x)) + r): the residual only passes
    the gradient through."""
    for n, (h, w) in enumerate([(pad + 1, pad + 1), (pad + 1, 6), (7, pad + 1), (5, 7)]):
        if h * w == 1:
            continue
        x = _rand((2, h, w, 3), 40 + n + 7 * pad, 1.7) + 0.3
        r = _rand((2, h, w, 3), 50 + n)
        gp = _rand((2, h + 2 * pad, w + 2 * pad, 3), 60 + n + pad)
        xa = _nchw(x).clone().requires_grad_(True)
        y = _torch_act(F.instance_norm(xa, eps=1e-5), act) + _nchw(r)
        if pad:
            y = F.pad(y, (pad,) * 4, mode="reflect")
        y.backward(_nchw(gp).contiguous())
        mean, rstd = _stats(x)
        g = R.fold(gp, pad)
        for ns in (1, 3):
            part, _, _ = R.partials(x, ns, 1, g, mean, rstd, act)
            a = part.sum(1) / (h * w)
            if act == R.ACT_LRELU:      # the mathematical slope for the comparison with torch
                xh = R.xhat(x, mean, rstd)
                gm = R.act_grad(g, xh, act, 0.2)
                a = torch.stack((gm.sum((1, 2)), (gm * xh).sum((1, 2))), -1) / (h * w)
            dx, s = R.backward(x, g, mean, rstd, a[..., 0], a[..., 1], act, slope=0.2)
            torch.testing.assert_close(dx, _nhwc(xa.grad), rtol=1e-9, atol=1e-9)
            assert bool((s >= 0).all())


# ------------------------------------------------------------------------------------------------------------------ op for op
def _grid_case(seed, shape=(2, 5, 7, 4)):
    gen = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, s: torch.randint(lo, hi + 1, s, generator=gen).to(torch.float64)
    b, c = shape[0], shape[3]
    x, r, g = ri(-8, 8, shape), ri(-8, 8, shape), ri(-4, 4, shape)
    mean = ri(-2, 2, (b, c))
    rstd = 2.0 ** ri(-2, 1, (b, c))
    return x, r, g, mean, rstd, ri(-8, 8, (b, c)) / 4, ri(-4, 4, (b, c)) / 4


@pytest.mark.parametrize("act", ACTS)
def test_op_for_op_variants_equal_the_plain_ones_on_the_exact_grid(act):
    """On the grid of tests/test_instnorm_exact_gpu.py nothing rounds for no activation and ReLU: every variant is the plain
    float64 result, which is an fp32 value.  LeakyReLU's 0.2f v rounds: the variants stay within 2^-23 of the plain result."""
    x, r, g, mean, rstd, s1, s2 = _grid_case(3)
    plain, plain_r = R.forward(x, mean, rstd, act), R.forward(x, mean, rstd, act, r)
    dx, s = R.backward(x, g, mean, rstd, s1, s2, act)
    ops, ops_r, con = R.forward_ops(x, mean, rstd, act), R.forward_ops(x, mean, rstd, act, r), R.forward_contracted(x, mean, rstd, act, r)
    dxo = R.backward_ops(x, g, mean, rstd, s1, s2, act)
    if act != R.ACT_LRELU:
        for v in (plain, plain_r, dx):
            assert torch.equal(R.f32(v), v)
        assert torch.equal(R.bf16(plain), plain) and torch.equal(R.bf16(plain_r), plain_r)
        assert torch.equal(ops, plain) and torch.equal(ops_r, plain_r) and torch.equal(con, plain_r) and torch.equal(dxo, dx)
        assert float(dx.abs().max()) <= 52 and torch.equal(dx * 64, (dx * 64).round())
    else:
        for got, want in ((ops, plain), (ops_r, plain_r), (con, plain_r)):
            assert bool(((got - want).abs() <= 2.0 ** -23 * (want.abs() + 8)).all())
        assert bool(((dxo - dx).abs() <= 2.0 ** -22 * (dx.abs() + s)).all())
        assert torch.equal(R.f32(ops), ops) and torch.equal(R.f32(dxo), dxo)
        pos = R.xhat(x, mean, rstd) > 0
        assert torch.equal(ops[pos], plain[pos]) and bool((ops != plain).any())


def test_op_for_op_variants_round_where_fp32_does():
    """Generic fp32 inputs: the variants equal the same expression evaluated in torch float32 (CPU float32 ops round every step)."""
    gen = torch.Generator().manual_seed(9)
    mk = lambda *s: torch.randn(s, generator=gen)
    x, r, g = mk(2, 5, 7, 4) * 1.7 + 0.3, mk(2, 5, 7, 4), mk(2, 5, 7, 4)
    mean, rstd, s1, s2 = mk(2, 4) * 0.1, mk(2, 4).abs() + 0.5, mk(2, 4) * 0.1, mk(2, 4) * 0.1
    bc = lambda t: t[:, None, None, :]
    xh = (x - bc(mean)) * bc(rstd)
    d = [t.double() for t in (x, r, g, mean, rstd, s1, s2)]
    slope = torch.tensor(0.2, dtype=torch.float32)
    for act in ACTS:
        y = xh if act == R.ACT_NONE else torch.where(xh > 0, xh, torch.zeros_like(xh) if act == R.ACT_RELU else slope * xh)
        assert torch.equal(R.forward_ops(d[0], d[3], d[4], act), y.double())
        assert torch.equal(R.forward_ops(d[0], d[3], d[4], act, d[1]), (y + r).double())
    # the backward holds one FMA, which float32 torch ops cannot express: its result is within half an ulp of the exact one
    dxo = R.backward_ops(d[0], d[2], d[3], d[4], d[5], d[6], R.ACT_NONE)
    t = (g - bc(s1)).double()
    inner = -xh.double() * bc(d[6]) + t
    assert torch.equal(dxo, R.f32(bc(d[4]) * R.f32(inner)))
    assert bool(((R.f32(inner) - inner).abs() <= 2.0 ** -24 * inner.abs()).all())


def test_storage_rounding_once_and_split_pair_planes():
    v = _rand((1000,), 5, 30.0).float().double()
    assert torch.equal(R.store("fp32", v)[0], v)
    assert torch.equal(R.store("bf16", v)[0], v.float().bfloat16().double())
    hi, lo = R.store("pair", v)
    assert torch.equal(hi, v.float().bfloat16().double())
    assert torch.equal(lo, (v.float() - v.float().bfloat16().float()).bfloat16().double())
    assert bool(((R.stored_value("pair", v) - v).abs() <= 2.0 ** -16 * v.abs()).all())
    assert torch.equal(R.stored_value("fp32", v), v)
