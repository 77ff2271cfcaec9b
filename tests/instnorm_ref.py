"""Float64 CPU reference of the InstanceNorm kernel family (csrc/norm_act.hip), written from the C ABI's definition.

Everything is a float64 torch tensor on the CPU, activations NHWC [B, H, W, C], per-(sample, channel) statistics [B, C].

  slab partition   per = ceil(HW / nslabs); slab s owns the row-major pixels [s per, min((s + 1) per, HW)); an empty slab sums
                   to zero (`slab_bounds`).
  partials         [B, nslabs, C, 2].  MODE 0: (sum x, sum x^2).  MODE 1: (sum g m, sum g m xhat) with xhat = (x - mean) rstd,
                   m = act'(xhat) under a STRICT xhat > 0 mask, g = fold(dout) (`partials`, which also returns the sums of the
                   terms' magnitudes and the slabs' pixel counts: the inputs of a summation-error bound).
  finalize         sums over the slabs in double, invHW = the FLOAT32 value 1 / HW, eps = the FLOAT32 value 1e-5f widened to double,
                   var clamped at 0.  Mode 0: (mean, rstd).  Mode 1: the two plain means (`finalize`; the results are float64,
                   the kernels store them rounded once to fp32: `f32`).
  fold             the transpose of F.pad(mode="reflect") for any pad < min(H, W), written with index arithmetic (`fold`).
  forward          act((x - mean) rstd) [+ res]                      (`forward`)
  backward         rstd (g m - s1 - xhat s2)                          (`backward`)
  op for op        `forward_ops` / `backward_ops` round to fp32 exactly where in_fwd_px, chunk_add and in_bwd_px do (fp contract
                   off, one explicit FMA): d = fl(x - mean), xhat = fl(d rstd), LeakyReLU fl(0.2f xhat), fl(. + res); backward
                   gg = g or fl(0.2f g), t = fl(gg - s1), inner = fl(fma(-xhat, s2, t)), dx = fl(rstd inner).  A float32 + - x
                   evaluated in float64 and rounded once is correctly rounded (53 >= 2 * 24 + 2 bits); the FMA is evaluated as
                   the float64 expression -xhat s2 + t (the product is exact in float64) and rounded once.
  storage          once to fp32 / bf16; a split pair holds hi = bf16(v), lo = bf16(v - hi) (`store`, `stored_value`).
                   CAUTION, split-pair backward: in_bwd_px leaves the outer product rstd * inner contractible, and the pair
                   store may take its lo plane from fma(rstd, inner, -hi) = bf16(rstd inner - hi) with the product UNROUNDED,
                   where `backward_ops` + `store("pair", .)` give bf16(fl(rstd inner) - hi).  The two agree whenever
                   rstd inner is an fp32 value -- every rstd of tests/test_instnorm_exact_gpu.py is a power of two.  A case
                   with a general rstd and pair storage has to accept both lo planes.

The LeakyReLU slope is the float32 value 0.2f everywhere (`SLOPE`); `slope=0.2` gives the mathematical function, which is what
tests/test_instnorm_ref.py compares with stock torch.
"""
import numpy as np
import torch

ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2
SLOPE = float(np.float32(0.2))           # LRELU_SLOPE of csrc/common.h as the kernels see it
EPS = float(np.float32(1e-5))            # IN_EPS
F64 = torch.float64


def f32(v):
    """v rounded once to float32, as float64."""
    return v.to(torch.float32).to(F64)


def bf16(v):
    """v (float32-representable) rounded once to bfloat16, as float64."""
    return v.to(torch.float32).to(torch.bfloat16).to(F64)


def inv_hw(hw):
    """The kernels' 1.0f / (float)HW."""
    return float(np.float32(1.0) / np.float32(hw))


# ------------------------------------------------------------------------------------------------------------------ slabs
def slab_bounds(hw, nslabs):
    """[(begin, end)] of every slab; an empty slab has begin == end."""
    assert hw >= 1 and nslabs >= 1
    per = -(-hw // nslabs)
    return [(min(s * per, hw), min((s + 1) * per, hw)) for s in range(nslabs)]


# ------------------------------------------------------------------------------------------------------------------ fold
def _reflect(i, n):
    """Index inside [0, n) that F.pad(mode="reflect") reads for position i of the axis (no edge repeat)."""
    if i < 0:
        i = -i
    if i > n - 1:
        i = 2 * (n - 1) - i
    assert 0 <= i < n, "reflection needs pad < size"
    return i


def fold(g, pad):
    """The transpose of reflection padding: g [B, H + 2 pad, W + 2 pad, C] on the padded grid -> [B, H, W, C], every padded
    position added onto the interior pixel it was copied from."""
    if pad == 0:
        return g.clone()
    b, hp, wp, c = g.shape
    h, w = hp - 2 * pad, wp - 2 * pad
    assert 0 < pad < min(h, w), (pad, h, w)
    rows = torch.tensor([_reflect(j - pad, h) for j in range(hp)])
    cols = torch.tensor([_reflect(i - pad, w) for i in range(wp)])
    t = torch.zeros((b, h, wp, c), dtype=g.dtype).index_add_(1, rows, g)
    return torch.zeros((b, h, w, c), dtype=g.dtype).index_add_(2, cols, t)


# ------------------------------------------------------------------------------------------------------------------ pieces
def _bc(s):
    return s[:, None, None, :]


def xhat(x, mean, rstd):
    return (x - _bc(mean)) * _bc(rstd)


def act_mask(xh, act, slope=SLOPE):
    """act'(xhat): 1 where xhat > 0 (strictly), else 0 (ReLU) / the slope (LeakyReLU)."""
    if act == ACT_RELU:
        return (xh > 0).to(F64)
    if act == ACT_LRELU:
        return torch.where(xh > 0, torch.ones_like(xh), torch.full_like(xh, slope))
    assert act == ACT_NONE, act
    return torch.ones_like(xh)


def act_fwd(xh, act, slope=SLOPE):
    """act(xhat); the zero side of ReLU is +0 as in the kernels (xhat > 0 ? xhat : 0)."""
    if act == ACT_RELU:
        return torch.where(xh > 0, xh, torch.zeros_like(xh))
    if act == ACT_LRELU:
        return torch.where(xh > 0, xh, slope * xh)
    assert act == ACT_NONE, act
    return xh


def act_grad(g, xh, act, slope=SLOPE):
    """g act'(xhat), with +0 where ReLU masks."""
    if act == ACT_RELU:
        return torch.where(xh > 0, g, torch.zeros_like(g))
    return g * act_mask(xh, act, slope)


# ------------------------------------------------------------------------------------------------------------------ statistics
def partials(x, nslabs, mode=0, g=None, mean=None, rstd=None, act=ACT_NONE):
    """(part, mag, count): part [B, nslabs, C, 2] as above, mag the same sums over the terms' magnitudes, count [nslabs] the
    slabs' pixel counts.  `g` is the ALREADY FOLDED gradient on the interior grid."""
    b, h, w, c = x.shape
    if mode == 0:
        t0, t1 = x, x * x
    else:
        xh = xhat(x, mean, rstd)
        t0 = act_grad(g, xh, act)
        t1 = t0 * xh
    t = torch.stack((t0, t1), -1).reshape(b, h * w, c, 2)
    part = torch.zeros((b, nslabs, c, 2), dtype=F64)
    mag = torch.zeros_like(part)
    bounds = slab_bounds(h * w, nslabs)
    for s, (p0, p1) in enumerate(bounds):
        part[:, s] = t[:, p0:p1].sum(1)
        mag[:, s] = t[:, p0:p1].abs().sum(1)
    return part, mag, torch.tensor([p1 - p0 for p0, p1 in bounds])


def finalize(part, hw, mode=0):
    """Mode 0: (mean, rstd); mode 1: the two plain means -- float64 [B, C] each, before the kernels' one rounding to fp32."""
    a = part.to(F64).sum(1)
    inv = inv_hw(hw)
    m = a[..., 0] * inv
    if mode == 1:
        return m, a[..., 1] * inv
    var = (a[..., 1] * inv - m * m).clamp_min(0.0)
    return m, 1.0 / torch.sqrt(var + EPS)


# ------------------------------------------------------------------------------------------------------------------ elementwise
def forward(x, mean, rstd, act, res=None, slope=SLOPE):
    y = act_fwd(xhat(x, mean, rstd), act, slope)
    return y if res is None else y + res


def backward(x, g, mean, rstd, s1, s2, act, slope=SLOPE):
    """dx and S = rstd (|g m| + |s1| + |xhat s2|), the magnitude a per-element rounding bound scales with."""
    xh = xhat(x, mean, rstd)
    gm = act_grad(g, xh, act, slope)
    dx = _bc(rstd) * (gm - _bc(s1) - xh * _bc(s2))
    return dx, _bc(rstd).abs() * (gm.abs() + _bc(s1).abs() + (xh * _bc(s2)).abs())


def xhat_ops(x, mean, rstd):
    """(d, xhat) with the kernels' two roundings: d = fl(x - mean), xhat = fl(d rstd)."""
    d = f32(x - _bc(mean))
    return d, f32(d * _bc(rstd))


def forward_ops(x, mean, rstd, act, res=None):
    """in_fwd_px + chunk_add, rounding for rounding (fp32 result as float64)."""
    _, xh = xhat_ops(x, mean, rstd)
    if act == ACT_RELU:
        y = torch.where(xh > 0, xh, torch.zeros_like(xh))
    elif act == ACT_LRELU:
        y = torch.where(xh > 0, xh, f32(SLOPE * xh))
    else:
        assert act == ACT_NONE, act
        y = xh
    return y if res is None else f32(y + res)


def forward_contracted(x, mean, rstd, act, res):
    """The one other result a kernel WITHOUT the contract pragma may give with a residual: the last product of the activation
    and the residual add fused into one FMA -- fl(d rstd + res) where the activation passes xhat through, fl(0.2f xhat + res) on
    LeakyReLU's negative side (ReLU's zero side has no product: fl(0 + res) = res either way)."""
    d, xh = xhat_ops(x, mean, rstd)
    through = f32(d * _bc(rstd) + res)
    if act == ACT_NONE:
        return through
    if act == ACT_RELU:
        return torch.where(xh > 0, through, res)
    assert act == ACT_LRELU, act
    return torch.where(xh > 0, through, f32(SLOPE * xh + res))


def backward_ops(x, g, mean, rstd, s1, s2, act):
    """in_bwd_px, rounding for rounding (fp32 result as float64)."""
    _, xh = xhat_ops(x, mean, rstd)
    if act == ACT_RELU:
        gg = torch.where(xh > 0, g, torch.zeros_like(g))
    elif act == ACT_LRELU:
        gg = torch.where(xh > 0, g, f32(SLOPE * g))
    else:
        assert act == ACT_NONE, act
        gg = g
    t = f32(gg - _bc(s1))
    inner = f32(-xh * _bc(s2) + t)
    return f32(_bc(rstd) * inner)


# ------------------------------------------------------------------------------------------------------------------ storage
def store(kind, v):
    """The planes a kernel stores for the fp32 value v: (v,) for "fp32", (bf16(v),) for "bf16", (hi, lo) for "pair"."""
    if kind == "fp32":
        return (f32(v),)
    hi = bf16(v)
    if kind == "bf16":
        return (hi,)
    assert kind == "pair", kind
    return hi, bf16(f32(v) - hi)


def stored_value(kind, v):
    """What a buffer of `kind` holds after v was stored: the sum of its planes."""
    return sum(store(kind, v))
