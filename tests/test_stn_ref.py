"""CPU: tests/stn_ref.py (the warp reference of test_loss_stn_gpu.py) against the float32 torch restatement of the reference
program's transformer, and the reason a float64 torch oracle cannot stand in for it.

Bounds: forward and d_src within 2^-20 (|want| + S) per element (torch's float32 weights, products and sums against the float64
ones: a few float32 roundings each, more at a destination many samples pile up on); d_flow within 1e-5 (1 + S) for EVERY element
-- one sample on another cell would differ by a neighbour difference of src, O(1) -- so the cells floor() picks agree everywhere.
"""
import pytest
import torch

from oracle import ref_models
from stn_ref import warp_ref

SHAPES = [(37, 53), (40, 40), (5, 7), (96, 80), (2, 3), (2, 2), (33, 2)]
SCALES = [0.0, 1e-5, 1e-3, 3.0, 50.0]


def _inputs(h, w, scale, seed, b=2):
    gen = torch.Generator().manual_seed(seed)
    src = torch.randn(b, 1, h, w, generator=gen)
    flow = scale * torch.randn(b, 2, h, w, generator=gen)
    gout = torch.randn(b, 1, h, w, generator=gen)
    return src, flow, gout


def _torch_warp(src, flow, gout, dtype):
    s = src.to(dtype).requires_grad_(True)
    f = flow.to(dtype).requires_grad_(True)
    out = ref_models.Transformer_2D()(s, f)
    d_src, d_flow = torch.autograd.grad(out, (s, f), gout.to(dtype))
    return out.detach().double(), d_src.double(), d_flow.double()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_warp_ref_agrees_with_float32_torch_in_every_pixel(shape):
    h, w = shape
    worst = {"out": 0.0, "d_src": 0.0, "d_flow": 0.0}
    for n, scale in enumerate(SCALES):
        src, flow, gout = _inputs(h, w, scale, 100 * h + w + n)
        res = warp_ref(src, flow, gout)
        got, S = dict(zip(("out", "d_src", "d_flow"), res[:3])), res[4]
        want = dict(zip(("out", "d_src", "d_flow"), _torch_warp(src, flow, gout, torch.float32)))
        for name in ("out", "d_src", "d_flow"):
            err = (got[name] - want[name]).abs()
            bound = 1e-5 * (1.0 + S[name]) if name == "d_flow" else 2.0 ** -20 * (want[name].abs() + S[name])
            frac = float((err / bound.clamp_min(1e-300)).max()) if bool((bound > 0).any()) else 0.0
            worst[name] = max(worst[name], frac)
            bad = err > bound
            assert not bool(bad.any()), "%s %dx%d scale %g: %d of %d elements out of bound, max error %.3g" % (
                name, h, w, scale, int(bad.sum()), bad.numel(), float(err.max()))
    print("maxerr warp_ref %dx%d " % shape + " ".join("%s %.3g" % kv for kv in worst.items()) + " of the bound")


def test_warp_ref_counts_and_border():
    """A flow that sends every sample of a column far to the right: the whole column lands on x = W - 1, whose x1 == W neighbour
    does not exist: only that column receives anything (one or two rows per sample), and nothing is lost: sum d_src = sum gout."""
    src, flow, gout = _inputs(6, 5, 0.0, 7, b=1)
    flow[:, 1] = 100.0
    out, d_src, d_flow, k, S = warp_ref(src, flow, gout)
    assert float((out[0, 0] - src[0, 0, :, -1:].double()).abs().max()) < 1e-5
    assert float(d_flow[:, 1].abs().max()) == 0.0            # clipped: multiplier 0
    assert float(k[0, 0, :, :-1].max()) == 0.0 and 6 * 5 <= float(k.sum()) <= 6 * 5 * 2 - 5
    assert abs(float(d_src.sum()) - float(gout.double().sum())) < 1e-12


def test_float64_grid_sample_picks_other_cells_at_zero_flow():
    """Why the GPU tests use warp_ref and not torch in float64: at flow = 0 (40 x 40) the coordinates are integers up to rounding,
    float64 rounds them to other sides than float32 does, and d_flow -- a neighbour difference of src -- differs by more than
    1e-4 at more than 5 % of the pixels (36 % measured with these inputs)."""
    src, flow, gout = _inputs(40, 40, 0.0, 3)
    d32 = _torch_warp(src, flow, gout, torch.float32)[2]
    d64 = _torch_warp(src, flow, gout, torch.float64)[2]
    frac = float(((d32 - d64).abs() > 1e-4).any(1).double().mean())
    print("float64 vs float32 grid_sample: d_flow differs at %.1f %% of the pixels" % (100 * frac))
    assert frac > 0.05
