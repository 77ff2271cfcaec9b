"""CPU: tests/conv_ref.py (the reference of tests/test_conv_exact_gpu.py) against torch in float64 -- exact equality on
integer inputs: forward / transposed / backward-data / weight-gradient sums through the tap lists the engine builds, zero
and reflection padding, the parity classes, the reflection fold as the adjoint of F.pad, and the bf16 / split-pair stores."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conv_ref import (ACT_LRELU, ACT_NONE, ACT_RELU, PAD_REFLECT, PAD_ZERO, PAIR_GRANULE, STRIP_PLAN, act_f32,
                      assert_exact_domain, band_plan, band_slabs, conv3x3_f64, conv_classes_ref, conv_pair_ref, conv_taps_ref,
                      convT3x3_f64, convT_classes, epilogue, fold_frame, frame_mask, fused_store_bf16, int_grid, linear_slabs,
                      moments_ref, pack_tap, pad_index, pair_f64, pair_grid, pair_split, place, plan_edges, slab_moments_ref,
                      store_bf16, store_pair, strip_plan, tile_slabs, unpack_tap, wgrad_pair_ref, wgrad_taps_ref)


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _w_taps(w):
    """torch weight [Cout, Cin, kh, kw] -> [kh kw, Cout, Cin]"""
    co, ci, kh, kw = w.shape
    return w.permute(2, 3, 0, 1).reshape(kh * kw, co, ci).contiguous()


def _fwd_taps(k, pad):
    return [pack_tap(ky - pad, kx - pad, ky * k + kx) for ky in range(k) for kx in range(k)]


def test_tap_words_and_class_lists_match_the_engine():
    from cta_gan_amd import ops
    from cta_gan_amd.engine import _convT_classes
    for dy, dx, wi in ((-3, 2, 0), (0, 0, 48), (63, -64, 255)):
        assert pack_tap(dy, dx, wi) == ops.pack_tap(dy, dx, wi) and unpack_tap(pack_tap(dy, dx, wi)) == (dy, dx, wi)
    for k, pad in ((3, 1), (4, 1)):
        assert convT_classes(k, pad) == _convT_classes(k, pad)
    assert (PAD_ZERO, PAD_REFLECT, ACT_NONE, ACT_RELU, ACT_LRELU) == (ops.PAD_ZERO, ops.PAD_REFLECT, ops.ACT_NONE, ops.ACT_RELU,
                                                                      ops.ACT_LRELU)


@pytest.mark.parametrize("k,stride,pad", [(3, 1, 1), (3, 2, 1), (4, 1, 1), (4, 2, 1), (7, 1, 3), (1, 1, 0)],
                         ids=["3x3s1", "3x3s2", "4x4s1", "4x4s2", "7x7", "1x1"])
@pytest.mark.parametrize("size", [(9, 12), (10, 7)], ids=["9x12", "10x7"])
def test_forward_equals_conv2d(k, stride, pad, size):
    rng = np.random.default_rng(k * 10 + stride)
    h, w = size
    x = int_grid(rng, (2, h, w, 5), -3, 3)
    wt = int_grid(rng, (6, 5, k, k), -3, 3)
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    got = conv_taps_ref(x, _w_taps(wt), _fwd_taps(k, pad), ho, wo, stride, PAD_ZERO)
    assert torch.equal(_nchw(got), F.conv2d(_nchw(x), wt, stride=stride, padding=pad))
    s = conv_taps_ref(x.abs(), _w_taps(wt).abs(), _fwd_taps(k, pad), ho, wo, stride, PAD_ZERO)
    assert bool((s >= got.abs()).all())
    assert_exact_domain(s)
    if pad:
        gotr = conv_taps_ref(x, _w_taps(wt), _fwd_taps(k, pad), ho, wo, stride, PAD_REFLECT)
        assert torch.equal(_nchw(gotr), F.conv2d(F.pad(_nchw(x), (pad,) * 4, mode="reflect"), wt, stride=stride))


@pytest.mark.parametrize("size", [(7, 9), (6, 4)], ids=["7x9", "6x4"])
def test_transposed_equals_conv_transpose2d_through_the_four_classes(size):
    rng = np.random.default_rng(3)
    h, w = size
    x = int_grid(rng, (2, h, w, 4), -3, 3)
    wt = int_grid(rng, (4, 6, 3, 3), -3, 3)                       # (Cin, Cout, kh, kw)
    want = F.conv_transpose2d(_nchw(x), wt, stride=2, padding=1, output_padding=1)
    wtaps = wt.permute(2, 3, 1, 0).reshape(9, 6, 4)
    got = conv_classes_ref(x, wtaps, convT_classes(3, 1), h, w, PAD_ZERO)
    assert torch.equal(_nchw(got), want)


@pytest.mark.parametrize("k,stride", [(3, 1), (4, 1), (3, 2), (4, 2)], ids=["3x3s1", "4x4s1", "3x3s2", "4x4s2"])
@pytest.mark.parametrize("size", [(8, 10), (9, 7)], ids=["8x10", "9x7"])
def test_backward_data_equals_autograd(k, stride, size):
    rng = np.random.default_rng(k + stride)
    h, w = size
    x = _nchw(int_grid(rng, (2, h, w, 3), -3, 3)).requires_grad_(True)
    wt = int_grid(rng, (5, 3, k, k), -3, 3)
    y = F.conv2d(x, wt, stride=stride, padding=1)
    g = int_grid(rng, tuple(y.shape), -3, 3)
    y.backward(g)
    gn = _nhwc(g)
    wb = wt.permute(2, 3, 1, 0).reshape(k * k, 3, 5)              # [tap][Cin][Cout]: N = Cin, K = Cout
    if stride == 1:
        taps = [pack_tap(1 - ky, 1 - kx, ky * k + kx) for ky in range(k) for kx in range(k)]
        got = conv_taps_ref(gn, wb, taps, h, w, 1, PAD_ZERO)
    else:
        got = torch.zeros(2, h, w, 3, dtype=torch.float64)
        for py, px, taps in convT_classes(k, 1):
            hs, ws = (h - py + 1) // 2, (w - px + 1) // 2
            place(got, conv_taps_ref(gn, wb, taps, hs, ws, 1, PAD_ZERO), 2, py, px)
    assert torch.equal(_nchw(got), x.grad)


def test_reflect_backward_data_is_frame_plus_interior_plus_fold():
    """Backward-data of ReflectionPad2d(1) + Conv2d(3): the gradient on the padded grid (flipped taps, zero padding; ring =
    the frame launch, interior = the tile-aligned launch), folded: equals autograd's gradient of the unpadded input."""
    rng = np.random.default_rng(8)
    h, w = 6, 9
    x = _nchw(int_grid(rng, (2, h, w, 3), -3, 3)).requires_grad_(True)
    wt = int_grid(rng, (4, 3, 3, 3), -3, 3)
    y = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), wt)
    g = int_grid(rng, tuple(y.shape), -3, 3)
    y.backward(g)
    wb = wt.permute(2, 3, 1, 0).reshape(9, 3, 4)
    taps = [pack_tap(-ky, -kx, ky * 3 + kx) for ky in range(3) for kx in range(3)]
    dxp = conv_taps_ref(_nhwc(g), wb, taps, h + 2, w + 2, 1, PAD_ZERO)
    ring = frame_mask(h + 2, w + 2)
    poisoned = torch.where(ring[None, :, :, None], dxp, torch.full_like(dxp, 777.0))      # the interior is not read
    taps_in = [pack_tap(1 - ky, 1 - kx, ky * 3 + kx) for ky in range(3) for kx in range(3)]
    inner = conv_taps_ref(_nhwc(g), wb, taps_in, h, w, 1, PAD_ZERO)
    assert torch.equal(inner, dxp[:, 1:-1, 1:-1])
    assert torch.equal(_nchw(inner + fold_frame(poisoned)), x.grad)
    assert int(ring.sum()) == 2 * (w + 2) + 2 * h


def test_fold_is_the_adjoint_of_reflection_pad():
    rng = np.random.default_rng(4)
    a = int_grid(rng, (2, 5, 7, 3), -3, 3)
    gp = int_grid(rng, (2, 7, 9, 3), -3, 3)
    ap = _nhwc(F.pad(_nchw(a), (1, 1, 1, 1), mode="reflect"))
    lhs = (ap * gp).sum()
    rhs = (a * (gp[:, 1:-1, 1:-1] + fold_frame(gp))).sum()
    assert float(lhs) == float(rhs)


@pytest.mark.parametrize("k,stride", [(3, 1), (3, 2), (4, 2), (1, 1)], ids=["3x3s1", "3x3s2", "4x4s2", "1x1"])
def test_weight_gradient_equals_conv2d_weight(k, stride):
    rng = np.random.default_rng(20 + k)
    pad = 1 if k > 1 else 0
    h, w = (9, 11) if stride == 1 else (11, 12)
    x = int_grid(rng, (2, h, w, 3), -3, 3)
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    g = int_grid(rng, (2, ho, wo, 5), -3, 3)
    want = torch.nn.grad.conv2d_weight(_nchw(x), (5, 3, k, k), _nchw(g), stride=stride, padding=pad)
    taps = _fwd_taps(k, pad)
    dw, part = wgrad_taps_ref(g, x, taps, stride, PAD_ZERO, slabs=linear_slabs(ho, wo, 16))
    assert torch.equal(dw.view(k, k, 5, 3).permute(2, 3, 0, 1), want)
    assert part.shape[0] == 2 * ((ho * wo + 15) // 16) and torch.equal(part.sum(0), dw)
    dw2, part2 = wgrad_taps_ref(g, x, taps, stride, PAD_ZERO, slabs=tile_slabs(ho, wo, 16))
    assert torch.equal(part2.sum(0), dw) and not torch.equal(part2[0], part[0])
    # a slab's partial is the sum over ITS pixels: only sample 0, rows-major pixels 0 .. 15
    ids, _ = linear_slabs(ho, wo, 16)
    g0 = g.clone()
    g0[1:] = 0
    g0[0][ids != 0] = 0
    assert torch.equal(wgrad_taps_ref(g0, x, taps, stride, PAD_ZERO), part[0])
    if k == 3 and stride == 1:      # reflection padding
        wantr = torch.nn.grad.conv2d_weight(F.pad(_nchw(x), (1, 1, 1, 1), mode="reflect"), (5, 3, 3, 3), _nchw(g))
        assert torch.equal(wgrad_taps_ref(g, x, taps, 1, PAD_REFLECT).view(3, 3, 5, 3).permute(2, 3, 0, 1), wantr)


def test_transposed_weight_gradient_with_the_roles_swapped():
    """ConvTranspose2d(k=3, s=2, p=1, op=1): dW[ci][co][ky][kx] = sum x[ci, q] g[co, 2 q + k - 1] -- the stride-2 weight
    gradient with the layer's INPUT on the small grid in the role of G."""
    rng = np.random.default_rng(9)
    x = _nchw(int_grid(rng, (2, 5, 6, 4), -3, 3))
    wt = int_grid(rng, (4, 3, 3, 3), -3, 3).requires_grad_(True)
    y = F.conv_transpose2d(x, wt, stride=2, padding=1, output_padding=1)
    g = int_grid(rng, tuple(y.shape), -3, 3)
    y.backward(g)
    dw = wgrad_taps_ref(_nhwc(x), _nhwc(g), _fwd_taps(3, 1), 2, PAD_ZERO)      # [t][ci][co]
    assert torch.equal(dw.view(3, 3, 4, 3).permute(2, 3, 0, 1), wt.grad)


def test_pad_index():
    idx = torch.arange(-2, 7)
    r, ok = pad_index(idx, 5, PAD_REFLECT)
    assert r.tolist() == [2, 1, 0, 1, 2, 3, 4, 3, 2] and bool(ok.all())
    r, ok = pad_index(idx, 5, PAD_ZERO)
    assert ok.tolist() == [False, False, True, True, True, True, True, False, False]


def test_store_helpers_equal_torch_bfloat16():
    rng = np.random.default_rng(12)
    v = np.concatenate([rng.standard_normal(4096).astype(np.float32) * 300,
                        np.arange(-5000, 5001).astype(np.float32),
                        np.array([257.0, 258.0, 259.0, 385.0, 387.0, -0.0, 0.0, 1e-30, 3.0e38], dtype=np.float32)])
    t = torch.from_numpy(v)
    assert torch.equal(store_bf16(v).view(torch.int16), t.bfloat16().view(torch.int16))
    hi, lo = store_pair(v)
    assert torch.equal(hi.view(torch.int16), t.bfloat16().view(torch.int16))
    assert torch.equal(lo.view(torch.int16), (t - t.bfloat16().float()).bfloat16().view(torch.int16))
    ints = np.arange(-5000, 5001).astype(np.float32)
    frac = float((store_bf16(ints).float().numpy() != ints).mean())
    assert frac > 0.8      # most integers of the output range are not bf16 values: the output rounding is exercised


def test_pair_grid_splits_exactly():
    rng = np.random.default_rng(13)
    v = pair_grid(rng, (4, 1000))
    hi, lo = pair_split(v)
    assert torch.equal(hi, torch.round(v)) and bool((hi.abs() >= 1).all()) and bool((hi.abs() <= 2).all())
    assert torch.equal(lo, v - hi) and set((lo / PAIR_GRANULE).unique().tolist()) == {-1.0, 0.0, 1.0}
    x = pair_grid(rng, (1, 5, 6, 32))
    w = pair_grid(rng, (9, 8, 32))
    taps = _fwd_taps(3, 1)
    xh, xl = pair_split(x)
    wh, wl = pair_split(w)
    full = conv_taps_ref(x, w, taps, 5, 6, 1, PAD_ZERO)
    assert torch.equal(conv_pair_ref(x, w, taps, 5, 6, 1, PAD_ZERO), full - conv_taps_ref(xl, wl, taps, 5, 6, 1, PAD_ZERO))
    g = pair_grid(rng, (1, 5, 6, 8))
    gh, gl = pair_split(g)
    dw, s = wgrad_pair_ref(g, x, taps, 1, PAD_ZERO)
    assert torch.equal(dw, wgrad_taps_ref(g, x, taps, 1, PAD_ZERO) - wgrad_taps_ref(gl, xl, taps, 1, PAD_ZERO))
    assert bool((s >= dw.abs()).all())


def test_epilogue_in_float32():
    acc = torch.tensor([-7.0, -1.0, 0.0, 3.0, 1001.0], dtype=torch.float64)
    b = torch.tensor([0.125] * 5, dtype=torch.float64)
    v = epilogue(acc, b, ACT_LRELU)
    assert v.dtype == np.float32
    want = F.leaky_relu((acc.float() + b.float()), 0.2)
    assert np.array_equal(v, want.numpy())
    assert np.array_equal(act_f32(np.float32([-2, 0, 2]), ACT_RELU), np.float32([0, 0, 2]))
    # res is added to the ROUNDED result: 257 -> bf16 256, + 1 = 257 -> 256; adding first would give 258
    out = fused_store_bf16(np.full((1, 4, 4, 1), 257.0, dtype=np.float32), res=torch.ones(1, 4, 4, 1, dtype=torch.float64))
    assert float(out[0, 0, 0, 0]) == 256.0
    assert float(store_bf16(np.float32([258.0]))[0]) == 258.0


# ---------------------------------------------------------------------------- helpers of tests/test_strip_exact_gpu.py
# The shapes of tests/test_strip_exact_gpu.py with their plans on 256 compute units, worked out by hand:
# (kernel, B, rows, cols) -> (band_rows, nbands, rows of the last band, nstrips, columns of the last strip)
STRIP_CASES_CU256 = {
    ("strip32", 1024, 32, 32): (32, 1, 32, 2, 16),       # 3072 slots / 2048 strips = 1 band
    ("strip32", 64, 65, 255): (32, 3, 1, 16, 15),        # 3072 / 1024 = 3 bands of ceil(65 / 3) = 22 -> 32 rows
    ("strip32", 64, 70, 255): (32, 3, 6, 16, 15),
    ("strip32", 61, 67, 257): (34, 2, 33, 17, 1),        # 3072 / 1037 = 2 bands of 34
    ("strip32", 8, 3972, 33): (32, 125, 4, 3, 1),        # 3072 / 24 = 128 bands of ceil(3972 / 128) = 32 rows
    ("strip32p", 1024, 32, 32): (32, 1, 32, 2, 16),
    ("strip32p", 64, 65, 255): (33, 2, 32, 16, 15),      # 2048 / 1024 = 2 bands of 33
    ("strip32p", 61, 67, 257): (67, 1, 67, 17, 1),       # 2048 / 1037 = 1 band
    ("stript", 1024, 16, 16): (16, 1, 16, 1, 16),
    ("stript", 908, 17, 17): (17, 1, 17, 2, 1),
    ("stript", 8, 133, 250): (34, 4, 31, 16, 10),        # 512 / 128 = 4 bands of 34
    ("striptp", 1024, 16, 16): (16, 1, 16, 1, 16),
    ("striptp", 908, 17, 17): (17, 1, 17, 2, 1),
    ("striptp", 8, 133, 250): (67, 2, 66, 16, 10),       # 256 / 128 = 2 bands of 67
    ("strips2", 2048, 8, 16): (8, 1, 8, 1, 16),
    ("strips2", 1821, 9, 16): (9, 1, 9, 1, 16),
    ("strips2", 8, 131, 256): (33, 4, 32, 16, 16),       # 512 / 128 = 4 bands of 33
    ("strips2p", 2048, 8, 16): (8, 1, 8, 1, 16),
    ("strips2p", 8, 131, 256): (66, 2, 65, 16, 16),      # 256 / 128 = 2 bands of 66
    ("strips2w", 1024, 8, 16): (8, 1, 8, 1, 16),
    ("strips2w", 911, 9, 16): (9, 1, 9, 1, 16),
    ("strips2w", 8, 129, 128): (65, 2, 64, 8, 16),       # 256 / (2 x 64) = 2 bands of 65
}


def test_band_plan_mirror_reproduces_the_hand_computed_plans():
    """band_plan / strip_plan against the plans worked out by hand for 256 compute units (the table the GPU cases were chosen
    from), and against a literal transcription of csrc/conv_dispatch.h on a sweep."""
    assert set(k for k, _, _, _ in STRIP_CASES_CU256) == set(STRIP_PLAN)
    for (kernel, b, rows, cols), want in STRIP_CASES_CU256.items():
        assert strip_plan(kernel, 256, b, rows, cols) == want, (kernel, b, rows, cols)
    # the GPU module's own case lists are these shapes, and on 256 compute units each meets the edge it is named for
    import test_strip_exact_gpu as gpu
    cases = [("strip32", c["b"], c["h"], c["w"], c["edge"]) for c in gpu.STRIP32.values()]
    cases += [("strip32p", c["b"], c["h"], c["w"], c["edge"]) for c in gpu.STRIP32P.values()]
    cases += [(c["kernel"], c["b"], c["rows"], c["cols"], c["edge"]) for d in (gpu.STRIDED, gpu.STRIDED_PAIR) for c in d.values()]
    assert set(c[:4] for c in cases) == set(STRIP_CASES_CU256)
    for kernel, b, rows, cols, edge in cases:
        assert edge(gpu.Plan(*STRIP_CASES_CU256[(kernel, b, rows, cols)]), b), (kernel, b, rows, cols)

    def c_plan(rows, min_band, slots, strips):
        nb = slots // strips
        if nb < 1:
            nb = 1
        band = (rows + nb - 1) // nb
        if band < min_band:
            band = min_band
        return band, (rows + band - 1) // band
    for rows in (8, 9, 31, 32, 33, 65, 133, 512, 3972):
        for min_band in (8, 16, 32):
            for slots in (104, 256, 512, 3072):
                for strips in (1, 24, 128, 1037, 4096):
                    band, nbands = band_plan(rows, min_band, slots, strips)
                    assert (band, nbands) == c_plan(rows, min_band, slots, strips)
                    assert band >= min_band and (nbands - 1) * band < rows <= nbands * band
    assert band_plan(512, 32, 3072, 512) == (86, 6) and band_plan(65, 32, 3072, 1024) == (32, 3)
    assert plan_edges(65, 255, 32) == (32, 3, 1, 16, 15) and plan_edges(64, 256, 32) == (32, 2, 32, 16, 16)


@pytest.mark.parametrize("grid", [(65, 255, 32, 1), (67, 257, 34, 1), (32, 32, 32, 1), (17, 17, 17, 2), (133, 250, 34, 2), (9, 16, 9, 1)],
                         ids=["65x255", "67x257", "32x32", "T17x17", "T133x250", "9x16"])
def test_band_slabs_partition_the_grid(grid):
    rows, cols, band, os_ = grid
    ids, cnt = band_slabs(rows, cols, band, os_)
    _, nbands, last_rows, nstrips, last_cols = plan_edges(rows, cols, band)
    assert tuple(ids.shape) == (rows * os_, cols * os_) and cnt == nbands * nstrips
    size = torch.bincount(ids.reshape(-1), minlength=cnt)
    assert int(size.sum()) == rows * cols * os_ * os_ and int(size.min()) > 0 and int(ids.min()) == 0 and int(ids.max()) == cnt - 1
    for band_i in range(nbands):
        for strip in range(nstrips):
            r = last_rows if band_i == nbands - 1 else band
            c = last_cols if strip == nstrips - 1 else 16
            assert int(size[band_i * nstrips + strip]) == r * c * os_ * os_
            # a slab is ONE rectangle: rows of band band_i, columns of strip `strip` (x os: the four classes of its grid pixels)
            blk = ids[band_i * band * os_:(band_i * band + r) * os_, strip * 16 * os_:(strip * 16 + c) * os_]
            assert bool((blk == band_i * nstrips + strip).all())
    # per-slab moments sum to the whole-sample moments, and a slab's moments are those of its pixels alone
    rng = np.random.default_rng(rows)
    acc = int_grid(rng, (2, rows * os_, cols * os_, 3), -50, 50)
    sm = slab_moments_ref(acc, (ids, cnt))
    assert torch.equal(sm.sum(1), moments_ref(acc))
    only = torch.where((ids == cnt - 1)[None, :, :, None], acc, torch.zeros_like(acc))
    assert torch.equal(sm[:, cnt - 1], moments_ref(only))


@pytest.mark.parametrize("flipped", [False, True], ids=["forward", "flipped"])
@pytest.mark.parametrize("pad_mode", [PAD_ZERO, PAD_REFLECT], ids=["zero", "reflect"])
def test_conv3x3_f64_equals_conv_taps_ref(flipped, pad_mode):
    rng = np.random.default_rng(31)
    x = int_grid(rng, (3, 7, 18, 8), -4, 4)
    w = int_grid(rng, (9, 6, 8), -4, 4)
    taps = [pack_tap(1 - ky, 1 - kx, ky * 3 + kx) if flipped else pack_tap(ky - 1, kx - 1, ky * 3 + kx)
            for ky in range(3) for kx in range(3)]
    assert torch.equal(conv3x3_f64(x, w, flipped, pad_mode, chunk=2), conv_taps_ref(x, w, taps, 7, 18, 1, pad_mode))


def test_strided_transposed_and_pair_f64_wrappers_equal_the_tap_references():
    rng = np.random.default_rng(32)
    x = int_grid(rng, (3, 10, 12, 8), -3, 3)
    w = int_grid(rng, (9, 6, 8), -3, 3)
    assert torch.equal(conv3x3_f64(x, w, stride=2, chunk=2), conv_taps_ref(x, w, _fwd_taps(3, 1), 5, 6, 2, PAD_ZERO))
    xt = int_grid(rng, (3, 5, 7, 8), -3, 3)
    assert torch.equal(convT3x3_f64(xt, w, chunk=2), conv_classes_ref(xt, w, convT_classes(3, 1), 5, 7, PAD_ZERO))
    xp, wp, xtp = pair_grid(rng, (2, 10, 12, 32)), pair_grid(rng, (9, 8, 32)), pair_grid(rng, (2, 5, 7, 32))
    flip = [pack_tap(1 - ky, 1 - kx, ky * 3 + kx) for ky in range(3) for kx in range(3)]
    assert torch.equal(pair_f64(conv3x3_f64, xp, wp, flipped=True, pad_mode=PAD_REFLECT), conv_pair_ref(xp, wp, flip, 10, 12, 1, PAD_REFLECT))
    assert torch.equal(pair_f64(conv3x3_f64, xp, wp, stride=2), conv_pair_ref(xp, wp, _fwd_taps(3, 1), 5, 6, 2, PAD_ZERO))
    want = torch.zeros(2, 10, 14, 8, dtype=torch.float64)
    for py, px, taps in convT_classes(3, 1):
        place(want, conv_pair_ref(xtp, wp, taps, 5, 7, 1, PAD_ZERO), 2, py, px)
    assert torch.equal(pair_f64(convT3x3_f64, xtp, wp), want)
