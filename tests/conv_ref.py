"""Plain reference of the convolution family, written at the level of the C ABI's own definition (include/ctagan_hip.h):

    Y[n, j*os+oy0, i*os+ox0, co] = act(bias[co] + sum_t sum_ci X[n, pad(j*is+dy_t), pad(i*is+dx_t), ci] * W[t][co][ci])
    part[z][t][m][c]             = sum over slab z of G[n, j, i, m] * X[n, pad(j*is+dy_t), pad(i*is+dx_t), c]

for the tests of csrc/conv_igemm.hip, conv_halo.h, conv_wgrad.hip, conv_small.hip, corr_small.hip, conv_tail.hip and
conv_cout1.hip (tests/test_conv_exact_gpu.py), of the sliding-window kernels csrc/conv_strip*.h (tests/test_strip_exact_gpu.py:
the band plan, the per-slab moments and the float64 torch wrappers for their large shapes are at the end of this file) and its
own check against torch (tests/test_conv_ref.py).

The accumulators are float64.  On INTEGER-GRID operands (small integers, or integers plus multiples of 2^-10 for the
split-pair mode) every product and every partial sum is a multiple of the grid's granule; while the sum of the terms'
magnitudes S stays below 2^24 granules, float32 accumulation is exact in any order -- on the matrix cores or on the vector
ALUs -- and a kernel has to reproduce these accumulators bit for bit.  `assert_exact_domain` checks that condition; the same
functions called with abs() operands return S.

The epilogue (bias, activation) is evaluated in numpy float32, spelled as act_apply spells it in csrc/common.h, and the
result is stored as the kernels store it: fp32 as is, bf16 by round-to-nearest-even, or as a split pair hi = bf16(v),
lo = bf16(v - hi).
"""
import numpy as np
import torch

PAD_ZERO, PAD_REFLECT = 0, 1
ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH = 0, 1, 2, 3
PAIR_GRANULE = 2.0 ** -10


# ---------------------------------------------------------------------------- operands
def int_grid(rng, shape, lo, hi):
    """float64 tensor of integers drawn uniformly from [lo, hi]."""
    return torch.from_numpy(rng.integers(lo, hi + 1, size=tuple(shape)).astype(np.float64))


def pair_grid(rng, shape):
    """Split-pair operands: a non-zero integer of magnitude <= 2 plus {-1, 0, 1} * 2^-10.  bf16 rounding of such a value gives
    hi = the integer (2^-10 is below half an ulp of 1 and of 2) and lo = the 2^-10 term, both exact."""
    k = rng.integers(1, 3, size=tuple(shape)) * rng.choice(np.array([-1, 1]), size=tuple(shape))
    e = rng.integers(-1, 2, size=tuple(shape))
    return torch.from_numpy(k.astype(np.float64) + e.astype(np.float64) * PAIR_GRANULE)


def pair_split(v):
    """(hi, lo) float64 planes of a float64 tensor whose values fp32 holds exactly: hi = bf16(v), lo = bf16(v - hi)."""
    hi, lo = store_pair(v.numpy().astype(np.float32))
    return hi.double(), lo.double()


def bias_grid(rng, n):
    """Biases: multiples of 1/8 in [-2, 2]."""
    return torch.from_numpy(rng.integers(-16, 17, size=(n,)).astype(np.float64) / 8.0)


def assert_exact_domain(s, granule=1.0):
    """`s` = sum of the magnitudes of the terms of every accumulator: below 2^24 granules every fp32 partial sum is exact."""
    m = float(torch.as_tensor(s).max()) / granule
    assert m < 2 ** 24, "not an exact case: sum of |terms| = %g granules >= 2^24" % m
    return m


# ---------------------------------------------------------------------------- taps, padding
def pack_tap(dy, dx, widx):
    return (dy + 64) | ((dx + 64) << 8) | (widx << 16)


def unpack_tap(tw):
    return (tw & 0xff) - 64, ((tw >> 8) & 0xff) - 64, tw >> 16


def pad_index(idx, n, pad_mode):
    """Source index and validity of the coordinates `idx` (a LongTensor) on an axis of n pixels: zero padding marks the
    coordinates outside [0, n) invalid; reflection mirrors once about the first / last pixel (the ABI allows no more)."""
    if pad_mode == PAD_REFLECT:
        r = torch.where(idx < 0, -idx, idx)
        r = torch.where(r >= n, 2 * (n - 1) - r, r)
        assert int(r.min()) >= 0 and int(r.max()) < n, "more than a single reflection"
        return r, torch.ones_like(idx, dtype=torch.bool)
    ok = (idx >= 0) & (idx < n)
    return idx.clamp(0, n - 1), ok


def _gather(x, dy, dx, hs, ws, is_, pad_mode):
    """x[n, pad(j*is+dy), pad(i*is+dx), :] for (j, i) in hs x ws, zero where the padding says so."""
    hi, wi = x.shape[1], x.shape[2]
    iy, oky = pad_index(torch.arange(hs) * is_ + dy, hi, pad_mode)
    ix, okx = pad_index(torch.arange(ws) * is_ + dx, wi, pad_mode)
    v = x[:, iy][:, :, ix]
    return v * (oky[:, None] & okx[None, :])[None, :, :, None].to(v.dtype)


def conv_taps_ref(x, w, taps, hs, ws, is_, pad_mode):
    """float64 accumulators [B, hs, ws, Cout] of the ABI's sum.  x: NHWC [B, Hi, Wi, Cin]; w: [slices, Cout, Cin], a tap word
    selects its slice.  With abs() operands the result is S = the sum of the terms' magnitudes."""
    x, w = x.double(), w.double()
    acc = torch.zeros(x.shape[0], hs, ws, w.shape[1], dtype=torch.float64)
    for tw in taps:
        dy, dx, wi_ = unpack_tap(tw)
        acc += _gather(x, dy, dx, hs, ws, is_, pad_mode) @ w[wi_].t()
    return acc


def conv_pair_ref(x, w, taps, hs, ws, is_, pad_mode):
    """Split-pair contraction as the ABI states it: x_hi.w_hi + x_hi.w_lo + x_lo.w_hi (x_lo.w_lo is dropped)."""
    xh, xl = pair_split(x)
    wh, wl = pair_split(w)
    return conv_taps_ref(xh, wh, taps, hs, ws, is_, pad_mode) + conv_taps_ref(xh, wl, taps, hs, ws, is_, pad_mode) \
        + conv_taps_ref(xl, wh, taps, hs, ws, is_, pad_mode)


def conv_pair_s(x, w, taps, hs, ws, is_, pad_mode):
    xh, xl = (t.abs() for t in pair_split(x))
    wh, wl = (t.abs() for t in pair_split(w))
    return conv_taps_ref(xh, wh + wl, taps, hs, ws, is_, pad_mode) + conv_taps_ref(xl, wh, taps, hs, ws, is_, pad_mode)


# ---------------------------------------------------------------------------- placement
def place(full, sub, os_, oy0, ox0):
    """Write the [B, hs, ws, C] sub-grid result into full[:, j*os+oy0, i*os+ox0, :C]."""
    hs, ws, c = sub.shape[1], sub.shape[2], sub.shape[3]
    full[:, oy0:oy0 + (hs - 1) * os_ + 1:os_, ox0:ox0 + (ws - 1) * os_ + 1:os_, :c] = sub
    return full


def frame_mask(hs, ws):
    """The pixel set of a frame launch: the 1-pixel ring of the hs x ws grid."""
    m = torch.zeros(hs, ws, dtype=torch.bool)
    m[0, :] = m[-1, :] = True
    m[:, 0] = m[:, -1] = True
    return m


def convT_classes(k, pad):
    """Parity classes of a stride-2 transposed conv, out[2j+py, 2i+px] = sum in[j+dy, i+dx] * W[ky, kx]: [(py, px, taps)].
    Derived here from the definition (ky = parity + pad - 2 d); tests/test_conv_ref.py ties it to engine._convT_classes."""
    def one(par):
        return [(ky, (par + pad - ky) // 2) for ky in range(k) if (par + pad - ky) % 2 == 0]
    return [(py, px, [pack_tap(dy, dx, ky * k + kx) for ky, dy in one(py) for kx, dx in one(px)])
            for py in (0, 1) for px in (0, 1)]


def conv_classes_ref(x, w, classes, hs, ws, pad_mode):
    """[B, 2 hs, 2 ws, Cout] accumulators of the four classes, each placed at its (py, px)."""
    full = torch.zeros(x.shape[0], 2 * hs, 2 * ws, w.shape[1], dtype=torch.float64)
    for py, px, taps in classes:
        place(full, conv_taps_ref(x, w, taps, hs, ws, 1, pad_mode), 2, py, px)
    return full


def fold_frame(fold):
    """What the `fold` epilogue adds: the frame of a [B, H+2, W+2, C] gradient on the 1-pixel reflection-padded grid, each
    frame pixel added to the interior pixel it mirrors -- [B, H, W, C]; the interior of `fold` is not read."""
    b, hp, wp, c = fold.shape
    h, w = hp - 2, wp - 2
    out = torch.zeros(b, h, w, c, dtype=fold.dtype)
    out[:, 1] += fold[:, 0, 1:-1]
    out[:, h - 2] += fold[:, hp - 1, 1:-1]
    out[:, :, 1] += fold[:, 1:-1, 0]
    out[:, :, w - 2] += fold[:, 1:-1, wp - 1]
    for ey, oy in ((0, 1), (hp - 1, h - 2)):
        for ex, ox in ((0, 1), (wp - 1, w - 2)):
            out[:, oy, ox] += fold[:, ey, ex]
    return out


# ---------------------------------------------------------------------------- weight gradient
def linear_slabs(hs, ws, slab):
    """Slab of every pixel for the per-tap kernel: runs of `slab` pixels in row-major order.  -> ([hs, ws] ids, count)"""
    ids = (torch.arange(hs * ws) // slab).view(hs, ws)
    return ids, (hs * ws + slab - 1) // slab


def tile_slabs(hs, ws, slab):
    """Slab of every pixel for the halo-resident kernels: 8 x 16 pixel tiles in row-major order, dealt in runs of
    ceil(tiles / sps) tiles to the sps = ceil(hs ws / slab) slabs."""
    sps = (hs * ws + slab - 1) // slab
    tx, ty = (ws + 15) // 16, (hs + 7) // 8
    per = (tx * ty + sps - 1) // sps
    tile = (torch.arange(hs)[:, None] // 8) * tx + torch.arange(ws)[None, :] // 16
    return tile // per, sps


def wgrad_taps_ref(g, x, taps, is_, pad_mode, slabs=None):
    """dw[t][m][c] = sum_pixels g[n, j, i, m] * x[n, pad(is j + dy_t), pad(is i + dx_t), c] in float64; t counts the tap LIST
    (a weight gradient has one slice per tap).  slabs = (ids [hs, ws], count): the per-slab partials [B * count, T, M, C] as
    well, in the order ops.conv_wgrad hands them to the reduce (sample-major).  abs() operands give S."""
    g, x = g.double(), x.double()
    b, hs, ws, m = g.shape
    c = x.shape[3]
    dw = torch.zeros(len(taps), m, c, dtype=torch.float64)
    part = None
    if slabs is not None:
        ids, cnt = slabs
        part = torch.zeros(b, cnt, len(taps), m, c, dtype=torch.float64)
        onehot = torch.nn.functional.one_hot(ids.reshape(-1), cnt).double()      # [hs ws, cnt]
    for t, tw in enumerate(taps):
        dy, dx, _ = unpack_tap(tw)
        xg = _gather(x, dy, dx, hs, ws, is_, pad_mode)
        dw[t] += g.reshape(-1, m).t() @ xg.reshape(-1, c)
        if part is not None:
            # [b, s, m, c] = sum_p onehot[p, s] g[b, p, m] xg[b, p, c]
            gs = g.reshape(b, hs * ws, 1, m) * onehot[None, :, :, None]
            part[:, :, t] += torch.einsum("bpsm,bpc->bsmc", gs, xg.reshape(b, hs * ws, c))
    if part is not None:
        return dw, part.reshape(b * cnt, len(taps), m, c)
    return dw


def wgrad_pair_ref(g, x, taps, is_, pad_mode):
    """g_hi x_hi + g_hi x_lo + g_lo x_hi (and its S)."""
    gh, gl = pair_split(g)
    xh, xl = pair_split(x)
    dw = wgrad_taps_ref(gh, xh + xl, taps, is_, pad_mode) + wgrad_taps_ref(gl, xh, taps, is_, pad_mode)
    s = wgrad_taps_ref(gh.abs(), xh.abs() + xl.abs(), taps, is_, pad_mode) + wgrad_taps_ref(gl.abs(), xh.abs(), taps, is_, pad_mode)
    return dw, s


# ---------------------------------------------------------------------------- epilogue and stores
def _f32(t):
    a = t.numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    a32 = a.astype(np.float32)
    assert np.array_equal(a32.astype(np.float64), a.astype(np.float64)), "accumulator is not an fp32 value"
    return a32


def act_f32(v, act):
    """act_apply of csrc/common.h in numpy float32 (tanh is not bit-reproducible: see tanh_ref)."""
    assert v.dtype == np.float32
    if act == ACT_RELU:
        return np.where(v > np.float32(0), v, np.float32(0)).astype(np.float32)
    if act == ACT_LRELU:
        return np.where(v > np.float32(0), v, (np.float32(0.2) * v).astype(np.float32)).astype(np.float32)
    assert act == ACT_NONE
    return v


def epilogue(acc, bias=None, act=ACT_NONE):
    """float32 numpy: act(acc + bias[co]), one rounded operation at a time."""
    v = _f32(acc)
    if bias is not None:
        v = (v + _f32(bias)).astype(np.float32)
    return act_f32(v, act)


def tanh_ref(acc, bias=None):
    """float64 tanh of the exact pre-activation."""
    v = acc.double()
    return torch.tanh(v + bias.double() if bias is not None else v)


def store_bf16(v):
    """float32 numpy -> torch.bfloat16 by round-to-nearest-even on the bits (finite values)."""
    assert v.dtype == np.float32
    u = np.ascontiguousarray(v).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return torch.from_numpy(r.view(np.int16).copy()).view(torch.bfloat16).reshape(v.shape)


def store_f32(v):
    assert v.dtype == np.float32
    return torch.from_numpy(np.ascontiguousarray(v))


def store_pair(v):
    """float32 numpy -> (hi, lo) bfloat16 planes: hi = bf16(v), lo = bf16(v - hi), as ops.to_pair / the pair epilogues do."""
    hi = store_bf16(v)
    lo = store_bf16((v - hi.float().numpy()).astype(np.float32))
    return hi, lo


def fused_store_bf16(v, res=None, fold=None):
    """The residual / fold epilogue of ctg_conv_igemm in the order csrc/conv_halo.h applies it (bf16): the conv result is
    ROUNDED to bf16 first, then res and the folded frame are added in fp32 and the sum is rounded again."""
    f = store_bf16(v).float().numpy()
    if res is not None:
        f = (f + _f32(res)).astype(np.float32)
    if fold is not None:
        f = (f + _f32(fold_frame(fold.double()))).astype(np.float32)
    return store_bf16(f)


def fused_store_f32(v, res=None, fold=None):
    f = v
    if res is not None:
        f = (f + _f32(res)).astype(np.float32)
    if fold is not None:
        f = (f + _f32(fold_frame(fold.double()))).astype(np.float32)
    return store_f32(f)


def moments_ref(acc):
    """Exact (sum, sum of squares) per (sample, channel) of the accumulators [B, H, W, C] -> [B, C, 2] float64."""
    a = acc.double()
    return torch.stack([a.sum((1, 2)), (a * a).sum((1, 2))], dim=-1)


def first_diff(got, want):
    """Index, got and want of the first differing element (for failure messages), or None."""
    ne = (got != want) if got.dtype == want.dtype else (got.double() != want.double())
    if not bool(ne.any()):
        return None
    idx = tuple(int(i) for i in ne.nonzero()[0])
    return idx, float(got[idx]), float(want[idx]), int(ne.sum())


# ---------------------------------------------------------------------------- sliding-window ("strip") kernels
def band_plan(rows, min_band, slots, strips):
    """Mirror of band_plan in csrc/conv_dispatch.h with band_env = 0: as many bands per strip as fill `slots` once over `strips`
    strips, but no band shorter than min_band.  -> (band_rows, nbands)"""
    nb = max(1, slots // strips)
    band = max((rows + nb - 1) // nb, min_band)
    return band, (rows + band - 1) // band


def plan_edges(rows, cols, band_rows):
    """(band_rows, nbands, rows of the last band, nstrips, columns of the last strip) of a rows x cols grid cut into bands of
    band_rows rows and strips of 16 columns."""
    nbands, nstrips = (rows + band_rows - 1) // band_rows, (cols + 15) // 16
    return band_rows, nbands, rows - (nbands - 1) * band_rows, nstrips, cols - (nstrips - 1) * 16


def band_slabs(rows, cols, band_rows, os_=1):
    """Slab of every OUTPUT pixel of a strip kernel: slab = band * nstrips + strip, one band x one 16-column strip of the
    rows x cols grid the kernel walks.  os_ = 2 (the transposed kernels: the grid is the INPUT's): the four parity classes of a
    grid pixel -- output pixels (2 j + py, 2 i + px) -- lie in the slab of (j, i).  -> ([os rows, os cols] ids, count)"""
    nbands, nstrips = (rows + band_rows - 1) // band_rows, (cols + 15) // 16
    j, i = torch.arange(rows * os_) // os_, torch.arange(cols * os_) // os_
    return (j[:, None] // band_rows) * nstrips + i[None, :] // 16, nbands * nstrips


def slab_moments_ref(acc, slabs):
    """Exact per-slab (sum, sum of squares) of the accumulators [B, H, W, C] -> [B, count, C, 2] float64; slabs = band_slabs()."""
    ids, cnt = slabs
    a = acc.double()
    b, h, w, c = a.shape
    assert tuple(ids.shape) == (h, w)
    out = torch.zeros(b, cnt, c, 2, dtype=torch.float64)
    flat = a.reshape(b, h * w, c)
    idx = ids.reshape(-1)
    out[..., 0].index_add_(1, idx, flat)
    out[..., 1].index_add_(1, idx, flat * flat)
    return out


def _chunks(n, chunk):
    return [(s, min(n, s + chunk)) for s in range(0, n, chunk)]


def conv3x3_f64(x, w, flipped=False, pad_mode=PAD_ZERO, stride=1, chunk=16):
    """float64 torch conv2d over explicitly padded input, for the large shapes of the strip kernels: the ABI's sum for the nine
    taps of a 3x3 window in forward order (tap ky*3+kx reads x[s j + ky - 1, s i + kx - 1]) or flipped (backward-data: tap
    ky*3+kx reads x[j + 1 - ky, i + 1 - kx]), slice t of w [9, Cout, Cin] for tap t.  x NHWC [B, H, W, Cin] -> [B, Ho, Wo, Cout],
    `chunk` samples at a time.  Equals conv_taps_ref (tests/test_conv_ref.py)."""
    x, w = x.double(), w.double()
    co, ci = w.shape[1], w.shape[2]
    wt = w.view(3, 3, co, ci)
    if flipped:
        wt = wt.flip(0, 1)
    wt = wt.permute(2, 3, 0, 1).contiguous()
    out = []
    for s, e in _chunks(x.shape[0], chunk):
        xp = torch.nn.functional.pad(x[s:e].permute(0, 3, 1, 2), (1, 1, 1, 1), mode="reflect" if pad_mode == PAD_REFLECT else "constant")
        out.append(torch.nn.functional.conv2d(xp, wt, stride=stride).permute(0, 2, 3, 1))
    return torch.cat(out).contiguous()


def convT3x3_f64(x, w, chunk=16):
    """float64 ConvTranspose2d(k 3, stride 2, padding 1, output_padding 1): slice ky*3+kx of w [9, Cout, Cin] is the layer's
    weight[ci][co][ky][kx].  x NHWC [B, H, W, Cin] -> [B, 2 H, 2 W, Cout].  Equals conv_classes_ref with convT_classes(3, 1)."""
    x, w = x.double(), w.double()
    wt = w.view(3, 3, w.shape[1], w.shape[2]).permute(3, 2, 0, 1).contiguous()
    out = [torch.nn.functional.conv_transpose2d(x[s:e].permute(0, 3, 1, 2), wt, stride=2, padding=1, output_padding=1).permute(0, 2, 3, 1)
           for s, e in _chunks(x.shape[0], chunk)]
    return torch.cat(out).contiguous()


def pair_f64(conv, x, w, parts=None, **kw):
    """The split-pair contraction x_hi.w_hi + x_hi.w_lo + x_lo.w_hi through one of the float64 wrappers above (two passes:
    x_hi with w_hi + w_lo, x_lo with w_hi -- every term exact in float64).  Equals conv_pair_ref.  parts: (x_hi, x_lo) where the
    caller has them already."""
    xh, xl = parts if parts is not None else pair_split(x)
    wh, wl = pair_split(w)
    return conv(xh, wh + wl, **kw) + conv(xl, wh, **kw)


# kernel -> (min band, slots per CU, strips per (sample, 16-column strip)): read from the launchers (csrc/conv_strip*.h)
STRIP_PLAN = {"strip32": (32, 12, 1), "strip32p": (32, 8, 1), "stript": (16, 2, 1), "striptp": (16, 1, 1),
              "strips2": (8, 2, 1), "strips2p": (8, 1, 1), "strips2w": (8, 1, 2)}


def strip_plan(kernel, cu, b, rows, cols):
    """plan_edges of the band plan `kernel`'s launcher makes on a chip of `cu` compute units for b samples of rows x cols (the
    grid the kernel walks: the output's, for the transposed kernels the input's)."""
    min_band, per_cu, mult = STRIP_PLAN[kernel]
    band, _ = band_plan(rows, min_band, per_cu * cu, mult * b * ((cols + 15) // 16))
    return plan_edges(rows, cols, band)
