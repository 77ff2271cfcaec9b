// Per-pixel arithmetic of the CT window on a generator-range image.
// to_windowdata (trainer/HdTrainer.py:41-64 == trainer/CycTrainer.py:34-57) in the reference's float32 operation order, every
// operation rounded on its own: the masks of the test() loop hang on exact comparisons (== 0, >= 0.3) and the exported 8-bit
// level on an exact truncation.  Plain operators under `#pragma clang fp contract(off)` guarantee it: this toolchain's
// __fmul_rn / __fsub_rn are inline functions around the same operators compiled with contraction allowed, and with them the compiler
// fused `x * 4095 - 1024` into one multiply-add (one rounding instead of two: it moves a level where the product lies within
// an ulp of a level boundary).
// Shared by ctg_to_windowdata / ctg_window_metrics / ctg_ssim (csrc/metrics.hip) and ctg_export_slices (csrc/export.hip): one
// definition, the same bits.
#pragma once
#include "common.h"

struct WinParams { float wmin, dfac; };

__device__ __forceinline__ WinParams win_params(float wc, float ww) {
    // python floats in the reference: win_min = (2*c - w)/2.0 + 0.5, dFactor = 255.0 / (win_max - win_min);
    // a float32 array combined with them rounds each to float32 first
    const double c = (double)wc, w = (double)ww;
    const double wmin = (2.0 * c - w) / 2.0 + 0.5, wmax = (2.0 * c + w) / 2.0 + 0.5;
    WinParams p;
    p.wmin = (float)wmin;
    p.dfac = (float)(255.0 / (wmax - wmin));
    return p;
}

// the stored 12-bit pixel value of a generator-range sample: (v + 1) * 0.5 * 4095 (HdTrainer.py:42 and :539)
__device__ __forceinline__ float stored_value(float v) {
#pragma clang fp contract(off)
    return ((v + 1.0f) * 0.5f) * 4095.0f;
}

// the 8-bit window level of a stored value t, a whole number in [0, 255] (HdTrainer.py:43-61; NaN stays NaN): what
// ctg_project_finish (csrc/project.hip) applies to a projected pixel
__device__ __forceinline__ float stored_level(float t, const WinParams p) {
#pragma clang fp contract(off)
    if (t == 0.0f) t = -2000.0f;
    t = t - 1024.0f;
    t = t - p.wmin;
    t = truncf(t * p.dfac);
    if (t > 255.0f) t = 255.0f;
    if (t < 0.0f) t = 0.0f;
    return t;
}

// the 8-bit window level of a generator-range sample (HdTrainer.py:42-61)
__device__ __forceinline__ float window_level(float v, const WinParams p) { return stored_level(stored_value(v), p); }

// level -> [-1, 1] (HdTrainer.py:62-63)
__device__ __forceinline__ float level_rescale(float t) {
#pragma clang fp contract(off)
    t = __fdiv_rn(t, 255.0f);
    return __fdiv_rn(t - 0.5f, 0.5f);
}

__device__ __forceinline__ float window_one(float v, const WinParams p) { return level_rescale(window_level(v, p)); }

// The four masked images of one pixel of the test() loop (HdTrainer.py:1008-1023, 1041-1047): the windowed pair (c, b) and the raw
// pair (fake * cc, real * bb), background := -1.  f = generated, r = reference sample.  Every product is rounded on its own and the
// masks hang on exact comparisons, so every kernel that needs these images calls this one definition (ctg_window_metrics, ctg_ssim
// mode 1, ctg_window_pairs): the same bits.
struct MaskedPixel { float c, b, fm, rm; };

// numpy's pair of masked assignments `m[m < 0.3] = 0; m[m >= 0.3] = 1`: a NaN meets neither comparison and stays NaN, so a NaN
// sample makes its pixel NaN in every image its mask multiplies (HdTrainer.py:1010-1011, 1016-1017)
__device__ __forceinline__ float threshold_mask(float v) { return v >= 0.3f ? 1.f : (v < 0.3f ? 0.f : v); }

__device__ __forceinline__ MaskedPixel masked_pixel(float f, float r, const WinParams p, int aliased) {
    MaskedPixel o;
    // b = W(real); bb = b >= 0.3; b = b*bb; b[b == 0] = -1
    float b = window_one(r, p);
    const float bb = threshold_mask(b);
    b = __fmul_rn(b, bb);
    if (b == 0.f) b = -1.f;
    // c = W(fake)*bb; cc = c >= 0.3; c = c*cc; c[c == 0] = -1
    float c = __fmul_rn(window_one(f, p), bb);
    const float cc = threshold_mask(c);
    c = __fmul_rn(c, cc);
    if (c == 0.f) c = -1.f;
    if (aliased) {
        // trainer/CycTrainer.py:288-298 writes `bb = b` / `cc = c` WITHOUT a copy, so thresholding the masks also
        // thresholds b and c: its windowed pair is the two binary masks mapped to +-1 (mask * mask: a NaN mask stays NaN)
        b = bb == 0.f ? -1.f : __fmul_rn(bb, bb);
        c = cc == 0.f ? -1.f : __fmul_rn(cc, cc);
    }
    o.c = c;
    o.b = b;
    // raw maps under the same masks
    float rm = __fmul_rn(r, bb);
    if (rm == 0.f) rm = -1.f;
    float fm = __fmul_rn(f, cc);
    if (fm == 0.f) fm = -1.f;
    o.fm = fm;
    o.rm = rm;
    return o;
}
