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

// the 8-bit window level, a whole number in [0, 255] (HdTrainer.py:42-61; NaN stays NaN)
__device__ __forceinline__ float window_level(float v, const WinParams p) {
#pragma clang fp contract(off)
    float t = stored_value(v);
    if (t == 0.0f) t = -2000.0f;
    t = t - 1024.0f;
    t = t - p.wmin;
    t = truncf(t * p.dfac);
    if (t > 255.0f) t = 255.0f;
    if (t < 0.0f) t = 0.0f;
    return t;
}

// level -> [-1, 1] (HdTrainer.py:62-63)
__device__ __forceinline__ float level_rescale(float t) {
#pragma clang fp contract(off)
    t = __fdiv_rn(t, 255.0f);
    return __fdiv_rn(t - 0.5f, 0.5f);
}

__device__ __forceinline__ float window_one(float v, const WinParams p) { return level_rescale(window_level(v, p)); }
