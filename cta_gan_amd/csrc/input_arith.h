// Per-pixel arithmetic of the input pipeline.
// read_ori_w (trainer/datasets.py:36-71), in the reference's float64 numpy arithmetic with the float32 cast of its
// transform: one raw HU value (SimpleITK convention) -> the windowed image and the full-range image, both in [-1, 1].
// Shared by ctg_hu_to_inputs (csrc/metrics.hip) and ctg_hu_affine_inputs (csrc/augment.hip): one definition, the same bits.
#pragma once
#include "common.h"

// wmin = (2 c - w) / 2 + 0.5, dfac = 255 / (wmax - wmin) of the window (centre c, width w), computed on the host in double
static inline void hu_window_params(float wc, float ww, double* wmin, double* dfac) {
    const double c = (double)wc, w = (double)ww;
    const double lo = (2.0 * c - w) / 2.0 + 0.5, hi = (2.0 * c + w) / 2.0 + 0.5;
    *wmin = lo;
    *dfac = 255.0 / (hi - lo);
}

// image1: CT window -> 8-bit levels -> [-1, 1]
__device__ __forceinline__ float hu_windowed(short hu, double wmin, double dfac) {
    const double d1 = (double)hu;
    double t = trunc((d1 - wmin) * dfac);
    t = t > 255.0 ? 255.0 : t;
    t = t < 0.0 ? 0.0 : t;
    t = t / 255.0;
    return (float)((t - 0.5) / 0.5);
}

// image2: full 12-bit range -> [-1, 1].  `data = data1 + 1024` (datasets.py:38) runs on the int16 array SimpleITK hands back and
// stays int16 in numpy: above 31743 it wraps to a negative value, which the clamp below then sends to 0 like air.  Reproduced (the
// conversion of an out-of-range int to short is modular here): the whole int16 domain equals the reference bit for bit
// (tests/test_metrics_exact_gpu.py).  This changes every caller above HU 31743: ctg_hu_to_inputs, series_inputs_kernel
// (csrc/export.hip: the inference path's generator input) and SrcHu (csrc/augment.hip: the training loaders' augmentation).  No
// CT stores such values; csrc/subtract.hip's `a = max(ct + 1024, 0)` is int32, does not wrap and differs from this there.
__device__ __forceinline__ float hu_fullrange(short hu) {
    double f = (double)(short)((int)hu + 1024);
    f = f < 0.0 ? 0.0 : f;
    f = f / 4095.0;
    return (float)((f - 0.5) / 0.5);
}

// Resize = F.interpolate(mode="nearest") (trainer/utils.py:13-32): the source index of output index o along an axis of n source
// pixels, scale = (float)n / (float)n_out computed on the host
__device__ __forceinline__ int nearest_src_index(int o, float scale, int n) {
    const int i = (int)floorf(__fmul_rn((float)o, scale));
    return i < n - 1 ? i : n - 1;
}
