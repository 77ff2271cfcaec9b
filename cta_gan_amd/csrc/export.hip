// Series inference, the way in and the way back (the export half of every trainer's test() loop):
//   newimg = (fake_BB + 1) * 0.5 * 4095; newimg.astype(np.int16)      trainer/HdTrainer.py:539-543, 1062-1066 (CycTrainer.py:337-340,
//                                                                      p2pTrainer.py:288-291, RegTrainer.py:360-363)
//   the 8-bit window level of to_windowdata                            HdTrainer.py:41-61 (before its rescale to [-1, 1])
//   read_ori_w's full-range image + Resize                             trainer/datasets.py:36-71, trainer/utils.py:13-32
// ctg_export_slices turns the generator's fp32 planes into the scanner's int16 pixels and the window's uint8 levels in one pass
// (7 bytes per pixel instead of the >= 22 of the composed elementwise ops); ctg_series_inputs writes only the plane test() feeds
// the generator.  Both gather by nearest_src_index when the series was scanned at another size than the generator runs at.
//
// Streaming form (equal sizes): a lane takes 8 consecutive pixels -- two 16-byte loads, both issued before the first use, one
// 16-byte store of int16 and one 8-byte store of uint8.  Scalar lanes cover the pixels in front of the first boundary at which
// all three addresses are aligned and behind the last whole group of 8, so a plane of odd H W (every later plane then starts
// misaligned) takes the same path.  No LDS, no inter-workgroup communication.
#include "common.h"
#include "input_arith.h"
#include "window_arith.h"

#define EXP_THREADS 256
#define EXP_MAX_BLOCKS_X 1024

typedef short i16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// astype(np.int16) of the stored value: truncation toward zero inside the int16 range (the whole of the reference's domain:
// tanh output gives 0 .. 4095); outside it the conversion saturates, NaN gives 0.  hu: SimpleITK's convention, value - 1024.
__device__ __forceinline__ short export_pixel(float v, int hu) {
    float t = stored_value(v);
    t = t > 32767.0f ? 32767.0f : t;
    t = t < -32768.0f ? -32768.0f : t;
    int q = t == t ? (int)t : 0;
    if (hu) {
        q -= 1024;
        q = q < -32768 ? -32768 : q;
    }
    return (short)q;
}

__device__ __forceinline__ unsigned export_level(float v, const WinParams p) {
    const float t = window_level(v, p);
    return t == t ? (unsigned)(int)t : 0u;
}

__device__ __forceinline__ void export_one(float v, const WinParams p, int hu, short* __restrict__ pix,
                                           unsigned char* __restrict__ level, long i) {
    if (pix != nullptr) pix[i] = export_pixel(v, hu);
    if (level != nullptr) level[i] = (unsigned char)export_level(v, p);
}

// grid (blocks, B); head: scalar pixels in front of the aligned body of each plane, per plane (HW when no common boundary exists)
__global__ __launch_bounds__(EXP_THREADS) void export_stream_kernel(const float* __restrict__ img, const float* __restrict__ wc,
                                                                    const float* __restrict__ ww, short* __restrict__ pix,
                                                                    unsigned char* __restrict__ level, long HW, int hu) {
    const int n = blockIdx.y;
    WinParams p = {0.f, 0.f};
    if (level != nullptr) p = win_params(wc[n], ww[n]);
    const float* __restrict__ src = img + (size_t)n * HW;
    short* __restrict__ dp = pix != nullptr ? pix + (size_t)n * HW : nullptr;
    unsigned char* __restrict__ dl = level != nullptr ? level + (size_t)n * HW : nullptr;
    // first pixel h at which src + h is 16-byte, dp + h 16-byte and dl + h 8-byte aligned: h = -e (mod 8) for the outputs'
    // element misalignment e, and the same h must be -e_src (mod 4); pointers that disagree leave the plane to the scalar lanes
    const unsigned e_src = (unsigned)(((uintptr_t)src >> 2) & 3);
    const unsigned e_out = dp != nullptr ? (unsigned)(((uintptr_t)dp >> 1) & 7) : (unsigned)((uintptr_t)dl & 7);
    long head = (8 - e_out) & 7;
    const bool agree = ((head + e_src) & 3) == 0 && (dl == nullptr || (((uintptr_t)dl + head) & 7) == 0);
    head = (agree && head < HW) ? head : HW;
    const long nvec = (HW - head) >> 3;
    const long tail0 = head + 8 * nvec;
    const long t = (long)blockIdx.x * EXP_THREADS + threadIdx.x, step = (long)gridDim.x * EXP_THREADS;
    for (long i = t; i < head; i += step) export_one(src[i], p, hu, dp, dl, i);
    for (long k = t; k < nvec; k += step) {
        const long i = head + 8 * k;
        const f32x4 a = *reinterpret_cast<const f32x4*>(src + i);
        const f32x4 b = *reinterpret_cast<const f32x4*>(src + i + 4);
        const float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
        if (dp != nullptr) {
            i16x8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = export_pixel(v[j], hu);
            *reinterpret_cast<i16x8*>(dp + i) = o;
        }
        if (dl != nullptr) {
            unsigned lo = 0, hi = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                lo |= export_level(v[j], p) << (8 * j);
                hi |= export_level(v[4 + j], p) << (8 * j);
            }
            *reinterpret_cast<u32x2*>(dl + i) = u32x2{lo, hi};
        }
    }
    for (long i = tail0 + t; i < HW; i += step) export_one(src[i], p, hu, dp, dl, i);
}

// another output size: every output pixel gathers its source by ctg_resize_nearest's rule
__global__ __launch_bounds__(EXP_THREADS) void export_gather_kernel(const float* __restrict__ img, const float* __restrict__ wc,
                                                                    const float* __restrict__ ww, int Hi, int Wi,
                                                                    short* __restrict__ pix, unsigned char* __restrict__ level,
                                                                    int Ho, int Wo, float sh, float sw, int hu) {
    const int n = blockIdx.y;
    WinParams p = {0.f, 0.f};
    if (level != nullptr) p = win_params(wc[n], ww[n]);
    const float* __restrict__ src = img + (size_t)n * Hi * Wi;
    const int total = Ho * Wo;
    short* __restrict__ dp = pix != nullptr ? pix + (size_t)n * total : nullptr;
    unsigned char* __restrict__ dl = level != nullptr ? level + (size_t)n * total : nullptr;
    for (int i = blockIdx.x * EXP_THREADS + threadIdx.x; i < total; i += gridDim.x * EXP_THREADS) {
        const int oy = i / Wo, ox = i - oy * Wo;
        const int iy = nearest_src_index(oy, sh, Hi), ix = nearest_src_index(ox, sw, Wi);
        export_one(src[(size_t)iy * Wi + ix], p, hu, dp, dl, i);
    }
}

__global__ __launch_bounds__(EXP_THREADS) void series_inputs_kernel(const short* __restrict__ hu, int Hi, int Wi,
                                                                    float* __restrict__ full, int Ho, int Wo, float sh, float sw) {
    const int n = blockIdx.y;
    const short* __restrict__ src = hu + (size_t)n * Hi * Wi;
    const int total = Ho * Wo;
    float* __restrict__ dst = full + (size_t)n * total;
    for (int i = blockIdx.x * EXP_THREADS + threadIdx.x; i < total; i += gridDim.x * EXP_THREADS) {
        const int oy = i / Wo, ox = i - oy * Wo;
        const int iy = nearest_src_index(oy, sh, Hi), ix = nearest_src_index(ox, sw, Wi);
        dst[i] = hu_fullrange(src[(size_t)iy * Wi + ix]);
    }
}

static bool export_sizes_ok(int B, int Hi, int Wi, int Ho, int Wo) {
    if (B < 1 || B > 65535 || Hi < 1 || Wi < 1 || Ho < 1 || Wo < 1) return false;
    return (long)Hi * Wi < (1L << 31) && (long)Ho * Wo < (1L << 31);
}

static unsigned export_blocks(long items) {
    const long b = (items + EXP_THREADS - 1) / EXP_THREADS;
    return (unsigned)(b < 1 ? 1 : (b < EXP_MAX_BLOCKS_X ? b : EXP_MAX_BLOCKS_X));
}

extern "C" int ctg_export_slices(const float* img, const float* wc, const float* ww, int B, int Hi, int Wi, short* pix,
                                 unsigned char* level, int Ho, int Wo, int hu, void* stream) {
    CTG_ENTER();
    if (img == nullptr || (pix == nullptr && level == nullptr) || !export_sizes_ok(B, Hi, Wi, Ho, Wo)) return CTG_EINVAL;
    if (level != nullptr && (wc == nullptr || ww == nullptr)) return CTG_EINVAL;
    if (((uintptr_t)img & 3) != 0 || ((uintptr_t)pix & 1) != 0) return CTG_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (Ho == Hi && Wo == Wi) {
        const long HW = (long)Hi * Wi;
        hipLaunchKernelGGL(export_stream_kernel, dim3(export_blocks((HW + 7) / 8), B), dim3(EXP_THREADS), 0, st, img, wc, ww, pix,
                           level, HW, hu);
    } else {
        hipLaunchKernelGGL(export_gather_kernel, dim3(export_blocks((long)Ho * Wo), B), dim3(EXP_THREADS), 0, st, img, wc, ww, Hi,
                           Wi, pix, level, Ho, Wo, (float)Hi / (float)Ho, (float)Wi / (float)Wo, hu);
    }
    return ctg_launch_status();
}

extern "C" int ctg_series_inputs(const short* hu, int B, int Hi, int Wi, float* full, int Ho, int Wo, void* stream) {
    CTG_ENTER();
    if (hu == nullptr || full == nullptr || !export_sizes_ok(B, Hi, Wi, Ho, Wo)) return CTG_EINVAL;
    hipLaunchKernelGGL(series_inputs_kernel, dim3(export_blocks((long)Ho * Wo), B), dim3(EXP_THREADS), 0, (hipStream_t)stream, hu,
                       Hi, Wi, full, Ho, Wo, (float)Hi / (float)Ho, (float)Wi / (float)Wo);
    return ctg_launch_status();
}
