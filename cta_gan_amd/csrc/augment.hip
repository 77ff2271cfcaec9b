// Training augmentation of the reference's loaders on the device: RandomAffine(degrees, translate, scale, fillcolor) on a float
// ('F' mode) PIL image followed by Resize (trainer/HdTrainer.py:130-142,641-653, CycTrainer.py:91-99, p2pTrainer.py:81-89,
// RegTrainer.py:122-132; applied per image in trainer/datasets.py:103-119,218-232).  torchvision's PIL path ends in
// Image.transform(size, AFFINE, inverse matrix, NEAREST, fillcolor), which for a rotated float image is PIL's 16.16 fixed-point
// loop: pure integer arithmetic on six coefficients the host derives (cta_gan_amd/trainer/augment.py), so the gather below
// returns PIL's pixels bit for bit.  The nearest Resize that follows is a second gather; both are composed per output pixel.
//
// Streaming gather: one workgroup per output row of a plane, the plane's six coefficients and the row's source row are
// wave-uniform, each lane stores 16 bytes (4 pixels); scalar lanes cover the pixels in front of the first 16-byte boundary of the
// row and behind the last one, so any width and any 4-byte-aligned destination take the same path.
#include "common.h"
#include "input_arith.h"

#define AFF_THREADS 128
#define AFF_MAX_SIDE 32768

struct SrcF32 {
    const float* __restrict__ p;
    __device__ __forceinline__ float operator()(size_t i) const { return p[i]; }
};

// raw HU plane converted on the fly: a gather commutes with a pointwise map
struct SrcHu {
    const short* __restrict__ p;
    double wmin, dfac;
    int full;   // 0: windowed image, 1: full-range image (wave-uniform)
    __device__ __forceinline__ float operator()(size_t i) const {
        const short v = p[i];
        return full ? hu_fullrange(v) : hu_windowed(v, wmin, dfac);
    }
};

// One output row `oy` of one plane.  coef: the plane's (A0 .. A5); drow: &dst[plane][oy][0].
template <typename Src>
__device__ __forceinline__ void affine_row(const Src src, const int* __restrict__ coef, int Hi, int Wi, float fill,
                                           float* __restrict__ drow, int oy, int Wo, float sh, float sw) {
    const long A0 = coef[0], A1 = coef[1], A2 = coef[2], A3 = coef[3], A4 = coef[4], A5 = coef[5];
    // the pixel of the Hi x Wi warped image that the nearest resize reads, then PIL's fixed-point source position of that pixel
    const int iy = nearest_src_index(oy, sh, Hi);
    const long bx = A2 + A1 * iy, by = A5 + A4 * iy;
    auto pixel = [&](int ox) -> float {
        const int ix = nearest_src_index(ox, sw, Wi);
        const long xs = (bx + A0 * ix) >> 16, ys = (by + A3 * ix) >> 16;      // arithmetic shifts
        return (xs >= 0 && xs < Wi && ys >= 0 && ys < Hi) ? src((size_t)ys * Wi + (size_t)xs) : fill;
    };
    // [0, head): scalar up to the first 16-byte boundary; [head, head + 4 nvec): 16-byte stores; the rest (< 4): scalar
    int head = (4 - (int)(((uintptr_t)drow >> 2) & 3)) & 3;
    head = head < Wo ? head : Wo;
    const int nvec = (Wo - head) >> 2;
    const int tail0 = head + 4 * nvec;
    const int t = threadIdx.x;
    if (t < head) drow[t] = pixel(t);
    for (int k = t; k < nvec; k += AFF_THREADS) {
        const int x = head + 4 * k;
        *reinterpret_cast<f32x4*>(drow + x) = f32x4{pixel(x), pixel(x + 1), pixel(x + 2), pixel(x + 3)};
    }
    if (t < Wo - tail0) drow[tail0 + t] = pixel(tail0 + t);
}

__global__ __launch_bounds__(AFF_THREADS) void affine_nearest_kernel(const float* __restrict__ src, const int* __restrict__ coef,
                                                                     int Hi, int Wi, float fill, float* __restrict__ dst,
                                                                     int Ho, int Wo, float sh, float sw) {
    const int n = blockIdx.x / Ho, oy = blockIdx.x - n * Ho;
    affine_row(SrcF32{src + (size_t)n * Hi * Wi}, coef + (size_t)n * 6, Hi, Wi, fill, dst + ((size_t)n * Ho + oy) * Wo, oy, Wo,
               sh, sw);
}

__global__ __launch_bounds__(AFF_THREADS) void hu_affine_inputs_kernel(const short* __restrict__ hu, const int* __restrict__ coef,
                                                                       int Hi, int Wi, double wmin, double dfac, float fill,
                                                                       float* __restrict__ win, float* __restrict__ full,
                                                                       int Ho, int Wo, float sh, float sw) {
    const int q = blockIdx.x / Ho, oy = blockIdx.x - q * Ho;      // q = 2 b + (0: windowed, 1: full range)
    const int b = q >> 1, which = q & 1;
    float* __restrict__ dst = which ? full : win;
    affine_row(SrcHu{hu + (size_t)b * Hi * Wi, wmin, dfac, which}, coef + (size_t)q * 6, Hi, Wi, fill,
               dst + ((size_t)b * Ho + oy) * Wo, oy, Wo, sh, sw);
}

static bool affine_sizes_ok(int planes, int Hi, int Wi, int Ho, int Wo) {
    if (planes < 1 || Hi < 1 || Wi < 1 || Ho < 1 || Wo < 1) return false;
    if (Hi > AFF_MAX_SIDE || Wi > AFF_MAX_SIDE || Ho > AFF_MAX_SIDE || Wo > AFF_MAX_SIDE) return false;
    if ((long)Ho * Wo >= (1L << 31)) return false;
    return (long)planes * Ho < (1L << 31);      // one workgroup per output row of a plane
}

extern "C" int ctg_affine_nearest(const float* src, const int* coef, int N, int Hi, int Wi, float fill, float* dst, int Ho,
                                  int Wo, void* stream) {
    CTG_ENTER();
    if (src == nullptr || coef == nullptr || dst == nullptr || !affine_sizes_ok(N, Hi, Wi, Ho, Wo)) return CTG_EINVAL;
    hipLaunchKernelGGL(affine_nearest_kernel, dim3((unsigned)N * Ho), dim3(AFF_THREADS), 0, (hipStream_t)stream, src, coef, Hi,
                       Wi, fill, dst, Ho, Wo, (float)Hi / (float)Ho, (float)Wi / (float)Wo);
    return ctg_launch_status();
}

extern "C" int ctg_hu_affine_inputs(const short* hu, const int* coef, int B, int Hi, int Wi, float wc, float ww, float fill,
                                    float* win, float* full, int Ho, int Wo, void* stream) {
    CTG_ENTER();
    if (hu == nullptr || coef == nullptr || win == nullptr || full == nullptr || ww <= 0.f) return CTG_EINVAL;
    if (B < 1 || B > (1 << 29) || !affine_sizes_ok(2 * B, Hi, Wi, Ho, Wo)) return CTG_EINVAL;
    double wmin, dfac;
    hu_window_params(wc, ww, &wmin, &dfac);
    hipLaunchKernelGGL(hu_affine_inputs_kernel, dim3(2u * B * Ho), dim3(AFF_THREADS), 0, (hipStream_t)stream, hu, coef, Hi, Wi,
                       wmin, dfac, fill, win, full, Ho, Wo, (float)Hi / (float)Ho, (float)Wi / (float)Wo);
    return ctg_launch_status();
}
