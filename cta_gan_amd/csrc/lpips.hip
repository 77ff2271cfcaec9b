// LPIPS (AlexNet, lpips 0.1) of the test() loops, the parts that are not a convolution:
//   `loss_fn_alex.forward(torch.tensor(x), torch.tensor(y))`  trainer/HdTrainer.py:26-28, 504-513, 531-536 and the twins in
//   CycTrainer.py / p2pTrainer.py / RegTrainer.py.
// The five convolutions run on ctg_im2col_pack / ctg_conv_igemm (fp32 MFMA); here are AlexNet's two 3x3 / stride-2 max-pools and the
// per-layer distance  l_k = mean_pixels sum_c lin_k[c] (n(f_k(x)) - n(f_k(y)))^2,  n(f) = f / (sqrt(sum_c f^2) + 1e-10).
// fp32 NHWC throughout; the distance is HBM-bound (one pass over both feature maps) and summed in fp64 through a two-stage partials
// buffer -- no floating-point atomics, the same bits on every run.
#include "common.h"

// ------------------------------------------------------------------ nn.MaxPool2d(kernel_size=3, stride=2), no padding, floor
// One lane per 16-byte chunk of an output pixel; its nine window chunks are fetched before the first is looked at.  The update
// rule is ATen's (`val > max || isnan(val)`, window in scan order), so the result equals F.max_pool2d bit for bit.
__global__ __launch_bounds__(256) void maxpool3s2_fwd_kernel(const float* __restrict__ x, int x_ld, float* __restrict__ out, int o_ld,
                                                             int H, int W, int C, int Ho, int Wo, long items) {
    const int CPP = C / 4;
    for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < items; it += (long)gridDim.x * 256) {
        const unsigned pixu = (unsigned)it / (unsigned)CPP;   // 32-bit: items < 2^31 is checked by the host side
        const long pix = pixu;
        const int ch = (int)(it - pix * CPP) * 4;
        const int ox = (int)(pixu % (unsigned)Wo);
        const int oy = (int)((pixu / (unsigned)Wo) % (unsigned)Ho);
        const int n = (int)(pixu / ((unsigned)Wo * (unsigned)Ho));
        const float* base = x + (((size_t)n * H + 2 * oy) * W + 2 * ox) * x_ld + ch;      // 2 * oy + 2 <= H - 1: no border case
        f32x4 w[9];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) w[ky * 3 + kx] = *reinterpret_cast<const f32x4*>(base + ((size_t)ky * W + kx) * x_ld);
        f32x4 m = w[0];
#pragma unroll
        for (int t = 1; t < 9; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (w[t][e] > m[e] || w[t][e] != w[t][e]) m[e] = w[t][e];
        *reinterpret_cast<f32x4*>(out + pix * o_ld + ch) = m;
    }
}

extern "C" int ctg_maxpool3s2_fwd(const float* x, int x_ld, float* out, int o_ld, int B, int H, int W, int C, void* stream) {
    CTG_ENTER();
    if (x == nullptr || out == nullptr || B < 1 || H < 3 || W < 3 || C < 4 || C % 4) return CTG_EINVAL;
    if (x_ld < C || o_ld < C || x_ld % 4 || o_ld % 4 || ((uintptr_t)x & 15) || ((uintptr_t)out & 15)) return CTG_EINVAL;
    const int Ho = (H - 3) / 2 + 1, Wo = (W - 3) / 2 + 1;
    const long items = (long)B * Ho * Wo * (C / 4);
    if (items >= (1L << 31)) return CTG_EINVAL;   // the kernel decodes item indices in 32 bits
    const long blocks = (items + 255) / 256;
    hipLaunchKernelGGL(maxpool3s2_fwd_kernel, dim3((unsigned)(blocks > 8192 ? 8192 : blocks)), dim3(256), 0, (hipStream_t)stream, x,
                       x_ld, out, o_ld, H, W, C, Ho, Wo, items);
    return ctg_launch_status();
}

// ------------------------------------------------------------------ per-layer distance
#define LP_GROUP 16                       // lanes that own one pixel: 16 x 16 bytes = 64 channels per trip over the channels
#define LP_GPB (256 / LP_GROUP)           // pixel groups per workgroup
#define LP_MAX_BLOCKS 64                  // partials per pair

// sum over the 16 lanes of a pixel group, the total in every lane (xor butterfly inside the group: DPP row operations)
__device__ __forceinline__ float group16_sum(float v) {
#pragma unroll
    for (int o = LP_GROUP / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// f [2P][HW][f_ld]: pair p = images p ("x") and P + p ("y").  grid (nblk, P); group g of workgroup b owns the pixels
// (b * LP_GPB + g) * PIX + {0 .. PIX-1}, + nblk * LP_GPB * PIX per trip.  NCH = C / 64 chunks per lane and side: 2 * NCH * PIX
// 16-byte loads are issued before the first is used (>= 4 for every C).
template <int NCH, int PIX>
__global__ __launch_bounds__(256) void lpips_layer_partial_kernel(const float* __restrict__ f, int f_ld, const float* __restrict__ lin,
                                                                  int P, long HW, double* __restrict__ part) {
    __shared__ double red[LP_GPB];
    const int p = blockIdx.y;
    const int sub = threadIdx.x & (LP_GROUP - 1), grp = threadIdx.x / LP_GROUP;
    const float* __restrict__ X = f + (size_t)p * HW * f_ld;
    const float* __restrict__ Y = f + (size_t)(P + p) * HW * f_ld;
    f32x4 lw[NCH];
#pragma unroll
    for (int j = 0; j < NCH; ++j) lw[j] = *reinterpret_cast<const f32x4*>(lin + (j * LP_GROUP + sub) * 4);
    const long step = (long)gridDim.x * LP_GPB * PIX;
    const long trips = (HW + step - 1) / step;      // the same for every lane: the shuffles below run with all lanes
    double acc = 0.0;
    long pix0 = ((long)blockIdx.x * LP_GPB + grp) * PIX;
    for (long t = 0; t < trips; ++t, pix0 += step) {
        f32x4 xv[PIX][NCH], yv[PIX][NCH];
#pragma unroll
        for (int q = 0; q < PIX; ++q) {
            const bool ok = pix0 + q < HW;
            const size_t off = (size_t)(ok ? pix0 + q : 0) * f_ld + sub * 4;
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                xv[q][j] = ok ? *reinterpret_cast<const f32x4*>(X + off + j * (LP_GROUP * 4)) : f32x4{0.f, 0.f, 0.f, 0.f};
                yv[q][j] = ok ? *reinterpret_cast<const f32x4*>(Y + off + j * (LP_GROUP * 4)) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
#pragma unroll
        for (int q = 0; q < PIX; ++q) {
            float sx = 0.f, sy = 0.f;
#pragma unroll
            for (int j = 0; j < NCH; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    sx += xv[q][j][e] * xv[q][j][e];
                    sy += yv[q][j][e] * yv[q][j][e];
                }
            sx = group16_sum(sx);
            sy = group16_sum(sy);
            // an all-zero pixel: 0 * (1 / 1e-10) = 0, as 0 / 1e-10 in the reference
            const float rx = 1.f / (sqrtf(sx) + 1e-10f), ry = 1.f / (sqrtf(sy) + 1e-10f);
            float d = 0.f;
#pragma unroll
            for (int j = 0; j < NCH; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    // both products rounded before the subtraction: contracted into fma(x, rx, -(y ry)) the difference of two EQUAL
                    // pixels is the rounding error of one product, not 0 (LPIPS(x, x) must be exactly 0)
#pragma clang fp contract(off)
                    const float df = xv[q][j][e] * rx - yv[q][j][e] * ry;
                    d += lw[j][e] * (df * df);
                }
            d = group16_sum(d);
            if (pix0 + q < HW) acc += (double)d;
        }
    }
    if (sub == 0) red[grp] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
#pragma unroll
        for (int g = 0; g < LP_GPB; ++g) s += red[g];      // fixed order: the same bits on every run
        part[(size_t)p * gridDim.x + blockIdx.x] = s;
    }
}

__global__ void lpips_layer_final_kernel(const double* __restrict__ part, int nblk, int P, long HW, int k, double* __restrict__ out) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += part[(size_t)p * nblk + b];
    out[(size_t)p * 5 + k] = s / (double)HW;
}

// Partials per pair for HW pixels: min(64, ceil(HW / 16)); the caller sizes `part` for P * 64 doubles.
static inline int lpips_blocks(long HW) {
    const long b = (HW + LP_GPB - 1) / LP_GPB;
    return (int)(b < 1 ? 1 : (b > LP_MAX_BLOCKS ? LP_MAX_BLOCKS : b));
}

extern "C" int ctg_lpips_layer(const float* f, int f_ld, const float* lin, int P, long HW, int C, int k, double* part, double* out,
                               void* stream) {
    CTG_ENTER();
    if (f == nullptr || lin == nullptr || part == nullptr || out == nullptr) return CTG_EINVAL;
    if (P < 1 || P > 65535 || HW < 1 || k < 0 || k > 4) return CTG_EINVAL;
    if (C < 64 || C > 384 || C % 64 || f_ld < C || f_ld % 4 || ((uintptr_t)f & 15) || ((uintptr_t)lin & 15)) return CTG_EINVAL;
    const int nblk = lpips_blocks(HW);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(nblk, P), blk(256);
#define LP_LAUNCH(NCH, PIX) \
    hipLaunchKernelGGL((lpips_layer_partial_kernel<NCH, PIX>), grid, blk, 0, st, f, f_ld, lin, P, HW, part)
    switch (C / 64) {
        case 1: LP_LAUNCH(1, 2); break;
        case 2: LP_LAUNCH(2, 1); break;
        case 3: LP_LAUNCH(3, 1); break;
        case 4: LP_LAUNCH(4, 1); break;
        case 5: LP_LAUNCH(5, 1); break;
        default: LP_LAUNCH(6, 1); break;
    }
#undef LP_LAUNCH
    hipLaunchKernelGGL(lpips_layer_final_kernel, dim3((P + 63) / 64), dim3(64), 0, st, part, nblk, P, HW, k, out);
    return ctg_launch_status();
}
