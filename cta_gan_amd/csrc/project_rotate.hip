// Series inference, the rotating view: the maximum- / minimum-intensity or mean projection of the exported int16 volume at any
// angle about the cranio-caudal axis (cta_gan_amd/infer.py: SeriesRotator).  project.hip has the three body axes; like them the
// reference has no counterpart (its test() writes slices only).
//
// A row of a rotated projection depends on one slice only: out[a][n][u] reduces slice n along the ray of detector column u at
// angle a.  A chunk of K slices therefore finishes rows n0 .. n0+K-1 of every angle in one launch: no accumulator, no atomics, no
// identity fill, no finish pass.  Rays take T unit steps and sample the nearest pixel on a 16.16 fixed-point grid (the technique
// of ctg_affine_nearest, csrc/augment.hip): the sample of (u, t) is pixel
//     xi = (c0 + c1 u + c2 t) >> 16,   yi = (c3 + c4 u + c5 t) >> 16       (arithmetic shift; counted when inside the slice)
// with six int32 coefficients per angle formed on the host (infer.py: rotation_coefficients).  Everything up to the 8-bit level
// is integer arithmetic, equal to numpy bit for bit; max, min and sum are exact and commutative.
//
// One 256-thread workgroup per (slice, segment of ROT_WG_U detector columns, angle), the angle fastest over the grid so that a
// slice stays cache-resident across its angles.  A wave owns ROT_UL = 8 neighbouring rays and walks them with 8 lanes each: lane
// (ul, tl) takes the steps t = tl (mod 8) of ray ul, so one gather instruction of the wave covers an 8 x 8 patch of (u, t) -- at
// most 12 rows of the slice at any angle, where 64 lanes along u touch 64 rows at 90 degrees, one cache line each (the first
// version of this kernel: 233 us per 16 x 512 x 512 chunk and 36 angles against 148 for this one, LAB_NOTES section 15) -- and
// the 8 partial results of a ray meet at the end in three xor-shuffles; max, min, sum and count are exact and commutative, so the order does not show.  The steps of a ray that can lie
// inside the slice form one interval [lo, hi] (two linear inequalities per axis, exact integer division, once per ray); the lanes
// walk only that interval, ROT_INFLIGHT gathers issued before the first is used.  The six coefficients are workgroup-uniform
// (scalar loads).  Whatever the interval says, a sample is read only after its own index passed the bounds check, and a sample
// that fails it reads pixel 0 of the slice and is not counted: every address is inside the slice whatever the table holds.  The
// fixed-point sums are formed in unsigned arithmetic (wraps, never undefined) and read as int32.
//
// Bilinear sampling (ctg_project_rotate_bilinear; LERP below) shares the table, the detector, the interval and the definition of
// "counted" -- pixel (X >> 16, Y >> 16) in the slice, X and Y carrying the + 0.5 of the nearest rule -- so a ray's count and the
// place of `fill` are those of nearest sampling.  The value of a counted sample is interpolated about the centre-based position
//     Xc = X - 32768, Yc = Y - 32768:   x0 = Xc >> 16, fx = (Xc >> 8) & 255,   y0 = Yc >> 16, fy = (Yc >> 8) & 255
//     v = ((p[ya][xa] (256 - fx) + p[ya][xb] fx) (256 - fy) + (p[yb][xa] (256 - fx) + p[yb][xb] fx) fy + 32768) >> 16
// with xa = clamp(x0), xb = clamp(x0 + 1) to 0 .. W-1 and ya, yb likewise (the edge pixel replicated; x0 is -1 in the first half
// pixel): four 16-bit loads, since only 2-byte alignment is promised.  The clamps keep every address inside the slice whatever
// the table holds, and a sample that is not counted still reads pixel 0.  The weights sum to 65536, so v is an int16 value.
// Oversampled rays (steps of 1 / s voxel) are a matter of the table and of T alone: both kernels take them as they are.
//
// Depth of the maximum (ctg_project_rotate_depth; kernels of their own at the end of this file, the ones above are not touched):
// for mode max and min a ray also reports the step t at which its value was found -- the first counted step from the viewer's
// end, t = 0, that attains it (np.argmax / np.argmin over the counted samples) -- and the level attenuated by that depth.  A
// lane packs (value, t) into one 32-bit key whose unsigned order is "better value first, then smaller t":
//     b = value + 32768 (0 .. 65535);   max: key = b << 16 | (65535 - t), unsigned max, identity 0
//                                       min: key = b << 16 | t,           unsigned min, identity 0xffffffff
// so the walk, the in-flight gathers and the three xor-shuffles stay what they are, on keys instead of values.  T <= 4096 keeps a
// real key off the identity, which therefore also says "no counted sample": depth -1 and `fill`.  The depth cue (cue 0 .. 256):
//     w = 256 - (cue t) / T  (C division; 1 <= w <= 256 since t < T; a missed ray keeps 256),   cued = (level w + 128) >> 8.
#include "common.h"
#include "rotate_sample.h"
#include "window_arith.h"

#define ROT_THREADS 256
#define ROT_UL 8            // rays of a wave
#define ROT_TL 8            // lanes of a ray: lane tl takes the steps t = tl (mod ROT_TL)
#define ROT_WG_U (ROT_THREADS / 64 * ROT_UL)
#define ROT_INFLIGHT 4      // gathers a lane issues before it uses the first
#define ROT_MAX_DIM 4096    // H, W, U, T, A: each term of the fixed-point sum stays below 2^28

enum { ROT_MAX = 0, ROT_MIN = 1, ROT_SUM = 2 };

// rot_clip, rot_lerp and rot_clamp: rotate_sample.h (shared with csrc/project_render.hip)

template <int MODE> __device__ __forceinline__ int rot_op(int a, int b) {
    if constexpr (MODE == ROT_MAX) return a > b ? a : b;
    else if constexpr (MODE == ROT_MIN) return a < b ? a : b;
    else return a + b;
}

template <int MODE, bool LERP>
__global__ __launch_bounds__(ROT_THREADS) void project_rotate_kernel(const short* __restrict__ pix, int H, int W, int n0, int N,
                                                                     const int* __restrict__ coef, int A, int U, int T, int nseg,
                                                                     int fill, float wc, float ww, int add,
                                                                     short* __restrict__ values, unsigned char* __restrict__ level) {
    const unsigned a = blockIdx.x % (unsigned)A, rest = blockIdx.x / (unsigned)A;
    const unsigned seg = rest % (unsigned)nseg, k = rest / (unsigned)nseg;
    const int lane = threadIdx.x & 63, tl = lane / ROT_UL;
    const int u = (int)(seg * ROT_WG_U + (threadIdx.x >> 6) * ROT_UL + lane % ROT_UL);
    const bool live = u < U;      // (every lane stays for the shuffles; the 8 lanes of a ray are live together)
    const int* __restrict__ c = coef + (size_t)a * 6;
    const unsigned c2 = (unsigned)c[2], c5 = (unsigned)c[5];
    const unsigned X0 = (unsigned)c[0] + (unsigned)c[1] * (unsigned)u, Y0 = (unsigned)c[3] + (unsigned)c[4] * (unsigned)u;
    int lo = 0, hi = live ? T - 1 : -1;
    rot_clip((int)X0, (int)c2, (W << 16) - 1, lo, hi);
    rot_clip((int)Y0, (int)c5, (H << 16) - 1, lo, hi);
    const short* __restrict__ slice = pix + (size_t)k * H * W;
    int acc = MODE == ROT_MAX ? -32768 : (MODE == ROT_MIN ? 32767 : 0), cnt = 0;
    int t = (lo & ~(ROT_TL - 1)) + tl;      // lo >= 0
    unsigned X = X0 + c2 * (unsigned)t, Y = Y0 + c5 * (unsigned)t;
    const unsigned dX = c2 * ROT_TL, dY = c5 * ROT_TL;
    for (; t <= hi; t += ROT_TL * ROT_INFLIGHT) {
        bool ok[ROT_INFLIGHT];
        if constexpr (LERP) {
            int p[ROT_INFLIGHT][4], fx[ROT_INFLIGHT], fy[ROT_INFLIGHT];      // 4 ROT_INFLIGHT gathers before the first is used
#pragma unroll
            for (int j = 0; j < ROT_INFLIGHT; ++j) {
                const int xi = (int)X >> 16, yi = (int)Y >> 16;
                ok[j] = t + j * ROT_TL <= hi && xi >= 0 && xi < W && yi >= 0 && yi < H;
                const int Xc = (int)(X - 32768u), Yc = (int)(Y - 32768u);
                fx[j] = (Xc >> 8) & 255;
                fy[j] = (Yc >> 8) & 255;
                const int x0 = Xc >> 16, y0 = Yc >> 16;      // in -32768 .. 32767: x0 + 1 cannot wrap
                const int xa = ok[j] ? rot_clamp(x0, W - 1) : 0, xb = ok[j] ? rot_clamp(x0 + 1, W - 1) : 0;
                const int ra = ok[j] ? rot_clamp(y0, H - 1) * W : 0, rb = ok[j] ? rot_clamp(y0 + 1, H - 1) * W : 0;
                p[j][0] = slice[ra + xa];
                p[j][1] = slice[ra + xb];
                p[j][2] = slice[rb + xa];
                p[j][3] = slice[rb + xb];
                X += dX;
                Y += dY;
            }
#pragma unroll
            for (int j = 0; j < ROT_INFLIGHT; ++j) {
                if (!ok[j]) continue;
                acc = rot_op<MODE>(acc, rot_lerp(p[j][0], p[j][1], p[j][2], p[j][3], fx[j], fy[j]));
                ++cnt;
            }
        } else {
            int raw[ROT_INFLIGHT];
#pragma unroll
            for (int j = 0; j < ROT_INFLIGHT; ++j) {
                const int xi = (int)X >> 16, yi = (int)Y >> 16;
                ok[j] = t + j * ROT_TL <= hi && xi >= 0 && xi < W && yi >= 0 && yi < H;
                raw[j] = slice[ok[j] ? yi * W + xi : 0];
                X += dX;
                Y += dY;
            }
#pragma unroll
            for (int j = 0; j < ROT_INFLIGHT; ++j) {
                if (!ok[j]) continue;
                acc = rot_op<MODE>(acc, raw[j]);
                ++cnt;
            }
        }
    }
#pragma unroll
    for (int o = ROT_UL; o < 64; o <<= 1) {      // the 8 lanes of a ray: lane, lane ^ 8, ^ 16, ^ 32
        acc = rot_op<MODE>(acc, __shfl_xor(acc, o, 64));
        cnt += __shfl_xor(cnt, o, 64);
    }
    if (!live || tl != 0) return;
    int v = fill;
    if (cnt > 0) v = MODE == ROT_SUM ? acc / cnt : acc;      // C division: truncates toward zero
    const size_t o = ((size_t)a * N + (size_t)n0 + k) * U + u;
    if (values != nullptr) values[o] = (short)v;
    if (level != nullptr) level[o] = (unsigned char)(int)stored_level((float)(v + add), win_params(wc, ww));
}

template <int MODE, bool LERP>
static void rotate_launch(const short* pix, int K, int H, int W, int n0, int N, const int* coef, int A, int U, int T, int fill,
                          float wc, float ww, int hu, short* values, unsigned char* level, hipStream_t st) {
    const int nseg = (U + ROT_WG_U - 1) / ROT_WG_U;
    hipLaunchKernelGGL((project_rotate_kernel<MODE, LERP>), dim3((unsigned)((long)K * nseg * A)), dim3(ROT_THREADS), 0, st, pix, H, W, n0, N,
                       coef, A, U, T, nseg, fill, wc, ww, hu ? 1024 : 0, values, level);
}

// both entry points: the argument checks and the launch
template <bool LERP>
static int rotate_entry(const short* pix, int K, int H, int W, int n0, int N, const int* coef, int A, int U, int T, int mode, int fill,
                        float wc, float ww, int hu, short* values, unsigned char* level, void* stream) {
    if (pix == nullptr || coef == nullptr || (values == nullptr && level == nullptr)) return CTG_EINVAL;
    if (K < 1 || n0 < 0 || N < 1 || n0 > N - K) return CTG_EINVAL;
    if (H < 1 || H > ROT_MAX_DIM || W < 1 || W > ROT_MAX_DIM || U < 1 || U > ROT_MAX_DIM || T < 1 || T > ROT_MAX_DIM) return CTG_EINVAL;
    if (A < 1 || A > ROT_MAX_DIM || mode < ROT_MAX || mode > ROT_SUM || fill < -32768 || fill > 32767) return CTG_EINVAL;
    if (((uintptr_t)pix & 1) != 0 || ((uintptr_t)coef & 3) != 0 || ((uintptr_t)values & 1) != 0) return CTG_EINVAL;
    // one workgroup per (slice, segment, angle): the grid's x dimension
    if ((long)K * ((U + ROT_WG_U - 1) / ROT_WG_U) * A > 0x7fffffffL) return CTG_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (mode == ROT_MAX) rotate_launch<ROT_MAX, LERP>(pix, K, H, W, n0, N, coef, A, U, T, fill, wc, ww, hu, values, level, st);
    else if (mode == ROT_MIN) rotate_launch<ROT_MIN, LERP>(pix, K, H, W, n0, N, coef, A, U, T, fill, wc, ww, hu, values, level, st);
    else rotate_launch<ROT_SUM, LERP>(pix, K, H, W, n0, N, coef, A, U, T, fill, wc, ww, hu, values, level, st);
    return ctg_launch_status();
}

extern "C" int ctg_project_rotate(const short* pix, int K, int H, int W, int n0, int N, const int* coef, int A, int U, int T,
                                  int mode, int fill, float wc, float ww, int hu, short* values, unsigned char* level,
                                  void* stream) {
    CTG_ENTER();
    return rotate_entry<false>(pix, K, H, W, n0, N, coef, A, U, T, mode, fill, wc, ww, hu, values, level, stream);
}

extern "C" int ctg_project_rotate_bilinear(const short* pix, int K, int H, int W, int n0, int N, const int* coef, int A, int U,
                                           int T, int mode, int fill, float wc, float ww, int hu, short* values,
                                           unsigned char* level, void* stream) {
    CTG_ENTER();
    return rotate_entry<true>(pix, K, H, W, n0, N, coef, A, U, T, mode, fill, wc, ww, hu, values, level, stream);
}

// ------------------------------------------------------------------------------------------------------------ depth of the maximum
__device__ __forceinline__ unsigned rot_key_identity(int mode) { return mode == ROT_MAX ? 0u : 0xffffffffu; }

template <int MODE> __device__ __forceinline__ unsigned rot_key(int v, int t) {
    const unsigned b = (unsigned)(v + 32768) << 16;
    return MODE == ROT_MAX ? b | (65535u - (unsigned)t) : b | (unsigned)t;
}

template <int MODE> __device__ __forceinline__ unsigned rot_key_op(unsigned a, unsigned b) {
    if constexpr (MODE == ROT_MAX) return a > b ? a : b;
    else return a < b ? a : b;
}

// project_rotate_kernel with keys for values: the same table, interval, bounds-checked addresses and "counted" rule
template <int MODE, bool LERP>
__global__ __launch_bounds__(ROT_THREADS) void project_rotate_depth_kernel(const short* __restrict__ pix, int H, int W, int n0, int N,
                                                                           const int* __restrict__ coef, int A, int U, int T, int nseg,
                                                                           int fill, int cue, float wc, float ww, int add,
                                                                           short* __restrict__ values, unsigned char* __restrict__ level,
                                                                           short* __restrict__ depth, unsigned char* __restrict__ cued) {
    static_assert(MODE == ROT_MAX || MODE == ROT_MIN, "a depth exists for max and min only");
    const unsigned a = blockIdx.x % (unsigned)A, rest = blockIdx.x / (unsigned)A;
    const unsigned seg = rest % (unsigned)nseg, k = rest / (unsigned)nseg;
    const int lane = threadIdx.x & 63, tl = lane / ROT_UL;
    const int u = (int)(seg * ROT_WG_U + (threadIdx.x >> 6) * ROT_UL + lane % ROT_UL);
    const bool live = u < U;      // (every lane stays for the shuffles; the 8 lanes of a ray are live together)
    const int* __restrict__ c = coef + (size_t)a * 6;
    const unsigned c2 = (unsigned)c[2], c5 = (unsigned)c[5];
    const unsigned X0 = (unsigned)c[0] + (unsigned)c[1] * (unsigned)u, Y0 = (unsigned)c[3] + (unsigned)c[4] * (unsigned)u;
    int lo = 0, hi = live ? T - 1 : -1;
    rot_clip((int)X0, (int)c2, (W << 16) - 1, lo, hi);
    rot_clip((int)Y0, (int)c5, (H << 16) - 1, lo, hi);
    const short* __restrict__ slice = pix + (size_t)k * H * W;
    unsigned acc = rot_key_identity(MODE);
    int t = (lo & ~(ROT_TL - 1)) + tl;      // lo >= 0
    unsigned X = X0 + c2 * (unsigned)t, Y = Y0 + c5 * (unsigned)t;
    const unsigned dX = c2 * ROT_TL, dY = c5 * ROT_TL;
    for (; t <= hi; t += ROT_TL * ROT_INFLIGHT) {
        bool ok[ROT_INFLIGHT];
        if constexpr (LERP) {
            int p[ROT_INFLIGHT][4], fx[ROT_INFLIGHT], fy[ROT_INFLIGHT];      // 4 ROT_INFLIGHT gathers before the first is used
#pragma unroll
            for (int j = 0; j < ROT_INFLIGHT; ++j) {
                const int xi = (int)X >> 16, yi = (int)Y >> 16;
                ok[j] = t + j * ROT_TL <= hi && xi >= 0 && xi < W && yi >= 0 && yi < H;
                const int Xc = (int)(X - 32768u), Yc = (int)(Y - 32768u);
                fx[j] = (Xc >> 8) & 255;
                fy[j] = (Yc >> 8) & 255;
                const int x0 = Xc >> 16, y0 = Yc >> 16;      // in -32768 .. 32767: x0 + 1 cannot wrap
                const int xa = ok[j] ? rot_clamp(x0, W - 1) : 0, xb = ok[j] ? rot_clamp(x0 + 1, W - 1) : 0;
                const int ra = ok[j] ? rot_clamp(y0, H - 1) * W : 0, rb = ok[j] ? rot_clamp(y0 + 1, H - 1) * W : 0;
                p[j][0] = slice[ra + xa];
                p[j][1] = slice[ra + xb];
                p[j][2] = slice[rb + xa];
                p[j][3] = slice[rb + xb];
                X += dX;
                Y += dY;
            }
#pragma unroll
            for (int j = 0; j < ROT_INFLIGHT; ++j) {
                if (!ok[j]) continue;
                acc = rot_key_op<MODE>(acc, rot_key<MODE>(rot_lerp(p[j][0], p[j][1], p[j][2], p[j][3], fx[j], fy[j]), t + j * ROT_TL));
            }
        } else {
            int raw[ROT_INFLIGHT];
#pragma unroll
            for (int j = 0; j < ROT_INFLIGHT; ++j) {
                const int xi = (int)X >> 16, yi = (int)Y >> 16;
                ok[j] = t + j * ROT_TL <= hi && xi >= 0 && xi < W && yi >= 0 && yi < H;
                raw[j] = slice[ok[j] ? yi * W + xi : 0];
                X += dX;
                Y += dY;
            }
#pragma unroll
            for (int j = 0; j < ROT_INFLIGHT; ++j) {
                if (!ok[j]) continue;
                acc = rot_key_op<MODE>(acc, rot_key<MODE>(raw[j], t + j * ROT_TL));
            }
        }
    }
#pragma unroll
    for (int o = ROT_UL; o < 64; o <<= 1)      // the 8 lanes of a ray: lane, lane ^ 8, ^ 16, ^ 32
        acc = rot_key_op<MODE>(acc, (unsigned)__shfl_xor((int)acc, o, 64));
    if (!live || tl != 0) return;
    int v = fill, d = -1, w = 256;
    if (acc != rot_key_identity(MODE)) {      // a real key never equals the identity (t <= 4095)
        v = (int)(acc >> 16) - 32768;
        d = MODE == ROT_MAX ? 65535 - (int)(acc & 65535u) : (int)(acc & 65535u);
        w = 256 - cue * d / T;
    }
    const size_t o = ((size_t)a * N + (size_t)n0 + k) * U + u;
    if (values != nullptr) values[o] = (short)v;
    if (depth != nullptr) depth[o] = (short)d;
    if (level == nullptr && cued == nullptr) return;
    const int l = (int)stored_level((float)(v + add), win_params(wc, ww));
    if (level != nullptr) level[o] = (unsigned char)l;
    if (cued != nullptr) cued[o] = (unsigned char)((l * w + 128) >> 8);
}

template <int MODE, bool LERP>
static void rotate_depth_launch(const short* pix, int K, int H, int W, int n0, int N, const int* coef, int A, int U, int T, int fill,
                                int cue, float wc, float ww, int hu, short* values, unsigned char* level, short* depth,
                                unsigned char* cued, hipStream_t st) {
    const int nseg = (U + ROT_WG_U - 1) / ROT_WG_U;
    hipLaunchKernelGGL((project_rotate_depth_kernel<MODE, LERP>), dim3((unsigned)((long)K * nseg * A)), dim3(ROT_THREADS), 0, st, pix, H,
                       W, n0, N, coef, A, U, T, nseg, fill, cue, wc, ww, hu ? 1024 : 0, values, level, depth, cued);
}

extern "C" int ctg_project_rotate_depth(const short* pix, int K, int H, int W, int n0, int N, const int* coef, int A, int U, int T,
                                        int mode, int sampling, int fill, int cue, float wc, float ww, int hu, short* values,
                                        unsigned char* level, short* depth, unsigned char* cued, void* stream) {
    CTG_ENTER();
    if (pix == nullptr || coef == nullptr) return CTG_EINVAL;
    if (values == nullptr && level == nullptr && depth == nullptr && cued == nullptr) return CTG_EINVAL;
    if (K < 1 || n0 < 0 || N < 1 || n0 > N - K) return CTG_EINVAL;
    if (H < 1 || H > ROT_MAX_DIM || W < 1 || W > ROT_MAX_DIM || U < 1 || U > ROT_MAX_DIM || T < 1 || T > ROT_MAX_DIM) return CTG_EINVAL;
    if (A < 1 || A > ROT_MAX_DIM || fill < -32768 || fill > 32767) return CTG_EINVAL;
    // a depth exists for max and min only; T <= 4096 is an int16 depth and keeps a key off the identity
    if ((mode != ROT_MAX && mode != ROT_MIN) || sampling < 0 || sampling > 1 || cue < 0 || cue > 256) return CTG_EINVAL;
    if (((uintptr_t)pix & 1) != 0 || ((uintptr_t)coef & 3) != 0 || ((uintptr_t)values & 1) != 0 || ((uintptr_t)depth & 1) != 0)
        return CTG_EINVAL;
    // one workgroup per (slice, segment, angle): the grid's x dimension
    if ((long)K * ((U + ROT_WG_U - 1) / ROT_WG_U) * A > 0x7fffffffL) return CTG_EINVAL;
    hipStream_t st = (hipStream_t)stream;
#define ROT_DEPTH_GO(M, L) rotate_depth_launch<M, L>(pix, K, H, W, n0, N, coef, A, U, T, fill, cue, wc, ww, hu, values, level, depth, cued, st)
    if (mode == ROT_MAX) {
        if (sampling) ROT_DEPTH_GO(ROT_MAX, true);
        else ROT_DEPTH_GO(ROT_MAX, false);
    } else {
        if (sampling) ROT_DEPTH_GO(ROT_MIN, true);
        else ROT_DEPTH_GO(ROT_MIN, false);
    }
#undef ROT_DEPTH_GO
    return ctg_launch_status();
}
