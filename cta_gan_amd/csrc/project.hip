// Series inference, what a reader looks at first: the maximum- / minimum-intensity and mean ("ray-sum") projections of the exported
// int16 volume along the three body axes, accumulated chunk by chunk as the chunks leave ctg_export_slices (cta_gan_amd/infer.py:
// SeriesProjector).  The reference has no counterpart (its test() writes slices only); the 8-bit level of a projection is the tail
// of to_windowdata (trainer/HdTrainer.py:43-61) on the projected stored value, window_arith.h: stored_level.
//
// ctg_project_accumulate is exact int32 arithmetic (max, min, sum of int16): no float, the same bits whatever the arrival order.
// A lane owns 8 consecutive pixels x0 .. x0+7 of a row (x0 a multiple of 8), a wave 512 pixels of it.  A row whose address is
// 16-byte aligned is read with one 16-byte load per lane; any other row (W % 8 != 0, planes of odd H W, a base pointer that is
// only 2-byte aligned) by the same lanes with 2-byte loads, and so are the W % 8 pixels behind the last whole group.  Because the
// lane -> pixel map never depends on the address, the accumulators of a lane stay in registers across slices and rows.
// One launch, two kinds of workgroup (the first row_blocks workgroups of the grid are of the first kind):
//   project_rows         a wave owns (row, 512-pixel segment) and loops over the K slices, PRJ_INFLIGHT loads issued before the
//                        first use.  axial: 8 running values per lane, combined into the slab's plane (plain read-modify-write,
//                        nobody else touches these pixels) when the slab closes or the chunk ends.  sagittal: the row's value by
//                        an in-wave reduction, one int32 atomic per wave and slice (rows wider than 512 have several waves).
//   project_cols         a wave owns (slice, band of PRJ_BAND rows, segment), reduces the band in registers and hands the 512
//                        values through LDS from lane-major to pixel-major order, so that each atomic wave instruction covers
//                        256 contiguous bytes of the coronal row: H / PRJ_BAND atomics per coronal value instead of H.
// Both kinds read the chunk, so it is requested twice within one launch (a chunk of 16 x 512 x 512 is 8 MB: the second request
// is served by the Infinity Cache or L2).
// ctg_project_finish: accumulator -> int16 value (+ the truncating division of the mean) and its 8-bit window level, one pass.
#include "common.h"
#include "window_arith.h"

#define PRJ_THREADS 256
#define PRJ_WAVES (PRJ_THREADS / 64)
#define PRJ_SEG 512        // pixels of a row one wave covers: 64 lanes x 8
#define PRJ_BAND 16        // rows a wave reduces in registers before its coronal atomics
#define PRJ_INFLIGHT 4     // loads a lane issues before it uses the first
#define PRJ_MAX_BLOCKS 2048

enum { PRJ_MAX = 0, PRJ_MIN = 1, PRJ_SUM = 2 };

typedef short i16x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

template <int MODE> __device__ __forceinline__ constexpr int prj_identity() {
    return MODE == PRJ_MAX ? -32768 : (MODE == PRJ_MIN ? 32767 : 0);
}

template <int MODE> __device__ __forceinline__ int prj_op(int a, int b) {
    if constexpr (MODE == PRJ_MAX) return a > b ? a : b;
    else if constexpr (MODE == PRJ_MIN) return a < b ? a : b;
    else return a + b;
}

template <int MODE> __device__ __forceinline__ void prj_atomic(int* p, int v) {
    if constexpr (MODE == PRJ_MAX) atomicMax(p, v);
    else if constexpr (MODE == PRJ_MIN) atomicMin(p, v);
    else atomicAdd(p, v);
}

template <int MODE> __device__ __forceinline__ int prj_wave_reduce(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = prj_op<MODE>(v, __shfl_xor(v, o, 64));
    return v;
}

// pixels p[0 .. cnt-1] of a lane (cnt <= 8), the identity behind them; nothing is read for cnt == 0
template <int MODE> __device__ __forceinline__ i16x8 prj_load8(const short* __restrict__ p, int cnt) {
    if (cnt == 8 && ((uintptr_t)p & 15) == 0) return *reinterpret_cast<const i16x8*>(p);
    i16x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = j < cnt ? p[j] : (short)prj_identity<MODE>();
    return v;
}

// dst[0 .. cnt-1] = op(dst, acc): the pixels belong to this lane alone
template <int MODE> __device__ __forceinline__ void prj_combine8(int* __restrict__ dst, const int (&acc)[8], int cnt) {
    if (cnt == 8 && ((uintptr_t)dst & 15) == 0) {
        i32x4 a = *reinterpret_cast<const i32x4*>(dst), b = *reinterpret_cast<const i32x4*>(dst + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            a[j] = prj_op<MODE>(a[j], acc[j]);
            b[j] = prj_op<MODE>(b[j], acc[4 + j]);
        }
        *reinterpret_cast<i32x4*>(dst) = a;
        *reinterpret_cast<i32x4*>(dst + 4) = b;
        return;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (j < cnt) dst[j] = prj_op<MODE>(dst[j], acc[j]);
}

// one wave per (row y, segment); items = H * nseg
template <int MODE>
__device__ __forceinline__ void project_rows(const short* __restrict__ pix, int K, int H, int W, int nseg, int n0, int thick,
                                             int* __restrict__ axial, int* __restrict__ sagittal, unsigned block) {
    const int lane = threadIdx.x & 63;
    const long item = (long)block * PRJ_WAVES + (threadIdx.x >> 6);
    if (item >= (long)H * nseg) return;      // (no barrier on this path)
    const int y = (int)(item / nseg), seg = (int)(item - (long)y * nseg);
    const int x0 = seg * PRJ_SEG + lane * 8;
    const int cnt = W - x0 >= 8 ? 8 : (W - x0 > 0 ? W - x0 : 0);
    const long HW = (long)H * W;
    const short* __restrict__ row = pix + (long)y * W + x0;
    int acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = prj_identity<MODE>();
    int slab = n0 / thick, left = thick - n0 % thick;      // slices the open slab still takes
    for (int k0 = 0; k0 < K; k0 += PRJ_INFLIGHT) {
        i16x8 raw[PRJ_INFLIGHT];
#pragma unroll
        for (int u = 0; u < PRJ_INFLIGHT; ++u) raw[u] = prj_load8<MODE>(row + (long)(k0 + u) * HW, k0 + u < K ? cnt : 0);
#pragma unroll
        for (int u = 0; u < PRJ_INFLIGHT; ++u) {
            const int k = k0 + u;
            if (k >= K) break;
            int r = prj_identity<MODE>();
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int v = raw[u][j];
                acc[j] = prj_op<MODE>(acc[j], v);
                r = prj_op<MODE>(r, v);
            }
            if (sagittal != nullptr) {
                r = prj_wave_reduce<MODE>(r);
                if (lane == 0) prj_atomic<MODE>(sagittal + (long)(n0 + k) * H + y, r);
            }
            --left;
            if (left == 0 || k == K - 1) {
                if (axial != nullptr && cnt > 0) prj_combine8<MODE>(axial + ((long)slab * H + y) * W + x0, acc, cnt);
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] = prj_identity<MODE>();
                if (left == 0) {
                    ++slab;
                    left = thick;
                }
            }
        }
    }
}

// one wave per (slice k, band of PRJ_BAND rows, segment); items = K * nband * nseg
template <int MODE>
__device__ __forceinline__ void project_cols(const short* __restrict__ pix, int K, int H, int W, int nseg, int nband, int n0,
                                             int* __restrict__ coronal, unsigned block, int (*part)[PRJ_SEG]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long item = (long)block * PRJ_WAVES + wave;
    const bool live = item < (long)K * nband * nseg;      // a dead wave still meets the barrier
    int acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = prj_identity<MODE>();
    int k = 0, seg = 0;
    if (live) {
        seg = (int)(item % nseg);
        const long t = item / nseg;
        const int band = (int)(t % nband);
        k = (int)(t / nband);
        const int x0 = seg * PRJ_SEG + lane * 8;
        const int cnt = W - x0 >= 8 ? 8 : (W - x0 > 0 ? W - x0 : 0);
        const int y0 = band * PRJ_BAND, y1 = y0 + PRJ_BAND < H ? y0 + PRJ_BAND : H;
        const short* __restrict__ col = pix + (long)k * H * W + x0;
        for (int y = y0; y < y1; y += PRJ_INFLIGHT) {
            i16x8 raw[PRJ_INFLIGHT];
#pragma unroll
            for (int u = 0; u < PRJ_INFLIGHT; ++u) raw[u] = prj_load8<MODE>(col + (long)(y + u) * W, y + u < y1 ? cnt : 0);
#pragma unroll
            for (int u = 0; u < PRJ_INFLIGHT; ++u)
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] = prj_op<MODE>(acc[j], raw[u][j]);
        }
    }
    // lane-major -> pixel-major: atomic j of the wave then covers pixels 64 j .. 64 j + 63 of the segment, 256 contiguous bytes
#pragma unroll
    for (int j = 0; j < 8; ++j) part[wave][lane * 8 + j] = acc[j];
    __syncthreads();
    if (!live) return;
    int* __restrict__ dst = coronal + (long)(n0 + k) * W;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int i = j * 64 + lane, x = seg * PRJ_SEG + i;
        if (x < W) prj_atomic<MODE>(dst + x, part[wave][i]);
    }
}

// workgroups 0 .. row_blocks-1: rows (axial, sagittal); the rest: columns (coronal).  A workgroup is of one kind as a whole.
template <int MODE>
__global__ __launch_bounds__(PRJ_THREADS) void project_kernel(const short* __restrict__ pix, int K, int H, int W, int nseg, int nband,
                                                              int n0, int thick, int* __restrict__ axial, int* __restrict__ coronal,
                                                              int* __restrict__ sagittal, unsigned row_blocks) {
    __shared__ int part[PRJ_WAVES][PRJ_SEG];
    if (blockIdx.x < row_blocks) project_rows<MODE>(pix, K, H, W, nseg, n0, thick, axial, sagittal, blockIdx.x);
    else project_cols<MODE>(pix, K, H, W, nseg, nband, n0, coronal, blockIdx.x - row_blocks, part);
}

template <int MODE>
static void project_launch(const short* pix, int K, int H, int W, int n0, int thick, int* axial, int* coronal, int* sagittal,
                           hipStream_t st) {
    const int nseg = (W + PRJ_SEG - 1) / PRJ_SEG, nband = (H + PRJ_BAND - 1) / PRJ_BAND;
    const long row_items = (axial != nullptr || sagittal != nullptr) ? (long)H * nseg : 0;
    const long col_items = coronal != nullptr ? (long)K * nband * nseg : 0;
    const unsigned row_blocks = (unsigned)((row_items + PRJ_WAVES - 1) / PRJ_WAVES);
    const unsigned col_blocks = (unsigned)((col_items + PRJ_WAVES - 1) / PRJ_WAVES);
    hipLaunchKernelGGL(project_kernel<MODE>, dim3(row_blocks + col_blocks), dim3(PRJ_THREADS), 0, st, pix, K, H, W, nseg, nband, n0,
                       thick, axial, coronal, sagittal, row_blocks);
}

extern "C" int ctg_project_accumulate(const short* pix, int K, int H, int W, int n0, int thick, int mode, int* axial, int* coronal,
                                      int* sagittal, void* stream) {
    CTG_ENTER();
    if (pix == nullptr || (axial == nullptr && coronal == nullptr && sagittal == nullptr)) return CTG_EINVAL;
    // 65535 x 32767 < 2^31: a sum over fewer than 65536 int16 values stays inside int32
    if (K < 1 || K > 65535 || H < 1 || H > 65535 || W < 1 || W > 65535 || thick < 1 || thick > 65535) return CTG_EINVAL;
    if (n0 < 0 || n0 > (1 << 30) || mode < PRJ_MAX || mode > PRJ_SUM) return CTG_EINVAL;
    // (the widest grid: one wave per slice, band and segment)
    if ((long)K * ((H + PRJ_BAND - 1) / PRJ_BAND) * ((W + PRJ_SEG - 1) / PRJ_SEG) > (1L << 31)) return CTG_EINVAL;
    if (((uintptr_t)pix & 1) != 0 || (((uintptr_t)axial | (uintptr_t)coronal | (uintptr_t)sagittal) & 3) != 0) return CTG_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (mode == PRJ_MAX) project_launch<PRJ_MAX>(pix, K, H, W, n0, thick, axial, coronal, sagittal, st);
    else if (mode == PRJ_MIN) project_launch<PRJ_MIN>(pix, K, H, W, n0, thick, axial, coronal, sagittal, st);
    else project_launch<PRJ_SUM>(pix, K, H, W, n0, thick, axial, coronal, sagittal, st);
    return ctg_launch_status();
}

// ------------------------------------------------------------------------------------------------------------ finish
__device__ __forceinline__ int finish_value(int a, long i, long last0, int mode, int div, int div_last) {
    if (mode == PRJ_SUM) a = a / (i >= last0 ? div_last : div);      // C division: truncates toward zero
    a = a > 32767 ? 32767 : a;
    return a < -32768 ? -32768 : a;
}

__device__ __forceinline__ unsigned finish_level(int v, int add, const WinParams p) {
    return (unsigned)(int)stored_level((float)(v + add), p);
}

// 8 items per lane where all three addresses allow it (vec), the rest one by one
__global__ __launch_bounds__(PRJ_THREADS) void project_finish_kernel(const int* __restrict__ acc, long total, long last0, int mode,
                                                                     int div, int div_last, float wc, float ww, int add,
                                                                     short* __restrict__ values, unsigned char* __restrict__ level,
                                                                     int vec) {
    WinParams p = {0.f, 0.f};
    if (level != nullptr) p = win_params(wc, ww);
    const long nvec = vec ? total >> 3 : 0;
    const long t = (long)blockIdx.x * PRJ_THREADS + threadIdx.x, step = (long)gridDim.x * PRJ_THREADS;
    for (long g = t; g < nvec; g += step) {
        const long i = 8 * g;
        const i32x4 a = *reinterpret_cast<const i32x4*>(acc + i), b = *reinterpret_cast<const i32x4*>(acc + i + 4);
        int v[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] = finish_value(a[j], i + j, last0, mode, div, div_last);
            v[4 + j] = finish_value(b[j], i + 4 + j, last0, mode, div, div_last);
        }
        if (values != nullptr) {
            i16x8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = (short)v[j];
            *reinterpret_cast<i16x8*>(values + i) = o;
        }
        if (level != nullptr) {
            unsigned lo = 0, hi = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                lo |= finish_level(v[j], add, p) << (8 * j);
                hi |= finish_level(v[4 + j], add, p) << (8 * j);
            }
            *reinterpret_cast<u32x2*>(level + i) = u32x2{lo, hi};
        }
    }
    for (long i = 8 * nvec + t; i < total; i += step) {
        const int v = finish_value(acc[i], i, last0, mode, div, div_last);
        if (values != nullptr) values[i] = (short)v;
        if (level != nullptr) level[i] = (unsigned char)finish_level(v, add, p);
    }
}

extern "C" int ctg_project_finish(const int* acc, int planes, long plane_items, int mode, int div, int div_last, float wc, float ww,
                                  int hu, short* values, unsigned char* level, void* stream) {
    CTG_ENTER();
    if (acc == nullptr || (values == nullptr && level == nullptr) || planes < 1 || plane_items < 1) return CTG_EINVAL;
    if (mode < PRJ_MAX || mode > PRJ_SUM || (mode == PRJ_SUM && (div < 1 || div_last < 1))) return CTG_EINVAL;
    if (plane_items > (1L << 40) / planes || ((uintptr_t)acc & 3) != 0 || ((uintptr_t)values & 1) != 0) return CTG_EINVAL;
    const long total = (long)planes * plane_items;
    const int vec = ((uintptr_t)acc & 15) == 0 && ((uintptr_t)values & 15) == 0 && ((uintptr_t)level & 7) == 0;
    long blocks = ((total + 7) / 8 + PRJ_THREADS - 1) / PRJ_THREADS;
    blocks = blocks < 1 ? 1 : (blocks < PRJ_MAX_BLOCKS ? blocks : PRJ_MAX_BLOCKS);
    hipLaunchKernelGGL(project_finish_kernel, dim3((unsigned)blocks), dim3(PRJ_THREADS), 0, (hipStream_t)stream, acc, total,
                       (long)(planes - 1) * plane_items, mode, div, div_last, wc, ww, hu ? 1024 : 0, values, level, vec);
    return ctg_launch_status();
}

// ------------------------------------------------------------------------------------------------------------ depth of the maximum
// ctg_project_accumulate_depth / ctg_project_finish_depth: for mode max and min a projection also reports where along the projected
// axis its value was found -- the smallest voxel coordinate that attains it (np.argmax / np.argmin over the axis): the slice n
// (axial; global, also with slabs), the row y (coronal), the column x (sagittal).  An accumulator item is one 32-bit key whose
// unsigned order is "better value first, then smaller coordinate":
//     b = value + 32768 (0 .. 65535);   max: key = b << 16 | (65535 - d), unsigned max, identity 0
//                                       min: key = b << 16 | d,           unsigned min, identity 0xffffffff
// so the lane -> pixel map, the two kinds of workgroup, the in-wave reduction, the LDS hand-over and the atomics are those of
// project_rows / project_cols above on keys instead of values (kernels of their own: the plain ones are not touched).  A pixel
// behind the end of a row takes no part: its key is the identity.  d <= 32766 keeps a real key off the identity.
template <int MODE> __device__ __forceinline__ constexpr unsigned prk_identity() { return MODE == PRJ_MAX ? 0u : 0xffffffffu; }

template <int MODE> __device__ __forceinline__ unsigned prk_key(int v, int d) {
    const unsigned b = (unsigned)(v + 32768) << 16;
    return MODE == PRJ_MAX ? b | (65535u - (unsigned)d) : b | (unsigned)d;
}

template <int MODE> __device__ __forceinline__ unsigned prk_op(unsigned a, unsigned b) {
    if constexpr (MODE == PRJ_MAX) return a > b ? a : b;
    else return a < b ? a : b;
}

template <int MODE> __device__ __forceinline__ void prk_atomic(unsigned* p, unsigned v) {
    if constexpr (MODE == PRJ_MAX) atomicMax(p, v);
    else atomicMin(p, v);
}

template <int MODE> __device__ __forceinline__ unsigned prk_wave_reduce(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = prk_op<MODE>(v, (unsigned)__shfl_xor((int)v, o, 64));
    return v;
}

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// dst[0 .. cnt-1] = op(dst, acc): the pixels belong to this lane alone
template <int MODE> __device__ __forceinline__ void prk_combine8(unsigned* __restrict__ dst, const unsigned (&acc)[8], int cnt) {
    if (cnt == 8 && ((uintptr_t)dst & 15) == 0) {
        u32x4 a = *reinterpret_cast<const u32x4*>(dst), b = *reinterpret_cast<const u32x4*>(dst + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            a[j] = prk_op<MODE>(a[j], acc[j]);
            b[j] = prk_op<MODE>(b[j], acc[4 + j]);
        }
        *reinterpret_cast<u32x4*>(dst) = a;
        *reinterpret_cast<u32x4*>(dst + 4) = b;
        return;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (j < cnt) dst[j] = prk_op<MODE>(dst[j], acc[j]);
}

// one wave per (row y, segment); items = H * nseg.  axial keys carry n0 + k, sagittal keys the pixel's x
template <int MODE>
__device__ __forceinline__ void project_rows_depth(const short* __restrict__ pix, int K, int H, int W, int nseg, int n0, int thick,
                                                   unsigned* __restrict__ axial, unsigned* __restrict__ sagittal, unsigned block) {
    const int lane = threadIdx.x & 63;
    const long item = (long)block * PRJ_WAVES + (threadIdx.x >> 6);
    if (item >= (long)H * nseg) return;      // (no barrier on this path)
    const int y = (int)(item / nseg), seg = (int)(item - (long)y * nseg);
    const int x0 = seg * PRJ_SEG + lane * 8;
    const int cnt = W - x0 >= 8 ? 8 : (W - x0 > 0 ? W - x0 : 0);
    const long HW = (long)H * W;
    const short* __restrict__ row = pix + (long)y * W + x0;
    unsigned acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = prk_identity<MODE>();
    int slab = n0 / thick, left = thick - n0 % thick;      // slices the open slab still takes
    for (int k0 = 0; k0 < K; k0 += PRJ_INFLIGHT) {
        i16x8 raw[PRJ_INFLIGHT];
#pragma unroll
        for (int u = 0; u < PRJ_INFLIGHT; ++u) raw[u] = prj_load8<MODE>(row + (long)(k0 + u) * HW, k0 + u < K ? cnt : 0);
#pragma unroll
        for (int u = 0; u < PRJ_INFLIGHT; ++u) {
            const int k = k0 + u;
            if (k >= K) break;
            unsigned r = prk_identity<MODE>();
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int v = raw[u][j];
                if (j < cnt) {
                    acc[j] = prk_op<MODE>(acc[j], prk_key<MODE>(v, n0 + k));
                    r = prk_op<MODE>(r, prk_key<MODE>(v, x0 + j));
                }
            }
            if (sagittal != nullptr) {
                r = prk_wave_reduce<MODE>(r);
                if (lane == 0) prk_atomic<MODE>(sagittal + (long)(n0 + k) * H + y, r);
            }
            --left;
            if (left == 0 || k == K - 1) {
                if (axial != nullptr && cnt > 0) prk_combine8<MODE>(axial + ((long)slab * H + y) * W + x0, acc, cnt);
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] = prk_identity<MODE>();
                if (left == 0) {
                    ++slab;
                    left = thick;
                }
            }
        }
    }
}

// one wave per (slice k, band of PRJ_BAND rows, segment); items = K * nband * nseg.  coronal keys carry the band loop's row y
template <int MODE>
__device__ __forceinline__ void project_cols_depth(const short* __restrict__ pix, int K, int H, int W, int nseg, int nband, int n0,
                                                   unsigned* __restrict__ coronal, unsigned block, unsigned (*part)[PRJ_SEG]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long item = (long)block * PRJ_WAVES + wave;
    const bool live = item < (long)K * nband * nseg;      // a dead wave still meets the barrier
    unsigned acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = prk_identity<MODE>();
    int k = 0, seg = 0;
    if (live) {
        seg = (int)(item % nseg);
        const long t = item / nseg;
        const int band = (int)(t % nband);
        k = (int)(t / nband);
        const int x0 = seg * PRJ_SEG + lane * 8;
        const int cnt = W - x0 >= 8 ? 8 : (W - x0 > 0 ? W - x0 : 0);
        const int y0 = band * PRJ_BAND, y1 = y0 + PRJ_BAND < H ? y0 + PRJ_BAND : H;
        const short* __restrict__ col = pix + (long)k * H * W + x0;
        for (int y = y0; y < y1; y += PRJ_INFLIGHT) {
            i16x8 raw[PRJ_INFLIGHT];
#pragma unroll
            for (int u = 0; u < PRJ_INFLIGHT; ++u) raw[u] = prj_load8<MODE>(col + (long)(y + u) * W, y + u < y1 ? cnt : 0);
#pragma unroll
            for (int u = 0; u < PRJ_INFLIGHT; ++u)
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (y + u < y1 && j < cnt) acc[j] = prk_op<MODE>(acc[j], prk_key<MODE>(raw[u][j], y + u));
        }
    }
    // lane-major -> pixel-major: atomic j of the wave then covers pixels 64 j .. 64 j + 63 of the segment, 256 contiguous bytes
#pragma unroll
    for (int j = 0; j < 8; ++j) part[wave][lane * 8 + j] = acc[j];
    __syncthreads();
    if (!live) return;
    unsigned* __restrict__ dst = coronal + (long)(n0 + k) * W;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int i = j * 64 + lane, x = seg * PRJ_SEG + i;
        if (x < W) prk_atomic<MODE>(dst + x, part[wave][i]);
    }
}

template <int MODE>
__global__ __launch_bounds__(PRJ_THREADS) void project_depth_kernel(const short* __restrict__ pix, int K, int H, int W, int nseg,
                                                                    int nband, int n0, int thick, unsigned* __restrict__ axial,
                                                                    unsigned* __restrict__ coronal, unsigned* __restrict__ sagittal,
                                                                    unsigned row_blocks) {
    __shared__ unsigned part[PRJ_WAVES][PRJ_SEG];
    if (blockIdx.x < row_blocks) project_rows_depth<MODE>(pix, K, H, W, nseg, n0, thick, axial, sagittal, blockIdx.x);
    else project_cols_depth<MODE>(pix, K, H, W, nseg, nband, n0, coronal, blockIdx.x - row_blocks, part);
}

template <int MODE>
static void project_depth_launch(const short* pix, int K, int H, int W, int n0, int thick, int* axial, int* coronal, int* sagittal,
                                 hipStream_t st) {
    const int nseg = (W + PRJ_SEG - 1) / PRJ_SEG, nband = (H + PRJ_BAND - 1) / PRJ_BAND;
    const long row_items = (axial != nullptr || sagittal != nullptr) ? (long)H * nseg : 0;
    const long col_items = coronal != nullptr ? (long)K * nband * nseg : 0;
    const unsigned row_blocks = (unsigned)((row_items + PRJ_WAVES - 1) / PRJ_WAVES);
    const unsigned col_blocks = (unsigned)((col_items + PRJ_WAVES - 1) / PRJ_WAVES);
    hipLaunchKernelGGL(project_depth_kernel<MODE>, dim3(row_blocks + col_blocks), dim3(PRJ_THREADS), 0, st, pix, K, H, W, nseg, nband,
                       n0, thick, (unsigned*)axial, (unsigned*)coronal, (unsigned*)sagittal, row_blocks);
}

extern "C" int ctg_project_accumulate_depth(const short* pix, int K, int H, int W, int n0, int thick, int mode, int* axial,
                                            int* coronal, int* sagittal, void* stream) {
    CTG_ENTER();
    if (pix == nullptr || (axial == nullptr && coronal == nullptr && sagittal == nullptr)) return CTG_EINVAL;
    if (K < 1 || K > 65535 || H < 1 || W < 1 || thick < 1 || thick > 65535) return CTG_EINVAL;
    // a depth exists for max and min only, and is an int16: no axis extent above 32767 (which also keeps a key off the identity)
    if ((mode != PRJ_MAX && mode != PRJ_MIN) || n0 < 0 || n0 > 32767 - K || H > 32767 || W > 32767) return CTG_EINVAL;
    if ((long)K * ((H + PRJ_BAND - 1) / PRJ_BAND) * ((W + PRJ_SEG - 1) / PRJ_SEG) > (1L << 31)) return CTG_EINVAL;
    if (((uintptr_t)pix & 1) != 0 || (((uintptr_t)axial | (uintptr_t)coronal | (uintptr_t)sagittal) & 3) != 0) return CTG_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (mode == PRJ_MAX) project_depth_launch<PRJ_MAX>(pix, K, H, W, n0, thick, axial, coronal, sagittal, st);
    else project_depth_launch<PRJ_MIN>(pix, K, H, W, n0, thick, axial, coronal, sagittal, st);
    return ctg_launch_status();
}

// keyed accumulator -> value, level, depth, depth-cued level.  Plane s of the accumulator is a ray bundle of its own: its rays
// start at coordinate s thick and are E = min(thick, extent - s thick) long (axial: the slab's clipped thickness; coronal and
// sagittal: planes = 1 and thick = extent = H / W).  d = depth - s thick, w = 256 - (cue d) / E, cued = (level w + 128) >> 8.
// An item no chunk has reached still holds the identity: the mode's identity value, depth -1, w = 256.
__global__ __launch_bounds__(PRJ_THREADS) void project_finish_depth_kernel(const unsigned* __restrict__ acc, long total, long plane_items,
                                                                           int mode, int thick, int extent, int cue, float wc, float ww,
                                                                           int add, short* __restrict__ values,
                                                                           unsigned char* __restrict__ level, short* __restrict__ depth,
                                                                           unsigned char* __restrict__ cued) {
    WinParams p = {0.f, 0.f};
    if (level != nullptr || cued != nullptr) p = win_params(wc, ww);
    const unsigned identity = mode == PRJ_MAX ? 0u : 0xffffffffu;
    const long t = (long)blockIdx.x * PRJ_THREADS + threadIdx.x, step = (long)gridDim.x * PRJ_THREADS;
    for (long i = t; i < total; i += step) {
        const unsigned key = acc[i];
        const int v = (int)(key >> 16) - 32768;
        int d = -1, w = 256;
        if (key != identity) {
            d = mode == PRJ_MAX ? 65535 - (int)(key & 65535u) : (int)(key & 65535u);
            const int start = (int)(i / plane_items) * thick;
            const int len = extent - start < thick ? extent - start : thick;
            w = 256 - cue * (d - start) / len;
            w = w < 1 ? 1 : (w > 256 ? 256 : w);      // (a key that belongs to another plan than thick / extent: stay in range)
        }
        if (values != nullptr) values[i] = (short)v;
        if (depth != nullptr) depth[i] = (short)d;
        if (level == nullptr && cued == nullptr) continue;
        const int l = (int)finish_level(v, add, p);
        if (level != nullptr) level[i] = (unsigned char)l;
        if (cued != nullptr) cued[i] = (unsigned char)((l * w + 128) >> 8);
    }
}

extern "C" int ctg_project_finish_depth(const int* acc, int planes, long plane_items, int mode, int thick, int extent, int cue,
                                        float wc, float ww, int hu, short* values, unsigned char* level, short* depth,
                                        unsigned char* cued, void* stream) {
    CTG_ENTER();
    if (acc == nullptr || planes < 1 || plane_items < 1) return CTG_EINVAL;
    if (values == nullptr && level == nullptr && depth == nullptr && cued == nullptr) return CTG_EINVAL;
    if ((mode != PRJ_MAX && mode != PRJ_MIN) || cue < 0 || cue > 256) return CTG_EINVAL;
    // every plane starts inside the axis: its rays are at least one voxel long
    if (thick < 1 || extent < 1 || extent > 32767 || (long)(planes - 1) * thick >= extent) return CTG_EINVAL;
    if (plane_items > (1L << 40) / planes || ((uintptr_t)acc & 3) != 0 || ((uintptr_t)values & 1) != 0 || ((uintptr_t)depth & 1) != 0)
        return CTG_EINVAL;
    const long total = (long)planes * plane_items;
    long blocks = (total + PRJ_THREADS - 1) / PRJ_THREADS;
    blocks = blocks < 1 ? 1 : (blocks < PRJ_MAX_BLOCKS ? blocks : PRJ_MAX_BLOCKS);
    hipLaunchKernelGGL(project_finish_depth_kernel, dim3((unsigned)blocks), dim3(PRJ_THREADS), 0, (hipStream_t)stream,
                       (const unsigned*)acc, total, plane_items, mode, thick, extent, cue, wc, ww, hu ? 1024 : 0, values, level, depth,
                       cued);
    return ctg_launch_status();
}
