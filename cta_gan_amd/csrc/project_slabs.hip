// Series inference, the mode a CTA is read in: sliding thin-slab projections (STS-MIP / MinIP / mean) of the exported int16
// volume along the three body axes (cta_gan_amd/infer.py: SeriesSlabs).  project.hip has the whole-volume projections and the
// axial slabs that do not overlap; like them the reference has no counterpart (its test() writes slices only).
//
// One rule for every axis.  Along an axis of extent L, slabs of T voxels (T clipped to L) move on by S voxels, 1 <= S <= T:
// slab j covers [j S, min(j S + T, L)), J = 1 if L <= T, else ceil((L - T) / S) + 1 slabs.  Only the last slab can be short and
// its mean has its own divisor; with S == T this is the plan of ctg_project_accumulate.  (j S < L for every j < J.)
//
// ctg_project_slabs_inplane: slabs along y (coronal, out[j][n][x]) or along x (sagittal, out[j][n][y]).  A row out[j][n][.]
// depends on slice n alone, as a row of a rotated view does, so a chunk of K slices finishes rows n0 .. n0+K-1 of every slab plane
// in one launch: no accumulator, no atomics, no identity fill, no finish pass; the 8-bit level (window_arith.h: stored_level) is
// written in the same pass.  Both kernels re-reduce the T lines of every slab directly (the chunk is what ctg_export_slices has
// just written: the T / S re-reads are served by L2) and write every output byte once:
//   slabs_rows_kernel  coronal.  A wave owns (slice, slab, 512-pixel segment), a lane 8 consecutive pixels x0 .. x0+7 (x0 a
//                      multiple of 8) as in project.hip: 16-byte loads where the row's address allows, 2-byte loads by the same
//                      lanes where it does not (the lane -> pixel map never depends on the address), SLB_INFLIGHT loads issued
//                      before the first use; one 16-byte store of values and one 8-byte store of levels per lane.
//   slabs_cols_kernel  sagittal: the reduction runs along x, the output rows along y.  A workgroup owns (slice, band of 64 rows,
//                      group of 32 neighbouring slabs).  It walks the columns the group needs in chunks of 256, each staged in
//                      LDS by coalesced loads (8 pixels per lane along x); then lane = row and wave = 8 slabs of the group:
//                      every lane reduces its row's part of each of its slabs out of LDS (the row pitch is an odd number of
//                      dwords: the 64 rows of one column lie in 64 different banks).  The 32 x 64 results go through LDS once more,
//                      slab-major with y contiguous, so that a lane stores 8 neighbouring y of one slab: 16 bytes of values.
//                      Neighbouring groups share T - S columns only.
// ctg_project_accumulate_sliding: the axial slabs, chunk by chunk.  int32 accumulators [J][H][W] that hold the mode's identity;
// slice n is combined into every slab j with j S <= n < j S + T.  A wave owns (slab, row, segment), reduces the slab's slices of
// this chunk in registers and combines them into the accumulator by a plain read-modify-write (nobody else touches these pixels
// in this launch, and the launches of one volume are ordered on one stream).  max, min and sum of integers are exact and
// commutative: chunks may arrive in any order, and with S == T the accumulators equal ctg_project_accumulate's bit for bit.
// ctg_project_finish finishes them unchanged.
// On a 16 x 512 x 512 chunk at (T, S) = (10, 5) / (10, 1) the kernels take 5.8 / 11.4 us (coronal), 11.2 / 24.7 us (sagittal) and
// 5.8 / 12.5 us (axial), ctg_project_accumulate's axial pass 6.0 us on the same chunk (LAB_NOTES section 19).  No sliding-window
// scheme (blocks of gcd(T, S) lines, van Herk prefix / suffix maxima) was measured against this baseline, so none is here.
// The small helpers (op, identity, 8-pixel load, 8-pixel combine) repeat project.hip's on purpose: that file stays as it is.
#include "common.h"
#include "window_arith.h"

#define SLB_THREADS 256
#define SLB_WAVES (SLB_THREADS / 64)
#define SLB_SEG 512          // pixels of a row one wave covers: 64 lanes x 8
#define SLB_INFLIGHT 4       // loads a lane issues before it uses the first
#define SLB_ROWS 64          // rows of a sagittal tile: one per lane
#define SLB_SPW 8            // slabs a wave of the sagittal kernel reduces
#define SLB_GROUP (SLB_WAVES * SLB_SPW)
#define SLB_CW 256           // columns of a sagittal tile
#define SLB_PITCH (SLB_CW / 2 + 1)      // dwords per tile row (two pixels per dword), odd
#define SLB_MAX_DIM 65535

enum { SLB_MAX = 0, SLB_MIN = 1, SLB_SUM = 2 };
enum { SLB_CORONAL = 0, SLB_SAGITTAL = 1 };

typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef int s32x4 __attribute__((ext_vector_type(4)));
typedef unsigned slb_u32x2 __attribute__((ext_vector_type(2)));

// J of the rule above; T already clipped to L
static inline int slab_count(int L, int T, int S) { return L <= T ? 1 : (L - T + S - 1) / S + 1; }

template <int MODE> __device__ __forceinline__ constexpr int slb_identity() {
    return MODE == SLB_MAX ? -32768 : (MODE == SLB_MIN ? 32767 : 0);
}

template <int MODE> __device__ __forceinline__ int slb_op(int a, int b) {
    if constexpr (MODE == SLB_MAX) return a > b ? a : b;
    else if constexpr (MODE == SLB_MIN) return a < b ? a : b;
    else return a + b;
}

// pixels p[0 .. cnt-1] of a lane (cnt <= 8), the identity behind them; nothing is read for cnt == 0
template <int MODE> __device__ __forceinline__ s16x8 slb_load8(const short* __restrict__ p, int cnt) {
    if (cnt == 8 && ((uintptr_t)p & 15) == 0) return *reinterpret_cast<const s16x8*>(p);
    s16x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = j < cnt ? p[j] : (short)slb_identity<MODE>();
    return v;
}

// items o .. o+cnt-1 of both outputs (cnt <= 8) from v: wide stores where all 8 are wanted and the address allows
__device__ __forceinline__ void slb_store8(short* __restrict__ values, unsigned char* __restrict__ level, size_t o,
                                           const int (&v)[8], int cnt, int add, const WinParams p) {
    if (values != nullptr) {
        short* dst = values + o;
        if (cnt == 8 && ((uintptr_t)dst & 15) == 0) {
            s16x8 q;
#pragma unroll
            for (int j = 0; j < 8; ++j) q[j] = (short)v[j];
            *reinterpret_cast<s16x8*>(dst) = q;
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < cnt) dst[j] = (short)v[j];
        }
    }
    if (level != nullptr) {
        unsigned char* dst = level + o;
        unsigned l[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) l[j] = (unsigned)(int)stored_level((float)(v[j] + add), p);
        if (cnt == 8 && ((uintptr_t)dst & 7) == 0) {
            *reinterpret_cast<slb_u32x2*>(dst) =
                slb_u32x2{l[0] | l[1] << 8 | l[2] << 16 | l[3] << 24, l[4] | l[5] << 8 | l[6] << 16 | l[7] << 24};
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < cnt) dst[j] = (unsigned char)l[j];
        }
    }
}

// ---------------------------------------------------------------------------------------------------- coronal: slabs along y
// one wave per (slice k, slab j, segment); items = K * J * nseg, the segment fastest
template <int MODE>
__global__ __launch_bounds__(SLB_THREADS) void slabs_rows_kernel(const short* __restrict__ pix, int K, int H, int W, int nseg, int n0,
                                                                 int N, int J, int T, int S, float wc, float ww, int add,
                                                                 short* __restrict__ values, unsigned char* __restrict__ level) {
    const int lane = threadIdx.x & 63;
    const long item = (long)blockIdx.x * SLB_WAVES + (threadIdx.x >> 6);
    if (item >= (long)K * J * nseg) return;      // (no barrier in this kernel)
    const int seg = (int)(item % nseg);
    const long t = item / nseg;
    const int j = (int)(t % J), k = (int)(t / J);
    const int x0 = seg * SLB_SEG + lane * 8;
    const int cnt = W - x0 >= 8 ? 8 : (W - x0 > 0 ? W - x0 : 0);
    if (cnt == 0) return;
    const int y0 = j * S, y1 = y0 + T < H ? y0 + T : H;
    const short* __restrict__ col = pix + (size_t)k * H * W + x0;
    int acc[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = slb_identity<MODE>();
    for (int y = y0; y < y1; y += SLB_INFLIGHT) {
        s16x8 raw[SLB_INFLIGHT];
#pragma unroll
        for (int u = 0; u < SLB_INFLIGHT; ++u) raw[u] = slb_load8<MODE>(col + (size_t)(y + u) * W, y + u < y1 ? cnt : 0);
#pragma unroll
        for (int u = 0; u < SLB_INFLIGHT; ++u)
#pragma unroll
            for (int q = 0; q < 8; ++q) acc[q] = slb_op<MODE>(acc[q], raw[u][q]);
    }
    if constexpr (MODE == SLB_SUM) {
        const int div = y1 - y0;      // the slab's own length; C division truncates toward zero
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[q] /= div;
    }
    WinParams p = {0.f, 0.f};
    if (level != nullptr) p = win_params(wc, ww);
    slb_store8(values, level, ((size_t)j * N + (size_t)(n0 + k)) * W + x0, acc, cnt, add, p);
}

// --------------------------------------------------------------------------------------------------- sagittal: slabs along x
// one workgroup per (slice k, band of SLB_ROWS rows, group of SLB_GROUP slabs); the group fastest
template <int MODE>
__global__ __launch_bounds__(SLB_THREADS) void slabs_cols_kernel(const short* __restrict__ pix, int H, int W, int nband, int ngroup,
                                                                 int n0, int N, int J, int T, int S, float wc, float ww, int add,
                                                                 short* __restrict__ values, unsigned char* __restrict__ level) {
    __shared__ unsigned tile[SLB_ROWS * SLB_PITCH];      // two pixels per dword: x even in the low half
    __shared__ __attribute__((aligned(16))) short res[SLB_GROUP][SLB_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned group = blockIdx.x % (unsigned)ngroup, rest = blockIdx.x / (unsigned)ngroup;
    const int band = (int)(rest % (unsigned)nband), k = (int)(rest / (unsigned)nband);
    const int j0 = (int)group * SLB_GROUP, ya = band * SLB_ROWS;
    const int jl = j0 + SLB_GROUP - 1 < J - 1 ? j0 + SLB_GROUP - 1 : J - 1;      // the group's last slab (j0 < J by the grid)
    const int xe = jl * S + T < W ? jl * S + T : W;                              // the columns the group needs end here
    const short* __restrict__ slice = pix + (size_t)k * H * W;
    int acc[SLB_SPW];
#pragma unroll
    for (int i = 0; i < SLB_SPW; ++i) acc[i] = slb_identity<MODE>();
    const int jw = j0 + wave * SLB_SPW;
    // chunks start at a multiple of 8 pixels: which pixels a lane loads is fixed by x, not by the address
    for (int c0 = (j0 * S) & ~7; c0 < xe; c0 += SLB_CW) {
        const int gc = tid & 31;                          // 8-pixel group of the chunk
        const int x = c0 + gc * 8;
        s16x8 raw[SLB_ROWS / 8];
#pragma unroll
        for (int i = 0; i < SLB_ROWS / 8; ++i) {
            const int y = ya + (tid >> 5) + 8 * i;
            const int cnt = y < H ? (xe - x >= 8 ? 8 : (xe - x > 0 ? xe - x : 0)) : 0;
            raw[i] = slb_load8<MODE>(slice + (size_t)y * W + x, cnt);
        }
#pragma unroll
        for (int i = 0; i < SLB_ROWS / 8; ++i) {
            unsigned* dst = tile + ((tid >> 5) + 8 * i) * SLB_PITCH + gc * 4;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                dst[q] = (unsigned)(unsigned short)raw[i][2 * q] | (unsigned)(unsigned short)raw[i][2 * q + 1] << 16;
        }
        __syncthreads();
        const unsigned* __restrict__ trow = tile + lane * SLB_PITCH;
#pragma unroll
        for (int i = 0; i < SLB_SPW; ++i) {
            const int j = jw + i;      // wave-uniform, and so are the bounds of the loop below
            if (j >= J) break;
            const int a = (j * S > c0 ? j * S : c0) - c0;
            int b = j * S + T < W ? j * S + T : W;
            b = (b < c0 + SLB_CW ? b : c0 + SLB_CW) - c0;
            for (int xx = a; xx < b; ++xx)
                acc[i] = slb_op<MODE>(acc[i], (int)(short)(trow[xx >> 1] >> ((xx & 1) * 16)));
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < SLB_SPW; ++i) {
        const int j = jw + i;
        int v = acc[i];
        if constexpr (MODE == SLB_SUM) {
            if (j < J) v /= (j * S + T < W ? j * S + T : W) - j * S;      // the slab's own length
        }
        res[wave * SLB_SPW + i][lane] = (short)v;      // (a row past H or a slab past J: never stored)
    }
    __syncthreads();
    // slab-major -> y-major: a lane takes 8 neighbouring rows of one slab
    const int g = tid >> 3, r0 = (tid & 7) * 8, j = j0 + g;
    const int cnt = H - (ya + r0) >= 8 ? 8 : (H - (ya + r0) > 0 ? H - (ya + r0) : 0);
    if (j >= J || cnt == 0) return;
    const s16x8 r = *reinterpret_cast<const s16x8*>(&res[g][r0]);
    int v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = r[q];
    WinParams p = {0.f, 0.f};
    if (level != nullptr) p = win_params(wc, ww);
    slb_store8(values, level, ((size_t)j * N + (size_t)(n0 + k)) * H + ya + r0, v, cnt, add, p);
}

template <int MODE>
static void inplane_launch(const short* pix, int K, int H, int W, int n0, int N, int axis, int J, int T, int S, float wc, float ww,
                           int hu, short* values, unsigned char* level, long blocks, hipStream_t st) {
    const int add = hu ? 1024 : 0;
    if (axis == SLB_CORONAL)
        hipLaunchKernelGGL(slabs_rows_kernel<MODE>, dim3((unsigned)blocks), dim3(SLB_THREADS), 0, st, pix, K, H, W,
                           (W + SLB_SEG - 1) / SLB_SEG, n0, N, J, T, S, wc, ww, add, values, level);
    else
        hipLaunchKernelGGL(slabs_cols_kernel<MODE>, dim3((unsigned)blocks), dim3(SLB_THREADS), 0, st, pix, H, W,
                           (H + SLB_ROWS - 1) / SLB_ROWS, (J + SLB_GROUP - 1) / SLB_GROUP, n0, N, J, T, S, wc, ww, add, values, level);
}

extern "C" int ctg_project_slabs_inplane(const short* pix, int K, int H, int W, int n0, int N, int axis, int thick, int step,
                                         int mode, float wc, float ww, int hu, short* values, unsigned char* level, void* stream) {
    CTG_ENTER();
    if (pix == nullptr || (values == nullptr && level == nullptr)) return CTG_EINVAL;
    if (K < 1 || K > SLB_MAX_DIM || H < 1 || H > SLB_MAX_DIM || W < 1 || W > SLB_MAX_DIM || N < 1 || N > SLB_MAX_DIM) return CTG_EINVAL;
    if (thick < 1 || thick > SLB_MAX_DIM || step < 1 || step > thick) return CTG_EINVAL;
    if (n0 < 0 || n0 > N - K || mode < SLB_MAX || mode > SLB_SUM || (axis != SLB_CORONAL && axis != SLB_SAGITTAL)) return CTG_EINVAL;
    if (((uintptr_t)pix & 1) != 0 || ((uintptr_t)values & 1) != 0) return CTG_EINVAL;
    const int L = axis == SLB_CORONAL ? H : W;
    const int T = thick < L ? thick : L, J = slab_count(L, T, step);
    const long blocks = axis == SLB_CORONAL
        ? ((long)K * J * ((W + SLB_SEG - 1) / SLB_SEG) + SLB_WAVES - 1) / SLB_WAVES
        : (long)K * ((H + SLB_ROWS - 1) / SLB_ROWS) * ((J + SLB_GROUP - 1) / SLB_GROUP);
    if (blocks > 0x7fffffffL) return CTG_EINVAL;      // the grid's x dimension
    hipStream_t st = (hipStream_t)stream;
    if (mode == SLB_MAX) inplane_launch<SLB_MAX>(pix, K, H, W, n0, N, axis, J, T, step, wc, ww, hu, values, level, blocks, st);
    else if (mode == SLB_MIN) inplane_launch<SLB_MIN>(pix, K, H, W, n0, N, axis, J, T, step, wc, ww, hu, values, level, blocks, st);
    else inplane_launch<SLB_SUM>(pix, K, H, W, n0, N, axis, J, T, step, wc, ww, hu, values, level, blocks, st);
    return ctg_launch_status();
}

// ------------------------------------------------------------------------------------------------------ axial: sliding slabs
// dst[0 .. cnt-1] = op(dst, acc): the pixels belong to this lane alone
template <int MODE> __device__ __forceinline__ void slb_combine8(int* __restrict__ dst, const int (&acc)[8], int cnt) {
    if (cnt == 8 && ((uintptr_t)dst & 15) == 0) {
        s32x4 a = *reinterpret_cast<const s32x4*>(dst), b = *reinterpret_cast<const s32x4*>(dst + 4);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            a[q] = slb_op<MODE>(a[q], acc[q]);
            b[q] = slb_op<MODE>(b[q], acc[4 + q]);
        }
        *reinterpret_cast<s32x4*>(dst) = a;
        *reinterpret_cast<s32x4*>(dst + 4) = b;
        return;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q)
        if (q < cnt) dst[q] = slb_op<MODE>(dst[q], acc[q]);
}

// one wave per (slab j = jlo .. jlo+nj-1, row y, segment); items = nj * H * nseg.  Every slab of the range meets the chunk.
template <int MODE>
__global__ __launch_bounds__(SLB_THREADS) void slabs_axial_kernel(const short* __restrict__ pix, int K, int H, int W, int nseg, int n0,
                                                                  int T, int S, int jlo, int nj, int* __restrict__ axial) {
    const int lane = threadIdx.x & 63;
    const long item = (long)blockIdx.x * SLB_WAVES + (threadIdx.x >> 6);
    if (item >= (long)nj * H * nseg) return;      // (no barrier in this kernel)
    const int seg = (int)(item % nseg);
    const long t = item / nseg;
    const int y = (int)(t % H), j = jlo + (int)(t / H);
    const int x0 = seg * SLB_SEG + lane * 8;
    const int cnt = W - x0 >= 8 ? 8 : (W - x0 > 0 ? W - x0 : 0);
    if (cnt == 0) return;
    const int ka = (j * S > n0 ? j * S : n0) - n0, kb = (j * S + T < n0 + K ? j * S + T : n0 + K) - n0;
    if (ka >= kb) return;
    const size_t HW = (size_t)H * W;
    const short* __restrict__ row = pix + (size_t)y * W + x0;
    int acc[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = slb_identity<MODE>();
    for (int k = ka; k < kb; k += SLB_INFLIGHT) {
        s16x8 raw[SLB_INFLIGHT];
#pragma unroll
        for (int u = 0; u < SLB_INFLIGHT; ++u) raw[u] = slb_load8<MODE>(row + (size_t)(k + u) * HW, k + u < kb ? cnt : 0);
#pragma unroll
        for (int u = 0; u < SLB_INFLIGHT; ++u)
#pragma unroll
            for (int q = 0; q < 8; ++q) acc[q] = slb_op<MODE>(acc[q], raw[u][q]);
    }
    slb_combine8<MODE>(axial + ((size_t)j * H + y) * W + x0, acc, cnt);
}

extern "C" int ctg_project_accumulate_sliding(const short* pix, int K, int H, int W, int n0, int N, int thick, int step, int mode,
                                              int* axial, void* stream) {
    CTG_ENTER();
    if (pix == nullptr || axial == nullptr) return CTG_EINVAL;
    // 65535 x 32767 < 2^31: a sum over fewer than 65536 int16 values stays inside int32
    if (K < 1 || K > SLB_MAX_DIM || H < 1 || H > SLB_MAX_DIM || W < 1 || W > SLB_MAX_DIM || N < 1 || N > SLB_MAX_DIM) return CTG_EINVAL;
    if (thick < 1 || thick > SLB_MAX_DIM || step < 1 || step > thick) return CTG_EINVAL;
    if (n0 < 0 || n0 > N - K || mode < SLB_MAX || mode > SLB_SUM) return CTG_EINVAL;
    if (((uintptr_t)pix & 1) != 0 || ((uintptr_t)axial & 3) != 0) return CTG_EINVAL;
    const int T = thick < N ? thick : N, J = slab_count(N, T, step);
    // the slabs that meet slices n0 .. n0+K-1: j S + T > n0 and j S <= n0 + K - 1, j < J (the slabs cover [0, N): never empty)
    const int jlo = n0 < T ? 0 : (n0 - T) / step + 1;
    int jhi = (n0 + K - 1) / step;
    jhi = jhi < J - 1 ? jhi : J - 1;
    if (jhi < jlo) return CTG_EINVAL;
    const int nj = jhi - jlo + 1, nseg = (W + SLB_SEG - 1) / SLB_SEG;
    const long blocks = ((long)nj * H * nseg + SLB_WAVES - 1) / SLB_WAVES;
    if (blocks > 0x7fffffffL) return CTG_EINVAL;      // the grid's x dimension
    hipStream_t st = (hipStream_t)stream;
#define SLB_AXIAL(M) hipLaunchKernelGGL(slabs_axial_kernel<M>, dim3((unsigned)blocks), dim3(SLB_THREADS), 0, st, pix, K, H, W, nseg, \
                                        n0, T, step, jlo, nj, axial)
    if (mode == SLB_MAX) SLB_AXIAL(SLB_MAX);
    else if (mode == SLB_MIN) SLB_AXIAL(SLB_MIN);
    else SLB_AXIAL(SLB_SUM);
#undef SLB_AXIAL
    return ctg_launch_status();
}
