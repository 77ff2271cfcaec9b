// Series inference, the subtraction volume: synthesized CTA minus the CT it was made from (cta_gan_amd/infer.py:
// SeriesTranslator(subtract=True), subtract_volume).  The generator writes its output on the input's pixel grid, so the pair is
// registered by construction and the difference of the stored values is the contrast-enhancement map: bone cancels without a
// segmentation.  The reference has no counterpart.
//
// Per pixel, int32 throughout (tests/subtract_np.py is the numpy restatement, equal bit for bit):
//   a = max(ct_hu + 1024, 0)                 the stored value the generator was fed (input_arith.h: hu_fullrange before its scaling)
//   b = cta + (cta_is_hu ? 1024 : 0)         the stored value of the synthesized pixel (both conventions of ctg_export_slices)
//   d = b - a;  median != 0: d = the median of the 3 x 3 in-plane neighbourhood of d, the edge pixel replicated outside the plane
//   d = 0 where ct_hu < ct_min, ct_hu > ct_max or d < floor (the centre pixel, after the median; equality keeps the pixel)
//   sub = clamp(d, -32768, 32767);  level = stored_level((float)(sub + 1024), win_params(wc, ww)): ctg_project_finish's, hu = 1
//
// Work split: a wave owns (slice, band of SUB_BAND rows, segment of 512 pixels) and slides down its band; a lane owns 8 consecutive
// pixels x0 .. x0+7 (x0 a multiple of 8).  A row whose address is 16-byte aligned is read with one 16-byte load per lane and input;
// any other row (W % 8 != 0, planes of odd H W, a base pointer that is only 2-byte aligned) by the same lanes with 2-byte loads, as
// project.hip does -- the lane -> pixel map never depends on the address, so the three rows of d the median needs stay in registers
// while the band slides: every input row is fetched once per band, plus the two halo rows.  SUB_AHEAD rows of loads are issued
// before the arithmetic of the current rows waits on anything.  The left / right neighbour of a lane's outer pixels comes from the
// neighbouring lane by shuffle; only lanes 0 and 63 of a wave fetch one extra pixel per row and input.  Replicated edges are index
// clamps, so every load index lies inside the plane.  Median of 9: each column of three is sorted once (three compare-exchanges,
// shared by the three outputs that use the column), the result is med3(max of the lows, med3 of the mids, min of the highs).
// median == 0 is a compile-time variant without halo rows, halo pixels or shuffles.  No LDS, no atomics, no scratch, no barrier:
// waves are independent.
#include "common.h"
#include "window_arith.h"

#define SUB_THREADS 256
#define SUB_WAVES (SUB_THREADS / 64)
#define SUB_SEG 512        // pixels of a row one wave covers: 64 lanes x 8
#ifndef SUB_BAND          // rows a wave produces.  The halo rows cost 2 / SUB_BAND extra requests (served by L2), but the kernel is
#define SUB_BAND 4        // bound by how many waves are in flight, not by those: on a 16 x 512 x 512 chunk 4 rows (2048 waves)
#endif                    // measured 13.1 us, 8 rows (1024 waves) 15.2 us, 16 rows (512 waves) 23.4 us (LAB_NOTES section 17)
#define SUB_AHEAD 2        // rows whose loads are in flight ahead of the arithmetic (the row loop is unrolled by this)
#define SUB_MAX_BLOCKS (1 << 20)

typedef short i16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// what a lane fetches of one row: its 8 pixels of both inputs and, on lanes 0 / 63 of a median wave, the pixel beside them
struct SubRaw {
    i16x8 cta, ct;
    short cta_l, ct_l, cta_r, ct_r;
};

// pixels min(x0 + j, W - 1), j = 0 .. 7, of a row: `row` points at the row's pixel 0; cnt = pixels of the lane inside the row
__device__ __forceinline__ i16x8 sub_load8(const short* __restrict__ row, int x0, int W, int cnt) {
    const short* __restrict__ p = row + x0;
    if (cnt == 8 && ((uintptr_t)p & 15) == 0) return *reinterpret_cast<const i16x8*>(p);
    i16x8 v;
    if (cnt <= 0) {      // a lane behind the row's end: the replicated last pixel, one load
        const short e = row[W - 1];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = e;
        return v;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = p[j < cnt ? j : cnt - 1];
    return v;
}

template <bool MED>
__device__ __forceinline__ SubRaw sub_fetch(const short* __restrict__ cta, const short* __restrict__ ct, int y, int x0, int W,
                                            int cnt, int lane, bool live) {
    SubRaw r;
    r.cta = r.ct = i16x8{0, 0, 0, 0, 0, 0, 0, 0};
    r.cta_l = r.ct_l = r.cta_r = r.ct_r = 0;
    if (!live) return r;      // (the same for the whole wave)
    const long off = (long)y * W;
    r.cta = sub_load8(cta + off, x0, W, cnt);
    r.ct = sub_load8(ct + off, x0, W, cnt);
    if constexpr (MED) {
        if (lane == 0) {
            const int xl = x0 > 0 ? x0 - 1 : 0;
            r.cta_l = cta[off + xl];
            r.ct_l = ct[off + xl];
        }
        if (lane == 63) {
            const int xr = x0 + 8 < W ? x0 + 8 : W - 1;
            r.cta_r = cta[off + xr];
            r.ct_r = ct[off + xr];
        }
    }
    return r;
}

__device__ __forceinline__ int sub_diff(int cta, int ct, int add) {
    const int a = ct + 1024;
    return cta + add - (a > 0 ? a : 0);
}

__device__ __forceinline__ int sub_med3(int a, int b, int c) {
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    const int m = hi < c ? hi : c;
    return lo > m ? lo : m;
}

// a row of d as the median sees it: column 0 = the pixel left of the lane's, 1 .. 8 the lane's own, 9 the pixel right of them
struct SubRow { int d[10]; };

template <bool MED> __device__ __forceinline__ SubRow sub_row(const SubRaw& r, int add, int lane) {
    SubRow o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o.d[1 + j] = sub_diff(r.cta[j], r.ct[j], add);
    o.d[0] = o.d[9] = 0;
    if constexpr (MED) {
        const int left = __shfl_up(o.d[8], 1, 64), right = __shfl_down(o.d[1], 1, 64);
        o.d[0] = lane == 0 ? sub_diff(r.cta_l, r.ct_l, add) : left;
        o.d[9] = lane == 63 ? sub_diff(r.cta_r, r.ct_r, add) : right;
    }
    return o;
}

struct SubArgs { int add, floor, ct_min, ct_max; };

// the row's 8 outputs of a lane; ct = the centre row's ct_hu.  sub / level point at the lane's first pixel (or are null)
__device__ __forceinline__ void sub_emit(const int (&d)[8], const i16x8 ct, const SubArgs& q, const WinParams win,
                                         short* __restrict__ sub, unsigned char* __restrict__ level, int cnt) {
    int v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = ct[j];
        int t = (c < q.ct_min || c > q.ct_max || d[j] < q.floor) ? 0 : d[j];
        t = t > 32767 ? 32767 : t;
        v[j] = t < -32768 ? -32768 : t;
    }
    if (sub != nullptr) {
        if (cnt == 8 && ((uintptr_t)sub & 15) == 0) {
            i16x8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = (short)v[j];
            *reinterpret_cast<i16x8*>(sub) = o;
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < cnt) sub[j] = (short)v[j];
        }
    }
    if (level != nullptr) {
        unsigned l[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) l[j] = (unsigned)(int)stored_level((float)(v[j] + 1024), win);
        if (cnt == 8 && ((uintptr_t)level & 7) == 0) {
            *reinterpret_cast<u32x2*>(level) = u32x2{l[0] | (l[1] << 8) | (l[2] << 16) | (l[3] << 24),
                                                     l[4] | (l[5] << 8) | (l[6] << 16) | (l[7] << 24)};
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < cnt) level[j] = (unsigned char)l[j];
        }
    }
}

// the 8 medians of a lane from the three rows around the centre row
__device__ __forceinline__ void sub_median(const SubRow& p, const SubRow& c, const SubRow& n, int (&out)[8]) {
    int lo[10], mid[10], hi[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) {      // sort the column (p, c, n)
        const int a = p.d[k] < c.d[k] ? p.d[k] : c.d[k], b = p.d[k] < c.d[k] ? c.d[k] : p.d[k];
        const int m = b < n.d[k] ? b : n.d[k];
        hi[k] = b < n.d[k] ? n.d[k] : b;
        lo[k] = a < m ? a : m;
        mid[k] = a < m ? m : a;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        int l = lo[j] > lo[j + 1] ? lo[j] : lo[j + 1];
        l = l > lo[j + 2] ? l : lo[j + 2];
        int h = hi[j] < hi[j + 1] ? hi[j] : hi[j + 1];
        h = h < hi[j + 2] ? h : hi[j + 2];
        out[j] = sub_med3(l, sub_med3(mid[j], mid[j + 1], mid[j + 2]), h);
    }
}

// one wave per item (slice, band, segment), grid-strided; items = B * nband * nseg
template <bool MED>
__global__ __launch_bounds__(SUB_THREADS) void subtract_kernel(const short* __restrict__ cta, const short* __restrict__ ct_hu, long items,
                                                               int H, int W, int nseg, int nband, SubArgs q, float wc, float ww,
                                                               short* __restrict__ sub, unsigned char* __restrict__ level) {
    WinParams win = {0.f, 0.f};
    if (level != nullptr) win = win_params(wc, ww);
    const int lane = threadIdx.x & 63;
    const long HW = (long)H * W;
    for (long item = (long)blockIdx.x * SUB_WAVES + (threadIdx.x >> 6); item < items; item += (long)gridDim.x * SUB_WAVES) {
        const int seg = (int)(item % nseg);
        const long t = item / nseg;
        const int band = (int)(t % nband);
        const long b = t / nband;
        const int x0 = seg * SUB_SEG + lane * 8;
        const int cnt = W - x0 >= 8 ? 8 : (W - x0 > 0 ? W - x0 : 0);
        const int y0 = band * SUB_BAND, y1 = y0 + SUB_BAND < H ? y0 + SUB_BAND : H;
        const short* __restrict__ pa = cta + b * HW;
        const short* __restrict__ pc = ct_hu + b * HW;
        short* __restrict__ ps = sub != nullptr ? sub + b * HW + x0 : nullptr;
        unsigned char* __restrict__ pl = level != nullptr ? level + b * HW + x0 : nullptr;
        // step s handles source row clamp(ys + s, 0, H - 1); with the median the first two steps only fill the window and step
        // s >= 2 writes output row y0 + s - 2 (its centre row arrived at step s - 1)
        const int ys = MED ? y0 - 1 : y0, steps = y1 - y0 + (MED ? 2 : 0);
        auto fetch = [&](int s) {
            int y = ys + s;
            y = y < 0 ? 0 : (y > H - 1 ? H - 1 : y);
            return sub_fetch<MED>(pa, pc, y, x0, W, cnt, lane, s < steps);
        };
        SubRaw raw[SUB_AHEAD];
#pragma unroll
        for (int u = 0; u < SUB_AHEAD; ++u) raw[u] = fetch(u);
        SubRow prev, cur, next;
        i16x8 ct_cur = raw[0].ct, ct_next = raw[0].ct;
        prev = cur = next = sub_row<MED>(raw[0], q.add, lane);
        for (int s0 = 0; s0 < steps; s0 += SUB_AHEAD) {
            SubRaw ahead[SUB_AHEAD];
#pragma unroll
            for (int u = 0; u < SUB_AHEAD; ++u) ahead[u] = fetch(s0 + SUB_AHEAD + u);
#pragma unroll
            for (int u = 0; u < SUB_AHEAD; ++u) {
                const int s = s0 + u;
                if (s < steps) {      // (the same for the whole wave: the shuffles inside see all 64 lanes)
                    prev = cur;
                    cur = next;
                    ct_cur = ct_next;
                    next = sub_row<MED>(raw[u], q.add, lane);
                    ct_next = raw[u].ct;
                    int d[8];
                    if constexpr (MED) {
                        if (s >= 2) {
                            sub_median(prev, cur, next, d);
                            const long o = (long)(y0 + s - 2) * W;
                            if (cnt > 0) sub_emit(d, ct_cur, q, win, ps != nullptr ? ps + o : nullptr, pl != nullptr ? pl + o : nullptr, cnt);
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < 8; ++j) d[j] = next.d[1 + j];
                        const long o = (long)(y0 + s) * W;
                        if (cnt > 0) sub_emit(d, ct_next, q, win, ps != nullptr ? ps + o : nullptr, pl != nullptr ? pl + o : nullptr, cnt);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < SUB_AHEAD; ++u) raw[u] = ahead[u];
        }
    }
}

extern "C" int ctg_subtract_slices(const short* cta, const short* ct_hu, int B, int H, int W, int cta_is_hu, int median, int floor,
                                   int ct_min, int ct_max, float wc, float ww, short* sub, unsigned char* level, void* stream) {
    CTG_ENTER();
    if (cta == nullptr || ct_hu == nullptr || (sub == nullptr && level == nullptr)) return CTG_EINVAL;
    if (B < 1 || B > 65535 || H < 1 || H > 65535 || W < 1 || W > 65535 || ct_min > ct_max) return CTG_EINVAL;
    if ((((uintptr_t)cta | (uintptr_t)ct_hu | (uintptr_t)sub) & 1) != 0) return CTG_EINVAL;
    const int nseg = (W + SUB_SEG - 1) / SUB_SEG, nband = (H + SUB_BAND - 1) / SUB_BAND;
    const long items = (long)B * nband * nseg;
    long blocks = (items + SUB_WAVES - 1) / SUB_WAVES;
    blocks = blocks < SUB_MAX_BLOCKS ? blocks : SUB_MAX_BLOCKS;
    const SubArgs q = {cta_is_hu ? 1024 : 0, floor, ct_min, ct_max};
    hipStream_t st = (hipStream_t)stream;
    if (median)
        hipLaunchKernelGGL(subtract_kernel<true>, dim3((unsigned)blocks), dim3(SUB_THREADS), 0, st, cta, ct_hu, items, H, W, nseg, nband,
                           q, wc, ww, sub, level);
    else
        hipLaunchKernelGGL(subtract_kernel<false>, dim3((unsigned)blocks), dim3(SUB_THREADS), 0, st, cta, ct_hu, items, H, W, nseg,
                           nband, q, wc, ww, sub, level);
    return ctg_launch_status();
}
