// Series inference, the volume-rendered rotating view: front-to-back compositing of the exported int16 volume at any angle about
// the cranio-caudal axis (cta_gan_amd/infer.py: SeriesRenderer).  The third display of a CTA beside the thin slabs (project_slabs.hip)
// and the rotating MIP (project_rotate.hip); like them the reference has no counterpart (its test() writes slices only).
//
// Geometry, sampling and the "counted" rule are those of project_rotate.hip, unchanged: the same coefficient table, detector,
// interval [lo, hi] per ray, nearest or bilinear value (rot_lerp of the four clamped pixels), and an uncounted sample reads pixel 0
// and takes no part.  A row of a rendered view depends on one slice only, so a chunk of K slices finishes rows n0 .. n0+K-1 of every
// angle in one launch.
//
// Arithmetic (the definition; include/ctagan_hip.h has it in full).  A counted sample of value v has the class
//     l = stored_level((float)(v + add), win_params(wc, ww)),  0 .. 255        (the transfer function's own window)
// and the transfer table gives its colour (R, G, B, each min(., 255)) and alpha A = min(., 32768), 32768 = opaque.  A ray starts
// from Tr = 32768, C = 0 and takes its counted samples in ascending step t:
//     wgt = (Tr A) >> 15;   C[c] += wgt col[c];   Tr -= wgt;   depth := t the first time 32768 - Tr >= surface;   Tr <= stop ends the ray
// all in uint32: wgt <= Tr, the weights telescope to 32768 - Tr, so C[c] <= 32768 * 255 < 2^23 and every output fits 8 bits.
//
// The fold.  "over" is ordered and, with the floor, not associative: the xor-shuffle fold of the MIP kernels does not carry over.
// But the ordered part is the Tr chain alone -- it needs the alphas, not the colours -- and once a sample's wgt is known its
// contribution wgt col is a plain term of an exact sum.  So the layout of project_rotate_kernel stays (one 256-thread workgroup
// per (slice, 32 detector columns, angle); a wave owns 8 rays and walks each with 8 lanes, lane (ul, tl) gathering the steps
// t = tl (mod 8), REN_INFLIGHT gathers in flight: the 8 x 8 patch that keeps the gathers coalesced at 90 degrees), every lane
// classifies its own samples (one 8-byte LDS read of the staged table each), and per trip of 32 steps the 8 lanes of a ray read
// one another's alphas in step order -- two alphas to a word, 16 cross-lane reads for 32 steps -- and ALL run the chain, so Tr,
// depth and "ended" are uniform over the ray's lanes without a broadcast.  Lane tl keeps the wgt of its own samples and adds
// wgt col into its own partial C; the partials (exact, below 2^23) meet at the end in the three xor-shuffles.  An uncounted step
// enters the chain with alpha 0: wgt = 0 leaves C, Tr, depth and "ended" as they are (32768 - Tr >= surface and Tr <= stop can
// only become true at a step that lowers Tr), which is "skipped".  A ray that has ended pulls its hi in, so its lanes gather
// pixel 0 from then on, and the wave leaves the loop when none of its rays has steps left.  The loop condition is wave-uniform:
// every lane is active at every cross-lane read.
//
// Addresses: as in project_rotate.hip a sample is read only after its own index passed the bounds check (bilinear: clamped), and
// one that fails it reads pixel 0: inside the slice whatever the table holds.  A class is `& 255` of an int: inside the staged
// table whatever the window holds.
#include "common.h"
#include "rotate_sample.h"
#include "window_arith.h"

#define REN_THREADS 256
#define REN_UL 8            // rays of a wave
#define REN_TL 8            // lanes of a ray: lane tl takes the steps t = tl (mod REN_TL)
#define REN_WG_U (REN_THREADS / 64 * REN_UL)
#define REN_INFLIGHT 4      // gathers a lane issues before it uses the first (even: two alphas travel in one word)
#define REN_TRIP (REN_TL * REN_INFLIGHT)
#define REN_MAX_DIM 4096    // H, W, U, T, A: each term of the fixed-point sum stays below 2^28; T <= 4096 is an int16 depth
#define REN_ONE 32768u      // full transparency of a ray / an opaque alpha

static_assert(REN_THREADS == 256, "one thread stages one class of the transfer table");
static_assert(REN_INFLIGHT % 2 == 0, "alphas cross the lanes in pairs");

template <bool LERP>
__global__ __launch_bounds__(REN_THREADS) void project_render_kernel(const short* __restrict__ pix, int H, int W, int n0, int N,
                                                                     const int* __restrict__ coef, int A, int U, int T, int nseg,
                                                                     const unsigned short* __restrict__ lut, unsigned stop,
                                                                     unsigned surface, unsigned bg_r, unsigned bg_g, unsigned bg_b,
                                                                     float wc, float ww, int add, unsigned char* __restrict__ rgb,
                                                                     unsigned char* __restrict__ opacity, short* __restrict__ depth) {
    __shared__ uint2 tab[256];      // class -> (R | G << 8 | B << 16, alpha), clamped once
    {
        const unsigned short* __restrict__ e = lut + threadIdx.x * 4;      // (only 2-byte alignment is promised)
        const unsigned r = e[0], g = e[1], b = e[2], al = e[3];
        tab[threadIdx.x] = make_uint2((r < 255u ? r : 255u) | (g < 255u ? g : 255u) << 8 | (b < 255u ? b : 255u) << 16,
                                      al < REN_ONE ? al : REN_ONE);
    }
    __syncthreads();
    const unsigned a = blockIdx.x % (unsigned)A, rest = blockIdx.x / (unsigned)A;
    const unsigned seg = rest % (unsigned)nseg, k = rest / (unsigned)nseg;
    const int lane = threadIdx.x & 63, tl = lane / REN_UL, ul = lane % REN_UL;
    const int u = (int)(seg * REN_WG_U + (threadIdx.x >> 6) * REN_UL + ul);
    const bool live = u < U;      // (every lane stays for the cross-lane reads; the 8 lanes of a ray are live together)
    const int* __restrict__ c = coef + (size_t)a * 6;
    const unsigned c2 = (unsigned)c[2], c5 = (unsigned)c[5];
    const unsigned X0 = (unsigned)c[0] + (unsigned)c[1] * (unsigned)u, Y0 = (unsigned)c[3] + (unsigned)c[4] * (unsigned)u;
    int lo = 0, hi = live ? T - 1 : -1;
    rot_clip((int)X0, (int)c2, (W << 16) - 1, lo, hi);
    rot_clip((int)Y0, (int)c5, (H << 16) - 1, lo, hi);
    const short* __restrict__ slice = pix + (size_t)k * H * W;
    const WinParams wp = win_params(wc, ww);
    unsigned Tr = REN_ONE, C0 = 0, C1 = 0, C2 = 0;      // Tr, d and ended: the same in the 8 lanes of a ray; C: this lane's share
    int d = -1;
    bool ended = false;
    int base = lo & ~(REN_TL - 1);      // lo >= 0; the first step of the ray's current trip, the lane's own is base + tl
    unsigned X = X0 + c2 * (unsigned)(base + tl), Y = Y0 + c5 * (unsigned)(base + tl);
    const unsigned dX = c2 * REN_TL, dY = c5 * REN_TL;
    while (__any(base <= hi)) {      // wave-uniform: all 64 lanes take every trip
        const int t = base + tl;
        bool ok[REN_INFLIGHT];
        int val[REN_INFLIGHT];
        if constexpr (LERP) {
            int p[REN_INFLIGHT][4], fx[REN_INFLIGHT], fy[REN_INFLIGHT];      // 4 REN_INFLIGHT gathers before the first is used
#pragma unroll
            for (int j = 0; j < REN_INFLIGHT; ++j) {
                const int xi = (int)X >> 16, yi = (int)Y >> 16;
                ok[j] = t + j * REN_TL <= hi && xi >= 0 && xi < W && yi >= 0 && yi < H;
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
            for (int j = 0; j < REN_INFLIGHT; ++j) val[j] = rot_lerp(p[j][0], p[j][1], p[j][2], p[j][3], fx[j], fy[j]);
        } else {
#pragma unroll
            for (int j = 0; j < REN_INFLIGHT; ++j) {
                const int xi = (int)X >> 16, yi = (int)Y >> 16;
                ok[j] = t + j * REN_TL <= hi && xi >= 0 && xi < W && yi >= 0 && yi < H;
                val[j] = slice[ok[j] ? yi * W + xi : 0];
                X += dX;
                Y += dY;
            }
        }
        unsigned col[REN_INFLIGHT], alpha[REN_INFLIGHT];      // each lane classifies its own samples
#pragma unroll
        for (int j = 0; j < REN_INFLIGHT; ++j) {
            const int l = (int)stored_level((float)(val[j] + add), wp) & 255;
            const uint2 e = tab[l];
            col[j] = e.x;
            alpha[j] = ok[j] ? e.y : 0u;      // an uncounted step: alpha 0 changes nothing in the chain
        }
#pragma unroll
        for (int pr = 0; pr < REN_INFLIGHT / 2; ++pr) {
            const int packed = (int)(alpha[2 * pr] | alpha[2 * pr + 1] << 16);      // alpha <= 32768 = 0x8000
            unsigned q[REN_TL];
#pragma unroll
            for (int s = 0; s < REN_TL; ++s) q[s] = (unsigned)__shfl(packed, s * REN_UL + ul, 64);      // lane (ul, s): step s of the slot
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const int j = 2 * pr + half;
                unsigned mine = 0;
#pragma unroll
                for (int s = 0; s < REN_TL; ++s) {      // the steps base + 8 j + s, in order
                    const unsigned al = half ? q[s] >> 16 : q[s] & 0xffffu;
                    const unsigned wgt = ended ? 0u : (Tr * al) >> 15;      // Tr, al <= 2^15
                    mine = s == tl ? wgt : mine;
                    Tr -= wgt;
                    d = (d < 0 && REN_ONE - Tr >= surface) ? base + j * REN_TL + s : d;
                    ended = ended || Tr <= stop;
                }
                C0 += mine * (col[j] & 255u);
                C1 += mine * ((col[j] >> 8) & 255u);
                C2 += mine * (col[j] >> 16);
            }
        }
        if (ended) hi = -1;      // no step left: the lanes of this ray gather pixel 0 until the wave is through
        base += REN_TRIP;
    }
#pragma unroll
    for (int o = REN_UL; o < 64; o <<= 1) {      // the 8 lanes of a ray: lane, lane ^ 8, ^ 16, ^ 32; exact sums below 2^23
        C0 += (unsigned)__shfl_xor((int)C0, o, 64);
        C1 += (unsigned)__shfl_xor((int)C1, o, 64);
        C2 += (unsigned)__shfl_xor((int)C2, o, 64);
    }
    if (!live || tl != 0) return;
    const size_t o = ((size_t)a * N + (size_t)n0 + k) * U + u;
    if (rgb != nullptr) {      // C + bg Tr <= 255 * 32768
        rgb[o * 3 + 0] = (unsigned char)((C0 + bg_r * Tr + 16384u) >> 15);
        rgb[o * 3 + 1] = (unsigned char)((C1 + bg_g * Tr + 16384u) >> 15);
        rgb[o * 3 + 2] = (unsigned char)((C2 + bg_b * Tr + 16384u) >> 15);
    }
    if (opacity != nullptr) opacity[o] = (unsigned char)(((REN_ONE - Tr) * 255u + 16384u) >> 15);
    if (depth != nullptr) depth[o] = (short)d;
}

extern "C" int ctg_project_render(const short* pix, int K, int H, int W, int n0, int N, const int* coef, int A, int U, int T,
                                  const unsigned short* lut, int sampling, int stop, int surface, int bg_r, int bg_g, int bg_b,
                                  float wc, float ww, int hu, unsigned char* rgb, unsigned char* opacity, short* depth,
                                  void* stream) {
    CTG_ENTER();
    if (pix == nullptr || coef == nullptr || lut == nullptr) return CTG_EINVAL;
    if (rgb == nullptr && opacity == nullptr && depth == nullptr) return CTG_EINVAL;
    if (K < 1 || n0 < 0 || N < 1 || n0 > N - K) return CTG_EINVAL;
    if (H < 1 || H > REN_MAX_DIM || W < 1 || W > REN_MAX_DIM || U < 1 || U > REN_MAX_DIM || T < 1 || T > REN_MAX_DIM) return CTG_EINVAL;
    if (A < 1 || A > REN_MAX_DIM || sampling < 0 || sampling > 1) return CTG_EINVAL;
    if (stop < 0 || stop > 32767 || surface < 1 || surface > 32768) return CTG_EINVAL;
    if (bg_r < 0 || bg_r > 255 || bg_g < 0 || bg_g > 255 || bg_b < 0 || bg_b > 255) return CTG_EINVAL;
    if (((uintptr_t)pix & 1) != 0 || ((uintptr_t)coef & 3) != 0 || ((uintptr_t)lut & 1) != 0 || ((uintptr_t)depth & 1) != 0)
        return CTG_EINVAL;
    // one workgroup per (slice, segment, angle): the grid's x dimension
    const int nseg = (U + REN_WG_U - 1) / REN_WG_U;
    if ((long)K * nseg * A > 0x7fffffffL) return CTG_EINVAL;
    const dim3 grid((unsigned)((long)K * nseg * A)), block(REN_THREADS);
    hipStream_t st = (hipStream_t)stream;
#define REN_GO(L) hipLaunchKernelGGL((project_render_kernel<L>), grid, block, 0, st, pix, H, W, n0, N, coef, A, U, T, nseg, lut, \
                                     (unsigned)stop, (unsigned)surface, (unsigned)bg_r, (unsigned)bg_g, (unsigned)bg_b, wc, ww,  \
                                     hu ? 1024 : 0, rgb, opacity, depth)
    if (sampling) REN_GO(true);
    else REN_GO(false);
#undef REN_GO
    return ctg_launch_status();
}
