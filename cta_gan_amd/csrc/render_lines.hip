// Series inference, shaded volume rendering along lines in any direction: front-to-back compositing of the resident int16 volume
// along the rays of a line table, every sample's colour shaded by the local gradient (cta_gan_amd/infer.py: VolumeRenderer,
// headlight).  The rays of project_render.hip cannot leave their slice and its colours are flat; this kernel takes the table,
// the "counted" rule and the sampling of reformat.hip (reformat_sample.h: the same bits) and the classification and the chain of
// project_render.hip, and adds the shading.  Like them the reference has no counterpart (its test() writes slices only).
//
// The definition (include/ctagan_hip.h has it in full).  Sample (l, i, k) lies at X = x0 + xu i + xk k (Y, Z likewise), is
// counted exactly when voxel (xi, yi, zi) = (X >> 16, Y >> 16, Z >> 16) lies in the volume, has the nearest or trilinear value v
// of reformat.hip and the class stored_level(v + add) & 255; the staged table gives col = min(R, G, B, 255) and A = min(alpha,
// 32768), and the ray runs project_render.hip's chain over its counted samples in ascending k:
//     wgt = (Tr A) >> 15;   C[c] += wgt cols[c];   Tr -= wgt;   depth := k the first time 32768 - Tr >= surface;   Tr <= stop ends
// Without a light cols = col.  With one, the sample is shaded at its own voxel, whichever the sampling:
//     dx = p[zi][yi][min(xi+1, W-1)] - p[zi][yi][max(xi-1, 0)]  (dy, dz likewise: central differences, the edge replicated)
//     gx = clamp(dx, +-4095), gy likewise, gz = clamp((dz zscale + 128) >> 8, +-4095)       zscale = 256 / aspect in 8.8
//     m = gx^2 + gy^2 + gz^2 <= 3 * 4095^2 < 2^26;   l[c] = clamp(light[l][c], +-4096);   dot = |gx l[0] + gy l[1] + gz l[2]| < 2^26
//     shade = 256 where m < gmin2 (a flat region shows its class colour), else with n = floor(sqrt(m)) >= 1:
//         diff = min((dot / n) >> 4, 256);   shade = ambient + (((256 - ambient) diff + 128) >> 8)            <= 256
//     cols[c] = (col[c] shade + 128) >> 8 <= 255
// so C[c] <= 32768 * 255 still holds and no output needs a clamp.  The absolute value makes the lighting two-sided.  All of it is
// integer arithmetic; the float sqrt only seeds the integer square root, which is then corrected to the exact floor (m < 2^26 and
// a seed within 1 of the root: one step down, one step up).  Opacity and depth do not depend on the shading.
//
// When the gradient is loaded.  The colour of a sample is needed only where its weight is not 0, and that is known only after the
// chain; under a vessel preset most samples are transparent and most rays end early.  So a lane loads the six neighbours after
// the chain of a trip, for those of its own samples whose wgt != 0, all of a trip's loads issued before the first is used (a
// lane none of whose four samples has weight skips the block).  The positions are recomputed from the trip's first: no address
// is kept across the chain.  The other order -- the six loads issued with the sample, for every counted sample -- was built and
// measured (LAB_NOTES section 27): no faster where every sample carries weight, 1.3 - 1.6 x slower where few do.  It is not kept.
//
// Safety, as in both parents: a sample is read only after its own voxel index passed the bounds check (nearest) or through
// clamped indices (trilinear); the six gradient addresses are formed from a voxel index that passed the bounds check again and are
// clamped into the volume; a sample that is not counted (or has no weight) reads voxel 0, its six gradient loads included.  The
// fixed-point sums are unsigned, the class is `& 255`, the light is clamped in the kernel: every address and every product is
// defined whatever the tables hold.
//
// Layout: reformat_rays_kernel's geometry (one 256-thread workgroup per (line, segment of 32 columns); a wave on 8 rays x 8 lanes,
// lane (ul, tl) on the steps k = tl (mod 8); rot_clip three times; RLN_INFLIGHT samples in flight) with project_render_kernel's
// chain (the table clamped in 2 KB of LDS; the alphas cross the 8 lanes of a ray two to a word; all 8 lanes run the Tr chain;
// each lane adds wgt cols for its own samples; three xor-shuffles at the end; a wave-uniform loop condition).  T = 1 is a ray of
// one step through the same kernel.
#include "common.h"
#include "reformat_sample.h"
#include "rotate_sample.h"
#include "window_arith.h"

#define RLN_THREADS 256
#define RLN_UL 8            // rays of a wave
#define RLN_TL 8            // lanes of a ray: lane tl takes the steps k = tl (mod RLN_TL)
#define RLN_WG_U (RLN_THREADS / 64 * RLN_UL)
#define RLN_INFLIGHT 4      // samples a lane issues before it uses the first (even: two alphas travel in one word)
#define RLN_TRIP (RLN_TL * RLN_INFLIGHT)
#define RLN_MAX_DIM 4096    // N, H, W, U, T: (dim << 16) - 1 stays below 2^28; T <= 4096 is an int16 depth
#define RLN_ONE 32768u      // full transparency of a ray / an opaque alpha
#define RLN_GMAX 4095       // a gradient component: three squares stay below 2^26
#define RLN_LMAX 4096       // a light component: unit length

static_assert(RLN_THREADS == 256, "one thread stages one class of the transfer table");
static_assert(RLN_INFLIGHT % 2 == 0, "alphas cross the lanes in pairs");

__device__ __forceinline__ int rln_clamp(int v, int m) { return v < -m ? -m : (v > m ? m : v); }

// The six neighbours of one sample's voxel (issued, not used) and the shade they give.  ok = false reads voxel 0 six times.
struct RlnGrad {
    int p[6];

    __device__ __forceinline__ void issue(const RfmVol& v, unsigned X, unsigned Y, unsigned Z, bool ok) {
        ok = ok && rfm_inside(v, X, Y, Z);
        const int xi = ok ? (int)X >> 16 : 0, yi = ok ? (int)Y >> 16 : 0, zi = ok ? (int)Z >> 16 : 0;      // inside the volume
        const int xm = xi > 0 ? xi - 1 : 0, xp = ok && xi < v.W - 1 ? xi + 1 : xi;
        const int ym = yi > 0 ? yi - 1 : 0, yp = ok && yi < v.H - 1 ? yi + 1 : yi;
        const int zm = zi > 0 ? zi - 1 : 0, zp = ok && zi < v.N - 1 ? zi + 1 : zi;
        const size_t plane = (size_t)v.H * v.W;
        const short* __restrict__ s = v.p + (size_t)zi * plane;
        p[0] = s[yi * v.W + xm];
        p[1] = s[yi * v.W + xp];
        p[2] = s[ym * v.W + xi];
        p[3] = s[yp * v.W + xi];
        p[4] = v.p[(size_t)zm * plane + yi * v.W + xi];
        p[5] = v.p[(size_t)zp * plane + yi * v.W + xi];
    }

    // 0 .. 256
    __device__ __forceinline__ unsigned shade(int l0, int l1, int l2, int zscale, unsigned ambient, unsigned gmin2) const {
        const int gx = rln_clamp(p[1] - p[0], RLN_GMAX), gy = rln_clamp(p[3] - p[2], RLN_GMAX);
        const int gz = rln_clamp(((p[5] - p[4]) * zscale + 128) >> 8, RLN_GMAX);      // |dz zscale| <= 65535 * 4096 < 2^31
        const unsigned m = (unsigned)(gx * gx) + (unsigned)(gy * gy) + (unsigned)(gz * gz);
        if (m < gmin2) return 256u;
        unsigned n = (unsigned)sqrtf((float)m);      // a seed within 1 of the root; m >= gmin2 >= 1
        n -= n * n > m ? 1u : 0u;
        n += (n + 1u) * (n + 1u) <= m ? 1u : 0u;
        const int sd = gx * l0 + gy * l1 + gz * l2;      // three terms of at most 4095 * 4096 each
        const unsigned dot = (unsigned)(sd < 0 ? -sd : sd);
        const unsigned q = (dot / n) >> 4, diff = q < 256u ? q : 256u;
        return ambient + (((256u - ambient) * diff + 128u) >> 8);
    }
};

template <bool LERP, bool SHADE>
__global__ __launch_bounds__(RLN_THREADS) void render_lines_kernel(RfmVol vol, const int* __restrict__ lines, int U, int T, int nseg,
                                                                   const unsigned short* __restrict__ lut, unsigned stop,
                                                                   unsigned surface, unsigned bg_r, unsigned bg_g, unsigned bg_b,
                                                                   float wc, float ww, int add, const int* __restrict__ light,
                                                                   int zscale, unsigned ambient, unsigned gmin2,
                                                                   unsigned char* __restrict__ rgb, unsigned char* __restrict__ opacity,
                                                                   short* __restrict__ depth) {
    __shared__ uint2 tab[256];      // class -> (R | G << 8 | B << 16, alpha), clamped once
    {
        const unsigned short* __restrict__ e = lut + threadIdx.x * 4;      // (only 2-byte alignment is promised)
        const unsigned r = e[0], g = e[1], b = e[2], al = e[3];
        tab[threadIdx.x] = make_uint2((r < 255u ? r : 255u) | (g < 255u ? g : 255u) << 8 | (b < 255u ? b : 255u) << 16,
                                      al < RLN_ONE ? al : RLN_ONE);
    }
    __syncthreads();
    const unsigned l = blockIdx.x / (unsigned)nseg, seg = blockIdx.x % (unsigned)nseg;
    const int lane = threadIdx.x & 63, tl = lane / RLN_UL, ul = lane % RLN_UL;
    const int u = (int)(seg * RLN_WG_U + (threadIdx.x >> 6) * RLN_UL + ul);
    const bool live = u < U;      // (every lane stays for the cross-lane reads; the 8 lanes of a ray are live together)
    const int* __restrict__ c = lines + (size_t)l * 9;
    const unsigned cx = (unsigned)c[2], cy = (unsigned)c[5], cz = (unsigned)c[8];
    const unsigned X0 = (unsigned)c[0] + (unsigned)c[1] * (unsigned)u, Y0 = (unsigned)c[3] + (unsigned)c[4] * (unsigned)u;
    const unsigned Z0 = (unsigned)c[6] + (unsigned)c[7] * (unsigned)u;
    int l0 = 0, l1 = 0, l2 = 0;      // the line's light, workgroup-uniform
    if constexpr (SHADE) {
        const int* __restrict__ lv = light + (size_t)l * 3;
        l0 = rln_clamp(lv[0], RLN_LMAX);
        l1 = rln_clamp(lv[1], RLN_LMAX);
        l2 = rln_clamp(lv[2], RLN_LMAX);
    }
    int lo = 0, hi = live ? T - 1 : -1;
    rot_clip((int)X0, (int)cx, (vol.W << 16) - 1, lo, hi);
    rot_clip((int)Y0, (int)cy, (vol.H << 16) - 1, lo, hi);
    rot_clip((int)Z0, (int)cz, (vol.N << 16) - 1, lo, hi);
    const WinParams wp = win_params(wc, ww);
    unsigned Tr = RLN_ONE, C0 = 0, C1 = 0, C2 = 0;      // Tr, d and ended: the same in the 8 lanes of a ray; C: this lane's share
    int d = -1;
    bool ended = false;
    int base = lo & ~(RLN_TL - 1);      // lo >= 0; the first step of the ray's current trip, the lane's own is base + tl
    unsigned X = X0 + cx * (unsigned)(base + tl), Y = Y0 + cy * (unsigned)(base + tl), Z = Z0 + cz * (unsigned)(base + tl);
    const unsigned dX = cx * RLN_TL, dY = cy * RLN_TL, dZ = cz * RLN_TL;
    while (__any(base <= hi)) {      // wave-uniform: all 64 lanes take every trip
        const int t = base + tl;
        const unsigned Xt = X, Yt = Y, Zt = Z;      // the lane's first sample of this trip
        bool ok[RLN_INFLIGHT];
        RfmSample<LERP> s[RLN_INFLIGHT];
#pragma unroll
        for (int j = 0; j < RLN_INFLIGHT; ++j) {
            ok[j] = t + j * RLN_TL <= hi && rfm_inside(vol, X, Y, Z);
            s[j].issue(vol, X, Y, Z, ok[j]);
            X += dX;
            Y += dY;
            Z += dZ;
        }
        unsigned col[RLN_INFLIGHT], alpha[RLN_INFLIGHT], mine[RLN_INFLIGHT];      // each lane classifies its own samples
#pragma unroll
        for (int j = 0; j < RLN_INFLIGHT; ++j) {
            const int cls = (int)stored_level((float)(s[j].value() + add), wp) & 255;
            const uint2 e = tab[cls];
            col[j] = e.x;
            alpha[j] = ok[j] ? e.y : 0u;      // an uncounted step: alpha 0 changes nothing in the chain
        }
#pragma unroll
        for (int pr = 0; pr < RLN_INFLIGHT / 2; ++pr) {
            const int packed = (int)(alpha[2 * pr] | alpha[2 * pr + 1] << 16);      // alpha <= 32768 = 0x8000
            unsigned q[RLN_TL];
#pragma unroll
            for (int k = 0; k < RLN_TL; ++k) q[k] = (unsigned)__shfl(packed, k * RLN_UL + ul, 64);      // lane (ul, k): step k of the slot
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const int j = 2 * pr + half;
                unsigned own = 0;
#pragma unroll
                for (int k = 0; k < RLN_TL; ++k) {      // the steps base + 8 j + k, in order
                    const unsigned al = half ? q[k] >> 16 : q[k] & 0xffffu;
                    const unsigned wgt = ended ? 0u : (Tr * al) >> 15;      // Tr, al <= 2^15
                    own = k == tl ? wgt : own;
                    Tr -= wgt;
                    d = (d < 0 && RLN_ONE - Tr >= surface) ? base + j * RLN_TL + k : d;
                    ended = ended || Tr <= stop;
                }
                mine[j] = own;
            }
        }
        unsigned sh[RLN_INFLIGHT];
#pragma unroll
        for (int j = 0; j < RLN_INFLIGHT; ++j) sh[j] = 256u;
        if constexpr (SHADE) {
            unsigned any = 0;
#pragma unroll
            for (int j = 0; j < RLN_INFLIGHT; ++j) any |= mine[j];
            if (any != 0u) {      // only where a colour is needed
                RlnGrad g[RLN_INFLIGHT];
#pragma unroll
                for (int j = 0; j < RLN_INFLIGHT; ++j)
                    g[j].issue(vol, Xt + dX * (unsigned)j, Yt + dY * (unsigned)j, Zt + dZ * (unsigned)j, mine[j] != 0u);
#pragma unroll
                for (int j = 0; j < RLN_INFLIGHT; ++j) sh[j] = g[j].shade(l0, l1, l2, zscale, ambient, gmin2);
            }
        }
#pragma unroll
        for (int j = 0; j < RLN_INFLIGHT; ++j) {
            unsigned r = col[j] & 255u, g = (col[j] >> 8) & 255u, b = col[j] >> 16;
            if constexpr (SHADE) {
                r = (r * sh[j] + 128u) >> 8;
                g = (g * sh[j] + 128u) >> 8;
                b = (b * sh[j] + 128u) >> 8;
            }
            C0 += mine[j] * r;
            C1 += mine[j] * g;
            C2 += mine[j] * b;
        }
        if (ended) hi = -1;      // no step left: the lanes of this ray read voxel 0 until the wave is through
        base += RLN_TRIP;
    }
#pragma unroll
    for (int o = RLN_UL; o < 64; o <<= 1) {      // the 8 lanes of a ray: lane, lane ^ 8, ^ 16, ^ 32; exact sums below 2^23
        C0 += (unsigned)__shfl_xor((int)C0, o, 64);
        C1 += (unsigned)__shfl_xor((int)C1, o, 64);
        C2 += (unsigned)__shfl_xor((int)C2, o, 64);
    }
    if (!live || tl != 0) return;
    const size_t o = (size_t)l * U + u;
    if (rgb != nullptr) {      // C + bg Tr <= 255 * 32768
        rgb[o * 3 + 0] = (unsigned char)((C0 + bg_r * Tr + 16384u) >> 15);
        rgb[o * 3 + 1] = (unsigned char)((C1 + bg_g * Tr + 16384u) >> 15);
        rgb[o * 3 + 2] = (unsigned char)((C2 + bg_b * Tr + 16384u) >> 15);
    }
    if (opacity != nullptr) opacity[o] = (unsigned char)(((RLN_ONE - Tr) * 255u + 16384u) >> 15);
    if (depth != nullptr) depth[o] = (short)d;
}

extern "C" int ctg_render_lines(const short* vol, int N, int H, int W, const int* lines, int L, int U, int T,
                                const unsigned short* lut, int sampling, int stop, int surface, int bg_r, int bg_g, int bg_b,
                                float wc, float ww, int hu, const int* light, int zscale, int ambient, int gmin2,
                                unsigned char* rgb, unsigned char* opacity, short* depth, void* stream) {
    CTG_ENTER();
    if (vol == nullptr || lines == nullptr || lut == nullptr) return CTG_EINVAL;
    if (rgb == nullptr && opacity == nullptr && depth == nullptr) return CTG_EINVAL;
    if (N < 1 || N > RLN_MAX_DIM || H < 1 || H > RLN_MAX_DIM || W < 1 || W > RLN_MAX_DIM) return CTG_EINVAL;
    if (U < 1 || U > RLN_MAX_DIM || T < 1 || T > RLN_MAX_DIM || L < 1) return CTG_EINVAL;
    if (sampling < 0 || sampling > 1 || stop < 0 || stop > 32767 || surface < 1 || surface > 32768) return CTG_EINVAL;
    if (bg_r < 0 || bg_r > 255 || bg_g < 0 || bg_g > 255 || bg_b < 0 || bg_b > 255) return CTG_EINVAL;
    if (zscale < 1 || zscale > 4096 || ambient < 0 || ambient > 256 || gmin2 < 1 || gmin2 > (1 << 26)) return CTG_EINVAL;
    if (((uintptr_t)vol & 1) != 0 || ((uintptr_t)lines & 3) != 0 || ((uintptr_t)lut & 1) != 0 || ((uintptr_t)light & 3) != 0 ||
        ((uintptr_t)depth & 1) != 0)
        return CTG_EINVAL;
    // one workgroup per (line, segment of 32 columns): the grid's x dimension
    const int nseg = (U + RLN_WG_U - 1) / RLN_WG_U;
    if ((long)L * nseg > 0x7fffffffL) return CTG_EINVAL;
    const dim3 grid((unsigned)((long)L * nseg)), block(RLN_THREADS);
    hipStream_t st = (hipStream_t)stream;
    const RfmVol v{vol, N, H, W};
#define RLN_GO(S, G) hipLaunchKernelGGL((render_lines_kernel<S, G>), grid, block, 0, st, v, lines, U, T, nseg, lut, (unsigned)stop, \
                                        (unsigned)surface, (unsigned)bg_r, (unsigned)bg_g, (unsigned)bg_b, wc, ww, hu ? 1024 : 0,   \
                                        light, zscale, (unsigned)ambient, (unsigned)gmin2, rgb, opacity, depth)
    if (light != nullptr) {
        if (sampling) RLN_GO(true, true);
        else RLN_GO(false, true);
    } else {
        if (sampling) RLN_GO(true, false);
        else RLN_GO(false, false);
    }
#undef RLN_GO
    return ctg_launch_status();
}
