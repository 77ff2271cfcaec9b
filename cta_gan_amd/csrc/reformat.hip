// Series inference, lines in any direction: oblique planes, tumbling views and curved reformats of the exported int16 volume
// (cta_gan_amd/infer.py: view_lines, orbit_lines, oblique_lines, curved_lines, VolumeReformatter).  The kernels of project.hip,
// project_slabs.hip, project_rotate.hip and project_render.hip make displays whose rows depend on one slice only; a line that
// crosses slices needs the whole volume on the device, which about 150 MB of int16 allows.  Like them the reference has no
// counterpart (its test() writes slices only).
//
// The table: int32 [L][9], one row (x0, xu, xk, y0, yu, yk, z0, zu, zk) per output line.  Sample (l, i, k), i in 0 .. U-1 along
// the line and k in 0 .. T-1 along its ray, lies at the 16.16 fixed-point position
//     X = x0 + xu i + xk k,   Y = y0 + yu i + yk k,   Z = z0 + zu i + zk k
// formed on the host with the + 0.5 of the nearest rule inside (infer.py, as rotation_coefficients does), and is counted exactly
// when voxel (X >> 16, Y >> 16, Z >> 16) (arithmetic shift) lies in the volume.  out[l][i] is the max, min or mean over the
// counted samples of the ray -- the mean is the sum over the ray's own count by C division -- and `fill` where none is counted;
// the level is stored_level(v + (hu ? 1024 : 0)) in the same pass, as project_rotate.hip writes it.  T = 1 is a plain reformat
// (MPR), T > 1 a slab or a projection along the ray.  Everything up to the 8-bit level is integer arithmetic, equal to numpy
// bit for bit (tests/reformat_np.py).
//
// Sampling 0 is nearest: the voxel above.  Sampling 1 is trilinear in exact integers about the centre-based position
// Xc = X - 32768 (Y, Z likewise):  x0 = Xc >> 16, fx = (Xc >> 8) & 255 for each axis,
//     v0 = rot_lerp(four in-plane neighbours on slice clamp(z0), fx, fy),   v1 = the same on slice clamp(z0 + 1),
//     v  = (v0 (256 - fz) + v1 fz + 128) >> 8
// with the in-plane neighbours clamped as the bilinear rotation clamps them (rotate_sample.h, unchanged): two roundings, each
// defined.  v0 and v1 are int16 values (rot_lerp), the two weights sum to 256, so |v0 (256 - fz) + v1 fz| <= 2^23 and v is an
// int16 value: -32768 and 32767 come back as themselves and a constant volume stays constant.  Eight 16-bit loads per sample,
// since only 2-byte alignment is promised.  With fz = 0 (an integer z + 0.5) v = v0: the bilinear rotation's value.
//
// Safety: a sample is read only after its own voxel index passed the bounds check (nearest), or through indices clamped into
// the volume (trilinear), and a sample that is not counted reads voxel 0: every address is inside the volume whatever the table
// holds.  The fixed-point sums are formed in unsigned arithmetic (wraps, never undefined) and read as int32; ops.LineTable
// refuses a table whose sums could leave int32 (|c0| + |cu| (U-1) + |ck| (T-1) < 2^31 per line and axis), under which the
// interval below is exact.  Steps above one voxel are in range: anisotropic volumes need them.
//
// T > 1 keeps the rotation kernel's layout: a wave owns RFM_UL = 8 neighbouring rays of one line and walks them with 8 lanes
// each, lane (ul, tl) taking the steps t = tl (mod 8), so that one gather instruction covers an 8 x 8 patch of (i, k); rot_clip,
// applied three times, gives the interval of steps that can be inside the volume and the lanes walk only that, RFM_INFLIGHT
// gathers issued before the first is used; the 8 partials of a ray meet in three xor-shuffles (max, min, sum and count are exact
// and commutative).  One 256-thread workgroup per (line, segment of 32 columns); the nine coefficients are workgroup-uniform.
//
// T = 1 has no ray to share out, so it is an instantiation of its own with one output pixel per lane and no shuffles.  Two
// layouts exist: a wave on an 8 x 8 patch of (line, column) -- when the lines are neighbouring rows of a plane, a gather of the
// wave then touches a patch of the plane, at most a dozen rows of a slice, at any orientation (the argument of
// project_rotate.hip) -- and a wave on 64 columns of one line, which touches 64 rows where the line runs along y or z.
// Which is faster depends on the sampling (RFM_T1_ROWS below; LAB_NOTES has both times of both); CTG_REFORMAT_T1 = 1 / 2 forces
// the patch / the columns for both (a developer A/B switch, ctg_knobs.h).
#include "common.h"
#include "ctg_knobs.h"
#include "reformat_sample.h"
#include "rotate_sample.h"
#include "window_arith.h"

#define RFM_THREADS 256
#define RFM_UL 8            // rays of a wave
#define RFM_TL 8            // lanes of a ray: lane tl takes the steps t = tl (mod RFM_TL)
#define RFM_WG_U (RFM_THREADS / 64 * RFM_UL)
#define RFM_INFLIGHT 4      // samples a lane issues before it uses the first
#define RFM_MAX_DIM 4096    // N, H, W, U, T: (dim << 16) - 1 stays below 2^28
#define RFM_PATCH 8         // T = 1: a wave on RFM_PATCH x RFM_PATCH (line, column)
#define RFM_T1_ROWS(sampling) ((sampling) == 0)      // T = 1: nearest on 64 columns of one line, trilinear on the patch

enum { RFM_MAX = 0, RFM_MIN = 1, RFM_SUM = 2 };

template <int MODE> __device__ __forceinline__ int rfm_op(int a, int b) {
    if constexpr (MODE == RFM_MAX) return a > b ? a : b;
    else if constexpr (MODE == RFM_MIN) return a < b ? a : b;
    else return a + b;
}

__device__ __forceinline__ void rfm_store(int v, size_t o, float wc, float ww, int add, short* __restrict__ values,
                                          unsigned char* __restrict__ level) {
    if (values != nullptr) values[o] = (short)v;
    if (level != nullptr) level[o] = (unsigned char)(int)stored_level((float)(v + add), win_params(wc, ww));
}

// T > 1: 8 rays x 8 lanes per wave
template <int MODE, bool LERP>
__global__ __launch_bounds__(RFM_THREADS) void reformat_rays_kernel(RfmVol vol, const int* __restrict__ lines, int U, int T, int nseg,
                                                                    int fill, float wc, float ww, int add,
                                                                    short* __restrict__ values, unsigned char* __restrict__ level) {
    const unsigned l = blockIdx.x / (unsigned)nseg, seg = blockIdx.x % (unsigned)nseg;
    const int lane = threadIdx.x & 63, tl = lane / RFM_UL;
    const int u = (int)(seg * RFM_WG_U + (threadIdx.x >> 6) * RFM_UL + lane % RFM_UL);
    const bool live = u < U;      // (every lane stays for the shuffles; the 8 lanes of a ray are live together)
    const int* __restrict__ c = lines + (size_t)l * 9;
    const unsigned cx = (unsigned)c[2], cy = (unsigned)c[5], cz = (unsigned)c[8];
    const unsigned X0 = (unsigned)c[0] + (unsigned)c[1] * (unsigned)u, Y0 = (unsigned)c[3] + (unsigned)c[4] * (unsigned)u;
    const unsigned Z0 = (unsigned)c[6] + (unsigned)c[7] * (unsigned)u;
    int lo = 0, hi = live ? T - 1 : -1;
    rot_clip((int)X0, (int)cx, (vol.W << 16) - 1, lo, hi);
    rot_clip((int)Y0, (int)cy, (vol.H << 16) - 1, lo, hi);
    rot_clip((int)Z0, (int)cz, (vol.N << 16) - 1, lo, hi);
    int acc = MODE == RFM_MAX ? -32768 : (MODE == RFM_MIN ? 32767 : 0), cnt = 0;
    int t = (lo & ~(RFM_TL - 1)) + tl;      // lo >= 0
    unsigned X = X0 + cx * (unsigned)t, Y = Y0 + cy * (unsigned)t, Z = Z0 + cz * (unsigned)t;
    const unsigned dX = cx * RFM_TL, dY = cy * RFM_TL, dZ = cz * RFM_TL;
    for (; t <= hi; t += RFM_TL * RFM_INFLIGHT) {
        bool ok[RFM_INFLIGHT];
        RfmSample<LERP> s[RFM_INFLIGHT];
#pragma unroll
        for (int j = 0; j < RFM_INFLIGHT; ++j) {
            ok[j] = t + j * RFM_TL <= hi && rfm_inside(vol, X, Y, Z);
            s[j].issue(vol, X, Y, Z, ok[j]);
            X += dX;
            Y += dY;
            Z += dZ;
        }
#pragma unroll
        for (int j = 0; j < RFM_INFLIGHT; ++j) {
            if (!ok[j]) continue;
            acc = rfm_op<MODE>(acc, s[j].value());
            ++cnt;
        }
    }
#pragma unroll
    for (int o = RFM_UL; o < 64; o <<= 1) {      // the 8 lanes of a ray: lane, lane ^ 8, ^ 16, ^ 32
        acc = rfm_op<MODE>(acc, __shfl_xor(acc, o, 64));
        cnt += __shfl_xor(cnt, o, 64);
    }
    if (!live || tl != 0) return;
    int v = fill;
    if (cnt > 0) v = MODE == RFM_SUM ? acc / cnt : acc;      // C division: truncates toward zero
    rfm_store(v, (size_t)l * U + u, wc, ww, add, values, level);
}

// T = 1: one output pixel per lane; the one sample is the ray, so max, min and mean are the sample itself.  PATCH: a wave on
// 8 lines x 8 columns, a workgroup on 8 lines x 32 columns; otherwise a wave on 64 columns of one line, a workgroup on 256.
template <bool LERP, bool PATCH>
__global__ __launch_bounds__(RFM_THREADS) void reformat_plane_kernel(RfmVol vol, const int* __restrict__ lines, int L, int U, int nseg,
                                                                     int fill, float wc, float ww, int add,
                                                                     short* __restrict__ values, unsigned char* __restrict__ level) {
    const unsigned band = blockIdx.x / (unsigned)nseg, seg = blockIdx.x % (unsigned)nseg;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned l, u;      // (unsigned: the last band of L = 2^31 - 1 lines reaches past int)
    if constexpr (PATCH) {
        l = band * RFM_PATCH + (unsigned)(lane / RFM_PATCH);
        u = seg * (RFM_THREADS / 64 * RFM_PATCH) + (unsigned)(wave * RFM_PATCH + lane % RFM_PATCH);
    } else {
        l = band;
        u = seg * RFM_THREADS + threadIdx.x;
    }
    if (l >= (unsigned)L || u >= (unsigned)U) return;
    const int* __restrict__ c = lines + (size_t)l * 9;
    const unsigned X = (unsigned)c[0] + (unsigned)c[1] * (unsigned)u, Y = (unsigned)c[3] + (unsigned)c[4] * (unsigned)u;
    const unsigned Z = (unsigned)c[6] + (unsigned)c[7] * (unsigned)u;
    const bool ok = rfm_inside(vol, X, Y, Z);
    RfmSample<LERP> s;
    s.issue(vol, X, Y, Z, ok);
    rfm_store(ok ? s.value() : fill, (size_t)l * U + u, wc, ww, add, values, level);
}

template <int MODE, bool LERP>
static void reformat_rays_launch(const RfmVol& vol, const int* lines, int L, int U, int T, int fill, float wc, float ww, int hu,
                                 short* values, unsigned char* level, hipStream_t st) {
    const int nseg = (U + RFM_WG_U - 1) / RFM_WG_U;
    hipLaunchKernelGGL((reformat_rays_kernel<MODE, LERP>), dim3((unsigned)((long)L * nseg)), dim3(RFM_THREADS), 0, st, vol, lines, U, T,
                       nseg, fill, wc, ww, hu ? 1024 : 0, values, level);
}

template <bool LERP, bool PATCH>
static void reformat_plane_launch(const RfmVol& vol, const int* lines, int L, int U, int fill, float wc, float ww, int hu,
                                  short* values, unsigned char* level, hipStream_t st) {
    const int cols = PATCH ? RFM_THREADS / 64 * RFM_PATCH : RFM_THREADS, rows = PATCH ? RFM_PATCH : 1;
    const int nseg = (U + cols - 1) / cols;
    hipLaunchKernelGGL((reformat_plane_kernel<LERP, PATCH>), dim3((unsigned)(((long)L + rows - 1) / rows * nseg)), dim3(RFM_THREADS), 0,
                       st, vol, lines, L, U, nseg, fill, wc, ww, hu ? 1024 : 0, values, level);
}

extern "C" int ctg_reformat_lines(const short* vol, int N, int H, int W, const int* lines, int L, int U, int T, int mode,
                                  int sampling, int fill, float wc, float ww, int hu, short* values, unsigned char* level,
                                  void* stream) {
    CTG_ENTER();
    if (vol == nullptr || lines == nullptr || (values == nullptr && level == nullptr)) return CTG_EINVAL;
    if (N < 1 || N > RFM_MAX_DIM || H < 1 || H > RFM_MAX_DIM || W < 1 || W > RFM_MAX_DIM) return CTG_EINVAL;
    if (U < 1 || U > RFM_MAX_DIM || T < 1 || T > RFM_MAX_DIM || L < 1) return CTG_EINVAL;
    if (mode < RFM_MAX || mode > RFM_SUM || sampling < 0 || sampling > 1 || fill < -32768 || fill > 32767) return CTG_EINVAL;
    if (((uintptr_t)vol & 1) != 0 || ((uintptr_t)lines & 3) != 0 || ((uintptr_t)values & 1) != 0) return CTG_EINVAL;
    // the largest grid any layout makes of (L, U): one workgroup per (line, segment of 32 columns)
    if ((long)L * ((U + RFM_WG_U - 1) / RFM_WG_U) > 0x7fffffffL) return CTG_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const RfmVol v{vol, N, H, W};
    if (T == 1) {
        const int forced = ctg_knobs().reformat_t1;
        const bool rows = forced == 2 || (forced != 1 && RFM_T1_ROWS(sampling));
#define RFM_PLANE_GO(S, P) reformat_plane_launch<S, P>(v, lines, L, U, fill, wc, ww, hu, values, level, st)
        if (sampling) {
            if (rows) RFM_PLANE_GO(true, false);
            else RFM_PLANE_GO(true, true);
        } else {
            if (rows) RFM_PLANE_GO(false, false);
            else RFM_PLANE_GO(false, true);
        }
#undef RFM_PLANE_GO
        return ctg_launch_status();
    }
#define RFM_RAYS_GO(M, S) reformat_rays_launch<M, S>(v, lines, L, U, T, fill, wc, ww, hu, values, level, st)
    if (sampling) {
        if (mode == RFM_MAX) RFM_RAYS_GO(RFM_MAX, true);
        else if (mode == RFM_MIN) RFM_RAYS_GO(RFM_MIN, true);
        else RFM_RAYS_GO(RFM_SUM, true);
    } else {
        if (mode == RFM_MAX) RFM_RAYS_GO(RFM_MAX, false);
        else if (mode == RFM_MIN) RFM_RAYS_GO(RFM_MIN, false);
        else RFM_RAYS_GO(RFM_SUM, false);
    }
#undef RFM_RAYS_GO
    return ctg_launch_status();
}
