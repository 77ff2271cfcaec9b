// Series inference, the lumen along a centreline: at every position of the line a fan of K rays in the cross-section, each walked
// outward from the centre until the density leaves the lumen's band, the crossing placed between the two samples by linear
// interpolation (cta_gan_amd/infer.py: lumen_lines, lumen_profile, lumen_stenosis, VolumeLumen; ops.lumen_sections).  The curved
// reformat (reformat.hip) shows the vessel; this measures it.  The reference has no counterpart.
//
// The table: int32 [R][K][9] in the row format of reformat.hip.  Section r has the centre C = (x0, y0, z0) of its row (r, 0) and
// ray j the step D_j = (xk, yk, zk) of row (r, j); sample k of ray j lies at the 16.16 position C + k D_j and is counted by
// rfm_inside.  The other entries of a row (the c0 of the rays j > 0, every cu) are not read.  The value of a sample is RfmSample's
// (reformat_sample.h, unchanged).  include/ctagan_hip.h has the rule of the walk, the recentring and the outputs; every figure is
// integer arithmetic, equal to numpy bit for bit (tests/lumen_np.py).
//
// Layout: lane = ray.  A wave carries 64 / K sections in groups of K neighbouring lanes, a workgroup of 256 threads four waves; a
// group whose section index is not below R does nothing but take part in the shuffles.  The centre sample is loaded by the
// group's lane 0 and handed to the others by a shuffle.  A lane keeps LUM_INFLIGHT samples in flight ahead of the one it tests
// (the gathers of a ray are a dependent chain otherwise: one latency per step); what is loaded past the stop is thrown away, and
// it is safe to load because RfmSample clamps or checks every address and a sample that is not counted reads voxel 0.  A lane
// leaves the walk when its ray has stopped, so a group is done when all its rays are.  The reductions over a section -- the sum,
// the neighbour products, the chord minimum and maximum with their rays, the open count and the three sums of the move -- are
// xor-shuffles with offsets below K, which stay inside the group; an int64 travels as two halves.  All shuffles run in converged
// code: the walk is the only divergent region.
//
// Safety: every volume address as in reformat.hip; every store is a vector store to an index derived from a section index that
// was checked against R.  The fixed-point sums are formed in unsigned arithmetic and read as int32; ops.lumen_sections refuses a
// table in which |c0| + (1 + 2 recentre) (T-1) max_j |ck_j| could reach 2^31, under which nothing wraps: one move is at most
// 2 (T-1) max_j |ck_j| on an axis, because rho <= 256 (T-1).
#include "common.h"
#include "reformat_sample.h"

#define LUM_THREADS 256
#define LUM_INFLIGHT 4        // samples a lane issues before it tests the first
#define LUM_MAX_STEPS 256     // T: rho <= 255 * 256 = 65280
#define LUM_MAX_RECENTRE 4
#define LUM_MAX_DIM 4096      // N, H, W, as for the line tables

// lane ^ o of an int64, as two halves
__device__ __forceinline__ long long lum_shfl_xor64(long long v, int o) {
    const int lo = __shfl_xor((int)(unsigned)((unsigned long long)v & 0xffffffffull), o, 64);
    const int hi = __shfl_xor((int)((unsigned long long)v >> 32), o, 64);
    return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo);
}

template <bool LERP, int K>
__global__ __launch_bounds__(LUM_THREADS) void lumen_sections_kernel(RfmVol vol, const int* __restrict__ lines, int R, int T, int lo,
                                                                     int hi, int half, int base, int recentre, int* __restrict__ radii,
                                                                     long long* __restrict__ cross, int* __restrict__ sections,
                                                                     int* __restrict__ centres) {
    constexpr int LOGK = K == 8 ? 3 : (K == 16 ? 4 : (K == 32 ? 5 : 6));
    static_assert((1 << LOGK) == K, "K is 8, 16, 32 or 64");
    const int lane = threadIdx.x & 63, j = lane & (K - 1), first = lane & ~(K - 1);
    const long r = ((long)blockIdx.x * (LUM_THREADS / 64) + (threadIdx.x >> 6)) * (64 / K) + lane / K;
    const bool live = r < (long)R;      // (the same for the K lanes of a group)
    const int* __restrict__ c0 = lines + (size_t)(live ? r : 0) * K * 9;      // row (r, 0): the centre
    const int* __restrict__ cj = c0 + j * 9;                                 // row (r, j): the step
    unsigned CX = (unsigned)c0[0], CY = (unsigned)c0[3], CZ = (unsigned)c0[6];
    const unsigned dX = (unsigned)cj[2], dY = (unsigned)cj[5], dZ = (unsigned)cj[8];

    // what the last walk of the section left: kept while the section no longer walks
    int rho = 0, open = 0, outside = 0, lor = lo;
    int sum = 0, kmin = 0, kmax = 0, nopen = 0;
    long long crs = 0;
    bool act = live;
    for (int it = 0;; ++it) {
        // the centre sample: one load per section
        const bool cin = rfm_inside(vol, CX, CY, CZ);
        int s0 = 0;
        if (act && j == 0 && cin) {
            RfmSample<LERP> s;
            s.issue(vol, CX, CY, CZ, true);
            s0 = s.value();
        }
        s0 = __shfl(s0, first, 64);
        if (act) {
            outside = (!cin || s0 < lo || s0 > hi) ? 1 : 0;
            lor = lo;
            rho = 0;
            open = 0;
            if (!outside) {
                if (half) {
                    const int mid = (s0 + base) >> 1;
                    lor = mid > lo ? mid : lo;
                }
                int prev = s0, k = 1;
                bool stopped = false;
                unsigned X = CX + dX, Y = CY + dY, Z = CZ + dZ;
                while (!stopped && k < T) {
                    bool ok[LUM_INFLIGHT];
                    RfmSample<LERP> s[LUM_INFLIGHT];
#pragma unroll
                    for (int f = 0; f < LUM_INFLIGHT; ++f) {
                        ok[f] = k + f < T && rfm_inside(vol, X, Y, Z);
                        s[f].issue(vol, X, Y, Z, ok[f]);
                        X += dX;
                        Y += dY;
                        Z += dZ;
                    }
#pragma unroll
                    for (int f = 0; f < LUM_INFLIGHT; ++f) {
                        if (stopped || k + f >= T) continue;
                        const int at = (k + f - 1) << 8;
                        if (!ok[f]) {
                            rho = at;
                            open = 1;
                            stopped = true;
                            continue;
                        }
                        const int v = s[f].value();
                        if (v < lor) {
                            rho = at + ((prev - lor) << 8) / (prev - v);      // 0 <= prev - lor < prev - v
                            stopped = true;
                        } else if (v > hi) {
                            rho = at + ((hi - prev) << 8) / (v - prev);       // 0 <= hi - prev < v - prev
                            stopped = true;
                        } else {
                            prev = v;
                        }
                    }
                    k += LUM_INFLIGHT;
                }
                if (!stopped) {
                    rho = (T - 1) << 8;
                    open = 1;
                }
            }
        }
        // the section's figures (every lane, converged): a section that no longer walks gives what it gave before
        const int next = __shfl(rho, first | ((j + 1) & (K - 1)), 64), opp = __shfl(rho, lane ^ (K / 2), 64);
        const int chord = rho + opp, jj = j & (K / 2 - 1);      // chord <= 130560 < 2^17; the two ends of a chord make one key
        sum = rho;
        nopen = open;
        crs = (long long)rho * next;
        kmin = (chord << 6) | jj;             // the least key: the least chord, the lowest j on a tie
        kmax = (chord << 6) | (63 - jj);      // the greatest key: the greatest chord, the lowest j on a tie
        long long SX = (long long)rho * (int)dX, SY = (long long)rho * (int)dY, SZ = (long long)rho * (int)dZ;
#pragma unroll
        for (int o = 1; o < K; o <<= 1) {
            sum += __shfl_xor(sum, o, 64);
            nopen += __shfl_xor(nopen, o, 64);
            crs += lum_shfl_xor64(crs, o);
            const int a = __shfl_xor(kmin, o, 64), b = __shfl_xor(kmax, o, 64);
            kmin = a < kmin ? a : kmin;
            kmax = b > kmax ? b : kmax;
            SX += lum_shfl_xor64(SX, o);
            SY += lum_shfl_xor64(SY, o);
            SZ += lum_shfl_xor64(SZ, o);
        }
        if (it >= recentre) break;      // (uniform)
        act = act && !outside && nopen == 0;
        if (act) {      // twice the mean boundary point, rounded to nearest: an arithmetic shift
            CX += (unsigned)(int)((SX + ((long long)K << 6)) >> (7 + LOGK));
            CY += (unsigned)(int)((SY + ((long long)K << 6)) >> (7 + LOGK));
            CZ += (unsigned)(int)((SZ + ((long long)K << 6)) >> (7 + LOGK));
        }
        if (__ballot(act) == 0ull) break;      // (uniform)
    }
    if (!live) return;
    radii[(size_t)r * K + j] = rho;
    if (j == 0) {
        cross[r] = crs;
        int* __restrict__ s = sections + (size_t)r * 8;
        s[0] = sum;
        s[1] = kmin >> 6;
        s[2] = kmax >> 6;
        s[3] = kmin & 63;
        s[4] = 63 - (kmax & 63);
        s[5] = nopen;
        s[6] = outside;
        s[7] = lor;
        int* __restrict__ p = centres + (size_t)r * 3;
        p[0] = (int)CX;
        p[1] = (int)CY;
        p[2] = (int)CZ;
    }
}

template <bool LERP, int K>
static void lumen_sections_launch(const RfmVol& vol, const int* lines, int R, int T, int lo, int hi, int edge, int base, int recentre,
                                  int* radii, long long* cross, int* sections, int* centres, hipStream_t st) {
    const long per = (long)(LUM_THREADS / 64) * (64 / K);
    hipLaunchKernelGGL((lumen_sections_kernel<LERP, K>), dim3((unsigned)(((long)R + per - 1) / per)), dim3(LUM_THREADS), 0, st, vol, lines,
                       R, T, lo, hi, edge, base, recentre, radii, cross, sections, centres);
}

extern "C" int ctg_lumen_sections(const short* vol, int N, int H, int W, const int* lines, int R, int K, int T, int lo, int hi,
                                  int sampling, int edge, int base, int recentre, int* radii, long long* cross, int* sections,
                                  int* centres, void* stream) {
    CTG_ENTER();
    if (vol == nullptr || lines == nullptr || radii == nullptr || cross == nullptr || sections == nullptr || centres == nullptr)
        return CTG_EINVAL;
    if (N < 1 || N > LUM_MAX_DIM || H < 1 || H > LUM_MAX_DIM || W < 1 || W > LUM_MAX_DIM) return CTG_EINVAL;
    if (R < 1 || (K != 8 && K != 16 && K != 32 && K != 64) || (long)R * K > 0x7fffffffL) return CTG_EINVAL;
    if (T < 2 || T > LUM_MAX_STEPS || recentre < 0 || recentre > LUM_MAX_RECENTRE) return CTG_EINVAL;
    if (lo < -32768 || hi > 32767 || lo > hi || sampling < 0 || sampling > 1 || edge < 0 || edge > 1) return CTG_EINVAL;
    if (edge == 1 && (base < -32768 || base > lo)) return CTG_EINVAL;
    if (((uintptr_t)vol & 1) != 0 || ((uintptr_t)lines & 3) != 0 || ((uintptr_t)radii & 3) != 0 || ((uintptr_t)cross & 7) != 0 ||
        ((uintptr_t)sections & 3) != 0 || ((uintptr_t)centres & 3) != 0)
        return CTG_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const RfmVol v{vol, N, H, W};
#define LUM_GO(S, KK) lumen_sections_launch<S, KK>(v, lines, R, T, lo, hi, edge, base, recentre, radii, cross, sections, centres, st)
    if (sampling) {
        if (K == 8) LUM_GO(true, 8);
        else if (K == 16) LUM_GO(true, 16);
        else if (K == 32) LUM_GO(true, 32);
        else LUM_GO(true, 64);
    } else {
        if (K == 8) LUM_GO(false, 8);
        else if (K == 16) LUM_GO(false, 16);
        else if (K == 32) LUM_GO(false, 32);
        else LUM_GO(false, 64);
    }
#undef LUM_GO
    return ctg_launch_status();
}
