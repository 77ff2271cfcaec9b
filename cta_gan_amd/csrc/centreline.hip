// Series inference, the vessel centreline between clicked voxels of the resident volume (cta_gan_amd/infer.py: VolumeCentreline,
// centreline_volume, SeriesTranslator(centreline=...); ops.centreline_clearance / centreline_field / centreline_trace): the path a
// curved reformat is laid along, as a minimal-cost path over a clearance map.  The reference has no counterpart.
// include/ctagan_hip.h has the contract; tests/centreline_np.py is the numpy restatement, equal bit for bit.
//
//   cl_clear_x / _y / _z    clear[v] = min(R^2, the squared distance to the nearest background voxel inside the volume), z scaled
//                           by zq (aspect^2 in 8.8 fixed point), as three separable passes of capped brute-force windows: the
//                           distance along the row (at most R), then min over |dy| < R of g^2 + dy^2, then min over the slices
//                           with q(|dz|) < R^2 of that + q(|dz|).  A lane per voxel, lanes along x; uint16 in, uint16 out.
//   cl_seed_kernel          dist = 0xFFFFFFFF everywhere but 0 at `start`; active, marks and stats zeroed; the tile of start marked.
//   cl_relax_kernel         round r.  A workgroup owns a tile CL_TZ x CL_TY x CL_TX = 8 x 16 x 32 voxels and leaves at once unless
//                           active[r & 1][tile] is set (it clears it: nobody else reads that entry in this round).  It loads dist
//                           and the cost pen[clear] of the tile plus a one-voxel halo into LDS (24 KB + 12 KB, the pen table 2 KB),
//                           then relaxes the 4096 interior voxels, 16 per thread, in place until a sweep changes nothing or
//                           CL_LOCAL_ITERS sweeps are done; a value in LDS is always the cost of some path, so a thread may read a
//                           neighbour before or after its owner lowered it.  Every lowered voxel goes back with an agent-scope
//                           atomicMin, and every neighbouring tile whose face, edge or corner was lowered -- and the tile itself
//                           when it ran into the sweep cap -- is marked in active[(r + 1) & 1]; marks[r] counts the marks.
//                           Every read of `dist` is a relaxed agent-scope atomic load (the L2s of the 8 XCDs are not coherent for
//                           plain accesses).  The halo is read-only, so a neighbour that lowers it in the same round is seen one
//                           round later: that tile marks this one.  min(., SAT) is monotone, so the least fixed point is unique
//                           and the field does not depend on the order in which anything lands.
//   cl_saturated_kernel     after the last round: stats[3] = 1 when a voxel reads SAT (from the final field, not from a transient).
//   cl_trace_kernel         a wave per end, lanes 0 .. 25 hold the 26 neighbours; the predecessor is the smallest linear index among
//                           those that explain dist[v], found by a wave minimum.
//
// Safety: no workgroup ever waits for another -- no flags polled, no tickets, no cooperative launch; every hand-over is a kernel
// boundary.  The loops that depend on memory are the local sweeps (at most CL_LOCAL_ITERS), the walk of the trace (at most
// max_points, and only while dist strictly decreases) and the windows of the clearance (at most R, or N, steps).  Every neighbour
// address is formed from indices that passed a bounds check; an index read from `ends` is range-checked before it indexes
// anything; what is read from `pen` is clamped into 1 .. 4095 and `clear` indexes it only below R^2 + 1.  Integer arithmetic only.
#include "common.h"

#define CL_TZ 8
#define CL_TY 16
#define CL_TX 32
#define CL_THREADS 256
#define CL_TILE (CL_TZ * CL_TY * CL_TX)
#define CL_PER (CL_TILE / CL_THREADS)      // interior voxels per thread
#define CL_HY (CL_TY + 2)
#define CL_HX (CL_TX + 2)
#define CL_CELLS ((CL_TZ + 2) * CL_HY * CL_HX)
#define CL_LOCAL_ITERS 64      // most sweeps of a tile per launch; a tile that is not done by then marks itself
#ifndef CL_LOCAL        // 0: the A/B build without the LDS iteration -- an active tile relaxes each of its voxels once per round
#define CL_LOCAL 1      // on global memory (LAB_NOTES has both timings)
#endif
#define CL_MAX_R 32
#define CL_MAX_ENDS 64
#define CL_MAX_ROUNDS (1 << 20)
#define CL_MAX_POINTS (1 << 24)
#define CL_UNREACHED 0xFFFFFFFFu
#define CL_SAT 0xFFFFFFFEu
#define CL_STREAM_THREADS 256
#define CL_STREAM_BLOCKS 4096

typedef unsigned short u16;

struct ClSteps {
    int s[5];      // in-plane face, in-plane edge, z alone, z + one in-plane, z + two in-plane
};

__device__ __forceinline__ constexpr int cl_kind(int dz, int dy, int dx) {
    const int k = (dy != 0) + (dx != 0);
    return dz == 0 ? k - 1 : 2 + k;
}

// min(d + w, SAT) for d <= SAT, w < 2^21
__device__ __forceinline__ unsigned cl_add(unsigned d, unsigned w) {
    const unsigned s = d + w;
    return (s < d || s > CL_SAT) ? CL_SAT : s;
}

__device__ __forceinline__ unsigned cl_pen(const u16* __restrict__ pen, int c) {
    const unsigned p = pen[c];
    return p < 1u ? 1u : (p > 4095u ? 4095u : p);
}

__device__ __forceinline__ unsigned cl_ld(const unsigned* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---------------------------------------------------------------------------------------------------------------- clearance
__global__ __launch_bounds__(CL_STREAM_THREADS) void cl_clear_x_kernel(const short* __restrict__ vol, long V, int W, int lo, int hi, int R,
                                                                        u16* __restrict__ g) {
    for (long i = (long)blockIdx.x * CL_STREAM_THREADS + threadIdx.x; i < V; i += (long)gridDim.x * CL_STREAM_THREADS) {
        const int x = (int)(i % W);
        const long row = i - x;
        const int v = vol[i];
        int r = 0;
        if (v >= lo && v <= hi) {
            r = R;
            for (int d = 1; d < R; ++d) {
                bool hit = false;
                if (x - d >= 0) {
                    const int a = vol[row + x - d];
                    hit = a < lo || a > hi;
                }
                if (!hit && x + d < W) {
                    const int a = vol[row + x + d];
                    hit = a < lo || a > hi;
                }
                if (hit) {
                    r = d;
                    break;
                }
            }
        }
        g[i] = (u16)r;
    }
}

__global__ __launch_bounds__(CL_STREAM_THREADS) void cl_clear_y_kernel(const u16* __restrict__ g, long V, int H, int W, int R,
                                                                        u16* __restrict__ out) {
    for (long i = (long)blockIdx.x * CL_STREAM_THREADS + threadIdx.x; i < V; i += (long)gridDim.x * CL_STREAM_THREADS) {
        const int y = (int)((i / W) % H);
        const int c = g[i];
        int best = c * c;      // c <= R: at most R^2; 0 on background
        for (int d = 1; d < R; ++d) {
            const int dd = d * d;
            if (dd >= best) break;      // every further term is at least dd
            if (y - d >= 0) {
                const int t = g[i - (long)d * W];
                best = min(best, t * t + dd);
            }
            if (y + d < H) {
                const int t = g[i + (long)d * W];
                best = min(best, t * t + dd);
            }
        }
        out[i] = (u16)best;
    }
}

__global__ __launch_bounds__(CL_STREAM_THREADS) void cl_clear_z_kernel(const u16* __restrict__ f, long V, int N, long HW, int zq,
                                                                        u16* __restrict__ out) {
    for (long i = (long)blockIdx.x * CL_STREAM_THREADS + threadIdx.x; i < V; i += (long)gridDim.x * CL_STREAM_THREADS) {
        const int z = (int)(i / HW);
        int best = f[i];      // at most R^2; 0 on background
        for (int d = 1; d < N; ++d) {
            const long q = ((long)d * d * zq + 128) >> 8;      // non-decreasing in d
            if (q >= best) break;      // every further term is at least q
            if (z - d >= 0) best = min(best, (int)f[i - (long)d * HW] + (int)q);
            if (z + d < N) best = min(best, (int)f[i + (long)d * HW] + (int)q);
        }
        out[i] = (u16)best;
    }
}

// ---------------------------------------------------------------------------------------------------------------- field
__global__ __launch_bounds__(CL_STREAM_THREADS) void cl_seed_kernel(const u16* __restrict__ clear, long V, long start, long start_tile,
                                                                     unsigned* __restrict__ dist, int* __restrict__ active, long tiles2,
                                                                     int* __restrict__ marks, int max_rounds, int* __restrict__ stats) {
    const long t0 = (long)blockIdx.x * CL_STREAM_THREADS + threadIdx.x, step = (long)gridDim.x * CL_STREAM_THREADS;
    const bool ok = start >= 0 && start < V && clear[start] != 0;
    for (long i = t0; i < V; i += step) dist[i] = (ok && i == start) ? 0u : CL_UNREACHED;
    for (long i = t0; i < tiles2; i += step) active[i] = (ok && i == start_tile) ? 1 : 0;
    for (long i = t0; i < max_rounds; i += step) marks[i] = 0;
    if (t0 < 8) stats[t0] = (t0 == 0 && !ok) ? 1 : 0;
}

// the tiles to mark for a lowered voxel at (lz, ly, lx) of the tile: bit (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1), the centre included
__device__ __forceinline__ unsigned cl_mark_bits(int lz, int ly, int lx) {
    const unsigned xs = 2u | (lx == 0 ? 1u : 0u) | (lx == CL_TX - 1 ? 4u : 0u);
    const unsigned ys = (xs << 3) | (ly == 0 ? xs : 0u) | (ly == CL_TY - 1 ? xs << 6 : 0u);
    return (ys << 9) | (lz == 0 ? ys : 0u) | (lz == CL_TZ - 1 ? ys << 18 : 0u);
}

// the workgroup's marks into active[(r + 1) & 1] and their count into marks[r]; bits as cl_mark_bits
__device__ __forceinline__ void cl_publish(unsigned bits, unsigned* smask, int tz, int ty, int tx, int tzn, int tyn, int txn,
                                           int* __restrict__ next, int* __restrict__ mark) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bits |= (unsigned)__shfl_xor((int)bits, o, 64);
    if ((threadIdx.x & 63) == 0 && bits != 0) atomicOr(smask, bits);
    __syncthreads();
    if (threadIdx.x < 64) {      // (wave 0, whole)
        const int b = threadIdx.x;
        bool set = false;
        if (b < 27 && ((*smask >> b) & 1u)) {
            const int nz = tz + b / 9 - 1, ny = ty + (b / 3) % 3 - 1, nx = tx + b % 3 - 1;
            if (nz >= 0 && nz < tzn && ny >= 0 && ny < tyn && nx >= 0 && nx < txn) {
                __hip_atomic_store(next + ((long)nz * tyn + ny) * txn + nx, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                set = true;
            }
        }
        const int n = __popcll(__ballot(set));
        if (b == 0 && n != 0) atomicAdd(mark, n);
    }
}

__global__ __launch_bounds__(CL_THREADS) void cl_relax_kernel(const u16* __restrict__ clear, int N, int H, int W, int tzn, int tyn, int txn,
                                                               const u16* __restrict__ pen, int R2, ClSteps st,
                                                               unsigned* __restrict__ dist, int* __restrict__ active, long tiles,
                                                               int* __restrict__ marks, int r) {
    __shared__ unsigned smask;
    __shared__ int sactive;
    const int tile = blockIdx.x;
    int* mine = active + (long)(r & 1) * tiles + tile;
    if (threadIdx.x == 0) {
        sactive = __hip_atomic_load(mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        smask = 0u;
    }
    __syncthreads();
    if (sactive == 0) return;      // (the same for the whole workgroup)
    if (threadIdx.x == 0) __hip_atomic_store(mine, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int tx = tile % txn, ty = (tile / txn) % tyn, tz = tile / (txn * tyn);
    const int z0 = tz * CL_TZ, y0 = ty * CL_TY, x0 = tx * CL_TX;
    int* next = active + (long)((r + 1) & 1) * tiles;
    unsigned bits = 0u;
#if CL_LOCAL
    __shared__ unsigned sd[CL_CELLS];
    __shared__ u16 sc[CL_CELLS];
    __shared__ u16 spen[CL_MAX_R * CL_MAX_R + 1];
    for (int c = threadIdx.x; c <= R2; c += CL_THREADS) spen[c] = (u16)cl_pen(pen, c);
    __syncthreads();
    for (int cell = threadIdx.x; cell < CL_CELLS; cell += CL_THREADS) {
        const int lx = cell % CL_HX, ly = (cell / CL_HX) % CL_HY, lz = cell / (CL_HX * CL_HY);
        const int z = z0 + lz - 1, y = y0 + ly - 1, x = x0 + lx - 1;
        unsigned d = CL_UNREACHED;
        unsigned cost = 0u;
        if (z >= 0 && z < N && y >= 0 && y < H && x >= 0 && x < W) {
            const long i = ((long)z * H + y) * W + x;
            const int c = clear[i];
            if (c != 0) {      // (background keeps UNREACHED whatever the memory holds)
                cost = spen[c < R2 ? c : R2];
                d = cl_ld(dist + i);
            }
        }
        sd[cell] = d;
        sc[cell] = (u16)cost;
    }
    __syncthreads();
    volatile unsigned* vd = sd;
    unsigned orig[CL_PER];
#pragma unroll
    for (int k = 0; k < CL_PER; ++k) {
        const int j = threadIdx.x + k * CL_THREADS;
        const int lx = j % CL_TX, ly = (j / CL_TX) % CL_TY, lz = j / (CL_TX * CL_TY);
        orig[k] = sd[((lz + 1) * CL_HY + ly + 1) * CL_HX + lx + 1];
    }
    int more = 0;
    for (int it = 0; it < CL_LOCAL_ITERS; ++it) {
        int changed = 0;
#pragma unroll 1
        for (int k = 0; k < CL_PER; ++k) {
            const int j = threadIdx.x + k * CL_THREADS;
            const int lx = j % CL_TX, ly = (j / CL_TX) % CL_TY, lz = j / (CL_TX * CL_TY);
            const int cell = ((lz + 1) * CL_HY + ly + 1) * CL_HX + lx + 1;
            const unsigned cost = sc[cell];
            if (cost == 0u) continue;
            const unsigned d = vd[cell];
            unsigned best = d;
#pragma unroll
            for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) {
                        if (dz == 0 && dy == 0 && dx == 0) continue;
                        const unsigned nd = vd[cell + (dz * CL_HY + dy) * CL_HX + dx];
                        if (nd == CL_UNREACHED) continue;
                        const unsigned cand = cl_add(nd, (unsigned)st.s[cl_kind(dz, dy, dx)] * cost);
                        best = cand < best ? cand : best;
                    }
            if (best < d) {
                vd[cell] = best;
                changed = 1;
            }
        }
        more = __syncthreads_or(changed);
        if (!more) break;
    }
#pragma unroll
    for (int k = 0; k < CL_PER; ++k) {
        const int j = threadIdx.x + k * CL_THREADS;
        const int lx = j % CL_TX, ly = (j / CL_TX) % CL_TY, lz = j / (CL_TX * CL_TY);
        const unsigned val = sd[((lz + 1) * CL_HY + ly + 1) * CL_HX + lx + 1];
        if (val < orig[k]) {      // (only a voxel inside the volume has a cost, so only such a voxel is ever lowered)
            const long i = ((long)(z0 + lz) * H + (y0 + ly)) * W + (x0 + lx);
            __hip_atomic_fetch_min(dist + i, val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            bits |= cl_mark_bits(lz, ly, lx);
        }
    }
    bits &= ~(1u << 13);
    if (more) bits |= 1u << 13;      // the sweep cap: this tile goes on in the next round
#else
#pragma unroll 1
    for (int k = 0; k < CL_PER; ++k) {
        const int j = threadIdx.x + k * CL_THREADS;
        const int lx = j % CL_TX, ly = (j / CL_TX) % CL_TY, lz = j / (CL_TX * CL_TY);
        const int z = z0 + lz, y = y0 + ly, x = x0 + lx;
        if (z >= N || y >= H || x >= W) continue;
        const long i = ((long)z * H + y) * W + x;
        const int c = clear[i];
        if (c == 0) continue;
        const unsigned cost = cl_pen(pen, c < R2 ? c : R2);
        const unsigned d = cl_ld(dist + i);
        unsigned best = d;
#pragma unroll
        for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    if (dz == 0 && dy == 0 && dx == 0) continue;
                    const int nz = z + dz, ny = y + dy, nx = x + dx;
                    if (nz < 0 || nz >= N || ny < 0 || ny >= H || nx < 0 || nx >= W) continue;
                    const long ni = ((long)nz * H + ny) * W + nx;
                    if (clear[ni] == 0) continue;
                    const unsigned nd = cl_ld(dist + ni);
                    if (nd == CL_UNREACHED) continue;
                    const unsigned cand = cl_add(nd, (unsigned)st.s[cl_kind(dz, dy, dx)] * cost);
                    best = cand < best ? cand : best;
                }
        if (best < d) {
            __hip_atomic_fetch_min(dist + i, best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            bits |= cl_mark_bits(lz, ly, lx);      // the centre included: the voxel's neighbours inside the tile are due next round
        }
    }
#endif
    cl_publish(bits, &smask, tz, ty, tx, tzn, tyn, txn, next, marks + r);
}

__global__ __launch_bounds__(CL_STREAM_THREADS) void cl_saturated_kernel(const unsigned* __restrict__ dist, long V, int* __restrict__ stats) {
    bool sat = false;
    for (long i = (long)blockIdx.x * CL_STREAM_THREADS + threadIdx.x; i < V; i += (long)gridDim.x * CL_STREAM_THREADS)
        sat = sat || dist[i] == CL_SAT;
    if (__ballot(sat) != 0 && (threadIdx.x & 63) == 0) stats[3] = 1;
}

// ---------------------------------------------------------------------------------------------------------------- trace
__global__ void cl_trace_zero_kernel(int* __restrict__ stats) {
    if (threadIdx.x == 1 || threadIdx.x == 2 || threadIdx.x == 4) stats[threadIdx.x] = 0;
}

__global__ __launch_bounds__(64) void cl_trace_kernel(const u16* __restrict__ clear, int N, int H, int W, const u16* __restrict__ pen, int R2,
                                                       ClSteps st, const unsigned* __restrict__ dist, const int* __restrict__ ends,
                                                       int max_points, int* __restrict__ paths, int* __restrict__ counts,
                                                       int* __restrict__ stats) {
    const int e = blockIdx.x, lane = threadIdx.x;
    const long V = (long)N * H * W;
    int* __restrict__ path = paths + (long)e * max_points;
    // the lane's neighbour: lanes 0 .. 25 walk the 27 offsets without the centre
    const int o = lane < 13 ? lane : lane + 1;
    const int dz = o / 9 - 1, dy = (o / 3) % 3 - 1, dx = o % 3 - 1;
    const int k = (dy != 0) + (dx != 0);
    const unsigned len = (unsigned)st.s[dz == 0 ? (k > 0 ? k - 1 : 0) : 2 + k];
    int v = ends[e];      // (the same for the whole wave, as everything below but the lane's neighbour)
    int n = 0, count = 0;
    const bool inside = v >= 0 && v < V;
    int cv = 0;
    unsigned dv = CL_UNREACHED;
    if (inside) {
        cv = clear[v];
        dv = dist[v];
    }
    if (!inside || cv == 0 || dv == CL_UNREACHED) {
        if (lane == 0) atomicAdd(&stats[1], 1);
    } else {
        for (;;) {      // at most max_points rounds
            if (n >= max_points) {
                count = -1;
                if (lane == 0) atomicAdd(&stats[2], 1);
                break;
            }
            if (lane == 0) path[n] = v;
            ++n;
            if (dv == 0u) {
                count = n;
                break;
            }
            const unsigned w = len * cl_pen(pen, cv < R2 ? cv : R2);      // step(u -> v): the length of the move times pen[clear[v]]
            const int x = v % W, y = (v / W) % H, z = v / (W * H);
            const int nz = z + dz, ny = y + dy, nx = x + dx;
            int cand = 0x7fffffff, cu = 0;
            unsigned du = CL_UNREACHED;
            if (lane < 26 && nz >= 0 && nz < N && ny >= 0 && ny < H && nx >= 0 && nx < W) {
                const int u = (int)(((long)nz * H + ny) * W + nx);
                cu = clear[u];
                du = dist[u];
                if (cu != 0 && du != CL_UNREACHED && du < dv && cl_add(du, w) == dv) cand = u;
            }
            int best = cand;
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) best = min(best, __shfl_xor(best, s, 64));
            if (best == 0x7fffffff) {      // nothing explains dist[v]: a saturated or foreign field
                count = -2;
                if (lane == 0) {
                    atomicAdd(&stats[4], 1);
                    stats[6] = 1;
                }
                break;
            }
            // the winner's lane hands over its clearance and distance (a wave-uniform lane index)
            const int src = __ffsll((long long)__ballot(cand == best)) - 1;
            v = best;
            cv = __shfl(cu, src, 64);
            dv = (unsigned)__shfl((int)du, src, 64);      // strictly below the last dv: the walk ends
        }
    }
    for (int i = n + lane; i < max_points; i += 64) path[i] = -1;
    if (lane == 0) counts[e] = count;
}

// ---------------------------------------------------------------------------------------------------------------- entries
static inline unsigned cl_stream_blocks(long items) {
    long b = (items + CL_STREAM_THREADS - 1) / CL_STREAM_THREADS;
    b = b < 1 ? 1 : b;
    return (unsigned)(b < CL_STREAM_BLOCKS ? b : CL_STREAM_BLOCKS);
}

static inline bool cl_sides_ok(int N, int H, int W) {
    if (N < 1 || N > 4096 || H < 1 || H > 4096 || W < 1 || W > 4096) return false;
    return (long)N * H * W <= 2147483647L;
}

static inline bool cl_steps_ok(int s0, int s1, int s2, int s3, int s4) {
    const int s[5] = {s0, s1, s2, s3, s4};
    for (int i = 0; i < 5; ++i)
        if (s[i] < 1 || s[i] > 255) return false;
    return true;
}

static inline long cl_tiles(int N, int H, int W, int* tzn, int* tyn, int* txn) {
    *tzn = (N + CL_TZ - 1) / CL_TZ;
    *tyn = (H + CL_TY - 1) / CL_TY;
    *txn = (W + CL_TX - 1) / CL_TX;
    return (long)*tzn * *tyn * *txn;      // at most 2^31 / 1 voxels in tiles of 4096, times the waste of partial tiles: below 2^24
}

extern "C" int ctg_centreline_clearance(const short* vol, int N, int H, int W, int lo, int hi, int R, int zq, unsigned short* scratch,
                                        unsigned short* clear, void* stream) {
    CTG_ENTER();
    if (vol == nullptr || scratch == nullptr || clear == nullptr || scratch == clear) return CTG_EINVAL;
    if (!cl_sides_ok(N, H, W)) return CTG_EINVAL;
    if (lo > hi || lo < -32768 || hi > 32767 || R < 1 || R > CL_MAX_R || zq < 16 || zq > 65535) return CTG_EINVAL;
    if ((((uintptr_t)vol | (uintptr_t)scratch | (uintptr_t)clear) & 1) != 0) return CTG_EINVAL;
    const long V = (long)N * H * W;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(cl_stream_blocks(V)), block(CL_STREAM_THREADS);
    hipLaunchKernelGGL(cl_clear_x_kernel, grid, block, 0, st, vol, V, W, lo, hi, R, clear);
    hipLaunchKernelGGL(cl_clear_y_kernel, grid, block, 0, st, clear, V, H, W, R, scratch);
    hipLaunchKernelGGL(cl_clear_z_kernel, grid, block, 0, st, scratch, V, N, (long)H * W, zq, clear);
    return ctg_launch_status();
}

extern "C" int ctg_centreline_seed(const unsigned short* clear, int N, int H, int W, long start, unsigned* dist, int* active, int* marks,
                                   int max_rounds, int* stats, void* stream) {
    CTG_ENTER();
    if (clear == nullptr || dist == nullptr || active == nullptr || marks == nullptr || stats == nullptr) return CTG_EINVAL;
    if (!cl_sides_ok(N, H, W) || max_rounds < 1 || max_rounds > CL_MAX_ROUNDS) return CTG_EINVAL;
    if (((uintptr_t)clear & 1) != 0 || (((uintptr_t)dist | (uintptr_t)active | (uintptr_t)marks | (uintptr_t)stats) & 3) != 0) return CTG_EINVAL;
    const long V = (long)N * H * W;
    int tzn, tyn, txn;
    const long tiles = cl_tiles(N, H, W, &tzn, &tyn, &txn);
    long start_tile = -1;
    if (start >= 0 && start < V) {
        const int x = (int)(start % W), y = (int)((start / W) % H), z = (int)(start / ((long)W * H));
        start_tile = ((long)(z / CL_TZ) * tyn + y / CL_TY) * txn + x / CL_TX;      // in active[0]
    }
    hipLaunchKernelGGL(cl_seed_kernel, dim3(cl_stream_blocks(V)), dim3(CL_STREAM_THREADS), 0, (hipStream_t)stream, clear, V, start,
                       start_tile, dist, active, 2 * tiles, marks, max_rounds, stats);
    return ctg_launch_status();
}

extern "C" int ctg_centreline_relax(const unsigned short* clear, int N, int H, int W, const unsigned short* pen, int R, int s0, int s1,
                                    int s2, int s3, int s4, unsigned* dist, int* active, int* marks, int max_rounds, int first_round,
                                    int rounds, int* stats, void* stream) {
    CTG_ENTER();
    if (clear == nullptr || pen == nullptr || dist == nullptr || active == nullptr || marks == nullptr || stats == nullptr) return CTG_EINVAL;
    if (!cl_sides_ok(N, H, W) || R < 1 || R > CL_MAX_R || !cl_steps_ok(s0, s1, s2, s3, s4)) return CTG_EINVAL;
    if (max_rounds < 1 || max_rounds > CL_MAX_ROUNDS || first_round < 0 || rounds < 0 || (long)first_round + rounds > max_rounds) return CTG_EINVAL;
    if ((((uintptr_t)clear | (uintptr_t)pen) & 1) != 0 || (((uintptr_t)dist | (uintptr_t)active | (uintptr_t)marks | (uintptr_t)stats) & 3) != 0)
        return CTG_EINVAL;
    int tzn, tyn, txn;
    const long tiles = cl_tiles(N, H, W, &tzn, &tyn, &txn);
    const ClSteps steps = {{s0, s1, s2, s3, s4}};
    hipStream_t st = (hipStream_t)stream;
    for (int r = first_round; r < first_round + rounds; ++r)
        hipLaunchKernelGGL(cl_relax_kernel, dim3((unsigned)tiles), dim3(CL_THREADS), 0, st, clear, N, H, W, tzn, tyn, txn, pen, R * R, steps,
                           dist, active, tiles, marks, r);
    return ctg_launch_status();
}

extern "C" int ctg_centreline_saturated(const unsigned* dist, long V, int* stats, void* stream) {
    CTG_ENTER();
    if (dist == nullptr || stats == nullptr || V < 1 || V > 2147483647L) return CTG_EINVAL;
    if ((((uintptr_t)dist | (uintptr_t)stats) & 3) != 0) return CTG_EINVAL;
    hipLaunchKernelGGL(cl_saturated_kernel, dim3(cl_stream_blocks(V)), dim3(CL_STREAM_THREADS), 0, (hipStream_t)stream, dist, V, stats);
    return ctg_launch_status();
}

extern "C" int ctg_centreline_trace(const unsigned short* clear, int N, int H, int W, const unsigned short* pen, int R, int s0, int s1,
                                    int s2, int s3, int s4, const unsigned* dist, const int* ends, int E, int max_points, int* paths,
                                    int* counts, int* stats, void* stream) {
    CTG_ENTER();
    if (clear == nullptr || pen == nullptr || dist == nullptr || ends == nullptr || paths == nullptr || counts == nullptr || stats == nullptr)
        return CTG_EINVAL;
    if (!cl_sides_ok(N, H, W) || R < 1 || R > CL_MAX_R || !cl_steps_ok(s0, s1, s2, s3, s4)) return CTG_EINVAL;
    if (E < 1 || E > CL_MAX_ENDS || max_points < 1 || max_points > CL_MAX_POINTS) return CTG_EINVAL;
    if ((((uintptr_t)clear | (uintptr_t)pen) & 1) != 0 ||
        (((uintptr_t)dist | (uintptr_t)ends | (uintptr_t)paths | (uintptr_t)counts | (uintptr_t)stats) & 3) != 0)
        return CTG_EINVAL;
    const ClSteps steps = {{s0, s1, s2, s3, s4}};
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(cl_trace_zero_kernel, dim3(1), dim3(64), 0, st, stats);
    hipLaunchKernelGGL(cl_trace_kernel, dim3((unsigned)E), dim3(64), 0, st, clear, N, H, W, pen, R * R, steps, dist, ends, max_points, paths,
                       counts, stats);
    return ctg_launch_status();
}
