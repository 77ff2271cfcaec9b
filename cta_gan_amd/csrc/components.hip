// Series inference, connected components of the resident volume (cta_gan_amd/infer.py: VolumeComponents, components_volume,
// SeriesTranslator(components=...); ops.components_label / components_select / components_apply).  Despeckle, keep the K largest,
// keep what a seed voxel lies in: the cleanup every projection-type display wants in front of it.  The reference has no counterpart.
// include/ctagan_hip.h has the contract; tests/components_np.py is the numpy restatement, equal bit for bit.
//
// The label of a component is the smallest linear index in it, so the result does not depend on the order in which atomics land.
// A union-find forest lives in `labels`: labels[i] = a voxel of the same component with an index <= i ("parent"), a root points
// at itself, background holds -1.  Parents only ever decrease, which is what every loop below leans on.
//
//   cc_local_kernel<CONN>   a workgroup owns a tile CC_TZ x CC_TY x CC_TX = 4 x 16 x 64 voxels, wave w its slice w, one row of 64
//                           voxels per step, a lane per voxel.  The forest of the tile is built in LDS (16 KB of int32 local
//                           indices plus the 64-bit foreground mask of every row): a lane starts at the head of its own x-run,
//                           read off the __ballot of the foreground bit, then unions with its forward neighbours (the 3 / 9 / 13
//                           of c = 6 / 18 / 26 that precede it in (z, y, x) order, x - 1 already served by the run) inside the tile
//                           by atomicMin on LDS.  A union is left out where the lane's left neighbour makes the same one (both
//                           left voxels foreground: the two runs are already joined through them).  After a barrier every lane walks
//                           to its local root and stores that root's global linear index.  Local (lz, ly, lx) order and global
//                           order are both lexicographic in (z, y, x), so the smallest local index is the smallest global one.
//   cc_merge_kernel<CONN>   the same tile map; every foreground voxel with a forward neighbour in ANOTHER tile (rows lz = 0,
//                           ly = 0, ly = 15, and lanes 0 / 63 of the other rows) unions with it on the global array.  Every read of
//                           `labels` in this kernel is a relaxed agent-scope atomic load and every write an agent-scope atomicMin
//                           (the L2s of the 8 XCDs are not coherent for plain accesses); every decision is taken from an atomic's
//                           returned value, so a stale parent only costs a step.
//   cc_flatten_kernel       labels[i] = the root of i.  A concurrent reader sees the old parent or the root: both are valid chains.
//   cc_sizes_kernel         after the flatten the lanes of a run share a root: a wave folds a run into (root, length), a workgroup
//                           sums those per root in an LDS table and issues one global atomicAdd per root and chunk of 8192 voxels.
//   cc_select_*             seeds mark their roots in `keep`; one sweep counts components and candidates; the order "size descending,
//                           root ascending" is that of the 64-bit key size << 32 | (0xffffffff - root), and pass p finds the
//                           largest key below that of pass p - 1: a workgroup maximum, then one 64-bit atomicMax per workgroup --
//                           exact, whatever the arrival order.  The pass keys are the one piece of state the library keeps itself
//                           (cc_keys below: 66 words per call in flight, CC_SLOTS calls).
//   cc_apply_kernel         streaming, a lane owns 8 voxels, 16-byte accesses where the address allows, `keep` gathered through labels.
//
// Safety: no workgroup ever waits for another -- no flags, no tickets, no cooperative launch; every hand-over is a kernel boundary.
// The only loops that depend on memory are cc_find and cc_union, and both end whatever the memory holds (see there); a value that
// breaks the forest's invariant sets stats[6] and ends the loop.  Labels handed in by the caller (select, apply) are range-checked
// before they index anything.  Integer arithmetic only, but for the window level of window_arith.h.
#include "common.h"
#include "window_arith.h"

#define CC_TZ 4
#define CC_TY 16
#define CC_TX 64
#define CC_THREADS (64 * CC_TZ)      // wave w owns slice w of the tile
#define CC_TILE (CC_TZ * CC_TY * CC_TX)
#ifndef CC_LOCAL        // 0: the A/B build without the LDS phase -- every voxel starts as its own root and the merge kernel unions
#define CC_LOCAL 1      // over every forward neighbour (LAB_NOTES has both timings)
#endif
#define CC_STREAM_THREADS 256
#define CC_STREAM_BLOCKS 4096      // most workgroups of a grid-strided sweep
#define CC_MAX_TOP 64
#define CC_SLOTS 16

typedef short i16x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned long long u64;

// pass keys of ctg_components_select: [slot][0] = all ones, [slot][1 + p] the key of pass p; a call takes the next slot in turn
__device__ u64 cc_keys[CC_SLOTS][CC_MAX_TOP + 2];

// the forest in LDS (plain reads, atomicMin on LDS) and in global memory (relaxed agent-scope atomics only)
struct CcLds {
    int* lab;
    __device__ __forceinline__ int ld(int i) const { return *(volatile int*)(lab + i); }
    __device__ __forceinline__ int amin(int i, int v) const { return atomicMin(lab + i, v); }
};
struct CcGlobal {
    int* lab;
    __device__ __forceinline__ int ld(int i) const { return __hip_atomic_load(lab + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ int amin(int i, int v) const {
        return __hip_atomic_fetch_min(lab + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// The root of x.  Termination: a step goes on only with 0 <= p < x, so x strictly decreases and stays inside [0, x0]: at most x0
// steps, no address outside the array, whatever the memory holds.  p == x is the root; anything else sets *err and ends the walk.
template <typename M> __device__ __forceinline__ int cc_find(const M& m, int x, int* err) {
    for (;;) {
        const int p = m.ld(x);
        if (p == x) return x;
        if (p < 0 || p > x) {
            *err = 1;
            return x;
        }
        x = p;
    }
}

// Join the trees of a and b (both valid indices).  Termination: a round goes on only after an atomicMin on hi = max(a, b) returned
// old with 0 <= old < hi, and continues with (old, lo), lo < hi: the maximum of the pair strictly decreases, so at most max(a, b)
// rounds.  old == hi: hi was a root and now hangs under lo.  old < hi: somebody else moved hi first -- hi now hangs under min(old,
// lo), and the other of the two still has to be joined to it.  Anything else sets *err and ends the loop.
template <typename M> __device__ __forceinline__ void cc_union(const M& m, int a, int b, int* err) {
    for (;;) {
        a = cc_find(m, a, err);
        b = cc_find(m, b, err);
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int old = m.amin(hi, lo);
        if (old == hi) return;
        if (old < 0 || old > hi) {
            *err = 1;
            return;
        }
        a = old;
        b = lo;
    }
}

// does connectivity CONN join voxels that differ by (dz, dy, dx), each in -1 .. 1?
template <int CONN> __device__ __forceinline__ constexpr bool cc_adjacent(int dz, int dy, int dx) {
    const int s = (dz != 0) + (dy != 0) + (dx != 0);
    return s >= 1 && s <= (CONN == 6 ? 1 : (CONN == 18 ? 2 : 3));
}

__global__ void cc_stats_zero_kernel(int* __restrict__ stats) {
    if (threadIdx.x < 8) stats[threadIdx.x] = 0;
}

template <int CONN>
__global__ __launch_bounds__(CC_THREADS) void cc_local_kernel(const short* __restrict__ vol, int N, int H, int W, int lo, int hi,
                                                              int tyn, int txn, int* __restrict__ labels, int* __restrict__ stats) {
    __shared__ int lab[CC_TILE];
    __shared__ u64 rowm[CC_TZ * CC_TY];
    const CcLds m = {lab};
    const int lane = threadIdx.x & 63, lz = threadIdx.x >> 6;
    const int tile = blockIdx.x;
    const int tx = tile % txn, ty = (tile / txn) % tyn, tz = tile / (txn * tyn);
    const int z = tz * CC_TZ + lz, x = tx * CC_TX + lane, y0 = ty * CC_TY;
    int err = 0, nfg = 0;
    for (int ly = 0; ly < CC_TY; ++ly) {
        const int y = y0 + ly;
        const bool inside = z < N && y < H && x < W;
        int v = 0;
        if (inside) v = vol[((long)z * H + y) * W + x];
        const bool fg = inside && v >= lo && v <= hi;
        const u64 mask = __ballot(fg);
        const u64 gaps = ~mask & ((1ull << lane) - 1);      // background lanes left of this one
        const int head = gaps != 0 ? 64 - __clzll((long long)gaps) : 0;
        const int li = (lz * CC_TY + ly) * CC_TX;
        lab[li + lane] = fg ? li + (CC_LOCAL ? head : lane) : -1;
        if (lane == 0) rowm[lz * CC_TY + ly] = mask;
        nfg += __popcll(mask);
    }
    __syncthreads();
#if CC_LOCAL
    for (int ly = 0; ly < CC_TY; ++ly) {
        const int row = lz * CC_TY + ly;
        const u64 mask = rowm[row];
        if (((mask >> lane) & 1) == 0) continue;
        const bool left = lane > 0 && ((mask >> (lane - 1)) & 1);
#pragma unroll
        for (int dz = -1; dz <= 0; ++dz)
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy) {
                if (dz == 0 && dy >= 0) continue;      // forward rows only: the previous slice, or the previous row of this one
                if (!cc_adjacent<CONN>(dz, dy, 0) && !cc_adjacent<CONN>(dz, dy, 1)) continue;
                if (lz + dz < 0 || ly + dy < 0 || ly + dy >= CC_TY) continue;      // another tile: cc_merge_kernel
                const int nrow = row + dz * CC_TY + dy;
                const u64 nm = rowm[nrow];
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    if (!cc_adjacent<CONN>(dz, dy, dx)) continue;
                    const int xx = lane + dx;
                    if (xx < 0 || xx >= CC_TX || ((nm >> xx) & 1) == 0) continue;
                    if (left && xx > 0 && ((nm >> (xx - 1)) & 1)) continue;      // the left neighbour joins the same two runs
                    cc_union(m, row * CC_TX + lane, nrow * CC_TX + xx, &err);
                }
            }
    }
    __syncthreads();
#endif
    for (int ly = 0; ly < CC_TY; ++ly) {
        const int y = y0 + ly;
        if (!(z < N && y < H && x < W)) continue;
        const int li = (lz * CC_TY + ly) * CC_TX + lane;
        int g = -1;
        if (lab[li] >= 0) {
            const int r = cc_find(m, li, &err);      // r in 0 .. li: a foreground voxel of this tile, inside the volume
            const int rz = r / (CC_TY * CC_TX), ry = (r / CC_TX) % CC_TY, rx = r % CC_TX;
            g = (int)(((long)(tz * CC_TZ + rz) * H + (y0 + ry)) * W + (tx * CC_TX + rx));
        }
        labels[((long)z * H + y) * W + x] = g;
    }
    if (lane == 0 && nfg != 0) atomicAdd(&stats[0], nfg);
    if (err) stats[6] = 1;
}

template <int CONN>
__global__ __launch_bounds__(CC_THREADS) void cc_merge_kernel(int N, int H, int W, int tyn, int txn, int* __restrict__ labels,
                                                              int* __restrict__ stats) {
    const CcGlobal m = {labels};
    const int lane = threadIdx.x & 63, lz = threadIdx.x >> 6;
    const int tile = blockIdx.x;
    const int tx = tile % txn, ty = (tile / txn) % tyn, tz = tile / (txn * tyn);
    const int z = tz * CC_TZ + lz, x = tx * CC_TX + lane;
    if (z >= N || x >= W) return;
    int err = 0;
    for (int ly = 0; ly < CC_TY; ++ly) {
        const int y = ty * CC_TY + ly;
        if (y >= H) break;
        // only these voxels have a forward neighbour in another tile
        if (CC_LOCAL && !(lz == 0 || ly == 0 || ly == CC_TY - 1 || lane == 0 || lane == CC_TX - 1)) continue;
        const int i = (int)(((long)z * H + y) * W + x);
        const int l = m.ld(i);
        if (l < 0) continue;
        if (l > i) {
            err = 1;
            continue;
        }
#pragma unroll
        for (int dz = -1; dz <= 0; ++dz)
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    if (!cc_adjacent<CONN>(dz, dy, dx)) continue;
                    if (!(dz < 0 || (dz == 0 && (dy < 0 || (dy == 0 && dx < 0))))) continue;      // forward neighbours only
                    const bool other = lz + dz < 0 || ly + dy < 0 || ly + dy >= CC_TY || lane + dx < 0 || lane + dx >= CC_TX;
                    if (CC_LOCAL && !other) continue;      // joined in LDS already
                    const int nz = z + dz, ny = y + dy, nx = x + dx;
                    if (nz < 0 || ny < 0 || ny >= H || nx < 0 || nx >= W) continue;
                    const int ni = (int)(((long)nz * H + ny) * W + nx);
                    const int nl = m.ld(ni);
                    if (nl < 0) continue;
                    if (nl > ni) {
                        err = 1;
                        continue;
                    }
                    cc_union(m, l, nl, &err);      // from the parents just read: members of the same two trees, closer to the roots
                }
    }
    if (err) stats[6] = 1;
}

__global__ __launch_bounds__(CC_STREAM_THREADS) void cc_flatten_kernel(int* __restrict__ labels, long V, int* __restrict__ stats) {
    const CcGlobal m = {labels};
    int err = 0;
    for (long i = (long)blockIdx.x * CC_STREAM_THREADS + threadIdx.x; i < V; i += (long)gridDim.x * CC_STREAM_THREADS) {
        const int l = m.ld((int)i);
        if (l < 0) continue;
        if (l > i) {
            err = 1;
            continue;
        }
        const int r = cc_find(m, l, &err);
        if (r != l) __hip_atomic_store(labels + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (err) stats[6] = 1;
}

// ---------------------------------------------------------------------------------------------------------------- select
// zero `sizes` and `keep` (dword stores on the aligned body of keep), entries 1 .. 5 of stats and the call's pass keys
__global__ __launch_bounds__(CC_STREAM_THREADS) void cc_select_zero_kernel(int* __restrict__ sizes, unsigned char* __restrict__ keep,
                                                                           long V, int* __restrict__ stats, u64* __restrict__ keys) {
    const long t0 = (long)blockIdx.x * CC_STREAM_THREADS + threadIdx.x, step = (long)gridDim.x * CC_STREAM_THREADS;
    if (t0 >= 1 && t0 <= 5) stats[t0] = 0;
    if (t0 < CC_MAX_TOP + 2) keys[t0] = t0 == 0 ? ~0ull : 0ull;
    for (long i = t0; i < V; i += step) sizes[i] = 0;
    long head = (long)((4 - ((uintptr_t)keep & 3)) & 3);
    head = head < V ? head : V;
    const long words = (V - head) >> 2, tail = head + (words << 2);
    unsigned* __restrict__ body = reinterpret_cast<unsigned*>(keep + head);
    for (long i = t0; i < words; i += step) body[i] = 0u;
    if (t0 < head) keep[t0] = 0;
    if (t0 < V - tail) keep[tail + t0] = 0;
}

// labels as the caller handed them in: -1 .. V - 1, anything else counts as background and sets the flag
__device__ __forceinline__ int cc_checked_label(int l, long V, int* err) {
    if (l < -1 || l >= V) {
        *err = 1;
        return -1;
    }
    return l;
}

// A workgroup counts a chunk of CC_SIZES_CHUNK consecutive voxels at a time.  A wave first folds every run of equal labels on
// consecutive lanes into one (root, length) at the run's head (after the flatten the lanes of an x-run share a root); the heads then
// add into a small hash table in LDS (open addressing, CC_SIZES_PROBES slots tried; a head that finds none adds to global memory
// itself), and after a barrier the table is flushed: one global atomicAdd per distinct root and chunk.  So a component of millions
// of voxels costs one add per chunk it touches, not one per voxel or run -- on the random volume of LAB_NOTES, where runs are one
// voxel long and one component holds 2.4 million voxels, adding per run took 24.9 ms for 67 M voxels.
#define CC_SIZES_CHUNK (CC_STREAM_THREADS * 32)
#define CC_SIZES_SLOTS 2048
#define CC_SIZES_PROBES 4

__global__ __launch_bounds__(CC_STREAM_THREADS) void cc_sizes_kernel(const int* __restrict__ labels, long V, long chunks,
                                                                     int* __restrict__ sizes, int* __restrict__ stats) {
    __shared__ int key[CC_SIZES_SLOTS], cnt[CC_SIZES_SLOTS];
    const int lane = threadIdx.x & 63;
    int err = 0;
    for (int s = threadIdx.x; s < CC_SIZES_SLOTS; s += CC_STREAM_THREADS) {
        key[s] = -1;
        cnt[s] = 0;
    }
    __syncthreads();
    for (long chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {      // (the same trip count for the whole workgroup)
        const long c0 = chunk * CC_SIZES_CHUNK;
        // whole waves: i - lane is the same for the 64 lanes, so the shuffle and the ballot see all of them
        for (int k = 0; k < CC_SIZES_CHUNK / CC_STREAM_THREADS; ++k) {
            const long i = c0 + (long)k * CC_STREAM_THREADS + threadIdx.x;
            const int l = i < V ? cc_checked_label(labels[i], V, &err) : -1;
            const int prev = __shfl_up(l, 1, 64);
            const bool head = lane == 0 || l != prev;
            const u64 heads = __ballot(head);
            const u64 rest = lane < 63 ? heads >> (lane + 1) : 0ull;      // the heads right of this lane
            const int len = rest != 0 ? __ffsll((long long)rest) : 64 - lane;
            if (head && l >= 0) {
                unsigned s = ((unsigned)l * 2654435761u) >> 16;
                bool placed = false;
#pragma unroll
                for (int p = 0; p < CC_SIZES_PROBES && !placed; ++p) {
                    const int slot = (int)((s + p) & (CC_SIZES_SLOTS - 1));
                    const int old = atomicCAS(&key[slot], -1, l);
                    if (old == -1 || old == l) {
                        atomicAdd(&cnt[slot], len);
                        placed = true;
                    }
                }
                if (!placed) atomicAdd(&sizes[l], len);
            }
        }
        __syncthreads();
        for (int s = threadIdx.x; s < CC_SIZES_SLOTS; s += CC_STREAM_THREADS) {
            const int l = key[s];
            if (l >= 0) {      // (a key came through cc_checked_label: inside 0 .. V - 1)
                atomicAdd(&sizes[l], cnt[s]);
                key[s] = -1;
                cnt[s] = 0;
            }
        }
        __syncthreads();
    }
    if (err) stats[6] = 1;
}

// a seed marks its root with 2 in keep; a seed outside the volume or on background is counted
__global__ void cc_select_seeds_kernel(const int* __restrict__ labels, long V, const int* __restrict__ seeds, int S,
                                       unsigned char* __restrict__ keep, int* __restrict__ stats) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const int seed = seeds[s];
    int err = 0, l = -1;
    if (seed >= 0 && seed < V) l = cc_checked_label(labels[seed], V, &err);
    if (l >= 0) keep[l] = 2;
    else atomicAdd(&stats[5], 1);
    if (err) stats[6] = 1;
}

__device__ __forceinline__ int cc_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// every root: count it, decide whether it is a candidate, and write its keep: 0 no candidate, 1 kept (largest == 0: every candidate),
// 2 candidate still to be ranked (largest > 0)
__global__ __launch_bounds__(CC_STREAM_THREADS) void cc_select_count_kernel(const int* __restrict__ sizes, long V, int min_voxels, int S,
                                                                            int largest, unsigned char* __restrict__ keep,
                                                                            int* __restrict__ stats) {
    int comp = 0, cand = 0, vox = 0;
    for (long r = (long)blockIdx.x * CC_STREAM_THREADS + threadIdx.x; r < V; r += (long)gridDim.x * CC_STREAM_THREADS) {
        const int s = sizes[r];
        if (s <= 0) continue;
        ++comp;
        const bool c = s >= min_voxels && (S == 0 || keep[r] == 2);
        keep[r] = c ? (largest == 0 ? 1 : 2) : 0;
        if (c) {
            ++cand;
            vox += s;      // the sizes of distinct components: the total stays below V
        }
    }
    comp = cc_wave_sum(comp);
    cand = cc_wave_sum(cand);
    vox = cc_wave_sum(vox);
    if ((threadIdx.x & 63) == 0) {
        if (comp) atomicAdd(&stats[1], comp);
        if (cand) atomicAdd(&stats[2], cand);
        if (largest == 0 && cand) {
            atomicAdd(&stats[3], cand);
            atomicAdd(&stats[4], vox);
        }
    }
}

// pass p: keys[1 + p] = the largest key of a candidate below keys[p] (keys[0] = all ones); 0 when none is left
__global__ __launch_bounds__(CC_STREAM_THREADS) void cc_select_pass_kernel(const int* __restrict__ sizes, long V,
                                                                           const unsigned char* __restrict__ keep, u64* __restrict__ keys,
                                                                           int p) {
    __shared__ u64 part[CC_STREAM_THREADS / 64];
    const u64 below = keys[p];
    if (below == 0) return;      // the pass before found nothing: nothing is left (the same for every workgroup)
    u64 best = 0;
    for (long r = (long)blockIdx.x * CC_STREAM_THREADS + threadIdx.x; r < V; r += (long)gridDim.x * CC_STREAM_THREADS) {
        const int s = sizes[r];
        if (s <= 0 || keep[r] == 0) continue;
        const u64 key = ((u64)(unsigned)s << 32) | (u64)(0xffffffffu - (unsigned)r);
        if (key < below && key > best) best = key;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u64 other = ((u64)(unsigned)__shfl_xor((int)(best >> 32), o, 64) << 32) | (unsigned)__shfl_xor((int)(unsigned)best, o, 64);
        best = other > best ? other : best;
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < CC_STREAM_THREADS / 64; ++w) best = part[w] > best ? part[w] : best;
        if (best != 0) atomicMax(&keys[1 + p], best);
    }
}

// one thread: the ranked roots into keep (largest > 0) and top, the kept counts of a ranked selection into stats
__global__ void cc_select_finish_kernel(const u64* __restrict__ keys, long V, int passes, int largest, int ntop,
                                        unsigned char* __restrict__ keep, int* __restrict__ top, int* __restrict__ stats) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int kept = 0, vox = 0;
    for (int p = 0; p < (passes > ntop ? passes : ntop); ++p) {
        const u64 key = p < passes ? keys[1 + p] : 0ull;
        const long root = (long)(0xffffffffu - (unsigned)key);
        const int size = (int)(key >> 32);
        const bool got = key != 0 && root < V;
        if (got && largest > 0) {
            keep[root] = 1;
            ++kept;
            vox += size;
        }
        if (p < ntop) {
            top[2 * p] = got ? (int)root : -1;
            top[2 * p + 1] = got ? size : 0;
        }
    }
    if (largest > 0) {
        stats[3] = kept;
        stats[4] = vox;
    }
}

// largest > 0: the candidates that were not ranked among the first `largest` lose their mark
__global__ __launch_bounds__(CC_STREAM_THREADS) void cc_select_clear_kernel(const int* __restrict__ sizes, long V,
                                                                            unsigned char* __restrict__ keep) {
    for (long r = (long)blockIdx.x * CC_STREAM_THREADS + threadIdx.x; r < V; r += (long)gridDim.x * CC_STREAM_THREADS)
        if (sizes[r] > 0 && keep[r] == 2) keep[r] = 0;
}

// ---------------------------------------------------------------------------------------------------------------- apply
// lane g owns voxels 8 g - shift .. 8 g - shift + 7 (those inside 0 .. V - 1), shift = the voxels by which vol misses 16-byte
// alignment: the body's loads of vol are aligned for any base pointer; the other arrays take the vector path where their own
// address allows and 2- / 4- / 1-byte accesses where not, with the same lane -> voxel map
__global__ __launch_bounds__(CC_STREAM_THREADS) void cc_apply_kernel(const short* __restrict__ vol, const int* __restrict__ labels,
                                                                     const unsigned char* __restrict__ keep, long V, int shift,
                                                                     long groups, int background, int fill, int add, float wc, float ww,
                                                                     short* __restrict__ out, unsigned char* __restrict__ level) {
    WinParams win = {0.f, 0.f};
    if (level != nullptr) win = win_params(wc, ww);
    for (long g = (long)blockIdx.x * CC_STREAM_THREADS + threadIdx.x; g < groups; g += (long)gridDim.x * CC_STREAM_THREADS) {
        const long i0 = g * 8 - shift;
        const int j0 = i0 < 0 ? (int)-i0 : 0, j1 = V - i0 >= 8 ? 8 : (int)(V - i0);      // the lane's voxels: j0 <= j < j1
        const bool full = j0 == 0 && j1 == 8;
        int v[8], l[8];
        if (full) {      // (vol + i0 is 16-byte aligned by the choice of shift)
            const i16x8 t = *reinterpret_cast<const i16x8*>(vol + i0);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = t[j];
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (j >= j0 && j < j1) ? vol[i0 + j] : 0;
        }
        if (full && ((uintptr_t)(labels + i0) & 15) == 0) {
            const i32x4 a = *reinterpret_cast<const i32x4*>(labels + i0), b = *reinterpret_cast<const i32x4*>(labels + i0 + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                l[j] = a[j];
                l[4 + j] = b[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) l[j] = (j >= j0 && j < j1) ? labels[i0 + j] : -1;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const bool fg = l[j] >= 0 && l[j] < V;      // (a label outside the volume reads as background: no gather through it)
            const bool kept = fg && keep[l[j]] == 1;
            v[j] = (fg ? kept : background != 0) ? v[j] : fill;
        }
        if (out != nullptr) {
            if (full && ((uintptr_t)(out + i0) & 15) == 0) {
                i16x8 o;
#pragma unroll
                for (int j = 0; j < 8; ++j) o[j] = (short)v[j];
                *reinterpret_cast<i16x8*>(out + i0) = o;
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (j >= j0 && j < j1) out[i0 + j] = (short)v[j];
            }
        }
        if (level != nullptr) {
            unsigned q[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) q[j] = (unsigned)(int)stored_level((float)(v[j] + add), win);
            if (full && ((uintptr_t)(level + i0) & 7) == 0) {
                *reinterpret_cast<u32x2*>(level + i0) = u32x2{q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24),
                                                              q[4] | (q[5] << 8) | (q[6] << 16) | (q[7] << 24)};
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (j >= j0 && j < j1) level[i0 + j] = (unsigned char)q[j];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- entries
static inline unsigned cc_stream_blocks(long items) {
    long b = (items + CC_STREAM_THREADS - 1) / CC_STREAM_THREADS;
    b = b < 1 ? 1 : b;
    return (unsigned)(b < CC_STREAM_BLOCKS ? b : CC_STREAM_BLOCKS);
}

static inline bool cc_volume_ok(long V) { return V >= 1 && V <= 2147483647L; }

template <int CONN>
static void cc_label_launch(const short* vol, int N, int H, int W, int lo, int hi, int* labels, int* stats, hipStream_t st) {
    const int tzn = (N + CC_TZ - 1) / CC_TZ, tyn = (H + CC_TY - 1) / CC_TY, txn = (W + CC_TX - 1) / CC_TX;
    const unsigned tiles = (unsigned)((long)tzn * tyn * txn);      // at most 1024 * 256 * 64 = 2^24
    hipLaunchKernelGGL(cc_local_kernel<CONN>, dim3(tiles), dim3(CC_THREADS), 0, st, vol, N, H, W, lo, hi, tyn, txn, labels, stats);
    hipLaunchKernelGGL(cc_merge_kernel<CONN>, dim3(tiles), dim3(CC_THREADS), 0, st, N, H, W, tyn, txn, labels, stats);
}

extern "C" int ctg_components_label(const short* vol, int N, int H, int W, int lo, int hi, int connectivity, int* labels, int* stats,
                                    void* stream) {
    CTG_ENTER();
    if (vol == nullptr || labels == nullptr || stats == nullptr) return CTG_EINVAL;
    if (N < 1 || N > 4096 || H < 1 || H > 4096 || W < 1 || W > 4096) return CTG_EINVAL;
    const long V = (long)N * H * W;
    if (!cc_volume_ok(V)) return CTG_EINVAL;
    if (lo > hi || lo < -32768 || hi > 32767) return CTG_EINVAL;
    if (connectivity != 6 && connectivity != 18 && connectivity != 26) return CTG_EINVAL;
    if (((uintptr_t)vol & 1) != 0 || (((uintptr_t)labels | (uintptr_t)stats) & 3) != 0) return CTG_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(cc_stats_zero_kernel, dim3(1), dim3(64), 0, st, stats);
    if (connectivity == 6) cc_label_launch<6>(vol, N, H, W, lo, hi, labels, stats, st);
    else if (connectivity == 18) cc_label_launch<18>(vol, N, H, W, lo, hi, labels, stats, st);
    else cc_label_launch<26>(vol, N, H, W, lo, hi, labels, stats, st);
    hipLaunchKernelGGL(cc_flatten_kernel, dim3(cc_stream_blocks(V)), dim3(CC_STREAM_THREADS), 0, st, labels, V, stats);
    return ctg_launch_status();
}

extern "C" int ctg_components_select(const int* labels, long V, int min_voxels, const int* seeds, int S, int largest, int ntop,
                                     int* sizes, unsigned char* keep, int* top, int* stats, void* stream) {
    CTG_ENTER();
    if (labels == nullptr || sizes == nullptr || keep == nullptr || stats == nullptr) return CTG_EINVAL;
    if (!cc_volume_ok(V) || min_voxels < 1 || S < 0 || (S > 0 && seeds == nullptr)) return CTG_EINVAL;
    if (largest < 0 || largest > CC_MAX_TOP || ntop < 0 || ntop > CC_MAX_TOP || (ntop > 0 && top == nullptr)) return CTG_EINVAL;
    if ((((uintptr_t)labels | (uintptr_t)sizes | (uintptr_t)stats | (uintptr_t)seeds | (uintptr_t)top) & 3) != 0) return CTG_EINVAL;
    static unsigned turn = 0;
    u64* keys = nullptr;
    if (hipGetSymbolAddress((void**)&keys, HIP_SYMBOL(cc_keys)) != hipSuccess || keys == nullptr) return ctg_launch_status();
    keys += (size_t)(__atomic_fetch_add(&turn, 1u, __ATOMIC_RELAXED) % CC_SLOTS) * (CC_MAX_TOP + 2);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(cc_stream_blocks(V)), block(CC_STREAM_THREADS);
    hipLaunchKernelGGL(cc_select_zero_kernel, grid, block, 0, st, sizes, keep, V, stats, keys);
    const long chunks = (V + CC_SIZES_CHUNK - 1) / CC_SIZES_CHUNK;
    hipLaunchKernelGGL(cc_sizes_kernel, dim3((unsigned)(chunks < 2 * CC_STREAM_BLOCKS ? chunks : 2 * CC_STREAM_BLOCKS)), block, 0, st, labels,
                       V, chunks, sizes, stats);
    if (S > 0) hipLaunchKernelGGL(cc_select_seeds_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, labels, V, seeds, S, keep, stats);
    hipLaunchKernelGGL(cc_select_count_kernel, grid, block, 0, st, sizes, V, min_voxels, S, largest, keep, stats);
    const int passes = largest > 0 ? largest : ntop;      // a ranked selection ends at `largest`; otherwise only `top` needs the order
    for (int p = 0; p < passes; ++p) hipLaunchKernelGGL(cc_select_pass_kernel, grid, block, 0, st, sizes, V, keep, keys, p);
    if (passes > 0 || ntop > 0) hipLaunchKernelGGL(cc_select_finish_kernel, dim3(1), dim3(64), 0, st, keys, V, passes, largest, ntop, keep, top, stats);
    if (largest > 0) hipLaunchKernelGGL(cc_select_clear_kernel, grid, block, 0, st, sizes, V, keep);
    return ctg_launch_status();
}

extern "C" int ctg_components_apply(const short* vol, const int* labels, const unsigned char* keep, long V, int background, int fill,
                                    float wc, float ww, int hu, short* out, unsigned char* level, void* stream) {
    CTG_ENTER();
    if (vol == nullptr || labels == nullptr || keep == nullptr || (out == nullptr && level == nullptr)) return CTG_EINVAL;
    if (!cc_volume_ok(V) || background < 0 || background > 1 || fill < -32768 || fill > 32767) return CTG_EINVAL;
    if ((((uintptr_t)vol | (uintptr_t)out) & 1) != 0 || ((uintptr_t)labels & 3) != 0) return CTG_EINVAL;
    const int shift = (int)(((uintptr_t)vol & 15) >> 1);
    const long groups = (V + shift + 7) / 8;
    hipLaunchKernelGGL(cc_apply_kernel, dim3(cc_stream_blocks(groups)), dim3(CC_STREAM_THREADS), 0, (hipStream_t)stream, vol, labels, keep,
                       V, shift, groups, background, fill, hu ? 1024 : 0, wc, ww, out, level);
    return ctg_launch_status();
}
