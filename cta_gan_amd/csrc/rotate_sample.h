// The sampling helpers the rotating kernels share (csrc/project_rotate.hip, csrc/project_render.hip): one definition, the same
// bits.  project_rotate.hip has the sampling rule they serve.
#pragma once
#include "common.h"

// [lo, hi] := its part with 0 <= b + c t <= lim (exact for tables in range, where nothing wraps; empty: hi < lo)
__device__ __forceinline__ void rot_clip(int b, int c, int lim, int& lo, int& hi) {
    if (c < 0) {      // 0 <= b + c t <= lim  <=>  0 <= (lim - b) + (-c) t <= lim
        b = (int)((unsigned)lim - (unsigned)b);
        c = (int)(0u - (unsigned)c);
    }
    const int room = (int)((unsigned)lim - (unsigned)b);
    if (room < 0 || (c == 0 && b < 0) || c < 0) {      // (c < 0 here: INT_MIN, no table in range has it)
        hi = lo - 1;
        return;
    }
    if (c == 0) return;
    const int first = b >= 0 ? 0 : (int)((0u - (unsigned)b + (unsigned)c - 1u) / (unsigned)c);      // ceil(-b / c)
    const int last = (int)((unsigned)room / (unsigned)c);                                            // floor((lim - b) / c)
    lo = lo > first ? lo : first;
    hi = hi < last ? hi : last;
}

// The value of a bilinear sample from its four pixels and two 8-bit fractions.  |top|, |bot| <= 32768 * 256 = 2^23 and the two
// weights of the second step sum to 256, so |top (256 - fy) + bot fy| <= 2^31 - reached only by four pixels of -32768 - and with
// the rounding half the sum lies in [-2^31 + 32768, 2^31 - 32768]: int32 holds it with nothing to spare.  Formed in unsigned
// arithmetic like the kernels' fixed-point sums and read as int32; the shift is arithmetic.
__device__ __forceinline__ int rot_lerp(int p00, int p01, int p10, int p11, int fx, int fy) {
    const unsigned wx = 256u - (unsigned)fx, wy = 256u - (unsigned)fy;
    const unsigned top = (unsigned)p00 * wx + (unsigned)p01 * (unsigned)fx;
    const unsigned bot = (unsigned)p10 * wx + (unsigned)p11 * (unsigned)fx;
    return (int)(top * wy + bot * (unsigned)fy + 32768u) >> 16;
}

__device__ __forceinline__ int rot_clamp(int v, int last) { return v < 0 ? 0 : (v > last ? last : v); }
