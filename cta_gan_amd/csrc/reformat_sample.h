// The volume sampling the kernels on lines in any direction share (csrc/reformat.hip, csrc/render_lines.hip): one definition of
// "counted" and of the nearest / trilinear value, the same bits.  reformat.hip has the rule they serve.
#pragma once
#include "common.h"
#include "rotate_sample.h"

struct RfmVol {
    const short* __restrict__ p;
    int N, H, W;
};

// counted: voxel (X >> 16, Y >> 16, Z >> 16) lies in the volume
__device__ __forceinline__ bool rfm_inside(const RfmVol& v, unsigned X, unsigned Y, unsigned Z) {
    const int xi = (int)X >> 16, yi = (int)Y >> 16, zi = (int)Z >> 16;
    return xi >= 0 && xi < v.W && yi >= 0 && yi < v.H && zi >= 0 && zi < v.N;
}

// The loads of one sample (issued, not used): 1 voxel (nearest) or the 8 around the centre-based position (trilinear).  ok =
// false reads voxel 0.
template <bool LERP> struct RfmSample {
    int p[LERP ? 8 : 1];
    int fx, fy, fz;

    __device__ __forceinline__ void issue(const RfmVol& v, unsigned X, unsigned Y, unsigned Z, bool ok) {
        if constexpr (LERP) {
            const int Xc = (int)(X - 32768u), Yc = (int)(Y - 32768u), Zc = (int)(Z - 32768u);
            fx = (Xc >> 8) & 255;
            fy = (Yc >> 8) & 255;
            fz = (Zc >> 8) & 255;
            const int x0 = Xc >> 16, y0 = Yc >> 16, z0 = Zc >> 16;      // in -32768 .. 32767: + 1 cannot wrap
            const int xa = ok ? rot_clamp(x0, v.W - 1) : 0, xb = ok ? rot_clamp(x0 + 1, v.W - 1) : 0;
            const int ra = ok ? rot_clamp(y0, v.H - 1) * v.W : 0, rb = ok ? rot_clamp(y0 + 1, v.H - 1) * v.W : 0;
            const size_t plane = (size_t)v.H * v.W;
            const short* __restrict__ s0 = v.p + (ok ? (size_t)rot_clamp(z0, v.N - 1) * plane : 0);
            const short* __restrict__ s1 = v.p + (ok ? (size_t)rot_clamp(z0 + 1, v.N - 1) * plane : 0);
            p[0] = s0[ra + xa];
            p[1] = s0[ra + xb];
            p[2] = s0[rb + xa];
            p[3] = s0[rb + xb];
            p[4] = s1[ra + xa];
            p[5] = s1[ra + xb];
            p[6] = s1[rb + xa];
            p[7] = s1[rb + xb];
        } else {
            const int xi = (int)X >> 16, yi = (int)Y >> 16, zi = (int)Z >> 16;
            p[0] = v.p[ok ? ((size_t)zi * v.H + yi) * v.W + xi : 0];
        }
    }

    __device__ __forceinline__ int value() const {
        if constexpr (LERP) {
            const int v0 = rot_lerp(p[0], p[1], p[2], p[3], fx, fy), v1 = rot_lerp(p[4], p[5], p[6], p[7], fx, fy);
            return (int)((unsigned)v0 * (256u - (unsigned)fz) + (unsigned)v1 * (unsigned)fz + 128u) >> 8;
        } else {
            return p[0];
        }
    }
};
