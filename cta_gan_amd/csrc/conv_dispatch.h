// Host-side helpers shared by the conv launchers (conv_igemm.hip, conv_wgrad.hip, conv_halo.h, the conv_strip*.h family): what a
// tap list looks like, how a strip kernel cuts its rows into bands, which tile a small grid gets, and the launch tail of a kernel
// with a dynamic LDS size.  A rule that a launcher and the code sizing a buffer for it must agree on is ONE function here.
#pragma once
#include "common.h"
#include "ctg_knobs.h"

// a tap word: input offset dy | dx << 8 (each biased by 64), weight index << 16
static inline int tap_dy(int tw) { return (tw & 0xff) - 64; }
static inline int tap_dx(int tw) { return ((tw >> 8) & 0xff) - 64; }

// bounding window of a set of tap offsets: kh x kw taps from (dy0, dx0)
struct TapWindow {
    int dymin = 127, dymax = -128, dxmin = 127, dxmax = -128;
    void add(int dy, int dx) {
        dymin = dy < dymin ? dy : dymin; dymax = dy > dymax ? dy : dymax;
        dxmin = dx < dxmin ? dx : dxmin; dxmax = dx > dxmax ? dx : dxmax;
    }
    int kh() const { return dymax - dymin + 1; }
    int kw() const { return dxmax - dxmin + 1; }
    int dy0() const { return dymin; }
    int dx0() const { return dxmin; }
};
static inline TapWindow tap_window(const int* taps, int ntaps) {
    TapWindow w;
    for (int t = 0; t < ntaps; ++t) w.add(tap_dy(taps[t]), tap_dx(taps[t]));
    return w;
}

// the 9 offsets of a 3x3 window in row-major order (dy ascending, dx fastest), or that order flipped (backward-data)
static inline bool taps_3x3(const int* taps, bool flipped) {
    for (int t = 0; t < 9; ++t) {
        const int dy = t / 3 - 1, dx = t % 3 - 1;
        if (tap_dy(taps[t]) != (flipped ? -dy : dy) || tap_dx(taps[t]) != (flipped ? -dx : dx)) return false;
    }
    return true;
}
// The halo kernel's compile-time tap walk (conv_halo.h, walk3x3) serves a FULL 3x3 window whose tap t uses weight slice t and
// sits at window position (t / 3, t % 3) -- 1: row-major, the forward convs -- or at (2 - t / 3, 2 - t % 3) -- 2: that order
// flipped, the backward-data launches.  0: any other tap list (fewer rows, another order, other weight slices): the generic loop.
static inline int taps_3x3_walk(const int* taps, int ntaps, int kh, int kw, int dy0, int dx0) {
    if (ntaps != 9 || kh != 3 || kw != 3) return 0;
    bool fwd = true, flip = true;
    for (int t = 0; t < 9; ++t) {
        if ((taps[t] >> 16) != t) return 0;
        const int ky = tap_dy(taps[t]) - dy0, kx = tap_dx(taps[t]) - dx0;
        fwd = fwd && ky == t / 3 && kx == t % 3;
        flip = flip && ky == 2 - t / 3 && kx == 2 - t % 3;
    }
    return fwd ? 1 : (flip ? 2 : 0);
}
// Conv2d(k=3, s=2, p=1) as ctg_conv_igemm gets it: tap t = (ky, kx) reads input (2 oy + ky - 1, 2 ox + kx - 1) with weight t
static inline bool taps_conv3x3_s2(const int* taps) {
    for (int t = 0; t < 9; ++t)
        if ((taps[t] >> 16) != t) return false;
    return taps_3x3(taps, false);
}
// the four parity classes of ConvTranspose2d(k=3, s=2, p=1, output_padding=1) as ctg_conv_igemm_classes gets them
// (engine._convT_classes(3, 1)): taps per class, class offsets, and (dy, dx, weight) of every tap
static inline bool taps_convT3x3_classes(const int* c_ntaps, const int* c_oy0, const int* c_ox0, const int* c_tap0, const int* taps) {
    static const int want_n[4] = {1, 2, 2, 4}, want_oy[4] = {0, 0, 1, 1}, want_ox[4] = {0, 1, 0, 1};
    static const int want_t[9][3] = {{0, 0, 4}, {0, 1, 3}, {0, 0, 5}, {1, 0, 1}, {0, 0, 7}, {1, 1, 0}, {1, 0, 2}, {0, 1, 6}, {0, 0, 8}};
    int t = 0;
    for (int q = 0; q < 4; ++q) {
        if (c_ntaps[q] != want_n[q] || c_oy0[q] != want_oy[q] || c_ox0[q] != want_ox[q] || c_tap0[q] != t) return false;
        for (int k = 0; k < want_n[q]; ++k, ++t)
            if (tap_dy(taps[t]) != want_t[t][0] || tap_dx(taps[t]) != want_t[t][1] || (taps[t] >> 16) != want_t[t][2]) return false;
    }
    return true;
}

// Band plan of the strip kernels: a workgroup (strip32: a wave) walks `band_rows` rows of one 16-column strip.  As many bands
// per strip as fill the `slots` units the chip holds at once exactly one time (one dispatch round, no tail) over `strips` =
// B x strips per row (x whatever else multiplies the grid), but no band shorter than min_band; band_env >= 8 overrides.
// Never fewer than 8 rows: the callers size the moments buffer for one slab per 8 x 16 pixels (ops.moments_slabs).
struct BandPlan { int band_rows, nbands; };
static inline BandPlan band_plan(int rows, int min_band, long slots, long strips, int band_env) {
    long nb = slots / strips;
    if (nb < 1) nb = 1;
    int band = (int)((rows + nb - 1) / nb);
    if (band < min_band) band = min_band;
    if (band_env >= 8) band = band_env;
    return BandPlan{band, (rows + band - 1) / band};
}

// set the kernel's dynamic LDS limit (once per device), launch, report
template <auto Kernel, typename Args>
static int launch_lds(dim3 grid, dim3 block, int smem, hipStream_t st, const Args& s) {
    static unsigned long long attr_mask = 0;       // per device
    const int rc = ctg_lds_attr_once((const void*)Kernel, smem, &attr_mask);
    if (rc != CTG_OK) return rc;
    hipLaunchKernelGGL(Kernel, grid, block, smem, st, s);
    return ctg_launch_status();
}

// The halo kernel's 8-row tiles (conv_halo.h, launch_halo_t: bf16 in and out, 128-channel tiles).  Small batches (the reference
// ships batchSize 1): 16x16-pixel tiles leave most of the 512 workgroup slots of the chip empty (128^2 x B=1 = 128 workgroups);
// 8x16-pixel tiles double the workgroups at the same bytes per FLOP.  The merged parity-class launch (ncls == 4) has four
// workgroups per spatial tile and no 8-row instantiation: it keeps 16x16.  ctg_conv_igemm checks the caller's nie_tiles against
// this choice, and ops._nie_tiles mirrors it.
static inline bool halo_th8(int Hs, int Ws, int Cout, int B, int ncls) {
    const long wgs = (long)((Hs + 15) / 16) * ((Ws + 15) / 16) * ((Cout + 127) / 128) * B;
    return !ctg_knobs().no_th8 && ncls != 4 && Hs >= 16 && wgs < ctg_knobs().th8_wgs;
}
