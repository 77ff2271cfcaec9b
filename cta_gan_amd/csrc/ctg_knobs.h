// Every CTG_* environment switch the kernel library reads: this is the only file under csrc/ that calls getenv.  All of them
// are developer A/B switches (scripts/README.md lists them with the Python package's); none changes what a default run
// computes.  The environment is read ONCE per process, at the first launch that asks for a knob: set the variables before
// the library is first used, a later change is not seen.
#pragma once
#include <stdlib.h>

namespace ctg_env {
static inline bool set(const char* name) { return getenv(name) != nullptr; }      // set at all, to whatever value
static inline int num(const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; }
static inline long lnum(const char* name, long dflt) { const char* v = getenv(name); return v ? atol(v) : dflt; }
}  // namespace ctg_env

struct CtgKnobs {
    // ---- which conv kernel serves a shape (conv_igemm.hip, conv_halo.h)
    const bool no_halo = ctg_env::set("CTG_NO_HALO");                 // no halo-resident kernels (forward, backward-data, weight gradient)
    const bool no_class_merge = ctg_env::set("CTG_NO_CLASS_MERGE");   // parity classes one launch each
    const bool no_s2d = ctg_env::set("CTG_NO_S2D");                   // stride-2 convs not as polyphase slices on the halo kernel
    const bool no_nie = ctg_env::set("CTG_NO_NIE");                   // no InstanceNorm in the conv epilogue (answer 2 = not served)
    const int nie_share = ctg_env::num("CTG_NIE_SHARE", 2);           // launches that may wait at once (used when > 0, else 2)
    const bool no_th8 = ctg_env::set("CTG_NO_TH8");                   // no 8-row tiles for small grids of the 128-channel tile
    const long th8_wgs = ctg_env::lnum("CTG_TH8_WGS", 384);           // ... which are used below this many workgroups
    const bool no_th8_64 = ctg_env::set("CTG_NO_TH8_64");             // no 8-row tiles for the 64-channel tile
    const bool no_mc_th8 = ctg_env::set("CTG_NO_MC_TH8");             // ... nor for its merged parity classes (split pair)
    const bool no_big_tile = ctg_env::set("CTG_NO_BIG_TILE");         // gather kernel: no 256x128 tile
    const bool frame_bn128 = ctg_env::set("CTG_FRAME_BN128");         // gather kernel: frame launches keep the 128-wide N tile
    const bool no_small_ring = ctg_env::set("CTG_NO_SMALL_RING");     // gather kernel: no 3-stage ring for launches of few workgroups
    // ---- sliding-window ("strip") kernels: off switch, rows per band (used when >= 8), grid knobs
    const bool no_strip = ctg_env::set("CTG_NO_STRIP");
    const int strip_band = ctg_env::num("CTG_STRIP_BAND", 0);
    const bool no_stript = ctg_env::set("CTG_NO_STRIPT");
    const int stript_band = ctg_env::num("CTG_STRIPT_BAND", 0);
    const int stript_xcd = ctg_env::num("CTG_STRIPT_XCD", 1);         // XCD-contiguous workgroup order (both transposed-conv kernels)
    const bool no_striptp = ctg_env::set("CTG_NO_STRIPTP");
    const int striptp_band = ctg_env::num("CTG_STRIPTP_BAND", 0);
    const int striptp_wgs = ctg_env::num("CTG_STRIPTP_WGS", 1);       // workgroups per CU the band plan counts on
    const bool no_strips2 = ctg_env::set("CTG_NO_STRIPS2");
    const int strips2_band = ctg_env::num("CTG_STRIPS2_BAND", 0);
    const bool no_strips2p = ctg_env::set("CTG_NO_STRIPS2P");
    const int strips2p_band = ctg_env::num("CTG_STRIPS2P_BAND", 0);
    const bool no_strips2w = ctg_env::set("CTG_NO_STRIPS2W");
    const int strips2w_band = ctg_env::num("CTG_STRIPS2W_BAND", 0);
    // ---- weight gradient (conv_wgrad.hip)
    const bool no_wg_1tap = ctg_env::set("CTG_NO_WG_1TAP");           // 1x1 convs not on the halo-resident kernel
    const bool no_wg_s2 = ctg_env::set("CTG_NO_WG_S2");               // stride-2 inputs not as polyphase components
    const bool no_wg_s2m = ctg_env::set("CTG_NO_WG_S2M");             // ... their four components one launch each
    const bool no_wg_phase_split = ctg_env::set("CTG_NO_WG_PHASE_SPLIT");   // split pair: the three sweeps in one workgroup
    const bool wg_noprefetch = ctg_env::set("CTG_WG_NOPREFETCH");
    const bool wg_noxcd = ctg_env::set("CTG_WG_NOXCD");
    const bool wg_no_reuse = ctg_env::set("CTG_WG_NO_REUSE");
    // ---- first-layer convs (conv_small.hip), elementwise kernels (norm_act.hip)
    const int small_wgs = ctg_env::num("CTG_SMALL_WGS", 768);         // persistent workgroups over the whole batch
    const bool no_smallb = ctg_env::set("CTG_NO_SMALLB");             // pix_grid: 16 pixels per lane at every batch size
    // ---- reformats (reformat.hip)
    const int reformat_t1 = ctg_env::num("CTG_REFORMAT_T1", 0);       // T = 1 layout: 1 an 8 x 8 patch per wave, 2 64 columns of one line; else per sampling
};

static inline const CtgKnobs& ctg_knobs() {
    static const CtgKnobs k;
    return k;
}
