/*
 * ctagan_hip.h -- C ABI of libctagan_hip.so, the gfx950 (MI355X) kernel library
 * behind the CTA-GAN G+D training-step hot path.
 *
 * The reference (yml-bit/CTA-GAN) has no native interface of its own: its hot
 * path is a chain of stock torch.nn layers (Model/HdGan.py, Model/CycleGan.py,
 * trainer/layers.py, trainer/reg.py, trainer/transformer.py) dispatched to
 * ATen/cuDNN.  Each entry point below names the reference call site(s) whose
 * ATen dispatch it replaces.  The Python binding a maintainer adds is the
 * ctypes table in cta_gan_amd/_lib.py.
 *
 * Conventions
 *   - plain device pointers, ints and a hipStream_t passed as void*; the library
 *     never allocates, frees or synchronises: buffers and workspaces are borrowed
 *     for the duration of the call, kernels are enqueued on `stream`.
 *   - return value: 0 ok, 1 invalid argument (CTG_EINVAL), 1000 + hipError_t.
 *   - activations are NHWC: [B][H][W][ld], `ld` >= C is the per-pixel pitch in
 *     ELEMENTS (a channel slice of a wider buffer needs no copy).
 *   - dtype: 0 = fp32, 1 = bf16 (storage type of activations / packed weights;
 *     accumulation, statistics and parameters are always fp32), 2 = split pair
 *     (the "bf16x3" mode's storage, accepted by the entry points that say so): a
 *     value x is two bf16 planes of its pixel row, hi = bf16(x) at p[c] and
 *     lo = bf16(x - hi) at p[c + ld / 2]; pointers and `ld` are in bf16 ELEMENTS,
 *     ld % 16 == 0, a dense tensor of C channels has ld = 2 C; 4 bytes per value
 *     like fp32, x = hi + lo to 2^-17, and both planes are ordinary bf16 NHWC
 *     tensors the MFMA kernels load without a conversion pass.  3 (ABI 11; ctg_in_bwd,
 *     ctg_in_bwd_partial, ctg_in_bwd_apply, ctg_in_bwd_stats, ctg_maxpool2_bwd only) = mixed:
 *     the SAVED FORWARD activation `x` is a split pair, every other operand plain bf16 --
 *     the plain bf16 backward of a split-pair forward ("bf16x3f") takes activation masks,
 *     the max-pool argmax and the InstanceNorm backward's xhat from hi + lo.
 *   - act: 0 none, 1 ReLU, 2 LeakyReLU(0.2), 3 tanh, 4 sigmoid.  pad_mode: 0 zero, 1 reflect.
 *   - taps: ntaps ints, each (dy + 64) | (dx + 64) << 8 | weight_slice << 16.
 */
#ifndef CTAGAN_HIP_H
#define CTAGAN_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever the signature or the meaning of an existing entry point changes: a binding compares it with the value it
 * was written against before it makes any other call (cta_gan_amd/_lib.py does), so a stale library is an error, not a
 * mis-typed call. */
#define CTG_ABI_VERSION 15
int ctg_abi_version(void);

/* ---- convolution: forward / backward-data / transposed, as one gather-GEMM ----
 * Y[n, j*os+oy0, i*os+ox0, co] = act(bias[co] + sum_t sum_ci X[n, pad(j*is+dy_t), pad(i*is+dx_t), ci] * W[t][co][ci])
 * for (j, i) in Hs x Ws (frame != 0: only the 1-pixel frame of that grid -- the ring of a padded-grid backward-data
 * pass whose interior is a second, tile-aligned call; stats_part must be NULL with it).  W is packed [slices][w_npad][Cin] (ctg_weight_pack).  out_f32 != 0 stores fp32
 * output (only for Cout <= 16).  Cin % 16 (fp32) / % 32 (bf16) == 0.
 * stats_part / stats_slabs_out (both may be NULL): when the call is served by the halo-resident kernel and has no
 * bias / activation, per-(sample, spatial tile, channel) partial (sum, sum of squares) of the results are written
 * to stats_part[B][slabs][Cout][2] and *stats_slabs_out = slabs (<= ceil(Hs/8)*ceil(Ws/16), the caller sizes the
 * buffer for that bound and reads it with the returned slab count); otherwise *stats_slabs_out = 0 and the caller runs ctg_in_stats.
 * epi->res / epi->fold (both may be NULL; unit-stride launches covering the whole output: os == is == 1, oy0 == ox0 == 0, Ho == Hs,
 * Wo == Ws, dtype-typed, served by the halo-resident kernel only -- CTG_EINVAL otherwise): res[B][Hs][Ws][res_ld] is added
 * to the rounded result (the skip gradient of a residual block, Model/HdGan.py:62); fold[B][Hs+2][Ws+2][fold_ld] is a
 * gradient on the 1-pixel reflection-padded grid of which only the frame is read and added to the interior pixels it
 * mirrors, so the backward-data pass of ReflectionPad2d(1) + Conv2d emits the unpadded gradient directly.
 * epi->bstats (bf16 launches with res / fold only): the emitted gradient g belongs to out = act(InstanceNorm(z)) [+ skip]
 * (Model/HdGan.py:54-59); the two sums of that InstanceNorm's backward are accumulated per (sample, tile, channel) while
 * g is stored -- ctg_in_bwd_stats then replaces ctg_in_bwd's own statistics pass; *stats_slabs_out returns the tile count.
 * dtype 2 (split pair, "bf16x3"): x is a split-pair tensor of Cin channels (Cin % 32 == 0), W the packed weights split along K
 * by ctg_split_weights -- 2 Cin bf16 per row, [w_hi 32 | w_lo 32] per 32 channels --, and each K step contracts
 * x_hi.w_hi + x_hi.w_lo + x_lo.w_hi on the bf16 matrix cores from ONE halo tile [hi 32 | lo 32] and one weight tile:
 * nn.Conv2d's fp32 product to ~1e-5 relative at a third of the bf16 MFMA rate.  out_f32 == 0: split-pair result (y_ld its
 * pitch; Cout % 8 == 0; epi->res / fold / bz split pairs too, and epi->bstats is served), 1: fp32 result.
 * Replaces: nn.Conv2d / nn.ConvTranspose2d (+ nn.ReflectionPad2d, bias, LeakyReLU / Tanh) forward and the
 * input-gradient half of their backward -- Model/HdGan.py:53-59,69-72,78-80,93-95,100-102,120-136,156-175;
 * Model/CycleGan.py:10-16,27-60,78-94; trainer/layers.py:85,97-104,282,295.                                  */
/* optional fused epilogue of ctg_conv_igemm (NULL = none); plain data, every member may be NULL / 0 */
typedef struct ctg_conv_epilogue {
    const void* res;      /* [B][Hs][Ws][res_ld] added to the result                                            */
    const void* fold;     /* [B][Hs+2][Ws+2][fold_ld] padded-grid gradient whose frame is folded into the result */
    const void* bz;       /* [B][Hs][Ws][bz_ld] input z of the InstanceNorm whose OUTPUT's gradient this launch emits */
    const float* bmean;   /* [B][Cout] mean / rstd of that InstanceNorm                                          */
    const float* brstd;
    float* bstats;        /* out: [B][tiles][Cout][2] partial (sum g m, sum g m xhat), tiles = the stats_slabs_out count */
    int res_ld, fold_ld, bz_ld;
    int bact;             /* activation fused behind that InstanceNorm: 0 none, 1 ReLU, 2 LeakyReLU(0.2)           */
    /* InstanceNorm of THIS launch's result in its epilogue: y = nie_act(IN(conv(x))) [+ res]; the conv result itself is never
     * stored (forward passes that keep nothing for a backward: Model/HdGan.py:53-63 under torch.no_grad(), HdTrainer.py:742-743).
     * nie_sync: 1 + nie_groups 64-bit words (nie_groups >= B * ceil(Cout / 128), else CTG_EINVAL), zeroed ONCE by the caller and then
     * owned by the library (monotonic arrival counters); one buffer per stream AND per nie_tiles = the group size the counters count
     * in: ceil(Hs / 16) * ceil(Ws / 16), or ceil(Hs / 8) * ceil(Ws / 16) for dtype 1 launches of fewer than 384 such tiles x
     * ceil(Cout / 128) x B (the 8-row tile variant; a mismatch is CTG_EINVAL).
     * Needs stats_part / stats_slabs_out; served for 3x3 unit-stride windows, Cout % 128 == 0, dtype 1 / 2 -- otherwise the call
     * returns 2 with nothing launched.
     *
     * What the in-launch exchange ASSUMES, and what happens when an assumption breaks:
     *  (1) Dispatch order.  The workgroups of a grid are placed in blockIdx order (x fastest, then y = the sample), and a placed
     *      workgroup keeps its slot until it ends.  A workgroup that waits for its sample's statistics therefore only waits for
     *      workgroups that were placed BEFORE any workgroup of a later sample -- provided every workgroup of ONE sample can be
     *      resident at once.  Inside a sample the ceil(Cout / 128) statistics groups are interleaved in dispatch order (the
     *      channel tile is the fastest tile index and the XCD-contiguous tile map deals the ids over eight runs), so the set that
     *      must fit is nie_tiles * ceil(Cout / 128) workgroups, not nie_tiles.
     *  (2) Residency.  That set must not exceed the chip's workgroup slots for this kernel (occupancy x compute units, queried
     *      per device) divided by the number of such launches that may wait at the same time -- streams of one process, or
     *      processes sharing the card: CTG_NIE_SHARE, default 2 (the reference-side callers issue these launches from one stream).  A launch that fails the test returns 2 (nothing launched; the
     *      caller runs the unfused conv + ctg_in_finalize + ctg_in_apply).  Kernels that never wait (everything else in this
     *      library) always drain, so they can delay a group but not starve it.
     *  (3) Memory ordering.  Tile moments and arrival counters are exchanged with relaxed AGENT-scope atomic accesses only
     *      (write-through stores, L2-bypassing loads); a workgroup waits for the acknowledgement of its moment stores
     *      (s_waitcnt vmcnt(0) + workgroup barrier) BEFORE its arrival increment, which is what orders "moments visible" before
     *      "arrival counted".  No release / acquire fence is used: on this multi-L2 part an agent-scope fence writes back and
     *      invalidates the whole L2 of the XCD (measured 4x on the launch).  The moments buffer (stats_part) must not be read by
     *      the caller as if it were coherent with its own cached loads -- ctg_in_finalize is not needed after such a launch.
     *  (4) Failure.  The wait is bounded: nie_budget polls of ~0.3 us (0 = the default 2^22, about a second).  A workgroup whose
     *      wait runs out stores NaN results for its tile and sets nie_sync[0] = 1.  The flag is sticky until the caller zeroes it;
     *      a caller MUST read it wherever it synchronises with the device anyway and treat a non-zero value as an error (the
     *      Python trainers raise and stop fusing for the rest of the process: cta_gan_amd/ops.py nie_check). */
    void* nie_sync;
    int nie_act;
    int nie_tiles;
    int nie_groups;       /* counter words behind nie_sync[0]                                                       */
    int nie_budget;       /* polls before a waiting workgroup gives up; 0 = default                                 */
} ctg_conv_epilogue;

int ctg_conv_igemm(int dtype, int out_f32, const void* x, const void* w, void* y, const float* bias,
                   int B, int Hi, int Wi, int Cin, int x_ld, int Ho, int Wo, int Cout, int y_ld,
                   int Hs, int Ws, int oy0, int ox0, int os, int is, int frame, int pad_mode, int act,
                   int w_npad, int ntaps, const int* taps_host, float* stats_part, int* stats_slabs_out,
                   const ctg_conv_epilogue* epi, void* stream);
/* The four parity classes of a stride-2 transposed conv (nn.ConvTranspose2d(k=3, s=2, p=1, output_padding=1), Model/HdGan.py:93-95)
 * or of the backward-data pass of a stride-2 conv (Model/HdGan.py:78-80, 124-131) in ONE launch: class q writes
 * out[2 j + cls_oy0[q], 2 i + cls_ox0[q]] = sum over its cls_ntaps[q] taps (taps = the classes' tap words back to back, encoded as
 * for ctg_conv_igemm), j < Hs, i < Ws.  The four workgroups of a spatial tile run back to back on one XCD and share the input
 * halo through L2.  bf16 in and out.  Returns 0, 1, 1000+hipError_t, or 2 = shape not served here (launch the classes one by one
 * with ctg_conv_igemm).  stats_part (optional, no bias / activation): B * 4 * ceil(Hs/8) * ceil(Ws/16) * Cout * 2 floats of
 * InstanceNorm partial moments, *stats_slabs_out = partials per sample. */
int ctg_conv_igemm_classes(int dtype, const void* x, const void* w, void* y, const float* bias, int B, int Hi, int Wi,
                           int Cin, int x_ld, int Ho, int Wo, int Cout, int y_ld, int Hs, int Ws, int pad_mode, int act,
                           int w_npad, const int* cls_ntaps, const int* cls_oy0, const int* cls_ox0, const int* taps,
                           float* stats_part, int* stats_slabs_out, void* stream);

/* ---- convolution weight gradient (split over pixel slabs, deterministic reduce) ----
 * part[z][t][m][c] = sum over slab z of G[n, j, i, m] * X[n, pad(j*is+dy_t), pad(i*is+dx_t), c];
 * part holds B*ceil(Hs*Ws/slab)*ntaps*Mc*Nc floats.  Mc, Nc % 32 == 0.
 * dtype 2 (split pairs, "bf16x3"): G_hi X_hi + G_hi X_lo + G_lo X_hi as three sweeps of every pixel tile into the same
 * accumulators (one partial, one launch: return 0) or, on small grids, in three workgroups writing three partials (return 3);
 * returns 2 when the shape is not served that way (the caller then makes three bf16 calls on the hi / lo plane views).  `part`
 * is sized three times as large in this mode.
 * Replaces: the weight-gradient half of convolution_backward for the same call sites.                      */
int ctg_conv_wgrad(int dtype, const void* g, const void* x, float* part, int B, int Hs, int Ws, int Mc, int g_ld,
                   int Hi, int Wi, int Nc, int x_ld, int is, int pad_mode, int slab, int ntaps,
                   const int* taps_host, void* stream);
/* dst[m*sm + c*sn + t*stp] (+)= sum_z part[z][t][m][c] for m < Mreal, c < Nreal */
int ctg_wgrad_reduce(const float* part, int Z, int ntaps, int Mc, int Nc, float* dst, int Mreal, int Nreal,
                     long sm, long sn, long stp, int accumulate, void* stream);
/* the same for `count` reductions given as parallel host arrays: every weight gradient of a network's backward */
int ctg_wgrad_reduce_multi(int count, const void* const* part, void* const* dst, const int* Z, const int* ntaps,
                           const int* Mc, const int* Nc, const int* Mreal, const int* Nreal, const long* sm,
                           const long* sn, const long* stp, const int* accumulate, void* stream);

/* ---- InstanceNorm2d(affine=False, eps=1e-5) fused with its neighbours ----
 * Replaces: nn.InstanceNorm2d + nn.ReLU / nn.LeakyReLU(0.2) + the residual add, forward and backward --
 * Model/HdGan.py:55-56,59,63,71-72,79-80,94-95,124-125,128-129,132-133,164,171-172; trainer/layers.py:14,282,295,299.
 * `part` = B*nslabs*C*2 floats scratch (nslabs <= 128); mean/rstd/s1/s2 = B*C floats.
 * pad > 0: `dout` lives on the reflection-padded grid (H+2pad, W+2pad) and is folded on load.                */
/* mean == NULL: only the partial moments part[B][nslabs][C][2] are produced (ctg_in_apply_part finalizes them) */
int ctg_in_stats(int dtype, const void* x, int x_ld, int B, int H, int W, int C, int nslabs, float* part,
                 float* mean, float* rstd, void* stream);
/* mode 0: mean / rstd from partial moments [B][nslabs][C][2] (any nslabs), e.g. those of ctg_conv_igemm; mode 1: the two plain
 * means (sum / HW) of the InstanceNorm backward from its partial sums */
int ctg_in_finalize(const float* part, int B, int C, int nslabs, int HW, int mode, float* mean, float* rstd, void* stream);
int ctg_in_apply(int dtype, const void* x, int x_ld, const float* mean, const float* rstd, int act,
                 const void* res, int r_ld, void* out, int o_ld, int B, int H, int W, int C, void* stream);
/* ctg_in_finalize + ctg_in_apply in one launch: (mean, rstd) come from the partial moments part[B][nslabs][C][2]
 * (nslabs <= 128; ctg_conv_igemm's stats_part or ctg_in_stats') in the kernel's prologue -- each workgroup owns one sample, one
 * group of 64 (bf16) / 32 (fp32) channels and a strip of pixels -- and are also written to mean / rstd [B][C] for the backward. */
int ctg_in_apply_part(int dtype, const void* x, int x_ld, const float* part, int nslabs, float* mean, float* rstd, int act,
                      const void* res, int r_ld, void* out, int o_ld, int B, int H, int W, int C, void* stream);
/* InstanceNorm backward, piecewise: the statistics pass (part[B][nslabs][C][2] = per-slab (sum g m, sum g m xhat), nslabs <= 128),
 * ctg_in_finalize(mode 1) into s1 / s2 [B][C], and the elementwise pass dx = rstd (g m - s1 - xhat s2); ctg_in_bwd = all three. */
int ctg_in_bwd_partial(int dtype, const void* x, int x_ld, const void* dout, int d_ld, int pad, const float* mean,
                       const float* rstd, int act, int B, int H, int W, int C, int nslabs, float* part, void* stream);
int ctg_in_bwd_apply(int dtype, const void* x, int x_ld, const void* dout, int d_ld, int pad, const float* mean,
                     const float* rstd, const float* s1, const float* s2, int act, void* dx, int dx_ld, int B, int H, int W,
                     int C, void* stream);
int ctg_in_bwd(int dtype, const void* x, int x_ld, const void* dout, int d_ld, int pad, const float* mean,
               const float* rstd, int act, void* dx, int dx_ld, int B, int H, int W, int C, int nslabs,
               float* part, float* s1, float* s2, void* stream);
/* ctg_in_finalize(mode 1) + ctg_in_bwd_apply in one launch from partial sums part[B][nslabs <= 128][C][2] that ctg_in_bwd_partial
 * or a fused conv epilogue (ctg_conv_epilogue.bstats) produced. */
int ctg_in_bwd_stats(int dtype, const void* x, int x_ld, const void* dout, int d_ld, int pad, const float* mean,
                     const float* rstd, int act, void* dx, int dx_ld, int B, int H, int W, int C, int nslabs,
                     const float* part, void* stream);
/* out = a + fold(b), then * act'(yact) (yact = saved activation OUTPUT); any of a / b / yact may be NULL.
 * Replaces: autograd's gradient accumulation at fan-out points, ReflectionPad2d backward and the
 * LeakyReLU / Tanh backward (Model/HdGan.py:63,102,121; trainer/layers.py:60-62,299).                       */
int ctg_grad_combine(int dtype, const void* a, int a_ld, const void* b, int b_ld, int pad, const void* yact,
                     int y_ld, int act, void* out, int o_ld, int B, int H, int W, int C, void* stream);
/* out[B][H][W][C] = fold(dp[B][H+2p][W+2p][C]) for tiny-channel fp32 maps (ReflectionPad2d backward of the
 * generator's 7x7 head when its input carries a gradient: CycTrainer.py:153,156) */
int ctg_fold_f32(const float* dp, float* out, int B, int H, int W, int C, int pad, void* stream);
/* out[i] = g[i] * act'(y[i]) over n fp32 elements of any count (y = the saved activation OUTPUT): Tanh / LeakyReLU
 * backward of the 1-/2-channel fp32 maps (Model/HdGan.py:102 on images whose pixel count is not a multiple of 4) */
int ctg_act_bwd_f32(const float* g, const float* y, int act, float* out, long n, void* stream);
/* the same with sum_out[0] (+)= sum(out): Tanh backward of the generator's 1-channel output and the bias gradient of its
 * last conv (Model/HdGan.py:100-102) in one pass; part >= 4096 floats scratch */
int ctg_act_bwd_sum_f32(const float* g, const float* y, int act, float* out, long n, float* part, float* sum_out,
                        int accumulate, void* stream);
/* db[c] (+)= sum_{n,y,x} fold(g)[n,y,x,c]: bias gradient of convs not followed by an InstanceNorm */
int ctg_bias_grad(int dtype, const void* g, int g_ld, int pad, int B, int H, int W, int C, int Creal, int nslabs,
                  float* part, float* db, int accumulate, void* stream);

/* the two in one pass for a conv + bias + (Leaky)ReLU layer (trainer/layers.py:97-104): gout = fold(g) * act'(yact) (yact = the
 * layer's saved output) is written for the conv's backward passes and db[c] (+)= its sum; act in {1, 2} */
int ctg_bias_grad_act(int dtype, const void* g, int g_ld, int pad, const void* yact, int y_ld, int act, void* gout,
                      int go_ld, int B, int H, int W, int C, int Creal, int nslabs, float* part, float* db,
                      int accumulate, void* stream);

/* ---- registration U-Net plumbing: nn.MaxPool2d(2) (trainer/layers.py:172), F.interpolate(bilinear,
 * align_corners=False) x2 (trainer/reg.py:93), torch.cat (reg.py:77,94) ---- */
int ctg_maxpool2_fwd(int dtype, const void* x, int x_ld, void* out, int o_ld, int B, int H, int W, int C, void* stream);
int ctg_maxpool2_bwd(int dtype, const void* x, int x_ld, const void* dout, int d_ld, void* dx, int dx_ld,
                     int accumulate, int B, int H, int W, int C, void* stream);
int ctg_bilinear_fwd(int dtype, const void* x, int x_ld, void* out, int o_ld, int B, int Hi, int Wi, int Ho, int Wo,
                     int C, void* stream);
int ctg_bilinear_bwd(int dtype, const void* dout, int d_ld, void* dx, int dx_ld, int B, int Hi, int Wi, int Ho,
                     int Wo, int C, void* stream);
int ctg_copy_channels(int dtype, const void* src, int s_ld, void* dst, int d_ld, int C, long P, void* stream);
/* fp32 [P][x_ld] (C channels, C % 32 == 0) -> bf16 [P][2C]: packed weights as the operand of the split-bf16 ("bf16x3")
 * convolutions: hi = bf16(w), lo = bf16(w - hi), per 32 channels [hi 32 | lo 32] = one K step of ctg_conv_igemm(dtype 2),
 * ctg_conv_igemm_classes(dtype 2) and ctg_conv_smallcin(dtype 2). */
int ctg_split_weights(const float* x, long x_ld, void* out, int C, long P, void* stream);
/* ctg_split_weights for `count` dense packs (x_ld == C) given as parallel host arrays, ONE launch per 32 packs: every stale split of a
 * network after an optimiser step (Model/HdGan.py: 24 convs in the Generator alone) instead of one small launch per pack. */
int ctg_split_weights_multi(int count, const void* const* x, void* const* out, const int* C, const long* P, void* stream);
/* fp32 rows <-> split-pair rows (C channels of P pixels): dir 0: src fp32 (pitch s_ld floats) -> dst split pair (pitch d_ld bf16
 * elements); dir 1: src split pair -> dst fp32.  Where "bf16x3" tensors meet fp32 ones: wide network inputs / outputs at the
 * Python boundary (a stand-alone ResidualBlock, Model/HdGan.py:49-63; the feature maps Discriminator_m returns, :229-256). */
int ctg_pair_convert(int dir, const void* src, long s_ld, void* dst, long d_ld, int C, long P, void* stream);
/* packers that put 1-/2-channel tensors on the MFMA path (first / last layers) */
int ctg_chan_pad(int dtype, const float* src, int Cs, void* dst, int Cpad, long P, void* stream);
int ctg_im2col_pack(int dtype, const float* s0, const float* s1, int Cin, int B, int Hi, int Wi, int kh, int kw,
                    int stride, int pad, int pad_mode, void* dst, int Ho, int Wo, int Kpad, void* stream);
/* First-layer conv (Cin in {1,2} fp32 image planes [B][Hi][Wi]) with the im2col tile built in LDS: replaces
 * nn.Conv2d(1|2, C, k) at Model/HdGan.py:70,120,158, Model/CycleGan.py:28,78, trainer/reg.py:77 and the
 * input-gradient of the 1-channel tail conv (HdGan.py:110).  w = [w_npad][Kpad] from ctg_weight_pack of
 * weight.view(Cout, Cin*kh*kw); Cout <= 64; Kpad in {32, 64}; stats_part/stats_slabs_out as in ctg_conv_igemm. */
/* w_layout 0: k = (c*kh + ky)*kw + kx as above; 1 ("kx window": one plane, stride 1, kh, kw <= 8, Kpad 64, Cout > 32, dtype 1 / 2):
 * w[n][8 ky + kx] -- a chunk of the im2col row is then 8 consecutive pixels of one patch row and the tile is assembled from
 * register windows (the 7x7 head of the generator and the input gradient of its 7x7 tail).  dtype 2: y a split pair, w split by
 * ctg_split_weights. */
int ctg_conv_smallcin(int dtype, const float* s0, const float* s1, int Cin, int B, int Hi, int Wi, int kh, int kw,
                      int stride, int pad, int pad_mode, const void* w, int w_npad, int Kpad, int w_layout, const float* bias,
                      int act, void* y, int y_ld, int Ho, int Wo, int Cout, float* stats_part, int* stats_slabs_out,
                      void* stream);
/* The Generator's last layer forward: y[B][H][W] fp32 = act(bias + conv7x7(reflection_pad3(x))), x (dtype) [B][H][W][x_ld]
 * with 64 channels, ONE output channel; wp (dtype) = [NS][8][16][SC], SC = 32 (bf16) / 16 (fp32) channels per slice,
 * wp[s][j][o*8+ky][ci] = weight[0][SC*s+ci][ky][j-o] (0 <= j-o <= 6, ky <= 6, else 0).
 * Replaces ReflectionPad2d(3) + Conv2d(64, 1, 7) + Tanh (Model/HdGan.py:108-111). */
int ctg_conv_tail7(int dtype, const void* x, int x_ld, const void* wp, const float* bias, float* y, int act, int B, int H,
                   int W, void* stream);
/* The PatchGAN's last layer, Conv2d(512, 1, 4, padding=1) (Model/HdGan.py:136-137, 217-219; Model/CycleGan.py:104), on the vector
 * ALUs in fp32 (ABI 10; csrc/conv_cout1.hip): dtype 1 (bf16) / 2 (split pair), Cin = 512, k = 4, zero padding 0 <= pad < k, stride 1,
 * Ho = Hi + 2 pad - 3.  w = fp32 [16 taps][512] (w[ky*4+kx][ci] = weight[0][ci][ky][kx]: the master weights, unrounded).
 *   fwd:   y[B][Ho][Wo] fp32 = act(bias[0] + conv(x)), x (dtype) [B][Hi][Wi][x_ld]; replaces F.conv2d of that layer.
 *   bwd:   dx (dtype) [B][Hi][Wi][dx_ld] = the input gradient for g = dL/dy fp32 [B][Ho][Wo] (the dX half of convolution_backward).
 *   wgrad: part[Z][16][512] fp32, Z workgroups' shares of dW[tap][ci] = sum g x; finish with
 *          ctg_wgrad_reduce(part, Z, 1, 16, 512, dW, 16, 512, sm = 1, sn = 16, ...) into weight[0][ci][ky][kx]. */
int ctg_conv_cout1_fwd(int dtype, const void* x, int x_ld, const float* w, const float* bias, float* y, int act, int B, int Hi,
                       int Wi, int Cin, int k, int pad, int Ho, int Wo, void* stream);
int ctg_conv_cout1_bwd(int dtype, const float* g, const float* w, void* dx, int dx_ld, int B, int Hi, int Wi, int Cin, int k,
                       int pad, int Ho, int Wo, void* stream);
int ctg_conv_cout1_wgrad(int dtype, const float* g, const void* x, int x_ld, float* part, int Z, int B, int Hi, int Wi, int Cin,
                         int k, int pad, int Ho, int Wo, void* stream);
/* Weight gradient of the same first layers and of the 1-channel tail conv (HdGan.py:110), bf16:
 * part[(n*wgs + w)][m][k] = workgroup w's share of C[m][k] = sum_q Gpad[q][m] * Ipad[q + tap_k] over the grid
 * [0,Hs) x [0,Ws); Gpad[q] = g[pad_g(q - gpad)] (g bf16 [B][Gh][Gw][g_ld], Mc in {32,64} channels), Ipad[j] =
 * image[pad_i(j - ipad)] (1|2 fp32 planes), k = (c*kh + ky)*kw + kx < 64.  Finish with
 * ctg_wgrad_reduce(part, B*wgs, 1, Mc, 64, ...).  Replaces the weight-gradient half of convolution_backward.
 * g_ld < 0 (ABI 8): g is a split pair of pitch -g_ld (a multiple of 16, >= 2 Mc; lo plane -g_ld / 2 elements behind hi) and the
 * launch accumulates g_hi.I_hi + g_hi.I_lo + g_lo.I_hi with I_hi = bf16(I), I_lo = bf16(I - I_hi): each plane of g is read once. */
int ctg_corr_smallcin(const void* g, int Gh, int Gw, int g_ld, int Mc, int gpad, int g_pad_mode, const float* i0,
                      const float* i1, int Cin, int Ih, int Iw, int kh, int kw, int ipad, int i_pad_mode, int B,
                      int Hs, int Ws, float* part, int wgs, void* stream);
/* dst[t][n][k] = src[n*sn + k*sk + t*stp], zero padded to [ntaps][Npad][Kpad]; fp32 master -> dtype */
int ctg_weight_pack(int dtype, const float* src, long sn, long sk, long stp, int Nreal, int Kreal, void* dst,
                    int ntaps, int Npad, int Kpad, void* stream);
/* the same for `count` tensors given as parallel host arrays: all packs of a network after an optimiser step */
int ctg_weight_pack_multi(int dtype, int count, const void* const* src, void* const* dst, const long* sn,
                          const long* sk, const long* stp, const int* nreal, const int* kreal, const int* ntaps,
                          const int* npad, const int* kpad, void* stream);

/* ---- spatial transformer: Transformer_2D.forward (trainer/transformer.py:11-31) = pixel grid + flow ->
 * F.grid_sample(bilinear, align_corners=True, padding_mode="border"); 1-channel src, 2-channel flow given by
 * element strides (n, c, y, x).  dsrc is zeroed then scatter-added; dflow uses flow's strides. ---- */
int ctg_warp_fwd(const float* src, const float* flow, long fs_n, long fs_c, long fs_y, long fs_x, float* out,
                 int B, int H, int W, void* stream);
/* det_ws (may be NULL): B*H*W + 1 eight-byte words of workspace.  With it d_src is scattered in 64-bit fixed point (integer
 * atomics are associative: two runs are bit-identical whatever the arrival order) instead of with float atomics, whose result
 * depends on the order in the last bits -- the deterministic test / debug mode (CTG_DETERMINISTIC=1). */
int ctg_warp_bwd(const float* src, const float* flow, long fs_n, long fs_c, long fs_y, long fs_x,
                 const float* gout, float* dsrc, float* dflow, int B, int H, int W, void* det_ws, void* stream);

/* ---- losses.  `part` >= 4096 floats scratch; `out` / `gscale` are 1-element device buffers ----
 * smoothness: smooothing_loss (trainer/utils.py:165-173).  l1: nn.L1Loss (HdTrainer.py:721; CycTrainer.py:154,157);
 * with mask != NULL the stage-2 masked variant of HdTrainer.py:726-735.  avgpool: F.avg_pool2d over the whole
 * PatchGAN map (Model/HdGan.py:145,279,288).                                                                */
/* `weight`: the loss weight (Smooth_lamda / Corr_lamda1 / Corr_lamda2 of Yaml/HdGan.yaml:10-15) folded into the reduction's scale
 * (forward) and into the gradient (backward, on top of gscale) -- no scalar multiply launches around the loss */
int ctg_smooth_fwd(const float* f, long sn, long sc, long sy, long sx, int B, int C, int H, int W, float weight, float* part,
                   float* out, void* stream);
int ctg_smooth_bwd(const float* f, long sn, long sc, long sy, long sx, int B, int C, int H, int W, float weight,
                   const float* gscale, float* df, int accumulate, void* stream);
int ctg_l1_fwd(const float* a, const float* b, const float* mask, long n, float weight, float* part, float* out, void* stream);
int ctg_l1_bwd(const float* a, const float* b, const float* mask, long n, float weight, const float* gscale, float* da,
               int accumulate, void* stream);
/* LSGAN loss of GANLoss (Model/HdGan.py:276-285) on a 1-channel PatchGAN map x[B][HW], fused: out = sum_b s_b (mean(x[b]) - t_b)^2,
 * (t_b, s_b) = (t0, s0) for b < nb else (t1, s1) -- s = loss weight * w_i / group size; nb < B serves the fake and the real half
 * of the D step's batched pass (HdTrainer.py:745-747) at once.  pooled[B]: the per-sample means, kept for ctg_lsgan_bwd
 * (dx[b][i] = gscale * 2 s_b (pooled_b - t_b) / HW).  mode 0: the squared error above (nn.MSELoss, use_lsgan=True); mode 1:
 * nn.BCELoss's -(t log p + (1 - t) log(1 - p)), logs clamped at -100 (use_lsgan=False, Model/HdGan.py:266-267). */
int ctg_lsgan_fwd(const float* x, int B, int HW, int nb, float t0, float s0, float t1, float s1, int mode, float* pooled,
                  float* out, void* stream);
int ctg_lsgan_bwd(const float* pooled, int B, int HW, int nb, float t0, float s0, float t1, float s1, int mode,
                  const float* gscale, float* dx, void* stream);
/* out = scalars[0] + ... + scalars[count-1] (count <= 8 one-element device buffers): the sum of the step's loss terms
 * (HdTrainer.py:736) in one launch */
int ctg_sum_scalars(int count, const void* const* scalars, float* out, void* stream);
int ctg_avgpool_fwd(const float* x, int B, int HW, float* out, void* stream);
int ctg_avgpool_bwd(const float* gout, int B, int HW, float* dx, void* stream);

/* ---- evaluation path of test()/validation: to_windowdata (trainer/HdTrainer.py:41-64,
 * CycTrainer.py:34-57) over B slices of HW pixels with per-slice window centre / width; and the windowed + raw
 * MAE / PSNR / UQI of HdTrainer.py:1008-1050,1089-1125: out[B][2][3] doubles = {windowed, raw} x {MAE, PSNR, UQI};
 * part = B*nblk*20 doubles of workspace.  aliased = 1 reproduces trainer/CycTrainer.py:288-298, where `bb = b` / `cc = c`
 * are aliases and the windowed pair degenerates to the two +-1 masks.  Both entries: B <= 65535 (B is a grid dimension),
 * otherwise CTG_EINVAL; ctg_window_metrics: HW >= 2, 1 <= nblk <= 4096.  The sums behind `out` are double from the first
 * addition (every term formed in double from the fp32 images); a NaN sample makes its slice's numbers NaN, MAE included
 * (the reference's nanmean MAE is finite: a deliberate difference). ---- */
int ctg_to_windowdata(const float* img, const float* wc, const float* ww, float* out, int B, long HW, void* stream);
/* Mean structural similarity of B slice pairs [B][H][W] (ABI 9): what skimage.measure.compare_ssim(x, y) returns with its
 * defaults (7x7 uniform window, sample covariance, K1 0.01, K2 0.03, float64) -- the validation pass of every trainer's train()
 * (trainer/HdTrainer.py:242-258, 765-781; CycTrainer.py:203-218; p2pTrainer.py:153-166; RegTrainer.py:206-221) and the SSIM /
 * SSIMw lines of test() (HdTrainer.py:1028, 1053).  data_range: 2 for the reference's float images.  mode 0: the pair as given,
 * out[B] doubles (wc / ww unused); mode 1: the two masked pairs ctg_window_metrics builds, out[B][2] = {windowed, raw}.
 * part: 2 * B * ceil((H-6)/16) * ceil((W-6)/16) doubles of workspace.  H, W >= 7. */
int ctg_ssim(const float* fake, const float* real, const float* wc, const float* ww, int B, int H, int W, int mode, int aliased,
             double data_range, double* part, double* out, void* stream);
int ctg_window_metrics(const float* fake, const float* real, const float* wc, const float* ww, int B, long HW,
                       int nblk, int aliased, double* part, double* out, void* stream);
/* input pipeline arithmetic (section 8f rank 2): read_ori_w after the DICOM read (trainer/datasets.py:36-71): raw HU
 * (int16, SimpleITK convention) -> windowed image (centre wc, width ww; the reference hard-codes 50 / 400) and the
 * full-range image, both in [-1, 1]; Resize = F.interpolate(mode="nearest") (trainer/utils.py:13-32) on B planes.
 * `full` wraps above HU 31743 as the reference does (`data1 + 1024` on the reader's int16 array stays int16 in numpy): such a
 * value becomes negative and is clamped to -1 like air.  The same arithmetic (csrc/input_arith.h: hu_fullrange) serves
 * ctg_series_inputs and ctg_hu_affine_inputs; ctg_subtract_slices' `a = max(ct_hu + 1024, 0)` is int32 and does NOT wrap, so
 * above HU 31743 it is no longer the stored value ctg_series_inputs fed the generator (no CT holds such values). */
int ctg_hu_to_inputs(const short* hu, float wc, float ww, float* win, float* full, long n, void* stream);
int ctg_resize_nearest(const float* src, int B, int Hi, int Wi, float* dst, int Ho, int Wo, void* stream);
/* training augmentation of every loader (ABI 12; trainer/HdTrainer.py:130-142,641-653, CycTrainer.py:91-99, p2pTrainer.py:81-89,
 * RegTrainer.py:122-132, applied per image in trainer/datasets.py:103-119,218-232): RandomAffine(degrees, translate, scale,
 * fillcolor) on a float PIL image -- Image.transform(AFFINE, NEAREST), PIL's 16.16 fixed-point loop -- followed by Resize, as
 * one gather.  src: N planes [Hi][Wi] fp32; coef: device int32 [N][6] = (A0 .. A5), PIL's fixed-point coefficients of each
 * plane's inverse matrix (cta_gan_amd/trainer/augment.py: fixed_coefficients); dst [N][Ho][Wo].  Output pixel (oy, ox) reads
 * the pixel (iy, ix) of the Hi x Wi warped image by ctg_resize_nearest's index rule (the identity for Ho == Hi, Wo == Wi),
 * and that pixel is src[n][ys][xs] with xs = (A2 + A1 iy + A0 ix) >> 16, ys = (A5 + A4 iy + A3 ix) >> 16 (64-bit, arithmetic
 * shift) when 0 <= xs < Wi and 0 <= ys < Hi, `fill` otherwise.  Sides 1 .. 32768.
 * ctg_hu_affine_inputs: the same gather on raw HU, B planes [Hi][Wi] int16 (ctg_hu_to_inputs' input) -> win / full
 * [B][Ho][Wo], each pixel ctg_hu_to_inputs' value of the source pixel or `fill`; coef [B][2][6]: plane 0 the windowed image's
 * coefficients, plane 1 the full-range image's (the reference draws them independently).  Equals ctg_hu_to_inputs ->
 * ctg_affine_nearest -> ctg_resize_nearest bit for bit. */
int ctg_affine_nearest(const float* src, const int* coef, int N, int Hi, int Wi, float fill, float* dst, int Ho, int Wo,
                       void* stream);
int ctg_hu_affine_inputs(const short* hu, const int* coef, int B, int Hi, int Wi, float wc, float ww, float fill, float* win,
                         float* full, int Ho, int Wo, void* stream);

/* ---- series inference, the way back (ABI 13): the export half of every trainer's test() loop (trainer/HdTrainer.py:539-552,
 * 1062-1075; CycTrainer.py:337-340, p2pTrainer.py:288-291, RegTrainer.py:360-363) without its DICOM container ----
 * ctg_export_slices: img = the generator's fp32 output planes [B][Hi][Wi]; wc / ww = per-slice window centre / width on the
 * device, as ctg_to_windowdata takes them (read only when level != NULL).  One pass writes
 *   pix   int16 [B][Ho][Wo]: `newimg = (fake_BB + 1) * 0.5 * 4095; newimg.astype(np.int16)` (HdTrainer.py:539, 543) -- the three
 *         float32 operations one after another, each rounded, then truncated toward zero; hu != 0 subtracts 1024 after the
 *         truncation (SimpleITK's convention, the inverse of the + 1024 of ctg_hu_to_inputs' full-range image).  The reference's
 *         domain is the generator's tanh range [-1, 1], where the value is 0 .. 4095; outside it the conversion saturates to
 *         the int16 range (also after the hu subtraction) and NaN gives 0 -- numpy leaves both undefined.
 *   level uint8 [B][Ho][Wo]: the 8-bit window level to_windowdata (HdTrainer.py:41-61) computes before it rescales to [-1, 1]
 *         (:62-63), `== 0 -> -2000` included: level / 255 rescaled IS ctg_to_windowdata's value, bit for bit (NaN gives 0).
 * Either of pix / level may be NULL to skip it (not both).  (Ho, Wo) != (Hi, Wi): every output pixel gathers its source by
 * ctg_resize_nearest's index rule, so a series scanned at another size than the generator runs at comes back at its own.
 * img 4-byte, pix 2-byte aligned; the 16-byte streaming path needs no more than that.  B <= 65535, planes below 2^31 pixels.
 * The reference's 8-bit DICOM branch (`astype(np.int8)`, :544-545) is not built.
 * ctg_series_inputs: raw HU int16 [B][Hi][Wi] (ctg_hu_to_inputs' input) -> only the full-range plane [B][Ho][Wo] that test()
 * feeds the generator (`A2`; trainer/datasets.py:36-71 + Resize, trainer/utils.py:13-32), gathered by the same index rule:
 * equals ctg_hu_to_inputs' `full` -> ctg_resize_nearest bit for bit. */
int ctg_export_slices(const float* img, const float* wc, const float* ww, int B, int Hi, int Wi, short* pix,
                      unsigned char* level, int Ho, int Wo, int hu, void* stream);
int ctg_series_inputs(const short* hu, int B, int Hi, int Wi, float* full, int Ho, int Wo, void* stream);

/* ---- series inference, projections (ABI 15): the maximum- / minimum-intensity and mean projections of the exported volume along
 * the three body axes, accumulated chunk by chunk behind ctg_export_slices (cta_gan_amd/infer.py: SeriesProjector.update /
 * .result, SeriesTranslator(project=...), project_volume).  The reference has no counterpart: its test() writes slices only.
 * ctg_project_accumulate: pix = int16 [K][H][W], contiguous, 2-byte aligned: slices n0 .. n0+K-1 of a volume of N slices.
 *   mode 0 max, 1 min, 2 sum.  int32 accumulators, each may be NULL (not all three):
 *     axial    [S][H][W], S = ceil(N / thick): slice n belongs to slab n / thick (slabs do not overlap; thick >= N is the whole
 *              volume); chunks and slabs straddle each other freely, the slab index comes from n0;
 *     coronal  [N][W], the reduction over H;  sagittal [N][H], the reduction over W: rows n0 .. n0+K-1 are completed by this call.
 *   The caller fills every accumulator with the mode's identity (-32768, 32767, 0) before the first chunk; the call always combines
 *   (coronal and sagittal with int32 atomics) and never first-writes, and the calls of one volume are ordered on one stream.  Exact
 *   integer arithmetic: the same bits on every run.  The caller sizes the accumulators for n0 + K <= N.  K, H, W, thick 1 .. 65535
 *   (a sum of fewer than 65536 int16 values stays inside int32), n0 >= 0; anything else is CTG_EINVAL.
 * ctg_project_finish: acc = one accumulator array of `planes` planes of `plane_items` items -> values int16 and level uint8 of
 *   the same shape in one pass; either may be NULL (not both).  mode 2: value = acc / div, C integer division (truncating toward
 *   zero), div_last instead of div in the last plane (the last axial slab may be shorter); coronal / sagittal: planes = 1 and
 *   div = div_last = H / W.  mode 0, 1: the accumulator itself.  level = the tail of to_windowdata (trainer/HdTrainer.py:43-61) on
 *   the stored value t = (float)(value + (hu ? 1024 : 0)): t == 0 -> -2000; t - 1024; t - wmin; trunc(t * dfac); clamp to
 *   [0, 255] -- float32, every operation rounded on its own, wmin / dfac as ctg_export_slices forms them from (wc, ww): the level
 *   ctg_export_slices gives a pixel of that stored value. ---- */
int ctg_project_accumulate(const short* pix, int K, int H, int W, int n0, int thick, int mode, int* axial, int* coronal,
                           int* sagittal, void* stream);
int ctg_project_finish(const int* acc, int planes, long plane_items, int mode, int div, int div_last, float wc, float ww, int hu,
                       short* values, unsigned char* level, void* stream);

/* ---- series inference, rotating projections (added under ABI 15: purely additive, no existing signature or meaning moves, so
 * the version stays 15): the maximum- / minimum-intensity or mean projection of the exported volume at any view angle about the
 * cranio-caudal axis, chunk by chunk behind ctg_export_slices (cta_gan_amd/infer.py: SeriesRotator.update,
 * SeriesTranslator(rotate=...), rotate_volume).  The reference has no counterpart.
 * ctg_project_rotate: pix = int16 [K][H][W], contiguous, 2-byte aligned (a view into a larger buffer is fine): slices
 *   n0 .. n0+K-1 of a volume of N slices.  coef = int32 [A][6] on the device, one row (c0 .. c5) per angle.  A view has a detector
 *   of U columns and rays of T unit steps; the sample of (u, t) is pixel
 *       xi = (c0 + c1 u + c2 t) >> 16,   yi = (c3 + c4 u + c5 t) >> 16      (arithmetic shift)
 *   of the slice and counts only when 0 <= xi < W and 0 <= yi < H.  For the angle theta about ((W-1)/2, (H-1)/2) the host forms, in
 *   float64 with r(v) = floor(v 65536 + 0.5), cu = (U-1)/2, ct = (T-1)/2 (infer.py: rotation_coefficients):
 *       c0 = r(cx - cu cos + ct sin + 0.5)  c1 = r(cos)  c2 = r(-sin)      c3 = r(cy - cu sin - ct cos + 0.5)  c4 = r(sin)  c5 = r(cos)
 *   (theta = 0: the coronal view, rays along y; 90: the sagittal view; the + 0.5 makes the sampling nearest).  The caller keeps
 *   |c1|, |c2|, |c4|, |c5| <= 65536 and |c0|, |c3| < 2^29, so that with H, W, U, T <= 4096 the sums stay inside int32; the kernel
 *   bounds-checks every sample index and is memory-safe whatever the table holds (the sums wrap).
 *   mode 0 max, 1 min, 2 mean = sum / count of the ray's own counted samples, C integer division (truncating toward zero); a ray
 *   without a counted sample gets `fill` (an int16 value).  values int16 [A][N][U] and level uint8 [A][N][U], either may be NULL
 *   (not both): one launch writes rows n0 .. n0+K-1 of all A planes and nothing else.  level = what ctg_project_finish gives that
 *   value for (wc, ww, hu), written in the same pass.  Exact integer arithmetic up to the level: the same bits as numpy.
 *   CTG_EINVAL: pix or coef NULL, both outputs NULL, K < 1, n0 < 0, n0 + K > N, H / W / U / T / A outside 1 .. 4096, mode outside
 *   0 .. 2, fill outside int16, a misaligned pointer. ---- */
int ctg_project_rotate(const short* pix, int K, int H, int W, int n0, int N, const int* coef, int A, int U, int T, int mode,
                       int fill, float wc, float ww, int hu, short* values, unsigned char* level, void* stream);

/* ---- series inference, rotating projections with bilinear sampling (added under ABI 15: purely additive, no existing signature
 * or meaning moves, so the version stays 15): cta_gan_amd/infer.py: SeriesRotator(sampling="bilinear"), rotate_volume,
 * SeriesTranslator(rotate_sampling="bilinear"); ops.project_rotate(sampling="bilinear").
 * ctg_project_rotate_bilinear: the arguments, the checks, the table, the detector, the modes, `fill`, the level and the rows
 *   written are those of ctg_project_rotate, and so is what counts: with X = c0 + c1 u + c2 t and Y = c3 + c4 u + c5 t (they
 *   carry the + 0.5 of the nearest rule) sample (u, t) counts exactly when pixel (X >> 16, Y >> 16) lies in the slice, so a ray's
 *   count and the place of `fill` do not depend on the sampling.  The value of a counted sample, all shifts arithmetic:
 *       Xc = X - 32768            Yc = Y - 32768                    (the centre-based position, 16.16)
 *       x0 = Xc >> 16             fx = (Xc >> 8) & 255              (x0 may be -1; a fraction of 8 bits)
 *       y0 = Yc >> 16             fy = (Yc >> 8) & 255
 *       xa = clamp(x0, 0, W-1)    xb = clamp(x0 + 1, 0, W-1)        (the edge pixel replicated)
 *       ya = clamp(y0, 0, H-1)    yb = clamp(y0 + 1, 0, H-1)
 *       top = p[ya][xa] (256 - fx) + p[ya][xb] fx        bot = p[yb][xa] (256 - fx) + p[yb][xb] fx
 *       v   = (top (256 - fy) + bot fy + 32768) >> 16
 *   The weights sum to 65536, so v is an int16 value; the sum before the shift lies in [-2^31 + 32768, 2^31 - 32768].  max and min
 *   run over v, the mean is the int32 sum of v (at most 4096 samples) / the ray's count, truncating toward zero.  Memory-safe
 *   whatever the table holds: the clamps keep the four addresses inside the slice, a sample that is not counted reads pixel 0.
 * Oversampled rays, for either entry, are a matter of the table: t voxels in T = t s steps of 1 / s voxel have ct = (T - 1) / (2 s),
 *   c2 = r(-sin / s), c5 = r(cos / s) and the other four as above (infer.py: rotation_coefficients(..., oversample=s)); T <= 4096.
 *   Exact integer arithmetic up to the level: the same bits as numpy (tests/rotate_lerp_np.py). ---- */
int ctg_project_rotate_bilinear(const short* pix, int K, int H, int W, int n0, int N, const int* coef, int A, int U, int T, int mode,
                                int fill, float wc, float ww, int hu, short* values, unsigned char* level, void* stream);

/* ---- series inference, the subtraction volume (added under ABI 15: purely additive, no existing signature or meaning moves, so
 * the version stays 15): synthesized CTA minus the CT it was made from, chunk by chunk behind ctg_export_slices
 * (cta_gan_amd/infer.py: SeriesTranslator(subtract=True), subtract_volume).  The generator writes on its input's pixel grid, so the
 * pair is registered by construction and bone cancels in the difference.
 * ctg_subtract_slices: cta = int16 [B][H][W], the synthesized pixels as ctg_export_slices wrote them (cta_is_hu != 0: its hu
 *   convention, stored value - 1024); ct_hu = int16 [B][H][W], the raw HU the generator was fed (ctg_series_inputs' input).  Both
 *   contiguous and 2-byte aligned: a view one plane into a larger buffer and planes of odd H W are fine.  Per pixel, in int32:
 *     a = max(ct_hu + 1024, 0);   b = cta + (cta_is_hu ? 1024 : 0);   d = b - a
 *     median != 0: d = the median of the 3 x 3 in-plane neighbourhood of d, the edge pixel replicated outside the plane
 *                  (scipy.ndimage.median_filter(size=3, mode='nearest') of every plane; H = 1 or W = 1 is legal)
 *     d = 0 where ct_hu < ct_min, ct_hu > ct_max or d < floor: the centre pixel, after the median; equality keeps the pixel
 *           (ct_min = -32768 and ct_max = 32767 switch the band off, floor = INT_MIN the floor)
 *     sub = clamp(d, -32768, 32767)
 *     level = what ctg_project_finish gives the value `sub` for (wc, ww, hu = 1): the window a HU difference is viewed in.
 *   sub int16 [B][H][W] (2-byte aligned) and level uint8 [B][H][W]; either may be NULL (not both).  The outputs must not overlap
 *   the inputs: with the median a pixel is read by the workgroups of its neighbours, so an in-place call is wrong.  One launch,
 *   nothing allocates or synchronises.  Exact integer arithmetic up to the level: the same bits as numpy.
 *   CTG_EINVAL: cta or ct_hu NULL, both outputs NULL, B / H / W outside 1 .. 65535, ct_min > ct_max, a misaligned pointer. ---- */
int ctg_subtract_slices(const short* cta, const short* ct_hu, int B, int H, int W, int cta_is_hu, int median, int floor, int ct_min,
                        int ct_max, float wc, float ww, short* sub, unsigned char* level, void* stream);

/* ---- series inference, sliding thin-slab projections (added under ABI 15: purely additive, no existing signature or meaning
 * moves, so the version stays 15): the projection of a slab of `thick` voxels that moves on by `step` voxels, along any of the
 * three body axes, chunk by chunk behind ctg_export_slices (cta_gan_amd/infer.py: SeriesSlabs.update, SeriesTranslator(slabs=...),
 * slab_volume).  The reference has no counterpart.
 * One rule for every axis of extent L (N slices, H rows, W columns): 1 <= step <= thick is checked against the thick given, then
 *   T = min(thick, L); slab j covers [j step, min(j step + T, L)); J = 1 if L <= T, else ceil((L - T) / step) + 1.  Only the last
 *   slab can be short (its mean divides by its own length); step == thick is the plan of ctg_project_accumulate.
 * ctg_project_slabs_inplane: pix = int16 [K][H][W], contiguous, 2-byte aligned (a view into a larger buffer is fine): slices
 *   n0 .. n0+K-1 of a volume of N slices.  axis 0: coronal, slabs along y, out[j][n][x] = the reduction over the rows of slab j,
 *   [J][N][W]; axis 1: sagittal, slabs along x, out[j][n][y] = the reduction over the columns of slab j, [J][N][H].  mode 0 max,
 *   1 min, 2 mean = the exact sum / the slab's own length, C integer division (truncating toward zero).  values int16 and level
 *   uint8 of that shape, either may be NULL (not both): one launch writes rows n0 .. n0+K-1 of all J planes and nothing else.
 *   level = what ctg_project_finish gives that value for (wc, ww, hu), written in the same pass.  Integer arithmetic up to the
 *   level: the same bits as numpy.
 * ctg_project_accumulate_sliding: the axial slabs.  axial = int32 [J][H][W] that holds the mode's identity before the first chunk
 *   (J from N, thick, step by the rule); slice n is combined into every slab that covers it, in place by a plain read-modify-write
 *   (never first-writes; the calls of one volume are ordered on one stream, in any order, every slice once).  mode 0 max, 1 min,
 *   2 sum.  With step == thick the accumulators equal ctg_project_accumulate's bit for bit; ctg_project_finish(axial, J, H W,
 *   mode, T, the last slab's length, ...) finishes them.
 *   CTG_EINVAL (both): a required pointer NULL or misaligned (pix, values 2 bytes; axial 4), K / H / W / N / thick outside
 *   1 .. 65535 (a sum of fewer than 65536 int16 values stays inside int32), step outside 1 .. thick, mode outside 0 .. 2, axis
 *   outside 0 .. 1, n0 < 0, n0 + K > N, a grid beyond 2^31 - 1 workgroups.  Nothing is launched then. ---- */
int ctg_project_slabs_inplane(const short* pix, int K, int H, int W, int n0, int N, int axis, int thick, int step, int mode,
                              float wc, float ww, int hu, short* values, unsigned char* level, void* stream);
int ctg_project_accumulate_sliding(const short* pix, int K, int H, int W, int n0, int N, int thick, int step, int mode, int* axial,
                                   void* stream);

/* ---- series inference, the depth of the maximum (added under ABI 15: purely additive, no existing signature or meaning moves, so
 * the version stays 15): a maximum-intensity projection throws the depth away -- front and back look the same in a rotating MIP,
 * and a pixel cannot be sent back to the voxel it came from.  These entries give, beside the value and its level, the depth plane
 * (how far along the ray the value was found) and the depth-cued level (the level attenuated by that depth): cta_gan_amd/infer.py:
 * SeriesRotator(depth=True), SeriesProjector(depth=True), rotate_volume, project_volume, SeriesTranslator(depth=True), ray_voxel.
 * Definitions, for all three entries:
 *   Modes: 0 max and 1 min.  A mean has no depth: mode 2 is CTG_EINVAL.
 *   Depth of a ray: the index along the ray of the first sample, from the viewer's end, that attains the projected value: the
 *     smallest index wins a tie, np.argmax / np.argmin over the axis.  Rotating projection: the step t in 0 .. T-1 (steps of 1 / s
 *     voxel when oversampled; step 0 is the end nearest the viewer), over counted samples only; a ray that misses the slice
 *     (count 0) has depth -1.  Axis projections: the voxel coordinate along the projected axis -- the slice n (global, also with
 *     axial slabs), the row y (coronal), the column x (sagittal).  Depth planes are int16: an axis extent above 32767 is CTG_EINVAL.
 *   Packed key: with b = value + 32768 in 0 .. 65535 and depth d,
 *       max: key = b << 16 | (65535 - d), combined by the unsigned maximum, identity 0
 *       min: key = b << 16 | d,           combined by the unsigned minimum, identity 0xffffffff
 *     so "better value first, then nearer depth" is the order of one 32-bit word, and every reduction stays order-free.  Keyed
 *     accumulators are int32 arrays filled with 0 / -1 (the identities' bits); the kernels read and combine them as unsigned.
 *   Depth cue: an integer cue in 0 .. 256.  With E the length of the ray and d the depth measured from the ray's own start,
 *       w = 256 - (cue d) / E  (C division: 1 <= w <= 256 because d < E; a missed ray keeps w = 256),  cued = (level w + 128) >> 8
 *     E = T steps (rotation), H (coronal), W (sagittal), the slab's own length min(thick, N - slab thick) (axial; only the last
 *     slab can be short), and d = n - slab thick for axial.  cue = 0 reproduces level bit for bit; cued <= level always.
 * ctg_project_rotate_depth: the arguments, the checks, the table, the detector, the interval, the "counted" rule, `fill` and the
 *   rows written are those of ctg_project_rotate; sampling 0 = nearest, 1 = bilinear (the value of ctg_project_rotate_bilinear).
 *   Outputs [A][N][U]: values int16, level uint8, depth int16, cued uint8; any may be NULL, not all four.  values and level equal
 *   what ctg_project_rotate / _bilinear write for the same arguments.  One launch, no accumulator.
 * ctg_project_accumulate_depth: the arguments, the checks and the chunk handling of ctg_project_accumulate on keyed accumulators of
 *   the same shapes: axial [S][H][W] keys carry n0 + k, coronal [N][W] keys the row y, sagittal [N][H] keys the column x.  Chunks in
 *   any order, every slice once.  K, thick 1 .. 65535; n0 + K, H, W <= 32767.
 * ctg_project_finish_depth: acc = one keyed accumulator of `planes` planes of `plane_items` items -> values int16, level uint8,
 *   depth int16, cued uint8 of the same shape; any may be NULL, not all four.  Plane s holds rays that start at coordinate s thick
 *   of an axis of `extent` voxels (axial: planes = S, thick, extent = N; coronal: planes = 1, thick = extent = H; sagittal:
 *   planes = 1, thick = extent = W); (planes - 1) thick < extent <= 32767.  thick and extent must be those the accumulator was
 *   filled under (the thick of the ctg_project_accumulate_depth calls, the axis' full extent): the keys carry global coordinates
 *   and nothing can check them against another plan -- with another plan `cued` is meaningless (w is kept in 1 .. 256, nothing
 *   else).  An item no chunk reached has the mode's identity value and depth -1.  level as ctg_project_finish. ---- */
int ctg_project_rotate_depth(const short* pix, int K, int H, int W, int n0, int N, const int* coef, int A, int U, int T, int mode,
                             int sampling, int fill, int cue, float wc, float ww, int hu, short* values, unsigned char* level,
                             short* depth, unsigned char* cued, void* stream);
int ctg_project_accumulate_depth(const short* pix, int K, int H, int W, int n0, int thick, int mode, int* axial, int* coronal,
                                 int* sagittal, void* stream);
int ctg_project_finish_depth(const int* acc, int planes, long plane_items, int mode, int thick, int extent, int cue, float wc,
                             float ww, int hu, short* values, unsigned char* level, short* depth, unsigned char* cued, void* stream);

/* ---- series inference, the volume-rendered rotating view (added under ABI 15: purely additive, no existing signature or meaning
 * moves, so the version stays 15): front-to-back compositing along the rays of the rotating projections, the display that keeps
 * the depth a MIP throws away.  cta_gan_amd/infer.py: SeriesRenderer, render_volume, SeriesTranslator(render=...),
 * transfer_function; ops.project_render, ops.TransferTable.  The reference has no counterpart.
 * ctg_project_render: pix, K, H, W, n0, N, coef, A, U, T, wc, ww, hu and stream, the table, the detector, the interval, the
 *   "counted" rule and the rows written are those of ctg_project_rotate_depth; sampling 0 = nearest (the pixel), 1 = bilinear (the
 *   value of ctg_project_rotate_bilinear).  An uncounted sample takes no part.
 *   Classification: a counted sample of value v has the class l = the 8-bit window level of v in the window (wc, ww) -- the
 *     transfer function's own window, independent of any display window -- with `hu` as everywhere (v + 1024 is the stored value):
 *     a whole number 0 .. 255.  lut = uint16 [256][4] on the device, 2-byte aligned: R, G, B, alpha of every class.  The kernel
 *     uses min(R, 255), min(G, 255), min(B, 255) and A = min(alpha, 32768); A = 32768 is opaque, so any table is defined.
 *   Compositing: over the ray's counted samples in ascending step t, from Tr = 32768 and C[3] = 0, all uint32:
 *       wgt = (Tr A) >> 15;   C[c] += wgt col[c]  (c = R, G, B);   Tr -= wgt;
 *       if depth < 0 and 32768 - Tr >= surface: depth = t;     if Tr <= stop: the ray ends (later samples take no part)
 *     wgt <= Tr; the weights sum to 32768 - Tr, hence C[c] <= 32768 * 255: nothing overflows and every output fits 8 bits.
 *     stop in 0 .. 32767 is part of the definition (0: only an opaque sample ends a ray); surface in 1 .. 32768.
 *   Outputs, any subset, at least one, each [A][N][U] (rows n0 .. n0+K-1 are written, nothing else):
 *     rgb uint8 [A][N][U][3]: (C[c] + bg_c Tr + 16384) >> 15, the background bg_r, bg_g, bg_b in 0 .. 255;
 *     opacity uint8: ((32768 - Tr) 255 + 16384) >> 15;
 *     depth int16 (2-byte aligned): the step of the first counted sample at which the accumulated opacity 32768 - Tr reaches
 *     `surface`, -1 if it never does.  A ray that misses the slice gives bg, opacity 0 and depth -1.
 *   Oversampled rays are a matter of the tables: T = t s steps, and the host corrects the alphas per step when it builds lut.
 *   Exact integer arithmetic: the same bits as numpy (tests/render_np.py).  One launch, no accumulator, no atomics.
 *   CTG_EINVAL, nothing launched: a null pix, coef or lut; no output; K < 1, n0 < 0, n0 + K > N; H, W, U, T or A outside
 *   1 .. 4096; sampling outside 0 .. 1; stop outside 0 .. 32767; surface outside 1 .. 32768; a bg outside 0 .. 255; pix, lut or
 *   depth not 2-byte aligned, coef not 4-byte aligned; a grid beyond 2^31 - 1 workgroups. ---- */
int ctg_project_render(const short* pix, int K, int H, int W, int n0, int N, const int* coef, int A, int U, int T,
                       const unsigned short* lut, int sampling, int stop, int surface, int bg_r, int bg_g, int bg_b, float wc,
                       float ww, int hu, unsigned char* rgb, unsigned char* opacity, short* depth, void* stream);

/* ---- series inference, lines in any direction (added under ABI 15: purely additive, no existing signature or meaning moves, so
 * the version stays 15): oblique planes, tumbling views and curved reformats -- every display whose rows cross slices, which the
 * entries above cannot make.  cta_gan_amd/infer.py: view_lines, orbit_lines, oblique_lines, curved_lines, VolumeReformatter,
 * reformat_volume, SeriesTranslator(reformat=...); ops.reformat_lines, ops.LineTable.  The reference has no counterpart.
 * ctg_reformat_lines: vol = the whole int16 volume [N][H][W] on the device, contiguous, 2-byte aligned.  lines = int32 [L][9] on
 *   the device, 4-byte aligned, one row (x0, xu, xk, y0, yu, yk, z0, zu, zk) per output line: sample (l, i, k), i in 0 .. U-1 and
 *   k in 0 .. T-1, lies at the 16.16 fixed-point position X = x0 + xu i + xk k, Y = y0 + yu i + yk k, Z = z0 + zu i + zk k (the
 *   + 0.5 of the nearest rule inside, as in the rotation's table) and is counted exactly when voxel (X >> 16, Y >> 16, Z >> 16),
 *   arithmetic shifts, lies in the volume.  out[l][i] = the max (mode 0), min (1) or mean (2: the exact sum over the ray's own
 *   count, C division) over the counted samples of ray (l, i); `fill` where none is counted.  T = 1 is a plain reformat, T > 1 a
 *   slab or projection along the ray.  values int16 [L][U] and level uint8 [L][U], either may be NULL (not both); level = the
 *   8-bit window level of v + (hu ? 1024 : 0) in (wc, ww), as ctg_project_rotate writes it, in the same pass.
 *   sampling 0 = nearest: the voxel above.  sampling 1 = trilinear in exact integers about the centre-based position
 *   Xc = X - 32768 (Y, Z likewise): x0 = Xc >> 16, fx = (Xc >> 8) & 255 per axis; v0 = the bilinear value of
 *   ctg_project_rotate_bilinear from fx, fy on slice clamp(z0), v1 the same on slice clamp(z0 + 1) (the in-plane neighbours
 *   clamped as there), v = (v0 (256 - fz) + v1 fz + 128) >> 8.  Two roundings, each defined; v is an int16 value for every input
 *   and a constant volume stays constant.  Which samples count does not depend on the sampling.
 *   Every address is bounds-checked or clamped whatever the table holds; the sums are formed in unsigned arithmetic and read as
 *   int32, so the caller keeps |c0| + |cu| (U-1) + |ck| (T-1) < 2^31 for every line and axis (ops.LineTable checks it on the host):
 *   beyond that the result is defined by the wrapped sums, still without an access outside the volume.
 *   Exact integer arithmetic: the same bits as numpy (tests/reformat_np.py).  One launch, no accumulator, no atomics.
 *   CTG_EINVAL, nothing launched: a null vol or lines; no output; N, H, W, U or T outside 1 .. 4096; L < 1; mode outside 0 .. 2;
 *   sampling outside 0 .. 1; fill outside int16; vol or values not 2-byte aligned, lines not 4-byte aligned; a grid beyond
 *   2^31 - 1 workgroups (L ceil(U / 32)). ---- */
int ctg_reformat_lines(const short* vol, int N, int H, int W, const int* lines, int L, int U, int T, int mode, int sampling,
                       int fill, float wc, float ww, int hu, short* values, unsigned char* level, void* stream);

/* ---- series inference, shaded volume rendering along lines in any direction (added under ABI 15: purely additive, no existing
 * signature or meaning moves, so the version stays 15): the compositing of ctg_project_render along the rays of a line table,
 * with trilinear sampling, anisotropic voxels inside the geometry and every sample's colour shaded by the local gradient.
 * cta_gan_amd/infer.py: VolumeRenderer, render_lines_volume, headlight, line_voxel, SeriesTranslator(render3d=...);
 * ops.render_lines, ops.LightTable.  The reference has no counterpart.
 * ctg_render_lines: vol, N, H, W, lines, L, U, T, the positions of the samples, the "counted" rule and the value v of a sample
 *   (sampling 0 = nearest, 1 = trilinear) are exactly those of ctg_reformat_lines; lut, stop, surface, bg_r, bg_g, bg_b, wc, ww, hu,
 *   the class of a counted sample, col = min(R, G, B, 255) and A = min(alpha, 32768) are exactly those of ctg_project_render.
 *   Compositing: over the ray's counted samples in ascending step k, from Tr = 32768 and C[3] = 0, all uint32:
 *       wgt = (Tr A) >> 15;   C[c] += wgt cols[c];   Tr -= wgt;
 *       if depth < 0 and 32768 - Tr >= surface: depth = k;     if Tr <= stop: the ray ends (later samples take no part)
 *   Shading: light = int32 [L][3] on the device, 4-byte aligned, one vector per line (4096 = unit length), or NULL: cols = col.
 *     Otherwise the colour of a counted sample is shaded at its own voxel (xi, yi, zi) = (X >> 16, Y >> 16, Z >> 16), the same for
 *     both samplings, p = the stored int16 values:
 *       dx = p[zi][yi][min(xi+1, W-1)] - p[zi][yi][max(xi-1, 0)], dy and dz likewise along y and z (central differences, the edge
 *         replicated; `hu` cancels);
 *       gx = clamp(dx, -4095, 4095), gy likewise, gz = clamp((dz zscale + 128) >> 8, -4095, 4095) (arithmetic shift), zscale =
 *         256 / aspect in 8.8 fixed point (aspect = slice spacing / pixel spacing);  m = gx^2 + gy^2 + gz^2 < 2^26;
 *       l[c] = clamp(light[l][c], -4096, 4096) -- clamped in the kernel, so any table is defined;
 *       dot = |gx l[0] + gy l[1] + gz l[2]| < 2^26: the absolute value makes the lighting two-sided;
 *       shade = 256 if m < gmin2 (a flat region shows its class colour); otherwise, with n = floor(sqrt(m)) >= 1 exactly,
 *         diff = min((dot / n) >> 4, 256) (C division) and shade = ambient + (((256 - ambient) diff + 128) >> 8);
 *       cols[c] = (col[c] shade + 128) >> 8 <= 255.
 *     So C[c] <= 32768 * 255 as in ctg_project_render and no output needs a clamp.  Opacity and depth do not depend on the shading.
 *   Outputs, any subset, at least one: rgb uint8 [L][U][3] = (C[c] + bg_c Tr + 16384) >> 15; opacity uint8 [L][U] =
 *     ((32768 - Tr) 255 + 16384) >> 15; depth int16 [L][U] (2-byte aligned) = the step of the first counted sample at which
 *     32768 - Tr reaches `surface`, -1 if it never does.  A ray that misses the volume gives bg, opacity 0 and depth -1.
 *   Every volume address is bounds-checked or clamped whatever the tables hold, and an uncounted sample reads voxel 0, its gradient
 *   included; the fixed-point sums are unsigned as in ctg_reformat_lines (the caller keeps the same range).  No floating point
 *   enters the gradient: a float square root only seeds the integer one, which is corrected to the exact floor.
 *   Exact integer arithmetic: the same bits as numpy (tests/render_lines_np.py).  One launch, no accumulator, no atomics.
 *   CTG_EINVAL, nothing launched: a null vol, lines or lut; no output; N, H, W, U or T outside 1 .. 4096; L < 1; sampling outside
 *   0 .. 1; stop outside 0 .. 32767; surface outside 1 .. 32768; a bg outside 0 .. 255; zscale outside 1 .. 4096; ambient outside
 *   0 .. 256; gmin2 outside 1 .. 67108864; vol, lut or depth not 2-byte aligned, lines or light not 4-byte aligned; a grid beyond
 *   2^31 - 1 workgroups (L ceil(U / 32)). ---- */
int ctg_render_lines(const short* vol, int N, int H, int W, const int* lines, int L, int U, int T, const unsigned short* lut,
                     int sampling, int stop, int surface, int bg_r, int bg_g, int bg_b, float wc, float ww, int hu,
                     const int* light, int zscale, int ambient, int gmin2, unsigned char* rgb, unsigned char* opacity,
                     short* depth, void* stream);

/* ---- series inference, connected components of the volume (added under ABI 15: purely additive, no existing signature or meaning
 * moves, so the version stays 15): despeckle, keep the K largest components, keep the component a seed voxel lies in -- the cleanup
 * in front of every projection-type display.  cta_gan_amd/infer.py: VolumeComponents, components_volume, root_voxel,
 * SeriesTranslator(components=...); ops.components_label, components_select, components_apply.  The reference has no counterpart.
 * Definitions.  vol = the whole int16 volume [N][H][W] on the device, contiguous, every side in 1 .. 4096 and V = N H W <= 2^31 - 1;
 *   the linear index of a voxel is i = (z H + y) W + x.  A voxel is foreground when lo <= vol[i] <= hi (lo <= hi, both inside int16;
 *   the stored values).  Two foreground voxels are adjacent when max(|dz|, |dy|, |dx|) = 1 and |dz| + |dy| + |dx| <= 1, 2, 3 for
 *   connectivity 6, 18, 26 -- in index space, no aspect -- and a component is a class of the transitive closure.
 * ctg_components_label: labels int32 [V] = -1 on background, otherwise the smallest linear index of the voxel's component (its
 *   root).  stats int32 [8] is zeroed, then [0] = the foreground voxels and [6] = the internal-error flag, which must read 0: it is
 *   set when a union-find walk meets a value that cannot be a parent (every such walk ends at once, inside the array).
 * ctg_components_select: labels as ctg_components_label left them.  sizes int32 [V]: sizes[r] = the voxels of the component with root
 *   r, 0 at every index that is no root.  Candidates are the roots with sizes[r] >= min_voxels and, if S > 0 seeds are given, with
 *   labels[seed] == r for some seed (seeds int32 [S], linear indices; a seed outside 0 .. V - 1 or on background selects nothing
 *   and is counted).  Candidates are ordered by size descending, then root ascending; largest = K > 0 keeps the first K, largest = 0
 *   keeps all.  keep uint8 [V] = 1 at kept roots, 0 elsewhere.  top int32 [ntop][2] = (root, size) of the first ntop kept components
 *   in that order, (-1, 0) beyond the kept count.  sizes and keep are zeroed by the call.  stats [1] = components, [2] = candidates,
 *   [3] = kept components, [4] = kept voxels, [5] = seeds that selected nothing; [0] and [7] are left alone, [6] is set (never
 *   cleared) when a label lies outside -1 .. V - 1 -- such a voxel counts as background.  The library keeps the ranking's pass keys
 *   in device memory of its own, one set per call in rotation: at most 16 calls of ctg_components_select in flight at once.
 * ctg_components_apply: out[i] = vol[i] where labels[i] >= 0 and keep[labels[i]] == 1; `fill` on foreground voxels whose component
 *   is dropped; on background vol[i] with background = 1 (despeckle: only dropped islands are erased) and `fill` with background = 0
 *   (mask: only kept components survive).  level[i] = the 8-bit window level of out[i] + (hu ? 1024 : 0) in (wc, ww), as
 *   ctg_project_finish writes it, in the same pass.  out int16 [V], level uint8 [V], either may be NULL (not both).
 * Nothing allocates or synchronises; no workgroup waits for another; exact integer arithmetic, the same bits as numpy
 *   (tests/components_np.py) whatever the order in which atomics land.
 * CTG_EINVAL, nothing launched: a null required pointer; N, H or W outside 1 .. 4096 or V outside 1 .. 2^31 - 1; lo > hi or either
 *   outside int16; connectivity not 6 / 18 / 26; min_voxels < 1; S < 0, or S > 0 with null seeds; largest or ntop outside 0 .. 64, or
 *   ntop > 0 with null top; fill outside int16; background outside 0 .. 1; vol or out not 2-byte aligned, an int32 array not 4-byte
 *   aligned. ---- */
int ctg_components_label(const short* vol, int N, int H, int W, int lo, int hi, int connectivity, int* labels, int* stats,
                         void* stream);
int ctg_components_select(const int* labels, long V, int min_voxels, const int* seeds, int S, int largest, int ntop, int* sizes,
                          unsigned char* keep, int* top, int* stats, void* stream);
int ctg_components_apply(const short* vol, const int* labels, const unsigned char* keep, long V, int background, int fill, float wc,
                         float ww, int hu, short* out, unsigned char* level, void* stream);

/* ---- series inference, the vessel centreline between clicked voxels (added under ABI 15: purely additive, no existing signature or
 * meaning moves, so the version stays 15): the minimal-cost path through the lumen from a start voxel to up to 64 end voxels, the
 * line a curved reformat is laid along.  cta_gan_amd/infer.py: VolumeCentreline, centreline_volume, SeriesTranslator(centreline=...);
 * ops.centreline_clearance, centreline_field, centreline_trace.  The reference has no counterpart.
 * Definitions.  vol, N, H, W, V, the linear index i = (z H + y) W + x and the foreground lo <= vol[i] <= hi as for the components.
 *   q(d) = (d d zq + 128) >> 8 with zq = aspect^2 in 8.8 fixed point (16 .. 65535; 256 = isotropic).  R = 1 .. 32.
 * ctg_centreline_clearance: clear uint16 [V] = 0 on background, on a foreground voxel min(R^2, min over the background voxels b inside
 *   the volume of dx^2 + dy^2 + q(|dz|)); voxels outside the volume are not background.  (With zq < 128, q(1) = 0: a foreground voxel
 *   above or below background then reads 0 and counts as background from here on.)  scratch uint16 [V], the caller's, not `clear`.
 *   Three launches.
 * The cost field.  steps s0 .. s4, each 1 .. 255: the length of a move to a 26-neighbour by kind -- in-plane face, in-plane edge,
 *   z alone, z + one in-plane axis, z + two.  pen uint16 [R^2 + 1], indexed by clear (a clear above R^2 reads pen[R^2]); what is read
 *   is clamped into 1 .. 4095; pen[0] is never read.  step(u -> v) = steps[kind(v - u)] pen[clear[v]].  A voxel is foreground when
 *   clear > 0.  dist uint32 [V]: 0xFFFFFFFF = unreached, SAT = 0xFFFFFFFE; dist[start] = 0 when start is foreground, otherwise
 *   dist[v] = the cheapest path from start to v through foreground voxels, every partial sum passed through min(., SAT): the least
 *   fixed point, the same bits in whatever order anything lands.
 * ctg_centreline_seed: dist = 0xFFFFFFFF but 0 at start; active int32 [2][tiles], marks int32 [max_rounds] and stats int32 [8] zeroed;
 *   the tile of start marked in active[0].  tiles = ceil(N / 8) ceil(H / 16) ceil(W / 32).  A start outside 0 .. V - 1 or on
 *   background marks nothing and sets stats[0] = 1.
 * ctg_centreline_relax: rounds first_round .. first_round + rounds - 1, one launch each.  In round r a workgroup per tile leaves at
 *   once unless active[r & 1][tile] is set; otherwise it clears that entry, relaxes the tile in LDS until nothing changes (or a fixed
 *   number of sweeps is reached: it then marks itself), writes every lowered voxel back by atomicMin, marks in active[(r + 1) & 1]
 *   every neighbouring tile whose face, edge or corner it lowered and adds the number of its marks to marks[r].  marks[r] == 0 after
 *   rounds 0 .. r: the field has reached its fixed point and later rounds do nothing.  stats is not touched.
 * ctg_centreline_saturated: stats[3] = 1 when a voxel of dist reads SAT (left alone otherwise); for the finished field.
 * ctg_centreline_trace: for each of E ends (int32 linear indices, 1 .. 64) paths int32 [E][max_points]: path[0] = end; from v with
 *   dist[v] > 0 the next voxel is the smallest linear index u among the foreground neighbours with dist[u] reached, dist[u] <
 *   dist[v] and min(dist[u] + step(u -> v), SAT) == dist[v]; the walk ends at dist == 0.  counts int32 [E] = the voxels written (end
 *   first, start last); 0 for an end outside the volume, on background or unreached (stats[1] counts them, the row is all -1); -1
 *   when max_points would be exceeded (stats[2]; the row holds the first max_points voxels); -2 when no such u exists (stats[4], and
 *   the internal-error flag stats[6] = 1, which must read 0: a saturated or foreign field; the row holds the voxels up to there).
 *   Entries beyond the voxels written hold -1.  stats [1], [2], [4] are zeroed by the call, [6] is only ever set.
 * Nothing allocates or synchronises; no workgroup waits for another; every loop that depends on memory has a bound that does not;
 *   exact integer arithmetic, the same bits as numpy (tests/centreline_np.py).
 * CTG_EINVAL, nothing launched: a null pointer; scratch == clear; N, H or W outside 1 .. 4096 or V above 2^31 - 1; lo > hi or either
 *   outside int16; R outside 1 .. 32; zq outside 16 .. 65535; a step outside 1 .. 255; max_rounds outside 1 .. 2^20; first_round < 0,
 *   rounds < 0 or first_round + rounds > max_rounds; E outside 1 .. 64; max_points outside 1 .. 2^24; a 16-bit array not 2-byte
 *   aligned, a 32-bit array not 4-byte aligned. ---- */
int ctg_centreline_clearance(const short* vol, int N, int H, int W, int lo, int hi, int R, int zq, unsigned short* scratch,
                             unsigned short* clear, void* stream);
int ctg_centreline_seed(const unsigned short* clear, int N, int H, int W, long start, unsigned* dist, int* active, int* marks,
                        int max_rounds, int* stats, void* stream);
int ctg_centreline_relax(const unsigned short* clear, int N, int H, int W, const unsigned short* pen, int R, int s0, int s1, int s2,
                         int s3, int s4, unsigned* dist, int* active, int* marks, int max_rounds, int first_round, int rounds,
                         int* stats, void* stream);
int ctg_centreline_saturated(const unsigned* dist, long V, int* stats, void* stream);
int ctg_centreline_trace(const unsigned short* clear, int N, int H, int W, const unsigned short* pen, int R, int s0, int s1, int s2,
                         int s3, int s4, const unsigned* dist, const int* ends, int E, int max_points, int* paths, int* counts,
                         int* stats, void* stream);

/* ---- series inference, the lumen profile along a centreline (added under ABI 15: purely additive, no existing signature or meaning
 * moves, so the version stays 15): at every position of the line the lumen's radius along K rays of the cross-section, from which the
 * host takes area, diameters and the stenosis grade.  cta_gan_amd/infer.py: lumen_lines, lumen_profile, lumen_stenosis, VolumeLumen,
 * lumen_volume, VolumeCentreline(lumen=...), SeriesTranslator(centreline={..., "lumen": ...}); ops.lumen_sections.  The reference has
 * no counterpart.
 * ctg_lumen_sections: vol, N, H, W, the 16.16 positions, the "counted" rule and the value of a sample (sampling 0 = nearest, 1 =
 *   trilinear) are exactly those of ctg_reformat_lines.  lines = int32 [R][K][9] on the device, 4-byte aligned, rows in the format of
 *   ctg_reformat_lines; K = 8, 16, 32 or 64 rays per section, T = 2 .. 256 steps per ray.  Section r has the centre C = (x0, y0, z0) of
 *   its row (r, 0), and ray j the step D_j = (xk, yk, zk) of row (r, j): sample k of ray j lies at C + k D_j.  Nothing else of a row is
 *   read (the host writes the centre into every row and xu = yu = zu = 0).
 *   One walk of a section: s0 = the value at C.  If C is not counted, s0 < lo or s0 > hi: outside = 1, lo_r = lo, every rho_j = 0 and no
 *     ray is open.  Otherwise outside = 0 and lo_r = lo (edge 0, "band") or max(lo, (s0 + base) >> 1) (edge 1, "half": half-way between
 *     the lumen's own density and a background `base` <= lo; arithmetic shift), so lo_r <= s0.  Ray j takes k = 1 .. T-1 in turn with
 *     prev = the value at k-1 (s0 at k = 1) and v = the value at k, and stops at the first k where
 *       the sample is not counted:   rho_j = 256 (k-1), and the ray is open;
 *       else v < lo_r:               rho_j = 256 (k-1) + (256 (prev - lo_r)) / (prev - v);
 *       else v > hi:                 rho_j = 256 (k-1) + (256 (hi - prev)) / (v - prev);
 *     a ray that never stops has rho_j = 256 (T-1) and is open.  lo_r <= prev <= hi holds throughout, so every numerator is >= 0 and
 *     below its denominator: C division is floor and the fraction lies in 0 .. 255.  rho is the lumen's radius along the ray in units of
 *     1 / 256 step, at most 65280.
 *   Recentring, `recentre` = 0 .. 4 times: after a walk with outside = 0 and no open ray the centre moves on each axis a by
 *     (S_a + 64 K) >> (7 + log2 K), S_a = sum_j rho_j D_j[a] in int64, arithmetic shift -- twice the mean boundary point, rounded to
 *     nearest, in the section's plane -- and the section is walked again from there; after any other walk the centre stays and the
 *     section is finished.  What is stored is the last walk's.
 *   Outputs, all on the device: radii int32 [R][K] = rho; cross int64 [R] (8-byte aligned) = sum_j rho_j rho_((j+1) mod K) (the polygon
 *     through the boundary points has the area sin(2 pi / K) / 2 times that); centres int32 [R][3] = the last centre (x, y, z), 16.16 with
 *     the + 0.5 inside like the table; sections int32 [R][8] = sum_j rho_j; dmin and dmax, the least and greatest chord rho_j +
 *     rho_(j+K/2) over j < K/2; jmin and jmax, their rays, the lowest j on a tie; the number of open rays; outside; lo_r.
 *   Every address is bounds-checked or clamped whatever the table holds; the sums are formed in unsigned arithmetic and read as int32, so
 *     the caller keeps |c0| + (1 + 2 recentre) (T-1) max_j |ck_j| < 2^31 on every axis of every section (a move is at most
 *     2 (T-1) max_j |ck_j|; ops.lumen_sections checks it on the host): beyond that the result is defined by the wrapped sums, still
 *     without an access outside the volume.
 *   Exact integer arithmetic: the same bits as numpy (tests/lumen_np.py).  One launch, no accumulator, no atomics.
 *   CTG_EINVAL, nothing launched: a null pointer; N, H or W outside 1 .. 4096; R < 1 or R K above 2^31 - 1; K not 8, 16, 32 or 64; T
 *   outside 2 .. 256; lo > hi or either outside int16; sampling or edge outside 0 .. 1; with edge 1 a base outside -32768 .. lo;
 *   recentre outside 0 .. 4; vol not 2-byte aligned, lines, radii, sections or centres not 4-byte aligned, cross not 8-byte aligned. ---- */
int ctg_lumen_sections(const short* vol, int N, int H, int W, const int* lines, int R, int K, int T, int lo, int hi, int sampling,
                       int edge, int base, int recentre, int* radii, long long* cross, int* sections, int* centres, void* stream);

/* ---- LPIPS (AlexNet, lpips 0.1) of the test() loops (ABI 14): `loss_fn_alex = lpips.LPIPS(net='alex')` (trainer/HdTrainer.py:26-28)
 * and its calls `loss_fn_alex.forward(torch.tensor(c), torch.tensor(b))` on the windowed and on the raw masked pair of every slice
 * (HdTrainer.py:504-513, 531-536, 1029-1031, 1054-1056; the twins in CycTrainer.py, p2pTrainer.py, RegTrainer.py).  The five
 * convolutions run on ctg_im2col_pack / ctg_conv_igemm in fp32; the three entries below are the rest.  fp32 only.
 * ctg_window_pairs: the four masked images ctg_window_metrics reduces, written out: out[4][B][HW] = [c, fake_m, b, real_m]
 *   (HdTrainer.py:1008-1023, 1041-1047), i.e. planes 0 .. 2B-1 the generated side and 2B .. 4B-1 the reference side of 2B pairs;
 *   `aliased` as in ctg_window_metrics, the same per-pixel arithmetic bit for bit.
 * ctg_maxpool3s2_fwd: nn.MaxPool2d(kernel_size=3, stride=2) of torchvision's AlexNet features (no padding, floor): NHWC
 *   [B][H][W][x_ld] -> [B][(H-3)/2+1][(W-3)/2+1][o_ld], C % 4 == 0, 16-byte aligned; equals F.max_pool2d bit for bit.
 * ctg_lpips_layer: one layer's distance (lpips/__init__.py: normalize_tensor, `(feats0 - feats1) ** 2`, NetLinLayer, spatial_average).
 *   f = features [2P][HW][f_ld], images 0 .. P-1 the "x" side and P .. 2P-1 the "y" side; lin[C] the 1x1 weights;
 *   out[p][k] = mean over pixels of sum_c lin[c] (n(x)[c] - n(y)[c])^2, n(v) = v / (sqrt(sum_c v^2) + 1e-10), for out[P][5] doubles and
 *   0 <= k < 5.  C % 64 == 0, 64 <= C <= 384 (CTG_EINVAL beyond).  part = P * 64 doubles of workspace; pixels are summed in fp64 in a
 *   fixed order (no atomics): the same bits on every run. ---- */
int ctg_window_pairs(const float* fake, const float* real, const float* wc, const float* ww, int B, long HW, int aliased,
                     float* out, void* stream);
int ctg_maxpool3s2_fwd(const float* x, int x_ld, float* out, int o_ld, int B, int H, int W, int C, void* stream);
int ctg_lpips_layer(const float* f, int f_ld, const float* lin, int P, long HW, int C, int k, double* part, double* out,
                    void* stream);

/* ---- torch.optim.Adam(lr, betas=(0.5, 0.999)) step over `count` fp32 tensors (HdTrainer.py:612-616,738-739,751;
 * CycTrainer.py:67-73,162,178,197).  Host arrays of device pointers; `step` is 1-based. ---- */
int ctg_adam_step(int count, void* const* params, const void* const* grads, void* const* exp_avg,
                  void* const* exp_avg_sq, const long* numel, float lr, float beta1, float beta2, float eps,
                  int step, const float* dev_state3, void* stream);
/* graph-capturable form: dev_state3 = {step, 1-b1^step, sqrt(1-b2^step)} lives on the device, ctg_adam_tick advances
 * it by one step inside the stream, ctg_adam_step(..., step ignored, dev_state3) reads the corrections from it */
int ctg_adam_tick(float* dev_state3, float beta1, float beta2, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CTAGAN_HIP_H */
