// Internal launcher prototypes (stream-ordered, non-allocating, return DMX_* codes).
#pragma once
#include "dmx_common.h"

#define DMX_GN_MAX_CHUNKS 512

// ---- elementwise.hip
size_t dmx_gn_scratch_floats(int B, int C, int G);
// partial sums of a GroupNorm input left by its producers (EPI_GNSTATS): see gn_parts_kernel (elementwise.hip)
struct GnRegion {
  float* part = nullptr;        // [image][slot][nq][2] fp32
  int tm = 0, P = 0, nq = 0;    // rows per slot; GEMM rows per image of the producing launch; quads per slot row (producer N / 4)
  int qoff = 0, cq = 0;         // first quad of this source in the normalised tensor; real quads of this source (C / 4)
};
struct GnParts { int n = 0; GnRegion r[8]; };
size_t dmx_gn_part_floats(int B, int P, int N);                      // fp32 elements of one region's buffer (worst case: 32-row slots)
int dmx_groupnorm_fwd(const act_t* x, act_t* y, const float* gamma, const float* beta, float* stats, float* scale,
                      float* shift, float* partial, int B, int P, int C, int G, float eps, int silu, hipStream_t st,
                      const GnParts* parts = nullptr);
int dmx_groupnorm_bwd(const act_t* x, const act_t* dy, const act_t* add, act_t* dx, const float* stats,
                      const float* scale, const float* shift, float* k0, float* k1, float* partial, int B, int P, int C,
                      int G, int silu, hipStream_t st, const GnParts* parts = nullptr);
int dmx_layernorm_fwd(const act_t* x, act_t* y, const float* gamma, const float* beta, int rows, int C, float eps,
                      hipStream_t st);
int dmx_softmax_fwd(const float* S, act_t* P, const float* colbias, long long rows, int N, long long lds, long long ldp,
                    int rows_per_bias, hipStream_t st);
int dmx_softmax_act(const act_t* S, act_t* P, const float* colbias, long long rows, int N, long long ldp, int rows_per_bias,
                    hipStream_t st);
int dmx_rowdot(const act_t* a, const act_t* b, float* out, long long rows, int C, long long lda, long long ldb, hipStream_t st);
int dmx_geglu(const act_t* x, act_t* y, long long rows, int I, hipStream_t st);
int dmx_silu(const act_t* x, act_t* y, long long n, hipStream_t st);
int dmx_upsample_nearest(const act_t* x, act_t* y, int B, int Hi, int Wi, int Ho, int Wo, int C, hipStream_t st);
int dmx_upsample2x_bwd(const act_t* dy, act_t* dx, int B, int Hi, int Wi, int C, hipStream_t st);
int dmx_transpose(const act_t* in, act_t* out, int R, int C, long long ldi, long long ldo, int Z, int Zi, long long sIo,
                  long long sIi, long long sOo, long long sOi, hipStream_t st);
int dmx_concat2(const act_t* a, const act_t* b, act_t* dst, long long rows, int Ca, int Cb, hipStream_t st);
int dmx_copy_channels(const act_t* src, act_t* dst, long long rows, int C, int lds, int ldd, int soff, int doff,
                      hipStream_t st);
int dmx_axpby(const act_t* x, const act_t* y0, act_t* y, float a, float b, long long n, hipStream_t st);
int dmx_nchw_f32_to_nhwc_bf16(const float* x, act_t* y, int B, int C, int HW, int Cp, float scale, hipStream_t st);
int dmx_nhwc_bf16_to_nchw_f32(const act_t* x, float* y, int B, int C, int HW, int Cp, float scale, hipStream_t st);
int dmx_f32_to_bf16(const float* x, act_t* y, long long n, float scale, hipStream_t st);
int dmx_bf16_to_f32(const act_t* x, float* y, long long n, float scale, hipStream_t st);
int dmx_extract_col(const act_t* x, float* y, long long rows, int ld, int col, hipStream_t st);
int dmx_gather_col_f32(const float* x, float* y, long long rows, int ld, int col, hipStream_t st);
int dmx_tanh_bwd_pad8(const float* dwav, const float* wav8, act_t* gz, long long rows, hipStream_t st);
// the same two for clips of T samples whose samples [s0, s1) are dead: zeros there by select, x / wav8 not read
int dmx_gather_col_f32_dead(const float* x, float* y, long long rows, int ld, int col, int T, int s0, int s1, hipStream_t st);
int dmx_tanh_bwd_pad8_dead(const float* dwav, const float* wav8, act_t* gz, long long rows, int T, int s0, int s1, hipStream_t st);
int dmx_scatter_col_pad8(const float* v, act_t* y, long long rows, float scale, hipStream_t st);
int dmx_gather_col_f32_to_act(const float* x, act_t* y, long long rows, int ld, int col, hipStream_t st);
int dmx_pad_col8_act(const act_t* v, act_t* y, long long rows, hipStream_t st);
int dmx_timestep_embed(const float* t, act_t* y, int B, int dim, hipStream_t st);

// ---- flash_attn.hip (forward-only fused attention for the U-Net)
bool dmx_flash_attn_ok(int dh, int C);
int dmx_flash_attn_fwd(const act_t* q, const act_t* k, const act_t* v, act_t* o, const float* colbias, int B, int Nq, int Nk,
                       int C, int heads, float scale, hipStream_t st, int ldq = 0, int ldk = 0, int ldv = 0, int* qt_out = nullptr);

// ---- mel.hip (STFT / mel measurement path, fp32)
int dmx_stft_tables(float* table, float* tableT, int n_fft, int bins, int Npad, int Kpad, int hann, hipStream_t st);
int dmx_stft_fwd(const float* wav, long long wav_stride, const float* table, float* X, int B, int L, int T, int n_fft, int hop, int Npad,
                 hipStream_t st);
int dmx_stft_bwd_frames(const float* Y, const float* tableT, float* dframe, int M, int n_fft, int Kpad, hipStream_t st);
int dmx_mel_fwd(const float* X, const float* fb, float* mel_lin, float* mel_out, int rows, int ldx, int bins, int n_mels, int power2,
                int to_db, float lo, float hi, hipStream_t st);
int dmx_mel_bwd(const float* X, const float* fb, const float* mel_lin, const float* dmel, float* Y, int rows, int ldx, int ldy, int bins,
                int n_mels, int power2, int to_db, float lo, float hi, hipStream_t st);
int dmx_stft_mag(const float* X, float* mag, int B, int T, int bins, int ldx, hipStream_t st);
int dmx_stft_mag_bwd(const float* X, const float* dmag, float* Y, int B, int T, int bins, int ldx, int ldy, hipStream_t st);
int dmx_overlap_add(const float* dframe, float* dwav, long long out_stride, int B, int T, int L, int n_fft, int hop, int accumulate,
                    hipStream_t st);
int dmx_l2_loss_grad(const float* ref, const float* pred, float* loss, float* dpred, int B, long long n, long long ref_stride, float gscale,
                     hipStream_t st);
int dmx_mask_mul(const float* x, long long xs, const float* mask, float* y, long long ys, int B, int L, int Ly, hipStream_t st);
int dmx_melscale(const float* mag, const float* fb, float* mel, int B, int T, int bins, int n_mels, float lo, float hi, hipStream_t st);
int dmx_absmax_normalize(float* x, float* inv_scale, int B, long long n, float target, hipStream_t st);

// ---- stft_mel.hip (fused STFT -> mel -> dB [-> L2] and its backward; n_fft = 1024, 64 mel columns)
struct DmxStftMelTables {
  const float2* tw;     // exp(-2 pi i m / 1024)
  const float* win;     // analysis window
  const int *klo, *klen; const float* fbc; int kmax;     // per mel column: first bin, bin count, weights [i][64]
  const int *mlo, *mlen; const float* fbr; int mmax;     // per bin: first mel column, column count, weights [i][576]
};
int dmx_stft_mel_parts(int L, int hop);                  // workgroups per clip of the forward launch (= partial sums per clip)
int dmx_stft_mel_fwd(const DmxStftMelTables& t, const float* wav, long long wav_stride, const float* mask, const float* ref, long long ref_stride,
                     float* mel_out, float* partial, int B, int L, int hop, int power2, int to_db, float lo, float hi, hipStream_t st,
                     const float* add = nullptr, long long add_stride = 0, const float* addmag = nullptr, float nscale = 0.f,
                     const float* thr = nullptr);
int dmx_stft_mel_bwd(const DmxStftMelTables& t, const float* wav, long long wav_stride, const float* mask, const float* ref, long long ref_stride,
                     const float* dmel, const float* partial, float gscale, float* loss, float* dwav, long long dwav_stride, int Lfull,
                     int accumulate, int B, int L, int hop, int power2, int to_db, float lo, float hi, hipStream_t st,
                     const float* add = nullptr, long long add_stride = 0, const float* addmag = nullptr, float nscale = 0.f,
                     const float* thr = nullptr);
// measurement noise: sample-domain `add` (B, >= L; row stride add_stride) enters as wav * mask + nscale * add, magnitude-domain `addmag`
// (B, 513, frames; power2 = 0 only) as |X| + nscale * addmag, in the forward and in the backward's recomputation alike;
// hard clipping: thr (B) per-clip thresholds c > 0, y = min(max(wav * mask, -c), c) + nscale * add, gradient through -c <= wav * mask <= c only

// ---- tf_gain.hip (time-frequency gain: STFT at hop 256 with zero extension, real gain per bin and frame, inverse STFT; n_fft = 1024, Hann)
int dmx_tf_gain_frames(int L);                           // ceil(L / 256) + 3
// out[b, 0:L] = A(x[b, 0:L]), +0 on [L, full); gain (T, 513) rows per clip, clip stride 0 = one grid for every clip; uses t.tw and t.win
// gain_frame_stride: 513 = a grid, 0 = one 513-row per clip that every frame reads (clip stride then 0 or >= 513)
int dmx_tf_gain(const DmxStftMelTables& t, const float* x, long long x_stride, const float* gain, long long gain_clip_stride,
                long long gain_frame_stride, float* out, long long out_stride, int B, int L, int full, hipStream_t st);

// ---- mdct_quant.hip (codec restoration: MDCT at N = 512 with zero extension and the sine window, a per-coefficient map, the transpose)
struct DmxMdctTables {
  const float2* tw;     // exp(-2 pi i m / 1024), the FFT's (the table of DmxStftMelTables)
  const float2* pre;    // exp(-i pi n / 1024), n = 0 .. 1023
  const float2* post;   // exp(-i pi 256.5 (k + 1/2) / 512), k = 0 .. 511
  const float* win;     // sin(pi (n + 1/2) / 1024)
};
constexpr int DMX_MDCT_QUANT = 0, DMX_MDCT_PASS = 1, DMX_MDCT_PROJECT = 2;
int dmx_mdct_num_frames(int L);                          // ceil(L / 512) + 1
// out[b, 0:L] = Phi^T f(Phi x[b, 0:L]), +0 on [L, full); step (T, 512) rows per clip, clip stride 0 = one grid for every clip;
// codes (B, T, 512) int32: QUANT writes them when given, PROJECT reads them, PASS ignores them
int dmx_mdct_run(const DmxMdctTables& t, const float* x, long long x_stride, const float* step, long long step_clip_stride, int* codes, float* out,
                 long long out_stride, int B, int L, int full, int mode, hipStream_t st);

// ---- tf_eq.hip (blind equalisation: the gradient of a loss in a time-invariant gain curve g[513], and its Adam + projection update)
int dmx_tf_wgrad_segments(int L);                        // ceil(frames / 16)
// part[b, seg, 0:513] = the terms of frames [16 seg, 16 seg + 16) of dg[b, k] = (h_k / 1536) sum_t Re(X[k, t] conj(U[k, t])); uses t.tw, t.win
int dmx_tf_wgrad(const DmxStftMelTables& t, const float* x, long long x_stride, const float* dy, long long dy_stride, float* part, int B, int L,
                 hipStream_t st);

// ---- drc.hip (dynamic-range compression at block rate and the transpose of its Jacobian; three launches per direction).  Like
// waveshape.hip it needs no handle: its launchers are the C ABI's own dmx_drc_fwd / dmx_drc_bwd (include/diffmusic_hip.h)
constexpr int DMX_DRC_BLOCK = 64;                        // samples per sidechain block; state (B, 3, H) and tape (B, H), H = ceil(L / 64)

// ---- drc_fit.hip (blind de-compression: the gradient of a loss in the compressor's parameters as one row of five per segment of 256
// blocks, and the Adam + box update of a clip's parameters with its table row; one launch each).  No handle either: its launchers are the
// C ABI's own dmx_drc_pgrad / dmx_drc_update; the level and the static curve are drc.hip's, from drc_common.h
constexpr int DMX_DRC_FIT_SEGMENT = 256;                 // blocks per partial row; part (B, ceil(H / 256), 5)
constexpr int DMX_DRC_FIT_PARAMS = 5;                    // T, k, makeup, ln aA, ln aR

// ---- warp.hip (wow and flutter: a clip read along a given delay curve, four-point Catmull-Rom, and the transpose as a gather; one launch
// per direction).  Like waveshape.hip it needs no handle: its launchers are the C ABI's own dmx_warp_fwd / dmx_warp_bwd
constexpr int DMX_WARP_BLOCK = 64;                       // samples per knot interval; a curve is H + 1 knots, H = ceil(L / 64)

// ---- warp_fit.hip (blind wow and flutter: the gradient of a loss in the knots of the delay curve as one pair per block, and the Adam +
// projection update of a coarse curve with its expansion into the fine one; one launch each).  No handle either: its launchers are the C
// ABI's own dmx_warp_wgrad / dmx_warp_update; the position arithmetic is warp.hip's, from warp_common.h

// ---- declick.hip (declicking: the autoregressive click detector, the dilation of its flags into a per-clip sample mask, the per-clip mask
// product and the output blend; one launch each).  No handle: its launchers are the C ABI's own dmx_click_detect / dmx_click_mask /
// dmx_mask_rows / dmx_declick_blend
constexpr int DMX_CLICK_FRAME = 1024;                    // samples per frame; a (B, F, 16), sigma (B, F), F = ceil(L / 1024)
constexpr int DMX_CLICK_ORDER = 16;                      // order of the autoregressive model
constexpr int DMX_CLICK_MAX_GUARD = 64;                  // largest guard (click_mask) and fade (declick_blend)

// ---- sched.hip
int dmx_pred_x0(const float* x, const float* eps, float* x0, long long n, float sqrt_a, float sqrt_1ma, hipStream_t st);
int dmx_pred_x0_ex(const float* x, const float* m, float* x0, long long n, float sqrt_a, float sqrt_1ma, int ptype, float clip_r, hipStream_t st);
int dmx_cfg_combine(const float* eps2, float* out, long long n, float scale, hipStream_t st);
int dmx_sched_update(int mode, const float* x, const float* eps, const float* x0, const float* g0, const float* inv_scale,
                     const float* noise, float* prev, float* x0_out, float* grad_out, int B, int n, float alpha_t, float alpha_prev,
                     float sigma, float rate, float eps_small, int global_norm, hipStream_t st, int ptype = 0, float clip_r = 0.f);
