/* diffmusic_hip.h -- C ABI of the MI355X-native DiffMusic hot-path library (libdiffmusic_hip.so).
 *
 * The reference (jwliao1209/DiffMusic) is pure Python and has no FFI layer; its boundary for this
 * path is three duck-typed protocols: Scheduler.step()
 * (diffmusic/schedulers/scheduling_dps.py:137-219 and siblings), Pipeline.__call__()
 * (diffmusic/pipelines/pipeline_musicldm.py:491-799) and BaseOperator
 * (diffmusic/inverse_problem/operator.py:6-14).  The Python facade in diffmusic_amd/ keeps those
 * protocols and binds the entry points below with ctypes (INTEGRATION.md shows the stub a
 * maintainer of the reference would add).  Each entry point cites the reference call site whose
 * third-party / PyTorch computation it replaces.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless the name ends in _host; tensors are contiguous;
 *  - `stream` is a hipStream_t passed as void*; calls are stream-ordered, never synchronise and
 *    never allocate (model creation / parameter loading / finalize excepted);
 *  - workspaces are caller-owned device buffers; query sizes with the *_workspace_bytes calls;
 *  - return value 0 = OK, negative = error (dmx_last_error() gives the message);
 *  - 16-bit activation tensors (`uint16_t*`) are raw fp16 bit patterns (bf16 when the library was
 *    built with -DDMX_BF16; query dmx_act_dtype()), channels-last.
 */
#ifndef DIFFMUSIC_HIP_H
#define DIFFMUSIC_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Additive changes do not bump the version: dmx_audio_guidance_{fwd,bwd}_ex and dmx_noise_add (measurement noise inside the guided
 * step), dmx_vae_encoder_* / dmx_vae_encode_fwd / dmx_latent_init / dmx_conv2d_raw (VAE encoder, warm-started sampling),
 * dmx_track_stitch_fwd / dmx_track_stitch_bwd (track mode: overlapping windows as one sample) and dmx_audio_guidance_{fwd,bwd}_shaped /
 * dmx_clip_fwd / dmx_clip_bwd / dmx_declip_project (declipping: a hard clip inside and beside the guidance pair) and dmx_fir_clip_fwd /
 * dmx_fir_clip_bwd / dmx_fir_wgrad / dmx_fir_wgrad_workspace_floats / dmx_ir_update (blind dereverberation: one fitted response per clip)
 * and dmx_stem_mix_fwd / dmx_stem_mix_bwd / dmx_stem_project (source separation: the stems of a mixture as the batch) and dmx_audio_tf_gain /
 * dmx_audio_tf_frames (time-frequency masking: a real gain on the STFT) and dmx_audio_tf_curve / dmx_audio_tf_wgrad /
 * dmx_audio_tf_wgrad_segments / dmx_audio_eq_update (blind equalisation: a fitted gain curve per clip) and dmx_drc_fwd / dmx_drc_bwd
 * (de-compression: a dynamic-range compressor and the transpose of its Jacobian) and dmx_warp_fwd / dmx_warp_bwd (wow and flutter: a clip
 * read along a delay curve, and the transpose) and dmx_warp_wgrad / dmx_warp_update (blind wow and flutter: the delay curve fitted) and dmx_drc_fwd_p / dmx_drc_bwd_p / dmx_drc_pgrad /
 * dmx_drc_update (blind de-compression: the compressor's parameters per clip on the device, and fitted) and dmx_click_detect /
 * dmx_click_mask / dmx_mask_rows / dmx_declick_blend (declicking: a click detector and per-clip sample masks) and dmx_mdct_frames / dmx_mdct_quant /
 * dmx_mdct_project (codec restoration: an MDCT quantiser, its straight-through transpose and its cell projection) are new symbols, and every earlier entry point keeps its signature.  A binding that meets a version-4 library without them names the missing
 * symbol and asks for a rebuild. */
#define DMX_ABI_VERSION 4   /* 4: dmx_htsat_* / dmx_gram_* (CLAP HTS-AT audio tower of the style-guidance operator).  Earlier:  2: dmx_flash_attn_raw takes row-major V (ld = ldv) instead of per-head V^T; GemmDesc grew.  3: GemmDesc grew (EPI_LNFOLD / EPI_ROWSTATS / EPI_GNSTATS / EPI_GNBWD: colsum, ln_eps, rowstats_in, rowstats_out, nslots, gn_part, gnb_*) */
#define DMX_MAX_STAGES 8

typedef struct dmx_model dmx_model; /* opaque network handle (weights repacked for MFMA) */

/* transformers SpeechT5HifiGanConfig fields used by the vocoder (operator.py:126-130 call site) */
typedef struct dmx_hifigan_config {
  int model_in_dim;             /* 64 */
  int upsample_initial_channel; /* 1024 */
  int num_upsamples;            /* 5 */
  int upsample_rates[DMX_MAX_STAGES];
  int upsample_kernel_sizes[DMX_MAX_STAGES];
  int num_kernels;              /* 3 */
  int resblock_kernel_sizes[DMX_MAX_STAGES];
  int num_dilations;            /* 3 */
  int resblock_dilation_sizes[DMX_MAX_STAGES * DMX_MAX_STAGES]; /* [kernel][dilation] */
  float leaky_relu_slope;       /* 0.1 */
} dmx_hifigan_config;

/* diffusers AutoencoderKL decoder config (scheduling_dps.py:195-197 call site) */
typedef struct dmx_vae_config {
  int latent_channels;          /* 8 */
  int out_channels;             /* 1 */
  int num_blocks;               /* 3 */
  int block_out_channels[DMX_MAX_STAGES]; /* 128,256,512 */
  int layers_per_block;         /* 2 */
  int norm_num_groups;          /* 32 */
  float eps;                    /* 1e-6 */
} dmx_vae_config;

/* diffusers UNet2DConditionModel config as used by MusicLDM (pipeline_musicldm.py:696-703) and,
 * with cross_attention contexts, AudioLDM2 (plpeline_audioldm2.py:1147-1154) */
typedef struct dmx_unet_config {
  int in_channels, out_channels; /* 8, 8 */
  int num_blocks;                /* 4 */
  int block_out_channels[DMX_MAX_STAGES];
  int layers_per_block;          /* 2 */
  int attention_heads;           /* 8 */
  int norm_num_groups;           /* 32 */
  int down_attn[DMX_MAX_STAGES]; /* 0,1,1,1 */
  int up_attn[DMX_MAX_STAGES];   /* 1,1,1,0 */
  int class_embed_dim;           /* 512 (simple_projection, concat) ; 0 = none */
  int num_attn_per_layer;        /* MusicLDM 1 ; AudioLDM2 3 (one Transformer2DModel per cross_attention_dim entry) */
  int attn_cross_dims[4];        /* per transformer: <= 0 self-attention (context None), > 0 cross-attention width;
                                    the k-th positive entry attends context k (AudioLDM2: {0, 768, 1024}) */
} dmx_unet_config;

int dmx_abi_version(void);
int dmx_act_dtype(void); /* 1 = fp16 (default build), 0 = bf16 */
const char* dmx_last_error(void);

/* ---- model lifecycle ------------------------------------------------------------------------ */
dmx_model* dmx_hifigan_create(const dmx_hifigan_config* cfg);
dmx_model* dmx_vae_decoder_create(const dmx_vae_config* cfg);
dmx_model* dmx_unet_create(const dmx_unet_config* cfg);
void dmx_model_destroy(dmx_model* m);
int dmx_model_num_params(const dmx_model* m);
const char* dmx_model_param_name(const dmx_model* m, int i);
size_t dmx_model_param_numel(const dmx_model* m, int i);
int dmx_model_param_ndim(const dmx_model* m, int i);
int dmx_model_param_dim(const dmx_model* m, int i, int d);
/* copy one fp32 parameter (upstream naming, e.g. "resblocks.3.convs1.0.weight") from host memory */
int dmx_model_load_param(dmx_model* m, const char* name, const float* data_host, size_t numel);
/* repack all parameters into the MFMA layouts; fails if any parameter is missing */
int dmx_model_finalize(dmx_model* m, void* stream);

/* ---- HiFi-GAN vocoder: replaces `vocoder(mel)` (operator.py:126-130) and its autograd backward */
int dmx_hifigan_out_len(const dmx_model* m, int frames);
size_t dmx_hifigan_workspace_bytes(dmx_model* m, int batch, int frames);
/* mel (B, frames, model_in_dim) f16 -> wav (B, out_len) fp32; keeps the backward state in ws */
int dmx_hifigan_fwd(dmx_model* m, const uint16_t* mel, float* wav, int batch, int frames, void* ws, size_t ws_bytes,
                    void* stream);
/* dwav (B, out_len) fp32 -> dmel (B, frames, model_in_dim) f16; ws as left by the forward call */
int dmx_hifigan_bwd(dmx_model* m, const float* dwav, uint16_t* dmel, void* stream);
/* The same forward for a caller whose loss never looks at the output samples [s0, s1) of any clip (an inpainting hole) and whose
   dwav is exactly zero there: wav comes back 0.0f on the span and bit-equal to dmx_hifigan_fwd elsewhere, and the dmx_hifigan_bwd call
   that follows returns the dmel of the plain pair (whatever dwav holds on the span is taken as zero).  In between, the narrow
   stages run no work for the rows that reach only the span.  A span too short to save a whole slab of rows anywhere (or s1 <= s0)
   makes this call dmx_hifigan_fwd. */
int dmx_hifigan_fwd_dead(dmx_model* m, const uint16_t* mel, float* wav, int batch, int frames, int s0, int s1, void* ws,
                         size_t ws_bytes, void* stream);
/* What the last forward call skipped, per upsampling stage (n = capacity of the arrays, any of them may be NULL): pair-kernel slabs
   per clip skipped / in all over the stage's forward and backward launches, and the dead rows [lo, hi) of the stage's output.  All
   zero after a plain forward or for a stage that skips nothing.  Returns the number of stages, or -1. */
int dmx_hifigan_dead_plan(dmx_model* m, int* skipped, int* total, int* lo, int* hi, int n);
/* Host arithmetic of that plan for ONE layer (no GPU): the input rows [*lo, *hi) of a 1-D convolution (kernel k, dilation, padding,
   stride 1) or transposed convolution (stride) that feed only the output rows [a, b); t_in / t_out are the two lengths. */
int dmx_conv_dead_rows(int k, int dil, int pad, int stride, int transposed, int t_in, int t_out, int a, int b, int* lo, int* hi);

/* ---- VAE decoder: replaces `vae.decode(z).sample` (scheduling_dps.py:195-197) + backward ------- */
size_t dmx_vae_workspace_bytes(dmx_model* m, int batch, int h, int w);
/* z (B, latent_channels, h, w) fp32 NCHW, multiplied by z_scale -> mel (B, 4h, 4w) f16 (+ fp32 copy if mel_f32) */
int dmx_vae_decode_fwd(dmx_model* m, const float* z, float z_scale, uint16_t* mel, float* mel_f32, int batch, int h, int w,
                       int keep_state, void* ws, size_t ws_bytes, void* stream);
/* dmel (B, 4h, 4w) f16 -> dz (B, latent_channels, h, w) fp32 NCHW, multiplied by z_scale */
int dmx_vae_decode_bwd(dmx_model* m, const uint16_t* dmel, float z_scale, float* dz, void* stream);

/* ---- VAE encoder: `vae.encode(x).latent_dist` of diffusers AutoencoderKL (the vendored pipeline_stable_audio.py:477 call site), forward
 * only.  Same config struct as the decoder (the input has `out_channels` channels, 1 for both models); parameter names are the
 * checkpoint's "encoder. ..." and "quant_conv. ..." tensors.  batch <= 64; frames and bins positive multiples of 2^(num_blocks-1);
 * latent_channels a multiple of 4. ------------------------------------------------------------------------------------------------- */
dmx_model* dmx_vae_encoder_create(const dmx_vae_config* cfg);
size_t dmx_vae_encoder_workspace_bytes(dmx_model* m, int batch, int frames, int bins);   /* 0: unsupported shape (dmx_last_error()) */
/* mel (B, frames, bins) fp32, one channel (the vocoder's input layout); log_floor > 0: ln(max(mel, log_floor)) is taken on load ->
 * moments (B, h * w, 2 * latent_channels) fp32 channels-last = [mean | logvar] before the clamp, h = frames / s, w = bins / s */
int dmx_vae_encode_fwd(dmx_model* m, const float* mel, float log_floor, float* moments, int batch, int frames, int bins, void* ws,
                       size_t ws_bytes, void* stream);
/* moments (B, hw, 2L) -> mean, logvar (B, L, hw) fp32 NCHW, logvar clamped to [-30, 20] (DiagonalGaussianDistribution) and, when x != NULL,
 * x = sqrt_abar * scaling_factor * (mean + exp(0.5 logvar) * eps) + sqrt_1m_abar * noise  (B, L, hw): the start latent of a warm-started
 * trajectory.  eps, noise (B, L, hw) fp32; eps NULL = posterior mode, noise NULL = no noise term. */
int dmx_latent_init(const float* moments, float* mean, float* logvar, float* x, const float* eps, const float* noise, int batch,
                    int latent_channels, int hw, float sqrt_abar, float scaling_factor, float sqrt_1m_abar, void* stream);

/* ---- U-Net forward: replaces `self.unet(latent_model_input, t, ..., class_labels=...)` -------- */
size_t dmx_unet_workspace_bytes(dmx_model* m, int batch, int h, int w);
/* x (B, in_ch, h, w) fp32 NCHW, t (B) fp32 timesteps, class_labels (B, class_embed_dim) fp32 -> eps (B, out_ch, h, w) fp32 */
int dmx_unet_fwd(dmx_model* m, const float* x, const float* t, const float* class_labels, float* eps, int batch, int h,
                 int w, void* ws, size_t ws_bytes, void* stream);
/* AudioLDM2 variant (plpeline_audioldm2.py:1147-1154): ctx0 (B, n0, d0) = generated_prompt_embeds (GPT-2), ctx1 (B, n1, d1) =
 * prompt_embeds (T5), bias1 (B, n1) additive score bias = (1 - attention_mask) * -10000; all fp32; n0, n1 multiples of 4 */
int dmx_unet_fwd_ctx(dmx_model* m, const float* x, const float* t, const float* class_labels, const float* ctx0, int n0,
                     const float* ctx1, int n1, const float* bias1, float* eps, int batch, int h, int w, void* ws,
                     size_t ws_bytes, void* stream);
size_t dmx_unet_workspace_bytes_ctx(dmx_model* m, int batch, int h, int w, int n0, int n1);

/* ---- CLAP HTS-AT audio tower (transformers ClapAudioModel; `StyleGuidanceOperator.transform`, diffmusic/inverse_problem/operator.py:253-271,
 * config 5 of BASELINE.json): forward with tape and input-gradient backward, hand-written like the three networks above.  Parameter names
 * are the `ClapAudioModel.state_dict()` keys ("audio_encoder. ..."). ---------------------------------------------------------------------- */
typedef struct dmx_htsat_config {
  int spec_size;      /* 256: side of the mel "image" */
  int num_mel_bins;   /* 64 */
  int patch_size;     /* 4 (= stride) */
  int embed_dim;      /* 96 */
  int window_size;    /* 8 */
  int num_stages;     /* 4 (0: the input stage and the final LayerNorm alone, for tests of the input stage) */
  int depths[4];      /* 2, 2, 6, 2 */
  int num_heads[4];   /* 4, 8, 16, 32 (head dim 24 in every stage) */
  float ln_eps;       /* 1e-5 */
  float bn_eps;       /* 1e-5 */
} dmx_htsat_config;
dmx_model* dmx_htsat_create(const dmx_htsat_config* cfg);
/* tokens x channels of the feature map dmx_htsat_fwd returns (64 x 768 for the default configuration) */
int dmx_htsat_feature_dims(dmx_model* m, int* tokens, int* channels);
size_t dmx_htsat_workspace_bytes(dmx_model* m, int batch, int frames);      /* forward tape + backward scratch */
/* mel (B, frames, num_mel_bins) fp32 log-mel (ClapFeatureExtractor's input_features without the channel axis), 2 <= frames <= 1024 ->
 * feat (B, tokens, channels) fp32 = the tower's last_hidden_state (after the final LayerNorm), tokens in grid order.  keep_state != 0
 * keeps the tape in `ws` for dmx_htsat_bwd.  The first call with a new `frames` builds that length's bicubic tables (allocates). */
int dmx_htsat_fwd(dmx_model* m, const float* mel, int batch, int frames, float* feat, int keep_state, void* ws, size_t ws_bytes, void* stream);
/* dfeat (B, tokens, channels) fp32 -> dmel (B, frames, num_mel_bins) fp32, multiplied by scale[b] when scale != NULL (the inverse of a
 * per-clip normalisation the caller applied to dfeat: the sweep runs in 16 bits). */
int dmx_htsat_bwd(dmx_model* m, const float* dfeat, const float* scale, float* dmel, void* stream);
/* test hook: copies a tape tensor of the last dmx_htsat_fwd(keep_state = 1) into dst (16-bit activations, token-major): which = 0 block
 * input, 1 q|k|v, 2 hidden state after attention, 3 MLP pre-activation; block == the stage's depth: the stage output before patch merging.
 * Returns the tensor's element count (0: no such tensor); copies only when dst_elems is at least that. */
size_t dmx_htsat_tape_raw(dmx_model* m, int stage, int block, int which, void* dst, size_t dst_elems, void* stream);
/* Gram matrix of token features: G[b] = F[b]^T F[b] / T, F (B, T, C) fp32 -> G (B, C, C); and dF = F (dG + dG^T) / T */
int dmx_gram_fwd(const float* F, float* G, int batch, int tokens, int channels, void* stream);
int dmx_gram_bwd(const float* F, const float* dG, float* dF, int batch, int tokens, int channels, void* stream);

/* ---- STFT / mel measurement path (fp32): replaces torchaudio MelSpectrogram + AmplitudeToDB / MelScale and
 * torch.stft as used by the operators (diffmusic/inverse_problem/operator.py:23-33,143-147,162-170) and the
 * autograd sweep through them (diffmusic/schedulers/scheduling_dps.py:202-212) ------------------------------- */
typedef struct dmx_audio dmx_audio;
/* fb_host: (n_fft/2+1, n_mels) fp32 mel filterbank in host memory; window_hann: 1 = periodic hann, 0 = rectangular */
dmx_audio* dmx_audio_create(int n_fft, int hop, int n_mels, int window_hann, const float* fb_host);
void dmx_audio_destroy(dmx_audio* a);
int dmx_audio_num_frames(const dmx_audio* a, int L);
int dmx_audio_num_bins(const dmx_audio* a); /* n_fft / 2 + 1 */
size_t dmx_audio_state_bytes(const dmx_audio* a, int batch, int L);
/* wav (B, L) fp32 (row stride wav_stride) -> mel_out (B, frames, n_mels) fp32.  power2: |X|^2 (1) or |X| (0);
 * to_db: 10*log10(max(.,1e-10)); then clamp(lo, hi).  `state` keeps what the backward call needs (the spectrum on the dense-DFT path,
 * a copy of the waveform on the fused n_fft = 1024 path). */
int dmx_audio_transform_fwd(dmx_audio* a, const float* wav, long long wav_stride, float* mel_out, void* state, int batch, int L,
                            int power2, int to_db, float lo, float hi, void* stream);
/* dmel (B, frames, n_mels) -> dwav (B, L) (row stride dwav_stride), same flags as the forward call */
int dmx_audio_transform_bwd(dmx_audio* a, const float* dmel, float* dwav, long long dwav_stride, void* state, int batch, int L,
                            int power2, int to_db, float lo, float hi, int accumulate, void* stream);
/* Fused guidance pair for n_fft = 1024 (dmx_audio_is_fused): everything between the vocoder output and its gradient in one forward and
 * one backward launch -- y = wav * mask (mask NULL: y = wav; MusicInpaintingOperator.forward, operator.py:132-133), transform(y) as
 * above (operator.py:23-33 / :143-147), loss[b] = ||ref[b] - transform(y[b])||_2 (torch.linalg.norm, scheduling_dps.py:205-211) and
 * dwav = gscale * d loss / d wav (torch.autograd.grad, scheduling_dps.py:212), written for samples [0, L) and zeroed on [L, Lfull).
 * ref: (B or 1, frames, n_mels) with row stride ref_stride elements per clip (0 = one reference for all clips).  The spectrum is never
 * stored: the backward launch recomputes it from wav.  `state` carries the per-workgroup partial sums of the loss from _fwd to _bwd
 * (same stream).  mel_out may be NULL.  Returns DMX_ERR_SHAPE for handles / lengths the fused kernels do not cover. */
int dmx_audio_is_fused(const dmx_audio* a, int L);
int dmx_audio_guidance_fwd(dmx_audio* a, const float* wav, long long wav_stride, const float* mask, const float* ref, long long ref_stride,
                           float* mel_out, void* state, int batch, int L, int power2, int to_db, float lo, float hi, void* stream);
int dmx_audio_guidance_bwd(dmx_audio* a, const float* wav, long long wav_stride, const float* mask, const float* ref, long long ref_stride,
                           float gscale, float* loss, float* dwav, long long dwav_stride, int Lfull, void* state, int batch, int L,
                           int power2, int to_db, float lo, float hi, void* stream);
/* The same pair with the measurement noise of the step (the `self.noiser(...)` that ends every operator's forward, operator.py:132-133,
 * :170-171 ...; noise.py:13-18), as standard-normal draws z scaled by noise_scale = sigma inside the kernels:
 *   add    (batch, >= L) fp32, row stride add_stride, sample domain:     y = wav * mask + noise_scale * add
 *   addmag (batch, n_fft/2+1, frames) fp32, power2 = 0 only:             |STFT(y)| + noise_scale * addmag
 * Either may be NULL (both NULL = dmx_audio_guidance_{fwd,bwd}, which are these calls with NULLs).  The noise does not depend on wav, so
 * it has no backward term; _bwd_ex must be given the pointers _fwd_ex saw, because it recomputes the forward. */
int dmx_audio_guidance_fwd_ex(dmx_audio* a, const float* wav, long long wav_stride, const float* mask, const float* ref, long long ref_stride,
                              float* mel_out, void* state, int batch, int L, int power2, int to_db, float lo, float hi, const float* add,
                              long long add_stride, const float* addmag, float noise_scale, void* stream);
int dmx_audio_guidance_bwd_ex(dmx_audio* a, const float* wav, long long wav_stride, const float* mask, const float* ref, long long ref_stride,
                              float gscale, float* loss, float* dwav, long long dwav_stride, int Lfull, void* state, int batch, int L,
                              int power2, int to_db, float lo, float hi, const float* add, long long add_stride, const float* addmag,
                              float noise_scale, void* stream);
/* The same pair with a hard clip between the mask and the noise (the declipping operator; no counterpart in the reference):
 *   thr (batch) fp32, per-clip thresholds c[b] > 0:   y = min(max(wav * mask, -c), c) + noise_scale * add
 * and dwav passes the gradient through the samples with -c <= wav * mask <= c only (inclusive, torch.clamp's rule).  A NaN sample stays
 * NaN.  thr NULL = dmx_audio_guidance_{fwd,bwd}_ex, which are these calls with NULL.  _bwd_shaped must be given the pointers _fwd_shaped
 * saw.  Like the other two pairs: DMX_ERR_SHAPE for handles / lengths the fused kernels do not cover. */
int dmx_audio_guidance_fwd_shaped(dmx_audio* a, const float* wav, long long wav_stride, const float* mask, const float* ref, long long ref_stride,
                                  float* mel_out, void* state, int batch, int L, int power2, int to_db, float lo, float hi, const float* add,
                                  long long add_stride, const float* addmag, float noise_scale, const float* thr, void* stream);
int dmx_audio_guidance_bwd_shaped(dmx_audio* a, const float* wav, long long wav_stride, const float* mask, const float* ref, long long ref_stride,
                                  float gscale, float* loss, float* dwav, long long dwav_stride, int Lfull, void* state, int batch, int L,
                                  int power2, int to_db, float lo, float hi, const float* add, long long add_stride, const float* addmag,
                                  float noise_scale, const float* thr, void* stream);
/* Hard clipping on materialised waveforms (csrc/waveshape.hip), thr (batch) per-clip thresholds c[b] > 0, every row stride >= its length:
 *   clip_fwd        y[b, i]    = min(max(x[b, i], -c), c), i < L                          x (batch, >= L) -> y (batch, L)
 *   clip_bwd        dwav[b, i] = dy[b, i] where -c <= wav[b, i] <= c, else 0, i < L; 0 for L <= i < Lfull
 *   declip_project  out[b, i]  = meas where |meas| < c; max(xhat, c) where meas >= c; min(xhat, -c) where meas <= -c   (the output stage
 *                   of declipping: reliable samples kept, clipped samples made consistent with the measurement)
 * One launch each, no workspace; NaN samples stay NaN. */
int dmx_clip_fwd(const float* x, long long x_stride, const float* thr, float* y, long long y_stride, int batch, int L, void* stream);
int dmx_clip_bwd(const float* dy, long long dy_stride, const float* wav, long long wav_stride, const float* thr, float* dwav,
                 long long dwav_stride, int batch, int L, int Lfull, void* stream);
int dmx_declip_project(const float* xhat, long long xhat_stride, const float* meas, long long meas_stride, const float* thr, float* out,
                       long long out_stride, int batch, int L, void* stream);
/* Dynamic-range compression on materialised waveforms (csrc/drc.hip): a feed-forward compressor whose sidechain
 * runs on blocks of 64 samples, H = ceil(L / 64) blocks per clip, the clip taken as zero outside [0, L).  Parameters, shared by all clips:
 * threshold_db and makeup_db (finite, within +-200), slope = 1 - 1 / ratio in [0, 1] (1 = limiter), knee_db in [0, 200], a_att and a_rel in
 * (0, 1], the follower's per-block coefficients 1 - exp(-64 / (fs t)).
 *   drc_fwd   y[b, 0:L] = g x; state (batch, 3, H) receives the rows p (block power), G (block gain) and s (gain reduction in dB) of each
 *             clip, tape (batch, H) one byte per block: bits 0-1 the region of the static curve, bit 2 the attack gate
 *   drc_bwd   dx[b, 0:L] = the transpose of the Jacobian of drc_fwd at x applied to dy, +0 on [L, Lfull); takes the state and the tape that
 *             drc_fwd wrote for the same x and parameters and never decides a gate again; work: batch * H floats of scratch
 * Three launches each, no atomics, bit-reproducible and independent of the batch position.  A NaN sample of x: drc_fwd gives NaN from the
 * first sample of its block to the end of its clip (y; G and s from that block on) and leaves everything before it bit-equal; drc_bwd gives
 * NaN for the WHOLE dx of that clip (the backward recurrence carries it to block 0).  Other clips are untouched by both.  DMX_ERR_SHAPE, with nothing written, for a null
 * pointer, batch outside 1 .. 65535, L < 1, Lfull < L, a length above 2^30, a row stride below its row, or a parameter outside its range. */
int dmx_drc_fwd(const float* x, long long x_stride, float* y, long long y_stride, float* state, unsigned char* tape, int batch, int L,
                float threshold_db, float slope, float knee_db, float a_att, float a_rel, float makeup_db, void* stream);
int dmx_drc_bwd(const float* dy, long long dy_stride, const float* x, long long x_stride, const float* state, const unsigned char* tape,
                float* work, float* dx, long long dx_stride, int batch, int L, int Lfull, float threshold_db, float slope, float knee_db,
                float a_att, float a_rel, float makeup_db, void* stream);
/* Blind de-compression (csrc/drc.hip, csrc/drc_fit.hip): the compressor above with one parameter row per clip on
 * the device, and those rows fitted inside the guided loop.  theta (batch, 8) fp32 contiguous holds T, k, makeup, aA, aR, 1 - aA, 1 - aR,
 * k / (2 knee_db) (0 when knee_db = 0), the derived entries computed in double and rounded once; knee_db stays a host scalar.
 *   drc_fwd_p   dmx_drc_fwd with the parameters of clip b read from theta[b]: the same three launches and the same arithmetic, so a table
 *               whose rows all hold the parameters of a dmx_drc_fwd call gives y, state and tape bit-equal to it.
 *   drc_bwd_p   dmx_drc_bwd likewise (dx bit-equal on such a table); it keeps what the parameter gradient needs: work is (batch, 2, H), row 0
 *               ds and row 1 dc, and bq0 (batch,) receives Bq[0] = sum_r dy[r] x[r] (1 - (r + 1) / 64) of each clip.
 *               The table's values are operands only, never indices.  A row with a non-finite entry makes y, G, s and dx of that clip NaN
 *               from block 0 on; other clips are untouched.
 *   drc_pgrad   the gradient in phi = (T, k, makeup, ln aA, ln aR) of the loss whose cotangent dmx_drc_bwd_p was given, as partial rows
 *               part (batch, ceil(H / 256), 5), one per segment of 256 blocks; the gradient is their sum over the segments.  A fixed
 *               reduction order, no atomics: the same bits whatever the batch and the clip's place in it.
 *   drc_update  adds a clip's partial rows in ascending order, takes one Adam step per parameter with the arithmetic of dmx_ir_update
 *               (csrc/adam_step.h) and its own lr[q] (0 freezes parameter q: value, moments and table entries keep their bits), clamps to
 *               [lo[q], hi[q]] and rewrites the clip's row of theta; phi, m, v (batch, 5) and theta are updated in place, k is the 1-based
 *               count of updates.  A clip with a non-finite gradient or step keeps all four untouched (decided on the device).
 * DMX_ERR_SHAPE, with nothing written, for what dmx_drc_fwd / dmx_drc_bwd refuse, a null table, knee_db outside [0, 200], k < 1, an lr
 * that is negative or not finite, a beta outside [0, 1), eps < 0, or a box outside T, makeup in +-200, slope in [0, 1], ln a in [-80, 0]. */
int dmx_drc_fwd_p(const float* x, long long x_stride, float* y, long long y_stride, float* state, unsigned char* tape, const float* theta,
                  int batch, int L, float knee_db, void* stream);
int dmx_drc_bwd_p(const float* dy, long long dy_stride, const float* x, long long x_stride, const float* state, const unsigned char* tape,
                  const float* theta, float* work, float* bq0, float* dx, long long dx_stride, int batch, int L, int Lfull, float knee_db,
                  void* stream);
int dmx_drc_pgrad(const float* state, const unsigned char* tape, const float* work, const float* bq0, const float* theta, float* part,
                  int batch, int L, float knee_db, void* stream);
int dmx_drc_update(const float* part, float* phi, float* m, float* v, float* theta, int batch, int L, int k, const double* lr, double beta1,
                   double beta2, double eps, float knee_db, const double* lo, const double* hi, void* stream);
/* Wow and flutter on materialised waveforms (csrc/warp.hip): the clip, taken as zero outside [0, L), read at
 * n + delta(n), where delta is linear between the H + 1 knots of `delay` (fp32, in samples, one knot per 64 samples, H = ceil(L / 64));
 * four-point Catmull-Rom on the taps i - 1 .. i + 2, i = n + floor(delta), a tap outside the clip skipped.  delay_stride = 0: one curve for
 * every clip; otherwise >= H + 1 floats between the clips' curves.  Contract on the curve, checked by the callers on the host: finite,
 * |d[j]| <= 4096, |d[j+1] - d[j]| <= 16.  Outside it the results are unspecified but every access stays inside the buffers, and a
 * non-finite delta(n) gives y[n] = NaN.
 *   warp_fwd   y[b, 0:L] = A x, y (batch, L) contiguous
 *   warp_bwd   dx[b, 0:L] = A^T dy, +0 on [L, full); dy (batch, L) and dx (batch, full) contiguous.  A gather: no atomics
 * One launch each, bit-reproducible and independent of the batch position.  A NaN at x[m] makes exactly the y[n] NaN whose four taps
 * include m (a zero weight does not shield it), a NaN at dy[n] exactly the dx[m] among the taps of n; other clips are untouched.
 * DMX_ERR_SHAPE, with nothing written, for a null pointer, batch outside 1 .. 65535, L < 1, full < L, a length above 2^30, x_stride < L,
 * or a delay stride that is neither 0 nor at least H + 1. */
int dmx_warp_fwd(const float* x, long long x_stride, const float* delay, long long delay_stride, float* y, int batch, int L, void* stream);
int dmx_warp_bwd(const float* dy, const float* delay, long long delay_stride, float* dx, int batch, int L, int full, void* stream);
/* Blind wow and flutter (csrc/warp_fit.hip): the delay curve of dmx_warp_fwd fitted inside the guided loop.  The
 * estimate lives on coarse knots c[0 .. P], one every S = knot_stride fine knots (S a power of two in 1 .. 64, P = ceil(H / S)); the fine
 * curve is d[S p + q] = fmaf(q / S, c[p+1] - c[p], c[p]).
 *   warp_wgrad   from the cotangent dy = dLoss/dy (batch, L) contiguous at y = A_d x and x (batch, >= L): g[n] = dy[n] sum_k w'[k](f(n))
 *                x[i(n) + k], w' the derivatives of the Catmull-Rom weights, out-of-clip taps skipped, NaN where delta(n) is not finite;
 *                part[b, j, 0] = sum_r (1 - r / 64) g[64 j + r], part[b, j, 1] = sum_r (r / 64) g[64 j + r] over n < L, part (batch, H, 2)
 *                contiguous.  The gradient in the fine knots is dd[j] = part[j, 0] + part[j - 1, 1].  No atomics, a fixed butterfly order:
 *                the same bits on every call, whatever the batch and the clip's place in it; other clips never see a clip's NaN.
 *   warp_update  dc[p] = sum over j ascending with |j - S p| < S, 0 <= j <= H of (1 - |j - S p| / S) dd[j]; Adam on (c, m, v) with the
 *                arithmetic of dmx_ir_update (csrc/adam_step.h), k the 1-based count of updates; anchor = 1 ("mean") subtracts the mean of
 *                the stepped knots, anchor = 0 ("none") does not; every knot is clamped to +-max_delay; c, m, v (batch, P + 1) and the
 *                expanded fine curve (batch, H + 1) are written in place.  A clip with a non-finite dc[p], stepped knot or mean keeps all
 *                four untouched (decided on the device).  0 < max_delay <= min(4096, 8 knot_stride) keeps every written curve inside the
 *                contract of dmx_warp_bwd.
 * One launch each.  DMX_ERR_SHAPE, with nothing written, for a null pointer, batch < 1 (wgrad: outside 1 .. 65535), L outside 1 .. 2^30,
 * x_stride < L, a delay stride that is neither 0 nor at least H + 1, a knot_stride that is no power of two in 1 .. 64, k < 1, lr <= 0, a
 * beta outside [0, 1), eps < 0, max_delay outside its range, an anchor other than 0 or 1. */
int dmx_warp_wgrad(const float* dy, const float* x, long long x_stride, const float* delay, long long delay_stride, float* part, int batch,
                   int L, void* stream);
int dmx_warp_update(const float* part, float* coarse, float* m, float* v, float* fine, int batch, int L, int knot_stride, int k, double lr,
                    double beta1, double beta2, double eps, double max_delay, int anchor, void* stream);
/* Declicking (csrc/declick.hip): impulsive noise found by an autoregressive detector and hidden from the loss by a
 * mask with one row per clip.  Per clip, y zero outside [0, L); frames of N = 1024 samples, F = ceil(L / 1024), model order 16.
 *   click_detect   per frame j: the autocorrelation r[0 .. 16] of the 2048 samples from j N - 512 under the periodic Hann window; a = 0
 *                  unless r[0] is a finite positive number, else Levinson-Durbin on (r[0] (1 + 1e-3), r[1], ..); the residual
 *                  e[n] = y[n] - sum_i a[i] y[n - i] of the frame's live samples; sigma = med / 0.6745f, med the |e| of rank ceil(c / 2) of
 *                  the c live samples, ordered by the bit pattern; flags[n] = |e[n]| > threshold * (sigma > sigma_floor ? sigma :
 *                  sigma_floor), strict, a NaN never flagged.  a (batch, F, 16), e (batch, L), sigma (batch, F), flags (batch, L) bytes
 *                  0 / 1, r null or (batch, F, 17), all contiguous.  One workgroup per (frame, clip), fixed-order reductions, no atomics.
 *   click_mask     mask[b, n] = 0 where a flagged q has |q - n| <= guard, else 1; masked[b] = the number of zeros.  flags and mask
 *                  (batch, L) contiguous.
 *   mask_rows      y[b, n] = x[b, n] * mask[b, n] (one rounded product), n < L, +0 on [L, Ly); y (batch, Ly) contiguous.  mask_stride 0:
 *                  one (L) mask for every clip; otherwise >= L floats between the clips' rows.  Its own transpose (Ly = full).
 *   declick_blend  out[b, n] = y where no mask zero lies within `fade` samples of n, x where mask[b, n] = 0, else
 *                  fl(fl(w y) + fl(fl(1 - w) x)), w = fl(d / (fade + 1)), d the distance to the nearest zero.  out (batch, L) contiguous.
 * Bit-reproducible and independent of the batch and the batch position; any bits in y are safe (a non-finite sample reaches only the
 * frames whose window holds it, which get a = 0).  DMX_ERR_SHAPE, with nothing written and the offending argument named, for
 * threshold <= 0 or not finite, sigma_floor < 0 or not finite, guard or fade outside 0 .. 64; and for a null pointer, batch outside
 * 1 .. 65535, a length outside 1 .. 2^30, Ly < L, a row stride < L (with batch > 1; one row uses no stride), a mask stride that is neither
 * 0 nor at least L. */
int dmx_click_detect(const float* y, long long y_stride, float* a, float* e, float* sigma, unsigned char* flags, float* r, int batch, int L,
                     float threshold, float sigma_floor, void* stream);
int dmx_click_mask(const unsigned char* flags, float* mask, int* masked, int batch, int L, int guard, void* stream);
int dmx_mask_rows(const float* x, long long x_stride, const float* mask, long long mask_stride, float* y, int batch, int L, int Ly,
                  void* stream);
int dmx_declick_blend(const float* x, long long x_stride, const float* y, long long y_stride, const float* mask, long long mask_stride,
                      float* out, int batch, int L, int fade, void* stream);
/* out[i] = y[i] + scale * z[i], i < n (the noiser on a materialised measurement A(x): super-resolution, dereverberation, wav_form) */
int dmx_noise_add(const float* y, const float* z, float* out, long long n, float scale, void* stream);
/* PhaseRetrievalOperator.forward: |torch.stft(wav)| as (B, n_fft/2+1, frames) fp32 */
int dmx_audio_stft_mag(dmx_audio* a, const float* wav, long long wav_stride, float* mag, void* state, int batch, int L, void* stream);
/* gradient of a loss on that magnitude (PhaseRetrievalOperator.forward, operator.py:156-163, differentiated by
 * torch.autograd in scheduling_dps.py:199-212 when supervised_space == "wav_form"): dmag (batch, bins, frames) -> dwav;
 * uses the spectrum the last dmx_audio_stft_mag left in `state` */
int dmx_audio_stft_mag_bwd(dmx_audio* a, const float* dmag, float* dwav, long long dwav_stride, void* state, int batch, int L,
                           int accumulate, void* stream);
/* Time-frequency gain (csrc/tf_gain.hip): out[b, 0:L] = A(x[b, 0:L]) and +0 on [L, full), where A multiplies the
 * STFT of the zero-extended clip (n_fft 1024, hop 256, periodic Hann, frames = ceil(L / 256) + 3, frame t at sample (t - 3) * 256) by the real
 * gain and resynthesises by windowed overlap-add divided by c = 1.5.  A is symmetric: the same call is its transpose.  gain: (frames, 513)
 * fp32 rows per clip -- bins contiguous -- with gain_clip_stride floats between clips, 0 = one grid for every clip.  Uses the handle's
 * twiddle and window tables: the handle must have n_fft = 1024 and the Hann window.  One launch, no workspace, bit-reproducible.
 * DMX_ERR_SHAPE, with nothing written, for any other handle, L < 1, full < L, x_stride < L, out_stride < full, a non-zero
 * gain_clip_stride < frames * 513, or a null pointer.  dmx_audio_tf_frames(L) = ceil(L / 256) + 3 (0 for L < 1). */
int dmx_audio_tf_frames(int L);
int dmx_audio_tf_gain(dmx_audio* a, const float* x, long long x_stride, const float* gain, long long gain_clip_stride, float* out,
                      long long out_stride, int batch, int L, int full, void* stream);
/* Blind equalisation (csrc/tf_gain.hip, csrc/tf_eq.hip): the gain of dmx_audio_tf_gain constant in time, G[k, t] =
 * g[k], one curve per clip, fitted inside the guided loop.  Same handle requirement (n_fft 1024, Hann) and frame conventions.
 *   tf_curve   dmx_audio_tf_gain with the gain row of EVERY frame at curve + b * curve_clip_stride: curve (513) fp32 per clip,
 *              curve_clip_stride 0 = one curve for every clip.  Bit for bit dmx_audio_tf_gain of the curve broadcast over the frames; the
 *              same refusals, with a non-zero curve_clip_stride < 513 in place of the grid's.
 *   tf_wgrad   the gradient of a loss in g from x and the cotangent dy = dLoss/dy at y = A_g(x), both (batch, >= L), zero outside [0, L):
 *              dg[b, k] = (h_k / 1536) sum_t Re(X[k, t] conj(U[k, t])), h_0 = h_512 = 1, else 2, X and U the analysis STFTs of x and dy,
 *              as `segments` partial rows, partials (batch, segments, 513): row s holds the frames [16 s, 16 s + 16) added in increasing t.
 *              segments = dmx_audio_tf_wgrad_segments(L) = ceil((ceil(L / 256) + 3) / 16) (0 for L < 1).  No atomics: the same bits on
 *              every call, and a clip's rows depend neither on the batch nor on its place in it; dy = 0 gives +0 everywhere.
 *              DMX_ERR_SHAPE, with nothing written, for another handle, a null pointer, L < 1, a row stride < L, batch > 65535.
 *   eq_update  dg = sum_s partials[b, s, :] in increasing s, then per clip, k the 1-based count of updates since the last reset:
 *                m <- b1 m + (1 - b1) dg;  v <- b2 v + (1 - b2) dg dg;  g~ = max(g - lr (m / (1 - b1^k)) / (sqrt(v / (1 - b2^k)) + eps), 0)
 *                g <- g~ / max_k g~ (normalize = 1, "peak") or g~ (normalize = 0, "none")
 *              the arithmetic of dmx_ir_update (csrc/adam_step.h), scalars taken in double on the host and rounded once.  A clip with a
 *              non-finite element in dg or g~, or with max g~ = 0 under "peak", keeps its g, m and v untouched (decided on the device).
 *              DMX_ERR_SHAPE for a null pointer, batch < 1, segments < 1, k < 1, lr <= 0, a beta outside [0, 1), eps < 0.
 * One launch each. */
int dmx_audio_tf_curve(dmx_audio* a, const float* x, long long x_stride, const float* curve, long long curve_clip_stride, float* out,
                       long long out_stride, int batch, int L, int full, void* stream);
int dmx_audio_tf_wgrad_segments(int L);
int dmx_audio_tf_wgrad(dmx_audio* a, const float* x, long long x_stride, const float* dy, long long dy_stride, float* partials, int batch, int L,
                       void* stream);
int dmx_audio_eq_update(const float* partials, int segments, float* g, float* m, float* v, int batch, int k, double lr, double beta1,
                        double beta2, double eps, int normalize, void* stream);
/* Codec restoration (csrc/mdct_quant.hip): out[b, 0:L] = Phi^T f(Phi x[b, 0:L]) and +0 on [L, full).  Phi is the MDCT
 * of the zero-extended clip: N = 512 coefficients per frame, frame length 1024, hop 512, window sin(pi (n + 1/2) / 1024), frames =
 * dmx_mdct_frames(L) = ceil(L / 512) + 1 (0 for L < 1), frame t at sample (t - 1) * 512, scaled by sqrt(2 / N); Phi^T Phi = I on the clip.
 * step: (frames, 512) fp32 rows per clip -- coefficients contiguous -- with step_clip_stride floats between clips, 0 = one grid for every clip.
 *   mdct_quant    pass = 0: f = Q, q = rint(C / D) (round-half-even, correctly rounded division), Q(C) = q D; D = 0 is transparent, D = +inf
 *                 discards the coefficient (value 0, code 0); |C / D| >= 2^23, a NaN quotient, a negative or NaN step pass C through.  codes,
 *                 when not null, receives q as (batch, frames, 512) int32, INT32_MIN for every coefficient that was not coded.
 *                 pass = 1: f(C) = C where D is not +inf, else 0 -- the straight-through transpose of the quantiser; codes is ignored.
 *   mdct_project  f clamps C into [(q - 1/2) D, (q + 1/2) D], q read from codes (batch, frames, 512), on whole frames (1 <= t <= L / 512 - 1),
 *                 where 0 < D < inf and q is not INT32_MIN; every other coefficient is left as it is.
 * Uses the handle's FFT twiddles and its MDCT tables: the handle must have n_fft = 1024.  One launch, no workspace, no atomics: the same bits
 * on every call, alone, in a batch and at another batch position.  DMX_ERR_SHAPE, with nothing written, for another handle, L < 1, full < L,
 * x_stride < L, out_stride < full, a non-zero step_clip_stride < frames * 512, a null pointer (codes of mdct_project included), batch > 65535. */
int dmx_mdct_frames(int L);
int dmx_mdct_quant(dmx_audio* a, const float* x, long long x_stride, const float* step, long long step_clip_stride, int* codes, float* out,
                   long long out_stride, int batch, int L, int full, int pass, void* stream);
int dmx_mdct_project(dmx_audio* a, const float* x, long long x_stride, const float* step, long long step_clip_stride, const int* codes, float* out,
                     long long out_stride, int batch, int L, int full, void* stream);
/* PhaseRetrievalOperator.transform on a given magnitude (B, bins, frames) -> (B, frames, n_mels) */
int dmx_audio_melscale(dmx_audio* a, const float* mag, float* mel_out, int batch, int frames, float lo, float hi, void* stream);
/* MusicInpaintingOperator.forward (operator.py:132-133): y[b,t] = x[b,t]*mask[t] (t<L), 0 for L<=t<Ly; mask NULL = copy */
int dmx_mask_apply(const float* x, long long x_stride, const float* mask, float* y, long long y_stride, int batch, int L, int Ly,
                   void* stream);
/* per-clip loss[b] = ||ref_b - pred_b||_2 (torch.linalg.norm, scheduling_dps.py:211) and dpred = gscale * dloss/dpred */
int dmx_l2_loss(const float* ref, long long ref_stride, const float* pred, float* loss, float* dpred, int batch, long long n,
                float gscale, void* stream);
/* Track mode (diffmusic_amd/inverse_problem/track.py; no counterpart in the reference, which restores one window): `windows` <= 64
 * windows of L samples, window w at track sample starts_host[w] (HOST array, increasing by less than L, first 0, last T - L), taper
 * u(i) = min(i + 0.5, L - 0.5 - i, R) / R with 0 < R <= L / 2, L <= 2^22, den[n] = sum of u over the windows that cover track sample n.
 *   fwd  S:   track[n]   = sum_w (u(n - start[w]) / den[n]) * wav[w, n - start[w]]          wav (windows, >= L), row stride wav_stride
 *   bwd  S^T: dwav[w, i] = (u(i) / den[start[w] + i]) * dtrack[start[w] + i] for i < L, 0 for L <= i < full; row stride dwav_stride
 * A sample that one window covers has weight exactly 1 (copied bit for bit).  One launch each, no workspace. */
int dmx_track_stitch_fwd(const float* wav, long long wav_stride, float* track, const int* starts_host, int windows, int L, int R, int T,
                         void* stream);
int dmx_track_stitch_bwd(const float* dtrack, float* dwav, long long dwav_stride, const int* starts_host, int windows, int L, int R, int T,
                         int full, void* stream);
/* Source separation (diffmusic_amd/inverse_problem/mixture.py, csrc/mix.hip; no counterpart in the reference): `stems` K <= 16 stems as
 * the batch, rows stem-major (row k * groups + w is stem k of group w; groups = 1 for one window, = W for the windows of a track), gains
 * g_k as a HOST array of `stems` finite floats, NULL = all ones.
 *   mix_fwd  M:    mix[w, n]             = ((g_0 x[0 G + w, n] + g_1 x[1 G + w, n]) + ...)  ascending k; wav (K G, >= L), row stride
 *                  wav_stride; mix (G, L) contiguous
 *   mix_bwd  M^T:  dwav[k G + w, i]      = g_k dmix[w, i] for i < L, +0.0f for L <= i < full; dmix (G, L) contiguous, row stride dwav_stride
 *   project  P:    out[k, n]             = x[k, n] + c_k (y[n] - mix(x)[n]), c_k = g_k / sum_j g_j^2 taken in double and rounded once
 *                  (groups = 1): the minimum-norm correction after which the stems sum to the mixture y (1, L); out (K, L) contiguous
 * Every product and sum is rounded on its own and a sum's first term is taken as it is, so a plain fp32 loop restates each bit for bit and
 * K = 1, g = 1 copies.  One launch each, no workspace.  Refused without a launch: stems outside 1..16, groups < 1, L < 1, a row stride
 * below its length, full < L, a non-finite gain (DMX_ERR_PARAM), more than 65535 rows in the grid. */
int dmx_stem_mix_fwd(const float* wav, long long wav_stride, float* mix, const float* gains_host, int stems, int groups, int L, void* stream);
int dmx_stem_mix_bwd(const float* dmix, float* dwav, long long dwav_stride, const float* gains_host, int stems, int groups, int L, int full,
                     void* stream);
int dmx_stem_project(const float* x, long long x_stride, const float* y, float* out, const float* gains_host, int stems, int L, void* stream);
/* per-clip x *= target/max|x| ; inv_scale[b] = max|x|/target  (keeps the fp16 backward sweep in range) */
int dmx_grad_normalize(float* x, float* inv_scale, int batch, long long n, float target, void* stream);

/* Polyphase / dense FIR (fp32): out[j*new + p] = sum_t h[p][t] * in[j*orig + t - off], zero outside [0, Lin).
 * Replaces torchaudio Resample in SuperResolutionOperator.forward (operator.py:203-205; h = sinc-hann kernel (new, taps),
 * off = width) and F.conv1d in MusicDereverberationOperator.forward (operator.py:247-249; orig = new = 1, off = taps/2). */
int dmx_fir_fwd(const float* in, long long in_stride, const float* h, float* out, long long out_stride, int batch, int Lin, int Lout,
                int taps, int orig, int new_, int off, void* stream);
/* transpose of dmx_fir_fwd (gradient w.r.t. `in`); h_rev = time-reversed taps, required only for the dense 1:1 case */
int dmx_fir_bwd(const float* dout, long long dout_stride, const float* h, const float* h_rev, float* din, long long din_stride, int batch,
                int Lin, int Lout, int taps, int orig, int new_, int off, void* stream);
/* Blind dereverberation (csrc/fir.hip, csrc/fir_blind.hip; no counterpart in the reference, whose dereverberation always knows its
 * response): one response per clip, h (batch, taps), fitted inside the guided loop.  Geometry of the dense 1:1 dmx_fir_fwd: off = taps / 2,
 * Lout = L + 2 * (taps / 2) - taps + 1, x zero outside [0, L); taps may exceed L.
 *   fir_clip_fwd  y[b, o]  = sum_t h[b, t] * x[b, o + t - off]                     = dmx_fir_fwd of clip b alone with h[b], bit for bit
 *   fir_clip_bwd  dx[b, i] = sum_t h[b, t] * dy[b, i - t + off], i < Lin           = dmx_fir_bwd of clip b alone; h_rev[b, t] = h[b, taps-1-t]
 *   fir_wgrad     dh[b, t] = sum_o dy[b, o] * x[b, o + t - off]                    as `segments` partial rows, partials (batch, segments, taps):
 *                 row s holds the terms o in [4096 s, 4096 (s + 1)), dh is their sum over s.  segments = ceil(Lout / 4096) =
 *                 dmx_fir_wgrad_workspace_floats(batch, Lout, taps) / (batch * taps).  No atomics: the same bits on every call, and a
 *                 clip's rows depend neither on the batch nor on its place in it.
 *   ir_update     g = sum_s partials[b, s, :] in increasing s, then per clip, k the 1-based count of updates since the last reset:
 *                   m <- b1 m + (1 - b1) g;  v <- b2 v + (1 - b2) g g;  h' = h - lr (m / (1 - b1^k)) / (sqrt(v / (1 - b2^k)) + eps)
 *                   h <- h' / max_t |h'|  (the peak normalisation of generate_impulse_response), h_rev <- its reverse
 *                 in fp32, the scalars 1 - b, 1 - b^k taken in double on the host and rounded once.  A clip with a non-finite element in g
 *                 or h', or with max|h'| = 0, keeps its h, h_rev, m and v untouched (decided on the device).  One workgroup per clip:
 *                 taps <= 8192, DMX_ERR_SHAPE above.
 * One launch each. */
int dmx_fir_clip_fwd(const float* in, long long in_stride, const float* h, float* out, long long out_stride, int batch, int Lin, int Lout,
                     int taps, void* stream);
int dmx_fir_clip_bwd(const float* dout, long long dout_stride, const float* h, const float* h_rev, float* din, long long din_stride, int batch,
                     int Lin, int Lout, int taps, void* stream);
size_t dmx_fir_wgrad_workspace_floats(int batch, int Lout, int taps);
int dmx_fir_wgrad(const float* dy, long long dy_stride, const float* x, long long x_stride, float* partials, size_t partial_floats, int batch,
                  int L, int Lout, int taps, void* stream);
int dmx_ir_update(const float* partials, int segments, float* h, float* h_rev, float* m, float* v, int batch, int taps, double lr, double beta1,
                  double beta2, double eps, int k, void* stream);

/* ---- scheduler arithmetic (diffmusic/schedulers/scheduling_{ddim,dps,mpgd,dsg,diffmusic}.py step bodies) -------------- */
#define DMX_SCHED_DDIM 0
#define DMX_SCHED_DPS 1
#define DMX_SCHED_MPGD 2
#define DMX_SCHED_DSG 3
#define DMX_SCHED_DIFFMUSIC 4
/* x0 = (x - sqrt(1-a_t) eps)/sqrt(a_t) */
int dmx_sched_pred_x0(const float* x, const float* eps, float* x0, long long n, float alpha_t, void* stream);
/* the other prediction types of the diffusers DDIM parent every reference scheduler subclasses (scheduling_dps.py:15-61): prediction_type
 * 0 epsilon (as above), 1 sample (x0 = model_output), 2 v_prediction (x0 = sqrt(a_t) x - sqrt(1-a_t) v); clip_range > 0 clamps x0 to
 * [-clip_range, clip_range] (clip_sample) */
int dmx_sched_pred_x0_ex(const float* x, const float* model_output, float* x0, long long n, float alpha_t, int prediction_type, float clip_range,
                         void* stream);
/* classifier-free guidance combine on a (2B, ...) U-Net output (pipeline_musicldm.py:706-708) */
int dmx_sched_cfg_combine(const float* eps2, float* out, long long n, float scale, void* stream);
/* fused update: g0 = dLoss/dx0 (times 1/inv_scale[b]); see csrc/sched.hip for the per-mode formulas */
int dmx_sched_step(int mode, const float* x, const float* eps, const float* x0, const float* g0, const float* inv_scale,
                   const float* noise, float* prev, float* x0_out, float* grad_out, int batch, int n, float alpha_t, float alpha_prev,
                   float sigma, float rate, float eps_small, int global_norm, void* stream);
/* dmx_sched_step for a parent step of another prediction type / with clip_sample: the gradient w.r.t. x_t passes through x0(x_t), i.e.
 * d x0 / d x_t = 1 / sqrt(a_t), 0 or sqrt(a_t), and zero where x0 sits on the clip bound */
int dmx_sched_step_ex(int mode, const float* x, const float* eps, const float* x0, const float* g0, const float* inv_scale,
                      const float* noise, float* prev, float* x0_out, float* grad_out, int batch, int n, float alpha_t, float alpha_prev,
                      float sigma, float rate, float eps_small, int global_norm, int prediction_type, float clip_range, void* stream);

/* Device-side N(0,1) noise, Philox4x32-10 + Box-Muller (csrc/rng.hip): optional replacement for the host draw + upload of
 * randn_tensor (diffmusic/torch_utils.py:31-76) that DSG / DiffMusic pay every step (scheduling_dsg.py:215).  out (batch, n)
 * fp32; clip b uses key seeds_host[b] (HOST array of `batch` <= 64 values); element i = normal (i & 3) of Philox block
 * offset + i / 4, so a draw depends only on (seed_b, offset, i) -- not on the batch composition or the number of GPUs. */
int dmx_randn_philox(float* out, int batch, long long n, const unsigned long long* seeds_host, unsigned long long offset, void* stream);

/* ---- measurement hooks: HIP events around every implicit-GEMM launch (bench.py roofline leg) ---------- */
void dmx_prof_begin(void);
int dmx_prof_end(double* total_ms, double* total_flops); /* returns the number of launches recorded */
/* of the region closed by the last dmx_prof_end: launches / kernel ms / FLOPs / algorithmic operand bytes of gemm_glds_kernel (LDS-DMA tiles) alone */
int dmx_prof_dominant(double* ms, double* flops, double* bytes);

/* ---- low-level test hook: one implicit-GEMM launch described by the internal descriptor --------*/
int dmx_gemm_raw(const void* desc, size_t desc_bytes, void* stream);
/* Host arithmetic (no GPU): 1 when the tap-stationary 320 x 256 tile (tile_cfg 20 / 21 / 22) can take the launch the descriptor
 * describes, 0 when not.  dmx_gemm_last_cfg_raw(): the tile configuration the most recent dmx_gemm_raw launch was dispatched to. */
int dmx_gemm_slab_eligible(const void* desc, size_t desc_bytes);
int dmx_gemm_last_cfg_raw(void);
/* test hook for the fused forward attention of the U-Net (diffusers Attention inside UNet2DConditionModel,
 * pipeline_musicldm.py:696-703): q (B,Nq,C), k (B,Nk,C), v (B,Nk,ldv) fp16 channels-last (ldv = 0: C), o (B,Nq,C); colbias optional
 * (B,Nk) fp32 additive key bias. */
int dmx_flash_attn_raw(const void* q, const void* k, const void* v, void* o, const float* colbias, int B, int Nq, int Nk, int ldv,
                       int C, int heads, float scale, void* stream);
/* test hook: the same kernel with all three row strides, as the U-Net's attention layers call it (q / k / v as slices of one fused QKV
 * buffer: ldq = ldk = ldv = 3C; pre-projected context: ldq = C, ldk = ldv = the context buffer's row stride; 0 = C).  *qt_out (HOST
 * pointer, may be NULL) receives the query-tile form the launch took: 1 = 64 queries per workgroup, 2 = 128; 0 when nothing was launched. */
int dmx_flash_attn_ld_raw(const void* q, const void* k, const void* v, void* o, const float* colbias, int B, int Nq, int Nk, int ldq,
                          int ldk, int ldv, int C, int heads, float scale, int* qt_out, void* stream);
/* test hooks: the row kernels around the attention, each with its internal launcher's parameters.
 * softmax: S (rows, N) fp32 (ld = lds) or 16-bit (ld = ldp, in place allowed) -> P (rows, N) 16-bit (ld = ldp, columns [N, ldp) zeroed);
 *   colbias optional (rows / rows_per_bias, N) fp32 additive; N % 4 == 0, N <= 4096, lds % 4 == 0, ldp % 4 == 0.
 * transpose: in[z][r][c] (R x C, row stride ldi) -> out[z][c][r] (row stride ldo) for z = zo * Zi + zi < Z with batch strides
 *   sIo / sIi / sOo / sOi (elements).
 * rowdot: out[r] = sum_c a[r, c] b[r, c] in fp32; C, lda, ldb multiples of 8.
 * layernorm: y = (x - mean) * rstd * gamma + beta over rows of C (a multiple of 8) 16-bit values; gamma / beta fp32.
 * geglu: x (rows, 2I) = [value | gate] -> y (rows, I) = value * gelu_erf(gate); I a multiple of 8. */
int dmx_softmax_raw(const float* S, void* P, const float* colbias, long long rows, int N, long long lds, long long ldp, int rows_per_bias,
                    void* stream);
int dmx_softmax_act_raw(const void* S, void* P, const float* colbias, long long rows, int N, long long ldp, int rows_per_bias, void* stream);
int dmx_transpose_raw(const void* in, void* out, int R, int C, long long ldi, long long ldo, int Z, int Zi, long long sIo, long long sIi,
                      long long sOo, long long sOi, void* stream);
int dmx_rowdot_raw(const void* a, const void* b, float* out, long long rows, int C, long long lda, long long ldb, void* stream);
int dmx_layernorm_raw(const void* x, void* y, const float* gamma, const float* beta, int rows, int C, float eps, void* stream);
int dmx_geglu_raw(const void* x, void* y, long long rows, int I, void* stream);
/* test hook: fp32 scratch that lets small-M / deep-K launches run split-K (NULL disables it); the U-Net executor
 * installs its own */
int dmx_gemm_splitk_workspace(void* ws, size_t bytes);
/* test hook for the fused convolution pair (HiFi-GAN resblock step, C = 32 / 64 / 128): stage `a` (may be NULL: plain slab
 * convolution) feeds stage `b` through LDS.  Returns DMX_ERR_SHAPE when the shape is not handled by the fused kernel. */
int dmx_conv_pair_raw(const void* desc_a, const void* desc_b, size_t desc_bytes, void* stream);
/* the same launch with dead rows (csrc/conv_pair.h PairDead): dead = {skip0, skip1, zero0, zero1} per clip, NULL = none.  *skipped / *total
 * (HOST pointers, may be NULL) receive how many output slabs per clip the launch skips and how many there are. */
int dmx_conv_pair_dead_raw(const void* desc_a, const void* desc_b, size_t desc_bytes, const int* dead, int* skipped, int* total, void* stream);
/* test hook: n (<= 3) mutually independent fused pairs of one width as ONE grid, longest problem first (the k = 3 / 7 / 11 branches
 * of a HiFi-GAN resblock step, transformers HifiGanResidualBlock.forward); descs_a / descs_b: n consecutive descriptors each. */
int dmx_conv_pair_group_raw(int n, const void* descs_a, const void* descs_b, size_t desc_bytes, void* stream);
/* the grouped launch with dead rows per problem: dead = 4 n ints ({skip0, skip1, zero0, zero1} of problem j at dead + 4 j) or NULL */
int dmx_conv_pair_group_dead_raw(int n, const void* descs_a, const void* descs_b, size_t desc_bytes, const int* dead, void* stream);
/* test hook: GroupNorm (+ SiLU) forward as the U-Net / VAE executors run it (diffusers ResnetBlock2D norm1 / norm2, Attention
 * group_norm; reached from pipeline_musicldm.py:696-703 and scheduling_dps.py:195-197).  x, y (B, P, C) fp16 channels-last;
 * stats (B, G, 2) = (mean, rstd), scale / shift (B, C) fp32 outputs; partial: fp32 scratch of dmx_groupnorm_scratch_floats(B, C, G). */
size_t dmx_groupnorm_scratch_floats(int B, int C, int G);
int dmx_groupnorm_raw(const void* x, void* y, const float* gamma, const float* beta, float* stats, float* scale, float* shift,
                      float* partial, int B, int P, int C, int G, float eps, int silu, void* stream);
/* GroupNorm whose statistics come from partial sums the PRODUCERS of x wrote in their GEMM epilogues (GemmDesc flag EPI_GNSTATS,
 * gn_part): nreg (1..8) regions, part[i] = buffer of dmx_groupnorm_part_floats(B, P_i, N_i) floats, geom[6 i ..] = {rows per slot (what
 * dmx_gemm_last_tile_rows_raw() reported after the producing launch), GEMM rows per image of that launch, N_i / 4, first 4-channel
 * quad of the source in x, real quads of the source, 0}.  Same outputs as dmx_groupnorm_raw; no statistics pass over x. */
size_t dmx_groupnorm_part_floats(int B, int P, int N);
int dmx_groupnorm_parts_raw(const void* x, void* y, const float* gamma, const float* beta, float* stats, float* scale, float* shift,
                            int B, int P, int C, int G, float eps, int silu, int nreg, float* const* part, const int* geom, void* stream);
int dmx_gemm_last_tile_rows_raw(void);
/* test hook: one 2-D convolution as the executors build it (weights w_host (Co, Ci, k, k) and bias b_host (Co) fp32 in HOST memory):
 * x (B, Hi, Wi, pad8(Ci)) -> y (B, Ho, Wo, pad8(Co)) 16-bit channels-last, pad_lo zero rows / columns before the image and pad_hi after
 * it (Ho = (Hi + pad_lo + pad_hi - k) / stride + 1).  Allocates and synchronises. */
int dmx_conv2d_raw(const float* w_host, const float* b_host, const void* x, void* y, int B, int Hi, int Wi, int Ci, int Co, int k, int stride,
                   int pad_lo, int pad_hi, void* stream);
/* GroupNorm(+SiLU) backward (input gradient): the two per-group sums from EPI_GNBWD partial sums of the dgrad launch that produced dy
 * (nreg regions, as above) or, with nreg == 0, from the classic pass over x and dy.  stats / scale / shift: the forward's outputs;
 * k0, k1: (B, C) fp32 scratch; partial: dmx_groupnorm_scratch_floats(B, C, G) floats (used when nreg == 0); add: optional tensor added to dx. */
int dmx_groupnorm_bwd_raw(const void* x, const void* dy, const void* add, void* dx, const float* stats, const float* scale, const float* shift,
                          float* k0, float* k1, float* partial, int B, int P, int C, int G, int silu, int nreg, float* const* part,
                          const int* geom, void* stream);
/* test hooks: the kernels of the CLAP HTS-AT tower (csrc/htsat.hip) one at a time, each through the launcher the tower itself calls.
 * 16-bit tensors are activations (dmx_act_dtype), token-major; gamma / beta / bias tables / mel / dimg / dmel fp32.
 * ln_rows: LayerNorm over `rows` rows of C channels (merge = 0) or of the 4C channels of the 2 x 2 tokens a patch merging gathers from an
 *   H x W grid (merge = 1, row r = image r / (H/2 W/2), cell r mod (H/2 W/2); parts (2oy, 2ox) | (2oy + 1, 2ox) | (2oy, 2ox + 1) |
 *   (2oy + 1, 2ox + 1)); y (rows, row width) 16-bit or fp32 (out_fp32).  Backward: dy (rows, row width) 16-bit or fp32 (dy_fp32), dx written
 *   at the rows' source positions in x's layout, `add` (optional, x's layout, merge = 0 only) added.  C % 8 == 0, row width <= 1536.
 * gelu: erf-GELU over n8 groups of 8 values; the backward's du may be dy.
 * win_attn: window-8 attention of q|k|v rows (B, H W, 3C), heads of 24 channels, relative position bias table (225, heads), cyclic shift
 *   (0 .. 7) with -100 between shift regions; out (B, H W, C); backward: dout (B, H W, C) -> dqkv (B, H W, 3C).  H, W multiples of 8.
 * embed: the fused input stage of handle m (BatchNorm, bicubic stretch, image fold, patch convolution, LayerNorm): mel (batch, frames,
 *   num_mel_bins) -> tokens (batch, (spec_size / 4)^2, embed_dim); backward from mel and dtok: dimg (batch, Tout, num_mel_bins) is the gradient
 *   of the stretched, BatchNorm'ed image (Tout = spec_size^2 / num_mel_bins), dmel (batch, frames, num_mel_bins) its pull-back through the
 *   stretch times scale[b] (scale may be NULL).  2 <= frames <= Tout.  Neither touches the tape of a kept forward. */
int dmx_htsat_ln_rows_fwd_raw(const void* x, void* y, const float* gamma, const float* beta, long long rows, int C, int merge, int H, int W,
                              float eps, int out_fp32, void* stream);
int dmx_htsat_ln_rows_bwd_raw(const void* x, const void* dy, const void* add, void* dx, const float* gamma, long long rows, int C, int merge,
                              int H, int W, float eps, int dy_fp32, void* stream);
int dmx_htsat_gelu_fwd_raw(const void* u, void* y, long long n8, void* stream);
int dmx_htsat_gelu_bwd_raw(const void* u, const void* dy, void* du, long long n8, void* stream);
int dmx_htsat_win_attn_fwd_raw(const void* qkv, void* out, const float* bias_table, int B, int H, int W, int C, int heads, int shift,
                               void* stream);
int dmx_htsat_win_attn_bwd_raw(const void* qkv, const void* dout, void* dqkv, const float* bias_table, int B, int H, int W, int C, int heads,
                               int shift, void* stream);
int dmx_htsat_embed_fwd_raw(dmx_model* m, const float* mel, int batch, int frames, void* tokens, void* stream);
int dmx_htsat_embed_bwd_raw(dmx_model* m, const float* mel, int batch, int frames, const void* dtok, const float* scale, float* dimg,
                            float* dmel, void* stream);

#ifdef __cplusplus
}
#endif
#endif
