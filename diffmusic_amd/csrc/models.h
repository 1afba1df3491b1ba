// Network executors (HiFi-GAN, VAE decoder, U-Net): common base.
#pragma once
#include "layers.h"
#include "../../include/diffmusic_hip.h"

enum { DMX_MODEL_HIFIGAN = 1, DMX_MODEL_VAE = 2, DMX_MODEL_UNET = 3, DMX_MODEL_HTSAT = 4, DMX_MODEL_VAE_ENC = 5 };

struct Model {
  int kind = 0;
  ParamStore ps;
  Arena arena;
  bool finalized = false;
  bool dry = false;  // dry run: only workspace accounting, no launches
  virtual ~Model() { ps.free_all(); }
  virtual int finalize(hipStream_t st) = 0;
};
struct dmx_model { Model* impl; };

// launch unless dry-running
#define RUN(expr) do { if (!dry) { int rc_ = (expr); if (rc_ != DMX_OK) return rc_; } } while (0)
#define CHECK_WS(name) do { if (arena.overflow) { dmx_set_error(name " workspace too small: need %zu bytes", arena.peak); return DMX_ERR_WORKSPACE; } } while (0)

Model* dmx_make_hifigan(const dmx_hifigan_config* c);
int dmx_hifigan_out_len_impl(Model* m, int T);
int dmx_hifigan_fwd_impl(Model* m, const act_t* mel, float* wav, int B, int T, void* ws, size_t wsb, hipStream_t st);
int dmx_hifigan_bwd_impl(Model* m, const float* dwav, act_t* dmel, hipStream_t st);
int dmx_hifigan_fwd_dead_impl(Model* m, const act_t* mel, float* wav, int B, int T, int s0, int s1, void* ws, size_t wsb, hipStream_t st);
int dmx_hifigan_dead_plan_impl(Model* m, int* skipped, int* total, int* lo, int* hi, int n);
int dmx_conv_dead_rows_impl(int k, int dil, int pad, int stride, int transposed, int t_in, int t_out, int a, int b, int* lo, int* hi);
size_t dmx_hifigan_ws_impl(Model* m, int B, int T);

Model* dmx_make_vae(const dmx_vae_config* c);
size_t dmx_vae_ws_impl(Model* m, int B, int h, int w);
int dmx_vae_fwd_impl(Model* m, const float* z, float zs, act_t* mel, float* mel32, int B, int h, int w, int keep, void* ws, size_t wsb,
                     hipStream_t st);
int dmx_vae_bwd_impl(Model* m, const act_t* dmel, float zs, float* dz, hipStream_t st);
// AutoencoderKL encoder (vae_enc.hip): forward only; and the output stage moments -> mean / logvar / noised start latent
Model* dmx_make_vae_encoder(const dmx_vae_config* c);
size_t dmx_vae_enc_ws_impl(Model* m, int B, int T, int F);
int dmx_vae_enc_fwd_impl(Model* m, const float* mel, float log_floor, float* moments, int B, int T, int F, void* ws, size_t wsb, hipStream_t st);
int dmx_latent_init_impl(const float* moments, float* mean, float* logvar, float* x, const float* eps, const float* noise, int B, int L, int P,
                         float sqrt_abar, float scaling_factor, float sqrt_1m_abar, hipStream_t st);
int dmx_conv2d_raw_impl(const float* w_host, const float* b_host, const act_t* x, act_t* y, int B, int Hi, int Wi, int Ci, int Co, int k,
                        int stride, int pad_lo, int pad_hi, hipStream_t st);
Model* dmx_make_unet(const dmx_unet_config* c);
size_t dmx_unet_ws_impl(Model* m, int B, int h, int w, int n0, int n1);
int dmx_unet_fwd_impl(Model* m, const float* x, const float* t, const float* cls, float* eps, int B, int h, int w, void* ws, size_t wsb,
                      hipStream_t st, const float* c0, int n0, const float* c1, int n1, const float* bias1);

// CLAP HTS-AT audio tower (style-guidance operator): forward with tape + input-gradient backward, and the Gram matrix of its features
Model* dmx_make_htsat(const dmx_htsat_config* c);
size_t dmx_htsat_ws_impl(Model* m, int B, int frames);
int dmx_htsat_fwd_impl(Model* m, const float* mel, int B, int frames, float* feat, int keep, void* ws, size_t wsb, hipStream_t st);
int dmx_htsat_bwd_impl(Model* m, const float* dfeat, const float* scale, float* dmel, hipStream_t st);
void dmx_htsat_dims_impl(Model* m, int* tokens, int* channels);
size_t dmx_htsat_tape_impl(Model* m, int stage, int block, int which, const act_t** p);
int dmx_htsat_ln_fwd_impl(const act_t* x, void* y, const float* gamma, const float* beta, long long rows, int C, int merge, int H, int W,
                          float eps, int out_fp32, hipStream_t st);
int dmx_htsat_ln_bwd_impl(const act_t* x, const void* dy, const act_t* add, act_t* dx, const float* gamma, long long rows, int C, int merge,
                          int H, int W, float eps, int dy_fp32, hipStream_t st);
int dmx_htsat_gelu_fwd_impl(const act_t* u, act_t* y, long long n8, hipStream_t st);
int dmx_htsat_gelu_bwd_impl(const act_t* u, const act_t* dy, act_t* du, long long n8, hipStream_t st);
int dmx_htsat_win_attn_fwd_impl(const act_t* qkv, act_t* out, const float* bias_table, int B, int H, int W, int C, int heads, int shift,
                                hipStream_t st);
int dmx_htsat_win_attn_bwd_impl(const act_t* qkv, const act_t* dout, act_t* dqkv, const float* bias_table, int B, int H, int W, int C,
                                int heads, int shift, hipStream_t st);
int dmx_htsat_embed_fwd_impl(Model* m, const float* mel, int B, int frames, act_t* tokens, hipStream_t st);
int dmx_htsat_embed_bwd_impl(Model* m, const float* mel, int B, int frames, const act_t* dtok, const float* scale, float* dimg, float* dmel,
                             hipStream_t st);
int dmx_gram_fwd_impl(const float* F, float* G, int B, int T, int C, hipStream_t st);
int dmx_gram_bwd_impl(const float* F, const float* dG, float* dF, int B, int T, int C, hipStream_t st);
