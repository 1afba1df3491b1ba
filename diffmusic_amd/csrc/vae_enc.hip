// AutoencoderKL encoder forward (diffusers 0.31.0 semantics: Encoder + quant_conv -> the moments of DiagonalGaussianDistribution), the
// other half of the autoencoder whose decoder is vae.hip.  Replaces `vae.encode(audio).latent_dist` of the vendored
// pipeline_stable_audio.py:477 for warm-started sampling (an initial mel -> a noised start latent).  Forward only, no tape.
//
// Built from the decoder's blocks (blocks.h): Resnet2D, GnLayer with partial sums from the producing GEMM's epilogue, VaeMidAttention,
// conv_fwd_2d_gn.  New device code: the input stage (fp32 one-channel mel -> channels-last 16-bit, optional ln(max(x, floor)) on load), the
// output stage (moments -> mean / clamped logvar / noised start latent) and the asymmetric padding of the downsampler's descriptor
// (ConvLayer::pad_h_hi / pad_w_hi, layers.hip).
#include "blocks.h"

namespace {

// ---- input stage: mel (rows) fp32, one channel -> (rows, Cp) 16-bit with the channel in column 0 and zeros in the padding.  Four pixels
// per lane: one 16-byte load, 16-byte stores (Cp / 8 per pixel).  log_floor > 0: ln(max(x, log_floor)) on load.
__global__ __launch_bounds__(256) void mel_to_nhwc_kernel(const float* __restrict__ x, act_t* __restrict__ y, long long rows, int Cp, float log_floor) {
  const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i >= rows) return;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  const int n = rows - i >= 4 ? 4 : (int)(rows - i);
  if (n == 4) {
    const float4 q = *reinterpret_cast<const float4*>(x + i);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
    for (int k = 0; k < n; ++k) v[k] = x[i + k];
  }
  const int nv = Cp >> 3;
  for (int k = 0; k < n; ++k) {
    const float f = log_floor > 0.f ? logf(fmaxf(v[k], log_floor)) : v[k];
    uint4* dst = reinterpret_cast<uint4*>(y + (i + k) * Cp);
    dst[0] = make_uint4((uint32_t)f2a(f), 0u, 0u, 0u);
    for (int q = 1; q < nv; ++q) dst[q] = make_uint4(0u, 0u, 0u, 0u);
  }
}

// ---- output stage: moments (B, P, 2L) fp32 channels-last -> mean, logvar (B, L, P) fp32 NCHW, logvar clamped to [-30, 20]
// (DiagonalGaussianDistribution), and optionally x = sa * sf * (mean + exp(0.5 logvar) * eps) + s1 * noise (eps NULL: the mode; noise NULL:
// no noise term).  One lane = 4 pixels x 4 channels: 16-byte loads of the moments, a 4 x 4 transpose in registers, 16-byte NCHW accesses.
// Needs L % 4 == 0; P % 4 != 0 takes the scalar tail path (4-byte accesses).
struct LatentInitArgs {
  const float* mom; float *mean, *logvar, *x; const float *eps, *noise;
  int B, L, P; float sa, sf, s1;
};
__global__ __launch_bounds__(256) void latent_init_kernel(LatentInitArgs a) {
  const int p4n = (a.P + 3) >> 2, c4n = a.L >> 2;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)a.B * c4n * p4n) return;
  const int pq = (int)(t % p4n), cq = (int)((t / p4n) % c4n), b = (int)(t / ((long long)p4n * c4n));
  const int p0 = pq * 4, c0 = cq * 4, ld = 2 * a.L;
  const int np = a.P - p0 >= 4 ? 4 : a.P - p0;
  float m[4][4], lv[4][4];            // [pixel][channel]
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k < np) {
      const float* row = a.mom + ((long long)b * a.P + p0 + k) * ld;
      const float4 qm = *reinterpret_cast<const float4*>(row + c0);
      const float4 ql = *reinterpret_cast<const float4*>(row + a.L + c0);
      m[k][0] = qm.x; m[k][1] = qm.y; m[k][2] = qm.z; m[k][3] = qm.w;
      lv[k][0] = ql.x; lv[k][1] = ql.y; lv[k][2] = ql.z; lv[k][3] = ql.w;
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) { m[k][c] = 0.f; lv[k][c] = 0.f; }
    }
  }
  const bool vec = (a.P & 3) == 0;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const long long o = ((long long)b * a.L + c0 + c) * a.P + p0;
    float mm[4], ll[4], xx[4], ee[4] = {0.f, 0.f, 0.f, 0.f}, nn[4] = {0.f, 0.f, 0.f, 0.f};
    if (a.x) {
      if (vec) {
        if (a.eps) { const float4 q = *reinterpret_cast<const float4*>(a.eps + o); ee[0] = q.x; ee[1] = q.y; ee[2] = q.z; ee[3] = q.w; }
        if (a.noise) { const float4 q = *reinterpret_cast<const float4*>(a.noise + o); nn[0] = q.x; nn[1] = q.y; nn[2] = q.z; nn[3] = q.w; }
      } else {
        for (int k = 0; k < np; ++k) { if (a.eps) ee[k] = a.eps[o + k]; if (a.noise) nn[k] = a.noise[o + k]; }
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      mm[k] = m[k][c];
      ll[k] = fminf(fmaxf(lv[k][c], -30.f), 20.f);
      float z = mm[k];
      if (a.eps) z = mm[k] + expf(0.5f * ll[k]) * ee[k];
      xx[k] = a.sa * a.sf * z;
      if (a.noise) xx[k] += a.s1 * nn[k];
    }
    if (vec) {
      *reinterpret_cast<float4*>(a.mean + o) = make_float4(mm[0], mm[1], mm[2], mm[3]);
      *reinterpret_cast<float4*>(a.logvar + o) = make_float4(ll[0], ll[1], ll[2], ll[3]);
      if (a.x) *reinterpret_cast<float4*>(a.x + o) = make_float4(xx[0], xx[1], xx[2], xx[3]);
    } else {
      for (int k = 0; k < np; ++k) { a.mean[o + k] = mm[k]; a.logvar[o + k] = ll[k]; if (a.x) a.x[o + k] = xx[k]; }
    }
  }
}

}  // namespace

#define CHECK_LAUNCH() (hipGetLastError() == hipSuccess ? DMX_OK : DMX_ERR_LAUNCH)

static int dmx_mel_to_nhwc(const float* x, act_t* y, long long rows, int Cp, float log_floor, hipStream_t st) {
  const long long nthr = (rows + 3) / 4;
  hipLaunchKernelGGL(mel_to_nhwc_kernel, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, st, x, y, rows, Cp, log_floor);
  return CHECK_LAUNCH();
}

int dmx_latent_init_impl(const float* moments, float* mean, float* logvar, float* x, const float* eps, const float* noise, int B, int L, int P,
                         float sqrt_abar, float scaling_factor, float sqrt_1m_abar, hipStream_t st) {
  if (B < 1 || L < 4 || (L & 3) || P < 1) { dmx_set_error("latent_init: latent_channels must be a positive multiple of 4 (got %d), batch and h*w positive", L); return DMX_ERR_SHAPE; }
  if (!moments || !mean || !logvar) { dmx_set_error("latent_init: moments, mean and logvar are required"); return DMX_ERR_SHAPE; }
  LatentInitArgs a{moments, mean, logvar, x, x ? eps : nullptr, x ? noise : nullptr, B, L, P, sqrt_abar, scaling_factor, sqrt_1m_abar};
  const long long nthr = (long long)B * (L >> 2) * ((P + 3) >> 2);
  hipLaunchKernelGGL(latent_init_kernel, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, st, a);
  return CHECK_LAUNCH();
}

struct VaeEncoder : Model {
  dmx_vae_config cfg;
  ConvLayer conv_in, conv_out, quant;
  std::vector<std::vector<Resnet2D>> down_res;
  std::vector<ConvLayer> down_conv;
  Resnet2D mid0, mid1;
  VaeMidAttention attn;
  GnLayer norm_out;
  float* gn_partial = nullptr;
  int Cmid = 0;

  explicit VaeEncoder(const dmx_vae_config& c) : cfg(c) {
    kind = DMX_MODEL_VAE_ENC;
    const int nb = c.num_blocks, G = c.norm_num_groups;
    const float eps = c.eps;
    Cmid = c.block_out_channels[nb - 1];
    // the input has the decoder's output channels (dmx_vae_config carries no in_channels: the checkpoint reader refuses configs where they differ)
    conv_in = make_conv2d(ps, "encoder.conv_in", c.out_channels, c.block_out_channels[0], 3, 1, 1, false);
    int prev = c.block_out_channels[0];
    for (int i = 0; i < nb; ++i) {
      const int ch = c.block_out_channels[i];
      std::vector<Resnet2D> rs(c.layers_per_block);                       // (the decoder's blocks have layers_per_block + 1)
      for (int j = 0; j < c.layers_per_block; ++j)
        rs[j].build(ps, "encoder.down_blocks." + std::to_string(i) + ".resnets." + std::to_string(j), j == 0 ? prev : ch, ch, 0, G, eps, false);
      down_res.push_back(rs);
      // Downsample2D(padding = 0): F.pad(x, (0, 1, 0, 1)) then conv 3x3 stride 2
      if (i != nb - 1) down_conv.push_back(make_conv2d_asym(ps, "encoder.down_blocks." + std::to_string(i) + ".downsamplers.0.conv", ch, ch, 3, 2, 0, 1));
      prev = ch;
    }
    mid0.build(ps, "encoder.mid_block.resnets.0", Cmid, Cmid, 0, G, eps, false);
    attn.build(ps, "encoder.mid_block.attentions.0", Cmid, G, eps, false);
    mid1.build(ps, "encoder.mid_block.resnets.1", Cmid, Cmid, 0, G, eps, false);
    norm_out.build(ps, "encoder.conv_norm_out", Cmid, G, eps);
    conv_out = make_conv2d(ps, "encoder.conv_out", Cmid, 2 * c.latent_channels, 3, 1, 1, false);
    quant = make_conv2d(ps, "quant_conv", 2 * c.latent_channels, 2 * c.latent_channels, 1, 1, 0, false);
    gn_partial = (float*)ps.dalloc(dmx_gn_scratch_floats(64, 2048, G) * sizeof(float));
  }

  int finalize(hipStream_t st) override {
    CTRY(pack_layer(ps, conv_in, st));
    CTRY(pack_layer(ps, conv_out, st));
    CTRY(pack_layer(ps, quant, st));
    for (auto& rs : down_res) for (auto& r : rs) CTRY(r.pack(ps, st));
    for (auto& l : down_conv) CTRY(pack_layer(ps, l, st));
    CTRY(mid0.pack(ps, st));
    CTRY(mid1.pack(ps, st));
    norm_out.bind(ps);
    CTRY(attn.pack(ps, st));
    return DMX_OK;
  }

  // mel (B, T, F) fp32 (one channel) -> moments (B, (T / s) * (F / s), 2 * latent) fp32, s = 2^(num_blocks - 1)
  int forward(const float* mel, float log_floor, float* moments, int B, int T, int F, void* ws, size_t wsb, hipStream_t st) {
    const int nb = cfg.num_blocks, s = 1 << (nb - 1);
    if (B < 1 || B > 64) { dmx_set_error("vae encoder: batch %d unsupported (1 <= batch <= 64)", B); return DMX_ERR_SHAPE; }
    if (T < s || F < s || T % s || F % s) {
      dmx_set_error("vae encoder: frames %d and bins %d must be positive multiples of 2^(num_blocks-1) = %d", T, F, s);
      return DMX_ERR_SHAPE;
    }
    dry = (ws == nullptr);
    arena.reset(ws, dry ? (size_t)-1 : wsb);
    Ctx cx{&arena, st, dry, gn_partial};
    Arena& A = arena;
    int H = T, W = F;
    size_t P = (size_t)H * W;
    act_t* in16 = A.bf(B * P * conv_in.Cip);
    CRUN(dmx_mel_to_nhwc(mel, in16, (long long)B * P, conv_in.Cip, log_floor, st));
    act_t* x = A.bf(B * P * conv_in.Cop);
    // xp: GroupNorm partial sums of x, written by the launch that produced it (as in the decoder: no statistics pass, and the canonical
    // slot order that keeps a clip's result independent of the batch around it)
    GnParts xp = gn_parts_new(cx, B, P, conv_in.Cop);
    CTRY(conv_fwd_2d_gn(cx, conv_in, in16, x, B, H, W, Epi(), &xp, conv_in.Co));
    for (int i = 0; i < nb; ++i) {
      const int ch = cfg.block_out_channels[i];
      for (int j = 0; j < cfg.layers_per_block; ++j) {
        act_t* y = A.bf(B * P * ch);
        GnParts yp = gn_parts_new(cx, B, P, pad8(ch));
        CTRY(down_res[i][j].fwd(cx, x, y, B, H, W, nullptr, nullptr, nullptr, 0, &xp, &yp));
        x = y; xp = yp;
      }
      if (i != nb - 1) {
        const int H2 = H / 2, W2 = W / 2;
        act_t* y = A.bf((size_t)B * H2 * W2 * ch);
        GnParts yp = gn_parts_new(cx, B, (size_t)H2 * W2, down_conv[i].Cop);     // (as the U-Net's stride-2 sampler: statistics from the epilogue)
        CTRY(conv_fwd_2d_gn(cx, down_conv[i], x, y, B, H, W, Epi(), &yp, ch));
        x = y; xp = yp; H = H2; W = W2; P = (size_t)H * W;
      }
    }
    act_t* y = A.bf(B * P * Cmid);
    GnParts yp = gn_parts_new(cx, B, P, pad8(Cmid));
    CTRY(mid0.fwd(cx, x, y, B, H, W, nullptr, nullptr, nullptr, 0, &xp, &yp));
    x = y; xp = yp;
    CTRY(attn.fwd(cx, x, &y, B, H, W, false, &xp, &yp));      // mid attention (one head of dim Cmid); no tape
    x = y; xp = yp;
    y = A.bf(B * P * Cmid);
    yp = gn_parts_new(cx, B, P, pad8(Cmid));
    CTRY(mid1.fwd(cx, x, y, B, H, W, nullptr, nullptr, nullptr, 0, &xp, &yp));
    x = y; xp = yp;
    {
      const GnTape tn = norm_out.alloc(cx, B);
      act_t* n = A.bf(B * P * Cmid);
      act_t* m16 = A.bf(B * P * conv_out.Cop);
      CTRY(norm_out.fwd(cx, x, n, B, (int)P, 1, tn, &xp));
      Epi e;
      CRUN(conv_fwd_2d(conv_out, n, m16, B, H, W, e, st));
      Epi eq; eq.flags = EPI_F32OUT;
      CRUN(conv_fwd_2d(quant, m16, moments, B, H, W, eq, st));      // rows of quant.Cop = 2 * latent floats: the moments tensor itself
    }
    CHECK_WS("vae encoder");
    return DMX_OK;
  }
};

Model* dmx_make_vae_encoder(const dmx_vae_config* c) {
  if (c->num_blocks < 1 || c->layers_per_block < 1 || c->latent_channels < 4 || (c->latent_channels & 3)) {
    dmx_set_error("vae encoder: latent_channels must be a positive multiple of 4 (got %d), num_blocks and layers_per_block positive", c->latent_channels);
    return nullptr;
  }
  if (c->out_channels != 1) {
    dmx_set_error("vae encoder: the input stage takes a one-channel (B, frames, bins) mel (config out_channels = in_channels = %d)", c->out_channels);
    return nullptr;
  }
  return new VaeEncoder(*c);
}
size_t dmx_vae_enc_ws_impl(Model* m, int B, int T, int F) {
  VaeEncoder* v = static_cast<VaeEncoder*>(m);
  v->arena.peak = 0;
  const int rc = v->forward(nullptr, 0.f, nullptr, B, T, F, nullptr, 0, nullptr);
  v->dry = false;
  return rc == DMX_OK ? v->arena.peak + 256 : 0;
}
int dmx_vae_enc_fwd_impl(Model* m, const float* mel, float log_floor, float* moments, int B, int T, int F, void* ws, size_t wsb, hipStream_t st) {
  return static_cast<VaeEncoder*>(m)->forward(mel, log_floor, moments, B, T, F, ws, wsb, st);
}

// test hook (dmx_conv2d_raw): one 2-D convolution through make_conv2d / make_conv2d_asym + pack_layer + conv_fwd_2d, the path every
// executor takes.  Allocates, synchronises and frees: not for the hot path.
int dmx_conv2d_raw_impl(const float* w_host, const float* b_host, const act_t* x, act_t* y, int B, int Hi, int Wi, int Ci, int Co, int k,
                        int stride, int pad_lo, int pad_hi, hipStream_t st) {
  if (B < 1 || Hi < 1 || Wi < 1 || Ci < 1 || Co < 1 || k < 1 || k * k > DMX_MAX_TAPS || stride < 1 || pad_lo < 0 || pad_hi < 0 ||
      Hi + pad_lo + pad_hi < k || Wi + pad_lo + pad_hi < k) { dmx_set_error("conv2d_raw: bad geometry"); return DMX_ERR_SHAPE; }
  ParamStore ps;
  ConvLayer L = pad_lo == pad_hi ? make_conv2d(ps, "conv", Ci, Co, k, stride, pad_lo, false) : make_conv2d_asym(ps, "conv", Ci, Co, k, stride, pad_lo, pad_hi);
  int rc = ps.load("conv.weight", w_host, (size_t)Co * Ci * k * k);
  if (rc == DMX_OK) rc = ps.load("conv.bias", b_host, (size_t)Co);
  if (rc == DMX_OK) rc = pack_layer(ps, L, st);
  Epi e;
  if (rc == DMX_OK) rc = conv_fwd_2d(L, x, y, B, Hi, Wi, e, st);
  (void)hipStreamSynchronize(st);
  ps.free_all();
  return rc;
}
