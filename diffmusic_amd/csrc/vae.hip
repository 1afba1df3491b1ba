// AutoencoderKL decoder forward + input-gradient backward (diffusers 0.31.0 semantics, SURVEY.md
// section 8c Appendix B6).  Replaces `vae.decode(1/sf * x0).sample` inside every guided step
// (reference: diffmusic/schedulers/scheduling_dps.py:195-197) and the autograd sweep through it
// (scheduling_dps.py:211-212).  Tape = each resnet's input + mid activation + GroupNorm statistics,
// and that of the single-head mid attention (VaeMidAttention, blocks.h); conv dgrad needs only weights.
#include "blocks.h"

struct VaeDecoder : Model {
  dmx_vae_config cfg;
  ConvLayer post_quant, conv_in, conv_out;
  Resnet2D mid0, mid1;
  VaeMidAttention attn;
  GnLayer norm_out;
  std::vector<std::vector<Resnet2D>> up_res;
  std::vector<ConvLayer> up_conv;
  std::vector<int> up_ch;
  float* gn_partial = nullptr;
  int Cmid = 0;
  bool up2x = true;            // fold the nearest x2 upsampling into the 3x3 convolution that follows it
  // tape
  int B = 0, h = 0, w = 0;
  bool have_tape = false;
  ResnetTape t_mid0, t_mid1;
  std::vector<std::vector<ResnetTape>> t_up;
  GnTape t_norm_out;
  const act_t* final_x = nullptr;

  explicit VaeDecoder(const dmx_vae_config& c) : cfg(c) {
    kind = DMX_MODEL_VAE;
    const int nb = c.num_blocks, G = c.norm_num_groups;
    const float eps = c.eps;
    Cmid = c.block_out_channels[nb - 1];
    post_quant = make_conv2d(ps, "post_quant_conv", c.latent_channels, c.latent_channels, 1, 1, 0, true);
    conv_in = make_conv2d(ps, "decoder.conv_in", c.latent_channels, Cmid, 3, 1, 1, true);
    mid0.build(ps, "decoder.mid_block.resnets.0", Cmid, Cmid, 0, G, eps, true);
    attn.build(ps, "decoder.mid_block.attentions.0", Cmid, G, eps, true);
    mid1.build(ps, "decoder.mid_block.resnets.1", Cmid, Cmid, 0, G, eps, true);
    int prev = Cmid;
    for (int i = 0; i < nb; ++i) {
      const int ch = c.block_out_channels[nb - 1 - i];
      std::vector<Resnet2D> rs(c.layers_per_block + 1);
      for (int j = 0; j <= c.layers_per_block; ++j)
        rs[j].build(ps, "decoder.up_blocks." + std::to_string(i) + ".resnets." + std::to_string(j), j == 0 ? prev : ch, ch, 0, G, eps, true);
      up_res.push_back(rs);
      up_ch.push_back(ch);
      if (i != nb - 1) up_conv.push_back(make_conv2d(ps, "decoder.up_blocks." + std::to_string(i) + ".upsamplers.0.conv", ch, ch, 3, 1, 1, true));
      prev = ch;
    }
    norm_out.build(ps, "decoder.conv_norm_out", prev, G, eps);
    conv_out = make_conv2d(ps, "decoder.conv_out", prev, c.out_channels, 3, 1, 1, true);
    gn_partial = (float*)ps.dalloc(dmx_gn_scratch_floats(64, 2048, G) * sizeof(float));
  }

  int finalize(hipStream_t st) override {
    CTRY(pack_layer(ps, post_quant, st));
    CTRY(pack_layer(ps, conv_in, st));
    CTRY(pack_layer(ps, conv_out, st));
    CTRY(mid0.pack(ps, st));
    CTRY(mid1.pack(ps, st));
    norm_out.bind(ps);
    CTRY(attn.pack(ps, st));
    for (auto& rs : up_res) for (auto& r : rs) CTRY(r.pack(ps, st));
    for (auto& l : up_conv) { CTRY(pack_layer(ps, l, st)); CTRY(pack_layer_up2x(ps, l, st)); }
    up2x = getenv("DMX_NO_UP2X") == nullptr;
    return DMX_OK;
  }

  // z (B, latent, h, w) fp32 NCHW -> mel (B, H*W) with H = h*2^(nb-1)
  int forward(const float* z, float z_scale, act_t* mel, float* mel_f32, int B_, int h_, int w_, bool keep, void* ws, size_t wsb,
              hipStream_t st) {
    if (B_ > 64) { dmx_set_error("vae: batch > 64 unsupported"); return DMX_ERR_SHAPE; }
    dry = (ws == nullptr);
    arena.reset(ws, dry ? (size_t)-1 : wsb);
    Ctx cx{&arena, st, dry, gn_partial};
    Arena& A = arena;
    B = B_; h = h_; w = w_;
    have_tape = false;
    const int nb = cfg.num_blocks, Lp = post_quant.Cip;
    int H = h, W = w;
    size_t P = (size_t)H * W;
    t_up.assign(nb, std::vector<ResnetTape>(cfg.layers_per_block + 1));
    ResnetTape* nt = nullptr;
    act_t* z16 = A.bf(B * P * Lp);
    act_t* a0 = A.bf(B * P * Lp);
    act_t* x = A.bf(B * P * Cmid);
    CRUN(dmx_nchw_f32_to_nhwc_bf16(z, z16, B, cfg.latent_channels, (int)P, Lp, z_scale, st));
    Epi e0;
    CRUN(conv_fwd_2d(post_quant, z16, a0, B, H, W, e0, st));
    // xp: GroupNorm partial sums of the current tensor x, written by the launch that produced it (EPI_GNSTATS): every GroupNorm of the
    // decoder whose input comes straight out of a GEMM epilogue runs without its statistics pass
    GnParts xp = gn_parts_new(cx, B, P, conv_in.Cop);
    CTRY(conv_fwd_2d_gn(cx, conv_in, a0, x, B, H, W, e0, &xp, Cmid));
    act_t* y = A.bf(B * P * Cmid);
    GnParts yp = gn_parts_new(cx, B, P, pad8(Cmid));
    CTRY(mid0.fwd(cx, x, y, B, H, W, nullptr, keep ? &t_mid0 : nt, nullptr, 0, &xp, &yp));
    x = y; xp = yp;
    CTRY(attn.fwd(cx, x, &y, B, H, W, keep, &xp, &yp));      // mid attention (one head of dim Cmid)
    x = y; xp = yp;
    y = A.bf(B * P * Cmid);
    yp = gn_parts_new(cx, B, P, pad8(Cmid));
    CTRY(mid1.fwd(cx, x, y, B, H, W, nullptr, keep ? &t_mid1 : nt, nullptr, 0, &xp, &yp));
    x = y; xp = yp;
    for (int i = 0; i < nb; ++i) {
      const int ch = up_ch[i];
      for (int j = 0; j <= cfg.layers_per_block; ++j) {
        y = A.bf(B * P * ch);
        yp = gn_parts_new(cx, B, P, pad8(ch));
        CTRY(up_res[i][j].fwd(cx, x, y, B, H, W, nullptr, keep ? &t_up[i][j] : nt, nullptr, 0, &xp, &yp));
        x = y; xp = yp;
      }
      if (i != nb - 1) {
        const int H2 = H * 2, W2 = W * 2;
        const size_t P2 = (size_t)H2 * W2;
        y = A.bf(B * P2 * ch);
        CTRY(upsample_conv_fwd_gn(cx, up_conv[i], x, y, B, H, W, H2, W2, ch, up2x, &yp));
        x = y; xp = yp; H = H2; W = W2; P = P2;
      }
    }
    final_x = x;
    t_norm_out = norm_out.alloc(cx, B);
    {
      const size_t mk = A.mark();
      act_t* n = A.bf(B * P * norm_out.g.C);
      float* m8 = A.f32(B * P * 8);
      CTRY(norm_out.fwd(cx, x, n, B, (int)P, 1, t_norm_out, &xp));
      Epi e; e.flags = EPI_F32OUT;
      CRUN(conv_fwd_2d(conv_out, n, m8, B, H, W, e, st));
      if (mel_f32) CRUN(dmx_gather_col_f32(m8, mel_f32, (long long)B * P, 8, 0, st));
      if (mel) CRUN(dmx_gather_col_f32_to_act(m8, mel, (long long)B * P, 8, 0, st));
      A.release(mk);
    }
    CHECK_WS("vae");
    have_tape = keep;
    return DMX_OK;
  }

  // dmel (B, H*W) fp16 -> dz (B, latent, h, w) fp32 NCHW (times z_scale)
  int backward(const act_t* dmel, float z_scale, float* dz, hipStream_t st) {
    if (!have_tape && !dry) { dmx_set_error("vae backward without a kept forward"); return DMX_ERR_STATE; }
    Ctx cx{&arena, st, dry, gn_partial};
    Arena& A = arena;
    const size_t mk0 = A.mark();
    const int nb = cfg.num_blocks;
    int H = h << (nb - 1), W = w << (nb - 1);
    size_t P = (size_t)H * W;
    Epi e;
    act_t* g8 = A.bf(B * P * 8);
    act_t* gn = A.bf(B * P * norm_out.g.C);
    act_t* g = A.bf(B * P * norm_out.g.C);
    CRUN(dmx_pad_col8_act(dmel, g8, (long long)B * P, st));
    {
      GnParts bpo;
      CTRY(norm_out.conv_bwd_2d_gn(cx, conv_out, g8, gn, B, H, W, final_x, 1, t_norm_out, &bpo));
      CTRY(norm_out.bwd(cx, final_x, gn, nullptr, g, B, (int)P, 1, t_norm_out, &bpo));
    }
    for (int i = nb - 1; i >= 0; --i) {
      const int ch = up_ch[i];
      if (i != nb - 1) {   // upsampler of block i sits after its resnets: undo it first
        const int Hl = H / 2, Wl = W / 2;
        act_t* gl = A.bf((size_t)B * Hl * Wl * ch);
        const size_t mk = A.mark();
        if (up2x) {
          CRUN(conv_up2x_bwd(up_conv[i], g, gl, B, Hl, Wl, e, st));      // dgrad of the folded convolution: one 4x4-tap stride-2 launch
        } else {
          act_t* gu = A.bf(B * P * ch);
          CRUN(conv_bwd_2d(up_conv[i], g, gu, B, H, W, e, st));
          CRUN(dmx_upsample2x_bwd(gu, gl, B, Hl, Wl, ch, st));
        }
        A.release(mk);
        g = gl; H = Hl; W = Wl; P = (size_t)H * W;
      }
      for (int j = cfg.layers_per_block; j >= 0; --j) {
        act_t* gx = A.bf(B * P * up_res[i][j].Cin);
        CTRY(up_res[i][j].bwd(cx, g, gx, B, H, W, t_up[i][j]));
        g = gx;
      }
    }
    {
      act_t* gx = A.bf(B * P * Cmid);
      CTRY(mid1.bwd(cx, g, gx, B, H, W, t_mid1));
      g = gx;
    }
    {
      act_t* gx = A.bf(B * P * Cmid);
      CTRY(attn.bwd(cx, g, gx, B, H, W));
      g = gx;
    }
    {
      act_t* gx = A.bf(B * P * Cmid);
      CTRY(mid0.bwd(cx, g, gx, B, H, W, t_mid0));
      g = gx;
    }
    const int Lp = post_quant.Cip;
    act_t* g1 = A.bf(B * P * Lp);
    act_t* g2 = A.bf(B * P * Lp);
    CRUN(conv_bwd_2d(conv_in, g, g1, B, H, W, e, st));
    CRUN(conv_bwd_2d(post_quant, g1, g2, B, H, W, e, st));
    CRUN(dmx_nhwc_bf16_to_nchw_f32(g2, dz, B, cfg.latent_channels, (int)P, Lp, z_scale, st));
    CHECK_WS("vae");
    A.release(mk0);
    return DMX_OK;
  }
};

Model* dmx_make_vae(const dmx_vae_config* c) { return new VaeDecoder(*c); }
size_t dmx_vae_ws_impl(Model* m, int B, int h, int w) {
  VaeDecoder* v = static_cast<VaeDecoder*>(m);
  v->arena.peak = 0;
  v->forward(nullptr, 1.f, nullptr, nullptr, B, h, w, true, nullptr, 0, nullptr);
  v->backward(nullptr, 1.f, nullptr, nullptr);
  v->have_tape = false;
  v->dry = false;
  return v->arena.peak + 256;
}
int dmx_vae_fwd_impl(Model* m, const float* z, float zs, act_t* mel, float* mel32, int B, int h, int w, int keep, void* ws, size_t wsb,
                     hipStream_t st) {
  return static_cast<VaeDecoder*>(m)->forward(z, zs, mel, mel32, B, h, w, keep != 0, ws, wsb, st);
}
int dmx_vae_bwd_impl(Model* m, const act_t* dmel, float zs, float* dz, hipStream_t st) {
  return static_cast<VaeDecoder*>(m)->backward(dmel, zs, dz, st);
}
