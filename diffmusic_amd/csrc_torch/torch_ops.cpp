// TORCH_LIBRARY(diffmusic_hip, m): the PyTorch-ROCm custom-op layer over the C ABI of libdiffmusic_hip.so (SURVEY.md section
// 8b.4).  Every op is a thin wrapper: it checks device / dtype / contiguity, allocates the outputs with torch's caching
// allocator, takes torch's CURRENT HIP stream and calls the `extern "C"` launcher declared in include/diffmusic_hip.h -- the
// launchers never allocate, synchronise or throw, so an op is one stream-ordered enqueue.  A non-zero return code becomes a
// c10::Error carrying dmx_last_error().  Network / audio handles (dmx_model*, dmx_audio*) travel as int64 values obtained
// from the *_create calls of the C ABI (diffmusic_amd/engine.py owns them).
//
// Callers on the reference side are its three protocols (Scheduler.step, Pipeline.__call__, BaseOperator); the reference
// lines each op replaces are cited at the C-ABI declarations.
#include <ATen/ATen.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>   // torch-ROCm tensors report DeviceType::CUDA: the guard / stream types that accept it
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include "../../include/diffmusic_hip.h"

// entry points added to C-ABI version 4 without a version bump: weak, so that a libdiffmusic_hip.so of that version built before them
// still lets this library load far enough to say what is missing (TORCH_LIBRARY init below)
#pragma weak dmx_vae_encoder_create
#pragma weak dmx_vae_encoder_workspace_bytes
#pragma weak dmx_vae_encode_fwd
#pragma weak dmx_latent_init
#pragma weak dmx_track_stitch_fwd
#pragma weak dmx_track_stitch_bwd
#pragma weak dmx_audio_guidance_fwd_shaped
#pragma weak dmx_audio_guidance_bwd_shaped
#pragma weak dmx_clip_fwd
#pragma weak dmx_clip_bwd
#pragma weak dmx_declip_project
#pragma weak dmx_hifigan_fwd_dead
#pragma weak dmx_hifigan_dead_plan
#pragma weak dmx_fir_clip_fwd
#pragma weak dmx_fir_clip_bwd
#pragma weak dmx_fir_wgrad
#pragma weak dmx_fir_wgrad_workspace_floats
#pragma weak dmx_ir_update
#pragma weak dmx_stem_mix_fwd
#pragma weak dmx_stem_mix_bwd
#pragma weak dmx_stem_project
#pragma weak dmx_audio_tf_gain
#pragma weak dmx_audio_tf_frames
#pragma weak dmx_audio_tf_curve
#pragma weak dmx_audio_tf_wgrad_segments
#pragma weak dmx_audio_tf_wgrad
#pragma weak dmx_audio_eq_update
#pragma weak dmx_drc_fwd
#pragma weak dmx_drc_bwd
#pragma weak dmx_warp_fwd
#pragma weak dmx_warp_bwd
#pragma weak dmx_warp_wgrad
#pragma weak dmx_warp_update
#pragma weak dmx_drc_fwd_p
#pragma weak dmx_drc_bwd_p
#pragma weak dmx_drc_pgrad
#pragma weak dmx_drc_update
#pragma weak dmx_click_detect
#pragma weak dmx_click_mask
#pragma weak dmx_mask_rows
#pragma weak dmx_declick_blend
#pragma weak dmx_mdct_frames
#pragma weak dmx_mdct_quant
#pragma weak dmx_mdct_project

namespace {

// every op makes its first tensor's device current for its own duration, so the outputs are allocated there and the launch goes to
// THAT device's current stream (a tensor on a non-current device must not be enqueued on the current device's stream)
#define DMX_DEVICE_OF(t) const c10::hip::HIPGuardMasqueradingAsCUDA dmx_guard_((t).device())
inline void* cur_stream() { return (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream(); }
inline void same_numel(const at::Tensor& a, const at::Tensor& b, const char* what) {
  TORCH_CHECK(a.numel() == b.numel() && a.device() == b.device(), what, ": size / device mismatch");
}

inline void ok(int rc, const char* what) {
  TORCH_CHECK(rc == 0, "diffmusic_hip::", what, " failed with code ", rc, ": ", dmx_last_error());
}
inline void f32_cuda(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor (the diffmusic_hip ops have no CPU fallback)");
  TORCH_CHECK(t.scalar_type() == at::kFloat && t.is_contiguous(), name, " must be contiguous fp32");
}
inline void act_cuda(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous(), name, " must be a contiguous GPU tensor");
  TORCH_CHECK(t.scalar_type() == (dmx_act_dtype() == 1 ? at::kHalf : at::kBFloat16), name, " must have the library's 16-bit activation dtype");
}
inline const float* fp(const std::optional<at::Tensor>& t) { return t.has_value() ? t->data_ptr<float>() : nullptr; }

// ---- scheduler arithmetic (scheduling_{ddim,dps,mpgd,dsg,diffmusic}.py step bodies; pipeline_musicldm.py:706-708)
// ptype / clip_r: the DDIM parent's other branches (sample / v_prediction, clip_sample); the defaults keep the epsilon kernel
at::Tensor sched_pred_x0(const at::Tensor& x, const at::Tensor& eps, double alpha_t, int64_t ptype, double clip_r) {
  f32_cuda(x, "x"); f32_cuda(eps, "eps");
  same_numel(x, eps, "sched_pred_x0(x, eps)");
  DMX_DEVICE_OF(x);
  at::Tensor x0 = at::empty_like(x);
  if (ptype == 0 && clip_r == 0.0)
    ok(dmx_sched_pred_x0(x.data_ptr<float>(), eps.data_ptr<float>(), x0.data_ptr<float>(), x.numel(), (float)alpha_t, cur_stream()), "sched_pred_x0");
  else
    ok(dmx_sched_pred_x0_ex(x.data_ptr<float>(), eps.data_ptr<float>(), x0.data_ptr<float>(), x.numel(), (float)alpha_t, (int)ptype, (float)clip_r,
                            cur_stream()), "sched_pred_x0");
  return x0;
}
at::Tensor cfg_combine(const at::Tensor& eps2, double scale) {
  f32_cuda(eps2, "eps2");
  TORCH_CHECK(eps2.dim() >= 1 && eps2.size(0) % 2 == 0, "eps2 must hold the [uncond | text] halves of the CFG batch");
  DMX_DEVICE_OF(eps2);
  auto sizes = eps2.sizes().vec();
  sizes[0] /= 2;
  at::Tensor out = at::empty(sizes, eps2.options());
  ok(dmx_sched_cfg_combine(eps2.data_ptr<float>(), out.data_ptr<float>(), out.numel(), (float)scale, cur_stream()), "cfg_combine");
  return out;
}
// returns (prev_sample, x0_updated): the second is MPGD's guided x0 (scheduling_mpgd.py:202) and None for every other mode.
// grad_out: caller-owned tensor like x that receives the applied gradient; ptype / clip_r as in sched_pred_x0
std::tuple<at::Tensor, std::optional<at::Tensor>> sched_update(int64_t mode, const at::Tensor& x, const at::Tensor& eps, const at::Tensor& x0,
                                                const std::optional<at::Tensor>& g0, const std::optional<at::Tensor>& inv_scale,
                                                const std::optional<at::Tensor>& noise, double alpha_t, double alpha_prev, double sigma,
                                                double rate, double eps_small, bool global_norm, int64_t ptype, double clip_r,
                                                const std::optional<at::Tensor>& grad_out) {
  f32_cuda(x, "x"); f32_cuda(eps, "eps"); f32_cuda(x0, "x0");
  TORCH_CHECK(x.dim() >= 1 && x.size(0) >= 1, "x must have a batch dimension");
  same_numel(x, eps, "sched_update(x, eps)"); same_numel(x, x0, "sched_update(x, x0)");
  const int B = (int)x.size(0);
  const int n = (int)(x.numel() / B);
  if (g0) { f32_cuda(*g0, "g0"); same_numel(x, *g0, "sched_update(x, g0)"); }
  if (inv_scale) { f32_cuda(*inv_scale, "inv_scale"); TORCH_CHECK(inv_scale->numel() == B && inv_scale->device() == x.device(), "inv_scale must hold one value per clip"); }
  if (noise) { f32_cuda(*noise, "noise"); same_numel(x, *noise, "sched_update(x, noise)"); }
  if (grad_out) { f32_cuda(*grad_out, "grad_out"); same_numel(x, *grad_out, "sched_update(x, grad_out)"); }
  TORCH_CHECK(mode == DMX_SCHED_DDIM || (g0 && inv_scale), "guided modes need g0 and inv_scale");
  DMX_DEVICE_OF(x);
  at::Tensor prev = at::empty_like(x);
  std::optional<at::Tensor> x0_out;
  if (mode == DMX_SCHED_MPGD) x0_out = at::empty_like(x);
  float* const x0o = x0_out ? x0_out->data_ptr<float>() : nullptr;
  float* const go = grad_out ? grad_out->data_ptr<float>() : nullptr;
  if (ptype == 0 && clip_r == 0.0)
    ok(dmx_sched_step((int)mode, x.data_ptr<float>(), eps.data_ptr<float>(), x0.data_ptr<float>(), fp(g0), fp(inv_scale), fp(noise),
                      prev.data_ptr<float>(), x0o, go, B, n, (float)alpha_t, (float)alpha_prev, (float)sigma, (float)rate, (float)eps_small,
                      global_norm ? 1 : 0, cur_stream()), "sched_update");
  else
    ok(dmx_sched_step_ex((int)mode, x.data_ptr<float>(), eps.data_ptr<float>(), x0.data_ptr<float>(), fp(g0), fp(inv_scale), fp(noise),
                         prev.data_ptr<float>(), x0o, go, B, n, (float)alpha_t, (float)alpha_prev, (float)sigma, (float)rate, (float)eps_small,
                         global_norm ? 1 : 0, (int)ptype, (float)clip_r, cur_stream()), "sched_update");
  return {prev, x0_out};
}
at::Tensor randn_philox(at::IntArrayRef shape, at::IntArrayRef seeds, int64_t offset, at::Device device) {
  TORCH_CHECK(!shape.empty() && (int64_t)seeds.size() == shape[0] && shape[0] <= 64, "need one seed per clip (batch <= 64)");
  TORCH_CHECK(device.is_cuda(), "randn_philox draws on the GPU");
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(device);
  at::Tensor out = at::empty(shape, at::TensorOptions().dtype(at::kFloat).device(device));
  std::vector<unsigned long long> s(seeds.begin(), seeds.end());
  ok(dmx_randn_philox(out.data_ptr<float>(), (int)shape[0], out.numel() / shape[0], s.data(), (unsigned long long)offset, cur_stream()), "randn_philox");
  return out;
}

// ---- measurement operators (operator.py) and the loss (scheduling_dps.py:211)
at::Tensor mask_mul(const at::Tensor& x, const std::optional<at::Tensor>& mask, int64_t L, int64_t Ly) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kFloat && x.dim() == 2 && x.stride(1) == 1, "x must be (B, >= L) fp32 on the GPU");
  DMX_DEVICE_OF(x);
  if (mask) f32_cuda(*mask, "mask");
  at::Tensor y = at::empty({x.size(0), Ly}, x.options());
  ok(dmx_mask_apply(x.data_ptr<float>(), x.stride(0), fp(mask), y.data_ptr<float>(), Ly, (int)x.size(0), (int)L, (int)Ly, cur_stream()), "mask_mul");
  return y;
}
// (loss (B), dpred like pred, or None when want_grad is false)
std::tuple<at::Tensor, std::optional<at::Tensor>> l2norm(const at::Tensor& ref, const at::Tensor& pred, double gscale, bool want_grad) {
  f32_cuda(ref, "ref"); f32_cuda(pred, "pred");
  DMX_DEVICE_OF(pred);
  const int B = (int)pred.size(0);
  const long long n = pred.numel() / B;
  TORCH_CHECK((ref.numel() == n || ref.numel() == n * B) && ref.device() == pred.device(), "ref must match pred or broadcast over the batch");
  at::Tensor loss = at::empty({B}, pred.options());
  std::optional<at::Tensor> dpred;
  if (want_grad) dpred = at::empty_like(pred);
  ok(dmx_l2_loss(ref.data_ptr<float>(), ref.numel() == n && B > 1 ? 0 : n, pred.data_ptr<float>(), loss.data_ptr<float>(),
                 dpred ? dpred->data_ptr<float>() : nullptr, B, n, (float)gscale, cur_stream()), "l2norm");
  return {loss, dpred};
}
at::Tensor resample_fwd(const at::Tensor& x, const at::Tensor& h, int64_t Lin, int64_t Lout, int64_t orig, int64_t new_, int64_t off) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kFloat && x.dim() == 2 && x.stride(1) == 1, "x must be (B, >= Lin) fp32 on the GPU");
  DMX_DEVICE_OF(x);
  f32_cuda(h, "h");
  at::Tensor y = at::empty({x.size(0), Lout}, x.options());
  ok(dmx_fir_fwd(x.data_ptr<float>(), x.stride(0), h.data_ptr<float>(), y.data_ptr<float>(), Lout, (int)x.size(0), (int)Lin, (int)Lout,
                 (int)h.size(-1), (int)orig, (int)new_, (int)off, cur_stream()), "resample_fwd");
  return y;
}
at::Tensor resample_bwd(const at::Tensor& dy, const at::Tensor& h, const std::optional<at::Tensor>& h_rev, int64_t Lin, int64_t Lfull,
                        int64_t orig, int64_t new_, int64_t off) {
  f32_cuda(dy, "dy"); f32_cuda(h, "h");
  DMX_DEVICE_OF(dy);
  at::Tensor d = at::zeros({dy.size(0), Lfull}, dy.options());
  ok(dmx_fir_bwd(dy.data_ptr<float>(), dy.size(1), h.data_ptr<float>(), fp(h_rev), d.data_ptr<float>(), Lfull, (int)dy.size(0), (int)Lin,
                 (int)dy.size(1), (int)h.size(-1), (int)orig, (int)new_, (int)off, cur_stream()), "resample_bwd");
  return d;
}
// blind dereverberation (include/diffmusic_hip.h dmx_fir_clip_{fwd,bwd} / dmx_fir_wgrad / dmx_ir_update): one response per clip
inline void wave_rows(const at::Tensor& x, int64_t L, const char* name) {
  TORCH_CHECK(x.is_cuda(), name, " must be a GPU tensor (the diffmusic_hip ops have no CPU fallback)");
  TORCH_CHECK(x.scalar_type() == at::kFloat && x.dim() == 2 && x.stride(1) == 1 && L >= 1 && x.size(1) >= L, name, " must be (B, >= L) fp32");
}
inline int64_t taps_of(const at::Tensor& h, const at::Tensor& like, int64_t B, const char* name) {
  f32_cuda(h, name);
  TORCH_CHECK(h.dim() == 2 && h.size(0) == B && h.size(1) >= 1 && h.device() == like.device(), name, " must hold one response per clip, (B, taps)");
  return h.size(1);
}
at::Tensor fir_clip_fwd(const at::Tensor& x, const at::Tensor& h, int64_t Lin) {
  wave_rows(x, Lin, "x");
  DMX_DEVICE_OF(x);
  const int64_t B = x.size(0), n = taps_of(h, x, B, "h"), Lout = Lin + 2 * (n / 2) - n + 1;
  at::Tensor y = at::empty({B, Lout}, x.options());
  ok(dmx_fir_clip_fwd(x.data_ptr<float>(), x.stride(0), h.data_ptr<float>(), y.data_ptr<float>(), Lout, (int)B, (int)Lin, (int)Lout, (int)n,
                      cur_stream()), "fir_clip_fwd");
  return y;
}
at::Tensor fir_clip_bwd(const at::Tensor& dy, const at::Tensor& h, const at::Tensor& h_rev, int64_t Lin, int64_t Lfull) {
  f32_cuda(dy, "dy");
  TORCH_CHECK(dy.dim() == 2, "dy must be (B, Lout)");
  DMX_DEVICE_OF(dy);
  const int64_t B = dy.size(0), Lout = dy.size(1), n = taps_of(h, dy, B, "h");
  TORCH_CHECK(taps_of(h_rev, dy, B, "h_rev") == n && Lfull >= Lin && Lin >= 1 && Lout == Lin + 2 * (n / 2) - n + 1,
              "fir_clip_bwd: h_rev like h, Lout = Lin + 2 * (taps / 2) - taps + 1, Lfull >= Lin");
  at::Tensor d = at::zeros({B, Lfull}, dy.options());
  ok(dmx_fir_clip_bwd(dy.data_ptr<float>(), Lout, h.data_ptr<float>(), h_rev.data_ptr<float>(), d.data_ptr<float>(), Lfull, (int)B, (int)Lin,
                      (int)Lout, (int)n, cur_stream()), "fir_clip_bwd");
  return d;
}
at::Tensor fir_wgrad(const at::Tensor& dy, const at::Tensor& x, int64_t L, int64_t taps) {
  f32_cuda(dy, "dy");
  wave_rows(x, L, "x");
  TORCH_CHECK(dy.dim() == 2 && x.size(0) == dy.size(0) && x.device() == dy.device() && taps >= 1 &&
              dy.size(1) == L + 2 * (taps / 2) - taps + 1, "fir_wgrad: dy (B, Lout) with Lout = L + 2 * (taps / 2) - taps + 1, x (B, >= L)");
  DMX_DEVICE_OF(dy);
  const int64_t B = dy.size(0), Lout = dy.size(1);
  const int64_t segments = (int64_t)(dmx_fir_wgrad_workspace_floats((int)B, (int)Lout, (int)taps) / (size_t)(B * taps));
  at::Tensor part = at::empty({B, segments, taps}, dy.options());
  ok(dmx_fir_wgrad(dy.data_ptr<float>(), Lout, x.data_ptr<float>(), x.stride(0), part.data_ptr<float>(), (size_t)part.numel(), (int)B, (int)L,
                   (int)Lout, (int)taps, cur_stream()), "fir_wgrad");
  return part;
}
void ir_update(const at::Tensor& partials, at::Tensor h, at::Tensor h_rev, at::Tensor m, at::Tensor v, int64_t k, double lr, double beta1,
               double beta2, double eps) {
  f32_cuda(partials, "partials");
  TORCH_CHECK(partials.dim() == 3, "partials must be (B, segments, taps)");
  DMX_DEVICE_OF(partials);
  const int64_t B = partials.size(0), n = partials.size(2);
  TORCH_CHECK(taps_of(h, partials, B, "h") == n && taps_of(h_rev, partials, B, "h_rev") == n && taps_of(m, partials, B, "m") == n &&
              taps_of(v, partials, B, "v") == n, "ir_update: h, h_rev, m and v must be (B, taps) like the partial rows");
  ok(dmx_ir_update(partials.data_ptr<float>(), (int)partials.size(1), h.data_ptr<float>(), h_rev.data_ptr<float>(), m.data_ptr<float>(),
                   v.data_ptr<float>(), (int)B, (int)n, lr, beta1, beta2, eps, (int)k, cur_stream()), "ir_update");
}
// a caller-owned waveform-shaped result (`dwav=` / `out=`): (B, >= L) fp32 rows of any stride on `like`'s device, else a fresh (B, cols)
inline at::Tensor rows_out(const std::optional<at::Tensor>& given, const at::Tensor& like, int64_t L, int64_t cols, bool zeroed, const char* name) {
  if (!given) return zeroed ? at::zeros({like.size(0), cols}, like.options()) : at::empty({like.size(0), cols}, like.options());
  TORCH_CHECK(given->is_cuda() && given->device() == like.device() && given->scalar_type() == at::kFloat && given->dim() == 2 &&
              given->stride(1) == 1 && given->size(0) == like.size(0) && given->size(1) >= L, name, " must be (B, >= L) fp32 on the input's device");
  return *given;
}
// out: caller-owned contiguous (B, frames, 64) result
at::Tensor logmel_fwd(int64_t audio, const at::Tensor& wav, const at::Tensor& state, int64_t L, bool power2, bool to_db, double lo, double hi,
                      const std::optional<at::Tensor>& out) {
  dmx_audio* a = reinterpret_cast<dmx_audio*>(audio);
  TORCH_CHECK(wav.is_cuda() && wav.scalar_type() == at::kFloat && wav.dim() == 2 && wav.stride(1) == 1, "wav must be (B, >= L) fp32 on the GPU");
  DMX_DEVICE_OF(wav);
  TORCH_CHECK(state.is_cuda() && (size_t)state.nbytes() >= dmx_audio_state_bytes(a, (int)wav.size(0), (int)L), "state buffer too small");
  const int64_t T = dmx_audio_num_frames(a, (int)L);
  if (out) { f32_cuda(*out, "out"); TORCH_CHECK(out->numel() == wav.size(0) * T * 64 && out->device() == wav.device(), "out must be (B, frames, 64)"); }
  at::Tensor mel = out ? *out : at::empty({wav.size(0), T, 64}, wav.options());
  ok(dmx_audio_transform_fwd(a, wav.data_ptr<float>(), wav.stride(0), mel.data_ptr<float>(), state.data_ptr(), (int)wav.size(0), (int)L,
                             power2, to_db, (float)lo, (float)hi, cur_stream()), "logmel_fwd");
  return mel;
}
// dwav: caller-owned (B, >= L) result with any row stride, overwritten up to L
at::Tensor logmel_bwd(int64_t audio, const at::Tensor& dmel, const at::Tensor& state, int64_t L, bool power2, bool to_db, double lo, double hi,
                      const std::optional<at::Tensor>& dwav) {
  dmx_audio* a = reinterpret_cast<dmx_audio*>(audio);
  f32_cuda(dmel, "dmel");
  DMX_DEVICE_OF(dmel);
  at::Tensor d = rows_out(dwav, dmel, L, L, false, "dwav");
  ok(dmx_audio_transform_bwd(a, dmel.data_ptr<float>(), d.data_ptr<float>(), d.stride(0), state.data_ptr(), (int)dmel.size(0), (int)L, power2, to_db,
                             (float)lo, (float)hi, 0, cur_stream()), "logmel_bwd");
  return d;
}
inline void thr_ok(const std::optional<at::Tensor>& thr, const at::Tensor& like, int64_t B) {
  if (!thr) return;
  f32_cuda(*thr, "thr");
  TORCH_CHECK(thr->numel() == B && thr->device() == like.device(), "thr must hold one threshold per clip on the waveform's device");
}
// fused guidance of the mel-space operators (include/diffmusic_hip.h dmx_audio_guidance_{fwd,bwd}_shaped, which the shorter C entry points
// forward to with null pointers): (loss (B), dwav (B, Lfull)).  The step's measurement noise, used as sigma * noise: standard-normal `noise`
// (B, >= L) in the sample domain and / or `noise_mag` (B, bins, frames) on the magnitudes; thr (B): per-clip hard-clip thresholds between
// the mask and the noise
std::tuple<at::Tensor, at::Tensor> mel_guidance(int64_t audio, const at::Tensor& wav, const std::optional<at::Tensor>& mask, const at::Tensor& ref,
                                                at::Tensor state, int64_t L, int64_t Lfull, bool power2, bool to_db, double lo, double hi, double gscale,
                                                const std::optional<at::Tensor>& noise, const std::optional<at::Tensor>& noise_mag, double sigma,
                                                const std::optional<at::Tensor>& thr) {
  dmx_audio* a = reinterpret_cast<dmx_audio*>(audio);
  TORCH_CHECK(wav.is_cuda() && wav.scalar_type() == at::kFloat && wav.dim() == 2 && wav.stride(1) == 1 && wav.size(1) >= L, "wav must be (B, >= L) fp32 on the GPU");
  DMX_DEVICE_OF(wav);
  f32_cuda(ref, "ref");
  if (mask) { f32_cuda(*mask, "mask"); TORCH_CHECK(mask->numel() >= L && mask->device() == wav.device(), "mask must hold L samples"); }
  const int B = (int)wav.size(0), T = dmx_audio_num_frames(a, (int)L);
  thr_ok(thr, wav, B);
  if (noise) TORCH_CHECK(noise->is_cuda() && noise->device() == wav.device() && noise->scalar_type() == at::kFloat && noise->dim() == 2 && noise->stride(1) == 1 &&
                         noise->size(0) == B && noise->size(1) >= L, "noise must be (B, >= L) fp32 on wav's device");
  if (noise_mag) {
    f32_cuda(*noise_mag, "noise_mag");
    TORCH_CHECK(!power2 && noise_mag->device() == wav.device() && noise_mag->numel() == (int64_t)B * dmx_audio_num_bins(a) * T,
                "noise_mag must be (B, bins, frames) and goes with power2 = False");
  }
  TORCH_CHECK(ref.device() == wav.device() && (ref.numel() == (int64_t)T * 64 || ref.numel() == (int64_t)B * T * 64), "ref must be (B or 1, frames, 64)");
  TORCH_CHECK(state.is_cuda() && (size_t)state.nbytes() >= dmx_audio_state_bytes(a, B, (int)L), "state buffer too small");
  TORCH_CHECK(Lfull >= L, "Lfull < L");
  const long long rs = ref.numel() == (int64_t)T * 64 && B > 1 ? 0 : (long long)T * 64;
  const long long ns = noise ? noise->stride(0) : 0;
  at::Tensor loss = at::empty({B}, wav.options()), dwav = at::empty({B, Lfull}, wav.options());
  ok(dmx_audio_guidance_fwd_shaped(a, wav.data_ptr<float>(), wav.stride(0), fp(mask), ref.data_ptr<float>(), rs, nullptr, state.data_ptr(), B, (int)L,
                                   power2, to_db, (float)lo, (float)hi, fp(noise), ns, fp(noise_mag), (float)sigma, fp(thr), cur_stream()),
     "mel_guidance (forward)");
  ok(dmx_audio_guidance_bwd_shaped(a, wav.data_ptr<float>(), wav.stride(0), fp(mask), ref.data_ptr<float>(), rs, (float)gscale, loss.data_ptr<float>(),
                                   dwav.data_ptr<float>(), Lfull, (int)Lfull, state.data_ptr(), B, (int)L, power2, to_db, (float)lo, (float)hi, fp(noise), ns,
                                   fp(noise_mag), (float)sigma, fp(thr), cur_stream()), "mel_guidance (backward)");
  return {loss, dwav};
}
// hard clipping on materialised waveforms (include/diffmusic_hip.h dmx_clip_fwd / dmx_clip_bwd / dmx_declip_project)
inline void rows_ok(const at::Tensor& x, int64_t L, const char* name) {
  TORCH_CHECK(x.is_cuda(), name, " must be a GPU tensor (the diffmusic_hip ops have no CPU fallback)");
  TORCH_CHECK(x.scalar_type() == at::kFloat && x.dim() == 2 && x.stride(1) == 1 && L >= 1 && x.size(1) >= L, name, " must be (B, >= L) fp32");
}
at::Tensor clip_fwd(const at::Tensor& x, const at::Tensor& thr, int64_t L) {
  rows_ok(x, L, "x");
  DMX_DEVICE_OF(x);
  thr_ok(thr, x, x.size(0));
  at::Tensor y = at::empty({x.size(0), L}, x.options());
  ok(dmx_clip_fwd(x.data_ptr<float>(), x.stride(0), thr.data_ptr<float>(), y.data_ptr<float>(), L, (int)x.size(0), (int)L, cur_stream()), "clip_fwd");
  return y;
}
at::Tensor clip_bwd(const at::Tensor& dy, const at::Tensor& wav, const at::Tensor& thr, int64_t Lfull) {
  f32_cuda(dy, "dy");
  TORCH_CHECK(dy.dim() == 2 && Lfull >= dy.size(1), "dy must be (B, L) with L <= Lfull");
  const int64_t B = dy.size(0), L = dy.size(1);
  rows_ok(wav, L, "wav");
  TORCH_CHECK(wav.size(0) == B && wav.device() == dy.device(), "wav must hold dy's clips");
  DMX_DEVICE_OF(dy);
  thr_ok(thr, dy, B);
  at::Tensor d = at::empty({B, Lfull}, dy.options());
  ok(dmx_clip_bwd(dy.data_ptr<float>(), L, wav.data_ptr<float>(), wav.stride(0), thr.data_ptr<float>(), d.data_ptr<float>(), Lfull, (int)B, (int)L,
                  (int)Lfull, cur_stream()), "clip_bwd");
  return d;
}
at::Tensor declip_project(const at::Tensor& wav, const at::Tensor& measurement, const at::Tensor& thr, int64_t L) {
  rows_ok(wav, L, "wav"); rows_ok(measurement, L, "measurement");
  TORCH_CHECK(measurement.size(0) == wav.size(0) && measurement.device() == wav.device(), "measurement must hold wav's clips");
  DMX_DEVICE_OF(wav);
  thr_ok(thr, wav, wav.size(0));
  at::Tensor out = at::empty({wav.size(0), L}, wav.options());
  ok(dmx_declip_project(wav.data_ptr<float>(), wav.stride(0), measurement.data_ptr<float>(), measurement.stride(0), thr.data_ptr<float>(),
                        out.data_ptr<float>(), L, (int)wav.size(0), (int)L, cur_stream()), "declip_project");
  return out;
}
// dynamic-range compression (include/diffmusic_hip.h dmx_drc_fwd / dmx_drc_bwd): x (B, >= L) -> y (B, L), state (B, 3, H) fp32 (rows p, G, s),
// tape (B, H) uint8 (bits 0-1 region, bit 2 attack), H = ceil(L / 64); the backward takes them back and returns (B, Lfull)
std::tuple<at::Tensor, at::Tensor, at::Tensor> drc_fwd(const at::Tensor& x, int64_t L, double threshold_db, double slope, double knee_db, double a_att,
                                                       double a_rel, double makeup_db) {
  rows_ok(x, L, "x");
  TORCH_CHECK(L <= (int64_t(1) << 30), "L must be <= 2^30");
  DMX_DEVICE_OF(x);
  const int64_t B = x.size(0), H = (L + 63) / 64;
  at::Tensor y = at::empty({B, L}, x.options());
  at::Tensor state = at::empty({B, 3, H}, x.options());
  at::Tensor tape = at::empty({B, H}, x.options().dtype(at::kByte));
  ok(dmx_drc_fwd(x.data_ptr<float>(), x.stride(0), y.data_ptr<float>(), L, state.data_ptr<float>(), tape.data_ptr<uint8_t>(), (int)std::min<int64_t>(B, 65536),
                 (int)L, (float)threshold_db, (float)slope, (float)knee_db, (float)a_att, (float)a_rel, (float)makeup_db, cur_stream()), "drc_fwd");
  return {y, state, tape};
}
at::Tensor drc_bwd(const at::Tensor& dy, const at::Tensor& x, const at::Tensor& state, const at::Tensor& tape, int64_t Lfull, double threshold_db,
                   double slope, double knee_db, double a_att, double a_rel, double makeup_db) {
  TORCH_CHECK(dy.is_cuda(), "dy must be a GPU tensor (the diffmusic_hip ops have no CPU fallback)");
  TORCH_CHECK(dy.scalar_type() == at::kFloat && dy.dim() == 2 && dy.stride(1) == 1 && dy.size(1) >= 1 && Lfull >= dy.size(1) &&
              Lfull <= (int64_t(1) << 30), "dy must be (B, L) fp32 with 1 <= L <= Lfull <= 2^30");
  const int64_t B = dy.size(0), L = dy.size(1), H = (L + 63) / 64;
  rows_ok(x, L, "x");
  TORCH_CHECK(x.size(0) == B && x.device() == dy.device(), "x must hold dy's clips");
  DMX_DEVICE_OF(dy);
  f32_cuda(state, "state");
  TORCH_CHECK(state.device() == dy.device() && state.dim() == 3 && state.size(0) == B && state.size(1) == 3 && state.size(2) == H,
              "state must be (", B, ", 3, ", H, ") on dy's device");
  TORCH_CHECK(tape.is_cuda() && tape.device() == dy.device() && tape.scalar_type() == at::kByte && tape.is_contiguous() && tape.dim() == 2 &&
              tape.size(0) == B && tape.size(1) == H, "tape must be contiguous uint8 (", B, ", ", H, ") on dy's device");
  at::Tensor work = at::empty({B, H}, dy.options());
  at::Tensor d = at::empty({B, Lfull}, dy.options());
  ok(dmx_drc_bwd(dy.data_ptr<float>(), dy.stride(0), x.data_ptr<float>(), x.stride(0), state.data_ptr<float>(), tape.data_ptr<uint8_t>(),
                 work.data_ptr<float>(), d.data_ptr<float>(), Lfull, (int)std::min<int64_t>(B, 65536), (int)L, (int)Lfull, (float)threshold_db, (float)slope,
                 (float)knee_db, (float)a_att, (float)a_rel, (float)makeup_db, cur_stream()), "drc_bwd");
  return d;
}
// blind de-compression (include/diffmusic_hip.h dmx_drc_fwd_p / dmx_drc_bwd_p / dmx_drc_pgrad / dmx_drc_update): the compressor with one
// parameter row per clip, theta (B, 8) fp32 on the device; the backward also returns work (B, 2, H) (rows ds, dc) and bq0 (B,), from which
// drc_pgrad makes part (B, ceil(H / 256), 5); drc_update writes phi, m, v (B, 5) and theta
static void drc_table_ok(const at::Tensor& theta, int64_t B, const at::Tensor& like) {
  f32_cuda(theta, "theta");
  TORCH_CHECK(theta.device() == like.device() && theta.dim() == 2 && theta.size(0) == B && theta.size(1) == 8, "theta must be (", B,
              ", 8) on the clips' device");
}
static void drc_tape_ok(const at::Tensor& state, const at::Tensor& tape, int64_t B, int64_t H, const at::Tensor& like) {
  f32_cuda(state, "state");
  TORCH_CHECK(state.device() == like.device() && state.dim() == 3 && state.size(0) == B && state.size(1) == 3 && state.size(2) == H,
              "state must be (", B, ", 3, ", H, ") on the clips' device");
  TORCH_CHECK(tape.is_cuda() && tape.device() == like.device() && tape.scalar_type() == at::kByte && tape.is_contiguous() && tape.dim() == 2 &&
              tape.size(0) == B && tape.size(1) == H, "tape must be contiguous uint8 (", B, ", ", H, ") on the clips' device");
}
std::tuple<at::Tensor, at::Tensor, at::Tensor> drc_fwd_p(const at::Tensor& x, int64_t L, const at::Tensor& theta, double knee_db) {
  rows_ok(x, L, "x");
  TORCH_CHECK(L <= (int64_t(1) << 30), "L must be <= 2^30");
  const int64_t B = x.size(0), H = (L + 63) / 64;
  drc_table_ok(theta, B, x);
  DMX_DEVICE_OF(x);
  at::Tensor y = at::empty({B, L}, x.options());
  at::Tensor state = at::empty({B, 3, H}, x.options());
  at::Tensor tape = at::empty({B, H}, x.options().dtype(at::kByte));
  ok(dmx_drc_fwd_p(x.data_ptr<float>(), x.stride(0), y.data_ptr<float>(), L, state.data_ptr<float>(), tape.data_ptr<uint8_t>(),
                   theta.data_ptr<float>(), (int)std::min<int64_t>(B, 65536), (int)L, (float)knee_db, cur_stream()), "drc_fwd_p");
  return {y, state, tape};
}
std::tuple<at::Tensor, at::Tensor, at::Tensor> drc_bwd_p(const at::Tensor& dy, const at::Tensor& x, const at::Tensor& state, const at::Tensor& tape,
                                                         const at::Tensor& theta, int64_t Lfull, double knee_db) {
  TORCH_CHECK(dy.is_cuda(), "dy must be a GPU tensor (the diffmusic_hip ops have no CPU fallback)");
  TORCH_CHECK(dy.scalar_type() == at::kFloat && dy.dim() == 2 && dy.stride(1) == 1 && dy.size(1) >= 1 && Lfull >= dy.size(1) &&
              Lfull <= (int64_t(1) << 30), "dy must be (B, L) fp32 with 1 <= L <= Lfull <= 2^30");
  const int64_t B = dy.size(0), L = dy.size(1), H = (L + 63) / 64;
  rows_ok(x, L, "x");
  TORCH_CHECK(x.size(0) == B && x.device() == dy.device(), "x must hold dy's clips");
  drc_tape_ok(state, tape, B, H, dy);
  drc_table_ok(theta, B, dy);
  DMX_DEVICE_OF(dy);
  at::Tensor work = at::empty({B, 2, H}, dy.options());
  at::Tensor bq0 = at::empty({B}, dy.options());
  at::Tensor d = at::empty({B, Lfull}, dy.options());
  ok(dmx_drc_bwd_p(dy.data_ptr<float>(), dy.stride(0), x.data_ptr<float>(), x.stride(0), state.data_ptr<float>(), tape.data_ptr<uint8_t>(),
                   theta.data_ptr<float>(), work.data_ptr<float>(), bq0.data_ptr<float>(), d.data_ptr<float>(), Lfull,
                   (int)std::min<int64_t>(B, 65536), (int)L, (int)Lfull, (float)knee_db, cur_stream()), "drc_bwd_p");
  return {d, work, bq0};
}
at::Tensor drc_pgrad(const at::Tensor& state, const at::Tensor& tape, const at::Tensor& work, const at::Tensor& bq0, const at::Tensor& theta,
                     int64_t L, double knee_db) {
  TORCH_CHECK(L >= 1 && L <= (int64_t(1) << 30), "1 <= L <= 2^30");
  f32_cuda(work, "work");
  const int64_t H = (L + 63) / 64, B = work.size(0);
  TORCH_CHECK(work.dim() == 3 && B >= 1 && work.size(1) == 2 && work.size(2) == H, "work must be (B, 2, ", H, ")");
  drc_tape_ok(state, tape, B, H, work);
  drc_table_ok(theta, B, work);
  f32_cuda(bq0, "bq0");
  TORCH_CHECK(bq0.device() == work.device() && bq0.dim() == 1 && bq0.size(0) == B, "bq0 must be (", B, ",) on work's device");
  DMX_DEVICE_OF(work);
  at::Tensor part = at::empty({B, (H + 255) / 256, 5}, work.options());
  ok(dmx_drc_pgrad(state.data_ptr<float>(), tape.data_ptr<uint8_t>(), work.data_ptr<float>(), bq0.data_ptr<float>(), theta.data_ptr<float>(),
                   part.data_ptr<float>(), (int)std::min<int64_t>(B, 65536), (int)L, (float)knee_db, cur_stream()), "drc_pgrad");
  return part;
}
void drc_update(const at::Tensor& part, at::Tensor phi, at::Tensor m, at::Tensor v, at::Tensor theta, int64_t L, int64_t k, at::ArrayRef<double> lr,
                double beta1, double beta2, double eps, double knee_db, at::ArrayRef<double> lo, at::ArrayRef<double> hi) {
  f32_cuda(part, "part");
  TORCH_CHECK(L >= 1 && L <= (int64_t(1) << 30), "1 <= L <= 2^30");
  TORCH_CHECK(lr.size() == 5 && lo.size() == 5 && hi.size() == 5, "lr, lo and hi must hold five numbers each (T, k, makeup, ln aA, ln aR)");
  const int64_t H = (L + 63) / 64, B = part.size(0);
  TORCH_CHECK(part.dim() == 3 && B >= 1 && part.size(1) == (H + 255) / 256 && part.size(2) == 5, "part must be (B, ", (H + 255) / 256, ", 5)");
  for (const at::Tensor* t : {&phi, &m, &v}) {
    f32_cuda(*t, "phi / m / v");
    TORCH_CHECK(t->dim() == 2 && t->size(0) == B && t->size(1) == 5 && t->device() == part.device(), "phi, m and v must be (", B, ", 5) on part's device");
  }
  drc_table_ok(theta, B, part);
  DMX_DEVICE_OF(part);
  ok(dmx_drc_update(part.data_ptr<float>(), phi.data_ptr<float>(), m.data_ptr<float>(), v.data_ptr<float>(), theta.data_ptr<float>(), (int)B, (int)L,
                    (int)k, lr.data(), beta1, beta2, eps, (float)knee_db, lo.data(), hi.data(), cur_stream()), "drc_update");
}
// wow and flutter (include/diffmusic_hip.h dmx_warp_fwd / dmx_warp_bwd): x (B, >= length) -> (B, length) read along the delay curve;
// delay (H + 1) for every clip or (B, H + 1), H = ceil(length / 64), contiguous; the transpose takes dy (B, length) and returns (B, full)
static int64_t warp_delay_stride(const at::Tensor& delay, int64_t B, int64_t length, const at::Tensor& like) {
  const int64_t K = (length + 63) / 64 + 1;
  f32_cuda(delay, "delay");
  TORCH_CHECK(delay.device() == like.device() && ((delay.dim() == 1 && delay.size(0) == K) || (delay.dim() == 2 && delay.size(0) == B && delay.size(1) == K)),
              "delay must be (", K, ") or (", B, ", ", K, ") = ceil(length / 64) + 1 knots on the clips' device");
  return delay.dim() == 1 ? 0 : K;
}
at::Tensor warp_fwd(const at::Tensor& x, const at::Tensor& delay, int64_t length) {
  rows_ok(x, length, "x");
  TORCH_CHECK(length <= (int64_t(1) << 30), "length must be <= 2^30");
  const int64_t B = x.size(0), ds = warp_delay_stride(delay, B, length, x);
  DMX_DEVICE_OF(x);
  at::Tensor y = at::empty({B, length}, x.options());
  ok(dmx_warp_fwd(x.data_ptr<float>(), x.stride(0), delay.data_ptr<float>(), ds, y.data_ptr<float>(), (int)std::min<int64_t>(B, 65536), (int)length,
                  cur_stream()), "warp_fwd");
  return y;
}
at::Tensor warp_bwd(const at::Tensor& dy, const at::Tensor& delay, int64_t length, int64_t full) {
  f32_cuda(dy, "dy");
  TORCH_CHECK(dy.dim() == 2 && length >= 1 && dy.size(1) == length && full >= length && full <= (int64_t(1) << 30),
              "dy must be contiguous (B, length) fp32 with 1 <= length <= full <= 2^30");
  const int64_t B = dy.size(0), ds = warp_delay_stride(delay, B, length, dy);
  DMX_DEVICE_OF(dy);
  at::Tensor d = at::empty({B, full}, dy.options());
  ok(dmx_warp_bwd(dy.data_ptr<float>(), delay.data_ptr<float>(), ds, d.data_ptr<float>(), (int)std::min<int64_t>(B, 65536), (int)length, (int)full,
                  cur_stream()), "warp_bwd");
  return d;
}
// blind wow and flutter (include/diffmusic_hip.h dmx_warp_wgrad / dmx_warp_update): the gradient of a loss in the fine knots as one pair
// per block, part (B, H, 2), and the Adam + projection update of the coarse curve with its expansion; coarse, m, v and fine are written
at::Tensor warp_wgrad(const at::Tensor& dy, const at::Tensor& x, const at::Tensor& delay, int64_t length) {
  rows_ok(x, length, "x");
  f32_cuda(dy, "dy");
  TORCH_CHECK(length <= (int64_t(1) << 30), "length must be <= 2^30");
  TORCH_CHECK(dy.dim() == 2 && dy.size(0) == x.size(0) && dy.size(1) == length && dy.device() == x.device(),
              "dy must be contiguous (B, length) fp32 on x's device");
  const int64_t B = x.size(0), H = (length + 63) / 64, ds = warp_delay_stride(delay, B, length, x);
  DMX_DEVICE_OF(x);
  at::Tensor part = at::empty({B, H, 2}, x.options());
  ok(dmx_warp_wgrad(dy.data_ptr<float>(), x.data_ptr<float>(), x.stride(0), delay.data_ptr<float>(), ds, part.data_ptr<float>(),
                    (int)std::min<int64_t>(B, 65536), (int)length, cur_stream()), "warp_wgrad");
  return part;
}
void warp_update(const at::Tensor& part, at::Tensor coarse, at::Tensor m, at::Tensor v, at::Tensor fine, int64_t length, int64_t knot_stride,
                 int64_t k, double lr, double beta1, double beta2, double eps, double max_delay, bool mean) {
  f32_cuda(part, "part");
  TORCH_CHECK(length >= 1 && length <= (int64_t(1) << 30) && knot_stride >= 1 && knot_stride <= 64, "1 <= length <= 2^30 and 1 <= knot_stride <= 64");
  const int64_t H = (length + 63) / 64, P = (H + knot_stride - 1) / knot_stride;
  TORCH_CHECK(part.dim() == 3 && part.size(0) >= 1 && part.size(1) == H && part.size(2) == 2, "part must be (B, ", H, ", 2)");
  DMX_DEVICE_OF(part);
  const int64_t B = part.size(0);
  for (const at::Tensor* t : {&coarse, &m, &v}) {
    f32_cuda(*t, "coarse / m / v");
    TORCH_CHECK(t->dim() == 2 && t->size(0) == B && t->size(1) == P + 1 && t->device() == part.device(), "coarse, m and v must be (", B, ", ", P + 1, ") on part's device");
  }
  f32_cuda(fine, "fine");
  TORCH_CHECK(fine.dim() == 2 && fine.size(0) == B && fine.size(1) == H + 1 && fine.device() == part.device(), "fine must be (", B, ", ", H + 1, ") on part's device");
  ok(dmx_warp_update(part.data_ptr<float>(), coarse.data_ptr<float>(), m.data_ptr<float>(), v.data_ptr<float>(), fine.data_ptr<float>(), (int)B,
                     (int)length, (int)knot_stride, (int)k, lr, beta1, beta2, eps, max_delay, mean ? 1 : 0, cur_stream()), "warp_update");
}
// declicking (include/diffmusic_hip.h dmx_click_detect / dmx_click_mask / dmx_mask_rows / dmx_declick_blend): y (B, >= L) -> a (B, F, 16),
// e (B, L), sigma (B, F), flags (B, L) uint8, r (B, F, 17), F = ceil(L / 1024); flags -> mask (B, L) fp32 and masked (B) int32; the mask
// is (L) for every clip or (B, L), contiguous
static int64_t click_mask_stride(const at::Tensor& mask, int64_t B, int64_t L, const at::Tensor& like) {
  f32_cuda(mask, "mask");
  TORCH_CHECK(mask.device() == like.device() && ((mask.dim() == 1 && mask.size(0) == L) || (mask.dim() == 2 && mask.size(0) == B && mask.size(1) == L)),
              "mask must be (", L, ") or (", B, ", ", L, ") on the clips' device");
  return mask.dim() == 1 ? 0 : L;
}
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor> click_detect(const at::Tensor& y, int64_t L, double threshold, double sigma_floor) {
  rows_ok(y, L, "y");
  TORCH_CHECK(L <= (int64_t(1) << 30), "L must be <= 2^30");
  DMX_DEVICE_OF(y);
  const int64_t B = y.size(0), F = (L + 1023) / 1024;
  at::Tensor a = at::empty({B, F, 16}, y.options()), e = at::empty({B, L}, y.options()), sigma = at::empty({B, F}, y.options());
  at::Tensor flags = at::empty({B, L}, y.options().dtype(at::kByte)), r = at::empty({B, F, 17}, y.options());
  ok(dmx_click_detect(y.data_ptr<float>(), y.stride(0), a.data_ptr<float>(), e.data_ptr<float>(), sigma.data_ptr<float>(), flags.data_ptr<uint8_t>(),
                      r.data_ptr<float>(), (int)std::min<int64_t>(B, 65536), (int)L, (float)threshold, (float)sigma_floor, cur_stream()), "click_detect");
  return {a, e, sigma, flags, r};
}
std::tuple<at::Tensor, at::Tensor> click_mask(const at::Tensor& flags, int64_t guard) {
  TORCH_CHECK(flags.is_cuda(), "flags must be a GPU tensor (the diffmusic_hip ops have no CPU fallback)");
  TORCH_CHECK(flags.scalar_type() == at::kByte && flags.is_contiguous() && flags.dim() == 2 && flags.size(1) >= 1 && flags.size(1) <= (int64_t(1) << 30),
              "flags must be contiguous uint8 (B, L), 1 <= L <= 2^30");
  DMX_DEVICE_OF(flags);
  const int64_t B = flags.size(0), L = flags.size(1);
  at::Tensor mask = at::empty({B, L}, flags.options().dtype(at::kFloat)), masked = at::empty({B}, flags.options().dtype(at::kInt));
  ok(dmx_click_mask(flags.data_ptr<uint8_t>(), mask.data_ptr<float>(), masked.data_ptr<int>(), (int)std::min<int64_t>(B, 65536), (int)L,
                    (int)std::max<int64_t>(std::min<int64_t>(guard, 1 << 20), -1), cur_stream()), "click_mask");
  return {mask, masked};
}
at::Tensor mask_rows(const at::Tensor& x, const at::Tensor& mask, int64_t L, int64_t Ly) {
  rows_ok(x, L, "x");
  TORCH_CHECK(Ly >= L && Ly <= (int64_t(1) << 30), "Ly must be in L .. 2^30");
  const int64_t B = x.size(0), ms = click_mask_stride(mask, B, L, x);
  DMX_DEVICE_OF(x);
  at::Tensor y = at::empty({B, Ly}, x.options());
  ok(dmx_mask_rows(x.data_ptr<float>(), x.stride(0), mask.data_ptr<float>(), ms, y.data_ptr<float>(), (int)std::min<int64_t>(B, 65536), (int)L, (int)Ly,
                   cur_stream()), "mask_rows");
  return y;
}
at::Tensor declick_blend(const at::Tensor& x, const at::Tensor& y, const at::Tensor& mask, int64_t L, int64_t fade) {
  rows_ok(x, L, "x"); rows_ok(y, L, "y");
  TORCH_CHECK(L <= (int64_t(1) << 30) && y.size(0) == x.size(0) && y.device() == x.device(), "y must hold x's clips, L <= 2^30");
  const int64_t B = x.size(0), ms = click_mask_stride(mask, B, L, x);
  DMX_DEVICE_OF(x);
  at::Tensor out = at::empty({B, L}, x.options());
  ok(dmx_declick_blend(x.data_ptr<float>(), x.stride(0), y.data_ptr<float>(), y.stride(0), mask.data_ptr<float>(), ms, out.data_ptr<float>(),
                       (int)std::min<int64_t>(B, 65536), (int)L, (int)std::max<int64_t>(std::min<int64_t>(fade, 1 << 20), -1), cur_stream()), "declick_blend");
  return out;
}
// time-frequency gain (include/diffmusic_hip.h dmx_audio_tf_gain): x (B, >= L), gain_t (frames, 513) shared or (B, frames, 513) -> (B, Lfull)
// out: caller-owned (B, >= Lfull) fp32 with any row stride; only out[:, :Lfull] is written
at::Tensor tf_gain(int64_t audio, const at::Tensor& x, const at::Tensor& gain_t, int64_t L, int64_t Lfull, const std::optional<at::Tensor>& out) {
  rows_ok(x, L, "x");
  TORCH_CHECK(Lfull >= L, "Lfull must be >= L");
  DMX_DEVICE_OF(x);
  f32_cuda(gain_t, "gain_t");
  const int64_t B = x.size(0), T = dmx_audio_tf_frames((int)L);
  TORCH_CHECK(gain_t.device() == x.device() && ((gain_t.dim() == 2 && gain_t.size(0) == T && gain_t.size(1) == 513) ||
              (gain_t.dim() == 3 && gain_t.size(0) == B && gain_t.size(1) == T && gain_t.size(2) == 513)),
              "gain_t must be (", T, ", 513) or (", B, ", ", T, ", 513) on x's device");
  at::Tensor y = rows_out(out, x, Lfull, Lfull, false, "out");
  ok(dmx_audio_tf_gain((dmx_audio*)audio, x.data_ptr<float>(), x.stride(0), gain_t.data_ptr<float>(), gain_t.dim() == 3 ? T * 513 : 0,
                       y.data_ptr<float>(), y.stride(0), (int)B, (int)L, (int)Lfull, cur_stream()), "tf_gain");
  return y;
}
// codec restoration (include/diffmusic_hip.h dmx_mdct_quant / dmx_mdct_project): x (B, >= L), step_t (frames, 512) shared or (B, frames, 512),
// frames = ceil(L / 512) + 1 -> (B, Lfull).  out: caller-owned (B, >= Lfull) fp32 with any row stride; only out[:, :Lfull] is written
inline int64_t mdct_step_ok(const at::Tensor& x, const at::Tensor& step_t, int64_t L, int64_t Lfull) {
  rows_ok(x, L, "x");
  TORCH_CHECK(Lfull >= L, "Lfull must be >= L");
  f32_cuda(step_t, "step_t");
  const int64_t B = x.size(0), T = dmx_mdct_frames((int)L);
  TORCH_CHECK(step_t.device() == x.device() && ((step_t.dim() == 2 && step_t.size(0) == T && step_t.size(1) == 512) ||
              (step_t.dim() == 3 && step_t.size(0) == B && step_t.size(1) == T && step_t.size(2) == 512)),
              "step_t must be (", T, ", 512) or (", B, ", ", T, ", 512) on x's device");
  return T;
}
// -> (y, codes): codes (B, frames, 512) int32 with want_codes (the quantiser only), else None; passthrough: the straight-through transpose
std::tuple<at::Tensor, std::optional<at::Tensor>> mdct_quant(int64_t audio, const at::Tensor& x, const at::Tensor& step_t, int64_t L, int64_t Lfull,
                                                             bool passthrough, bool want_codes, const std::optional<at::Tensor>& out) {
  const int64_t T = mdct_step_ok(x, step_t, L, Lfull), B = x.size(0);
  TORCH_CHECK(!(passthrough && want_codes), "mdct_quant: the pass-through form codes nothing (want_codes goes with the quantiser)");
  DMX_DEVICE_OF(x);
  at::Tensor y = rows_out(out, x, Lfull, Lfull, false, "out");
  std::optional<at::Tensor> codes;
  if (want_codes) codes = at::empty({B, T, 512}, x.options().dtype(at::kInt));
  ok(dmx_mdct_quant((dmx_audio*)audio, x.data_ptr<float>(), x.stride(0), step_t.data_ptr<float>(), step_t.dim() == 3 ? T * 512 : 0,
                    codes ? codes->data_ptr<int>() : nullptr, y.data_ptr<float>(), y.stride(0), (int)B, (int)L, (int)Lfull, passthrough ? 1 : 0,
                    cur_stream()), "mdct_quant");
  return {y, codes};
}
at::Tensor mdct_project(int64_t audio, const at::Tensor& x, const at::Tensor& step_t, const at::Tensor& codes, int64_t L, int64_t Lfull,
                        const std::optional<at::Tensor>& out) {
  const int64_t T = mdct_step_ok(x, step_t, L, Lfull), B = x.size(0);
  TORCH_CHECK(codes.is_cuda() && codes.device() == x.device() && codes.scalar_type() == at::kInt && codes.is_contiguous() && codes.dim() == 3 &&
              codes.size(0) == B && codes.size(1) == T && codes.size(2) == 512, "codes must be contiguous int32 (", B, ", ", T, ", 512) on x's device");
  DMX_DEVICE_OF(x);
  at::Tensor y = rows_out(out, x, Lfull, Lfull, false, "out");
  ok(dmx_mdct_project((dmx_audio*)audio, x.data_ptr<float>(), x.stride(0), step_t.data_ptr<float>(), step_t.dim() == 3 ? T * 512 : 0,
                      codes.data_ptr<int>(), y.data_ptr<float>(), y.stride(0), (int)B, (int)L, (int)Lfull, cur_stream()), "mdct_project");
  return y;
}
// blind equalisation (include/diffmusic_hip.h dmx_audio_tf_curve / dmx_audio_tf_wgrad / dmx_audio_eq_update): one gain curve per clip
at::Tensor tf_curve(int64_t audio, const at::Tensor& x, const at::Tensor& curve, int64_t L, int64_t Lfull) {
  rows_ok(x, L, "x");
  TORCH_CHECK(Lfull >= L, "Lfull must be >= L");
  DMX_DEVICE_OF(x);
  f32_cuda(curve, "curve");
  const int64_t B = x.size(0);
  TORCH_CHECK(curve.device() == x.device() && ((curve.dim() == 1 && curve.size(0) == 513) ||
              (curve.dim() == 2 && curve.size(0) == B && curve.size(1) == 513)), "curve must be (513) or (", B, ", 513) on x's device");
  at::Tensor out = at::empty({B, Lfull}, x.options());
  ok(dmx_audio_tf_curve((dmx_audio*)audio, x.data_ptr<float>(), x.stride(0), curve.data_ptr<float>(), curve.dim() == 2 ? 513 : 0,
                        out.data_ptr<float>(), Lfull, (int)B, (int)L, (int)Lfull, cur_stream()), "tf_curve");
  return out;
}
at::Tensor tf_wgrad(int64_t audio, const at::Tensor& dy, const at::Tensor& x, int64_t L) {
  rows_ok(x, L, "x");
  rows_ok(dy, L, "dy");
  TORCH_CHECK(dy.size(0) == x.size(0) && dy.device() == x.device(), "tf_wgrad: dy and x must be (B, >= L) on one device");
  DMX_DEVICE_OF(x);
  const int64_t B = x.size(0);
  at::Tensor part = at::empty({B, (int64_t)dmx_audio_tf_wgrad_segments((int)L), 513}, x.options());
  ok(dmx_audio_tf_wgrad((dmx_audio*)audio, x.data_ptr<float>(), x.stride(0), dy.data_ptr<float>(), dy.stride(0), part.data_ptr<float>(), (int)B,
                        (int)L, cur_stream()), "tf_wgrad");
  return part;
}
void eq_update(const at::Tensor& partials, at::Tensor g, at::Tensor m, at::Tensor v, int64_t k, double lr, double beta1, double beta2, double eps,
               bool peak) {
  f32_cuda(partials, "partials");
  TORCH_CHECK(partials.dim() == 3 && partials.size(2) == 513, "partials must be (B, segments, 513)");
  DMX_DEVICE_OF(partials);
  const int64_t B = partials.size(0);
  TORCH_CHECK(taps_of(g, partials, B, "g") == 513 && taps_of(m, partials, B, "m") == 513 && taps_of(v, partials, B, "v") == 513,
              "eq_update: g, m and v must be (B, 513) like the partial rows");
  ok(dmx_audio_eq_update(partials.data_ptr<float>(), (int)partials.size(1), g.data_ptr<float>(), m.data_ptr<float>(), v.data_ptr<float>(), (int)B,
                         (int)k, lr, beta1, beta2, eps, peak ? 1 : 0, cur_stream()), "eq_update");
}
at::Tensor noise_add(const at::Tensor& y, const at::Tensor& noise, double sigma) {
  f32_cuda(y, "y"); f32_cuda(noise, "noise");
  same_numel(y, noise, "noise_add(y, noise)");
  DMX_DEVICE_OF(y);
  at::Tensor out = at::empty_like(y);
  ok(dmx_noise_add(y.data_ptr<float>(), noise.data_ptr<float>(), out.data_ptr<float>(), y.numel(), (float)sigma, cur_stream()), "noise_add");
  return out;
}
// track mode (include/diffmusic_hip.h dmx_track_stitch_{fwd,bwd}): the windows wav (W, >= L) at `starts` -> the (1, T) track, and the transpose
at::Tensor track_stitch_fwd(const at::Tensor& wav, at::IntArrayRef starts, int64_t L, int64_t R, int64_t T) {
  TORCH_CHECK(wav.is_cuda() && wav.scalar_type() == at::kFloat && wav.dim() == 2 && wav.stride(1) == 1, "wav must be (W, >= L) fp32 on the GPU");
  TORCH_CHECK((int64_t)starts.size() == wav.size(0) && wav.size(1) >= L, "one start per window, windows of at least L samples");
  DMX_DEVICE_OF(wav);
  at::Tensor track = at::empty({1, T}, wav.options());
  std::vector<int> s(starts.begin(), starts.end());
  ok(dmx_track_stitch_fwd(wav.data_ptr<float>(), wav.stride(0), track.data_ptr<float>(), s.data(), (int)s.size(), (int)L, (int)R, (int)T, cur_stream()),
     "track_stitch_fwd");
  return track;
}
at::Tensor track_stitch_bwd(const at::Tensor& dtrack, at::IntArrayRef starts, int64_t L, int64_t R, int64_t Lfull) {
  f32_cuda(dtrack, "dtrack");
  TORCH_CHECK(!starts.empty(), "one start per window");
  DMX_DEVICE_OF(dtrack);
  at::Tensor dwav = at::empty({(int64_t)starts.size(), Lfull}, dtrack.options());
  std::vector<int> s(starts.begin(), starts.end());
  ok(dmx_track_stitch_bwd(dtrack.data_ptr<float>(), dwav.data_ptr<float>(), Lfull, s.data(), (int)s.size(), (int)L, (int)R, (int)dtrack.numel(), (int)Lfull,
                          cur_stream()), "track_stitch_bwd");
  return dwav;
}
// source separation (include/diffmusic_hip.h dmx_stem_mix_{fwd,bwd} / dmx_stem_project): K stems as the batch, rows stem-major; the launchers
// refuse what they can see (stem count, lengths, strides, gains), the wrappers what only they can (row count, gain count, devices)
struct StemGainsArg {
  std::vector<float> g;
  bool given = false;
  StemGainsArg(const std::optional<at::ArrayRef<double>>& gains, int64_t K, const char* what) {
    if (!gains.has_value()) return;
    TORCH_CHECK((int64_t)gains->size() == K, what, ": ", gains->size(), " gains for ", K, " stems");
    given = true;
    for (double v : *gains) g.push_back((float)v);
  }
  const float* ptr() const { return given ? g.data() : nullptr; }
};
inline void stem_rows_ok(const at::Tensor& x, int64_t rows, int64_t L, const char* what) {
  TORCH_CHECK(x.is_cuda(), what, ": a GPU tensor is required (the diffmusic_hip ops have no CPU fallback)");
  TORCH_CHECK(x.scalar_type() == at::kFloat && x.dim() == 2 && x.stride(1) == 1 && x.size(0) == rows && x.size(1) >= L, what, ": expected (", rows,
              ", >= ", L, ") fp32 with unit column stride");
}
at::Tensor stem_mix_fwd(const at::Tensor& wav, std::optional<at::ArrayRef<double>> gains, int64_t K, int64_t G, int64_t L) {
  stem_rows_ok(wav, K * G, L, "stem_mix_fwd");
  const StemGainsArg g(gains, K, "stem_mix_fwd");
  DMX_DEVICE_OF(wav);
  at::Tensor mix = at::empty({std::max<int64_t>(G, 0), std::max<int64_t>(L, 0)}, wav.options());
  ok(dmx_stem_mix_fwd(wav.data_ptr<float>(), wav.stride(0), mix.data_ptr<float>(), g.ptr(), (int)K, (int)G, (int)L, cur_stream()), "stem_mix_fwd");
  return mix;
}
at::Tensor stem_mix_bwd(const at::Tensor& dmix, std::optional<at::ArrayRef<double>> gains, int64_t K, int64_t Lfull) {
  TORCH_CHECK(dmix.is_cuda(), "stem_mix_bwd: dmix must be a GPU tensor (the diffmusic_hip ops have no CPU fallback)");
  TORCH_CHECK(dmix.scalar_type() == at::kFloat && dmix.dim() == 2 && dmix.is_contiguous(), "stem_mix_bwd: dmix must be contiguous (G, L) fp32");
  const StemGainsArg g(gains, K, "stem_mix_bwd");
  DMX_DEVICE_OF(dmix);
  const int64_t G = dmix.size(0), L = dmix.size(1);
  at::Tensor dwav = at::empty({std::max<int64_t>(K, 0) * G, std::max<int64_t>(Lfull, 0)}, dmix.options());
  ok(dmx_stem_mix_bwd(dmix.data_ptr<float>(), dwav.data_ptr<float>(), Lfull, g.ptr(), (int)K, (int)G, (int)L, (int)Lfull, cur_stream()), "stem_mix_bwd");
  return dwav;
}
at::Tensor stem_project(const at::Tensor& x, const at::Tensor& y, std::optional<at::ArrayRef<double>> gains, int64_t L) {
  const int64_t K = x.dim() == 2 ? x.size(0) : 0;
  stem_rows_ok(x, K, L, "stem_project");
  TORCH_CHECK(y.is_cuda() && y.scalar_type() == at::kFloat && y.is_contiguous() && y.numel() == L && y.device() == x.device(),
              "stem_project: y must be a contiguous (1, L) fp32 tensor on x's device");
  const StemGainsArg g(gains, K, "stem_project");
  DMX_DEVICE_OF(x);
  at::Tensor out = at::empty({K, L}, x.options());
  ok(dmx_stem_project(x.data_ptr<float>(), x.stride(0), y.data_ptr<float>(), out.data_ptr<float>(), g.ptr(), (int)K, (int)L, cur_stream()), "stem_project");
  return out;
}
at::Tensor stft_mag_fwd(int64_t audio, const at::Tensor& wav, const at::Tensor& state, int64_t L) {
  dmx_audio* a = reinterpret_cast<dmx_audio*>(audio);
  TORCH_CHECK(wav.is_cuda() && wav.scalar_type() == at::kFloat && wav.dim() == 2 && wav.stride(1) == 1, "wav must be (B, >= L) fp32 on the GPU");
  DMX_DEVICE_OF(wav);
  const int T = dmx_audio_num_frames(a, (int)L);
  TORCH_CHECK((size_t)state.nbytes() >= dmx_audio_state_bytes(a, (int)wav.size(0), (int)L), "state buffer too small");
  at::Tensor mag = at::empty({wav.size(0), dmx_audio_num_bins(a), T}, wav.options());
  ok(dmx_audio_stft_mag(a, wav.data_ptr<float>(), wav.stride(0), mag.data_ptr<float>(), state.data_ptr(), (int)wav.size(0), (int)L, cur_stream()), "stft_mag_fwd");
  return mag;
}
// dwav: caller-owned (B, >= L) result with any row stride, overwritten up to L; without it the op returns (B, Lfull) with zeros past L
at::Tensor stft_mag_bwd(int64_t audio, const at::Tensor& dmag, const at::Tensor& state, int64_t L, int64_t Lfull, const std::optional<at::Tensor>& dwav) {
  dmx_audio* a = reinterpret_cast<dmx_audio*>(audio);
  f32_cuda(dmag, "dmag");
  DMX_DEVICE_OF(dmag);
  at::Tensor d = rows_out(dwav, dmag, L, Lfull, true, "dwav");
  ok(dmx_audio_stft_mag_bwd(a, dmag.data_ptr<float>(), d.data_ptr<float>(), d.stride(0), state.data_ptr(), (int)dmag.size(0), (int)L, 0, cur_stream()), "stft_mag_bwd");
  return d;
}
at::Tensor melscale_fwd(int64_t audio, const at::Tensor& mag, double lo, double hi) {
  dmx_audio* a = reinterpret_cast<dmx_audio*>(audio);
  f32_cuda(mag, "mag");
  DMX_DEVICE_OF(mag);
  at::Tensor mel = at::empty({mag.size(0), mag.size(2), 64}, mag.options());
  ok(dmx_audio_melscale(a, mag.data_ptr<float>(), mel.data_ptr<float>(), (int)mag.size(0), (int)mag.size(2), (float)lo, (float)hi, cur_stream()), "melscale_fwd");
  return mel;
}

// ---- networks (handles from dmx_*_create; workspaces are caller-owned byte tensors sized by *_workspace_bytes)
// c0, c1, bias1 (all three or none): the AudioLDM2UNet2DConditionModel call (plpeline_audioldm2.py:1147-1154) with GPT-2 states c0 (B, n0, d0),
// T5 states c1 (B, n1, d1) + additive key bias.  out_channels: of the U-Net when they differ from x's; eps is (B, out_channels or C, h, w)
at::Tensor unet_fwd(int64_t model, const at::Tensor& x, const at::Tensor& t, const std::optional<at::Tensor>& class_labels, at::Tensor ws,
                    const std::optional<at::Tensor>& c0, const std::optional<at::Tensor>& c1, const std::optional<at::Tensor>& bias1,
                    std::optional<int64_t> out_channels) {
  f32_cuda(x, "x"); f32_cuda(t, "t");
  TORCH_CHECK(x.dim() == 4, "x must be (B, C, h, w)");
  if (class_labels) f32_cuda(*class_labels, "class_labels");
  TORCH_CHECK(c0.has_value() == c1.has_value() && c1.has_value() == bias1.has_value(), "unet_fwd: c0, c1 and bias1 go together, all three or none");
  if (c0) {
    f32_cuda(*c0, "encoder_hidden_states"); f32_cuda(*c1, "encoder_hidden_states_1"); f32_cuda(*bias1, "bias1");
    TORCH_CHECK(c0->dim() == 3 && c1->dim() == 3 && c0->size(0) == x.size(0) && c1->size(0) == x.size(0) && bias1->numel() == c1->size(0) * c1->size(1),
                "context tensors must be (B, tokens, dim) with one additive bias per T5 token");
  }
  DMX_DEVICE_OF(x);
  at::Tensor eps = at::empty({x.size(0), out_channels.value_or(x.size(1)), x.size(2), x.size(3)}, x.options());
  ok(dmx_unet_fwd_ctx(reinterpret_cast<dmx_model*>(model), x.data_ptr<float>(), t.data_ptr<float>(), fp(class_labels), fp(c0), c0 ? (int)c0->size(1) : 0,
                      fp(c1), c1 ? (int)c1->size(1) : 0, fp(bias1), eps.data_ptr<float>(), (int)x.size(0), (int)x.size(2), (int)x.size(3), ws.data_ptr(),
                      ws.nbytes(), cur_stream()), "unet_fwd");
  return eps;
}
// returns (mel 16-bit, mel fp32 or None): `vae.decode(z).sample` (scheduling_dps.py:195-197)
std::tuple<at::Tensor, std::optional<at::Tensor>> vae_dec_fwd(int64_t model, const at::Tensor& z, double z_scale, bool keep_state, bool want_f32,
                                                              int64_t scale_factor, at::Tensor ws) {
  f32_cuda(z, "z");
  DMX_DEVICE_OF(z);
  const int B = (int)z.size(0), h = (int)z.size(2), w = (int)z.size(3);
  at::Tensor mel = at::empty({B, scale_factor * h, scale_factor * w}, z.options().dtype(dmx_act_dtype() == 1 ? at::kHalf : at::kBFloat16));
  std::optional<at::Tensor> mel32;
  if (want_f32) mel32 = at::empty({B, scale_factor * h, scale_factor * w}, z.options());
  ok(dmx_vae_decode_fwd(reinterpret_cast<dmx_model*>(model), z.data_ptr<float>(), (float)z_scale, (uint16_t*)mel.data_ptr(),
                        mel32 ? mel32->data_ptr<float>() : nullptr, B, h, w, keep_state, ws.data_ptr(), ws.nbytes(), cur_stream()), "vae_dec_fwd");
  return {mel, mel32};
}
// `vae.encode(mel).latent_dist` moments (include/diffmusic_hip.h dmx_vae_encode_fwd): (B, h * w, 2 * latent) fp32
at::Tensor vae_enc_fwd(int64_t model, const at::Tensor& mel, double log_floor, int64_t latent_channels, int64_t scale_factor, at::Tensor ws) {
  f32_cuda(mel, "mel");
  TORCH_CHECK(mel.dim() == 3 && scale_factor >= 1, "mel must be (B, frames, bins)");
  DMX_DEVICE_OF(mel);
  const int B = (int)mel.size(0), T = (int)mel.size(1), F = (int)mel.size(2);
  at::Tensor mom = at::empty({B, (T / scale_factor) * (F / scale_factor), 2 * latent_channels}, mel.options());
  ok(dmx_vae_encode_fwd(reinterpret_cast<dmx_model*>(model), mel.data_ptr<float>(), (float)log_floor, mom.data_ptr<float>(), B, T, F,
                        ws.data_ptr(), ws.nbytes(), cur_stream()), "vae_enc_fwd");
  return mom;
}
// (mean, clamped logvar, noised start latent or None) from the moments (dmx_latent_init)
std::tuple<at::Tensor, at::Tensor, std::optional<at::Tensor>> latent_init(const at::Tensor& moments, int64_t h, int64_t w, const std::optional<at::Tensor>& eps,
                                                                          const std::optional<at::Tensor>& noise, double sqrt_abar, double scaling_factor,
                                                                          double sqrt_1m_abar, bool want_x) {
  f32_cuda(moments, "moments");
  TORCH_CHECK(moments.dim() == 3 && moments.size(1) == h * w && moments.size(2) % 2 == 0, "moments must be (B, h * w, 2 * latent_channels)");
  DMX_DEVICE_OF(moments);
  const int64_t B = moments.size(0), L = moments.size(2) / 2;
  at::Tensor mean = at::empty({B, L, h, w}, moments.options()), logvar = at::empty({B, L, h, w}, moments.options());
  if (eps) { f32_cuda(*eps, "eps"); same_numel(mean, *eps, "latent_init(eps)"); }
  if (noise) { f32_cuda(*noise, "noise"); same_numel(mean, *noise, "latent_init(noise)"); }
  std::optional<at::Tensor> x;
  if (want_x) x = at::empty({B, L, h, w}, moments.options());
  ok(dmx_latent_init(moments.data_ptr<float>(), mean.data_ptr<float>(), logvar.data_ptr<float>(), x ? x->data_ptr<float>() : nullptr, fp(eps), fp(noise),
                     (int)B, (int)L, (int)(h * w), (float)sqrt_abar, (float)scaling_factor, (float)sqrt_1m_abar, cur_stream()), "latent_init");
  return {mean, logvar, x};
}
// per-clip rescale of the waveform gradient before the 16-bit backward sweep (max |g| -> target), IN PLACE; returns the factors that undo it
at::Tensor grad_normalize_(at::Tensor dwav, double target) {
  f32_cuda(dwav, "dwav");
  TORCH_CHECK(dwav.dim() == 2, "dwav must be (B, samples)");
  DMX_DEVICE_OF(dwav);
  at::Tensor inv = at::empty({dwav.size(0)}, dwav.options());
  ok(dmx_grad_normalize(dwav.data_ptr<float>(), inv.data_ptr<float>(), (int)dwav.size(0), dwav.size(1), (float)target, cur_stream()), "grad_normalize");
  return inv;
}
at::Tensor vae_dec_bwd(int64_t model, const at::Tensor& dmel, double z_scale, int64_t latent_channels, int64_t scale_factor) {
  act_cuda(dmel, "dmel");
  DMX_DEVICE_OF(dmel);
  at::Tensor dz = at::empty({dmel.size(0), latent_channels, dmel.size(1) / scale_factor, dmel.size(2) / scale_factor}, dmel.options().dtype(at::kFloat));
  ok(dmx_vae_decode_bwd(reinterpret_cast<dmx_model*>(model), (const uint16_t*)dmel.data_ptr(), (float)z_scale, dz.data_ptr<float>(), cur_stream()), "vae_dec_bwd");
  return dz;
}
// [s0, s1): samples of every clip that the caller's loss never looks at: zeros there, the same bits elsewhere (an empty span: the plain forward)
at::Tensor hifigan_fwd(int64_t model, const at::Tensor& mel, at::Tensor ws, int64_t s0, int64_t s1) {
  act_cuda(mel, "mel");
  DMX_DEVICE_OF(mel);
  dmx_model* m = reinterpret_cast<dmx_model*>(model);
  const int B = (int)mel.size(0), T = (int)mel.size(1);
  at::Tensor wav = at::empty({B, dmx_hifigan_out_len(m, T)}, mel.options().dtype(at::kFloat));
  ok(dmx_hifigan_fwd_dead(m, (const uint16_t*)mel.data_ptr(), wav.data_ptr<float>(), B, T, (int)s0, (int)s1, ws.data_ptr(), ws.nbytes(), cur_stream()),
     "hifigan_fwd");
  return wav;
}
std::vector<int64_t> hifigan_dead_plan(int64_t model, int64_t stages) {
  const int n = (int)stages;
  std::vector<int> a[4];
  for (auto& v : a) v.assign(n > 0 ? n : 1, 0);
  TORCH_CHECK(dmx_hifigan_dead_plan(reinterpret_cast<dmx_model*>(model), a[0].data(), a[1].data(), a[2].data(), a[3].data(), n) >= 0, "hifigan_dead_plan");
  std::vector<int64_t> out;
  for (int s = 0; s < n; ++s) for (auto& v : a) out.push_back(v[s]);
  return out;
}
at::Tensor hifigan_bwd(int64_t model, const at::Tensor& dwav, int64_t frames, int64_t model_in_dim) {
  f32_cuda(dwav, "dwav");
  DMX_DEVICE_OF(dwav);
  at::Tensor dmel = at::empty({dwav.size(0), frames, model_in_dim}, dwav.options().dtype(dmx_act_dtype() == 1 ? at::kHalf : at::kBFloat16));
  ok(dmx_hifigan_bwd(reinterpret_cast<dmx_model*>(model), dwav.data_ptr<float>(), (uint16_t*)dmel.data_ptr(), cur_stream()), "hifigan_bwd");
  return dmel;
}

// ---- CLAP HTS-AT tower of the style-guidance operator (operator.py:253-271) and the Gram matrix of its token features
at::Tensor htsat_fwd(int64_t model, const at::Tensor& mel, bool keep_state, at::Tensor ws) {
  f32_cuda(mel, "mel");
  TORCH_CHECK(mel.dim() == 3, "mel must be (B, frames, mel bins)");
  DMX_DEVICE_OF(mel);
  dmx_model* m = reinterpret_cast<dmx_model*>(model);
  int tokens = 0, channels = 0;
  ok(dmx_htsat_feature_dims(m, &tokens, &channels), "htsat_feature_dims");
  at::Tensor feat = at::empty({mel.size(0), tokens, channels}, mel.options());
  ok(dmx_htsat_fwd(m, mel.data_ptr<float>(), (int)mel.size(0), (int)mel.size(1), feat.data_ptr<float>(), keep_state, ws.data_ptr(), ws.nbytes(),
                   cur_stream()), "htsat_fwd");
  return feat;
}
at::Tensor htsat_bwd(int64_t model, const at::Tensor& dfeat, const std::optional<at::Tensor>& scale, int64_t frames, int64_t bins) {
  f32_cuda(dfeat, "dfeat");
  DMX_DEVICE_OF(dfeat);
  if (scale) { f32_cuda(*scale, "scale"); TORCH_CHECK(scale->numel() == dfeat.size(0) && scale->device() == dfeat.device(), "scale must hold one value per clip"); }
  at::Tensor dmel = at::empty({dfeat.size(0), frames, bins}, dfeat.options());
  ok(dmx_htsat_bwd(reinterpret_cast<dmx_model*>(model), dfeat.data_ptr<float>(), fp(scale), dmel.data_ptr<float>(), cur_stream()), "htsat_bwd");
  return dmel;
}
at::Tensor gram_fwd(const at::Tensor& feat) {
  f32_cuda(feat, "feat");
  TORCH_CHECK(feat.dim() == 3, "feat must be (B, tokens, channels)");
  DMX_DEVICE_OF(feat);
  at::Tensor g = at::empty({feat.size(0), feat.size(2), feat.size(2)}, feat.options());
  ok(dmx_gram_fwd(feat.data_ptr<float>(), g.data_ptr<float>(), (int)feat.size(0), (int)feat.size(1), (int)feat.size(2), cur_stream()), "gram_fwd");
  return g;
}
at::Tensor gram_bwd(const at::Tensor& feat, const at::Tensor& dgram) {
  f32_cuda(feat, "feat"); f32_cuda(dgram, "dgram");
  TORCH_CHECK(feat.dim() == 3 && dgram.numel() == feat.size(0) * feat.size(2) * feat.size(2) && dgram.device() == feat.device(), "dgram must be (B, C, C)");
  DMX_DEVICE_OF(feat);
  at::Tensor d = at::empty_like(feat);
  ok(dmx_gram_bwd(feat.data_ptr<float>(), dgram.data_ptr<float>(), d.data_ptr<float>(), (int)feat.size(0), (int)feat.size(1), (int)feat.size(2), cur_stream()), "gram_bwd");
  return d;
}

}  // namespace

// the version of include/diffmusic_hip.h this op library was COMPILED against (the loaded libdiffmusic_hip.so reports its own through
// dmx_abi_version(); the two are compared when the library is loaded, below)
int64_t abi_version() { return DMX_ABI_VERSION; }

TORCH_LIBRARY(diffmusic_hip, m) {
  // A stale or copied op library would call entry points of another ABI version with this one's struct layouts and argument lists
  // (version 2 changed dmx_flash_attn_raw and GemmDesc): refuse to load instead -- torch.ops.load_library raises, and
  // diffmusic_amd.ops.enabled() falls back to the ctypes binding (which checks the same number) with one warning.
  TORCH_CHECK(dmx_abi_version() == DMX_ABI_VERSION, "libdiffmusic_torch_ops.so was built against C-ABI version ", DMX_ABI_VERSION,
              " but the loaded libdiffmusic_hip.so reports ", dmx_abi_version(), ": rebuild with `python -m diffmusic_amd.build`");
  {
    const std::pair<const char*, const void*> added[] = {{"dmx_vae_encoder_create", (const void*)&dmx_vae_encoder_create},
                                                         {"dmx_vae_encoder_workspace_bytes", (const void*)&dmx_vae_encoder_workspace_bytes},
                                                         {"dmx_vae_encode_fwd", (const void*)&dmx_vae_encode_fwd},
                                                         {"dmx_latent_init", (const void*)&dmx_latent_init},
                                                         {"dmx_track_stitch_fwd", (const void*)&dmx_track_stitch_fwd},
                                                         {"dmx_track_stitch_bwd", (const void*)&dmx_track_stitch_bwd},
                                                         {"dmx_audio_guidance_fwd_shaped", (const void*)&dmx_audio_guidance_fwd_shaped},
                                                         {"dmx_audio_guidance_bwd_shaped", (const void*)&dmx_audio_guidance_bwd_shaped},
                                                         {"dmx_clip_fwd", (const void*)&dmx_clip_fwd},
                                                         {"dmx_clip_bwd", (const void*)&dmx_clip_bwd},
                                                         {"dmx_declip_project", (const void*)&dmx_declip_project},
                                                         {"dmx_hifigan_fwd_dead", (const void*)&dmx_hifigan_fwd_dead},
                                                         {"dmx_hifigan_dead_plan", (const void*)&dmx_hifigan_dead_plan},
                                                         {"dmx_fir_clip_fwd", (const void*)&dmx_fir_clip_fwd},
                                                         {"dmx_fir_clip_bwd", (const void*)&dmx_fir_clip_bwd},
                                                         {"dmx_fir_wgrad", (const void*)&dmx_fir_wgrad},
                                                         {"dmx_fir_wgrad_workspace_floats", (const void*)&dmx_fir_wgrad_workspace_floats},
                                                         {"dmx_ir_update", (const void*)&dmx_ir_update},
                                                         {"dmx_stem_mix_fwd", (const void*)&dmx_stem_mix_fwd},
                                                         {"dmx_stem_mix_bwd", (const void*)&dmx_stem_mix_bwd},
                                                         {"dmx_stem_project", (const void*)&dmx_stem_project},
                                                         {"dmx_audio_tf_gain", (const void*)&dmx_audio_tf_gain},
                                                         {"dmx_audio_tf_frames", (const void*)&dmx_audio_tf_frames},
                                                         {"dmx_audio_tf_curve", (const void*)&dmx_audio_tf_curve},
                                                         {"dmx_audio_tf_wgrad_segments", (const void*)&dmx_audio_tf_wgrad_segments},
                                                         {"dmx_audio_tf_wgrad", (const void*)&dmx_audio_tf_wgrad},
                                                         {"dmx_audio_eq_update", (const void*)&dmx_audio_eq_update},
                                                         {"dmx_drc_fwd", (const void*)&dmx_drc_fwd},
                                                         {"dmx_drc_bwd", (const void*)&dmx_drc_bwd},
                                                         {"dmx_warp_fwd", (const void*)&dmx_warp_fwd},
                                                         {"dmx_warp_bwd", (const void*)&dmx_warp_bwd},
                                                         {"dmx_warp_wgrad", (const void*)&dmx_warp_wgrad},
                                                         {"dmx_warp_update", (const void*)&dmx_warp_update},
                                                         {"dmx_drc_fwd_p", (const void*)&dmx_drc_fwd_p},
                                                         {"dmx_drc_bwd_p", (const void*)&dmx_drc_bwd_p},
                                                         {"dmx_drc_pgrad", (const void*)&dmx_drc_pgrad},
                                                         {"dmx_drc_update", (const void*)&dmx_drc_update},
                                                         {"dmx_click_detect", (const void*)&dmx_click_detect},
                                                         {"dmx_click_mask", (const void*)&dmx_click_mask},
                                                         {"dmx_mask_rows", (const void*)&dmx_mask_rows},
                                                         {"dmx_declick_blend", (const void*)&dmx_declick_blend},
                                                         {"dmx_mdct_frames", (const void*)&dmx_mdct_frames},
                                                         {"dmx_mdct_quant", (const void*)&dmx_mdct_quant},
                                                         {"dmx_mdct_project", (const void*)&dmx_mdct_project}};
    for (const auto& s : added)
      TORCH_CHECK(s.second != nullptr, "the loaded libdiffmusic_hip.so reports C-ABI version ", DMX_ABI_VERSION, " but does not export `", s.first,
                  "` (a build from before the VAE encoder / track-mode / declipping / blind-dereverberation / source-separation / time-frequency-masking / blind-equalisation / de-compression / wow-and-flutter / blind-wow-and-flutter / blind-de-compression / declicking / codec-restoration entry points): rebuild with `python -m diffmusic_amd.build --force`");
  }
  m.def("abi_version() -> int", &abi_version);
  // Schemas: ops that write into a caller-owned tensor besides their outputs declare it (a!): `state` of the measurement front end
  // (written by *_fwd / mel_guidance, read by the matching *_bwd) and the network workspaces `ws` (written by *_fwd; the model handle's
  // tape points into it and *_bwd reads it), and the optional caller-owned results (`out`, `dwav`, `grad_out`), which an op that is given
  // one writes and returns.  One op per operation: what an operation can do beyond its plain form is a defaulted argument, keyword-only
  // where the ctypes function of the same name has it keyword-only (tests/test_abi.py holds the two signatures equal).  The C ABI keeps
  // its additive ladder (_ex / _shaped / _ctx / _dead) for C callers; an op calls the longest rung.  Handles travel as ints: effects behind a handle are invisible to the schema, so under
  // torch.compile / functionalization a forward and its backward must still be kept in program order by the caller (eager use today).
  m.def("sched_pred_x0(Tensor x, Tensor eps, float alpha_t, *, int ptype=0, float clip_r=0.0) -> Tensor", &sched_pred_x0);
  m.def("cfg_combine(Tensor eps2, float scale) -> Tensor", &cfg_combine);
  m.def("sched_update(int mode, Tensor x, Tensor eps, Tensor x0, Tensor? g0, Tensor? inv_scale, Tensor? noise, float alpha_t, float alpha_prev, "
        "float sigma, float rate, float eps_small, bool global_norm, *, int ptype=0, float clip_r=0.0, Tensor(a!)? grad_out=None) -> (Tensor, Tensor?)", &sched_update);
  m.def("randn_philox(int[] shape, int[] seeds, int offset, Device device) -> Tensor", &randn_philox);
  m.def("mask_mul(Tensor x, Tensor? mask, int L, int Ly) -> Tensor", &mask_mul);
  m.def("l2norm(Tensor ref, Tensor pred, float gscale, *, bool want_grad=True) -> (Tensor, Tensor?)", &l2norm);
  m.def("resample_fwd(Tensor x, Tensor h, int Lin, int Lout, int orig, int new_, int off) -> Tensor", &resample_fwd);
  m.def("resample_bwd(Tensor dy, Tensor h, Tensor? h_rev, int Lin, int Lfull, int orig, int new_, int off) -> Tensor", &resample_bwd);
  m.def("fir_clip_fwd(Tensor x, Tensor h, int Lin) -> Tensor", &fir_clip_fwd);
  m.def("fir_clip_bwd(Tensor dy, Tensor h, Tensor h_rev, int Lin, int Lfull) -> Tensor", &fir_clip_bwd);
  m.def("fir_wgrad(Tensor dy, Tensor x, int L, int taps) -> Tensor", &fir_wgrad);
  m.def("ir_update(Tensor partials, Tensor(a!) h, Tensor(b!) h_rev, Tensor(c!) m, Tensor(d!) v, int k, float lr, float beta1, float beta2, "
        "float eps) -> ()", &ir_update);
  m.def("logmel_fwd(int audio, Tensor wav, Tensor(a!) state, int L, bool power2, bool to_db, float lo, float hi, *, Tensor(b!)? out=None) -> Tensor", &logmel_fwd);
  m.def("logmel_bwd(int audio, Tensor dmel, Tensor state, int L, bool power2, bool to_db, float lo, float hi, *, Tensor(a!)? dwav=None) -> Tensor", &logmel_bwd);
  m.def("mel_guidance(int audio, Tensor wav, Tensor? mask, Tensor ref, Tensor(a!) state, int L, int Lfull, bool power2, bool to_db, float lo, "
        "float hi, float gscale, Tensor? noise=None, Tensor? noise_mag=None, float sigma=0.0, Tensor? thr=None) -> (Tensor, Tensor)", &mel_guidance);
  m.def("clip_fwd(Tensor x, Tensor thr, int L) -> Tensor", &clip_fwd);
  m.def("clip_bwd(Tensor dy, Tensor wav, Tensor thr, int Lfull) -> Tensor", &clip_bwd);
  m.def("declip_project(Tensor wav, Tensor measurement, Tensor thr, int L) -> Tensor", &declip_project);
  m.def("drc_fwd(Tensor x, int L, float threshold_db, float slope, float knee_db, float a_att, float a_rel, float makeup_db) -> (Tensor, Tensor, Tensor)",
        &drc_fwd);
  m.def("drc_bwd(Tensor dy, Tensor x, Tensor state, Tensor tape, int Lfull, float threshold_db, float slope, float knee_db, float a_att, float a_rel, "
        "float makeup_db) -> Tensor", &drc_bwd);
  m.def("drc_fwd_p(Tensor x, int L, Tensor theta, float knee_db) -> (Tensor, Tensor, Tensor)", &drc_fwd_p);
  m.def("drc_bwd_p(Tensor dy, Tensor x, Tensor state, Tensor tape, Tensor theta, int Lfull, float knee_db) -> (Tensor, Tensor, Tensor)", &drc_bwd_p);
  m.def("drc_pgrad(Tensor state, Tensor tape, Tensor work, Tensor bq0, Tensor theta, int L, float knee_db) -> Tensor", &drc_pgrad);
  m.def("drc_update(Tensor part, Tensor(a!) phi, Tensor(b!) m, Tensor(c!) v, Tensor(d!) theta, int L, int k, float[] lr, float beta1, "
        "float beta2, float eps, float knee_db, float[] lo, float[] hi) -> ()", &drc_update);
  m.def("warp_fwd(Tensor x, Tensor delay, int length) -> Tensor", &warp_fwd);
  m.def("warp_bwd(Tensor dy, Tensor delay, int length, int full) -> Tensor", &warp_bwd);
  m.def("warp_wgrad(Tensor dy, Tensor x, Tensor delay, int length) -> Tensor", &warp_wgrad);
  m.def("warp_update(Tensor part, Tensor(a!) coarse, Tensor(b!) m, Tensor(c!) v, Tensor(d!) fine, int length, int knot_stride, int k, float lr, "
        "float beta1, float beta2, float eps, float max_delay, bool mean) -> ()", &warp_update);
  m.def("click_detect(Tensor y, int L, float threshold, float sigma_floor) -> (Tensor, Tensor, Tensor, Tensor, Tensor)", &click_detect);
  m.def("click_mask(Tensor flags, int guard) -> (Tensor, Tensor)", &click_mask);
  m.def("mask_rows(Tensor x, Tensor mask, int L, int Ly) -> Tensor", &mask_rows);
  m.def("declick_blend(Tensor x, Tensor y, Tensor mask, int L, int fade) -> Tensor", &declick_blend);
  m.def("noise_add(Tensor y, Tensor noise, float sigma) -> Tensor", &noise_add);
  m.def("tf_gain(int audio, Tensor x, Tensor gain_t, int L, int Lfull, *, Tensor(a!)? out=None) -> Tensor", &tf_gain);
  m.def("mdct_quant(int audio, Tensor x, Tensor step_t, int L, int Lfull, *, bool passthrough=False, bool want_codes=False, "
        "Tensor(a!)? out=None) -> (Tensor, Tensor?)", &mdct_quant);
  m.def("mdct_project(int audio, Tensor x, Tensor step_t, Tensor codes, int L, int Lfull, *, Tensor(a!)? out=None) -> Tensor", &mdct_project);
  m.def("tf_curve(int audio, Tensor x, Tensor curve, int L, int Lfull) -> Tensor", &tf_curve);
  m.def("tf_wgrad(int audio, Tensor dy, Tensor x, int L) -> Tensor", &tf_wgrad);
  m.def("eq_update(Tensor partials, Tensor(a!) g, Tensor(b!) m, Tensor(c!) v, int k, float lr, float beta1, float beta2, float eps, bool peak) "
        "-> ()", &eq_update);
  m.def("track_stitch_fwd(Tensor wav, int[] starts, int L, int R, int T) -> Tensor", &track_stitch_fwd);
  m.def("track_stitch_bwd(Tensor dtrack, int[] starts, int L, int R, int Lfull) -> Tensor", &track_stitch_bwd);
  m.def("stem_mix_fwd(Tensor wav, float[]? gains, int K, int G, int L) -> Tensor", &stem_mix_fwd);
  m.def("stem_mix_bwd(Tensor dmix, float[]? gains, int K, int Lfull) -> Tensor", &stem_mix_bwd);
  m.def("stem_project(Tensor x, Tensor y, float[]? gains, int L) -> Tensor", &stem_project);
  m.def("stft_mag_fwd(int audio, Tensor wav, Tensor(a!) state, int L) -> Tensor", &stft_mag_fwd);
  m.def("stft_mag_bwd(int audio, Tensor dmag, Tensor state, int L, int Lfull, *, Tensor(a!)? dwav=None) -> Tensor", &stft_mag_bwd);
  m.def("melscale_fwd(int audio, Tensor mag, float lo, float hi) -> Tensor", &melscale_fwd);
  m.def("unet_fwd(int model, Tensor x, Tensor t, Tensor? class_labels, Tensor(a!) ws, Tensor? c0=None, Tensor? c1=None, Tensor? bias1=None, *, "
        "int? out_channels=None) -> Tensor", &unet_fwd);
  m.def("vae_dec_fwd(int model, Tensor z, float z_scale, bool keep_state, bool want_f32, int scale_factor, Tensor(a!) ws) -> (Tensor, Tensor?)", &vae_dec_fwd);
  m.def("vae_dec_bwd(int model, Tensor dmel, float z_scale, int latent_channels, int scale_factor) -> Tensor", &vae_dec_bwd);
  m.def("vae_enc_fwd(int model, Tensor mel, float log_floor, int latent_channels, int scale_factor, Tensor(a!) ws) -> Tensor", &vae_enc_fwd);
  m.def("latent_init(Tensor moments, int h, int w, Tensor? eps, Tensor? noise, float sqrt_abar, float scaling_factor, float sqrt_1m_abar, "
        "bool want_x) -> (Tensor, Tensor, Tensor?)", &latent_init);
  m.def("grad_normalize_(Tensor(a!) dwav, float target) -> Tensor", &grad_normalize_);
  m.def("hifigan_fwd(int model, Tensor mel, Tensor(a!) ws, int s0=0, int s1=0) -> Tensor", &hifigan_fwd);
  m.def("hifigan_bwd(int model, Tensor dwav, int frames, int model_in_dim) -> Tensor", &hifigan_bwd);
  m.def("hifigan_dead_plan(int model, int stages) -> int[]", &hifigan_dead_plan);
  m.def("htsat_fwd(int model, Tensor mel, bool keep_state, Tensor(a!) ws) -> Tensor", &htsat_fwd);
  m.def("htsat_bwd(int model, Tensor dfeat, Tensor? scale, int frames, int bins) -> Tensor", &htsat_bwd);
  m.def("gram_fwd(Tensor feat) -> Tensor", &gram_fwd);
  m.def("gram_bwd(Tensor feat, Tensor dgram) -> Tensor", &gram_bwd);
}
