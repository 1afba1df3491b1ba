// Blind de-compression (no counterpart in the reference): the parameters of the compressor of drc.hip (section 8.9)
// are UNKNOWN -- the guided loop fits them next to the audio.  Per clip the fitted vector is phi = (T, k, m, ln aA, ln aR): threshold in dB,
// slope k = 1 - 1 / ratio, make-up in dB and the logarithms of the attack and release coefficients; the knee width W is given.  The kernels
// of drc.hip read the table row theta[b] = (T, k, m, aA, aR, 1 - aA, 1 - aR, k / (2 W)) that the update writes.  Two kernels, fp32:
//
//   drc_pgrad   the gradient of a loss in phi from what dmx_drc_fwd_p / dmx_drc_bwd_p left: state (p, s), the tape, the work rows ds and dc,
//               Bq[0].  With d, c and c' by the tape's region (drc_common.h: the expressions of drc_power and drc_apply_bwd) and
//               s[-1] = 0, per block j
//                 tT = -(dc c')      tk = dc e,  e = 0 | (d + W/2)^2 (1 / (2 W)) | d by region      tA = att ? dc (c - s[j-1]) : 0
//                 tR = att ? 0 : dc (c - s[j-1])      tm = -ds
//               A workgroup of 256 threads owns a segment of 256 blocks, thread = block (one term per sum and thread; blocks past H give +0);
//               each sum is the butterfly v <- v + v(lane xor t), t = 32 .. 1, inside a wave, then the four waves in ascending order.
//               Segment 0 adds (ln 10 / 20) G[-1] Bq[0] to its tm sum, G[-1] = block_gain(0, m).  part[b, seg, 0:5] = (gT, gk, gm, glnA,
//               glnR) of the segment.  No atomics: a clip's rows are the same bits alone, in a batch and at another batch position.
//   drc_update  one wave per clip, lane q < 5 owns parameter q: its gradient is the sum of part[b, seg, q] over seg ascending from +0; one
//               Adam step (adam_step.h) with its own lr[q]; the clamp to the caller's box; then the lane rewrites its entries of theta[b]:
//               T | k and kq = (float)((double)k / (2 (double)W)) (0 when W = 0) | m | aA = expf(ln aA) and bA = (float)(1 - (double)aA) |
//               aR, bR.  lr[q] = 0 freezes parameter q: its value, its moments and its table entries keep their bits.  A clip with a
//               non-finite gradient (any of the five) or a non-finite step of a live parameter keeps its whole state, decided on the device.
//               Any bits in `part` are safe: nothing is indexed by a value.
// The boxes keep every row the update writes inside the contract of dmx_drc_fwd: |T|, |m| <= 200, 0 <= k <= 1, ln a in [-80, 0] so that
// 0 < expf(ln a) <= 1.
#include "dmx_common.h"
#include "kernels.h"
#include "drc_common.h"
#include "adam_step.h"
#include "../../include/diffmusic_hip.h"
#include <cmath>
void dmx_set_error(const char* fmt, ...);

namespace {

constexpr int SEG = DMX_DRC_FIT_SEGMENT;   // blocks per segment = threads of the gradient's workgroup
constexpr int NP = DMX_DRC_FIT_PARAMS;     // 5
constexpr int MAX_L = 1 << 30;
constexpr float LN10_20 = 0.11512925464970229f;

struct Five { float v0, v1, v2, v3, v4; };
__device__ __forceinline__ float pick(const Five& f, int q) { return q == 0 ? f.v0 : q == 1 ? f.v1 : q == 2 ? f.v2 : q == 3 ? f.v3 : f.v4; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int t = 32; t >= 1; t >>= 1) v = __fadd_rn(v, __shfl_xor(v, t, 64));
  return v;
}

__global__ __launch_bounds__(SEG) void drc_pgrad_kernel(const float* __restrict__ state, const unsigned char* __restrict__ tape,
                                                        const float* __restrict__ work, const float* __restrict__ bq0, float* __restrict__ part,
                                                        int H, int nseg, float inv2W, ByTable src) {
  __shared__ float ws[SEG / 64][NP];
  const int b = blockIdx.y, seg = blockIdx.x, tid = threadIdx.x, j = seg * SEG + tid;
  const DrcParams P = src.clip(b);
  float t[NP] = {0.f, 0.f, 0.f, 0.f, 0.f};
  if (j < H) {
    const int tp = tape[(size_t)b * H + j], rg = tp & 3;
    const float p = state_row(state, b, H, 0)[j];
    const float sprev = j > 0 ? state_row(state, b, H, 2)[j - 1] : 0.f;
    const float ds = work[(size_t)b * 2 * H + j], dc = work[((size_t)b * 2 + 1) * H + j];
    const float d = level_over_threshold(p, P.T);
    const float c = curve_by_region(d, rg, P), cp = curve_slope(p, rg, P);
    float e = 0.f;
    if (rg == 2) e = d;
    else if (rg == 1) { const float u = d + P.halfW; e = __fmul_rn(__fmul_rn(u, u), inv2W); }
    const float lag = __fmul_rn(dc, __fsub_rn(c, sprev));
    t[0] = -__fmul_rn(dc, cp);
    t[1] = __fmul_rn(dc, e);
    t[2] = -ds;
    t[3] = (tp & 4) ? lag : 0.f;
    t[4] = (tp & 4) ? 0.f : lag;
  }
#pragma unroll
  for (int q = 0; q < NP; ++q) t[q] = wave_sum(t[q]);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int q = 0; q < NP; ++q) ws[tid >> 6][q] = t[q];
  }
  __syncthreads();
  if (tid < NP) {
    float g = ws[0][tid];
#pragma unroll
    for (int w = 1; w < SEG / 64; ++w) g = __fadd_rn(g, ws[w][tid]);
    if (tid == 2 && seg == 0) g = __fadd_rn(g, __fmul_rn(__fmul_rn(LN10_20, block_gain(0.f, P.makeup)), bq0[b]));
    part[((size_t)b * nseg + seg) * NP + tid] = g;
  }
}

struct Box { Five lo, hi; };

__global__ __launch_bounds__(64) void drc_update_kernel(const float* __restrict__ part, float* __restrict__ phi, float* __restrict__ m,
                                                        float* __restrict__ v, float* __restrict__ theta, int nseg, AdamStep a, Five lr, Box box,
                                                        float W) {
  const int b = blockIdx.x, q = threadIdx.x;
  const bool mine = q < NP;
  float g = 0.f, mn = 0.f, vn = 0.f, hn = 0.f;
  bool live = false, bad = false;
  if (mine) {
    for (int s = 0; s < nseg; ++s) g = __fadd_rn(g, part[((size_t)b * nseg + s) * NP + q]);
    a.lr = pick(lr, q);
    live = a.lr != 0.f;
    adam_tap(g, m[(size_t)b * NP + q], v[(size_t)b * NP + q], phi[(size_t)b * NP + q], a, mn, vn, hn);
    bad = !isfinite(g) || (live && !(isfinite(hn) && isfinite(mn) && isfinite(vn)));
  }
  if (__any(bad)) return;                                    // the whole clip keeps its state
  if (!mine || !live) return;
  hn = fminf(fmaxf(hn, pick(box.lo, q)), pick(box.hi, q));
  phi[(size_t)b * NP + q] = hn;
  m[(size_t)b * NP + q] = mn;
  v[(size_t)b * NP + q] = vn;
  float* row = theta + (size_t)b * DRC_ROW;
  if (q == 0) row[0] = hn;
  else if (q == 1) { row[1] = hn; row[7] = W > 0.f ? (float)((double)hn / (2.0 * (double)W)) : 0.f; }
  else if (q == 2) row[2] = hn;
  else {
    const float al = expf(hn);                               // in (0, 1]: ln a is boxed to [-80, 0]
    row[q] = al;                                             // 3: aA, 4: aR
    row[q + 2] = (float)(1.0 - (double)al);                  // 5: bA, 6: bR
  }
}

}  // namespace

extern "C" int dmx_drc_pgrad(const float* state, const unsigned char* tape, const float* work, const float* bq0, const float* theta, float* part,
                             int batch, int L, float knee_db, void* stream) {
  if (!state || !tape || !work || !bq0 || !theta || !part || batch < 1 || batch > 65535 || L < 1 || L > MAX_L ||
      !(std::isfinite(knee_db) && knee_db >= 0.f && knee_db <= 200.f)) {
    dmx_set_error("drc_pgrad: state (batch, 3, H), tape (batch, H), work (batch, 2, H), bq0 (batch,), theta (batch, 8), part (batch, "
                  "ceil(H / 256), 5), all contiguous, H = ceil(L / 64), 1 <= batch <= 65535, 1 <= L <= 2^30, 0 <= knee_db <= 200");
    return DMX_ERR_SHAPE;
  }
  const int H = cdiv(L, R), nseg = cdiv(H, SEG);
  const float inv2W = knee_db > 0.f ? (float)(1.0 / (2.0 * (double)knee_db)) : 0.f;
  hipLaunchKernelGGL(drc_pgrad_kernel, dim3((unsigned)nseg, (unsigned)batch), dim3(SEG), 0, (hipStream_t)stream, state, tape, work, bq0, part, H,
                     nseg, inv2W, ByTable{theta, knee_db});
  return hipGetLastError() == hipSuccess ? DMX_OK : DMX_ERR_LAUNCH;
}

extern "C" int dmx_drc_update(const float* part, float* phi, float* m, float* v, float* theta, int batch, int L, int k, const double* lr,
                              double beta1, double beta2, double eps, float knee_db, const double* lo, const double* hi, void* stream) {
  if (!part || !phi || !m || !v || !theta || !lr || !lo || !hi || batch < 1 || L < 1 || L > MAX_L ||
      !(std::isfinite(knee_db) && knee_db >= 0.f && knee_db <= 200.f)) {
    dmx_set_error("drc_update: part (batch, ceil(H / 256), 5), phi, m and v (batch, 5), theta (batch, 8), all contiguous, lr, lo and hi five "
                  "host doubles each, H = ceil(L / 64), batch >= 1, 1 <= L <= 2^30, 0 <= knee_db <= 200");
    return DMX_ERR_SHAPE;
  }
  bool lr_ok = true;
  for (int q = 0; q < NP; ++q) lr_ok = lr_ok && std::isfinite(lr[q]) && lr[q] >= 0.0;
  if (!lr_ok || !adam_args_ok(1.0, beta1, beta2, eps, k)) {
    dmx_set_error("drc_update: every lr finite and >= 0 (0 freezes that parameter), betas in [0, 1), eps >= 0 and k >= 1 (the 1-based count "
                  "of updates) are required");
    return DMX_ERR_SHAPE;
  }
  // the box: T and m within +-200, k within [0, 1], ln a within [-80, 0]
  const double wlo[NP] = {-200.0, 0.0, -200.0, -80.0, -80.0}, whi[NP] = {200.0, 1.0, 200.0, 0.0, 0.0};
  for (int q = 0; q < NP; ++q) {
    const float l = (float)lo[q], h = (float)hi[q];
    if (!(l <= h && l >= (float)wlo[q] && h <= (float)whi[q])) {
      dmx_set_error("drc_update: the box needs lo <= hi with T and makeup within +-200 dB, the slope within [0, 1] and ln a within [-80, 0]; "
                    "entry %d is [%g, %g]", q, lo[q], hi[q]);
      return DMX_ERR_SHAPE;
    }
  }
  const int H = cdiv(L, R), nseg = cdiv(H, SEG);
  const Five lr5 = {(float)lr[0], (float)lr[1], (float)lr[2], (float)lr[3], (float)lr[4]};
  const Box box = {{(float)lo[0], (float)lo[1], (float)lo[2], (float)lo[3], (float)lo[4]},
                   {(float)hi[0], (float)hi[1], (float)hi[2], (float)hi[3], (float)hi[4]}};
  hipLaunchKernelGGL(drc_update_kernel, dim3((unsigned)batch), dim3(64), 0, (hipStream_t)stream, part, phi, m, v, theta, nseg,
                     adam_step_of(1.0, beta1, beta2, eps, k), lr5, box, knee_db);
  return hipGetLastError() == hipSuccess ? DMX_OK : DMX_ERR_LAUNCH;
}
