// Blind equalisation (no counterpart in the reference): the gain of the time-frequency operator of tf_gain.hip is
// constant in time, G[k, t] = g[k], and UNKNOWN -- the guided loop fits one curve g[b, 0:513] per clip next to the audio.  Two kernels, fp32:
//
//   weight gradient  dg[b, k] = (h_k / (c 1024)) sum_{t = 0 .. T - 1} Re(X[k, t] conj(U[k, t])),  h_0 = h_512 = 1, else 2, c = 1.5
//                    X, U the analysis STFTs of x and of the cotangent u = dLoss/dy (both zero outside [0, L)) in the conventions of
//                    tf_gain.hip: n_fft 1024, hop 256, periodic Hann, T = ceil(L / 256) + 3, frame t at sample (t - 3) * 256
//   update           Adam on (g, m, v) from dg (adam_step.h, the arithmetic of ir_update), the clamp at zero (a magnitude response is not
//                    negative) and, optionally, the peak normalisation g <- g / max_k g that pins the scale between g and x
//
// A_g(x) = (1 / c) P^T W F^-1 diag(g) F W P x is linear in g, and <u, A_g x> = (1 / c) sum_t <F W P u, diag(g) F W P x> / 1024 over the full
// spectrum of 1024 bins; the bins k and 1024 - k carry the same g and conjugate products, which gives the formula above.
//
// tf_wgrad_kernel: grid (ceil(T / SEG), B), 256 threads.  Wave w takes the frames t0 + w, t0 + w + 4, ... of its segment, one at a time in
// its own LDS buffer: x with the window applied, fft1024<false>, its 9 bins k = lane + 64 j < 513 into registers, then u the same way in
// the SAME buffer, and acc[j] += X.x * U.x + X.y * U.y in increasing t.  The next frame's samples are fetched under the FFTs.  Two real
// transforms per frame instead of one packed complex one: the packed form computes Im(Z[k] Z[1024 - k]) / 2, in which |X|^2 - |U|^2 cancels
// only up to rounding -- its error does not vanish with u and grows with |X|^2; here U = 0 gives exactly +0 and the error is bilinear.
// The four waves' rows are combined through LDS as ((a0 + a1) + a2) + a3, times fp32(1 / 1536) and h_k, one row part[b, seg, 0:513] per
// workgroup: no atomics, an order fixed by t and SEG alone, so a clip's rows do not depend on the batch or on its place in it.  No halo:
// frames are not overlap-added.
//
// eq_update_kernel: one workgroup of 576 threads per clip, thread = bin; dg = the rows summed in segment order.
#include "dmx_common.h"
#include "kernels.h"
#include "fft1024.h"
#include "adam_step.h"
#include "../../include/diffmusic_hip.h"
#include <cstring>
void dmx_set_error(const char* fmt, ...);

namespace {

constexpr int NF = 1024;
constexpr int NB = NF / 2 + 1;
constexpr int HOP = 256;
constexpr int HALO = NF / HOP - 1;
constexpr int SEG = 16;                  // frames per workgroup: 40 x 8 workgroups at B = 8, L = 160000
constexpr float WG_SCALE = 1.f / 1536.f; // 1 / (c * 1024), c = 1.5 (rounded once)
constexpr int EQ_T = 576;                // update: nine waves, thread = bin

struct WgParams {
  const float* x; long long x_stride;
  const float* dy; long long dy_stride;
  float* part;                           // (B, S, 513)
  int L, T, S;
  const float2* tw;
  const float* win;
};

// samples n = lane + 64 j of frame t, zero outside [0, L) (nothing is read there)
__device__ __forceinline__ void wg_fetch(const float* __restrict__ xr, int L, int t, float (&x)[16], int lane) {
  const int p0 = (t - HALO) * HOP;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int s = p0 + lane + 64 * j;
    x[j] = (s >= 0 && s < L) ? xr[s] : 0.f;
  }
}

__global__ __launch_bounds__(256) void tf_wgrad_kernel(const WgParams P) {
  __shared__ float2 s_tw[NF];
  __shared__ float2 s_buf[4][NF];
  __shared__ float s_row[4][NB];
  // 48 KB of static LDS (twiddles, four frame buffers, four rows): three workgroups share a CU of gfx950 (160 KiB)
  static_assert(sizeof(float2) * NF * 5 + sizeof(float) * 4 * NB <= 80 * 1024, "tf_wgrad_kernel: at least two workgroups per CU must fit the 160 KiB of gfx950 LDS");
#if !defined(__gfx950__) && defined(__HIP_DEVICE_COMPILE__)
#error "tf_eq.hip sizes its LDS for gfx950 (160 KiB per CU)"
#endif
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y, seg = blockIdx.x;
  const int L = P.L;
  const int t0 = seg * SEG, t1 = min(t0 + SEG, P.T);
  for (int i = tid; i < NF; i += 256) s_tw[i] = P.tw[i];
  float win[16], xs[16], us[16], acc[9];
#pragma unroll
  for (int j = 0; j < 16; ++j) win[j] = P.win[lane + 64 * j];
#pragma unroll
  for (int j = 0; j < 9; ++j) acc[j] = 0.f;
  __syncthreads();
  const float* xr = P.x + (long long)b * P.x_stride;
  const float* ur = P.dy + (long long)b * P.dy_stride;
  float2* buf = s_buf[wave];
  if (t0 + wave < t1) {
    wg_fetch(xr, L, t0 + wave, xs, lane);
    wg_fetch(ur, L, t0 + wave, us, lane);
  }
  for (int t = t0 + wave; t < t1; t += 4) {                // wave-uniform
#pragma unroll
    for (int j = 0; j < 16; ++j) buf[lane + 64 * j] = make_float2(xs[j] * win[j], 0.f);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (t + 4 < t1) wg_fetch(xr, L, t + 4, xs, lane);      // in flight under this frame's two FFTs
    fft1024<false>(buf, s_tw, lane);
    float2 X[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      const int k = lane + 64 * j;
      X[j] = k < NB ? buf[k] : make_float2(0.f, 0.f);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
    for (int j = 0; j < 16; ++j) buf[lane + 64 * j] = make_float2(us[j] * win[j], 0.f);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (t + 4 < t1) wg_fetch(ur, L, t + 4, us, lane);
    fft1024<false>(buf, s_tw, lane);
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      const int k = lane + 64 * j;
      if (k < NB) {
        const float2 U = buf[k];
        acc[j] += X[j].x * U.x + X[j].y * U.y;             // Re(X conj(U))
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  }
#pragma unroll
  for (int j = 0; j < 9; ++j) {
    const int k = lane + 64 * j;
    if (k < NB) s_row[wave][k] = acc[j];
  }
  __syncthreads();
  float* row = P.part + ((long long)b * P.S + seg) * NB;
  for (int k = tid; k < NB; k += 256) {
    const float s = ((s_row[0][k] + s_row[1][k]) + s_row[2][k]) + s_row[3][k];
    row[k] = (s * WG_SCALE) * ((k == 0 || k == NF / 2) ? 1.f : 2.f);
  }
}

// One workgroup per clip, thread = bin: dg = the partial rows summed in segment order, Adam, the clamp at zero, max_k over the clip, the
// peak normalisation.  A clip with a non-finite dg or clamped step, or with a zero peak under the normalisation, is left exactly as it was.
__global__ __launch_bounds__(EQ_T) void eq_update_kernel(const float* __restrict__ ws, int nseg, float* __restrict__ g, float* __restrict__ m,
                                                         float* __restrict__ v, AdamStep a, int peak) {
  __shared__ float smax[EQ_T / 64];
  __shared__ int sbad[EQ_T / 64];
  const int b = blockIdx.x, k = threadIdx.x;
  const float* part = ws + (long long)b * nseg * NB;
  float mn = 0.f, vn = 0.f, gt = 0.f, mx = 0.f;
  int bad = 0;
  if (k < NB) {
    float d = 0.f;
    for (int s = 0; s < nseg; ++s) d += part[(long long)s * NB + k];
    float hn;
    adam_tap(d, m[(long long)b * NB + k], v[(long long)b * NB + k], g[(long long)b * NB + k], a, mn, vn, hn);
    gt = hn > 0.f ? hn : (hn != hn ? hn : 0.f);            // max(hn, 0) that keeps a NaN and gives +0
    bad = !(isfinite(d) && isfinite(gt));
    mx = bad ? 0.f : gt;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    mx = fmaxf(mx, __shfl_xor(mx, d, 64));
    bad |= __shfl_xor(bad, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    smax[threadIdx.x >> 6] = mx;
    sbad[threadIdx.x >> 6] = bad;
  }
  __syncthreads();
  for (int w = 0; w < EQ_T / 64; ++w) {
    mx = fmaxf(mx, smax[w]);
    bad |= sbad[w];
  }
  if (bad || (peak && !(mx > 0.f))) return;                 // uniform over the workgroup
  if (k < NB) {
    g[(long long)b * NB + k] = peak ? gt / mx : gt;
    m[(long long)b * NB + k] = mn;
    v[(long long)b * NB + k] = vn;
  }
}

}  // namespace

int dmx_tf_wgrad_segments(int L) { return cdiv(dmx_tf_gain_frames(L), SEG); }

int dmx_tf_wgrad(const DmxStftMelTables& t, const float* x, long long x_stride, const float* dy, long long dy_stride, float* part, int B, int L,
                 hipStream_t st) {
  if (!x || !dy || !part || B < 1 || B > 65535 || L < 1 || L > 0x7fffffff - 2 * NF || x_stride < L || dy_stride < L) return DMX_ERR_SHAPE;
  WgParams P;
  memset(&P, 0, sizeof(P));
  P.x = x; P.x_stride = x_stride; P.dy = dy; P.dy_stride = dy_stride; P.part = part;
  P.L = L; P.T = dmx_tf_gain_frames(L); P.S = cdiv(P.T, SEG); P.tw = t.tw; P.win = t.win;
  hipLaunchKernelGGL(tf_wgrad_kernel, dim3(P.S, B), dim3(256), 0, st, P);
  return hipGetLastError() == hipSuccess ? DMX_OK : DMX_ERR_LAUNCH;
}

extern "C" int dmx_audio_eq_update(const float* partials, int segments, float* g, float* m, float* v, int batch, int k, double lr, double beta1,
                                   double beta2, double eps, int normalize, void* stream) {
  if (!partials || !g || !m || !v || batch < 1 || segments < 1) {
    dmx_set_error("eq_update: partials (batch, segments, 513) with segments >= 1, g, m and v (batch, 513) are required");
    return DMX_ERR_SHAPE;
  }
  if (!adam_args_ok(lr, beta1, beta2, eps, k)) {
    dmx_set_error("eq_update: lr > 0, betas in [0, 1), eps >= 0 and k >= 1 (the 1-based count of updates) are required");
    return DMX_ERR_SHAPE;
  }
  if (normalize != 0 && normalize != 1) {
    dmx_set_error("eq_update: normalize is 0 (none) or 1 (peak)");
    return DMX_ERR_SHAPE;
  }
  hipLaunchKernelGGL(eq_update_kernel, dim3((unsigned)batch), dim3(EQ_T), 0, (hipStream_t)stream, partials, segments, g, m, v,
                     adam_step_of(lr, beta1, beta2, eps, k), normalize);
  return hipGetLastError() == hipSuccess ? DMX_OK : DMX_ERR_LAUNCH;
}
