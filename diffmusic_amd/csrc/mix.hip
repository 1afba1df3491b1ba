// Source separation: K stems as the batch, mixed under ONE loss (inverse_problem/mixture.py).  Rows are stem-major: row k * G + w is
// stem k of group w (G = 1 for one window, G = W for the windows of a track).
//
//   M    (stem_mix_fwd): mix[w, n]         = ((g_0 x[0 G + w, n] + g_1 x[1 G + w, n]) + ...)    ascending k, n < L
//   M^T  (stem_mix_bwd): dwav[k G + w, i]  = g_k dmix[w, i]                                     for i < L, +0.0f for L <= i < full
//   P    (stem_project): p[k, n]           = x[k, n] + c_k (y[n] - mix(x)[n]),  c_k = g_k / sum_j g_j^2    (G = 1)
//
// Every product and every sum is rounded on its own (the meaning of __fmul_rn / __fadd_rn: no contraction into an FMA; see `fmul_rn`
// below for why they are restated here), and the first term of a sum is taken as it is: a plain fp32 torch loop restates each kernel bit
// for bit, and K = 1, g = 1 copies (-0.0f and NaN included).  P is the minimum-norm correction after which the stems sum to the mixture:
// r = y - mix(x) in M's own op order, then a separate multiply and add per stem.
//
// All three are one pass: 4 consecutive samples per lane, 16-byte loads and stores where a row's address allows it (decided per row:
// strides are arbitrary and a row may sit 4 bytes off), scalar otherwise, no atomics, no table in memory -- the gains travel by value in
// the kernel arguments (K <= 16, 64 bytes).  M reads K G L floats and writes G L; M^T reads G L and writes K G full.  At K = 4,
// L = 163 840 that is 3.3 MB and 3.3 MB: launch latency, next to a vocoder step.
#include <cmath>

#include "dmx_common.h"
#include "kernels.h"
#include "../../include/diffmusic_hip.h"
void dmx_set_error(const char* fmt, ...);

// No expression of this file may be contracted.  The toolkit's __fmul_rn / __fadd_rn are a plain `*` and `+` compiled under the contraction
// mode of its own header, so a product that feeds a sum through them still fuses once both are inlined; these two are the same operations
// under this pragma, which is what keeps them apart.
#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ float fmul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float fadd_rn(float a, float b) { return a + b; }

constexpr int MIX_MAX_STEMS = 16;
struct StemGains { float g[MIX_MAX_STEMS]; };

__device__ __forceinline__ bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// samples i .. i + 3 of a row with n valid samples (positions >= n read nothing and give 0)
__device__ __forceinline__ void load4(const float* row, int i, int n, float (&v)[4]) {
  if (i + 3 < n && aligned16(row + i)) {
    const float4 t = *reinterpret_cast<const float4*>(row + i);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = i + e < n ? row[i + e] : 0.f;
  }
}
__device__ __forceinline__ void store4(float* row, int i, int n, const float (&v)[4]) {
  if (i + 3 < n && aligned16(row + i)) {
    *reinterpret_cast<float4*>(row + i) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) if (i + e < n) row[i + e] = v[e];
  }
}

// acc = ((g_0 x_0 + g_1 x_1) + ...) of samples i .. i + 3 of group w; rows k * G + w of `wav`
__device__ __forceinline__ void mix4(const float* __restrict__ wav, long long stride, const StemGains& a, int K, int G, int w, int i, int L,
                                     float (&acc)[4]) {
  for (int k = 0; k < K; ++k) {
    float v[4];
    load4(wav + ((long long)k * G + w) * stride, i, L, v);
    const float g = a.g[k];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float term = fmul_rn(g, v[e]);
      acc[e] = k == 0 ? term : fadd_rn(acc[e], term);      // the first term is taken as it is: -0.0f stays -0.0f
    }
  }
}

// grid (ceil(L / 4 / 256), G)
__global__ __launch_bounds__(256) void stem_mix_fwd_kernel(const float* __restrict__ wav, long long stride, float* __restrict__ mix, StemGains a,
                                                           int K, int G, int L) {
  const long long il = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (il >= L) return;
  const int i = (int)il, w = blockIdx.y;
  float acc[4];
  mix4(wav, stride, a, K, G, w, i, L, acc);
  store4(mix + (long long)w * L, i, L, acc);
}

// grid (ceil(full / 4 / 256), K * G)
__global__ __launch_bounds__(256) void stem_mix_bwd_kernel(const float* __restrict__ dmix, float* __restrict__ dwav, long long stride, StemGains a,
                                                           int G, int L, int full) {
  const long long il = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (il >= full) return;
  const int i = (int)il, row = blockIdx.y, k = row / G, w = row - k * G;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (i < L) {
    load4(dmix + (long long)w * L, i, L, v);
    const float g = a.g[k];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = i + e < L ? fmul_rn(g, v[e]) : 0.f;      // the tail past L is +0.0f whatever the gain's sign
  }
  store4(dwav + (long long)row * stride, i, full, v);
}

// grid (ceil(L / 4 / 256)); c holds c_k = g_k / sum_j g_j^2
__global__ __launch_bounds__(256) void stem_project_kernel(const float* __restrict__ x, long long stride, const float* __restrict__ y,
                                                           float* __restrict__ out, StemGains a, StemGains c, int K, int L) {
  const long long il = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (il >= L) return;
  const int i = (int)il;
  float r[4], m[4];
  mix4(x, stride, a, K, 1, 0, i, L, m);
  load4(y, i, L, r);
#pragma unroll
  for (int e = 0; e < 4; ++e) r[e] = fadd_rn(r[e], -m[e]);
  for (int k = 0; k < K; ++k) {
    float v[4];
    load4(x + (long long)k * stride, i, L, v);
    const float ck = c.g[k];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = fadd_rn(v[e], fmul_rn(ck, r[e]));
    store4(out + (long long)k * L, i, L, v);
  }
}

// the gains a launch may carry: K in 1 .. 16 finite values, a null host pointer = all ones
int check_gains(const char* what, const float* gains_host, int K, StemGains* out) {
  if (K < 1 || K > MIX_MAX_STEMS) { dmx_set_error("%s: 1 <= stems <= %d (got %d)", what, MIX_MAX_STEMS, K); return DMX_ERR_SHAPE; }
  for (int k = 0; k < MIX_MAX_STEMS; ++k) out->g[k] = k < K ? (gains_host ? gains_host[k] : 1.0f) : 0.0f;
  for (int k = 0; k < K; ++k)
    if (!std::isfinite(out->g[k])) { dmx_set_error("%s: gain %d is not finite", what, k); return DMX_ERR_PARAM; }
  return DMX_OK;
}

// blocks of 256 lanes x 4 samples over n samples; 0 when the count does not fit a grid dimension
unsigned blocks_x(int n) {
  const long long b = (((long long)n + 3) / 4 + 255) / 256;
  return b >= 1 && b <= 2147483647LL ? (unsigned)b : 0u;
}

}  // namespace

extern "C" int dmx_stem_mix_fwd(const float* wav, long long wav_stride, float* mix, const float* gains_host, int stems, int groups, int L,
                                void* stream) {
  StemGains a;
  const int rc = check_gains("stem_mix_fwd", gains_host, stems, &a);
  if (rc != DMX_OK) return rc;
  if (groups < 1 || L < 1) { dmx_set_error("stem_mix_fwd: groups >= 1 and L >= 1 (groups=%d L=%d)", groups, L); return DMX_ERR_SHAPE; }
  if (!wav || !mix || wav_stride < L) { dmx_set_error("stem_mix_fwd: wav (stems * groups, >= L) with row stride >= L and mix (groups, L) are required"); return DMX_ERR_SHAPE; }
  const unsigned bx = blocks_x(L);
  if (bx == 0 || groups > 65535) { dmx_set_error("stem_mix_fwd: grid out of range (groups=%d <= 65535, L=%d)", groups, L); return DMX_ERR_SHAPE; }
  hipLaunchKernelGGL(stem_mix_fwd_kernel, dim3(bx, (unsigned)groups), dim3(256), 0, (hipStream_t)stream, wav, wav_stride, mix, a, stems, groups, L);
  return hipGetLastError() == hipSuccess ? DMX_OK : DMX_ERR_LAUNCH;
}

extern "C" int dmx_stem_mix_bwd(const float* dmix, float* dwav, long long dwav_stride, const float* gains_host, int stems, int groups, int L,
                                int full, void* stream) {
  StemGains a;
  const int rc = check_gains("stem_mix_bwd", gains_host, stems, &a);
  if (rc != DMX_OK) return rc;
  if (groups < 1 || L < 1) { dmx_set_error("stem_mix_bwd: groups >= 1 and L >= 1 (groups=%d L=%d)", groups, L); return DMX_ERR_SHAPE; }
  if (full < L) { dmx_set_error("stem_mix_bwd: full >= L (full=%d L=%d)", full, L); return DMX_ERR_SHAPE; }
  if (!dmix || !dwav || dwav_stride < full) {
    dmx_set_error("stem_mix_bwd: dmix (groups, L) and dwav (stems * groups, full) with row stride >= full are required");
    return DMX_ERR_SHAPE;
  }
  const unsigned bx = blocks_x(full);
  const long long rows = (long long)stems * groups;
  if (bx == 0 || rows > 65535) { dmx_set_error("stem_mix_bwd: grid out of range (stems * groups=%lld <= 65535, full=%d)", rows, full); return DMX_ERR_SHAPE; }
  hipLaunchKernelGGL(stem_mix_bwd_kernel, dim3(bx, (unsigned)rows), dim3(256), 0, (hipStream_t)stream, dmix, dwav, dwav_stride, a, groups, L, full);
  return hipGetLastError() == hipSuccess ? DMX_OK : DMX_ERR_LAUNCH;
}

extern "C" int dmx_stem_project(const float* x, long long x_stride, const float* y, float* out, const float* gains_host, int stems, int L,
                                void* stream) {
  StemGains a, c;
  const int rc = check_gains("stem_project", gains_host, stems, &a);
  if (rc != DMX_OK) return rc;
  if (L < 1) { dmx_set_error("stem_project: L >= 1 (L=%d)", L); return DMX_ERR_SHAPE; }
  if (!x || !y || !out || x_stride < L) { dmx_set_error("stem_project: x (stems, >= L) with row stride >= L, y (1, L) and out (stems, L) are required"); return DMX_ERR_SHAPE; }
  double ss = 0.0;
  for (int k = 0; k < stems; ++k) ss += (double)a.g[k] * (double)a.g[k];
  for (int k = 0; k < MIX_MAX_STEMS; ++k) c.g[k] = k < stems ? (float)((double)a.g[k] / ss) : 0.0f;      // float64, rounded once
  for (int k = 0; k < stems; ++k)
    if (!std::isfinite(c.g[k])) { dmx_set_error("stem_project: the gains give no finite correction (sum of squares %g)", ss); return DMX_ERR_PARAM; }
  const unsigned bx = blocks_x(L);
  if (bx == 0) { dmx_set_error("stem_project: grid out of range (L=%d)", L); return DMX_ERR_SHAPE; }
  hipLaunchKernelGGL(stem_project_kernel, dim3(bx), dim3(256), 0, (hipStream_t)stream, x, x_stride, y, out, a, c, stems, L);
  return hipGetLastError() == hipSuccess ? DMX_OK : DMX_ERR_LAUNCH;
}
