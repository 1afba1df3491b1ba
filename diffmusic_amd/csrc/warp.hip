// Wow and flutter on materialised waveforms (the time-warp operator; no counterpart in the reference): the clip read at a position that
// drifts against the sample clock by a given, slowly varying delay curve, and the transpose of that linear map.  DESIGN.md section 8.10 has
// the definition; per clip, x zero outside [0, L), R = 64 samples per block, H = ceil(L / 64), the curve H + 1 knots d[0 .. H] in samples:
//
//   n = 64 j + r      delta(n) = d[j] + (r / 64) (d[j+1] - d[j])      i(n) = n + (int) floorf(delta)      f(n) = delta - floorf(delta) in [0, 1]
//   w[-1] = f ((-0.5 f + 1) f - 0.5)    w[0] = (1.5 f - 2.5) (f f) + 1    w[1] = f ((-1.5 f + 2) f + 0.5)    w[2] = (f f) (0.5 f - 0.5)
//   y[n]  = sum over k = -1, 0, 1, 2 with 0 <= i + k < L of w[k] x[i + k]                            (four-point Catmull-Rom)
//   dx[m] = sum over n, ascending, with i(n) in [m - 2, m + 1] of w[m - i(n)](f(n)) dy[n]            (the transpose, as a gather)
//
// Arithmetic, in this order whatever the batch, the batch position or the load path (explicit fmaf / __fmul_rn / __fsub_rn, so the build's
// contraction cannot change it):
//   delta = fmaf(r / 64, d[j+1] - d[j], d[j])         r / 64 is exact; fl = floorf(delta); f = delta - fl
//   w[-1] = f * fmaf(fmaf(-0.5, f, 1), f, -0.5)       w[0] = fmaf(fmaf(1.5, f, -2.5), f * f, 1)
//   w[1]  = f * fmaf(fmaf(-1.5, f, 2), f, 0.5)        w[2] = (f * f) * fmaf(0.5, f, -0.5)
//   acc = +0, then acc = fmaf(w, v, acc) once per term: the taps k = -1, 0, 1, 2 in the forward, the contributing n ascending in the
//   transpose.  A tap outside [0, L) is skipped: neither loaded nor multiplied.
// d = 0 therefore returns x bit for bit and a constant integer d the shifted x (f = 0 gives the weights 0, 1, 0, 0 exactly), and f = 1 (a
// tiny negative delta rounds there) gives 0, 0, 1, 0: the same sample as f = 0 one tap on.  A NaN at x[m] reaches exactly the y[n] whose
// four taps include m -- a zero weight times NaN is NaN -- and a NaN at dy[n] exactly the dx[m] among the taps of n.
//
//   warp_fwd   a thread owns four consecutive outputs (one block, one pair of knots); the taps are plain cached loads, the store follows
//              the float4 / scalar row rule of waveshape.hip
//   warp_bwd   a thread owns the input sample m: a binary search of SEARCH_STEPS fixed iterations over [max(0, m - 4099), min(L, m + 4099))
//              for the first n with i(n) >= m - 2 (i is non-decreasing under the curve's contract), i(n) evaluated from the knots; then at
//              most GATHER_CAP terms in ascending n while i(n) <= m + 1 (the contract allows six).  No atomics, no scratch row.
//
// Any bits in `delay` are safe: every index is compared with [0, L) before its load, both loops of the transpose have constant trip
// bounds, and the float-to-int conversion comes after a clamp to +-(2^30 - 64) (which also keeps i + 2 inside an int).  Outside the
// contract (finite knots, |d| <= 4096, |d[j+1] - d[j]| <= 16) the results are unspecified, except that a non-finite delta(n) gives
// y[n] = NaN.
#include "dmx_common.h"
#include "kernels.h"
#include "warp_common.h"                   // R, INT_CLAMP, warp_delta, warp_split, warp_weight, warp_pos: shared with warp_fit.hip
#include "../../include/diffmusic_hip.h"
#include <cmath>
void dmx_set_error(const char* fmt, ...);

namespace {

constexpr int REACH = 4099;                // the search window: |delta| <= 4096 and the four taps
constexpr int SEARCH_STEPS = 14;           // 2^14 > 2 * REACH
constexpr int GATHER_CAP = 8;              // terms of the transpose per input sample (six under the contract)

__device__ __forceinline__ bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

__global__ __launch_bounds__(256) void warp_fwd_kernel(const float* __restrict__ x, long long xs, const float* __restrict__ delay, long long ds,
                                                       float* __restrict__ y, int L) {
  const int b = blockIdx.y, n0 = 4 * (blockIdx.x * 256 + threadIdx.x);
  if (n0 >= L) return;
  const float* xr = x + (long long)b * xs;
  const float* dr = delay + (long long)b * ds;
  float* yr = y + (long long)b * L;
  const int j = n0 >> 6, r0 = n0 & (R - 1);
  const float d0 = dr[j], d1 = dr[j + 1];
  float v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float delta = warp_delta(d0, d1, r0 + e);
    float f;
    const int i = n0 + e + warp_split(delta, f);
    float acc = 0.f;
#pragma unroll
    for (int k = -1; k <= 2; ++k) {
      const int t = i + k;
      if (t >= 0 && t < L) acc = fmaf(warp_weight(k, f), xr[t], acc);
    }
    v[e] = fabsf(delta) <= 3.4028234663852886e38f ? acc : __builtin_nanf("");
  }
  if (aligned16(yr) && n0 + 3 < L) {
    *reinterpret_cast<float4*>(yr + n0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) if (n0 + e < L) yr[n0 + e] = v[e];
  }
}

__global__ __launch_bounds__(256) void warp_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ delay, long long ds,
                                                       float* __restrict__ dx, int L, int full) {
  const int b = blockIdx.y, m = blockIdx.x * 256 + threadIdx.x;
  if (m >= full) return;
  float* out = dx + (long long)b * full + m;
  if (m >= L) { *out = 0.f; return; }
  const float* gr = dy + (long long)b * L;
  const float* dr = delay + (long long)b * ds;
  int lo = m - REACH > 0 ? m - REACH : 0, hi = L - m > REACH ? m + REACH : L;           // lo <= m < hi <= L
  float f;
#pragma unroll 1
  for (int it = 0; it < SEARCH_STEPS; ++it) {
    if (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);                 // lo <= mid < hi <= L
      if (warp_pos(dr, mid, f) >= m - 2) hi = mid; else lo = mid + 1;
    }
  }
  float acc = 0.f;
#pragma unroll 1
  for (int q = 0; q < GATHER_CAP; ++q) {
    const int n = lo + q;                                    // lo >= 0
    if (n >= L) break;
    const int c = m - warp_pos(dr, n, f);
    if (c < -1) break;                                       // i(n) > m + 1, and so is every later one
    if (c <= 2) acc = fmaf(warp_weight(c, f), gr[n], acc);
  }
  *out = acc;
}

constexpr int MAX_L = 1 << 30;

bool delay_stride_ok(long long ds, int L) { return ds == 0 || ds >= (long long)cdiv(L, R) + 1; }

}  // namespace

extern "C" int dmx_warp_fwd(const float* x, long long x_stride, const float* delay, long long delay_stride, float* y, int batch, int L,
                            void* stream) {
  if (!x || !delay || !y || batch < 1 || batch > 65535 || L < 1 || L > MAX_L || x_stride < L || !delay_stride_ok(delay_stride, L)) {
    dmx_set_error("warp_fwd: x (batch, >= L) with row stride >= L, y (batch, L) contiguous, delay (H + 1) with stride 0 or (batch, >= H + 1), "
                  "H = ceil(L / 64), 1 <= batch <= 65535, 1 <= L <= 2^30");
    return DMX_ERR_SHAPE;
  }
  hipLaunchKernelGGL(warp_fwd_kernel, dim3((unsigned)cdiv(cdiv(L, 4), 256), (unsigned)batch), dim3(256), 0, (hipStream_t)stream, x, x_stride,
                     delay, delay_stride, y, L);
  return hipGetLastError() == hipSuccess ? DMX_OK : DMX_ERR_LAUNCH;
}

extern "C" int dmx_warp_bwd(const float* dy, const float* delay, long long delay_stride, float* dx, int batch, int L, int full, void* stream) {
  if (!dy || !delay || !dx || batch < 1 || batch > 65535 || L < 1 || L > MAX_L || full < L || full > MAX_L || !delay_stride_ok(delay_stride, L)) {
    dmx_set_error("warp_bwd: dy (batch, L) and dx (batch, full >= L) contiguous, delay (H + 1) with stride 0 or (batch, >= H + 1), "
                  "H = ceil(L / 64), 1 <= batch <= 65535, 1 <= L <= full <= 2^30");
    return DMX_ERR_SHAPE;
  }
  hipLaunchKernelGGL(warp_bwd_kernel, dim3((unsigned)cdiv(full, 256), (unsigned)batch), dim3(256), 0, (hipStream_t)stream, dy, delay,
                     delay_stride, dx, L, full);
  return hipGetLastError() == hipSuccess ? DMX_OK : DMX_ERR_LAUNCH;
}
