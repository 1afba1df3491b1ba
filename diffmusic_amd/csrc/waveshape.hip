// Hard clipping on materialised waveforms (the declipping operator; no counterpart in the reference, whose operators are all linear
// maps or magnitudes): A(x)[b, s] = min(max(x[b, s], -c[b]), c[b]) with one threshold c[b] > 0 per clip, its transpose-Jacobian
// product, and the output stage that makes a restored clip consistent with the clipped measurement.  The fused mel guidance applies
// the same clip on load (stft_mel.hip); these kernels serve wav_form space, clips the fused kernels do not cover, the measurement
// side (`forward`) and `project`.
//
// All three are memory-bound row maps.  A thread owns four consecutive samples of one row; a row whose start is 16-byte aligned is
// read / written as float4 (row strides are arbitrary, so this is decided per row and per tensor -- uniform over a workgroup, which
// never spans rows), the others and every row's last partial quad go sample by sample.  The clamps are written with comparisons: a
// NaN sample fails them and stays NaN, as with torch.clamp (fminf / fmaxf would return the bound).
#include "dmx_common.h"
#include "kernels.h"
#include "../../include/diffmusic_hip.h"
void dmx_set_error(const char* fmt, ...);

namespace {

__device__ __forceinline__ bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// samples i .. i + 3 of a row with n valid samples (positions >= n read nothing and give 0)
__device__ __forceinline__ void load4(const float* row, bool vec, int i, int n, float (&v)[4]) {
  if (vec && i + 3 < n) {
    const float4 t = *reinterpret_cast<const float4*>(row + i);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = i + e < n ? row[i + e] : 0.f;
  }
}
__device__ __forceinline__ void store4(float* row, bool vec, int i, int n, const float (&v)[4]) {
  if (vec && i + 3 < n) {
    *reinterpret_cast<float4*>(row + i) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) if (i + e < n) row[i + e] = v[e];
  }
}

// y[b, i] = clip(x[b, i], c[b]), i < L
__global__ __launch_bounds__(256) void clip_fwd_kernel(const float* __restrict__ x, long long xs, const float* __restrict__ thr,
                                                       float* __restrict__ y, long long ys, int L) {
  const int b = blockIdx.y, i = 4 * (blockIdx.x * 256 + threadIdx.x);
  if (i >= L) return;
  const float* xr = x + (long long)b * xs;
  float* yr = y + (long long)b * ys;
  const float c = thr[b];
  float v[4];
  load4(xr, aligned16(xr), i, L, v);
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = v[e] < -c ? -c : (v[e] > c ? c : v[e]);
  store4(yr, aligned16(yr), i, L, v);
}

// dwav[b, i] = dy[b, i] where -c[b] <= wav[b, i] <= c[b] (inclusive: torch.clamp's rule at equality), 0 elsewhere and on L <= i < full
__global__ __launch_bounds__(256) void clip_bwd_kernel(const float* __restrict__ dy, long long dys, const float* __restrict__ wav, long long ws,
                                                       const float* __restrict__ thr, float* __restrict__ dwav, long long ds, int L, int full) {
  const int b = blockIdx.y, i = 4 * (blockIdx.x * 256 + threadIdx.x);
  if (i >= full) return;
  const float* gr = dy + (long long)b * dys;
  const float* wr = wav + (long long)b * ws;
  float* dr = dwav + (long long)b * ds;
  const float c = thr[b];
  float g[4], w[4];
  load4(gr, aligned16(gr), i, L, g);                       // zeros past L: the tail
  load4(wr, aligned16(wr), i, L, w);
#pragma unroll
  for (int e = 0; e < 4; ++e) if (!(w[e] >= -c && w[e] <= c)) g[e] = 0.f;
  store4(dr, aligned16(dr), i, full, g);
}

// out[b, i] = y where |y| < c (a reliable sample), max(xhat, c) where y >= c, min(xhat, -c) where y <= -c;  y = meas[b, i], c = c[b]
__global__ __launch_bounds__(256) void declip_project_kernel(const float* __restrict__ xhat, long long xs, const float* __restrict__ meas,
                                                             long long ms, const float* __restrict__ thr, float* __restrict__ out, long long os,
                                                             int L) {
  const int b = blockIdx.y, i = 4 * (blockIdx.x * 256 + threadIdx.x);
  if (i >= L) return;
  const float* xr = xhat + (long long)b * xs;
  const float* mr = meas + (long long)b * ms;
  float* orow = out + (long long)b * os;
  const float c = thr[b];
  float x[4], y[4];
  load4(xr, aligned16(xr), i, L, x);
  load4(mr, aligned16(mr), i, L, y);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float o = y[e];
    if (y[e] >= c) o = x[e] > c ? x[e] : c;
    else if (y[e] <= -c) o = x[e] < -c ? x[e] : -c;
    x[e] = o;
  }
  store4(orow, aligned16(orow), i, L, x);
}

inline dim3 row_grid(int n, int B) { return dim3((unsigned)cdiv(cdiv(n, 4), 256), (unsigned)B); }

}  // namespace

extern "C" int dmx_clip_fwd(const float* x, long long x_stride, const float* thr, float* y, long long y_stride, int batch, int L, void* stream) {
  if (!x || !thr || !y || batch < 1 || batch > 65535 || L < 1 || x_stride < L || y_stride < L) {
    dmx_set_error("clip_fwd: x (batch, >= L), y (batch, L) with row strides >= L, thr (batch), 1 <= batch <= 65535");
    return DMX_ERR_SHAPE;
  }
  hipLaunchKernelGGL(clip_fwd_kernel, row_grid(L, batch), dim3(256), 0, (hipStream_t)stream, x, x_stride, thr, y, y_stride, L);
  return hipGetLastError() == hipSuccess ? DMX_OK : DMX_ERR_LAUNCH;
}

extern "C" int dmx_clip_bwd(const float* dy, long long dy_stride, const float* wav, long long wav_stride, const float* thr, float* dwav,
                            long long dwav_stride, int batch, int L, int Lfull, void* stream) {
  if (!dy || !wav || !thr || !dwav || batch < 1 || batch > 65535 || L < 1 || Lfull < L || dy_stride < L || wav_stride < L || dwav_stride < Lfull) {
    dmx_set_error("clip_bwd: dy (batch, L), wav (batch, >= L), dwav (batch, Lfull >= L) with row strides >= their lengths, thr (batch)");
    return DMX_ERR_SHAPE;
  }
  hipLaunchKernelGGL(clip_bwd_kernel, row_grid(Lfull, batch), dim3(256), 0, (hipStream_t)stream, dy, dy_stride, wav, wav_stride, thr, dwav,
                     dwav_stride, L, Lfull);
  return hipGetLastError() == hipSuccess ? DMX_OK : DMX_ERR_LAUNCH;
}

extern "C" int dmx_declip_project(const float* xhat, long long xhat_stride, const float* meas, long long meas_stride, const float* thr, float* out,
                                  long long out_stride, int batch, int L, void* stream) {
  if (!xhat || !meas || !thr || !out || batch < 1 || batch > 65535 || L < 1 || xhat_stride < L || meas_stride < L || out_stride < L) {
    dmx_set_error("declip_project: xhat (batch, >= L), meas and out (batch, L) with row strides >= L, thr (batch)");
    return DMX_ERR_SHAPE;
  }
  hipLaunchKernelGGL(declip_project_kernel, row_grid(L, batch), dim3(256), 0, (hipStream_t)stream, xhat, xhat_stride, meas, meas_stride, thr, out,
                     out_stride, L);
  return hipGetLastError() == hipSuccess ? DMX_OK : DMX_ERR_LAUNCH;
}
