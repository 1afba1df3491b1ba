// Track mode: W overlapping windows of L samples as ONE sample of T samples (inverse_problem/track.py).
//
//   S   (track_stitch_fwd): track[n]   = sum_w (u(n - start[w]) / den[n]) * wav[w, n - start[w]]   over the windows that cover n
//   S^T (track_stitch_bwd): dwav[w, i] = (u(i) / den[start[w] + i]) * dtrack[start[w] + i]         for i < L, 0 for L <= i < full
//
// with the taper u(i) = min(i + 0.5, L - 0.5 - i, R) / R and den[n] = sum_w u(n - start[w]).  The 1 / R of the taper cancels in the
// quotient, so both kernels form it from the numerators m(i) = min(i + 0.5, L - 0.5 - i, R): half-integers, exact in fp32 for the
// windows the launcher accepts (L <= 2^22), and so is their sum over the (two or three) covering windows.  A sample that one window
// covers has the weight m / m == 1.0f and is copied bit for bit; where windows overlap the only roundings are one division per window
// and the additions of the products.
//
// Both are one pass: 4 consecutive samples per lane, 16-byte loads and stores where the addresses allow it (a window's start need not
// be a multiple of 4; such a window is read with scalar loads), no atomics, no table in memory: the window starts travel by value in
// the kernel arguments (W <= 64, 256 bytes).  At W = 8, L = 163 840 a launch moves about 10 MB.
#include "dmx_common.h"
#include "kernels.h"
#include "layers.h"

namespace {

constexpr int TRACK_MAX_WINDOWS = 64;
constexpr int TRACK_MAX_WINDOW_LEN = 1 << 22;      // i + 0.5 and the sum of three numerators stay exact in fp32 (the launcher refuses longer windows)
struct TrackStarts { int s[TRACK_MAX_WINDOWS]; };

__device__ __forceinline__ float taper_num(int i, int L, int R) { return fminf(fminf((float)i + 0.5f, (float)(L - i) - 0.5f), (float)R); }
__device__ __forceinline__ bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

__global__ __launch_bounds__(256) void track_stitch_fwd_kernel(const float* __restrict__ wav, long long wav_stride, float* __restrict__ track,
                                                               TrackStarts a, int W, int L, int R, int T) {
  const long long n0l = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (n0l >= T) return;
  const int n0 = (int)n0l;
  float den[4] = {0.f, 0.f, 0.f, 0.f}, acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int w = 0; w < W; ++w) {
    const int lo = n0 - a.s[w];
    if (lo + 3 < 0 || lo >= L) continue;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int i = lo + e;
      if (i >= 0 && i < L) den[e] += taper_num(i, L, R);
    }
  }
  unsigned seen = 0;
  for (int w = 0; w < W; ++w) {
    const int lo = n0 - a.s[w];
    if (lo + 3 < 0 || lo >= L) continue;
    const float* p = wav + (long long)w * wav_stride + lo;
    float v[4];
    if (lo >= 0 && lo + 3 < L && aligned16(p)) {
      const float4 q = *reinterpret_cast<const float4*>(p);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (lo + e >= 0 && lo + e < L) ? p[e] : 0.f;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int i = lo + e;
      if (i >= 0 && i < L) {
        const float term = (taper_num(i, L, R) / den[e]) * v[e];
        acc[e] = (seen >> e & 1u) ? acc[e] + term : term;      // the first term is taken as it is: -0.0f stays -0.0f
        seen |= 1u << e;
      }
    }
  }
  float* o = track + n0;
  if (n0 + 3 < T && aligned16(o)) {
    *reinterpret_cast<float4*>(o) = make_float4(acc[0], acc[1], acc[2], acc[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) if (n0 + e < T) o[e] = acc[e];
  }
}

// grid (ceil(full / 4 / 256), W)
__global__ __launch_bounds__(256) void track_stitch_bwd_kernel(const float* __restrict__ dtrack, float* __restrict__ dwav, long long dwav_stride,
                                                               TrackStarts a, int W, int L, int R, int full) {
  const long long i0l = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i0l >= full) return;
  const int i0 = (int)i0l, w = blockIdx.y, s = a.s[w];
  float out[4] = {0.f, 0.f, 0.f, 0.f};
  if (i0 < L) {
    const float* p = dtrack + s + i0;
    float v[4];
    if (i0 + 3 < L && aligned16(p)) {
      const float4 q = *reinterpret_cast<const float4*>(p);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = i0 + e < L ? p[e] : 0.f;
    }
    float den[4] = {0.f, 0.f, 0.f, 0.f};
    for (int w2 = 0; w2 < W; ++w2) {
      const int lo = s + i0 - a.s[w2];
      if (lo + 3 < 0 || lo >= L) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = lo + e;
        if (i >= 0 && i < L) den[e] += taper_num(i, L, R);
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) if (i0 + e < L) out[e] = (taper_num(i0 + e, L, R) / den[e]) * v[e];
  }
  float* o = dwav + (long long)w * dwav_stride + i0;
  if (i0 + 3 < full && aligned16(o)) {
    *reinterpret_cast<float4*>(o) = make_float4(out[0], out[1], out[2], out[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) if (i0 + e < full) o[e] = out[e];
  }
}

// the layout a launch may touch memory for: W windows of L samples that start at 0, end at T and leave no sample uncovered
int check_layout(const char* what, const int* starts_host, int W, int L, int R, int T, TrackStarts* out) {
  if (!starts_host || W < 1 || W > TRACK_MAX_WINDOWS) { dmx_set_error("%s: 1 <= windows <= %d (got %d)", what, TRACK_MAX_WINDOWS, W); return DMX_ERR_SHAPE; }
  if (L > TRACK_MAX_WINDOW_LEN) { dmx_set_error("%s: windows of at most %d samples (got %d): the taper is formed in fp32", what, TRACK_MAX_WINDOW_LEN, L); return DMX_ERR_SHAPE; }
  if (L < 1 || R < 1 || R > L / 2 || T < L) { dmx_set_error("%s: need 0 < R <= L / 2 and T >= L (L=%d R=%d T=%d)", what, L, R, T); return DMX_ERR_SHAPE; }
  if (starts_host[0] != 0 || starts_host[W - 1] != T - L) { dmx_set_error("%s: the first window starts at 0 and the last at T - L", what); return DMX_ERR_SHAPE; }
  for (int w = 0; w < TRACK_MAX_WINDOWS; ++w) out->s[w] = w < W ? starts_host[w] : 0;
  for (int w = 1; w < W; ++w)
    if (starts_host[w] <= starts_host[w - 1] || starts_host[w] - starts_host[w - 1] >= L) {
      dmx_set_error("%s: window starts must increase by less than L (window %d: %d after %d)", what, w, starts_host[w], starts_host[w - 1]);
      return DMX_ERR_SHAPE;
    }
  return DMX_OK;
}

}  // namespace

extern "C" int dmx_track_stitch_fwd(const float* wav, long long wav_stride, float* track, const int* starts_host, int windows, int L, int R, int T,
                                    void* stream) {
  TrackStarts a;
  const int rc = check_layout("track_stitch_fwd", starts_host, windows, L, R, T, &a);
  if (rc != DMX_OK) return rc;
  if (!wav || !track || wav_stride < L) { dmx_set_error("track_stitch_fwd: wav (W, >= L) with row stride >= L and track (T) are required"); return DMX_ERR_SHAPE; }
  const long long threads = ((long long)T + 3) / 4;
  hipLaunchKernelGGL(track_stitch_fwd_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, wav, wav_stride, track, a,
                     windows, L, R, T);
  return hipGetLastError() == hipSuccess ? DMX_OK : DMX_ERR_LAUNCH;
}

extern "C" int dmx_track_stitch_bwd(const float* dtrack, float* dwav, long long dwav_stride, const int* starts_host, int windows, int L, int R, int T,
                                    int full, void* stream) {
  TrackStarts a;
  const int rc = check_layout("track_stitch_bwd", starts_host, windows, L, R, T, &a);
  if (rc != DMX_OK) return rc;
  if (!dtrack || !dwav || full < L || dwav_stride < full) {
    dmx_set_error("track_stitch_bwd: dtrack (T) and dwav (W, full >= L) with row stride >= full are required");
    return DMX_ERR_SHAPE;
  }
  const long long threads = ((long long)full + 3) / 4;
  hipLaunchKernelGGL(track_stitch_bwd_kernel, dim3((unsigned)((threads + 255) / 256), (unsigned)windows), dim3(256), 0, (hipStream_t)stream, dtrack, dwav,
                     dwav_stride, a, windows, L, R, full);
  return hipGetLastError() == hipSuccess ? DMX_OK : DMX_ERR_LAUNCH;
}
