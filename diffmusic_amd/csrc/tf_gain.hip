// Time-frequency gain: A(x) = (1/c) P^T W F^-1 G F W P x, a real gain G[k, t] on the STFT of a clip, resynthesised to a waveform.
// n_fft = 1024, hop = 256, periodic Hann window w, fp32 throughout.
//
//   frames     t = 0 .. T - 1, T = ceil(L / 256) + 3; frame t covers samples s = (t - 3) * 256 + n, n = 0 .. 1023; x is ZERO outside [0, L)
//              (no reflect padding: with the zero extension every sample of [0, L) lies in exactly four frames and A is symmetric)
//   analysis   X[k, t] = sum_n w[n] x[s] exp(-2 pi i k n / 1024), k = 0 .. 512
//   gain       Y[k, t] = G[k, t] X[k, t], G real and finite, of any sign; Y[1024 - k] = conj(Y[k]) for k = 1 .. 511
//   synthesis  f_t = Re IDFT(Y[:, t]) (the imaginary parts of DC and Nyquist drop out of the real part, as in irfft);
//              A(x)[s] = (1/c) sum_{t covers s} w[n] f_t[n], c = sum_j w[n + 256 j]^2 = 1.5 for every n
//
// A workgroup owns a slab of SLAB_HOPS consecutive output hops h0 .. h1 - 1 and walks the frames h0 .. h1 + 2 that touch it: the three
// frames past each slab edge are recomputed by the neighbouring slab as well (its halo).  One wave handles one frame at a time: load with
// the window applied, fft1024<false>, gain and Hermitian half, fft1024<true>, 1/1024 and the window, overlap-add into the WAVE'S OWN
// accumulator in LDS.  Wave w takes the frames h0 + w, h0 + w + 4, ...: the four frames that cover a sample are consecutive, so each of the
// four accumulators receives exactly one of them, and the sample is ((acc0 + acc1) + acc2) + acc3 times fp32(2 / 3) -- no atomics, an order
// that depends on the slab and the frame only: bit-reproducible, and independent of the clip's batch position and of the batch size.
// Only the slab's own samples below L are written; the last slab of a clip writes +0.0f to out[b, L : full).
//
// gain is read as (T, 513) rows (lane = bin: 256-byte reads); clip stride 0 = one grid for every clip.  The public layout of the operator
// stays (513, T); it keeps the transposed device copy (inverse_problem/operator.py, TimeFrequencyMaskOperator).  The distance between the
// gain rows of consecutive frames is a parameter: 513 for a grid, 0 for ONE 513-row that every frame reads (a gain constant in time, the
// equalisation curve of BlindEqualizationOperator).  Only the address changes, no arithmetic.
#include "dmx_common.h"
#include "kernels.h"
#include "fft1024.h"
#include <cstring>

namespace {

constexpr int NF = 1024;
constexpr int NB = NF / 2 + 1;
constexpr int HOP = 256;
constexpr int HALO = NF / HOP - 1;       // frames past a slab edge that still reach into the slab
constexpr int SLAB_HOPS = 8;             // 11 frames for 8 hops of output: 27 % of the FFTs are halo
constexpr int SLAB = SLAB_HOPS * HOP;
constexpr float INV_C = 2.f / 3.f;       // 1 / c, c = 1.5 (rounded once)

struct TfParams {
  const float* x; long long x_stride;
  const float* gain; long long gain_stride;   // (T, 513) rows; clip stride 0 = shared
  long long gain_frame_stride;                // floats between the rows of consecutive frames: 513, or 0 = one row for every frame
  float* out; long long out_stride;
  int L, full, T, H;                    // H = ceil(L / 256) output hops
  const float2* tw;
  const float* win;
};

// samples n = lane + 64 j of frame t, zero outside [0, L) (nothing is read there)
__device__ __forceinline__ void tf_fetch(const float* __restrict__ xr, int L, int t, float (&x)[16], int lane) {
  const int p0 = (t - HALO) * HOP;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int s = p0 + lane + 64 * j;
    x[j] = (s >= 0 && s < L) ? xr[s] : 0.f;
  }
}

__global__ __launch_bounds__(256) void tf_gain_kernel(const TfParams P) {
  __shared__ float2 s_tw[NF];
  __shared__ float2 s_buf[4][NF];
  __shared__ float s_acc[4][SLAB];
  // 72 KB of static LDS: legal because gfx950 has 160 KiB per CU; two workgroups share a CU
  static_assert(sizeof(float2) * NF * 5 + sizeof(float) * 4 * SLAB <= 80 * 1024, "tf_gain_kernel: two workgroups per CU must fit the 160 KiB of gfx950 LDS");
#if !defined(__gfx950__) && defined(__HIP_DEVICE_COMPILE__)
#error "tf_gain.hip sizes its LDS for gfx950 (160 KiB per CU)"
#endif
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y;
  const int L = P.L;
  const int h0 = blockIdx.x * SLAB_HOPS, h1 = min(h0 + SLAB_HOPS, P.H);
  const int s0 = h0 * HOP, s1 = min(h1 * HOP, L);
  const int t1 = h1 + HALO;                                // frames h0 .. t1 - 1 touch the slab; t1 <= T
  for (int i = tid; i < NF; i += 256) s_tw[i] = P.tw[i];
  float win[16], xs[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) win[j] = P.win[lane + 64 * j];
  for (int i = tid; i < 4 * SLAB; i += 256) (&s_acc[0][0])[i] = 0.f;
  __syncthreads();
  const float* xr = P.x + (long long)b * P.x_stride;
  const float* gr = P.gain + (long long)b * P.gain_stride;
  float2* buf = s_buf[wave];
  float* acc = s_acc[wave];
  if (h0 + wave < t1) tf_fetch(xr, L, h0 + wave, xs, lane);
  for (int t = h0 + wave; t < t1; t += 4) {                // wave-uniform
#pragma unroll
    for (int j = 0; j < 16; ++j) buf[lane + 64 * j] = make_float2(xs[j] * win[j], 0.f);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (t + 4 < t1) tf_fetch(xr, L, t + 4, xs, lane);      // in flight under this frame's two FFTs
    fft1024<false>(buf, s_tw, lane);
    // Y[k] = G[k, t] X[k] on the one-sided bins (read from the lower half only), conjugates into the upper half
    const float* g = gr + (long long)t * P.gain_frame_stride;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      const int k = lane + 64 * j;
      if (k < NB) {
        const float gk = g[k];
        const float2 v = buf[k];
        const float2 y = make_float2(gk * v.x, gk * v.y);
        buf[k] = y;
        if (k >= 1 && k < NF / 2) buf[NF - k] = make_float2(y.x, -y.y);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    fft1024<true>(buf, s_tw, lane);
    // overlap-add into this wave's accumulator: positions of the frame inside the slab (1 / 1024 is exact)
    const int p0 = (t - HALO) * HOP - s0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int n = lane + 64 * j;
      const int i = p0 + n;
      if (i >= 0 && i < SLAB) acc[i] += (buf[n].x * (1.f / NF)) * win[j];
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  }
  __syncthreads();
  float* out = P.out + (long long)b * P.out_stride;
  for (int i = tid; i < s1 - s0; i += 256)
    out[s0 + i] = (((s_acc[0][i] + s_acc[1][i]) + s_acc[2][i]) + s_acc[3][i]) * INV_C;
  if (blockIdx.x == gridDim.x - 1)
    for (int i = L + tid; i < P.full; i += 256) out[i] = 0.f;
}

}  // namespace

int dmx_tf_gain_frames(int L) { return cdiv(L, HOP) + HALO; }

int dmx_tf_gain(const DmxStftMelTables& t, const float* x, long long x_stride, const float* gain, long long gain_clip_stride,
                long long gain_frame_stride, float* out, long long out_stride, int B, int L, int full, hipStream_t st) {
  if (!x || !gain || !out || B < 1 || B > 65535 || L < 1 || full < L || L > 0x7fffffff - 2 * NF || x_stride < L || out_stride < full) return DMX_ERR_SHAPE;
  const int T = dmx_tf_gain_frames(L);
  if (gain_frame_stride != 0 && gain_frame_stride != NB) return DMX_ERR_SHAPE;
  if (gain_clip_stride != 0 && gain_clip_stride < (gain_frame_stride ? (long long)T * NB : (long long)NB)) return DMX_ERR_SHAPE;
  TfParams P;
  memset(&P, 0, sizeof(P));
  P.x = x; P.x_stride = x_stride; P.gain = gain; P.gain_stride = gain_clip_stride; P.gain_frame_stride = gain_frame_stride; P.out = out; P.out_stride = out_stride;
  P.L = L; P.full = full; P.T = T; P.H = T - HALO; P.tw = t.tw; P.win = t.win;
  hipLaunchKernelGGL(tf_gain_kernel, dim3(cdiv(P.H, SLAB_HOPS), B), dim3(256), 0, st, P);
  return hipGetLastError() == hipSuccess ? DMX_OK : DMX_ERR_LAUNCH;
}
