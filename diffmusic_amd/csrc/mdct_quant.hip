// MDCT quantiser: A(x) = Phi^T f(Phi x), a per-coefficient map f between the MDCT of a clip and its transpose -- the measurement of a lossy
// codec (MP3 / AAC / Vorbis: an MDCT whose coefficients were quantised, one step per band and frame, everything above a cut-off discarded).
// N = 512 coefficients per frame, frame length 2N = 1024, hop N, sine window, fp32 throughout.
//
//   frames     t = 0 .. T - 1, T = ceil(L / 512) + 1; frame t covers samples s = (t - 1) * 512 + n, n = 0 .. 1023; x is ZERO outside [0, L):
//              every sample of [0, L) lies in exactly two frames, and with w[n]^2 + w[n + 512]^2 = 1 (Princen-Bradley) Phi^T Phi = I on the clip
//   analysis   C[k, t] = sqrt(2 / N) sum_n w[n] x[s] cos(pi / N (n + 1/2 + N / 2)(k + 1/2)), k = 0 .. 511, w[n] = sin(pi (n + 1/2) / 1024)
//   map        QUANT    f = Q: q = rint(C / D), Q(C) = q D; D = 0 transparent (C), D = +inf discards (0, code 0); |C / D| >= 2^23, a NaN
//                       quotient, a negative or NaN step pass C through; the code of every coefficient that was not coded is INT32_MIN
//              PASS     f(c) = c where D is not +inf, else 0 (the straight-through transpose of QUANT)
//              PROJECT  f = clamp of c into [(q - 1/2) D, (q + 1/2) D] with q read from `codes`, on WHOLE frames (1 <= t <= L / 512 - 1: all
//                       1024 samples inside the clip), where 0 < D < inf and q is not INT32_MIN; every other coefficient is left as it is
//   synthesis  A(x)[s] = sum_{t covers s} sqrt(2 / N) w[n] sum_k f(C[k, t]) cos(...)          (the transpose of the analysis)
//
// The MDCT goes through the wave-level 1024-point FFT of fft1024.h, with n0 = 256.5:
//   forward    u[n] = (w[n] x[s]) pre[n], pre[n] = exp(-i pi n / 1024); fft1024<false>; C[k] = Re(U[k] post[k]) sqrt(2 / N) for k < 512,
//              post[k] = exp(-i pi n0 (k + 1/2) / 512)
//   transpose  Z[k] = f(C[k]) conj(post[k]) for k < 512, zero above; fft1024<true>; (Re(z[n] conj(pre[n])) sqrt(2 / N)) w[n]
// pre, post and w are computed in double on the host and rounded once (audio_api.hip).
//
// Structure as in tf_gain.hip: a workgroup owns a slab of SLAB_HOPS output hops h0 .. h1 - 1 of one clip and walks the frames h0 .. h1 that
// touch it (frame h1 is recomputed by the next slab: its halo, 12.5 % extra, no communication).  One wave handles one frame at a time in the
// wave's own LDS buffer and adds its output into the accumulator of the frame's PARITY: the two frames that cover a sample are consecutive,
// so each of the two accumulators receives exactly one of them, and two frames of one parity do not overlap, so no position of an
// accumulator is written by two waves.  The sample is acc0 + acc1 -- no atomics, an order fixed by the slab and the frame alone: the same
// bits alone, in a batch and at another batch position.  Only [0, L) of the slab is written; the clip's last slab writes +0.0f to [L, full).
// The accumulators start at +0.0f, so a sample whose two frames give only zeros of either sign is exactly +0.0f.
//
// step is read as (T, 512) rows (lane = coefficient); clip stride 0 = one grid for every clip.  The public layout of the operator stays
// (512, T); it keeps the transposed device copy (inverse_problem/operator.py, CodecOperator).  codes are (B, T, 512) int32, written by the
// slab that owns the frame (the halo frame by the next one; the same bits either way).  Any bits in x, step and codes are safe: they only
// ever enter arithmetic and comparisons, never an address.
#include "dmx_common.h"
#include "kernels.h"
#include "fft1024.h"
#include <climits>
#include <cstring>

namespace {

constexpr int NF = 1024;
constexpr int NC = NF / 2;               // coefficients per frame = hop
constexpr int SLAB_HOPS = 8;             // 9 frames for 8 hops of output
constexpr int SLAB = SLAB_HOPS * NC;
constexpr float SCALE = 0.0625f;         // sqrt(2 / 512) = 1 / 16, exact
constexpr float Q_LIMIT = 8388608.f;     // 2^23: below it rint() and the int conversion are exact
constexpr int NOT_CODED = INT_MIN;

struct MdctParams {
  const float* x; long long x_stride;
  const float* step; long long step_stride;   // (T, 512) rows; clip stride 0 = shared
  int* codes;                                 // (B, T, 512): QUANT writes (optional), PROJECT reads
  float* out; long long out_stride;
  int L, full, T, H;                          // H = ceil(L / 512) output hops, T = H + 1
  const float2 *tw, *pre, *post;
  const float* win;
};

// samples n = lane + 64 j of frame t, zero outside [0, L) (nothing is read there)
__device__ __forceinline__ void mdct_fetch(const float* __restrict__ xr, int L, int t, float (&x)[16], int lane) {
  const int p0 = (t - 1) * NC;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int s = p0 + lane + 64 * j;
    x[j] = (s >= 0 && s < L) ? xr[s] : 0.f;
  }
}

// Q(c) for the step d; code = q, or NOT_CODED where c passes through
__device__ __forceinline__ float mdct_quantise(float c, float d, int& code) {
  code = NOT_CODED;
  if (!(d > 0.f)) return c;                               // 0: transparent; negative or NaN: like a NaN quotient
  if (d == INFINITY) { code = 0; return 0.f; }            // discarded
  const float r = c / d;                                  // correctly rounded (no fast-math in this build)
  if (!(fabsf(r) < Q_LIMIT)) return c;                    // too many cells, or NaN
  const float q = rintf(r);                               // round-half-even
  code = (int)q;
  return q * d;
}

template <int MODE>
__global__ __launch_bounds__(256) void mdct_quant_kernel(const MdctParams P) {
  __shared__ float2 s_tw[NF];
  __shared__ float2 s_buf[4][NF];
  __shared__ float s_acc[2][SLAB];
  // 72 KB of static LDS: legal because gfx950 has 160 KiB per CU; two workgroups share a CU
  static_assert(sizeof(float2) * NF * 5 + sizeof(float) * 2 * SLAB <= 80 * 1024, "mdct_quant_kernel: two workgroups per CU must fit the 160 KiB of gfx950 LDS");
#if !defined(__gfx950__) && defined(__HIP_DEVICE_COMPILE__)
#error "mdct_quant.hip sizes its LDS for gfx950 (160 KiB per CU)"
#endif
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y;
  const int L = P.L;
  const int h0 = blockIdx.x * SLAB_HOPS, h1 = min(h0 + SLAB_HOPS, P.H);
  const int s0 = h0 * NC, s1 = min(h1 * NC, L);
  const int t1 = h1 + 1;                                   // frames h0 .. t1 - 1 touch the slab; t1 <= T
  const int whole_hi = L / NC - 1;                         // whole frames: 1 <= t <= whole_hi
  for (int i = tid; i < NF; i += 256) s_tw[i] = P.tw[i];
  float win[16], xs[16];
  float2 pre[16], post[8];
#pragma unroll
  for (int j = 0; j < 16; ++j) { win[j] = P.win[lane + 64 * j]; pre[j] = P.pre[lane + 64 * j]; }
#pragma unroll
  for (int j = 0; j < 8; ++j) post[j] = P.post[lane + 64 * j];
  for (int i = tid; i < 2 * SLAB; i += 256) (&s_acc[0][0])[i] = 0.f;
  __syncthreads();
  const float* xr = P.x + (long long)b * P.x_stride;
  const float* dr = P.step + (long long)b * P.step_stride;
  int* cr = P.codes ? P.codes + (long long)b * P.T * NC : nullptr;
  float2* buf = s_buf[wave];
  if (h0 + wave < t1) mdct_fetch(xr, L, h0 + wave, xs, lane);
  for (int t = h0 + wave; t < t1; t += 4) {                // wave-uniform
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float xw = xs[j] * win[j];
      buf[lane + 64 * j] = make_float2(xw * pre[j].x, xw * pre[j].y);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (t + 4 < t1) mdct_fetch(xr, L, t + 4, xs, lane);    // in flight under this frame's two FFTs
    fft1024<false>(buf, s_tw, lane);
    // C[k] = Re(U[k] post[k]) / 16, the map, Z[k] = f(C[k]) conj(post[k]); every lane reads and writes its own bins k < 512 only
    const float* d = dr + (long long)t * NC;
    const bool owner = t < h1 || h1 == P.H;                // the halo frame's codes are the next slab's to write
    const bool whole = t >= 1 && t <= whole_hi;
    float fz[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = lane + 64 * j;
      const float2 v = buf[k];
      const float c = (v.x * post[j].x - v.y * post[j].y) * SCALE;
      const float dk = d[k];
      if (MODE == DMX_MDCT_QUANT) {
        int code;
        fz[j] = mdct_quantise(c, dk, code);
        if (cr && owner) cr[(long long)t * NC + k] = code;
      } else if (MODE == DMX_MDCT_PASS) {
        fz[j] = dk == INFINITY ? 0.f : c;
      } else {
        const int q = cr[(long long)t * NC + k];
        float f = c;
        if (whole && dk > 0.f && dk < INFINITY && q != NOT_CODED) {
          const float lo = ((float)q - 0.5f) * dk, hi = ((float)q + 0.5f) * dk;
          f = c < lo ? lo : (c > hi ? hi : c);             // a NaN stays a NaN
        }
        fz[j] = f;
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      buf[lane + 64 * j] = make_float2(fz[j] * post[j].x, -(fz[j] * post[j].y));
      buf[NC + lane + 64 * j] = make_float2(0.f, 0.f);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    fft1024<true>(buf, s_tw, lane);
    // overlap-add into the accumulator of the frame's parity: positions of the frame inside the slab.  No race: frames of one parity are
    // 1024 samples apart, so every position of an accumulator is touched by exactly one wave, once, after the zero fill and its barrier.
    // It is `+=` on the +0.0f fill and not a store so that a term of -0.0f leaves +0.0f (dead samples are exactly +0.0f).
    float* acc = s_acc[t & 1];
    const int p0 = (t - 1) * NC - s0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int n = lane + 64 * j;
      const int i = p0 + n;
      const float2 z = buf[n];
      if (i >= 0 && i < SLAB) acc[i] += ((z.x * pre[j].x + z.y * pre[j].y) * SCALE) * win[j];
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  }
  __syncthreads();
  float* out = P.out + (long long)b * P.out_stride;
  for (int i = tid; i < s1 - s0; i += 256) out[s0 + i] = s_acc[0][i] + s_acc[1][i];
  if (blockIdx.x == gridDim.x - 1)
    for (int i = L + tid; i < P.full; i += 256) out[i] = 0.f;
}

}  // namespace

int dmx_mdct_num_frames(int L) { return cdiv(L, NC) + 1; }

int dmx_mdct_run(const DmxMdctTables& t, const float* x, long long x_stride, const float* step, long long step_clip_stride, int* codes, float* out,
                 long long out_stride, int B, int L, int full, int mode, hipStream_t st) {
  if (!t.tw || !t.pre || !t.post || !t.win || !x || !step || !out || B < 1 || B > 65535 || L < 1 || full < L || L > 0x7fffffff - 2 * NF ||
      x_stride < L || out_stride < full)
    return DMX_ERR_SHAPE;
  const int T = dmx_mdct_num_frames(L);
  if (step_clip_stride != 0 && step_clip_stride < (long long)T * NC) return DMX_ERR_SHAPE;
  if (mode != DMX_MDCT_QUANT && mode != DMX_MDCT_PASS && mode != DMX_MDCT_PROJECT) return DMX_ERR_SHAPE;
  if (mode == DMX_MDCT_PROJECT && !codes) return DMX_ERR_SHAPE;
  MdctParams P;
  memset(&P, 0, sizeof(P));
  P.x = x; P.x_stride = x_stride; P.step = step; P.step_stride = step_clip_stride; P.codes = mode == DMX_MDCT_PASS ? nullptr : codes;
  P.out = out; P.out_stride = out_stride; P.L = L; P.full = full; P.T = T; P.H = T - 1;
  P.tw = t.tw; P.pre = t.pre; P.post = t.post; P.win = t.win;
  const dim3 grid(cdiv(P.H, SLAB_HOPS), B), block(256);
  if (mode == DMX_MDCT_QUANT) hipLaunchKernelGGL(mdct_quant_kernel<DMX_MDCT_QUANT>, grid, block, 0, st, P);
  else if (mode == DMX_MDCT_PASS) hipLaunchKernelGGL(mdct_quant_kernel<DMX_MDCT_PASS>, grid, block, 0, st, P);
  else hipLaunchKernelGGL(mdct_quant_kernel<DMX_MDCT_PROJECT>, grid, block, 0, st, P);
  return hipGetLastError() == hipSuccess ? DMX_OK : DMX_ERR_LAUNCH;
}
