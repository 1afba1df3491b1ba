// Declicking (impulsive noise: clicks, crackle, ticks, dropouts; no counterpart in the reference): the autoregressive click detector, the
// dilation of its flags into one sample mask per clip, the per-clip mask product and the output blend.  DESIGN.md section 8.13 has the
// definition; per clip, y zero outside [0, L), N = 1024 samples per frame, P = 16 the model order, F = ceil(L / N) frames.  For frame j,
// live samples n in [jN, min(L, (j+1)N)), c of them:
//
//   s[i]  = h[i] y[jN - 512 + i], i = 0 .. 2047       h the periodic Hann window of 2048 = sin^2(pi i / 2048)
//   r[k]  = sum_{i=0}^{2047-k} s[i] s[i+k], k = 0 .. 16
//   a     = 0 unless r[0] is a finite positive number, else Levinson-Durbin on (r[0] (1 + 1e-3), r[1], .., r[16])
//   e[n]  = y[n] - sum_{i=1}^{16} a[i] y[n-i]
//   med   = the |e[n]| of rank ceil(c / 2) (1-based, ascending by the uint32 bit pattern of |e|, so NaNs come last)
//   sigma = med / 0.6745f                              flag[n] = |e[n]| > K * (sigma > floor ? sigma : floor)
//
// Arithmetic of click_detect, in this order whatever the batch or the batch position (explicit fmaf / __f*_rn, so the build's contraction
// cannot change it); t = 0 .. 255 is the thread:
//   h[i]    = w * w, w = sinpif(i / 2048) (i / 2048 is exact); s[i] = h[i] * y
//   r[k]    = (w0 + w1) + (w2 + w3), w the tree over a wave's 64 lanes (strides 32, 16, .., 1: p[l] += p[l + stride]) of
//             p[t] = fmaf chain, from +0, over i = t, t + 256, .. while i + k <= 2047 (ascending)
//   a       one thread, fp32: E = r[0] * 1.001f; for m = 1 .. 16: acc = r[m], then acc = fmaf(-a[i], r[m-i], acc) for i = 1 .. m-1;
//           k = acc / E; a'[i] = fmaf(-k, a[m-i], a[i]) for i < m, a'[m] = k; E = E * (1 - k * k) as fmaf(-k, k, 1) * E
//   e[n]    = y[n] - acc, acc = fmaf chain from +0 over i = 1 .. 16 of a[i] y[n-i]
//   med     32-round bitwise select on the keys (integers: no order to fix); sigma one IEEE division; the threshold one product
// A NaN or Inf in the window makes r[0] non-finite, so that frame has a = 0 and e = y, except that the 16 samples after the bad one are
// NaN too (0 * NaN in their history); a frame whose window does not hold it has no history that does (the window reaches 512 samples
// back).  A NaN |e| is never flagged (the compare is false), and a NaN median gives sigma = NaN, for which the threshold is K * floor.
//
//   click_detect   one workgroup of 256 threads per (frame, clip); 2048 raw and 2048 windowed samples, the per-wave partial sums, the
//                  Levinson arrays and the select counters in LDS (about 17 KB static); the select keys stay in registers
//   click_mask     one workgroup of 1024 threads per clip, looping over the clip: m[n] = 0 where a flag lies within `guard` samples; the
//                  zeros are counted in integers (exact in any order), reduced through LDS, no atomics
//   mask_rows      y[b, n] = x[b, n] * m[b, n], n < L, +0 on [L, Ly): the forward (Ly = L) and its own transpose (Ly = full)
//   declick_blend  out = y where no m = 0 lies within `fade` samples, x where m = 0, else w y + (1 - w) x as two rounded products and one
//                  rounded sum, w = d / (fade + 1), d the distance to the nearest m = 0
// Every index is compared with [0, L) before its load; nothing depends on the values of y except through arithmetic.
#include "dmx_common.h"
#include "kernels.h"
#include "../../include/diffmusic_hip.h"
#include <cmath>
void dmx_set_error(const char* fmt, ...);

namespace {

constexpr int N = DMX_CLICK_FRAME;         // samples per frame
constexpr int P = DMX_CLICK_ORDER;         // model order
constexpr int W = 2 * N;                   // window length
constexpr int LEAD = N / 2;                // the window starts LEAD samples before the frame
constexpr int T = 256;                     // threads of click_detect
constexpr int MAX_L = 1 << 30;

__global__ __launch_bounds__(T) void click_detect_kernel(const float* __restrict__ y, long long ys, float* __restrict__ a_out,
                                                         float* __restrict__ e_out, float* __restrict__ sigma_out,
                                                         unsigned char* __restrict__ flags, float* __restrict__ r_out, int L, int F, float K,
                                                         float floor_) {
  __shared__ float sy[W];                  // y[jN - LEAD + i], zero outside [0, L)
  __shared__ float ss[W];                  // windowed
  __shared__ float wpart[(P + 1) * (T / 64)];
  __shared__ float sr[P + 1], sa[P + 1], san[P + 1];
  __shared__ int cnt[T / 64];
  const int j = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  const float* yr = y + (long long)b * ys;
  const int base = j * N - LEAD;           // j * N < L <= 2^30
  for (int i = t; i < W; i += T) {
    const int n = base + i;
    const float v = (n >= 0 && n < L) ? yr[n] : 0.f;
    const float w = sinpif((float)i * (1.f / W));
    sy[i] = v;
    ss[i] = __fmul_rn(__fmul_rn(w, w), v);
  }
  __syncthreads();
#pragma unroll 1
  for (int k = 0; k <= P; ++k) {
    float p = 0.f;
    for (int i = t; i + k < W; i += T) p = fmaf(ss[i], ss[i + k], p);
    for (int o = 32; o > 0; o >>= 1) p = __fadd_rn(p, __shfl_down(p, o, 64));      // lane 0: the tree over its wave's 64 lanes
    if ((t & 63) == 0) wpart[k * (T / 64) + (t >> 6)] = p;
  }
  __syncthreads();
  if (t == 0) {                            // Levinson-Durbin, one thread; its arrays live in LDS (dynamic indices, no scratch)
    for (int k = 0; k <= P; ++k) {
      const float* w = wpart + k * (T / 64);
      sr[k] = __fadd_rn(__fadd_rn(w[0], w[1]), __fadd_rn(w[2], w[3]));
      sa[k] = 0.f;
    }
    if (sr[0] > 0.f && sr[0] <= 3.4028234663852886e38f) {
      float E = __fmul_rn(sr[0], 1.001f);
#pragma unroll 1
      for (int m = 1; m <= P; ++m) {
        float acc = sr[m];
        for (int i = 1; i < m; ++i) acc = fmaf(-sa[i], sr[m - i], acc);
        const float k = __fdiv_rn(acc, E);
        for (int i = 1; i < m; ++i) san[i] = fmaf(-k, sa[m - i], sa[i]);
        for (int i = 1; i < m; ++i) sa[i] = san[i];
        sa[m] = k;
        E = __fmul_rn(fmaf(-k, k, 1.f), E);
      }
    }
  }
  __syncthreads();
  if (t <= P && r_out) r_out[((long long)b * F + j) * (P + 1) + t] = sr[t];
  if (t >= 1 && t <= P) a_out[((long long)b * F + j) * P + (t - 1)] = sa[t];
  // the residual of the frame's samples: thread t owns n = jN + t + 256 q
  const int live = L - j * N < N ? L - j * N : N;          // c >= 1
  float ev[N / T];
  unsigned key[N / T];
#pragma unroll
  for (int q = 0; q < N / T; ++q) {
    const int o = t + T * q;               // offset in the frame; sy index LEAD + o, history down to LEAD + o - 16 >= 0
    float acc = 0.f;
#pragma unroll
    for (int i = 1; i <= P; ++i) acc = fmaf(sa[i], sy[LEAD + o - i], acc);
    ev[q] = __fsub_rn(sy[LEAD + o], acc);
    key[q] = o < live ? (__float_as_uint(ev[q]) & 0x7fffffffu) : 0xffffffffu;
  }
  // the key of rank ceil(c / 2): a 32-round bitwise select over the 1024 keys (dead ones are the largest)
  unsigned prefix = 0u;
  int rank = (live + 1) / 2 - 1;           // 0-based
#pragma unroll 1
  for (int bit = 31; bit >= 0; --bit) {
    const unsigned him = bit == 31 ? 0u : ~((2u << bit) - 1u), one = 1u << bit;
    int c0 = 0;
#pragma unroll
    for (int q = 0; q < N / T; ++q) c0 += ((key[q] & him) == prefix && !(key[q] & one)) ? 1 : 0;
    for (int o = 32; o > 0; o >>= 1) c0 += __shfl_down(c0, o, 64);
    if ((t & 63) == 0) cnt[t >> 6] = c0;
    __syncthreads();
    int tot = 0;
#pragma unroll
    for (int w = 0; w < T / 64; ++w) tot += cnt[w];
    __syncthreads();
    if (rank >= tot) { rank -= tot; prefix |= one; }
  }
  const float sigma = __fdiv_rn(__uint_as_float(prefix), 0.6745f);
  const float thr = __fmul_rn(K, sigma > floor_ ? sigma : floor_);
  if (t == 0) sigma_out[(long long)b * F + j] = sigma;
#pragma unroll
  for (int q = 0; q < N / T; ++q) {
    const int o = t + T * q;
    if (o < live) {
      const long long at = (long long)b * L + j * N + o;
      e_out[at] = ev[q];
      flags[at] = fabsf(ev[q]) > thr ? 1 : 0;
    }
  }
}

constexpr int MT = 1024;                   // threads of click_mask

__global__ __launch_bounds__(MT) void click_mask_kernel(const unsigned char* __restrict__ flags, float* __restrict__ mask,
                                                        int* __restrict__ masked, int L, int guard) {
  __shared__ int cnt[MT / 64];
  const int b = blockIdx.x, t = threadIdx.x;
  const unsigned char* fr = flags + (long long)b * L;
  float* mr = mask + (long long)b * L;
  int zeros = 0;
  for (int n0 = 0; n0 < L; n0 += MT) {     // n0 <= 2^30 - 1, n0 + t stays inside an int
    const int n = n0 + t;
    if (n < L) {
      const int lo = n - guard > 0 ? n - guard : 0, hi = L - 1 - n > guard ? n + guard : L - 1;
      int hit = 0;
      for (int q = lo; q <= hi; ++q) hit |= fr[q];
      mr[n] = hit ? 0.f : 1.f;
      zeros += hit ? 1 : 0;
    }
  }
  for (int o = 32; o > 0; o >>= 1) zeros += __shfl_down(zeros, o, 64);
  if ((t & 63) == 0) cnt[t >> 6] = zeros;
  __syncthreads();
  if (t == 0) {
    int tot = 0;
    for (int w = 0; w < MT / 64; ++w) tot += cnt[w];
    masked[b] = tot;
  }
}

__global__ __launch_bounds__(256) void mask_rows_kernel(const float* __restrict__ x, long long xs, const float* __restrict__ m, long long ms,
                                                        float* __restrict__ y, int L, int Ly) {
  const int b = blockIdx.y, n0 = 4 * (blockIdx.x * 256 + threadIdx.x);
  const float* xr = x + (long long)b * xs;
  const float* mr = m + (long long)b * ms;
  float* yr = y + (long long)b * Ly;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int n = n0 + e;
    if (n < Ly) yr[n] = n < L ? __fmul_rn(xr[n], mr[n]) : 0.f;
  }
}

__global__ __launch_bounds__(256) void declick_blend_kernel(const float* __restrict__ x, long long xs, const float* __restrict__ y, long long ys,
                                                            const float* __restrict__ m, long long ms, float* __restrict__ out, int L, int fade) {
  const int b = blockIdx.y, n = blockIdx.x * 256 + threadIdx.x;
  if (n >= L) return;
  const float* mr = m + (long long)b * ms;
  const float xv = x[(long long)b * xs + n], yv = y[(long long)b * ys + n];
  int d = fade + 1;                        // none within fade
  if (mr[n] == 0.f) {
    d = 0;
  } else {
    for (int q = 1; q <= fade; ++q) {
      const bool left = n - q >= 0 && mr[n - q] == 0.f, right = n + q < L && mr[n + q] == 0.f;
      if (left || right) { d = q; break; }
    }
  }
  float o = yv;
  if (d == 0) {
    o = xv;
  } else if (d <= fade) {
    const float w = __fdiv_rn((float)d, (float)(fade + 1));
    o = __fadd_rn(__fmul_rn(w, yv), __fmul_rn(__fsub_rn(1.f, w), xv));
  }
  out[(long long)b * L + n] = o;
}

bool mask_stride_ok(long long ms, int L) { return ms == 0 || ms >= L; }
// a row stride below the row length; with one row the stride is never used (a (1, L) view may carry any)
bool short_stride(long long stride, int L, int batch) { return batch > 1 && stride < L; }

}  // namespace

extern "C" int dmx_click_detect(const float* y, long long y_stride, float* a, float* e, float* sigma, unsigned char* flags, float* r, int batch,
                                int L, float threshold, float sigma_floor, void* stream) {
  if (!y || !a || !e || !sigma || !flags || batch < 1 || batch > 65535 || L < 1 || L > MAX_L || short_stride(y_stride, L, batch)) {
    dmx_set_error("click_detect: y (batch, >= L) with row stride >= L, a (batch, F, 16), e and flags (batch, L), sigma (batch, F), r null or "
                  "(batch, F, 17), F = ceil(L / 1024), 1 <= batch <= 65535, 1 <= L <= 2^30");
    return DMX_ERR_SHAPE;
  }
  if (!(threshold > 0.f) || !(threshold <= 3.4028234663852886e38f)) {
    dmx_set_error("click_detect: threshold = %g: a finite number > 0 (the multiple K of the robust scale above which a residual is a click)",
                  (double)threshold);
    return DMX_ERR_SHAPE;
  }
  if (!(sigma_floor >= 0.f) || !(sigma_floor <= 3.4028234663852886e38f)) {
    dmx_set_error("click_detect: sigma_floor = %g: a finite number >= 0 (the smallest robust scale a frame is given)", (double)sigma_floor);
    return DMX_ERR_SHAPE;
  }
  const int F = cdiv(L, N);
  hipLaunchKernelGGL(click_detect_kernel, dim3((unsigned)F, (unsigned)batch), dim3(T), 0, (hipStream_t)stream, y, y_stride, a, e, sigma, flags, r,
                     L, F, threshold, sigma_floor);
  return hipGetLastError() == hipSuccess ? DMX_OK : DMX_ERR_LAUNCH;
}

extern "C" int dmx_click_mask(const unsigned char* flags, float* mask, int* masked, int batch, int L, int guard, void* stream) {
  if (!flags || !mask || !masked || batch < 1 || batch > 65535 || L < 1 || L > MAX_L) {
    dmx_set_error("click_mask: flags and mask (batch, L) contiguous, masked (batch), 1 <= batch <= 65535, 1 <= L <= 2^30");
    return DMX_ERR_SHAPE;
  }
  if (guard < 0 || guard > DMX_CLICK_MAX_GUARD) {
    dmx_set_error("click_mask: guard = %d: 0 .. %d samples on each side of a flagged sample", guard, DMX_CLICK_MAX_GUARD);
    return DMX_ERR_SHAPE;
  }
  hipLaunchKernelGGL(click_mask_kernel, dim3((unsigned)batch), dim3(MT), 0, (hipStream_t)stream, flags, mask, masked, L, guard);
  return hipGetLastError() == hipSuccess ? DMX_OK : DMX_ERR_LAUNCH;
}

extern "C" int dmx_mask_rows(const float* x, long long x_stride, const float* mask, long long mask_stride, float* y, int batch, int L, int Ly,
                             void* stream) {
  if (!x || !mask || !y || batch < 1 || batch > 65535 || L < 1 || Ly < L || Ly > MAX_L || short_stride(x_stride, L, batch) || !mask_stride_ok(mask_stride, L)) {
    dmx_set_error("mask_rows: x (batch, >= L) with row stride >= L, mask (L) with stride 0 or (batch, >= L), y (batch, Ly >= L) contiguous, "
                  "1 <= batch <= 65535, 1 <= L <= Ly <= 2^30");
    return DMX_ERR_SHAPE;
  }
  hipLaunchKernelGGL(mask_rows_kernel, dim3((unsigned)cdiv(cdiv(Ly, 4), 256), (unsigned)batch), dim3(256), 0, (hipStream_t)stream, x, x_stride,
                     mask, mask_stride, y, L, Ly);
  return hipGetLastError() == hipSuccess ? DMX_OK : DMX_ERR_LAUNCH;
}

extern "C" int dmx_declick_blend(const float* x, long long x_stride, const float* y, long long y_stride, const float* mask, long long mask_stride,
                                 float* out, int batch, int L, int fade, void* stream) {
  if (!x || !y || !mask || !out || batch < 1 || batch > 65535 || L < 1 || L > MAX_L || short_stride(x_stride, L, batch) || short_stride(y_stride, L, batch) ||
      !mask_stride_ok(mask_stride, L)) {
    dmx_set_error("declick_blend: x and y (batch, >= L) with row strides >= L, mask (L) with stride 0 or (batch, >= L), out (batch, L) "
                  "contiguous, 1 <= batch <= 65535, 1 <= L <= 2^30");
    return DMX_ERR_SHAPE;
  }
  if (fade < 0 || fade > DMX_CLICK_MAX_GUARD) {
    dmx_set_error("declick_blend: fade = %d: 0 .. %d samples of cross-fade on each side of a masked run", fade, DMX_CLICK_MAX_GUARD);
    return DMX_ERR_SHAPE;
  }
  hipLaunchKernelGGL(declick_blend_kernel, dim3((unsigned)cdiv(L, 256), (unsigned)batch), dim3(256), 0, (hipStream_t)stream, x, x_stride, y,
                     y_stride, mask, mask_stride, out, L, fade);
  return hipGetLastError() == hipSuccess ? DMX_OK : DMX_ERR_LAUNCH;
}
