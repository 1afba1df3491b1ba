// Blind wow and flutter (no counterpart in the reference): the delay curve of the time-warp operator (warp.hip,
// section 8.10) is UNKNOWN -- the guided loop fits it next to the audio.  The estimate lives on coarse knots c[0 .. P], one every S =
// knot_stride fine knots (S a power of two <= 64, P = ceil(H / S)); the fine curve warp.hip reads is its linear interpolation
//   d[S p + q] = fmaf(q / S, c[p+1] - c[p], c[p])                                (q / S exact; q = 0 gives c[p], c[P+1] is never read)
// Two kernels, fp32, explicit fmaf / __fmul_rn / __fadd_rn / __fsub_rn so the build's contraction cannot change the order:
//
//   warp_wgrad   the gradient in the FINE knots as one pair per block.  With u = dLoss/dy at y = A_d x and n = 64 j + r (i, f as in warp.hip,
//                from warp_common.h):
//                  w'[-1] = fmaf(fmaf(-1.5, f, 2), f, -0.5)   w'[0] = fmaf(4.5, f, -5) * f   w'[1] = fmaf(fmaf(-4.5, f, 4), f, 0.5)
//                  w'[2]  = fmaf(1.5, f, -1) * f                                                  (the derivatives of the four weights in delta)
//                  s = +0, then s = fmaf(w'[k], x[i + k], s) for k = -1, 0, 1, 2 with 0 <= i + k < L (others neither loaded nor multiplied)
//                  g = u[n] * s, NaN where delta(n) is not finite, +0 for n >= L (nothing loaded)
//                  part[b, j, 0] = sum_r (1 - r / 64) g      part[b, j, 1] = sum_r (r / 64) g            (the weights are exact)
//                One wave owns one block, lane = r; both sums are the butterfly v <- v + v(lane xor t) for t = 32, 16, 8, 4, 2, 1, after
//                which every lane holds the same bits (fp32 addition commutes); lane 0 stores the pair.  No atomics, no LDS, an order fixed
//                by r alone: a clip's rows are the same bits alone, in a batch and at another batch position.
//   warp_update  one workgroup per clip, threads stride over the coarse knots.  dd[j] = part[j, 0] + part[j - 1, 1] (part[H, 0] and
//                part[-1, 1] do not exist), dc[p] = sum over j ascending with |j - S p| < S, 0 <= j <= H, by acc = fmaf(1 - |j - S p| / S,
//                dd[j], acc) from +0; one Adam step (adam_step.h) gives c~; anchor "mean": mean = (sum of c~) / (P + 1), the sum as
//                per-thread partials over p = tid, tid + 256, ... ascending and then the tree lds[t] += lds[t + h], h = 128 .. 1;
//                c = min(max(c~ - mean, -M), M).  A clip with a non-finite dc[p], c~[p] or mean keeps (c, m, v, d) bit for bit, decided
//                on the device.  Two passes over the knots (decide, then write), the second recomputing the first's values; then, behind
//                a barrier, the fine curve from the clip's new c.  Any bits in `part` are safe: nothing is indexed by a value.
//
// |c| <= M and M <= 8 S give |d[j+1] - d[j]| = |c[p+1] - c[p]| / S <= 16: every curve this kernel writes lies inside the contract of
// warp.hip, with no slope projection.  (Two knots at opposite clamps give exactly 16 S / S: the products are exact.  Knots within an ulp
// of opposite clamps can round a fine step to 16 + 2^-15; warp_bwd visits GATHER_CAP = 8 terms where the contract needs six.)
#include "dmx_common.h"
#include "kernels.h"
#include "warp_common.h"
#include "adam_step.h"
#include "../../include/diffmusic_hip.h"
#include <cmath>
void dmx_set_error(const char* fmt, ...);

namespace {

constexpr int UPD_T = 256;                 // threads of the update's workgroup
constexpr int MAX_L = 1 << 30;

// d w[k] / d delta at the fraction f, k = -1 .. 2
__device__ __forceinline__ float warp_dweight(int k, float f) {
  switch (k) {
    case -1: return fmaf(fmaf(-1.5f, f, 2.f), f, -0.5f);
    case 0: return __fmul_rn(fmaf(4.5f, f, -5.f), f);
    case 1: return fmaf(fmaf(-4.5f, f, 4.f), f, 0.5f);
    default: return __fmul_rn(fmaf(1.5f, f, -1.f), f);
  }
}

__global__ __launch_bounds__(256) void warp_wgrad_kernel(const float* __restrict__ dy, const float* __restrict__ x, long long xs,
                                                         const float* __restrict__ delay, long long ds, float* __restrict__ part, int L,
                                                         int H) {
  const int b = blockIdx.y, lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= H) return;                                        // wave-uniform
  const int n = j * R + lane;                                // < 64 H <= 2^30 + 63
  float g = 0.f;
  if (n < L) {
    const float* xr = x + (long long)b * xs;
    const float* dr = delay + (long long)b * ds;
    const float delta = warp_delta(dr[j], dr[j + 1], lane);  // j + 1 <= H: both knots exist
    float f;
    const int i = n + warp_split(delta, f);
    float s = 0.f;
#pragma unroll
    for (int k = -1; k <= 2; ++k) {
      const int t = i + k;
      if (t >= 0 && t < L) s = fmaf(warp_dweight(k, f), xr[t], s);
    }
    g = __fmul_rn(dy[(long long)b * L + n], s);
    if (!(fabsf(delta) <= 3.4028234663852886e38f)) g = __builtin_nanf("");
  }
  const float wr = (float)lane * (1.f / R);
  float a = __fmul_rn(1.f - wr, g), c = __fmul_rn(wr, g);    // 1 - r / 64 is exact
#pragma unroll
  for (int t = 32; t >= 1; t >>= 1) {
    a = __fadd_rn(a, __shfl_xor(a, t, 64));
    c = __fadd_rn(c, __shfl_xor(c, t, 64));
  }
  if (lane == 0) *reinterpret_cast<float2*>(part + ((long long)b * H + j) * 2) = make_float2(a, c);
}

// dc[p] of one clip from its partial pairs
__device__ __forceinline__ float coarse_grad(const float* __restrict__ part, int p, int S, int H) {
  const long long c = (long long)p * S;                      // <= H + S - 1
  const int lo = c - (S - 1) > 0 ? (int)(c - (S - 1)) : 0, hi = c + (S - 1) < H ? (int)(c + (S - 1)) : H;
  const float inv = 1.f / (float)S;                          // exact: S is a power of two
  float acc = 0.f;
  for (int j = lo; j <= hi; ++j) {
    const float dd = j == 0 ? part[0] : (j == H ? part[2 * (long long)(H - 1) + 1] : __fadd_rn(part[2 * (long long)j], part[2 * (long long)j - 1]));
    const int dist = j >= c ? (int)(j - c) : (int)(c - j);
    acc = fmaf(1.f - (float)dist * inv, dd, acc);
  }
  return acc;
}

__global__ __launch_bounds__(UPD_T) void warp_update_kernel(const float* __restrict__ parts, float* __restrict__ coarse, float* __restrict__ m,
                                                            float* __restrict__ v, float* __restrict__ fine, int H, int S, int P, AdamStep a,
                                                            float M, int anchor) {
  __shared__ float ssum[UPD_T];
  __shared__ int sbad;
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* part = parts + (long long)b * H * 2;
  float* cr = coarse + (long long)b * (P + 1);
  float* mr = m + (long long)b * (P + 1);
  float* vr = v + (long long)b * (P + 1);
  float* fr = fine + (long long)b * (H + 1);
  if (tid == 0) sbad = 0;
  __syncthreads();
  float sum = 0.f;
  int bad = 0;
  for (int p = tid; p <= P; p += UPD_T) {                    // pass 1: decide
    const float dc = coarse_grad(part, p, S, H);
    float mn, vn, cn;
    adam_tap(dc, mr[p], vr[p], cr[p], a, mn, vn, cn);
    bad |= !(isfinite(dc) && isfinite(cn));
    sum = __fadd_rn(sum, cn);
  }
  ssum[tid] = sum;
  if (bad) sbad = 1;
  __syncthreads();
  for (int h = UPD_T / 2; h >= 1; h >>= 1) {
    if (tid < h) ssum[tid] = __fadd_rn(ssum[tid], ssum[tid + h]);
    __syncthreads();
  }
  const float mean = anchor ? __fdiv_rn(ssum[0], (float)(P + 1)) : 0.f;
  if (sbad || !isfinite(mean)) return;                       // uniform over the workgroup
  for (int p = tid; p <= P; p += UPD_T) {                    // pass 2: the same values again, written
    const float dc = coarse_grad(part, p, S, H);
    float mn, vn, cn;
    adam_tap(dc, mr[p], vr[p], cr[p], a, mn, vn, cn);
    cr[p] = fminf(fmaxf(__fsub_rn(cn, mean), -M), M);
    mr[p] = mn;
    vr[p] = vn;
  }
  __syncthreads();                                           // the clip's new knots are visible to its workgroup
  const float inv = 1.f / (float)S;
  for (int j = tid; j <= H; j += UPD_T) {
    const int p = j / S, q = j - p * S;                      // p <= P; q = 0 where p = P (S P >= H)
    const float c0 = cr[p];
    fr[j] = q == 0 ? c0 : fmaf((float)q * inv, __fsub_rn(cr[p + 1], c0), c0);
  }
}

bool delay_stride_ok(long long ds, int L) { return ds == 0 || ds >= (long long)cdiv(L, R) + 1; }
bool knot_stride_ok(int S) { return S >= 1 && S <= 64 && (S & (S - 1)) == 0; }

}  // namespace

extern "C" int dmx_warp_wgrad(const float* dy, const float* x, long long x_stride, const float* delay, long long delay_stride, float* part,
                              int batch, int L, void* stream) {
  if (!dy || !x || !delay || !part || batch < 1 || batch > 65535 || L < 1 || L > MAX_L || x_stride < L || !delay_stride_ok(delay_stride, L)) {
    dmx_set_error("warp_wgrad: dy (batch, L) contiguous, x (batch, >= L) with row stride >= L, delay (H + 1) with stride 0 or (batch, >= H + 1), "
                  "part (batch, H, 2) contiguous, H = ceil(L / 64), 1 <= batch <= 65535, 1 <= L <= 2^30");
    return DMX_ERR_SHAPE;
  }
  const int H = cdiv(L, R);
  hipLaunchKernelGGL(warp_wgrad_kernel, dim3((unsigned)cdiv(H, 4), (unsigned)batch), dim3(256), 0, (hipStream_t)stream, dy, x, x_stride, delay,
                     delay_stride, part, L, H);
  return hipGetLastError() == hipSuccess ? DMX_OK : DMX_ERR_LAUNCH;
}

extern "C" int dmx_warp_update(const float* part, float* coarse, float* m, float* v, float* fine, int batch, int L, int knot_stride, int k,
                               double lr, double beta1, double beta2, double eps, double max_delay, int anchor, void* stream) {
  if (!part || !coarse || !m || !v || !fine || batch < 1 || L < 1 || L > MAX_L || !knot_stride_ok(knot_stride)) {
    dmx_set_error("warp_update: part (batch, H, 2), coarse, m and v (batch, P + 1), fine (batch, H + 1), all contiguous, H = ceil(L / 64), "
                  "P = ceil(H / knot_stride), knot_stride a power of two in 1 .. 64, batch >= 1, 1 <= L <= 2^30");
    return DMX_ERR_SHAPE;
  }
  if (!adam_args_ok(lr, beta1, beta2, eps, k)) {
    dmx_set_error("warp_update: lr > 0, betas in [0, 1), eps >= 0 and k >= 1 (the 1-based count of updates) are required");
    return DMX_ERR_SHAPE;
  }
  const double box = 8.0 * knot_stride < 4096.0 ? 8.0 * knot_stride : 4096.0;
  if (!(max_delay > 0.0 && max_delay <= box)) {
    dmx_set_error("warp_update: 0 < max_delay <= min(4096, 8 * knot_stride) keeps every written curve inside the contract of warp_bwd");
    return DMX_ERR_SHAPE;
  }
  if (anchor != 0 && anchor != 1) {
    dmx_set_error("warp_update: anchor is 0 (none) or 1 (mean)");
    return DMX_ERR_SHAPE;
  }
  const int H = cdiv(L, R), P = cdiv(H, knot_stride);
  hipLaunchKernelGGL(warp_update_kernel, dim3((unsigned)batch), dim3(UPD_T), 0, (hipStream_t)stream, part, coarse, m, v, fine, H, knot_stride,
                     P, adam_step_of(lr, beta1, beta2, eps, k), (float)max_delay, anchor);
  return hipGetLastError() == hipSuccess ? DMX_OK : DMX_ERR_LAUNCH;
}
