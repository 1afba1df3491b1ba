// Dynamic-range compression on materialised waveforms (the de-compression operator; no counterpart in the reference): a feed-forward
// compressor / limiter whose sidechain runs at block rate, R = 64 samples, and the transpose of its Jacobian.  DESIGN.md section 8.9 has
// the definition and the derivation; per clip, x zero outside [0, L), H = ceil(L / 64) blocks:
//
//   p[j] = (1/64) sum_r x[64 j + r]^2          l = 10 log10(p + 1e-10)        d = l - T
//   c[j] = 0 (2 d < -W, region 0) | kq (d + W/2)^2 (2 d <= W, region 1; kq = k / (2 W)) | k d (region 2)         k = 1 - 1 / ratio
//   s[j] = s[j-1] + (c[j] > s[j-1] ? aA : aR) (c[j] - s[j-1]),  s[-1] = 0            G[j] = 10^((makeup - s[j]) / 20), G[-1] from s = 0
//   y[64 j + r] = (G[j-1] + ((r + 1) / 64) (G[j] - G[j-1])) x[64 j + r]
//
// Three launches per direction: a parallel block reduction, the serial follower, a parallel apply.
//   forward   drc_power    a thread owns four consecutive samples (the float4 / scalar row rule of waveshape.hip), 16 lanes own a block;
//                          writes p[j], c[j] (into the s row) and the region bits of the tape byte
//             drc_follow   lane = clip, one thread walks the H blocks: c and the tape bytes are prefetched a chunk of 16 ahead into
//                          registers, so the dependent chain (compare, select, subtract, multiply-add) holds no load and, in whole
//                          chunks, no branch; writes s[j] over c[j] and bit 2 (att) of the tape byte
//             drc_apply    a workgroup owns 16 blocks: its first 17 threads evaluate G[j0 - 1 .. j0 + 15] from s into LDS (and the owners
//                          store G[j]), then every thread interpolates and multiplies.  17 / 16 H exponentials and H logarithms per clip
//   backward  drc_dgain    the same 16-lane reduction of q = dy x against the weights w_r and 1 - w_r; a workgroup also reduces the block after
//                          its last one, so that ds[j] = -(ln 10 / 20) G[j] (A[j] + B[j+1]) leaves the kernel complete, into `work`
//             drc_follow_bwd  lane = clip, backwards in time, gates from the tape: tot = ds[j] + carry, dc[j] = a tot, carry = (1 - a) tot;
//                          dc[j] replaces ds[j] in `work`
//             drc_apply_bwd   dp[j] = dc[j] c'[j] (10 / ln 10) / (p[j] + eps) per block in LDS (c' from the tape's region, never re-decided),
//                          then dx = g dy + dp (2 / 64) x; zeros on [L, full)
// Two parameter routes, one arithmetic (drc_common.h): dmx_drc_fwd / dmx_drc_bwd pass host scalars shared by the batch (ByValue);
// dmx_drc_fwd_p / dmx_drc_bwd_p read row b of a device table theta (batch, 8) = T, k, makeup, aA, aR, 1 - aA, 1 - aR, k / (2 W) for clip b
// (ByTable; section 8.12, the blind operator).  The power and apply-backward kernels index the row by blockIdx.y, a follower lane reads its
// own coefficients once before the chain; the table's values are operands only, and a row with a non-finite entry makes its clip NaN from
// block 0 on.  The table backward keeps ds beside dc (work is (batch, 2, H)) and Bq[0] of each clip for drc_fit.hip.
// Reductions, in this order whatever the batch, the batch position or the load path: a lane adds its four terms left to right, then the
// 16 lanes of a block add pairwise over lane distances 1, 2, 4, 8 (xor butterfly: every lane holds the same bits).  No atomics.
// log10f and exp10f are the accurate library routines.  A NaN sample makes p, c and s NaN from its block on: the forward's outputs are NaN
// from the first sample of that block to the end of the clip and untouched before it; the backward's dx is NaN for that whole clip (the
// recurrence carries it down to block 0).  Other clips are untouched.
// The followers read rows that start at any multiple of 4 bytes (c, ds) or of 1 byte (tape), H elements apart across lanes: the compiler
// merges a chunk's loads and stores into dwordx4 accesses at those alignments, which the global address space allows; they are uncoalesced
// across lanes by construction (one cache line per clip and chunk), which is what lane = clip costs at large batches.
#include "dmx_common.h"
#include "kernels.h"
#include "drc_common.h"
#include "../../include/diffmusic_hip.h"
#include <cmath>
void dmx_set_error(const char* fmt, ...);

namespace {

constexpr int WG_BLOCKS = 16;         // blocks per workgroup of 256 threads x 4 samples
constexpr int CHUNK = 16;             // blocks the follower prefetches ahead
constexpr float C10 = 4.3429448190325175f;          // 10 / ln 10
constexpr float NEG_LN10_20 = -0.11512925464970229f; // -(ln 10) / 20

__device__ __forceinline__ bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// samples i .. i + 3 of a row with n valid samples (positions >= n read nothing and give 0)
__device__ __forceinline__ void load4(const float* row, bool vec, long long i, long long n, float (&v)[4]) {
  if (vec && i + 3 < n) {
    const float4 t = *reinterpret_cast<const float4*>(row + i);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = i + e < n ? row[i + e] : 0.f;
  }
}
__device__ __forceinline__ void store4(float* row, bool vec, long long i, long long n, const float (&v)[4]) {
  if (vec && i + 3 < n) {
    *reinterpret_cast<float4*>(row + i) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) if (i + e < n) row[i + e] = v[e];
  }
}

// the sum over the 16 lanes of a block, the same bits in every lane
__device__ __forceinline__ float block_sum(float v) {
#pragma unroll
  for (int m = 1; m < 16; m <<= 1) v += __shfl_xor(v, m);
  return v;
}

// Every kernel that reads a parameter is a template on its source (drc_common.h): ByValue is the host-scalar route of dmx_drc_fwd /
// dmx_drc_bwd, ByTable the per-clip device table of dmx_drc_fwd_p / dmx_drc_bwd_p.  The arithmetic is one text for both.
template <class Src>
__global__ __launch_bounds__(256) void drc_power_kernel(const float* __restrict__ x, long long xs, float* __restrict__ state,
                                                        unsigned char* __restrict__ tape, int L, int H, Src src) {
  const int b = blockIdx.y;
  const long long i = 4ll * (blockIdx.x * 256 + threadIdx.x);
  const float* xr = x + (long long)b * xs;
  float v[4];
  load4(xr, aligned16(xr), i, L, v);
  float q = v[0] * v[0];
#pragma unroll
  for (int e = 1; e < 4; ++e) q += v[e] * v[e];
  q = block_sum(q);
  const int j = (int)(i / R);
  if ((threadIdx.x & 15) != 0 || j >= H) return;
  const DrcParams P = src.clip(b);
  const float p = q * (1.f / R);
  const float d = level_over_threshold(p, P.T);
  float c;
  const int rg = curve_decide(d, P, c);
  state_row(state, b, H, 0)[j] = p;
  state_row(state, b, H, 2)[j] = c;                        // the follower replaces it by s[j]
  tape[(size_t)b * H + j] = (unsigned char)rg;
}

// one chunk of the follower: CHUNK blocks from j0 upwards.  GUARD = false for a whole chunk (no branch in the loads or in the chain),
// true for the clip's last, partial one
template <bool GUARD>
__device__ __forceinline__ void follow_load(const float* srow, const unsigned char* trow, int j0, int H, float (&c)[CHUNK],
                                            unsigned char (&t)[CHUNK]) {
#pragma unroll
  for (int k = 0; k < CHUNK; ++k) {
    const bool in = !GUARD || j0 + k < H;
    c[k] = in ? srow[j0 + k] : 0.f;
    t[k] = in ? trow[j0 + k] : (unsigned char)0;
  }
}
template <bool GUARD>
__device__ __forceinline__ float follow_steps(float* srow, unsigned char* trow, int j0, int H, const float (&c)[CHUNK],
                                              const unsigned char (&t)[CHUNK], float s, float aA, float aR) {
#pragma unroll
  for (int k = 0; k < CHUNK; ++k) {
    if (!GUARD || j0 + k < H) {
      const bool att = c[k] > s;                           // a NaN compares false: release
      s = s + (att ? aA : aR) * (c[k] - s);
      srow[j0 + k] = s;
      trow[j0 + k] = (unsigned char)(t[k] | (att ? 4 : 0));
    }
  }
  return s;
}

template <class Src>
__global__ __launch_bounds__(64) void drc_follow_kernel(float* __restrict__ state, unsigned char* __restrict__ tape, int B, int H, Src src) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  float aA, aR;
  src.follower(b, aA, aR);                                 // once, before the chain
  float* srow = state_row(state, b, H, 2);
  unsigned char* trow = tape + (size_t)b * H;
  const int whole = H / CHUNK;
  float cn[CHUNK], cc[CHUNK];
  unsigned char tn[CHUNK], tc[CHUNK];
  if (whole > 0) follow_load<false>(srow, trow, 0, H, cn, tn);
  float s = 0.f;
  for (int m = 0; m < whole; ++m) {
#pragma unroll
    for (int k = 0; k < CHUNK; ++k) { cc[k] = cn[k]; tc[k] = tn[k]; }
    if (m + 1 < whole) follow_load<false>(srow, trow, (m + 1) * CHUNK, H, cn, tn);     // issued before the chain, waited for one chunk later
    s = follow_steps<false>(srow, trow, m * CHUNK, H, cc, tc, s, aA, aR);
  }
  if (whole * CHUNK < H) {
    follow_load<true>(srow, trow, whole * CHUNK, H, cn, tn);
    follow_steps<true>(srow, trow, whole * CHUNK, H, cn, tn, s, aA, aR);
  }
}

template <class Src>
__global__ __launch_bounds__(256) void drc_apply_kernel(const float* __restrict__ x, long long xs, float* __restrict__ y, long long ys,
                                                        float* __restrict__ state, int L, int H, Src src) {
  __shared__ float Gs[WG_BLOCKS + 1];
  const int b = blockIdx.y, tid = threadIdx.x, j0 = blockIdx.x * WG_BLOCKS;
  if (tid <= WG_BLOCKS) {
    const int j = j0 - 1 + tid;
    const float makeup = src.makeup(b);
    float g = 0.f;
    if (j < H) {
      g = block_gain(j < 0 ? 0.f : state_row(state, b, H, 2)[j], makeup);
      if (tid > 0) state_row(state, b, H, 1)[j] = g;
    }
    Gs[tid] = g;
  }
  __syncthreads();
  const long long i = 4ll * (blockIdx.x * 256 + tid);
  if (i >= L) return;
  const float* xr = x + (long long)b * xs;
  float* yr = y + (long long)b * ys;
  const float gp = Gs[tid >> 4], dg = Gs[(tid >> 4) + 1] - gp;
  const int r0 = 4 * (tid & 15);
  float v[4];
  load4(xr, aligned16(xr), i, L, v);
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = (gp + (float)(r0 + e + 1) * (1.f / R) * dg) * v[e];
  store4(yr, aligned16(yr), i, L, v);
}

// A = sum_r q[r] w_r and B = sum_r q[r] (1 - w_r) of the block the 16 lanes own, q = dy x, w_r = (r + 1) / 64
__device__ __forceinline__ void weighted_sums(const float* gr, bool gvec, const float* xr, bool xvec, long long i, int L, float& A, float& Bq) {
  float g[4], v[4];
  load4(gr, gvec, i, L, g);
  load4(xr, xvec, i, L, v);
  const int r0 = (int)(i & (R - 1));
  float a = 0.f, c = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float q = g[e] * v[e], w = (float)(r0 + e + 1) * (1.f / R);
    if (e == 0) { a = q * w; c = q * (1.f - w); } else { a += q * w; c += q * (1.f - w); }
  }
  A = block_sum(a);
  Bq = block_sum(c);
}

// KEEP (the table route, for drc_fit.hip): a clip's work is two rows, ds and dc, and Bq[0] of the clip goes to bq0[b]
template <bool KEEP>
__device__ __forceinline__ size_t work_row(int b, int H) { return (size_t)b * H * (KEEP ? 2 : 1); }

template <bool KEEP>
__global__ __launch_bounds__(256) void drc_dgain_kernel(const float* __restrict__ dy, long long dys, const float* __restrict__ x, long long xs,
                                                        const float* __restrict__ state, float* __restrict__ work, float* __restrict__ bq0, int L,
                                                        int H) {
  __shared__ float As[WG_BLOCKS], Bs[WG_BLOCKS + 1];
  const int b = blockIdx.y, tid = threadIdx.x, j0 = blockIdx.x * WG_BLOCKS;
  const float* gr = dy + (long long)b * dys;
  const float* xr = x + (long long)b * xs;
  const bool gvec = aligned16(gr), xvec = aligned16(xr);
  float A, Bq;
  weighted_sums(gr, gvec, xr, xvec, 4ll * (blockIdx.x * 256 + tid), L, A, Bq);
  if ((tid & 15) == 0) { As[tid >> 4] = A; Bs[tid >> 4] = Bq; }
  if (tid < 16) {                                          // the block after the workgroup's last one (zeros past L)
    weighted_sums(gr, gvec, xr, xvec, (long long)R * (j0 + WG_BLOCKS) + 4 * tid, L, A, Bq);
    if (tid == 0) Bs[WG_BLOCKS] = Bq;
  }
  __syncthreads();
  const int j = j0 + tid;
  if (tid < WG_BLOCKS && j < H) {
    float dG = As[tid];
    if (j + 1 < H) dG += Bs[tid + 1];
    work[work_row<KEEP>(b, H) + j] = (state_row(state, b, H, 1)[j] * dG) * NEG_LN10_20;
  }
  if (KEEP && blockIdx.x == 0 && tid == 0) bq0[b] = Bs[0];
}

// one chunk of the backward recurrence: CHUNK blocks from `top` downwards
template <bool GUARD>
__device__ __forceinline__ void follow_bwd_load(const float* wrow, const unsigned char* trow, int top, float (&d)[CHUNK], unsigned char (&t)[CHUNK]) {
#pragma unroll
  for (int k = 0; k < CHUNK; ++k) {
    const bool in = !GUARD || top - k >= 0;
    d[k] = in ? wrow[top - k] : 0.f;
    t[k] = in ? trow[top - k] : (unsigned char)0;
  }
}
template <bool GUARD>
__device__ __forceinline__ float follow_bwd_steps(float* orow, int top, const float (&d)[CHUNK], const unsigned char (&t)[CHUNK], float carry,
                                                  float aA, float aR, float bA, float bR) {
#pragma unroll
  for (int k = 0; k < CHUNK; ++k) {
    if (!GUARD || top - k >= 0) {
      const bool att = (t[k] & 4) != 0;
      const float tot = d[k] + carry;
      orow[top - k] = (att ? aA : aR) * tot;
      carry = (att ? bA : bR) * tot;
    }
  }
  return carry;
}

template <class Src>
__global__ __launch_bounds__(64) void drc_follow_bwd_kernel(float* __restrict__ work, const unsigned char* __restrict__ tape, int B, int H,
                                                            Src src) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  float aA, aR, bA, bR;
  src.follower_bwd(b, aA, aR, bA, bR);                     // once, before the chain
  float* wrow = work + work_row<Src::TABLE>(b, H);         // ds
  float* orow = wrow + (Src::TABLE ? H : 0);               // dc: over ds, or the row after it
  const unsigned char* trow = tape + (size_t)b * H;
  const int whole = H / CHUNK;
  float dn[CHUNK], dc[CHUNK];
  unsigned char tn[CHUNK], tc[CHUNK];
  if (whole > 0) follow_bwd_load<false>(wrow, trow, H - 1, dn, tn);
  float carry = 0.f;
  for (int m = 0; m < whole; ++m) {
#pragma unroll
    for (int k = 0; k < CHUNK; ++k) { dc[k] = dn[k]; tc[k] = tn[k]; }
    if (m + 1 < whole) follow_bwd_load<false>(wrow, trow, H - 1 - (m + 1) * CHUNK, dn, tn);
    carry = follow_bwd_steps<false>(orow, H - 1 - m * CHUNK, dc, tc, carry, aA, aR, bA, bR);
  }
  if (whole * CHUNK < H) {
    const int top = H - 1 - whole * CHUNK;
    follow_bwd_load<true>(wrow, trow, top, dn, tn);
    follow_bwd_steps<true>(orow, top, dn, tn, carry, aA, aR, bA, bR);
  }
}

template <class Src>
__global__ __launch_bounds__(256) void drc_apply_bwd_kernel(const float* __restrict__ dy, long long dys, const float* __restrict__ x, long long xs,
                                                            const float* __restrict__ state, const unsigned char* __restrict__ tape,
                                                            const float* __restrict__ work, float* __restrict__ dx, long long dxs, int L,
                                                            int full, int H, Src src) {
  __shared__ float Gs[WG_BLOCKS + 1], Ds[WG_BLOCKS];
  const int b = blockIdx.y, tid = threadIdx.x, j0 = blockIdx.x * WG_BLOCKS;
  const DrcParams P = src.clip(b);
  const float* dcrow = work + work_row<Src::TABLE>(b, H) + (Src::TABLE ? H : 0);
  if (tid <= WG_BLOCKS) {
    const int j = j0 - 1 + tid;
    Gs[tid] = j < 0 ? block_gain(0.f, P.makeup) : (j < H ? state_row(state, b, H, 1)[j] : 0.f);
  }
  if (tid < WG_BLOCKS) {
    const int j = j0 + tid;
    float dp = 0.f;
    if (j < H) {
      const int rg = tape[(size_t)b * H + j] & 3;
      const float p = state_row(state, b, H, 0)[j];
      const float slope = curve_slope(p, rg, P);
      dp = ((dcrow[j] * slope) * C10) / (p + EPS) * (2.f / R);
    }
    Ds[tid] = dp;
  }
  __syncthreads();
  const long long i = 4ll * (blockIdx.x * 256 + tid);
  if (i >= full) return;
  const float* gr = dy + (long long)b * dys;
  const float* xr = x + (long long)b * xs;
  float* dr = dx + (long long)b * dxs;
  const float gp = Gs[tid >> 4], dg = Gs[(tid >> 4) + 1] - gp, dp = Ds[tid >> 4];
  const int r0 = 4 * (tid & 15);
  float g[4], v[4];
  load4(gr, aligned16(gr), i, L, g);
  load4(xr, aligned16(xr), i, L, v);
#pragma unroll
  for (int e = 0; e < 4; ++e)
    g[e] = i + e < L ? (gp + (float)(r0 + e + 1) * (1.f / R) * dg) * g[e] + dp * v[e] : 0.f;      // the tail is zero whatever the state holds
  store4(dr, aligned16(dr), i, full, g);
}

inline dim3 row_grid(int n, int B) { return dim3((unsigned)cdiv(cdiv(n, 4), 256), (unsigned)B); }

bool drc_params(const char* who, float T, float slope, float knee, float aA, float aR, float makeup, DrcParams& P) {
  const bool ok = std::isfinite(T) && std::fabs(T) <= 200.f && slope >= 0.f && slope <= 1.f && std::isfinite(knee) && knee >= 0.f && knee <= 200.f &&
                  aA > 0.f && aA <= 1.f && aR > 0.f && aR <= 1.f && std::isfinite(makeup) && std::fabs(makeup) <= 200.f;
  if (!ok) {
    dmx_set_error("%s: threshold_db and makeup_db finite within +-200, 0 <= slope = 1 - 1 / ratio <= 1, 0 <= knee_db <= 200, attack and release "
                  "coefficients in (0, 1]", who);
    return false;
  }
  P.T = T; P.k = slope; P.W = knee; P.halfW = 0.5f * knee;
  P.kq = knee > 0.f ? (float)((double)slope / (2.0 * (double)knee)) : 0.f;
  P.aA = aA; P.aR = aR; P.bA = (float)(1.0 - (double)aA); P.bR = (float)(1.0 - (double)aR);
  P.makeup = makeup;
  return true;
}

constexpr int MAX_L = 1 << 30;

bool fwd_shapes(const char* who, const void* x, const void* y, const void* state, const void* tape, int batch, int L, long long x_stride,
                long long y_stride) {
  if (!x || !y || !state || !tape || batch < 1 || batch > 65535 || L < 1 || L > MAX_L || x_stride < L || y_stride < L) {
    dmx_set_error("%s: x (batch, >= L), y (batch, L) with row strides >= L, state (batch, 3, H) and tape (batch, H) contiguous, "
                  "H = ceil(L / 64), 1 <= batch <= 65535, 1 <= L <= 2^30", who);
    return false;
  }
  return true;
}
bool bwd_shapes(const char* who, const char* work_shape, const void* dy, const void* x, const void* state, const void* tape, const void* work,
                const void* dx, int batch, int L, int Lfull, long long dy_stride, long long x_stride, long long dx_stride) {
  if (!dy || !x || !state || !tape || !work || !dx || batch < 1 || batch > 65535 || L < 1 || L > MAX_L || Lfull < L || Lfull > MAX_L ||
      dy_stride < L || x_stride < L || dx_stride < Lfull) {
    dmx_set_error("%s: dy and x (batch, >= L), dx (batch, Lfull >= L) with row strides >= their lengths, state (batch, 3, H), tape and "
                  "work %s contiguous, H = ceil(L / 64), 1 <= batch <= 65535, 1 <= L <= Lfull <= 2^30", who, work_shape);
    return false;
  }
  return true;
}
bool table_ok(const char* who, const float* theta, float knee) {
  if (!theta || !(std::isfinite(knee) && knee >= 0.f && knee <= 200.f)) {
    dmx_set_error("%s: theta (batch, 8) fp32 on the device, rows T, k, makeup, aA, aR, 1 - aA, 1 - aR, k / (2 knee_db), and 0 <= knee_db <= 200",
                  who);
    return false;
  }
  return true;
}

// the three launches of a direction, for either parameter source
template <class Src>
int launch_fwd(const float* x, long long x_stride, float* y, long long y_stride, float* state, unsigned char* tape, int batch, int L,
               const Src& src, hipStream_t st) {
  const int H = cdiv(L, R);
  hipLaunchKernelGGL(drc_power_kernel<Src>, row_grid(L, batch), dim3(256), 0, st, x, x_stride, state, tape, L, H, src);
  hipLaunchKernelGGL(drc_follow_kernel<Src>, dim3((unsigned)cdiv(batch, 64)), dim3(64), 0, st, state, tape, batch, H, src);
  hipLaunchKernelGGL(drc_apply_kernel<Src>, row_grid(L, batch), dim3(256), 0, st, x, x_stride, y, y_stride, state, L, H, src);
  return hipGetLastError() == hipSuccess ? DMX_OK : DMX_ERR_LAUNCH;
}
template <class Src>
int launch_bwd(const float* dy, long long dy_stride, const float* x, long long x_stride, const float* state, const unsigned char* tape,
               float* work, float* bq0, float* dx, long long dx_stride, int batch, int L, int Lfull, const Src& src, hipStream_t st) {
  const int H = cdiv(L, R);
  hipLaunchKernelGGL(drc_dgain_kernel<Src::TABLE>, row_grid(L, batch), dim3(256), 0, st, dy, dy_stride, x, x_stride, state, work, bq0, L, H);
  hipLaunchKernelGGL(drc_follow_bwd_kernel<Src>, dim3((unsigned)cdiv(batch, 64)), dim3(64), 0, st, work, tape, batch, H, src);
  hipLaunchKernelGGL(drc_apply_bwd_kernel<Src>, row_grid(Lfull, batch), dim3(256), 0, st, dy, dy_stride, x, x_stride, state, tape,
                     (const float*)work, dx, dx_stride, L, Lfull, H, src);
  return hipGetLastError() == hipSuccess ? DMX_OK : DMX_ERR_LAUNCH;
}

}  // namespace

extern "C" int dmx_drc_fwd(const float* x, long long x_stride, float* y, long long y_stride, float* state, unsigned char* tape, int batch, int L,
                           float threshold_db, float slope, float knee_db, float a_att, float a_rel, float makeup_db, void* stream) {
  if (!fwd_shapes("drc_fwd", x, y, state, tape, batch, L, x_stride, y_stride)) return DMX_ERR_SHAPE;
  ByValue src;
  if (!drc_params("drc_fwd", threshold_db, slope, knee_db, a_att, a_rel, makeup_db, src.P)) return DMX_ERR_SHAPE;
  return launch_fwd(x, x_stride, y, y_stride, state, tape, batch, L, src, (hipStream_t)stream);
}

extern "C" int dmx_drc_bwd(const float* dy, long long dy_stride, const float* x, long long x_stride, const float* state, const unsigned char* tape,
                           float* work, float* dx, long long dx_stride, int batch, int L, int Lfull, float threshold_db, float slope, float knee_db,
                           float a_att, float a_rel, float makeup_db, void* stream) {
  if (!bwd_shapes("drc_bwd", "(batch, H)", dy, x, state, tape, work, dx, batch, L, Lfull, dy_stride, x_stride, dx_stride)) return DMX_ERR_SHAPE;
  ByValue src;
  if (!drc_params("drc_bwd", threshold_db, slope, knee_db, a_att, a_rel, makeup_db, src.P)) return DMX_ERR_SHAPE;
  return launch_bwd(dy, dy_stride, x, x_stride, state, tape, work, nullptr, dx, dx_stride, batch, L, Lfull, src, (hipStream_t)stream);
}

// The same three launches per direction with the parameters of clip b read from theta[b, 0:8] on the device (drc_common.h, ByTable).  The
// backward keeps what the parameter gradient needs: work is (batch, 2, H), rows ds and dc, and bq0 (batch,) holds Bq[0] of each clip.
extern "C" int dmx_drc_fwd_p(const float* x, long long x_stride, float* y, long long y_stride, float* state, unsigned char* tape, const float* theta,
                             int batch, int L, float knee_db, void* stream) {
  if (!fwd_shapes("drc_fwd_p", x, y, state, tape, batch, L, x_stride, y_stride) || !table_ok("drc_fwd_p", theta, knee_db)) return DMX_ERR_SHAPE;
  return launch_fwd(x, x_stride, y, y_stride, state, tape, batch, L, ByTable{theta, knee_db}, (hipStream_t)stream);
}

extern "C" int dmx_drc_bwd_p(const float* dy, long long dy_stride, const float* x, long long x_stride, const float* state,
                             const unsigned char* tape, const float* theta, float* work, float* bq0, float* dx, long long dx_stride, int batch,
                             int L, int Lfull, float knee_db, void* stream) {
  if (!bwd_shapes("drc_bwd_p", "(batch, 2, H)", dy, x, state, tape, work, dx, batch, L, Lfull, dy_stride, x_stride, dx_stride) ||
      !table_ok("drc_bwd_p", theta, knee_db))
    return DMX_ERR_SHAPE;
  if (!bq0) {
    dmx_set_error("drc_bwd_p: bq0 (batch,) fp32 is required");
    return DMX_ERR_SHAPE;
  }
  return launch_bwd(dy, dy_stride, x, x_stride, state, tape, work, bq0, dx, dx_stride, batch, L, Lfull, ByTable{theta, knee_db},
                    (hipStream_t)stream);
}
