// Blind dereverberation (no counterpart in the reference, whose MusicDereverberationOperator always knows its response): the impulse
// response is an unknown that the guided loop fits next to the audio.  Two kernels, fp32 throughout:
//   weight gradient  dh[b, t] = sum_o dy[b, o] * x[b, o + t - off],  t in [0, taps), o in [0, Lout), x zero outside [0, L)
//   update           Adam on (h, m, v) from dh, then the peak normalisation h <- h' / max|h'| of generate_impulse_response
// with the conventions of dmx_fir_fwd in the dense 1:1 case (off = taps / 2, Lout = L + 2 * (taps / 2) - taps + 1).
//
// dh is a correlation with `taps` outputs that each reduce over Lout terms (5000 x 160000 at production size), so both are split: grid =
// (tap tiles, reduction segments, batch).  A block owns WTILE = 1024 taps, four CONSECUTIVE ones per thread, and the WSEG = 4096 outputs of
// its segment in chunks of WCH = 512: dy[chunk] and the x window under it are staged in LDS as fir_dense_kernel does, and four outputs are
// taken per pass, so a thread reads its 4 + 3 window samples as two 16-byte LDS reads (lane stride 16 bytes: conflict-free) and the four
// dy values as one broadcast read, for 16 FMAs.  A tap's terms are added in increasing o, every block writes one row of the workspace
// (batch, segments, taps), and the update sums the rows in segment order: no atomics, the same bits every time, and nothing in a clip's
// result depends on the batch or on the clip's place in it (the segment length is a constant).
#include <cmath>
#include "dmx_common.h"
#include "kernels.h"
#include "adam_step.h"
#include "../../include/diffmusic_hip.h"
void dmx_set_error(const char* fmt, ...);

namespace {

constexpr int WT = 256, WR = 4, WTILE = WT * WR, WCH = 512, WSEG = 4096;
constexpr int UT = 1024, UMAX = 8192;                       // update: threads per clip, most taps

__global__ __launch_bounds__(WT) void fir_wgrad_kernel(const float* __restrict__ dy, long long dy_stride, const float* __restrict__ x,
                                                       long long x_stride, float* __restrict__ ws, int L, int Lout, int taps, int off) {
  __shared__ __attribute__((aligned(16))) float sdy[WCH];
  __shared__ __attribute__((aligned(16))) float sx[WCH + WTILE];
  const int t0 = blockIdx.x * WTILE, seg = blockIdx.y, b = blockIdx.z;
  const int o_beg = seg * WSEG, o_end = min(Lout, o_beg + WSEG);
  const float* dyr = dy + (long long)b * dy_stride;
  const float* xr = x + (long long)b * x_stride;
  float acc[WR] = {0.f, 0.f, 0.f, 0.f};
  for (int o0 = o_beg; o0 < o_end; o0 += WCH) {
    __syncthreads();
    for (int i = threadIdx.x; i < WCH; i += WT) sdy[i] = o0 + i < o_end ? dyr[o0 + i] : 0.f;
    for (int i = threadIdx.x; i < WCH + WTILE; i += WT) {
      const int s = o0 + t0 - off + i;                      // sx[i] = x[o0 + i + t0 - off]: output o0 + oo under tap t0 + tt sits at oo + tt
      sx[i] = (s >= 0 && s < L) ? xr[s] : 0.f;
    }
    __syncthreads();
    const int no = min(WCH, (o_end - o0 + 3) & ~3);         // whole quads: the zeros staged past o_end add nothing
    const float* win = sx + WR * threadIdx.x;
    for (int oo = 0; oo < no; oo += 4) {
      const float4 d = *reinterpret_cast<const float4*>(sdy + oo);
      const float4 a = *reinterpret_cast<const float4*>(win + oo);
      const float4 c = *reinterpret_cast<const float4*>(win + oo + 4);
      const float dv[4] = {d.x, d.y, d.z, d.w};
      const float w[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < WR; ++r) acc[r] += dv[j] * w[j + r];
    }
  }
  float* row = ws + ((long long)b * gridDim.y + seg) * taps;
#pragma unroll
  for (int r = 0; r < WR; ++r) {
    const int t = t0 + WR * threadIdx.x + r;
    if (t < taps) row[t] = acc[r];
  }
}

// One workgroup per clip: g = the partial rows summed in segment order, Adam, max|h'| over the clip, h = h' / max|h'| and its reverse.
// A clip with a non-finite g or h', or with max|h'| == 0, is left exactly as it was (decided here: no host round trip).
__global__ __launch_bounds__(UT) void ir_update_kernel(const float* __restrict__ ws, int nseg, float* __restrict__ h, float* __restrict__ h_rev,
                                                       float* __restrict__ m, float* __restrict__ v, int taps, AdamStep a) {
  __shared__ float sg[UMAX];
  __shared__ float smax[UT / 64];
  __shared__ int sbad[UT / 64];
  const int b = blockIdx.x;
  const float* part = ws + (long long)b * nseg * taps;
  float* hb = h + (long long)b * taps;
  float* rb = h_rev + (long long)b * taps;
  float* mb = m + (long long)b * taps;
  float* vb = v + (long long)b * taps;
  float mx = 0.f;
  int bad = 0;
  for (int i = threadIdx.x; i < taps; i += UT) {
    float g = 0.f;
    for (int s = 0; s < nseg; ++s) g += part[(long long)s * taps + i];
    sg[i] = g;
    float mn, vn, hn;
    adam_tap(g, mb[i], vb[i], hb[i], a, mn, vn, hn);
    bad |= !(isfinite(g) && isfinite(hn));
    mx = fmaxf(mx, fabsf(hn));
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
  for (int w = 0; w < UT / 64; ++w) {
    mx = fmaxf(mx, smax[w]);
    bad |= sbad[w];
  }
  if (bad || !(mx > 0.f)) return;                           // uniform over the workgroup
  for (int i = threadIdx.x; i < taps; i += UT) {
    float mn, vn, hn;
    adam_tap(sg[i], mb[i], vb[i], hb[i], a, mn, vn, hn);
    const float hv = hn / mx;
    hb[i] = hv;
    rb[taps - 1 - i] = hv;
    mb[i] = mn;
    vb[i] = vn;
  }
}

inline int wgrad_segments(int Lout) { return cdiv(Lout, WSEG); }

}  // namespace

extern "C" size_t dmx_fir_wgrad_workspace_floats(int batch, int Lout, int taps) {
  if (batch < 1 || Lout < 1 || taps < 1) return 0;
  return (size_t)batch * (size_t)wgrad_segments(Lout) * (size_t)taps;
}

extern "C" int dmx_fir_wgrad(const float* dy, long long dy_stride, const float* x, long long x_stride, float* partials, size_t partial_floats,
                             int batch, int L, int Lout, int taps, void* stream) {
  if (!dy || !x || !partials || batch < 1 || batch > 65535 || L < 1 || taps < 1 || Lout < 1 || Lout != L + 2 * (taps / 2) - taps + 1 ||
      dy_stride < Lout || x_stride < L || (long long)L + taps > (1ll << 30)) {
    dmx_set_error("fir_wgrad: dy (batch, Lout), x (batch, >= L) with row strides >= their lengths, Lout = L + 2 * (taps / 2) - taps + 1 >= 1, "
                  "1 <= batch <= 65535, L + taps <= 2^30");
    return DMX_ERR_SHAPE;
  }
  const int nseg = wgrad_segments(Lout);
  if (partial_floats < (size_t)batch * nseg * taps) {
    dmx_set_error("fir_wgrad: the workspace holds %zu floats, (batch, segments, taps) = (%d, %d, %d) are needed", partial_floats, batch, nseg, taps);
    return DMX_ERR_SHAPE;
  }
  hipLaunchKernelGGL(fir_wgrad_kernel, dim3((unsigned)cdiv(taps, WTILE), (unsigned)nseg, (unsigned)batch), dim3(WT), 0, (hipStream_t)stream, dy,
                     dy_stride, x, x_stride, partials, L, Lout, taps, taps / 2);
  return hipGetLastError() == hipSuccess ? DMX_OK : DMX_ERR_LAUNCH;
}

extern "C" int dmx_ir_update(const float* partials, int segments, float* h, float* h_rev, float* m, float* v, int batch, int taps, double lr,
                             double beta1, double beta2, double eps, int k, void* stream) {
  if (!partials || !h || !h_rev || !m || !v || batch < 1 || segments < 1 || taps < 1) {
    dmx_set_error("ir_update: partials (batch, segments, taps), h, h_rev, m and v (batch, taps) are required");
    return DMX_ERR_SHAPE;
  }
  if (taps > UMAX) {
    dmx_set_error("ir_update: %d taps, one workgroup per clip covers at most %d", taps, UMAX);
    return DMX_ERR_SHAPE;
  }
  if (!adam_args_ok(lr, beta1, beta2, eps, k)) {
    dmx_set_error("ir_update: lr > 0, betas in [0, 1), eps >= 0 and k >= 1 (the 1-based count of updates) are required");
    return DMX_ERR_SHAPE;
  }
  const AdamStep a = adam_step_of(lr, beta1, beta2, eps, k);
  hipLaunchKernelGGL(ir_update_kernel, dim3((unsigned)batch), dim3(UT), 0, (hipStream_t)stream, partials, segments, h, h_rev, m, v, taps, a);
  return hipGetLastError() == hipSuccess ? DMX_OK : DMX_ERR_LAUNCH;
}
