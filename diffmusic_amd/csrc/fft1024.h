// 1024-point complex FFT of one wave in LDS: radix-4 Stockham, five in-place passes, both directions (unnormalised).  Shared by the fused
// STFT -> mel kernels (stft_mel.hip) and the time-frequency gain kernel (tf_gain.hip); both include this header, so they run the same
// arithmetic in the same order.  Twiddles: s_tw[m] = exp(-2 pi i m / 1024), m = 0 .. 1023, in LDS.
#pragma once
#include "dmx_common.h"

namespace {

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// radix-4 butterfly, natural output order y_r = sum_q v_q exp(-/+ 2 pi i r q / 4)
template <bool INV>
__device__ __forceinline__ void bfly4(float2& v0, float2& v1, float2& v2, float2& v3) {
  const float2 a = make_float2(v0.x + v2.x, v0.y + v2.y), b = make_float2(v0.x - v2.x, v0.y - v2.y);
  const float2 c = make_float2(v1.x + v3.x, v1.y + v3.y);
  const float2 d0 = make_float2(v1.x - v3.x, v1.y - v3.y);
  const float2 d = INV ? make_float2(-d0.y, d0.x) : make_float2(d0.y, -d0.x);        // * (+i) : * (-i)
  v0 = make_float2(a.x + c.x, a.y + c.y);
  v2 = make_float2(a.x - c.x, a.y - c.y);
  v1 = make_float2(b.x + d.x, b.y + d.y);
  v3 = make_float2(b.x - d.x, b.y - d.y);
}

// One Stockham pass over the wave's 1024 complex points, IN PLACE: every lane first reads the 16 inputs of its four butterflies
// (j = lane + 64 m), then writes their 16 outputs.  LDS instructions of one wave execute in issue order and all 64 lanes issue
// together, so every read of the pass precedes every write of the pass; the fences keep the compiler from mixing the two groups.
template <int NS, bool INV>
__device__ __forceinline__ void fft_pass(float2* buf, const float2* s_tw, int lane) {
  float2 v[4][4];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int j = lane + 64 * m;
#pragma unroll
    for (int q = 0; q < 4; ++q) v[m][q] = buf[j + 256 * q];
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int j = lane + 64 * m;
    const int k = j & (NS - 1);
    if (NS > 1) {
#pragma unroll
      for (int q = 1; q < 4; ++q) {
        float2 w = s_tw[q * k * (256 / NS)];
        if (INV) w.y = -w.y;
        v[m][q] = cmul(v[m][q], w);
      }
    }
    bfly4<INV>(v[m][0], v[m][1], v[m][2], v[m][3]);
    const int j0 = ((j - k) << 2) + k;
#pragma unroll
    for (int q = 0; q < 4; ++q) buf[j0 + q * NS] = v[m][q];
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

template <bool INV>
__device__ __forceinline__ void fft1024(float2* buf, const float2* s_tw, int lane) {
  fft_pass<1, INV>(buf, s_tw, lane);
  fft_pass<4, INV>(buf, s_tw, lane);
  fft_pass<16, INV>(buf, s_tw, lane);
  fft_pass<64, INV>(buf, s_tw, lane);
  fft_pass<256, INV>(buf, s_tw, lane);
}

}  // namespace
