// The position arithmetic of the time-warp operator, shared by warp.hip (the operator and its transpose) and warp_fit.hip (the gradient in
// the knots): both include this header, so they decide delta, floorf and the fraction with the same operations in the same order.
// DESIGN.md section 8.10 has the definitions.
#pragma once
#include <cmath>
#include "dmx_common.h"
#include "kernels.h"

namespace {

constexpr int R = DMX_WARP_BLOCK;          // samples per knot interval
constexpr float INT_CLAMP = 1073741760.f;  // 2^30 - 64, an fp32 number

// delta(n) for r = n mod 64 between the knots d0 = d[j] and d1 = d[j+1]
__device__ __forceinline__ float warp_delta(float d0, float d1, int r) { return fmaf((float)r * (1.f / R), __fsub_rn(d1, d0), d0); }

// delta -> the integer offset floorf(delta), clamped before the conversion (a NaN becomes -INT_CLAMP), and the fraction
__device__ __forceinline__ int warp_split(float delta, float& f) {
  const float fl = floorf(delta);
  f = __fsub_rn(delta, fl);
  return (int)fminf(fmaxf(fl, -INT_CLAMP), INT_CLAMP);
}

// the Catmull-Rom weight of tap k = -1 .. 2 at the fraction f
__device__ __forceinline__ float warp_weight(int k, float f) {
  const float ff = __fmul_rn(f, f);
  switch (k) {
    case -1: return __fmul_rn(f, fmaf(fmaf(-0.5f, f, 1.f), f, -0.5f));
    case 0: return fmaf(fmaf(1.5f, f, -2.5f), ff, 1.f);
    case 1: return __fmul_rn(f, fmaf(fmaf(-1.5f, f, 2.f), f, 0.5f));
    default: return __fmul_rn(ff, fmaf(0.5f, f, -0.5f));
  }
}

// i(n) and f(n) of a clip from its knots; 0 <= n < L, so both knots exist
__device__ __forceinline__ int warp_pos(const float* __restrict__ dr, int n, float& f) {
  const int j = n >> 6;
  return n + warp_split(warp_delta(dr[j], dr[j + 1], n & (R - 1)), f);
}

}  // namespace
