// One Adam step of one parameter in fp32, shared by the four blind operators' update kernels (fir_blind.hip: the taps of an impulse response;
// tf_eq.hip: the bins of a curve; warp_fit.hip: delay knots; drc_fit.hip: compressor parameters): same arithmetic, same order, in all four.
#pragma once
#include <cmath>
#include "dmx_common.h"

namespace {

// One Adam step of one tap, every operation rounded on its own (no contraction: the two passes of the update must agree bit for bit)
struct AdamStep {                                            // host scalars of one step, each rounded to fp32 from its float64 value
  float lr, b1, b2, omb1, omb2, eps, bc1, bc2;               // omb = 1 - beta, bc = 1 - beta^k (1 - 0.999f would be off by 1e-5 of itself)
};
__device__ __forceinline__ void adam_tap(float g, float m, float v, float h, const AdamStep& a, float& mn, float& vn, float& hn) {
#pragma clang fp contract(off)
  mn = a.b1 * m + a.omb1 * g;
  vn = a.b2 * v + (a.omb2 * g) * g;
  hn = h - a.lr * (mn / a.bc1) / (sqrtf(vn / a.bc2) + a.eps);
}

// the scalars of update k (1-based) from their float64 values
inline AdamStep adam_step_of(double lr, double beta1, double beta2, double eps, int k) {
  return {(float)lr, (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps,
          (float)(1.0 - std::pow(beta1, (double)k)), (float)(1.0 - std::pow(beta2, (double)k))};
}
inline bool adam_args_ok(double lr, double beta1, double beta2, double eps, int k) {
  return lr > 0.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0 && k >= 1;
}

}  // namespace
