// What drc.hip (the compressor and the transpose of its Jacobian) and drc_fit.hip (the gradient in the compressor's parameters) share, so
// that both evaluate the level and the static curve with the same expressions: the constants, the parameter block, the level over the
// threshold, the block gain, the curve and its slope by region, and the two sources a kernel can take its parameters from.
#pragma once
#include "dmx_common.h"
#include "kernels.h"

namespace {

constexpr int R = DMX_DRC_BLOCK;      // samples per sidechain block
constexpr float EPS = 1e-10f;
constexpr int DRC_ROW = 8;            // floats of a table row: T, k, makeup, aA, aR, bA, bR, kq

struct DrcParams { float T, k, W, halfW, kq, aA, aR, bA, bR, makeup; };

__device__ __forceinline__ float level_over_threshold(float p, float T) { return 10.f * log10f(p + EPS) - T; }
__device__ __forceinline__ float block_gain(float s, float makeup) { return exp10f((makeup - s) * 0.05f); }

// the static curve at d = level - T: the region it decides and c
__device__ __forceinline__ int curve_decide(float d, const DrcParams& P, float& c) {
  int rg = 2;
  c = P.k * d;
  if (2.f * d < -P.W) { rg = 0; c = 0.f; }
  else if (2.f * d <= P.W) { rg = 1; const float t = d + P.halfW; c = P.kq * t * t; }
  return rg;
}
// c by a region decided earlier (the tape's), never re-decided
__device__ __forceinline__ float curve_by_region(float d, int rg, const DrcParams& P) {
  float c = 0.f;
  if (rg == 2) c = P.k * d;
  else if (rg == 1) { const float t = d + P.halfW; c = P.kq * t * t; }
  return c;
}
// dc / dd by the tape's region; p is only read in region 1
__device__ __forceinline__ float curve_slope(float p, int rg, const DrcParams& P) {
  float slope = 0.f;
  if (rg == 2) slope = P.k;
  else if (rg == 1) slope = 2.f * P.kq * (level_over_threshold(p, P.T) + P.halfW);
  return slope;
}

// state (B, 3, H): rows p, G, s of a clip
__device__ __forceinline__ float* state_row(float* state, int b, int H, int row) { return state + ((size_t)b * 3 + row) * H; }
__device__ __forceinline__ const float* state_row(const float* state, int b, int H, int row) { return state + ((size_t)b * 3 + row) * H; }

// Where a kernel takes its parameters from, chosen at compile time.  ByValue: host scalars shared by the batch.  ByTable: a device table
// (batch, 8) fp32, one row per clip, W a host scalar.  A row's values are only ever operands, never indices; a row with a non-finite entry
// gets T = makeup = NaN, which makes c, s and G of that clip NaN from block 0 on whatever the other entries hold.
struct ByValue {
  static constexpr bool TABLE = false;
  DrcParams P;
  __device__ __forceinline__ DrcParams clip(int) const { return P; }
  __device__ __forceinline__ void follower(int, float& aA, float& aR) const { aA = P.aA; aR = P.aR; }
  __device__ __forceinline__ void follower_bwd(int, float& aA, float& aR, float& bA, float& bR) const { aA = P.aA; aR = P.aR; bA = P.bA; bR = P.bR; }
  __device__ __forceinline__ float makeup(int) const { return P.makeup; }
};
struct ByTable {
  static constexpr bool TABLE = true;
  const float* theta;
  float W;
  __device__ __forceinline__ DrcParams clip(int b) const {
    const float* t = theta + (size_t)b * DRC_ROW;
    DrcParams P;
    P.T = t[0]; P.k = t[1]; P.makeup = t[2]; P.aA = t[3]; P.aR = t[4]; P.bA = t[5]; P.bR = t[6]; P.kq = t[7];
    P.W = W; P.halfW = 0.5f * W;
    bool fin = true;
#pragma unroll
    for (int e = 0; e < DRC_ROW; ++e) fin = fin && isfinite(t[e]);
    if (!fin) P.T = P.makeup = __builtin_nanf("");
    return P;
  }
  __device__ __forceinline__ void follower(int b, float& aA, float& aR) const {
    const float* t = theta + (size_t)b * DRC_ROW;
    aA = t[3]; aR = t[4];
  }
  __device__ __forceinline__ void follower_bwd(int b, float& aA, float& aR, float& bA, float& bR) const {
    const float* t = theta + (size_t)b * DRC_ROW;
    aA = t[3]; aR = t[4]; bA = t[5]; bR = t[6];
  }
  __device__ __forceinline__ float makeup(int b) const { return theta[(size_t)b * DRC_ROW + 2]; }
};

}  // namespace
