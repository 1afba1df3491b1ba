// Fused convolution-pair launcher (conv_pair.hip) and the profiling hooks it shares with gemm_conv.hip.
#pragma once
#include <cstdlib>
#include <cstring>
#include "dmx_common.h"

// Rows of a clip that a pair launch may leave alone (HiFi-GAN under an inpainting mask: hifigan.hip, DeadPlan), both per clip, [lo, hi):
//   skip: output rows nobody reads.  The launcher rounds the interval INWARD to whole output slabs and runs no workgroup for them; the
//         partly dead slabs at its edges run as always.  Nothing is written to a skipped slab (tensor, tape bits, accumulation).
//   zero: rows of the first stage's input whose true value is zero but which memory need not hold (a producer skipped them): loaded
//         as zeros, like the rows outside the clip.  The second stage's residual must then be the same tensor (taken from the slab).
// Every row that is still computed runs the instructions it always ran.
struct PairDead { int skip0 = 0, skip1 = 0, zero0 = 0, zero1 = 0; };

bool dmx_conv_pair_eligible(const GemmDesc* a, const GemmDesc& b);
int dmx_conv_pair_launch(const GemmDesc* a, const GemmDesc& b, hipStream_t st, const PairDead* dead = nullptr);
// n (<= 3) mutually independent pairs of one width as a single grid, longest first (the branches of a HiFi-GAN resblock step);
// dead: nullptr or n entries
int dmx_conv_pair_group_launch(int n, const GemmDesc* const* a, const GemmDesc* const* b, hipStream_t st, const PairDead* dead = nullptr);
// output slabs per clip of the launch of this pair (a == nullptr: single stage): how many `dead` skips, and how many there are
void dmx_conv_pair_slabs(const GemmDesc* a, const GemmDesc& b, const PairDead* dead, int* skipped, int* total);

// profiling records for launches that do not go through dmx_gemm_launch (no-ops unless dmx_prof_begin is active)
int dmx_prof_open(hipStream_t st);
void dmx_prof_close(int rec, hipStream_t st, double flops, double bytes, int M, int N, int K, int taps, int flags, int cfg);
