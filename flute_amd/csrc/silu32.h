// silu32: the one activation of the fused SwiGLU launches - the row form (qgemm_grouped.h, Glu mode) and the block form
// (qgemm_block2.h, GM = 3) include it from here, so both compute the same bits from the same g.
#pragma once
#include <hip/hip_runtime.h>

namespace flute_amd {

// silu32(g) = g / (1 + exp(-g)), fp32.  expf is within 1 ulp (2^-23 relative), the sum 1 + t and the quotient are
// correctly rounded (2^-24 each; IEEE division is hipcc's default), and an error of t enters 1 + t scaled by
// t / (1 + t) < 1: relative error <= 2^-23 + 2 * 2^-24 = 2^-22 to first order, for every |g| <= 88 (exp(88) is finite;
// exp(-88) underflows against the 1).  With the fp32 product by u (2^-24) behind it: eps_s = 2^-21 covers both.
__device__ __forceinline__ float silu32(float g) { return g / (1.0f + expf(-g)); }

}  // namespace flute_amd
