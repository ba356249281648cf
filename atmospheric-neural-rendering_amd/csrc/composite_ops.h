// The per-sample expressions and wave scans of the f32 composite (composite.hip) that the
// forward-only render kernel (field_fused.hip, render_kernel) shares with it.
#pragma once

#include "anr_common.h"

namespace anr {

// alpha = 1 - exp(-x) (graphics_utils.py:38) as -expm1(-x): accurate to an ulp of alpha
// itself. Evaluated as 1 - expf(-x), f32 loses log2(1/x) bits to cancellation, and at
// BASELINE configs[2]'s 1,024 samples per ray x = sigma * delta is ~1e-6 at
// initialisation: dL/dcolor = w * dL/dC then carries 2e-2 relative error and the GPU
// exp's rounding bias accumulates in the dir-MLP gradient (tools/composite_diag.py).
__device__ __forceinline__ float alpha_of(float x) { return -expm1f(-x); }

// Exclusive multiplicative scan across the wave (lane 0 gets 1).
__device__ __forceinline__ float wave_excl_prod(float v, int lane) {
  float incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const float o = shfl_up(incl, d);
    if (lane >= d) incl *= o;
  }
  const float ex = shfl_up(incl, 1);
  return lane == 0 ? 1.0f : ex;
}
__device__ __forceinline__ float wave_prod(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v *= shfl_xor(v, m);
  return v;
}

}  // namespace anr
