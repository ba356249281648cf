// The per-sample device functions of the reference-numerics composite (ref16.hip), shared
// with the forward-only render kernel (field_fused.hip, render_kernel). Every function
// body switches fp contraction off itself, so a translation unit that contracts by default
// forms the same roundings.
#pragma once

#include "anr_common.h"

namespace anr {
namespace ref16 {

// Round an f32 VALUE to f16. The asm barrier makes the f32 rounding of the expression that
// produced x happen first: without it the backend fuses h(a * b) and h(a + b) into one
// v_fma_mixlo_f16, which rounds the EXACT product / sum to f16 once, where torch's f16 ops
// round to f32 (opmath) and then to f16. The two differ when the f32 result lands on an f16
// tie (z_vals * scale -> f16 km, x * (1 / max_i), norm * d, gt + eps): measured on the
// PSNR test's first step, 6 of 65,536 dL/dsigma moved between neighbouring samples (an f16
// z one ulp off shifts a mid-point, i.e. swaps two deltas) -- the r04 N = 1,024 PSNR drift
// (tools/r5/composite_ref16_diag.py).
__device__ __forceinline__ float h(float x) {
#pragma clang fp contract(off)
  asm("" : "+v"(x));
  return __half2float(__float2half_rn(x));
}

// f64 -> f16 with ONE rounding (round to odd into f32, then nearest-even into f16: the
// f32 intermediate has 13 more bits than f16, so the double rounding is exact)
__device__ __forceinline__ float h64(double d) {
#pragma clang fp contract(off)
  float f = static_cast<float>(d);
  if (static_cast<double>(f) != d && f != 0.0f && isfinite(f)) {
    uint32_t u = __float_as_uint(f);
    if (fabs(static_cast<double>(f)) > fabs(d)) u -= 1;  // rounded away from zero: truncate
    f = __uint_as_float(u | 1u);
  }
  return h(f);
}

// delta_i = diff([0, (z_0 + z_1) / 2, ..., (z_{N-2} + z_{N-1}) / 2, z_{N-1}])_i in f16
// (graphics_utils.py:31-35), z_vals (f32) * scale -> f16 first (graphics_utils.py:28); from
// the raw f32 z values at i - 1, i, i + 1 (zm / zp unused at the ends)
__device__ __forceinline__ float delta_z(float zm, float z0, float zp, float zs, int i, int N) {
#pragma clang fp contract(off)
  const float zi = h(z0 * zs);
  const float lo = i == 0 ? h(zi * 0.0f) : h(h(h(zm * zs) + zi) * 0.5f);
  const float hi = i == N - 1 ? zi : h(h(zi + h(zp * zs)) * 0.5f);
  return h(hi - lo);
}

// A wavefront is the whole workgroup here: LDS written by one lane and read by another
// needs only program order (LDS executes a wave's instructions in issue order) and a
// compiler barrier. __syncthreads() would also wait for every global load and store in
// flight (its workgroup-scope release), which is what kept these kernels latency-bound.
__device__ __forceinline__ void wave_sync() {
#pragma clang fp contract(off)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct Sample {
  float delta, e, alpha, q2;  // q2 = 1 - alpha + 1e-10 (= om = 1 - alpha in f16)
};

__device__ __forceinline__ Sample from_e(float e, float dl) {
#pragma clang fp contract(off)
  Sample s;
  s.delta = dl;
  s.e = e;
  s.alpha = h(1.0f - s.e);                            // 1 - exp
  s.q2 = h(h(1.0f - s.alpha) + 1e-10f);               // 1 - alpha + 1e-10 (:45)
  return s;
}

__device__ __forceinline__ Sample sample(float sig, float dl) {
#pragma clang fp contract(off)
  const float x = h(-sig * dl);                       // -sigma * delta   (:38)
  return from_e(h64(exp(static_cast<double>(x))), dl);  // exp
}

// f32 x f16 and f32 + f16 with one rounding, as the f32 ops on the converted f16 value:
// fma(a, q, +0) = round(a * q) (a * q >= 0 here, so no -0 case) and fma(x, 1, acc) =
// round(acc + x); one v_fma_mix_f32 each instead of a conversion and the op -- the serial
// scans are most of these kernels' VALU issue
__device__ __forceinline__ float mul_h(float a, _Float16 q) {
#pragma clang fp contract(off)
  return __builtin_fmaf(a, static_cast<float>(q), 0.0f);
}
__device__ __forceinline__ float add_h(float acc, _Float16 x) {
#pragma clang fp contract(off)
  return __builtin_fmaf(static_cast<float>(x), 1.0f, acc);
}

}  // namespace ref16
}  // namespace anr
