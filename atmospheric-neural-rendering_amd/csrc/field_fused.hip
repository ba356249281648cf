// K6+K7 fused: the whole per-sample Instant-NGP radiance field after the hash encoding,
// forward and backward, in one kernel each (f16 MFMA, f32 accumulation).
//
//   pos_out = pos_mlp(enc)                       32 -> W -> 16     (instant_ngp.py:163-164)
//   sigma   = relu(pos_out[:, 0])                                  (:178,184)
//   x_dir   = [SH2(dir) | pos_out[:, 1:16] | 1.0 ...]              (:165-169)
//   color   = relu(dir_mlp(x_dir))               32 -> W (x NHD) -> 16  (:170-171,183)
//
// multi_band_extinction (S = 2..4 density outputs, :46-48): sigma = relu(pos_out[:, :S]),
// x_dir = [SH2(dir) | pos_out[:, S:16] | 1.0 ...] with 20 - S inputs. S is a compile-time
// parameter of the kernels (S = 20 - dir.n_input); the S = 1 instantiations are the code
// they were before it existed.
//
// Layers are evaluated in transposed form on v_mfma_f32_16x16x32_f16, out^T = W · in^T,
// with 16 samples as the MFMA's N dimension. The C tile of one layer (lane = sample
// l&15, units 4(l>>4)+i of each 16-unit block) is, after ReLU and f16 conversion, the B
// operand of the next layer once that layer's weight columns are permuted the same way
// (perm32 below) — so no activation of the forward chain, and no gradient of the
// backward dAct chain, goes through LDS. The packed weight buffer (anr_ingp_field_pack)
// stores every weight matrix directly in MFMA A-fragment order, lane-linear, with those
// permutations (and the dir-input column order) applied.
//
// Backward: per 32-sample tile the forward is recomputed; each layer's input and output
// gradient tiles are written to LDS once, row-major, and read back transposed with
// ds_read_b64_tr_b16 as the operands of dW += G^T · X (contraction over the 32 samples),
// which accumulates in registers across all tiles of a wavefront and is flushed with
// one f32 atomic per element at the end. Gradients are scaled in f16 by one power of two
// per wavefront (pre-pass over |dL/dcolor| and |dL/dsigma|) and unscaled in f32.
// dL/dpos_out never leaves the registers; the kernel writes only dL/denc (f32).

#include <type_traits>

#include "anr_common.h"
#include "composite_ops.h"
#include "hash_levels.h"
#include "ref16_ops.h"

// Profiling ablations (tools/field_ablate.sh); 0 in every product build. Bits:
// 1 no dW MFMAs, 2 no layer-input stores, 4 no gradient-tile stores, 8 no mask reads.
#ifndef FIELD_EXP
#define FIELD_EXP 0
#endif
// Stage barrier of the backward: which instruction classes may be scheduled across the
// point where a stage's LDS reads have been issued (sched_barrier mask: 0x1 ALU, 0x2
// VALU, 0x4 SALU, 0x8 MFMA; memory instructions never cross).
#ifndef FIELD_STAGE_MASK
#define FIELD_STAGE_MASK 0
#endif

namespace anr {
namespace field {

#ifdef FIELD_STAMP
// per-stage cycle totals of wavefront 0 of the backward (s_memtime), debug builds only
__device__ unsigned long long g_stamp[16];
#define STAMP(k)                                                             \
  do {                                                                       \
    __builtin_amdgcn_sched_barrier(0);                                       \
    unsigned long long t_;                                                   \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_));        \
    __builtin_amdgcn_sched_barrier(0);                                       \
    if (stamp_on) { st_acc[k] += t_ - st_last; }                             \
    st_last = t_;                                                            \
  } while (0)
#else
#define STAMP(k) do {} while (0)
#endif

// 16-bit operand carriers. With BF = false they hold f16 values; with BF = true
// (BASELINE configs[4]: bf16 MFMA MLP over the f16 hash features) the same vectors carry
// bf16 bit patterns: only the MFMA opcodes, the f32 -> 16-bit conversions, the ReLU and
// the constants differ, everything in between (LDS tiles, transposed reads, ReLU masks
// on the bits) is type-blind.
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef __bf16 b4 __attribute__((ext_vector_type(4)));
typedef __bf16 b8 __attribute__((ext_vector_type(8)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef short s4v __attribute__((vector_size(8)));
typedef short s4e __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s4v lds_s4v;

template <bool BF>
__device__ __forceinline__ f4 mma32(h8 a, h8 b, f4 c) {
  if constexpr (BF)
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(b8, a),
                                                   __builtin_bit_cast(b8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}
// dW accumulation: the accumulator lives in AGPRs for the whole kernel (the rest of the
// kernel's MFMAs write VGPRs). The compiler does not see these as MFMAs, so every VALU
// access to an accumulator goes through agpr_fence() + agpr_pin() first (result-latency
// wait states); volatile keeps them in program order with the fence.
template <bool BF>
__device__ __forceinline__ void mma32_acc(f4& acc, h8 a, h8 b) {
  if constexpr ((FIELD_EXP & 1) != 0) return;
  if constexpr (BF)
    asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(b));
  else
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(b));
}
// the same with operands fresh from VALU (the register-transposed backward): two wait
// states between a VALU write of an operand and the MFMA reading it (hipcc pads nothing
// inside an asm statement). Volatile, so these stay in program order with agpr_fence():
// the register allocator may copy the accumulators between AGPRs at a loop exit
// (v_accvgpr_mov / _read, measured in the bf16 W=64 instantiation), and such a copy must
// not read an accumulator that an MFMA is still writing — every tile ends with a fence.
template <bool BF>
__device__ __forceinline__ void mma32_acc_v(f4& acc, h8 a, h8 b) {
  if constexpr ((FIELD_EXP & 1) != 0) return;
  if constexpr (BF)
    asm volatile("s_nop 1\n\tv_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(b));
  else
    asm volatile("s_nop 1\n\tv_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(b));
}
__device__ __forceinline__ void agpr_fence() {
  asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7" ::: "memory");
}
// After agpr_fence(): an empty volatile asm that "rewrites" each accumulator, so no read
// or copy of it (v_accvgpr_read / _mov are register-only, which a "memory" clobber does
// not order) can be scheduled above the fence.
template <int N>
__device__ __forceinline__ void agpr_pin(f4 (&acc)[N]) {
  if constexpr ((FIELD_EXP & 1) != 0) return;
#pragma unroll
  for (int i = 0; i < N; ++i) asm volatile("" : "+a"(acc[i]));
}
template <bool BF>
__device__ __forceinline__ f4 mma16(h4 a, h4 b, f4 c) {
  if constexpr (BF)
    return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s4e, a),
                                                     __builtin_bit_cast(s4e, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0);
}
// one f32 -> the 16-bit operand type (round to nearest even), as bits in a _Float16
template <bool BF>
__device__ __forceinline__ _Float16 cvt1(float v) {
  if constexpr (BF)
    return __builtin_bit_cast(_Float16, static_cast<__bf16>(v));
  else
    return static_cast<_Float16>(v);
}

// B-operand slot k' (0..31) of a 32-wide K block -> unit index when the operand is the
// concatenation of two C tiles' lane values (4 from block 2kb, 4 from block 2kb+1).
__host__ __device__ constexpr int perm32(int k) {
  return ((k & 4) ? 16 : 0) + 4 * (k >> 3) + (k & 3);
}
// Dir-MLP input slot k' -> tcnn input column. Lane group g holds pos_out[4g..4g+3] in
// slots 8g..8g+3 (pos_out[p] is column p+3; slot 0 carries a 1.0 padding column instead
// of pos_out[0] = density), and SH2 (g = 0) or more 1.0 padding (g > 0) in 8g+4..8g+7.
// With S density outputs pos_out[p >= S] is column 4 + p - S and the S slots of the
// densities carry 1.0 padding like the 12 of g > 0: for S <= 3 (rows 32 wide) the 12 + S
// padding slots map one to one onto the padding columns 20 - S .. 31; for S = 4 the rows
// are 16 wide, all of them real inputs, and a padding slot has no column (-1: zero weight
// in the fragments, its dW sum dropped).
template <int S>
__host__ __device__ constexpr int dir_col(int k) {
  const int g = k >> 3, j = k & 7;
  if constexpr (S == 1) {
    return j < 4 ? ((g == 0 && j == 0) ? 19 : 4 * g + j + 3) : (g == 0 ? j - 4 : 20 + 4 * (g - 1) + (j - 4));
  } else {
    if (j >= 4) return g == 0 ? j - 4 : (S == 4 ? -1 : 20 + 4 * (g - 1) + (j - 4));
    const int p = 4 * g + j;
    return p < S ? (S == 4 ? -1 : 20 - S + p) : 4 + p - S;
  }
}

template <int W, int NHD, int S = 1>
struct Net {
  static_assert(S >= 1 && S <= 4, "1 to 4 density outputs");
  // width of the first dir layer's parameter rows: n_input_padded of 20 - S inputs
  static constexpr int LD0 = S == 4 ? 16 : 32;
  static_assert(W == 32 || W == 64, "width 32 or 64");
  static_assert(NHD == 1 || NHD == 2, "1 or 2 dir hidden layers");
  static constexpr int NT = W / 16, KB = W / 32;
  static constexpr int F32 = 512, F16 = 256;  // halves per 16x16x32 / 16x16x16 A fragment
  // parameter offsets (tcnn order, each layer row-major [out][in])
  static constexpr int P0 = 0, P1 = 32 * W, NPOS = 32 * W + 16 * W;
  static constexpr int D0 = 0, D1 = LD0 * W, D2 = LD0 * W + (NHD - 1) * W * W;
  static constexpr int NDIR = D2 + 16 * W;
  // packed fragment offsets (halves): forward A = W, backward A = W^T
  static constexpr int oFP0 = 0;                                  // [NT]
  static constexpr int oFP1 = oFP0 + NT * F32;                    // [KB]
  static constexpr int oFD0 = oFP1 + KB * F32;                    // [NT]
  static constexpr int oFD1 = oFD0 + NT * F32;                    // [NT][KB] (NHD == 2)
  static constexpr int oFD2 = oFD1 + (NHD - 1) * NT * KB * F32;   // [KB]
  static constexpr int n_fwd = oFD2 + KB * F32;
  static constexpr int oBD2 = n_fwd;                              // [NT] 16x16x16
  static constexpr int oBD1 = oBD2 + NT * F16;                    // [NT][KB] (NHD == 2)
  static constexpr int oBD0 = oBD1 + (NHD - 1) * NT * KB * F32;   // [KB]
  static constexpr int oBP1 = oBD0 + KB * F32;                    // [NT] 16x16x16
  static constexpr int oBP0 = oBP1 + NT * F16;                    // [2][KB]
  static constexpr int n_packed = oBP0 + 2 * KB * F32;
  static constexpr int n_bwd = n_packed - n_fwd;
  // backward per-wave LDS tiles (32 samples, row-major, +8 halves of padding per row)
  static constexpr int LX = 40, LH = W + 8;
  static constexpr int oXpe = 0;                  // enc            [32][LX]
  static constexpr int oXph = oXpe + 32 * LX;     // pos hidden     [32][LH]
  static constexpr int oXde = oXph + 32 * LH;     // dir input (k') [32][LX]
  static constexpr int oXd0 = oXde + 32 * LX;     // dir hidden 0   [32][LH]
  static constexpr int oXd1 = oXd0 + 32 * LH;     // dir hidden 1   [32][LH] (NHD == 2)
  static constexpr int wave_x = oXd1 + (NHD - 1) * 32 * LH;  // layer-input tiles
  static constexpr int oGa = 0, oGb = 32 * LH, wave_g = 2 * 32 * LH;  // gradient tiles
  static constexpr int wave_lds = wave_x + wave_g;
};

// ---------------------------------------------------------------------------------
// weight packing (f32 master params -> f16 fragments)
// ---------------------------------------------------------------------------------
template <int W, int NHD, bool BF, int S = 1>
__global__ void pack_kernel(const float* __restrict__ pp, const float* __restrict__ pd,
                            _Float16* __restrict__ out) {
  using N = Net<W, NHD, S>;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= N::n_packed) return;
  int f, r, k;
  auto frag32 = [&](int base) {
    const int o = e - base;
    f = o / N::F32;
    const int w = o - f * N::F32, lane = w >> 3;
    r = lane & 15;
    k = 8 * (lane >> 4) + (w & 7);
  };
  auto frag16 = [&](int base) {
    const int o = e - base;
    f = o / N::F16;
    const int w = o - f * N::F16, lane = w >> 2;
    r = lane & 15;
    k = 4 * (lane >> 4) + (w & 3);
  };
  constexpr int W_ = W;
  float v;
  if (e < N::oFP1) {
    frag32(N::oFP0);
    v = pp[N::P0 + (16 * f + r) * 32 + k];
  } else if (e < N::oFD0) {
    frag32(N::oFP1);
    v = pp[N::P1 + r * W_ + 32 * f + perm32(k)];
  } else if (e < N::oFD1) {
    frag32(N::oFD0);
    if constexpr (S == 1) {
      v = pd[N::D0 + (16 * f + r) * 32 + dir_col<1>(k)];
    } else {
      const int c = dir_col<S>(k);
      v = c < 0 ? 0.0f : pd[N::D0 + (16 * f + r) * N::LD0 + c];
    }
  } else if (e < N::oFD2) {
    frag32(N::oFD1);
    const int nt = f / N::KB, kb = f - nt * N::KB;
    v = pd[N::D1 + (16 * nt + r) * W_ + 32 * kb + perm32(k)];
  } else if (e < N::oBD2) {
    frag32(N::oFD2);
    v = pd[N::D2 + r * W_ + 32 * f + perm32(k)];
  } else if (e < N::oBD1) {
    frag16(N::oBD2);
    v = pd[N::D2 + k * W_ + 16 * f + r];
  } else if (e < N::oBD0) {
    frag32(N::oBD1);
    const int kt = f / N::KB, kb = f - kt * N::KB;
    v = pd[N::D1 + (32 * kb + perm32(k)) * W_ + 16 * kt + r];
  } else if (e < N::oBP1) {
    frag32(N::oBD0);
    // row r = pos_out unit r: its column of the dir input (the densities have none)
    if constexpr (S == 1)
      v = r == 0 ? 0.0f : pd[N::D0 + (32 * f + perm32(k)) * 32 + r + 3];
    else
      v = r < S ? 0.0f : pd[N::D0 + (32 * f + perm32(k)) * N::LD0 + 4 + r - S];
  } else if (e < N::oBP0) {
    frag16(N::oBP1);
    v = pp[N::P1 + k * W_ + 16 * f + r];
  } else {
    frag32(N::oBP0);
    const int kt = f / N::KB, kb = f - kt * N::KB;
    v = pp[N::P0 + (32 * kb + perm32(k)) * 32 + 16 * kt + r];
  }
  out[e] = cvt1<BF>(v);
}

struct Args {
  const _Float16* packed;
  const _Float16* enc;
  // row r, levels 4g..4g+3 (one lane's 8 values) at enc + r * enc_stride + g * enc_gstride:
  // row layout (M, >= 32): gstride 8; level-quad planes (anr_hashgrid_fwd_planes,
  // enc_stride = -plane at the ABI): enc_stride 8, gstride = plane
  int64_t enc_stride;
  int64_t enc_gstride;
  const float* dirs;
  uint32_t n_per_ray;
  int64_t M;
  int n_out;
  float* sigma;
  float* color;
  int64_t color_stride;
  const float* d_sigma;
  const float* d_color;
  int64_t d_color_stride;
  float* d_enc;
  int64_t d_enc_stride;
  float* g_pos;
  float* g_dir;
  // occupancy-compacted samples (nullable): row r of enc / d_enc is sample rows[r] of the
  // dense (ray-major) arrays sigma, color, d_sigma, d_color; its ray is rows[r] / n_per_ray
  const int32_t* rows;
  // > 0: reference numerics (tcnn's loss-scaled f16 backward, anr_ingp_field_bwd_ref16):
  // fixed gradient scale, f16 module-boundary gradients; 0: per-wavefront dynamic scale
  float loss_scale;
  // nullable: per 32-row tile, 1 if the tile's incoming gradients had a nonzero value (the
  // tile was walked), 0 if it was skipped (dL/denc rows zero) -- the hash-grid backward
  // then skips those rows without loading them (anr_hashgrid_bwd_tiles)
  uint8_t* tile_nz;
  // anr_ingp_field_bwd_ref16_rows: dL/denc as f16 rows (instead of d_enc) and per 32-row
  // tile a word of row bits, bit i set when row 32 t + i has a nonzero value
  _Float16* d_enc_h;
  uint32_t* row_nz;
  // its pos / list passes (workspace): the tiles with a nonzero dL/dcolor and their count
  int32_t* tile_list;
  uint32_t* tile_count;
  // the reference-numerics f16 interchange with the f16 composite (element strides as
  // above). anr_ingp_field_fwd_h: sigma / colour stored as f16, the f32 value the f32
  // kernel stores rounded to nearest even (instead of sigma / color);
  // anr_ingp_field_bwd_ref16_rows_h: dL/dsigma / dL/dcolor read as f16 (instead of
  // d_sigma / d_color; f16 -> f32 is exact, so the arithmetic after the load is the same)
  _Float16* sigma_h;
  _Float16* color_h;
  const _Float16* d_sigma_h;
  const _Float16* d_color_h;
};

// ROWS is a compile-time choice: a run-time test on a.rows in the prefetch paths put a
// branch join (and with it a wait for the in-flight loads) in front of the MFMAs
template <bool ROWS>
__device__ __forceinline__ int64_t dense_row(const Args& a, int64_t row) {
  if constexpr (ROWS) return static_cast<int64_t>(a.rows[row]);
  return row;
}

__device__ __forceinline__ h8 cat(h4 a, h4 b) {
  return h8{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
}
// f32 accumulators -> 16-bit (round to nearest even, v_cvt_pk_{f16,bf16}_f32)
template <bool BF>
__device__ __forceinline__ h4 to_h4(f4 v) {
  if constexpr (BF)
    return __builtin_bit_cast(h4, __builtin_convertvector(v, b4));
  else
    return __builtin_convertvector(v, h4);
}
// -> ReLU: f16 after the conversion (v_pk_max_f16), bf16 before it (v_max_f32)
template <bool BF>
__device__ __forceinline__ h4 relu_h4(f4 v) {
  if constexpr (BF) {
    return to_h4<true>(__builtin_elementwise_max(v, f4{0.0f, 0.0f, 0.0f, 0.0f}));
  } else {
    const h4 x = __builtin_convertvector(v, h4);
    return __builtin_elementwise_max(x, h4{0, 0, 0, 0});
  }
}
// the f16 hash features as MFMA operands (bf16: f16 -> f32 -> bf16, round to nearest)
template <bool BF>
__device__ __forceinline__ h8 enc_in(h8 e) {
  if constexpr (BF) {
    const h4 lo = {e[0], e[1], e[2], e[3]}, hi = {e[4], e[5], e[6], e[7]};
    const h4 a = to_h4<true>(__builtin_convertvector(lo, f4));
    const h4 b = to_h4<true>(__builtin_convertvector(hi, f4));
    return h8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  } else {
    return e;
  }
}
// ReLU derivative: keep g where the forward activation (>= 0, f16) is nonzero. On the bits:
// v_pk_min_u16(act, 1) is 0 or 1 per half and v_pk_mul_lo_u16 by it keeps or clears g
// (two instructions per pair; written as asm because the compiler expands it to compares
// and selects). The result feeds MFMAs, and hipcc pads nothing for a VALU write inside an
// asm statement: the two wait states a VALU-written MFMA operand needs end the string.
// mask_bits takes g in the 16-bit operand type, mask_h4 converts it first.
__device__ __forceinline__ h4 mask_bits(h4 g, h4 act) {
  typedef uint32_t u2 __attribute__((ext_vector_type(2)));
  const u2 gb = __builtin_bit_cast(u2, g), ab = __builtin_bit_cast(u2, act);
  uint32_t m0, m1;
  asm("v_pk_min_u16 %0, %2, 1 op_sel_hi:[1,0]\n\t"
      "v_pk_min_u16 %1, %3, 1 op_sel_hi:[1,0]\n\t"
      "v_pk_mul_lo_u16 %0, %4, %0\n\t"
      "v_pk_mul_lo_u16 %1, %5, %1\n\t"
      "s_nop 1"
      : "=&v"(m0), "=&v"(m1)
      : "v"(ab.x), "v"(ab.y), "v"(gb.x), "v"(gb.y));
  return __builtin_bit_cast(h4, u2{m0, m1});
}
template <bool BF>
__device__ __forceinline__ h4 mask_h4(f4 g, h4 act) {
  return mask_bits(to_h4<BF>(g), act);
}
// Rank-1 pieces of the pos pass (f16). d2 holds two f16 scalars, HALF picks one.
// w * d: one f16 multiply per value (v_pk_mul_f16 with the scalar's half broadcast by
// op_sel), denormals kept, the exact product rounded once.
template <int HALF>
__device__ __forceinline__ h4 scale_h4(h4 w, uint32_t d2) {
  typedef uint32_t u2 __attribute__((ext_vector_type(2)));
  const u2 wb = __builtin_bit_cast(u2, w);
  uint32_t p0, p1;
  if constexpr (HALF == 0) {
    asm("v_pk_mul_f16 %0, %1, %2 op_sel:[0,0] op_sel_hi:[1,0]" : "=v"(p0) : "v"(wb.x), "v"(d2));
    asm("v_pk_mul_f16 %0, %1, %2 op_sel:[0,0] op_sel_hi:[1,0]" : "=v"(p1) : "v"(wb.y), "v"(d2));
  } else {
    asm("v_pk_mul_f16 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1]" : "=v"(p0) : "v"(wb.x), "v"(d2));
    asm("v_pk_mul_f16 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1]" : "=v"(p1) : "v"(wb.y), "v"(d2));
  }
  return __builtin_bit_cast(h4, u2{p0, p1});
}
// acc[i] += x[i] * d in f32 (v_fma_mix_f32 reads the f16 halves as they are: the product is
// exact, the sum rounded once)
template <int HALF>
__device__ __forceinline__ void fma_h4(float (&acc)[4], h4 x, uint32_t d2) {
  typedef uint32_t u2 __attribute__((ext_vector_type(2)));
  const u2 xb = __builtin_bit_cast(u2, x);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if constexpr (HALF == 0) {
      asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[0,0,0] op_sel_hi:[1,1,0]" : "+v"(acc[2 * j]) : "v"(xb[j]), "v"(d2));
      asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,1,0]" : "+v"(acc[2 * j + 1]) : "v"(xb[j]), "v"(d2));
    } else {
      asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[0,1,0] op_sel_hi:[1,1,0]" : "+v"(acc[2 * j]) : "v"(xb[j]), "v"(d2));
      asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[1,1,0]" : "+v"(acc[2 * j + 1]) : "v"(xb[j]), "v"(d2));
    }
  }
}

// Reference numerics: splitting the subnormal part off the gradient operand of the dX MFMAs
// (v_mfma_f32_16x16x32_f16 sums deeply subnormal products inexactly) was measured and
// reverted (+0.4 ms): profiles/r05_mfma_precision.log, DESIGN section 11, item 3.

// Global inputs of one 16-sample half-tile for this lane, loaded a tile ahead.
struct Rows {
  h8 xe;          // enc[row][8g .. 8g+7]
  float dx, dy, dz;  // direction of the row's ray, remapped 2d-1 (g == 0 lanes)
  f4 dc;          // dL/dcolor[row][4g .. 4g+3] (backward)
  float ds;       // dL/dsigma[row] (backward, g == 0 lanes)
};

template <bool ROWS, bool HG = false, int S = 1>
__device__ __forceinline__ void load_rows(const Args& a, int64_t row, int g, bool bwd, Rows& in) {
  in.xe = h8{};
  in.dx = in.dy = in.dz = 0.0f;
  in.dc = f4{0.0f, 0.0f, 0.0f, 0.0f};
  in.ds = 0.0f;
  if (row >= a.M) return;
  in.xe = *reinterpret_cast<const h8*>(a.enc + row * a.enc_stride + g * a.enc_gstride);
  const int64_t drow = dense_row<ROWS>(a, row);
  if (g == 0) {
    const uint32_t ray = static_cast<uint32_t>(drow) / a.n_per_ray;
    const float* d = a.dirs + static_cast<int64_t>(ray) * 3;
    in.dx = d[0] * 2.0f - 1.0f;
    in.dy = d[1] * 2.0f - 1.0f;
    in.dz = d[2] * 2.0f - 1.0f;
    if constexpr (S > 1) {
      static_assert(!HG, "S > 1: f32 gradients");  // load_dsig() loads the S values
    } else if constexpr (HG) {
      if (bwd && a.d_sigma_h) in.ds = static_cast<float>(a.d_sigma_h[drow]);
    } else {
      if (bwd && a.d_sigma) in.ds = a.d_sigma[drow];
    }
  }
  if constexpr (HG) {
    if (bwd) {  // 8 B per row where the f32 form loads 16
      const int c0 = 4 * g;
      const _Float16* dcp = a.d_color_h + drow * a.d_color_stride + c0;
      if (c0 + 3 < a.n_out && (a.d_color_stride & 3) == 0) {
        in.dc = __builtin_convertvector(*reinterpret_cast<const h4*>(dcp), f4);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (c0 + i < a.n_out) in.dc[i] = static_cast<float>(dcp[i]);
      }
    }
  } else if (bwd) {
    const int c0 = 4 * g;
    const float* dcp = a.d_color + drow * a.d_color_stride + c0;
    if (c0 + 3 < a.n_out && (a.d_color_stride & 3) == 0) {
      in.dc = *reinterpret_cast<const f4*>(dcp);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (c0 + i < a.n_out) in.dc[i] = dcp[i];
    }
  }
}

// S > 1: dL/dsigma[row][0 .. S-1] of the dense row (load_rows's in.ds stays 0); unused
// slots, rows past M and a null d_sigma give 0.
template <bool ROWS, int S>
__device__ __forceinline__ f4 load_dsig(const Args& a, int64_t row) {
  f4 v = {0.0f, 0.0f, 0.0f, 0.0f};
  if (row < a.M && a.d_sigma) {
    const int64_t drow = dense_row<ROWS>(a, row);
#pragma unroll
    for (int j = 0; j < S; ++j) v[j] = a.d_sigma[drow * S + j];
  }
  return v;
}

// Input row of the dir MLP for the sample in this lane (B-operand slots 8g..8g+7).
// Branch-free (per-lane selects): a divergent branch here gives the compiler a place to
// merge other g == 0 code into, including uses of the backward's prefetched loads, which
// then wait for those loads at once.
// S density outputs: slots j < S of g == 0 carry 1.0 in place of pos_out[j].
template <bool BF, int S = 1>
__device__ __forceinline__ h8 dir_input(const Rows& in, bool valid, int g, f4 po) {
  const _Float16 one = cvt1<BF>(1.0f);
  const h8 lead = {one, S > 1 ? one : cvt1<BF>(po[1]), S > 2 ? one : cvt1<BF>(po[2]),
                   S > 3 ? one : cvt1<BF>(po[3]),
                   cvt1<BF>(0.28209479177387814f), cvt1<BF>(-0.48860251190291987f * in.dy),
                   cvt1<BF>(0.48860251190291987f * in.dz), cvt1<BF>(-0.48860251190291987f * in.dx)};
  const h8 rest = {cvt1<BF>(po[0]), cvt1<BF>(po[1]), cvt1<BF>(po[2]), cvt1<BF>(po[3]), one, one,
                   one, one};
  typedef uint32_t u4 __attribute__((ext_vector_type(4)));
  const u4 l = __builtin_bit_cast(u4, lead), r = __builtin_bit_cast(u4, rest);
  const bool g0 = g == 0;
  u4 v;
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = valid ? (g0 ? l[i] : r[i]) : 0u;
  return __builtin_bit_cast(h8, v);
}

template <int W, int NHD>
struct FwdWeights {
  using N = Net<W, NHD>;
  h8 p0[N::NT], p1[N::KB], d0[N::NT], d1[NHD == 2 ? N::NT * N::KB : 1], d2[N::KB];
  // dir = false: the pos network's fragments only (tile_forward without the dir network)
  __device__ void load(const _Float16* pk, int lane, bool dir = true) {
    auto ld = [&](int off) { return *reinterpret_cast<const h8*>(pk + off + lane * 8); };
#pragma unroll
    for (int i = 0; i < N::NT; ++i) p0[i] = ld(N::oFP0 + i * N::F32);
#pragma unroll
    for (int i = 0; i < N::KB; ++i) p1[i] = ld(N::oFP1 + i * N::F32);
    if (!dir) return;
#pragma unroll
    for (int i = 0; i < N::NT; ++i) d0[i] = ld(N::oFD0 + i * N::F32);
    if constexpr (NHD == 2) {
#pragma unroll
      for (int i = 0; i < N::NT * N::KB; ++i) d1[i] = ld(N::oFD1 + i * N::F32);
    }
#pragma unroll
    for (int i = 0; i < N::KB; ++i) d2[i] = ld(N::oFD2 + i * N::F32);
  }
  __device__ h8 P0(int i) const { return p0[i]; }
  __device__ h8 P1(int i) const { return p1[i]; }
  __device__ h8 D0(int i) const { return d0[i]; }
  __device__ h8 D1(int i) const { return d1[i]; }
  __device__ h8 D2(int i) const { return d2[i]; }
};

// The same fragments read from a packed copy in LDS (backward kernel).
template <int W, int NHD>
struct LdsWeights {
  using N = Net<W, NHD>;
  const _Float16* base;
  int lane;
  __device__ h8 frag(int off) const { return *reinterpret_cast<const h8*>(base + off + lane * 8); }
  __device__ h8 P0(int i) const { return frag(N::oFP0 + i * N::F32); }
  __device__ h8 P1(int i) const { return frag(N::oFP1 + i * N::F32); }
  __device__ h8 D0(int i) const { return frag(N::oFD0 + i * N::F32); }
  __device__ h8 D1(int i) const { return frag(N::oFD1 + i * N::F32); }
  __device__ h8 D2(int i) const { return frag(N::oFD2 + i * N::F32); }
};

// Forward of NM 16-sample tiles, layer by layer across the tiles (independent MFMAs back
// to back, so no result is consumed right after the instruction that produces it).
template <int W, int NHD>
struct Tile {
  using N = Net<W, NHD>;
  h8 xe, xd;
  h4 hp[N::NT], hd0[N::NT], hd1[NHD == 2 ? N::NT : 1];
  f4 po, col;
};

struct NoSink {
  __device__ void xe(int, h8) const {}
  __device__ void xd(int, h8) const {}
  __device__ void hp(int, int, h4) const {}
  __device__ void hd0(int, int, h4) const {}
  __device__ void hd1(int, int, h4) const {}
};

// sink: receives every layer input as soon as it is computed (the backward writes them
// to LDS there, so they need not stay live in registers)
// dir = false (wave-uniform): the pos network only; col = 0 (the backward of a tile whose
// dL/dcolor is zero in every row needs nothing of the dir network)
template <int W, int NHD, int NM, bool BF, int S, typename WS, typename SK>
__device__ __forceinline__ void tile_forward(const WS& fw, const Rows* in, const bool* valid,
                                             int g, Tile<W, NHD>* t, const SK& sink,
                                             bool dir = true) {
  using N = Net<W, NHD>;
  const f4 z4 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int mt = 0; mt < NM; ++mt) {
    t[mt].xe = enc_in<BF>(in[mt].xe);
    sink.xe(mt, t[mt].xe);
  }
#pragma unroll
  for (int nt = 0; nt < N::NT; ++nt) {
    const h8 w = fw.P0(nt);
#pragma unroll
    for (int mt = 0; mt < NM; ++mt) {
      t[mt].hp[nt] = relu_h4<BF>(mma32<BF>(w, t[mt].xe, z4));
      sink.hp(mt, nt, t[mt].hp[nt]);
    }
  }
#pragma unroll
  for (int mt = 0; mt < NM; ++mt) t[mt].po = z4;
#pragma unroll
  for (int kb = 0; kb < N::KB; ++kb) {
    const h8 w = fw.P1(kb);
#pragma unroll
    for (int mt = 0; mt < NM; ++mt) t[mt].po = mma32<BF>(w, cat(t[mt].hp[2 * kb], t[mt].hp[2 * kb + 1]), t[mt].po);
  }
  if (!dir) {
#pragma unroll
    for (int mt = 0; mt < NM; ++mt) t[mt].col = z4;
    return;
  }
#pragma unroll
  for (int mt = 0; mt < NM; ++mt) {
    t[mt].xd = dir_input<BF, S>(in[mt], valid[mt], g, t[mt].po);
    sink.xd(mt, t[mt].xd);
  }
#pragma unroll
  for (int nt = 0; nt < N::NT; ++nt) {
    const h8 w = fw.D0(nt);
#pragma unroll
    for (int mt = 0; mt < NM; ++mt) {
      t[mt].hd0[nt] = relu_h4<BF>(mma32<BF>(w, t[mt].xd, z4));
      sink.hd0(mt, nt, t[mt].hd0[nt]);
    }
  }
  if constexpr (NHD == 2) {
#pragma unroll
    for (int nt = 0; nt < N::NT; ++nt) {
      f4 acc[NM];
#pragma unroll
      for (int mt = 0; mt < NM; ++mt) acc[mt] = z4;
#pragma unroll
      for (int kb = 0; kb < N::KB; ++kb) {
        const h8 w = fw.D1(nt * N::KB + kb);
#pragma unroll
        for (int mt = 0; mt < NM; ++mt)
          acc[mt] = mma32<BF>(w, cat(t[mt].hd0[2 * kb], t[mt].hd0[2 * kb + 1]), acc[mt]);
      }
#pragma unroll
      for (int mt = 0; mt < NM; ++mt) {
        t[mt].hd1[nt] = relu_h4<BF>(acc[mt]);
        sink.hd1(mt, nt, t[mt].hd1[nt]);
      }
    }
  }
#pragma unroll
  for (int mt = 0; mt < NM; ++mt) t[mt].col = z4;
#pragma unroll
  for (int kb = 0; kb < N::KB; ++kb) {
    const h8 w = fw.D2(kb);
#pragma unroll
    for (int mt = 0; mt < NM; ++mt) {
      const h4* last = NHD == 2 ? t[mt].hd1 : t[mt].hd0;
      t[mt].col = mma32<BF>(w, cat(last[2 * kb], last[2 * kb + 1]), t[mt].col);
    }
  }
}

// Raw inputs of one 16-sample tile of the forward, prefetched a tile ahead for tiles with
// all rows in range: every lane loads its row's encoding slice and its ray's direction
// (the four lane groups read the same direction: one cache line), nothing is computed on
// them until the next iteration, so no wait for these loads is placed in front of the
// current tile's MFMAs.
struct FwdRaw {
  h8 xe;
  float d0, d1, d2;
};

template <bool ROWS>
__device__ __forceinline__ void load_fwd_raw(const Args& a, int64_t row, int g, FwdRaw& r) {
  r.xe = *reinterpret_cast<const h8*>(a.enc + row * a.enc_stride + g * a.enc_gstride);
  const uint32_t ray = static_cast<uint32_t>(dense_row<ROWS>(a, row)) / a.n_per_ray;
  const float* d = a.dirs + static_cast<int64_t>(ray) * 3;
  r.d0 = d[0];
  r.d1 = d[1];
  r.d2 = d[2];
}

__device__ __forceinline__ void fwd_raw_to_rows(const FwdRaw& r, Rows& in) {
  in.xe = r.xe;
  in.dx = r.d0 * 2.0f - 1.0f;
  in.dy = r.d1 * 2.0f - 1.0f;
  in.dz = r.d2 * 2.0f - 1.0f;
  in.dc = f4{0.0f, 0.0f, 0.0f, 0.0f};
  in.ds = 0.0f;
}

// Uniform-tile forward (UT): dense rows, n_per_ray a multiple of 16, 4 colour outputs,
// 16-byte aligned colour rows, byte offsets below 2^31 — the bench and training shape.
// A 16-row tile is then one ray's samples, so its direction is one scalar load (scalar
// cache and lgkmcnt, not the vector-memory queue), and the outputs go out as raw buffer
// stores, one sigma and one 4-wide colour store per lane with no branch (lanes with
// nothing to write get an out-of-range offset, which the hardware drops). Every tile then
// issues the same vector-memory instructions (one input load, two stores), so the wait
// for the next tile's prefetched encodings is vmcnt(2) and leaves this tile's stores in
// flight. In the general form the per-lane guarded stores and the branch-sunk direction
// remap made the compiler wait with vmcnt(0) twice per tile: one store round trip and
// one prefetch round trip per tile.
typedef uint32_t u4v __attribute__((vector_size(16)));
typedef uint32_t u2v __attribute__((vector_size(8)));
typedef uint32_t u3v __attribute__((ext_vector_type(3)));
typedef __attribute__((address_space(4))) const float const_f32;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t out_rsrc(const void* p, int64_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, static_cast<int>(bytes),
                                           0x00020000);
}

// Four waves per SIMD: at the compiler's free choice the W = 64 forward took 136 VGPRs
// (3 waves); capped at 128 it fits in 126 without spills, and the fourth wave hides more
// of the per-tile prefetch latency (field fwd 0.204 -> 0.201 ms, step -0.02 ms;
// profiles/r03_field_fwd_occ.log). The grid is sized from the same occupancy query.
//
// HO (anr_ingp_field_fwd_h): the same values stored as f16 -- a.sigma_h / a.color_h, each
// the f32 value of the f32 form rounded to nearest even after its max(., 0). The
// uniform-tile form keeps its shape: one 2-byte sigma and one 8-byte colour buffer store
// per lane and tile, and the same two dropped stores ahead of the loop.
//
// S > 1 (multi-band extinction, f32 outputs, dense rows): sigma is (M, S) row-major and the
// g == 0 lane stores its row's S values relu(pos_out[0 .. S-1]) -- its own four accumulator
// registers -- as one store (8 / 12 / 16 bytes).
typedef float f2 __attribute__((ext_vector_type(2)));
struct f3s {
  float x, y, z;
};
template <int S>
__device__ __forceinline__ void store_sigma(float* p, const f4& po) {
  if constexpr (S == 1) {
    p[0] = fmaxf(po[0], 0.0f);
  } else if constexpr (S == 2) {
    *reinterpret_cast<f2*>(p) = f2{fmaxf(po[0], 0.0f), fmaxf(po[1], 0.0f)};
  } else if constexpr (S == 3) {
    *reinterpret_cast<f3s*>(p) = f3s{fmaxf(po[0], 0.0f), fmaxf(po[1], 0.0f), fmaxf(po[2], 0.0f)};
  } else {
    *reinterpret_cast<f4*>(p) =
        f4{fmaxf(po[0], 0.0f), fmaxf(po[1], 0.0f), fmaxf(po[2], 0.0f), fmaxf(po[3], 0.0f)};
  }
}
template <int W, int NHD, bool ROWS, bool BF, bool UT, bool HO = false, int S = 1>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) fwd_kernel(Args a) {
  static_assert(!(UT && ROWS), "the uniform-tile form needs dense rows");
  static_assert(!(HO && ROWS), "f16 outputs: dense rows only");
  static_assert(S == 1 || !(HO || ROWS), "S > 1: f32 outputs, dense rows");
  const int lane = threadIdx.x & 63, g = lane >> 4, li = lane & 15;
  // wave index through readfirstlane: the tile loop then runs on scalar registers
  const int waves = blockDim.x >> 6, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  FwdWeights<W, NHD> fw;
  fw.load(a.packed, lane);
  const int64_t n_tiles = (a.M + 15) / 16;
  const int64_t n_full = a.M / 16;  // tiles with all 16 rows in range
  const int64_t tstride = static_cast<int64_t>(gridDim.x) * waves;
  int64_t tile = static_cast<int64_t>(blockIdx.x) * waves + wave;
  auto store = [&](const Tile<W, NHD>& t, int64_t row) {
    if (row < a.M) {
      const int64_t drow = dense_row<ROWS>(a, row);
      const int c0 = 4 * g;
      if constexpr (HO) {
        if (g == 0) a.sigma_h[drow] = static_cast<_Float16>(fmaxf(t.po[0], 0.0f));
        _Float16* cp = a.color_h + drow * a.color_stride + c0;
        if (c0 + 3 < a.n_out && (a.color_stride & 3) == 0) {
          f4 v;
#pragma unroll
          for (int i = 0; i < 4; ++i) v[i] = fmaxf(t.col[i], 0.0f);
          *reinterpret_cast<h4*>(cp) = to_h4<false>(v);
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (c0 + i < a.n_out) cp[i] = static_cast<_Float16>(fmaxf(t.col[i], 0.0f));
        }
        return;
      }
      if constexpr (S == 1) {
        if (g == 0) a.sigma[drow] = fmaxf(t.po[0], 0.0f);
      } else {
        if (g == 0) store_sigma<S>(a.sigma + drow * S, t.po);
      }
      if (c0 + 3 < a.n_out && (a.color_stride & 3) == 0) {
        f4 v;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = fmaxf(t.col[i], 0.0f);
        *reinterpret_cast<f4*>(a.color + drow * a.color_stride + c0) = v;
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (c0 + i < a.n_out) a.color[drow * a.color_stride + c0 + i] = fmaxf(t.col[i], 0.0f);
      }
    }
  };
  auto body = [&](const Rows& cur, int64_t row) {
    Tile<W, NHD> t;
    const bool valid = row < a.M;
    tile_forward<W, NHD, 1, BF, S>(fw, &cur, &valid, g, &t, NoSink{});
    store(t, row);
  };
  if constexpr (UT) {
    constexpr uint32_t ES = HO ? 2u : 4u;  // bytes per output element
    const __amdgpu_buffer_rsrc_t rsig =
        HO ? out_rsrc(a.sigma_h, a.M * ES) : out_rsrc(a.sigma, a.M * ES * S);
    const __amdgpu_buffer_rsrc_t rcol = HO ? out_rsrc(a.color_h, a.M * a.color_stride * ES)
                                           : out_rsrc(a.color, a.M * a.color_stride * ES);
    const uint32_t cs_bytes = static_cast<uint32_t>(a.color_stride) * ES;
    auto enc_ptr = [&](int64_t t) {
      return reinterpret_cast<const h8*>(a.enc + (t * 16 + li) * a.enc_stride + g * a.enc_gstride);
    };
    h8 nxe;
    if (tile < n_full) {
      nxe = *enc_ptr(tile);
      // two dropped stores: the loop is entered with the vector-memory queue of its back
      // edge (an input load, then a tile's two stores)
      if constexpr (HO) {
        __builtin_amdgcn_raw_buffer_store_b16(uint16_t{0}, rsig, 0x80000000u, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b64(u2v{0u, 0u}, rcol, 0x80000000u, 0, 0);
      } else {
        __builtin_amdgcn_raw_buffer_store_b32(0u, rsig, 0x80000000u, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b128(u4v{0u, 0u, 0u, 0u}, rcol, 0x80000000u, 0, 0);
      }
    }
    for (; tile < n_full; tile += tstride) {
      Rows cur;
      cur.xe = nxe;
      // wave-uniform ray and direction; readfirstlane (convergent) also keeps the loads from
      // being sunk into dir_input's g == 0 branch as vector loads
      const uint32_t ray =
          __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(tile * 16) / a.n_per_ray);
      const const_f32* d = (const_f32*)(a.dirs + static_cast<int64_t>(ray) * 3);
      auto sdir = [&](int k) {
        return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, d[k])));
      };
      cur.dx = sdir(0) * 2.0f - 1.0f;
      cur.dy = sdir(1) * 2.0f - 1.0f;
      cur.dz = sdir(2) * 2.0f - 1.0f;
      cur.dc = f4{0.0f, 0.0f, 0.0f, 0.0f};
      cur.ds = 0.0f;
      const int64_t tn = tile + tstride < n_full ? tile + tstride : tile;
      nxe = *enc_ptr(tn);
      Tile<W, NHD> t;
      const bool valid = true;
      tile_forward<W, NHD, 1, BF, S>(fw, &cur, &valid, g, &t, NoSink{});
      const uint32_t row = static_cast<uint32_t>(tile * 16 + li);
      const uint32_t so = g == 0 ? row * (ES * S) : 0x80000000u;
      const uint32_t co = g == 0 ? row * cs_bytes : 0x80000000u;
      if constexpr (HO) {
        const _Float16 sh = static_cast<_Float16>(fmaxf(t.po[0], 0.0f));
        __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(uint16_t, sh), rsig, so, 0, 0);
        const f4 cv = {fmaxf(t.col[0], 0.0f), fmaxf(t.col[1], 0.0f), fmaxf(t.col[2], 0.0f),
                       fmaxf(t.col[3], 0.0f)};
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2v, to_h4<false>(cv)), rcol, co,
                                              0, 0);
        continue;
      }
      if constexpr (S == 1) {
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(fmaxf(t.po[0], 0.0f)), rsig, so, 0, 0);
      } else {  // the row's S densities, one store
        const uint32_t s0 = __float_as_uint(fmaxf(t.po[0], 0.0f));
        const uint32_t s1 = __float_as_uint(fmaxf(t.po[1], 0.0f));
        const uint32_t s2 = __float_as_uint(fmaxf(t.po[2], 0.0f));
        const uint32_t s3 = __float_as_uint(fmaxf(t.po[3], 0.0f));
        if constexpr (S == 2)
          __builtin_amdgcn_raw_buffer_store_b64(u2v{s0, s1}, rsig, so, 0, 0);
        else if constexpr (S == 3)
          __builtin_amdgcn_raw_buffer_store_b96(u3v{s0, s1, s2}, rsig, so, 0, 0);
        else
          __builtin_amdgcn_raw_buffer_store_b128(u4v{s0, s1, s2, s3}, rsig, so, 0, 0);
      }
      const u4v v = {__float_as_uint(fmaxf(t.col[0], 0.0f)), __float_as_uint(fmaxf(t.col[1], 0.0f)),
                     __float_as_uint(fmaxf(t.col[2], 0.0f)), __float_as_uint(fmaxf(t.col[3], 0.0f))};
      __builtin_amdgcn_raw_buffer_store_b128(v, rcol, co, 0, 0);
    }
  } else {
    // full tiles: the next tile's inputs are in flight while this one computes (the
    // prefetch index is clamped, so the loop body has no branch around the loads)
    FwdRaw nraw;
    if (tile < n_full) load_fwd_raw<ROWS>(a, tile * 16 + li, g, nraw);
    for (; tile < n_full; tile += tstride) {
      Rows cur;
      fwd_raw_to_rows(nraw, cur);
      const int64_t tn = tile + tstride < n_full ? tile + tstride : tile;
      load_fwd_raw<ROWS>(a, tn * 16 + li, g, nraw);
      body(cur, tile * 16 + li);
    }
  }
  for (; tile < n_tiles; tile += tstride) {  // the last, partial tile
    Rows cur;
    load_rows<ROWS>(a, tile * 16 + li, g, false, cur);
    body(cur, tile * 16 + li);
  }
}

// ---------------------------------------------------------------------------------
// Hash-grid forward + field forward in one kernel (r06). A wavefront
// takes 64 consecutive samples (one ray segment: n_per_ray is a multiple of 64) at a time:
//  1. hash phase, one lane per sample: the 16 levels as four level quads (plane_quad, the
//     arithmetic of anr_hashgrid_fwd_planes), each stored to its plane for the backward
//     and to the wavefront's LDS stage;
//  2. field phase, the four 16-sample tiles of the uniform-tile forward: lane group g reads
//     quad g of its sample from the stage -- exactly the B fragment of the first layer --
//     and tile_forward runs on weight fragments read from LDS.
// The planes are written once and never re-read by the forward (the separate field
// forward read all 64 B per sample back from HBM), and one wavefront's gathers overlap
// other wavefronts' MFMA tiles on the same CU. Bit-identical to anr_hashgrid_fwd_planes
// followed by anr_ingp_field_fwd (same per-level arithmetic, same MFMA sequence).
struct HashArgs {
  GridLevels G;
  const float* x;
  uint32_t x_bytes;
  const __half* table;
  uint32_t table_bytes;
  _Float16* planes;
  uint32_t plane_bytes;  // bytes from one level-quad plane to the next
  uint32_t out_bytes;    // bytes of the plane buffer (range check of the stores)
};

template <int W, int NHD, bool BF, int WAVES, int OCC>
__global__ void __launch_bounds__(64 * WAVES) __attribute__((amdgpu_waves_per_eu(OCC)))
hf_fwd_kernel(Args a, HashArgs h) {
  using N = Net<W, NHD>;
  typedef uint32_t u4q __attribute__((vector_size(16)));
  __shared__ __attribute__((aligned(16))) _Float16 wsm[N::n_fwd];
  // per wavefront: quad q of lane l's sample at stage[wave][q][l]
  __shared__ __attribute__((aligned(16))) u4q stage[WAVES][4][64];
  const int lane = threadIdx.x & 63, g = lane >> 4, li = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int e = threadIdx.x * 8; e < N::n_fwd; e += 64 * WAVES * 8)
    *reinterpret_cast<h8*>(wsm + e) = *reinterpret_cast<const h8*>(a.packed + e);
  __syncthreads();
  const __amdgpu_buffer_rsrc_t rx = wave_rsrc(h.x, h.x_bytes);
  const __amdgpu_buffer_rsrc_t rt = wave_rsrc(h.table, h.table_bytes);
  const __amdgpu_buffer_rsrc_t ro = wave_rsrc(h.planes, h.out_bytes);
  const __amdgpu_buffer_rsrc_t rsig = out_rsrc(a.sigma, a.M * 4);
  const __amdgpu_buffer_rsrc_t rcol = out_rsrc(a.color, a.M * a.color_stride * 4);
  const uint32_t cs_bytes = static_cast<uint32_t>(a.color_stride) * 4u;
  const int64_t n_super = (a.M + 63) / 64;
  const int64_t sstride = static_cast<int64_t>(gridDim.x) * WAVES;
  for (int64_t st = static_cast<int64_t>(blockIdx.x) * WAVES + wave; st < n_super; st += sstride) {
    const uint32_t m = static_cast<uint32_t>(st * 64) + lane;
    // ---- hash phase: lane = sample (coordinates past x's end read as 0, stores past M
    // dropped by the range check)
    float xv[3];
    load_row<3>(rx, m * 12u, xv);
    const uint32_t orow = m < a.M ? m * 16u : 0x80000000u;
#pragma unroll 1
    for (int q = 0; q < 4; ++q) {
      uint32_t p[4];
      plane_quad<3, __half, false>(h.G, 16, q, xv, rt, p);
      const u4q v = {p[0], p[1], p[2], p[3]};
      __builtin_amdgcn_raw_buffer_store_b128(v, ro, static_cast<uint32_t>(q) * h.plane_bytes + orow,
                                             0, 0);
      stage[wave][q][lane] = v;
    }
    // one wavefront's LDS accesses complete in order: the stage is read back below without
    // a barrier (the fence keeps the compiler from hoisting the reads above the writes)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // ---- field phase: the segment is one ray (n_per_ray % 64 == 0): scalar direction
    const uint32_t ray =
        __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(st * 64) / a.n_per_ray);
    const const_f32* d = (const_f32*)(a.dirs + static_cast<int64_t>(ray) * 3);
    auto sdir = [&](int k) {
      return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, d[k])));
    };
    Rows cur;
    cur.dx = sdir(0) * 2.0f - 1.0f;
    cur.dy = sdir(1) * 2.0f - 1.0f;
    cur.dz = sdir(2) * 2.0f - 1.0f;
    cur.dc = f4{0.0f, 0.0f, 0.0f, 0.0f};
    cur.ds = 0.0f;
#pragma unroll 1
    for (int t = 0; t < 4; ++t) {
      cur.xe = __builtin_bit_cast(h8, stage[wave][g][16 * t + li]);
      const uint32_t row = static_cast<uint32_t>(st * 64) + 16 * t + li;
      const bool valid = row < a.M;
      // per-tile opaque fragment base: the weight fragments are read from LDS at their
      // MFMAs instead of being hoisted out of the loops into 80 registers
      int zoff = 0;
      asm volatile("" : "+v"(zoff));
      const LdsWeights<W, NHD> fw{wsm + zoff, lane};
      Tile<W, NHD> tt;
      tile_forward<W, NHD, 1, BF, 1>(fw, &cur, &valid, g, &tt, NoSink{});
      const uint32_t so = g == 0 && valid ? row * 4u : 0x80000000u;
      const uint32_t co = g == 0 && valid ? row * cs_bytes : 0x80000000u;
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(fmaxf(tt.po[0], 0.0f)), rsig, so, 0, 0);
      const u4v v = {__float_as_uint(fmaxf(tt.col[0], 0.0f)), __float_as_uint(fmaxf(tt.col[1], 0.0f)),
                     __float_as_uint(fmaxf(tt.col[2], 0.0f)), __float_as_uint(fmaxf(tt.col[3], 0.0f))};
      __builtin_amdgcn_raw_buffer_store_b128(v, rcol, co, 0, 0);
    }
    // the next segment's stage writes stay behind this segment's reads
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
}

// ---------------------------------------------------------------------------------
// Forward-only render (anr_ingp_render): hf_fwd_kernel's hash and field phases with the
// composite behind them, nothing written per sample. One wavefront renders one ray and
// takes its n_per_ray / 64 segments in order:
//  1. hash phase, one lane per sample: plane_quad into the wavefront's LDS stage only;
//  2. field phase: the four 16-sample tiles through tile_forward (the MFMA sequence of
//     fwd_kernel, so sigma and colour are anr_ingp_field_fwd's / _fwd_h's values bit for
//     bit); the g == 0 lanes, which hold a sample's density and 4 colours in the C layout,
//     put them into LDS at the sample's slot;
//  3. composite phase, one lane per sample again, with the carries that cross a segment
//     boundary in registers (RefCarry / BuildCarry).
// REF = true (reference numerics): the arithmetic of ref16::fwd_kernel on the f16-rounded
// sigma and colour. Its f16 cumprod accumulator, f32 product and f32 band sums are serial
// chains in sample order with no other order that rounds the same way, so they run as
// 64-step chains per segment: lane 0 walks the cumprod and the product over the segment's
// q2 in LDS, lanes 0..3 a band sum each over the products h(colour * w). The carries (cp,
// pr in lane 0, the band sums in lanes 0..3) are the accumulators themselves, so the
// chain over all segments is the one fwd_kernel forms: bit-identical maps.
// REF = false (build numerics): composite.hip's per-sample f32 expressions; the
// transmittance is a wave scan inside the segment times the carry of the segments before
// it, the band sums and the surface product accumulate per lane and are reduced across
// the wave once per ray. The order of the f32 sums differs from rb::fwd_kernel's, so this
// form is held to a tolerance against it, not to bits.
struct RenderArgs {
  const float* z;   // (B, n_per_ray) f32, as the sampler wrote it
  float zs;         // z_scale
  const void* cs;   // (B, 4) surface colour, nullable: f16 (REF) or f32
  void* cmap;       // (B, 4) outputs: f16 (REF) or f32; atmo / surf nullable
  void* atmo;
  void* surf;
  int64_t B;
};

constexpr int kRenderPad = 72;  // LDS row of a segment's f16 values (ref16.hip kPad)
struct __attribute__((aligned(16))) RenderRefLds {
  _Float16 q2[kRenderPad];
  _Float16 T[kRenderPad];
  _Float16 t[4][kRenderPad];  // f16(f16(color) * w) per band
};
struct RenderNoLds {};

struct RefCarry {
  _Float16 cp = 1.0f;  // lane 0: the cumprod's f16 accumulator
  float pr = 1.0f;     // lane 0: prod over samples of q2, f32 accumulator
  float acc = 0.0f;    // lane c < 4: band c's sum over samples, f32 accumulator
};

// One segment in reference numerics: sg / col are the f16 values of the sample in this lane
// (sample i = s0 + lane of N), zm / z0 / zp the raw z at i - 1, i, i + 1.
__device__ __forceinline__ void render_seg_ref(RenderRefLds& L, RefCarry& k, float sg,
                                               const float (&col)[4], float zm, float z0,
                                               float zp, float zs, int i, int N, int lane) {
#pragma clang fp contract(off)
  using namespace ::anr::ref16;
  const Sample sm = sample(sg, delta_z(zm, z0, zp, zs, i, N));
  L.q2[lane] = static_cast<_Float16>(sm.q2);
  wave_sync();
  if (lane == 0) {
    for (int l8 = 0; l8 < 64; l8 += 8) {
      const h8 q = *reinterpret_cast<const h8*>(&L.q2[l8]);
      h8 tv;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        tv[j] = k.cp;                  // cumprod(...)[:, :-1]
        k.cp = k.cp * q[j];            // = h(cp * q2)
        k.pr = mul_h(k.pr, q[j]);      // (1 - alpha).prod
      }
      *reinterpret_cast<h8*>(&L.T[l8]) = tv;
    }
  }
  wave_sync();
  const float w = h(sm.alpha * static_cast<float>(L.T[lane]));  // alpha * T
#pragma unroll
  for (int c = 0; c < 4; ++c) L.t[c][lane] = static_cast<_Float16>(h(col[c] * w));
  wave_sync();
  if (lane < 4) {
    for (int l8 = 0; l8 < 64; l8 += 8) {
      const h8 tv = *reinterpret_cast<const h8*>(&L.t[lane][l8]);
#pragma unroll
      for (int j = 0; j < 8; ++j) k.acc = add_h(k.acc, tv[j]);
    }
  }
  wave_sync();
}

// The ray's maps from the carries (ref16::fwd_kernel's epilogue): lane c < 4 writes band c.
__device__ __forceinline__ void render_end_ref(const RenderArgs& r, const RefCarry& k, int64_t b,
                                               int lane) {
#pragma clang fp contract(off)
  using namespace ::anr::ref16;
  const float prr = h(__shfl(k.pr, 0));
  if (lane < 4) {
    const __half* cs = static_cast<const __half*>(r.cs);
    const int64_t o = b * 4 + lane;
    const float atmo = h(k.acc);
    const float surf = cs ? h(prr * h(__half2float(cs[o]))) : 0.0f;
    static_cast<__half*>(r.cmap)[o] = __float2half_rn(cs ? h(atmo + surf) : atmo);
    if (r.atmo) static_cast<__half*>(r.atmo)[o] = __float2half_rn(atmo);
    if (r.surf && cs) static_cast<__half*>(r.surf)[o] = __float2half_rn(surf);
  }
}

struct BuildCarry {
  float T = 1.0f;    // uniform: the transmittance entering the segment
  float pom = 1.0f;  // per lane: product of (1 - alpha) over the lane's samples
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // per lane: sums of colour * w
};

// One segment in build numerics (composite.hip's expressions, rb::deltas' delta).
__device__ __forceinline__ void render_seg_build(BuildCarry& k, float sg, const float (&col)[4],
                                                 float zm, float z0, float zp, float zs, int i,
                                                 int N, int lane) {
#pragma clang fp contract(off)
  const float zi = z0 * zs, zprev = zm * zs, znext = zp * zs;
  const float lo = i == 0 ? zi * 0.0f : (zprev + zi) / 2.0f;
  const float hi = i == N - 1 ? zi : (zi + znext) / 2.0f;
  const float dl = hi - lo;
  const float al = alpha_of(sg * dl);
  const float t = (1.0f - al) + 1e-10f;
  const float Tin = k.T * wave_excl_prod(t, lane);
  const float w = al * Tin;
#pragma unroll
  for (int c = 0; c < 4; ++c) k.acc[c] += col[c] * w;
  k.pom *= 1.0f - al;
  k.T = shfl(Tin * t, 63);
}

__device__ __forceinline__ void render_end_build(const RenderArgs& r, const BuildCarry& k,
                                                 int64_t b, int lane) {
#pragma clang fp contract(off)
  const float stot = wave_prod(k.pom);
  float atmo[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) atmo[c] = wave_sum(k.acc[c]);
  if (lane < 4) {
    const float* cs = static_cast<const float*>(r.cs);
    const int64_t o = b * 4 + lane;
    const float at = lane == 0 ? atmo[0] : lane == 1 ? atmo[1] : lane == 2 ? atmo[2] : atmo[3];
    const float surf = cs ? stot * cs[o] : 0.0f;
    static_cast<float*>(r.cmap)[o] = at + surf;
    if (r.atmo) static_cast<float*>(r.atmo)[o] = at;
    if (r.surf && cs) static_cast<float*>(r.surf)[o] = surf;
  }
}

template <int W, int NHD, bool BF, bool REF, int WAVES, int OCC>
__global__ void __launch_bounds__(64 * WAVES) __attribute__((amdgpu_waves_per_eu(OCC)))
render_kernel(Args a, HashArgs h, RenderArgs r) {
  using N = Net<W, NHD>;
  typedef uint32_t u4q __attribute__((vector_size(16)));
  __shared__ __attribute__((aligned(16))) _Float16 wsm[N::n_fwd];
  // per wavefront: quad q of lane l's sample at stage[wave][q][l]
  __shared__ __attribute__((aligned(16))) u4q stage[WAVES][4][64];
  // per wavefront: the segment's field outputs, sigma at [0][sample], band c at [1 + c][sample]
  __shared__ float outs[WAVES][5][64];
  __shared__ typename std::conditional<REF, RenderRefLds, RenderNoLds>::type scan[WAVES];
  const int lane = threadIdx.x & 63, g = lane >> 4, li = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int e = threadIdx.x * 8; e < N::n_fwd; e += 64 * WAVES * 8)
    *reinterpret_cast<h8*>(wsm + e) = *reinterpret_cast<const h8*>(a.packed + e);
  __syncthreads();  // the only block-wide barrier: the ray loop below is per wavefront
  const __amdgpu_buffer_rsrc_t rx = wave_rsrc(h.x, h.x_bytes);
  const __amdgpu_buffer_rsrc_t rt = wave_rsrc(h.table, h.table_bytes);
  const int n = static_cast<int>(a.n_per_ray);
  const int64_t rstride = static_cast<int64_t>(gridDim.x) * WAVES;
  for (int64_t b = static_cast<int64_t>(blockIdx.x) * WAVES + wave; b < r.B; b += rstride) {
    const const_f32* d = (const_f32*)(a.dirs + b * 3);
    auto sdir = [&](int k) {
      return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, d[k])));
    };
    Rows cur;
    cur.dx = sdir(0) * 2.0f - 1.0f;
    cur.dy = sdir(1) * 2.0f - 1.0f;
    cur.dz = sdir(2) * 2.0f - 1.0f;
    cur.dc = f4{0.0f, 0.0f, 0.0f, 0.0f};
    cur.ds = 0.0f;
    const float* zr = r.z + b * n;
    typename std::conditional<REF, RefCarry, BuildCarry>::type carry;
#pragma unroll 1
    for (int s0 = 0; s0 < n; s0 += 64) {
      const int i = s0 + lane;
      // z of the sample and of its neighbours (across a segment edge: from the row), in
      // flight during the hash and field phases
      const float z0 = zr[i];
      const float zm = i > 0 ? zr[i - 1] : 0.0f;
      const float zp = i < n - 1 ? zr[i + 1] : 0.0f;
      // ---- hash phase: lane = sample (every sample of the ray is in range)
      const uint32_t m = static_cast<uint32_t>(b * n + i);
      float xv[3];
      load_row<3>(rx, m * 12u, xv);
#pragma unroll 1
      for (int q = 0; q < 4; ++q) {
        uint32_t p[4];
        plane_quad<3, __half, false>(h.G, 16, q, xv, rt, p);
        stage[wave][q][lane] = u4q{p[0], p[1], p[2], p[3]};
      }
      ::anr::ref16::wave_sync();
      // ---- field phase
#pragma unroll 1
      for (int t = 0; t < 4; ++t) {
        cur.xe = __builtin_bit_cast(h8, stage[wave][g][16 * t + li]);
        const bool valid = true;
        int zoff = 0;  // opaque fragment base, as hf_fwd_kernel
        asm volatile("" : "+v"(zoff));
        const LdsWeights<W, NHD> fw{wsm + zoff, lane};
        Tile<W, NHD> tt;
        tile_forward<W, NHD, 1, BF, 1>(fw, &cur, &valid, g, &tt, NoSink{});
        if (g == 0) {
          const float sv = fmaxf(tt.po[0], 0.0f);
          const f4 cv = {fmaxf(tt.col[0], 0.0f), fmaxf(tt.col[1], 0.0f), fmaxf(tt.col[2], 0.0f),
                         fmaxf(tt.col[3], 0.0f)};
          if constexpr (REF) {  // anr_ingp_field_fwd_h's roundings
            const h4 ch = to_h4<false>(cv);
            outs[wave][0][16 * t + li] = static_cast<float>(static_cast<_Float16>(sv));
#pragma unroll
            for (int c = 0; c < 4; ++c) outs[wave][1 + c][16 * t + li] = static_cast<float>(ch[c]);
          } else {
            outs[wave][0][16 * t + li] = sv;
#pragma unroll
            for (int c = 0; c < 4; ++c) outs[wave][1 + c][16 * t + li] = cv[c];
          }
        }
      }
      ::anr::ref16::wave_sync();
      // ---- composite phase: lane = sample
      const float sg = outs[wave][0][lane];
      const float col[4] = {outs[wave][1][lane], outs[wave][2][lane], outs[wave][3][lane],
                            outs[wave][4][lane]};
      if constexpr (REF)
        render_seg_ref(scan[wave], carry, sg, col, zm, z0, zp, r.zs, i, n, lane);
      else
        render_seg_build(carry, sg, col, zm, z0, zp, r.zs, i, n, lane);
      // the next segment's stage / outs writes stay behind this segment's reads
      ::anr::ref16::wave_sync();
    }
    if constexpr (REF)
      render_end_ref(r, carry, b, lane);
    else
      render_end_build(r, carry, b, lane);
  }
}

// lane (column c = l&15 of a 16-column block at col0) receives rows 8g..8g+7 of that
// column of a row-major LDS tile: two 4x16 hardware-transposed reads
__device__ __forceinline__ h8 tr_read(const _Float16* base, int ld, int col0, int lane) {
  const int li = lane & 15, g = lane >> 4;
  const _Float16* p0 = base + (8 * g + (li >> 2)) * ld + col0 + 4 * (li & 3);
  const _Float16* p1 = p0 + 4 * ld;
  const s4v v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4v*)(p0));
  const s4v v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4v*)(p1));
  return cat(__builtin_bit_cast(h4, v0), __builtin_bit_cast(h4, v1));
}

// C-layout (sample l&15, units 4g..4g+3) read back from row `mrow` of a row-major tile
__device__ __forceinline__ h4 ld4(const _Float16* base, int ld, int mrow, int col) {
  if constexpr ((FIELD_EXP & 8) != 0) return h4{1, 1, 1, 1};
  return *reinterpret_cast<const h4*>(base + mrow * ld + col);
}

// C-layout (sample l&15, units 4g..4g+3) store into row `mrow` of a row-major tile
__device__ __forceinline__ void st4(_Float16* base, int ld, int mrow, int col, h4 v) {
  *reinterpret_cast<h4*>(base + mrow * ld + col) = v;
}
// gradient-tile store (ablation bit 4)
__device__ __forceinline__ void st4g(_Float16* base, int ld, int mrow, int col, h4 v) {
  if constexpr ((FIELD_EXP & 4) != 0) return;
  *reinterpret_cast<h4*>(base + mrow * ld + col) = v;
}

// Density only: relu(pos_out[:, 0]) of tile_forward's pos MLP, the dir MLP (70 % of the
// field's MFMA work) skipped -- the extract loop (instant_ngp.py:208-247: only the
// extinction is read) and the occupancy grid's density. The same MFMA sequence as the
// full forward's pos half, so sigma is bit-identical to anr_ingp_field_fwd's. Weights in
// registers, one 16-row tile per wavefront step, the next tile's encodings in flight.
template <int W, int NHD, bool BF, int S = 1>
__global__ void __launch_bounds__(256) density_kernel(Args a) {
  using N = Net<W, NHD>;
  const int lane = threadIdx.x & 63, g = lane >> 4, li = lane & 15;
  const int waves = blockDim.x >> 6, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  h8 p0[N::NT], p1[N::KB];
#pragma unroll
  for (int i = 0; i < N::NT; ++i)
    p0[i] = *reinterpret_cast<const h8*>(a.packed + N::oFP0 + i * N::F32 + lane * 8);
#pragma unroll
  for (int i = 0; i < N::KB; ++i)
    p1[i] = *reinterpret_cast<const h8*>(a.packed + N::oFP1 + i * N::F32 + lane * 8);
  const f4 z4 = {0.0f, 0.0f, 0.0f, 0.0f};
  const int64_t n_tiles = (a.M + 15) / 16;
  const int64_t tstride = static_cast<int64_t>(gridDim.x) * waves;
  int64_t tile = static_cast<int64_t>(blockIdx.x) * waves + wave;
  auto load = [&](int64_t t) -> h8 {
    const int64_t row = t * 16 + li;
    if (row < a.M) return *reinterpret_cast<const h8*>(a.enc + row * a.enc_stride + g * a.enc_gstride);
    return h8{};
  };
  h8 nxe = tile < n_tiles ? load(tile) : h8{};
  for (; tile < n_tiles; tile += tstride) {
    const h8 xe = enc_in<BF>(nxe);
    const int64_t tn = tile + tstride;
    if (tn < n_tiles) nxe = load(tn);
    h4 hp[N::NT];
#pragma unroll
    for (int nt = 0; nt < N::NT; ++nt) hp[nt] = relu_h4<BF>(mma32<BF>(p0[nt], xe, z4));
    f4 po = z4;
#pragma unroll
    for (int kb = 0; kb < N::KB; ++kb) po = mma32<BF>(p1[kb], cat(hp[2 * kb], hp[2 * kb + 1]), po);
    const int64_t row = tile * 16 + li;
    if constexpr (S == 1) {
      if (g == 0 && row < a.M) a.sigma[row] = fmaxf(po[0], 0.0f);
    } else {
      if (g == 0 && row < a.M) store_sigma<S>(a.sigma + row * S, po);
    }
  }
}

// The f16 gradient scale's input for a wavefront with tiles [t_begin, t_end):
// absmax_kernel's value (0 for a wavefront without rows).
__device__ __forceinline__ float wave_grad_max(const Args& a, const float* wmax, int64_t w_id,
                                               int64_t t_begin, int64_t t_end) {
  (void)a;
  return t_begin >= t_end ? 0.0f : wmax[w_id];
}

// Rows of the backward's wavefront w: tiles [w*tpw, (w+1)*tpw) of 32 rows. The f16
// gradient scale of a wavefront is set from max(|dL/dcolor|, |dL/dsigma|) over its rows,
// which this kernel computes first (one block per wavefront range, full occupancy).
// S > 1: dL/dsigma is (M, S) and the maximum runs over all S columns.
template <bool ROWS, int S = 1>
__global__ void __launch_bounds__(1024) absmax_kernel(Args a, int64_t rows_per_wave, float* wmax) {
  const int64_t r0 = static_cast<int64_t>(blockIdx.x) * rows_per_wave;
  const int64_t r1 = r0 + rows_per_wave < a.M ? r0 + rows_per_wave : a.M;
  float m = 0.0f;
  if constexpr (S > 1) {
    for (int64_t rr = r0 + threadIdx.x; rr < r1; rr += blockDim.x) {
      const int64_t r = dense_row<ROWS>(a, rr);
      for (int c = 0; c < a.n_out; ++c) m = fmaxf(m, fabsf(a.d_color[r * a.d_color_stride + c]));
      if (a.d_sigma) {
#pragma unroll
        for (int j = 0; j < S; ++j) m = fmaxf(m, fabsf(a.d_sigma[r * S + j]));
      }
    }
  } else
  if (a.n_out == 4 && (a.d_color_stride & 3) == 0) {
    // four rows per thread per iteration, loads issued before any max (one wait each)
    const int64_t step = blockDim.x;
    int64_t rr = r0 + threadIdx.x;
    for (; rr + 3 * step < r1; rr += 4 * step) {
      f4 d[4];
      float sg[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int64_t r = dense_row<ROWS>(a, rr + k * step);
        d[k] = *reinterpret_cast<const f4*>(a.d_color + r * a.d_color_stride);
        sg[k] = a.d_sigma ? a.d_sigma[r] : 0.0f;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k)
        m = fmaxf(m, fmaxf(fmaxf(fmaxf(fabsf(d[k][0]), fabsf(d[k][1])),
                                 fmaxf(fabsf(d[k][2]), fabsf(d[k][3]))), fabsf(sg[k])));
    }
    for (; rr < r1; rr += step) {
      const int64_t r = dense_row<ROWS>(a, rr);
      const f4 d = *reinterpret_cast<const f4*>(a.d_color + r * a.d_color_stride);
      m = fmaxf(m, fmaxf(fmaxf(fabsf(d[0]), fabsf(d[1])), fmaxf(fabsf(d[2]), fabsf(d[3]))));
      if (a.d_sigma) m = fmaxf(m, fabsf(a.d_sigma[r]));
    }
  } else {
    for (int64_t rr = r0 + threadIdx.x; rr < r1; rr += blockDim.x) {
      const int64_t r = dense_row<ROWS>(a, rr);
      for (int c = 0; c < a.n_out; ++c) m = fmaxf(m, fabsf(a.d_color[r * a.d_color_stride + c]));
      if (a.d_sigma) m = fmaxf(m, fabsf(a.d_sigma[r]));
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  __shared__ float part[16];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < static_cast<int>(blockDim.x >> 6); ++i) m = fmaxf(m, part[i]);
    wmax[blockIdx.x] = m;
  }
}

// Raw global inputs of one 16-sample half-tile of a FULL tile in the FAST case (n_out == 4,
// aligned d_color rows, d_sigma present), prefetched a tile ahead. Nothing is computed
// on the loaded values here — any use would make the compiler wait for the load right
// away; raw_to_rows() converts them one tile later. Every lane loads its row's direction,
// d_sigma and d_color (same addresses across the lane groups: no extra traffic).
// HG (f16 gradients, a.d_sigma_h / a.d_color_h): the row's dL/dcolor is one 8-byte load and
// its dL/dsigma a 2-byte load (zero-extended into a 32-bit register), converted to f32 --
// exactly -- by raw_to_rows() like the rest.
// S > 1 (f32 gradients): the row's S values of dL/dsigma in dsb (an empty base at S = 1,
// so that form keeps its members).
template <int S>
struct RawDsig {
  float dsb[S];
};
template <>
struct RawDsig<1> {};
template <bool HG, int S = 1>
struct RawRowsT : RawDsig<S> {
  h8 xe;
  float d0, d1, d2;
  typename std::conditional<HG, uint32_t, float>::type ds;
  typename std::conditional<HG, h4, f4>::type dc;
};

template <bool ROWS, bool HG, int S = 1>
__device__ __forceinline__ void load_raw(const Args& a, int64_t row, int g, RawRowsT<HG, S>& r) {
  r.xe = *reinterpret_cast<const h8*>(a.enc + row * a.enc_stride + g * a.enc_gstride);
  const int64_t drow = dense_row<ROWS>(a, row);
  const uint32_t ray = static_cast<uint32_t>(drow) / a.n_per_ray;
  const float* d = a.dirs + static_cast<int64_t>(ray) * 3;
  r.d0 = d[0];
  r.d1 = d[1];
  r.d2 = d[2];
  if constexpr (HG) {
    r.ds = reinterpret_cast<const uint16_t*>(a.d_sigma_h)[drow];
    r.dc = *reinterpret_cast<const h4*>(a.d_color_h + drow * a.d_color_stride);
  } else if constexpr (S > 1) {
    if constexpr (S == 2) {
      const f2 v = *reinterpret_cast<const f2*>(a.d_sigma + drow * 2);
      r.dsb[0] = v[0];
      r.dsb[1] = v[1];
    } else if constexpr (S == 4) {
      const f4 v = *reinterpret_cast<const f4*>(a.d_sigma + drow * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) r.dsb[j] = v[j];
    } else {
#pragma unroll
      for (int j = 0; j < S; ++j) r.dsb[j] = a.d_sigma[drow * S + j];
    }
    r.dc = *reinterpret_cast<const f4*>(a.d_color + drow * a.d_color_stride);
  } else {
    r.ds = a.d_sigma[drow];
    r.dc = *reinterpret_cast<const f4*>(a.d_color + drow * a.d_color_stride);
  }
}

// the OR of a raw f16 dL/dcolor row's bits (the f32 form has no use for it)
__device__ __forceinline__ uint32_t or_bits(h4 v) {
  typedef uint32_t u2 __attribute__((ext_vector_type(2)));
  const u2 b = __builtin_bit_cast(u2, v);
  return b.x | b.y;
}
__device__ __forceinline__ uint32_t or_bits(f4) { return 0u; }

template <bool HG, int S = 1>
__device__ __forceinline__ void raw_to_rows(const RawRowsT<HG, S>& r, int g, Rows& in) {
  in.xe = r.xe;
  in.dx = r.d0 * 2.0f - 1.0f;
  in.dy = r.d1 * 2.0f - 1.0f;
  in.dz = r.d2 * 2.0f - 1.0f;
  const f4 z4 = {0.0f, 0.0f, 0.0f, 0.0f};
  if constexpr (HG) {
    in.ds = static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>(r.ds)));
    in.dc = g == 0 ? __builtin_convertvector(r.dc, f4) : z4;
  } else if constexpr (S > 1) {
    in.ds = 0.0f;  // the S values go to the kernel's own registers (r.dsb)
    in.dc = g == 0 ? r.dc : z4;
  } else {
    in.ds = r.ds;
    in.dc = g == 0 ? r.dc : z4;
  }
}

// ---------------------------------------------------------------------------------
// Backward, register-transposed: no layer input or gradient tile goes through LDS (LDS
// holds the packed weights and the block's dW sums). (The r01 generation that staged
// every tile in LDS and read it back with ds_read_b64_tr_b16, and r03's variant with only
// the dW operand transposes through LDS, were A/B generations; removed in r04.)
//
// dW += G^T · X contracts over the samples, so both operands need the samples along K
// (lane = unit, samples in the lane's registers) while the chain holds every tile with
// lane = sample. The transpose is one MFMA against a constant 0/1 matrix: a C-layout
// tile (lane = sample l&15, units 4g..4g+3) read as the A operand of a 16x16x16 MFMA is
// the tile with samples as rows, and times the identity it comes back in C layout with
// lane = unit l&15 and samples 4g..4g+3 — exact (one 1·x product per output, the other
// terms 0·x = 0 for finite x). Tiles held as 8-slot B operands (the encoding, the dir
// input) go through a 16x16x32 MFMA against [I|0] or [0|I]. The dW A operand of a
// 32-sample tile is then cat(transpose(half 0), transpose(half 1)), i.e. samples in the
// order (4g..4g+3, 16+4g..16+4g+3) along K, and the B operand the same: the contraction
// is order-blind.
// ReLU masks are the forward's activations, kept in registers.
// ---------------------------------------------------------------------------------
template <bool BF>
struct TrConst {
  h4 id;      // I16 as a 16x16x16 B operand: lane (column c = l&15) holds rows 4g..4g+3
  h8 sel[2];  // [I16; 0] and [0; I16] (32 x 16) as 16x16x32 B operands: slot 16kb + c
  __device__ void init(int lane) {
    const int c = lane & 15, g = lane >> 4;
    const _Float16 one = cvt1<BF>(1.0f), zero = cvt1<BF>(0.0f);
#pragma unroll
    for (int i = 0; i < 4; ++i) id[i] = 4 * g + i == c ? one : zero;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int j = 0; j < 8; ++j) sel[kb][j] = 8 * g + j == 16 * kb + c ? one : zero;
  }
};
// C-layout tile (lane = sample, 4 units) -> (lane = unit, 4 samples)
template <bool BF>
__device__ __forceinline__ h4 tr_c(h4 t, h4 id) {
  return to_h4<BF>(mma16<BF>(t, id, f4{0.0f, 0.0f, 0.0f, 0.0f}));
}
// B-operand tile (lane = sample, slots 8g..8g+7) -> (lane = slot 16kb + l&15, 4 samples)
template <bool BF>
__device__ __forceinline__ h4 tr_b(h8 x, h8 sel) {
  return to_h4<BF>(mma32<BF>(x, sel, f4{0.0f, 0.0f, 0.0f, 0.0f}));
}


// ---- forms of the backward kernel: bwd_rt_kernel<W, NHD, BF, S, F> is compiled for a form F
// that names its numerics, what it writes dL/denc as, which pass it is and how its inputs
// arrive. The entry points and plan_bwd / plan_bwd_ref pick forms by these names.
enum class Pass { whole, pos, list };
struct GeneralColor : std::false_type {};  // dL/dcolor of any n_out / stride, d_sigma nullable
struct FastColor : std::true_type {};      // n_out == 4, aligned rows, d_sigma: prefetched a tile ahead
struct DenseRows : std::false_type {};     // row r is sample r
struct GatheredRows : std::true_type {};   // row r is sample a.rows[r] (occupancy-compacted)
struct F32Grads : std::false_type {};      // a.d_sigma / a.d_color
struct F16Grads : std::true_type {};       // a.d_sigma_h / a.d_color_h, as the f16 composite backward
                                           // writes them (10 B per row instead of 20); converted to
                                           // f32, exactly, as they are loaded
template <bool REF_, bool RMASK_, Pass PASS_, typename Grads, typename Rows, typename Color>
struct Form {
  // Reference numerics (tcnn's loss-scaled f16 backward, f16 only): the gradient scale is the
  // fixed a.loss_scale instead of the per-wavefront power of two, the ReLU masks test the
  // f16-rounded outputs, and the gradients that cross tinycudann module boundaries are rounded
  // as they are there: dL/dpos_out[1:16] comes back from dir_mlp as f16(f16(g_scaled) / scale)
  // (an f16 division that keeps subnormals, as torch's does:
  // tests/test_field_ref16_oracle_gpu.py) and is rescaled for pos_mlp, and dL/denc is written
  // as f16(f16(g_scaled) / scale) (tinycudann/modules.py: input_grad / loss_scale in the f16
  // input's dtype). Build numerics otherwise.
  static constexpr bool REF = REF_;
  // dL/denc as f16 rows (a.d_enc_h; the values are f16 numbers already) plus one bit per row,
  // set when any of the row's 32 values is nonzero (a.row_nz, a word per 32-row tile);
  // f32 rows (a.d_enc) otherwise
  static constexpr bool RMASK = RMASK_;
  static constexpr Pass PASS = PASS_;
  static constexpr bool POS = PASS == Pass::pos;    // no dir network in this kernel
  static constexpr bool LIST = PASS == Pass::list;  // walks a.tile_list, the general tile path
  static constexpr bool HG = Grads::value, ROWS = Rows::value, FAST = Color::value;
  // full tiles of the pos pass with f16 gradients: "any dL/dcolor nonzero" from the raw bits
  static constexpr bool RAWC = POS && HG;
  static_assert(!HG || RMASK, "f16 gradients: the reference-numerics f16-rows forms");
  static_assert(!RMASK || REF, "f16 rows and row bits: reference numerics");
  static_assert(PASS == Pass::whole || (RMASK && FAST),
                "the pos / list passes write f16 rows and use the fast d_color layout");
  static_assert(!(REF && ROWS), "reference numerics: dense rows");
  // the forms a numeric type BF and S density outputs exist for
  template <bool BF, int S>
  static constexpr bool fits() {
    static_assert(!(REF && BF), "reference numerics are f16");
    static_assert(S == 1 || (!REF && !ROWS), "S > 1: build numerics, dense rows");
    return true;
  }
};
// build numerics: per-wavefront dynamic scale, f32 gradients and rows. S > 1 (dense rows):
// d_sigma is (M, S); dL/dpos_out[j < S] is d_sigma[j] through unit j's own ReLU (the dir network
// has no input from those units), all in the g == 0 lane's four registers
template <typename Color, typename Rows>
struct Build : Form<false, false, Pass::whole, F32Grads, Rows, Color> {};
// anr_ingp_field_bwd_ref16: reference numerics, dL/denc as f32 rows
template <typename Color>
struct RefF32Rows : Form<true, false, Pass::whole, F32Grads, DenseRows, Color> {};
// anr_ingp_field_bwd_ref16_rows (_h: F16Grads) without a workspace: f16 rows and row bits
template <typename Color, typename Grads>
struct RefF16Rows : Form<true, true, Pass::whole, Grads, DenseRows, Color> {};
// its pos pass, with a workspace: RefF16Rows on the tiles whose dL/dcolor is zero in every row,
// the pos network only (no dir registers, dW accumulators or LDS sums: more waves fit a SIMD);
// a tile with a nonzero dL/dcolor is appended to a.tile_list and left alone. Rank-1 output
// layer (w1r), f16 dL/denc from accumulator to store, zero tests on the f16 bits: bound by VALU
// issue (profiles/pos_rank1_summary.md). Same dL/denc, row bits and list as RefF16Rows, g_pos
// up to the f32 order of row 0 of dW_P1
template <typename Grads>
struct PosPass : Form<true, true, Pass::pos, Grads, DenseRows, FastColor> {};
// the list pass, launched after it: RefF16Rows on exactly the listed tiles (count read on the
// device), the whole network
template <typename Grads>
struct ListPass : Form<true, true, Pass::list, Grads, DenseRows, FastColor> {};

template <int W, int NHD, bool BF, int S, typename F>
__global__ void __launch_bounds__(256) bwd_rt_kernel(Args a, float target, int64_t tpw,
                                                     const float* wmax) {
  static_assert(F::template fits<BF, S>(), "no such backward kernel");
  using RawRows = RawRowsT<F::HG, S>;
  // MT 16-sample halves per tile, the dW contraction over NP pairs of them. (64-sample
  // tiles, MT = 4, measured 6 % slower at the same 1 wave/SIMD: profiles/r03_field_bwd_ab.log)
  constexpr int MT = 2, TR = 16 * MT, NP = MT / 2;
  using N = Net<W, NHD, S>;
  constexpr int NT = N::NT, KB = N::KB;
  if constexpr (F::LIST) {
    // the list pass: a block none of whose waves has a listed tile leaves before its
    // prologue (weights into LDS, sums zeroed): in the settled state the list is empty and
    // the whole launch was ~26 us of prologues (rocprof r06_c). Block-uniform exit.
    const uint32_t cnt = static_cast<uint32_t>(
        __builtin_amdgcn_readfirstlane(static_cast<int>(*a.tile_count)));
    if (static_cast<uint64_t>(blockIdx.x) * (blockDim.x >> 6) >= cnt) return;
  }
  __shared__ __attribute__((aligned(16))) _Float16 wsm[N::n_packed];
  // the block's dW partials (pos parameters, then dir), summed here before the one global
  // flush per block
  __shared__ float red[F::POS ? N::NPOS : N::NPOS + N::NDIR];
  const int lane = threadIdx.x & 63, g = lane >> 4, li = lane & 15;
  const int waves = blockDim.x >> 6, wave = threadIdx.x >> 6;
  for (int e = threadIdx.x * 8; e < N::n_packed; e += blockDim.x * 8)
    *reinterpret_cast<h8*>(wsm + e) = *reinterpret_cast<const h8*>(a.packed + e);
  constexpr int NRED = F::POS ? N::NPOS : N::NPOS + N::NDIR;
  for (int e = threadIdx.x; e < NRED; e += blockDim.x) red[e] = 0.0f;
  __syncthreads();
  // per-tile opaque copy of the fragment base: the weight fragments are re-read from LDS
  // each tile instead of being hoisted into registers
  const _Float16* wbt = wsm;
  auto bfrag32 = [&](int off) { return *reinterpret_cast<const h8*>(wbt + off + lane * 8); };
  auto bfrag16 = [&](int off) { return *reinterpret_cast<const h4*>(wbt + off + lane * 4); };
  TrConst<BF> tc;
  tc.init(lane);
  // dW operand transposes (MFMA against the constant 0/1 operands)
  auto trc = [&](h4 x) -> h4 { return tr_c<BF>(x, tc.id); };
  auto trb = [&](h8 x, h4& o0, h4& o1) {
    o0 = tr_b<BF>(x, tc.sel[0]);
    o1 = tr_b<BF>(x, tc.sel[1]);
  };
  // POS: dL/dpos_out is dL/dsigma in unit 0 and exact zeros in the other 15 units, so the
  // output layer's backward is rank 1: dhp = P1[0][:] * dpo0 (one f16 product per value,
  // what the MFMA's single nonzero term rounded to f16 is) and only row 0 of dW_P1 gets
  // sums. Row 0 of P1 for this lane's units 16 kt + 4 g + i stays in registers (k = 0 of
  // the transposed fragment: lane 4 g + i, element 0), row 0 of dW_P1 is summed per lane
  // in f32 over the lane's samples and reduced over the 16 sample lanes after the loop.
  h4 w1r[NT];
  float dP1r[NT][4];
  if constexpr (F::POS) {
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        w1r[kt][i] = wsm[N::oBP1 + kt * N::F16 + 16 * g + 4 * i];
        dP1r[kt][i] = 0.0f;
      }
    }
  }

  const int64_t n_tiles = (a.M + TR - 1) / TR;
  const int64_t w_id = static_cast<int64_t>(blockIdx.x) * waves + wave;
  const int64_t t_begin = w_id * tpw;
  const int64_t t_end = t_begin + tpw < n_tiles ? t_begin + tpw : n_tiles;
  const int64_t n_full = a.M / TR;

  f4 dD2[NT], dD1[NHD == 2 ? NT * NT : 1], dD0[NT * 2], dP1[NT], dP0[NT * 2];
  const f4 z4 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int i = 0; i < NT; ++i) dD2[i] = dP1[i] = z4;
#pragma unroll
  for (int i = 0; i < NT * 2; ++i) dD0[i] = dP0[i] = z4;
  if constexpr (NHD == 2) {
#pragma unroll
    for (int i = 0; i < NT * NT; ++i) dD1[i] = z4;
  }
  float s = 1.0f, inv_s = 1.0f;
  if constexpr (F::REF) {
    s = a.loss_scale;
    inv_s = 1.0f / a.loss_scale;
  } else if constexpr (!BF) {
    const float gm = wave_grad_max(a, wmax, w_id, t_begin, t_end);
    if (gm > 0.0f) {
      int e = static_cast<int>(floorf(log2f(target / gm)));
      e = e < -60 ? -60 : (e > 100 ? 100 : e);
      s = ldexpf(1.0f, e);
      inv_s = ldexpf(1.0f, -e);
    }
  }
  // f32 -> f16 -> f32 (the reference's f16 tensors between modules)
  auto r16 = [](float v) { return static_cast<float>(static_cast<_Float16>(v)); };
  Rows cur[MT];
  f4 curb[S > 1 ? MT : 1];  // S > 1: dL/dsigma[row][0 .. S-1] of cur's rows
  // the next tile's raw inputs, loaded a tile ahead into alternating register sets (the
  // full-tile loop runs two tiles per trip): with one set, the loop-carried copy of the
  // prefetch registers lands wherever the register allocator puts it, and where that is
  // early in the tile it waits on the loads just issued (1 wave/SIMD: nothing hides it)
  RawRows nr0[MT], nr1[MT];
  const int64_t t_full_end = t_end < n_full ? t_end : n_full;
  if constexpr (F::FAST) {
    if (t_begin < t_full_end) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) load_raw<F::ROWS, F::HG, S>(a, t_begin * TR + mt * 16 + li, g, nr0[mt]);
      // drained once, so the loop entry carries no pending loads: entered with the first
      // prefetch in flight, the waitcnt pass merges that state with the back edge's (the
      // prefetch, then the tile's d_enc stores) into a wait for everything, stores
      // included, at the head of every tile
      __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    }
  }
  // FAST full tiles hand their dL/denc rows to the NEXT tile's head, which stores them
  // between its input conversion and its prefetch. Stored at the tile's end, they were the
  // newest entries of the in-order vmcnt queue when the next head waited for its
  // prefetched inputs, so every tile head also waited for the previous tile's store acks
  // (vmcnt(0) a few instructions after the stores). The first head stores zeros to its own
  // rows (rewritten by that tile's real values later, same wave, same addresses).
  f4 pend[2][MT];
  int64_t pend_tile = t_begin;
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) pend[kt][mt] = f4{0.0f, 0.0f, 0.0f, 0.0f};
  // POS: the deferred rows as the f16 values that are stored (pend unused), scaled back by
  // one packed f16 multiply where 1 / loss_scale is an f16 number (any power of two in
  // range): f16(acc) * inv_s is then exact in f32 either way and rounded to f16 once
  h4 pendh[2][MT];
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) pendh[kt][mt] = h4{0, 0, 0, 0};
  const _Float16 inv_h = static_cast<_Float16>(inv_s);
  const bool inv_is_h = static_cast<float>(inv_h) == inv_s;
  // one lane's 4 values of dL/denc row `row`, columns 16 kt + 4 g .. + 3
  auto put = [&](int64_t row, int kt, const f4& v) {
    if constexpr (F::RMASK) {
      const h4 hv = {static_cast<_Float16>(v[0]), static_cast<_Float16>(v[1]),
                     static_cast<_Float16>(v[2]), static_cast<_Float16>(v[3])};
      *reinterpret_cast<h4*>(a.d_enc_h + row * a.d_enc_stride + 16 * kt + 4 * g) = hv;
    } else {
      *reinterpret_cast<f4*>(a.d_enc + row * a.d_enc_stride + 16 * kt + 4 * g) = v;
    }
  };
  // RMASK: the tile's row bits from each lane's "my 8 values of row (mt, li) are not all
  // zero" (uniform control flow: the ballots need every lane); rows of a row's four lanes
  // g = 0..3 sit at ballot bits li + 16 g
  auto put_mask = [&](int64_t tile, const bool (&nz)[MT]) {
    if constexpr (F::RMASK) {
      uint32_t word = 0;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const uint64_t b = __ballot(nz[mt]);
        const uint32_t r = static_cast<uint32_t>((b | (b >> 16) | (b >> 32) | (b >> 48)) & 0xFFFFull);
        word |= r << (16 * mt);
      }
      if (lane == 0) a.row_nz[tile] = word;
    }
  };
  auto nz_of = [](const f4& v0, const f4& v1) {
    return v0[0] != 0.0f || v0[1] != 0.0f || v0[2] != 0.0f || v0[3] != 0.0f || v1[0] != 0.0f ||
           v1[1] != 0.0f || v1[2] != 0.0f || v1[3] != 0.0f;
  };
  auto store_pend = [&]() {
    if constexpr (F::POS) {
      typedef uint32_t u2 __attribute__((ext_vector_type(2)));
      bool nz[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        _Float16* const p = a.d_enc_h + (pend_tile * TR + mt * 16 + li) * a.d_enc_stride + 4 * g;
        *reinterpret_cast<h4*>(p) = pendh[0][mt];
        *reinterpret_cast<h4*>(p + 16) = pendh[1][mt];
        // any of the 8 values nonzero (-0 is zero): the bits without the signs
        const u2 b0 = __builtin_bit_cast(u2, pendh[0][mt]), b1 = __builtin_bit_cast(u2, pendh[1][mt]);
        nz[mt] = ((b0.x | b0.y | b1.x | b1.y) & 0x7FFF7FFFu) != 0u;
      }
      put_mask(pend_tile, nz);
      return;
    }
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) put(pend_tile * TR + mt * 16 + li, kt, pend[kt][mt]);
    if constexpr (F::RMASK) {
      bool nz[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) nz[mt] = nz_of(pend[0][mt], pend[1][mt]);
      put_mask(pend_tile, nz);
    }
  };
  // the dW MFMAs issued so far have written their accumulators before anything (a loop-exit
  // copy) reads them
  auto fence = [&]() {
    agpr_fence();
    if constexpr (!F::POS) {
      agpr_pin(dD2);
      agpr_pin(dD1);
      agpr_pin(dD0);
      agpr_pin(dP1);
    }
    agpr_pin(dP0);
  };
  // dX of a layer, one 16-unit block: the layer's KB K blocks of W^T (fragments w[kb]) times
  // the gradient tiles gr
  auto dx_block = [&](const h8* w, const h4(&gr)[MT][NT], f4(&dx)[MT]) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) dx[mt] = z4;
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        dx[mt] = mma32<BF>(w[kb], cat(gr[mt][2 * kb], gr[mt][2 * kb + 1]), dx[mt]);
    }
  };
  // One tile, as eight steps: 1 the tile head, 2 the gradient-free exit, 3 the colour-free
  // decision and the list append, 4 the forward recompute, 5 the dir network's backward, 6 the
  // pos output layer, 7 the pos input layer with the dL/denc emit; 8, the dW flush, ends the
  // kernel. (A step as a function or lambda of its own changes the machine code, see DESIGN
  // section 5 "Forms", so they stay one body.) nraw holds the tile's prefetched inputs, nnext
  // takes the next tile's (FAST full tiles).
  auto process = [&](auto full_c, int64_t tile, RawRows(&nraw)[MT], RawRows(&nnext)[MT]) {
    constexpr bool FULL = decltype(full_c)::value;
    {
      int zoff = 0;
      asm volatile("" : "+v"(zoff));
      wbt = wsm + zoff;
    }
    // POS, f16 gradients, full tiles: "any dL/dcolor nonzero" from the raw bits of the row's
    // four f16 values (every lane group loaded the same four), not from eight f32 compares
    constexpr bool RAWC = F::RAWC && FULL;
    uint32_t dcor = 0;
    // ---- 1, the tile's inputs
    if constexpr (F::FAST && FULL) {
      // the tile's head: this tile's prefetched inputs are converted here (hoisted into the
      // previous tile, the conversion waits on loads just issued) and the next tile's loads
      // are issued here (the scheduler otherwise sinks them toward the tile's end)
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        // ordered (volatile) uses of the prefetched registers: without them the select /
        // remap of raw_to_rows floats up to the loads in the previous tile. The scalars
        // are copied by a real v_mov, not an empty tied asm: the remap's packed FMA wants
        // (d1, d2) in an aligned pair, and a tied operand would move that copy up to the
        // dwordx3 load (where it waits for it)
        RawRows rr = nraw[mt];
        asm volatile("v_mov_b32 %0, %1" : "=v"(rr.d0) : "v"(nraw[mt].d0));
        asm volatile("v_mov_b32 %0, %1" : "=v"(rr.d1) : "v"(nraw[mt].d1));
        asm volatile("v_mov_b32 %0, %1" : "=v"(rr.d2) : "v"(nraw[mt].d2));
        if constexpr (S == 1) {
          asm volatile("v_mov_b32 %0, %1" : "=v"(rr.ds) : "v"(nraw[mt].ds));
        } else {
#pragma unroll
          for (int j = 0; j < S; ++j)
            asm volatile("v_mov_b32 %0, %1" : "=v"(rr.dsb[j]) : "v"(nraw[mt].dsb[j]));
        }
        asm volatile("" : "+v"(rr.dc));
        if constexpr (RAWC) dcor |= or_bits(rr.dc);
        raw_to_rows(rr, g, cur[mt]);
        if constexpr (S > 1) {
          curb[mt] = z4;
#pragma unroll
          for (int j = 0; j < S; ++j) curb[mt][j] = rr.dsb[j];
        }
      }
      store_pend();
      const int64_t tn = tile + 1 < t_full_end ? tile + 1 : tile;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) load_raw<F::ROWS, F::HG, S>(a, tn * TR + mt * 16 + li, g, nnext[mt]);
      __builtin_amdgcn_sched_barrier(0);
    } else {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        load_rows<F::ROWS, F::HG, S>(a, tile * TR + mt * 16 + li, g, true, cur[mt]);
      if constexpr (S > 1) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
          curb[mt] = load_dsig<F::ROWS, S>(a, tile * TR + mt * 16 + li);
      }
    }
    const bool full = FULL;
    {
      // ---- 2. A tile whose incoming gradients (dL/dcolor, dL/dsigma) are zero in every row adds
      // exactly nothing to dW and has dL/denc = 0: store the zeros, skip the recompute and
      // the backward (wave-uniform). Under the reference numerics tcnn's x128 f16 backward
      // leaves most tiles so once training settles (profiles/r05_state160.log); the build
      // numerics' f32 gradients almost never are, and pay one test per tile.
      bool nz = RAWC && (dcor & 0x7FFF7FFFu) != 0u;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        nz = nz || cur[mt].ds != 0.0f;
        if constexpr (!RAWC)
          nz = nz || cur[mt].dc[0] != 0.0f || cur[mt].dc[1] != 0.0f || cur[mt].dc[2] != 0.0f ||
               cur[mt].dc[3] != 0.0f;
        if constexpr (S > 1) {
#pragma unroll
          for (int j = 0; j < S; ++j) nz = nz || curb[mt][j] != 0.0f;
        }
      }
      const bool walk = __any(nz);
      if (a.tile_nz && lane == 0) a.tile_nz[tile] = walk ? 1 : 0;
      if (!walk) {
        const f4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
        if constexpr (F::FAST && FULL) {
#pragma unroll
          for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
              pend[kt][mt] = zero4;
              pendh[kt][mt] = h4{0, 0, 0, 0};
            }
          pend_tile = tile;
          return;
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          const int64_t row = tile * TR + mt * 16 + li;
          if (full || row < a.M) {
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) put(row, kt, zero4);
          }
        }
        if constexpr (F::RMASK) {
          bool nz[MT];
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) nz[mt] = false;
          put_mask(tile, nz);
        }
        return;
      }
    }
    // ---- 3. A tile whose dL/dcolor is zero in every row (reference numerics: every tile once
    // training settles -- tcnn's f16 composite backward rounds the per-sample colour
    // gradients of the atmosphere's tiny weights to zero, profiles/r05_hash_bwd_state_tiles
    // .log): the dir network's backward adds exactly 0 to its dW and returns dX = 0, so
    // neither it nor the dir half of the forward recompute runs (wave-uniform); dL/dpos_out
    // is then dL/dsigma alone. Exact for finite weights and activations (0 * x = 0).
    // Reference numerics, fast d_color layout only: the build numerics' f32 colour
    // gradients are never all zero, and the branch costs their kernel registers (spills);
    // in the general-layout kernel the branch's register copies read dW accumulators right
    // behind their inline-asm MFMAs (tools/mfma_hazards.py)
    bool dir_walk = true;
    if constexpr (RAWC) {
      dir_walk = __any((dcor & 0x7FFF7FFFu) != 0u);
    } else if constexpr (F::REF && F::FAST) {
      bool cnz = false;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        cnz = cnz || cur[mt].dc[0] != 0.0f || cur[mt].dc[1] != 0.0f || cur[mt].dc[2] != 0.0f ||
              cur[mt].dc[3] != 0.0f;
      dir_walk = __any(cnz);
    }
    if constexpr (F::POS) {
      if (dir_walk) {  // the list pass takes this tile (d_enc rows and bits included)
        if (lane == 0) a.tile_list[atomicAdd(a.tile_count, 1u)] = static_cast<int32_t>(tile);
        return;
      }
    }
    // ---- 4, forward recompute of both 16-sample halves; every activation stays in registers
    Tile<W, NHD> t[MT];
    h4 gc[MT];
    bool dens[MT];
    bool densb[S > 1 ? MT : 1][4];  // S > 1: the S density units' ReLU masks
    {
      bool valid[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) valid[mt] = full || tile * TR + mt * 16 + li < a.M;
      FwdWeights<W, NHD> fwl;
      fwl.load(wbt, lane, !F::POS && dir_walk);
      tile_forward<W, NHD, MT, BF, S>(fwl, cur, valid, g, t, NoSink{}, !F::POS && dir_walk);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        dens[mt] = (F::REF ? r16(t[mt].po[0]) : t[mt].po[0]) > 0.0f;
        if constexpr (S > 1) {
#pragma unroll
          for (int j = 0; j < 4; ++j) densb[mt][j] = t[mt].po[j] > 0.0f;
        }
        f4 gv;
#pragma unroll
        for (int i = 0; i < 4; ++i)
          gv[i] = (F::REF ? r16(t[mt].col[i]) : t[mt].col[i]) > 0.0f ? cur[mt].dc[i] * s : 0.0f;
        gc[mt] = to_h4<BF>(gv);
      }
    }
    h4 dpo[MT];
    if (!F::POS && dir_walk) {
      auto last = [&](int mt, int kt) -> h4 { return NHD == 2 ? t[mt].hd1[kt] : t[mt].hd0[kt]; };
      // ---- 5, the dir network. dir output layer: dW_D2 (16 x W) += gc^T · X_last ; dX_last = D2^T gc
      // Each layer's W^T fragments are read from LDS at the start of the layer and pinned
      // there (sched_barrier): the dW half of the layer, which needs no weights, then covers
      // the LDS latency that a read placed at its use exposes (1 wave/SIMD).
      h4 dl[MT][NT];
      {
        h4 wd2[NT];
  #pragma unroll
        for (int kt = 0; kt < NT; ++kt) wd2[kt] = bfrag16(N::oBD2 + kt * N::F16);
        __builtin_amdgcn_sched_barrier(0);
        h8 ga[NP];
  #pragma unroll
        for (int pr = 0; pr < NP; ++pr)
          ga[pr] = cat(trc(gc[2 * pr]), trc(gc[2 * pr + 1]));
  #pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
  #pragma unroll
          for (int pr = 0; pr < NP; ++pr) {
            const h8 xl = cat(trc(last(2 * pr, kt)), trc(last(2 * pr + 1, kt)));
            mma32_acc_v<BF>(dD2[kt], ga[pr], xl);
          }
  #pragma unroll
          for (int mt = 0; mt < MT; ++mt) dl[mt][kt] = mask_h4<BF>(mma16<BF>(wd2[kt], gc[mt], z4), last(mt, kt));
        }
      }
      // ---- dir hidden layer 1 (NHD == 2): dW_D1 (W x W) += dl^T · X_d0 ; dh0 = D1^T dl
      h4 dh0[MT][NT];
      if constexpr (NHD == 2) {
        h8 wd1[NT * KB];
  #pragma unroll
        for (int i = 0; i < NT * KB; ++i) wd1[i] = bfrag32(N::oBD1 + i * N::F32);
        __builtin_amdgcn_sched_barrier(0);
  #pragma unroll
        for (int pr = 0; pr < NP; ++pr) {
          h8 gb[NT];
  #pragma unroll
          for (int nt = 0; nt < NT; ++nt)
            gb[nt] = cat(trc(dl[2 * pr][nt]), trc(dl[2 * pr + 1][nt]));
  #pragma unroll
          for (int kt = 0; kt < NT; ++kt) {
            const h8 xb = cat(trc(t[2 * pr].hd0[kt]), trc(t[2 * pr + 1].hd0[kt]));
  #pragma unroll
            for (int nt = 0; nt < NT; ++nt) mma32_acc_v<BF>(dD1[nt * NT + kt], gb[nt], xb);
          }
        }
  #pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
          f4 acc[MT];
          dx_block(wd1 + kt * KB, dl, acc);
  #pragma unroll
          for (int mt = 0; mt < MT; ++mt) dh0[mt][kt] = mask_h4<BF>(acc[mt], t[mt].hd0[kt]);
        }
      } else {
  #pragma unroll
        for (int mt = 0; mt < MT; ++mt)
  #pragma unroll
          for (int kt = 0; kt < NT; ++kt) dh0[mt][kt] = dl[mt][kt];
      }
      // ---- dir input layer: dW_D0 (W x 32, k' order) += dh0^T · X_de ; dpos = D0^T dh0
      {
        h8 wd0[KB];
  #pragma unroll
        for (int kb = 0; kb < KB; ++kb) wd0[kb] = bfrag32(N::oBD0 + kb * N::F32);
        __builtin_amdgcn_sched_barrier(0);
  #pragma unroll
        for (int pr = 0; pr < NP; ++pr) {
          h4 a0, a1, b0, b1;
          trb(t[2 * pr].xd, a0, a1);
          trb(t[2 * pr + 1].xd, b0, b1);
          const h8 x0 = cat(a0, b0), x1 = cat(a1, b1);
  #pragma unroll
          for (int nt = 0; nt < NT; ++nt) {
            const h8 gd = cat(trc(dh0[2 * pr][nt]), trc(dh0[2 * pr + 1][nt]));
            mma32_acc_v<BF>(dD0[nt * 2], gd, x0);
            mma32_acc_v<BF>(dD0[nt * 2 + 1], gd, x1);
          }
        }
        f4 acc[MT];
        dx_block(wd0, dh0, acc);
  #pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          if constexpr (F::REF) {
  #pragma unroll
            for (int i = 0; i < 4; ++i) acc[mt][i] = r16(r16(r16(acc[mt][i]) * inv_s) * s);
          }
          if constexpr (S == 1) {
            // pos_out[:, 0] is the density: its gradient is dL/dsigma through the ReLU
            const float dsv = dens[mt] ? cur[mt].ds * s : 0.0f;
            acc[mt][0] = g == 0 ? dsv : acc[mt][0];
          } else {
            // pos_out[:, j < S]: band j's density, dL/dsigma[j] through its own ReLU
#pragma unroll
            for (int j = 0; j < S; ++j) {
              const float dsv = densb[mt][j] ? curb[mt][j] * s : 0.0f;
              acc[mt][j] = g == 0 ? dsv : acc[mt][j];
            }
          }
          dpo[mt] = to_h4<BF>(acc[mt]);
        }
      }
    } else if constexpr (!F::POS) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        f4 acc = z4;
        acc[0] = g == 0 && dens[mt] ? cur[mt].ds * s : 0.0f;
        dpo[mt] = to_h4<BF>(acc);
      }
    }
    // ---- 6, pos output layer: dW_P1 (16 x W) += dpo^T · X_ph ; dhp = P1^T dpo
    h4 dhp[MT][NT];
    if constexpr (F::POS) {
      // rank 1 (see w1r): dpo0 = f16(dL/dsigma * scale) through the density ReLU, formed in
      // the row's g == 0 lane (the one holding pos_out[0]) and handed to its other three
      // lane groups, both halves of the tile in one 32-bit word
      uint32_t pk = 0;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const _Float16 d = static_cast<_Float16>(g == 0 && dens[mt] ? cur[mt].ds * s : 0.0f);
        pk |= static_cast<uint32_t>(__builtin_bit_cast(uint16_t, d)) << (16 * mt);
      }
      pk = static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(li << 2, static_cast<int>(pk)));
      static_assert(MT == 2, "dpo0 of the tile's two halves in one word");
#pragma unroll
      for (int kt = 0; kt < NT; ++kt) {
        dhp[0][kt] = mask_bits(scale_h4<0>(w1r[kt], pk), t[0].hp[kt]);
        dhp[1][kt] = mask_bits(scale_h4<1>(w1r[kt], pk), t[1].hp[kt]);
        fma_h4<0>(dP1r[kt], t[0].hp[kt], pk);
        fma_h4<1>(dP1r[kt], t[1].hp[kt], pk);
      }
    } else {
      h4 wp1[NT];
#pragma unroll
      for (int kt = 0; kt < NT; ++kt) wp1[kt] = bfrag16(N::oBP1 + kt * N::F16);
      __builtin_amdgcn_sched_barrier(0);
      h8 ga[NP];
#pragma unroll
      for (int pr = 0; pr < NP; ++pr)
        ga[pr] = cat(trc(dpo[2 * pr]), trc(dpo[2 * pr + 1]));
#pragma unroll
      for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
        for (int pr = 0; pr < NP; ++pr) {
          const h8 xp = cat(trc(t[2 * pr].hp[kt]), trc(t[2 * pr + 1].hp[kt]));
          mma32_acc_v<BF>(dP1[kt], ga[pr], xp);
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) dhp[mt][kt] = mask_h4<BF>(mma16<BF>(wp1[kt], dpo[mt], z4), t[mt].hp[kt]);
      }
    }
    // ---- 7, pos input layer: dW_P0 (W x 32) += dhp^T · X_pe ; d_enc = P0^T dhp
    {
      h8 wp0[2 * KB];
#pragma unroll
      for (int i = 0; i < 2 * KB; ++i) wp0[i] = bfrag32(N::oBP0 + i * N::F32);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int pr = 0; pr < NP; ++pr) {
        h4 a0, a1, b0, b1;
        trb(t[2 * pr].xe, a0, a1);
        trb(t[2 * pr + 1].xe, b0, b1);
        const h8 x0 = cat(a0, b0), x1 = cat(a1, b1);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          const h8 gp = cat(trc(dhp[2 * pr][nt]), trc(dhp[2 * pr + 1][nt]));
          mma32_acc_v<BF>(dP0[nt * 2], gp, x0);
          mma32_acc_v<BF>(dP0[nt * 2 + 1], gp, x1);
        }
      }
      // RMASK outside the pend path: the tile's rows, kept until both column halves are out
      f4 keep[F::RMASK && !(F::FAST && FULL) ? 2 : 1][MT];
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        f4 acc[MT];
        dx_block(wp0 + kt * KB, dhp, acc);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          const int64_t row = tile * TR + mt * 16 + li;
          if constexpr (F::POS && F::FAST && FULL) {
            // the stored f16 values directly (see pendh)
            h4 hv = to_h4<false>(acc[mt]);
            if (inv_is_h) {
              hv = hv * h4{inv_h, inv_h, inv_h, inv_h};
            } else {
#pragma unroll
              for (int i = 0; i < 4; ++i)
                hv[i] = static_cast<_Float16>(static_cast<float>(hv[i]) * inv_s);
            }
            pendh[kt][mt] = hv;
            continue;
          }
          f4 v = acc[mt] * inv_s;
          if constexpr (F::REF) {
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = r16(r16(acc[mt][i]) * inv_s);
          }
          if constexpr (F::RMASK && !(F::FAST && FULL)) keep[kt][mt] = (full || row < a.M) ? v : z4;
          if (full || row < a.M) {
            if constexpr (F::FAST && FULL)
              pend[kt][mt] = v;
            else
              put(row, kt, v);
          }
        }
      }
      if constexpr (F::FAST && FULL) pend_tile = tile;
      if constexpr (F::RMASK && !(F::FAST && FULL)) {
        bool nz[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) nz[mt] = nz_of(keep[0][mt], keep[1][mt]);
        put_mask(tile, nz);
      }
    }
    // the last dW MFMAs of the tile have written their accumulators before anything
    // (a loop-exit copy) reads them
    fence();
  };
  if constexpr (F::LIST) {
    // the listed tiles, strided over the grid's wavefronts (the general per-tile path: a
    // listed tile's neighbours are not this wave's)
    const int64_t nw = static_cast<int64_t>(gridDim.x) * waves;
    const int64_t cnt = static_cast<int64_t>(__builtin_amdgcn_readfirstlane(
        static_cast<int>(*a.tile_count)));
    for (int64_t i = w_id; i < cnt; i += nw)
      process(std::integral_constant<bool, false>{},
              static_cast<int64_t>(__builtin_amdgcn_readfirstlane(a.tile_list[i])), nr0, nr1);
  } else {
    {
      const std::integral_constant<bool, true> full_tile;
      int64_t tile = t_begin;
      for (; tile + 1 < t_full_end; tile += 2) {
        process(full_tile, tile, nr0, nr1);
        process(full_tile, tile + 1, nr1, nr0);
      }
      if (tile < t_full_end) process(full_tile, tile, nr0, nr1);
      if constexpr (F::FAST) {
        if (t_begin < t_full_end) store_pend();
      }
    }
    for (int64_t tile = t_full_end > t_begin ? t_full_end : t_begin; tile < t_end; ++tile)
      process(std::integral_constant<bool, false>{}, tile, nr0, nr1);
  }

  fence();
  // ---- 8, dW flush: each wavefront's partials (unscaled by its own gradient scale) go into the
  // block's LDS sums, then the block adds them to the f32 gradients with one coalesced
  // atomic per parameter: a quarter of the r03 memory-side requests (one set per
  // wavefront; ~33 us per launch at 1,024 wavefronts, fixed in M)
  float* const rpos = red;
  float* const rdir = red + N::NPOS;
  auto flush = [&](float* dst, int ld, const f4& d, int n0, int k) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (d[i] != 0.0f) atomicAdd(dst + (n0 + 4 * g + i) * ld + k, d[i] * inv_s);
  };
#pragma unroll
  for (int kt = 0; kt < NT; ++kt) {
    if constexpr (!F::POS) {
      flush(rdir + N::D2, W, dD2[kt], 0, 16 * kt + li);
      flush(rpos + N::P1, W, dP1[kt], 0, 16 * kt + li);
    } else {
      // row 0 of dW_P1: the lane's sums over its samples, added over the 16 sample lanes of
      // its group (the four groups hold different units); lane li == 0 adds the total
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float v = dP1r[kt][i];
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) v += __shfl_xor(v, m, 64);
        if (li == 0 && v != 0.0f) atomicAdd(rpos + N::P1 + 16 * kt + 4 * g + i, v * inv_s);
      }
    }
  }
  if constexpr (NHD == 2 && !F::POS) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int kt = 0; kt < NT; ++kt) flush(rdir + N::D1, W, dD1[nt * NT + kt], 16 * nt, 16 * kt + li);
  }
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      if constexpr (!F::POS) {
        if constexpr (S == 1) {
          flush(rdir + N::D0, 32, dD0[nt * 2 + kt], 16 * nt, dir_col<1>(16 * kt + li));
        } else {
          // a padding slot's sum goes to its padding column, or nowhere (S = 4: no column)
          const int c = dir_col<S>(16 * kt + li);
          if (c >= 0) flush(rdir + N::D0, N::LD0, dD0[nt * 2 + kt], 16 * nt, c);
        }
      }
      flush(rpos + N::P0, 32, dP0[nt * 2 + kt], 16 * nt, 16 * kt + li);
    }
  __syncthreads();
  for (int e = threadIdx.x; e < NRED; e += blockDim.x) {
    const float v = red[e];
    if (v != 0.0f) atomicAdd(e < N::NPOS ? a.g_pos + e : a.g_dir + (e - N::NPOS), v);
  }
}

// ---------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------
static int g_target_log2 = 6;  // f16 gradient scale: max |dL/dout| of a wavefront -> 2^6
// forward form: 1 = the uniform-tile kernel where the shapes allow (default), 0 = always
// the general kernel; test / A-B hook anr_ingp_field_force_fwd
static int g_fwd_ut = 1;

// ---- run-time values as compile-time tags: each helper calls `f` with the tag of its value
// and answers `none` for a value it has no kernels for
template <int W_, int NHD_>
struct NetTag {
  static constexpr int W = W_, NHD = NHD_;
};
template <int V>
using int_c = std::integral_constant<int, V>;

// v: variant() of a pos/dir pair, 10 W + NHD
template <typename R, typename F>
static R with_net(int v, R none, F&& f) {
  switch (v) {
    case 321: return f(NetTag<32, 1>{});
    case 322: return f(NetTag<32, 2>{});
    case 641: return f(NetTag<64, 1>{});
    case 642: return f(NetTag<64, 2>{});
  }
  return none;
}
// ns: the pair's density outputs (n_sigma)
template <typename R, typename F>
static R with_bands(int ns, R none, F&& f) {
  switch (ns) {
    case 1: return f(int_c<1>{});
    case 2: return f(int_c<2>{});
    case 3: return f(int_c<3>{});
    case 4: return f(int_c<4>{});
  }
  return none;
}
template <typename F>
static auto with_bool(bool b, F&& f) {
  return b ? f(std::true_type{}) : f(std::false_type{});
}
// f(net, bands, bf) for a (variant, n_sigma, bf16 MFMA) triple
template <typename R, typename F>
static R with_variant(int v, int ns, bool bf, R none, F&& f) {
  return with_net(v, none, [&](auto net) {
    return with_bands(ns, none, [&](auto s) {
      return with_bool(bf, [&](auto b) { return f(net, s, b); });
    });
  });
}

// ---- launch plans: one per pass, for every S. They launch only kernels the library has
// always had: a form without one (S > 1 with rows, f16 outputs, f16 gradients or reference
// numerics; bf16 with reference numerics) answers no_kernel, behind `if constexpr` so that no
// kernel is instantiated for it.
enum class Plan { ok, no_kernel, workspace };

constexpr int kBlockWaves = 4;  // wavefronts per block of the forward, density and backward kernels
using FieldKernel = void (*)(Args);
using BwdKernel = void (*)(Args, float, int64_t, const float*);

// a grid-stride pass over 16-row tiles, a tile per wavefront, on at most `resident` blocks
static Plan launch_tiles16(FieldKernel k, int64_t resident, const Args& a, hipStream_t st) {
  const int64_t tiles = (a.M + 15) / 16;
  const int64_t blocks = persistent_blocks((tiles + kBlockWaves - 1) / kBlockWaves, resident);
  hipLaunchKernelGGL(k, dim3(blocks), dim3(64 * kBlockWaves), 0, st, a);
  return Plan::ok;
}

// the uniform-tile form (see fwd_kernel): dense rows whose 16-row tiles are one ray each,
// 4 colour outputs in 16-byte aligned rows, byte offsets of the outputs (`out_bytes` per
// element) below 2^31. S <= 4 <= color_stride: the sigma offsets stay below the colour rows'.
static bool fwd_uniform(const Args& a, int out_bytes) {
  return g_fwd_ut && a.rows == nullptr && a.n_per_ray % 16 == 0 && a.n_out == 4 &&
         (a.color_stride & 3) == 0 && a.M * a.color_stride * out_bytes < (int64_t{1} << 31);
}

template <int W, int NHD, bool BF, int S>
static Plan plan_fwd(const Args& a, hipStream_t st) {
  const bool ho = a.color_h != nullptr;  // f16 outputs (same grid as the f32 form)
  if ((ho && a.rows) || (S > 1 && (ho || a.rows))) return Plan::no_kernel;
  const bool ut = fwd_uniform(a, ho ? 2 : 4);
  const FieldKernel general = fwd_kernel<W, NHD, false, BF, false, false, S>;
  FieldKernel k = ut ? fwd_kernel<W, NHD, false, BF, true, false, S> : general;
  if constexpr (S == 1) {
    if (ho)
      k = ut ? fwd_kernel<W, NHD, false, BF, true, true> : fwd_kernel<W, NHD, false, BF, false, true>;
    else if (a.rows)
      k = fwd_kernel<W, NHD, true, BF, false>;
  }
  // every forward form runs the grid of the general f32 one
  return launch_tiles16(
      k, resident_blocks(reinterpret_cast<const void*>(general), 64 * kBlockWaves), a, st);
}

template <int W, int NHD, bool BF, int S>
static Plan plan_density(const Args& a, hipStream_t st) {
  // 8 blocks (32 waves) per CU, grid-stride
  return launch_tiles16(density_kernel<W, NHD, BF, S>, 8 * device_cus(), a, st);
}

// Backward launch geometry: one resident wavefront per slot (4 per block), each owning a
// contiguous range of 32-sample tiles. The f16 backward needs one float per wavefront of
// caller-owned workspace for the gradient maxima; bf16 needs none.
struct BwdGeom {
  int64_t blocks, nw, tpw;
};
// the grid of the 4-wave backward kernel `fn` over M rows
static BwdGeom tile_geom(int64_t M, BwdKernel fn) {
  const int64_t tiles = (M + 31) / 32;
  const int64_t blocks = persistent_blocks(
      (tiles + kBlockWaves - 1) / kBlockWaves,
      resident_blocks(reinterpret_cast<const void*>(fn), 64 * kBlockWaves));
  const int64_t nw = blocks * kBlockWaves;
  return {blocks, nw, (tiles + nw - 1) / nw};
}
// the kernel of form Fast or General, by the d_color layout
template <int W, int NHD, bool BF, int S, typename Fast, typename General>
static BwdKernel bwd_kernel(bool fast) {
  static_assert(Fast::FAST && !General::FAST, "the two d_color layouts of one form");
  return fast ? bwd_rt_kernel<W, NHD, BF, S, Fast> : bwd_rt_kernel<W, NHD, BF, S, General>;
}
// every whole-network form of one d_color layout (fast or general) runs the grid of its
// Build, dense-rows instantiation
template <int W, int NHD, bool BF, int S>
static BwdGeom bwd_geom(int64_t M, bool fast) {
  return tile_geom(M, bwd_kernel<W, NHD, BF, S, Build<FastColor, DenseRows>,
                                 Build<GeneralColor, DenseRows>>(fast));
}

template <int W, int NHD, bool BF, int S>
static int64_t bwd_workspace(int64_t M) {
  if (BF || M <= 0) return 0;
  // the larger wave count of the fast and general d_color layouts, so a workspace sized
  // once serves whichever runs
  int64_t n = 0;
  for (int f = 0; f < 2; ++f) {
    const int64_t w = bwd_geom<W, NHD, BF, S>(M, f == 1).nw;
    n = w > n ? w : n;
  }
  return static_cast<int64_t>(sizeof(float)) * n;
}

static void launch_bwd(BwdKernel k, int64_t blocks, const Args& a, float target, int64_t tpw,
                       const float* wmax, hipStream_t st) {
  hipLaunchKernelGGL(k, dim3(static_cast<unsigned>(blocks)), dim3(64 * kBlockWaves), 0, st, a, target,
                     tpw, wmax);
}

// reference numerics, f16 (Grads = F16Grads) or f32 incoming gradients
template <int W, int NHD, typename Grads>
static Plan plan_bwd_ref(const Args& a, bool fast, hipStream_t st) {
  if (a.d_enc_h && fast && a.tile_list) {
    // the pos pass over every tile, on a grid of its own occupancy (more waves per SIMD: no
    // dir network's registers or LDS sums in it), then the list pass over the tiles it left
    // (nonzero dL/dcolor), at most one per wavefront of a grid of its occupancy
    const BwdKernel pos = bwd_rt_kernel<W, NHD, false, 1, PosPass<Grads>>;
    const BwdKernel list = bwd_rt_kernel<W, NHD, false, 1, ListPass<Grads>>;
    const BwdGeom pg = tile_geom(a.M, pos);
    if (hipMemsetAsync(a.tile_count, 0, sizeof(uint32_t), st) != hipSuccess)
      return Plan::no_kernel;
    launch_bwd(pos, pg.blocks, a, 0.0f, pg.tpw, nullptr, st);
    launch_bwd(list, resident_blocks(reinterpret_cast<const void*>(list), 64 * kBlockWaves), a, 0.0f,
               0, nullptr, st);
    return Plan::ok;
  }
  BwdKernel k = nullptr;
  if (a.d_enc_h)  // f16 rows and row bits
    k = bwd_kernel<W, NHD, false, 1, RefF16Rows<FastColor, Grads>,
                   RefF16Rows<GeneralColor, Grads>>(fast);
  else if constexpr (!Grads::value)  // f32 rows
    k = bwd_kernel<W, NHD, false, 1, RefF32Rows<FastColor>, RefF32Rows<GeneralColor>>(fast);
  if (!k) return Plan::no_kernel;  // f16 gradients come with f16 rows only
  const BwdGeom gm = bwd_geom<W, NHD, false, 1>(a.M, fast);
  launch_bwd(k, gm.blocks, a, 0.0f, gm.tpw, nullptr, st);
  return Plan::ok;
}

template <int W, int NHD, bool BF, int S>
static Plan plan_bwd(const Args& a, float* ws, int64_t ws_bytes, hipStream_t st) {
  using N = Net<W, NHD, S>;
  const bool hg = a.d_color_h != nullptr;  // f16 gradients (the f16-rows forms only)
  const bool ref = a.loss_scale > 0.0f;
  const bool fast = a.n_out == 4 && (a.d_color_stride & 3) == 0 &&
                    (hg ? a.d_sigma_h != nullptr : a.d_sigma != nullptr);
  if (S > 1 && (a.rows || hg || ref)) return Plan::no_kernel;
  if (ref) {
    if constexpr (BF || S > 1) {
      return Plan::no_kernel;
    } else {
      if (a.rows) return Plan::no_kernel;
      return hg ? plan_bwd_ref<W, NHD, F16Grads>(a, fast, st)
                : plan_bwd_ref<W, NHD, F32Grads>(a, fast, st);
    }
  }
  // build numerics: the wavefronts' gradient maxima (f16 only), then the fast or general kernel
  const size_t lds = static_cast<size_t>(N::n_packed) * 2 + sizeof(float) * (N::NPOS + N::NDIR);
  if (lds > 160 * 1024) return Plan::no_kernel;
  const BwdGeom gm = bwd_geom<W, NHD, BF, S>(a.M, fast);
  if (!BF && (ws == nullptr || ws_bytes < static_cast<int64_t>(sizeof(float)) * gm.nw))
    return Plan::workspace;
  void (*amax)(Args, int64_t, float*) = absmax_kernel<false, S>;
  BwdKernel k = bwd_kernel<W, NHD, BF, S, Build<FastColor, DenseRows>,
                           Build<GeneralColor, DenseRows>>(fast);
  if constexpr (S == 1) {
    if (a.rows) {
      amax = absmax_kernel<true>;
      k = bwd_kernel<W, NHD, BF, 1, Build<FastColor, GatheredRows>,
                     Build<GeneralColor, GatheredRows>>(fast);
    }
  }
  if (!BF) hipLaunchKernelGGL(amax, dim3(gm.nw), dim3(1024), 0, st, a, gm.tpw * 32, ws);
  launch_bwd(k, gm.blocks, a, ldexpf(1.0f, g_target_log2), gm.tpw, ws, st);
  return Plan::ok;
}

// Density outputs S of a dir network: its 20 - S inputs are SH2 (4) and pos_out[S:16]
// (multi_band_extinction: S = num_bands; 1 otherwise). Meaningful once variant() != 0.
static int n_sigma(const anr_mlp_desc* dir) { return 20 - dir->n_input; }

// 10 W + NHD of a supported pos/dir pair (with_net's list), or 0
static int variant(const anr_mlp_desc* pos, const anr_mlp_desc* dir) {
  if (!pos || !dir) return 0;
  if (pos->n_input != 32 || pos->n_input_padded != 32 || pos->n_output != 16 ||
      pos->n_output_padded != 16 || pos->n_hidden_layers != 1 ||
      pos->output_activation != ANR_ACT_NONE)
    return 0;
  if (dir->n_input < 16 || dir->n_input > 19 ||
      dir->n_input_padded != (dir->n_input + 15) / 16 * 16 || dir->n_output < 1 || dir->n_output > 16 ||
      dir->n_output_padded != 16 || dir->width != pos->width ||
      (dir->n_hidden_layers != 1 && dir->n_hidden_layers != 2))
    return 0;
  if (pos->width != 32 && pos->width != 64) return 0;
  return pos->width * 10 + dir->n_hidden_layers;
}

// fused hash-grid + field forward: a persistent grid of HF_WAVES-wavefront blocks, as many
// as the device holds at once, each wavefront walking 64-sample segments grid-stride
constexpr int HF_WAVES = 8;
// register cap of the fused forward: 6 waves per SIMD. It runs without run-leader gathers
// (plane_quad's LEADERS off): with them it measured 0.74-0.79 ms at caps of 4, 5 and 6 against 0.64-0.65 ms
// without (profiles/r06_hash_field_fwd_variants.log).
constexpr int HF_OCC = 6;
template <int W, int NHD, bool BF>
static Plan plan_hf(const Args& a, const HashArgs& h, hipStream_t st) {
  const auto k = hf_fwd_kernel<W, NHD, BF, HF_WAVES, HF_OCC>;
  const int64_t n_super = (a.M + 63) / 64;
  const int64_t blocks =
      persistent_blocks((n_super + HF_WAVES - 1) / HF_WAVES,
                        resident_blocks(reinterpret_cast<const void*>(k), 64 * HF_WAVES));
  hipLaunchKernelGGL(k, dim3(blocks), dim3(64 * HF_WAVES), 0, st, a, h);
  return Plan::ok;
}

// forward-only render: a persistent grid of RN_WAVES-wavefront blocks, as many as the device
// holds at once, a wavefront per ray
constexpr int RN_WAVES = 8;
constexpr int RN_OCC = 4;
template <int W, int NHD, bool BF, bool REF>
static Plan plan_render(const Args& a, const HashArgs& h, const RenderArgs& r, hipStream_t st) {
  const auto k = render_kernel<W, NHD, BF, REF, RN_WAVES, RN_OCC>;
  const int64_t blocks =
      persistent_blocks((r.B + RN_WAVES - 1) / RN_WAVES,
                        resident_blocks(reinterpret_cast<const void*>(k), 64 * RN_WAVES));
  hipLaunchKernelGGL(k, dim3(blocks), dim3(64 * RN_WAVES), 0, st, a, h, r);
  return Plan::ok;
}

// Entry points that stay at one density output answer a multi-band pair with this.
static bool multi_band(const anr_mlp_desc* pos, const anr_mlp_desc* dir) {
  return variant(pos, dir) != 0 && n_sigma(dir) > 1;
}
static int refuse_bands(const char* entry) {
  ::anr::set_error("%s: unsupported for a dir network with more than one density output "
                   "(multi_band_extinction): anr_ingp_field_fwd / _density / _bwd take it", entry);
  return ANR_E_UNSUPPORTED;
}

}  // namespace field
}  // namespace anr

using namespace anr::field;

extern "C" int anr_ingp_field_supported(const anr_mlp_desc* pos, const anr_mlp_desc* dir) {
  return variant(pos, dir) != 0;
}

extern "C" int64_t anr_ingp_field_packed_size(const anr_mlp_desc* pos, const anr_mlp_desc* dir) {
  return with_net(variant(pos, dir), int64_t{0},
                  [](auto net) { return int64_t{Net<net.W, net.NHD>::n_packed}; });
}

extern "C" int64_t anr_ingp_field_bwd_workspace_bytes(const anr_mlp_desc* pos,
                                                      const anr_mlp_desc* dir,
                                                      int32_t mma_dtype, int64_t M) {
  const int v = variant(pos, dir);
  if (v == 0) return 0;
  return with_variant(v, n_sigma(dir), mma_dtype == ANR_BF16, int64_t{0},
                      [&](auto net, auto s, auto bf) {
                        return bwd_workspace<net.W, net.NHD, bf(), s()>(M);
                      });
}

extern "C" int anr_ingp_field_force_fwd(int32_t mode) {
  const int prev = g_fwd_ut;
  if (mode == 0 || mode == 1) g_fwd_ut = mode;
  return prev;
}

extern "C" int anr_ingp_field_set_grad_scale(int32_t log2_target) {
  const int prev = g_target_log2;
  g_target_log2 = log2_target;
  return prev;
}

static bool mma_ok(int32_t t) { return t == ANR_F16 || t == ANR_BF16; }
static bool aligned(const void* p, uintptr_t bytes) {
  return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0;
}
// S > 1: a row's S densities leave (arrive) as one access of 4 S bytes, 4 for S = 3
static int band_align(int ns) { return ns == 3 ? 4 : 4 * ns; }

// enc_stride >= 32 (multiple of 8): row layout; enc_stride = -P: level-quad planes of P
// f16 elements each (P >= 8 M, multiple of 8), as anr_hashgrid_fwd_planes writes them
static bool set_enc(Args& a, const void* enc, int64_t enc_stride, int64_t M) {
  a.enc = static_cast<const _Float16*>(enc);
  if (enc_stride >= 32 && enc_stride % 8 == 0) {
    a.enc_stride = enc_stride;
    a.enc_gstride = 8;
    return true;
  }
  if (enc_stride < 0 && -enc_stride >= 8 * M && (-enc_stride) % 8 == 0) {
    a.enc_stride = 8;
    a.enc_gstride = -enc_stride;
    return true;
  }
  return false;
}

extern "C" int anr_ingp_field_pack(const anr_mlp_desc* pos, const anr_mlp_desc* dir,
                                   int32_t mma_dtype, const float* pos_params,
                                   const float* dir_params, void* packed, anr_stream_t stream) {
  const int v = variant(pos, dir);
  ANR_CHECK_ARG(v != 0, "anr_ingp_field_pack: unsupported pos/dir MLP pair");
  ANR_CHECK_ARG(mma_ok(mma_dtype), "anr_ingp_field_pack: mma_dtype must be ANR_F16 or ANR_BF16");
  ANR_CHECK_ARG(pos_params && dir_params && packed, "anr_ingp_field_pack: null pointer");
  with_variant(v, n_sigma(dir), mma_dtype == ANR_BF16, 0, [&](auto net, auto s, auto bf) {
    hipLaunchKernelGGL((pack_kernel<net.W, net.NHD, bf(), s()>),
                       dim3((Net<net.W, net.NHD>::n_packed + 255) / 256), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), pos_params, dir_params,
                       static_cast<_Float16*>(packed));
    return 0;
  });
  ANR_CHECK_LAUNCH("anr_ingp_field_pack");
  return ANR_OK;
}

// what only some forward entries pass; zero: absent
struct FwdForm {
  const int32_t* rows;  // anr_ingp_field_fwd_rows
  bool half_out;        // anr_ingp_field_fwd_h: sigma and color are f16
};

static int field_fwd(const anr_mlp_desc* pos, const anr_mlp_desc* dir, int32_t mma_dtype,
                     const void* packed, const void* enc, int64_t enc_stride, const float* dirs,
                     int64_t n_per_ray, int64_t M, void* sigma, void* color,
                     int64_t color_stride, anr_stream_t stream, const FwdForm& f) {
  const int v = variant(pos, dir);
  ANR_CHECK_ARG(v != 0, "anr_ingp_field_fwd: unsupported pos/dir MLP pair");
  ANR_CHECK_ARG(mma_ok(mma_dtype), "anr_ingp_field_fwd: mma_dtype must be ANR_F16 or ANR_BF16");
  ANR_CHECK_ARG(M >= 0 && M < (1LL << 31), "anr_ingp_field_fwd: bad M");
  if (M == 0) return ANR_OK;
  const int ns = n_sigma(dir);
  if (ns > 1 && (f.half_out || f.rows))
    return refuse_bands(f.half_out ? "anr_ingp_field_fwd_h" : "anr_ingp_field_fwd_rows");
  ANR_CHECK_ARG(packed && enc && dirs && sigma && color, "anr_ingp_field_fwd: null pointer");
  ANR_CHECK_ARG(ns == 1 || aligned(sigma, band_align(ns)),
                "anr_ingp_field_fwd: sigma (M, %d) must be %d-byte aligned", ns, band_align(ns));
  ANR_CHECK_ARG(n_per_ray >= 1 && n_per_ray < (1LL << 31) && color_stride >= dir->n_output,
                "anr_ingp_field_fwd: bad shape/stride");
  ANR_CHECK_ARG(aligned(enc, 16) && aligned(packed, 16),
                "anr_ingp_field_fwd: enc/packed must be 16-byte aligned");
  Args a{};
  a.packed = static_cast<const _Float16*>(packed);
  ANR_CHECK_ARG(set_enc(a, enc, enc_stride, M),
                "anr_ingp_field: bad enc_stride %lld (>= 32, multiple of 8: rows; -P: level-quad "
                "planes of P >= 8 M)", (long long)enc_stride);
  a.dirs = dirs;
  a.n_per_ray = static_cast<uint32_t>(n_per_ray);
  a.M = M;
  a.n_out = dir->n_output;
  if (f.half_out) {
    ANR_CHECK_ARG(f.rows == nullptr, "anr_ingp_field_fwd_h: dense rows only");
    // 4-wide colour rows go out as one 8-byte store
    ANR_CHECK_ARG((color_stride & 3) != 0 || aligned(color, 8),
                  "anr_ingp_field_fwd_h: color must be 8-byte aligned");
    a.sigma_h = static_cast<_Float16*>(sigma);
    a.color_h = static_cast<_Float16*>(color);
  } else {
    a.sigma = static_cast<float*>(sigma);
    a.color = static_cast<float*>(color);
  }
  a.color_stride = color_stride;
  a.rows = f.rows;
  const Plan rc = with_variant(v, ns, mma_dtype == ANR_BF16, Plan::no_kernel,
                               [&](auto net, auto s, auto bf) {
                                 return plan_fwd<net.W, net.NHD, bf(), s()>(
                                     a, reinterpret_cast<hipStream_t>(stream));
                               });
  ANR_CHECK_ARG(rc == Plan::ok, "anr_ingp_field_fwd: no kernel for this shape");
  ANR_CHECK_LAUNCH("anr_ingp_field_fwd");
  return ANR_OK;
}

// The configuration the hash+field forward and the render take (v: variant() of the pair).
static bool hash_field_config(const anr_hashgrid_desc* grid, int32_t table_dtype, int v,
                              const anr_mlp_desc* dir, int32_t mma_dtype, int64_t n_per_ray) {
  return v != 0 && mma_ok(mma_dtype) && table_dtype == ANR_F16 && grid->n_dims == 3 &&
         grid->n_features == 2 && grid->n_levels == 16 && dir->n_output == 4 && n_per_ray >= 64 &&
         n_per_ray % 64 == 0;
}
// Their shared arguments: M samples x of rays of n_per_ray, the table and the field. False
// when the byte range of x (with a segment's overrun) or of the table reaches 2^31.
static bool set_hash_field(Args& a, HashArgs& h, const ::anr::GridLevels& G, const float* x,
                           int64_t M, const void* table, const void* packed, const float* dirs,
                           int64_t n_per_ray) {
  const int64_t lim = int64_t(1) << 31;
  const int64_t t_bytes = static_cast<int64_t>(G.offset[15] + G.size[15]) * 4;
  if ((M + 64) * 12 >= lim || t_bytes >= lim) return false;
  a.packed = static_cast<const _Float16*>(packed);
  a.dirs = dirs;
  a.n_per_ray = static_cast<uint32_t>(n_per_ray);
  a.M = M;
  a.n_out = 4;
  h.G = G;
  h.x = x;
  h.x_bytes = static_cast<uint32_t>(M * 12);
  h.table = static_cast<const __half*>(table);
  h.table_bytes = static_cast<uint32_t>(t_bytes);
  return true;
}

extern "C" int anr_ingp_hash_field_fwd(const anr_hashgrid_desc* grid, const float* x, int64_t M,
                                      const void* table, int32_t table_dtype, void* planes,
                                      int64_t plane_stride, const anr_mlp_desc* pos,
                                      const anr_mlp_desc* dir, int32_t mma_dtype,
                                      const void* packed, const float* dirs, int64_t n_per_ray,
                                      float* sigma, float* color, int64_t color_stride,
                                      anr_stream_t stream) {
  const int v = variant(pos, dir);
  if (M == 0) return ANR_OK;
  if (v != 0 && n_sigma(dir) > 1) return refuse_bands("anr_ingp_hash_field_fwd");
  ANR_CHECK_ARG(grid && x && table && planes && packed && dirs && sigma && color,
                "anr_ingp_hash_field_fwd: null pointer");
  if (!hash_field_config(grid, table_dtype, v, dir, mma_dtype, n_per_ray) || color_stride < 4 ||
      color_stride % 4 != 0) {
    ::anr::set_error("anr_ingp_hash_field_fwd: unsupported configuration (3-D f16 grid of 16 "
                     "levels x 2 features, a supported field pair with 4 colour outputs, "
                     "samples per ray a multiple of 64, colour rows 16-byte aligned)");
    return ANR_E_UNSUPPORTED;
  }
  ANR_CHECK_ARG(M > 0 && plane_stride >= 8 * M && plane_stride % 8 == 0,
                "anr_ingp_hash_field_fwd: bad M / plane_stride (>= 8 M, multiple of 8)");
  ANR_CHECK_ARG(aligned(planes, 16) && aligned(packed, 16) && aligned(color, 16),
                "anr_ingp_hash_field_fwd: planes / packed / color must be 16-byte aligned");
  ::anr::GridLevels G;
  ANR_CHECK_ARG(::anr::make_levels(grid, &G), "anr_ingp_hash_field_fwd: descriptor not initialised");
  const int64_t lim = int64_t(1) << 31;
  const int64_t o_bytes = (3 * plane_stride + 8 * M) * 2;
  Args a{};
  HashArgs h{};
  ANR_CHECK_ARG(set_hash_field(a, h, G, x, M, table, packed, dirs, n_per_ray) && o_bytes < lim &&
                    plane_stride * 2 < lim && M * color_stride * 4 < lim,
                "anr_ingp_hash_field_fwd: byte ranges must stay below 2^31");
  a.sigma = sigma;
  a.color = color;
  a.color_stride = color_stride;
  h.planes = static_cast<_Float16*>(planes);
  h.plane_bytes = static_cast<uint32_t>(plane_stride * 2);
  h.out_bytes = static_cast<uint32_t>(o_bytes);
  const Plan rc = with_net(v, Plan::no_kernel, [&](auto net) {
    return with_bool(mma_dtype == ANR_BF16, [&](auto bf) {
      return plan_hf<net.W, net.NHD, bf()>(a, h, reinterpret_cast<hipStream_t>(stream));
    });
  });
  ANR_CHECK_ARG(rc == Plan::ok, "anr_ingp_hash_field_fwd: no kernel for this shape");
  ANR_CHECK_LAUNCH("anr_ingp_hash_field_fwd");
  return ANR_OK;
}

extern "C" int anr_ingp_render(const anr_hashgrid_desc* grid, const float* coords, const float* z,
                               const float* dirs, int64_t B, int64_t n_per_ray, const void* table,
                               int32_t table_dtype, const anr_mlp_desc* pos,
                               const anr_mlp_desc* dir, int32_t mma_dtype, const void* packed,
                               const void* color_surf, float z_scale, int32_t numerics,
                               void* color_map, void* atmo, void* surf, anr_stream_t stream) {
  ANR_CHECK_ARG(B >= 0, "anr_ingp_render: bad B");
  if (B == 0) return ANR_OK;
  ANR_CHECK_ARG(grid && coords && z && dirs && table && pos && dir && packed && color_map,
                "anr_ingp_render: null pointer (color_surf, atmo and surf may be null)");
  ANR_CHECK_ARG(numerics == ANR_RENDER_BUILD || numerics == ANR_RENDER_REFERENCE,
                "anr_ingp_render: numerics must be ANR_RENDER_BUILD or ANR_RENDER_REFERENCE");
  const int v = variant(pos, dir);
  if (v != 0 && n_sigma(dir) > 1) return refuse_bands("anr_ingp_render");
  if (!hash_field_config(grid, table_dtype, v, dir, mma_dtype, n_per_ray)) {
    ::anr::set_error("anr_ingp_render: unsupported configuration (3-D f16 grid of 16 levels x 2 "
                     "features, a supported field pair with one density and 4 colour outputs, "
                     "f16 or bf16 MFMA, samples per ray a positive multiple of 64)");
    return ANR_E_UNSUPPORTED;
  }
  if (!aligned(packed, 16)) {
    ::anr::set_error("anr_ingp_render: unsupported: packed weights must be 16-byte aligned");
    return ANR_E_UNSUPPORTED;
  }
  ::anr::GridLevels G;
  ANR_CHECK_ARG(::anr::make_levels(grid, &G), "anr_ingp_render: descriptor not initialised");
  const int64_t lim = int64_t(1) << 31;
  Args a{};
  HashArgs h{};
  if (n_per_ray >= lim || B >= lim / n_per_ray ||
      !set_hash_field(a, h, G, coords, B * n_per_ray, table, packed, dirs, n_per_ray)) {
    ::anr::set_error("anr_ingp_render: unsupported: byte ranges must stay below 2^31");
    return ANR_E_UNSUPPORTED;
  }
  RenderArgs r{};
  r.z = z;
  r.zs = z_scale;
  r.cs = color_surf;
  r.cmap = color_map;
  r.atmo = atmo;
  r.surf = surf;
  r.B = B;
  const Plan rc = with_net(v, Plan::no_kernel, [&](auto net) {
    return with_bool(mma_dtype == ANR_BF16, [&](auto bf) {
      return with_bool(numerics == ANR_RENDER_REFERENCE, [&](auto ref) {
        return plan_render<net.W, net.NHD, bf(), ref()>(a, h, r,
                                                        reinterpret_cast<hipStream_t>(stream));
      });
    });
  });
  ANR_CHECK_ARG(rc == Plan::ok, "anr_ingp_render: no kernel for this shape");
  ANR_CHECK_LAUNCH("anr_ingp_render");
  return ANR_OK;
}

// what only some backward entries pass; zero: absent
struct BwdForm {
  const int32_t* rows;      // anr_ingp_field_bwd_rows
  float loss_scale;         // > 0: reference numerics (the ref16 entries)
  uint8_t* tile_nz;         // _ref16_tiles
  void* d_enc_h;            // _ref16_rows: dL/denc as f16 rows (d_enc null), with
  uint32_t* row_nz;         //   the row bits
  void* tiles_ws;           //   and the pos / list passes' workspace (nullable)
  bool half_grad;           // _ref16_rows_h: d_sigma and d_color are f16
  void* workspace;          // build numerics: the wavefronts' gradient maxima
  int64_t workspace_bytes;
};

static int field_bwd(const anr_mlp_desc* pos, const anr_mlp_desc* dir, int32_t mma_dtype,
                     const void* packed, const void* enc, int64_t enc_stride, const float* dirs,
                     int64_t n_per_ray, int64_t M, const void* d_sigma, const void* d_color,
                     int64_t d_color_stride, float* d_enc, int64_t d_enc_stride, float* g_pos,
                     float* g_dir, anr_stream_t stream, const BwdForm& f) {
  const int v = variant(pos, dir);
  ANR_CHECK_ARG(v != 0, "anr_ingp_field_bwd: unsupported pos/dir MLP pair");
  ANR_CHECK_ARG(f.loss_scale == 0.0f ||
                    (f.loss_scale > 0.0f && mma_dtype == ANR_F16 && f.rows == nullptr),
                "anr_ingp_field_bwd: reference numerics need f16 MMA and dense rows");
  ANR_CHECK_ARG(mma_ok(mma_dtype), "anr_ingp_field_bwd: mma_dtype must be ANR_F16 or ANR_BF16");
  ANR_CHECK_ARG(M >= 0 && M < (1LL << 31), "anr_ingp_field_bwd: bad M");
  if (M == 0) return ANR_OK;
  const int ns = n_sigma(dir);
  if (ns > 1 && (f.loss_scale > 0.0f || f.rows))
    return refuse_bands(f.rows ? "anr_ingp_field_bwd_rows" : "anr_ingp_field_bwd_ref16");
  ANR_CHECK_ARG(packed && enc && dirs && d_color && (d_enc || (f.d_enc_h && f.row_nz)) && g_pos &&
                    g_dir,
                "anr_ingp_field_bwd: null pointer");
  ANR_CHECK_ARG(ns == 1 || aligned(d_sigma, band_align(ns)),
                "anr_ingp_field_bwd: d_sigma (M, %d) must be %d-byte aligned", ns, band_align(ns));
  ANR_CHECK_ARG(f.d_enc_h == nullptr || f.loss_scale > 0.0f,
                "anr_ingp_field_bwd: f16 rows and row bits are reference numerics only");
  ANR_CHECK_ARG(n_per_ray >= 1 && n_per_ray < (1LL << 31) && d_color_stride >= dir->n_output &&
                    d_enc_stride >= 32 && d_enc_stride % 4 == 0,
                "anr_ingp_field_bwd: bad shape/stride");
  ANR_CHECK_ARG(aligned(enc, 16) && aligned(packed, 16) && aligned(d_enc, 16) &&
                    aligned(f.d_enc_h, 8),
                "anr_ingp_field_bwd: enc/packed/d_enc must be 16-byte aligned (f16 rows: 8)");
  Args a{};
  a.packed = static_cast<const _Float16*>(packed);
  ANR_CHECK_ARG(set_enc(a, enc, enc_stride, M),
                "anr_ingp_field: bad enc_stride %lld (>= 32, multiple of 8: rows; -P: level-quad "
                "planes of P >= 8 M)", (long long)enc_stride);
  a.dirs = dirs;
  a.n_per_ray = static_cast<uint32_t>(n_per_ray);
  a.M = M;
  a.n_out = dir->n_output;
  if (f.half_grad) {  // f16 dL/dsigma, dL/dcolor: 4-wide rows are read as one 8-byte load
    ANR_CHECK_ARG(f.d_enc_h != nullptr, "anr_ingp_field_bwd: f16 gradients need the f16-rows form");
    ANR_CHECK_ARG((d_color_stride & 3) != 0 || aligned(d_color, 8),
                  "anr_ingp_field_bwd: f16 d_color must be 8-byte aligned");
    a.d_sigma_h = static_cast<const _Float16*>(d_sigma);
    a.d_color_h = static_cast<const _Float16*>(d_color);
  } else {
    a.d_sigma = static_cast<const float*>(d_sigma);
    a.d_color = static_cast<const float*>(d_color);
  }
  a.d_color_stride = d_color_stride;
  a.d_enc = d_enc;
  a.d_enc_stride = d_enc_stride;
  a.g_pos = g_pos;
  a.g_dir = g_dir;
  a.rows = f.rows;
  a.loss_scale = f.loss_scale;
  a.tile_nz = f.tile_nz;
  a.d_enc_h = static_cast<_Float16*>(f.d_enc_h);
  a.row_nz = f.row_nz;
  if (f.tiles_ws) {  // ref16_rows_workspace_bytes: the count, then one int32 per 32-row tile
    a.tile_count = static_cast<uint32_t*>(f.tiles_ws);
    a.tile_list = reinterpret_cast<int32_t*>(static_cast<char*>(f.tiles_ws) + 256);
  }
  const Plan rc = with_variant(v, ns, mma_dtype == ANR_BF16, Plan::no_kernel,
                               [&](auto net, auto s, auto bf) {
                                 return plan_bwd<net.W, net.NHD, bf(), s()>(
                                     a, static_cast<float*>(f.workspace), f.workspace_bytes,
                                     reinterpret_cast<hipStream_t>(stream));
                               });
  ANR_CHECK_ARG(rc != Plan::workspace,
                "anr_ingp_field_bwd: workspace missing or smaller than "
                "anr_ingp_field_bwd_workspace_bytes()");
  ANR_CHECK_ARG(rc == Plan::ok, "anr_ingp_field_bwd: no kernel for this shape");
  ANR_CHECK_LAUNCH("anr_ingp_field_bwd");
  return ANR_OK;
}

extern "C" int anr_ingp_field_fwd(const anr_mlp_desc* pos, const anr_mlp_desc* dir,
                                  int32_t mma_dtype, const void* packed, const void* enc,
                                  int64_t enc_stride, const float* dirs, int64_t n_per_ray,
                                  int64_t M, float* sigma, float* color, int64_t color_stride,
                                  anr_stream_t stream) {
  return field_fwd(pos, dir, mma_dtype, packed, enc, enc_stride, dirs, n_per_ray, M, sigma, color,
                   color_stride, stream, FwdForm{});
}

extern "C" int anr_ingp_field_fwd_h(const anr_mlp_desc* pos, const anr_mlp_desc* dir,
                                    int32_t mma_dtype, const void* packed, const void* enc,
                                    int64_t enc_stride, const float* dirs, int64_t n_per_ray,
                                    int64_t M, void* sigma, void* color, int64_t color_stride,
                                    anr_stream_t stream) {
  FwdForm f{};
  f.half_out = true;
  return field_fwd(pos, dir, mma_dtype, packed, enc, enc_stride, dirs, n_per_ray, M, sigma, color,
                   color_stride, stream, f);
}

extern "C" int anr_ingp_field_density(const anr_mlp_desc* pos, const anr_mlp_desc* dir,
                                      int32_t mma_dtype, const void* packed, const void* enc,
                                      int64_t enc_stride, int64_t M, float* sigma,
                                      anr_stream_t stream) {
  const int v = variant(pos, dir);
  ANR_CHECK_ARG(v != 0, "anr_ingp_field_density: unsupported pos/dir MLP pair");
  ANR_CHECK_ARG(mma_ok(mma_dtype), "anr_ingp_field_density: mma_dtype must be ANR_F16 or ANR_BF16");
  ANR_CHECK_ARG(M >= 0 && M < (1LL << 31), "anr_ingp_field_density: bad M");
  if (M == 0) return ANR_OK;
  ANR_CHECK_ARG(packed && enc && sigma, "anr_ingp_field_density: null pointer");
  const int ns = n_sigma(dir);
  ANR_CHECK_ARG(ns == 1 || aligned(sigma, band_align(ns)),
                "anr_ingp_field_density: sigma (M, %d) must be %d-byte aligned", ns,
                band_align(ns));
  ANR_CHECK_ARG(aligned(enc, 16) && aligned(packed, 16),
                "anr_ingp_field_density: enc/packed must be 16-byte aligned");
  Args a{};
  a.packed = static_cast<const _Float16*>(packed);
  ANR_CHECK_ARG(set_enc(a, enc, enc_stride, M), "anr_ingp_field_density: bad enc_stride");
  a.M = M;
  a.sigma = sigma;
  const Plan rc = with_variant(v, ns, mma_dtype == ANR_BF16, Plan::no_kernel,
                               [&](auto net, auto s, auto bf) {
                                 return plan_density<net.W, net.NHD, bf(), s()>(
                                     a, reinterpret_cast<hipStream_t>(stream));
                               });
  ANR_CHECK_ARG(rc == Plan::ok, "anr_ingp_field_density: no kernel for this shape");
  ANR_CHECK_LAUNCH("anr_ingp_field_density");
  return ANR_OK;
}

extern "C" int anr_ingp_field_bwd(const anr_mlp_desc* pos, const anr_mlp_desc* dir,
                                  int32_t mma_dtype, const void* packed, const void* enc,
                                  int64_t enc_stride, const float* dirs, int64_t n_per_ray,
                                  int64_t M, const float* d_sigma, const float* d_color,
                                  int64_t d_color_stride, float* d_enc, int64_t d_enc_stride,
                                  float* g_pos, float* g_dir, void* workspace,
                                  int64_t workspace_bytes, anr_stream_t stream) {
  BwdForm f{};
  f.workspace = workspace;
  f.workspace_bytes = workspace_bytes;
  return field_bwd(pos, dir, mma_dtype, packed, enc, enc_stride, dirs, n_per_ray, M, d_sigma,
                   d_color, d_color_stride, d_enc, d_enc_stride, g_pos, g_dir, stream, f);
}

extern "C" int anr_ingp_field_bwd_ref16(const anr_mlp_desc* pos, const anr_mlp_desc* dir,
                                        const void* packed, const void* enc, int64_t enc_stride,
                                        const float* dirs, int64_t n_per_ray, int64_t M,
                                        const float* d_sigma, const float* d_color,
                                        int64_t d_color_stride, float* d_enc,
                                        int64_t d_enc_stride, float* g_pos, float* g_dir,
                                        float loss_scale, anr_stream_t stream) {
  if (M != 0 && multi_band(pos, dir)) return refuse_bands("anr_ingp_field_bwd_ref16");
  ANR_CHECK_ARG(loss_scale > 0.0f, "anr_ingp_field_bwd_ref16: loss_scale must be > 0");
  BwdForm f{};
  f.loss_scale = loss_scale;
  return field_bwd(pos, dir, ANR_F16, packed, enc, enc_stride, dirs, n_per_ray, M, d_sigma,
                   d_color, d_color_stride, d_enc, d_enc_stride, g_pos, g_dir, stream, f);
}

extern "C" int anr_ingp_field_bwd_ref16_tiles(const anr_mlp_desc* pos, const anr_mlp_desc* dir,
                                              const void* packed, const void* enc,
                                              int64_t enc_stride, const float* dirs,
                                              int64_t n_per_ray, int64_t M, const float* d_sigma,
                                              const float* d_color, int64_t d_color_stride,
                                              float* d_enc, int64_t d_enc_stride, float* g_pos,
                                              float* g_dir, float loss_scale, uint8_t* tile_nz,
                                              anr_stream_t stream) {
  if (M != 0 && multi_band(pos, dir)) return refuse_bands("anr_ingp_field_bwd_ref16_tiles");
  ANR_CHECK_ARG(loss_scale > 0.0f, "anr_ingp_field_bwd_ref16_tiles: loss_scale must be > 0");
  ANR_CHECK_ARG(tile_nz != nullptr, "anr_ingp_field_bwd_ref16_tiles: null tile_nz");
  BwdForm f{};
  f.loss_scale = loss_scale;
  f.tile_nz = tile_nz;
  return field_bwd(pos, dir, ANR_F16, packed, enc, enc_stride, dirs, n_per_ray, M, d_sigma,
                   d_color, d_color_stride, d_enc, d_enc_stride, g_pos, g_dir, stream, f);
}

extern "C" int64_t anr_ingp_field_bwd_ref16_rows_workspace_bytes(int64_t M) {
  return M <= 0 ? 0 : 256 + 4 * ((M + 31) / 32);
}

// anr_ingp_field_bwd_ref16_rows and _rows_h (half_grad: f16 d_sigma / d_color)
static int field_bwd_ref16_rows(const char* entry, bool half_grad, const anr_mlp_desc* pos,
                                const anr_mlp_desc* dir, const void* packed, const void* enc,
                                int64_t enc_stride, const float* dirs, int64_t n_per_ray,
                                int64_t M, const void* d_sigma, const void* d_color,
                                int64_t d_color_stride, void* d_enc_h, int64_t d_enc_stride,
                                float* g_pos, float* g_dir, float loss_scale, uint32_t* row_nz,
                                void* workspace, int64_t workspace_bytes, anr_stream_t stream) {
  if (M != 0 && multi_band(pos, dir)) return refuse_bands(entry);
  ANR_CHECK_ARG(loss_scale > 0.0f, "%s: loss_scale must be > 0", entry);
  ANR_CHECK_ARG(d_enc_h != nullptr && row_nz != nullptr, "%s: null d_enc / row_nz", entry);
  ANR_CHECK_ARG(workspace == nullptr ||
                    workspace_bytes >= anr_ingp_field_bwd_ref16_rows_workspace_bytes(M),
                "%s: workspace smaller than anr_ingp_field_bwd_ref16_rows_workspace_bytes()",
                entry);
  ANR_CHECK_ARG(aligned(workspace, 256), "%s: workspace must be 256-byte aligned", entry);
  BwdForm f{};
  f.loss_scale = loss_scale;
  f.d_enc_h = d_enc_h;
  f.row_nz = row_nz;
  f.tiles_ws = workspace;
  f.half_grad = half_grad;
  return field_bwd(pos, dir, ANR_F16, packed, enc, enc_stride, dirs, n_per_ray, M, d_sigma,
                   d_color, d_color_stride, nullptr, d_enc_stride, g_pos, g_dir, stream, f);
}

extern "C" int anr_ingp_field_bwd_ref16_rows(const anr_mlp_desc* pos, const anr_mlp_desc* dir,
                                             const void* packed, const void* enc,
                                             int64_t enc_stride, const float* dirs,
                                             int64_t n_per_ray, int64_t M, const float* d_sigma,
                                             const float* d_color, int64_t d_color_stride,
                                             void* d_enc_h, int64_t d_enc_stride, float* g_pos,
                                             float* g_dir, float loss_scale, uint32_t* row_nz,
                                             void* workspace, int64_t workspace_bytes,
                                             anr_stream_t stream) {
  return field_bwd_ref16_rows("anr_ingp_field_bwd_ref16_rows", false, pos, dir, packed, enc,
                              enc_stride, dirs, n_per_ray, M, d_sigma, d_color, d_color_stride,
                              d_enc_h, d_enc_stride, g_pos, g_dir, loss_scale, row_nz, workspace,
                              workspace_bytes, stream);
}

extern "C" int anr_ingp_field_bwd_ref16_rows_h(const anr_mlp_desc* pos, const anr_mlp_desc* dir,
                                               const void* packed, const void* enc,
                                               int64_t enc_stride, const float* dirs,
                                               int64_t n_per_ray, int64_t M, const void* d_sigma,
                                               const void* d_color, int64_t d_color_stride,
                                               void* d_enc_h, int64_t d_enc_stride, float* g_pos,
                                               float* g_dir, float loss_scale, uint32_t* row_nz,
                                               void* workspace, int64_t workspace_bytes,
                                               anr_stream_t stream) {
  return field_bwd_ref16_rows("anr_ingp_field_bwd_ref16_rows_h", true, pos, dir, packed, enc,
                              enc_stride, dirs, n_per_ray, M, d_sigma, d_color, d_color_stride,
                              d_enc_h, d_enc_stride, g_pos, g_dir, loss_scale, row_nz, workspace,
                              workspace_bytes, stream);
}

extern "C" int anr_ingp_field_fwd_rows(const anr_mlp_desc* pos, const anr_mlp_desc* dir,
                                       int32_t mma_dtype, const void* packed, const void* enc,
                                       int64_t enc_stride, const float* dirs, int64_t n_per_ray,
                                       int64_t M, const int32_t* rows, float* sigma,
                                       float* color, int64_t color_stride,
                                       anr_stream_t stream) {
  if (M != 0 && multi_band(pos, dir)) return refuse_bands("anr_ingp_field_fwd_rows");
  ANR_CHECK_ARG(rows || M == 0, "anr_ingp_field_fwd_rows: null rows");
  FwdForm f{};
  f.rows = rows;
  return field_fwd(pos, dir, mma_dtype, packed, enc, enc_stride, dirs, n_per_ray, M, sigma, color,
                   color_stride, stream, f);
}

extern "C" int anr_ingp_field_bwd_rows(const anr_mlp_desc* pos, const anr_mlp_desc* dir,
                                       int32_t mma_dtype, const void* packed, const void* enc,
                                       int64_t enc_stride, const float* dirs, int64_t n_per_ray,
                                       int64_t M, const int32_t* rows, const float* d_sigma,
                                       const float* d_color, int64_t d_color_stride,
                                       float* d_enc, int64_t d_enc_stride, float* g_pos,
                                       float* g_dir, void* workspace, int64_t workspace_bytes,
                                       anr_stream_t stream) {
  if (M != 0 && multi_band(pos, dir)) return refuse_bands("anr_ingp_field_bwd_rows");
  ANR_CHECK_ARG(rows || M == 0, "anr_ingp_field_bwd_rows: null rows");
  BwdForm f{};
  f.rows = rows;
  f.workspace = workspace;
  f.workspace_bytes = workspace_bytes;
  return field_bwd(pos, dir, mma_dtype, packed, enc, enc_stride, dirs, n_per_ray, M, d_sigma,
                   d_color, d_color_stride, d_enc, d_enc_stride, g_pos, g_dir, stream, f);
}

#ifdef FIELD_STAMP
extern "C" int anr_debug_field_stamps(unsigned long long* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(anr::field::g_stamp), sizeof(unsigned long long) * 16) == hipSuccess ? 0 : -1;
}
#endif
