// K3 / K4: multi-resolution hash-grid encoding, forward and backward.
//
// Replaces tinycudann.Encoding(n, {"otype": "HashGrid", ...}) at
// src/atmonr/pipelines/instant_ngp.py:60-63 (3-D positions, called at :163/:236) and the
// 2-D surface grid nested in the surface Composite (:78-80, called at :173).
// Semantics (tiny-cuda-nn GridEncoding; the reference pins no version — see DESIGN.md):
//   scale_l = 2^(l * log2(per_level_scale)) * base_resolution - 1     (f32)
//   res_l   = ceil(scale_l) + 1
//   pos     = fma(scale_l, x, 0.5); cell = floor(pos); w = pos - cell (linear)
//   index   = dense stride index while stride <= T_l, else XOR prime hash; % T_l
//   out[l*F + f] = sum over 2^D corners of prod(w or 1-w) * table[(off_l + index)*F + f]
//
// The per-sample arithmetic (cell split, corner weight, corner indices with the dense wrap,
// coordinate row load) is stated once, in hash_levels.h, and used wherever it leaves the
// machine code in place (DESIGN.md §5 K3/K4 "Forms": the generic v1 kernels spell some of it
// out); grid_index there is the plain definition the others are tested against.
//
// Samples are ray-major, so consecutive samples of a ray usually stay in the same cell of a
// level (always on the coarse levels, ~4 samples per cell on the finest). The walkers (v1,
// v6, v2) put a lane on one level of a CHUNK of K consecutive samples and touch the table
// only when the cell changes; the planes forward (v9) puts a lane on one sample. Which
// kernel serves which entry point:
//
//   entry point                shape                                   kernel
//   anr_hashgrid_fwd_planes    2 features, <= 16 levels, 2-D to 4-D    hashgrid_fwd_planes_kernel
//     (training step, extract)
//   anr_hashgrid_fwd, _runs    2 features, <= 16 levels, 2-D / 3-D,    hashgrid_fwd_v6_kernel
//                              byte ranges below 2^31
//                              every other grid (1/2/4/8 features,     hashgrid_fwd_kernel (v1)
//                              4-D, > 16 levels), or mode 1 / 6
//   anr_hashgrid_bwd           2 features, <= 16 levels, 2-D / 3-D,    hashgrid_bwd_v2_kernel
//                              gradient table below 2 GB:
//                                3-D, strides (3, 32)                    <DenseWalk<3, 32>>
//                                other strides, 2-D, or mode 7           <DenseWalk<0, 0>>
//                              every other grid, or mode 1             hashgrid_bwd_kernel (v1)
//   anr_hashgrid_bwd_rows      the <3, 32> shape with 16 levels        <RowBitsWalk>
//     (training step)          otherwise                               zero_clear_rows_kernel, then
//                                                                      as anr_hashgrid_bwd
//   anr_hashgrid_bwd_tiles     the <3, 32> shape, chunks of whole      <TileMaskWalk>
//                              32-row tiles; otherwise                 as anr_hashgrid_bwd
//   anr_hashgrid_bwd_count_requests   3-D v2 shape                     <CountRequests>
//
// (modes: anr_hashgrid_force_v1, the tests' hook; 0 is the default.) The fused hash + field
// forward and the render kernel (field_fused.hip) run v9's plane_quad inside their own loops.

#include "anr_common.h"
#include "hash_levels.h"

#include <cmath>
#include <initializer_list>
#include <type_traits>
#include <cstdlib>

namespace anr {

// Samples per prefetch batch of the v2 backward walker. 6 rather than 8: the batch's
// scalar coordinates (two batches of 3 x BS SGPRs) spilled 40 SGPRs at 8, 3 at 6; on the
// settled reference-numerics step's own inputs 0.717 -> 0.690 ms (with the max-ILP
// scheduler 0.689; profiles/r05_hash_bwd_variants.log). The tile-mask walk keeps 8.
constexpr int kBwdBatch = 6;
// Samples per coordinate prefetch batch of the forward walkers
constexpr int kFwdBatch = 4;

// Corner addressing for the v2 walkers, where a lane owns the x-offset b and the NC =
// 2^(D-1) corners over dims 1..D-1. The per-dimension components of the cell are formed
// once per cell; corner c then costs an xor (hashed) or add (dense) with compile-time
// component choice after unrolling, and the hashed / dense choice is a select on the
// level's flag, not a branch. The dense wrap (only for points outside [0, 1]) is one
// rarely-taken branch for all corners.
template <int D>
struct LaneCorners {
  static constexpr int NC = 1 << (D - 1);
  // lattice offset bit of corner c (0..NC-1) along dim d >= 1
  __device__ static int bit(int c, int d) { return (c >> (d - 1)) & 1; }
  __device__ static void indices(const LevelIdx<D>& li, const uint32_t* cell, int b,
                                 uint32_t* idx) {
    const uint32_t cx = (cell[0] + static_cast<uint32_t>(b)) * li.mul[0];
    uint32_t c1[2], c2[2] = {0u, 0u};
    c1[0] = cell[1] * li.mul[1];
    c1[1] = c1[0] + li.mul[1];
    if constexpr (D == 3) {
      c2[0] = cell[2] * li.mul[2];
      c2[1] = c2[0] + li.mul[2];
    }
    uint32_t sum[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      uint32_t hx = cx ^ c1[c & 1];
      sum[c] = cx + c1[c & 1];
      if constexpr (D == 3) {
        hx ^= c2[c >> 1];
        sum[c] += c2[c >> 1];
      }
      idx[c] = li.hashed ? (hx & (li.T - 1u)) : sum[c];
    }
    // a dense corner sum can reach T only with a corner on the far face or outside the
    // grid: below that every sum is <= res^D - 1 < T (one test per cell, not per corner;
    // the unsigned max also catches negative cell coordinates). A branch-free form (selects
    // on every flush, the modulo behind one wave-uniform test) measured slower: hash bwd
    // 0.39-0.41 -> 0.45-0.47 ms (profiles/r06_hash_dense_wrap_ab.log)
    uint32_t gm = cell[0] + static_cast<uint32_t>(b);
#pragma unroll
    for (int d = 1; d < D; ++d) gm = gm > cell[d] ? gm : cell[d];
    if (!li.hashed && gm >= li.res1) {
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (!li.hashed && sum[c] >= li.T) {
          const uint32_t s1 = sum[c] - li.T;
          idx[c] = s1 < li.T ? s1 : sum[c] % li.T;
        }
    }
  }
  // A corner with offset o along a dim keeps its lattice point in the new cell iff
  // n = o + (old - new) is 0 or 1; it then becomes corner n there.
  __device__ static bool leaves(int c, const int* dl) {
    // bitwise, not short-circuit: || became a divergent branch (exec save / restore) per
    // corner in the walk's flush
    bool out = static_cast<unsigned>((c & 1) + dl[1]) > 1u;
    if constexpr (D == 3) out = out | (static_cast<unsigned>((c >> 1) + dl[2]) > 1u);
    return out;
  }
  // Carry accumulators onto the new cell's corners, one dimension at a time with
  // compile-time corner structure (dl = old - new per dim; all leave if x moved).
  __device__ static void carry(const float* a, const int* dl, bool keepx, float* n) {
    const int dy = dl[1];
    const bool y0 = dy == 0, ym = dy == -1, yp = dy == 1;
    float t[NC];
#pragma unroll
    for (int z = 0; z < NC / 2; ++z) {
      const float a0 = a[2 * z], a1 = a[2 * z + 1];
      t[2 * z] = y0 ? a0 : (ym ? a1 : 0.0f);
      t[2 * z + 1] = y0 ? a1 : (yp ? a0 : 0.0f);
    }
    if constexpr (D == 3) {
      const int dz = dl[2];
      const bool z0 = dz == 0, zm = dz == -1, zp = dz == 1;
#pragma unroll
      for (int y = 0; y < 2; ++y) {
        n[y] = z0 ? t[y] : (zm ? t[y + 2] : 0.0f);
        n[y + 2] = z0 ? t[y + 2] : (zp ? t[y] : 0.0f);
      }
    } else {
      n[0] = t[0];
      n[1] = t[1];
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) n[c] = keepx ? n[c] : 0.0f;
  }
};

template <typename T, int F>
struct Vec {
  __device__ static void load(const T* p, float* v) {
#pragma unroll
    for (int f = 0; f < F; ++f) v[f] = to_f32<T>(p[f]);
  }
};
template <>
struct Vec<__half, 2> {
  __device__ static void load(const __half* p, float* v) {
    const __half2 h = *reinterpret_cast<const __half2*>(p);
    const float2 f = __half22float2(h);
    v[0] = f.x;
    v[1] = f.y;
  }
};
template <>
struct Vec<float, 2> {
  __device__ static void load(const float* p, float* v) {
    const float2 f = *reinterpret_cast<const float2*>(p);
    v[0] = f.x;
    v[1] = f.y;
  }
};

template <typename TO, int F>
__device__ __forceinline__ void store_feat(TO* p, const float* v) {
#pragma unroll
  for (int f = 0; f < F; ++f) p[f] = from_f32<TO>(v[f]);
}
template <>
__device__ __forceinline__ void store_feat<__half, 2>(__half* p, const float* v) {
  *reinterpret_cast<__half2*>(p) = __floats2half2_rn(v[0], v[1]);
}

// A wavefront serves lpw consecutive levels (lane % lpw) of 64/lpw chunks (lane / lpw);
// wavefronts cycle through the n_groups level groups of a block of chunks. Grouping few
// levels per wave keeps the divergent gather path to the waves whose levels actually
// change cell (fine levels: often; coarse levels: almost never).
template <int D, int F, typename TT, typename TO>
__global__ void __launch_bounds__(256) hashgrid_fwd_kernel(
    GridLevels G, int n_levels, int lpw, int n_groups, const float* __restrict__ x,
    int64_t x_stride, int64_t M, int64_t K, const TT* __restrict__ table,
    TO* __restrict__ out, int64_t out_stride) {
  // level group = block index mod n_groups: consecutive blocks go to different XCDs
  // (round-robin dispatch), so with n_groups = 8 each XCD's L2 serves the table slice of
  // its own levels only (speed only; any block placement gives the same result)
  const int lane = static_cast<int>(threadIdx.x & 63);
  const int lg = static_cast<int>(blockIdx.x % n_groups);
  const int64_t wave_in = (static_cast<int64_t>(blockIdx.x / n_groups) * blockDim.x + threadIdx.x) >> 6;
  const int64_t chunk = wave_in * (64 / lpw) + lane / lpw;
  const int level = lg * lpw + lane % lpw;
  const int64_t m0 = chunk * K;
  if (level >= n_levels || m0 >= M) return;
  const int64_t m1 = m0 + K < M ? m0 + K : M;

  const float scale = G.scale[level];
  const uint32_t res = G.res[level];
  const uint32_t T = G.size[level];
  const TT* __restrict__ grid = table + static_cast<int64_t>(G.offset[level]) * F;
  LevelIdx<D> li;
  li.init(T, res);

  uint32_t cell[D];
  bool have = false;
#pragma unroll
  for (int d = 0; d < D; ++d) cell[d] = 0u;
  float val[1 << D][F];

  // All 2^D corners are gathered together on a cell change: one divergent region, so
  // the waits for the gathers do not also wait for the younger coordinate prefetches
  // (per-corner conditional gathers, tried, cost more than the loads they save).
  auto step = [&](int64_t m, const float* xv) {
    float w[D];
    uint32_t g[D];
    bool same = have;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const float p = fmaf(scale, xv[d], 0.5f);
      const float fl = floorf(p);
      g[d] = static_cast<uint32_t>(static_cast<int>(fl));
      w[d] = p - fl;
      same = same & (g[d] == cell[d]);
    }
    if (!same) {
      have = true;
      uint32_t comp[D][2];
      li.dims(g, comp);
#pragma unroll
      for (int c = 0; c < (1 << D); ++c)
        Vec<TT, F>::load(grid + static_cast<int64_t>(li.corner(comp, c)) * F, val[c]);
#pragma unroll
      for (int d = 0; d < D; ++d) cell[d] = g[d];
    }
    float acc[F];
#pragma unroll
    for (int f = 0; f < F; ++f) acc[f] = 0.0f;
#pragma unroll
    for (int c = 0; c < (1 << D); ++c) {
      float wt = 1.0f;  // corner_weight, spelled out: see DESIGN.md §5 K3/K4 "Forms"
#pragma unroll
      for (int d = 0; d < D; ++d) wt *= ((c >> d) & 1) ? w[d] : 1.0f - w[d];
#pragma unroll
      for (int f = 0; f < F; ++f) acc[f] = fmaf(wt, val[c][f], acc[f]);
    }
    store_feat<TO, F>(out + m * out_stride + level * F, acc);
  };

  // coordinates prefetched one batch ahead (indices clamped to the chunk: no branch)
  constexpr int BS = kFwdBatch;
  float xb[BS][D], xn[BS][D];
  auto load_batch = [&](int64_t mb, float (*xo)[D]) {
#pragma unroll
    for (int j = 0; j < BS; ++j) {
      const int64_t m = mb + j < m1 ? mb + j : m1 - 1;
#pragma unroll
      for (int d = 0; d < D; ++d) xo[j][d] = x[m * x_stride + d];
    }
  };
  load_batch(m0, xb);
  for (int64_t mb = m0; mb < m1; mb += BS) {
    load_batch(mb + BS, xn);
#pragma unroll
    for (int j = 0; j < BS; ++j)
      if (mb + j < m1) step(mb + j, xb[j]);
#pragma unroll
    for (int j = 0; j < BS; ++j)
#pragma unroll
      for (int d = 0; d < D; ++d) xb[j][d] = xn[j][d];
  }
}

template <int D, int F, typename TG>
__global__ void __launch_bounds__(256) hashgrid_bwd_kernel(
    GridLevels G, int n_levels, int lanes_per_chunk, const float* __restrict__ x,
    int64_t x_stride, int64_t M, int64_t K, const TG* __restrict__ dout,
    int64_t dout_stride, float* __restrict__ dtable) {
  const int64_t gtid = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t chunk = gtid / lanes_per_chunk;
  const int level = static_cast<int>(gtid % lanes_per_chunk);
  const int64_t m0 = chunk * K;
  if (level >= n_levels || m0 >= M) return;
  const int64_t m1 = m0 + K < M ? m0 + K : M;

  const float scale = G.scale[level];
  const uint32_t res = G.res[level];
  const uint32_t T = G.size[level];
  float* __restrict__ grad = dtable + static_cast<int64_t>(G.offset[level]) * F;

  uint32_t cell[D];
  bool have = false;
  float acc[1 << D][F];
#pragma unroll
  for (int d = 0; d < D; ++d) cell[d] = 0u;
#pragma unroll
  for (int c = 0; c < (1 << D); ++c)
#pragma unroll
    for (int f = 0; f < F; ++f) acc[c][f] = 0.0f;

  auto flush = [&]() {
#pragma unroll
    for (int c = 0; c < (1 << D); ++c) {
      bool any = false;
#pragma unroll
      for (int f = 0; f < F; ++f) any = any || (acc[c][f] != 0.0f);
      if (any) {
        uint32_t gc[D];
#pragma unroll
        for (int d = 0; d < D; ++d) gc[d] = cell[d] + ((c >> d) & 1);
        const uint32_t idx = grid_index<D>(T, res, gc);
        float* dst = grad + static_cast<int64_t>(idx) * F;
#pragma unroll
        for (int f = 0; f < F; ++f) {
          if (acc[c][f] != 0.0f) atomicAdd(dst + f, acc[c][f]);
          acc[c][f] = 0.0f;
        }
      }
    }
  };

  for (int64_t m = m0; m < m1; ++m) {
    float w[D];
    uint32_t g[D];
    cell_split<D>(scale, x + m * x_stride, g, w);
    bool same = have;
#pragma unroll
    for (int d = 0; d < D; ++d) same = same & (g[d] == cell[d]);
    if (!same) {
      if (have) flush();
      have = true;
#pragma unroll
      for (int d = 0; d < D; ++d) cell[d] = g[d];
    }
    float gv[F];
#pragma unroll
    for (int f = 0; f < F; ++f) gv[f] = to_f32<TG>(dout[m * dout_stride + level * F + f]);
#pragma unroll
    for (int c = 0; c < (1 << D); ++c) {
      float wt = 1.0f;  // corner_weight, spelled out: see DESIGN.md §5 K3/K4 "Forms"
#pragma unroll
      for (int d = 0; d < D; ++d) wt *= ((c >> d) & 1) ? w[d] : 1.0f - w[d];
#pragma unroll
      for (int f = 0; f < F; ++f) acc[c][f] = fmaf(wt, gv[f], acc[c][f]);
    }
  }
  if (have) flush();
}

// ---------------------------------------------------------------------------------------
// Forward v6 (F = 2, L <= 16): v1's decomposition (lane = one level of one of the 4
// chunks a wavefront walks side by side) with the per-sample instruction stream rebuilt.
// A wavefront takes the gather path whenever any of its 64 lanes changes cell (~99 % of
// samples on the bench geometry), and its lanes mix dense and hashed levels, so in v1
// every per-corner branch (hashed / dense / dense wrap) ran both ways on nearly every
// sample, next to 64-bit clamped coordinate indices. Here:
//   * corner indices are branch-free apart from the dense wrap (LevelIdx::corners);
//   * memory goes through buffer descriptors with 32-bit offsets: reads past the end of x
//     return 0 and writes past the last row are dropped by the hardware range check, so
//     the walk has no per-sample bounds checks and a wave-uniform trip count;
//   * f16 corner features are interpolated straight from the packed pair (v_fma_mix_f32
//     reads the f16 operand in place: no conversions).
// Same corner order, weights and fma chain as v1: results are bit-identical to it. The
// default forward since r02 (0.667 -> 0.648 ms at bench size).
template <typename TO>
__device__ __forceinline__ void store2(__amdgpu_buffer_rsrc_t r, uint32_t off, float a0, float a1);
template <>
__device__ __forceinline__ void store2<__half>(__amdgpu_buffer_rsrc_t r, uint32_t off, float a0,
                                               float a1) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, __floats2half2_rn(a0, a1)),
                                        r, off, 0, 0);
}
template <>
__device__ __forceinline__ void store2<float>(__amdgpu_buffer_rsrc_t r, uint32_t off, float a0,
                                              float a1) {
  using v2 = uint32_t __attribute__((vector_size(8)));
  const v2 v = {__float_as_uint(a0), __float_as_uint(a1)};
  __builtin_amdgcn_raw_buffer_store_b64(v, r, off, 0, 0);
}

// One lane's walk of v6: level ``level`` over the K samples of the chunk starting at m0,
// writing each sample's 2 features at oo, oo + ostep, ... of the output buffer.
template <int D, typename TT, typename TO>
__device__ __forceinline__ void fwd_walk_v6(const GridLevels& G, int level, int64_t m0, int K,
                                            __amdgpu_buffer_rsrc_t rx, uint32_t xs4,
                                            __amdgpu_buffer_rsrc_t rt, __amdgpu_buffer_rsrc_t ro,
                                            uint32_t oo, uint32_t ostep) {
  using R = Raw2<TT>;
  const float scale = G.scale[level];
  const uint32_t res = G.res[level];
  const uint32_t T = G.size[level];
  const uint32_t base = G.offset[level] * R::bytes;
  LevelIdx<D> li;
  li.init(T, res);
  const uint32_t hmask = T - 1u;

  uint32_t xo = static_cast<uint32_t>(m0) * xs4;

  uint32_t cell[D];
  bool have = false;
#pragma unroll
  for (int d = 0; d < D; ++d) cell[d] = 0u;
  typename R::type val[1 << D];
#pragma unroll
  for (int c = 0; c < (1 << D); ++c) val[c] = {};

  auto step = [&](const float* xv) {
    float w[D];
    uint32_t g[D];
    bool same = have;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const float p = fmaf(scale, xv[d], 0.5f);
      const float fl = floorf(p);
      g[d] = static_cast<uint32_t>(static_cast<int>(fl));
      w[d] = p - fl;
      same = same & (g[d] == cell[d]);
    }
    if (!same) {
      uint32_t comp[D][2];
      li.dims(g, comp);
      uint32_t idx[1 << D], sum[1 << D];
#pragma unroll
      for (int c = 0; c < (1 << D); ++c) {
        uint32_t hx = 0u, sm = 0u;
#pragma unroll
        for (int d = 0; d < D; ++d) {
          hx ^= comp[d][(c >> d) & 1];
          sm += comp[d][(c >> d) & 1];
        }
        sum[c] = sm;
        idx[c] = li.hashed ? (hx & hmask) : sm;
      }
      uint32_t gmax = g[0];
#pragma unroll
      for (int d = 1; d < D; ++d) gmax = gmax > g[d] ? gmax : g[d];
      if (!li.hashed && gmax >= res - 1u) {
#pragma unroll
        for (int c = 0; c < (1 << D); ++c)
          if (sum[c] >= T) {
            const uint32_t s1 = sum[c] - T;
            idx[c] = s1 < T ? s1 : sum[c] % T;
          }
      }
#pragma unroll
      for (int c = 0; c < (1 << D); ++c) val[c] = R::load(rt, base + idx[c] * R::bytes);
#pragma unroll
      for (int d = 0; d < D; ++d) cell[d] = g[d];
      have = true;
    }
    float a0 = 0.0f, a1 = 0.0f;
#pragma unroll
    for (int c = 0; c < (1 << D); ++c) {
      float wt = 1.0f;
#pragma unroll
      for (int d = 0; d < D; ++d) wt *= ((c >> d) & 1) ? w[d] : 1.0f - w[d];
      R::fma2(wt, val[c], a0, a1);
    }
    store2<TO>(ro, oo, a0, a1);
    oo += ostep;
  };

  // coordinates prefetched one batch ahead; past the end of x the loads return 0
  constexpr int BS = kFwdBatch;
  float xb[BS][D], xn[BS][D];
  auto load_batch = [&](float (*xo_)[D]) {
#pragma unroll
    for (int j = 0; j < BS; ++j) {
      if constexpr (D == 3) {
        const auto v = __builtin_amdgcn_raw_buffer_load_b96(rx, xo, 0, 0);
        xo_[j][0] = __uint_as_float(v[0]);
        xo_[j][1] = __uint_as_float(v[1]);
        xo_[j][2] = __uint_as_float(v[2]);
      } else {
        const auto v = __builtin_amdgcn_raw_buffer_load_b64(rx, xo, 0, 0);
        xo_[j][0] = __uint_as_float(v[0]);
        xo_[j][1] = __uint_as_float(v[1]);
      }
      xo += xs4;
    }
  };
  load_batch(xb);
  for (int jb = 0; jb < K; jb += BS) {  // wave-uniform trip count
    load_batch(xn);
#pragma unroll
    for (int j = 0; j < BS; ++j)
      if (jb + j < K) step(xb[j]);
#pragma unroll
    for (int j = 0; j < BS; ++j)
#pragma unroll
      for (int d = 0; d < D; ++d) xb[j][d] = xn[j][d];
  }
}

template <int D, typename TT, typename TO>
__global__ void __launch_bounds__(256) hashgrid_fwd_v6_kernel(
    GridLevels G, int n_levels, const float* __restrict__ x, uint32_t x_bytes, uint32_t xs4,
    int64_t M, int K, const TT* __restrict__ table, uint32_t table_bytes,
    TO* __restrict__ out, uint32_t out_bytes, uint32_t os_bytes) {
  const int level = static_cast<int>(threadIdx.x & 15);
  const int64_t chunk = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 4;
  const int64_t m0 = chunk * K;
  if (level >= n_levels || m0 >= M) return;
  fwd_walk_v6<D, TT, TO>(
      G, level, m0, K, wave_rsrc(x, x_bytes), xs4, wave_rsrc(table, table_bytes),
      wave_rsrc(out, out_bytes),
      static_cast<uint32_t>(m0) * os_bytes + static_cast<uint32_t>(level) * 2u * sizeof(TO),
      os_bytes);
}

// ---------------------------------------------------------------------------------------
// Forward v9 "quad planes" (F = 2, f16 output): one lane per SAMPLE, every level, output
// in level-quad planes -- plane q holds levels 4q..4q+3 of every row, 16 B per row
// (level l feature f of row m at out[(l / 4) * plane + 8 m + 2 (l % 4) + f]). The walkers
// (v1 / v6) keep a lane on one level of one chunk and re-gather only on a cell change,
// but their wavefronts touch 4-16 chunks far apart, so each gather instruction lands on as
// many unrelated lines. Here a wavefront's 64 lanes are 64 consecutive samples of one
// ray: a corner gather's addresses coincide wherever neighbouring samples share a cell
// (all of them on the coarse levels, ~4 per cell on the finest), the coordinate load is
// one contiguous 768 B, and each quad's store is one contiguous 1 KiB (a level-major row
// layout written lane by lane leaves partial lines: 1.57 ms measured, against 0.47 for
// the planes). Every sample gathers its 8 corners per level (no cell reuse inside a
// lane). Same corner order, weights and fma chain as v6: bit-identical values. Measured
// on the bench coordinates (profiles/r05_hash_fwd_planes.log): v6 0.634 ms, v9 0.47-0.50
// ms; pinning level pairs to XCDs (block b -> XCD b % 8) made it slower (0.77 / 1.13 ms:
// every XCD then reads every coordinate).
template <int D, typename TT>
__global__ void __launch_bounds__(256) hashgrid_fwd_planes_kernel(
    GridLevels G, int n_levels, const float* __restrict__ x, uint32_t x_bytes, uint32_t xs4,
    int64_t M, const TT* __restrict__ table, uint32_t table_bytes, __half* __restrict__ out,
    uint32_t out_bytes, uint32_t plane_bytes) {
  const int64_t m = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  const __amdgpu_buffer_rsrc_t rx = wave_rsrc(x, x_bytes);
  const __amdgpu_buffer_rsrc_t rt = wave_rsrc(table, table_bytes);
  const __amdgpu_buffer_rsrc_t ro = wave_rsrc(out, out_bytes);
  const uint32_t xo = static_cast<uint32_t>(m) * xs4;  // past the end: loads return 0
  float xv[D];
  load_row<D>(rx, xo, xv);
  // rows past M: the stores are dropped by the range check (offset >= out_bytes)
  const uint32_t orow = m < M ? static_cast<uint32_t>(m) * 16u : 0x80000000u;
  const int n_quads = (n_levels + 3) >> 2;
  for (int q = 0; q < n_quads; ++q) {
    uint32_t packed[4];
    plane_quad<D, TT, true>(G, n_levels, q, xv, rt, packed);
    typedef uint32_t u4q __attribute__((vector_size(16)));
    const u4q v = {packed[0], packed[1], packed[2], packed[3]};
    __builtin_amdgcn_raw_buffer_store_b128(v, ro, static_cast<uint32_t>(q) * plane_bytes + orow,
                                           0, 0);
  }
}

// Distinct 64-B segments among the active lanes' addresses: the memory-side requests one
// wave-level float atomic instruction makes (MI355X_MICROARCH.md "Global float atomics").
// Called in divergent code: the count is returned to the instruction's first active lane
// only (0 elsewhere), so per-lane sums add every instruction exactly once.
__device__ __forceinline__ uint32_t distinct_segments(bool active, uint64_t seg) {
  uint64_t mask = __ballot(active);
  const uint64_t execm = __ballot(true);
  const bool first = (__lane_id() == __ffsll(static_cast<unsigned long long>(execm)) - 1);
  uint32_t n = 0;
  while (mask) {
    const int l = __ffsll(static_cast<unsigned long long>(mask)) - 1;
    const uint32_t lo = __shfl(static_cast<uint32_t>(seg), l);
    const uint32_t hi = __shfl(static_cast<uint32_t>(seg >> 32), l);
    const uint64_t s = (static_cast<uint64_t>(hi) << 32) | lo;
    mask &= ~__ballot(active && seg == s);
    ++n;
  }
  return first ? n : 0;
}

// ---------------------------------------------------------------------------------------
// The walks of the v2 backward: which rows of a chunk a wavefront loads and steps through.
// A walk type states its batch size BS, its compile-time row strides XS / DS (0: the
// run-time ones), what it needs beyond the common arguments (Args) and, in check<D>(), which
// combinations exist.

// Every row of the chunk in batches of BS, the next batch prefetched. With both strides
// known (the fused field's (M,3) coordinates and (M,32) dL/denc) every prefetch address is a
// per-batch scalar base plus immediate offsets: the walk issues no per-sample address
// arithmetic (r01 spent ~25 scalar instructions per sample on 64-bit clamped indices), and
// only a chunk's last two batches clamp. A batch, and inside a walked batch a sample, whose
// dL/dy is zero in every lane is passed over (do_batch).
template <int XS_, int DS_>
struct DenseWalk {
  static constexpr int XS = XS_, DS = DS_, BS = kBwdBatch;
  static constexpr bool kCount = false;
  struct Args {};
  template <int D>
  static constexpr void check() {
    static_assert((XS == 0 && DS == 0) || (XS == 3 && DS == 32 && D == 3),
                  "run-time strides, or the fused field's layout (3-D only)");
  }
};
// anr_hashgrid_bwd_tiles: the field backward marked the 32-row tiles whose dL/dy is zero in
// every row (it skipped them); their batches are neither loaded nor walked. The mask is laid
// out for batches of 8: a 32-row tile is 4 of them.
struct TileMaskWalk {
  static constexpr int XS = 3, DS = 32, BS = 8;
  static constexpr bool kCount = false;
  struct Args {
    const uint8_t* tile_nz;  // one flag per 32-row tile
  };
  template <int D>
  static constexpr void check() {
    static_assert(D == 3 && 32 % BS == 0, "fused-field layout; whole batches per tile");
  }
};
// anr_hashgrid_bwd_rows: one bit per dL/dy row (32 rows per word, written by
// anr_ingp_field_bwd_ref16_rows); only the rows whose bit is set are loaded and walked, after
// an LDS compaction in which every lane of the wavefront takes part (so: 16 levels).
struct RowBitsWalk {
  static constexpr int XS = 3, DS = 32, BS = kBwdBatch;
  static constexpr bool kCount = false;
  struct Args {
    const uint32_t* row_nz;
  };
  template <int D>
  static constexpr void check() {
    static_assert(D == 3, "fused-field layout");
    static_assert(BS % 2 == 0, "row indices are read in pairs");
  }
};
// The request-count instrument (anr_hashgrid_bwd_count_requests): the dense walk at run-time
// strides, but every flush instruction adds its number of distinct 64-B segments to *count
// instead of issuing the atomics (dtable is not written).
struct CountRequests {
  static constexpr int XS = 0, DS = 0, BS = kBwdBatch;
  static constexpr bool kCount = true;
  struct Args {
    unsigned long long* count;
  };
  template <int D>
  static constexpr void check() {
    static_assert(D == 3, "3-D grids are instrumented");
  }
};

// ---------------------------------------------------------------------------------------
// Backward v2 (F = 2, L <= 16): 4 lanes per level, one chunk of K consecutive samples per
// wave. lane = 4*level + 2*b + f owns feature f of the 2^(D-1) corners whose x-offset is b.
// The 4 lanes of a level touch entries (x, x+1) x features (0, 1): adjacent addresses on
// dense levels (and on hashed levels when x is even, since the first hash prime is 1),
// so one wave instruction issues one memory request per level instead of four. When
// the sample moves to a neighbouring cell with the same x, corners shared by the two
// cells keep their accumulated gradient. A corner whose sum is exactly zero issues no
// request: under build numerics such sums are rare, under the reference numerics most
// samples' f16 dL/denc underflow to zero (tcnn's x128 loss scale rounds them away), and the
// memory-side request count at the chunk ends alone fell from 20.8 M to 18.7 M per launch
// after the first step (profiles/r04_close PMC). A pending sum may so arrive in two atomics
// instead of one: f32 order, as any run.
template <int D, typename TG, typename Walk>
__global__ void __launch_bounds__(256) hashgrid_bwd_v2_kernel(
    GridLevels G, int n_levels, const float* __restrict__ x, int64_t x_stride_rt, int64_t M,
    int64_t K, const TG* __restrict__ dout, int64_t dout_stride_rt, float* __restrict__ dtable,
    typename Walk::Args wa) {
  Walk::template check<D>();
  constexpr int NC = LaneCorners<D>::NC;
  constexpr int XS = Walk::XS, DS = Walk::DS, BS = Walk::BS;
  constexpr bool COUNT = Walk::kCount;
  const int64_t x_stride = XS > 0 ? XS : x_stride_rt;
  const int64_t dout_stride = DS > 0 ? DS : dout_stride_rt;
  const int lane = threadIdx.x & 63;
  const int level = lane >> 2, b = (lane >> 1) & 1, f = lane & 1;
  const int64_t chunk = __builtin_amdgcn_readfirstlane(
      static_cast<int>((static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6));
  const int64_t m0 = chunk * K;
  // chunk bounds are wave-uniform: kept in scalar registers
  const int64_t m1 = static_cast<int64_t>(__builtin_amdgcn_readfirstlane(
      static_cast<int>(m0 + K < M ? K : M - m0))) + m0;
  if (m0 >= M || level >= n_levels) return;
  const float scale = G.scale[level];
  const uint32_t res = G.res[level];
  const uint32_t T = G.size[level];
  float* __restrict__ grad = dtable + static_cast<int64_t>(G.offset[level]) * 2 + f;
  LevelIdx<D> li;
  li.init(T, res);
  // The flushes are buffer atomics whose non-flushing lanes get an offset past the
  // table: the hardware range check drops them, so a flush is one select and one atomic
  // instruction, not a divergent branch (exec save / test / restore: scalar instructions,
  // which bounded this walk — SQ counters, profiles/r04_sq_close.md)
  const uint32_t table_bytes = (G.offset[n_levels - 1] + G.size[n_levels - 1]) * 8u;
  const __amdgpu_buffer_rsrc_t rg = wave_rsrc(dtable, table_bytes);
  const uint32_t gbase = (G.offset[level] * 2u + static_cast<uint32_t>(f)) * 4u;
  constexpr uint32_t kDrop = 0x80000000u;  // >= table_bytes (ABI: tables < 2 GB)

  uint32_t cell[D];
  bool have = false;
#pragma unroll
  for (int d = 0; d < D; ++d) cell[d] = 0u;
  float acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = 0.0f;
  uint32_t n_req = 0;  // COUNT only (wave-uniform)
  auto flush = [&](bool out, uint32_t e, float v) {
    if constexpr (COUNT) {
      n_req += distinct_segments(
          out, reinterpret_cast<uintptr_t>(grad + static_cast<int64_t>(e) * 2) >> 6);
    } else {
      __builtin_amdgcn_raw_ptr_buffer_atomic_fadd_f32(v, rg, out ? gbase + e * 8u : kDrop, 0, 0);
    }
  };

  auto step = [&](const float* xv, float gv) {
    float w[D];
    uint32_t g[D];
    bool same = have;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const float p = fmaf(scale, xv[d], 0.5f);
      const float fl = floorf(p);
      g[d] = static_cast<uint32_t>(static_cast<int>(fl));
      w[d] = p - fl;
      same = same & (g[d] == cell[d]);
    }
    if (!same) {
      if (have) {
        uint32_t idx[NC];
        LaneCorners<D>::indices(li, cell, b, idx);
        const bool keepx = g[0] == cell[0];
        int dl[D];
        dl[0] = 0;
#pragma unroll
        for (int d = 1; d < D; ++d) dl[d] = static_cast<int>(cell[d] - g[d]);
        float nacc[NC];
        LaneCorners<D>::carry(acc, dl, keepx, nacc);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          // a leaving corner whose sum is exactly zero issues no request
          const bool out = ((!keepx) | LaneCorners<D>::leaves(c, dl)) & (acc[c] != 0.0f);
          flush(out, idx[c], acc[c]);
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[c] = nacc[c];
      }
#pragma unroll
      for (int d = 0; d < D; ++d) cell[d] = g[d];
      have = true;
    }
    const float wx = b ? w[0] : 1.0f - w[0];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      float wt = wx;
#pragma unroll
      for (int d = 1; d < D; ++d) wt *= LaneCorners<D>::bit(c, d) ? w[d] : 1.0f - w[d];
      acc[c] = fmaf(wt, gv, acc[c]);
    }
  };

  // Batches of BS samples: the next batch's coordinates and gradients are loaded while
  // this one is processed (indices clamped to the chunk, so the loads need no branch).
  float xb[BS][D], xn[BS][D];
  TG gb[BS], gn[BS];
  const int col = level * 2 + f;
  auto load_batch = [&](int64_t mb, float (*xo)[D], TG* go) {
    if ((XS > 0 && DS > 0) && mb + BS <= m1) {  // wave-uniform: a full batch, no clamp
      // the batch's coordinates are the same for every lane: scalar loads through the
      // constant address space (24 dwords: one s_load_dwordx16 + one x8) instead of 24
      // vector loads of one broadcast dword each (hash bwd live 1.18 -> 1.06 ms, bench
      // profiles/r04_hash_bwd_scalar_x_ab.log)
      typedef __attribute__((address_space(4))) const float cf32;
      const cf32* __restrict__ xp = (const cf32*)(x + mb * XS);
      const TG* __restrict__ dp = dout + mb * DS;
#pragma unroll
      for (int j = 0; j < BS; ++j)
#pragma unroll
        for (int d = 0; d < D; ++d) xo[j][d] = xp[j * XS + d];
#pragma unroll
      for (int j = 0; j < BS; ++j) go[j] = dp[j * DS + col];
    } else {
#pragma unroll
      for (int j = 0; j < BS; ++j) {
        const int64_t m = mb + j < m1 ? mb + j : m1 - 1;
#pragma unroll
        for (int d = 0; d < D; ++d) xo[j][d] = x[m * x_stride + d];
        go[j] = dout[m * dout_stride + col];
      }
    }
  };
  // the chunk's end: every held corner with a nonzero sum
  auto flush_all = [&]() {
    if (have) {
      uint32_t idx[NC];
      LaneCorners<D>::indices(li, cell, b, idx);
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        flush(acc[c] != 0.0f, idx[c], acc[c]);
        acc[c] = 0.0f;
      }
      have = false;
    }
  };
  // A batch whose dL/dy is zero in every lane (all 16 levels x 2 features of its BS
  // samples: the reference numerics' f16 underflow leaves half of the 8-sample batches so
  // at the bench state) adds nothing and is skipped with one test; inside a walked batch a
  // SAMPLE whose dL/dy row is zero in every lane is not walked either. The pending cell is
  // kept across the skipped ones, and the walk stays exact because the next walked sample's
  // cell test / carry handles any jump (every corner leaves when a coordinate moves by more
  // than one cell). A pending sum may so arrive in two atomics instead of one: f32 order,
  // as any run.
  auto do_batch = [&](int64_t mb) {
    bool nzb = false;
#pragma unroll
    for (int j = 0; j < BS; ++j) nzb = nzb || (mb + j < m1 && to_f32<TG>(gb[j]) != 0.0f);
    if (__any(nzb)) {
#pragma unroll
      for (int j = 0; j < BS; ++j) {
        const float gv = to_f32<TG>(gb[j]);
        if (mb + j < m1 && __any(gv != 0.0f)) step(xb[j], gv);
      }
    }
  };
  auto advance = [&]() {
#pragma unroll
    for (int j = 0; j < BS; ++j) {
      gb[j] = gn[j];
#pragma unroll
      for (int d = 0; d < D; ++d) xb[j][d] = xn[j][d];
    }
  };
  // ---- the walk: three forms
  if constexpr (std::is_same<Walk, RowBitsWalk>::value) {
    const uint32_t* __restrict__ row_nz = wa.row_nz;
    // The chunk's set rows, compacted in order into this wave's LDS slot (K <= 256, a
    // multiple of 32; 64 rows per round: lane l tests row r0 + l), then walked in batches of
    // BS with the next batch's coordinates (scalar loads) and gradients prefetched. Every
    // loaded row is nonzero in some lane, so no per-sample test remains; the rows whose bit
    // is clear are exactly those the dense walk's per-sample skip passes over, so the same
    // corner sums reach the same entries.
    // K <= 256 rows, then 2 BS copies of the last set row: a batch (and the prefetch past
    // the end) reads its BS indices in pairs with no clamp
    __shared__ __attribute__((aligned(16))) uint32_t sidx[4][256 + 2 * BS];
    uint32_t* my = sidx[threadIdx.x >> 6];
    typedef __attribute__((address_space(4))) const uint32_t cu32;
    int n = 0;
    for (int64_t r0 = m0; r0 < m1; r0 += 64) {
      const cu32* mp = (const cu32*)(row_nz + (r0 >> 5));
      const uint32_t lo = mp[0];
      const uint32_t hi = r0 + 32 < m1 ? mp[1] : 0u;
      uint64_t bits = (static_cast<uint64_t>(hi) << 32) | lo;
      const int64_t span = m1 - r0;
      if (span < 64) bits &= (1ull << span) - 1ull;
      const int below = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(bits >> 32),
                                                   __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(bits), 0u));
      if ((bits >> lane) & 1ull) my[n + below] = static_cast<uint32_t>(r0 - m0 + lane);
      n += __popcll(bits);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (n > 0) {
      const uint32_t last = my[n - 1];
      if (lane < 2 * BS) my[n + lane] = last;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    typedef __attribute__((address_space(4))) const float cf32;
    // chunk-relative bases: a row's addresses are 32-bit scalar offsets from them
    const float* __restrict__ xc = x + m0 * 3;
    const TG* __restrict__ dc = dout + m0 * 32 + col;
    auto load_rows = [&](int bb, float (*xo)[D], TG* go) {
      uint32_t r[BS];
#pragma unroll
      for (int j = 0; j < BS; j += 2) {
        const uint2 q = *reinterpret_cast<const uint2*>(my + bb + j);
        r[j] = q.x;
        r[j + 1] = q.y;
      }
#pragma unroll
      for (int j = 0; j < BS; ++j) {
        const uint32_t i = __builtin_amdgcn_readfirstlane(r[j]);
        const cf32* xp = (const cf32*)(xc + i * 3u);
#pragma unroll
        for (int d = 0; d < D; ++d) xo[j][d] = xp[d];
        go[j] = dc[i * 32u];
      }
    };
    if (n > 0) {
      load_rows(0, xb, gb);
      for (int bb = 0; bb < n; bb += BS) {
        load_rows(bb + BS, xn, gn);
#pragma unroll
        for (int j = 0; j < BS; ++j)
          if (bb + j < n) step(xb[j], to_f32<TG>(gb[j]));
        advance();
      }
    }
  } else if constexpr (!std::is_same<Walk, TileMaskWalk>::value) {
    // every row of the chunk, the next batch prefetched
    load_batch(m0, xb, gb);
    for (int64_t mb = m0; mb < m1; mb += BS) {
      load_batch(mb + BS, xn, gn);
      do_batch(mb);
      advance();
    }
  } else {
    // the batches of the flagged tiles only. A chunk (K <= 256 rows, a multiple of 32,
    // tile-aligned) is <= 32 batches of 8: one wave-uniform bit mask, walked in order with
    // the next set batch prefetched.
    const int nbatch = static_cast<int>((m1 - m0 + BS - 1) / BS);
    const int ntile = static_cast<int>((m1 - m0 + 31) >> 5);
    const uint8_t* tf = wa.tile_nz + (m0 >> 5);
    uint32_t bm = 0;
    for (int t = 0; t < ntile; ++t)
      if (tf[t]) bm |= 0xFu << (4 * t);
    if (nbatch < 32) bm &= (1u << nbatch) - 1u;
    if (bm) {
      int j = __builtin_ctz(bm);
      bm &= bm - 1u;
      load_batch(m0 + static_cast<int64_t>(j) * BS, xb, gb);
      while (true) {
        const bool more = bm != 0u;
        const int jn = more ? __builtin_ctz(bm) : j;  // no further batch: reload j (unused)
        load_batch(m0 + static_cast<int64_t>(jn) * BS, xn, gn);
        do_batch(m0 + static_cast<int64_t>(j) * BS);
        if (!more) break;
        advance();
        j = jn;
        bm &= bm - 1u;
      }
    }
  }
  flush_all();
  if constexpr (COUNT) {
    // per lane (lanes above n_levels have returned; an instrument, not the hot path)
    if (n_req) atomicAdd(wa.count, static_cast<unsigned long long>(n_req));
  }
}

// v2: one chunk per wave. Every chunk ends with a flush of all its held corners, so a
// chunk should be long (requests per sample on the bench coordinates, tools/
// hash_bwd_requests.py: K = 32 / 64 / 128 / 256 / 512 -> 4.42 / 3.33 / 2.79 / 2.51 / 2.37),
// but the grid still needs waves to hide the walk's latency. Measured (r04 sweep,
// profiles/r04_hash_bwd_ksweep.md): at 1,024 rays x 1,024 samples K = 256 (4,096 waves)
// takes 0.176 ms against 0.295 ms at the r03 rule's K = 32 and 0.244 ms at K = 512; at
// 8,192 rays K = 256 / 512 / 1024 take 1.219 / 1.200 / 1.287 ms -- but in the bench step
// K = 512 makes the STEP slower (3.227 / 3.228 ms at 256 vs 3.270 / 3.267 at 512, alternating
// runs on one box, hash bwd 1.139 vs 1.129 ms: profiles/r04_hash_bwd_k_step_ab.log). Rule:
// 256 samples per chunk down to 4,096 chunks, shorter below that.
static int64_t pick_chunk_v2(int64_t M) {
  int64_t K = M / 4096;
  if (K < 1) K = 1;
  if (K > 256) K = 256;
  return K;
}

// anr_hashgrid_force_v1 (the tests' hook) selects the kernel generation per direction. Mode 0
// (default): forward v6, backward v2, measured fastest on the ray-coherent bench workload; 1:
// both v1, the generic kernels every shape falls back to; 6: forward v1, backward v2; 7: as 0
// with the backward's run-time-stride form (A/B of the compile-time strides).
static bool valid_mode(int m) { return m == 0 || m == 1 || m == 6 || m == 7; }
static int g_hashgrid_mode = 0;
static bool fwd_v6() { return g_hashgrid_mode == 0 || g_hashgrid_mode == 7; }
static bool bwd_v2() { return g_hashgrid_mode != 1; }

// Levels per wavefront of the v1 forward walker (the kernel takes 1, 2, 4, 8, 16, 32 or 64):
// 8 / 32 measured 0.99 / 0.81 ms against 0.65 ms at 16 on the bench coordinates.
constexpr int kFwdLpw = 16;

// Bytes of a table over all levels, at `entry_bytes` (features x element size) per entry.
static int64_t table_bytes(const GridLevels& G, int n_levels, int64_t entry_bytes) {
  return (static_cast<int64_t>(G.offset[n_levels - 1]) + G.size[n_levels - 1]) * entry_bytes;
}

// Samples per chunk: long chunks amortise the per-cell gathers/atomics, but the grid
// must still fill 256 CUs. Aim for >= 64K chunks (bench size: 128 samples per chunk,
// forward 0.656 -> 0.646 ms against 64).
// run > 0: the points come in runs of `run` neighbours (anr_hashgrid_fwd_runs), and a
// chunk is one run (up to 256 points), so no chunk straddles two runs. On the extract grid
// (81-point columns, 250 m apart in altitude) the default M / 65,536 = 40-point chunks
// ended or began mid-column every time: 0.782 ms per 2.65 M points against 0.412 ms with
// 81-point chunks (profiles/r04_extract_chunk_sweep.log).
static int64_t pick_chunk(int64_t M, int64_t run = 0) {
  if (run > 0 && run <= 256) return run;
  int64_t K = M / 65536;
  if (K < 1) K = 1;
  if (K > 128) K = 128;
  return K;
}

// 32-bit buffer offsets: a kernel that addresses through a buffer descriptor needs every one
// of its byte ranges below 2^31 (the descriptor's range check, and the drop offset of masked
// stores and atomics, sit at 2 GB)
static bool fits_buffer(std::initializer_list<int64_t> byte_ranges) {
  for (const int64_t b : byte_ranges)
    if (b >= (int64_t{1} << 31)) return false;
  return true;
}
static int64_t elem_bytes(int32_t dt) { return dt == ANR_F16 ? 2 : 4; }

// The element type of a dtype code, handed to a generic callable: with_dtype(dt, [&](auto t)
// { using T = typename decltype(t)::type; ... })
template <typename T>
struct Type {
  using type = T;
};
template <typename Fn>
static void with_dtype(int32_t dt, Fn fn) {
  if (dt == ANR_F16) fn(Type<__half>{});
  else fn(Type<float>{});
}

template <int D, int F>
static int launch_fwd(const GridLevels& G, const anr_hashgrid_desc* d, const float* x,
                      int64_t x_stride, int64_t M, const void* table, int32_t tdt,
                      void* out, int32_t odt, int64_t out_stride, hipStream_t s, int64_t run) {
  const int64_t K = pick_chunk(M, run);
  const int64_t chunks = ceil_div(M, K);
  // v6: 2 features, 2-D or 3-D (4-D runs the generic walker), at most 16 levels, every byte
  // range (the prefetch past the last chunk included) within a buffer descriptor
  if constexpr (F == 2 && D <= 3) {
    const int64_t esz_o = elem_bytes(odt);
    const int64_t x_bytes = ((M - 1) * x_stride + D) * 4;
    const int64_t t_bytes = table_bytes(G, d->n_levels, 2 * elem_bytes(tdt));
    const int64_t o_bytes = ((M - 1) * out_stride + d->n_levels * 2) * esz_o;
    if (d->n_levels <= 16 && fwd_v6() &&
        fits_buffer({x_bytes, t_bytes, o_bytes, (M + K) * x_stride * 4,
                     (M + K) * out_stride * esz_o})) {
      const dim3 grid(static_cast<unsigned>(ceil_div(chunks, 16))), block(256);
      with_dtype(tdt, [&](auto tt) {
        with_dtype(odt, [&](auto to) {
          using TT = typename decltype(tt)::type;
          using TO = typename decltype(to)::type;
          hipLaunchKernelGGL((hashgrid_fwd_v6_kernel<D, TT, TO>), grid, block, 0, s, G,
                             d->n_levels, x, static_cast<uint32_t>(x_bytes),
                             static_cast<uint32_t>(x_stride * 4), M, static_cast<int>(K),
                             static_cast<const TT*>(table), static_cast<uint32_t>(t_bytes),
                             static_cast<TO*>(out), static_cast<uint32_t>(o_bytes),
                             static_cast<uint32_t>(out_stride * esz_o));
        });
      });
      ANR_CHECK_LAUNCH("anr_hashgrid_fwd(v6)");
      return ANR_OK;
    }
  }
  // every other grid: the generic v1 walker
  const int lpw = kFwdLpw;
  const int n_groups = static_cast<int>(ceil_div(d->n_levels, lpw));
  const int64_t blocks_per_group = ceil_div(ceil_div(chunks, 64 / lpw), 4);
  const dim3 grid(static_cast<unsigned>(blocks_per_group * n_groups)), block(256);
  with_dtype(tdt, [&](auto tt) {
    with_dtype(odt, [&](auto to) {
      using TT = typename decltype(tt)::type;
      using TO = typename decltype(to)::type;
      hipLaunchKernelGGL((hashgrid_fwd_kernel<D, F, TT, TO>), grid, block, 0, s, G, d->n_levels,
                         lpw, n_groups, x, x_stride, M, K, static_cast<const TT*>(table),
                         static_cast<TO*>(out), out_stride);
    });
  });
  ANR_CHECK_LAUNCH("anr_hashgrid_fwd");
  return ANR_OK;
}

// The v2 backward walker's grids: 2 features, at most 16 levels, 2-D or 3-D (LaneCorners,
// its corner carry, has no 4-D form), and not switched off by anr_hashgrid_force_v1 ...
static bool bwd_v2_shape(const anr_hashgrid_desc* d) {
  return d->n_features == 2 && d->n_dims <= 3 && d->n_levels <= 16 && bwd_v2();
}
// ... and a gradient table within a buffer descriptor: larger tables (2^24 entries x 16
// levels) take the v1 walker
static bool bwd_v2_takes(const anr_hashgrid_desc* d, const GridLevels& G) {
  return bwd_v2_shape(d) && fits_buffer({table_bytes(G, d->n_levels, 2 * 4)});
}
// The fused field's layout: 3-D coordinates in rows of 3, dL/denc in rows of 32
static bool fused_layout(const anr_hashgrid_desc* d, int64_t x_stride, int64_t dout_stride) {
  return d->n_dims == 3 && x_stride == 3 && dout_stride == 32;
}

// One launch of the v2 walker over chunks of K rows, a chunk per wavefront, dL/dy in f16 or
// f32; wa: what the walk takes beyond the common arguments.
template <int D, typename Walk>
static void launch_bwd_v2(const GridLevels& G, const anr_hashgrid_desc* d, const float* x,
                          int64_t x_stride, int64_t M, int64_t K, const void* dout, int32_t gdt,
                          int64_t dout_stride, float* dtable, hipStream_t s,
                          typename Walk::Args wa = {}) {
  const dim3 grid(static_cast<unsigned>(ceil_div(ceil_div(M, K), 4))), block(256);
  with_dtype(gdt, [&](auto tg) {
    using TG = typename decltype(tg)::type;
    hipLaunchKernelGGL((hashgrid_bwd_v2_kernel<D, TG, Walk>), grid, block, 0, s, G, d->n_levels,
                       x, x_stride, M, K, static_cast<const TG*>(dout), dout_stride, dtable, wa);
  });
}

template <int D, int F>
static int launch_bwd(const GridLevels& G, const anr_hashgrid_desc* d, const float* x,
                      int64_t x_stride, int64_t M, const void* dout, int32_t gdt,
                      int64_t dout_stride, float* dtable, hipStream_t s) {
  if constexpr (F == 2 && D <= 3) {
    if (bwd_v2_takes(d, G)) {
      const int64_t K = pick_chunk_v2(M);
      bool fused = false;
      if constexpr (D == 3) {
        // compile-time strides for the fused field's layout (mode 7: A/B against the run-time ones)
        fused = fused_layout(d, x_stride, dout_stride) && g_hashgrid_mode != 7;
        if (fused)
          launch_bwd_v2<D, DenseWalk<3, 32>>(G, d, x, x_stride, M, K, dout, gdt, dout_stride,
                                             dtable, s);
      }
      if (!fused)
        launch_bwd_v2<D, DenseWalk<0, 0>>(G, d, x, x_stride, M, K, dout, gdt, dout_stride,
                                          dtable, s);
      ANR_CHECK_LAUNCH("anr_hashgrid_bwd(v2)");
      return ANR_OK;
    }
  }
  // every other grid: the generic v1 walker
  const int lpc = d->n_levels <= 16 ? 16 : 32;
  const int64_t K = pick_chunk(M);
  const int64_t threads = ceil_div(M, K) * lpc;
  const dim3 grid(static_cast<unsigned>(ceil_div(threads, 256))), block(256);
  with_dtype(gdt, [&](auto tg) {
    using TG = typename decltype(tg)::type;
    hipLaunchKernelGGL((hashgrid_bwd_kernel<D, F, TG>), grid, block, 0, s, G, d->n_levels, lpc,
                       x, x_stride, M, K, static_cast<const TG*>(dout), dout_stride, dtable);
  });
  ANR_CHECK_LAUNCH("anr_hashgrid_bwd");
  return ANR_OK;
}

// fn(D, F) as integral constants for the descriptor's (n_dims, n_features)
template <int... Vs, typename Fn>
static bool with_int(int v, Fn fn) {
  return ((v == Vs ? (fn(std::integral_constant<int, Vs>{}), true) : false) || ...);
}
template <typename Fn>
static int with_shape(const anr_hashgrid_desc* d, Fn fn) {
  int rc = ANR_E_UNSUPPORTED;
  bool found = false;
  with_int<2, 3, 4>(d->n_dims, [&](auto dims) {
    found = with_int<1, 2, 4, 8>(d->n_features, [&](auto feats) { rc = fn(dims, feats); });
  });
  if (!found)
    set_error("hashgrid: unsupported n_dims=%d n_features=%d", d->n_dims, d->n_features);
  return rc;
}

static bool is_float(int32_t dt) { return dt == ANR_F16 || dt == ANR_F32; }

// The argument check of every entry point, each message under the entry's own name `fn`:
// pointers, row count and strides (row_min: the least row_stride, 0 = the grid's n_levels x
// n_features values; hint: appended to the shape message), dtypes. The level tables follow
// (check_levels), after whatever an entry point checks in between.
static int check_call(const char* fn, const anr_hashgrid_desc* d, bool pointers, int64_t M,
                      int64_t x_stride, int64_t row_stride, int64_t row_min, bool dtypes,
                      const char* hint = "") {
  ANR_CHECK_ARG(d && pointers, "%s: null argument", fn);
  if (row_min == 0) row_min = static_cast<int64_t>(d->n_levels) * d->n_features;
  ANR_CHECK_ARG(M >= 0 && x_stride >= d->n_dims && row_stride >= row_min,
                "%s: bad shape/stride%s", fn, hint);
  ANR_CHECK_ARG(dtypes, "%s: bad dtype", fn);
  return ANR_OK;
}
static int check_levels(const char* fn, const anr_hashgrid_desc* d, GridLevels* G) {
  ANR_CHECK_ARG(make_levels(d, G), "%s: descriptor not initialised", fn);
  return ANR_OK;
}

}  // namespace anr

extern "C" int anr_hashgrid_force_v1(int32_t mode) {
  ANR_CHECK_ARG(anr::valid_mode(mode), "anr_hashgrid_force_v1: mode %d is not 0, 1, 6 or 7",
                mode);
  const int prev = anr::g_hashgrid_mode;
  anr::g_hashgrid_mode = mode;
  return prev;
}

// max_dims: 3 for anr_hashgrid_init (its contract since ABI 1), 4 for anr_hashgrid_init_nd
static int hashgrid_init(anr_hashgrid_desc* d, int32_t n_dims, int32_t max_dims,
                         int32_t n_levels, int32_t n_features, int32_t base_resolution,
                         float per_level_scale, int32_t log2_hashmap_size) {
  using namespace anr;
  ANR_CHECK_ARG(d, "anr_hashgrid_init: null desc");
  ANR_CHECK_ARG(n_dims >= 2 && n_dims <= max_dims,
                "anr_hashgrid_init: n_dims must be in [2, %d]", max_dims);
  ANR_CHECK_ARG(n_levels >= 1 && n_levels <= ANR_MAX_LEVELS,
                "anr_hashgrid_init: n_levels must be in [1, %d]", ANR_MAX_LEVELS);
  ANR_CHECK_ARG(n_features == 1 || n_features == 2 || n_features == 4 || n_features == 8,
                "anr_hashgrid_init: n_features must be 1, 2, 4 or 8");
  ANR_CHECK_ARG(log2_hashmap_size >= 4 && log2_hashmap_size <= 30,
                "anr_hashgrid_init: log2_hashmap_size out of range");
  ANR_CHECK_ARG(base_resolution >= 1 && per_level_scale >= 1.0f,
                "anr_hashgrid_init: bad resolution parameters");
  memset(d, 0, sizeof(*d));
  d->n_dims = n_dims;
  d->n_levels = n_levels;
  d->n_features = n_features;
  d->base_resolution = base_resolution;
  d->per_level_scale = per_level_scale;
  d->log2_hashmap_size = log2_hashmap_size;
  const float log2_pls = std::log2(per_level_scale);
  const uint32_t max_params = 0xffffffffu / 2;
  uint64_t offset = 0;
  for (int l = 0; l < n_levels; ++l) {
    const float scale =
        std::exp2(static_cast<float>(l) * log2_pls) * static_cast<float>(base_resolution) -
        1.0f;
    const uint32_t res = static_cast<uint32_t>(std::ceil(scale)) + 1u;
    uint64_t params_in_level;
    if (std::pow(static_cast<float>(res), static_cast<float>(n_dims)) >
        static_cast<float>(max_params)) {
      params_in_level = max_params;
    } else {
      params_in_level = 1;
      for (int k = 0; k < n_dims; ++k) params_in_level *= res;
    }
    params_in_level = (params_in_level + 7) / 8 * 8;
    const uint64_t T = 1ull << log2_hashmap_size;
    if (params_in_level > T) params_in_level = T;
    d->scales[l] = scale;
    d->resolutions[l] = res;
    d->offsets[l] = static_cast<uint32_t>(offset);
    offset += params_in_level;
    ANR_CHECK_ARG(offset < (1ull << 32), "anr_hashgrid_init: table too large");
  }
  d->offsets[n_levels] = static_cast<uint32_t>(offset);
  d->n_params = static_cast<int64_t>(offset) * n_features;
  return ANR_OK;
}

extern "C" int anr_hashgrid_init(anr_hashgrid_desc* d, int32_t n_dims, int32_t n_levels,
                                 int32_t n_features, int32_t base_resolution,
                                 float per_level_scale, int32_t log2_hashmap_size) {
  return hashgrid_init(d, n_dims, 3, n_levels, n_features, base_resolution, per_level_scale,
                       log2_hashmap_size);
}

extern "C" int anr_hashgrid_init_nd(anr_hashgrid_desc* d, int32_t n_dims, int32_t n_levels,
                                    int32_t n_features, int32_t base_resolution,
                                    float per_level_scale, int32_t log2_hashmap_size) {
  return hashgrid_init(d, n_dims, 4, n_levels, n_features, base_resolution, per_level_scale,
                       log2_hashmap_size);
}

extern "C" int anr_hashgrid_bwd_count_requests(const anr_hashgrid_desc* d, const float* x,
                                               int64_t x_stride, int64_t M, const void* dout,
                                               int32_t dout_dtype, int64_t dout_stride,
                                               const float* dtable, unsigned long long* count,
                                               anr_stream_t stream) {
  using namespace anr;
  constexpr const char* fn = "anr_hashgrid_bwd_count_requests";
  if (const int rc = check_call(fn, d, x && dout && dtable && count, M, x_stride, dout_stride, 0,
                                is_float(dout_dtype)))
    return rc;
  if (!(d->n_dims == 3 && bwd_v2_shape(d))) {
    set_error("%s: only the v2 backward (3-D, 2 features, <= 16 levels) is instrumented", fn);
    return ANR_E_UNSUPPORTED;
  }
  GridLevels G;
  if (const int rc = check_levels(fn, d, &G)) return rc;
  // gradient tables of 2 GB or more take the v1 walker in launch_bwd, whose requests this
  // v2 instrument does not model
  if (!bwd_v2_takes(d, G)) {
    set_error("%s: gradient table of 2 GB or more (the backward runs the uninstrumented v1 "
              "walker there)", fn);
    return ANR_E_UNSUPPORTED;
  }
  if (M == 0) return ANR_OK;
  float* tab = const_cast<float*>(dtable);  // not written by this walk
  launch_bwd_v2<3, CountRequests>(G, d, x, x_stride, M, pick_chunk_v2(M), dout, dout_dtype,
                                  dout_stride, tab, as_stream(stream), {count});
  ANR_CHECK_LAUNCH(fn);
  return ANR_OK;
}

extern "C" int64_t anr_hashgrid_bwd_chunk(int64_t M) {
  return M > 0 ? anr::pick_chunk_v2(M) : 0;
}

// anr_hashgrid_fwd and anr_hashgrid_fwd_runs under the name fn
static int hashgrid_fwd(const char* fn, const anr_hashgrid_desc* d, const float* x,
                        int64_t x_stride, int64_t M, int64_t run_length, const void* table,
                        int32_t table_dtype, void* out, int32_t out_dtype, int64_t out_stride,
                        anr_stream_t stream) {
  using namespace anr;
  if (M == 0) return ANR_OK;
  ANR_CHECK_ARG(d && x && table && out, "%s: null argument", fn);
  ANR_CHECK_ARG(run_length >= 0, "%s: run_length %lld < 0", fn, (long long)run_length);
  if (const int rc = check_call(fn, d, true, M, x_stride, out_stride, 0,
                                is_float(table_dtype) && is_float(out_dtype)))
    return rc;
  GridLevels G;
  if (const int rc = check_levels(fn, d, &G)) return rc;
  return with_shape(d, [&](auto dims, auto feats) {
    return launch_fwd<dims(), feats()>(G, d, x, x_stride, M, table, table_dtype, out, out_dtype,
                                       out_stride, as_stream(stream), run_length);
  });
}

extern "C" int anr_hashgrid_fwd_runs(const anr_hashgrid_desc* d, const float* x,
                                     int64_t x_stride, int64_t M, int64_t run_length,
                                     const void* table, int32_t table_dtype, void* out,
                                     int32_t out_dtype, int64_t out_stride,
                                     anr_stream_t stream) {
  return hashgrid_fwd("anr_hashgrid_fwd_runs", d, x, x_stride, M, run_length, table, table_dtype,
                      out, out_dtype, out_stride, stream);
}

extern "C" int anr_hashgrid_fwd(const anr_hashgrid_desc* d, const float* x,
                                int64_t x_stride, int64_t M, const void* table,
                                int32_t table_dtype, void* out, int32_t out_dtype,
                                int64_t out_stride, anr_stream_t stream) {
  return hashgrid_fwd("anr_hashgrid_fwd", d, x, x_stride, M, 0, table, table_dtype, out,
                      out_dtype, out_stride, stream);
}

extern "C" int anr_hashgrid_fwd_planes(const anr_hashgrid_desc* d, const float* x,
                                       int64_t x_stride, int64_t M, const void* table,
                                       int32_t table_dtype, void* out, int64_t plane_stride,
                                       anr_stream_t stream) {
  using namespace anr;
  constexpr const char* fn = "anr_hashgrid_fwd_planes";
  if (M == 0) return ANR_OK;
  // a plane holds 8 values per row; the alignment is tested between shape and dtype
  if (const int rc = check_call(fn, d, x && table && out, M, x_stride, plane_stride, 8 * M, true,
                                " (plane_stride >= 8 M)"))
    return rc;
  ANR_CHECK_ARG((reinterpret_cast<uintptr_t>(out) & 15) == 0 && (plane_stride & 7) == 0,
                "%s: out and plane_stride must be 16-byte aligned", fn);
  ANR_CHECK_ARG(is_float(table_dtype), "%s: bad dtype", fn);
  ANR_CHECK_ARG(d->n_features == 2 && d->n_levels <= 16 && d->n_dims >= 2 && d->n_dims <= 4,
                "%s: 2 features, <= 16 levels, 2-D to 4-D", fn);
  GridLevels G;
  if (const int rc = check_levels(fn, d, &G)) return rc;
  const int64_t n_quads = (d->n_levels + 3) / 4;
  const int64_t x_bytes = ((M - 1) * x_stride + d->n_dims) * 4;
  const int64_t t_bytes = table_bytes(G, d->n_levels, 2 * elem_bytes(table_dtype));
  const int64_t o_bytes = ((n_quads - 1) * plane_stride + 8 * M) * 2;
  ANR_CHECK_ARG(fits_buffer({x_bytes, t_bytes, o_bytes, (M + 256) * x_stride * 4,
                             plane_stride * 2}),
                "%s: byte ranges must stay below 2^31", fn);
  const dim3 grid(static_cast<unsigned>(ceil_div(M, 256))), block(256);
  with_int<2, 3, 4>(d->n_dims, [&](auto dims) {
    with_dtype(table_dtype, [&](auto tt) {
      using TT = typename decltype(tt)::type;
      hipLaunchKernelGGL((hashgrid_fwd_planes_kernel<dims(), TT>), grid, block, 0,
                         as_stream(stream), G, d->n_levels, x, static_cast<uint32_t>(x_bytes),
                         static_cast<uint32_t>(x_stride * 4), M, static_cast<const TT*>(table),
                         static_cast<uint32_t>(t_bytes), static_cast<__half*>(out),
                         static_cast<uint32_t>(o_bytes), static_cast<uint32_t>(plane_stride * 2));
    });
  });
  ANR_CHECK_LAUNCH(fn);
  return ANR_OK;
}

extern "C" int anr_hashgrid_bwd_tiles(const anr_hashgrid_desc* d, const float* x,
                                      int64_t x_stride, int64_t M, const void* dout,
                                      int32_t dout_dtype, int64_t dout_stride, float* dtable,
                                      const uint8_t* tile_nz, anr_stream_t stream) {
  using namespace anr;
  constexpr const char* fn = "anr_hashgrid_bwd_tiles";
  if (M == 0) return ANR_OK;
  if (const int rc = check_call(fn, d, x && dout && dtable && tile_nz, M, x_stride, dout_stride,
                                0, is_float(dout_dtype)))
    return rc;
  GridLevels G;
  if (const int rc = check_levels(fn, d, &G)) return rc;
  const int64_t K = pick_chunk_v2(M);
  if (!(fused_layout(d, x_stride, dout_stride) && bwd_v2_takes(d, G) && K % 32 == 0)) {
    // outside the tiled walker's shapes: the flags are an optimisation only
    return anr_hashgrid_bwd(d, x, x_stride, M, dout, dout_dtype, dout_stride, dtable, stream);
  }
  launch_bwd_v2<3, TileMaskWalk>(G, d, x, x_stride, M, K, dout, dout_dtype, dout_stride, dtable,
                                 as_stream(stream), {tile_nz});
  ANR_CHECK_LAUNCH(fn);
  return ANR_OK;
}

namespace anr {
// rows whose bit is clear -> 0 (anr_hashgrid_bwd_rows outside its walker: the dense walker
// reads every row, and a clear row need not have been written)
template <typename TG>
__global__ void zero_clear_rows_kernel(TG* __restrict__ dout, int64_t stride, int64_t M, int ncol,
                                       const uint32_t* __restrict__ row_nz) {
  const int64_t n = M * ncol;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < n;
       e += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t m = e / ncol;
    if (((row_nz[m >> 5] >> (m & 31)) & 1u) == 0u) dout[m * stride + e % ncol] = TG(0.0f);
  }
}
}  // namespace anr

extern "C" int anr_hashgrid_bwd_rows(const anr_hashgrid_desc* d, const float* x,
                                     int64_t x_stride, int64_t M, void* dout,
                                     int32_t dout_dtype, int64_t dout_stride, float* dtable,
                                     const uint32_t* row_nz, anr_stream_t stream) {
  using namespace anr;
  constexpr const char* fn = "anr_hashgrid_bwd_rows";
  if (M == 0) return ANR_OK;
  if (const int rc = check_call(fn, d, x && dout && dtable && row_nz, M, x_stride, dout_stride,
                                0, is_float(dout_dtype)))
    return rc;
  GridLevels G;
  if (const int rc = check_levels(fn, d, &G)) return rc;
  // chunks of whole 32-row words (the rule's length rounded down, at least one word)
  int64_t K = pick_chunk_v2(M) / 32 * 32;
  if (K < 32) K = 32;
  if (K > 256) K = 256;
  if (!(fused_layout(d, x_stride, dout_stride) && bwd_v2_takes(d, G) && d->n_levels == 16 &&
        M < (int64_t{1} << 31))) {
    // outside the row-mask walker's shapes: the clear rows are zeroed in place, then the
    // dense walker reads every row
    const int ncol = d->n_levels * d->n_features;
    const int64_t nb = ceil_div(M * ncol, 256), blocks = nb < 4096 ? nb : 4096;
    with_dtype(dout_dtype, [&](auto tg) {
      using TG = typename decltype(tg)::type;
      hipLaunchKernelGGL(zero_clear_rows_kernel<TG>, dim3(static_cast<unsigned>(blocks)),
                         dim3(256), 0, as_stream(stream), static_cast<TG*>(dout), dout_stride, M,
                         ncol, row_nz);
    });
    ANR_CHECK_LAUNCH("anr_hashgrid_bwd_rows(zero)");
    return anr_hashgrid_bwd(d, x, x_stride, M, dout, dout_dtype, dout_stride, dtable, stream);
  }
  launch_bwd_v2<3, RowBitsWalk>(G, d, x, x_stride, M, K, dout, dout_dtype, dout_stride, dtable,
                                as_stream(stream), {row_nz});
  ANR_CHECK_LAUNCH(fn);
  return ANR_OK;
}

extern "C" int anr_hashgrid_bwd(const anr_hashgrid_desc* d, const float* x,
                                int64_t x_stride, int64_t M, const void* dout,
                                int32_t dout_dtype, int64_t dout_stride, float* dtable,
                                anr_stream_t stream) {
  using namespace anr;
  if (M == 0) return ANR_OK;
  constexpr const char* fn = "anr_hashgrid_bwd";
  if (const int rc = check_call(fn, d, x && dout && dtable, M, x_stride, dout_stride, 0,
                                is_float(dout_dtype)))
    return rc;
  GridLevels G;
  if (const int rc = check_levels(fn, d, &G)) return rc;
  return with_shape(d, [&](auto dims, auto feats) {
    return launch_bwd<dims(), feats()>(G, d, x, x_stride, M, dout, dout_dtype, dout_stride,
                                       dtable, as_stream(stream));
  });
}
