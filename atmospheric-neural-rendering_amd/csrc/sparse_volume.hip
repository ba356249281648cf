// Sparse volume of a global-grid extract, and the orbit video's march over it: the voxels a
// global-grid extract keeps are a thin curved shell inside an axis-aligned box (11.7 % of it
// at the default grid), and a dense cube of that box passes anr_volume_render's 2^31-byte
// limit. The volume is the traversal's own bitmap with a rank per word, and the values in
// bitmap order.
//
// Layout. Box extents (ni, nj, nk), i fastest; a row of ni voxels takes row_pitch bits, a
// multiple of 32 that is >= ni (the bitmap of csrc/voxels.hip). Per bitmap word one 8-byte
// cell {bits, rank}: bit b of word w of row (j, k) is voxel (32 w + b, j, k), rank is the
// number of set bits in all words before it. values[rank + popcount(bits & ((1 << b) - 1))]
// is that voxel's value: one 8-byte load tells whether a corner is present and where its
// value sits, and the two x-neighbours of a sample share the cell unless they straddle a
// word. Pad bits are never set.
//
// Coarse level. One bit per brick of 8 x 8 x 8 sample cells. A sample at p reads the voxels
// floor(p) + {0, 1}^3, floor(p) in [-1, n - 1] per axis; brick (bi, bj, bk) holds the samples
// with (floor(p) + 1) >> 3 = (bi, bj, bk), so there are (n >> 3) + 1 bricks per axis, bi
// fastest, packed 32 to a word with no row pitch. A brick is live if any present voxel v has
// v or v - 1 (per axis) as a floor(p) inside it; a sample in a dead brick has all eight
// corners absent, and the trilinear value of eight zeros is +0.0 in the written order, so
// returning +0.0 there without the eight lookups changes no bit of the output.
//
// Build: mark (one thread per input voxel: an atomic OR for its bit and for its up to eight
// bricks, the brick OR skipped by a plain load when the bit is already set), popcount per
// word, the caller's exclusive scan into the rank fields, place (one thread per input voxel
// writes its value at its rank). Every step is independent of the input order. A voxel
// outside the box is not marked, so the caller's count test (total popcount = n) refuses it
// together with duplicates.
//
// The march is volume_march.h, shared with the dense cube: same steps at the same t, only
// the source of the eight values differs, so the output equals anr_volume_render's on the
// densified cube bit for bit.

#include "volume_march.h"

#pragma clang fp contract(off)

namespace anr {

constexpr int kSpvThreads = 256;
constexpr int kSpvBrickLog2 = 3;  // bricks of 8^3 sample cells

struct SpvGeom {
  const uint2* cells;
  const float* values;
  const uint32_t* coarse;
  int32_t nx, ny, nz;
  int32_t pitch_words;
  int32_t nbx, nby;
};

template <bool kSkip, bool kStats>
struct SparseVol {
  const uint2* cells;
  const float* values;
  const uint32_t* coarse;
  int32_t nx, ny, nz;
  int32_t pitch_words;
  int32_t nbx, nby;
  unsigned long long n_samples, n_skipped;

  __device__ __forceinline__ explicit SparseVol(const SpvGeom& g)
      : cells(g.cells), values(g.values), coarse(g.coarse), nx(g.nx), ny(g.ny), nz(g.nz),
        pitch_words(g.pitch_words), nbx(g.nbx), nby(g.nby), n_samples(0), n_skipped(0) {}

  __device__ __forceinline__ float cell_value(uint2 c, int b) const {
    if (!((c.x >> b) & 1u)) return 0.0f;
    return values[c.y + __popc(c.x & ((1u << b) - 1u))];
  }

  // Voxels (i, jj, kk) and (i + 1, jj, kk), i in [-1, nx - 1]: 0 where absent or outside.
  __device__ __forceinline__ void row_pair(int i, int jj, int kk, float* a, float* b) const {
    *a = 0.0f;
    *b = 0.0f;
    if (jj < 0 || kk < 0 || jj >= ny || kk >= nz) return;
    const int32_t base = (kk * ny + jj) * pitch_words;
    const int i1 = i + 1;
    int w0 = -1;
    uint2 c0 = make_uint2(0u, 0u);
    if (i >= 0) {
      w0 = i >> 5;
      c0 = cells[base + w0];
      *a = cell_value(c0, i & 31);
    }
    if (i1 < nx) {  // also keeps a full row (ni = row_pitch) from wrapping into the next one
      const int w1 = i1 >> 5;
      const uint2 c1 = w1 == w0 ? c0 : cells[base + w1];
      *b = cell_value(c1, i1 & 31);
    }
  }

  __device__ __forceinline__ float sample(float px, float py, float pz) {
    const float fx = floorf(px), fy = floorf(py), fz = floorf(pz);
    // no corner inside the box (NaN lands here too): nothing to read, and the float -> int
    // conversions below stay in range
    if (!(fx >= -1.0f && fy >= -1.0f && fz >= -1.0f && fx <= static_cast<float>(nx - 1) &&
          fy <= static_cast<float>(ny - 1) && fz <= static_cast<float>(nz - 1)))
      return 0.0f;
    const float wx = px - fx, wy = py - fy, wz = pz - fz;
    const int i = static_cast<int>(fx), j = static_cast<int>(fy), k = static_cast<int>(fz);
    if (kStats) ++n_samples;
    if (kSkip) {
      const int32_t brick = (((k + 1) >> kSpvBrickLog2) * nby + ((j + 1) >> kSpvBrickLog2)) * nbx +
                            ((i + 1) >> kSpvBrickLog2);
      if (!((coarse[brick >> 5] >> (brick & 31)) & 1u)) {
        if (kStats) ++n_skipped;
        return 0.0f;
      }
    }
    float v000, v001, v010, v011, v100, v101, v110, v111;
    row_pair(i, j, k, &v000, &v100);
    row_pair(i, j, k + 1, &v001, &v101);
    row_pair(i, j + 1, k, &v010, &v110);
    row_pair(i, j + 1, k + 1, &v011, &v111);
    return vol_trilerp(v000, v001, v010, v011, v100, v101, v110, v111, wx, wy, wz);
  }
};

// The volume with its light volume: tau in value order, so the rank that finds a corner's
// density finds its tau.
template <bool kSkip, bool kStats>
struct SparseVolLit : SparseVol<kSkip, kStats> {
  using Base = SparseVol<kSkip, kStats>;
  const float* tau;

  __device__ __forceinline__ SparseVolLit(const SpvGeom& g, const float* t) : Base(g), tau(t) {}

  // The value and its index in values (and tau) of bit b of cell c; 0 and -1 where absent.
  __device__ __forceinline__ void cell_at(uint2 c, int b, float* v, int32_t* at) const {
    *v = 0.0f;
    *at = -1;
    if (!((c.x >> b) & 1u)) return;
    *at = static_cast<int32_t>(c.y + __popc(c.x & ((1u << b) - 1u)));
    *v = this->values[*at];
  }

  // row_pair, with the indices.
  __device__ __forceinline__ void row_pair_at(int i, int jj, int kk, float* a, float* b,
                                              int32_t* ia, int32_t* ib) const {
    *a = 0.0f;
    *b = 0.0f;
    *ia = -1;
    *ib = -1;
    if (jj < 0 || kk < 0 || jj >= this->ny || kk >= this->nz) return;
    const int32_t base = (kk * this->ny + jj) * this->pitch_words;
    const int i1 = i + 1;
    int w0 = -1;
    uint2 c0 = make_uint2(0u, 0u);
    if (i >= 0) {
      w0 = i >> 5;
      c0 = this->cells[base + w0];
      cell_at(c0, i & 31, a, ia);
    }
    if (i1 < this->nx) {
      const int w1 = i1 >> 5;
      const uint2 c1 = w1 == w0 ? c0 : this->cells[base + w1];
      cell_at(c1, i1 & 31, b, ib);
    }
  }

  // sample(p), and in *tau_hat, where that is >= cutoff, the mean of tau over the corners
  // with density > 0 (vol_lit_corners). A dead brick has no such corner.
  __device__ __forceinline__ float lit_sample(float px, float py, float pz, float cutoff,
                                              float* tau_hat) {
    const float fx = floorf(px), fy = floorf(py), fz = floorf(pz);
    if (!(fx >= -1.0f && fy >= -1.0f && fz >= -1.0f && fx <= static_cast<float>(this->nx - 1) &&
          fy <= static_cast<float>(this->ny - 1) && fz <= static_cast<float>(this->nz - 1)))
      return 0.0f;
    const float wx = px - fx, wy = py - fy, wz = pz - fz;
    const int i = static_cast<int>(fx), j = static_cast<int>(fy), k = static_cast<int>(fz);
    if (kStats) ++this->n_samples;
    if (kSkip) {
      const int32_t brick =
          (((k + 1) >> kSpvBrickLog2) * this->nby + ((j + 1) >> kSpvBrickLog2)) * this->nbx +
          ((i + 1) >> kSpvBrickLog2);
      if (!((this->coarse[brick >> 5] >> (brick & 31)) & 1u)) {
        if (kStats) ++this->n_skipped;
        return 0.0f;
      }
    }
    // corners in x-outer, z-inner order
    float v[8];
    int32_t at[8];
    row_pair_at(i, j, k, &v[0], &v[4], &at[0], &at[4]);
    row_pair_at(i, j, k + 1, &v[1], &v[5], &at[1], &at[5]);
    row_pair_at(i, j + 1, k, &v[2], &v[6], &at[2], &at[6]);
    row_pair_at(i, j + 1, k + 1, &v[3], &v[7], &at[3], &at[7]);
    const float dens = vol_trilerp(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], wx, wy, wz);
    if (dens < cutoff) return dens;
    float tv[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) tv[c] = v[c] > 0.0f ? tau[at[c]] : 0.0f;
    *tau_hat = vol_lit_corners(v, tv, wx, wy, wz);
    return dens;
  }
};

template <bool kSkip, bool kStats>
__global__ void __launch_bounds__(kVolThreads) sparse_volume_render_lit_kernel(
    SpvGeom g, const float* __restrict__ tau, const anr_camera* __restrict__ cams, int32_t H,
    int32_t W, int32_t tiles_x, int32_t tiles_y, VolMarch m, float* __restrict__ rgba,
    unsigned long long* __restrict__ counters) {
  SparseVolLit<kSkip, kStats> vol(g, tau);
  vol_march_pixel<true>(vol, cams, H, W, tiles_x, tiles_y, m, rgba);
  if (kStats) {
    if (vol.n_samples) atomicAdd(counters + 0, vol.n_samples);
    if (vol.n_skipped) atomicAdd(counters + 1, vol.n_skipped);
  }
}

// One thread per value, in value order, so the 64 lanes of a wavefront are 64 present voxels
// that follow each other in the bitmap and every lane walks. The thread finds its voxel from
// the ranks: the last word whose rank is <= r holds it (an empty word shares its rank with
// the next word, so it is never the last), as the (r - rank)-th set bit. About 27 dependent
// 8-byte loads at the default grid, against a walk of hundreds of samples.
template <bool kSkip>
__global__ void __launch_bounds__(kSpvThreads) sparse_volume_light_kernel(
    SpvGeom g, int32_t n_words, int32_t n_values, VolMarch m, float* __restrict__ tau) {
  const int64_t r64 = static_cast<int64_t>(blockIdx.x) * kSpvThreads + threadIdx.x;
  if (r64 >= n_values) return;
  const uint32_t r = static_cast<uint32_t>(r64);
  int32_t lo = 0, hi = n_words - 1;  // the answer lies in [lo, hi]; rank of word 0 is 0
  while (lo < hi) {
    const int32_t mid = lo + (hi - lo + 1) / 2;
    if (g.cells[mid].y <= r)
      lo = mid;
    else
      hi = mid - 1;
  }
  const uint2 c = g.cells[lo];
  float t = 0.0f;
  // ranks that disagree with the bitmap find no bit: the voxel keeps 0
  if (c.y <= r && r - c.y < static_cast<uint32_t>(__popc(c.x)) && g.values[r] > 0.0f) {
    uint32_t bits = c.x;
    for (uint32_t q = r - c.y; q > 0; --q) bits &= bits - 1u;
    const int32_t row = lo / g.pitch_words;
    const int32_t k = row / g.ny;
    const float p[3] = {static_cast<float>((lo - row * g.pitch_words) * 32 + (__ffs(bits) - 1)),
                        static_cast<float>(row - k * g.ny), static_cast<float>(k)};
    SparseVol<kSkip, false> vol(g);
    t = vol_light_tau(vol, p, m);
  }
  tau[r] = t;
}

template <bool kSkip, bool kStats>
__global__ void __launch_bounds__(kVolThreads) sparse_volume_render_kernel(
    SpvGeom g, const anr_camera* __restrict__ cams, int32_t H, int32_t W, int32_t tiles_x,
    int32_t tiles_y, VolMarch m, float* __restrict__ rgba,
    unsigned long long* __restrict__ counters) {
  SparseVol<kSkip, kStats> vol(g);
  vol_march_pixel(vol, cams, H, W, tiles_x, tiles_y, m, rgba);
  if (kStats) {
    if (vol.n_samples) atomicAdd(counters + 0, vol.n_samples);
    if (vol.n_skipped) atomicAdd(counters + 1, vol.n_skipped);
  }
}

template <bool kSkip>
__global__ void __launch_bounds__(kSpvThreads) sparse_volume_sample_kernel(
    SpvGeom g, const float* __restrict__ pos, int64_t P, float* __restrict__ out) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kSpvThreads + threadIdx.x;
  if (r >= P) return;
  SparseVol<kSkip, false> vol(g);
  out[r] = vol.sample(pos[r * 3 + 0], pos[r * 3 + 1], pos[r * 3 + 2]);
}

struct SpvBox {
  int32_t i0, j0, k0;
  int32_t ni, nj, nk;
  int32_t pitch_words;
  int32_t nbx, nby, nbz;
  int64_t n_words;
  int64_t coarse_words;
};

// The input voxel's box-relative index, false when it lies outside the box.
__device__ __forceinline__ bool spv_index(const int32_t* __restrict__ voxels, int64_t r,
                                          const SpvBox& box, int32_t* i, int32_t* j, int32_t* k) {
  const int64_t a = static_cast<int64_t>(voxels[r * 3 + 0]) - box.i0;
  const int64_t b = static_cast<int64_t>(voxels[r * 3 + 1]) - box.j0;
  const int64_t c = static_cast<int64_t>(voxels[r * 3 + 2]) - box.k0;
  if (a < 0 || b < 0 || c < 0 || a >= box.ni || b >= box.nj || c >= box.nk) return false;
  *i = static_cast<int32_t>(a);
  *j = static_cast<int32_t>(b);
  *k = static_cast<int32_t>(c);
  return true;
}

__global__ void __launch_bounds__(kSpvThreads) sparse_volume_mark_kernel(
    const int32_t* __restrict__ voxels, int64_t n, SpvBox box, uint32_t* __restrict__ cells,
    uint32_t* __restrict__ coarse) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kSpvThreads + threadIdx.x;
  if (r >= n) return;
  int32_t i, j, k;
  if (!spv_index(voxels, r, box, &i, &j, &k)) return;
  const int64_t w = static_cast<int64_t>(k * box.nj + j) * box.pitch_words + (i >> 5);
  atomicOr(cells + 2 * w, 1u << (i & 31));
  // the bricks of the samples that read this voxel: floor(p) = v or v - 1 per axis, brick
  // index (floor(p) + 1) >> 3
  const int32_t bi[2] = {(i + 1) >> kSpvBrickLog2, i >> kSpvBrickLog2};
  const int32_t bj[2] = {(j + 1) >> kSpvBrickLog2, j >> kSpvBrickLog2};
  const int32_t bk[2] = {(k + 1) >> kSpvBrickLog2, k >> kSpvBrickLog2};
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    if (c == 1 && bk[1] == bk[0]) continue;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      if (b == 1 && bj[1] == bj[0]) continue;
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        if (a == 1 && bi[1] == bi[0]) continue;
        const int32_t brick = (bk[c] * box.nby + bj[b]) * box.nbx + bi[a];
        const uint32_t mask = 1u << (brick & 31);
        // a stale value only costs the shortcut: OR is idempotent
        if (!(coarse[brick >> 5] & mask)) atomicOr(coarse + (brick >> 5), mask);
      }
    }
  }
}

__global__ void __launch_bounds__(kSpvThreads) sparse_volume_popcount_kernel(
    const uint2* __restrict__ cells, int64_t n_words, int32_t* __restrict__ counts) {
  const int64_t w = static_cast<int64_t>(blockIdx.x) * kSpvThreads + threadIdx.x;
  if (w < n_words) counts[w] = __popc(cells[w].x);
}

__global__ void __launch_bounds__(kSpvThreads) sparse_volume_place_kernel(
    const int32_t* __restrict__ voxels, const float* __restrict__ values, int64_t n,
    double density_scale, SpvBox box, const uint2* __restrict__ cells, int64_t n_values,
    float* __restrict__ out) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kSpvThreads + threadIdx.x;
  if (r >= n) return;
  int32_t i, j, k;
  if (!spv_index(voxels, r, box, &i, &j, &k)) return;
  const int64_t w = static_cast<int64_t>(k * box.nj + j) * box.pitch_words + (i >> 5);
  const uint2 c = cells[w];
  const int b = i & 31;
  if (!((c.x >> b) & 1u)) return;  // a bitmap that is not this input's
  const int64_t at = static_cast<int64_t>(c.y) + __popc(c.x & ((1u << b) - 1u));
  if (at >= n_values) return;  // ranks that disagree with the bitmap cannot write past the end
  const double v = static_cast<double>(values[r]);
  out[at] = v == v ? static_cast<float>(v * density_scale) : 0.0f;
}

// The box of an entry's arguments; a message when they are bad, nullptr otherwise.
static const char* spv_box(int32_t i0, int32_t j0, int32_t k0, int32_t ni, int32_t nj, int32_t nk,
                           int64_t row_pitch, SpvBox* box) {
  if (ni < 1 || nj < 1 || nk < 1) return "extents must be >= 1";
  if (row_pitch < ni || row_pitch % 32 != 0 || row_pitch > (1LL << 31))
    return "row_pitch must be a multiple of 32 that is >= ni";
  if (static_cast<int64_t>(i0) + ni > (1LL << 31) || static_cast<int64_t>(j0) + nj > (1LL << 31) ||
      static_cast<int64_t>(k0) + nk > (1LL << 31))
    return "origin + extent overflows int32";
  int64_t words = 0;
  if (__builtin_mul_overflow(row_pitch / 32, static_cast<int64_t>(nj), &words) ||
      __builtin_mul_overflow(words, static_cast<int64_t>(nk), &words) || words >= (1LL << 31))
    return "2^31 bitmap words or more (32-bit offsets)";
  const int64_t nbx = (ni >> kSpvBrickLog2) + 1, nby = (nj >> kSpvBrickLog2) + 1,
                nbz = (nk >> kSpvBrickLog2) + 1;
  // bricks <= (ni / 8 + 1) (nj / 8 + 1) (nk / 8 + 1): each factor below 2^28 + 1
  int64_t bricks = 0;
  if (__builtin_mul_overflow(nbx, nby, &bricks) || __builtin_mul_overflow(bricks, nbz, &bricks) ||
      bricks >= (1LL << 31))
    return "2^31 bricks or more (32-bit offsets)";
  *box = SpvBox{i0, j0, k0, ni, nj, nk, static_cast<int32_t>(row_pitch / 32),
                static_cast<int32_t>(nbx), static_cast<int32_t>(nby), static_cast<int32_t>(nbz),
                words, ceil_div(bricks, 32)};
  return nullptr;
}

// Checks an anr_sparse_volume; the accessor's geometry in *g.
static const char* spv_geom(const anr_sparse_volume* v, int32_t skip, SpvGeom* g) {
  if (v == nullptr) return "null pointer (volume)";
  SpvBox box;
  const char* why = spv_box(0, 0, 0, v->ni, v->nj, v->nk, v->row_pitch, &box);
  if (why) return why;
  if (v->n_values < 1 || v->n_values >= (1LL << 31)) return "n_values must be in [1, 2^31)";
  if (skip != 0 && skip != 1) return "skip must be 0 or 1";
  *g = SpvGeom{reinterpret_cast<const uint2*>(v->cells), v->values, v->coarse, v->ni, v->nj,
               v->nk, box.pitch_words, box.nbx, box.nby};
  return nullptr;
}

}  // namespace anr

extern "C" int64_t anr_sparse_volume_coarse_words(int32_t ni, int32_t nj, int32_t nk) {
  anr::SpvBox box;
  // the smallest row pitch; the brick count does not depend on it
  const int64_t pitch = ni >= 1 ? anr::ceil_div(ni, 32) * 32 : 32;
  return anr::spv_box(0, 0, 0, ni, nj, nk, pitch, &box) == nullptr ? box.coarse_words : 0;
}

extern "C" int anr_sparse_volume_mark(const int32_t* voxels, int64_t n, int32_t i0, int32_t j0,
                                      int32_t k0, int32_t ni, int32_t nj, int32_t nk,
                                      int64_t row_pitch, uint32_t* cells, uint32_t* coarse,
                                      anr_stream_t stream) {
  using namespace anr;
  ANR_CHECK_ARG(n >= 1, "anr_sparse_volume_mark: no voxels (n = %lld)", static_cast<long long>(n));
  ANR_CHECK_ARG(n < (1LL << 31), "anr_sparse_volume_mark: 2^31 voxels or more");
  SpvBox box;
  const char* why = spv_box(i0, j0, k0, ni, nj, nk, row_pitch, &box);
  ANR_CHECK_ARG(why == nullptr, "anr_sparse_volume_mark: %s", why);
  ANR_CHECK_ARG(voxels && cells && coarse, "anr_sparse_volume_mark: null pointer");
  hipLaunchKernelGGL(sparse_volume_mark_kernel, dim3(static_cast<unsigned>(ceil_div(n, kSpvThreads))),
                     dim3(kSpvThreads), 0, as_stream(stream), voxels, n, box, cells, coarse);
  ANR_CHECK_LAUNCH("anr_sparse_volume_mark");
  return ANR_OK;
}

extern "C" int anr_sparse_volume_popcount(const uint32_t* cells, int64_t n_words, int32_t* counts,
                                          anr_stream_t stream) {
  using namespace anr;
  ANR_CHECK_ARG(n_words >= 1 && n_words < (1LL << 31),
                "anr_sparse_volume_popcount: n_words must be in [1, 2^31)");
  ANR_CHECK_ARG(cells && counts, "anr_sparse_volume_popcount: null pointer");
  hipLaunchKernelGGL(sparse_volume_popcount_kernel,
                     dim3(static_cast<unsigned>(ceil_div(n_words, kSpvThreads))), dim3(kSpvThreads),
                     0, as_stream(stream), reinterpret_cast<const uint2*>(cells), n_words, counts);
  ANR_CHECK_LAUNCH("anr_sparse_volume_popcount");
  return ANR_OK;
}

extern "C" int anr_sparse_volume_place(const int32_t* voxels, const float* values, int64_t n,
                                       double density_scale, int32_t i0, int32_t j0, int32_t k0,
                                       int32_t ni, int32_t nj, int32_t nk, int64_t row_pitch,
                                       const uint32_t* cells, int64_t n_values, float* out,
                                       anr_stream_t stream) {
  using namespace anr;
  ANR_CHECK_ARG(n >= 1, "anr_sparse_volume_place: no voxels (n = %lld)", static_cast<long long>(n));
  ANR_CHECK_ARG(n < (1LL << 31) && n_values >= 1 && n_values < (1LL << 31),
                "anr_sparse_volume_place: 2^31 voxels or more, or no values");
  ANR_CHECK_ARG(std::isfinite(density_scale), "anr_sparse_volume_place: density_scale not finite");
  SpvBox box;
  const char* why = spv_box(i0, j0, k0, ni, nj, nk, row_pitch, &box);
  ANR_CHECK_ARG(why == nullptr, "anr_sparse_volume_place: %s", why);
  ANR_CHECK_ARG(voxels && values && cells && out, "anr_sparse_volume_place: null pointer");
  hipLaunchKernelGGL(sparse_volume_place_kernel,
                     dim3(static_cast<unsigned>(ceil_div(n, kSpvThreads))), dim3(kSpvThreads), 0,
                     as_stream(stream), voxels, values, n, density_scale, box,
                     reinterpret_cast<const uint2*>(cells), n_values, out);
  ANR_CHECK_LAUNCH("anr_sparse_volume_place");
  return ANR_OK;
}

extern "C" int anr_sparse_volume_sample(const anr_sparse_volume* volume, int32_t skip,
                                        const float* positions, int64_t P, float* out,
                                        anr_stream_t stream) {
  using namespace anr;
  SpvGeom g;
  const char* why = spv_geom(volume, skip, &g);
  ANR_CHECK_ARG(why == nullptr, "anr_sparse_volume_sample: %s", why);
  ANR_CHECK_ARG(P >= 0 && P < (1LL << 31) * kSpvThreads, "anr_sparse_volume_sample: bad P %lld",
                static_cast<long long>(P));
  if (P == 0) return ANR_OK;
  ANR_CHECK_ARG(g.cells && g.values && (g.coarse || !skip) && positions && out,
                "anr_sparse_volume_sample: null pointer");
  const dim3 grid(static_cast<unsigned>(ceil_div(P, kSpvThreads))), block(kSpvThreads);
  if (skip)
    hipLaunchKernelGGL(sparse_volume_sample_kernel<true>, grid, block, 0, as_stream(stream), g,
                       positions, P, out);
  else
    hipLaunchKernelGGL(sparse_volume_sample_kernel<false>, grid, block, 0, as_stream(stream), g,
                       positions, P, out);
  ANR_CHECK_LAUNCH("anr_sparse_volume_sample");
  return ANR_OK;
}

extern "C" int anr_sparse_volume_render(const anr_sparse_volume* volume, int32_t skip,
                                        const anr_camera* cameras, int64_t F, int64_t H, int64_t W,
                                        const anr_volume_params* params, float* rgba,
                                        int64_t* counters, anr_stream_t stream) {
  using namespace anr;
  ANR_CHECK_ARG(params != nullptr, "anr_sparse_volume_render: null pointer (params)");
  SpvGeom g;
  const char* why = spv_geom(volume, skip, &g);
  ANR_CHECK_ARG(why == nullptr, "anr_sparse_volume_render: %s", why);
  VolMarch m;
  int64_t tiles_x = 0, tiles_y = 0;
  bool empty = true;
  const int rc = vol_plan("anr_sparse_volume_render", g.nx, g.ny, g.nz, F, H, W, params, &m,
                          &tiles_x, &tiles_y, &empty);
  if (rc != ANR_OK || empty) return rc;
  ANR_CHECK_ARG(g.cells && g.values && (g.coarse || !skip) && cameras && rgba,
                "anr_sparse_volume_render: null pointer");
  const dim3 grid(static_cast<unsigned>(tiles_x * tiles_y * F)), block(kVolThreads);
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counters);
  const int32_t h = static_cast<int32_t>(H), w = static_cast<int32_t>(W);
  const int32_t tx = static_cast<int32_t>(tiles_x), ty = static_cast<int32_t>(tiles_y);
#define ANR_SPV_LAUNCH(S, C)                                                                   \
  hipLaunchKernelGGL((sparse_volume_render_kernel<S, C>), grid, block, 0, as_stream(stream), g, \
                     cameras, h, w, tx, ty, m, rgba, cnt)
  if (skip && cnt)
    ANR_SPV_LAUNCH(true, true);
  else if (skip)
    ANR_SPV_LAUNCH(true, false);
  else if (cnt)
    ANR_SPV_LAUNCH(false, true);
  else
    ANR_SPV_LAUNCH(false, false);
#undef ANR_SPV_LAUNCH
  ANR_CHECK_LAUNCH("anr_sparse_volume_render");
  return ANR_OK;
}

extern "C" int anr_sparse_volume_light(const anr_sparse_volume* volume, int32_t skip,
                                       const anr_volume_params* params, float* tau,
                                       anr_stream_t stream) {
  using namespace anr;
  ANR_CHECK_ARG(params != nullptr, "anr_sparse_volume_light: null pointer (params)");
  SpvGeom g;
  const char* why = spv_geom(volume, skip, &g);
  ANR_CHECK_ARG(why == nullptr, "anr_sparse_volume_light: %s", why);
  VolMarch m;
  int64_t tiles_x = 0, tiles_y = 0;
  bool empty = true;
  // the plan of a 1 x 1 image: its refusals and the walk's integer bound
  const int rc = vol_plan("anr_sparse_volume_light", g.nx, g.ny, g.nz, 1, 1, 1, params, &m,
                          &tiles_x, &tiles_y, &empty);
  if (rc != ANR_OK) return rc;
  ANR_CHECK_ARG(g.cells && g.values && (g.coarse || !skip) && tau,
                "anr_sparse_volume_light: null pointer");
  const int32_t n_values = static_cast<int32_t>(volume->n_values);
  const int32_t n_words = g.pitch_words * g.ny * g.nz;  // < 2^31: spv_box
  const dim3 grid(static_cast<unsigned>(ceil_div(volume->n_values, kSpvThreads)));
  if (skip)
    hipLaunchKernelGGL(sparse_volume_light_kernel<true>, grid, dim3(kSpvThreads), 0,
                       as_stream(stream), g, n_words, n_values, m, tau);
  else
    hipLaunchKernelGGL(sparse_volume_light_kernel<false>, grid, dim3(kSpvThreads), 0,
                       as_stream(stream), g, n_words, n_values, m, tau);
  ANR_CHECK_LAUNCH("anr_sparse_volume_light");
  return ANR_OK;
}

extern "C" int anr_sparse_volume_render_lit(const anr_sparse_volume* volume, const float* tau,
                                            int32_t skip, const anr_camera* cameras, int64_t F,
                                            int64_t H, int64_t W, const anr_volume_params* params,
                                            float* rgba, int64_t* counters, anr_stream_t stream) {
  using namespace anr;
  ANR_CHECK_ARG(params != nullptr, "anr_sparse_volume_render_lit: null pointer (params)");
  SpvGeom g;
  const char* why = spv_geom(volume, skip, &g);
  ANR_CHECK_ARG(why == nullptr, "anr_sparse_volume_render_lit: %s", why);
  VolMarch m;
  int64_t tiles_x = 0, tiles_y = 0;
  bool empty = true;
  const int rc = vol_plan("anr_sparse_volume_render_lit", g.nx, g.ny, g.nz, F, H, W, params, &m,
                          &tiles_x, &tiles_y, &empty);
  if (rc != ANR_OK || empty) return rc;
  ANR_CHECK_ARG(g.cells && g.values && (g.coarse || !skip) && tau && cameras && rgba,
                "anr_sparse_volume_render_lit: null pointer");
  const dim3 grid(static_cast<unsigned>(tiles_x * tiles_y * F)), block(kVolThreads);
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counters);
  const int32_t h = static_cast<int32_t>(H), w = static_cast<int32_t>(W);
  const int32_t tx = static_cast<int32_t>(tiles_x), ty = static_cast<int32_t>(tiles_y);
#define ANR_SPV_LAUNCH(S, C)                                                                  \
  hipLaunchKernelGGL((sparse_volume_render_lit_kernel<S, C>), grid, block, 0, as_stream(stream), \
                     g, tau, cameras, h, w, tx, ty, m, rgba, cnt)
  if (skip && cnt)
    ANR_SPV_LAUNCH(true, true);
  else if (skip)
    ANR_SPV_LAUNCH(true, false);
  else if (cnt)
    ANR_SPV_LAUNCH(false, true);
  else
    ANR_SPV_LAUNCH(false, false);
#undef ANR_SPV_LAUNCH
  ANR_CHECK_LAUNCH("anr_sparse_volume_render_lit");
  return ANR_OK;
}
