// Exact voxel traversal of rays into a bitmap, and the bitmap's ordered compaction: the hot
// path of the global-grid extract (datasets/harp2_extract.py:794-903; the reference walks
// its rays with graphics_utils.voxel_traversal, a Python loop after Amanatides & Woo that
// accumulates tmax += tdelta in f32 and calls torch.unique per chunk of rays).
//
// Bitmap: one bit per voxel of a box with origin (i0, j0, k0) and extents (ni, nj, nk), i
// along x and fastest, k slowest. A row of ni voxels takes row_pitch bits, a multiple of 32
// that is >= ni, so every x-row starts on a uint32 word; bit b of word w of a row is voxel
// i = i0 + 32 w + b. The pad bits of a row are never set.
//
// Traversal: one thread per ray, f64, no contraction. The number of steps is known before
// the walk, sum over the axes of |floor(end_a) - floor(u_a)|, so the loop has no
// floating-point termination test and cannot pass the end voxel. Every step advances the
// axis, among those not yet at their end index, whose next boundary is crossed first; the
// crossing time comes from the boundary index itself, t_a = (b_a - u_a) * (1 / d_a), never
// from a running sum. Ties go to the lowest axis. An axis whose two floors agree (d_a = 0
// among them) never advances. Each axis moves monotonically between its two floors, so a ray
// whose two end voxels lie in the box stays in it: the walk needs no bounds test, and a ray
// with an end voxel outside the box marks nothing and is counted instead.
//
// Marking: consecutive steps of a ray often stay in one word (steps along x), and the rays
// of neighbouring pixels walk the same voxels. The thread keeps the current word index and
// a pending mask in registers and writes the mask when the word changes and at the end. A
// plain load first skips the atomic when every pending bit is already set; a stale value
// only costs that shortcut, because OR is idempotent. The write is a no-return atomicOr.
//
// Compaction: count per block of 1024 words, exclusive scan by the caller, then every thread
// writes the voxels of its four words in ascending bit order, so the output is in ascending
// bitmap order whatever the rays' order, chunking or run.

#include "anr_common.h"

#pragma clang fp contract(off)

namespace anr {

constexpr int kVoxThreads = 256;
constexpr int kVoxWords = 4;  // bitmap words per thread in count / compact
constexpr int kVoxBlockWords = kVoxThreads * kVoxWords;

struct VoxBox {
  int32_t i0, j0, k0;
  int32_t ni, nj, nk;
  int64_t pitch_words;  // uint32 words per x-row
  int64_t n_words;      // pitch_words * nj * nk
};

// Block-wide exclusive scan of one count per thread (4 waves).
__device__ __forceinline__ int vox_excl_scan(int v, int* total) {
  __shared__ int wsum[kVoxThreads / kWave];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int y = __shfl_up(x, d, kWave);
    if (lane >= d) x += y;
  }
  if (lane == 63) wsum[wave] = x;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < kVoxThreads / kWave; ++w) {
    if (w < wave) base += wsum[w];
    tot += wsum[w];
  }
  *total = tot;
  return base + x - v;
}

template <bool kShortcut>
__device__ __forceinline__ void vox_flush(uint32_t* __restrict__ bitmap, int64_t w,
                                          uint32_t mask) {
  if (kShortcut) {
    const uint32_t seen = bitmap[w];
    if ((seen & mask) == mask) return;
  }
  atomicOr(bitmap + w, mask);
}

template <bool kShortcut>
__global__ void __launch_bounds__(kVoxThreads) voxel_traverse_kernel(
    const double* __restrict__ u, const double* __restrict__ end, int64_t R, VoxBox box,
    uint32_t* __restrict__ bitmap, unsigned long long* __restrict__ counters) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kVoxThreads + threadIdx.x;
  if (r >= R) return;
  double p[3], d[3], fu[3], fe[3];
  bool finite = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    p[a] = u[r * 3 + a];
    const double e = end[r * 3 + a];
    finite = finite && isfinite(p[a]) && isfinite(e);
    d[a] = e - p[a];
    fu[a] = floor(p[a]);
    fe[a] = floor(e);
  }
  if (!finite) {
    atomicAdd(counters + 0, 1ULL);
    return;
  }
  // both end voxels inside the box (compared as doubles: exact, and no int overflow)
  const double lo[3] = {static_cast<double>(box.i0), static_cast<double>(box.j0),
                        static_cast<double>(box.k0)};
  const double ext[3] = {static_cast<double>(box.ni), static_cast<double>(box.nj),
                         static_cast<double>(box.nk)};
  bool inside = true;
  double steps_d = 0.0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    inside = inside && fu[a] >= lo[a] && fu[a] < lo[a] + ext[a] && fe[a] >= lo[a] &&
             fe[a] < lo[a] + ext[a];
    steps_d += fabs(fe[a] - fu[a]);
  }
  if (!inside) {
    // its voxels are not marked: count them (saturating far below 2^64 for wild endpoints)
    const double n = steps_d + 1.0;
    atomicAdd(counters + 1, n < 1e15 ? static_cast<unsigned long long>(n) : 1000000000000000ULL);
    return;
  }
  // indices relative to the box, all in [0, extent)
  int32_t idx[3], last[3], sgn[3];
  double inv[3], bnd[3], dbnd[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    idx[a] = static_cast<int32_t>(fu[a] - lo[a]);
    last[a] = static_cast<int32_t>(fe[a] - lo[a]);
    sgn[a] = last[a] > idx[a] ? 1 : -1;
    inv[a] = 1.0 / d[a];  // used only while idx != last, where d[a] != 0
    // the next integer boundary along a, as a double: an integer below 2^31, so it and its
    // +-1 updates are exact (this is the boundary index, not a running time)
    bnd[a] = sgn[a] > 0 ? fu[a] + 1.0 : fu[a];
    dbnd[a] = static_cast<double>(sgn[a]);
  }
  const int64_t steps = static_cast<int64_t>(steps_d);
  const int64_t row_words = box.pitch_words;
  int64_t row = (static_cast<int64_t>(idx[2]) * box.nj + idx[1]) * row_words;
  int64_t w = row + (idx[0] >> 5);
  uint32_t mask = 1u << (idx[0] & 31);
  for (int64_t s = 0; s < steps; ++s) {
    int best = -1;
    double tbest = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (idx[a] != last[a]) {
        const double t = (bnd[a] - p[a]) * inv[a];
        if (best < 0 || t < tbest) {
          best = a;
          tbest = t;
        }
      }
    }
    // steps counts exactly the moves left, so an axis is always found
    if (best == 0) {
      idx[0] += sgn[0];
      bnd[0] += dbnd[0];
    } else if (best == 1) {
      idx[1] += sgn[1];
      bnd[1] += dbnd[1];
      row += sgn[1] * row_words;
    } else {
      idx[2] += sgn[2];
      bnd[2] += dbnd[2];
      row += sgn[2] * row_words * box.nj;
    }
    const int64_t wn = row + (idx[0] >> 5);
    if (wn != w) {
      vox_flush<kShortcut>(bitmap, w, mask);
      w = wn;
      mask = 0u;
    }
    mask |= 1u << (idx[0] & 31);
  }
  vox_flush<kShortcut>(bitmap, w, mask);
}

__global__ void __launch_bounds__(kVoxThreads) voxel_count_kernel(
    const uint32_t* __restrict__ bitmap, int64_t n_words, int32_t* __restrict__ counts) {
  const int64_t w0 = static_cast<int64_t>(blockIdx.x) * kVoxBlockWords + threadIdx.x * kVoxWords;
  int c = 0;
#pragma unroll
  for (int i = 0; i < kVoxWords; ++i)
    if (w0 + i < n_words) c += __popc(bitmap[w0 + i]);
  int total;
  vox_excl_scan(c, &total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kVoxThreads) voxel_compact_kernel(
    const uint32_t* __restrict__ bitmap, VoxBox box, const int64_t* __restrict__ offsets,
    int64_t n_out, int32_t* __restrict__ out) {
  const int64_t w0 = static_cast<int64_t>(blockIdx.x) * kVoxBlockWords + threadIdx.x * kVoxWords;
  uint32_t words[kVoxWords];
  int c = 0;
#pragma unroll
  for (int i = 0; i < kVoxWords; ++i) {
    words[i] = w0 + i < box.n_words ? bitmap[w0 + i] : 0u;
    c += __popc(words[i]);
  }
  int total;
  int64_t o = offsets[blockIdx.x] + vox_excl_scan(c, &total);
#pragma unroll
  for (int i = 0; i < kVoxWords; ++i) {
    uint32_t m = words[i];
    if (m == 0u) continue;
    const int64_t row = (w0 + i) / box.pitch_words;
    const int32_t wi = static_cast<int32_t>((w0 + i) - row * box.pitch_words);
    const int32_t k = box.k0 + static_cast<int32_t>(row / box.nj);
    const int32_t j = box.j0 + static_cast<int32_t>(row % box.nj);
    while (m != 0u) {
      const int b = __ffs(m) - 1;
      m &= m - 1u;
      if (o < n_out) {  // offsets that disagree with the bitmap cannot write past the output
        out[o * 3 + 0] = box.i0 + wi * 32 + b;
        out[o * 3 + 1] = j;
        out[o * 3 + 2] = k;
      }
      ++o;
    }
  }
}

// The box of an entry's arguments; nullptr and a message in *why when they are bad.
static const char* make_box(int32_t i0, int32_t j0, int32_t k0, int32_t ni, int32_t nj,
                            int32_t nk, int64_t row_pitch, VoxBox* box) {
  if (ni < 1 || nj < 1 || nk < 1) return "extents must be >= 1";
  if (row_pitch < ni || row_pitch % 32 != 0 || row_pitch > (1LL << 31))
    return "row_pitch must be a multiple of 32 that is >= ni";
  // the far corner must be an int32 index too
  if (static_cast<int64_t>(i0) + ni > (1LL << 31) || static_cast<int64_t>(j0) + nj > (1LL << 31) ||
      static_cast<int64_t>(k0) + nk > (1LL << 31))
    return "origin + extent overflows int32";
  int64_t bits = 0;
  if (__builtin_mul_overflow(row_pitch, static_cast<int64_t>(nj), &bits) ||
      __builtin_mul_overflow(bits, static_cast<int64_t>(nk), &bits) || bits >= (1LL << 46))
    return "bit count of the box overflows (2^46 bits or more)";
  *box = VoxBox{i0, j0, k0, ni, nj, nk, row_pitch / 32, bits / 32};
  return nullptr;
}

}  // namespace anr

extern "C" int64_t anr_voxel_n_blocks(int64_t n_words) {
  return n_words <= 0 ? 0 : anr::ceil_div(n_words, anr::kVoxBlockWords);
}

extern "C" int anr_voxel_traverse(const double* u, const double* end, int64_t R, int32_t i0,
                                  int32_t j0, int32_t k0, int32_t ni, int32_t nj, int32_t nk,
                                  int64_t row_pitch, uint32_t* bitmap, int64_t* counters,
                                  int32_t shortcut, anr_stream_t stream) {
  using namespace anr;
  ANR_CHECK_ARG(R >= 0 && R < (1LL << 31), "anr_voxel_traverse: bad R %lld",
                static_cast<long long>(R));
  VoxBox box;
  const char* why = make_box(i0, j0, k0, ni, nj, nk, row_pitch, &box);
  ANR_CHECK_ARG(why == nullptr, "anr_voxel_traverse: %s", why);
  ANR_CHECK_ARG(shortcut == 0 || shortcut == 1, "anr_voxel_traverse: shortcut must be 0 or 1");
  if (R == 0) return ANR_OK;
  ANR_CHECK_ARG(u && end && bitmap && counters, "anr_voxel_traverse: null pointer");
  const dim3 grid(static_cast<unsigned>(ceil_div(R, kVoxThreads))), block(kVoxThreads);
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counters);
  if (shortcut)
    hipLaunchKernelGGL(voxel_traverse_kernel<true>, grid, block, 0, as_stream(stream), u, end, R,
                       box, bitmap, cnt);
  else
    hipLaunchKernelGGL(voxel_traverse_kernel<false>, grid, block, 0, as_stream(stream), u, end, R,
                       box, bitmap, cnt);
  ANR_CHECK_LAUNCH("anr_voxel_traverse");
  return ANR_OK;
}

extern "C" int anr_voxel_count(const uint32_t* bitmap, int32_t ni, int32_t nj, int32_t nk,
                               int64_t row_pitch, int32_t* counts, anr_stream_t stream) {
  using namespace anr;
  VoxBox box;
  const char* why = make_box(0, 0, 0, ni, nj, nk, row_pitch, &box);
  ANR_CHECK_ARG(why == nullptr, "anr_voxel_count: %s", why);
  ANR_CHECK_ARG(bitmap && counts, "anr_voxel_count: null pointer");
  const int64_t blocks = ceil_div(box.n_words, kVoxBlockWords);  // < 2^31 (make_box)
  hipLaunchKernelGGL(voxel_count_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kVoxThreads), 0,
                     as_stream(stream), bitmap, box.n_words, counts);
  ANR_CHECK_LAUNCH("anr_voxel_count");
  return ANR_OK;
}

extern "C" int anr_voxel_compact(const uint32_t* bitmap, int32_t i0, int32_t j0, int32_t k0,
                                 int32_t ni, int32_t nj, int32_t nk, int64_t row_pitch,
                                 const int64_t* offsets, int64_t n_out, int32_t* voxels,
                                 anr_stream_t stream) {
  using namespace anr;
  VoxBox box;
  const char* why = make_box(i0, j0, k0, ni, nj, nk, row_pitch, &box);
  ANR_CHECK_ARG(why == nullptr, "anr_voxel_compact: %s", why);
  ANR_CHECK_ARG(n_out >= 0 && n_out < (1LL << 60) / 12, "anr_voxel_compact: bad n_out %lld",
                static_cast<long long>(n_out));
  if (n_out == 0) return ANR_OK;
  ANR_CHECK_ARG(bitmap && offsets && voxels, "anr_voxel_compact: null pointer");
  const int64_t blocks = ceil_div(box.n_words, kVoxBlockWords);  // < 2^31 (make_box)
  hipLaunchKernelGGL(voxel_compact_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kVoxThreads),
                     0, as_stream(stream), bitmap, box, offsets, n_out, voxels);
  ANR_CHECK_LAUNCH("anr_voxel_compact");
  return ANR_OK;
}
