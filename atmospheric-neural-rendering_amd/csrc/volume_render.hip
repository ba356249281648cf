// Single-scattering ray marcher over a dense density cube: the hot path of the orbit video
// of an extracted volume (the reference's scripts/make_video.py shells out, per frame, to
// OpenVDB's vdb_render, a CPU ray marcher). The arithmetic is this project's own definition,
// written after vdb_render's VolumeRender and its defaults; parity with vdb_render: unpinned.
//
// Cube: (nx, ny, nz) f32, contiguous, z fastest: voxel (i, j, k) at (i * ny + j) * nz + k,
// sitting at the integer position (i, j, k). D(p) is the trilinear interpolation of the eight
// voxels around floor(p), voxels outside the array being 0, so D vanishes outside the box
// [-1, n_d] per axis, and rays are clipped to that box. The cube is read in place: a sample
// whose eight corners are all inside the array (the common case) takes eight unguarded loads,
// any other sample guards each corner. No padded or re-laid-out copy is made.
//
// Pixels: a 256-thread block renders a 16 x 16 pixel tile of one frame, each of its four
// wavefronts an 8 x 8 sub-tile, so the 64 rays of a wavefront stay close together: their
// gathers share cache lines and they leave the march at about the same step. One lane marches
// one pixel; nothing is shared between lanes, so lanes past the image edge simply return.
//
// Arithmetic: f32, evaluated in the order written here with no FMA contraction, which is the
// order tests/volume_checks.py states; expf, sqrtf and the divisions are correctly rounded or
// within one ulp. Every loop also carries an integer bound (the box diagonal over the step,
// plus two) that no ray inside the box can reach: a camera with wild values ends instead of
// marching forever in f32.

#include <cmath>

#include "anr_common.h"

#pragma clang fp contract(off)

namespace anr {

constexpr int kVolThreads = 256;
constexpr int kVolTile = 16;  // pixels per block side; a wavefront takes an 8 x 8 quarter

struct VolCube {
  const float* d;
  int32_t nx, ny, nz;
};

struct VolMarch {
  float ext[3], albedo[3], light[3];
  float primary_step, shadow_step, light_gain, cutoff;
  int32_t max_primary, max_shadow;
};

__device__ __forceinline__ float vol_lerp(float a, float b, float w) { return a + w * (b - a); }

__device__ __forceinline__ float vol_voxel(const VolCube& c, int i, int j, int k) {
  if (i < 0 || j < 0 || k < 0 || i >= c.nx || j >= c.ny || k >= c.nz) return 0.0f;
  return c.d[(i * c.ny + j) * c.nz + k];
}

// D(p): z pairs first (they are neighbours in memory), then y, then x.
__device__ __forceinline__ float vol_sample(const VolCube& c, float px, float py, float pz) {
  const float fx = floorf(px), fy = floorf(py), fz = floorf(pz);
  // no corner inside the array (NaN lands here too): nothing to read, and the float -> int
  // conversions below stay in range
  if (!(fx >= -1.0f && fy >= -1.0f && fz >= -1.0f && fx <= static_cast<float>(c.nx - 1) &&
        fy <= static_cast<float>(c.ny - 1) && fz <= static_cast<float>(c.nz - 1)))
    return 0.0f;
  const float wx = px - fx, wy = py - fy, wz = pz - fz;
  const int i = static_cast<int>(fx), j = static_cast<int>(fy), k = static_cast<int>(fz);
  float v000, v001, v010, v011, v100, v101, v110, v111;
  if (i >= 0 && j >= 0 && k >= 0 && i < c.nx - 1 && j < c.ny - 1 && k < c.nz - 1) {
    const float* q = c.d + ((i * c.ny + j) * c.nz + k);
    const int sy = c.nz, sx = c.ny * c.nz;
    v000 = q[0];
    v001 = q[1];
    v010 = q[sy];
    v011 = q[sy + 1];
    v100 = q[sx];
    v101 = q[sx + 1];
    v110 = q[sx + sy];
    v111 = q[sx + sy + 1];
  } else {
    v000 = vol_voxel(c, i, j, k);
    v001 = vol_voxel(c, i, j, k + 1);
    v010 = vol_voxel(c, i, j + 1, k);
    v011 = vol_voxel(c, i, j + 1, k + 1);
    v100 = vol_voxel(c, i + 1, j, k);
    v101 = vol_voxel(c, i + 1, j, k + 1);
    v110 = vol_voxel(c, i + 1, j + 1, k);
    v111 = vol_voxel(c, i + 1, j + 1, k + 1);
  }
  const float c00 = vol_lerp(v000, v001, wz), c01 = vol_lerp(v010, v011, wz);
  const float c10 = vol_lerp(v100, v101, wz), c11 = vol_lerp(v110, v111, wz);
  return vol_lerp(vol_lerp(c00, c01, wy), vol_lerp(c10, c11, wy), wx);
}

// Slab test of the ray o + t d against the box [-1, n_a] per axis. A zero direction component
// constrains nothing if the origin lies inside that slab and misses otherwise. False on a
// miss (tnear > tfar, the box behind the origin, or NaN anywhere).
__device__ __forceinline__ bool vol_clip(const VolCube& c, const float o[3], const float d[3],
                                         float* tnear, float* tfar) {
  const float hi[3] = {static_cast<float>(c.nx), static_cast<float>(c.ny),
                       static_cast<float>(c.nz)};
  float tn = -INFINITY, tf = INFINITY;
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (d[a] == 0.0f) {
      ok = ok && o[a] >= -1.0f && o[a] <= hi[a];
    } else {
      const float t1 = (-1.0f - o[a]) / d[a], t2 = (hi[a] - o[a]) / d[a];
      const float lo_t = t1 < t2 ? t1 : t2, hi_t = t1 < t2 ? t2 : t1;
      ok = ok && lo_t == lo_t && hi_t == hi_t;
      tn = lo_t > tn ? lo_t : tn;
      tf = hi_t < tf ? hi_t : tf;
    }
  }
  *tnear = tn;
  *tfar = tf;
  return ok && tn <= tf && tf >= 0.0f;
}

__global__ void __launch_bounds__(kVolThreads) volume_render_kernel(
    VolCube cube, const anr_camera* __restrict__ cams, int32_t H, int32_t W, int32_t tiles_x,
    int32_t tiles_y, VolMarch m, float* __restrict__ rgba) {
  // block -> (frame, tile); thread -> pixel of the tile, 8 x 8 per wavefront
  const int32_t tiles = tiles_x * tiles_y;
  const int32_t frame = blockIdx.x / tiles;
  const int32_t tile = blockIdx.x - frame * tiles;
  const int32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int32_t col = tx * kVolTile + (wave & 1) * 8 + (lane & 7);
  const int32_t row = ty * kVolTile + (wave >> 1) * 8 + (lane >> 3);
  if (col >= W || row >= H) return;
  float* out = rgba + ((static_cast<int64_t>(frame) * H + row) * W + col) * 4;

  const anr_camera cam = cams[frame];
  const float u = 2.0f * (static_cast<float>(col) + 0.5f) / static_cast<float>(W) - 1.0f;
  const float v = 2.0f * (static_cast<float>(row) + 0.5f) / static_cast<float>(H) - 1.0f;
  float dir[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) dir[a] = cam.forward[a] + u * cam.right[a] - v * cam.up[a];
  const float len = sqrtf(dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2]);
#pragma unroll
  for (int a = 0; a < 3; ++a) dir[a] = dir[a] / len;

  float t0, t1;
  if (!vol_clip(cube, cam.eye, dir, &t0, &t1)) {
    out[0] = 0.0f;
    out[1] = 0.0f;
    out[2] = 0.0f;
    out[3] = 0.0f;
    return;
  }
  t0 = t0 > 0.0f ? t0 : 0.0f;

  float T[3] = {1.0f, 1.0f, 1.0f}, L[3] = {0.0f, 0.0f, 0.0f};
  const float tstart = m.primary_step * ceilf(t0 / m.primary_step);
  for (int32_t n = 0; n < m.max_primary; ++n) {
    const float t = tstart + static_cast<float>(n) * m.primary_step;
    if (!(t <= t1)) break;
    float p[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = cam.eye[a] + t * dir[a];
    const float d = vol_sample(cube, p[0], p[1], p[2]);
    if (d < m.cutoff) continue;
    // shadow ray towards the light
    float sT[3] = {1.0f, 1.0f, 1.0f};
    float s0, s1;
    if (vol_clip(cube, p, m.light, &s0, &s1)) {
      for (int32_t q = 1; q <= m.max_shadow; ++q) {
        const float s = static_cast<float>(q) * m.shadow_step;
        if (!(s <= s1)) break;
        const float ds = vol_sample(cube, p[0] + s * m.light[0], p[1] + s * m.light[1],
                                    p[2] + s * m.light[2]);
        if (ds < m.cutoff) continue;
        const float gain = 1.0f + s * m.light_gain;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) sT[ch] *= expf(m.ext[ch] * ds * m.shadow_step / gain);
        if (sT[0] * sT[0] + sT[1] * sT[1] + sT[2] * sT[2] < m.cutoff) break;
      }
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float dT = expf(m.ext[ch] * d * m.primary_step);
      L[ch] += m.albedo[ch] * sT[ch] * T[ch] * (1.0f - dT);
      T[ch] *= dT;
    }
    if (T[0] * T[0] + T[1] * T[1] + T[2] * T[2] < m.cutoff) break;
  }
  out[0] = L[0];
  out[1] = L[1];
  out[2] = L[2];
  out[3] = 1.0f - (T[0] + T[1] + T[2]) / 3.0f;
}

}  // namespace anr

extern "C" int anr_volume_render(const float* density, int64_t nx, int64_t ny, int64_t nz,
                                 const anr_camera* cameras, int64_t F, int64_t H, int64_t W,
                                 const anr_volume_params* params, float* rgba,
                                 anr_stream_t stream) {
  using namespace anr;
  ANR_CHECK_ARG(params != nullptr, "anr_volume_render: null pointer (params)");
  ANR_CHECK_ARG(nx >= 1 && ny >= 1 && nz >= 1, "anr_volume_render: cube extents must be >= 1");
  ANR_CHECK_ARG(nx < (1LL << 31) && ny < (1LL << 31) && nz < (1LL << 31) &&
                    nx * ny < (1LL << 31) && nx * ny * nz * 4 < (1LL << 31),
                "anr_volume_render: cube of 2^31 bytes or more (32-bit offsets)");
  ANR_CHECK_ARG(F >= 0 && H >= 0 && W >= 0, "anr_volume_render: negative image size");
  const anr_volume_params& p = *params;
  ANR_CHECK_ARG(p.primary_step > 0.0f && p.shadow_step > 0.0f && std::isfinite(p.primary_step) &&
                    std::isfinite(p.shadow_step),
                "anr_volume_render: steps must be positive and finite");
  ANR_CHECK_ARG(p.light_gain >= 0.0f && p.cutoff >= 0.0f && std::isfinite(p.light_gain) &&
                    std::isfinite(p.cutoff),
                "anr_volume_render: negative coefficient (light_gain, cutoff)");
  double l2 = 0.0;
  for (int a = 0; a < 3; ++a) {
    ANR_CHECK_ARG(p.absorb[a] >= 0.0f && p.scatter[a] >= 0.0f && p.light_color[a] >= 0.0f &&
                      std::isfinite(p.absorb[a]) && std::isfinite(p.scatter[a]) &&
                      std::isfinite(p.light_color[a]),
                  "anr_volume_render: negative coefficient (absorb, scatter, light_color)");
    l2 += static_cast<double>(p.light_dir[a]) * p.light_dir[a];
  }
  ANR_CHECK_ARG(fabs(sqrt(l2) - 1.0) <= 1e-3, "anr_volume_render: light_dir must be unit length");
  if (F == 0 || H == 0 || W == 0) return ANR_OK;
  ANR_CHECK_ARG(H < (1LL << 24) && W < (1LL << 24), "anr_volume_render: image side of 2^24 or more");
  const int64_t tiles_x = ceil_div(W, kVolTile), tiles_y = ceil_div(H, kVolTile);
  ANR_CHECK_ARG(tiles_x * tiles_y < (1LL << 31) && F < (1LL << 31) &&
                    tiles_x * tiles_y * F < (1LL << 31),
                "anr_volume_render: too many pixels for one launch (2^31 tiles or more)");
  ANR_CHECK_ARG(density && cameras && rgba, "anr_volume_render: null pointer");

  VolMarch m;
  for (int a = 0; a < 3; ++a) {
    // f32 as the definition has them: ext = -(absorb + scatter), albedo = light_color *
    // scatter / (absorb + scatter), 0 where the denominator is 0
    const float sum = p.absorb[a] + p.scatter[a];
    m.ext[a] = -sum;
    m.albedo[a] = sum == 0.0f ? 0.0f : p.light_color[a] * p.scatter[a] / sum;
    m.light[a] = p.light_dir[a];
  }
  m.primary_step = p.primary_step;
  m.shadow_step = p.shadow_step;
  m.light_gain = p.light_gain;
  m.cutoff = p.cutoff;
  // no ray inside the box [-1, n] takes more steps than the box diagonal over the step
  const double diag = sqrt(static_cast<double>(nx + 1) * (nx + 1) +
                           static_cast<double>(ny + 1) * (ny + 1) +
                           static_cast<double>(nz + 1) * (nz + 1));
  const double np_ = diag / p.primary_step + 2.0, ns_ = diag / p.shadow_step + 2.0;
  ANR_CHECK_ARG(np_ < 2147483000.0 && ns_ < 2147483000.0,
                "anr_volume_render: steps too small for the cube (2^31 steps or more per ray)");
  m.max_primary = static_cast<int32_t>(np_) + 1;
  m.max_shadow = static_cast<int32_t>(ns_) + 1;

  const VolCube cube{density, static_cast<int32_t>(nx), static_cast<int32_t>(ny),
                     static_cast<int32_t>(nz)};
  hipLaunchKernelGGL(volume_render_kernel, dim3(static_cast<unsigned>(tiles_x * tiles_y * F)),
                     dim3(kVolThreads), 0, as_stream(stream), cube, cameras,
                     static_cast<int32_t>(H), static_cast<int32_t>(W),
                     static_cast<int32_t>(tiles_x), static_cast<int32_t>(tiles_y), m, rgba);
  ANR_CHECK_LAUNCH("anr_volume_render");
  return ANR_OK;
}
