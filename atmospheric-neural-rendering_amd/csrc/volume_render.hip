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
// The march itself (pixels, clip, loops, arithmetic order, integer bounds) is volume_march.h,
// shared with the sparse volume of sparse_volume.hip; this file is the dense accessor.
//
// Light volume (opt-in): anr_volume_light sums tau, one thread per voxel, into a second cube of
// the same layout (0 where the density is not > 0); anr_volume_render_lit marches with
// VolCubeLit, whose lit sample reads tau at the offsets of the eight densities.

#include "volume_march.h"

#pragma clang fp contract(off)

namespace anr {

struct VolCube {
  const float* d;
  int32_t nx, ny, nz;

  __device__ __forceinline__ float voxel(int i, int j, int k) const {
    if (i < 0 || j < 0 || k < 0 || i >= nx || j >= ny || k >= nz) return 0.0f;
    return d[(i * ny + j) * nz + k];
  }

  // D(p): z pairs first (they are neighbours in memory), then y, then x.
  __device__ __forceinline__ float sample(float px, float py, float pz) const {
    const float fx = floorf(px), fy = floorf(py), fz = floorf(pz);
    // no corner inside the array (NaN lands here too): nothing to read, and the float -> int
    // conversions below stay in range
    if (!(fx >= -1.0f && fy >= -1.0f && fz >= -1.0f && fx <= static_cast<float>(nx - 1) &&
          fy <= static_cast<float>(ny - 1) && fz <= static_cast<float>(nz - 1)))
      return 0.0f;
    const float wx = px - fx, wy = py - fy, wz = pz - fz;
    const int i = static_cast<int>(fx), j = static_cast<int>(fy), k = static_cast<int>(fz);
    float v000, v001, v010, v011, v100, v101, v110, v111;
    if (i >= 0 && j >= 0 && k >= 0 && i < nx - 1 && j < ny - 1 && k < nz - 1) {
      const float* q = d + ((i * ny + j) * nz + k);
      const int sy = nz, sx = ny * nz;
      v000 = q[0];
      v001 = q[1];
      v010 = q[sy];
      v011 = q[sy + 1];
      v100 = q[sx];
      v101 = q[sx + 1];
      v110 = q[sx + sy];
      v111 = q[sx + sy + 1];
    } else {
      v000 = voxel(i, j, k);
      v001 = voxel(i, j, k + 1);
      v010 = voxel(i, j + 1, k);
      v011 = voxel(i, j + 1, k + 1);
      v100 = voxel(i + 1, j, k);
      v101 = voxel(i + 1, j, k + 1);
      v110 = voxel(i + 1, j + 1, k);
      v111 = voxel(i + 1, j + 1, k + 1);
    }
    return vol_trilerp(v000, v001, v010, v011, v100, v101, v110, v111, wx, wy, wz);
  }
};

// The cube with its light volume: tau has the cube's layout.
struct VolCubeLit : VolCube {
  const float* tau;

  // sample(p), and in *tau_hat, where that is >= cutoff, the mean of tau over the corners
  // with density > 0 (vol_lit_corners). The same loads feed both, so d is sample(p)'s value.
  __device__ __forceinline__ float lit_sample(float px, float py, float pz, float cutoff,
                                              float* tau_hat) const {
    const float fx = floorf(px), fy = floorf(py), fz = floorf(pz);
    if (!(fx >= -1.0f && fy >= -1.0f && fz >= -1.0f && fx <= static_cast<float>(nx - 1) &&
          fy <= static_cast<float>(ny - 1) && fz <= static_cast<float>(nz - 1)))
      return 0.0f;
    const float wx = px - fx, wy = py - fy, wz = pz - fz;
    const int i = static_cast<int>(fx), j = static_cast<int>(fy), k = static_cast<int>(fz);
    // offsets of the corners in x-outer, z-inner order; -1 outside the array
    int at[8];
    float v[8];
    if (i >= 0 && j >= 0 && k >= 0 && i < nx - 1 && j < ny - 1 && k < nz - 1) {
      const int base = (i * ny + j) * nz + k, sy = nz, sx = ny * nz;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        at[c] = base + (c >> 2) * sx + ((c >> 1) & 1) * sy + (c & 1);
        v[c] = d[at[c]];
      }
    } else {
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int ci = i + (c >> 2), cj = j + ((c >> 1) & 1), ck = k + (c & 1);
        const bool in = ci >= 0 && cj >= 0 && ck >= 0 && ci < nx && cj < ny && ck < nz;
        at[c] = in ? (ci * ny + cj) * nz + ck : -1;
        v[c] = in ? d[at[c]] : 0.0f;
      }
    }
    const float dens = vol_trilerp(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], wx, wy, wz);
    if (dens < cutoff) return dens;
    float tv[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) tv[c] = v[c] > 0.0f ? tau[at[c]] : 0.0f;
    *tau_hat = vol_lit_corners(v, tv, wx, wy, wz);
    return dens;
  }
};

__global__ void __launch_bounds__(kVolThreads) volume_render_lit_kernel(
    VolCubeLit cube, const anr_camera* __restrict__ cams, int32_t H, int32_t W, int32_t tiles_x,
    int32_t tiles_y, VolMarch m, float* __restrict__ rgba) {
  vol_march_pixel<true>(cube, cams, H, W, tiles_x, tiles_y, m, rgba);
}

// One thread per voxel, z fastest: tau of the voxels with density > 0, 0 elsewhere.
__global__ void __launch_bounds__(kVolThreads) volume_light_kernel(VolCube cube, int32_t n,
                                                                   VolMarch m,
                                                                   float* __restrict__ tau) {
  const int32_t r = static_cast<int32_t>(blockIdx.x) * kVolThreads + threadIdx.x;
  if (r >= n) return;
  float t = 0.0f;
  if (cube.d[r] > 0.0f) {
    const int32_t ij = r / cube.nz;
    const float p[3] = {static_cast<float>(ij / cube.ny), static_cast<float>(ij % cube.ny),
                        static_cast<float>(r - ij * cube.nz)};
    t = vol_light_tau(cube, p, m);
  }
  tau[r] = t;
}

__global__ void __launch_bounds__(kVolThreads) volume_render_kernel(
    VolCube cube, const anr_camera* __restrict__ cams, int32_t H, int32_t W, int32_t tiles_x,
    int32_t tiles_y, VolMarch m, float* __restrict__ rgba) {
  vol_march_pixel(cube, cams, H, W, tiles_x, tiles_y, m, rgba);
}

}  // namespace anr

namespace anr {

// The refusals every dense entry shares (params, cube, image) and the launch plan.
static int vol_cube_plan(const char* who, int64_t nx, int64_t ny, int64_t nz, int64_t F, int64_t H,
                         int64_t W, const anr_volume_params* params, VolMarch* m, int64_t* tiles_x,
                         int64_t* tiles_y, bool* empty) {
  *empty = true;
  ANR_CHECK_ARG(params != nullptr, "%s: null pointer (params)", who);
  ANR_CHECK_ARG(nx >= 1 && ny >= 1 && nz >= 1, "%s: cube extents must be >= 1", who);
  ANR_CHECK_ARG(nx < (1LL << 31) && ny < (1LL << 31) && nz < (1LL << 31) &&
                    nx * ny < (1LL << 31) && nx * ny * nz * 4 < (1LL << 31),
                "%s: cube of 2^31 bytes or more (32-bit offsets)", who);
  return vol_plan(who, nx, ny, nz, F, H, W, params, m, tiles_x, tiles_y, empty);
}

}  // namespace anr

extern "C" int anr_volume_render(const float* density, int64_t nx, int64_t ny, int64_t nz,
                                 const anr_camera* cameras, int64_t F, int64_t H, int64_t W,
                                 const anr_volume_params* params, float* rgba,
                                 anr_stream_t stream) {
  using namespace anr;
  VolMarch m;
  int64_t tiles_x = 0, tiles_y = 0;
  bool empty = true;
  const int rc = vol_cube_plan("anr_volume_render", nx, ny, nz, F, H, W, params, &m, &tiles_x,
                               &tiles_y, &empty);
  if (rc != ANR_OK || empty) return rc;
  ANR_CHECK_ARG(density && cameras && rgba, "anr_volume_render: null pointer");

  const VolCube cube{density, static_cast<int32_t>(nx), static_cast<int32_t>(ny),
                     static_cast<int32_t>(nz)};
  hipLaunchKernelGGL(volume_render_kernel, dim3(static_cast<unsigned>(tiles_x * tiles_y * F)),
                     dim3(kVolThreads), 0, as_stream(stream), cube, cameras,
                     static_cast<int32_t>(H), static_cast<int32_t>(W),
                     static_cast<int32_t>(tiles_x), static_cast<int32_t>(tiles_y), m, rgba);
  ANR_CHECK_LAUNCH("anr_volume_render");
  return ANR_OK;
}

extern "C" int anr_volume_light(const float* density, int64_t nx, int64_t ny, int64_t nz,
                                const anr_volume_params* params, float* tau,
                                anr_stream_t stream) {
  using namespace anr;
  VolMarch m;
  int64_t tiles_x = 0, tiles_y = 0;
  bool empty = true;
  // the plan of a 1 x 1 image: its refusals and the walk's integer bound
  const int rc = vol_cube_plan("anr_volume_light", nx, ny, nz, 1, 1, 1, params, &m, &tiles_x,
                               &tiles_y, &empty);
  if (rc != ANR_OK) return rc;
  ANR_CHECK_ARG(density && tau, "anr_volume_light: null pointer");
  const VolCube cube{density, static_cast<int32_t>(nx), static_cast<int32_t>(ny),
                     static_cast<int32_t>(nz)};
  const int64_t n = nx * ny * nz;  // < 2^29
  hipLaunchKernelGGL(volume_light_kernel, dim3(static_cast<unsigned>(ceil_div(n, kVolThreads))),
                     dim3(kVolThreads), 0, as_stream(stream), cube, static_cast<int32_t>(n), m,
                     tau);
  ANR_CHECK_LAUNCH("anr_volume_light");
  return ANR_OK;
}

extern "C" int anr_volume_render_lit(const float* density, const float* tau, int64_t nx,
                                     int64_t ny, int64_t nz, const anr_camera* cameras, int64_t F,
                                     int64_t H, int64_t W, const anr_volume_params* params,
                                     float* rgba, anr_stream_t stream) {
  using namespace anr;
  VolMarch m;
  int64_t tiles_x = 0, tiles_y = 0;
  bool empty = true;
  const int rc = vol_cube_plan("anr_volume_render_lit", nx, ny, nz, F, H, W, params, &m, &tiles_x,
                               &tiles_y, &empty);
  if (rc != ANR_OK || empty) return rc;
  ANR_CHECK_ARG(density && tau && cameras && rgba, "anr_volume_render_lit: null pointer");

  VolCubeLit cube;
  cube.d = density;
  cube.nx = static_cast<int32_t>(nx);
  cube.ny = static_cast<int32_t>(ny);
  cube.nz = static_cast<int32_t>(nz);
  cube.tau = tau;
  hipLaunchKernelGGL(volume_render_lit_kernel,
                     dim3(static_cast<unsigned>(tiles_x * tiles_y * F)), dim3(kVolThreads), 0,
                     as_stream(stream), cube, cameras, static_cast<int32_t>(H),
                     static_cast<int32_t>(W), static_cast<int32_t>(tiles_x),
                     static_cast<int32_t>(tiles_y), m, rgba);
  ANR_CHECK_LAUNCH("anr_volume_render_lit");
  return ANR_OK;
}
