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

__global__ void __launch_bounds__(kVolThreads) volume_render_kernel(
    VolCube cube, const anr_camera* __restrict__ cams, int32_t H, int32_t W, int32_t tiles_x,
    int32_t tiles_y, VolMarch m, float* __restrict__ rgba) {
  vol_march_pixel(cube, cams, H, W, tiles_x, tiles_y, m, rgba);
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
  VolMarch m;
  int64_t tiles_x = 0, tiles_y = 0;
  bool empty = true;
  const int rc =
      vol_plan("anr_volume_render", nx, ny, nz, F, H, W, params, &m, &tiles_x, &tiles_y, &empty);
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
