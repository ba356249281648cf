// The single-scattering march of the orbit video, shared by the dense cube
// (volume_render.hip) and the sparse volume (sparse_volume.hip): the pixel's ray, the slab
// clip, the primary and the shadow loop, templated on the volume accessor. An accessor Vol has
//   int32_t nx, ny, nz;                       the box: D vanishes outside [-1, n_d] per axis
//   float sample(float px, float py, float pz);   D(p) as include/anr.h defines it
// and nothing else of it is used here, so both volumes take the same steps at the same t, and
// only where the eight values of a sample come from differs.
//
// Light volume (the second, opt-in shadow mode; include/anr.h "Light volume"): the light does
// not move during an orbit, so the shadow optical depth tau of every voxel is summed once
// (vol_light_tau: the shadow loop below without its early termination) and the lit march
// (vol_march_pixel<true>) interpolates it where the marched mode casts a shadow ray. An
// accessor of the lit march also has
//   float lit_sample(float px, float py, float pz, float cutoff, float* tau_hat);
// which returns sample(p) and, where that is >= cutoff, the weighted mean of tau over the
// corners with density > 0 (vol_lit_corners), from the same eight corner loads.
//
// Pixels: a 256-thread block renders a 16 x 16 pixel tile of one frame, each of its four
// wavefronts an 8 x 8 sub-tile, so the 64 rays of a wavefront stay close together: their
// gathers share cache lines and they leave the march at about the same step. One lane marches
// one pixel; nothing is shared between lanes, so lanes past the image edge simply return.
//
// Arithmetic: f32, evaluated in the order written here with no FMA contraction, which is the
// order tests/volume_checks.py states; expf, sqrtf and the divisions are correctly rounded or
// within one ulp. Every t comes from the step index, never from a running sum. Every loop also
// carries an integer bound (the box diagonal over the step, plus two) that no ray inside the
// box can reach: a camera with wild values ends instead of marching forever in f32.
//
// Include after `#pragma clang fp contract(off)`; the header sets it again for itself.
#pragma once

#include <cmath>

#include "anr_common.h"

#pragma clang fp contract(off)

namespace anr {

constexpr int kVolThreads = 256;
constexpr int kVolTile = 16;  // pixels per block side; a wavefront takes an 8 x 8 quarter

struct VolMarch {
  float ext[3], albedo[3], light[3];
  float primary_step, shadow_step, light_gain, cutoff;
  int32_t max_primary, max_shadow;
};

__device__ __forceinline__ float vol_lerp(float a, float b, float w) { return a + w * (b - a); }

// The trilinear value of eight corners v[x][y][z]: z pairs first, then y, then x.
__device__ __forceinline__ float vol_trilerp(float v000, float v001, float v010, float v011,
                                             float v100, float v101, float v110, float v111,
                                             float wx, float wy, float wz) {
  const float c00 = vol_lerp(v000, v001, wz), c01 = vol_lerp(v010, v011, wz);
  const float c10 = vol_lerp(v100, v101, wz), c11 = vol_lerp(v110, v111, wz);
  return vol_lerp(vol_lerp(c00, c01, wy), vol_lerp(c10, c11, wy), wx);
}

// Slab test of the ray o + t d against the box [-1, n_a] per axis. A zero direction component
// constrains nothing if the origin lies inside that slab and misses otherwise. False on a
// miss (tnear > tfar, the box behind the origin, or NaN anywhere).
__device__ __forceinline__ bool vol_clip(int32_t nx, int32_t ny, int32_t nz, const float o[3],
                                         const float d[3], float* tnear, float* tfar) {
  const float hi[3] = {static_cast<float>(nx), static_cast<float>(ny), static_cast<float>(nz)};
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

// tau of the voxel at p: the shadow loop of vol_march_pixel from p (the light ray clipped to
// the box, s = shadow_step, 2 shadow_step, ... <= s1, samples below cutoff skipped, the
// integer bound kept) as a plain sum of optical depths: never ended early, and the same for
// every channel. Shared by the dense and the sparse light build.
template <typename Vol>
__device__ __forceinline__ float vol_light_tau(Vol& vol, const float p[3], const VolMarch& m) {
  float tau = 0.0f;
  float s0, s1;
  if (!vol_clip(vol.nx, vol.ny, vol.nz, p, m.light, &s0, &s1)) return tau;
  for (int32_t q = 1; q <= m.max_shadow; ++q) {
    const float s = static_cast<float>(q) * m.shadow_step;
    if (!(s <= s1)) break;
    const float ds = vol.sample(p[0] + s * m.light[0], p[1] + s * m.light[1],
                                p[2] + s * m.light[2]);
    if (ds < m.cutoff) continue;
    tau += ds * m.shadow_step / (1.0f + s * m.light_gain);
  }
  return tau;
}

// tau_hat of a lit sample: over the eight corners v[x][y][z], x outermost, z innermost, the low
// corner first, ww = (wx_a * wy_b) * wz_c; a corner takes part if its density is > 0 (absent
// and outside corners arrive here as 0), and tau_hat = sum ww tau / sum ww, 0 with no corner.
__device__ __forceinline__ float vol_lit_corners(const float v[8], const float tau[8], float wx,
                                                 float wy, float wz) {
  const float ax[2] = {1.0f - wx, wx}, ay[2] = {1.0f - wy, wy}, az[2] = {1.0f - wz, wz};
  float num = 0.0f, den = 0.0f;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const float ww = (ax[c >> 2] * ay[(c >> 1) & 1]) * az[c & 1];
    if (v[c] > 0.0f) {
      num += ww * tau[c];
      den += ww;
    }
  }
  return den > 0.0f ? num / den : 0.0f;
}

// One pixel of one frame (block -> (frame, tile); thread -> pixel of the tile, 8 x 8 per
// wavefront). `vol` is the thread's own copy of the accessor. kLit: the shadow transmittance
// comes from the light volume (exp(ext * tau_hat)) instead of a shadow walk; everything else,
// the alpha channel included, is the marched mode's.
template <bool kLit = false, typename Vol>
__device__ __forceinline__ void vol_march_pixel(Vol& vol, const anr_camera* __restrict__ cams,
                                                int32_t H, int32_t W, int32_t tiles_x,
                                                int32_t tiles_y, const VolMarch& m,
                                                float* __restrict__ rgba) {
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
  if (!vol_clip(vol.nx, vol.ny, vol.nz, cam.eye, dir, &t0, &t1)) {
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
    float tau_hat = 0.0f;
    float d;
    if constexpr (kLit)
      d = vol.lit_sample(p[0], p[1], p[2], m.cutoff, &tau_hat);
    else
      d = vol.sample(p[0], p[1], p[2]);
    if (d < m.cutoff) continue;
    float sT[3] = {1.0f, 1.0f, 1.0f};
    if constexpr (kLit) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) sT[ch] = expf(m.ext[ch] * tau_hat);
    } else {
      // shadow ray towards the light
      float s0, s1;
      if (vol_clip(vol.nx, vol.ny, vol.nz, p, m.light, &s0, &s1)) {
        for (int32_t q = 1; q <= m.max_shadow; ++q) {
          const float s = static_cast<float>(q) * m.shadow_step;
          if (!(s <= s1)) break;
          const float ds = vol.sample(p[0] + s * m.light[0], p[1] + s * m.light[1],
                                      p[2] + s * m.light[2]);
          if (ds < m.cutoff) continue;
          const float gain = 1.0f + s * m.light_gain;
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) sT[ch] *= expf(m.ext[ch] * ds * m.shadow_step / gain);
          if (sT[0] * sT[0] + sT[1] * sT[1] + sT[2] * sT[2] < m.cutoff) break;
        }
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

// The refusals and the launch plan that do not depend on the kind of volume: image and
// parameter checks, VolMarch, and the tile counts. `who` names the entry in the messages.
// Returns ANR_OK with *empty = true when F * H * W = 0 (nothing to launch).
inline int vol_plan(const char* who, int64_t nx, int64_t ny, int64_t nz, int64_t F, int64_t H,
                    int64_t W, const anr_volume_params* params, VolMarch* m, int64_t* tiles_x,
                    int64_t* tiles_y, bool* empty) {
  *empty = true;
  ANR_CHECK_ARG(params != nullptr, "%s: null pointer (params)", who);
  ANR_CHECK_ARG(F >= 0 && H >= 0 && W >= 0, "%s: negative image size", who);
  const anr_volume_params& p = *params;
  ANR_CHECK_ARG(p.primary_step > 0.0f && p.shadow_step > 0.0f && std::isfinite(p.primary_step) &&
                    std::isfinite(p.shadow_step),
                "%s: steps must be positive and finite", who);
  ANR_CHECK_ARG(p.light_gain >= 0.0f && p.cutoff >= 0.0f && std::isfinite(p.light_gain) &&
                    std::isfinite(p.cutoff),
                "%s: negative coefficient (light_gain, cutoff)", who);
  double l2 = 0.0;
  for (int a = 0; a < 3; ++a) {
    ANR_CHECK_ARG(p.absorb[a] >= 0.0f && p.scatter[a] >= 0.0f && p.light_color[a] >= 0.0f &&
                      std::isfinite(p.absorb[a]) && std::isfinite(p.scatter[a]) &&
                      std::isfinite(p.light_color[a]),
                  "%s: negative coefficient (absorb, scatter, light_color)", who);
    l2 += static_cast<double>(p.light_dir[a]) * p.light_dir[a];
  }
  ANR_CHECK_ARG(fabs(sqrt(l2) - 1.0) <= 1e-3, "%s: light_dir must be unit length", who);
  if (F == 0 || H == 0 || W == 0) return ANR_OK;
  ANR_CHECK_ARG(H < (1LL << 24) && W < (1LL << 24), "%s: image side of 2^24 or more", who);
  *tiles_x = ceil_div(W, kVolTile);
  *tiles_y = ceil_div(H, kVolTile);
  ANR_CHECK_ARG(*tiles_x * *tiles_y < (1LL << 31) && F < (1LL << 31) &&
                    *tiles_x * *tiles_y * F < (1LL << 31),
                "%s: too many pixels for one launch (2^31 tiles or more)", who);
  for (int a = 0; a < 3; ++a) {
    // f32 as the definition has them: ext = -(absorb + scatter), albedo = light_color *
    // scatter / (absorb + scatter), 0 where the denominator is 0
    const float sum = p.absorb[a] + p.scatter[a];
    m->ext[a] = -sum;
    m->albedo[a] = sum == 0.0f ? 0.0f : p.light_color[a] * p.scatter[a] / sum;
    m->light[a] = p.light_dir[a];
  }
  m->primary_step = p.primary_step;
  m->shadow_step = p.shadow_step;
  m->light_gain = p.light_gain;
  m->cutoff = p.cutoff;
  // no ray inside the box [-1, n] takes more steps than the box diagonal over the step
  const double diag = sqrt(static_cast<double>(nx + 1) * (nx + 1) +
                           static_cast<double>(ny + 1) * (ny + 1) +
                           static_cast<double>(nz + 1) * (nz + 1));
  const double np_ = diag / p.primary_step + 2.0, ns_ = diag / p.shadow_step + 2.0;
  ANR_CHECK_ARG(np_ < 2147483000.0 && ns_ < 2147483000.0,
                "%s: steps too small for the cube (2^31 steps or more per ray)", who);
  m->max_primary = static_cast<int32_t>(np_) + 1;
  m->max_shadow = static_cast<int32_t>(ns_) + 1;
  *empty = false;
  return ANR_OK;
}

}  // namespace anr
