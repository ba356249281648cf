/*
 * anr.h — C ABI of libanr_hip.so, the MI355X (gfx950) kernels behind the AtmoNR
 * volumetric-renderer hot path.
 *
 * The reference (nasa/atmospheric-neural-rendering) has no C ABI: its hot path is
 * Python glue (samplers.py, datasets/harp2.py, graphics_utils.py, losses.py) around
 * tiny-cuda-nn's CUDA modules (tinycudann.Encoding / tinycudann.Network, bound through
 * pybind11 at pipelines/instant_ngp.py:4,60-85,163-174,236-237). Each entry point below
 * replaces one of those call sites; the reference line it stands in for is cited on it.
 * The Python host (atmonr_amd/_lib.py) binds these through ctypes; INTEGRATION.md shows
 * the binding.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer owned by the caller (torch's caching allocator);
 *     the library allocates no device memory of its own;
 *   - work is enqueued on `stream` (a hipStream_t, e.g. torch.cuda.current_stream()
 *     .cuda_stream); nothing synchronises the host;
 *   - return 0 on success, a negative ANR_E* code on error; anr_last_error() returns a
 *     thread-local message for the last failure. Errors never throw across the ABI;
 *   - sizes are int64; row strides are in ELEMENTS of the tensor's dtype;
 *   - dtype codes: ANR_F32 = 0, ANR_F16 = 1, ANR_BF16 = 2 (bf16: field MFMA operands only).
 */
#ifndef ANR_H_
#define ANR_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Version history, newest first.
 * ABI 5 (r06, the current version): the row-bit hash-grid backward and the f16-row field
 *   backward with its pos / list-pass workspace -- anr_hashgrid_bwd_rows,
 *   anr_ingp_field_bwd_ref16_rows and anr_ingp_field_bwd_ref16_rows_workspace_bytes.
 *   Added to ABI 5 since, without a version change (additive; every ABI 5 call behaves as it
 *   did), oldest first:
 *   - the include_height input -- 4-D hash grids (anr_hashgrid_init_nd; forward, backward and
 *     planes take its descriptors), anr_prep_params.mode 2 in anr_sample_uniform_bins
 *     ((B,N,4) coords), anr_append_heights and anr_append_heights_f64;
 *   - anr_ingp_field_fwd_h and anr_ingp_field_bwd_ref16_rows_h (the reference numerics' f16
 *     interchange between the field and the f16 composite); anr_composite_ref16_fwd_park and
 *     anr_composite_ref16_bwd_parked (the forward parks T, exp and the surface product for
 *     its backward, which then skips its replay of the forward);
 *   - multi-band extinction in the fused field -- dir descriptors of 16..18 inputs (S = 20 -
 *     n_input = 2..4 density outputs), refused before, are accepted by
 *     anr_ingp_field_supported / _packed_size / _pack / _fwd / _density / _bwd /
 *     _bwd_workspace_bytes, with sigma and d_sigma (M, S); no signature changes (see
 *     "K6 + K7 fused" below);
 *   - anr_grad_quantize_add_f16 (the per-call f16 rounding of a tcnn module's parameter
 *     gradient, added to the caller's);
 *   - anr_ingp_render -- the forward-only render (hash grid, field and composite in one
 *     kernel, no per-sample output), in reference and build numerics;
 *   - anr_voxel_traverse, anr_voxel_n_blocks, anr_voxel_count and anr_voxel_compact (the
 *     global-grid extract's exact voxel traversal into a bitmap and its ordered compaction);
 *   - anr_volume_render (the orbit video's single-scattering ray marcher over a dense
 *     density cube, with anr_camera and anr_volume_params);
 *   - anr_sparse_volume_coarse_words, anr_sparse_volume_mark, anr_sparse_volume_popcount,
 *     anr_sparse_volume_place, anr_sparse_volume_sample and anr_sparse_volume_render (the
 *     global-grid extract's sparse volume -- bitmap, rank and ordered values -- and the same
 *     march over it, with anr_sparse_volume);
 *   - anr_volume_light, anr_volume_render_lit, anr_sparse_volume_light and
 *     anr_sparse_volume_render_lit (the light volume: the shadow optical depth of every voxel,
 *     summed once per video, and the march that interpolates it -- a second, opt-in shadow
 *     mode beside the marched one, which is unchanged).
 * ABI 4 (r06): anr_ingp_hash_field_fwd.
 * ABI 3 (r05): anr_hashgrid_fwd_planes, and the fused field entry points' enc_stride < 0
 *   selecting the level-quad-plane layout it writes. */
#define ANR_ABI_VERSION 5

enum anr_dtype { ANR_F32 = 0, ANR_F16 = 1, ANR_BF16 = 2 };

enum anr_status {
  ANR_OK = 0,
  ANR_E_INVALID = -1,     /* bad argument (shape, dtype, unsupported config) */
  ANR_E_LAUNCH = -2,      /* hipLaunchKernel / hipGetLastError reported an error */
  ANR_E_UNSUPPORTED = -3  /* configuration outside the compiled kernel set */
};

typedef void* anr_stream_t; /* hipStream_t */

int anr_abi_version(void);
const char* anr_last_error(void);

/* ------------------------------------------------------------------------------------
 * K1 + K2: stratified ray sampler fused with the HARP2 "horizontal" point preprocessor.
 * ------------------------------------------------------------------------------------
 * anr_prep_params mirrors the closure built by HARP2Dataset.get_point_preprocessor
 * ("horizontal"), datasets/harp2.py:357-388, plus the Instant-NGP remap of
 * pipelines/instant_ngp.py:149,160.
 */
typedef struct {
  int32_t mode;            /* 0: no preprocessing (raw normalized xyz); 1: horizontal;
                            * 2: raw xyz with the normalised ellipsoidal height appended
                            * (include_height, samplers.py:168-195): 4-wide rows, see below */
  int32_t shift_lon;       /* dateline shift, harp2.py:366-370,379-380 */
  int32_t ngp_remap;       /* 1: out = (p+1)/2, out.z /= alt_compress (instant_ngp.py:149,160) */
  int32_t _pad;
  double scale;            /* dataset.scale  (Python float), harp2.py:376 */
  double offset[3];        /* dataset.offset (float64 tensor), harp2.py:376 */
  double lat_min, lat_range, lon_min, lon_range; /* f32 0-dim tensors, harp2.py:361-370 */
  double ray_origin_height;                      /* harp2.py:383 */
  float alt_compress;                            /* config alt_compress_factor */
  float _pad2;
} anr_prep_params;

/* sample_uniform_bins (samplers.py:8-47) [+ preprocess (harp2.py:372-386)].
 *   origin, dir: (B,3) f32; len: (B,) f32; u: (B,N) f32 uniform draws or NULL for bin
 *   midpoints (random=False, samplers.py:37-41); bins: (N+1,) f32 = torch.linspace(0,1,N+1).
 *   Outputs (each nullable): pts (B,N,3) f32 raw sample points (samplers.py:45);
 *   z (B,N) f32 (samplers.py:42); coords (B,N,3) f32 preprocessed (+remapped) points.
 *   z and pts are bit-identical to the reference for identical u (no FMA contraction).
 *   prep->mode 2 (include_height): coords is (B,N,4) f32, 16-byte aligned, rows
 *   [x, y, z, h] as anr_append_heights writes them, computed where the sample sits in
 *   registers. */
int anr_sample_uniform_bins(const float* origin, const float* dir, const float* len,
                            const float* u, const float* bins, int64_t B, int32_t N,
                            float* pts, float* z, const anr_prep_params* prep,
                            float* coords, anr_stream_t stream);

/* preprocess_coords applied to arbitrary points (extract path, instant_ngp.py:220-233).
 *   pts (P,3) f32 -> coords (P,3) f32. */
int anr_preprocess_points(const float* pts, int64_t P, const anr_prep_params* prep,
                          float* coords, anr_stream_t stream);

/* Same for f64 points (scripts/extract.py:203-209 passes (xyz - offset) / scale in f64;
 * the whole preprocessor, clip and NGP remap run in f64, the result is rounded to f32
 * once, where tcnn casts the encoder input). */
int anr_preprocess_points_f64(const double* pts, int64_t P, const anr_prep_params* prep,
                              float* coords, anr_stream_t stream);

/* The Instant-NGP include_height input (instant_ngp.py:149-160,224-233): pts (P,3)
 * -> out (P,4) f32 rows [x, y, z, h], out 16-byte aligned. prep->mode must be 2; scale,
 * offset, ray_origin_height, ngp_remap and alt_compress are read. With ngp_remap the points
 * are first remapped, p = (p + 1) / 2. h = f32(alt / ray_origin_height), alt the Bowring
 * ellipsoidal height (wgs_84.py:83-97) of p * scale + offset formed in f64 from the REMAPPED
 * points, as the reference's append_heights does (samplers.py:188); h is not confined to
 * [0, 1]. With ngp_remap column 2 (alone) is then divided by alt_compress. Without
 * ngp_remap this is samplers.append_heights on the points as given. _f64: remap and
 * compression in f64, every column rounded to f32 once (the extract path). No backward:
 * nothing in the Instant-NGP pipeline differentiates with respect to sample positions. */
int anr_append_heights(const float* pts, int64_t P, const anr_prep_params* prep, float* out,
                       anr_stream_t stream);
int anr_append_heights_f64(const double* pts, int64_t P, const anr_prep_params* prep,
                           float* out, anr_stream_t stream);

/* Backward of the preprocessor (the NeRF pipeline back-propagates into the sample points,
 * harp2.py:372-386): d_pts (P,3) f32 WRITTEN = J^T d_coords, J from fp64 forward-mode
 * derivatives of the same formula; clip passes the gradient where -1 <= value <= 1. */
int anr_preprocess_points_bwd(const float* pts, int64_t P, const anr_prep_params* prep,
                              const float* d_coords, float* d_pts, anr_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Ray-batch glue in front of K1 (csrc/gather.hip).
 * ------------------------------------------------------------------------------------
 * anr_gather_rows: dst_k[r] = src_k[idx[r]] for every column k in one launch (the
 * per-field indexing of HARP2Dataset.__getitem__ / __getbatch__, harp2.py:392-420).
 * idx (B,) int64; a column is a row-major array of row_bytes-byte rows (multiple of 4,
 * <= 4096); at most ANR_GATHER_MAX_COLS columns. */
#define ANR_GATHER_MAX_COLS 8
typedef struct {
  const void* src;
  void* dst;
  int64_t row_bytes;
} anr_gather_col;
int anr_gather_rows(const int64_t* idx, int64_t B, int32_t n_cols, const anr_gather_col* cols,
                    anr_stream_t stream);
/* Instant-NGP surface-network input (instant_ngp.py:143,150,173): out (B,5) f32 =
 * [((o + d*len) + 1) / 2 for x, y | d], with torch's f32 rounding of each op.
 * origin, dir (B,3) f32, len (B,) f32. */
int anr_ingp_surface_input(const float* origin, const float* dir, const float* len,
                           int64_t B, float* out, anr_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K3 / K4: multi-resolution hash-grid encoding (tinycudann.Encoding otype "HashGrid",
 * instant_ngp.py:60-63,163; surface 2-D grid :78-80,173).
 * ------------------------------------------------------------------------------------ */
#define ANR_MAX_LEVELS 32
typedef struct {
  int32_t n_dims;           /* 2 or 3; 4 through anr_hashgrid_init_nd */
  int32_t n_levels;         /* <= ANR_MAX_LEVELS */
  int32_t n_features;       /* features per level: 1, 2, 4 or 8 */
  int32_t base_resolution;
  float per_level_scale;
  int32_t log2_hashmap_size;
  int64_t n_params;         /* total table entries * n_features (filled by _init) */
  uint32_t offsets[ANR_MAX_LEVELS + 1]; /* first table entry of each level */
  uint32_t resolutions[ANR_MAX_LEVELS];
  float scales[ANR_MAX_LEVELS];
} anr_hashgrid_desc;

/* Fill offsets/resolutions/scales/n_params from the config (tcnn GridEncoding rules). */
int anr_hashgrid_init(anr_hashgrid_desc* d, int32_t n_dims, int32_t n_levels,
                      int32_t n_features, int32_t base_resolution, float per_level_scale,
                      int32_t log2_hashmap_size);

/* The same for 2 to 4 dimensions. anr_hashgrid_init keeps refusing n_dims = 4, as it always
 * has; the 4-D grid of include_height (instant_ngp.py:50) is asked for by name here. Every
 * entry point below takes either descriptor. */
int anr_hashgrid_init_nd(anr_hashgrid_desc* d, int32_t n_dims, int32_t n_levels,
                         int32_t n_features, int32_t base_resolution, float per_level_scale,
                         int32_t log2_hashmap_size);

/* Forward: x (M, n_dims) f32 in [0,1] with row stride x_stride; table (n_params) in
 * table_dtype; out (M, n_levels*n_features) written at row stride out_stride
 * (level-major: column l*F+f), out_dtype. Interpolation accumulates in f32. */
int anr_hashgrid_fwd(const anr_hashgrid_desc* d, const float* x, int64_t x_stride,
                     int64_t M, const void* table, int32_t table_dtype, void* out,
                     int32_t out_dtype, int64_t out_stride, anr_stream_t stream);
/* The same, for points that come in runs of run_length spatial neighbours (the altitudes
 * of one extract column, scripts/extract.py:180-211; a ray's samples): the walker's
 * chunks follow the runs (run_length <= 256; 0 = no hint, as anr_hashgrid_fwd). Outputs
 * do not depend on it. */
int anr_hashgrid_fwd_runs(const anr_hashgrid_desc* d, const float* x, int64_t x_stride,
                          int64_t M, int64_t run_length, const void* table,
                          int32_t table_dtype, void* out, int32_t out_dtype,
                          int64_t out_stride, anr_stream_t stream);

/* Kernel generation (test / A-B hook; process-wide; returns the previous mode, or
 * ANR_E_INVALID for an unknown mode): 0 = default (forward v6
 * branch-free walker -- v1 above 16 levels or past 32-bit buffer offsets -- backward v2
 * four-lanes-per-level), 1 = v1 both, 6 = forward v1 + backward v2 (the r01 default),
 * 7 = mode 0 with the backward's run-time-stride instantiation. */
int anr_hashgrid_force_v1(int32_t mode);
/* Samples per wavefront chunk the v2 backward uses for M points (host-side query: the
 * request counter of tools/hash_requests.py replays the kernel's chunking with it). */
int64_t anr_hashgrid_bwd_chunk(int64_t M);
/* Request-count instrument of the v2 backward: the same launch geometry and walk over
 * the same inputs as anr_hashgrid_bwd (dtable: the gradient buffer that launch would add
 * to -- its addresses decide the 64-B segments; NOT written), adding to *count (one u64,
 * device) the memory-side requests the real launch makes: per flush instruction, the
 * distinct 64-B segments of its active lanes (zero-sum corners skipped as there).
 * bench.py's hash-backward roofline counts its benched step this way. 3-D, 2 features,
 * <= 16 levels; ANR_E_UNSUPPORTED otherwise (2-D and 4-D grids included: their backward is
 * not the v2 walker this models). */
int anr_hashgrid_bwd_count_requests(const anr_hashgrid_desc* d, const float* x,
                                    int64_t x_stride, int64_t M, const void* dout,
                                    int32_t dout_dtype, int64_t dout_stride,
                                    const float* dtable, unsigned long long* count,
                                    anr_stream_t stream);

/* Backward: dout (M, L*F) (dout_dtype, row stride dout_stride) -> dtable (n_params)
 * f32, ACCUMULATED (caller zeroes). Duplicate corner updates inside a wavefront are
 * pre-summed before the f32 atomics (samples along one ray share cells). */
/* anr_hashgrid_bwd with the field backward's per-tile flags (r05): tile_nz[t] = 0 marks
 * rows [32 t, 32 t + 32) whose dL/dy is zero in every row (anr_ingp_field_bwd_ref16_tiles
 * writes them); the v2 walker neither loads nor walks those rows (their contributions
 * are zero). Same result as anr_hashgrid_bwd for such inputs; shapes outside the tiled
 * walker (not 3-D / 2 features / <= 16 levels, strides other than (3, 32), chunks not a
 * multiple of 32 rows) run anr_hashgrid_bwd and ignore the flags. */
int anr_hashgrid_bwd_tiles(const anr_hashgrid_desc* d, const float* x, int64_t x_stride,
                           int64_t M, const void* dout, int32_t dout_dtype, int64_t dout_stride,
                           float* dtable, const uint8_t* tile_nz, anr_stream_t stream);

/* anr_hashgrid_bwd with per-row bits (ABI 5): bit (m % 32) of row_nz[m / 32] set marks a
 * row m of dout with a nonzero value (anr_ingp_field_bwd_ref16_rows writes them); the v2
 * walker loads and walks only those rows. A row whose bit is clear is taken as zero and
 * need not have been written (anr_ingp_field_bwd_ref16_rows does not write it). Same
 * result as anr_hashgrid_bwd on dout with the clear rows zeroed; shapes other than 3-D /
 * 2 features / 16 levels / strides (3, 32) zero the clear rows IN PLACE (dout is written)
 * and run anr_hashgrid_bwd. Replaces the same call site as anr_hashgrid_bwd (tcnn HashGrid
 * backward, instant_ngp.py:163). */
int anr_hashgrid_bwd_rows(const anr_hashgrid_desc* d, const float* x, int64_t x_stride,
                          int64_t M, void* dout, int32_t dout_dtype, int64_t dout_stride,
                          float* dtable, const uint32_t* row_nz, anr_stream_t stream);

/* Level-quad-plane forward (r05; hashgrid.hip forward v9, one lane per sample): the same
 * features as anr_hashgrid_fwd with f16 output, laid out as planes of four levels: level
 * l, feature f of row m at out[(l / 4) * plane_stride + 8 m + 2 (l % 4) + f]
 * (plane_stride >= 8 M f16 elements, multiple of 8; out 16-byte aligned; a partial last
 * quad is zero-filled). 2 features, <= 16 levels, 2-D to 4-D. The fused field kernels read this
 * layout when given enc_stride = -plane_stride. Replaces the same call site as
 * anr_hashgrid_fwd (instant_ngp.py:163, the tcnn Encoding forward). */
int anr_hashgrid_fwd_planes(const anr_hashgrid_desc* d, const float* x, int64_t x_stride,
                            int64_t M, const void* table, int32_t table_dtype, void* out,
                            int64_t plane_stride, anr_stream_t stream);

int anr_hashgrid_bwd(const anr_hashgrid_desc* d, const float* x, int64_t x_stride,
                     int64_t M, const void* dout, int32_t dout_dtype, int64_t dout_stride,
                     float* dtable, anr_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K5: SphericalHarmonics / Identity encodings (tinycudann Composite members,
 * instant_ngp.py:69-72,165-169; surface :78-80).
 * ------------------------------------------------------------------------------------ */
/* SH of degree `degree` (1..4 -> degree^2 outputs) of x in [0,1]^3 remapped to 2x-1. */
int anr_sh_fwd(int32_t degree, const float* x, int64_t x_stride, int64_t M, void* out,
               int32_t out_dtype, int64_t out_stride, anr_stream_t stream);
/* d(SH)/dx: dout (M, degree^2) -> dx (M,3) f32, ACCUMULATED into dx. */
int anr_sh_bwd(int32_t degree, const float* x, int64_t x_stride, int64_t M,
               const void* dout, int32_t dout_dtype, int64_t dout_stride, float* dx,
               int64_t dx_stride, anr_stream_t stream);
/* Identity: out[:, :n] = x[:, :n] (dtype conversion). x may be f32 or f16. */
int anr_identity(const void* x, int32_t x_dtype, int64_t x_stride, int64_t M, int32_t n,
                 void* out, int32_t out_dtype, int64_t out_stride, anr_stream_t stream);
/* Fill out[:, :n] with a constant (tcnn pads encodings with 1.0). */
int anr_fill_cols(void* out, int32_t out_dtype, int64_t out_stride, int64_t M, int32_t n,
                  float value, anr_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K6 / K7: fully-fused MLP (tinycudann.Network otype "FullyFusedMLP",
 * instant_ngp.py:64-68,73-77,81-85). Bias-free; ReLU hidden activation; output
 * activation None or ReLU. Weight layout: layer k is a row-major (out_k, in_k) matrix,
 * layers concatenated; in_0 = n_input_padded, out_last = n_output_padded.
 * Input columns [n_input, n_input_padded) are read as 1.0 (tcnn encoding padding).
 * ------------------------------------------------------------------------------------ */
enum anr_activation { ANR_ACT_NONE = 0, ANR_ACT_RELU = 1 };
typedef struct {
  int32_t n_input, n_input_padded;   /* padded to a multiple of 16 */
  int32_t n_output, n_output_padded; /* padded to a multiple of 16 */
  int32_t width;                     /* 16, 32, 64 or 128 */
  int32_t n_hidden_layers;           /* >= 1 */
  int32_t activation;                /* ANR_ACT_RELU */
  int32_t output_activation;         /* ANR_ACT_NONE or ANR_ACT_RELU */
} anr_mlp_desc;

int64_t anr_mlp_n_params(const anr_mlp_desc* d);
/* Force the generic (shape-agnostic) MLP kernels instead of the compile-time specialised
 * ones (on != 0). Test hook; process-wide. Returns the previous setting. */
int anr_mlp_force_generic(int32_t on);
/* Forward. precision = ANR_F16 (f16 MFMA, f32 accumulate; params_f16 used) or ANR_F32
 * (f32 MFMA, exact f32; params_f32 used). in: (M, n_input) in_dtype; out: (M, n_output)
 * out_dtype. */
int anr_mlp_fwd(const anr_mlp_desc* d, int32_t precision, const void* params,
                const void* in, int32_t in_dtype, int64_t in_stride, int64_t M, void* out,
                int32_t out_dtype, int64_t out_stride, anr_stream_t stream);
/* Backward (recomputes the forward activations on chip). dout: (M, n_output);
 * din (nullable): (M, n_input) written (not accumulated); dparams: f32, ACCUMULATED. */
int anr_mlp_bwd(const anr_mlp_desc* d, int32_t precision, const void* params,
                const void* in, int32_t in_dtype, int64_t in_stride, int64_t M,
                const void* dout, int32_t dout_dtype, int64_t dout_stride, void* din,
                int32_t din_dtype, int64_t din_stride, float* dparams,
                anr_stream_t stream);
/* Scratch bytes anr_mlp_bwd_ws can use for M rows (0: it would not use any). With it the
 * specialised backward stores one dW row per wavefront and sums them in a fixed order
 * instead of adding with float atomics (small batches, e.g. the per-ray surface
 * network: deterministic and without the atomics' contention). */
int64_t anr_mlp_bwd_workspace_bytes(const anr_mlp_desc* d, int64_t M);
/* anr_mlp_bwd with a device workspace (f32-aligned, workspace_bytes long; may be null or
 * smaller than anr_mlp_bwd_workspace_bytes, then the atomics path runs). */
int anr_mlp_bwd_ws(const anr_mlp_desc* d, int32_t precision, const void* params,
                   const void* in, int32_t in_dtype, int64_t in_stride, int64_t M,
                   const void* dout, int32_t dout_dtype, int64_t dout_stride, void* din,
                   int32_t din_dtype, int64_t din_stride, float* dparams, void* workspace,
                   int64_t workspace_bytes, anr_stream_t stream);

/* Instant-NGP dir MLP with the dir encoding fused into its input
 * (instant_ngp.py:165-171): row r of the network input is
 * [SH degree 2 of dirs[r / n_per_ray] | pos_out[r, 1:16] | 1.0 padding] (n_input = 19,
 * padded 32), so the encoded tensor is never materialised.
 *   pos_out (M, >=16) f32 (pos_mlp output, row stride pos_stride); dirs (M/n_per_ray, 3)
 *   f32; color (M, n_output) out_dtype. Widths 32/64, 1-2 hidden layers. */
int anr_ingp_dir_mlp_fwd(const anr_mlp_desc* d, int32_t precision, const void* params,
                         const float* pos_out, int64_t pos_stride, const float* dirs,
                         int64_t n_per_ray, int64_t M, void* color, int32_t out_dtype,
                         int64_t out_stride, anr_stream_t stream);
/* Backward: d_color (M, n_output) f32, d_sigma (M,) f32 (nullable) -> d_pos_out (M, 16)
 * f32 WRITTEN: column 0 = d_sigma * [pos_out[:,0] > 0] (density ReLU, instant_ngp.py:184),
 * columns 1..15 = dL/d(pos_out[:, 1:16]); dparams f32 ACCUMULATED. */
int anr_ingp_dir_mlp_bwd(const anr_mlp_desc* d, int32_t precision, const void* params,
                         const float* pos_out, int64_t pos_stride, const float* dirs,
                         int64_t n_per_ray, int64_t M, const float* d_color,
                         int64_t d_color_stride, const float* d_sigma, float* d_pos_out,
                         int64_t d_pos_stride, float* dparams, anr_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K6 + K7 fused: the Instant-NGP radiance field after the hash encoding, one kernel each
 * way (replaces pos_mlp -> dir_encoder -> dir_mlp -> relu at instant_ngp.py:163-184).
 * ------------------------------------------------------------------------------------
 * Supported pairs: pos 32 -> W -> 16 (1 hidden layer, no output activation), dir (20 - S)
 * -> W (1 or 2 hidden layers) -> n_output <= 16, W in {32, 64}, S in {1, 2, 3, 4}.
 * S is the number of density outputs and is read from the dir descriptor, S = 20 -
 * dir.n_input: the dir network's inputs are SH2(dir) (4) and pos_out[:, S:16]
 * (instant_ngp.py:64-77). S = 1 is the reference's default; S = num_bands with
 * multi_band_extinction (instant_ngp.py:46-48,178,184). dir.n_input_padded must be tcnn's
 * (n_input + 15) / 16 * 16: 32 for S <= 3, 16 for S = 4, so the first dir layer's parameter
 * rows are 32 or 16 wide and anr_mlp_n_params(dir) differs accordingly; the packed size
 * does not depend on S.
 * With S > 1, sigma and d_sigma are (M, S) row-major f32, contiguous (row m at element
 * m * S), sigma[m][j] = relu(pos_out[m][j]); the pointers must be aligned to 4 S bytes
 * (4 bytes for S = 3). anr_ingp_field_fwd, anr_ingp_field_density, anr_ingp_field_bwd and
 * its workspace query take S > 1; anr_ingp_field_fwd_h, anr_ingp_field_fwd_rows / _bwd_rows,
 * anr_ingp_hash_field_fwd and every anr_ingp_field_bwd_ref16* entry stay at S = 1 and
 * return ANR_E_UNSUPPORTED for S > 1 (M = 0 still returns ANR_OK).
 * mma_dtype: ANR_F16 (the reference's tcnn precision: f16 operands, f32 accumulation) or
 * ANR_BF16 (BASELINE configs[4], beyond the reference: bf16 operands over the same f16
 * hash features, f32 accumulation; no gradient scaling). Pack, forward and backward of one
 * network must use the same mma_dtype.
 * Weights: anr_ingp_field_pack converts the f32 master parameters of both networks
 * (tcnn layout) into one 16-bit buffer of anr_ingp_field_packed_size elements (MFMA
 * fragment order); run it after every optimizer step.
 * enc (every entry point below): f16 hash features, enc_stride >= 32 (multiple of 8) for
 *   the row layout (M, enc_stride) with 16-byte aligned rows, or enc_stride = -P for the
 *   level-quad planes of anr_hashgrid_fwd_planes (P >= 8 M, multiple of 8).
 * Forward: enc, dirs (M/n_per_ray, 3) f32 ->
 *   sigma (M,) f32 = relu(pos_out[:,0]) ((M, S) = relu(pos_out[:, :S]) for S > 1),
 *   color (M, n_output) f32 = relu(dir_mlp(...)).
 * Backward: d_sigma (M,) f32 ((M, S) for S > 1; nullable), d_color (M, n_output) f32 -> d_enc (M, 32) f32
 *   WRITTEN; g_pos / g_dir f32 parameter gradients ACCUMULATED. `workspace` is caller-
 *   owned device memory of at least anr_ingp_field_bwd_workspace_bytes(pos, dir,
 *   mma_dtype, M) bytes (per-wavefront f16 gradient maxima; 0 bytes for bf16, then it may
 *   be NULL); it must not be shared with a concurrent backward launch. */
int anr_ingp_field_supported(const anr_mlp_desc* pos, const anr_mlp_desc* dir);
int64_t anr_ingp_field_packed_size(const anr_mlp_desc* pos, const anr_mlp_desc* dir);
/* f16 gradient scale target of the backward (max |dL/dout| per wavefront -> 2^v);
 * returns the previous value. Test hook; process-wide. */
int anr_ingp_field_set_grad_scale(int32_t log2_target);
/* Forward kernel form: 1 = the uniform-tile form wherever the shapes allow it (default:
 * dense rows, samples_per_ray a multiple of 16, 4 colour outputs, 16-byte aligned colour
 * rows; one scalar direction load per 16-row tile, branch-free output stores), 0 = always
 * the general form. Same math and bit-identical results. Test / A-B hook; process-wide;
 * other values keep the current mode. Returns the previous mode. */
int anr_ingp_field_force_fwd(int32_t mode);
int64_t anr_ingp_field_bwd_workspace_bytes(const anr_mlp_desc* pos, const anr_mlp_desc* dir,
                                           int32_t mma_dtype, int64_t M);
int anr_ingp_field_pack(const anr_mlp_desc* pos, const anr_mlp_desc* dir, int32_t mma_dtype,
                        const float* pos_params, const float* dir_params, void* packed,
                        anr_stream_t stream);
int anr_ingp_field_fwd(const anr_mlp_desc* pos, const anr_mlp_desc* dir, int32_t mma_dtype,
                       const void* packed, const void* enc, int64_t enc_stride,
                       const float* dirs, int64_t n_per_ray, int64_t M, float* sigma,
                       float* color, int64_t color_stride, anr_stream_t stream);
/* anr_ingp_field_fwd with f16 outputs: sigma (M) and color (M, color_stride) halves, each
 * the f32 value anr_ingp_field_fwd stores rounded to nearest even (above 65,504: inf) --
 * tcnn's f16 module outputs, as the reference-numerics composite reads them. color 8-byte
 * aligned when color_stride is a multiple of 4. Same kernel forms and grids. */
int anr_ingp_field_fwd_h(const anr_mlp_desc* pos, const anr_mlp_desc* dir, int32_t mma_dtype,
                         const void* packed, const void* enc, int64_t enc_stride,
                         const float* dirs, int64_t n_per_ray, int64_t M, void* sigma,
                         void* color, int64_t color_stride, anr_stream_t stream);
/* Hash-grid forward + field forward in one kernel (ABI 4, r06): the level-quad planes of
 * anr_hashgrid_fwd_planes (written for the backward: planes, plane_stride >= 8 M f16
 * elements) and sigma / color of anr_ingp_field_fwd, bit-identical to those two calls, with
 * the planes never re-read. Replaces the same call sites (instant_ngp.py:163-171: the tcnn
 * Encoding forward, pos_mlp, dir_encoder, dir_mlp). Shapes: 3-D f16 hash grid of 16 levels
 * x 2 features (x: (M, 3) f32 rows), a supported field pair with 4 colour outputs, samples
 * per ray a multiple of 64, 16-byte aligned planes / packed / colour rows;
 * ANR_E_UNSUPPORTED otherwise (the two calls then serve). */
int anr_ingp_hash_field_fwd(const anr_hashgrid_desc* grid, const float* x, int64_t M,
                            const void* table, int32_t table_dtype, void* planes,
                            int64_t plane_stride, const anr_mlp_desc* pos,
                            const anr_mlp_desc* dir, int32_t mma_dtype, const void* packed,
                            const float* dirs, int64_t n_per_ray, float* sigma, float* color,
                            int64_t color_stride, anr_stream_t stream);
/* Forward-only render: hash grid, field and composite in one kernel, nothing written per
 * sample. Replaces, for a render without a backward, instant_ngp.py:163-192 (the tcnn
 * Encoding forward, pos_mlp, dir_encoder, dir_mlp and the render_with_surface call) and
 * graphics_utils.py:6-77 (render / render_with_surface). One wavefront per ray walks the
 * ray's 64-sample segments in order; sigma and colour are anr_ingp_field_fwd's values
 * (anr_ingp_field_fwd_h's in reference numerics) and never leave the chip.
 *   coords (B * n_per_ray, 3) f32 and z (B, n_per_ray) f32 as anr_sample_uniform_bins writes
 *   them, dirs (B, 3) f32, table: the grid's f16 table, packed: anr_ingp_field_pack's buffer.
 *   numerics ANR_RENDER_REFERENCE: the arithmetic of anr_composite_ref16_fwd on the f16
 *   sigma / colour; color_surf (B, 4) and the outputs are f16; the maps are bit-identical to
 *   anr_ingp_field_fwd_h followed by anr_composite_ref16_fwd.
 *   numerics ANR_RENDER_BUILD: anr_composite_fwd's f32 expressions on the f32 sigma / colour;
 *   color_surf and the outputs are f32; the f32 sums run in another order than
 *   anr_composite_fwd's, so the maps agree with it to rounding, not to bits.
 *   color_map, atmo, surf: (B, 4) contiguous; color_surf, atmo and surf may be null (surf is
 *   written only with a color_surf; without one color_map is the atmospheric map).
 * Shapes: 3-D f16 hash grid of 16 levels x 2 features, a supported field pair with one
 * density and 4 colour outputs (W in {32, 64}, one or two hidden dir layers), mma_dtype
 * ANR_F16 or ANR_BF16, n_per_ray a positive multiple of 64, 16-byte aligned packed weights,
 * byte ranges below 2^31; ANR_E_UNSUPPORTED otherwise. B = 0: ANR_OK without a launch.
 * Allocates nothing and does not synchronise; the grid is sized from the current device's
 * CU count and the occupancy query. */
#define ANR_RENDER_BUILD 0
#define ANR_RENDER_REFERENCE 1
int anr_ingp_render(const anr_hashgrid_desc* grid, const float* coords, const float* z,
                    const float* dirs, int64_t B, int64_t n_per_ray, const void* table,
                    int32_t table_dtype, const anr_mlp_desc* pos, const anr_mlp_desc* dir,
                    int32_t mma_dtype, const void* packed, const void* color_surf,
                    float z_scale, int32_t numerics, void* color_map, void* atmo, void* surf,
                    anr_stream_t stream);
/* Density only: sigma[r] = relu(pos_mlp(enc[r])[0]) (f32; (M, S) for S > 1), bit-identical to
 * anr_ingp_field_fwd's sigma, without the dir MLP -- the extract loop
 * (scripts/extract.py:203-209 -> instant_ngp.py:208-247 reads only the extinction) and the
 * occupancy grid. Same descriptors and packed weights as anr_ingp_field_fwd. */
int anr_ingp_field_density(const anr_mlp_desc* pos, const anr_mlp_desc* dir, int32_t mma_dtype,
                           const void* packed, const void* enc, int64_t enc_stride, int64_t M,
                           float* sigma, anr_stream_t stream);
int anr_ingp_field_bwd(const anr_mlp_desc* pos, const anr_mlp_desc* dir, int32_t mma_dtype,
                       const void* packed, const void* enc, int64_t enc_stride,
                       const float* dirs, int64_t n_per_ray, int64_t M, const float* d_sigma,
                       const float* d_color, int64_t d_color_stride, float* d_enc,
                       int64_t d_enc_stride, float* g_pos, float* g_dir, void* workspace,
                       int64_t workspace_bytes, anr_stream_t stream);

/* The same kernels over occupancy-compacted samples (anr_occupancy_compact): row r of
 * enc / d_enc is dense sample rows[r] (int32, ray-major index < n_rays * n_per_ray) of
 * sigma, color, d_sigma, d_color, whose ray is rows[r] / n_per_ray. The forward writes
 * only the listed dense rows (the caller zero-fills the rest: culled samples have
 * sigma = 0), the backward reads dL/d(sigma, color) at those rows. */
int anr_ingp_field_fwd_rows(const anr_mlp_desc* pos, const anr_mlp_desc* dir,
                            int32_t mma_dtype, const void* packed, const void* enc,
                            int64_t enc_stride, const float* dirs, int64_t n_per_ray,
                            int64_t M, const int32_t* rows, float* sigma, float* color,
                            int64_t color_stride, anr_stream_t stream);
int anr_ingp_field_bwd_rows(const anr_mlp_desc* pos, const anr_mlp_desc* dir,
                            int32_t mma_dtype, const void* packed, const void* enc,
                            int64_t enc_stride, const float* dirs, int64_t n_per_ray,
                            int64_t M, const int32_t* rows, const float* d_sigma,
                            const float* d_color, int64_t d_color_stride, float* d_enc,
                            int64_t d_enc_stride, float* g_pos, float* g_dir, void* workspace,
                            int64_t workspace_bytes, anr_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Occupancy-grid sample culling (beyond the reference: BASELINE configs[4], SURVEY §8
 * f3; csrc/occupancy.hip). occ: gx*gy*gz bytes (x fastest), nonzero = occupied, over the
 * hash-grid domain [0,1] x [0,1] x [0, 1/zmul]. coords (M,3) f32 ray-major.
 * anr_occupancy_count writes counts[anr_occupancy_n_blocks(M)] (int32, kept samples per
 * block of 1024); the caller forms offsets = exclusive scan (int64) and the total K;
 * anr_occupancy_compact writes rows (K,) int32 (kept sample indices, ascending) and
 * coords_out (K,3). ------------------------------------------------------------------ */
int64_t anr_occupancy_n_blocks(int64_t M);
int anr_occupancy_count(const float* coords, int64_t M, const uint8_t* occ, int32_t gx,
                        int32_t gy, int32_t gz, float zmul, int32_t* counts,
                        anr_stream_t stream);
int anr_occupancy_compact(const float* coords, int64_t M, const uint8_t* occ, int32_t gx,
                          int32_t gy, int32_t gz, float zmul, const int64_t* offsets,
                          int32_t* rows, float* coords_out, anr_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Global-grid extract: exact voxel traversal of rays into a bitmap, and the bitmap's ordered
 * compaction (csrc/voxels.hip; the reference's graphics_utils.voxel_traversal and the
 * torch.unique calls of datasets/harp2_extract.py:845-867).
 * Box: origin (i0, j0, k0), extents (ni, nj, nk) >= 1, origin + extent <= 2^31. Bitmap: one
 * bit per voxel, i along x and fastest, k slowest; an x-row takes row_pitch bits, a multiple
 * of 32 that is >= ni, so bit b of word w of row (j, k) is voxel (i0 + 32 w + b, j, k); the
 * whole bitmap is row_pitch * nj * nk bits (fewer than 2^46) of caller-zeroed uint32 words.
 * anr_voxel_traverse: u, end (R, 3) f64, ray start and end in continuous voxel coordinates
 * (voxel edge 1). ORs the voxels of every ray into the bitmap, so several calls accumulate.
 * One thread per ray walks exactly sum_a |floor(end_a) - floor(u_a)| steps from floor(u);
 * each step advances the axis (among those not at their end index, ties to the lowest) with
 * the smallest crossing time t_a = (b_a - u_a) * (1 / d_a), b_a the next integer boundary:
 * no accumulated time. counters: two int64, added to (the caller zeroes them): [0] rays
 * skipped because an endpoint is not finite; [1] voxels not marked because their ray has an
 * end voxel outside the box (such a ray marks nothing; every other ray stays inside the
 * box). shortcut 1: a plain load skips the atomic OR of a word whose pending bits are all
 * set already; 0: always the atomic (same result; for timing). R = 0: ANR_OK, no launch.
 * anr_voxel_count writes counts[anr_voxel_n_blocks(row_pitch * nj * nk / 32)] (int32, set
 * bits per block of 1024 words); the caller forms offsets = exclusive scan (int64) and the
 * total n; anr_voxel_compact writes voxels (n_out, 3) int32 (i, j, k) in ascending bitmap
 * order (rows past n_out are not written). ------------------------------------------- */
int64_t anr_voxel_n_blocks(int64_t n_words);
int anr_voxel_traverse(const double* u, const double* end, int64_t R, int32_t i0, int32_t j0,
                       int32_t k0, int32_t ni, int32_t nj, int32_t nk, int64_t row_pitch,
                       uint32_t* bitmap, int64_t* counters, int32_t shortcut,
                       anr_stream_t stream);
int anr_voxel_count(const uint32_t* bitmap, int32_t ni, int32_t nj, int32_t nk,
                    int64_t row_pitch, int32_t* counts, anr_stream_t stream);
int anr_voxel_compact(const uint32_t* bitmap, int32_t i0, int32_t j0, int32_t k0, int32_t ni,
                      int32_t nj, int32_t nk, int64_t row_pitch, const int64_t* offsets,
                      int64_t n_out, int32_t* voxels, anr_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Orbit video of an extracted volume: single-scattering ray marcher over a dense density
 * cube (csrc/volume_render.hip; the reference's scripts/make_video.py:174-194 runs OpenVDB's
 * vdb_render, a CPU ray marcher, once per frame). The arithmetic below is this project's
 * definition, written after vdb_render's VolumeRender and its defaults; parity with
 * vdb_render: unpinned (neither its source nor its binary was available to compare with).
 * density: (nx, ny, nz) f32, contiguous, z fastest, read in place (no padded or re-laid-out
 * copy); nx * ny * nz * 4 < 2^31. Voxel (i, j, k) sits at position (i, j, k); D(p) is the
 * trilinear interpolation of the eight voxels around floor(p) (z pairs, then y, then x, each
 * a + w (b - a)), voxels outside the array being 0.
 * cameras: F anr_camera in DEVICE memory. forward, right, up: an orthogonal basis, right
 * scaled by tan(hfov / 2) and up by tan(hfov / 2) * H / W. Pixel (col, row), row 0 at the
 * top, looks along normalize(forward + (2 (col + 1/2) / W - 1) right - (2 (row + 1/2) / H - 1)
 * up).
 * params: a HOST struct, read during the call. Per channel ext = -(absorb + scatter), albedo =
 * light_color * scatter / (absorb + scatter) (0 where the denominator is 0); light_dir is a
 * unit vector towards the light.
 * Per pixel: the ray is clipped by a slab test to the box [-1, n_d] per axis, outside of which
 * D is 0, giving [t0, t1] with t0 clamped to >= 0; a direction component of exactly 0
 * constrains nothing if the eye lies inside that slab, and the ray misses otherwise. A miss
 * writes RGBA = 0. Else, with T = (1, 1, 1) and L = (0, 0, 0), for t = primary_step *
 * ceil(t0 / primary_step) + n * primary_step, n = 0, 1, ..., while t <= t1:
 *   d = D(eye + t dir); if d < cutoff the step is skipped; dT = exp(ext * d * primary_step);
 *   the shadow ray from that point along light_dir is clipped to the same box, giving [0, s1];
 *   with sT = (1, 1, 1), for s = shadow_step, 2 shadow_step, ... <= s1: ds = D(p + s
 *   light_dir); if ds < cutoff continue; sT *= exp(ext * ds * shadow_step / (1 + s *
 *   light_gain)); the shadow ray stops once |sT|^2 < cutoff;
 *   L += albedo * sT * T * (1 - dT), T *= dT; the pixel stops once |T|^2 < cutoff.
 * rgba: (F, H, W, 4) f32 WRITTEN: RGB = L, A = 1 - (T.r + T.g + T.b) / 3.
 * All of it in f32, in the order written, without FMA contraction (tests/volume_checks.py
 * restates it in numpy). Frames are independent: F cameras in one launch give the bits of F
 * launches. ANR_E_INVALID, before any launch: a null pointer, an extent < 1, a cube of 2^31
 * bytes or more, a step that is not positive, a negative coefficient, a light_dir whose
 * length is not 1 within 1e-3. F * H * W = 0: ANR_OK without a launch. Allocates nothing and
 * does not synchronise. ------------------------------------------------------------------ */
typedef struct {
  float eye[3], forward[3], right[3], up[3];
} anr_camera;
typedef struct {
  float absorb[3], scatter[3];
  float light_dir[3], light_color[3];
  float primary_step, shadow_step; /* in voxels */
  float light_gain, cutoff;
} anr_volume_params;
int anr_volume_render(const float* density, int64_t nx, int64_t ny, int64_t nz,
                      const anr_camera* cameras, int64_t F, int64_t H, int64_t W,
                      const anr_volume_params* params, float* rgba, anr_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Global view of a global-grid extract: a sparse volume and the same march over it
 * (csrc/sparse_volume.hip; the reference writes the global grid as a sparse OpenVDB file for
 * an external viewer). The volume describes the box [0, ni) x [0, nj) x [0, nk) in
 * box-relative indices: voxel (i, j, k) of the grid sits at position (i - i0, j - j0, k - k0).
 * cells: (n_words, 2) uint32, n_words = row_pitch / 32 * nj * nk < 2^31, one {bits, rank}
 * pair per word of the bitmap above (i fastest, row_pitch a multiple of 32 that is >= ni, bit
 * b of word w of row (j, k) is voxel (32 w + b, j, k), pad bits 0); rank is the number of set
 * bits in all words before it. values: (n_values) f32 in ascending bitmap order, so a present
 * voxel's value is values[rank + popcount(bits & ((1 << b) - 1))]; 1 <= n_values < 2^31.
 * coarse: anr_sparse_volume_coarse_words(ni, nj, nk) uint32 words, one bit per brick of
 * 8 x 8 x 8 samples: brick (bi, bj, bk), bi fastest among (n >> 3) + 1 per axis, holds the
 * samples with (floor(p) + 1) >> 3 = (bi, bj, bk) and is set if any present voxel v has v or
 * v - 1 (per axis) as such a floor(p). A sample in an unset brick has all eight corners
 * absent. coarse may be null when every call passes skip = 0.
 * Build, in this order, on caller-zeroed cells and coarse; each call is independent of the
 * order of the input voxels:
 *   anr_sparse_volume_mark: voxels (n, 3) int32 grid indices, 1 <= n < 2^31; sets each voxel's
 *     bit and its bricks. A voxel outside the box is not marked.
 *   anr_sparse_volume_popcount: counts[w] (n_words, int32) = popcount(bits of word w); the
 *     caller writes the exclusive prefix sum into the rank fields and refuses an input whose
 *     total differs from n (a duplicate, or a voxel outside the box).
 *   anr_sparse_volume_place: out[rank of voxel r] = values[r] * density_scale, the product in
 *     f64 and rounded once to f32, NaN becoming 0 (VDB's background); values (n) f32.
 * D(p) is anr_volume_render's: the trilinear interpolation of the eight voxels around
 * floor(p) (z pairs, then y, then x, each a + w (b - a)), absent voxels and voxels outside the
 * box being 0, so D vanishes outside [-1, n_d] per axis.
 * anr_sparse_volume_sample: positions (P, 3) f32 box-relative -> out (P) f32 D(p); NaN and
 * far-away positions give 0.
 * anr_sparse_volume_render: cameras (box-relative coordinates), params, rgba and every
 * refusal as anr_volume_render, except that no byte limit applies to the box. The output
 * equals, bit for bit, anr_volume_render on the densified cube ((ni, nj, nk) f32, zeros where
 * no voxel is): the march is the same code, and every t comes from the step index.
 * skip 1: a sample in an unset brick returns +0.0 without its eight lookups, which is the
 * value they give; 0: every sample looks its corners up (same output; for tests and timing).
 * counters: null, or two int64 in DEVICE memory, added to (the caller zeroes them): [0]
 * samples whose floor(p) lies in [-1, n - 1] on every axis, [1] those of them the coarse level
 * answered. volume is a HOST struct, read during the call. ANR_E_INVALID, before any launch:
 * a null pointer, an extent < 1, a bad row_pitch, 2^31 words or bricks or more, n_values
 * outside [1, 2^31), skip other than 0 or 1. P = 0 or F * H * W = 0: ANR_OK without a launch.
 * Nothing here allocates or synchronises. ------------------------------------------------ */
typedef struct {
  const uint32_t* cells; /* DEVICE (n_words, 2) {bits, rank} */
  const float* values;   /* DEVICE (n_values) */
  const uint32_t* coarse; /* DEVICE brick bits, or null (skip = 0 only) */
  int32_t ni, nj, nk;
  int32_t reserved; /* 0 */
  int64_t row_pitch;
  int64_t n_values;
} anr_sparse_volume;
int64_t anr_sparse_volume_coarse_words(int32_t ni, int32_t nj, int32_t nk);
int anr_sparse_volume_mark(const int32_t* voxels, int64_t n, int32_t i0, int32_t j0, int32_t k0,
                           int32_t ni, int32_t nj, int32_t nk, int64_t row_pitch,
                           uint32_t* cells, uint32_t* coarse, anr_stream_t stream);
int anr_sparse_volume_popcount(const uint32_t* cells, int64_t n_words, int32_t* counts,
                               anr_stream_t stream);
int anr_sparse_volume_place(const int32_t* voxels, const float* values, int64_t n,
                            double density_scale, int32_t i0, int32_t j0, int32_t k0, int32_t ni,
                            int32_t nj, int32_t nk, int64_t row_pitch, const uint32_t* cells,
                            int64_t n_values, float* out, anr_stream_t stream);
int anr_sparse_volume_sample(const anr_sparse_volume* volume, int32_t skip,
                             const float* positions, int64_t P, float* out,
                             anr_stream_t stream);
int anr_sparse_volume_render(const anr_sparse_volume* volume, int32_t skip,
                             const anr_camera* cameras, int64_t F, int64_t H, int64_t W,
                             const anr_volume_params* params, float* rgba, int64_t* counters,
                             anr_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Light volume: precomputed shadows, a second shadow mode of the two marchers above
 * (csrc/volume_march.h). The light does not move during an orbit, so the shadow optical depth
 * of every voxel is summed once and interpolated at each primary sample. An interpolated
 * shadow is not a marched one: this mode has its own definition, below, and its own yardstick
 * (tests/light_volume_checks.py); the marched entries are unchanged and remain the default.
 * Parity with vdb_render: unpinned. D(p), the slab clip, the cameras and anr_volume_params are
 * anr_volume_render's; all arithmetic is f32, in the written order, without FMA contraction.
 * Light volume tau: defined at every voxel v with density > 0; other voxels hold 0 and are
 * never read. It is the marched shadow loop from p = the voxel's position, the light ray
 * clipped to the box giving [0, s1]: for q = 1, 2, ... while s = q * shadow_step <= s1:
 * ds = D(p + s light_dir); skipped if ds < cutoff; else tau += ds * shadow_step / (1 + s *
 * light_gain). No early termination: tau is a plain sum and does not depend on the channels.
 * The loop keeps the march's integer bound.
 * Lit march: the primary loop of anr_volume_render with one change. At a sample with d >=
 * cutoff the shadow march is replaced by: over the eight corners floor(p) + {0, 1}^3, x
 * outermost and z innermost, the low corner first, ww = (wx_a * wy_b) * wz_c, where w_a is
 * 1 - w for the low corner and w for the high one and w = p - floor(p); a corner takes part
 * only if it lies inside the array (sparse: is present) and its density is > 0; num += ww *
 * tau_c and den += ww over the corners that take part; tau_hat = den > 0 ? num / den : 0;
 * sT[ch] = expf(ext[ch] * tau_hat). d, dT, T, the termination test and A are computed exactly
 * as in the marched mode, so the alpha channel of a lit frame equals the marched frame's bit
 * for bit. The corner rule depends on values, never on presence, so the sparse entries give
 * the bits of the dense ones on the densified cube in this mode too.
 * A tau is valid only for the density it was built from and for the same light_dir,
 * shadow_step, light_gain and cutoff; the entries cannot check that.
 * anr_volume_light: tau (nx, ny, nz) f32 WRITTEN, the cube's layout, every voxel (0 where the
 * density is not > 0); one thread per voxel. anr_sparse_volume_light: tau (n_values) f32
 * WRITTEN in value order, so the rank that finds a corner's density finds its tau; one thread
 * per value, which finds its voxel by a binary search of the ranks; skip as in the render.
 * Both take the whole anr_volume_params and refuse what the renders refuse in it.
 * anr_volume_render_lit, anr_sparse_volume_render_lit: the render entries' arguments and
 * refusals, plus tau (DEVICE, as written by the light entry of the same volume; null is
 * refused). F * H * W = 0: ANR_OK without a launch. There is no empty build: a cube has
 * extents >= 1 and a sparse volume n_values >= 1. None of the four allocates or synchronises.
 * ------------------------------------------------------------------------------------ */
int anr_volume_light(const float* density, int64_t nx, int64_t ny, int64_t nz,
                     const anr_volume_params* params, float* tau, anr_stream_t stream);
int anr_volume_render_lit(const float* density, const float* tau, int64_t nx, int64_t ny,
                          int64_t nz, const anr_camera* cameras, int64_t F, int64_t H, int64_t W,
                          const anr_volume_params* params, float* rgba, anr_stream_t stream);
int anr_sparse_volume_light(const anr_sparse_volume* volume, int32_t skip,
                            const anr_volume_params* params, float* tau, anr_stream_t stream);
int anr_sparse_volume_render_lit(const anr_sparse_volume* volume, const float* tau, int32_t skip,
                                 const anr_camera* cameras, int64_t F, int64_t H, int64_t W,
                                 const anr_volume_params* params, float* rgba, int64_t* counters,
                                 anr_stream_t stream);

/* ------------------------------------------------------------------------------------
 * NeRF path (configs/nerf.json): positional encoding (encoders.py:4-28) and the
 * hierarchical pdf sampler (samplers.py:50-103), forward and backward.
 * ------------------------------------------------------------------------------------ */
#define ANR_POSENC_MAX_DIMS 8
typedef struct {
  int32_t n_dims;       /* input coordinates per row */
  int32_t interleaved;  /* 1: int L (per coordinate [sin f0, cos f0, sin f1, ...]),
                           0: list L (per coordinate [sin f0..f(L-1), cos f0..f(L-1)]) */
  int32_t L[ANR_POSENC_MAX_DIMS]; /* frequencies per coordinate (interleaved: L[0] for all) */
} anr_posenc_desc;
/* Output width (2 * sum of L), or -1 for a bad descriptor. */
int32_t anr_posenc_width(const anr_posenc_desc* d);
/* out (P, >= width) f32 row r = encoding of x row r / rows_per_x (x (P/rows_per_x, n_dims)
 * f32); frequencies (2^l * pi) in f32 times x in f32, sinf/cosf. */
int anr_posenc_fwd(const anr_posenc_desc* d, const float* x, int64_t rows_per_x, int64_t P,
                   float* out, int64_t out_stride, anr_stream_t stream);
/* dx (P, n_dims) f32 WRITTEN from dL/dout (P, >= width). */
int anr_posenc_bwd(const anr_posenc_desc* d, const float* x, int64_t P, const float* dout,
                   int64_t dout_stride, float* dx, anr_stream_t stream);
/* AtmoNeRF Linear+ReLU backward (models/nerf.py:48-93; replaces autograd's
 * threshold_backward + bias-gradient reduction): g_out = g where y > 0 else 0, for
 * contiguous (M, C) f32 g, y, g_out (C a multiple of 4, <= 1024, 16-byte aligned); and
 * partial (n_parts, C) f32 WRITTEN with the column sums of g_out over n_parts row blocks
 * (fixed order; the bias gradient is their sum; M = 0 writes zeros, g/y/g_out may be
 * NULL then). */
int anr_relu_bwd_colsum(const float* g, const float* y, int64_t M, int32_t C, float* g_out,
                        float* partial, int32_t n_parts, anr_stream_t stream);
/* AtmoNeRF dense layers on the f32 matrix cores (csrc/nerf_mlp.hip). They replace the
 * nn.Linear / torch.cat / F.relu calls of src/atmonr/models/nerf.py:48-93 and their
 * autograd backward. Operands are row-major f32 with 16-byte-aligned rows: every leading
 * dimension and segment width is a multiple of 4.
 *
 * Forward: y (M x n, row stride ldy >= round_up(n, 4)) = [a1 | a2] W^T + bias, then ReLU
 * if relu != 0. Columns n .. round_up(n, 4) come out zero.
 *   a1 is M x q1 and a2 is M x q2 (q2 = 0: none; q1 % 16 == 0 when q2 > 0). They are the
 *   fc6 skip and fc10 direction concats, read in place.
 *   W is n x (q1+q2), as nn.Linear.weight. bias is nullable.
 *   relu_bits is nullable. If given, it receives M x ceil(n/64) 64-bit words, one bit
 *   per element: y[m][64w + 16j + 4g + r] > 0 is bit 16g + 4j + r of word w of row m.
 *   That is the ReLU mask for the layer's backward, 32x smaller than the activations. */
int anr_nerf_linear_fwd(const float* a1, int64_t lda1, int32_t q1, const float* a2,
                        int64_t lda2, int32_t q2, int64_t M, const float* w, int32_t n,
                        const float* bias, int32_t relu, float* y, int64_t ldy,
                        uint64_t* relu_bits, anr_stream_t stream);
/* Input gradient: [dx1 | dx2] (M x (p1+p2)) = g (M x n) W, with wt = W^T
 * ((p1+p2) x n, row stride ldwt).
 *   p1 % 4 == 0 and p2 % 4 == 0.
 *   If n % 4 != 0, g's and wt's columns n .. round_up(n, 4) must exist and be zero.
 *   dx1 (first p1 columns) is zeroed where the bit in mask_bits is clear. mask_bits is
 *   the relu_bits of the forward that produced the input, M x ceil(p1/64) words, or
 *   NULL for no mask. This is the ReLU backward of the layer below.
 *   dx2 (last p2 columns) is written, or added to if acc2 != 0. */
int anr_nerf_linear_dx(const float* g, int64_t ldg, int64_t M, int32_t n, const float* wt,
                       int64_t ldwt, int32_t p1, int32_t p2, const uint64_t* mask_bits,
                       float* dx1, int64_t ldx1, float* dx2, int64_t ldx2, int32_t acc2,
                       anr_stream_t stream);
/* Parameter gradients, ACCUMULATED: dw (n x (q1+q2), contiguous) += g^T [a1 | a2], and
 * db (n, nullable) += the column sums of g.
 *   g's columns n .. round_up(n, 4) must be zero.
 *   M is split over blocks into f32 partials in ws (anr_nerf_linear_dw_workspace bytes,
 *   16-byte aligned), summed in a fixed order: the result is deterministic. */
int64_t anr_nerf_linear_dw_workspace(int64_t M, int32_t n, int32_t k);
int anr_nerf_linear_dw(const float* g, int64_t ldg, int64_t M, int32_t n, const float* a1,
                       int64_t lda1, int32_t q1, const float* a2, int64_t lda2, int32_t q2,
                       float* dw, float* db, void* ws, int64_t ws_bytes, anr_stream_t stream);
/* sample_pdf forward, one wavefront per ray (3 <= Nc <= 64, 1 <= Nf <= 256).
 *   weights: coarse render weights, element (b, j) at b*w_ray_stride + j*w_sample_stride
 *   (channel 0 of (B, Nc, S)); z_coarse (B,Nc) f32 ascending; u (B,Nf) f32 draws.
 *   Outputs: z (B, Nc+Nf) sorted, pts (B, Nc+Nf, 3) = o + d*z (nullable), src (B, Nc+Nf)
 *   int32 (source of each sorted value: < Nc coarse, else Nc + sample), inds (B,Nf) int32
 *   = searchsorted(cdf, u, right=True), cdf (B, Nc-1) f32 (saved for the backward). */
int anr_sample_pdf_fwd(const float* weights, int64_t w_ray_stride, int32_t w_sample_stride,
                       const float* z_coarse, const float* u, const float* origin,
                       const float* dir, int64_t B, int32_t Nc, int32_t Nf, float* z,
                       float* pts, int32_t* src, int32_t* inds, float* cdf,
                       anr_stream_t stream);
/* Backward into the weights through t_in_bin (bin width detached): d_z (B, Nc+Nf) and/or
 * d_pts (B, Nc+Nf, 3) (each nullable) -> d_weights channel 0 WRITTEN (rest untouched). */
int anr_sample_pdf_bwd(const float* weights, int64_t w_ray_stride, int32_t w_sample_stride,
                       const float* z_coarse, const float* u, const float* dir,
                       const int32_t* src, const int32_t* inds, const float* cdf, int64_t B,
                       int32_t Nc, int32_t Nf, const float* d_z, const float* d_pts,
                       float* d_weights, anr_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K8: transmittance / alpha-composite integrator, render + render_with_surface
 * (graphics_utils.py:6-77), one wavefront per ray with shuffle prefix scans.
 * ------------------------------------------------------------------------------------
 * z (B,N) f32 multiplied by z_scale in f32 (instant_ngp.py:188 z_vals*(scale/1000));
 * color (B,N,C) and sigma (B,N,S) (S = 1 or C) in io_dtype; color_surf (B,C) or NULL
 * (plain render). Outputs (nullable unless noted): color_map (B,C) [required],
 * color_map_atmo, color_map_surf (B,C), weights (B,N,S), alpha (B,N,S); io_dtype.
 * Arithmetic is f32 internally. */
int anr_composite_fwd(const float* z, float z_scale, const void* color, const void* sigma,
                      const void* color_surf, int32_t io_dtype, int64_t B, int32_t N,
                      int32_t C, int32_t S, void* color_map, void* color_map_atmo,
                      void* color_map_surf, void* weights, void* alpha,
                      anr_stream_t stream);
/* Use the generic kernels instead of the register-blocked ones (C = 4, S in {1,4},
 * N/64 in {1,2,3,4,8,16}). Test hook; process-wide. Returns the previous setting. */
int anr_composite_force_generic(int32_t on);
/* Backward. Gradients in (nullable; io_dtype): d_color_map, d_atmo, d_surf (B,C),
 * d_weights (B,N,S), d_alpha (B,N,S). Outputs (nullable): d_color (B,N,C),
 * d_sigma (B,N,S), d_color_surf (B,C) (io_dtype), d_z (B,N) f32 (dL/dz before scaling
 * by z_scale is applied, i.e. w.r.t. the unscaled z input). Shapes outside the
 * register-blocked kernels, and S = 4 with N > 3840, run the generic backward, which stages
 * (2S+1)*N floats per ray in LDS and returns ANR_E_INVALID ("too large") above 64 KiB. */
int anr_composite_bwd(const float* z, float z_scale, const void* color, const void* sigma,
                      const void* color_surf, int32_t io_dtype, int64_t B, int32_t N,
                      int32_t C, int32_t S, const void* d_color_map, const void* d_atmo,
                      const void* d_surf, const void* d_weights, const void* d_alpha,
                      void* d_color, void* d_sigma, void* d_color_surf, float* d_z,
                      anr_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K9: losses (losses.py:5-33) on pred = take_along_dim(color_map, irgb_idx)
 * (instant_ngp.py:259-263). Writes the scalar loss (f32) and dL/dcolor_map (B,C).
 * ------------------------------------------------------------------------------------ */
enum anr_loss { ANR_LOSS_DARK = 0, ANR_LOSS_HDR = 1, ANR_LOSS_L1 = 2,
                ANR_LOSS_L1_PLUS_HDR = 3, ANR_LOSS_MSE = 4, ANR_LOSS_MSE_PLUS_HDR = 5 };
/* color_map (B,C) pred_dtype, irgb_idx (B,) int64, gt (B,) f32. loss_out: 1 f32.
 * grad_out (nullable): (B,C) pred_dtype, dL/dcolor_map scaled by grad_scale.
 * workspace: >= anr_loss_workspace_bytes(B) bytes (f32 partial sums). */
int64_t anr_loss_workspace_bytes(int64_t B);
int anr_loss_fwd_bwd(int32_t loss_type, const void* color_map, int32_t pred_dtype,
                     int32_t C, const int64_t* irgb_idx, const float* gt, int64_t B,
                     float max_i, float grad_scale, float* loss_out, void* grad_out,
                     void* workspace, anr_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Reference numerics (csrc/ref16.hip; opt-in, InstantNGPPipeline(numerics="reference")).
 * The reference's Instant-NGP composite and loss run as chains of torch f16 ops on f16
 * tinycudann outputs (graphics_utils.py:28-76, instant_ngp.py:259-263, losses.py:5-33),
 * and tcnn's backward is loss-scaled f16 (tinycudann/modules.py, loss scale 128). These
 * entry points reproduce those roundings op by op (oracle/ref_f16.py is the restatement;
 * torch's CUDA accumulation: f16 accumulator in cumprod / cumsum, f32 in sum / prod).
 * R rays per wavefront (2, or 1 below 8,192 rays): lane-parallel per-sample ops, the order-sensitive
 * accumulations as serial scans, lane r for ray r.
 * ------------------------------------------------------------------------------------
 * Forward: z (B,N) f32 times z_scale in f32 then rounded to f16; color (B,N,C), sigma
 * (B,N,1), color_surf (B,C) (nullable) in in_dtype, rounded to f16 on load. Outputs f16:
 * color_map (B,C) [required], color_map_atmo, color_map_surf (B,C), weights, alpha
 * (B,N,1) (nullable); color16 (B,N,C), sigma16 (B,N,1) (nullable): the f16-rounded
 * inputs, i.e. tcnn's f16 outputs the reference's forward returns (instant_ngp.py:194-206).
 * Replaces render_with_surface (graphics_utils.py:52-77) at instant_ngp.py:187-192 in that
 * mode. */
/* Rays per wavefront of the two composite kernels: 1, 2, 4 or 8, or 0 for the default
 * (2 from 8,192 rays up, else 1); halved while R * C > 64. Outputs do
 * not depend on it. */
int anr_composite_ref16_set_rays(int32_t rays_per_wave);
int anr_composite_ref16_fwd(const float* z, float z_scale, const void* color,
                            const void* sigma, const void* color_surf, int32_t in_dtype,
                            int64_t B, int32_t N, int32_t C, void* color_map,
                            void* color_map_atmo, void* color_map_surf, void* weights,
                            void* alpha, void* color16, void* sigma16, anr_stream_t stream);
/* Backward from dL/dcolor_map (B,C) f16 (torch's f16 autograd of the forward).
 * d_color (B,N,C), d_sigma (B,N,1) [required; both also scratch between the kernel's two
 * passes: the cumprod outputs and exp(-sigma delta), with out_dtype f16 and C >= 2 as one
 * 4-byte pair per sample in the ray's d_color rows] and
 * d_color_surf (B,C) (nullable) in out_dtype, holding f16 values. zero_rays: one int32
 * (device), incremented per ray in which alpha rounded to exactly 1 (torch's zero-input
 * backward branches, not reproduced: that ray's gradients are 0). */
int anr_composite_ref16_bwd(const float* z, float z_scale, const void* color,
                            const void* sigma, const void* color_surf, int32_t in_dtype,
                            int64_t B, int32_t N, int32_t C, const void* d_color_map,
                            void* d_color, void* d_sigma, void* d_color_surf,
                            int32_t out_dtype, int32_t* zero_rays, anr_stream_t stream);
/* The pair a training step runs: the forward also parks what the backward would otherwise
 * recompute from z and sigma, and the backward reads it back instead of replaying the
 * forward (no first pass, sigma is not read and may be null, d_color / d_sigma are outputs
 * only). Same arguments, outputs and gradients as the two entry points above, bit for bit.
 * park (B*N): per sample the f16 bits of T_i (the cumprod output, low half) and of
 * exp(-sigma_i delta_i) (high half). ray_park (B): the f16 bits of the surface product
 * prod(1 - alpha) in the low half, bit 16 set when an alpha of the ray rounded to exactly 1
 * (the rays zero_rays counts). Both required, 4-byte aligned, independent of the dtypes;
 * a park is valid only for the z / color / sigma / color_surf it was written from. */
int anr_composite_ref16_fwd_park(const float* z, float z_scale, const void* color,
                                 const void* sigma, const void* color_surf, int32_t in_dtype,
                                 int64_t B, int32_t N, int32_t C, void* color_map,
                                 void* color_map_atmo, void* color_map_surf, void* weights,
                                 void* alpha, void* color16, void* sigma16, uint32_t* park,
                                 uint32_t* ray_park, anr_stream_t stream);
int anr_composite_ref16_bwd_parked(const float* z, float z_scale, const void* color,
                                   const void* sigma, const void* color_surf,
                                   int32_t in_dtype, int64_t B, int32_t N, int32_t C,
                                   const void* d_color_map, void* d_color, void* d_sigma,
                                   void* d_color_surf, int32_t out_dtype, int32_t* zero_rays,
                                   const uint32_t* park, const uint32_t* ray_park,
                                   anr_stream_t stream);
/* Loss in f16 ops: color_map (B,C) f16, gt (B,) f32 (cast to f16 as instant_ngp.py:262),
 * loss_out: 1 f32 holding the f16 loss value, grad_out (B,C) f16 (nullable),
 * workspace >= anr_loss_workspace_bytes(B). */
int anr_loss_ref16_fwd_bwd(int32_t loss_type, const void* color_map, int32_t C,
                           const int64_t* irgb_idx, const float* gt, int64_t B, float max_i,
                           float* loss_out, void* grad_out, void* workspace,
                           anr_stream_t stream);
/* tcnn's parameter gradient of an f16 module at loss scale s: g <- f16(f16(g*s)/s), in
 * place over n f32 values (the value tinycudann/modules.py hands to torch). */
int anr_grad_quantize_f16(float* grad, int64_t n, float loss_scale, anr_stream_t stream);
/* One module call's parameter gradient, rounded the same way and added to the caller's
 * gradient: grad[i] += f16(f16(scratch[i]*s)/s), then scratch[i] = 0, over n f32 values
 * (tinycudann rounds per module call, so a call's sums are scattered into a zeroed scratch
 * of the module's, which this leaves zeroed for the next call). scratch and grad are any
 * two 4-byte-aligned, non-overlapping ranges (grad may be a view at any offset of a flat
 * bucket); n == 0 is accepted. Equal bit for bit to anr_grad_quantize_f16 on scratch
 * followed by grad += scratch. */
int anr_grad_quantize_add_f16(float* scratch, float* grad, int64_t n, float loss_scale,
                              anr_stream_t stream);
/* The fused field backward (anr_ingp_field_bwd) with tcnn's backward semantics: fixed
 * f16 gradient scale loss_scale (128), ReLU masks on the f16 outputs, and the
 * module-boundary gradients of the reference (dir_mlp -> dir_encoder -> pos_out, pos_mlp
 * -> pos_encoder) rounded as f16(f16(g_scaled)/loss_scale). f16 networks, dense rows; no
 * workspace. */
int anr_ingp_field_bwd_ref16(const anr_mlp_desc* pos, const anr_mlp_desc* dir,
                             const void* packed, const void* enc, int64_t enc_stride,
                             const float* dirs, int64_t n_per_ray, int64_t M,
                             const float* d_sigma, const float* d_color,
                             int64_t d_color_stride, float* d_enc, int64_t d_enc_stride,
                             float* g_pos, float* g_dir, float loss_scale,
                             anr_stream_t stream);
/* anr_ingp_field_bwd_ref16 that also writes, per 32-row tile t of the M rows, tile_nz[t]
 * = 1 if any row of the tile had a nonzero dL/dcolor or dL/dsigma (the tile was walked)
 * and 0 otherwise (skipped: its dL/denc rows are written as 0). tile_nz: ceil(M / 32)
 * bytes of device memory, for anr_hashgrid_bwd_tiles. */
int anr_ingp_field_bwd_ref16_tiles(const anr_mlp_desc* pos, const anr_mlp_desc* dir,
                                   const void* packed, const void* enc, int64_t enc_stride,
                                   const float* dirs, int64_t n_per_ray, int64_t M,
                                   const float* d_sigma, const float* d_color,
                                   int64_t d_color_stride, float* d_enc, int64_t d_enc_stride,
                                   float* g_pos, float* g_dir, float loss_scale,
                                   uint8_t* tile_nz, anr_stream_t stream);
/* anr_ingp_field_bwd_ref16 writing dL/denc as f16 rows (d_enc_h: (M, >= 32) halves, row
 * stride d_enc_stride, 8-byte aligned; the reference numerics' dL/denc values are f16
 * numbers, tinycudann/modules.py casts them to the f16 input's dtype, so the rows hold them
 * exactly) and one bit per row in row_nz (ceil(M / 32) words): bit (m % 32) of word m / 32
 * set iff row m has a nonzero value; every row is written (skipping the clear ones made
 * partial 128-B line writes: slower, profiles/r06_field_bwd_skip_clear_rows_ab.log). For
 * anr_hashgrid_bwd_rows (ABI 5).
 * workspace (nullable, 256-byte aligned, anr_ingp_field_bwd_ref16_rows_workspace_bytes(M)
 * bytes): with it the backward runs as a pos pass over the tiles whose dL/dcolor is zero in
 * every row (the dir network adds exactly 0 there) and a full pass over the others, listed
 * in the workspace by the first; the same results. Without it, one kernel does both. */
int64_t anr_ingp_field_bwd_ref16_rows_workspace_bytes(int64_t M);
int anr_ingp_field_bwd_ref16_rows(const anr_mlp_desc* pos, const anr_mlp_desc* dir,
                                  const void* packed, const void* enc, int64_t enc_stride,
                                  const float* dirs, int64_t n_per_ray, int64_t M,
                                  const float* d_sigma, const float* d_color,
                                  int64_t d_color_stride, void* d_enc_h, int64_t d_enc_stride,
                                  float* g_pos, float* g_dir, float loss_scale,
                                  uint32_t* row_nz, void* workspace, int64_t workspace_bytes,
                                  anr_stream_t stream);
/* anr_ingp_field_bwd_ref16_rows reading d_sigma (M) and d_color (M, d_color_stride) as f16
 * (the f16 composite backward's outputs; d_color 8-byte aligned when d_color_stride is a
 * multiple of 4). f16 -> f32 is exact: the same results as the f32 entry on the same
 * values, from half the gradient bytes. */
int anr_ingp_field_bwd_ref16_rows_h(const anr_mlp_desc* pos, const anr_mlp_desc* dir,
                                    const void* packed, const void* enc, int64_t enc_stride,
                                    const float* dirs, int64_t n_per_ray, int64_t M,
                                    const void* d_sigma, const void* d_color,
                                    int64_t d_color_stride, void* d_enc_h, int64_t d_enc_stride,
                                    float* g_pos, float* g_dir, float loss_scale,
                                    uint32_t* row_nz, void* workspace, int64_t workspace_bytes,
                                    anr_stream_t stream);
/* anr_mlp_bwd_ws in f16 with tcnn's fixed loss scale: dL/dinput written as
 * f16(f16(g_scaled)/loss_scale). Specialised (fused) MLP shapes only. */
int anr_mlp_bwd_ref16(const anr_mlp_desc* d, const void* params, const void* in,
                      int32_t in_dtype, int64_t in_stride, int64_t M, const void* dout,
                      int32_t dout_dtype, int64_t dout_stride, void* din, int32_t din_dtype,
                      int64_t din_stride, float* dparams, void* workspace,
                      int64_t workspace_bytes, float loss_scale, anr_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K10: fused AdamW (torch.optim.AdamW, instant_ngp.py:120-126; Adam nerf.py:70 is
 * weight_decay = 0, decoupled = 0) over one flat f32 parameter buffer.
 * ------------------------------------------------------------------------------------
 * step is the 1-based step count after increment. params_f16 (nullable) receives an
 * f16 shadow copy of the updated params (the tcnn forward precision). If zero_grad,
 * grad is zeroed after use (fused optimizer.zero_grad). decoupled = 1: AdamW
 * (p *= 1 - lr*wd); decoupled = 0: Adam with L2 (g += wd*p). */
int anr_adam_step(float* params, float* grad, float* exp_avg, float* exp_avg_sq,
                  void* params_f16, int64_t n, float lr, float beta1, float beta2,
                  float eps, float weight_decay, int32_t decoupled, int64_t step,
                  int32_t zero_grad, anr_stream_t stream);

/* Every tensor of one optimizer step (torch.optim.AdamW.step over all param groups,
 * instant_ngp.py:120-126 / trainer.py:105) in one launch: per tensor its own lr,
 * weight_decay and step count; beta1/2, eps, decoupled and zero_grad shared. Tensors
 * travel in the kernel arguments, ANR_ADAM_MAX_TENSORS per launch (more: several
 * launches, same stream). Same arithmetic as anr_adam_step. */
#define ANR_ADAM_MAX_TENSORS 16
typedef struct anr_adam_tensor {
  float* params;
  float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  void* params_f16; /* nullable f16 shadow */
  int64_t n;
  float lr;
  float weight_decay;
  int64_t step;
  /* > 0: the gradient is first rounded as tinycudann's f16 parameter gradient at this
   * loss scale, g <- f16(f16(g * s) / s) (anr_grad_quantize_f16, fused into the update's
   * read of g; reference numerics with a deferred quantisation). 0: g as it is. */
  float grad_quant;
} anr_adam_tensor;
int anr_adam_step_multi(const anr_adam_tensor* tensors, int32_t n_tensors, float beta1,
                        float beta2, float eps, int32_t decoupled, int32_t zero_grad,
                        anr_stream_t stream);

/* anr_adam_step_multi with the step count and the learning rates in DEVICE memory, so
 * that one captured launch serves every replay of a hipGraph of the train step
 * (torch.optim.AdamW(capturable=True) keeps its step on the device for the same reason;
 * trainer.py:105 is the call site). Per call: *d_step += 1 on the device, then every
 * tensor t is updated with step = *d_step and lr = d_lr[t] (the descriptors' lr and
 * step fields are ignored; weight_decay and the pointers are taken from them at the
 * call). d_scratch: 3 * ANR_ADAM_DEV_MAX_TENSORS floats of caller-owned device memory
 * (the per-tensor bias-corrected scalars). At most ANR_ADAM_DEV_MAX_TENSORS tensors.
 * Same arithmetic as anr_adam_step_multi (bias corrections in double). */
#define ANR_ADAM_DEV_MAX_TENSORS 64
int anr_adam_step_multi_dev(const anr_adam_tensor* tensors, int32_t n_tensors, float beta1,
                            float beta2, float eps, int32_t decoupled, int32_t zero_grad,
                            int64_t* d_step, const float* d_lr, float* d_scratch,
                            anr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ANR_H_ */
