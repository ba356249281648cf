// Host-only walk over the argument refusals of the sparse volume's entries, of the two
// marchers and of the four light-volume entries (csrc/sparse_volume.hip,
// csrc/volume_render.hip, the shared plan of csrc/volume_march.h), for a sanitizer build (tools/host_check/run.sh: -Xarch_host
// -fsanitize=address,undefined). Every call here is refused, or is empty, before any launch:
// the pointers are fake and never dereferenced. Nothing here needs a GPU.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "../../include/anr.h"

static int fails = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);   \
      ++fails;                                                \
    }                                                         \
  } while (0)

static bool says(const char* word) { return strstr(anr_last_error(), word) != nullptr; }

static anr_volume_params params() {
  anr_volume_params p;
  memset(&p, 0, sizeof(p));
  for (int a = 0; a < 3; ++a) {
    p.absorb[a] = 0.1f;
    p.scatter[a] = 0.7f;
    p.light_color[a] = 1.0f;
  }
  p.light_dir[1] = 1.0f;
  p.primary_step = 1.0f;
  p.shadow_step = 3.0f;
  p.light_gain = 0.2f;
  p.cutoff = 0.01f;
  return p;
}

int main() {
  float* const fake_f = reinterpret_cast<float*>(0x10000);
  uint32_t* const fake_u = reinterpret_cast<uint32_t*>(0x10000);
  int32_t* const fake_i = reinterpret_cast<int32_t*>(0x10000);
  anr_camera* const fake_c = reinterpret_cast<anr_camera*>(0x10000);
  const anr_volume_params ok = params();
  anr_sparse_volume v;
  memset(&v, 0, sizeof(v));
  v.cells = fake_u;
  v.values = fake_f;
  v.coarse = fake_u;
  v.ni = 70;
  v.nj = 9;
  v.nk = 11;
  v.row_pitch = 96;
  v.n_values = 100;

  // the volume descriptor, through both entries that read it
  struct {
    void (*edit)(anr_sparse_volume*);
    const char* word;
  } bad[] = {
      {[](anr_sparse_volume* s) { s->cells = nullptr; }, "null pointer"},
      {[](anr_sparse_volume* s) { s->values = nullptr; }, "null pointer"},
      {[](anr_sparse_volume* s) { s->coarse = nullptr; }, "null pointer"},
      {[](anr_sparse_volume* s) { s->nj = 0; }, "extents"},
      {[](anr_sparse_volume* s) { s->nk = -3; }, "extents"},
      {[](anr_sparse_volume* s) { s->row_pitch = 64; }, "row_pitch"},
      {[](anr_sparse_volume* s) { s->row_pitch = 97; }, "row_pitch"},
      {[](anr_sparse_volume* s) { s->row_pitch = (1LL << 31) + 32; }, "row_pitch"},
      {[](anr_sparse_volume* s) { s->ni = s->nj = s->nk = 1 << 14; s->row_pitch = 1 << 14; },
       "2^31 bitmap words"},
      {[](anr_sparse_volume* s) { s->ni = s->nj = s->nk = 0x7fffffff; s->row_pitch = 1LL << 31; },
       "2^31 bitmap words"},
      {[](anr_sparse_volume* s) { s->n_values = 0; }, "n_values"},
      {[](anr_sparse_volume* s) { s->n_values = 1LL << 31; }, "n_values"},
  };
  for (const auto& b : bad) {
    anr_sparse_volume s = v;
    b.edit(&s);
    CHECK(anr_sparse_volume_render(&s, 1, fake_c, 3, 16, 24, &ok, fake_f, 0, 0) == ANR_E_INVALID);
    CHECK(says("anr_sparse_volume_render") && says(b.word));
    CHECK(anr_sparse_volume_sample(&s, 1, fake_f, 10, fake_f, 0) == ANR_E_INVALID);
    CHECK(says("anr_sparse_volume_sample") && says(b.word));
  }
  CHECK(anr_sparse_volume_render(0, 1, fake_c, 3, 16, 24, &ok, fake_f, 0, 0) == ANR_E_INVALID);
  CHECK(anr_sparse_volume_sample(0, 1, fake_f, 10, fake_f, 0) == ANR_E_INVALID);
  CHECK(anr_sparse_volume_render(&v, 2, fake_c, 3, 16, 24, &ok, fake_f, 0, 0) == ANR_E_INVALID);
  CHECK(says("skip"));
  CHECK(anr_sparse_volume_sample(&v, -1, fake_f, 10, fake_f, 0) == ANR_E_INVALID && says("skip"));
  CHECK(anr_sparse_volume_sample(&v, 1, fake_f, -1, fake_f, 0) == ANR_E_INVALID);
  CHECK(anr_sparse_volume_sample(&v, 1, 0, 10, fake_f, 0) == ANR_E_INVALID && says("null"));
  CHECK(anr_sparse_volume_sample(&v, 1, 0, 0, 0, 0) == ANR_OK);
  {  // skip = 0 needs no brick level: only the null output stops the call
    anr_sparse_volume s = v;
    s.coarse = nullptr;
    CHECK(anr_sparse_volume_render(&s, 0, fake_c, 3, 16, 24, &ok, 0, 0, 0) == ANR_E_INVALID);
    CHECK(says("null pointer"));
  }

  // image and parameters: the same refusals from the sparse and the dense entry
  struct {
    void (*edit)(anr_volume_params*);
    const char* word;
  } badp[] = {
      {[](anr_volume_params* p) { p->primary_step = 0.0f; }, "steps must be positive"},
      {[](anr_volume_params* p) { p->shadow_step = -3.0f; }, "steps must be positive"},
      {[](anr_volume_params* p) { p->primary_step = NAN; }, "steps must be positive"},
      {[](anr_volume_params* p) { p->shadow_step = INFINITY; }, "steps must be positive"},
      {[](anr_volume_params* p) { p->primary_step = 1e-30f; }, "steps too small"},
      {[](anr_volume_params* p) { p->absorb[1] = -0.1f; }, "negative coefficient"},
      {[](anr_volume_params* p) { p->scatter[2] = NAN; }, "negative coefficient"},
      {[](anr_volume_params* p) { p->light_color[0] = -1.0f; }, "negative coefficient"},
      {[](anr_volume_params* p) { p->light_gain = -0.2f; }, "negative coefficient"},
      {[](anr_volume_params* p) { p->cutoff = -0.01f; }, "negative coefficient"},
      {[](anr_volume_params* p) { p->light_dir[1] = 1.01f; }, "unit length"},
      {[](anr_volume_params* p) { p->light_dir[1] = 0.0f; }, "unit length"},
      {[](anr_volume_params* p) { p->light_dir[0] = NAN; }, "unit length"},
  };
  for (const auto& b : badp) {
    anr_volume_params p = ok;
    b.edit(&p);
    CHECK(anr_sparse_volume_render(&v, 1, fake_c, 3, 16, 24, &p, fake_f, 0, 0) == ANR_E_INVALID);
    CHECK(says("anr_sparse_volume_render") && says(b.word));
    CHECK(anr_volume_render(fake_f, 7, 5, 6, fake_c, 3, 16, 24, &p, fake_f, 0) == ANR_E_INVALID);
    CHECK(says("anr_volume_render") && says(b.word));
  }
  const int64_t shapes[][3] = {{-1, 16, 24}, {3, -16, 24}, {3, 16, 1 << 24}, {1LL << 31, 16, 24},
                               {1 << 20, 1 << 12, 1 << 12}};
  for (const auto& s : shapes) {
    CHECK(anr_sparse_volume_render(&v, 1, fake_c, s[0], s[1], s[2], &ok, fake_f, 0, 0) ==
          ANR_E_INVALID);
    CHECK(anr_volume_render(fake_f, 7, 5, 6, fake_c, s[0], s[1], s[2], &ok, fake_f, 0) ==
          ANR_E_INVALID);
  }
  CHECK(anr_sparse_volume_render(&v, 1, 0, 0, 16, 24, &ok, 0, 0, 0) == ANR_OK);
  CHECK(anr_sparse_volume_render(&v, 1, 0, 3, 0, 24, &ok, 0, 0, 0) == ANR_OK);
  CHECK(anr_sparse_volume_render(&v, 1, fake_c, 3, 16, 24, 0, fake_f, 0, 0) == ANR_E_INVALID);
  CHECK(anr_sparse_volume_render(&v, 1, 0, 3, 16, 24, &ok, fake_f, 0, 0) == ANR_E_INVALID);
  CHECK(anr_sparse_volume_render(&v, 1, fake_c, 3, 16, 24, &ok, 0, 0, 0) == ANR_E_INVALID);
  CHECK(anr_volume_render(fake_f, 1024, 1024, 512, fake_c, 3, 16, 24, &ok, fake_f, 0) ==
        ANR_E_INVALID);
  CHECK(says("2^31 bytes"));
  {  // the box whose dense cube is refused above passes here up to the pointer check
    anr_sparse_volume s = v;
    s.ni = 973;
    s.nj = 873;
    s.nk = 791;
    s.row_pitch = 992;
    s.n_values = 78316315;
    CHECK(anr_sparse_volume_render(&s, 1, fake_c, 3, 16, 24, &ok, 0, 0, 0) == ANR_E_INVALID);
    CHECK(says("null pointer"));
  }

  // the light volume: the descriptor, the parameters and the image through the four entries
  for (const auto& b : bad) {
    anr_sparse_volume s = v;
    b.edit(&s);
    CHECK(anr_sparse_volume_light(&s, 1, &ok, fake_f, 0) == ANR_E_INVALID);
    CHECK(says("anr_sparse_volume_light") && says(b.word));
    CHECK(anr_sparse_volume_render_lit(&s, fake_f, 1, fake_c, 3, 16, 24, &ok, fake_f, 0, 0) ==
          ANR_E_INVALID);
    CHECK(says("anr_sparse_volume_render_lit") && says(b.word));
  }
  for (const auto& b : badp) {
    anr_volume_params p = ok;
    b.edit(&p);
    CHECK(anr_volume_light(fake_f, 7, 5, 6, &p, fake_f, 0) == ANR_E_INVALID);
    CHECK(says("anr_volume_light") && says(b.word));
    CHECK(anr_volume_render_lit(fake_f, fake_f, 7, 5, 6, fake_c, 3, 16, 24, &p, fake_f, 0) ==
          ANR_E_INVALID);
    CHECK(says("anr_volume_render_lit") && says(b.word));
    CHECK(anr_sparse_volume_light(&v, 1, &p, fake_f, 0) == ANR_E_INVALID);
    CHECK(says("anr_sparse_volume_light") && says(b.word));
    CHECK(anr_sparse_volume_render_lit(&v, fake_f, 1, fake_c, 3, 16, 24, &p, fake_f, 0, 0) ==
          ANR_E_INVALID);
    CHECK(says("anr_sparse_volume_render_lit") && says(b.word));
  }
  for (const auto& s : shapes) {
    CHECK(anr_sparse_volume_render_lit(&v, fake_f, 1, fake_c, s[0], s[1], s[2], &ok, fake_f, 0,
                                       0) == ANR_E_INVALID);
    CHECK(anr_volume_render_lit(fake_f, fake_f, 7, 5, 6, fake_c, s[0], s[1], s[2], &ok, fake_f,
                                0) == ANR_E_INVALID);
  }
  // a null tau, and every other null pointer
  CHECK(anr_volume_light(fake_f, 7, 5, 6, &ok, 0, 0) == ANR_E_INVALID && says("null pointer"));
  CHECK(anr_volume_light(0, 7, 5, 6, &ok, fake_f, 0) == ANR_E_INVALID && says("null pointer"));
  CHECK(anr_volume_light(fake_f, 7, 5, 6, 0, fake_f, 0) == ANR_E_INVALID && says("params"));
  CHECK(anr_volume_light(fake_f, 7, 0, 6, &ok, fake_f, 0) == ANR_E_INVALID && says("extents"));
  CHECK(anr_volume_light(fake_f, 1024, 1024, 512, &ok, fake_f, 0) == ANR_E_INVALID);
  CHECK(says("anr_volume_light") && says("2^31 bytes"));
  CHECK(anr_volume_render_lit(fake_f, 0, 7, 5, 6, fake_c, 3, 16, 24, &ok, fake_f, 0) ==
        ANR_E_INVALID);
  CHECK(says("anr_volume_render_lit") && says("null pointer"));
  CHECK(anr_volume_render_lit(0, fake_f, 7, 5, 6, fake_c, 3, 16, 24, &ok, fake_f, 0) ==
        ANR_E_INVALID);
  CHECK(anr_volume_render_lit(fake_f, fake_f, 7, 5, 6, 0, 3, 16, 24, &ok, fake_f, 0) ==
        ANR_E_INVALID);
  CHECK(anr_volume_render_lit(fake_f, fake_f, 7, 5, 6, fake_c, 3, 16, 24, &ok, 0, 0) ==
        ANR_E_INVALID);
  CHECK(anr_volume_render_lit(fake_f, fake_f, 7, 5, 6, fake_c, 3, 16, 24, 0, fake_f, 0) ==
        ANR_E_INVALID);
  CHECK(anr_volume_render_lit(fake_f, fake_f, 1024, 1024, 512, fake_c, 3, 16, 24, &ok, fake_f,
                              0) == ANR_E_INVALID);
  CHECK(says("2^31 bytes"));
  CHECK(anr_sparse_volume_light(&v, 1, &ok, 0, 0) == ANR_E_INVALID && says("null pointer"));
  CHECK(anr_sparse_volume_light(0, 1, &ok, fake_f, 0) == ANR_E_INVALID);
  CHECK(anr_sparse_volume_light(&v, 1, 0, fake_f, 0) == ANR_E_INVALID && says("params"));
  CHECK(anr_sparse_volume_light(&v, 2, &ok, fake_f, 0) == ANR_E_INVALID && says("skip"));
  CHECK(anr_sparse_volume_render_lit(&v, 0, 1, fake_c, 3, 16, 24, &ok, fake_f, 0, 0) ==
        ANR_E_INVALID);
  CHECK(says("anr_sparse_volume_render_lit") && says("null pointer"));
  CHECK(anr_sparse_volume_render_lit(0, fake_f, 1, fake_c, 3, 16, 24, &ok, fake_f, 0, 0) ==
        ANR_E_INVALID);
  CHECK(anr_sparse_volume_render_lit(&v, fake_f, -1, fake_c, 3, 16, 24, &ok, fake_f, 0, 0) ==
        ANR_E_INVALID);
  CHECK(says("skip"));
  CHECK(anr_sparse_volume_render_lit(&v, fake_f, 1, 0, 3, 16, 24, &ok, fake_f, 0, 0) ==
        ANR_E_INVALID);
  CHECK(anr_sparse_volume_render_lit(&v, fake_f, 1, fake_c, 3, 16, 24, &ok, 0, 0, 0) ==
        ANR_E_INVALID);
  // no pixels: ANR_OK without a launch, whatever the pointers
  CHECK(anr_volume_render_lit(0, 0, 7, 5, 6, 0, 0, 16, 24, &ok, 0, 0) == ANR_OK);
  CHECK(anr_volume_render_lit(0, 0, 7, 5, 6, 0, 3, 16, 0, &ok, 0, 0) == ANR_OK);
  CHECK(anr_sparse_volume_render_lit(&v, 0, 1, 0, 0, 16, 24, &ok, 0, 0, 0) == ANR_OK);
  CHECK(anr_sparse_volume_render_lit(&v, 0, 1, 0, 3, 0, 24, &ok, 0, 0, 0) == ANR_OK);
  {  // skip = 0 needs no brick level: only the null tau stops the calls
    anr_sparse_volume s = v;
    s.coarse = nullptr;
    CHECK(anr_sparse_volume_light(&s, 0, &ok, 0, 0) == ANR_E_INVALID && says("null pointer"));
    CHECK(anr_sparse_volume_render_lit(&s, 0, 0, fake_c, 3, 16, 24, &ok, fake_f, 0, 0) ==
          ANR_E_INVALID);
    CHECK(says("null pointer"));
  }

  // the build entries
  CHECK(anr_sparse_volume_mark(fake_i, 0, 0, 0, 0, 70, 9, 11, 96, fake_u, fake_u, 0) ==
        ANR_E_INVALID);
  CHECK(says("no voxels"));
  CHECK(anr_sparse_volume_mark(fake_i, -5, 0, 0, 0, 70, 9, 11, 96, fake_u, fake_u, 0) ==
        ANR_E_INVALID);
  CHECK(anr_sparse_volume_mark(fake_i, 1LL << 31, 0, 0, 0, 70, 9, 11, 96, fake_u, fake_u, 0) ==
        ANR_E_INVALID);
  CHECK(anr_sparse_volume_mark(fake_i, 5, 0x7ffffff0, 0, 0, 70, 9, 11, 96, fake_u, fake_u, 0) ==
        ANR_E_INVALID);
  CHECK(says("overflows int32"));
  CHECK(anr_sparse_volume_mark(fake_i, 5, 0, 0, 0, 70, 9, 11, 64, fake_u, fake_u, 0) ==
        ANR_E_INVALID);
  CHECK(anr_sparse_volume_mark(fake_i, 5, 0, 0, 0, 70, 9, 11, 96, fake_u, 0, 0) == ANR_E_INVALID);
  CHECK(anr_sparse_volume_mark(0, 5, 0, 0, 0, 70, 9, 11, 96, fake_u, fake_u, 0) == ANR_E_INVALID);
  CHECK(anr_sparse_volume_popcount(fake_u, 0, fake_i, 0) == ANR_E_INVALID);
  CHECK(anr_sparse_volume_popcount(fake_u, 1LL << 31, fake_i, 0) == ANR_E_INVALID);
  CHECK(anr_sparse_volume_popcount(0, 5, fake_i, 0) == ANR_E_INVALID);
  CHECK(anr_sparse_volume_place(fake_i, fake_f, 0, 1.0, 0, 0, 0, 70, 9, 11, 96, fake_u, 5, fake_f,
                                0) == ANR_E_INVALID);
  CHECK(anr_sparse_volume_place(fake_i, fake_f, 5, NAN, 0, 0, 0, 70, 9, 11, 96, fake_u, 5, fake_f,
                                0) == ANR_E_INVALID);
  CHECK(says("density_scale"));
  CHECK(anr_sparse_volume_place(fake_i, fake_f, 5, 1.0, 0, 0, 0, 70, 9, 11, 96, fake_u, 0, fake_f,
                                0) == ANR_E_INVALID);
  CHECK(anr_sparse_volume_place(fake_i, 0, 5, 1.0, 0, 0, 0, 70, 9, 11, 96, fake_u, 5, fake_f, 0) ==
        ANR_E_INVALID);
  // bricks: (n >> 3) + 1 per axis, 32 to a word; 0 for a box no entry takes
  CHECK(anr_sparse_volume_coarse_words(70, 9, 11) == (9 * 2 * 2 + 31) / 32);
  CHECK(anr_sparse_volume_coarse_words(973, 873, 791) == (122 * 110 * 99 + 31) / 32);
  CHECK(anr_sparse_volume_coarse_words(8, 8, 8) == 1);
  CHECK(anr_sparse_volume_coarse_words(0, 9, 11) == 0);
  CHECK(anr_sparse_volume_coarse_words(0x7fffffff, 0x7fffffff, 0x7fffffff) == 0);
  printf(fails ? "sparse_volume: %d check(s) failed\n" : "sparse_volume: ok\n", fails);
  return fails ? 1 : 0;
}
