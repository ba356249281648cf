// Host-only walk over the fused field's descriptor logic, for a sanitizer build
// (tools/host_check/run.sh: -Xarch_host -fsanitize=address,undefined): which pos / dir
// pairs anr_ingp_field_supported accepts for every number of density outputs S, the packed
// size and the parameter count of each, and the entries that refuse S > 1 before they look
// at a pointer. Nothing here launches a kernel or needs a GPU.
#include <stdio.h>
#include <string.h>

#include "../../include/anr.h"

static anr_mlp_desc desc(int n_in, int n_out, int width, int nh) {
  anr_mlp_desc d;
  memset(&d, 0, sizeof(d));
  d.n_input = n_in;
  d.n_input_padded = (n_in + 15) / 16 * 16;
  d.n_output = n_out;
  d.n_output_padded = 16;
  d.width = width;
  d.n_hidden_layers = nh;
  d.activation = ANR_ACT_RELU;
  d.output_activation = ANR_ACT_NONE;
  return d;
}

static int fails = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);   \
      ++fails;                                                \
    }                                                         \
  } while (0)

int main() {
  const int widths[2] = {32, 64};
  for (int wi = 0; wi < 2; ++wi)
    for (int nh = 1; nh <= 3; ++nh) {
      const int W = widths[wi];
      const anr_mlp_desc pos = desc(32, 16, W, 1);
      const anr_mlp_desc one = desc(19, 4, W, nh);
      for (int n_in = 12; n_in <= 24; ++n_in) {
        const anr_mlp_desc dir = desc(n_in, 4, W, nh);
        const int S = 20 - n_in;
        const int want = nh <= 2 && S >= 1 && S <= 4;
        CHECK(anr_ingp_field_supported(&pos, &dir) == want);
        const int64_t np = anr_mlp_n_params(&dir);
        CHECK(np == (int64_t)dir.n_input_padded * W + (int64_t)(nh - 1) * W * W + 16 * W);
        const int64_t packed = anr_ingp_field_packed_size(&pos, &dir);
        CHECK(want ? packed > 0 && packed == anr_ingp_field_packed_size(&pos, &one)
                   : packed == 0);
        if (!want) continue;
        CHECK(dir.n_input_padded == (S == 4 ? 16 : 32));
        // empty launches are fine everywhere
        CHECK(anr_ingp_field_fwd(&pos, &dir, ANR_F16, 0, 0, 32, 0, 1, 0, 0, 0, 4, 0) == ANR_OK);
        CHECK(anr_ingp_field_density(&pos, &dir, ANR_F16, 0, 0, 32, 0, 0, 0) == ANR_OK);
        CHECK(anr_ingp_field_bwd(&pos, &dir, ANR_F16, 0, 0, 32, 0, 1, 0, 0, 0, 4, 0, 32, 0, 0, 0,
                                 0, 0) == ANR_OK);
        // the entries that stay at one density output
        const int r = S > 1 ? ANR_E_UNSUPPORTED : ANR_E_INVALID;
        CHECK(anr_ingp_field_fwd_h(&pos, &dir, ANR_F16, 0, 0, 32, 0, 1, 10, 0, 0, 4, 0) == r);
        CHECK(anr_ingp_field_fwd_rows(&pos, &dir, ANR_F16, 0, 0, 32, 0, 1, 10, 0, 0, 0, 4, 0) == r);
        CHECK(anr_ingp_field_bwd_rows(&pos, &dir, ANR_F16, 0, 0, 32, 0, 1, 10, 0, 0, 0, 4, 0, 32,
                                      0, 0, 0, 0, 0) == r);
        CHECK(anr_ingp_field_bwd_ref16(&pos, &dir, 0, 0, 32, 0, 1, 10, 0, 0, 4, 0, 32, 0, 0,
                                       128.0f, 0) == r);
        CHECK(anr_ingp_field_bwd_ref16_rows(&pos, &dir, 0, 0, 32, 0, 1, 10, 0, 0, 4, 0, 32, 0, 0,
                                            128.0f, 0, 0, 0, 0) == r);
        // a descriptor with another padding is not tcnn's layout
        anr_mlp_desc bad = dir;
        bad.n_input_padded = dir.n_input_padded == 16 ? 32 : 48;
        CHECK(anr_ingp_field_supported(&pos, &bad) == 0);
      }
    }
  CHECK(anr_ingp_field_supported(0, 0) == 0);
  printf(fails ? "field_variants: %d check(s) failed\n" : "field_variants: ok\n", fails);
  return fails ? 1 : 0;
}
