// Stand-alone host check of bo_select_batch_bucb's argument validation and workspace carving
// (include/bo_amd.h): every call here returns before the first HIP call, so it needs no device.
// Built with the host sanitizers by scripts/bucb_host_sanitize.sh (CPU only).
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "bo_amd.h"

static int failures = 0;
#define EXPECT(cond)                                                     \
  do {                                                                   \
    if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

static bo_bucb_desc good(void) {
  bo_bucb_desc d;
  memset(&d, 0, sizeof(d));
  d.n_obj = 3; d.dim = 6; d.n_train = 1024; d.ld_k = 1024;
  d.cand_kind = BO_CAND_F64; d.q = 48; d.n_cand = 1 << 21; d.ld = 1 << 21;
  for (int o = 0; o < 3; ++o) { d.prior_var[o] = 2.0; d.length_scale[o] = 40.0; d.beta[o] = 2.0; }
  d.jitter = 1e-6; d.min_variance = 1e-10;
  return d;
}

int main(void) {
  static double dummy[4];
  bo_bucb_desc d = good();
  const size_t base = bo_select_batch_bucb_workspace_size(&d);
  EXPECT(base >= (size_t)3 * (1 << 21) * 8 + (size_t)3 * 48 * 1024 * 8);
  EXPECT(base < (size_t)4 * (1 << 21) * 8 + ((size_t)1 << 24));   // never (q - 1) n_obj n_cand doubles
  d.var_out = dummy;
  EXPECT(bo_select_batch_bucb_workspace_size(&d) + (size_t)3 * (1 << 21) * 8 == base);
  EXPECT(bo_select_batch_bucb_workspace_size(NULL) == 0);
  EXPECT(bo_select_batch_bucb(NULL, NULL, 0, NULL) == BO_ERR_ARG);
  // NULL arrays, then a missing / short workspace
  d = good();
  EXPECT(bo_select_batch_bucb(&d, dummy, base, NULL) == BO_ERR_ARG);
  d.x_train = d.kinv = d.std_mu = d.var = dummy; d.cand = dummy; d.top_val = dummy; d.top_idx = (int64_t*)dummy;
  EXPECT(bo_select_batch_bucb(&d, NULL, 0, NULL) == BO_ERR_WORKSPACE);
  EXPECT(bo_select_batch_bucb(&d, dummy, base - 1, NULL) == BO_ERR_WORKSPACE);
  d.var_out = dummy;                                                 // the input variance as output
  EXPECT(bo_select_batch_bucb(&d, dummy, base, NULL) == BO_ERR_ARG);
  // shapes
  const struct { int field; long long v; } bad[] = {{0, 0}, {0, 9}, {1, 0}, {1, 9}, {2, 0}, {2, 1 << 20}, {3, 1023},
                                                    {4, -1}, {4, 4}, {5, 0}, {5, 49}, {6, 0}, {7, -1}, {8, (1 << 21) - 1}};
  for (unsigned i = 0; i < sizeof(bad) / sizeof(bad[0]); ++i) {
    d = good();
    switch (bad[i].field) {
      case 0: d.n_obj = (int)bad[i].v; break;
      case 1: d.dim = (int)bad[i].v; break;
      case 2: d.n_train = bad[i].v; break;
      case 3: d.ld_k = bad[i].v; break;
      case 4: d.cand_kind = (int)bad[i].v; break;
      case 5: d.q = (int)bad[i].v; break;
      case 6: d.n_cand = bad[i].v; break;
      case 7: d.cand_offset = bad[i].v; break;
      default: d.ld = bad[i].v; break;
    }
    EXPECT(bo_select_batch_bucb_workspace_size(&d) == 0);
    EXPECT(bo_select_batch_bucb(&d, dummy, base, NULL) == BO_ERR_ARG);
  }
  d = good(); d.prior_var[2] = -1.0; EXPECT(bo_select_batch_bucb_workspace_size(&d) == 0);
  d = good(); d.length_scale[0] = NAN; EXPECT(bo_select_batch_bucb_workspace_size(&d) == 0);
  d = good(); d.jitter = INFINITY; EXPECT(bo_select_batch_bucb_workspace_size(&d) == 0);
  d = good(); d.min_variance = NAN; EXPECT(bo_select_batch_bucb_workspace_size(&d) == 0);
  // a grid: the shard must lie inside it, and its extents must not overflow
  d = good(); d.cand_kind = BO_CAND_GRID; d.dim = 2; d.n_cand = d.ld = 1 << 20;
  d.grid_shape[0] = d.grid_shape[1] = 1024;
  EXPECT(bo_select_batch_bucb_workspace_size(&d) > 0);
  d.cand_offset = 1; EXPECT(bo_select_batch_bucb_workspace_size(&d) == 0);
  d.cand_offset = 0; d.grid_shape[1] = 0; EXPECT(bo_select_batch_bucb_workspace_size(&d) == 0);
  d.grid_shape[0] = d.grid_shape[1] = (int64_t)1 << 40; EXPECT(bo_select_batch_bucb_workspace_size(&d) == 0);
  d.grid_shape[0] = d.grid_shape[1] = 1024; d.grid_lo[0] = (int64_t)1 << 60;
  EXPECT(bo_select_batch_bucb_workspace_size(&d) == 0);
  printf(failures ? "bucb host check: %d FAILED\n" : "bucb host check: ok\n", failures);
  return failures ? 1 : 0;
}
