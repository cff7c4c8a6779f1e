// Stand-alone host check of the EHVI's host side (include/bo_amd.h): bo_hvi_boxes -> bo_ehvi_tables
// on empty fronts, fronts with ties, duplicates, NaN rows and points below the reference point, and
// capacities one short of the need; then the argument checks of bo_expected_hypervolume_improvement
// that return before the first HIP call.  Needs no device.  Built with the host sanitizers by
// scripts/ehvi_host_sanitize.sh (CPU only).
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "bo_amd.h"

static int failures = 0;
#define EXPECT(cond)                                                     \
  do {                                                                   \
    if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

// boxes of `front` ([n][m]) above `ref`, then their tables; every bound must come back through its
// index, the edges strictly increasing; both calls also with one element too few.
static void check_front(const std::vector<double>& front, int m, const double* ref) {
  const int64_t n = (int64_t)front.size() / m;
  int64_t nb = 0;
  EXPECT(bo_hvi_boxes(front.data(), n, m, ref, NULL, 0, &nb) == BO_ERR_WORKSPACE);
  EXPECT(nb >= 1);
  std::vector<double> boxes((size_t)nb * 2 * m);           // exactly the need: one more write is an overflow
  int64_t nb2 = 0;
  if (nb > 1) {
    EXPECT(bo_hvi_boxes(front.data(), n, m, ref, boxes.data(), nb - 1, &nb2) == BO_ERR_WORKSPACE && nb2 == nb);
  }
  EXPECT(bo_hvi_boxes(front.data(), n, m, ref, boxes.data(), nb, &nb2) == BO_OK && nb2 == nb);
  int32_t ne[4] = {-1, -1, -1, -1};
  EXPECT(bo_ehvi_tables(boxes.data(), nb, m, NULL, 0, ne, NULL) == BO_ERR_WORKSPACE);
  int64_t total = 0;
  for (int k = 0; k < m; ++k) { EXPECT(ne[k] >= 1); total += ne[k]; }
  std::vector<double> edges((size_t)total);
  std::vector<int32_t> idx((size_t)nb * 2 * m, -5);
  int32_t ne2[4] = {0, 0, 0, 0};
  EXPECT(bo_ehvi_tables(boxes.data(), nb, m, edges.data(), total - 1, ne2, idx.data()) == BO_ERR_WORKSPACE);
  EXPECT(idx[0] == -5 && memcmp(ne, ne2, sizeof(int32_t) * m) == 0);
  EXPECT(bo_ehvi_tables(boxes.data(), nb, m, edges.data(), total, ne2, NULL) == BO_ERR_WORKSPACE);
  EXPECT(bo_ehvi_tables(boxes.data(), nb, m, edges.data(), total, ne2, idx.data()) == BO_OK);
  int64_t off = 0;
  for (int k = 0; k < m; ++k) {
    for (int j = 1; j < ne[k]; ++j) EXPECT(edges[off + j - 1] < edges[off + j]);
    for (int64_t b = 0; b < nb; ++b)
      for (int side = 0; side < 2; ++side) {
        const int32_t i = idx[b * 2 * m + side * m + k];
        const double v = boxes[b * 2 * m + side * m + k];
        EXPECT(i >= 0 && i <= ne[k] && (side == 1 || i < ne[k]));
        if (i >= 0 && i < ne[k]) EXPECT(edges[off + i] == v);
        else EXPECT(isinf(v) && v > 0);
      }
    off += ne[k];
  }
  if (n == 0) {
    EXPECT(nb == 1);
    for (int k = 0; k < m; ++k) EXPECT(ne[k] == 1 && edges[k] == ref[k]);
  }
}

int main(void) {
  const double ref[4] = {-1.0, -1.0, -1.0, -1.0};
  for (int m = 1; m <= 4; ++m) {
    check_front({}, m, ref);                                // empty front: one box, E_k = 1
    // ties, duplicates, a NaN row, a row below the reference point, a row on it
    std::vector<double> f;
    const double rows[][4] = {{2, 3, 1, 2}, {2, 3, 1, 2}, {3, 2, 1, 0}, {3, 1, 4, 0}, {NAN, 1, 1, 1},
                              {-2, 5, 5, 5}, {-1, 4, 4, 4}, {1, 3, 2, 2}, {0, 0, 5, 1}, {2, 2, 2, 2}};
    for (const auto& r : rows) f.insert(f.end(), r, r + m);
    check_front(f, m, ref);
    // a front the reference point dominates entirely: the empty front's single box
    std::vector<double> below;
    for (int i = 0; i < 3; ++i)
      for (int k = 0; k < m; ++k) below.push_back(-2.0 - i);
    check_front(below, m, ref);
  }
  // bo_ehvi_tables' own argument checks
  double box2[4] = {0.0, 0.0, INFINITY, INFINITY}, e[8];
  int32_t ne[4], idx[4];
  EXPECT(bo_ehvi_tables(box2, 1, 2, e, 8, NULL, idx) == BO_ERR_ARG);
  EXPECT(bo_ehvi_tables(NULL, 1, 2, e, 8, ne, idx) == BO_ERR_ARG);
  EXPECT(bo_ehvi_tables(box2, -1, 2, e, 8, ne, idx) == BO_ERR_ARG);
  EXPECT(bo_ehvi_tables(box2, 1, 0, e, 8, ne, idx) == BO_ERR_ARG);
  EXPECT(bo_ehvi_tables(box2, 1, 5, e, 8, ne, idx) == BO_ERR_ARG);
  EXPECT(bo_ehvi_tables(box2, 1, 2, NULL, 8, ne, idx) == BO_ERR_ARG);
  EXPECT(bo_ehvi_tables(box2, 1, 2, e, -1, ne, idx) == BO_ERR_ARG);
  EXPECT(bo_ehvi_tables(box2, 1, 2, e, 8, ne, idx) == BO_OK && ne[0] == 1 && ne[1] == 1 && idx[2] == 1);
  EXPECT(bo_ehvi_tables(NULL, 0, 2, NULL, 0, ne, NULL) == BO_OK && ne[0] == 0 && ne[1] == 0);
  box2[1] = NAN;       EXPECT(bo_ehvi_tables(box2, 1, 2, e, 8, ne, idx) == BO_ERR_ARG);
  box2[1] = INFINITY;  EXPECT(bo_ehvi_tables(box2, 1, 2, e, 8, ne, idx) == BO_ERR_ARG);
  box2[1] = 0.0; box2[2] = -INFINITY; EXPECT(bo_ehvi_tables(box2, 1, 2, e, 8, ne, idx) == BO_ERR_ARG);
  // the admission rule
  EXPECT(bo_ehvi_table_threads(0) == 256 && bo_ehvi_table_threads(80) == 256 && bo_ehvi_table_threads(81) == 128);
  EXPECT(bo_ehvi_table_threads(160) == 128 && bo_ehvi_table_threads(161) == 64);
  EXPECT(bo_ehvi_table_threads(320) == 64 && bo_ehvi_table_threads(321) == 0 && bo_ehvi_table_threads(-1) == 0);
  EXPECT(bo_ehvi_table_threads((int64_t)1 << 62) == 0);
  // bo_expected_hypervolume_improvement: everything that returns before the first HIP call
  static double d[4];
  static int32_t di[4];
  int32_t small[2] = {3, 3}, big[2] = {200, 121}, neg[2] = {3, -1}, zero[2] = {3, 0};
  EXPECT(bo_expected_hypervolume_improvement(NULL, d, d, 4, 2, 2, d, 1, d, small, di, 0, NULL) == BO_ERR_ARG);
  EXPECT(bo_expected_hypervolume_improvement(d, NULL, d, 4, 2, 2, d, 1, d, small, di, 0, NULL) == BO_ERR_ARG);
  EXPECT(bo_expected_hypervolume_improvement(d, d, NULL, 4, 2, 2, d, 1, d, small, di, 0, NULL) == BO_ERR_ARG);
  EXPECT(bo_expected_hypervolume_improvement(d, d, d, 1, 2, 2, d, 1, d, small, di, 0, NULL) == BO_ERR_ARG);
  EXPECT(bo_expected_hypervolume_improvement(d, d, d, 4, -1, 2, d, 1, d, small, di, 0, NULL) == BO_ERR_ARG);
  EXPECT(bo_expected_hypervolume_improvement(d, d, d, 4, 2, 0, d, 1, d, small, di, 0, NULL) == BO_ERR_ARG);
  EXPECT(bo_expected_hypervolume_improvement(d, d, d, 4, 2, 5, d, 1, d, small, di, 0, NULL) == BO_ERR_ARG);
  EXPECT(bo_expected_hypervolume_improvement(d, d, d, 4, 2, 2, d, -1, d, small, di, 0, NULL) == BO_ERR_ARG);
  EXPECT(bo_expected_hypervolume_improvement(d, d, d, 4, 2, 2, d, 1, d, small, di, -1, NULL) == BO_ERR_ARG);
  EXPECT(bo_expected_hypervolume_improvement(d, d, d, 4, 2, 2, d, 1, d, small, di, 3, NULL) == BO_ERR_ARG);
  EXPECT(bo_expected_hypervolume_improvement(d, d, d, 4, 2, 2, NULL, 1, d, small, di, 1, NULL) == BO_ERR_ARG);
  EXPECT(bo_expected_hypervolume_improvement(d, d, d, 4, 2, 2, d, 1, NULL, small, di, 2, NULL) == BO_ERR_ARG);
  EXPECT(bo_expected_hypervolume_improvement(d, d, d, 4, 2, 2, d, 1, d, NULL, di, 2, NULL) == BO_ERR_ARG);
  EXPECT(bo_expected_hypervolume_improvement(d, d, d, 4, 2, 2, d, 1, d, small, NULL, 2, NULL) == BO_ERR_ARG);
  EXPECT(bo_expected_hypervolume_improvement(d, d, d, 4, 2, 2, NULL, 1, NULL, NULL, NULL, 0, NULL) == BO_ERR_ARG);
  EXPECT(bo_expected_hypervolume_improvement(d, d, d, 4, 2, 2, d, 1, d, neg, di, 0, NULL) == BO_ERR_ARG);
  EXPECT(bo_expected_hypervolume_improvement(d, d, d, 4, 2, 2, d, 1, d, zero, di, 2, NULL) == BO_ERR_ARG);
  EXPECT(bo_expected_hypervolume_improvement(d, d, d, 4, 2, 2, d, 1, d, big, di, 2, NULL) == BO_ERR_UNSUPPORTED);
  EXPECT(bo_expected_hypervolume_improvement(d, d, d, 4, 2, 2, NULL, 1, d, big, di, 0, NULL) == BO_ERR_UNSUPPORTED);
  EXPECT(bo_expected_hypervolume_improvement(d, d, d, ((int64_t)1 << 36) + 1, ((int64_t)1 << 36) + 1, 2, d, 1, d,
                                             small, di, 0, NULL) == BO_ERR_UNSUPPORTED);
  // n = 0: nothing to do, in every form
  for (int form = 0; form <= 2; ++form)
    EXPECT(bo_expected_hypervolume_improvement(d, d, d, 0, 0, 2, d, 1, d, small, di, form, NULL) == BO_OK);
  printf(failures ? "ehvi host check: %d FAILED\n" : "ehvi host check: ok\n", failures);
  return failures ? 1 : 0;
}
