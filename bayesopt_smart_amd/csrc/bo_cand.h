// The candidates of one shard: "coordinate k of local candidate j" for every kind (bo_cand_kind),
// on the host (the checks and the packing of the description) and on the device (the decode).
// One copy, used by bo_select.hip, bo_bucb_impl.h (bo_bucb.hip, bo_kb.hip) and bo_ts.hip: what
// they compute for a point does not depend on the kind it is given in, nor on the shard.  The
// fused predict keeps its own load_candidate<DIM> (bo_predict_impl.h, tuned to its registers):
// the same decode.  No pragma here changes the floating-point contraction of an includer.
#pragma once

#include "bo_common.h"

// What a caller passes (a descriptor's fields, or an entry point's arguments); host only.
struct CandDesc {
  int kind;                      // bo_cand_kind
  const void* cand;              // device rows (I64 / F64), host bo_sobol_desc* (SOBOL), unused (GRID)
  const int64_t* grid_lo;        // kind GRID: [dim]
  const int64_t* grid_shape;
  int dim;
  long long offset, count;       // global index of local candidate 0; candidates of the shard
};

template <class D>
CandDesc bo_cand_desc(const D* d) {
  return CandDesc{d->cand_kind, d->cand, d->grid_lo, d->grid_shape, d->dim, d->cand_offset, d->n_cand};
}

// What a kernel needs to decode the shard.  The order of the fields is measured, not free: the
// posterior draws' path kernel at 8 dimensions sits at the SGPR limit, and with the counts ahead of
// the grid arrays its kernel-argument loads spill scalar registers.
struct CandArgs {
  int kind, dim;
  int idx32;                     // grid: every global index and every axis below 2^31 (32-bit decode)
  long long grid_lo[BO_MAX_DIM], grid_shape[BO_MAX_DIM];   // axes >= dim: shape 1
  long long n_cand, cand_offset;
  const void* rows;              // [n_cand][dim] int64 / f64 of the explicit kinds, else NULL
  SobolArgs sob;                 // kind BO_CAND_SOBOL
};

// The kind's range and, for a grid, the limits under which the decode is exact: every coordinate
// below 2^53 in magnitude, at most 2^62 points, the shard inside the grid.  (bo_misc.hip)
bool bo_cand_check(const CandDesc& d);
// Packs `d` (dim, offset and count valid; bo_cand_check, or the caller's own rule, passed).
// BO_OK, or bo_sobol_fill's status for a bad Sobol descriptor.  (bo_misc.hip)
int bo_cand_fill(CandArgs* a, const CandDesc& d);

// coordinate k (< dim) of local candidate j of the explicit kinds and the Sobol sequence
__device__ __forceinline__ double bo_cand_coord(const CandArgs& a, long long j, int k) {
  if (a.kind == BO_CAND_I64) return (double)((const long long*)a.rows)[j * a.dim + k];
  if (a.kind == BO_CAND_SOBOL) return bo_sobol_coord(a.sob, k, (unsigned long long)(a.cand_offset + j));
  return ((const double*)a.rows)[j * a.dim + k];
}

// c[k] = coordinate k of local candidate j, k < dim; padded coordinates 0.  CENTRED: minus
// centre[k] (differences of centred coordinates keep full precision for point sets far from the
// origin); otherwise `centre` is not read.  A grid index is taken apart by one chain of
// divisions, last axis fastest.
template <int DIMP, bool CENTRED>
__device__ __forceinline__ void bo_cand_load(const CandArgs& a, const double* centre, long long j,
                                             double (&c)[DIMP]) {
  auto put = [&](int k, double v) {
    if constexpr (CENTRED) v -= centre[k];
    c[k] = v;
  };
#pragma unroll
  for (int k = 0; k < DIMP; ++k) c[k] = 0.0;
  if (a.kind == BO_CAND_GRID) {
    if (a.idx32) {                       // 32-bit divisions (the 64-bit ones are ~10x longer)
      unsigned int gi = (unsigned int)(a.cand_offset + j);
#pragma unroll
      for (int k = DIMP - 1; k >= 0; --k) {
        if (k < a.dim) {
          const unsigned int n = (unsigned int)a.grid_shape[k];
          const unsigned int qq = gi / n;
          put(k, (double)(a.grid_lo[k] + (long long)(gi - qq * n)));
          gi = qq;
        }
      }
      return;
    }
    long long gi = a.cand_offset + j;
#pragma unroll
    for (int k = DIMP - 1; k >= 0; --k) {
      if (k < a.dim) {
        const long long n = a.grid_shape[k];
        const long long qq = gi / n;
        put(k, (double)(a.grid_lo[k] + (gi - qq * n)));
        gi = qq;
      }
    }
    return;
  }
#pragma unroll
  for (int k = 0; k < DIMP; ++k)
    if (k < a.dim) put(k, bo_cand_coord(a, j, k));
}
