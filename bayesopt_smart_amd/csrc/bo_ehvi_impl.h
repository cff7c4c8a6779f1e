// The per-candidate arithmetic of the expected hypervolume improvement (bo_ehvi.hip states the
// closed form and the two forms), shared by the translation units that scan it: bo_ehvi.hip (the
// plain scan) and bo_kb.hip (the scan that selects while it integrates).  One psi, one box order,
// one rule for the form: every scan built from these functions gives the same bits.  Every
// includer compiles its own copy (anonymous namespace).
#pragma once

#include "bo_common.h"

#include <math.h>
#include <string.h>

// every scan must round alike: no contraction but the fma written out below.  The pragma holds to
// the end of the including translation unit: headers that rely on the default contraction
// (bo_bucb_impl.h) are included before this one.
#pragma clang fp contract(off)

namespace {

constexpr int kEhviLdsBytes = 160 * 1024;      // LDS of a CU: one workgroup may hold all of it
constexpr int kEhviAuto2dEdges = 40;           // auto, 2 objectives: two 256-thread tables per CU

struct EhviArgs {
  double* acq;
  const double* mu;
  const double* var;
  long long ld, n;
  const double* boxes;     // direct: [n_boxes][2 m] (bo_hvi_boxes)
  const double* edges;     // table: the axes' edges, concatenated
  const int* box_idx;      // table: [n_boxes][2 m] indices into the axis' edges; E_k = +inf
  long long n_boxes;
  int n_edges[4], edge_off[4];
};

// sigma h(t), t = |d| rs with rs = 1 / sigma.  sigma = 0 gives t = inf (or NaN at d = 0) and the
// limit 0; h underflows to 0 well before t = 40.
__device__ __forceinline__ double ehvi_psi(double d, double sigma, double rs) {
  const double t = fabs(d * rs);
  double h = 0.0;
  if (t < 40.0) {
    const double e = exp(-0.5 * (t * t));
    h = e * (0.3989422804014327 - (0.5 * t) * erfcx(t * 0.7071067811865476));
  }
  return __builtin_fma(sigma, h, fmax(d, 0.0));
}

// What the constrained scan reads besides EhviArgs (include/bo_amd.h, bo_constrained_ehvi): the
// constraint outputs are the rows [n_obj, n_obj + n_con) of e.mu / e.var.
struct EhviConArgs {
  EhviArgs e;
  double* pof;             // optional [n]: P, the product of the constraints' probabilities
  int n_obj, n_con;
  double lo[BO_MAX_OBJ - 1], hi[BO_MAX_OBJ - 1];
};

// The upper tail Q(z) = 1 - Phi(z) = erfc(z / sqrt 2) / 2: positive, and relatively accurate, for
// every z (0 past z = 38.6, 1 at z = -inf).
__device__ __forceinline__ double ehvi_tail(double z) { return 0.5 * erfc(z * 0.7071067811865476); }

// P(lo <= Y <= hi), Y ~ N(mu, sigma^2), lo <= hi, either infinite on its own side, as a difference
// of positive tail terms, so that the result keeps its relative accuracy in both tails:
//   za = (lo - mu) / sigma, zb = (hi - mu) / sigma
//   za > 0:  Q(za) - Q(zb)      zb < 0:  Q(-zb) - Q(-za)      else:  (1 - Q(zb)) - Q(-za)
// sigma = 0 gives 1 inside [lo, hi] (the bounds included), else 0; (-inf, +inf) gives exactly 1;
// NaN in mu or sigma gives NaN.
__device__ __forceinline__ double ehvi_pof(double mu, double sigma, double lo, double hi) {
  if (mu != mu || sigma != sigma) return __builtin_nan("");
  if (sigma == 0.0) return (lo <= mu && mu <= hi) ? 1.0 : 0.0;
  const double za = (lo - mu) / sigma, zb = (hi - mu) / sigma;
  // the three cases share two tail evaluations: Q(t1) - Q(t2), or (1 - Q(t1)) - Q(t2)
  const bool above = za > 0.0, below = !above && zb < 0.0;
  const double q1 = ehvi_tail(above ? za : (below ? -zb : zb));
  const double q2 = ehvi_tail(above ? zb : -za);
  return ((above || below) ? q1 : 1.0 - q1) - q2;
}

// P = ((P_0 P_1) P_2) ... of candidate i, left to right; 1 without constraints.  The same
// non-temporal loads as ehvi_load's; a lane past the end computes on mu = 0, var = 1.
__device__ __forceinline__ double ehvi_pof_product(const EhviConArgs& c, long long i, bool valid) {
  double p = 1.0;
  for (int j = 0; j < c.n_con; ++j) {
    const long long row = (long long)(c.n_obj + j) * c.e.ld + i;
    const double mu = valid ? __builtin_nontemporal_load(c.e.mu + row) : 0.0;
    const double v = valid ? __builtin_nontemporal_load(c.e.var + row) : 1.0;
    const double pj = ehvi_pof(mu, sqrt(fabs(v)), c.lo[j], c.hi[j]);
    p = j == 0 ? pj : p * pj;
  }
  return p;
}

// The argument of a scan kernel: EhviArgs for the plain instantiation, EhviConArgs for the
// constrained one.  ehvi_finish turns the box sum h into the value stored: the plain scan's h, or
// fl(h P) with P stored where asked for.
template <bool CON> struct EhviScan { typedef EhviArgs Args; };
template <> struct EhviScan<true> { typedef EhviConArgs Args; };

__host__ __device__ __forceinline__ const EhviArgs& ehvi_base(const EhviArgs& a) { return a; }
__host__ __device__ __forceinline__ const EhviArgs& ehvi_base(const EhviConArgs& a) { return a.e; }

__device__ __forceinline__ double ehvi_finish(const EhviArgs&, long long, bool, double h) { return h; }
__device__ __forceinline__ double ehvi_finish(const EhviConArgs& c, long long i, bool valid, double h) {
  const double p = ehvi_pof_product(c, i, valid);
  if (valid && c.pof) bo_out_store(c.pof + i, p);
  return h * p;
}

template <int M>
__device__ __forceinline__ bool ehvi_load(const EhviArgs& a, long long i, bool valid, double* mu, double* sg,
                                          double* rs) {
  bool nan = false;
#pragma unroll
  for (int k = 0; k < M; ++k) {
    mu[k] = valid ? __builtin_nontemporal_load(a.mu + (long long)k * a.ld + i) : 0.0;
    const double v = valid ? __builtin_nontemporal_load(a.var + (long long)k * a.ld + i) : 1.0;
    nan = nan || (mu[k] != mu[k]) || (v != v);
    sg[k] = sqrt(fabs(v));
    rs[k] = 1.0 / sg[k];
  }
  return nan;
}

// Direct form, one candidate: psi at every bound of every box.  No store precedes the loads of
// the boxes, which are then scalar loads at a wave-uniform address, in order.
template <int M>
__device__ __forceinline__ double ehvi_direct_value(const EhviArgs& a, const double* mu, const double* sg,
                                                    const double* rs) {
  const double inf = __builtin_inf();
  double h = 0.0;
  const double* b = a.boxes;
  for (long long t = 0; t < a.n_boxes; ++t, b += 2 * M) {
    double v = 1.0;
#pragma unroll
    for (int k = 0; k < M; ++k) {
      const double pl = ehvi_psi(mu[k] - b[k], sg[k], rs[k]);
      const double pu = b[M + k] < inf ? ehvi_psi(mu[k] - b[M + k], sg[k], rs[k]) : 0.0;
      if (k < M - 1) v *= pl - pu;
      else h = __builtin_fma(v, pl - pu, h);
    }
  }
  return h;
}

// Table form, one candidate of a workgroup of T threads: psi_k at every edge into the thread's
// column `col` of the LDS table [sum E][T], then the box walk over that column.  A thread reads
// only the column it wrote, so there is no barrier.
template <int M, int T>
__device__ __forceinline__ double ehvi_table_value(const EhviArgs& a, double* col, const double* mu,
                                                   const double* sg, const double* rs) {
#pragma unroll
  for (int k = 0; k < M; ++k) {
    const double* e = a.edges + a.edge_off[k];
    double* c = col + a.edge_off[k] * T;
#pragma unroll 2
    for (int j = 0; j < a.n_edges[k]; ++j) c[j * T] = ehvi_psi(mu[k] - e[j], sg[k], rs[k]);
  }
  double h = 0.0;
  const int* b = a.box_idx;
  for (long long t = 0; t < a.n_boxes; ++t, b += 2 * M) {
    double v = 1.0;
#pragma unroll
    for (int k = 0; k < M; ++k) {
      const double pl = col[(a.edge_off[k] + b[k]) * T];
      const double pu = b[M + k] < a.n_edges[k] ? col[(a.edge_off[k] + b[M + k]) * T] : 0.0;
      if (k < M - 1) v *= pl - pu;
      else h = __builtin_fma(v, pl - pu, h);
    }
  }
  return h;
}

long long ehvi_blocks(long long n, int threads) { return (n + threads - 1) / threads; }

// The form of one scan (include/bo_amd.h states the admission rule and auto's rule; measured:
// profiles/ehvi_c3.jsonl).  Fills a->n_edges / a->edge_off from n_edges (host) and
// sets *sum_edges, *threads (the table form's workgroup, 0 when no table fits) and *table.
// BO_OK, or the status bo_expected_hypervolume_improvement returns for these arguments.
int ehvi_plan(int form, int n_obj, long long n_boxes, bool have_boxes, bool have_tables, const int32_t* n_edges,
              EhviArgs* a, int* sum_edges, int* threads, bool* table) {
  int64_t sum_e = 0;
  if (have_tables)
    for (int k = 0; k < n_obj; ++k) {
      if (n_edges[k] < 0 || (n_boxes > 0 && n_edges[k] < 1)) return BO_ERR_ARG;
      a->n_edges[k] = n_edges[k];
      a->edge_off[k] = (int)sum_e;
      sum_e += n_edges[k];
      if (sum_e > ((int64_t)1 << 20)) return BO_ERR_UNSUPPORTED;
    }
  *threads = have_tables ? bo_ehvi_table_threads(sum_e) : 0;
  if (form == 2 && *threads == 0) return BO_ERR_UNSUPPORTED;
  *table = form == 2 || (form == 0 && *threads != 0 && n_boxes > 0 &&
                         (!have_boxes || n_obj >= 3 || (n_obj == 2 && sum_e <= kEhviAuto2dEdges)));
  if (!*table && !have_boxes) return BO_ERR_UNSUPPORTED;     // auto, tables only, and they do not fit
  *sum_edges = (int)sum_e;
  return BO_OK;
}

}  // namespace
