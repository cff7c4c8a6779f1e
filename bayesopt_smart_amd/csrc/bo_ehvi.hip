// Expected hypervolume improvement (EHVI) of each candidate's posterior over the Pareto front of
// the evaluated points (maximisation, reference point r).  NOT in the reference, which has no
// EHVI: parity is unpinned by it (tests/ehvi_ref.py is the independent statement).
//
// With independent objectives Y_k ~ N(mu_k, sigma_k^2) (the reference's model: one GP per
// objective) and the disjoint boxes [l_b, u_b) of bo_hvi_boxes, the expectation of the box sum
// hvi_exact_kernel evaluates (bo_hvi.hip) has the closed form
//
//   EHVI = sum_b prod_k [ psi_k(l_bk) - psi_k(u_bk) ]
//   psi_k(a) = E[(Y_k - a)+] = sigma_k (phi(z) + z Phi(z)),  z = (mu_k - a) / sigma_k,  psi_k(+inf) = 0
//
// because E[max(0, min(Y, u) - l)] = psi(l) - psi(u) and the objectives are independent.
//
// Two forms, one psi, one box order, the same arithmetic per box (results equal bit for bit):
//   direct: psi at every bound of every box (2 m per box, the +inf bounds skipped), boxes read at
//           wave-uniform addresses;
//   table:  the boxes' bounds are copies of few edge coordinates (bo_ehvi_tables: per axis the
//           sorted unique finite bounds, E_k of them), so a thread evaluates psi_k at every edge
//           once into its own column of an LDS table [edge][thread] and the box sum is then
//           multiplies and adds over that column.
//
// psi is evaluated as  max(d, 0) + sigma h(|z|),  d = mu - a,  h(t) = phi(t) - t Phi(-t)
//                      = exp(-t^2/2) (1/sqrt(2 pi) - t erfcx(t / sqrt 2) / 2):
// phi + z Phi itself cancels for z < 0, and the linear part max(d, 0) is exact here.
// psi, the two box walks and the rule for the form live in bo_ehvi_impl.h, which bo_kb.hip
// includes as well.
//
// Outcome constraints (bo_constrained_ehvi; include/bo_amd.h states the quantity, its limits and
// its rounding rule): the same two kernels with a compile-time flag.  The constrained
// instantiations take EhviConArgs and multiply the box sum by P = prod_j P(lo_j <= Y_j <= hi_j) of
// the constraint rows (ehvi_pof, ehvi_finish in bo_ehvi_impl.h); the plain ones are unchanged.

#include "bo_ehvi_impl.h"

#include <algorithm>
#include <cmath>
#include <type_traits>
#include <vector>

namespace {

// One thread per candidate, one candidate per thread.  CON: the constrained scan (EhviConArgs),
// which multiplies the box sum by the probability of feasibility (ehvi_finish).
template <int M, bool CON>
__global__ __launch_bounds__(256) void ehvi_direct_kernel(const typename EhviScan<CON>::Args ca) {
  const EhviArgs& a = ehvi_base(ca);
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool valid = i < a.n;
  double mu[M], sg[M], rs[M];
  const bool nan = ehvi_load<M>(a, i, valid, mu, sg, rs);
  const double h = ehvi_finish(ca, i, valid, ehvi_direct_value<M>(a, mu, sg, rs));
  if (valid) bo_out_store(a.acq + i, nan ? __builtin_nan("") : h);
}

// One thread per candidate, one candidate per thread; T threads per workgroup; the table
// [sum E][T] in dynamic LDS (objective edges only, with or without constraints).
template <int M, int T, bool CON>
__global__ __launch_bounds__(T) void ehvi_table_kernel(const typename EhviScan<CON>::Args ca) {
  extern __shared__ double ehvi_tab[];
  const EhviArgs& a = ehvi_base(ca);
  const long long i = (long long)blockIdx.x * T + threadIdx.x;
  const bool valid = i < a.n;
  double mu[M], sg[M], rs[M];
  const bool nan = ehvi_load<M>(a, i, valid, mu, sg, rs);
  const double h = ehvi_finish(ca, i, valid, ehvi_table_value<M, T>(a, ehvi_tab + threadIdx.x, mu, sg, rs));
  if (valid) bo_out_store(a.acq + i, nan ? __builtin_nan("") : h);
}

template <class A>
int launch_direct(const A& ca, int m, hipStream_t s) {
  constexpr bool C = std::is_same<A, EhviConArgs>::value;
  const dim3 g((unsigned)ehvi_blocks(ehvi_base(ca).n, 256));
  switch (m) {
    case 1: hipLaunchKernelGGL((ehvi_direct_kernel<1, C>), g, dim3(256), 0, s, ca); break;
    case 2: hipLaunchKernelGGL((ehvi_direct_kernel<2, C>), g, dim3(256), 0, s, ca); break;
    case 3: hipLaunchKernelGGL((ehvi_direct_kernel<3, C>), g, dim3(256), 0, s, ca); break;
    case 4: hipLaunchKernelGGL((ehvi_direct_kernel<4, C>), g, dim3(256), 0, s, ca); break;
    default: return BO_ERR_UNSUPPORTED;
  }
  BO_CHECK_HIP(hipGetLastError());
  return BO_OK;
}

template <int M, int T, class A>
int launch_table_mt(const A& ca, int sum_e, hipStream_t s) {
  constexpr bool C = std::is_same<A, EhviConArgs>::value;
  const size_t lds = (size_t)sum_e * T * sizeof(double);
  if (lds > 64 * 1024)
    BO_CHECK_HIP(hipFuncSetAttribute((const void*)ehvi_table_kernel<M, T, C>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((ehvi_table_kernel<M, T, C>), dim3((unsigned)ehvi_blocks(ehvi_base(ca).n, T)), dim3(T),
                     lds, s, ca);
  BO_CHECK_HIP(hipGetLastError());
  return BO_OK;
}

template <int M, class A>
int launch_table_m(const A& ca, int sum_e, int threads, hipStream_t s) {
  switch (threads) {
    case 256: return launch_table_mt<M, 256>(ca, sum_e, s);
    case 128: return launch_table_mt<M, 128>(ca, sum_e, s);
    case 64: return launch_table_mt<M, 64>(ca, sum_e, s);
    default: return BO_ERR_UNSUPPORTED;
  }
}

template <class A>
int launch_table(const A& ca, int m, int sum_e, int threads, hipStream_t s) {
  switch (m) {
    case 1: return launch_table_m<1>(ca, sum_e, threads, s);
    case 2: return launch_table_m<2>(ca, sum_e, threads, s);
    case 3: return launch_table_m<3>(ca, sum_e, threads, s);
    case 4: return launch_table_m<4>(ca, sum_e, threads, s);
    default: return BO_ERR_UNSUPPORTED;
  }
}

// The scan behind both entry points: the checks the two share, the plan, the launch.  `con` null:
// the plain scan; else con->e is filled here and the constrained instantiation runs.
int ehvi_scan(EhviConArgs* con, double* acq, const double* mu, const double* var, int64_t ld, int64_t n,
              int32_t n_obj, const double* boxes, int64_t n_boxes, const double* edges, const int32_t* n_edges,
              const int32_t* box_idx, int32_t form, void* stream) {
  if (!acq || !mu || !var || n < 0 || ld < n || n_obj < 1 || n_obj > 4 || n_boxes < 0 || form < 0 || form > 2)
    return BO_ERR_ARG;
  if (n > ((int64_t)1 << 36)) return BO_ERR_UNSUPPORTED;     // one thread per candidate: the grid's limit
  const bool have_tables = n_edges && (n_boxes == 0 || (edges && box_idx));
  const bool have_boxes = n_boxes == 0 || boxes;
  if ((form == 1 && !have_boxes) || (form == 2 && !have_tables) || (form == 0 && !have_boxes && !have_tables))
    return BO_ERR_ARG;
  EhviArgs a;
  memset(&a, 0, sizeof(a));
  int sum_e = 0, threads = 0;
  bool table = false;
  const int st = ehvi_plan(form, n_obj, n_boxes, have_boxes, have_tables, n_edges, &a, &sum_e, &threads, &table);
  if (st != BO_OK) return st;
  if (n == 0) return BO_OK;
  a.acq = acq;
  a.mu = mu;
  a.var = var;
  a.ld = ld;
  a.n = n;
  a.boxes = boxes;
  a.edges = edges;
  a.box_idx = box_idx;
  a.n_boxes = n_boxes;
  if (con) {
    con->e = a;
    return table ? launch_table(*con, n_obj, (int)sum_e, threads, (hipStream_t)stream)
                 : launch_direct(*con, n_obj, (hipStream_t)stream);
  }
  return table ? launch_table(a, n_obj, (int)sum_e, threads, (hipStream_t)stream)
               : launch_direct(a, n_obj, (hipStream_t)stream);
}

}  // namespace

extern "C" {

// The table form's admission rule (include/bo_amd.h states it; tests/ehvi_ref.py mirrors it).
int bo_ehvi_table_threads(int64_t sum_edges) {
  if (sum_edges < 0) return 0;
  for (int t = 256; t >= 64; t /= 2)
    if (sum_edges <= kEhviLdsBytes / (t * (int)sizeof(double))) return t;
  return 0;
}

int bo_ehvi_tables(const double* boxes, int64_t n_boxes, int32_t n_obj, double* edges, int64_t edge_capacity,
                   int32_t* n_edges, int32_t* box_idx) {
  if (!n_edges || n_obj < 1 || n_obj > 4 || n_boxes < 0 || n_boxes > ((int64_t)1 << 26) ||
      (n_boxes > 0 && !boxes) || edge_capacity < 0 || (edge_capacity > 0 && !edges))
    return BO_ERR_ARG;
  const int m = n_obj;
  // a lower bound is finite, an upper bound finite or +inf, and neither is NaN
  for (int64_t b = 0; b < n_boxes; ++b)
    for (int k = 0; k < m; ++k) {
      const double lo = boxes[b * 2 * m + k], hi = boxes[b * 2 * m + m + k];
      if (!std::isfinite(lo) || hi != hi || hi == -__builtin_inf()) return BO_ERR_ARG;
    }
  std::vector<std::vector<double>> e(m);
  int64_t total = 0;
  for (int k = 0; k < m; ++k) {
    for (int64_t b = 0; b < n_boxes; ++b) {
      e[k].push_back(boxes[b * 2 * m + k]);
      if (std::isfinite(boxes[b * 2 * m + m + k])) e[k].push_back(boxes[b * 2 * m + m + k]);
    }
    std::sort(e[k].begin(), e[k].end());
    e[k].erase(std::unique(e[k].begin(), e[k].end()), e[k].end());
    n_edges[k] = (int32_t)e[k].size();
    total += (int64_t)e[k].size();
  }
  if (total > edge_capacity || (n_boxes > 0 && !box_idx)) return BO_ERR_WORKSPACE;
  int64_t off = 0;
  for (int k = 0; k < m; ++k) {
    std::copy(e[k].begin(), e[k].end(), edges + off);
    off += (int64_t)e[k].size();
    for (int64_t b = 0; b < n_boxes; ++b)
      for (int side = 0; side < 2; ++side) {
        const double v = boxes[b * 2 * m + side * m + k];
        box_idx[b * 2 * m + side * m + k] =
            std::isfinite(v) ? (int32_t)(std::lower_bound(e[k].begin(), e[k].end(), v) - e[k].begin())
                             : n_edges[k];
      }
  }
  return BO_OK;
}

int bo_expected_hypervolume_improvement(double* acq, const double* mu, const double* var, int64_t ld, int64_t n,
                                        int32_t n_obj, const double* boxes, int64_t n_boxes, const double* edges,
                                        const int32_t* n_edges, const int32_t* box_idx, int32_t form, void* stream) {
  return ehvi_scan(nullptr, acq, mu, var, ld, n, n_obj, boxes, n_boxes, edges, n_edges, box_idx, form, stream);
}

int bo_constrained_ehvi(double* acq, double* pof_out, const double* mu, const double* var, int64_t ld, int64_t n,
                        int32_t n_obj, int32_t n_con, const double* con_lo, const double* con_hi,
                        const double* boxes, int64_t n_boxes, const double* edges, const int32_t* n_edges,
                        const int32_t* box_idx, int32_t form, void* stream) {
  if (n_obj < 1 || n_obj > 4 || n_con < 0 || n_obj + n_con > BO_MAX_OBJ || (n_con > 0 && (!con_lo || !con_hi)))
    return BO_ERR_ARG;
  const double inf = __builtin_inf();
  for (int j = 0; j < n_con; ++j)      // lo <= hi, neither NaN, each infinite on its own side only
    if (!(con_lo[j] <= con_hi[j]) || con_lo[j] == inf || con_hi[j] == -inf) return BO_ERR_ARG;
  if (n_con == 0 && !pof_out)          // the plain scan
    return ehvi_scan(nullptr, acq, mu, var, ld, n, n_obj, boxes, n_boxes, edges, n_edges, box_idx, form, stream);
  EhviConArgs c;
  memset(&c, 0, sizeof(c));
  c.pof = pof_out;
  c.n_obj = n_obj;
  c.n_con = n_con;
  for (int j = 0; j < n_con; ++j) {
    c.lo[j] = con_lo[j];
    c.hi[j] = con_hi[j];
  }
  return ehvi_scan(&c, acq, mu, var, ld, n, n_obj, boxes, n_boxes, edges, n_edges, box_idx, form, stream);
}

}  // extern "C"
