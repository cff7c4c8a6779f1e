// The natural logarithm of the expected hypervolume improvement (acquisition "logehvi";
// include/bo_amd.h, bo_log_ehvi, states the quantity, its limits and its rounding rule).  NOT in the
// reference, which has no EHVI: parity is unpinned by it (tests/logehvi_ref.py is the independent
// statement, in mpmath, and restates this file's arithmetic in f64).
//
// bo_ehvi.hip's scan returns sum_b prod_k [psi_k(l_bk) - psi_k(u_bk)] as one f64: psi is cut off at
// |z| = 40 and products of small factors underflow before that, so a candidate some tens of standard
// deviations under the front gets exactly 0.  Here no transcendental enters the box walk either, but
// every psi is an EXTENDED-RANGE number
//     psi = m 2^e,   m an f64 in [1/4, 1) (or 0: the pair (0, 0)),   e an integer held in an f64
// (an f64 exponent: z = -1e6 needs e = -7.2e11, past an int32; beyond 2^53 every f64 is an integer and
// the lost fraction is a relative error of u in L).  Per bound, once (logehvi_psi):
//   d = mu - a >= 0:  max(d, 0) + sigma h(|z|) in f64, bo_ehvi_impl.h's psi, split by frexp;
//   d < 0, t = |z|:   psi = sigma B(t) exp(-t^2 / 2),  B(t) = 1/sqrt(2 pi) - t erfcx(t / sqrt 2) / 2 for
//                     t < 32 and (1/sqrt(2 pi)) w (1 - 3 w + 15 w^2 - ... + 34459425 w^8), w = 1 / t^2,
//                     from t = 32 on (the next term is below 3e-17 there, and the erfcx form has lost
//                     t^2 u by cancellation); x = -t^2 / 2 log2(e) is split into rint(x) and a fraction in
//                     [-1/2, 1/2], m = frexp(B exp2(fraction)) frexp(sigma); t^2 >= 1e300 gives 0;
//   sigma = 0:        max(d, 0), split by frexp.
// Per box: F_k = max(m_l - ldexp(m_u, e_u - e_l), 0) at exponent e_l (psi(l) >= psi(u): the upper bound
// is aligned to the lower), the product over k left to right with the exponents added and one frexp,
// then the running sum in box order, aligned to the running maximum exponent; a term with a zero
// factor is skipped.  Exponent differences are clamped to +-2000 before ldexp (far past f64's range).
// Per candidate: L = e ln 2 + ln m, once; m = 0 gives -inf.
//
// Constraints: lp = ((ln P_0 + ln P_1) + ...) is added to L.  With the two tail arguments of
// bo_ehvi_impl.h's ehvi_pof, 0 <= t1 <= t2 in the tail branches, and ln Q(t) = ln(erfcx(t / sqrt 2) / 2) - t^2 / 2:
//   tails, t1 >= 6:  ln P = ln Q(t1) + ln(-expm1(ln Q(t2) - ln Q(t1))), the difference of the logarithms as
//                    [ln(erfcx ..t2 / 2) - ln(erfcx ..t1 / 2)] - (t2 - t1)(t2 + t1) / 2 (-inf at t2 = +inf);
//   tails, t1 < 6:   ln P = ln(Q(t1) - Q(t2)) with Q = erfc(. / sqrt 2) / 2 itself, far from its underflow there
//                    (the difference of two logarithms of order 1 would lose what a thin interval leaves);
//   central:         ln P = log1p(-(Q(zb) + Q(-za))).
// t1^2 past f64's range (t1 above about 1.3e154) gives -inf, as z^2 >= 1e300 gives psi = 0.
//
// Two forms as the EHVI's, with the same bits: the direct form evaluates logehvi_psi at every finite
// bound of every box; the table form once per edge into the thread's column of an LDS table of 16
// bytes per edge and thread (a plane of mantissas, a plane of exponents).  The walk, the order and
// every rounding are the same function (logehvi_factor / logehvi_add) in both.

#include "bo_ehvi_impl.h"

#include <type_traits>

namespace {

constexpr int kLogEhviEdgeBytes = 16;          // an f64 mantissa and an f64 exponent per edge and thread
constexpr int kLogEhviAuto2dEdges = 20;        // auto, 2 objectives: two 256-thread tables per CU
constexpr int kLogEhviAutoThreads = 128;       // auto, 3 and 4 objectives: not the 64-thread table

struct Ext { double m, e; };

__device__ __forceinline__ Ext ext_split(double v) {     // v >= 0, finite
  int e;
  const double m = frexp(v, &e);
  return {m, (double)e};
}

__device__ __forceinline__ double ext_ldexp(double m, double de) {
  return ldexp(m, (int)fmax(fmin(de, 2000.0), -2000.0));
}

__device__ __forceinline__ Ext logehvi_psi(double d, double sigma, double rs) {
  if (sigma == 0.0) return ext_split((d > 0.0 && d < __builtin_inf()) ? d : 0.0);
  const double t = fabs(d * rs);
  if (!(d < 0.0)) {
    double h = 0.0;
    if (t < 40.0) {
      const double e = exp(-0.5 * (t * t));
      h = e * (0.3989422804014327 - (0.5 * t) * erfcx(t * 0.7071067811865476));
    }
    const double v = sigma * h + fmax(d, 0.0);
    return ext_split(v < __builtin_inf() ? v : 0.0);
  }
  const double t2 = t * t;
  if (!(t2 < 1e300)) return {0.0, 0.0};
  double b;
  if (t < 32.0) {
    b = 0.3989422804014327 - (0.5 * t) * erfcx(t * 0.7071067811865476);
  } else {
    const double w = 1.0 / t2;
    double s = 34459425.0;
    s = -2027025.0 + w * s;
    s = 135135.0 + w * s;
    s = -10395.0 + w * s;
    s = 945.0 + w * s;
    s = -105.0 + w * s;
    s = 15.0 + w * s;
    s = -3.0 + w * s;
    s = 1.0 + w * s;
    b = (0.3989422804014327 * w) * s;
  }
  const double x = (-0.5 * t2) * 1.4426950408889634;
  const double ei = rint(x);
  const Ext mb = ext_split(b * exp2(x - ei));
  const Ext ms = ext_split(sigma);
  const double m = mb.m * ms.m;
  if (!(m > 0.0)) return {0.0, 0.0};
  return {m, ei + (mb.e + ms.e)};
}

// One factor of a box: psi(l) - psi(u) >= 0 at psi(l)'s exponent.
__device__ __forceinline__ double logehvi_factor(Ext l, Ext u) { return fmax(l.m - ext_ldexp(u.m, u.e - l.e), 0.0); }

// s += v in extended range (v.m > 0 only), aligned to the larger exponent.
__device__ __forceinline__ void logehvi_add(Ext& s, double vm, double ve) {
  int dv;
  vm = frexp(vm, &dv);
  ve = ve + (double)dv;
  if (vm > 0.0) {
    const double e = fmax(s.e, ve);
    s.m = ext_ldexp(s.m, s.e - e) + ext_ldexp(vm, ve - e);
    s.e = e;
  }
}

__device__ __forceinline__ double logehvi_log(Ext s) {
  return s.m > 0.0 ? s.e * 0.6931471805599453 + log(s.m) : -__builtin_inf();
}

// ln P(lo <= Y <= hi): the branches of ehvi_pof, in logarithms (the file's head states the forms).
__device__ __forceinline__ double logehvi_ln_pof(double mu, double sigma, double lo, double hi) {
  if (mu != mu || sigma != sigma) return __builtin_nan("");
  if (sigma == 0.0) return (lo <= mu && mu <= hi) ? 0.0 : -__builtin_inf();
  const double za = (lo - mu) / sigma, zb = (hi - mu) / sigma;
  const bool above = za > 0.0, below = !above && zb < 0.0;
  const double t1 = above ? za : (below ? -zb : zb);
  const double t2 = above ? zb : -za;
  if ((above || below) && !(t1 < 6.0)) {
    const double l1 = log(0.5 * erfcx(t1 * 0.7071067811865476));
    const double l2 = log(0.5 * erfcx(t2 * 0.7071067811865476));
    const double dl = t2 < __builtin_inf() ? (l2 - l1) - (0.5 * (t2 - t1)) * (t2 + t1) : -__builtin_inf();
    return (l1 - 0.5 * (t1 * t1)) + log(-expm1(dl));
  }
  const double q1 = 0.5 * erfc(t1 * 0.7071067811865476), q2 = 0.5 * erfc(t2 * 0.7071067811865476);
  return (above || below) ? log(q1 - q2) : log1p(-(q1 + q2));
}

// lp of candidate i, left to right; 0 without constraints.  A lane past the end computes on mu = 0, var = 1.
__device__ __forceinline__ double logehvi_logpof(const EhviConArgs& c, long long i, bool valid) {
  double lp = 0.0;
  for (int j = 0; j < c.n_con; ++j) {
    const long long row = (long long)(c.n_obj + j) * c.e.ld + i;
    const double mu = valid ? __builtin_nontemporal_load(c.e.mu + row) : 0.0;
    const double v = valid ? __builtin_nontemporal_load(c.e.var + row) : 1.0;
    const double lj = logehvi_ln_pof(mu, sqrt(fabs(v)), c.lo[j], c.hi[j]);
    lp = j == 0 ? lj : lp + lj;
  }
  return lp;
}

__device__ __forceinline__ double logehvi_finish(const EhviArgs&, long long, bool, double l) { return l; }
__device__ __forceinline__ double logehvi_finish(const EhviConArgs& c, long long i, bool valid, double l) {
  const double lp = logehvi_logpof(c, i, valid);
  if (valid && c.pof) bo_out_store(c.pof + i, lp);
  return c.n_con > 0 ? l + lp : l;
}

template <int M>
__device__ __forceinline__ double logehvi_direct_value(const EhviArgs& a, const double* mu, const double* sg,
                                                       const double* rs) {
  const double inf = __builtin_inf();
  Ext s = {0.0, -inf};
  const double* b = a.boxes;
  for (long long t = 0; t < a.n_boxes; ++t, b += 2 * M) {
    double vm = 1.0, ve = 0.0;
#pragma unroll
    for (int k = 0; k < M; ++k) {
      const Ext pl = logehvi_psi(mu[k] - b[k], sg[k], rs[k]);
      Ext pu = {0.0, 0.0};
      if (b[M + k] < inf) pu = logehvi_psi(mu[k] - b[M + k], sg[k], rs[k]);
      const double f = logehvi_factor(pl, pu);
      vm = k == 0 ? f : vm * f;
      ve = k == 0 ? pl.e : ve + pl.e;
    }
    logehvi_add(s, vm, ve);
  }
  return logehvi_log(s);
}

// The table [2][sum E][T] of a workgroup of T threads: `col` is the thread's column of the mantissa
// plane, the exponent plane lies `plane` doubles further.  A thread reads only what it wrote.
template <int M, int T>
__device__ __forceinline__ double logehvi_table_value(const EhviArgs& a, double* col, int plane, const double* mu,
                                                      const double* sg, const double* rs) {
#pragma unroll
  for (int k = 0; k < M; ++k) {
    const double* e = a.edges + a.edge_off[k];
    double* c = col + a.edge_off[k] * T;
    for (int j = 0; j < a.n_edges[k]; ++j) {
      const Ext p = logehvi_psi(mu[k] - e[j], sg[k], rs[k]);
      c[j * T] = p.m;
      c[plane + j * T] = p.e;
    }
  }
  Ext s = {0.0, -__builtin_inf()};
  const int* b = a.box_idx;
  for (long long t = 0; t < a.n_boxes; ++t, b += 2 * M) {
    double vm = 1.0, ve = 0.0;
#pragma unroll
    for (int k = 0; k < M; ++k) {
      const int il = (a.edge_off[k] + b[k]) * T;
      const Ext pl = {col[il], col[plane + il]};
      Ext pu = {0.0, 0.0};
      if (b[M + k] < a.n_edges[k]) {
        const int iu = (a.edge_off[k] + b[M + k]) * T;
        pu = {col[iu], col[plane + iu]};
      }
      const double f = logehvi_factor(pl, pu);
      vm = k == 0 ? f : vm * f;
      ve = k == 0 ? pl.e : ve + pl.e;
    }
    logehvi_add(s, vm, ve);
  }
  return logehvi_log(s);
}

template <int M, bool CON>
__global__ __launch_bounds__(256) void logehvi_direct_kernel(const typename EhviScan<CON>::Args ca) {
  const EhviArgs& a = ehvi_base(ca);
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool valid = i < a.n;
  double mu[M], sg[M], rs[M];
  const bool nan = ehvi_load<M>(a, i, valid, mu, sg, rs);
  const double l = logehvi_finish(ca, i, valid, logehvi_direct_value<M>(a, mu, sg, rs));
  if (valid) bo_out_store(a.acq + i, nan ? __builtin_nan("") : l);
}

template <int M, int T, bool CON>
__global__ __launch_bounds__(T) void logehvi_table_kernel(const typename EhviScan<CON>::Args ca, int sum_e) {
  extern __shared__ double logehvi_tab[];
  const EhviArgs& a = ehvi_base(ca);
  const long long i = (long long)blockIdx.x * T + threadIdx.x;
  const bool valid = i < a.n;
  double mu[M], sg[M], rs[M];
  const bool nan = ehvi_load<M>(a, i, valid, mu, sg, rs);
  const double l =
      logehvi_finish(ca, i, valid, logehvi_table_value<M, T>(a, logehvi_tab + threadIdx.x, sum_e * T, mu, sg, rs));
  if (valid) bo_out_store(a.acq + i, nan ? __builtin_nan("") : l);
}

template <class A>
int launch_direct(const A& ca, int m, hipStream_t s) {
  constexpr bool C = std::is_same<A, EhviConArgs>::value;
  const dim3 g((unsigned)ehvi_blocks(ehvi_base(ca).n, 256));
  switch (m) {
    case 1: hipLaunchKernelGGL((logehvi_direct_kernel<1, C>), g, dim3(256), 0, s, ca); break;
    case 2: hipLaunchKernelGGL((logehvi_direct_kernel<2, C>), g, dim3(256), 0, s, ca); break;
    case 3: hipLaunchKernelGGL((logehvi_direct_kernel<3, C>), g, dim3(256), 0, s, ca); break;
    case 4: hipLaunchKernelGGL((logehvi_direct_kernel<4, C>), g, dim3(256), 0, s, ca); break;
    default: return BO_ERR_UNSUPPORTED;
  }
  BO_CHECK_HIP(hipGetLastError());
  return BO_OK;
}

template <int M, int T, class A>
int launch_table_mt(const A& ca, int sum_e, hipStream_t s) {
  constexpr bool C = std::is_same<A, EhviConArgs>::value;
  const size_t lds = (size_t)sum_e * T * kLogEhviEdgeBytes;
  if (lds > 64 * 1024)
    BO_CHECK_HIP(hipFuncSetAttribute((const void*)logehvi_table_kernel<M, T, C>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((logehvi_table_kernel<M, T, C>), dim3((unsigned)ehvi_blocks(ehvi_base(ca).n, T)), dim3(T), lds,
                     s, ca, sum_e);
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

// ehvi_plan's checks and edge offsets with this scan's admission rule and auto rule (include/bo_amd.h).
int logehvi_plan(int form, int n_obj, long long n_boxes, bool have_boxes, bool have_tables, const int32_t* n_edges,
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
  *threads = have_tables ? bo_logehvi_table_threads(sum_e) : 0;
  if (form == 2 && *threads == 0) return BO_ERR_UNSUPPORTED;
  *table = form == 2 || (form == 0 && *threads != 0 && n_boxes > 0 &&
                         (!have_boxes || (n_obj >= 3 && *threads >= kLogEhviAutoThreads) ||
                          (n_obj == 2 && sum_e <= kLogEhviAuto2dEdges)));
  if (!*table && !have_boxes) return BO_ERR_UNSUPPORTED;     // auto, tables only, and they do not fit
  *sum_edges = (int)sum_e;
  return BO_OK;
}

}  // namespace

extern "C" {

int bo_logehvi_table_threads(int64_t sum_edges) {
  if (sum_edges < 0) return 0;
  for (int t = 256; t >= 64; t /= 2)
    if (sum_edges <= kEhviLdsBytes / (t * kLogEhviEdgeBytes)) return t;
  return 0;
}

int bo_log_ehvi(double* acq, double* logpof_out, const double* mu, const double* var, int64_t ld, int64_t n,
                int32_t n_obj, int32_t n_con, const double* con_lo, const double* con_hi, const double* boxes,
                int64_t n_boxes, const double* edges, const int32_t* n_edges, const int32_t* box_idx, int32_t form,
                void* stream) {
  if (n_obj < 1 || n_obj > 4 || n_con < 0 || n_obj + n_con > BO_MAX_OBJ || (n_con > 0 && (!con_lo || !con_hi)))
    return BO_ERR_ARG;
  const double inf = __builtin_inf();
  for (int j = 0; j < n_con; ++j)      // lo <= hi, neither NaN, each infinite on its own side only
    if (!(con_lo[j] <= con_hi[j]) || con_lo[j] == inf || con_hi[j] == -inf) return BO_ERR_ARG;
  if (!acq || !mu || !var || n < 0 || ld < n || n_boxes < 0 || form < 0 || form > 2) return BO_ERR_ARG;
  if (n > ((int64_t)1 << 36)) return BO_ERR_UNSUPPORTED;     // one thread per candidate: the grid's limit
  const bool have_tables = n_edges && (n_boxes == 0 || (edges && box_idx));
  const bool have_boxes = n_boxes == 0 || boxes;
  if ((form == 1 && !have_boxes) || (form == 2 && !have_tables) || (form == 0 && !have_boxes && !have_tables))
    return BO_ERR_ARG;
  EhviConArgs c;
  memset(&c, 0, sizeof(c));
  int sum_e = 0, threads = 0;
  bool table = false;
  const int st = logehvi_plan(form, n_obj, n_boxes, have_boxes, have_tables, n_edges, &c.e, &sum_e, &threads, &table);
  if (st != BO_OK) return st;
  if (n == 0) return BO_OK;
  c.e.acq = acq;
  c.e.mu = mu;
  c.e.var = var;
  c.e.ld = ld;
  c.e.n = n;
  c.e.boxes = boxes;
  c.e.edges = edges;
  c.e.box_idx = box_idx;
  c.e.n_boxes = n_boxes;
  hipStream_t s = (hipStream_t)stream;
  if (n_con == 0 && !logpof_out)       // the plain scan
    return table ? launch_table(c.e, n_obj, sum_e, threads, s) : launch_direct(c.e, n_obj, s);
  c.pof = logpof_out;
  c.n_obj = n_obj;
  c.n_con = n_con;
  for (int j = 0; j < n_con; ++j) {
    c.lo[j] = con_lo[j];
    c.hi[j] = con_hi[j];
  }
  return table ? launch_table(c, n_obj, sum_e, threads, s) : launch_direct(c, n_obj, s);
}

}  // extern "C"
