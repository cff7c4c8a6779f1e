// Max-value entropy search for multi-objective problems (MESMO: Belakaria, Deshwal & Doppa 2019,
// after Wang & Jegelka 2017; opt-in acquisition "mes").  NOT in the reference, which has no
// information-theoretic acquisition: parity is unpinned by it (tests/mes_ref.py is the
// independent statement).  include/bo_amd.h states the quantity, its limits and its rounding rule.
//
// Two kernels beside bo_sample_paths (bo_ts.hip), which supplies the posterior draws:
//   bo_path_maxima        y*_sk = fl(shift_k + scale_k max_c paths[s][k][c]): one HBM pass over the
//                         paths, fixed-order partial maxima in the workspace (one per row and chunk
//                         of kChunk columns), then one finishing workgroup.  The max is exact, so
//                         neither the chunking nor a split into shards changes a bit.  No atomics.
//   bo_max_value_entropy  acq(c) = (1/S) sum_s sum_k g((y*_sk - mu_k(c)) / sigma_k(c)): one thread
//                         per candidate, the S n_obj maxima at wave-uniform addresses (scalar
//                         loads), 1 / sigma_k once per objective, s outer and k inner into one f64
//                         accumulator.
//
// g(x) = x phi(x) / (2 Phi(x)) - ln Phi(x) in three branches (mes_g); neither tail of the textbook
// form survives f64 (Phi -> 0 on the left, 1 - Phi -> 0 on the right).

#include "bo_common.h"

#include <cmath>

namespace {

struct MesVec {
  double shift[BO_MAX_OBJ], scale[BO_MAX_OBJ];
};

// the larger of a and v with NaN ignored (NaN only while nothing else was seen); exact
__device__ __forceinline__ double nanmax2(double a, double v) { return (v > a || a != a) ? v : a; }

constexpr int kMaxThreads = 256;
constexpr int kMaxUnroll = 8;
constexpr long long kChunk = (long long)kMaxThreads * kMaxUnroll * 4;     // 8192 columns per workgroup

// partial[r * n_chunks + c] = the NaN-ignoring maximum of paths[r][c kChunk .. min(n_cand, (c + 1) kChunk))
__global__ __launch_bounds__(kMaxThreads) void path_maxima_partial_kernel(double* __restrict__ partial,
                                                                         const double* __restrict__ paths,
                                                                         long long ld, long long n_cand,
                                                                         long long n_chunks) {
  __shared__ double red[kMaxThreads / 64];
  const long long c = blockIdx.x, r = blockIdx.y;
  const double* row = paths + r * ld;
  const long long j0 = c * kChunk;
  const long long j1 = j0 + kChunk < n_cand ? j0 + kChunk : n_cand;
  double m = __builtin_nan("");
  for (long long b = j0; b < j1; b += (long long)kMaxThreads * kMaxUnroll) {     // workgroup-uniform
    double v[kMaxUnroll];
#pragma unroll
    for (int u = 0; u < kMaxUnroll; ++u) {                // all loads in flight before any compare
      const long long j = b + (long long)u * kMaxThreads + threadIdx.x;
      v[u] = j < j1 ? __builtin_nontemporal_load(row + j) : __builtin_nan("");
    }
#pragma unroll
    for (int u = 0; u < kMaxUnroll; ++u) m = nanmax2(m, v[u]);
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) m = nanmax2(m, __shfl_xor(m, s, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kMaxThreads / 64; ++w) m = nanmax2(m, red[w]);
    partial[r * n_chunks + c] = m;
  }
}

// One workgroup: wave w finishes rows w, w + 4, ...; a zero of either sign counts as +0 (so the
// sign of a zero maximum does not depend on the order either), then the one fma.
__global__ __launch_bounds__(kMaxThreads) void path_maxima_finish_kernel(double* __restrict__ ystar,
                                                                        const double* __restrict__ partial,
                                                                        long long n_chunks, int n_rows, int n_obj,
                                                                        MesVec p) {
  const int lane = threadIdx.x & 63;
  for (int r = threadIdx.x >> 6; r < n_rows; r += kMaxThreads / 64) {          // wave-uniform
    double m = __builtin_nan("");
    for (long long c = lane; c < n_chunks; c += 64) m = nanmax2(m, partial[(long long)r * n_chunks + c]);
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) m = nanmax2(m, __shfl_xor(m, s, 64));
    const int k = r % n_obj;
    double sh = p.shift[0], sc = p.scale[0];
#pragma unroll
    for (int o = 1; o < BO_MAX_OBJ; ++o) {
      sh = k == o ? p.shift[o] : sh;
      sc = k == o ? p.scale[o] : sc;
    }
    if (lane == 0) ystar[r] = __builtin_fma(sc, m + 0.0, sh);
  }
}

// g(x) = x phi(x) / (2 Phi(x)) - ln Phi(x): the entropy of N(0, 1) minus the entropy of N(0, 1)
// truncated above at x.  >= 0, decreasing, g(0) = ln 2, g(+inf) = 0, g(-inf) = +inf, g(NaN) = NaN.
//   x >= 0:          q = erfc(x / sqrt 2) / 2 = 1 - Phi;  g = x phi / (2 (1 - q)) - log1p(-q)
//   -2^27 < x < 0:   t = -x / sqrt 2, E = erfcx(t) (Phi = exp(-t^2) E / 2):
//                    g = t^2 - t / (sqrt(pi) E) - ln(E / 2); the first two terms cancel to about
//                    -1/2 for large t, which the rounding rule's 1 + x^2 / 2 accounts for
//   x <= -2^27:      g = ln(-x) + (ln(2 pi) - 1) / 2, the asymptote (its error O(1 / x^2) is below
//                    half an ulp there, and the middle form would be inf - inf at -inf)
__device__ __forceinline__ double mes_g(double x) {
  if (x >= 0.0) {
    const double q = 0.5 * erfc(x * 0.7071067811865476);
    const double ph = exp(-0.5 * x * x) * 0.3989422804014327;
    const double xp = ph == 0.0 ? 0.0 : x * ph;          // x = +inf: inf * 0
    return xp / (2.0 * (1.0 - q)) - log1p(-q);
  }
  if (x <= -134217728.0) return log(-x) + 0.4189385332046727;
  const double t = -x * 0.7071067811865476;
  const double e = erfcx(t);
  const double r = t / (1.772453850905516 * e);
  return __builtin_fma(t, t, -r) - log(0.5 * e);          // NaN stays NaN
}

struct MesArgs {
  double* acq;
  const double* mu;
  const double* var;
  long long ld, n;
  const double* ystar;      // [S][M]
  int n_samples;
  double inv_s;             // fl(1 / S)
};

template <int M>
__global__ __launch_bounds__(256) void mes_scan_kernel(const MesArgs a) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  double mu[M], sg[M], rs[M];
#pragma unroll
  for (int k = 0; k < M; ++k) {
    mu[k] = __builtin_nontemporal_load(a.mu + (long long)k * a.ld + i);
    sg[k] = sqrt(fabs(__builtin_nontemporal_load(a.var + (long long)k * a.ld + i)));
    rs[k] = 1.0 / sg[k];
  }
  double acc = 0.0;
  const double* ys = a.ystar;
  for (int s = 0; s < a.n_samples; ++s, ys += M) {
#pragma unroll
    for (int k = 0; k < M; ++k) {
      const double d = ys[k] - mu[k];
      double g;
      if (sg[k] == 0.0)      // a point mass: nothing to learn below the maximum, everything above it
        g = d >= 0.0 ? 0.0 : (d < 0.0 ? __builtin_inf() : __builtin_nan(""));
      else
        g = mes_g(d * rs[k]);
      acc += g;
    }
  }
  bo_out_store(a.acq + i, acc * a.inv_s);
}

int launch_scan(const MesArgs& a, int m, hipStream_t s) {
  const dim3 g((unsigned)((a.n + 255) / 256));
  switch (m) {
    case 1: hipLaunchKernelGGL(mes_scan_kernel<1>, g, dim3(256), 0, s, a); break;
    case 2: hipLaunchKernelGGL(mes_scan_kernel<2>, g, dim3(256), 0, s, a); break;
    case 3: hipLaunchKernelGGL(mes_scan_kernel<3>, g, dim3(256), 0, s, a); break;
    case 4: hipLaunchKernelGGL(mes_scan_kernel<4>, g, dim3(256), 0, s, a); break;
    case 5: hipLaunchKernelGGL(mes_scan_kernel<5>, g, dim3(256), 0, s, a); break;
    case 6: hipLaunchKernelGGL(mes_scan_kernel<6>, g, dim3(256), 0, s, a); break;
    case 7: hipLaunchKernelGGL(mes_scan_kernel<7>, g, dim3(256), 0, s, a); break;
    case 8: hipLaunchKernelGGL(mes_scan_kernel<8>, g, dim3(256), 0, s, a); break;
    default: return BO_ERR_ARG;
  }
  BO_CHECK_HIP(hipGetLastError());
  return BO_OK;
}

bool counts_ok(int32_t n_samples, int32_t n_obj) {
  return n_samples >= 1 && n_samples <= BO_MAX_TOPQ && n_obj >= 1 && n_obj <= BO_MAX_OBJ;
}

long long chunks_of(int64_t n_cand) { return (long long)((n_cand + kChunk - 1) / kChunk); }

}  // namespace

extern "C" {

size_t bo_path_maxima_workspace_size(int64_t n_cand, int64_t n_rows) {
  if (n_cand < 0 || n_rows < 1 || n_rows > (int64_t)BO_MAX_TOPQ * BO_MAX_OBJ || n_cand > ((int64_t)1 << 40)) return 0;
  const size_t bytes = (size_t)n_rows * (size_t)chunks_of(n_cand) * sizeof(double);
  return (bytes + 255) / 256 * 256 + 256;
}

int bo_path_maxima(double* ystar, const double* paths, int64_t ld, int64_t n_cand, int32_t n_samples,
                   int32_t n_obj, const double* shift, const double* scale, void* workspace,
                   size_t workspace_bytes, void* stream) {
  if (!ystar || (!paths && n_cand > 0) || !shift || !scale || n_cand < 0 || ld < n_cand || !counts_ok(n_samples, n_obj))
    return BO_ERR_ARG;
  MesVec p;
  memset(&p, 0, sizeof(p));
  for (int k = 0; k < n_obj; ++k) {
    if (!std::isfinite(shift[k]) || !std::isfinite(scale[k]) || !(scale[k] > 0.0)) return BO_ERR_ARG;
    p.shift[k] = shift[k];
    p.scale[k] = scale[k];
  }
  const int n_rows = n_samples * n_obj;
  const size_t need = bo_path_maxima_workspace_size(n_cand, n_rows);
  if (need == 0) return BO_ERR_UNSUPPORTED;
  if (!workspace || workspace_bytes < need) return BO_ERR_WORKSPACE;
  const long long n_chunks = chunks_of(n_cand);
  if (n_chunks > 0x7FFFFFFFll) return BO_ERR_UNSUPPORTED;
  double* partial = (double*)workspace;
  hipStream_t s = (hipStream_t)stream;
  if (n_chunks > 0) {
    hipLaunchKernelGGL(path_maxima_partial_kernel, dim3((unsigned)n_chunks, (unsigned)n_rows), dim3(kMaxThreads), 0, s,
                       partial, paths, (long long)ld, (long long)n_cand, n_chunks);
    BO_CHECK_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(path_maxima_finish_kernel, dim3(1), dim3(kMaxThreads), 0, s, ystar, partial, n_chunks, n_rows,
                     (int)n_obj, p);
  BO_CHECK_HIP(hipGetLastError());
  return BO_OK;
}

int bo_max_value_entropy(double* acq, const double* mu, const double* var, int64_t ld, int64_t n, int32_t n_obj,
                         const double* ystar, int32_t n_samples, void* stream) {
  if (!acq || !mu || !var || !ystar || n < 0 || ld < n || !counts_ok(n_samples, n_obj)) return BO_ERR_ARG;
  if (n > ((int64_t)1 << 36)) return BO_ERR_UNSUPPORTED;     // one thread per candidate: the grid's limit
  if (n == 0) return BO_OK;
  MesArgs a;
  a.acq = acq;
  a.mu = mu;
  a.var = var;
  a.ld = ld;
  a.n = n;
  a.ystar = ystar;
  a.n_samples = n_samples;
  a.inv_s = 1.0 / (double)n_samples;
  return launch_scan(a, n_obj, (hipStream_t)stream);
}

}  // extern "C"
