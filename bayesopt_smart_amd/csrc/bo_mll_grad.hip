// The marginal log likelihood's analytic gradient in log(length scale), per objective, beside its
// value: bo_compute_mll_grad.
//
// Per objective o, with C = e + jitter I, e_ij = exp(-r2_ij / (2 ls^2)), yc = (y - pm) / std (the
// MLL's own standardisation: population std about its own mean, unscaled when that std is 0) and
// alpha = C^-1 yc:
//
//   d MLL_o / d log ls_o = 1/2 sum_ij (alpha_i alpha_j - C^-1_ij) e_ij r2_ij / ls^2
//
// (1/2 tr((alpha alpha^T - C^-1) dC/d log ls), dC_ij/d log ls = e_ij r2_ij / ls^2).  The prior
// variance does not appear: the MLL factors the correlation matrix, so d MLL / d pv is exactly 0.
//
// What runs:
//   1. the value: bo_compute_mll_each_jitter itself (same factorisation path and schedule, same
//      bits, kernel_matrix left as pv e); its BO_ERR_NOT_PD ends the call;
//   2. grad_corr_kernel builds the pv-free e into the workspace (fit_init_kernel's expression, so
//      the matrix inverted is the matrix factored, without the jitter), grad_center_kernel yc;
//   3. C^-1 by invert_k's augmented Cholesky with the MLL's jitter (bo_fit_cholesky_inverse), WITHOUT
//      invert_k's Newton step: the Cholesky inverse is the exact inverse of one symmetric C + dC,
//      |dC| <= c u, which is what the gradient's error scale assumes; the Newton step trades that for a
//      small residual C X - I column by column and adds rounding of the order u |X|^2 to X -- measured
//      on an MI355X over the tests' cases, the gradient's largest err / (u S) is 0.45 without the step
//      and 833 with it.  No LU or Gauss-Jordan after it: a failure is BO_ERR_NOT_PD;
//   4. grad_alpha_kernel: alpha, one wave per row of C^-1;
//   5. grad_tile_kernel: one workgroup per 32 x 32 tile of the N x N sum, x of the tile's rows
//      and columns staged in LDS, r2 recomputed from x, e and C^-1 read once; its partial goes to
//      the workspace;
//   6. grad_sum_kernel: the partials of an objective summed in a fixed order (tile t by thread
//      t mod 256 in ascending t, then a tree over the 256).
// No floating-point atomics anywhere: two calls give the same bits, whichever CU ran which tile.

#include "bo_common.h"

#include <string.h>

namespace {

constexpr int GT = 32;        // tile of the N x N sum (256 threads, 4 entries each)
constexpr int GDC = 8;        // coordinates of x staged per pass (BO_MAX_DIM; more dims: more passes)

struct GradParams {
  double pm[BO_MAX_OBJ], ls2[BO_MAX_OBJ];
};

// e[o][i][j] = exp(-0.5 |x_i - x_j|^2 / ls_o^2), n x n row-major per objective: the value
// fit_init_kernel factors (before its jitter), symmetric bit for bit (d * d, the same fma chain)
__global__ __launch_bounds__(256) void grad_corr_kernel(double* __restrict__ E, const double* __restrict__ x,
                                                        int dim, int n, int nt, GradParams p) {
  const int o = blockIdx.y, tid = threadIdx.x;
  const int ti = blockIdx.x / nt, tj = blockIdx.x % nt;
  double* Eo = E + (long long)o * n * n;
  const int cc = tid & 31;
  const long long j = (long long)tj * GT + cc;
#pragma unroll
  for (int pass = 0; pass < GT / 8; ++pass) {
    const long long i = (long long)ti * GT + (tid >> 5) + 8 * pass;
    if (i >= n || j >= n) continue;
    double sq = 0.0;
    for (int k = 0; k < dim; ++k) {
      const double d = x[i * dim + k] - x[j * dim + k];
      sq = __builtin_fma(d, d, sq);
    }
    Eo[i * n + j] = exp(-0.5 * sq / p.ls2[o]);
  }
}

// yc[o][i] = (y[i][o] - pm_o) / std, std the population std of y - pm about its own mean (two
// passes, as fit_init_kernel's var(y - pm)); unscaled when std == 0.  One workgroup per objective.
__global__ __launch_bounds__(256) void grad_center_kernel(double* __restrict__ yc, const double* __restrict__ y,
                                                          long long ld_y, int n, GradParams p) {
  __shared__ double red[256];
  const int o = blockIdx.x, tid = threadIdx.x;
  double s = 0.0;
  for (int i = tid; i < n; i += 256) s += y[(long long)i * ld_y + o] - p.pm[o];
  red[tid] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) { if (tid < w) red[tid] += red[tid + w]; __syncthreads(); }
  const double mean = red[0] / n;
  __syncthreads();
  s = 0.0;
  for (int i = tid; i < n; i += 256) {
    const double d = (y[(long long)i * ld_y + o] - p.pm[o]) - mean;
    s += d * d;
  }
  red[tid] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) { if (tid < w) red[tid] += red[tid + w]; __syncthreads(); }
  const double sd = sqrt(red[0] / n);
  for (int i = tid; i < n; i += 256) {
    const double v = y[(long long)i * ld_y + o] - p.pm[o];
    yc[(long long)o * n + i] = sd > 0.0 ? v / sd : v;
  }
}

// sum over the wave in a fixed order (xor butterfly: every lane ends with the same bits)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// alpha[o][i] = sum_j Cinv[o][i][j] yc[o][j]: one wave per row, lane l takes j = l, l + 64, ...
__global__ __launch_bounds__(256) void grad_alpha_kernel(double* __restrict__ alpha, const double* __restrict__ Cinv,
                                                         const double* __restrict__ yc, int n) {
  const int o = blockIdx.y, lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;                                   // wave-uniform
  const double* row = Cinv + ((long long)o * n + i) * n;
  const double* v = yc + (long long)o * n;
  double s = 0.0;
  for (int j = lane; j < n; j += 64) s = __builtin_fma(row[j], v[j], s);
  s = wave_sum(s);
  if (lane == 0) alpha[(long long)o * n + i] = s;
}

// Tile (ti, tj) of sum_ij (alpha_i alpha_j - Cinv_ij) e_ij r2_ij / ls^2 for objective blockIdx.y;
// thread (tid >> 5, tid & 31) takes rows (tid >> 5) + 8 pass of column tid & 31 (row-major reads,
// 256 bytes per 32 lanes).  part[o * nt * nt + tile].
__global__ __launch_bounds__(256) void grad_tile_kernel(double* __restrict__ part, const double* __restrict__ E,
                                                        const double* __restrict__ Cinv,
                                                        const double* __restrict__ alpha,
                                                        const double* __restrict__ x, int dim, int n, int nt,
                                                        GradParams p) {
  __shared__ double xr[GT][GDC + 1], xc[GT][GDC + 1];
  __shared__ double ar[GT], ac[GT];
  __shared__ double wsum[4];
  const int o = blockIdx.y, tid = threadIdx.x;
  const int ti = blockIdx.x / nt, tj = blockIdx.x % nt;
  const long long r0 = (long long)ti * GT, c0 = (long long)tj * GT;
  const int cc = tid & 31, rb = tid >> 5;
  const double* al = alpha + (long long)o * n;
  if (tid < GT) ar[tid] = r0 + tid < n ? al[r0 + tid] : 0.0;
  else if (tid < 2 * GT) ac[tid - GT] = c0 + (tid - GT) < n ? al[c0 + (tid - GT)] : 0.0;
  double sq[GT / 8];
#pragma unroll
  for (int pass = 0; pass < GT / 8; ++pass) sq[pass] = 0.0;
  for (int k0 = 0; k0 < dim; k0 += GDC) {
    const int kn = dim - k0 < GDC ? dim - k0 : GDC;
    __syncthreads();                                    // the previous pass's reads are done
    {
      const int pt = tid >> 3, k = tid & 7;             // 32 points x 8 coordinates: one each
      xr[pt][k] = (k < kn && r0 + pt < n) ? x[(r0 + pt) * dim + k0 + k] : 0.0;
      xc[pt][k] = (k < kn && c0 + pt < n) ? x[(c0 + pt) * dim + k0 + k] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int pass = 0; pass < GT / 8; ++pass) {
      const int rr = rb + 8 * pass;
      for (int k = 0; k < kn; ++k) {
        const double d = xr[rr][k] - xc[cc][k];
        sq[pass] = __builtin_fma(d, d, sq[pass]);
      }
    }
  }
  __syncthreads();                                      // ar / ac (dim >= 1: also synced above)
  const double* Eo = E + (long long)o * n * n;
  const double* Co = Cinv + (long long)o * n * n;
  const double ls2 = p.ls2[o];
  double s = 0.0;
#pragma unroll
  for (int pass = 0; pass < GT / 8; ++pass) {
    const int rr = rb + 8 * pass;
    const long long i = r0 + rr, j = c0 + cc;
    if (i < n && j < n) {
      const double w = __builtin_fma(ar[rr], ac[cc], -Co[i * n + j]);
      s = __builtin_fma(w, Eo[i * n + j] * (sq[pass] / ls2), s);
    }
  }
  s = wave_sum(s);
  if ((tid & 63) == 0) wsum[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) part[(long long)o * nt * nt + blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// grad[o] = 1/2 sum_t part[o][t]: thread t mod 256 adds its tiles in ascending t, then a tree
__global__ __launch_bounds__(256) void grad_sum_kernel(double* __restrict__ grad, const double* __restrict__ part,
                                                       long long tiles) {
  __shared__ double red[256];
  const int o = blockIdx.x, tid = threadIdx.x;
  const double* q = part + (long long)o * tiles;
  double s = 0.0;
  for (long long t = tid; t < tiles; t += 256) s += q[t];
  red[tid] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) { if (tid < w) red[tid] += red[tid + w]; __syncthreads(); }
  if (tid == 0) grad[o] = 0.5 * red[0];
}

inline size_t a256(size_t v) { return (v + 255) & ~(size_t)255; }

struct Carve {
  size_t at = 0;
  size_t operator()(size_t bytes) { const size_t off = at; at += a256(bytes); return off; }
};

// The one description of the workspace: byte offsets, every array padded to 256 bytes.
struct GradLayout { size_t fit, fit_bytes, e, cinv, yc, alpha, part, grad, total; };
GradLayout grad_layout(int n_obj, long long n) {
  Carve take;
  GradLayout L;
  const size_t mll = bo_compute_mll_workspace_size(n_obj, n), inv = bo_invert_k_workspace_size(n_obj, n);
  const long long nt = (n + GT - 1) / GT;
  L.fit_bytes = mll > inv ? mll : inv;
  L.fit = take(L.fit_bytes);                                       // the value's, then the inverse's workspace
  L.e = take((size_t)n_obj * n * n * sizeof(double));              // pv-free correlation matrices
  L.cinv = take((size_t)n_obj * n * n * sizeof(double));           // their inverses (with the jitter)
  L.yc = take((size_t)n_obj * n * sizeof(double));                 // standardised y
  L.alpha = take((size_t)n_obj * n * sizeof(double));              // C^-1 yc
  L.part = take((size_t)n_obj * nt * nt * sizeof(double));         // per-tile partial sums
  L.grad = take((size_t)n_obj * sizeof(double));                   // the result, read back by the host
  L.total = take.at;
  return L;
}

bool grad_in_limits(int32_t n_obj, int64_t n) {
  // bo_compute_mll's limits; the inverse's N range (2^15) is the narrower one
  return n_obj >= 1 && n_obj <= BO_MAX_OBJ && n >= 1 && n <= (1 << 15);
}

}  // namespace

extern "C" {

size_t bo_compute_mll_grad_workspace_size(int32_t n_obj, int64_t n) {
  if (!grad_in_limits(n_obj, n)) return 0;
  return grad_layout(n_obj, n).total;
}

int bo_compute_mll_grad(double* mll_obj, double* grad_log_ls, const double* x, int32_t dim, const double* y,
                        int64_t ld_y, double* km, int64_t ld, int32_t n_obj, const double* pm, const double* pv,
                        const double* ls, int64_t n, double jitter, void* ws, size_t ws_bytes, void* stream) {
  if (!mll_obj || !grad_log_ls || !x || !y || !km || !pm || !pv || !ls || n_obj < 1 || n_obj > BO_MAX_OBJ ||
      n < 1 || ld < n || ld_y < n_obj || dim < 1)
    return BO_ERR_ARG;
  if (!grad_in_limits(n_obj, n)) return BO_ERR_UNSUPPORTED;
  if (!ws || ws_bytes < bo_compute_mll_grad_workspace_size(n_obj, n)) return BO_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  char* w = (char*)ws;
  const GradLayout L = grad_layout(n_obj, n);
  // the value: compute_mll's own call -- its bits, its kernel_matrix, its error first
  int st = bo_compute_mll_each_jitter(mll_obj, x, dim, y, ld_y, km, ld, n_obj, pm, pv, ls, n, jitter, w + L.fit,
                                      L.fit_bytes, stream);
  if (st != BO_OK) return st;
  GradParams p;
  memset(&p, 0, sizeof(p));
  for (int o = 0; o < n_obj; ++o) {
    p.pm[o] = pm[o];
    p.ls2[o] = ls[o] * ls[o];
  }
  double* E = (double*)(w + L.e);
  double* Cinv = (double*)(w + L.cinv);
  double* yc = (double*)(w + L.yc);
  double* alpha = (double*)(w + L.alpha);
  double* part = (double*)(w + L.part);
  double* grad = (double*)(w + L.grad);
  const int nt = (int)((n + GT - 1) / GT);
  const dim3 tiles((unsigned)(nt * (long long)nt), (unsigned)n_obj);
  hipLaunchKernelGGL(grad_corr_kernel, tiles, dim3(256), 0, s, E, x, (int)dim, (int)n, nt, p);
  hipLaunchKernelGGL(grad_center_kernel, dim3((unsigned)n_obj), dim3(256), 0, s, yc, y, (long long)ld_y, (int)n, p);
  BO_CHECK_HIP(hipGetLastError());
  int32_t fail[BO_MAX_OBJ];
  st = bo_fit_cholesky_inverse(Cinv, E, n, n_obj, n, jitter, /*refine=*/false, fail, w + L.fit, L.fit_bytes, s);
  if (st != BO_OK) return st;
  for (int o = 0; o < n_obj; ++o)
    if (fail[o]) return BO_ERR_NOT_PD;
  hipLaunchKernelGGL(grad_alpha_kernel, dim3((unsigned)((n + 3) / 4), (unsigned)n_obj), dim3(256), 0, s, alpha,
                     (const double*)Cinv, (const double*)yc, (int)n);
  hipLaunchKernelGGL(grad_tile_kernel, tiles, dim3(256), 0, s, part, (const double*)E, (const double*)Cinv,
                     (const double*)alpha, x, (int)dim, (int)n, nt, p);
  hipLaunchKernelGGL(grad_sum_kernel, dim3((unsigned)n_obj), dim3(256), 0, s, grad, (const double*)part,
                     (long long)nt * nt);
  BO_CHECK_HIP(hipGetLastError());
  BO_CHECK_HIP(hipMemcpyAsync(grad_log_ls, grad, sizeof(double) * n_obj, hipMemcpyDeviceToHost, s));
  BO_CHECK_HIP(hipStreamSynchronize(s));
  return BO_OK;
}

}  // extern "C"
