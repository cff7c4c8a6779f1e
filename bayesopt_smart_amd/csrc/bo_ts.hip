// Posterior function draws by pathwise conditioning (Wilson et al. 2020) over a random-Fourier-
// feature prior: bo_sample_paths.  NOT in the reference.  include/bo_amd.h states the
// definition; DESIGN.md §12 the layout and the measurements.
//
// Per objective o the value of draw s at candidate c is ONE contraction of the D + N values the
// candidate generates -- D cosine features cos(2 pi (w'_i . (c - x0) + b'_i)), w' = Z / l / 2 pi,
// b' = B / 2 pi (the argument in turns: cospi reduces it exactly), then the N kernel values
// pv exp(-|c - x_n|^2 / 2 l^2) in the predict's exp2_tab form -- with the (D + N) x S matrix
//   W_o = [ sqrt(2 pv / D) Theta_o ; v_o ],     v_so = K^-1 (y_o - pm_o - g_so(X) - sqrt(jitter) E_so)
// on the f64 matrix cores (v_mfma_f64_16x16x4_f64: A = 16 candidates x 4 rows, one generated value
// per lane, lane l = (candidate l & 15, row 4k + (l >> 4)); B = 4 rows x 16 samples of W; every
// further 16-sample tile reuses the generated value).  The launches, all on the stream:
//   prep     the centred training rows, the feature rows (w', b'), W's feature part (W's training
//            part zeroed: its padding stays zero)
//   paths    prior-only over the training rows (kind F64): g(X)
//   resid    r = y - pm - g(X) - sqrt(jitter) E, in place
//   matvec   v = K^-1 r for the S n_obj right-hand sides (a wave per row, lanes stride the row,
//            xor tree: fixed order), into W and weights_out
//   paths    the hot path over the candidates
// An output element is one accumulator element of one wave: its own chain over the rows in row
// order, with the row chunks cut at the same rows for every candidate -- so the value of a
// candidate does not depend on the workgroup, the tile position or the shard it is computed in.
#include "bo_cand.h"

#include <math.h>
#include <string.h>

namespace {

constexpr int kThreads = 256;           // 4 waves
constexpr int kTiles = 2;               // 16-candidate tiles per wave: 128 candidates per workgroup
constexpr int kCandPerBlock = (kThreads / 64) * 16 * kTiles;
constexpr int kChunkDoubles = 4096;     // LDS doubles of one staged chunk (rows + weights): 32 KiB
constexpr int kMatRows = 16;            // K^-1 rows per workgroup of the mat-vec (4 per wave)
constexpr int kMatSamples = 4;          // right-hand sides per pass over a K^-1 row
constexpr int kMaxTrain = 65536;
constexpr int kMaxFeatures = 65536;     // BO_TS_MAX_FEATURES

struct TsArgs {
  int n_obj, dimp, n, np, nf, fp, ns, sp;   // np / fp: rows padded to 4; sp: samples to 16
  long long ld, ld_k, ld_y;
  CandArgs cand;         // the points of this pass (centred on training row 0): the training rows, then the shard
  const double* x_train;
  const double* y;
  const double* kinv;
  const double* z;
  const double* phase;
  const double* theta;
  const double* eps;
  double nl2[BO_MAX_OBJ], lpv[BO_MAX_OBJ], spv[BO_MAX_OBJ], amp[BO_MAX_OBJ], pm[BO_MAX_OBJ], ls[BO_MAX_OBJ];
  double sqrt_jitter;
  double* xr;            // [np][dimp + 1]        training rows minus row 0, slot dimp unused (0)
  double* fr;            // [n_obj][fp][dimp + 1] w' and, in slot dimp, b'
  double* w;             // [n_obj][fp + np][sp]  the weight matrix
  double* gx;            // [ns][n_obj][n]        g(X), then r
  double* out;           // [ns][n_obj][ld]
  double* weights_out;   // [ns][n_obj][n] or null
};

// Rows and weights in the staged layouts.  Padded rows (to multiples of 4) and padded samples
// (to multiples of 16) have weight 0 and generate finite values (cos(0), pv): they add exact zeros.
__global__ __launch_bounds__(256) void ts_prep_kernel(TsArgs a) {
  const int rs = a.dimp + 1;
  const long long n_xr = (long long)a.np * rs;
  const long long n_fr = (long long)a.n_obj * a.fp * rs;
  const long long n_w = (long long)a.n_obj * (a.fp + a.np) * a.sp;
  const double inv_2pi = 0.15915494309189535;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_xr + n_fr + n_w;
       i += (long long)gridDim.x * blockDim.x) {
    if (i < n_xr) {
      const int f = (int)(i / rs), k = (int)(i - (long long)f * rs);
      a.xr[i] = (f < a.n && k < a.cand.dim) ? a.x_train[(long long)f * a.cand.dim + k] - a.x_train[k] : 0.0;
    } else if (i < n_xr + n_fr) {
      const long long l = i - n_xr;
      const int k = (int)(l % rs);
      const long long of = l / rs;
      const int o = (int)(of / a.fp), f = (int)(of - (long long)o * a.fp);
      double v = 0.0;
      if (f < a.nf) {
        const long long zf = (long long)o * a.nf + f;
        if (k < a.cand.dim) v = (a.z[zf * a.cand.dim + k] / a.ls[o]) * inv_2pi;
        else if (k == a.dimp) v = a.phase[zf] * inv_2pi;
      }
      a.fr[l] = v;
    } else {
      const long long l = i - n_xr - n_fr;
      const int s = (int)(l % a.sp);
      const long long orow = l / a.sp;
      const int o = (int)(orow / (a.fp + a.np)), row = (int)(orow - (long long)o * (a.fp + a.np));
      double v = 0.0;
      if (row < a.nf && s < a.ns) v = a.amp[o] * a.theta[((long long)s * a.n_obj + o) * a.nf + row];
      a.w[l] = v;
    }
  }
}

__device__ __forceinline__ d4 mfma64(double a, double b, d4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// Fence between the last MFMA and the first read of its accumulator (bo_predict_impl.h mfma_fence:
// the wait states of the f64 MFMA supplied inside the asm statement, bo_common.h; the
// accumulators of this translation unit live in AGPRs, hence the "a" constraint)
__device__ __forceinline__ void mfma_fence(d4& x) { asm volatile(BO_NOPS_F64_MFMA : "+a"(x)); }

// ---------------------------------------------------------------------------------------
// The path kernel.  grid (ceil(n_cand / 128), n_obj); a wave owns kTiles tiles of 16 candidates.
// prior_only: the feature rows only and no standardisation (g over the training rows).
// ST = sample tiles of 16 (S padded to 16 ST).
// ---------------------------------------------------------------------------------------
template <int DIMP, int ST>
__global__ __launch_bounds__(kThreads) void ts_paths_kernel(TsArgs a, int prior_only) {
  constexpr int RS = DIMP + 1, SP = 16 * ST;
  constexpr int RC = (kChunkDoubles / (RS + SP)) & ~3;       // rows per staged chunk
  __shared__ double s_rows[RC * RS];
  __shared__ double s_w[RC * SP];
  __shared__ double s_exp[kExpTab];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, cl = lane & 15, kq = lane >> 4;
  const int o = blockIdx.y;
  for (int i = tid; i < kExpTab; i += kThreads) s_exp[i] = exp2((double)i / kExpTab);
  const long long jw = ((long long)blockIdx.x * (kThreads / 64) + wave) * (16 * kTiles);
  double c[kTiles][DIMP];
#pragma unroll
  for (int t = 0; t < kTiles; ++t) {
    const long long j = jw + 16 * t + cl;
#pragma unroll
    for (int k = 0; k < DIMP; ++k) c[t][k] = 0.0;
    if (j < a.cand.n_cand) bo_cand_load<DIMP, true>(a.cand, a.x_train, j, c[t]);
  }
  d4 acc[kTiles][ST];
#pragma unroll
  for (int t = 0; t < kTiles; ++t)
#pragma unroll
    for (int st = 0; st < ST; ++st) acc[t][st] = d4{0.0, 0.0, 0.0, 0.0};
  const double nl2 = a.nl2[o], lpv = a.lpv[o];
  const int n_phase = prior_only ? 1 : 2;
  for (int ph = 0; ph < n_phase; ++ph) {
    const int R = ph == 0 ? a.fp : a.np;
    const double* src_rows = ph == 0 ? a.fr + (long long)o * a.fp * RS : a.xr;
    const double* src_w = a.w + ((long long)o * (a.fp + a.np) + (ph == 0 ? 0 : a.fp)) * SP;
    for (int r0 = 0; r0 < R; r0 += RC) {
      const int rc = R - r0 < RC ? R - r0 : RC;              // a multiple of 4
      __syncthreads();                                        // the previous chunk is consumed
      for (int i = tid; i < rc * RS; i += kThreads) s_rows[i] = src_rows[(long long)r0 * RS + i];
      for (int i = tid; i < rc * SP; i += kThreads) s_w[i] = src_w[(long long)r0 * SP + i];
      __syncthreads();
      if (ph == 0) {
        for (int g = 0; g < rc; g += 4) {
          const double* rp = s_rows + (g + kq) * RS;
          double val[kTiles];
#pragma unroll
          for (int t = 0; t < kTiles; ++t) {
            double tt = rp[DIMP];                             // the argument in turns
#pragma unroll
            for (int k = 0; k < DIMP; ++k) tt = __builtin_fma(rp[k], c[t][k], tt);
            val[t] = cospi(tt + tt);
          }
#pragma unroll
          for (int st = 0; st < ST; ++st) {
            const double b = s_w[(g + kq) * SP + st * 16 + cl];
#pragma unroll
            for (int t = 0; t < kTiles; ++t) acc[t][st] = mfma64(val[t], b, acc[t][st]);
          }
        }
      } else {
        for (int g = 0; g < rc; g += 4) {
          const double* rp = s_rows + (g + kq) * RS;
          double val[kTiles];
#pragma unroll
          for (int t = 0; t < kTiles; ++t) {
            double sq = 0.0;
#pragma unroll
            for (int k = 0; k < DIMP; ++k) {
              const double d = rp[k] - c[t][k];
              sq = __builtin_fma(d, d, sq);
            }
            val[t] = exp2_tab(__builtin_fma(sq, nl2, lpv), s_exp);
          }
#pragma unroll
          for (int st = 0; st < ST; ++st) {
            const double b = s_w[(g + kq) * SP + st * 16 + cl];
#pragma unroll
            for (int t = 0; t < kTiles; ++t) acc[t][st] = mfma64(val[t], b, acc[t][st]);
          }
        }
      }
    }
  }
#pragma unroll
  for (int t = 0; t < kTiles; ++t)
#pragma unroll
    for (int st = 0; st < ST; ++st) mfma_fence(acc[t][st]);
  // C/D map of the f64 MFMA: column (sample) = lane & 15, row (candidate) = (lane >> 4) + 4 reg
  const double spv = a.spv[o];
#pragma unroll
  for (int t = 0; t < kTiles; ++t) {
#pragma unroll
    for (int st = 0; st < ST; ++st) {
      const int s = st * 16 + cl;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const long long j = jw + 16 * t + kq + 4 * reg;
        if (s < a.ns && j < a.cand.n_cand) {
          const double f = acc[t][st][reg];                   // f - pm
          bo_out_store(a.out + ((long long)s * a.n_obj + o) * a.ld + j, prior_only ? f : f / spv);
        }
      }
    }
  }
}

// r = y - pm - g(X) - sqrt(jitter) E, in place over gx [ns][n_obj][n]
__global__ __launch_bounds__(256) void ts_resid_kernel(TsArgs a) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)a.ns * a.n_obj * a.n) return;
  const int f = (int)(i % a.n);
  const int o = (int)((i / a.n) % a.n_obj);
  const double r0 = (a.y[(long long)f * a.ld_y + o] - a.pm[o]) - a.gx[i];
  a.gx[i] = __builtin_fma(-a.sqrt_jitter, a.eps[i], r0);
}

// fixed-order sum over the wave; every lane gets it
__device__ __forceinline__ double wave_sum(double s) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m, 64);
  return s;
}

// v_so = K_o^-1 r_so: grid (ceil(n / kMatRows), n_obj, ceil(ns / kMatSamples)); a wave per row at a
// time, kMatSamples right-hand sides per pass over the row
__global__ __launch_bounds__(256) void ts_matvec_kernel(TsArgs a) {
  const int o = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int s0 = blockIdx.z * kMatSamples;
  const double* K = a.kinv + (long long)o * a.ld_k * a.ld_k;
  const double* r[kMatSamples];
#pragma unroll
  for (int u = 0; u < kMatSamples; ++u) {
    const int s = s0 + u < a.ns ? s0 + u : a.ns - 1;
    r[u] = a.gx + ((long long)s * a.n_obj + o) * a.n;
  }
  for (int rr = 0; rr < kMatRows / 4; ++rr) {
    const int i = blockIdx.x * kMatRows + wave * (kMatRows / 4) + rr;   // wave-uniform
    if (i >= a.n) break;
    const double* row = K + (long long)i * a.ld_k;
    double acc[kMatSamples];
#pragma unroll
    for (int u = 0; u < kMatSamples; ++u) acc[u] = 0.0;
    for (int f = lane; f < a.n; f += 64) {
      const double kv = row[f];
#pragma unroll
      for (int u = 0; u < kMatSamples; ++u) acc[u] = __builtin_fma(kv, r[u][f], acc[u]);
    }
#pragma unroll
    for (int u = 0; u < kMatSamples; ++u) {
      const double v = wave_sum(acc[u]);
      const int s = s0 + u;
      if (lane == 0 && s < a.ns) {
        a.w[((long long)o * (a.fp + a.np) + a.fp + i) * a.sp + s] = v;
        if (a.weights_out) a.weights_out[((long long)s * a.n_obj + o) * a.n + i] = v;
      }
    }
  }
}

template <int DIMP>
hipError_t launch_paths(const TsArgs& a, int prior_only, hipStream_t s) {
  const dim3 grid((unsigned)((a.cand.n_cand + kCandPerBlock - 1) / kCandPerBlock), (unsigned)a.n_obj);
  switch (a.sp / 16) {
    case 1: hipLaunchKernelGGL((ts_paths_kernel<DIMP, 1>), grid, dim3(kThreads), 0, s, a, prior_only); break;
    case 2: hipLaunchKernelGGL((ts_paths_kernel<DIMP, 2>), grid, dim3(kThreads), 0, s, a, prior_only); break;
    default: hipLaunchKernelGGL((ts_paths_kernel<DIMP, 3>), grid, dim3(kThreads), 0, s, a, prior_only); break;
  }
  return hipGetLastError();
}

hipError_t launch_paths_dim(const TsArgs& a, int prior_only, hipStream_t s) {
  switch (a.dimp) {
    case 2: return launch_paths<2>(a, prior_only, s);
    case 4: return launch_paths<4>(a, prior_only, s);
    case 6: return launch_paths<6>(a, prior_only, s);
    default: return launch_paths<8>(a, prior_only, s);
  }
}

// Workspace layout (every region 256-byte aligned); false on bad arguments
struct Layout {
  size_t xr, fr, w, gx, total;
  int dimp, np, fp, sp;
};

size_t align256(size_t b) { return (b + 255) / 256 * 256; }

bool finite_d(double v) { return v == v && v > -__builtin_inf() && v < __builtin_inf(); }

bool make_layout(const bo_ts_desc* d, Layout* L) {
  if (!d) return false;
  if (d->n_obj < 1 || d->n_obj > BO_MAX_OBJ || d->dim < 1 || d->dim > BO_MAX_DIM) return false;
  if (d->n_train < 1 || d->n_train > kMaxTrain || d->ld_k < d->n_train || d->ld_y < d->n_obj) return false;
  if (d->n_samples < 1 || d->n_samples > BO_MAX_TOPQ) return false;
  if (d->n_features < 1 || d->n_features > kMaxFeatures) return false;
  if (d->n_cand < 1 || d->n_cand > (1LL << 36) || d->cand_offset < 0 || d->cand_offset > (1LL << 62) ||
      d->ld < d->n_cand)
    return false;
  if (!bo_cand_check(bo_cand_desc(d))) return false;
  for (int o = 0; o < d->n_obj; ++o) {
    if (!(d->prior_var[o] > 0.0) || !(d->prior_var[o] < __builtin_inf())) return false;
    if (!(d->length_scale[o] * d->length_scale[o] > 0.0)) return false;
    if (!finite_d(d->prior_mean[o])) return false;
  }
  if (!(d->jitter >= 0.0) || !(d->jitter < __builtin_inf())) return false;
  const size_t n = (size_t)d->n_train, no = (size_t)d->n_obj, ns = (size_t)d->n_samples;
  L->dimp = (d->dim + 1) & ~1;
  L->np = (int)((d->n_train + 3) & ~3LL);
  L->fp = (int)((d->n_features + 3) & ~3LL);
  L->sp = (d->n_samples + 15) & ~15;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t at = off; off += align256(bytes); return at; };
  L->xr = take((size_t)L->np * (L->dimp + 1) * 8);
  L->fr = take(no * L->fp * (L->dimp + 1) * 8);
  L->w = take(no * ((size_t)L->fp + L->np) * L->sp * 8);
  L->gx = take(ns * no * n * 8);
  L->total = off;
  return true;
}

}  // namespace

extern "C" {

size_t bo_sample_paths_workspace_size(const bo_ts_desc* d) {
  Layout L;
  if (!make_layout(d, &L)) return 0;
  return L.total;
}

int bo_sample_paths(const bo_ts_desc* d, void* ws, size_t ws_bytes, void* stream) {
  Layout L;
  if (!make_layout(d, &L)) return BO_ERR_ARG;
  if (!d->x_train || !d->y || !d->kinv || !d->z || !d->phase || !d->theta || !d->eps || !d->paths)
    return BO_ERR_ARG;
  if (d->cand_kind != BO_CAND_GRID && !d->cand) return BO_ERR_ARG;
  if (!ws || ws_bytes < L.total) return BO_ERR_WORKSPACE;
  if (((uintptr_t)ws & 15) != 0) return BO_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  // the two point sets of the path kernel: the training rows as explicit candidates (g(X)), and
  // the caller's shard -- a bad Sobol descriptor fails here, before the first launch
  CandArgs train, shard;
  (void)bo_cand_fill(&train, CandDesc{BO_CAND_F64, d->x_train, nullptr, nullptr, d->dim, 0, d->n_train});
  const int st_shard = bo_cand_fill(&shard, bo_cand_desc(d));
  if (st_shard != BO_OK) return st_shard;
  TsArgs a;
  memset(&a, 0, sizeof(a));
  a.n_obj = d->n_obj;
  a.dimp = L.dimp;
  a.n = (int)d->n_train;
  a.np = L.np;
  a.nf = (int)d->n_features;
  a.fp = L.fp;
  a.ns = d->n_samples;
  a.sp = L.sp;
  a.ld_k = d->ld_k;
  a.ld_y = d->ld_y;
  a.x_train = d->x_train;
  a.y = d->y;
  a.kinv = d->kinv;
  a.z = d->z;
  a.phase = d->phase;
  a.theta = d->theta;
  a.eps = d->eps;
  a.cand = train;
  for (int o = 0; o < d->n_obj; ++o) {
    const double ls = d->length_scale[o];
    a.nl2[o] = -0.5 / (ls * ls) * 1.4426950408889634;        // the predict's exponent, base 2
    a.lpv[o] = log2(d->prior_var[o]);
    a.spv[o] = sqrt(d->prior_var[o]);
    a.amp[o] = sqrt(2.0 * d->prior_var[o] / (double)d->n_features);
    a.pm[o] = d->prior_mean[o];
    a.ls[o] = ls;
  }
  a.sqrt_jitter = sqrt(d->jitter);
  char* base = (char*)ws;
  a.xr = (double*)(base + L.xr);
  a.fr = (double*)(base + L.fr);
  a.w = (double*)(base + L.w);
  a.gx = (double*)(base + L.gx);
  a.weights_out = d->weights_out;

  const long long prep_items = (long long)a.np * (a.dimp + 1) + (long long)a.n_obj * a.fp * (a.dimp + 1) +
                               (long long)a.n_obj * (a.fp + a.np) * a.sp;
  long long prep_blocks = (prep_items + 255) / 256;
  if (prep_blocks > 65536) prep_blocks = 65536;              // grid-stride beyond
  hipLaunchKernelGGL(ts_prep_kernel, dim3((unsigned)prep_blocks), dim3(256), 0, s, a);
  BO_CHECK_HIP(hipGetLastError());

  // g(X): the prior part over the training rows
  a.ld = d->n_train;
  a.out = a.gx;
  BO_CHECK_HIP(launch_paths_dim(a, 1, s));
  const long long n_r = (long long)a.ns * a.n_obj * a.n;
  hipLaunchKernelGGL(ts_resid_kernel, dim3((unsigned)((n_r + 255) / 256)), dim3(256), 0, s, a);
  BO_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(ts_matvec_kernel,
                     dim3((unsigned)((a.n + kMatRows - 1) / kMatRows), (unsigned)a.n_obj,
                          (unsigned)((a.ns + kMatSamples - 1) / kMatSamples)),
                     dim3(256), 0, s, a);
  BO_CHECK_HIP(hipGetLastError());

  // the candidates
  a.cand = shard;
  a.ld = d->ld;
  a.out = d->paths;
  BO_CHECK_HIP(launch_paths_dim(a, 0, s));
  return BO_OK;
}

}  // extern "C"
