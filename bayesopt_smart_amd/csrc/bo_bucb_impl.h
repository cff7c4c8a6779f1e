// The kernels, the workspace layout and the argument block of the hallucinated-observation
// update (bo_bucb.hip states the formulation), shared by the translation units that condition the
// variance on a pick: bo_bucb.hip (GP-BUCB) and bo_kb.hip (Kriging believer for the EHVI).  Every
// includer compiles its own copy (anonymous namespace).  The kernels rely on the default
// floating-point contraction: include this header BEFORE bo_ehvi_impl.h, whose
// `#pragma clang fp contract(off)` holds to the end of the translation unit.
#pragma once

#include "bo_cand.h"

#include <math.h>
#include <string.h>

namespace {

constexpr int kThreads = 256;           // candidates per workgroup of the candidate pass
constexpr int kChunkDoubles = 4096;     // LDS doubles of one staged chunk (rows + weights): 32 KiB
constexpr int kMatRows = 16;            // K^-1 rows per workgroup of the mat-vec (4 per wave)
constexpr int kMaxTrain = 65536;

enum { kSelect = 1, kWriteAcq = 2 };

struct BucbArgs {
  int n_obj, dimp, n, q, ldu;       // ldu = n + q: row stride of u
  long long ld, ld_k;
  CandArgs cand;                    // the shard; its points are centred on training row 0
  const double* x_train;
  const double* kinv;
  const double* std_mu;
  const double* var_in;
  double nl2[BO_MAX_OBJ], lpv[BO_MAX_OBJ], beta[BO_MAX_OBJ], inv_pv[BO_MAX_OBJ];
  double jitter, min_var;
  double* xc;            // [n][dimp]  training rows minus row 0
  double* pc;            // [q][dimp]  the picks' coordinates minus row 0
  double* kx;            // [n_obj][n] k_o(X, c_{p_t}) of the current pick
  double* kp;            // [n_obj][q] k_o(c_{p_r}, c_{p_t}), r <= t
  double* wv;            // [n_obj][q][n] w_r
  double* coef;          // [n_obj][q][q] A
  double* dd;            // [n_obj][q] d_s
  double* u;             // [n_obj][ldu]
  int* ok;               // [n_obj] this step's d_t is finite (and a pick exists)
  long long* pick;       // [q] local index of pick t, -1 = none
  unsigned int* mask;    // the call's own mask: the caller's plus the picks
  TopEntry* partial;     // [n_blocks]
  double* var_run;       // [n_obj][ld] running variance (var_out, or workspace)
  double* acq_out;
  double* top_val;
  long long* top_idx;
};

// xc[f][k] = x_train[f][k] - x_train[0][k] (padded coordinates 0)
__global__ __launch_bounds__(256) void bucb_prep_kernel(BucbArgs a) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)a.n * a.dimp) return;
  const int f = (int)(i / a.dimp), k = (int)(i - (long long)f * a.dimp);
  a.xc[i] = k < a.cand.dim ? a.x_train[(long long)f * a.cand.dim + k] - a.x_train[k] : 0.0;
}

// ---------------------------------------------------------------------------------------
// Candidate pass.  t < 0: the first pass (no update; the running variance starts as `var`).
// t >= 0: apply pick t's hallucinated observation.  flags: kSelect = recompute the summed UCB
// and write this workgroup's best entry; kWriteAcq = also write the acquisition to acq_out.
// NOB = objectives padded to 1, 2, 3, 4 or 8 (padded objectives have zero weights).
// ---------------------------------------------------------------------------------------
template <int DIMP, int NOB>
__global__ __launch_bounds__(kThreads) void bucb_cand_kernel(BucbArgs a, int t, int flags) {
  constexpr int RC = (kChunkDoubles / (DIMP + NOB)) & ~3;    // rows per staged chunk
  __shared__ __attribute__((aligned(16))) double s_rows[RC * DIMP];
  __shared__ double s_w[NOB * RC];
  __shared__ double s_exp[kExpTab];
  __shared__ TopEntry s_red[kThreads / 64];
  const int tid = threadIdx.x;
  const long long j = (long long)blockIdx.x * kThreads + tid;
  const bool valid = j < a.cand.n_cand;
  double acc[NOB];
#pragma unroll
  for (int o = 0; o < NOB; ++o) acc[o] = 0.0;

  if (t >= 0) {
    for (int i = tid; i < kExpTab; i += kThreads) s_exp[i] = exp2((double)i / kExpTab);
    double c[DIMP];
#pragma unroll
    for (int k = 0; k < DIMP; ++k) c[k] = 0.0;
    if (valid) bo_cand_load<DIMP, true>(a.cand, a.x_train, j, c);
    double nl2[NOB], lpv[NOB];
#pragma unroll
    for (int o = 0; o < NOB; ++o) {
      nl2[o] = o < a.n_obj ? a.nl2[o] : 0.0;
      lpv[o] = o < a.n_obj ? a.lpv[o] : 0.0;
    }
    const int R = a.n + t + 1;                                // rows of [X; picks 0..t]
    for (int r0 = 0; r0 < R; r0 += RC) {
      const int rc = R - r0 < RC ? R - r0 : RC;
      __syncthreads();                                        // the previous chunk is consumed
      for (int i = tid; i < rc * DIMP; i += kThreads) {
        const int row = r0 + i / DIMP, k = i % DIMP;
        s_rows[i] = row < a.n ? a.xc[(long long)row * DIMP + k] : a.pc[(long long)(row - a.n) * DIMP + k];
      }
      for (int i = tid; i < rc * NOB; i += kThreads) {
        const int o = i / rc, f = i - o * rc;
        s_w[o * RC + f] = o < a.n_obj ? a.u[(long long)o * a.ldu + r0 + f] : 0.0;
      }
      __syncthreads();
      if (valid) {
#pragma unroll 2
        for (int f = 0; f < rc; ++f) {
          const d2* r = (const d2*)(s_rows + f * DIMP);       // one address per wave: broadcast
          double sq = 0.0;
#pragma unroll
          for (int k = 0; k < DIMP / 2; ++k) {
            const d2 x = r[k];
            const double d0 = x.x - c[2 * k], d1 = x.y - c[2 * k + 1];
            sq = __builtin_fma(d0, d0, sq);
            sq = __builtin_fma(d1, d1, sq);
          }
#pragma unroll
          for (int o = 0; o < NOB; ++o)
            acc[o] = __builtin_fma(exp2_tab(__builtin_fma(sq, nl2[o], lpv[o]), s_exp), s_w[o * RC + f], acc[o]);
        }
      }
    }
  }

  double acq = 0.0;
  if (valid) {
#pragma unroll
    for (int o = 0; o < NOB; ++o) {
      if (o < a.n_obj) {
        const long long off = (long long)o * a.ld + j;
        double var = t < 0 ? a.var_in[off] : a.var_run[off];
        if (t >= 0 && a.ok[o]) var = fmax(var - acc[o] * acc[o], a.min_var);
        a.var_run[off] = var;
        if (flags & kSelect) {
          const double svar = var * a.inv_pv[o];                          // standardize_objectives
          const double ucb = a.std_mu[off] + a.beta[o] * sqrt(fabs(svar)); // acquisition.py:52
          acq = (o == 0) ? ucb : acq + ucb;                               // acquisition.py:108
        }
      }
    }
  }
  if (flags & kSelect) {
    if (valid && (flags & kWriteAcq) && a.acq_out) a.acq_out[j] = acq;
    long long gi = -1;
    if (valid && !((a.mask[j >> 5] >> (j & 31)) & 1u)) gi = a.cand.cand_offset + j;
    const TopEntry b = bo_block_best(acq, gi, s_red);
    if (tid == 0) a.partial[blockIdx.x] = b;
  }
}

// ---------------------------------------------------------------------------------------
// Pick t: the best of the per-workgroup entries in selection order (a strict total order, so
// the result does not depend on which thread saw which entry).  Records it; `gen`: also the
// pick's centred coordinates, k_o(X, c_p) and k_o(c_{p_r}, c_p) for the update that follows.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void bucb_pick_kernel(BucbArgs a, int t, long long n_part, int gen) {
  __shared__ TopEntry s_red[16];
  __shared__ double s_c[BO_MAX_DIM];
  const int tid = threadIdx.x;
  double bv = -__builtin_inf();
  long long bi = -1;
  for (long long l = tid; l < n_part; l += blockDim.x) {
    const TopEntry e = a.partial[l];
    if (bo_better(e.v, e.i, bv, bi)) { bv = e.v; bi = e.i; }
  }
  const TopEntry w = bo_block_best(bv, bi, s_red);
  long long p = w.i >= 0 ? w.i - a.cand.cand_offset : -1;
  if (p >= a.cand.n_cand) p = -1;                       // cannot happen: entries come from this shard
  if (tid == 0) {
    a.top_val[t] = p >= 0 ? w.v : -__builtin_inf();
    a.top_idx[t] = p >= 0 ? w.i : -1;
    a.pick[t] = p;
    if (p >= 0) a.mask[p >> 5] |= 1u << (p & 31);
  }
  if (!gen) return;
  if (tid == 0) {
    double c[BO_MAX_DIM];
    if (p >= 0) bo_cand_load<BO_MAX_DIM, true>(a.cand, a.x_train, p, c);
    for (int k = 0; k < BO_MAX_DIM; ++k) s_c[k] = p >= 0 ? c[k] : 0.0;
    for (int k = 0; k < a.dimp; ++k) a.pc[(long long)t * a.dimp + k] = s_c[k];
  }
  __syncthreads();
  const long long nk = (long long)a.n_obj * a.n;
  for (long long i = tid; i < nk; i += blockDim.x) {
    const int o = (int)(i / a.n), f = (int)(i - (long long)o * a.n);
    double sq = 0.0;
    for (int k = 0; k < a.dimp; ++k) {
      const double d = a.xc[(long long)f * a.dimp + k] - s_c[k];
      sq = __builtin_fma(d, d, sq);
    }
    a.kx[i] = p >= 0 ? exp2(__builtin_fma(sq, a.nl2[o], a.lpv[o])) : 0.0;
  }
  for (int i = tid; i < a.n_obj * (t + 1); i += blockDim.x) {
    const int o = i / (t + 1), r = i - o * (t + 1);
    double sq = 0.0;
    if (r < t)
      for (int k = 0; k < a.dimp; ++k) {
        const double d = a.pc[(long long)r * a.dimp + k] - s_c[k];
        sq = __builtin_fma(d, d, sq);
      }
    a.kp[o * a.q + r] = p >= 0 ? exp2(__builtin_fma(sq, a.nl2[o], a.lpv[o])) : 0.0;
  }
}

// fixed-order sum over the wave; every lane gets it
__device__ __forceinline__ double wave_sum(double s) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m, 64);
  return s;
}

// w_t = K_o^-1 k_o(X, c_{p_t}): grid (ceil(n / kMatRows), n_obj), one wave per row at a time
__global__ __launch_bounds__(256) void bucb_matvec_kernel(BucbArgs a, int t) {
  const int o = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double* kxo = a.kx + (long long)o * a.n;
  const double* K = a.kinv + (long long)o * a.ld_k * a.ld_k;
  double* w = a.wv + ((long long)o * a.q + t) * a.n;
  for (int rr = 0; rr < kMatRows / 4; ++rr) {
    const int i = blockIdx.x * kMatRows + wave * (kMatRows / 4) + rr;   // wave-uniform
    if (i >= a.n) break;
    const double* row = K + (long long)i * a.ld_k;
    double s = 0.0;
    for (int f = lane; f < a.n; f += 64) s = __builtin_fma(row[f], kxo[f], s);
    s = wave_sum(s);
    if (lane == 0) w[i] = s;
  }
}

// Row t of A, d_t and the weight vector u of objective blockIdx.x
__global__ __launch_bounds__(256) void bucb_coef_kernel(BucbArgs a, int t) {
  __shared__ double s_e[BO_MAX_TOPQ], s_a[BO_MAX_TOPQ];
  __shared__ double s_scale;
  __shared__ int s_ok;
  const int o = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double* kxo = a.kx + (long long)o * a.n;
  const double* wo = a.wv + (long long)o * a.q * a.n;
  // e[r] = cov0(p_t, p_r) = k(c_{p_t}, c_{p_r}) - k(X, c_{p_t}) . w_r
  for (int r = wave; r <= t; r += 4) {
    const double* wr = wo + (long long)r * a.n;
    double s = 0.0;
    for (int f = lane; f < a.n; f += 64) s = __builtin_fma(kxo[f], wr[f], s);
    s = wave_sum(s);
    if (lane == 0) s_e[r] = a.kp[o * a.q + r] - s;
  }
  __syncthreads();
  if (tid == 0) {
    double* A = a.coef + (long long)o * a.q * a.q;
    double* d = a.dd + o * a.q;
    for (int r = 0; r <= t; ++r) s_a[r] = r == t ? 1.0 : 0.0;
    double ctt = s_e[t];                                     // c_t[p_t]
    for (int s = 0; s < t; ++s) {
      const double* As = A + s * a.q;
      double cs = 0.0;                                       // c_s[p_t]
      for (int r = 0; r <= s; ++r) cs = __builtin_fma(As[r], s_e[r], cs);
      const double g = cs / d[s];
      for (int r = 0; r <= s; ++r) s_a[r] = __builtin_fma(-g, As[r], s_a[r]);
      ctt = __builtin_fma(-cs, g, ctt);                      // - v_s[p_t]^2
    }
    const double dt = fmax(ctt, 0.0) + a.jitter;
    const bool fin = a.pick[t] >= 0 && ctt == ctt && dt > 0.0 && dt < __builtin_inf();
    // a step that is left out (no pick, or d_t not finite) contributes nothing to later steps
    for (int r = 0; r <= t; ++r) A[t * a.q + r] = fin ? s_a[r] : 0.0;
    d[t] = fin ? dt : 1.0;
    s_scale = fin ? 1.0 / sqrt(dt) : 0.0;
    s_ok = fin ? 1 : 0;
    a.ok[o] = s_ok;
  }
  __syncthreads();
  const bool fin = s_ok != 0;
  const double sc = s_scale;
  double* uo = a.u + (long long)o * a.ldu;
  for (int f = tid; f < a.n; f += blockDim.x) {
    double s = 0.0;
    for (int r = 0; r <= t; ++r) s = __builtin_fma(s_a[r], wo[(long long)r * a.n + f], s);
    uo[f] = fin ? -sc * s : 0.0;
  }
  for (int r = tid; r <= t; r += blockDim.x) uo[a.n + r] = fin ? sc * s_a[r] : 0.0;
}

template <int DIMP>
hipError_t launch_cand(const BucbArgs& a, int t, int flags, unsigned blocks, hipStream_t s) {
  switch (a.n_obj) {
    case 1: hipLaunchKernelGGL((bucb_cand_kernel<DIMP, 1>), dim3(blocks), dim3(kThreads), 0, s, a, t, flags); break;
    case 2: hipLaunchKernelGGL((bucb_cand_kernel<DIMP, 2>), dim3(blocks), dim3(kThreads), 0, s, a, t, flags); break;
    case 3: hipLaunchKernelGGL((bucb_cand_kernel<DIMP, 3>), dim3(blocks), dim3(kThreads), 0, s, a, t, flags); break;
    case 4: hipLaunchKernelGGL((bucb_cand_kernel<DIMP, 4>), dim3(blocks), dim3(kThreads), 0, s, a, t, flags); break;
    default: hipLaunchKernelGGL((bucb_cand_kernel<DIMP, 8>), dim3(blocks), dim3(kThreads), 0, s, a, t, flags); break;
  }
  return hipGetLastError();
}

hipError_t launch_cand_dim(const BucbArgs& a, int t, int flags, unsigned blocks, hipStream_t s) {
  switch (a.dimp) {
    case 2: return launch_cand<2>(a, t, flags, blocks, s);
    case 4: return launch_cand<4>(a, t, flags, blocks, s);
    case 6: return launch_cand<6>(a, t, flags, blocks, s);
    default: return launch_cand<8>(a, t, flags, blocks, s);
  }
}

// Workspace layout (every region 256-byte aligned); false on bad arguments
struct Layout {
  size_t xc, pc, kx, kp, wv, coef, dd, u, ok, pick, mask, partial, var, total;
  long long blocks;
  int dimp;
};

size_t align256(size_t b) { return (b + 255) / 256 * 256; }

// d: the update's fields; c: the candidates (bo_cand_desc of the caller's own descriptor, which
// for bo_kb.hip is not `d`: d's candidate fields and d->dim are not read)
bool make_layout(const bo_bucb_desc* d, const CandDesc& c, Layout* L) {
  if (d->n_obj < 1 || d->n_obj > BO_MAX_OBJ || c.dim < 1 || c.dim > BO_MAX_DIM) return false;
  if (d->n_train < 1 || d->n_train > kMaxTrain || d->ld_k < d->n_train) return false;
  if (d->q < 1 || d->q > BO_MAX_TOPQ) return false;
  if (c.count < 1 || c.count > (1LL << 38) || c.offset < 0 || c.offset > (1LL << 62) || d->ld < c.count)
    return false;
  if (!bo_cand_check(c)) return false;
  for (int o = 0; o < d->n_obj; ++o) {
    if (!(d->prior_var[o] > 0.0) || !(d->prior_var[o] < __builtin_inf())) return false;
    if (!(d->length_scale[o] * d->length_scale[o] > 0.0)) return false;
    if (d->beta[o] != d->beta[o]) return false;
  }
  if (!(d->jitter >= 0.0) || !(d->jitter < __builtin_inf()) || !(d->min_variance >= 0.0)) return false;
  const size_t n = (size_t)d->n_train, q = (size_t)d->q, no = (size_t)d->n_obj;
  L->dimp = (c.dim + 1) & ~1;
  L->blocks = (c.count + kThreads - 1) / kThreads;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t at = off; off += align256(bytes); return at; };
  L->xc = take(n * L->dimp * 8);
  L->pc = take(q * L->dimp * 8);
  L->kx = take(no * n * 8);
  L->kp = take(no * q * 8);
  L->wv = take(no * q * n * 8);
  L->coef = take(no * q * q * 8);
  L->dd = take(no * q * 8);
  L->u = take(no * (n + q) * 8);
  L->ok = take(no * 4);
  L->pick = take(q * 8);
  L->mask = take(bo_excl_mask_bytes(c.count));
  L->partial = take((size_t)L->blocks * sizeof(TopEntry));
  L->var = d->var_out ? off : take(no * (size_t)d->ld * 8);   // the running variance
  L->total = off;
  return true;
}

// The kernels' argument block of (d, c) over the workspace `ws` laid out by L (host only; nothing
// is launched).  BO_OK, or the status of a bad Sobol descriptor.
int fill_args(const bo_bucb_desc* d, const CandDesc& c, const Layout& L, void* ws, BucbArgs* out) {
  BucbArgs& a = *out;
  memset(&a, 0, sizeof(a));
  const int st = bo_cand_fill(&a.cand, c);
  if (st != BO_OK) return st;
  a.n_obj = d->n_obj;
  a.dimp = L.dimp;
  a.n = (int)d->n_train;
  a.q = d->q;
  a.ldu = a.n + a.q;
  a.ld = d->ld;
  a.ld_k = d->ld_k;
  a.x_train = d->x_train;
  a.kinv = d->kinv;
  a.std_mu = d->std_mu;
  a.var_in = d->var;
  for (int o = 0; o < d->n_obj; ++o) {
    const double ls = d->length_scale[o];
    a.nl2[o] = -0.5 / (ls * ls) * 1.4426950408889634;        // the predict's exponent, base 2
    a.lpv[o] = log2(d->prior_var[o]);
    a.beta[o] = d->beta[o];
    a.inv_pv[o] = 1.0 / d->prior_var[o];
  }
  a.jitter = d->jitter;
  a.min_var = d->min_variance;
  char* base = (char*)ws;
  a.xc = (double*)(base + L.xc);
  a.pc = (double*)(base + L.pc);
  a.kx = (double*)(base + L.kx);
  a.kp = (double*)(base + L.kp);
  a.wv = (double*)(base + L.wv);
  a.coef = (double*)(base + L.coef);
  a.dd = (double*)(base + L.dd);
  a.u = (double*)(base + L.u);
  a.ok = (int*)(base + L.ok);
  a.pick = (long long*)(base + L.pick);
  a.mask = (unsigned int*)(base + L.mask);
  a.partial = (TopEntry*)(base + L.partial);
  a.var_run = d->var_out ? d->var_out : (double*)(base + L.var);
  a.acq_out = d->acq_out;
  a.top_val = d->top_val;
  a.top_idx = (long long*)d->top_idx;
  return BO_OK;
}

// the call's own mask: the caller's bits (its words over this shard), then the picks; and the
// centred training rows
int start_call(const BucbArgs& a, const uint32_t* mask, hipStream_t s) {
  const size_t mask_words = ((size_t)a.cand.n_cand + 31) / 32;
  if (mask)
    BO_CHECK_HIP(hipMemcpyAsync(a.mask, mask, mask_words * 4, hipMemcpyDeviceToDevice, s));
  else
    BO_CHECK_HIP(hipMemsetAsync(a.mask, 0, mask_words * 4, s));
  hipLaunchKernelGGL(bucb_prep_kernel, dim3((unsigned)(((long long)a.n * a.dimp + 255) / 256)), dim3(256), 0, s, a);
  BO_CHECK_HIP(hipGetLastError());
  return BO_OK;
}

// pick t's update up to the weight vector u: w_t = K^-1 k, then row t of A, d_t and u
int launch_weights(const BucbArgs& a, int t, hipStream_t s) {
  hipLaunchKernelGGL(bucb_matvec_kernel, dim3((unsigned)((a.n + kMatRows - 1) / kMatRows), (unsigned)a.n_obj),
                     dim3(256), 0, s, a, t);
  BO_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(bucb_coef_kernel, dim3((unsigned)a.n_obj), dim3(256), 0, s, a, t);
  BO_CHECK_HIP(hipGetLastError());
  return BO_OK;
}

}  // namespace

