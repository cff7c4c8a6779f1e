// Grid-convolution predict path: the posterior over a 2-D integer grid whose
// training points are grid points, with the variance's quadratic form regrouped over the
// MIDPOINTS of the training pairs.  For a candidate (i, j) and training points (r_n, c_n):
//
//   k_n k_m = pv^2 exp(-|x_n - x_m|^2 / 4l^2) E(2i - (r_n + r_m)) E(2j - (c_n + c_m)),
//   E(t) = exp(-t^2 / 4l^2)            [(i-a)^2 + (i-b)^2 = 2 (i - (a+b)/2)^2 + (a-b)^2 / 2]
//
// so with A = sym(K^-1) and w_nm = (2 - delta_nm) pv^2 A_nm exp(-|x_n - x_m|^2 / 4l^2), n <= m:
//
//   T(i, tau)  = sum_{n <= m, c_n + c_m = tau} w_nm E(2i - (r_n + r_m))    pair stage  (VALU)
//   q(i, j)    = sum_tau T(i, tau) E(2j - tau)                              GEMM, K = 2C - 1
//   mu(i, j)   = pm + sum_n [pv alpha_n H(i - r_n)] H(j - c_n)              GEMM, K = N
//   H(t) = exp(-t^2 / 2l^2)
//
// the same N^2 products as k' K^-1 k (update_variance, numba_kernels.py:491-535), grouped so that
// a candidate costs 2 (2C - 1) + 2 N matrix-core flops per objective instead of N^2.
//
// Three launches, each returning at once unless the device flag (predict_prep_kernel) says that
// every training point is a grid point:
//   conv_setup_kernel     integer coordinates; training points bucketed by column (stable
//                         counting sort);
//   conv_pair_kernel      T (one wave per tau) and Tm[n][i] = pv alpha_n H(i - r_n);
//   conv_contract_kernel  the two GEMMs on v_mfma_f64_16x16x4_f64, the epilogue of
//                         cm_predict_kernel, per-wave top-q lists in the TopEntry partial layout.
// No floating-point atomics; every sum runs in an order fixed by the inputs alone, and the K
// order of an output element does not depend on its tile, so shards reproduce the single call.

#include "bo_predict_impl.h"

namespace {

using bo::ConvArgs;

constexpr int kPairChunk = 256;          // pairs of one tau held in LDS at a time (per wave)
constexpr int kTauPerWg = 8;             // waves per workgroup of the pair stage, one tau each
constexpr int kPairThreads = 64 * kTauPerWg;
constexpr int kRowBlock = 16;            // rows per lane and pass of the pair stage
constexpr int kConvPF = 3;               // A-operand prefetch depth of the contraction (k-blocks)

// ---------------------------------------------------------------------------------------
// Setup: rc[n] = integer (row, column) of training point n; cstart / order = the points bucketed
// by column, ascending n inside a bucket.  One workgroup.
// LDS: cnt[C + 1] | col[n] | part[256]
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void conv_setup_kernel(const ConvArgs a) {
  if (__builtin_amdgcn_readfirstlane(*a.flag) != 0) return;
  extern __shared__ __attribute__((aligned(16))) int si[];
  int* cnt = si;
  int* col = cnt + (a.C + 1);
  int* part = col + a.n;
  const int tid = threadIdx.x;
  for (int c = tid; c <= a.C; c += 256) cnt[c] = 0;
  __syncthreads();
  for (int n = tid; n < a.n; n += 256) {
    const int r = (int)(a.x[2 * (long long)n] - (double)a.lo0);
    const int c = (int)(a.x[2 * (long long)n + 1] - (double)a.lo1);
    a.rc[2 * n] = r;
    a.rc[2 * n + 1] = c;
    col[n] = c;
    atomicAdd(cnt + c, 1);
  }
  __syncthreads();
  // exclusive scan of cnt[0 .. C]: contiguous segments per thread, then the 256 partial sums
  const int seg = (a.C + 1 + 255) / 256;
  const int c_lo = tid * seg, c_hi = c_lo + seg < a.C + 1 ? c_lo + seg : a.C + 1;
  int sum = 0;
  for (int c = c_lo; c < c_hi; ++c) sum += cnt[c];
  part[tid] = sum;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const int v = tid >= d ? part[tid - d] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  int run = part[tid] - sum;
  for (int c = c_lo; c < c_hi; ++c) {
    const int v = cnt[c];
    cnt[c] = run;
    a.cstart[c] = run;
    run += v;
  }
  __syncthreads();
  // stable placement: the rank of n among the earlier points of its column
  for (int n = tid; n < a.n; n += 256) {
    const int c = col[n];
    int rank = 0;
    for (int m = 0; m < n; ++m) rank += col[m] == c ? 1 : 0;
    a.order[cnt[c] + rank] = n;
  }
}

// ---------------------------------------------------------------------------------------
// Pair stage.  blockIdx.y = objective; blockIdx.x < tau_blocks: T for kTauPerWg values of tau;
// the blocks after them: Tm.
//
// One tau is one WAVE's (the waves of a workgroup share only the tables; after the tables are
// staged there is no workgroup barrier, so the waves' memory round trips overlap): the pairs
// (n <= m, c_n + c_m = tau) in (n ascending, m in bucket order) order -- lane l owns a contiguous
// range of n, counts its pairs (the partner bucket is column tau - c_n, the m >= n of it), a wave
// scan gives every n its place in the list -- written to the wave's LDS slice kPairChunk at a time
// as (w_nm, table base of r_n + r_m).  The lanes over the rows then accumulate w E(2i - sigma) in
// list order, kRowBlock rows per lane and list read (64 kRowBlock rows per pass over the list;
// the running sums stay in registers across the chunks), with a compensated sum.
// E table, split by parity so that consecutive rows read consecutive doubles:
//   E(2i - sigma) = tabE[par * 2R + i + (s >> 1)],  s = 2R - 2 - sigma,  par = s & 1.
// LDS: tabE[2][2R] | wl[waves][kPairChunk] | cstart[C + 1] | order[n] | rc[2n] | sl[waves][kPairChunk]
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPairThreads) void conv_pair_kernel(const ConvArgs a, int tau_blocks) {
  if (__builtin_amdgcn_readfirstlane(*a.flag) != 0) return;
  const int tid = threadIdx.x, o = blockIdx.y;
  const double nhl = a.nhl[o], pv = a.pv[o];
  if ((int)blockIdx.x >= tau_blocks) {
    // Tm[o][n][i] = pv alpha_n H(i - r_n); rows n >= N are zero
    const long long total = (long long)a.NP * a.ldr;
    const long long stride = (long long)(gridDim.x - tau_blocks) * kPairThreads;
    double* tm = a.Tm + (size_t)o * a.NP * a.ldr;
    for (long long t = (long long)(blockIdx.x - tau_blocks) * kPairThreads + tid; t < total; t += stride) {
      const int n = (int)(t / a.ldr), i = (int)(t - (long long)n * a.ldr);
      double v = 0.0;
      if (n < a.n && i < a.nrows) {
        const double d = (double)(a.row_lo + i - a.rc[2 * n]);
        v = pv * a.alpha[(size_t)o * a.n_pad + n] * exp(nhl * (d * d));
      }
      tm[t] = v;
    }
    return;
  }
  extern __shared__ __attribute__((aligned(16))) double sd[];
  const int R2 = 2 * a.R;
  double* tabE = sd;
  const int lane = tid & 63, wave = tid >> 6;
  double* wl = tabE + 2 * R2 + wave * kPairChunk;
  int* cstart = (int*)(tabE + 2 * R2 + kTauPerWg * kPairChunk);
  int* order = cstart + (a.C + 1);
  int* rc = order + a.n;
  int* sl = rc + 2 * a.n + wave * kPairChunk;
  for (int t = tid; t < 2 * R2; t += kPairThreads) {
    const int par = t >= R2 ? 1 : 0, h = t - par * R2;
    const double m = (double)(2 * h + par - (R2 - 2));
    tabE[t] = exp(0.5 * nhl * (m * m));
  }
  for (int t = tid; t <= a.C; t += kPairThreads) cstart[t] = a.cstart[t];
  for (int t = tid; t < a.n; t += kPairThreads) order[t] = a.order[t];
  for (int t = tid; t < 2 * a.n; t += kPairThreads) rc[t] = a.rc[t];
  __syncthreads();
  const int tau = blockIdx.x * kTauPerWg + wave;
  if (tau >= a.LT) return;
  double* Trow = a.T + ((size_t)o * a.LT + tau) * a.ldr;
  if (tau >= 2 * a.C - 1) {                           // the K padding of the contraction
    for (int i = lane; i < a.ldr; i += 64) Trow[i] = 0.0;
    return;
  }
  const int per = (a.n + 63) / 64;
  const int n_lo = lane * per < a.n ? lane * per : a.n;
  const int n_hi = n_lo + per < a.n ? n_lo + per : a.n;
  const double* ko = a.kinv + (size_t)o * a.ld_k * a.ld_k;
  // this lane's pairs: for each n, the m >= n of column tau - c_n
  int mine = 0;
  for (int n = n_lo; n < n_hi; ++n) {
    const int pc = tau - rc[2 * n + 1];
    if (pc < 0 || pc >= a.C) continue;
    for (int s = cstart[pc]; s < cstart[pc + 1]; ++s) mine += order[s] >= n ? 1 : 0;
  }
  int incl = mine;                                    // inclusive scan over the lanes
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int v = __shfl_up(incl, d, 64);
    if (lane >= d) incl += v;
  }
  const int total = __shfl(incl, 63, 64);
  const int first = incl - mine;
  // (a shard of more than 64 kRowBlock = 1024 rows rebuilds the weight list -- K^-1 loads and exp --
  // once per block of rows: the sums of a block stay in registers over the whole list instead.
  // One block at C3; the cost gate counts the blocks)
  for (int ib = 0; ib < a.ldr; ib += 64 * kRowBlock) {
    // the row sums as unevaluated pairs hi + lo (two-sum and the product's FMA residual): the terms
    // of one T entry cancel to 1e-4 .. 1e-5 of their magnitude (the conditioning of K), and a plain
    // sum's partial sums would leave their rounding in T
    double hi[kRowBlock], lo[kRowBlock];
    int it[kRowBlock];
#pragma unroll
    for (int k = 0; k < kRowBlock; ++k) {
      const int i = ib + lane + 64 * k;
      // rows past the shard's (the padding to ldr) read a valid table entry and are dropped
      it[k] = i < a.nrows ? i : a.nrows - 1;
      hi[k] = 0.0;
      lo[k] = 0.0;
    }
    for (int cb = 0; cb == 0 || cb < total; cb += kPairChunk) {
      const int cnt = total - cb < kPairChunk ? total - cb : kPairChunk;
      int pos = first;
      if (first < cb + cnt && first + mine > cb) {
        for (int n = n_lo; n < n_hi; ++n) {
          const int rn = rc[2 * n], cn = rc[2 * n + 1];
          const int pc = tau - cn;
          if (pc < 0 || pc >= a.C) continue;
          for (int s = cstart[pc]; s < cstart[pc + 1]; ++s) {
            const int m = order[s];
            if (m < n) continue;
            if (pos >= cb && pos < cb + cnt) {
              const int rm = rc[2 * m];
              const double dr = (double)(rn - rm), dc = (double)(cn - pc);
              const double sym = m == n ? ko[(size_t)n * a.ld_k + n]
                                        : ko[(size_t)n * a.ld_k + m] + ko[(size_t)m * a.ld_k + n];
              // (2 - delta) A_nm = K^-1[n][m] + K^-1[m][n] off the diagonal; the library's exp
              wl[pos - cb] = sym * (pv * pv) * exp(0.5 * nhl * (dr * dr + dc * dc));
              const int sp = R2 - 2 - (rn + rm);
              sl[pos - cb] = (sp & 1) * R2 + (sp >> 1) + a.row_lo;
            }
            ++pos;
          }
        }
      }
      // the wave's own LDS slice: written by some lanes, read by all
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      for (int p = 0; p < cnt; ++p) {
        const double w = wl[p];
        const double* e = tabE + sl[p];
#pragma unroll
        for (int k = 0; k < kRowBlock; ++k) {
          // (the rounded intrinsics keep the compiler from contracting the error-free forms)
          const double ev = e[it[k]];
          const double t = __dmul_rn(w, ev);
          const double te = __builtin_fma(w, ev, -t);
          const double s = __dadd_rn(hi[k], t);
          const double bb = __dsub_rn(s, hi[k]);
          const double se = __dadd_rn(__dsub_rn(hi[k], __dsub_rn(s, bb)), __dsub_rn(t, bb));
          hi[k] = s;
          lo[k] = __dadd_rn(lo[k], __dadd_rn(se, te));
        }
      }
      // the slice is rewritten by the next chunk
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
#pragma unroll
    for (int k = 0; k < kRowBlock; ++k) {
      const int i = ib + lane + 64 * k;
      if (i < a.ldr) Trow[i] = i < a.nrows ? hi[k] + lo[k] : 0.0;
    }
  }
}

// ---------------------------------------------------------------------------------------
// Contraction, epilogue and selection.  A wave owns 16 grid rows x 64 columns (4 column blocks:
// 4 accumulators per GEMM); the 4 waves of a workgroup take consecutive wave tiles (the same rows
// when the grid has >= 256 columns: their A loads hit the L1).  Per k-block of 16:
//   A: lane (il = l & 15, g = l >> 4) loads X[k0 + 4g + s][i0 + il], s = 0..3 (X = T or Tm, k-major:
//      16 lanes read 128 contiguous bytes), through a kConvPF-deep register ring;
//   B: MFMA step s pairs lane group g with k = k0 + 4g + s:
//      variance  E(2j - tau) = tabB[par * HB + j + (u >> 1)], u = LT - 1 - tau, par = u & 1
//                (split by parity: consecutive columns read consecutive doubles);
//      mean      H(j - c_n)  = tabH[j - c_n + C - 1].
// LDS: tabB[2][HB] | tabH[Cpad + C] | cn[NP]; rebuilt per objective.
// The k-blocks ascend for every tile alike; the accumulators are read behind mfma_fence.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void conv_load_a(const double* __restrict__ X, int ldr, int kb, int g, double (&v)[4]) {
  const double* p = X + (size_t)(16 * kb + 4 * g) * ldr;
#pragma unroll
  for (int s = 0; s < 4; ++s) v[s] = p[(size_t)s * ldr];
}

// acc[nb] += X[k-blocks][rows] . B; bgen(kb, bv) fills bv[s][nb], this lane's B values of k-block kb
// (k = 16 kb + 4 g + s, column block nb)
template <class BGen>
__device__ __forceinline__ void conv_gemm(const double* __restrict__ X, int ldr, int nkb, int g, d4 (&acc)[4],
                                          BGen&& bgen) {
  double ring[kConvPF][4];
#pragma unroll
  for (int p = 0; p < kConvPF; ++p) conv_load_a(X, ldr, p < nkb ? p : nkb - 1, g, ring[p]);
  for (int kb0 = 0; kb0 < nkb; kb0 += kConvPF) {
#pragma unroll
    for (int p = 0; p < kConvPF; ++p) {
      const int kb = kb0 + p;
      if (kb < nkb) {
        double av[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) av[s] = ring[p][s];
        const int nx = kb + kConvPF;
        conv_load_a(X, ldr, nx < nkb ? nx : nkb - 1, g, ring[p]);
        double bv[4][4];
        bgen(kb, bv);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int nb = 0; nb < 4; ++nb) acc[nb] = mfma64(av[s], bv[s][nb], acc[nb]);
      }
    }
  }
}

__global__ __launch_bounds__(256, 2) void conv_contract_kernel(const ConvArgs a) {
  if (__builtin_amdgcn_readfirstlane(*a.flag) != 0) return;
  extern __shared__ __attribute__((aligned(16))) double sd[];
  const int HB = a.Cpad + a.LT / 2;
  double* tabB = sd;
  double* tabH = tabB + 2 * HB;
  int* cn = (int*)(tabH + (a.Cpad + a.C));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, jl = lane & 15;
  const int cb_n = a.Cpad / 64;                                  // wave tiles along a grid row
  const long long n_wt = (long long)(a.ldr / 16) * cb_n;
  const long long gi_lo = a.cand_offset, gi_hi = a.cand_offset + a.n_cand;
  for (int t = tid; t < a.NP; t += 256) cn[t] = t < a.n ? a.rc[2 * t + 1] : 0;

  double lv = -__builtin_inf();                                  // the wave's top-q list, lanes 0..q-1
  long long li = -1;
  double tab_nhl = __builtin_nan("");                            // length scale of the tables in LDS
  for (long long base = (long long)blockIdx.x * 4; base < n_wt; base += (long long)gridDim.x * 4) {
    const long long wt = base + wave;
    const bool active = wt < n_wt;
    const long long wtc = active ? wt : n_wt - 1;
    const int i0 = (int)(wtc / cb_n) * 16, j0 = (int)(wtc % cb_n) * 64;
    double acq[4][4];
    for (int o = 0; o < a.n_obj; ++o) {
      // the tables depend on the length scale alone: rebuilt only when it changes (one objective,
      // or equal length scales: built once per workgroup; objectives with different length scales
      // on a grid of more wave tiles than 4 gridDim.x rebuild them per tile and objective, since
      // the acquisition sums the objectives of a tile in registers)
      const double nhl = a.nhl[o];
      if (!(nhl == tab_nhl)) {
        __syncthreads();                                         // the previous tables are done with
        for (int t = tid; t < 2 * HB; t += 256) {
          const int par = t >= HB ? 1 : 0, h = t - par * HB;
          const double m = (double)(2 * h + par - (a.LT - 1));
          tabB[t] = exp(0.5 * nhl * (m * m));
        }
        for (int t = tid; t < a.Cpad + a.C; t += 256) {
          const double m = (double)(t - (a.C - 1));
          tabH[t] = exp(nhl * (m * m));
        }
        __syncthreads();
        tab_nhl = nhl;
      }
      d4 aq[4], am[4];
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) {
        aq[nb] = (d4){0.0, 0.0, 0.0, 0.0};
        am[nb] = (d4){0.0, 0.0, 0.0, 0.0};
      }
      const double* Tq = a.T + (size_t)o * a.LT * a.ldr + i0 + jl;
      const double* Tm = a.Tm + (size_t)o * a.NP * a.ldr + i0 + jl;
      // variance: step s of lane group g is tau = 16 kb + 4 g + s; u = LT - 1 - tau is odd for even
      // s, and u >> 1 = hb (s = 0, 1) or hb - 1 (s = 2, 3), hb = LT/2 - 1 - 8 kb - 2 g  (>= 1)
      conv_gemm(Tq, a.ldr, a.LT / 16, g, aq, [&](int kb, double (&bv)[4][4]) {
        const int hb = a.LT / 2 - 1 - 8 * kb - 2 * g;
        const double* pe = tabB + hb + j0 + jl;                  // even u
        const double* po = pe + HB;                              // odd u
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
          bv[0][nb] = po[16 * nb];
          bv[1][nb] = pe[16 * nb];
          bv[2][nb] = po[16 * nb - 1];
          bv[3][nb] = pe[16 * nb - 1];
        }
      });
      conv_gemm(Tm, a.ldr, a.NP / 16, g, am, [&](int kb, double (&bv)[4][4]) {
        const int* c4 = cn + 16 * kb + 4 * g;
        const double* ph = tabH + j0 + jl + (a.C - 1);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const double* p = ph - c4[s];
#pragma unroll
          for (int nb = 0; nb < 4; ++nb) bv[s][nb] = p[16 * nb];
        }
      });
      mfma_fence<false>(aq[0], aq[1]);
      mfma_fence<false>(aq[2], aq[3]);
      mfma_fence<false>(am[0], am[1]);
      mfma_fence<false>(am[2], am[3]);
      const double pv = a.pv[o], pm = a.pm[o];
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          // D rows g + 4r, column jl of column block nb
          const double mu = pm + am[nb][r];                                // :486-488
          const double var = fmax(pv - aq[nb][r], a.min_var);              // :532-535
          const double smu = (mu - pm) * a.inv_rsq_pv[o];                   // :563-565
          const double svar = var * a.inv_pv[o];                            // :568-570
          const double u = smu + a.beta[o] * sqrt(fabs(svar));              // acquisition.py:52
          acq[nb][r] = (o == 0) ? u : acq[nb][r] + u;                       // acquisition.py:108
          const int row = a.row_lo + i0 + g + 4 * r, c = j0 + 16 * nb + jl;
          const long long gi = (long long)row * a.C + c;
          if (active && i0 + g + 4 * r < a.nrows && c < a.C && gi >= gi_lo && gi < gi_hi) {
            const long long off = (long long)o * a.ld_out + (gi - gi_lo);
            if (a.mu) bo_out_store(a.mu + off, mu);
            if (a.var) bo_out_store(a.var + off, var);
            if (a.std_mu) bo_out_store(a.std_mu + off, smu);
            if (a.std_var) bo_out_store(a.std_var + off, svar);
            if (a.ucb) bo_out_store(a.ucb + off, u);
          }
        }
      }
    }
    // global indices of this lane's 16 candidates (-1: outside the shard)
    long long gis[4][4];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = a.row_lo + i0 + g + 4 * r, c = j0 + 16 * nb + jl;
        const long long gi = (long long)row * a.C + c;
        const bool ok = active && i0 + g + 4 * r < a.nrows && c < a.C && gi >= gi_lo && gi < gi_hi;
        gis[nb][r] = ok ? gi : -1;
        if (ok && a.acq) bo_out_store(a.acq + (gi - gi_lo), acq[nb][r]);
      }
    }
    if (a.topq > 0) {
      // the wave's list and the tile's 1024 candidates, merged by rounds of extract-best: each lane
      // offers the best of its remaining candidates (and its list entry), the wave takes the best
      // offer (NaN first, then descending, ties by ascending index); a winner that is an evaluated
      // point (the prep launch's hash set, compared exactly) is dropped and the round repeated.
      // Skipped when no candidate comes before the list's last entry.
      const int q = a.topq;
      const unsigned long long kq = bo_readlane_u(bo_order_key(lv, li), q - 1);
      const long long iq = bo_readlane_i(li, q - 1);
      bool beats = false;
#pragma unroll
      for (int nb = 0; nb < 4; ++nb)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          beats = beats || bo_key_before(bo_order_key(acq[nb][r], gis[nb][r]), gis[nb][r], kq, iq);
      if (__ballot(beats) != 0ull) {
        unsigned int taken = 0;                                  // bit 16: the list entry
        double nv = -__builtin_inf();
        long long ni = -1;
        int filled = 0;
        while (filled < q) {
          unsigned long long bk = 0ull;
          long long bi = -1;
          int bs = -1;
#pragma unroll
          for (int nb = 0; nb < 4; ++nb) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int s = 4 * nb + r;
              const unsigned long long k = ((taken >> s) & 1u) ? 0ull : bo_order_key(acq[nb][r], gis[nb][r]);
              if (bo_key_before(k, gis[nb][r], bk, bi)) { bk = k; bi = gis[nb][r]; bs = s; }
            }
          }
          {
            const unsigned long long k = (lane < q && !((taken >> 16) & 1u)) ? bo_order_key(lv, li) : 0ull;
            if (bo_key_before(k, li, bk, bi)) { bk = k; bi = li; bs = 16; }
          }
          unsigned long long wk = bk;
          long long wi = bi;
#pragma unroll
          for (int m = 32; m > 0; m >>= 1) {
            const unsigned long long ok = __shfl_xor(wk, m, 64);
            const long long oi = __shfl_xor(wi, m, 64);
            if (bo_key_before(ok, oi, wk, wi)) { wk = ok; wi = oi; }
          }
          if (wk == 0ull) break;                                 // nothing left
          const bool win = bk == wk && bi == wi;
          bool excluded = false;
          if (win) {
            taken |= 1u << bs;
            if (bs != 16) {
              const long long row = wi / a.C, c = wi - row * a.C;
              double co[BO_MAX_DIM] = {(double)(a.lo0 + row), (double)(a.lo1 + c), 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
              excluded = bo_hash_contains(a.hkeys, a.hidx, a.hmask, a.excl_pts, 2, co, 2);
            }
          }
          if (__ballot(excluded) != 0ull) continue;
          if (lane == filled) { nv = bo_key_value(wk); ni = wi; }
          ++filled;
        }
        lv = nv;
        li = ni;
      }
    }
  }
  if (a.topq > 0) {
    if (lane < a.topq) {
      TopEntry* dst = a.partial + ((size_t)blockIdx.x * 4 + wave) * a.topq;
      dst[lane].v = lv;
      dst[lane].i = li;
    }
    // the lists of the merge that this grid does not fill
    if (blockIdx.x == 0) {
      const long long e0 = (long long)gridDim.x * 4 * a.topq, e1 = (long long)a.n_lists * a.topq;
      for (long long e = e0 + tid; e < e1; e += 256) {
        a.partial[e].v = -__builtin_inf();
        a.partial[e].i = -1;
      }
    }
  }
}

}  // namespace

namespace bo {

size_t conv_lds_setup(int n, int C) { return ((size_t)(C + 1) + n + 256) * sizeof(int); }

size_t conv_lds_pair(int n, int R, int C) {
  return ((size_t)4 * R + kTauPerWg * kPairChunk) * sizeof(double) +
         ((size_t)(C + 1) + 3 * (size_t)n + kTauPerWg * kPairChunk) * sizeof(int);
}

size_t conv_lds_contract(int n, int C) {
  const size_t Cpad = ((size_t)C + 63) / 64 * 64, LT = ((size_t)2 * C - 1 + 15) / 16 * 16;
  const size_t NP = ((size_t)n + 15) / 16 * 16;
  return (2 * (Cpad + LT / 2) + Cpad + C) * sizeof(double) + NP * sizeof(int);
}

template <class K>
static hipError_t conv_lds_attr(K k, size_t lds) {
  if (lds <= 64 * 1024) return hipSuccess;
  return hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

hipError_t launch_gridconv(const ConvArgs& ca, int grid, hipStream_t st) {
  const size_t l0 = conv_lds_setup(ca.n, ca.C), l1 = conv_lds_pair(ca.n, ca.R, ca.C),
               l2 = conv_lds_contract(ca.n, ca.C);
  hipError_t e;
  if ((e = conv_lds_attr(conv_setup_kernel, l0)) != hipSuccess) return e;
  if ((e = conv_lds_attr(conv_pair_kernel, l1)) != hipSuccess) return e;
  if ((e = conv_lds_attr(conv_contract_kernel, l2)) != hipSuccess) return e;
  hipLaunchKernelGGL(conv_setup_kernel, dim3(1), dim3(256), l0, st, ca);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const int tau_blocks = (ca.LT + kTauPerWg - 1) / kTauPerWg;
  const long long tm_elems = (long long)ca.NP * ca.ldr;
  const int tm_blocks = (int)((tm_elems + 1023) / 1024 < 256 ? (tm_elems + 1023) / 1024 : 256);
  hipLaunchKernelGGL(conv_pair_kernel, dim3(tau_blocks + tm_blocks, ca.n_obj), dim3(kPairThreads), l1, st, ca,
                     tau_blocks);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(conv_contract_kernel, dim3(grid), dim3(256), l2, st, ca);
  return hipGetLastError();
}

}  // namespace bo
