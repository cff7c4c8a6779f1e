// GIBBON batches for an information criterion on the device: bo_select_batch_gibbon
// (include/bo_amd.h states the definition; DESIGN.md §17 the identity, the launches and the
// measurements).
//
// NOT in the reference.  The batch criterion of GIBBON (Moss, Leslie, Gonzalez & Rayson 2021) is
// the sum of the single-point information terms plus, per objective, half the log-determinant of
// the batch's predictive correlation matrix.  Taken greedily, pick t's increment of that
// log-determinant is log(var^(t-1)[j] / var^0[j]) (the Schur complement of the correlation matrix
// of picks 1..t-1 extended by j), so the single-point array `base` is computed ONCE by the caller
// and every further pick costs the hallucinated-observation update of bo_bucb_impl.h plus one log
// per objective.  `base` only ever sees the unconditioned variance.
// Per pick, on the stream, nothing read back by the host -- the launches of bo_select_batch_bucb:
//   pick    1 workgroup   bucb_pick_kernel: p_t from the per-workgroup bests, its mask bit,
//                         k_o(X, c_p) and k_o(c_{p_r}, c_p)
//   matvec, coef          bucb_matvec_kernel, bucb_coef_kernel: the weight vector u
//   cand    n_cand/256    gibbon_cand_kernel below: ONE pass that regenerates the N + t + 1 kernel
//                         values of every candidate, contracts them with u (staged in LDS,
//                         broadcast reads), updates the running variance, adds the penalty to
//                         `base` and feeds the workgroup's best
// bo_bucb_impl.h is included as it is: its kernels are not edited, the candidate pass here is a
// kernel of this translation unit (the K* loop is bucb_cand_kernel's, the epilogue is not), so
// the objects of bo_bucb.hip and bo_kb.hip do not change.
#include "bo_bucb_impl.h"

namespace {

// ---------------------------------------------------------------------------------------
// Candidate pass.  t < 0: the first pass (no update; the running variance starts as `var`, the
// acquisition is `base` itself).  t >= 0: apply pick t's hallucinated observation; with kSelect
// the acquisition is base + 0.5 sum_o log(var_run_o / var_in_o).  kWriteAcq: also store it to
// acq_last.  NOB = objectives padded to 1, 2, 3, 4 or 8 (padded objectives have zero weights).
// The loop over [X; picks] is bucb_cand_kernel's: same staging, same order of the sums.
// ---------------------------------------------------------------------------------------
template <int DIMP, int NOB>
__global__ __launch_bounds__(kThreads) void gibbon_cand_kernel(BucbArgs a, const double* __restrict__ base,
                                                                double* __restrict__ acq_last, int t, int flags) {
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
    double pen = 0.0;                                         // sum_o log(var^t / var^0), o ascending
#pragma unroll
    for (int o = 0; o < NOB; ++o) {
      if (o < a.n_obj) {
        const long long off = (long long)o * a.ld + j;
        const double v0 = a.var_in[off];
        double var = t < 0 ? v0 : a.var_run[off];
        if (t >= 0 && a.ok[o]) var = fmax(var - acc[o] * acc[o], a.min_var);
        a.var_run[off] = var;
        if (t >= 0 && (flags & kSelect) && !(v0 == 0.0)) pen += log(var / v0);
      }
    }
    if (flags & kSelect) {
      acq = base[j];
      if (t >= 0) acq += 0.5 * pen;                           // 0.5 pen is exact: one rounding
    }
  }
  if (flags & kSelect) {
    if (valid && (flags & kWriteAcq) && acq_last) acq_last[j] = acq;
    long long gi = -1;
    if (valid && !((a.mask[j >> 5] >> (j & 31)) & 1u)) gi = a.cand.cand_offset + j;
    const TopEntry b = bo_block_best(acq, gi, s_red);
    if (tid == 0) a.partial[blockIdx.x] = b;
  }
}

template <int DIMP>
hipError_t launch_gibbon(const BucbArgs& a, const double* base, double* acq_last, int t, int flags, unsigned blocks,
                         hipStream_t s) {
  const dim3 g(blocks), b(kThreads);
  switch (a.n_obj) {
    case 1: hipLaunchKernelGGL((gibbon_cand_kernel<DIMP, 1>), g, b, 0, s, a, base, acq_last, t, flags); break;
    case 2: hipLaunchKernelGGL((gibbon_cand_kernel<DIMP, 2>), g, b, 0, s, a, base, acq_last, t, flags); break;
    case 3: hipLaunchKernelGGL((gibbon_cand_kernel<DIMP, 3>), g, b, 0, s, a, base, acq_last, t, flags); break;
    case 4: hipLaunchKernelGGL((gibbon_cand_kernel<DIMP, 4>), g, b, 0, s, a, base, acq_last, t, flags); break;
    default: hipLaunchKernelGGL((gibbon_cand_kernel<DIMP, 8>), g, b, 0, s, a, base, acq_last, t, flags); break;
  }
  return hipGetLastError();
}

hipError_t launch_gibbon_dim(const BucbArgs& a, const double* base, double* acq_last, int t, int flags,
                             unsigned blocks, hipStream_t s) {
  switch (a.dimp) {
    case 2: return launch_gibbon<2>(a, base, acq_last, t, flags, blocks, s);
    case 4: return launch_gibbon<4>(a, base, acq_last, t, flags, blocks, s);
    case 6: return launch_gibbon<6>(a, base, acq_last, t, flags, blocks, s);
    default: return launch_gibbon<8>(a, base, acq_last, t, flags, blocks, s);
  }
}

// the update's fields of `d` (bo_bucb_impl.h takes the candidates as bo_cand_desc(d))
bo_bucb_desc update_desc(const bo_gibbon_desc* d) {
  bo_bucb_desc b;
  memset(&b, 0, sizeof(b));
  b.n_obj = d->n_obj;
  b.n_train = d->n_train;
  b.x_train = d->x_train;
  b.kinv = d->kinv;
  b.ld_k = d->ld_k;
  b.q = d->q;
  for (int o = 0; o < BO_MAX_OBJ; ++o) {
    b.prior_var[o] = d->prior_var[o];
    b.length_scale[o] = d->length_scale[o];
  }
  b.jitter = d->jitter;
  b.min_variance = d->min_variance;
  b.var = d->var;
  b.ld = d->ld;
  b.mask = d->mask;
  b.top_val = d->top_val;
  b.top_idx = d->top_idx;
  b.var_out = d->var_out;
  return b;
}

}  // namespace

extern "C" {

size_t bo_select_batch_gibbon_workspace_size(const bo_gibbon_desc* d) {
  Layout L;
  if (!d) return 0;
  const bo_bucb_desc b = update_desc(d);
  if (!make_layout(&b, bo_cand_desc(d), &L)) return 0;
  return L.total;
}

int bo_select_batch_gibbon(const bo_gibbon_desc* d, void* ws, size_t ws_bytes, void* stream) {
  Layout L;
  if (!d) return BO_ERR_ARG;
  const bo_bucb_desc b = update_desc(d);
  if (!make_layout(&b, bo_cand_desc(d), &L)) return BO_ERR_ARG;
  if (!d->x_train || !d->kinv || !d->base || !d->var || !d->top_val || !d->top_idx) return BO_ERR_ARG;
  if (d->cand_kind != BO_CAND_GRID && !d->cand) return BO_ERR_ARG;
  if (d->var_out == d->var || d->var_out == d->base || d->acq_last == d->base || d->acq_last == d->var)
    return BO_ERR_ARG;                                        // the inputs stay as they are
  if (d->var_out && d->acq_last == d->var_out) return BO_ERR_ARG;
  if (!ws || ws_bytes < L.total) return BO_ERR_WORKSPACE;
  if (((uintptr_t)ws & 15) != 0) return BO_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  BucbArgs a;
  const int st = fill_args(&b, bo_cand_desc(d), L, ws, &a);
  if (st != BO_OK) return st;
  const int st0 = start_call(a, d->mask, s);
  if (st0 != BO_OK) return st0;
  const unsigned blocks = (unsigned)L.blocks;
  const int q = d->q;
  BO_CHECK_HIP(launch_gibbon_dim(a, d->base, d->acq_last, -1, kSelect | (q == 1 ? kWriteAcq : 0), blocks, s));
  for (int t = 0; t < q; ++t) {
    const bool last = t == q - 1;
    const bool update = !last || d->var_out != nullptr;      // the last update only feeds var_out
    hipLaunchKernelGGL(bucb_pick_kernel, dim3(1), dim3(1024), 0, s, a, t, (long long)L.blocks, update ? 1 : 0);
    BO_CHECK_HIP(hipGetLastError());
    if (!update) break;
    const int stw = launch_weights(a, t, s);
    if (stw != BO_OK) return stw;
    BO_CHECK_HIP(launch_gibbon_dim(a, d->base, d->acq_last, t, last ? 0 : (kSelect | (t == q - 2 ? kWriteAcq : 0)),
                                   blocks, s));
  }
  return BO_OK;
}

}  // extern "C"
