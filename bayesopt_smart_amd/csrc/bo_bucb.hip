// Batch selection by hallucinated observations (GP-BUCB) on the device: bo_select_batch_bucb.
//
// NOT in the reference.  It extends select_next_batch (bayesopt/acquisition.py:116-144), which
// takes the q best values of one acquisition array: here every pick after the first is taken
// from the summed UCB recomputed with the variance conditioned on the earlier picks
// (include/bo_amd.h states the definition; DESIGN.md §10 the layout and the measurements).
//
// The update is the "augmented weights" form.  With w_r = K^-1 k(X, c_{p_r}) and
// cov0(j, p) = k(c_j, c_p) - k_j . w_p, the recursion c_t[j] = cov0(j, p_t) - sum_{s<t} c_s[j]
// c_s[p_t] / d_s is linear in the columns cov0(., p_r): c_t[j] = sum_{r<=t} A[t][r] cov0(j, p_r),
// A unit lower triangular.  So v_t[j] = c_t[j] / sqrt(d_t) is ONE contraction of the N + t + 1
// kernel values of candidate j against [X; c_{p_0} .. c_{p_t}] with the weight vector
//   u[f] = -sum_r A[t][r] w_r[f] / sqrt(d_t)  (f < N),    u[N + r] = A[t][r] / sqrt(d_t):
// no candidate-sized workspace beyond the running variance (the stored-v form needs (q - 1) n_obj
// n_cand doubles).  Per pick, all on the stream, nothing read back by the host:
//   pick    1 workgroup   fixed-order reduction of the per-workgroup bests to p_t; records it,
//                         sets its bit in the call's copy of the mask, generates k_o(X, c_{p_t})
//   matvec  N/16 x n_obj  w_t = K^-1 k (a wave per row, lanes stride the row, xor tree)
//   coef    n_obj         cov0(p_t, p_r) for r <= t, row t of A, d_t, the weight vector u
//   cand    n_cand/256    the hot path: every candidate generates its N + t + 1 kernel values
//                         (coordinates centred on training row 0, exp2 by the predict's table
//                         form), contracts them with u staged in LDS (broadcast reads), updates
//                         its variance, recomputes the summed UCB and feeds the workgroup's best
// The squared distance is shared by the objectives; one thread owns one candidate and adds its
// terms in row order, so every result is independent of the workgroup scheduling.
// The kernels live in bo_bucb_impl.h, which bo_kb.hip includes as well.
#include "bo_bucb_impl.h"

extern "C" {

size_t bo_select_batch_bucb_workspace_size(const bo_bucb_desc* d) {
  Layout L;
  if (!d || !make_layout(d, bo_cand_desc(d), &L)) return 0;
  return L.total;
}

int bo_select_batch_bucb(const bo_bucb_desc* d, void* ws, size_t ws_bytes, void* stream) {
  Layout L;
  if (!d || !make_layout(d, bo_cand_desc(d), &L)) return BO_ERR_ARG;
  if (!d->x_train || !d->kinv || !d->std_mu || !d->var || !d->top_val || !d->top_idx) return BO_ERR_ARG;
  if (d->cand_kind != BO_CAND_GRID && !d->cand) return BO_ERR_ARG;
  if (d->var_out == d->var || d->var_out == d->std_mu) return BO_ERR_ARG;   // the inputs stay as they are
  if (!ws || ws_bytes < L.total) return BO_ERR_WORKSPACE;
  if (((uintptr_t)ws & 15) != 0) return BO_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  BucbArgs a;
  const int st = fill_args(d, bo_cand_desc(d), L, ws, &a);
  if (st != BO_OK) return st;
  const int st0 = start_call(a, d->mask, s);
  if (st0 != BO_OK) return st0;
  const unsigned blocks = (unsigned)L.blocks;
  const int q = d->q;
  BO_CHECK_HIP(launch_cand_dim(a, -1, kSelect | (q == 1 ? kWriteAcq : 0), blocks, s));
  for (int t = 0; t < q; ++t) {
    const bool last = t == q - 1;
    const bool update = !last || d->var_out != nullptr;      // the last update only feeds var_out
    hipLaunchKernelGGL(bucb_pick_kernel, dim3(1), dim3(1024), 0, s, a, t, (long long)L.blocks, update ? 1 : 0);
    BO_CHECK_HIP(hipGetLastError());
    if (!update) break;
    const int stw = launch_weights(a, t, s);
    if (stw != BO_OK) return stw;
    BO_CHECK_HIP(launch_cand_dim(a, t, last ? 0 : (kSelect | (t == q - 2 ? kWriteAcq : 0)), blocks, s));
  }
  return BO_OK;
}

}  // extern "C"
