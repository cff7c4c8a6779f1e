/*
 * bo_amd.h — C ABI of the MI355X-native GP-predict + acquisition hot path.
 *
 * Drop-in boundary for alebal123bal/BayesOpt_smart's inner loop
 * (bayesopt/bayesian_optimization.py:129-207, the functions it imports by name at
 * :24-42).  Every entry point names the reference function it replaces.
 *
 * Conventions (all entry points):
 *   - plain pointers and sizes; no torch / HIP types in the signatures;
 *   - "device" pointers are HIP device memory owned by the caller (the library never
 *     allocates or frees caller memory); "host" pointers are read during the call;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); every call is
 *     asynchronous on that stream unless stated otherwise;
 *   - the return value is a bo_status; no C++ exception crosses the ABI.
 *   - all floating point is IEEE binary64 (the reference's NUMBA_FLOAT_TYPE,
 *     bayesopt/config.py:54); the reference's float32 branch (config.py:57-61: jitters 1e-3 /
 *     1e-4, variance floor 1e-6) is reachable through the *_jitter entry points and
 *     BO_PREDICT_F32_FLOOR.
 */
#ifndef BO_AMD_H
#define BO_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BO_ABI_VERSION 5
#define BO_MAX_OBJ 8      /* objectives per call                              */
#define BO_MAX_DIM 8      /* input dimensions                                 */
#define BO_MAX_TOPQ 48    /* batch size of the fused top-q selection          */

typedef enum bo_status {
  BO_OK = 0,
  BO_ERR_ARG = 1,          /* invalid argument / shape                          */
  BO_ERR_UNSUPPORTED = 2,  /* valid but outside what this build implements       */
  BO_ERR_WORKSPACE = 3,    /* workspace missing or too small                     */
  BO_ERR_HIP = 4,          /* a HIP runtime call failed                          */
  BO_ERR_NOT_PD = 5,       /* matrix not positive definite (np.linalg.LinAlgError) */
  BO_ERR_SINGULAR = 6      /* singular matrix (np.linalg.LinAlgError)            */
} bo_status;

typedef enum bo_cand_kind {
  BO_CAND_I64 = 0,   /* explicit candidates, int64 [n_cand][dim] (the reference's input_space) */
  BO_CAND_F64 = 1,   /* explicit candidates, f64 [n_cand][dim] (e.g. a Sobol set)            */
  BO_CAND_GRID = 2,  /* implicit 'ij' integer grid: bayesian_optimization.py:338-340           */
  BO_CAND_SOBOL = 3  /* implicit unscrambled Sobol sequence, generated on the device from the
                        global index: point i of scipy.stats.qmc.Sobol(dim, scramble=False,
                        bits) mapped to lo + u * scale (bit-identical; `cand` is a HOST
                        bo_sobol_desc*, read during the call).  A candidate-shard generates its
                        own index range: no candidate array exists in HBM or crosses PCIe.   */
} bo_cand_kind;

/* Parameters of kind BO_CAND_SOBOL: coordinate k of point i is lo[k] + u_k(i) * scale[k]
 * (multiply, then add: numpy's `lo + sample * (hi - lo)`), u_k(i) = x_k(i) / 2^bits with
 * x_k(i) = XOR of the direction numbers v_kj over the set bits j of gray(i) = i ^ (i >> 1)
 * (Joe-Kuo direction numbers, the table scipy ships).  bits in [1, 32]; i < 2^bits. */
typedef struct bo_sobol_desc {
  int32_t bits;
  int32_t reserved;
  double lo[BO_MAX_DIM];
  double scale[BO_MAX_DIM];
} bo_sobol_desc;

/* HOST (no device, synchronous): coordinates out[t][k] (t < n, k < dim) of the Sobol points with
 * global indices idx[t], bit-identical to the device generator; the direction numbers
 * v[dim][bits] (uint32, row-major). */
int bo_sobol_points(const bo_sobol_desc* s, int32_t dim, const int64_t* idx, int64_t n, double* out);
int bo_sobol_direction_numbers(int32_t dim, int32_t bits, uint32_t* out);

int bo_abi_version(void);
const char* bo_status_string(int status);
/* number of HIP devices visible; <0 on HIP error (no compute launched) */
int bo_device_count(void);

/* ------------------------------------------------------------------------------------
 * Fused GP predict + acquisition + top-q:   replaces, for one candidate shard,
 *   update_k_star     bayesopt/numba_kernels.py:406-442
 *   update_mean       bayesopt/numba_kernels.py:450-488
 *   update_variance   bayesopt/numba_kernels.py:491-535
 *   standardize_objectives                 :538-570
 *   update_ucb        bayesopt/acquisition.py:55-81
 *   update_hypervolume_improvement         bayesopt/acquisition.py:89-108
 *   select_next_batch bayesopt/acquisition.py:116-144 (local top-q with exclusion)
 * No N x M k_star array is materialised: candidate tiles are generated, contracted
 * against K^-1 on the f64 matrix cores and reduced to outputs in one pass.
 * ---------------------------------------------------------------------------------- */
/* Variance formulation.  DENSE: q = k^T (K^-1 k) exactly as update_variance (2N^2 flops per
 * candidate and objective).  AUTO (default): q = 2 k^T (U k) with U the upper triangle of
 * sym(K^-1) = (K^-1 + K^-T)/2 and its diagonal halved -- the same quadratic form (k^T A k =
 * k^T sym(A) k), half the matrix-core work, no factorisation and no positive-definiteness
 * requirement. */
/* mode is a bit set: BO_PREDICT_DENSE forces the dense formulation; BO_PREDICT_NO_SEPARABLE
 * disables the integer-grid fast K* generation (K* = pv * R(f) * T[x_last - c_last], an exp
 * table over the last grid axis; used only when the candidates are a grid whose last axis is
 * a multiple of 16 and every training point's last coordinate is an integer on that axis,
 * checked on the device).  BO_PREDICT_FP32 (BASELINE config C5, "fp32 with fp64 reference
 * check"): K* and the upper-form contraction in f32 on v_mfma_f32_16x16x4_f32, the mean and
 * quadratic form accumulated in f32, everything after them in f64; every candidate evaluates
 * exp (no grid table); DENSE / NO_SEPARABLE are ignored with it. */
/* BO_PREDICT_F32_FLOOR: the posterior variance floor of the reference's float32 branch,
 * MIN_VARIANCE = 1e-6 (config.py:57-61), instead of the fp64 branch's 1e-10 (:63-66). */
/* Grid convolution (2-D integer grid whose training points are all grid points, checked on the
 * device; AUTO form only): the quadratic form regrouped over the midpoints of the training
 * pairs, q(i, j) = sum_tau T(i, tau) E(2j - tau), 2 (2C - 1) + 2N matrix-core flops per candidate
 * and objective instead of N^2.  Planned when a cost gate passes; BO_PREDICT_GRID_CONV plans it
 * whenever the shape allows, BO_PREDICT_NO_GRID_CONV (or BO_GRID_CONV=0 in the environment)
 * never.  When the device check fails the call runs the chunk-major kernel as before.
 * The path leaves out what cannot reach the result: training pairs with |w_nm| < 2^-100 pv for
 * every objective (q / pv loses less than 1e-24 for N <= 4096), and the k-blocks of the two
 * contractions in which E(2j - tau) < 2^-128 (variance) or H(j - c_n) < 2^-128 (mean) for every
 * column of a 64-column tile (the tables store such entries as +0.0, so a skipped block would
 * have added exact zeros).
 * BO_PREDICT_GRID_CONV_FULL plans the path like BO_PREDICT_GRID_CONV and runs every k-block over
 * the same tables and the same pair list: its outputs are bit for bit those of the banded run
 * whenever K^-1 and alpha are finite (the reference mode of the band's tests).  A non-finite
 * K^-1 entry or alpha_n spreads NaN only to the candidates inside the band around its pair's
 * midpoint column (its point's column), not along the whole grid row as 0 * NaN does where every
 * k-block is run; with BO_PREDICT_GRID_CONV_FULL it still reaches every column. */
typedef enum bo_predict_mode {
  BO_PREDICT_AUTO = 0,
  BO_PREDICT_DENSE = 1,
  BO_PREDICT_NO_SEPARABLE = 2,
  BO_PREDICT_FP32 = 4,
  BO_PREDICT_F32_FLOOR = 8,
  BO_PREDICT_NO_GRID_CONV = 16,
  BO_PREDICT_GRID_CONV = 32,
  BO_PREDICT_GRID_CONV_FULL = 64
} bo_predict_mode;

typedef struct bo_predict_desc {
  int32_t n_obj;              /* objectives (<= BO_MAX_OBJ)                                 */
  int32_t dim;                /* input dimensions (<= BO_MAX_DIM)                            */
  int64_t n_train;            /* N = current_eval                                            */
  const double* x_train;      /* device [n_train][dim] (x_vector[:N])                        */
  const double* y_train;      /* device, y_vector rows with row stride ld_y (>= n_obj)        */
  int64_t ld_y;
  const double* kinv;         /* device [n_obj][ld_k][ld_k]; leading N x N block = invert_k() */
  int64_t ld_k;
  int32_t cand_kind;          /* bo_cand_kind                                                 */
  int32_t mode;               /* bo_predict_mode                                              */
  const void* cand;           /* device [n_cand][dim] (kinds I64/F64); host bo_sobol_desc* (SOBOL) */
  int64_t n_cand;             /* candidates scored by this call                               */
  int64_t cand_offset;        /* global index of this call's first candidate                  */
  int64_t grid_lo[BO_MAX_DIM];     /* kind GRID: lower bound of each axis                    */
  int64_t grid_shape[BO_MAX_DIM];  /* kind GRID: points per axis (axis dim-1 fastest)        */
  const double* excl_points;  /* device [n_excl][dim] evaluated points; NULL = x_train        */
  int64_t n_excl;
  double prior_mean[BO_MAX_OBJ];
  double prior_var[BO_MAX_OBJ];
  double length_scale[BO_MAX_OBJ];
  double beta[BO_MAX_OBJ];
  /* optional device outputs (NULL = not written); per-objective arrays are
   * [n_obj][ld_out] and this call writes columns [0, n_cand) of each row. */
  double* mu;                 /* mu_objectives             */
  double* var;                /* variance_objectives       */
  double* std_mu;             /* std_mu_objectives         */
  double* std_var;            /* std_variance_objectives   */
  double* ucb;                /* ucb                       */
  double* acq;                /* acquisition_values [n_cand] */
  int64_t ld_out;
  /* top-q selection of this call's candidates (0 = none), ordered NaN first, then
   * descending acquisition value, ties by ascending global index; candidates equal to
   * an evaluated point are skipped.  Device outputs. */
  int32_t topq;
  int32_t reserved1;
  double* top_val;            /* [topq]                                          */
  int64_t* top_idx;           /* [topq] global candidate index, -1 = no candidate */
} bo_predict_desc;

/* bytes of device workspace bo_predict_acquire needs for `desc` (0 on bad args) */
size_t bo_predict_workspace_size(const bo_predict_desc* desc);
int bo_predict_acquire(const bo_predict_desc* desc, void* workspace, size_t workspace_bytes,
                       void* stream);

/* ------------------------------------------------------------------------------------
 * Unfused drop-ins with the reference's in-place semantics (device arrays).
 * ---------------------------------------------------------------------------------- */

/* update_k  bayesopt/numba_kernels.py:329-367: kernel_matrix[o][i][j] for
 * last_eval <= i < current_eval, i <= j < current_eval, then mirror.
 * kernel_matrix: device [n_obj][ld][ld]; x: device [*][dim]. prior_variance/length_scales host. */
int bo_update_k(double* kernel_matrix, int64_t ld, int32_t n_obj, const double* x, int32_t dim,
                int64_t last_eval, int64_t current_eval, const double* prior_variance,
                const double* length_scales, void* stream);

/* update_k_star  bayesopt/numba_kernels.py:406-442: k_star device [n_obj][ld_rows][n_cand];
 * candidates: explicit int64/f64 device array (kind I64/F64). Rows [last_eval, current_eval). */
int bo_update_k_star(double* k_star, int64_t ld_rows, int32_t n_obj, const double* x, int32_t dim,
                     int32_t cand_kind, const void* cand, int64_t n_cand, int64_t last_eval,
                     int64_t current_eval, const double* prior_variance,
                     const double* length_scales, void* stream);

/* update_mean + update_variance (numba_kernels.py:450-535) from a materialised k_star
 * (device [n_obj][ld_rows][n_cand]).  mu/var: device [n_obj][n_cand] (either may be NULL). */
int bo_update_mean_variance(double* mu, double* var, const double* k_star, int64_t ld_rows,
                            int32_t n_obj, int64_t n_cand, const double* kinv, int64_t ld_k,
                            const double* y, int64_t ld_y, int64_t current_eval,
                            const double* prior_mean, const double* prior_variance,
                            void* workspace, size_t workspace_bytes, void* stream);
size_t bo_update_mean_variance_workspace_size(int32_t n_obj, int64_t current_eval);

/* standardize_objectives + update_ucb + update_hypervolume_improvement
 * (numba_kernels.py:538-570, acquisition.py:55-108): elementwise over [n_obj][n_cand].
 * Any output may be NULL. */
int bo_standardize_ucb_hvi(double* std_mu, double* std_var, double* ucb, double* acq,
                           const double* mu, const double* var, int32_t n_obj, int64_t n_cand,
                           const double* prior_mean, const double* prior_variance,
                           const double* betas, void* stream);

/* update_ucb  bayesopt/acquisition.py:55-81: ucb[o][i] = mu[o][i] + betas[o] sqrt(|var[o][i]|)
 * (arrays [n_obj][n]; betas host). */
int bo_update_ucb(double* ucb, const double* mu, const double* var, int32_t n_obj, int64_t n,
                  const double* betas, void* stream);

/* update_hypervolume_improvement  bayesopt/acquisition.py:89-108: acq[i] = sum_o ucb[o][i]. */
int bo_update_hypervolume_improvement(double* acq, const double* ucb, int32_t n_obj, int64_t n,
                                      void* stream);

/* select_next_batch  bayesopt/acquisition.py:116-144 over an acquisition array:
 * top-q (q <= BO_MAX_TOPQ) skipping candidates equal to any evaluated point. */
int bo_select_topq(const double* acq, int64_t n_cand, int32_t cand_kind, const void* cand,
                   const int64_t* grid_lo, const int64_t* grid_shape, int32_t dim,
                   int64_t cand_offset, const double* excl_points, int64_t n_excl, int32_t topq,
                   double* top_val, int64_t* top_idx, void* workspace, size_t workspace_bytes,
                   void* stream);
size_t bo_select_topq_workspace_size(int64_t n_cand, int32_t topq);

/* The exclusion of acquisition.py:137-139 ("candidate equal in every coordinate to an evaluated
 * point") as a candidate bit mask, kept across iterations (ABI 5).  The evaluated set grows by
 * q points per iteration, so the mask is built once and then extended by the new rows only.
 *
 * bo_excl_mask_update: sets bit j (word j / 32, bit j % 32) of `mask` (device, bo_excl_mask_bytes
 * (n_cand)) for every local candidate j (global index cand_offset + j) equal to one of the rows
 * excl_points[first_excl .. n_excl) (device [n_excl][dim]); clear != 0 zeroes the mask first.
 * Candidates as bo_select_topq's.  Grid candidates: one thread per point, the grid index found
 * arithmetically.  Other kinds: a hash set of the new rows in `workspace`
 * (bo_excl_mask_workspace_size(n_excl - first_excl) bytes; unused for a grid) and one pass over
 * the candidates.
 * bo_select_topq_masked / bo_hvi_select_topq_masked: bo_select_topq / bo_hvi_select_topq with
 * the mask in place of the points: an excluded element is dropped as it is loaded (no hash build,
 * no probes).  Same results as the unmasked calls given the same evaluated points. */
size_t bo_excl_mask_bytes(int64_t n_cand);
size_t bo_excl_mask_workspace_size(int64_t n_excl);
int bo_excl_mask_update(uint32_t* mask, int64_t n_cand, int32_t cand_kind, const void* cand,
                        const int64_t* grid_lo, const int64_t* grid_shape, int32_t dim,
                        int64_t cand_offset, const double* excl_points, int64_t first_excl,
                        int64_t n_excl, int32_t clear, void* workspace, size_t workspace_bytes,
                        void* stream);
int bo_select_topq_masked(const double* acq, int64_t n_cand, int64_t cand_offset,
                          const uint32_t* mask, int32_t topq, double* top_val, int64_t* top_idx,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Batch selection by hallucinated observations (GP-BUCB; Desautels, Krause & Burdick 2014).
 * NOT in the reference: it extends select_next_batch (bayesopt/acquisition.py:116-144), whose
 * batch is the q best values of ONE acquisition array (on a smooth posterior, q neighbours of
 * one maximum).  Here pick t is the best candidate of the summed standardised UCB
 *   acq_t[j] = sum_o std_mu_o[j] + beta_o sqrt(|var_o^(t-1)[j]| / pv_o)
 * (select_next_batch's order: NaN first, descending value, ties by ascending global index;
 * masked candidates and earlier picks skipped), after which every objective's variance is
 * conditioned on an observation at that pick (the mean does not change):
 *   c_t[j]   = cov0(j, p_t) - sum_{s<t} v_s[j] v_s[p_t],   cov0(j, p) = k(c_j, c_p) - k_j^T K^-1 k_p
 *   d_t      = max(c_t[p_t], 0) + jitter,   v_t = c_t / sqrt(d_t)
 *   var^t[j] = max(var^(t-1)[j] - v_t[j]^2, min_variance)     (unchanged when d_t is not finite)
 * -- the posterior variance of a GP trained on X u {p_1..p_t} with `jitter` on every point.
 * q = 1 is select_next_batch's top-1.  No host synchronisation between the picks: each one
 * stays in device memory, the call is asynchronous on its stream and capturable in a HIP graph;
 * deterministic (fixed-order reductions).  std_mu / var / mask are not modified.
 * Fields shared with bo_predict_desc have its meaning; std_mu / var are that call's outputs. */
typedef struct bo_bucb_desc {
  int32_t n_obj;              /* objectives (<= BO_MAX_OBJ)                                   */
  int32_t dim;                /* input dimensions (<= BO_MAX_DIM)                              */
  int64_t n_train;            /* N >= 1                                                       */
  const double* x_train;      /* device [n_train][dim]                                        */
  const double* kinv;         /* device [n_obj][ld_k][ld_k]; leading N x N block = invert_k() */
  int64_t ld_k;
  int32_t cand_kind;          /* bo_cand_kind                                                 */
  int32_t q;                  /* picks, 1 .. BO_MAX_TOPQ                                      */
  const void* cand;           /* device [n_cand][dim] (kinds I64/F64); host bo_sobol_desc* (SOBOL) */
  int64_t n_cand;             /* candidates of this call (a shard)                            */
  int64_t cand_offset;        /* global index of this call's first candidate                  */
  int64_t grid_lo[BO_MAX_DIM];     /* kind GRID                                              */
  int64_t grid_shape[BO_MAX_DIM];  /* kind GRID (axis dim-1 fastest)                         */
  double prior_var[BO_MAX_OBJ];
  double length_scale[BO_MAX_OBJ];
  double beta[BO_MAX_OBJ];
  double jitter;              /* KERNEL_JITTER added by invert_k: 1e-6 (1e-3 float32 branch)  */
  double min_variance;        /* MIN_VARIANCE: 1e-10 (1e-6 float32 branch)                    */
  const double* std_mu;       /* device [n_obj][ld]: std_mu_objectives                        */
  const double* var;          /* device [n_obj][ld]: variance_objectives (already floored)    */
  int64_t ld;                 /* row stride of std_mu / var / var_out (>= n_cand)             */
  const uint32_t* mask;       /* device, bo_excl_mask_update's layout over this shard; NULL = none */
  double* top_val;            /* device [q]: acq_t[p_t] (-inf when no candidate is left)      */
  int64_t* top_idx;           /* device [q]: global index of pick t, -1 = no candidate left   */
  double* var_out;            /* optional device [n_obj][ld]: var^q                           */
  double* acq_out;            /* optional device [n_cand]: the acquisition pick q was taken from */
} bo_bucb_desc;
/* bytes of device workspace bo_select_batch_bucb needs for `desc` (0 on bad args) */
size_t bo_select_batch_bucb_workspace_size(const bo_bucb_desc* desc);
int bo_select_batch_bucb(const bo_bucb_desc* desc, void* workspace, size_t workspace_bytes,
                         void* stream);

/* ------------------------------------------------------------------------------------
 * Posterior function draws for Thompson-sampling batches: pathwise conditioning (Wilson et al.
 * 2020) over a random-Fourier-feature prior.  NOT in the reference.  Per objective o and draw s,
 * with x0 = training row 0 (the centre the predict uses), l = length_scale, pv = prior_var,
 * pm = prior_mean, D = n_features, N = n_train and the caller's random numbers
 *   Z [n_obj][D][dim], E [S][n_obj][N], Theta [S][n_obj][D]  standard normals,
 *   B [n_obj][D]                                             uniform on [0, 2 pi):
 *   w_oi     = Z_oi / l_o
 *   phi_oi(c) = sqrt(2 pv_o / D) cos(w_oi . (c - x0) + B_oi)          feature i of the prior
 *   g_so(c)  = sum_i Theta_soi phi_oi(c)                               prior draw
 *   r_so     = y_o - pm_o - g_so(X) - sqrt(jitter) E_so                [N]
 *   v_so     = kinv_o r_so                                             [N]
 *   f_so(c)  = pm_o + g_so(c) + sum_n k_o(c, x_n) v_son                the posterior draw
 *   z_so(c)  = (f_so(c) - pm_o) / sqrt(pv_o)                           `paths`, standardised like std_mu
 * For fixed (Z, B) the mean of f over (Theta, E) is exactly the posterior mean
 * pm + k kinv (y - pm); at a training point f_so(x_n) = y_on - sqrt(jitter) E_son - jitter v_son.
 * The call is a deterministic function of its arguments (no random numbers are drawn inside; a
 * workspace of any content gives the same bits), asynchronous on its stream, without host
 * synchronisation, capturable in a HIP graph.  The value of a candidate does not depend on the
 * shard (n_cand, cand_offset) it is computed in.  paths[s] takes the place of the `ucb` array of
 * bo_update_hypervolume_improvement / bo_hvi_select_topq_masked (shift = prior_mean, scale =
 * sqrt(prior_var)): the best candidate of draw s is pick s of the batch.
 * Fields shared with bo_bucb_desc have its meaning.  n_features <= BO_TS_MAX_FEATURES (any value,
 * not only multiples of 4); n_cand <= 2^36. */
#define BO_TS_MAX_FEATURES 65536
typedef struct bo_ts_desc {
  int32_t n_obj;              /* objectives (<= BO_MAX_OBJ)                                   */
  int32_t dim;                /* input dimensions (<= BO_MAX_DIM)                              */
  int64_t n_train;            /* N >= 1                                                       */
  const double* x_train;      /* device [n_train][dim]                                        */
  const double* y;            /* device, rows [n_obj] with row stride ld_y                    */
  int64_t ld_y;               /* >= n_obj                                                     */
  const double* kinv;         /* device [n_obj][ld_k][ld_k]; leading N x N block = invert_k() */
  int64_t ld_k;
  int32_t cand_kind;          /* bo_cand_kind                                                 */
  int32_t n_samples;          /* S, 1 .. BO_MAX_TOPQ                                          */
  const void* cand;           /* device [n_cand][dim] (kinds I64/F64); host bo_sobol_desc* (SOBOL) */
  int64_t n_cand;             /* candidates of this call (a shard)                            */
  int64_t cand_offset;        /* global index of this call's first candidate                  */
  int64_t grid_lo[BO_MAX_DIM];     /* kind GRID                                              */
  int64_t grid_shape[BO_MAX_DIM];  /* kind GRID (axis dim-1 fastest)                         */
  double prior_mean[BO_MAX_OBJ];
  double prior_var[BO_MAX_OBJ];
  double length_scale[BO_MAX_OBJ];
  double jitter;              /* KERNEL_JITTER added by invert_k: 1e-6 (1e-3 float32 branch)  */
  int64_t n_features;         /* D, 1 .. BO_TS_MAX_FEATURES                                   */
  const double* z;            /* device [n_obj][D][dim]                                       */
  const double* phase;        /* device [n_obj][D]                                            */
  const double* theta;        /* device [S][n_obj][D]                                         */
  const double* eps;          /* device [S][n_obj][N]                                         */
  double* paths;              /* device [S][n_obj][ld]: z_so, columns [0, n_cand) written     */
  int64_t ld;                 /* row stride of paths (>= n_cand)                              */
  double* weights_out;        /* optional device [S][n_obj][N]: the v that was used           */
} bo_ts_desc;
/* bytes of device workspace bo_sample_paths needs for `desc` (0 on bad args) */
size_t bo_sample_paths_workspace_size(const bo_ts_desc* desc);
int bo_sample_paths(const bo_ts_desc* desc, void* workspace, size_t workspace_bytes, void* stream);

/* is_pareto_efficient  bayesopt/pareto.py:12-45: mask[i] = 1 iff no row j dominates row i
 * (maximisation, weak dominance; NaN rows never dominate nor are dominated).
 * y: device [n][n_obj] row-major; mask: device uint8 [n]. Bit-exact. */
int bo_pareto_mask(const double* y, int64_t n, int32_t n_obj, uint8_t* mask, void* stream);

/* Exact hypervolume improvement (opt-in acquisition; the reference's
 * update_hypervolume_improvement, acquisition.py:89-108, is the sum of UCBs above and stays the
 * default).  The reference point it would use is bayesian_optimization.py:65 / :425 (unused
 * there).  Maximisation.
 *
 * bo_hvi_boxes (HOST, synchronous, no device memory): decomposes the region above ref_point not
 * dominated by `front` (host [n][n_obj] row-major; rows with NaN / not strictly above ref_point
 * are ignored, dominated rows are harmless) into disjoint boxes, host [*][2 n_obj]
 * (lower[n_obj], upper[n_obj]; upper may be +inf).  Writes the count to *n_boxes; returns
 * BO_ERR_WORKSPACE (count still written) when it exceeds `capacity`.  n_obj <= 4.
 *
 * bo_hypervolume_improvement_exact: acq[i] = sum_b prod_k max(0, min(p_k, upper_bk) - lower_bk)
 * = HV(front u {p}) - HV(front), p_k = shift[k] + scale[k] * ucb[k][i] (ucb device
 * [n_obj][ld], the standardised UCB; shift = prior mean, scale = sqrt(prior variance) give
 * mu + beta sigma in objective units).  boxes: device copy of bo_hvi_boxes' output.  NaN in p
 * gives NaN (selected first, as NaN is by the reference's argsort).  shift/scale host. */
/* bo_hvi_select_topq: the exact HVI of bo_hypervolume_improvement_exact written into acq AND
 * the top-q selection of bo_select_topq over it, in one pass over the UCB arrays, any
 * q <= BO_MAX_TOPQ, n_obj <= 4.  Arguments as those two functions'; workspace
 * bo_select_topq_workspace_size(n_cand, topq). */
int bo_hvi_select_topq(double* acq, const double* ucb, int64_t ld, int64_t n_cand, int32_t n_obj,
                       const double* shift, const double* scale, const double* boxes,
                       int64_t n_boxes, int32_t cand_kind, const void* cand, const int64_t* grid_lo,
                       const int64_t* grid_shape, int32_t dim, int64_t cand_offset,
                       const double* excl_points, int64_t n_excl, int32_t topq, double* top_val,
                       int64_t* top_idx, void* workspace, size_t workspace_bytes, void* stream);
int bo_hvi_select_topq_masked(double* acq, const double* ucb, int64_t ld, int64_t n_cand,
                              int32_t n_obj, const double* shift, const double* scale,
                              const double* boxes, int64_t n_boxes, int64_t cand_offset,
                              const uint32_t* mask, int32_t topq, double* top_val,
                              int64_t* top_idx, void* workspace, size_t workspace_bytes,
                              void* stream);
/* bo_box_volume_sum: out[0] (device) = sum_b prod_k max(0, min(upper_bk, upper[k]) - lower_bk)
 * over `boxes` (device, bo_hvi_boxes layout): the volume of the boxes clipped above at `upper`
 * (host [n_obj]).  With the boxes of the region a front does NOT dominate and upper = the
 * front's per-objective maximum, HV(front) = prod_k (upper_k - ref_k) - that volume; a rank's
 * share of the boxes gives its partial sum for the all-reduce "hypervolume accumulator"
 * (bayesopt_smart_amd/distributed.py).  Deterministic (one workgroup, fixed-order tree). */
int bo_box_volume_sum(const double* boxes, int64_t n_boxes, int32_t n_obj, const double* upper,
                      double* out, void* stream);
int bo_hvi_boxes(const double* front, int64_t n, int32_t n_obj, const double* ref_point,
                 double* boxes, int64_t capacity, int64_t* n_boxes);
int bo_hypervolume_improvement_exact(double* acq, const double* ucb, int64_t ld, int64_t n,
                                     int32_t n_obj, const double* shift, const double* scale,
                                     const double* boxes, int64_t n_boxes, void* stream);

/* Expected hypervolume improvement (EHVI; opt-in acquisition "ehvi").  NOT in the reference,
 * which has no EHVI: parity is unpinned by it.  With independent objectives
 * Y_k ~ N(mu_k, sigma_k^2), sigma_k = sqrt(|var_k|) (the UCB's convention), and the disjoint boxes
 * [l_b, u_b) of bo_hvi_boxes, the expectation of the box sum bo_hypervolume_improvement_exact
 * evaluates is
 *   EHVI = sum_b prod_k [ psi_k(l_bk) - psi_k(u_bk) ],
 *   psi_k(a) = E[(Y_k - a)+] = sigma_k (phi(z) + z Phi(z)), z = (mu_k - a) / sigma_k, psi_k(+inf) = 0.
 *
 * bo_ehvi_tables (HOST, synchronous, no device memory): the boxes' bounds are copies of few
 * coordinates (the reference point, the front's values, the columns' floors).  From `boxes`
 * (host, bo_hvi_boxes' output [n_boxes][2 n_obj]) it writes, per objective k, the sorted unique
 * finite bounds -- n_edges[k] = E_k of them, concatenated in `edges` (host, objective 0 first) --
 * and per box 2 n_obj int32 indices into its axis' edges (box_idx, host [n_boxes][2 n_obj], laid
 * out as the box: lower[n_obj], upper[n_obj]); index E_k stands for +inf.  The lookup is exact.
 * n_edges (host [n_obj]) is always written; returns BO_ERR_WORKSPACE, with nothing else written,
 * when sum_k E_k exceeds `edge_capacity` (doubles in `edges`).  An empty front (one box) gives
 * E_k = 1.  n_obj <= 4.
 *
 * bo_expected_hypervolume_improvement: acq[i] = EHVI of candidate i, from mu / var (device
 * [n_obj][ld], the predict's mu_objectives / variance_objectives in objective units).  NaN in any
 * mu_k or var_k gives NaN (selected first, as for the exact HVI); sigma = 0 gives the limit
 * psi(a) = max(mu - a, 0); n_boxes = 0 gives 0.  Asynchronous on `stream`, capturable in a HIP
 * graph, deterministic (fixed box order, no atomics).  `form`:
 *   1  direct: psi at every finite bound of every box; needs `boxes` (device copy of
 *      bo_hvi_boxes' output) only.
 *   2  table: one thread per candidate evaluates psi_k at every edge of every axis once into its
 *      column of an LDS table [edge][thread] and then walks the boxes' index tuples; needs
 *      `edges` (device), `n_edges` (HOST [n_obj]) and `box_idx` (device).  ADMISSION RULE: the
 *      table holds S = sum_k E_k doubles per thread; the workgroup is the largest
 *      T in {256, 128, 64} with 8 S T <= 163840 bytes (the 160 KiB LDS of a CU), i.e. T = 256 for
 *      S <= 80, 128 for S <= 160, 64 for S <= 320 -- bo_ehvi_table_threads returns T, or 0 when
 *      no table fits, and then form 2 returns BO_ERR_UNSUPPORTED.
 *   0  auto: the table form where it is admitted and was measured not slower than the direct
 *      form, else the direct form; pointers of the form not taken may be NULL.  AUTO'S RULE
 *      (profiles/ehvi_c3.jsonl, 2^20 candidates): with 3 or 4 objectives
 *      the table form wherever it is admitted (1.16x to 9.6x the direct form's speed at S = 36 ..
 *      303); with 2 objectives for S <= 40 only, where two 256-thread tables fit a CU (1.26x ..
 *      1.37x at S = 18, 34, 40; 0.88x and 0.92x at S = 42 and 66, where one table leaves a CU
 *      with one wave per SIMD); with 1 objective (one box, one psi) the direct form.
 * Both forms use one psi and one box order and give the same bits.  bo_ehvi_tables also returns
 * BO_ERR_WORKSPACE when box_idx is NULL with n_boxes > 0 (a query of the counts). */
int bo_ehvi_tables(const double* boxes, int64_t n_boxes, int32_t n_obj, double* edges,
                   int64_t edge_capacity, int32_t* n_edges, int32_t* box_idx);
int bo_ehvi_table_threads(int64_t sum_edges);
int bo_expected_hypervolume_improvement(double* acq, const double* mu, const double* var,
                                        int64_t ld, int64_t n, int32_t n_obj, const double* boxes,
                                        int64_t n_boxes, const double* edges,
                                        const int32_t* n_edges, const int32_t* box_idx,
                                        int32_t form, void* stream);

/* Outcome constraints: the feasibility-weighted EHVI (Gardner et al. 2014 and Gelbart et al. 2014
 * for EI, Feliot et al. 2017 for the hypervolume form).  NOT in the reference: parity is unpinned
 * by it.  The outputs are ordered objectives first, n_out = n_obj + n_con with 1 <= n_obj <= 4 and
 * n_out <= BO_MAX_OBJ; every output has its own independent GP.  Constraint j has bounds
 * lo_j <= hi_j, either infinite on its own side (lo = -inf, hi = +inf), neither NaN; a point is
 * feasible iff lo_j <= g_j <= hi_j for every j.  With the constraint rows of mu / var,
 * sigma = sqrt(|var|) (the UCB's and the EHVI's convention), za = (lo - mu) / sigma and
 * zb = (hi - mu) / sigma:
 *   P_j = Phi(zb) - Phi(za)       the probability that constraint j holds
 *   acq = EHVI(objective rows; the boxes of the FEASIBLE front above the reference point) prod_j P_j
 * P_j keeps its relative accuracy in both tails (when no candidate is likely feasible the order of
 * 1e-30 against 1e-40 is all a selection has): it is a difference of positive tail terms,
 * Q(z) = erfc(z / sqrt 2) / 2,
 *   Q(za) - Q(zb) for za > 0,   Q(-zb) - Q(-za) for zb < 0,   (1 - Q(zb)) - Q(-za) otherwise.
 * LIMITS: sigma = 0 gives 1 when lo <= mu <= hi (the bounds included), else 0; the bounds
 * (-inf, +inf) give exactly 1; NaN in any mu or var of any row, objective or constraint, gives
 * acq = NaN (selected first, as for the EHVI).
 * ROUNDING RULE: with E the value bo_expected_hypervolume_improvement gives for the objective rows
 * (the same bits, rule for the form and box order) and P = ((P_0 P_1) P_2) ... in f64, left to
 * right, acq = fl(E P); the table form and the direct form give the same bits.
 *
 * bo_constrained_ehvi: mu / var are device [n_obj + n_con][ld]; con_lo / con_hi are HOST [n_con]
 * (passed to the kernel by value); boxes, the tables and `form` are those of
 * bo_expected_hypervolume_improvement over the n_obj objectives (the table holds objective edges
 * only, so the admission rule and auto's rule are unchanged).  pof_out (optional, device [n])
 * receives P (NaN where a constraint row holds NaN).  n_con = 0 is the plain scan with the same
 * bits, and pof_out is then 1.  Every argument is checked before the device is touched: BO_ERR_ARG
 * for lo > hi, a NaN bound, lo = +inf, hi = -inf, n_obj outside 1..4, n_con < 0,
 * n_obj + n_con > BO_MAX_OBJ, or con_lo / con_hi NULL with n_con > 0; otherwise the statuses of
 * bo_expected_hypervolume_improvement.  Asynchronous on `stream`, capturable in a HIP graph,
 * deterministic. */
int bo_constrained_ehvi(double* acq, double* pof_out, const double* mu, const double* var,
                        int64_t ld, int64_t n, int32_t n_obj, int32_t n_con, const double* con_lo,
                        const double* con_hi, const double* boxes, int64_t n_boxes,
                        const double* edges, const int32_t* n_edges, const int32_t* box_idx,
                        int32_t form, void* stream);

/* The EHVI in log space (opt-in acquisition "logehvi"; LogEI / qLogEHVI: Ament et al., NeurIPS 2023).
 * NOT in the reference: parity is unpinned by it (tests/logehvi_ref.py is the independent statement,
 * in mpmath).  bo_expected_hypervolume_improvement returns one f64: psi is cut off at |z| = 40 and
 * products of small factors underflow before that, so every candidate some tens of posterior standard
 * deviations under the front gets exactly 0.0 and a batch that reaches into those zeros is filled in
 * index order.  This scan returns the natural logarithm of the same quantity, finite and correctly
 * ordered wherever the exact value is positive and its logarithm is an f64.  It is monotone in the
 * EHVI: where the linear values are distinct and did not underflow it selects the same batch.  With
 * the notation of bo_expected_hypervolume_improvement and bo_constrained_ehvi (sigma_k = sqrt(|var_k|),
 * bo_hvi_boxes' boxes, the constraint rows after the objective rows):
 *   psi_k(a) = sigma_k h(z),  z = (mu_k - a) / sigma_k,  h(z) = phi(z) + z Phi(z),  psi_k(+inf) = 0
 *   F_bk     = psi_k(l_bk) - psi_k(u_bk)
 *   T_b      = sum_k ln F_bk
 *   L        = ln sum_b exp(T_b)  [ + sum_j ln P_j ,  P_j = Phi(zb_j) - Phi(za_j) ]
 * LIMITS: sigma = 0 gives the limit psi(a) = max(mu - a, 0); a box with a zero factor contributes
 * nothing; when the exact EHVI is 0 (no box has all factors positive, or n_boxes = 0) L = -inf;
 * P_j = 0 (sigma = 0 outside the bounds, or lo = hi) gives -inf; the bounds (-inf, +inf) contribute
 * exactly 0; NaN in any mu or var of any row, objective or constraint, gives NaN (selected first, as
 * everywhere else).  z^2 >= 1e300 counts as psi = 0; likewise a constraint whose nearer tail
 * argument t has t^2 past f64's range (t above about 1.3e154) gives ln P_j = -inf.
 * -inf AND THE SELECTION: bo_select_topq / bo_select_topq_masked order NaN first, then descending
 * value, ties by ascending index, and -inf is an ordinary value in that order, the lowest: a free
 * candidate whose value is -inf IS selected once no higher value is left, with top_val = -inf and
 * its own top_idx >= 0.  The "no candidate" record is told apart by top_idx = -1 alone (its
 * top_val is -inf too).  So a batch larger than the number of candidates with a positive EHVI is
 * completed by the -inf candidates in index order, exactly as the linear scan's zeros are.
 * ARITHMETIC (bo_logehvi.hip states it in full): every psi is carried as an extended-range number
 * m 2^e (an f64 mantissa, an integer exponent held in an f64), produced once per bound from the
 * direct form for z >= 0, from exp(-z^2/2) [1/sqrt(2 pi) - |z| erfcx(|z| / sqrt 2) / 2] for
 * -32 < z < 0 and from the series in 1 / z^2 (9 terms) below; the box differences, products and the
 * running sum work on mantissas aligned by ldexp to a running maximum exponent, in box order, with
 * no atomics; the logarithm is taken once per candidate.  ln P_j is ln(Q(t1) - Q(t2)) of the two
 * tail terms while the nearer tail argument is below 6, and from there on comes from ln Q(z) =
 * ln(erfcx(z / sqrt 2) / 2) - z^2 / 2 and a log-difference of the two tails.  A candidate's bits do
 * not depend on its shard, on n or on ld.
 * ROUNDING RULE: with L_ref the same quantity from the same f64 mu, var, boxes and bounds at 60
 * digits and u = 2^-53, at every candidate
 *   c(z)     = 1 + min(z, 0)^2                    (the conditioning of ln h in z; 1 + z^2 for ln Q)
 *   kappa_bk = [psi(l) c(z_l) + psi(u) c(z_u)] / F_bk
 *   w_b      = exp(T_b - ln sum_b exp T_b)        (the reference's weights, they sum to 1)
 *   K        = sum_b w_b sum_k (kappa_bk + |ln F_bk|)  +  sum_j (kappa_j + |ln P_j|)
 *   |L - L_ref| <= u [ C K + n_boxes + 2 ],   C = 8,
 * kappa_j the same expression over the two tail terms of P_j; logpof_out alone meets
 * |lp - lp_ref| <= u [ C sum_j (kappa_j + |ln P_j|) + 2 ].  Where L_ref is -inf or NaN the value is
 * that.  C: the f64 restatement of this arithmetic (tests/logehvi_ref.py, logehvi_f64) measured a
 * worst (|L - L_ref| / u - n_boxes - 2)+ / K of 2.81 on the CPU over z from +8 to -1e6 and on both
 * sides of every branch switch, sigma from 1e-5 to 1e3, thin and wide boxes, 1 to 4 objectives and
 * 0, 1 and 7 constraints (2.67 at z = -32.1 with one objective, the first point of the series;
 * logpof alone 1.04); C is the smallest power of two at least twice that.
 * ON THE DEVICE (MI355X, tests/test_gpu_logehvi.py, every candidate, both forms): the worst
 * |L - L_ref| / bound is 0.357 (one objective, a one-point front), the worst fraction of logpof_out's
 * own bound 0.176 (3 objectives, 5 constraints), 0.242 over the 1023 candidates of the motivating
 * case; DESIGN.md section 19 lists the cases.
 *
 * bo_log_ehvi: the arguments of bo_constrained_ehvi, with the same checks, all before the device is
 * touched (BO_ERR_ARG for lo > hi, a NaN bound, lo = +inf, hi = -inf, n_obj outside 1..4,
 * n_con < 0, n_obj + n_con > BO_MAX_OBJ, con_lo / con_hi NULL with n_con > 0, a NULL acq / mu /
 * var, n < 0, ld < n, n_boxes < 0, form outside 0..2, or the pointers of the form asked for
 * missing); n = 0 returns BO_OK.  n_con = 0 is the plain form.  logpof_out (optional, device [n])
 * receives sum_j ln P_j (0 without constraints; NaN where a constraint row holds NaN).
 * Asynchronous on `stream`, capturable in a HIP graph, deterministic.  `form` as for the EHVI, and
 * the direct and the table form give the same bits, but the table holds 16 bytes per edge and
 * thread (mantissa and exponent).  ADMISSION RULE: the workgroup is the largest T in {256, 128, 64}
 * with 16 S T <= 163840 bytes, i.e. T = 256 for S <= 40, 128 for S <= 80, 64 for S <= 160 --
 * bo_logehvi_table_threads returns T, or 0 when no table fits, and then form 2 returns
 * BO_ERR_UNSUPPORTED.  AUTO'S RULE, from profiles/logehvi_c3.jsonl (2^20 candidates, 2 objectives)
 * and profiles/logehvi_c4.jsonl (2^21 candidates, 3 objectives), table against direct in one
 * process: with 2 objectives the table form for S <= 20 only, where two 256-thread tables fit a CU
 * (direct / table time 1.24x and 1.25x at S = 18 and 20; 0.84x, 0.87x and 0.87x at S = 22, 34 and
 * 40, where one table leaves a CU with one wave per SIMD; 0.48x at S = 42 and 66 with 128
 * threads); with 3 or 4 objectives the table form where its workgroup has at least 128 threads,
 * S <= 80 (2.25x at S = 27, 1.58x at S = 51; 0.99x at S = 99 with 64 threads, so the direct form
 * there; 4 objectives follow 3's rule and were not measured); with 1 objective (one box, one psi)
 * the direct form.  COST against the "ehvi" scan in the same process, each in its faster form:
 * 2.1x to 2.8x its time at 2 objectives (0.174 against 0.076 ms at a front of 8, 0.401 against
 * 0.148 ms at 16), 3.4x to 4.1x at 3 objectives (0.955 against 0.281 ms at a front of 8); direct
 * against direct it is 2.0x to 2.2x throughout; one constraint adds 4 to 13 %. */
int bo_logehvi_table_threads(int64_t sum_edges);
int bo_log_ehvi(double* acq, double* logpof_out, const double* mu, const double* var, int64_t ld,
                int64_t n, int32_t n_obj, int32_t n_con, const double* con_lo, const double* con_hi,
                const double* boxes, int64_t n_boxes, const double* edges, const int32_t* n_edges,
                const int32_t* box_idx, int32_t form, void* stream);

/* ------------------------------------------------------------------------------------
 * Max-value entropy search for multi-objective problems (MESMO: Belakaria, Deshwal & Doppa 2019,
 * after Wang & Jegelka 2017; opt-in acquisition "mes").  NOT in the reference: parity is unpinned
 * by it (tests/mes_ref.py is the independent statement).  Its cost is linear in the number of
 * objectives (1 <= n_obj <= BO_MAX_OBJ), and it needs no reference point and no front.  With
 * candidate c's posterior mu_k(c), var_k(c) (the predict's mu_objectives / variance_objectives),
 * sigma_k = sqrt(|var_k|) (the UCB's and the EHVI's convention) and S posterior draws f_sk
 * (bo_sample_paths' `paths` mapped back to objective units):
 *   y*_sk  = max over ALL candidates c of f_sk(c)          (evaluated points included)
 *   gamma  = (y*_sk - mu_k(c)) / sigma_k(c)                (as fl(fl(y* - mu) fl(1 / sigma)))
 *   g(x)   = x phi(x) / (2 Phi(x)) - ln Phi(x)             (>= 0, decreasing, g(0) = ln 2)
 *   acq(c) = (1/S) sum_s sum_k g(gamma_sk(c))
 * g(x) is the entropy of N(0, 1) minus the entropy of N(0, 1) truncated above at x: acq is the
 * expected reduction of the entropy of Y(c) given that no objective exceeds its sampled maximum.
 * g is evaluated in three branches (both tails of the textbook form are lost in f64):
 *   x >= 0:         q = erfc(x / sqrt 2) / 2;  g = x phi(x) / (2 (1 - q)) - log1p(-q)
 *   -2^27 < x < 0:  t = -x / sqrt 2, E = erfcx(t);  g = t^2 - t / (sqrt(pi) E) - ln(E / 2)
 *   x <= -2^27:     g = ln(-x) + (ln(2 pi) - 1) / 2    (-inf included)
 * LIMITS: sigma = 0 gives g = 0 if y* >= mu, else +inf; y* = +inf gives 0 and y* = -inf gives
 * +inf; NaN in any mu_k, var_k or y*_sk gives acq = NaN (selected first, as everywhere else).
 * The summation order is fixed -- s outer, k inner, one f64 accumulator, then one multiplication
 * by fl(1 / S) -- so the result is deterministic and a candidate's bits do not depend on its shard.
 * ROUNDING RULE: with u = 2^-53 and the reference g_ref, acq_ref computed in extended precision
 * from the same f64 mu, var and y* (the device's own y* taken as data),
 *   |acq - acq_ref| <= u / S sum_sk [32 (1 + gamma_sk^2 / 2) + S n_obj] g_ref(gamma_sk) + 2^-1022:
 * 1 + gamma^2 / 2 is the conditioning of exp(-gamma^2 / 2) and of the middle branch's
 * cancellation (t^2 - t / (sqrt(pi) E) -> -1/2); of the 32, the f64 evaluation of the three
 * branches measures 10.8 at worst (near x = -0.003), the three roundings of gamma add at most 6,
 * and the rest is left to the device's erfcx / exp / log.
 *
 * bo_path_maxima: ystar[r] = fl(shift_k + scale_k max_j paths[r][j]) -- one rounding, an fma --
 * for each of the n_samples * n_obj rows r = s * n_obj + k of `paths` (device, row stride ld,
 * columns [0, n_cand)); `ystar` is device [n_samples][n_obj]; shift / scale are HOST [n_obj],
 * passed to the kernel by value (the loop: prior_mean and sqrt(prior_variance)).  NaN entries are
 * ignored; an all-NaN or empty row gives NaN; a zero maximum of either sign counts as +0.  The
 * max is exact, so the result does not depend on the reduction order, and, the map being monotone
 * for scale > 0, the max over per-shard results is bit-equal to the unsharded result (several
 * ranks combine with one all-reduce MAX).  One pass over `paths`, fixed-order partial maxima in
 * the workspace, one finishing workgroup; no atomics.  The workspace size query returns 0 for
 * n_cand < 0 or n_rows outside [1, BO_MAX_TOPQ * BO_MAX_OBJ].
 * bo_max_value_entropy: the scan; acq is device [n], mu / var device [n_obj][ld], ystar device
 * [n_samples][n_obj], 1 <= n_samples <= BO_MAX_TOPQ, 1 <= n_obj <= BO_MAX_OBJ.  One thread per
 * candidate.
 * Both check every argument before the device is touched: BO_ERR_ARG for a NULL pointer (`paths` may be NULL when n_cand = 0: nothing is read), n_obj or
 * n_samples out of range, ld < n (ld < n_cand), a negative n, scale <= 0 or a non-finite scale or
 * shift; BO_ERR_WORKSPACE for a missing or short workspace.  Both are asynchronous on `stream`,
 * capturable in a HIP graph, deterministic, and synchronise with nothing. */
size_t bo_path_maxima_workspace_size(int64_t n_cand, int64_t n_rows);
int bo_path_maxima(double* ystar, const double* paths, int64_t ld, int64_t n_cand,
                   int32_t n_samples, int32_t n_obj, const double* shift, const double* scale,
                   void* workspace, size_t workspace_bytes, void* stream);
int bo_max_value_entropy(double* acq, const double* mu, const double* var, int64_t ld, int64_t n,
                         int32_t n_obj, const double* ystar, int32_t n_samples, void* stream);

/* ------------------------------------------------------------------------------------
 * Kriging-believer batches for the EHVI (Ginsbourger, Le Riche & Carraro 2010; opt-in
 * batch_strategy "kb").  NOT in the reference.  The q best values of one EHVI array are q
 * neighbours of one maximum; here the picks are taken one after the other, and after each one the
 * model is conditioned on a believed observation equal to its own posterior mean at the pick.
 * Inputs: the predict's mu_objectives / variance_objectives (`mu` / `var`, objective units,
 * [n_obj][ld]), the fitted state (x_train, kinv), the candidates as in bo_bucb_desc, a HOST front
 * [n_front][n_obj] and a HOST reference point, jitter and min_variance.  With front_0 = the given
 * front and var^0 = the given variance, for t = 1..q:
 *   boxes_t  = the decomposition bo_hvi_boxes gives for (front_{t-1}, ref_point)
 *   acq_t[j] = the EHVI of (mu[:, j], var^(t-1)[:, j]) over boxes_t, with the bits
 *              bo_expected_hypervolume_improvement gives for those arrays: the same psi, the same
 *              box order and the same `form` rule, applied to boxes_t (so the form, and the table
 *              form's workgroup size, may change from one pick to the next)
 *   p_t      = the best candidate of acq_t in the order of bo_select_topq (NaN first, then
 *              descending value, then ascending global index) among those neither masked nor
 *              already picked
 *   m_t      = mu[:, p_t], the believed observation; front_t = front_(t-1) u {m_t}.  A row with a
 *              NaN, or not strictly above the reference point, changes no box (bo_hvi_boxes
 *              ignores it)
 *   var^t    = the recursion c_t, d_t, v_t of bo_bucb_desc for a pick at p_t, floored at
 *              min_variance; unchanged for an objective whose d_t is not finite.  The mean does
 *              not move: a believed observation equals it.
 * When no candidate is left, top_idx[t] = -1, top_val[t] = -inf and believed[t] = NaN, and later
 * picks likewise.  q = 1 is the top-1 of the EHVI array.  n_obj <= 4 (the box decomposition's
 * limit), q <= BO_MAX_TOPQ, n_cand <= 2^36.  mu / var / mask / front are not modified.
 * Deterministic: fixed-order reductions, no atomics; a workspace and a host_ws of any content give
 * the same bits.
 *
 * The box decomposition runs on the HOST, so the call is host-synchronous once per pick: it reads
 * (p_t, m_t) back, waits for that copy alone -- the variance update of pick t is already enqueued
 * and runs meanwhile -- decomposes front_t and uploads boxes_(t+1) with their edge tables.  It is
 * therefore NOT capturable: on a capturing stream it returns BO_ERR_UNSUPPORTED before anything is
 * launched.  When it returns, pick q's work may still be running on the stream, but host_ws has
 * been read for the last time and is the caller's again.  The box count of
 * the later picks cannot be known from the descriptor: when a pick's decomposition exceeds
 * box_capacity the call returns BO_ERR_WORKSPACE with *n_boxes_max = that count (outputs are then
 * unspecified); the picks are deterministic, so a retry from the start with a larger capacity is
 * correct.  The edge buffers are sized exactly: an axis has at most n_front + q + 1 edges.  form 2
 * returns BO_ERR_UNSUPPORTED when a pick's table does not fit (bo_ehvi_table_threads).
 * Arguments are checked before the device is touched.  Fields shared with bo_bucb_desc have its
 * meaning. */
typedef struct bo_kb_desc {
  int32_t n_obj;              /* objectives (<= 4)                                            */
  int32_t dim;                /* input dimensions (<= BO_MAX_DIM)                              */
  int64_t n_train;            /* N >= 1                                                       */
  const double* x_train;      /* device [n_train][dim]                                        */
  const double* kinv;         /* device [n_obj][ld_k][ld_k]; leading N x N block = invert_k() */
  int64_t ld_k;
  int32_t cand_kind;          /* bo_cand_kind                                                 */
  int32_t q;                  /* picks, 1 .. BO_MAX_TOPQ                                      */
  const void* cand;           /* device [n_cand][dim] (kinds I64/F64); host bo_sobol_desc* (SOBOL) */
  int64_t n_cand;             /* candidates of this call (a shard)                            */
  int64_t cand_offset;        /* global index of this call's first candidate                  */
  int64_t grid_lo[BO_MAX_DIM];     /* kind GRID                                              */
  int64_t grid_shape[BO_MAX_DIM];  /* kind GRID (axis dim-1 fastest)                         */
  double prior_var[BO_MAX_OBJ];
  double length_scale[BO_MAX_OBJ];
  double jitter;              /* KERNEL_JITTER added by invert_k: 1e-6 (1e-3 float32 branch)  */
  double min_variance;        /* MIN_VARIANCE: 1e-10 (1e-6 float32 branch)                    */
  const double* mu;           /* device [n_obj][ld]: mu_objectives (objective units)          */
  const double* var;          /* device [n_obj][ld]: variance_objectives (already floored)    */
  int64_t ld;                 /* row stride of mu / var / var_out (>= n_cand)                 */
  const uint32_t* mask;       /* device, bo_excl_mask_update's layout over this shard; NULL = none */
  const double* front;        /* HOST [n_front][n_obj] (NULL when n_front = 0)                */
  int64_t n_front;            /* >= 0                                                         */
  double ref_point[4];        /* HOST values, finite                                          */
  int32_t form;               /* 0 auto, 1 direct, 2 table: bo_expected_hypervolume_improvement's */
  int32_t reserved;
  int64_t box_capacity;       /* >= 1: rows the device box buffers hold                       */
  void* host_ws;              /* HOST staging, bo_select_batch_kb_host_workspace_size bytes,
                                 8-byte aligned; pinned memory recommended (pageable memory
                                 serialises the host step behind the variance update)         */
  size_t host_ws_bytes;
  double* top_val;            /* device [q]: acq_t[p_t] (-inf when no candidate is left)      */
  int64_t* top_idx;           /* device [q]: global index of pick t, -1 = no candidate left   */
  double* believed;           /* device [q][n_obj]: m_t                                       */
  double* var_out;            /* optional device [n_obj][ld]: var^q                           */
  double* acq_first;          /* optional device [n_cand]: acq_1, the plain EHVI              */
  double* acq_last;           /* optional device [n_cand]: acq_q                              */
  int64_t* n_boxes_max;       /* optional HOST: the largest box count met                     */
} bo_kb_desc;
/* bytes of device / host workspace bo_select_batch_kb needs for `desc` (0 on bad args) */
size_t bo_select_batch_kb_workspace_size(const bo_kb_desc* desc);
size_t bo_select_batch_kb_host_workspace_size(const bo_kb_desc* desc);
int bo_select_batch_kb(const bo_kb_desc* desc, void* workspace, size_t workspace_bytes,
                       void* stream);

/* ------------------------------------------------------------------------------------
 * GIBBON batches for an information criterion (Moss, Leslie, Gonzalez & Rayson 2021; opt-in
 * batch_strategy "gibbon" of acquisition "mes").  NOT in the reference.  The q best values of one
 * max-value entropy array are q neighbours of one maximum.  GIBBON's batch criterion is the sum of
 * the single-point information terms plus, per objective, half the log-determinant of the batch's
 * predictive correlation matrix R_o; taken greedily, the increment of log det R_o for a candidate j
 * after picks p_1..p_(t-1) is log(var_o^(t-1)[j] / var_o^0[j]) (Schur complement).  So the
 * single-point array is computed once, with the unconditioned variance, and a later pick adds a
 * penalty to it.  Inputs: `base` (device [n_cand]: the single-point acquisition -- in the loop
 * bo_max_value_entropy's array; the call does not care what it is), `var` = var^0 (the predict's
 * variance_objectives, [n_obj][ld], floored), the fitted state (x_train, kinv), the candidates as
 * in bo_bucb_desc, jitter and min_variance.  For t = 1..q:
 *   acq_1[j] = base[j], bit for bit (the first pass adds nothing: a NaN in `var` enters from
 *              acq_2 on)
 *   acq_t[j] = fl(base[j] + 0.5 P),  P = sum_o log(fl(var_o^(t-1)[j] / var_o^0[j])), summed in
 *              f64 with o ascending, for t > 1; an objective with var_o^0[j] == 0 contributes 0;
 *              NaN in base, var^0 or var^(t-1) gives NaN (selected first, as everywhere else)
 *   p_t      = the best candidate of acq_t in the order of bo_select_topq (NaN first, then
 *              descending value, then ascending global index) among those neither masked nor
 *              already picked
 *   var^t    = the recursion c_t, d_t, v_t of bo_bucb_desc for a pick at p_t, floored at
 *              min_variance; unchanged for an objective whose d_t is not finite
 * When no candidate is left, top_idx[t] = -1 and top_val[t] = -inf, for this pick and all later
 * ones.  q = 1 is the masked top-1 of `base`.  q <= BO_MAX_TOPQ, n_obj <= BO_MAX_OBJ; every
 * candidate kind, shards by cand_offset / n_cand.  base / var / mask are not modified.
 * Asynchronous on its stream, no host synchronisation between the picks and -- unlike
 * bo_select_batch_kb, there being no host step -- capturable in a HIP graph.  Deterministic:
 * fixed-order reductions, no atomics; a workspace of any content gives the same bits.
 * Every argument is checked before the device is touched: BO_ERR_ARG for a NULL base / var /
 * x_train / kinv / top_val / top_idx (or `cand` of an explicit kind), an output that aliases an
 * input, a misaligned workspace and what bo_select_batch_bucb refuses; BO_ERR_WORKSPACE for a
 * missing or short workspace.  Fields shared with bo_bucb_desc have its meaning. */
typedef struct bo_gibbon_desc {
  int32_t n_obj;              /* objectives (<= BO_MAX_OBJ)                                   */
  int32_t dim;                /* input dimensions (<= BO_MAX_DIM)                              */
  int64_t n_train;            /* N >= 1                                                       */
  const double* x_train;      /* device [n_train][dim]                                        */
  const double* kinv;         /* device [n_obj][ld_k][ld_k]; leading N x N block = invert_k() */
  int64_t ld_k;
  int32_t cand_kind;          /* bo_cand_kind                                                 */
  int32_t q;                  /* picks, 1 .. BO_MAX_TOPQ                                      */
  const void* cand;           /* device [n_cand][dim] (kinds I64/F64); host bo_sobol_desc* (SOBOL) */
  int64_t n_cand;             /* candidates of this call (a shard)                            */
  int64_t cand_offset;        /* global index of this call's first candidate                  */
  int64_t grid_lo[BO_MAX_DIM];     /* kind GRID                                              */
  int64_t grid_shape[BO_MAX_DIM];  /* kind GRID (axis dim-1 fastest)                         */
  double prior_var[BO_MAX_OBJ];
  double length_scale[BO_MAX_OBJ];
  double jitter;              /* KERNEL_JITTER added by invert_k: 1e-6 (1e-3 float32 branch)  */
  double min_variance;        /* MIN_VARIANCE: 1e-10 (1e-6 float32 branch)                    */
  const double* base;         /* device [n_cand]: the single-point acquisition                */
  const double* var;          /* device [n_obj][ld]: var^0, variance_objectives (already floored) */
  int64_t ld;                 /* row stride of var / var_out (>= n_cand)                      */
  const uint32_t* mask;       /* device, bo_excl_mask_update's layout over this shard; NULL = none */
  double* top_val;            /* device [q]: acq_t[p_t] (-inf when no candidate is left)      */
  int64_t* top_idx;           /* device [q]: global index of pick t, -1 = no candidate left   */
  double* var_out;            /* optional device [n_obj][ld]: var^q                           */
  double* acq_last;           /* optional device [n_cand]: acq_q, the array pick q was taken from */
} bo_gibbon_desc;
/* bytes of device workspace bo_select_batch_gibbon needs for `desc` (0 on bad args) */
size_t bo_select_batch_gibbon_workspace_size(const bo_gibbon_desc* desc);
int bo_select_batch_gibbon(const bo_gibbon_desc* desc, void* workspace, size_t workspace_bytes,
                           void* stream);

/* ------------------------------------------------------------------------------------
 * GP fit on device.
 * ---------------------------------------------------------------------------------- */

/* invert_k  bayesopt/numba_kernels.py:370-403: out[o] = inv(K[o][:N,:N] + 1e-6 I) (the
 * reference's LAPACK gesv with the identity): a blocked Cholesky when K is symmetric, followed
 * by one Newton step X + X (I - (K + 1e-6 I) X) on the matrix cores (the residual of gesv's
 * backward-stable solves), or the blocked LU with partial pivoting (getrf's row choice) + getrs
 * when the Cholesky fails or K is not symmetric.  kernel_matrix device [n_obj][ld][ld];
 * out device [n_obj][n][n]. Returns BO_ERR_SINGULAR on an exactly singular pivot.
 * Synchronous (the status depends on the factorisation). */
int bo_invert_k(double* out, const double* kernel_matrix, int64_t ld, int32_t n_obj, int64_t n,
                void* workspace, size_t workspace_bytes, void* stream);
/* bo_invert_k_jitter with per-objective path control and report (ABI 4).  lu_hint (host
 * [n_obj], may be NULL): when EVERY objective's entry is non-zero the Cholesky attempt is skipped
 * and all of them go straight to the blocked LU -- the caller's knowledge that the previous
 * iteration's Cholesky failed for them (a drop-in loop at Powell-fitted length scales, where
 * cond(K + 1e-6 I) > 1e16).  The result is the LU path's either way.  path_out
 * (host [n_obj], may be NULL): 0 Cholesky (+ Newton step), 1 blocked LU, 2 Gauss-Jordan. */
int bo_invert_k_ex(double* out, const double* kernel_matrix, int64_t ld, int32_t n_obj, int64_t n,
                   double jitter, const int32_t* lu_hint, int32_t* path_out, void* workspace,
                   size_t workspace_bytes, void* stream);
/* Per-objective counts of the paths bo_invert_k took since the library was loaded (process-wide,
 * host counters): counts[0] Cholesky, [1] blocked LU (Cholesky failed or K not symmetric;
 * N <= 2048), [2] Gauss-Jordan (the same above N = 2048).  Diagnostics for the fallback's
 * frequency. */
int bo_invert_k_path_counts(int64_t* counts);
/* bo_invert_k with the diagonal jitter given: KERNEL_JITTER of config.py:57-66 (1e-6 in the fp64
 * branch, which bo_invert_k uses; 1e-3 in the float32 branch). */
int bo_invert_k_jitter(double* out, const double* kernel_matrix, int64_t ld, int32_t n_obj, int64_t n,
                       double jitter, void* workspace, size_t workspace_bytes, void* stream);
size_t bo_invert_k_workspace_size(int32_t n_obj, int64_t n);
/* Process-wide counts of the factorisation schedules bo_invert_k / bo_compute_mll* ran:
 * counts[0] the persistent launch (one task-queue kernel: panels and trailing-update tiles hand
 * off through flags), [1] one launch per 32-column step (N > 1536 by default -- more than 48
 * column blocks of 32; the environment variable BO_FIT_PERSIST_MAX_NBT sets that block count --
 * or BO_FIT_PATH=launches), [2] persistent launches that gave up a wait (bounded spin) and were
 * rerun step by step. */
int bo_fit_path_counts(int64_t* counts);

/* compute_mll  bayesopt/numba_kernels.py:152-235 (Gram rebuilt into kernel_matrix first, as
 * the reference does).  Writes the summed MLL to *mll_out (host).  Returns BO_ERR_NOT_PD when
 * a Cholesky pivot is not positive.  Synchronous. */
int bo_compute_mll(double* mll_out, const double* x, int32_t dim, const double* y, int64_t ld_y,
                   double* kernel_matrix, int64_t ld, int32_t n_obj, const double* prior_mean,
                   const double* prior_variance, const double* length_scales,
                   int64_t current_eval, void* workspace, size_t workspace_bytes, void* stream);
/* The per-objective terms of compute_mll: mll_obj[o] (host, [n_obj]); compute_mll is their sum in
 * objective order.  Each term depends on (x, y[:, o], pm[o], ls[o]) only -- the correlation
 * matrix K / pv does not depend on pv -- so a caller may memoise terms across calls (the Powell
 * driver of bayesopt_smart_amd.kernels does).  Same arguments and errors as bo_compute_mll. */
int bo_compute_mll_each(double* mll_obj, const double* x, int32_t dim, const double* y, int64_t ld_y,
                        double* kernel_matrix, int64_t ld, int32_t n_obj, const double* prior_mean,
                        const double* prior_var, const double* length_scale, int64_t n,
                        void* workspace, size_t workspace_bytes, void* stream);
/* bo_compute_mll_each with the correlation matrix's jitter given: CHOLESKY_JITTER of
 * config.py:57-66 (1e-8 in the fp64 branch, which bo_compute_mll_each uses; 1e-4 in float32). */
int bo_compute_mll_each_jitter(double* mll_obj, const double* x, int32_t dim, const double* y, int64_t ld_y,
                               double* kernel_matrix, int64_t ld, int32_t n_obj, const double* prior_mean,
                               const double* prior_var, const double* length_scale, int64_t n, double jitter,
                               void* workspace, size_t workspace_bytes, void* stream);
size_t bo_compute_mll_workspace_size(int32_t n_obj, int64_t n);

/* The per-objective MLL terms and their analytic gradients in the logarithm of the length scale
 * (additive in ABI 5).  Per objective o, with C = e + jitter I, e_ij = exp(-r2_ij / (2 ls^2)),
 * yc = (y - pm) / std (the MLL's own standardisation: population std about its own mean, left
 * unscaled when that std is 0) and alpha = C^-1 yc:
 *
 *   mll_obj[o]     (host, [n_obj])  the bits bo_compute_mll_each_jitter returns for the same
 *                  arguments (it is that call: same factorisation path and schedule; the side
 *                  effect is the same too, kernel_matrix ends as pv e);
 *   grad_log_ls[o] (host, [n_obj])  d MLL_o / d log ls_o
 *                  = 1/2 sum_ij (alpha_i alpha_j - C^-1_ij) e_ij r2_ij / ls^2;
 *                  the derivative in ls_o is this value divided by ls_o.
 *
 * The MLL does not depend on prior_var (the correlation matrix is factored), so its derivative in
 * prior_var is exactly 0 and is not returned.  C^-1 is the augmented-Cholesky inverse (bo_invert_k's
 * first path, without its Newton step, which measured three orders of magnitude less accurate for
 * this sum) of a pv-free copy of e built into the workspace; there is no LU or Gauss-Jordan fallback: BO_ERR_NOT_PD when the value's factorisation, or the inverse's, meets a
 * non-positive pivot (the value's error is returned before anything else runs).  The reduction
 * uses no floating-point atomics: per-tile partial sums are added in tile order, so two calls
 * return the same bits.  Limits: n_obj <= BO_MAX_OBJ, n <= 2^15 (the inverse's range); the size
 * function returns 0 outside them.  No allocation in the call; synchronous. */
int bo_compute_mll_grad(double* mll_obj, double* grad_log_ls, const double* x, int32_t dim, const double* y,
                        int64_t ld_y, double* kernel_matrix, int64_t ld, int32_t n_obj,
                        const double* prior_mean, const double* prior_var, const double* length_scale,
                        int64_t n, double jitter, void* workspace, size_t workspace_bytes, void* stream);
size_t bo_compute_mll_grad_workspace_size(int32_t n_obj, int64_t n);

/* ------------------------------------------------------------------------------------
 * The fit's driver, native (HOST code calling the device MLL): scipy.optimize.minimize(
 * method="Powell", bounds=...) as optimize_hyperparams_mll calls it (numba_kernels.py:238-321,
 * :305-315), restated from scipy 1.15's _minimize_powell / _linesearch_powell / _line_for_search /
 * _minimize_scalar_bounded operation for operation (tan/atan from the C library).
 * ---------------------------------------------------------------------------------- */
/* objective: *f = f(x[0..n)); a non-zero return aborts the minimisation with that status */
typedef int (*bo_objective_fn)(const double* x, int32_t n, double* f, void* user);
/* tan (which = 0) / atan (which = 1) of the one-sided line searches' transform; NULL = the C
 * library's.  A caller wanting scipy's evaluation points bit for bit passes numpy's (its SIMD
 * tan differs from the C library's in the last bit for ~0.5 % of arguments). */
typedef double (*bo_trig_fn)(double x, int32_t which);
typedef struct bo_powell_result {
  double fun;             /* final objective value                                          */
  int64_t nfev;           /* objective evaluations                                          */
  int64_t nit;            /* Powell iterations                                              */
  int64_t device_calls;   /* bo_optimize_hyperparams_mll: device MLL calls (memo misses)     */
  int32_t warnflag;       /* scipy's status: 0 success, 1 maxfev, 2 maxiter, 3 nan, 4 bounds  */
  int32_t reserved;
} bo_powell_result;
/* Minimise fn from x (in: x0, out: the result) within lb <= x <= ub (host [n]; +-inf allowed);
 * maxiter / maxfev < 0 = None (scipy's defaults).  direc (optional, host [n][n]) receives the
 * final direction set.  BO_ERR_UNSUPPORTED when a line search is unbounded in both directions
 * (scipy's bracketing Brent; the fit's bounds never need it). */
int bo_powell_minimize(bo_objective_fn fn, void* user, double* x, int32_t n, const double* lb,
                       const double* ub, double xtol, double ftol, int64_t maxiter, int64_t maxfev,
                       bo_trig_fn trig, double* direc, bo_powell_result* res);
/* optimize_hyperparams_mll (numba_kernels.py:238-321) as ONE call: Powell over [ls..., pv...] from
 * the given values (host, updated in place on success), bounds [min_bound, inf), maximising the
 * device MLL (bo_compute_mll_each_jitter; each per-objective term memoised per distinct ls_o, a
 * device call only for the objectives whose ls changed).  kernel_matrix ends as the Gram of the
 * last evaluated hyper-parameters (the reference's side effect).  Workspace:
 * bo_compute_mll_workspace_size(n_obj, n).  Synchronous. */
int bo_optimize_hyperparams_mll(const double* x, int32_t dim, const double* y, int64_t ld_y,
                                double* kernel_matrix, int64_t ld, int32_t n_obj, const double* prior_mean,
                                double* prior_variance, double* length_scales, int64_t n, double jitter,
                                double xtol, double ftol, int64_t maxiter, double min_bound, bo_trig_fn trig,
                                void* workspace, size_t workspace_bytes, void* stream, bo_powell_result* res,
                                double* direc);

/* ------------------------------------------------------------------------------------
 * Measurement hooks (bench.py): while enabled, each fused predict kernel launch (the
 * dominant kernel of bo_predict_acquire) is bracketed by HIP events on its stream;
 * bo_profile_stop synchronises them and returns the summed kernel time.
 * ---------------------------------------------------------------------------------- */
int bo_profile_start(int max_launches);
int bo_profile_stop(double* total_ms, int* launches);

/* ------------------------------------------------------------------------------------
 * Self test: D[16][16] = A[16][4] * B[4][16] on one f64 MFMA (layout check). Device ptrs.
 * ---------------------------------------------------------------------------------- */
int bo_selftest_mfma_f64(const double* a16x4, const double* b4x16, double* d16x16, void* stream);
/* the same on one v_mfma_f32_16x16x4_f32 (the BO_PREDICT_FP32 kernel's layout). Device ptrs. */
int bo_selftest_mfma_f32(const float* a16x4, const float* b4x16, float* d16x16, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BO_AMD_H */
