// Kriging-believer batches for the EHVI on the device: bo_select_batch_kb (include/bo_amd.h states
// the definition; DESIGN.md §13 the launches, the overlap and the measurements).
//
// NOT in the reference.  Pick t is the best candidate of the EHVI of (mu, var^(t-1)) over the boxes
// of the front extended by the believed observations m_1..m_(t-1) = the posterior means at the
// earlier picks; var^t is the variance conditioned on the picks, the hallucinated-observation
// update of bo_bucb_impl.h (a believed observation equals the mean, so the mean does not move).
// Per pick t, on the caller's stream:
//   scan    n_cand/T      the EHVI of every candidate (bo_ehvi_impl.h: the arithmetic, the form and
//                         the workgroup size T of bo_expected_hypervolume_improvement, chosen anew
//                         for this pick's boxes), stored when it is acq_first / acq_last, and this
//                         workgroup's best unmasked entry
//   pick    1 workgroup   bucb_pick_kernel: p_t from the per-workgroup bests, its mask bit,
//                         k_o(X, c_p) and k_o(c_{p_r}, c_p)
//   record  1 wave        m_t = mu[:, p_t] to believed[t] and, with p_t, to the read-back record
//   D2H     40 bytes      the record into host_ws, then an event
//   update                bucb_matvec_kernel, bucb_coef_kernel and the variance pass
//                         (bucb_cand_kernel without kSelect), enqueued BEFORE the host waits
//   host                  waits for the event only, decomposes front_t (bo_hvi_boxes), builds the
//                         edge tables (bo_ehvi_tables) into host_ws and enqueues one upload -- while
//                         the variance pass occupies the device
// One host staging block suffices: the host rewrites it only after the next pick's event, and
// stream order puts that event after the upload that read the block.
#include "bo_bucb_impl.h"   // first: its kernels keep the default contraction (see bo_ehvi_impl.h)
#include "bo_ehvi_impl.h"

namespace {

constexpr int kKbMinThreads = 64;      // the smallest workgroup of a scan: sizes the per-workgroup bests

// what the selection epilogue of a scan reads and writes
struct KbSel {
  const unsigned int* mask;    // the call's own mask: the caller's bits plus the picks
  TopEntry* partial;           // [workgroups of this scan]
  long long cand_offset;
};

// the read-back record of one pick
struct KbRec {
  long long p;                 // local index, -1 = no candidate left
  double m[4];
};

// the workgroup's best unmasked candidate of this scan; `red`: blockDim.x / 64 entries of LDS
__device__ __forceinline__ void kb_select(double acq, long long i, bool valid, const KbSel& s, TopEntry* red) {
  long long gi = -1;
  if (valid && !((s.mask[i >> 5] >> (i & 31)) & 1u)) gi = s.cand_offset + i;
  const TopEntry b = bo_block_best(acq, gi, red);
  if (threadIdx.x == 0) s.partial[blockIdx.x] = b;
}

// ehvi_direct_kernel with the selection epilogue (a.acq may be NULL: nothing is stored)
template <int M>
__global__ __launch_bounds__(256) void kb_direct_kernel(const EhviArgs a, const KbSel s) {
  __shared__ TopEntry s_red[256 / 64];
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool valid = i < a.n;
  double mu[M], sg[M], rs[M];
  const bool nan = ehvi_load<M>(a, i, valid, mu, sg, rs);
  const double h = ehvi_direct_value<M>(a, mu, sg, rs);
  const double acq = nan ? __builtin_nan("") : h;
  if (valid && a.acq) bo_out_store(a.acq + i, acq);
  kb_select(acq, i, valid, s, s_red);
}

// ehvi_table_kernel with the selection epilogue.  The reduction's T / 64 entries take the place
// of the table's first words once every thread has finished its walk (the barrier below), so the
// kernel has no static LDS and the table form's admission rule (8 S T <= 160 KiB) holds unchanged.
template <int M, int T>
__global__ __launch_bounds__(T) void kb_table_kernel(const EhviArgs a, const KbSel s) {
  extern __shared__ double kb_tab[];
  const long long i = (long long)blockIdx.x * T + threadIdx.x;
  const bool valid = i < a.n;
  double mu[M], sg[M], rs[M];
  const bool nan = ehvi_load<M>(a, i, valid, mu, sg, rs);
  const double h = ehvi_table_value<M, T>(a, kb_tab + threadIdx.x, mu, sg, rs);
  const double acq = nan ? __builtin_nan("") : h;
  if (valid && a.acq) bo_out_store(a.acq + i, acq);
  __syncthreads();                                   // every column has been walked
  kb_select(acq, i, valid, s, (TopEntry*)kb_tab);
}

// m_t = mu[:, p_t] (NaN when no candidate was left) to believed[t] and the read-back record
__global__ __launch_bounds__(64) void kb_record_kernel(BucbArgs a, const double* mu, double* believed, int t,
                                                       KbRec* rec) {
  const int o = threadIdx.x;
  const long long p = a.pick[t];
  if (o == 0) rec->p = p;
  if (o < 4) {
    const double v = (o < a.n_obj && p >= 0) ? mu[(long long)o * a.ld + p] : __builtin_nan("");
    rec->m[o] = v;
    if (o < a.n_obj) believed[t * a.n_obj + o] = v;
  }
}

int launch_kb_direct(const EhviArgs& e, const KbSel& sel, int m, hipStream_t s) {
  const dim3 g((unsigned)ehvi_blocks(e.n, 256));
  switch (m) {
    case 1: hipLaunchKernelGGL(kb_direct_kernel<1>, g, dim3(256), 0, s, e, sel); break;
    case 2: hipLaunchKernelGGL(kb_direct_kernel<2>, g, dim3(256), 0, s, e, sel); break;
    case 3: hipLaunchKernelGGL(kb_direct_kernel<3>, g, dim3(256), 0, s, e, sel); break;
    case 4: hipLaunchKernelGGL(kb_direct_kernel<4>, g, dim3(256), 0, s, e, sel); break;
    default: return BO_ERR_UNSUPPORTED;
  }
  BO_CHECK_HIP(hipGetLastError());
  return BO_OK;
}

template <int M, int T>
int launch_kb_table_mt(const EhviArgs& e, const KbSel& sel, int sum_e, hipStream_t s) {
  size_t lds = (size_t)sum_e * T * sizeof(double);
  if (lds < (T / 64) * sizeof(TopEntry)) lds = (T / 64) * sizeof(TopEntry);   // no edges: the reduction alone
  if (lds > 64 * 1024)
    BO_CHECK_HIP(hipFuncSetAttribute((const void*)kb_table_kernel<M, T>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds));
  hipLaunchKernelGGL((kb_table_kernel<M, T>), dim3((unsigned)ehvi_blocks(e.n, T)), dim3(T), lds, s, e, sel);
  BO_CHECK_HIP(hipGetLastError());
  return BO_OK;
}

template <int M>
int launch_kb_table_m(const EhviArgs& e, const KbSel& sel, int sum_e, int threads, hipStream_t s) {
  switch (threads) {
    case 256: return launch_kb_table_mt<M, 256>(e, sel, sum_e, s);
    case 128: return launch_kb_table_mt<M, 128>(e, sel, sum_e, s);
    case 64: return launch_kb_table_mt<M, 64>(e, sel, sum_e, s);
    default: return BO_ERR_UNSUPPORTED;
  }
}

// One pick's scan: the form and the workgroup size by bo_expected_hypervolume_improvement's rule
// for these boxes; *n_part = the workgroups that wrote a best entry.
int launch_scan(EhviArgs e, const KbSel& sel, int m, int form, const int32_t* n_edges, long long* n_part,
                hipStream_t s) {
  int sum_e = 0, threads = 0;
  bool table = false;
  const int st = ehvi_plan(form, m, e.n_boxes, true, true, n_edges, &e, &sum_e, &threads, &table);
  if (st != BO_OK) return st;
  if (!table) {
    *n_part = ehvi_blocks(e.n, 256);
    return launch_kb_direct(e, sel, m, s);
  }
  *n_part = ehvi_blocks(e.n, threads);
  switch (m) {
    case 1: return launch_kb_table_m<1>(e, sel, sum_e, threads, s);
    case 2: return launch_kb_table_m<2>(e, sel, sum_e, threads, s);
    case 3: return launch_kb_table_m<3>(e, sel, sum_e, threads, s);
    case 4: return launch_kb_table_m<4>(e, sel, sum_e, threads, s);
    default: return BO_ERR_UNSUPPORTED;
  }
}

// The device workspace: the update's regions (bo_bucb_impl.h), then the scan's; and the host
// staging block.  One pick's boxes, edges and box indices are packed back to back ("tab"), so
// that one copy uploads them.
struct KbLayout {
  Layout b;
  size_t partial, tab, rec, total;          // device
  size_t h_rec, h_front, h_tab, h_total;    // host
  size_t tab_bytes;
  int64_t edge_cap;
};

// the update's fields of `d` (bo_bucb_impl.h takes the candidates as bo_cand_desc(d))
bo_bucb_desc update_desc(const bo_kb_desc* d) {
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

bool make_kb_layout(const bo_kb_desc* d, KbLayout* L) {
  if (!d) return false;
  if (d->n_obj < 1 || d->n_obj > 4 || d->form < 0 || d->form > 2) return false;
  if (d->n_front < 0 || d->n_front > ((int64_t)1 << 20) || d->box_capacity < 1 ||
      d->box_capacity > ((int64_t)1 << 26) || d->n_cand > ((int64_t)1 << 36))
    return false;
  for (int k = 0; k < d->n_obj; ++k)
    if (!(d->ref_point[k] - d->ref_point[k] == 0.0)) return false;          // NaN or infinite
  const bo_bucb_desc b = update_desc(d);
  if (!make_layout(&b, bo_cand_desc(d), &L->b)) return false;
  const size_t m = (size_t)d->n_obj, cap = (size_t)d->box_capacity;
  L->edge_cap = (int64_t)m * (d->n_front + d->q + 1);
  L->tab_bytes = align256(cap * 2 * m * 8 + (size_t)L->edge_cap * 8 + cap * 2 * m * 4);
  size_t off = L->b.total;
  auto take = [&](size_t bytes) { const size_t at = off; off += align256(bytes); return at; };
  L->partial = take((size_t)ehvi_blocks(d->n_cand, kKbMinThreads) * sizeof(TopEntry));
  L->tab = take(L->tab_bytes);
  L->rec = take(sizeof(KbRec));
  L->total = off;
  off = 0;
  L->h_rec = take(sizeof(KbRec));
  L->h_front = take((size_t)(d->n_front + d->q) * m * 8);
  L->h_tab = take(L->tab_bytes);
  L->h_total = off;
  return true;
}

struct EventGuard {
  hipEvent_t ev = nullptr;
  ~EventGuard() { if (ev) (void)hipEventDestroy(ev); }
};

}  // namespace

extern "C" {

size_t bo_select_batch_kb_workspace_size(const bo_kb_desc* d) {
  KbLayout L;
  if (!make_kb_layout(d, &L)) return 0;
  return L.total;
}

size_t bo_select_batch_kb_host_workspace_size(const bo_kb_desc* d) {
  KbLayout L;
  if (!make_kb_layout(d, &L)) return 0;
  return L.h_total;
}

int bo_select_batch_kb(const bo_kb_desc* d, void* ws, size_t ws_bytes, void* stream) {
  KbLayout L;
  if (!make_kb_layout(d, &L)) return BO_ERR_ARG;
  if (!d->x_train || !d->kinv || !d->mu || !d->var || !d->top_val || !d->top_idx || !d->believed) return BO_ERR_ARG;
  if (d->cand_kind != BO_CAND_GRID && !d->cand) return BO_ERR_ARG;
  if (d->n_front > 0 && !d->front) return BO_ERR_ARG;
  if (d->var_out == d->var || d->var_out == d->mu) return BO_ERR_ARG;       // the inputs stay as they are
  if (!d->host_ws || d->host_ws_bytes < L.h_total) return BO_ERR_WORKSPACE;
  if (!ws || ws_bytes < L.total) return BO_ERR_WORKSPACE;
  if (((uintptr_t)ws & 15) != 0 || ((uintptr_t)d->host_ws & 7) != 0) return BO_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (s) {                                           // the host waits inside the call: not capturable
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return BO_ERR_UNSUPPORTED;
  }
  const bo_bucb_desc bd = update_desc(d);
  BucbArgs a;
  const int st_args = fill_args(&bd, bo_cand_desc(d), L.b, ws, &a);
  if (st_args != BO_OK) return st_args;
  const int m = d->n_obj, q = d->q;
  char* base = (char*)ws;
  char* hbase = (char*)d->host_ws;
  a.partial = (TopEntry*)(base + L.partial);         // one entry per workgroup of the narrowest scan
  char* dtab = base + L.tab;
  KbRec* drec = (KbRec*)(base + L.rec);
  KbRec* hrec = (KbRec*)(hbase + L.h_rec);
  double* hfront = (double*)(hbase + L.h_front);
  char* htab = hbase + L.h_tab;
  int64_t n_front = d->n_front, n_boxes = 0, boxes_max = 0;
  if (n_front > 0) memcpy(hfront, d->front, (size_t)n_front * m * 8);
  if (d->n_boxes_max) *d->n_boxes_max = 0;
  int32_t n_edges[4] = {0, 0, 0, 0};
  size_t used = 0, off_edges = 0, off_idx = 0;       // this pick's packing of the staging block

  // boxes, edges and box indices of the current front into the host staging block
  auto decompose = [&]() -> int {
    const int st = bo_hvi_boxes(hfront, n_front, m, d->ref_point, (double*)htab, d->box_capacity, &n_boxes);
    if (n_boxes > boxes_max) boxes_max = n_boxes;
    if (d->n_boxes_max) *d->n_boxes_max = boxes_max;
    if (st != BO_OK) return st;                      // BO_ERR_WORKSPACE: the count is in *n_boxes_max
    // packed: the boxes, then room for every edge there can be (an axis has at most
    // n_front + q + 1), then the indices
    off_edges = (size_t)n_boxes * 2 * m * 8;
    off_idx = off_edges + (size_t)L.edge_cap * 8;
    used = n_boxes > 0 ? off_idx + (size_t)n_boxes * 2 * m * 4 : 0;
    return bo_ehvi_tables((const double*)htab, n_boxes, m, (double*)(htab + off_edges), L.edge_cap, n_edges,
                          (int32_t*)(htab + off_idx));
  };

  const int st_first = decompose();                  // before anything is launched
  if (st_first != BO_OK) return st_first;
  EventGuard g;
  BO_CHECK_HIP(hipEventCreateWithFlags(&g.ev, hipEventDisableTiming));
  const int st_start = start_call(a, d->mask, s);
  if (st_start != BO_OK) return st_start;
  const unsigned blocks = (unsigned)L.b.blocks;
  BO_CHECK_HIP(launch_cand_dim(a, -1, 0, blocks, s));     // the running variance starts as `var`
  KbSel sel;
  sel.mask = a.mask;
  sel.partial = a.partial;
  sel.cand_offset = d->cand_offset;
  for (int t = 0; t < q; ++t) {
    const bool last = t == q - 1;
    const bool update = !last || d->var_out != nullptr;   // the last update only feeds var_out
    if (used > 0) BO_CHECK_HIP(hipMemcpyAsync(dtab, htab, used, hipMemcpyHostToDevice, s));
    if (last) BO_CHECK_HIP(hipEventRecord(g.ev, s));      // the last read of the staging block
    EhviArgs e;
    memset(&e, 0, sizeof(e));
    e.acq = t == 0 && d->acq_first ? d->acq_first : (last ? d->acq_last : nullptr);
    e.mu = d->mu;
    e.var = a.var_run;
    e.ld = d->ld;
    e.n = d->n_cand;
    e.boxes = (const double*)dtab;
    e.edges = (const double*)(dtab + off_edges);
    e.box_idx = (const int*)(dtab + off_idx);
    e.n_boxes = n_boxes;
    long long n_part = 0;
    const int st_scan = launch_scan(e, sel, m, d->form, n_edges, &n_part, s);
    if (st_scan != BO_OK) {                               // form 2 and this pick's table does not fit
      (void)hipStreamSynchronize(s);                      // the upload has read the staging block
      return st_scan;
    }
    if (q == 1 && d->acq_first && d->acq_last)            // one pick: acq_1 is acq_q
      BO_CHECK_HIP(hipMemcpyAsync(d->acq_last, d->acq_first, (size_t)d->n_cand * 8, hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(bucb_pick_kernel, dim3(1), dim3(1024), 0, s, a, t, n_part, update ? 1 : 0);
    BO_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(kb_record_kernel, dim3(1), dim3(64), 0, s, a, d->mu, d->believed, t, drec);
    BO_CHECK_HIP(hipGetLastError());
    if (!last) {
      BO_CHECK_HIP(hipMemcpyAsync(hrec, drec, sizeof(KbRec), hipMemcpyDeviceToHost, s));
      BO_CHECK_HIP(hipEventRecord(g.ev, s));
    }
    if (update) {
      const int st_w = launch_weights(a, t, s);
      if (st_w != BO_OK) return st_w;
      BO_CHECK_HIP(launch_cand_dim(a, t, 0, blocks, s));
    }
    if (last) break;
    // The host step, while the variance pass runs.  The event also orders this rewrite of the
    // staging block after the upload that read it (enqueued before this pick's scan).
    BO_CHECK_HIP(hipEventSynchronize(g.ev));
    if (hrec->p >= 0) {                              // no candidate left: the front stays as it is
      for (int k = 0; k < m; ++k) hfront[n_front * m + k] = hrec->m[k];
      ++n_front;
    }
    const int st_dec = decompose();
    if (st_dec != BO_OK) return st_dec;
  }
  // host_ws is the caller's again on return: wait for the last upload out of it (pick q's scan
  // and update are enqueued already and may still be running)
  BO_CHECK_HIP(hipEventSynchronize(g.ev));
  return BO_OK;
}

}  // extern "C"
