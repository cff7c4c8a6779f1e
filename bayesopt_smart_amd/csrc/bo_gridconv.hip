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
// The setup is a role block of the prep launch (conv_setup_block, bo_predict_impl.h); then three launches, each
// returning at once unless the device flag (predict_prep_kernel) says that every training point is a grid
// point: conv_list_kernel (the pair list and Tm), conv_acc_kernel (T) and conv_contract_kernel (the two GEMMs,
// the epilogue and the selection), each described where it stands.
// No floating-point atomics (the tickets are integers and order work, not sums); every sum runs
// in an order fixed by the inputs alone, and the K order of an output element does not depend on
// its tile, so shards reproduce the single call.

#include "bo_predict_impl.h"

namespace {

using namespace bo;   // ConvArgs, ConvSched and the kConv* constants they share with the setup block

constexpr int kListWaves = 4;            // waves per workgroup of the list kernel, one tau each
constexpr int kListChunk = 512;          // pairs of one tau staged in LDS at a time (per wave)
// rows per lane of a work item.  BO_BUILD_VARIANT=DEF_ACC_RB=16 builds the other candidate (A/B in
// DESIGN.md §9)
#ifndef BO_ACC_RB
#define BO_ACC_RB 8
#endif
constexpr int kAccRB = BO_ACC_RB;
constexpr int kAccRows = 64 * kAccRB;    // rows of a work item (tau, row block)
constexpr int kAccUnroll = 4;            // list entries loaded ahead of their terms
constexpr int kClassLists = kConvClasses * kConvShards;   // the class lists of the accumulate kernel's work order
static_assert(kClassLists % 64 == 0 && kClassLists <= 2 * 64 * kConvAccWaves &&
              (kConvShards & (kConvShards - 1)) == 0 && kConvShards <= 16 && kConvShards <= kConvCountStride,
              "conv_acc_kernel's scan and lookup of the class lists");
#ifndef BO_CONV_PF
#define BO_CONV_PF 3                      // BO_BUILD_VARIANT=DEF_CONV_PF=6: the A/B of DESIGN.md §9.6 item 6
#endif
constexpr int kConvPF = BO_CONV_PF;      // A-operand prefetch depth of the contraction (k-blocks)
constexpr int kContractWaves = 8;        // most waves of a contraction workgroup: two per SIMD, 256 VGPRs each
constexpr size_t kConvLdsBytes = 160 * 1024;
// a pair whose |w_nm| is below kPairDrop pv for every objective is left out of the list: at most
// N (N + 1) / 2 of them, so q / pv loses less than 1e-24 for N <= 4096
constexpr double kPairDrop = 0x1p-100;
// entries of the contraction's tables below kTabFlush are stored as +0.0: the k-blocks whose
// entries are all zero for a tile add nothing to it and are not run
constexpr double kTabFlush = 0x1p-128;

// The dynamic LDS of each kernel, described once: the kernel carves its pointers from the layout and
// launch_gridconv takes the launch's bytes from the same object.
struct ListLds {         // ints: cstart[C + 1] | order[n] | rc[2n] | nm[kListWaves][kListChunk]
  int order, rc, nm;
  size_t bytes;
  __host__ __device__ ListLds(int n, int C)
      : order(C + 1), rc(order + n), nm(rc + 2 * n), bytes((size_t)(nm + kListWaves * kListChunk) * sizeof(int)) {}
};
struct AccLds {          // doubles: tabE[2][2R]; then ints, to a whole double: cst[kClassLists + 1] | part[waves]
  int ints, part;        // `ints` in doubles, `part` in ints from there
  size_t bytes;
  __host__ __device__ explicit AccLds(int R)
      : ints(4 * R), part(kClassLists + 1),
        bytes((size_t)ints * sizeof(double) + (size_t)(part + kConvAccWaves + 1) / 2 * 2 * sizeof(int)) {}
};
struct ContractLds {     // doubles: tabB[2][HB] | tabH[Cpad + C - 1] | hband[2] (ints, one double); then ints: cn[NP],
                         // a training point's column in the low 16 bits and its row above them (both < 2^15);
                         // the doubles are the workspace's image of an objective's tables (conv_ctab_doubles)
  int HB, tabH, hband, cn;
  size_t bytes;          // the tables, or the `lists` top-q entries that the waves of a workgroup merge from offset 0
                         // once the tables are done with (more than the tables only on a grid of a few columns)
  __host__ __device__ ContractLds(int C, int Cpad, int LT, int NP, int lists = 0)
      : HB(Cpad + LT / 2), tabH(2 * HB), hband(tabH + Cpad + C - 1), cn(hband + 1),
        bytes((size_t)cn * sizeof(double) + (size_t)NP * sizeof(int)) {
    if (bytes < (size_t)lists * sizeof(TopEntry)) bytes = (size_t)lists * sizeof(TopEntry);
  }
};

// ---------------------------------------------------------------------------------------
// Pair list.  blockIdx.x < tau_blocks: the lists of kListWaves values of tau; the tm_blocks after
// them: Tm for every objective; the blocks after those: the exp tables of the two kernels behind
// this one, once per call and distinct length scale (conv_tables).
//
// One tau is one WAVE's: the pairs (n <= m, c_n + c_m = tau) in (n ascending, m in bucket order)
// order -- lane l owns a contiguous range of n, counts its pairs (the partner bucket is column
// tau - c_n, the m >= n of it), a wave scan gives every n its place in the list -- written to the
// workspace at pstart[tau] as the table base of r_n + r_m (once) and w_nm (per objective; the
// integer part of the list is the same for every objective).  pstart[tau], the pairs of every
// smaller tau, is the wave's own sum over the column buckets (no counts of other tau, no scan; the
// layout is that of an exclusive scan of the counts), written for the accumulate kernel.
// Only the pairs with |w_nm| >=
// kPairDrop pv for some objective are written, closed up in unchanged order (a ballot per 64 pairs
// and the wave's running count); pkept[tau] is their number (0 for an empty tau and for the padding
// tau up to LT).  The criterion reads the call's inputs alone, so every shard keeps the same pairs.
// E table of the accumulate kernel, split by parity so that consecutive rows read consecutive doubles:
//   E(2i - sigma) = tabE[par * 2R + i + (s >> 1)],  s = 2R - 2 - sigma,  par = s & 1.
// ---------------------------------------------------------------------------------------
// The end of a tau's list wave: pkept; a tau that kept nothing (empty, padding, or every pair dropped)
// gets its T rows written here as +0.0 and is no item of the accumulate kernel; with tickets (dyn) a
// tau that kept k pairs is appended to the list of its class and shard.
__device__ __forceinline__ void conv_list_done(const ConvArgs& a, int tau, int kept, int lane, int dyn) {
  if (kept == 0) {
    for (int o = 0; o < a.n_obj; ++o) {
      double* row = a.T + ((size_t)o * a.LT + tau) * a.ldr;
      for (int i = lane; i < a.ldr; i += 64) row[i] = 0.0;
    }
  }
  if (lane == 0) {
    a.pkept[tau] = kept;
    if (dyn && kept > 0) {
      const int e = 31 - __clz(kept);
      const int cls = 2 * e + (e > 0 ? (kept >> (e - 1)) & 1 : 0);
      const int sh = tau & (kConvShards - 1);
      const int slot = atomicAdd(a.ccount + cls * kConvCountStride + sh, 1);
      a.clist[(size_t)(cls * kConvShards + sh) * (a.LT / kConvShards) + slot] = tau;
    }
  }
}

// The tables of the accumulate kernel (tabE, described above) and of the contraction (tabB, tabH and the bands,
// described there), written to the workspace by thread t0 of nthr: they depend on (l_o, R, C) alone, so the
// objective that is the first with its length scale builds them and every workgroup behind copies them.
// Contraction entries below kTabFlush become +0.0 (a NaN entry compares false and stays); a band is the
// largest |t| that the same comparison kept, raised from the setup block's zero by one integer atomicMax per
// wave (integer maxima: no order in them).
__device__ __forceinline__ void conv_tables(const ConvArgs& a, int t0, int nthr, int lane) {
  const int R2 = 2 * a.R;
  const ContractLds L(a.C, a.Cpad, a.LT, a.NP);
  for (int o = 0; o < a.n_obj; ++o) {
    if (a.tix[o] != o) continue;
    const double nhl = a.nhl[o];
    double* tabE = a.tabE + (size_t)o * 2 * R2;
    for (int t = t0; t < 2 * R2; t += nthr) {
      const int par = t >= R2 ? 1 : 0, h = t - par * R2;
      const double m = (double)(2 * h + par - (R2 - 2));
      tabE[t] = exp(0.5 * nhl * (m * m));
    }
    double* tabB = a.ctab + (size_t)o * conv_ctab_doubles(a.C, a.Cpad, a.LT);
    double* tabH = tabB + L.tabH;
    int mq = 0;
    int mm = 0;
    for (int t = t0; t < 2 * L.HB; t += nthr) {
      const int par = t >= L.HB ? 1 : 0, h = t - par * L.HB;
      const int mi = 2 * h + par - (a.LT - 1);
      const double m = (double)mi;
      const double v = exp(0.5 * nhl * (m * m));
      const bool flush = v < kTabFlush;
      tabB[t] = flush ? 0.0 : v;
      if (!flush) mq = max(mq, abs(mi));
    }
    for (int t = t0; t < a.Cpad + a.C - 1; t += nthr) {
      const int mi = t - (a.C - 1);
      const double m = (double)mi;
      const double v = exp(nhl * (m * m));
      const bool flush = v < kTabFlush;
      tabH[t] = flush ? 0.0 : v;
      if (!flush) mm = max(mm, abs(mi));
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      mq = max(mq, __shfl_xor(mq, d, 64));
      mm = max(mm, __shfl_xor(mm, d, 64));
    }
    if (lane == 0) {
      int* hband = (int*)(tabB + L.hband);
      atomicMax(hband, mq);
      atomicMax(hband + 1, mm);
    }
  }
}

__global__ __launch_bounds__(64 * kListWaves) void conv_list_kernel(const ConvArgs a, int tau_blocks, int tm_blocks,
                                                                    int dyn) {
  if (__builtin_amdgcn_readfirstlane(*a.flag) != 0) return;
  const int tid = threadIdx.x;
  if ((int)blockIdx.x >= tau_blocks + tm_blocks) {
    conv_tables(a, (blockIdx.x - tau_blocks - tm_blocks) * (64 * kListWaves) + tid,
                (gridDim.x - tau_blocks - tm_blocks) * (64 * kListWaves), tid & 63);
    return;
  }
  if ((int)blockIdx.x >= tau_blocks) {
    // Tm[o][s][i] = pv alpha_n H(i - r_n), n = order[s]; rows s >= N are zero
    const long long total = (long long)a.NP * a.ldr;
    const long long stride = (long long)tm_blocks * (64 * kListWaves);
    for (int o = 0; o < a.n_obj; ++o) {
      const double nhl = a.nhl[o], pv = a.pv[o];
      double* tm = a.Tm + (size_t)o * a.NP * a.ldr;
      for (long long t = (long long)(blockIdx.x - tau_blocks) * (64 * kListWaves) + tid; t < total; t += stride) {
        const int s = (int)(t / a.ldr), i = (int)(t - (long long)s * a.ldr);
        double v = 0.0;
        if (s < a.n && i < a.nrows) {
          const int n = a.order[s];                           // rows in column-bucketed order
          const double d = (double)(a.row_lo + i - a.rc[2 * n]);
          v = pv * a.alpha[(size_t)o * a.n_pad + n] * exp(nhl * (d * d));
        }
        tm[t] = v;
      }
    }
    return;
  }
  extern __shared__ __attribute__((aligned(16))) int si[];
  const ListLds L(a.n, a.C);
  int* cstart = si;
  int* order = si + L.order;
  int* rc = si + L.rc;
  for (int t = tid; t <= a.C; t += 64 * kListWaves) cstart[t] = a.cstart[t];
  for (int t = tid; t < a.n; t += 64 * kListWaves) order[t] = a.order[t];
  for (int t = tid; t < 2 * a.n; t += 64 * kListWaves) rc[t] = a.rc[t];
  __syncthreads();
  const int lane = tid & 63, wave = tid >> 6;
  int* nm = si + L.nm + wave * kListChunk;             // the wave's slice: (n, m) in 16 + 16 bits
  const int tau = blockIdx.x * kListWaves + wave;
  if (tau >= a.LT) return;
  // the pairs n <= m with c_n + c_m < t, from the column buckets alone: with h[c] the points of column
  // c and cum(x) = cstart[clamp(x, 0, C)], the ordered pairs are sum_c h[c] cum(t - c); the n = m among
  // them (2 c_n < t) were counted once, every other pair twice.  At most n^2 + n <= 2^24 + 2^12.
  int s0 = 0, s1 = 0;                                 // t = tau and t = tau + 1
  for (int c = lane; c < a.C; c += 64) {
    const int h = cstart[c + 1] - cstart[c];
    const int x0 = tau - c, x1 = x0 + 1;
    s0 += h * cstart[x0 < 0 ? 0 : x0 > a.C ? a.C : x0];
    s1 += h * cstart[x1 < 0 ? 0 : x1 > a.C ? a.C : x1];
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    s0 += __shfl_xor(s0, d, 64);
    s1 += __shfl_xor(s1, d, 64);
  }
  const int h0 = (tau + 1) >> 1, h1 = (tau + 2) >> 1;
  const int p0 = __builtin_amdgcn_readfirstlane((s0 + cstart[h0 > a.C ? a.C : h0]) >> 1);
  const int total = __builtin_amdgcn_readfirstlane((s1 + cstart[h1 > a.C ? a.C : h1]) >> 1) - p0;
  if (lane == 0) a.pstart[tau] = p0;
  if (total == 0) {                                   // (the padding tau >= 2C - 1 among them)
    conv_list_done(a, tau, 0, lane, dyn);
    return;
  }
  const int R2 = 2 * a.R;
  const int per = (a.n + 63) / 64;
  const int n_lo = lane * per < a.n ? lane * per : a.n;
  const int n_hi = n_lo + per < a.n ? n_lo + per : a.n;
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
  const int first = incl - mine;
  int kept = 0;                                       // pairs of this tau written so far (wave-uniform)
  // kListChunk pairs at a time: the lanes that own them write (n, m) to the wave's slice in list
  // order; then a lane per pair, so that the K^-1 loads of 64 pairs are in flight together and the
  // list is written in whole lines
  for (int cb = 0; cb < total; cb += kListChunk) {
    const int cnt = total - cb < kListChunk ? total - cb : kListChunk;
    if (first < cb + cnt && first + mine > cb) {
      int pos = first;
      for (int n = n_lo; n < n_hi; ++n) {
        const int pc = tau - rc[2 * n + 1];
        if (pc < 0 || pc >= a.C) continue;
        for (int s = cstart[pc]; s < cstart[pc + 1]; ++s) {
          const int m = order[s];
          if (m < n) continue;
          if (pos >= cb && pos < cb + cnt) nm[pos - cb] = n | (m << 16);
          ++pos;
        }
      }
    }
    // the wave's own LDS slice: written by some lanes, read by all
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int pb = 0; pb < cnt; pb += 64) {
      const int p = pb + lane;
      // the objectives' weights in registers (the loop over BO_MAX_OBJ is unrolled: no indexed array)
      double wv[BO_MAX_OBJ];
      int sl = 0;
      bool keep = false;
      if (p < cnt) {
        const int n = nm[p] & 65535, m = nm[p] >> 16;
        const int rn = rc[2 * n], cn = rc[2 * n + 1], rm = rc[2 * m];
        const double dr = (double)(rn - rm), dc = (double)(cn - (tau - cn));
        const int sp = R2 - 2 - (rn + rm);
        sl = (sp & 1) * R2 + (sp >> 1) + a.row_lo;
#pragma unroll
        for (int o = 0; o < BO_MAX_OBJ; ++o) {
          if (o < a.n_obj) {
            const double* ko = a.kinv + (size_t)o * a.ld_k * a.ld_k;
            const double nhl = a.nhl[o], pv = a.pv[o];
            const double sym = m == n ? ko[(size_t)n * a.ld_k + n]
                                      : ko[(size_t)n * a.ld_k + m] + ko[(size_t)m * a.ld_k + n];
            // (2 - delta) A_nm = K^-1[n][m] + K^-1[m][n] off the diagonal; the library's exp
            wv[o] = sym * (pv * pv) * exp(0.5 * nhl * (dr * dr + dc * dc));
            // a pair is dropped when it is negligible for every objective (the list is shared); a
            // non-finite weight compares false and is kept
            keep = keep || !(fabs(wv[o]) < kPairDrop * pv);
          }
        }
      }
      // the kept pairs close up in list order: a lane's slot is the kept count before it
      const unsigned long long kb = __ballot(keep);
      if (keep) {
        const int dst = p0 + kept + __popcll(kb & ((1ull << lane) - 1ull));
        a.pair_sl[dst] = sl;
#pragma unroll
        for (int o = 0; o < BO_MAX_OBJ; ++o)
          if (o < a.n_obj) a.pair_w[(size_t)o * a.n_pairs + dst] = wv[o];
      }
      kept += __popcll(kb);
    }
    // the slice is rewritten by the next chunk
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  conv_list_done(a, tau, kept, lane, dyn);
}

// ---------------------------------------------------------------------------------------
// Accumulate.  blockIdx.y = objective.  A work item is (tau, block of kAccRows rows) of a tau that
// kept pairs; item t of an objective is row block t % nrb of the tau at position t / nrb of the class
// lists, taken from the class of the longest lists down (a class spans a factor below 2 in length:
// longest first up to that; the exact sort gave the same makespan in the greedy model of DESIGN.md §9).
// Persistent waves take the items through the objective's ticket (one lane's integer atomicAdd);
// no wave waits for another.  A wave runs down its tau's list -- w and the table base are
// wave-uniform loads -- and accumulates w E(2i - sigma) in list order, kAccRB rows per lane, with a
// compensated sum.  A T entry is produced by one wave in list order: neither the ticket order nor the
// order inside a class list is in any value.  Without tickets (no more items than waves) item t's tau
// is t / nrb, and a tau that kept nothing is skipped.
// ---------------------------------------------------------------------------------------
// FULL: every row of the block is a row of the shard (the table offsets of the lane's rows are
// immediates); else rows past the shard's (the padding to ldr) read a valid table entry and are
// written as zero
template <bool FULL>
__device__ __forceinline__ void conv_acc_item(const double* tabE, const double* __restrict__ w,
                                              const int* __restrict__ sl, int cnt, int ib, int lane, int nrows,
                                              int ldr, double* __restrict__ Trow) {
  // the row sums as unevaluated pairs hi + lo (two-sum and the product's FMA residual): the terms
  // of one T entry cancel to 1e-4 .. 1e-5 of their magnitude (the conditioning of K), and a plain
  // sum's partial sums would leave their rounding in T
  double hi[kAccRB], lo[kAccRB];
  int it[kAccRB];
#pragma unroll
  for (int k = 0; k < kAccRB; ++k) {
    const int i = ib + lane + 64 * k;
    it[k] = FULL ? 64 * k : (i < nrows ? i : nrows - 1);
    hi[k] = 0.0;
    lo[k] = 0.0;
  }
  const double* tb = FULL ? tabE + ib + lane : tabE;
  auto gather = [&](int s, double (&ev)[kAccRB]) {
    const double* e = tb + s;
#pragma unroll
    for (int k = 0; k < kAccRB; ++k) ev[k] = e[it[k]];
  };
  // the per-term operation sequence of the one-kernel pair stage, unchanged
  auto term = [&](double wv, const double (&ev)[kAccRB]) {
#pragma unroll
    for (int k = 0; k < kAccRB; ++k) {
      const double t = __dmul_rn(wv, ev[k]);
      const double te = __builtin_fma(wv, ev[k], -t);
      const double s2 = __dadd_rn(hi[k], t);
      const double bb = __dsub_rn(s2, hi[k]);
      const double se = __dadd_rn(__dsub_rn(hi[k], __dsub_rn(s2, bb)), __dsub_rn(t, bb));
      hi[k] = s2;
      lo[k] = __dadd_rn(lo[k], __dadd_rn(se, te));
    }
  };
  // kAccUnroll list entries per round: their (wave-uniform) loads go out together, and the table
  // gathers of an entry are issued before the terms of the entry before it
  int p = 0;
  for (; p + kAccUnroll <= cnt; p += kAccUnroll) {
    double wv[kAccUnroll];
    int sv[kAccUnroll];
#pragma unroll
    for (int u = 0; u < kAccUnroll; ++u) {
      wv[u] = w[p + u];
      sv[u] = sl[p + u];
    }
    double ev[2][kAccRB];
    gather(sv[0], ev[0]);
#pragma unroll
    for (int u = 0; u < kAccUnroll; ++u) {
      if (u + 1 < kAccUnroll) gather(sv[u + 1], ev[(u + 1) & 1]);
      term(wv[u], ev[u & 1]);
    }
  }
  for (; p < cnt; ++p) {
    double ev[kAccRB];
    gather(sl[p], ev);
    term(w[p], ev);
  }
#pragma unroll
  for (int k = 0; k < kAccRB; ++k) {
    const int i = ib + lane + 64 * k;
    if (FULL) Trow[i] = hi[k] + lo[k];
    else if (i < ldr) Trow[i] = i < nrows ? hi[k] + lo[k] : 0.0;
  }
}

// (seven of ConvArgs' pointers again as __restrict__ parameters: the compiler's alias information)
__global__ __launch_bounds__(64 * kConvAccWaves) void conv_acc_kernel(
    const ConvArgs a, const double* __restrict__ pair_w, const int* __restrict__ pair_sl,
    const int* __restrict__ pstart, const int* __restrict__ pkept, const int* __restrict__ ccount,
    const int* __restrict__ clist, int* __restrict__ ticket, double* __restrict__ T, int nrb, int ngrp, int dyn) {
  if (__builtin_amdgcn_readfirstlane(*a.flag) != 0) return;
  extern __shared__ __attribute__((aligned(16))) double sd[];
  const int tid = threadIdx.x, lane = tid & 63, o = blockIdx.y;
  const int R2 = 2 * a.R;
  const AccLds L(a.R);
  double* tabE = sd;
  int* cst = (int*)(sd + L.ints);                     // first position of each class list
  int* part = cst + L.part;
  // the list kernel's table of this objective's length scale, 16 bytes per load
  const double2* te = (const double2*)(a.tabE + (size_t)a.tix[o] * 2 * R2);
  for (int t = tid; t < R2; t += 64 * kConvAccWaves) ((double2*)tabE)[t] = te[t];
  if (dyn) {
    // the class lists one after the other, the longest class first (the shards of a class in turn):
    // list j is class kConvClasses - 1 - j / kConvShards, shard j % kConvShards; an exclusive scan of their
    // lengths, two lists per thread
    int c[2], sum = 0;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int j = 2 * tid + u;
      c[u] = j < kClassLists ? ccount[(kConvClasses - 1 - j / kConvShards) * kConvCountStride + j % kConvShards] : 0;
      sum += c[u];
    }
    int incl = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int v = __shfl_up(incl, d, 64);
      if (lane >= d) incl += v;
    }
    if (lane == 63) part[tid >> 6] = incl;
    __syncthreads();
    int run = incl - sum;
    for (int w = 0; w < (tid >> 6); ++w) run += part[w];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int j = 2 * tid + u;
      if (j < kClassLists) cst[j] = run;
      run += c[u];
      if (j == kClassLists - 1) cst[kClassLists] = run;
    }
  }
  __syncthreads();
  // (with tickets: the tau that kept pairs; a tau that kept nothing has its rows from the list kernel)
  const int n_items = (dyn ? cst[kClassLists] : a.LT) * nrb;
  const double* wo = pair_w + (size_t)o * a.n_pairs;
  // group g = blockIdx.x % ngrp owns the items g, g + ngrp, ... and a ticket of its own; a wave's
  // first item is its own index in the group (the setup block starts the tickets behind them)
  const int g = blockIdx.x % ngrp;
  int* tk = ticket + (o * kConvTicketGroups + g) * kConvTicketStride;
  for (int k = (blockIdx.x / ngrp) * kConvAccWaves + (tid >> 6);;) {
    const int t = k * ngrp + g;
    if (t >= n_items) break;
    // the next ticket is taken before this item's work, which hides its round trip
    int nx = 0;
    if (dyn && lane == 0) nx = atomicAdd(tk, 1);
    const int oi = t / nrb, rb = t - oi * nrb;
    int tau = oi;
    if (dyn) {
      // the list that holds position oi: the first whose end is past it.  Lane l looks at the last
      // of its kClassLists / 64 lists, then the lanes at the lists of the lane found
      constexpr int per = kClassLists / 64;
      const unsigned long long b1 = __ballot(cst[per * lane + per] > oi);
      const int l1 = __builtin_ctzll(b1);
      const unsigned long long b2 = __ballot(cst[per * l1 + (lane < per ? lane : per - 1) + 1] > oi);
      const int j = per * l1 + __builtin_ctzll(b2);
      const int cls = kConvClasses - 1 - j / kConvShards;
      const int* list = clist + (size_t)(cls * kConvShards + j % kConvShards) * (a.LT / kConvShards);
      tau = __builtin_amdgcn_readfirstlane(list[oi - cst[j]]);
    }
    const int p0 = __builtin_amdgcn_readfirstlane(pstart[tau]);
    const int cnt = __builtin_amdgcn_readfirstlane(pkept[tau]);        // the pairs that the list kept
    if (!dyn && cnt == 0) break;           // its rows are the list kernel's
    const int ib = rb * kAccRows;
    double* Trow = T + ((size_t)o * a.LT + tau) * a.ldr;
    if (ib + kAccRows <= a.nrows) conv_acc_item<true>(tabE, wo + p0, pair_sl + p0, cnt, ib, lane, a.nrows, a.ldr, Trow);
    else conv_acc_item<false>(tabE, wo + p0, pair_sl + p0, cnt, ib, lane, a.nrows, a.ldr, Trow);
    if (!dyn) break;                       // no more items than waves: no tickets
    k = __builtin_amdgcn_readfirstlane(nx);
  }
}

// ---------------------------------------------------------------------------------------
// Contraction, epilogue and selection.  A wave owns 16 grid rows x TW = 16 NB columns (NB column blocks:
// NB accumulators per GEMM; NB = 4, 2 or 1, the plan's choice: plan_gridconv); the 8 or 4 waves of a
// workgroup take consecutive wave tiles (the same rows when a grid row has that many tiles: their A loads
// hit the L1).  Cpad is a multiple of 64 for every NB, and the k-blocks are the absolute 16-row blocks in
// ascending order: an output element's sum does not depend on NB.  Per k-block of 16:
//   A: lane (il = l & 15, g = l >> 4) loads X[k0 + 4g + s][i0 + il], s = 0..3 (X = T or Tm, k-major:
//      16 lanes read 128 contiguous bytes), through a kConvPF-deep register ring;
//   B: MFMA step s pairs lane group g with k = k0 + 4g + s:
//      variance  E(2j - tau) = tabB[par * HB + j + (u >> 1)], u = LT - 1 - tau, par = u & 1
//                (split by parity: consecutive columns read consecutive doubles);
//      mean      H(j - c_n)  = tabH[j - c_n + C - 1]; the rows of Tm and cn[] are the training points
//                in column-bucketed order (`order`), so the points near a tile are consecutive rows.
// The tables tabB, tabH and hband (ContractLds) are the list kernel's (conv_tables), copied from the workspace
// when the objective's table index changes.
// Bands: table entries below kTabFlush are stored as +0.0, and hband holds the largest |t| of an entry
// that the same comparison kept (hq for E, hm for H).  A tile of columns j0 .. j0 + TW - 1 runs
//   variance  the k-blocks that hold a tau of [2 j0 - hq, 2 (j0 + TW - 1) + hq],
//   mean      the k-blocks that hold a row of cstart[j0 - hm] .. cstart[j0 + TW + hm] - 1;
// every other k-block multiplies finite T / Tm by exact zeros, and acc + 0 = acc: the outputs are those
// of ConvArgs::full (every k-block), bit for bit, and do not depend on what a shard's tiles skipped.
// The k-blocks ascend for every tile alike; the accumulators are read behind mfma_fence.
// Selection: a wave keeps a top-q list over its tiles; at the end the waves of a workgroup merge theirs in LDS
// and the workgroup writes one list, so the grid is bounded by the lists the final merge reads (n_lists), not
// by the waves.  BO_BUILD_VARIANT=CT_NOOUT / CT_NOSEL / CT_BCONST / CT_ACONST are timing-only builds
// without the output stores, the selection, the B operand's LDS reads or the A operand's loads
// (its CT_NOTAB went with the table build, item 7).
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void conv_load_a(const double* __restrict__ X, int ldr, int kb, int g, double (&v)[4]) {
#ifdef BO_ABL_CT_ACONST
  // ablation (timing only): no A loads, the operand is one value read once
#pragma unroll
  for (int s = 0; s < 4; ++s) v[s] = X[0];
#else
  const double* p = X + (size_t)(16 * kb + 4 * g) * ldr;
#pragma unroll
  for (int s = 0; s < 4; ++s) v[s] = p[(size_t)s * ldr];
#endif
}

// acc[nb] += X[k-blocks][rows] . B; bgen(kb, bv) fills bv[s][nb], this lane's B values of k-block kb
// (k = 16 kb + 4 g + s, column block nb), for kb = 0 .. nkb - 1 in ascending order (nkb >= 1).  A band
// that starts at k-block kb_lo passes X advanced by 16 kb_lo rows and a bgen whose base is moved by
// as much: the first block is then in the pointers, not in a register that lives through the loop
// (with one, the contraction kernel needed scratch)
template <int NB, class BGen>
__device__ __forceinline__ void conv_gemm(const double* __restrict__ X, int ldr, int nkb, int g, d4 (&acc)[NB],
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
        double bv[4][NB];
        bgen(kb, bv);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) acc[nb] = mfma64(av[s], bv[s][nb], acc[nb]);
      }
    }
  }
}

// NB column blocks per wave tile; 4 or 8 waves per workgroup (blockDim.x, the plan's choice)
template <int NB>
__global__ __launch_bounds__(64 * kContractWaves) void conv_contract_kernel(const ConvArgs a) {
  if (__builtin_amdgcn_readfirstlane(*a.flag) != 0) return;
  extern __shared__ __attribute__((aligned(16))) double sd[];
  const ContractLds L(a.C, a.Cpad, a.LT, a.NP);
  double* tabB = sd;
  double* tabH = sd + L.tabH;
  // (the last entry of tabH's region is read by no tile: j - c_n + C - 1 <= Cpad + C - 2)
  int* hband = (int*)(sd + L.hband);                             // the bands of tabB and tabH: hq, hm
  int* cn = (int*)(sd + L.cn);
  constexpr int TW = 16 * NB;                                    // columns of a wave tile
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nt = blockDim.x, W = nt >> 6;
  const int g = lane >> 4, jl = lane & 15;
  const int cb_n = a.Cpad / TW;                                  // wave tiles along a grid row
  const long long n_wt = (long long)(a.ldr / 16) * cb_n;
  const long long gi_lo = a.cand_offset, gi_hi = a.cand_offset + a.n_cand;
#ifndef BO_ABL_CT_NOOUT
  const bool outs = true;
#else
  const bool outs = a.ld_out < 0;                                // ablation (timing only): false, and not known to be
#endif
  for (int t = tid; t < a.NP; t += nt) {
    const int n = t < a.n ? a.order[t] : -1;
    cn[t] = n >= 0 ? a.rc[2 * n + 1] | (a.rc[2 * n] << 16) : 0;
  }

  double lv = -__builtin_inf();                                  // the wave's top-q list, lanes 0..q-1
  long long li = -1;
  int tab_ix = -1;                                               // the objective whose tables are in LDS
  for (long long base = (long long)blockIdx.x * W; base < n_wt; base += (long long)gridDim.x * W) {
    const long long wt = base + wave;
    const bool active = wt < n_wt;
    const long long wtc = active ? wt : n_wt - 1;
    const int i0 = (int)(wtc / cb_n) * 16, j0 = (int)(wtc % cb_n) * TW;
    double acq[NB][4];
    for (int o = 0; o < a.n_obj; ++o) {
      // the tables depend on the length scale alone: copied only when it changes (one objective,
      // or equal length scales: once per workgroup; objectives with different length scales
      // on a grid of more wave tiles than 4 gridDim.x copy them per tile and objective, since
      // the acquisition sums the objectives of a tile in registers)
      const int tx = a.tix[o];
      if (tx != tab_ix) {
        __syncthreads();                                         // the previous tables are done with
        // the list kernel's image of tabB | tabH | hband, 16 bytes per load (and a last double of its own
        // when their doubles are odd: cn[] starts behind it)
        const double* src = a.ctab + (size_t)tx * conv_ctab_doubles(a.C, a.Cpad, a.LT);
        for (int t = tid; t < L.cn / 2; t += nt) ((double2*)sd)[t] = ((const double2*)src)[t];
        if ((L.cn & 1) && tid == 0) sd[L.cn - 1] = src[L.cn - 1];
        __syncthreads();                                         // hband stays until the next copy
        tab_ix = tx;
      }
      // variance k-blocks: those that hold a tau with E(2j - tau) != 0 for a column of the tile,
      // tau in [2 j0 - hq, 2 (j0 + TW - 1) + hq]; the others multiply T by exact zeros.  (A tile of padding
      // columns alone, j0 >= C, can have its band past the last tau: it runs the last k-block.)
      int kq_lo = 0, kq_hi = a.LT / 16;
      if (!a.full) {
        const int hq = hband[0];                                 // largest |t| whose E(t) was not flushed
        const int t_hi = 2 * (j0 + TW - 1) + hq < a.LT - 1 ? 2 * (j0 + TW - 1) + hq : a.LT - 1;
        const int t_lo = 2 * j0 - hq > 0 ? (2 * j0 - hq < t_hi ? 2 * j0 - hq : t_hi) : 0;
        // (wave-uniform, and told so: as lane values they made the k loop a divergent one)
        kq_lo = __builtin_amdgcn_readfirstlane(t_lo >> 4);
        kq_hi = __builtin_amdgcn_readfirstlane((t_hi >> 4) + 1);
      }
      d4 aq[NB], am[NB];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        aq[nb] = (d4){0.0, 0.0, 0.0, 0.0};
        am[nb] = (d4){0.0, 0.0, 0.0, 0.0};
      }
      const double* Tq = a.T + ((size_t)o * a.LT + 16 * kq_lo) * a.ldr + i0 + jl;
      // mean k-blocks: the rows are in column order, so the points of the columns
      // [j0 - hm, j0 + TW - 1 + hm] are the rows cstart[..] .. cstart[..] - 1; H is zero for the others
      int km_lo = 0, km_hi = a.NP / 16;
      if (!a.full) {
        const int hm = hband[1];
        const int c_hi = j0 + TW + hm < a.C ? j0 + TW + hm : a.C;
        const int c_lo = j0 - hm > 0 ? (j0 - hm < a.C ? j0 - hm : a.C) : 0;
        km_lo = __builtin_amdgcn_readfirstlane(a.cstart[c_lo] >> 4);
        km_hi = __builtin_amdgcn_readfirstlane((a.cstart[c_hi] + 15) >> 4);
      }
      const double* Tm = a.Tm + ((size_t)o * a.NP + 16 * km_lo) * a.ldr + i0 + jl;
      // variance: step s of lane group g is tau = 16 (kq_lo + kb) + 4 g + s; u = LT - 1 - tau is odd
      // for even s, and u >> 1 = hb (s = 0, 1) or hb - 1 (s = 2, 3), hb = LT/2 - 1 - 8 (kq_lo + kb) - 2 g
      // (>= 1)
      const double* pe0 = tabB + (a.LT / 2 - 1 - 8 * kq_lo - 2 * g) + j0 + jl;
#ifdef BO_ABL_CT_BCONST
      const double bconst = pe0[0];                              // ablation (timing only): B from a register
#endif
      conv_gemm<NB>(Tq, a.ldr, kq_hi - kq_lo, g, aq, [&](int kb, double (&bv)[4][NB]) {
#ifdef BO_ABL_CT_BCONST
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) bv[s][nb] = bconst;
#else
        const double* pe = pe0 - 8 * kb;                         // even u
        const double* po = pe + L.HB;                              // odd u
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
          bv[0][nb] = po[16 * nb];
          bv[1][nb] = pe[16 * nb];
          bv[2][nb] = po[16 * nb - 1];
          bv[3][nb] = pe[16 * nb - 1];
        }
#endif
      });
      const int* cn0 = cn + 16 * km_lo + 4 * g;
      if (km_hi > km_lo) conv_gemm<NB>(Tm, a.ldr, km_hi - km_lo, g, am, [&](int kb, double (&bv)[4][NB]) {
#ifdef BO_ABL_CT_BCONST
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) bv[s][nb] = bconst;
#else
        const int* c4 = cn0 + 16 * kb;
        const double* ph = tabH + j0 + jl + (a.C - 1);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const double* p = ph - (c4[s] & 0xffff);
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) bv[s][nb] = p[16 * nb];
        }
#endif
      });
      if constexpr (NB == 1) {
        mfma_fence<false>(aq[0], am[0]);
      } else {
#pragma unroll
        for (int nb = 0; nb < NB; nb += 2) {
          mfma_fence<false>(aq[nb], aq[nb + 1]);
          mfma_fence<false>(am[nb], am[nb + 1]);
        }
      }
      const double pv = a.pv[o], pm = a.pm[o];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
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
          if (outs && active && i0 + g + 4 * r < a.nrows && c < a.C && gi >= gi_lo && gi < gi_hi) {
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
    // global indices of this lane's 4 NB candidates (-1: outside the shard)
    long long gis[NB][4];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = a.row_lo + i0 + g + 4 * r, c = j0 + 16 * nb + jl;
        const long long gi = (long long)row * a.C + c;
        const bool ok = active && i0 + g + 4 * r < a.nrows && c < a.C && gi >= gi_lo && gi < gi_hi;
        gis[nb][r] = ok ? gi : -1;
        if (outs && ok && a.acq) bo_out_store(a.acq + (gi - gi_lo), acq[nb][r]);
      }
    }
#ifndef BO_ABL_CT_NOSEL
    const bool select = a.topq > 0;
#else
    const bool select = a.topq > 0 && a.n_lists < 0;             // ablation (timing only): false, and not known to be
#endif
    if (select) {
      // the wave's list and the tile's 256 NB candidates, merged by rounds of extract-best: each lane
      // offers the best of its remaining candidates (and its list entry), the wave takes the best
      // offer (NaN first, then descending, ties by ascending index).  Evaluated points never win: when they
      // are the call's training points (excl_train) the tile's are taken out before the rounds; with an
      // exclusion set of the caller's a winner found in the prep launch's hash set (compared exactly) is
      // dropped and the round repeated.  Skipped when no candidate comes before the list's last entry.
      const int q = a.topq;
      const unsigned long long kq = bo_readlane_u(bo_order_key(lv, li), q - 1);
      const long long iq = bo_readlane_i(li, q - 1);
      bool beats = false;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          beats = beats || bo_key_before(bo_order_key(acq[nb][r], gis[nb][r]), gis[nb][r], kq, iq);
      if (__ballot(beats) != 0ull) {
        unsigned int taken = 0;                                  // bit 16: the list entry
        if (a.excl_train) {
          // the evaluated points are the training points: those of the tile's columns are the slice
          // cstart[j0] .. cstart[j0 + TW] - 1 of cn[], 64 a step and a lane each; the few in the tile's rows
          // are passed round one by one, and the lane that owns the candidate (D row g + 4 r, column jl of
          // block nb) takes it out of the rounds
          const int s_hi = __builtin_amdgcn_readfirstlane(a.cstart[j0 + TW < a.C ? j0 + TW : a.C]);
          for (int s0 = __builtin_amdgcn_readfirstlane(a.cstart[j0 < a.C ? j0 : a.C]); s0 < s_hi; s0 += 64) {
            const int e = s0 + lane < s_hi ? cn[s0 + lane] : 0;
            const int dr = (e >> 16) - (a.row_lo + i0), dc = (e & 0xffff) - j0;
            unsigned long long hits = __ballot(s0 + lane < s_hi && dr >= 0 && dr < 16);
            while (hits != 0ull) {
              const int src = __builtin_ctzll(hits);
              hits &= hits - 1ull;
              const int hr = __builtin_amdgcn_readlane(dr, src), hc = __builtin_amdgcn_readlane(dc, src);
              if (lane == 16 * (hr & 3) + (hc & 15)) taken |= 1u << (4 * (hc >> 4) + (hr >> 2));
            }
          }
        }
        double nv = -__builtin_inf();
        long long ni = -1;
        int filled = 0;
        while (filled < q) {
          unsigned long long bk = 0ull;
          long long bi = -1;
          int bs = -1;
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) {
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
            if (bs != 16 && !a.excl_train) {
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
    // One list per workgroup: the waves' lists (sorted, the empty entries last) go to LDS over the tables, and the
    // first wave merges them by q rounds over their heads -- lane w < W offers the head of list w, the wave takes
    // the best offer (the same order; the indices are distinct, so it is a total one) and that list moves on.
    const int q = a.topq;
    TopEntry* ml = (TopEntry*)sd;
    __syncthreads();                                             // the tables are done with
    if (lane < q) {
      ml[wave * q + lane].v = lv;
      ml[wave * q + lane].i = li;
    }
    __syncthreads();
    if (wave == 0) {
      int head = 0;
      double nv = -__builtin_inf();
      long long ni = -1;
      for (int r = 0; r < q; ++r) {
        const bool has = lane < W && head < q;
        const double hv = has ? ml[lane * q + head].v : -__builtin_inf();
        const long long hi = has ? ml[lane * q + head].i : -1;
        const unsigned long long bk = bo_order_key(hv, hi);
        unsigned long long wk = bk;
        long long wi = hi;
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) {
          const unsigned long long ok = __shfl_xor(wk, m, 64);
          const long long oi = __shfl_xor(wi, m, 64);
          if (bo_key_before(ok, oi, wk, wi)) { wk = ok; wi = oi; }
        }
        if (wk == 0ull) break;                                   // nothing left
        const bool win = bk == wk && hi == wi;
        if (win) ++head;
        const double wv = __shfl(hv, __builtin_ctzll(__ballot(win)), 64);
        if (lane == r) { nv = wv; ni = wi; }
      }
      if (lane < q) {
        TopEntry* dst = a.partial + (size_t)blockIdx.x * q;
        dst[lane].v = nv;
        dst[lane].i = ni;
      }
    }
    // the lists of the merge that this grid does not fill
    if (blockIdx.x == 0) {
      const long long e0 = (long long)gridDim.x * q, e1 = (long long)a.n_lists * q;
      for (long long e = e0 + tid; e < e1; e += nt) {
        a.partial[e].v = -__builtin_inf();
        a.partial[e].i = -1;
      }
    }
  }
}

}  // namespace

namespace bo {

// The plan's admission bound on (n, R, C), frozen: it decides which calls take this path (conv_planned of
// tests/gridconv_model.py mirrors it) and is the LDS of no kernel -- the tables of R, C and n plus 2048 doubles
// and 2048 ints.  The real layouts of the setup block, the list and the accumulate kernel each hold a part of its
// terms and are smaller for every (n, R, C); the contraction's tables are tested by themselves.
bool conv_lds_admits(int n, int R, int C, int Cpad, int LT, int NP) {
  const size_t bound = ((size_t)4 * R + 2048) * sizeof(double) + ((size_t)(C + 1) + 3 * (size_t)n + 2048) * sizeof(int);
  assert(ConvSetupLds(n, C, 256).bytes <= bound && ListLds(n, C).bytes <= bound && AccLds(R).bytes <= bound);
  assert(ContractLds(C, Cpad, LT, NP).hband == conv_ctab_band(C, Cpad, LT));   // the workspace's image of the tables
  return bound <= kConvLdsBytes && ContractLds(C, Cpad, LT, NP).bytes <= kConvLdsBytes;
}

template <class K>
static hipError_t conv_lds_attr(K k, size_t lds) {
  if (lds <= 64 * 1024) return hipSuccess;
  return hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

// The accumulate kernel's persistent waves: up to 4 workgroups (4 waves per SIMD) per CU as the
// table's LDS allows, shared evenly by the objectives; no more waves than the bound LT nrb on its
// items (their number is the device's: the tau that kept pairs).
ConvSched conv_acc_schedule(int R, int LT, int ldr, int n_obj, int cus) {
  ConvSched sc;
  sc.nrb = (ldr + kAccRows - 1) / kAccRows;
  const long long items = (long long)LT * sc.nrb;
  const size_t tab = (size_t)4 * R * sizeof(double);
  const int per_cu = (int)(kConvLdsBytes / tab < 4 ? kConvLdsBytes / tab : 4);
  long long wgs = (long long)(cus > 0 ? cus : 256) * per_cu / n_obj;
  if (wgs > (items + kConvAccWaves - 1) / kConvAccWaves) wgs = (items + kConvAccWaves - 1) / kConvAccWaves;
  if (wgs < 1) wgs = 1;
  sc.wgs = (int)wgs;
  sc.ngrp = (int)(wgs < kConvTicketGroups ? wgs : kConvTicketGroups);
  // tickets only when some wave can have a second item: not when the groups are of equal size and
  // hold no more items than waves (a wave's first item is its index in its group)
  sc.dyn = (items <= wgs * kConvAccWaves && wgs % sc.ngrp == 0) ? 0 : 1;
  return sc;
}

hipError_t launch_gridconv(const ConvArgs& ca, const ConvPlan& cp, const ConvSched& sc, hipStream_t st) {
  const size_t l1 = ListLds(ca.n, ca.C).bytes, la = AccLds(ca.R).bytes;
  const size_t l2 = ContractLds(ca.C, ca.Cpad, ca.LT, ca.NP, cp.waves * ca.topq).bytes;
  if (l1 > kConvLdsBytes || la > kConvLdsBytes) return hipErrorInvalidValue;   // (conv_lds_admits keeps them below)
  if (cp.waves < 1 || cp.waves > kContractWaves || cp.grid > ca.n_lists) return hipErrorInvalidValue;
  auto* contract = cp.nb == 4 ? conv_contract_kernel<4> : cp.nb == 2 ? conv_contract_kernel<2> : conv_contract_kernel<1>;
  hipError_t e;
  if ((e = conv_lds_attr(conv_list_kernel, l1)) != hipSuccess) return e;
  if ((e = conv_lds_attr(conv_acc_kernel, la)) != hipSuccess) return e;
  if ((e = conv_lds_attr(contract, l2)) != hipSuccess) return e;
  const int tau_blocks = (ca.LT + kListWaves - 1) / kListWaves;    // the padding tau too: their pkept
  const long long tm_elems = (long long)ca.NP * ca.ldr;
  const int tm_blocks = (int)((tm_elems + 1023) / 1024 < 512 ? (tm_elems + 1023) / 1024 : 512);
  // a thread per entry of the longer of the E tables, up to 64 blocks
  const long long tab_elems = 4LL * ca.R > 2LL * ca.Cpad + ca.LT ? 4LL * ca.R : 2LL * ca.Cpad + ca.LT;
  const int tab_blocks = (int)((tab_elems + 255) / 256 < 64 ? (tab_elems + 255) / 256 : 64);
  hipLaunchKernelGGL(conv_list_kernel, dim3(tau_blocks + tm_blocks + tab_blocks), dim3(64 * kListWaves), l1, st, ca,
                     tau_blocks, tm_blocks, sc.dyn);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(conv_acc_kernel, dim3((unsigned)sc.wgs, ca.n_obj), dim3(64 * kConvAccWaves), la, st, ca,
                     (const double*)ca.pair_w, (const int*)ca.pair_sl, (const int*)ca.pstart, (const int*)ca.pkept,
                     (const int*)ca.ccount, (const int*)ca.clist, ca.ticket, ca.T, sc.nrb, sc.ngrp, sc.dyn);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(contract, dim3(cp.grid), dim3(64 * cp.waves), l2, st, ca);
  return hipGetLastError();
}

}  // namespace bo
