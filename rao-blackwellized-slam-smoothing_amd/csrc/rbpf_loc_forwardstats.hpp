// Running two-slice statistics of the transition residual, once for every map: the forward-only form of FFBSm for an additive
// functional (Del Moral, Doucet & Singh 2010).  Every particle carries the conditional expectation of the functional accumulated so
// far, tau_t(i) [KF = NR (NR + 3) / 2]: the lower triangle by rows of sum_s r r' / dt_s, then sum_s r; one all-pairs step per time
// step moves it on:
//     D_t(j)      = log sum_i w_t(i) p(X[t+1][:, j] | X[t][:, i])
//     omega(i, j) = exp(log w_t(i) + logp(j | i) - D_t(j))                                  (sums to 1 over i, every omega <= 1)
//     tau_{t+1}(j) = sum_i omega(i, j) (tau_t(i) + s_t(i, j)),      tau_0 = 0,    s_t = [r r' s_scale ; r],  s_scale = 1 / dt_t
//     est_{t+1}   = sum_j w_{t+1}(j) tau_{t+1}(j)
// r is the un-whitened residual term.pair_res hands out (rbpf_loc_pairstats.hpp).  est_k is the FFBSm estimate of
// sum_{s<k} E[s_s | y_{0:k}] from the particles up to step k only; at the last step it is sum_t S_t / dt_t and sum_t m_t of the
// offline statistics pass, exactly.  Nothing N x N is stored.
//
// Kernels of one step t -> t + 1 (in stream order, after the family's prologue, which writes Xhat [NS + 1][N], log w_t last):
//   marginal_norm_pass_kernel<Term>, marginal_norm_merge_kernel   of rbpf_loc_marginal.hpp, unchanged, with logws_next = 0: D(j).
//   forward_stats_pass_kernel<Term>   grid = (successor blocks of 256) x (predecessor chunks of forward_stats_chunk(N, M)).  A lane
//                                     owns successor j and keeps its NS rows (load_next) and D(j) in registers.  The predecessors
//                                     come through LDS in tiles of forward_stats_tile(NS, NR) entries of E = NS + 1 + KF doubles (the
//                                     Xhat row, log w, tau_t(i)), read as broadcasts.  The tile depth falls with E so that a tile
//                                     never takes more than 32 KB: 256 entries up to E = 16, 128 up to 32, 64 above (dense-mag:
//                                     E = 35; NR = 8: E = 53).  Per pair l = log w(i) - D(j), pair_res with the CONSTANT bound
//                                     -kBackwardSkip (no running maximum: a pair below -746 contributes exactly 0), omega = exp(l),
//                                     KF times acc[k] = fma(omega, tau_i[k] + s_k, acc[k]) and reach += omega.  l = -inf contributes
//                                     nothing; a successor with D = -inf takes nothing.  Lanes past the end recompute the last
//                                     successor and store nothing.  Writes one [KF + 1] vector per (chunk, j): part [chunk][k][M].
//   forward_stats_merge_kernel        per j: plain sums in ascending chunk order -> tau_{t+1} [KF][M], reach [M]; D(j) = -inf: zeros.
//   forward_stats_reduce_kernel       one workgroup: est = sum_j w_{t+1}(j) tau_{t+1}(j), mass = sum_j w_{t+1}(j) reach(j) as strided
//                                     partials and the tree of marginal_tree_sum; writes one page [NR * NR + NR + 1]: S in both
//                                     triangles, m, the mass, kernel order.
// SUMMATION ORDER: fixed, a function of (N, M) only (and of the term's tile depth not at all: a chunk is whole tiles of every depth):
// ascending i inside a chunk, ascending chunk in the merge, strided partials and the tree in the reducer.  No atomics.
#pragma once
#include "../../include/rbpf.h"
#include "rbpf_internal.hpp"
#include "rbpf_loc_backward.hpp"
#include "rbpf_loc_marginal.hpp"
#include "rbpf_loc_pairstats.hpp"

namespace rbpf {

constexpr int forward_stats_carry(int NR) { return NR * (NR + 3) / 2; }       // KF: lower triangle of S by rows, then m
// predecessors per LDS tile: at most 32 KB of [entry][NS + 1 + KF] doubles
constexpr int forward_stats_tile(int NS, int NR) {
  return (NS + 1 + forward_stats_carry(NR)) <= 16 ? 256 : (NS + 1 + forward_stats_carry(NR)) <= 32 ? 128 : 64;
}

// predecessor chunk: enough (successor block) x (chunk) workgroups to give every CU about four, in whole tiles of 256 (a multiple of
// every tile depth).  The 2048 of kBackwardMaxChunk is the locate kernel's and does not bind here: the partials stay small.
inline int forward_stats_chunk(int N, int M) {
  const int bx = (M + kBackwardTile - 1) / kBackwardTile;
  const int want = std::max(1, (1024 + bx - 1) / bx);
  const int C = ((N + want - 1) / want + kBackwardTile - 1) / kBackwardTile * kBackwardTile;
  return std::max(C, kBackwardTile);
}
inline int forward_stats_chunks(int N, int M) {
  const int C = forward_stats_chunk(N, M);
  return (N + C - 1) / C;
}

template <class Term>
struct ForwardStatsArgs {
  int N, M;                        // predecessors, successors (M = N outside the probes)
  int C, nchunks;                  // predecessor chunks, forward_stats_chunk(N, M)
  typename Term::Head head;        // the term's integers (.first is 0)
  const double* Xhat;              // [NS + 1][N], last row log w_t
  const double* xn_next;           // [rows][M]: the successors, particles of step t + 1
  const double* D;                 // [M]
  const double* tau;               // [KF][N]: the carry of step t, kernel order
  double s_scale;                  // 1 / dt_t: what the S part of s is scaled by
  double* part;                    // [nchunks][KF + 1][M]
  Term term;
  template <class U>
  ForwardStatsArgs<U> with(const U& t) const { return {N, M, C, nchunks, head, Xhat, xn_next, D, tau, s_scale, part, t}; }
};

template <class Term>
__global__ __launch_bounds__(kBackwardTile) void forward_stats_pass_kernel(const ForwardStatsArgs<Term> a) {
  constexpr int NS = Term::NS;
  constexpr int NR = Term::NR;
  constexpr int S = NS + 1;
  constexpr int KF = forward_stats_carry(NR);
  constexpr int TRI = NR * (NR + 1) / 2;
  constexpr int E = S + KF;
  constexpr int TD = forward_stats_tile(NS, NR);
  __shared__ double tile[TD * E];                // [predecessor][its Xhat row, log w, tau]
  const int tid = threadIdx.x;
  const int j = blockIdx.x * kBackwardTile + tid;
  const int jl = min(j, a.M - 1);          // lanes past the end recompute the last successor; nothing of theirs is stored
  const int c = blockIdx.y;
  const int i0 = c * a.C, i1 = min(a.N, i0 + a.C);
  double x[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) x[k] = a.term.load_next(a.head, a.xn_next, a.M, jl, k);
  const double dj = a.D[jl];
  const double d = dj > -INFINITY ? dj : INFINITY;      // no predecessor reaches j: every l is -inf, nothing is taken
  double acc[KF + 1];
#pragma unroll
  for (int k = 0; k <= KF; ++k) acc[k] = 0.0;
  for (int base = i0; base < i1; base += TD) {
    const int cnt = min(TD, i1 - base);
    __syncthreads();
    for (int q = tid; q < TD * E; q += kBackwardTile) {
      const int p = q % TD, r = q / TD;          // (TD is a power of two; lanes walk p: the rows of Xhat and tau are read coalesced)
      if (p < cnt) tile[p * E + r] = r < S ? a.Xhat[(size_t)r * a.N + base + p] : a.tau[(size_t)(r - S) * a.N + base + p];
    }
    __syncthreads();
    for (int k = 0; k < cnt; ++k) {
      const double* h = tile + k * E;
      double l = h[NS] - d;
      double r[NR];
      if (!a.term.pair_res(a.head, h, x, -kBackwardSkip, l, r)) continue;
      if (l == -INFINITY) continue;
      const double om = exp(l);
      const double* ti = h + S;
#pragma unroll
      for (int p = 0; p < NR; ++p) {
        const double rs = r[p] * a.s_scale;
#pragma unroll
        for (int q = 0; q <= p; ++q) acc[p * (p + 1) / 2 + q] = fma(om, ti[p * (p + 1) / 2 + q] + rs * r[q], acc[p * (p + 1) / 2 + q]);
        acc[TRI + p] = fma(om, ti[TRI + p] + r[p], acc[TRI + p]);
      }
      acc[KF] += om;
    }
  }
  if (j < a.M) {
#pragma unroll
    for (int k = 0; k <= KF; ++k) a.part[((size_t)c * (KF + 1) + k) * a.M + j] = acc[k];
  }
}

// part [nchunks][K1][M] -> tau_next [K1 - 1][M], reach [M]: plain sums, ascending chunk; D(j) = -inf: zeros
inline __global__ void forward_stats_merge_kernel(int M, int K1, int nchunks, const double* __restrict__ part, const double* __restrict__ D,
                                                  double* __restrict__ tau_next, double* __restrict__ reach) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= M) return;
  const bool dead = !(D[j] > -INFINITY);
  for (int k = 0; k < K1; ++k) {
    double v = 0.0;
    for (int c = 0; c < nchunks; ++c) v += part[((size_t)c * K1 + k) * M + j];
    if (dead) v = 0.0;
    if (k + 1 < K1) tau_next[(size_t)k * M + j] = v;
    else reach[j] = v;
  }
}

// tau [KF][M], reach [M], w [M] -> out [NR * NR + NR + 1]: S [NR x NR] (both triangles), m [NR], the mass; kernel order.  One
// workgroup of 256.
inline __global__ __launch_bounds__(256) void forward_stats_reduce_kernel(int NR, int M, const double* __restrict__ tau,
                                                                          const double* __restrict__ reach, const double* __restrict__ w,
                                                                          double* __restrict__ out) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  const int tri = NR * (NR + 1) / 2, K = tri + NR + 1;
  int p = 0, q = 0;                              // (row, column) of value k while k < tri
  for (int k = 0; k < K; ++k) {
    const double* src = k + 1 < K ? tau + (size_t)k * M : reach;
    double acc = 0.0;
    for (int j = tid; j < M; j += 256) acc = fma(w[j], src[j], acc);
    const double v = marginal_tree_sum(acc, red, tid);
    if (tid == 0) {
      if (k < tri) { out[p + NR * q] = v; out[q + NR * p] = v; }
      else out[NR * NR + (k - tri)] = v;
    }
    if (k < tri && ++q > p) { ++p; q = 0; }
  }
}

inline __global__ void forward_stats_fill_kernel(int n, double v, double* __restrict__ x) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) x[i] = v;
}

// ---- host side -----------------------------------------------------------------------------------------------------------
// doubles of every buffer of a ForwardCarry (rbpf_loc_state.hpp), in the order of the struct
inline void forward_stats_counts(size_t rows, size_t n_res, size_t N, size_t M, size_t P, size_t cnt[10]) {
  const size_t KF = (size_t)forward_stats_carry((int)n_res);
  cnt[0] = (rows + 1) * N;
  cnt[1] = cnt[2] = marginal_part_count(N, M);
  cnt[3] = cnt[4] = cnt[5] = M;
  cnt[6] = (size_t)forward_stats_chunks((int)N, (int)M) * (KF + 1) * M;
  cnt[7] = 2 * KF * std::max(N, M);
  cnt[8] = M;
  cnt[9] = std::max<size_t>(P, 1) * (size_t)pair_stats_page((int)n_res);
}

// what the carry of a run of T steps takes from the pool (P = T - 1 pages)
inline size_t forward_stats_bytes(size_t rows, size_t n_res, size_t N, size_t T) {
  size_t cnt[10], b = 0;
  forward_stats_counts(rows, n_res, N, N, T > 1 ? T - 1 : 1, cnt);
  for (size_t v : cnt) b += v;
  return b * sizeof(double);
}

// all or nothing; tau_0 = 0 and the zeros are written in stream s
inline int forward_stats_take(ForwardCarry& f, DevicePool& pool, int nN, int rows, int n_res, int N, int M, int P, hipStream_t s) {
  size_t cnt[10];
  forward_stats_counts((size_t)rows, (size_t)n_res, (size_t)N, (size_t)M, (size_t)P, cnt);
  f = ForwardCarry();
  f.pool = &pool; f.nN = nN; f.rows = rows; f.n_res = n_res;
  double** slot[10] = {&f.Xhat, &f.pm, &f.ps, &f.zero, &f.D, &f.cj, &f.part, &f.tau, &f.reach, &f.pages};
  int st = RBPF_OK;
  for (int k = 0; k < 10 && st == RBPF_OK; ++k) st = pool.alloc(slot[k], cnt[k]);
  if (st == RBPF_OK) {
    hipError_t e = hipMemsetAsync(f.zero, 0, cnt[3] * sizeof(double), s);
    if (e == hipSuccess) e = hipMemsetAsync(f.tau, 0, cnt[7] * sizeof(double), s);
    if (e == hipSuccess) e = hipMemsetAsync(f.pages, 0, cnt[9] * sizeof(double), s);
    if (e != hipSuccess) st = hip_fail(e, "clearing the carry of the running statistics", __FILE__, __LINE__);
  }
  if (st != RBPF_OK) { f.release(); return st; }
  f.alive = true;
  return RBPF_OK;
}

// the sizes and buffers of a step into the norm pass's and the carry pass's arguments (head, xn_next and term are the caller's)
template <class Term>
void forward_stats_set(const ForwardCarry& f, int N, int M, MarginalArgs<Term>& a, ForwardStatsArgs<Term>& b) {
  marginal_set_sizes(a, N, M);
  a.Xhat = f.Xhat; a.cj = f.cj; a.part_m = f.pm; a.part_s = f.ps;
  b.N = N; b.M = M; b.C = forward_stats_chunk(N, M); b.nchunks = forward_stats_chunks(N, M);
  b.Xhat = f.Xhat; b.D = f.D; b.part = f.part;
}

// norm pass + merge (D) + carry pass + merge + reducer of one step, in stream order: tau (of step t) -> tau_next, reach, page;
// w_next [M]: the filter's weights of step t + 1
template <class Term>
hipError_t forward_stats_launch_step(const MarginalArgs<Term>& a, const ForwardStatsArgs<Term>& b, const double* zero, double* D, double* cj,
                                     double* tau_next, double* reach, const double* w_next, double* page, hipStream_t s) {
  constexpr int K1 = forward_stats_carry(Term::NR) + 1;
  const int bx = (a.M + kBackwardTile - 1) / kBackwardTile;
  hipLaunchKernelGGL((marginal_norm_pass_kernel<Term>), dim3(bx, a.nchunks), dim3(kBackwardTile), 0, s, a);
  hipLaunchKernelGGL(marginal_norm_merge_kernel, dim3((a.M + 255) / 256), dim3(256), 0, s, a.M, a.nchunks, a.part_m, a.part_s, zero, D, cj);
  hipLaunchKernelGGL((forward_stats_pass_kernel<Term>), dim3(bx, b.nchunks), dim3(kBackwardTile), 0, s, b);
  hipLaunchKernelGGL(forward_stats_merge_kernel, dim3((b.M + 255) / 256), dim3(256), 0, s, b.M, K1, b.nchunks, b.part, D, tau_next, reach);
  hipLaunchKernelGGL(forward_stats_reduce_kernel, dim3(1), dim3(256), 0, s, (int)Term::NR, b.M, tau_next, reach, w_next, page);
  return hipGetLastError();
}

// The carry between the caller's order (tau_S [n x n x N] both triangles, tau_m [n x N], column-major) and the kernels' [KF][ld]
// (lower triangle by rows, then m; kernel residual k is residual perm[k] of the caller, perm null: the identity).
inline void forward_stats_pack(int n, int N, const int* perm, const double* tau_S, const double* tau_m, double* out) {
  const int tri = n * (n + 1) / 2;
  for (int i = 0; i < N; ++i) {
    for (int p = 0; p < n; ++p) {
      const int pp = perm ? perm[p] : p;
      for (int q = 0; q <= p; ++q) {
        const int pq = perm ? perm[q] : q;
        out[(size_t)(p * (p + 1) / 2 + q) * N + i] = tau_S[(size_t)n * n * i + std::max(pp, pq) + (size_t)n * std::min(pp, pq)];   // the lower triangle is read
      }
      out[(size_t)(tri + p) * N + i] = tau_m[(size_t)n * i + pp];
    }
  }
}

inline void forward_stats_unpack(int n, int N, const int* perm, const double* in, double* tau_S, double* tau_m) {
  const int tri = n * (n + 1) / 2;
  for (int i = 0; i < N; ++i)
    for (int p = 0; p < n; ++p) {
      const int pp = perm ? perm[p] : p;
      for (int q = 0; q <= p && tau_S; ++q) {
        const int pq = perm ? perm[q] : q;
        const double v = in[(size_t)(p * (p + 1) / 2 + q) * N + i];
        tau_S[(size_t)n * n * i + pp + (size_t)n * pq] = v;
        tau_S[(size_t)n * n * i + pq + (size_t)n * pp] = v;
      }
      if (tau_m) tau_m[(size_t)n * i + pp] = in[(size_t)(tri + p) * N + i];
    }
}

// pages 0 .. folded - 1 and the carry of the latest step -> the caller's arrays (NULL outputs are skipped); the stream is idle
inline int forward_stats_copy_out(const ForwardCarry& f, int N, const int* perm, double* S_run, double* m_run, double* mass_run, double* tau_S,
                                  double* tau_m) {
  if (f.folded > 0 && (S_run || m_run || mass_run)) {
    BackwardWorkspace view;
    view.stat = f.pages;
    RB_TRY(pair_stats_copy_out(view, f.n_res, f.folded + 1, perm, S_run, m_run, mass_run));
  }
  if (tau_S || tau_m) {
    const size_t KF = (size_t)forward_stats_carry(f.n_res);
    std::vector<double> h(KF * N);
    HIPCHK(hipMemcpy(h.data(), f.tau + (size_t)f.cur * KF * N, h.size() * sizeof(double), hipMemcpyDeviceToHost));
    forward_stats_unpack(f.n_res, N, perm, h.data(), tau_S, tau_m);
  }
  return RBPF_OK;
}

// What the running statistics ask of the forward run: stored particles and weights, at least two steps done, no degenerate step
// among those done.  Selects the context's device and leaves its stream idle.
inline int forward_stats_check_forward(rbpf_ctx* c, const char* who) {
  if (!c->opt.keep_history || !c->opt.trace) {
    set_error(std::string(who) + " reads the stored particles and weights: create the context with keep_history = 1 and trace = 1");
    return RBPF_ERR_STATE;
  }
  if (c->t < 2) { set_error(std::string(who) + ": " + std::to_string(c->t) + " steps are done, the running statistics need at least 2"); return RBPF_ERR_STATE; }
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  std::vector<double> lse((size_t)c->t);
  HIPCHK(hipMemcpy(lse.data(), c->loc->d_lse, lse.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (int t = 0; t < c->t; ++t)
    if (!(lse[t] > std::log(1e-12))) {
      set_error("the forward run recorded a degenerate step (t = " + std::to_string(t) + "): its weights are no filtering distribution");
      return RBPF_ERR_STATE;
    }
  return RBPF_OK;
}

}  // namespace rbpf
