// Fixed-lag smoothing of the state, once for every map: the forward-only form of FFBSm for the per-step functionals of the last L
// steps.  Every particle carries, for each of the last L steps s, the conditional expectation of h_s(x_s) given its own state; one
// all-pairs pass per time step moves all of them on through the omega of rbpf_loc_forwardstats.hpp:
//     D_t(j)         = log sum_i w_t(i) p(X[t+1][:, j] | X[t][:, i])
//     omega(i, j)    = exp(log w_t(i) + logp(j | i) - D_t(j))                                (sums to 1 over i, every omega <= 1)
//     T0_t(i)        = h_t(X[t][:, i])                                                         (the enter kernel)
//     T^(l)_{t+1}(j) = sum_i omega(i, j) T^(l-1)_t(i),   l = 1 .. L                            (one pass over K = L H columns)
//     est(l, t+1)    = sum_j w_{t+1}(j) T^(l)_{t+1}(j) = E[h_{t+1-l}(x_{t+1-l}) | y_{0:t+1}],  l = 0 .. L
//     mass(t+1)      = sum_j w_{t+1}(j) sum_i omega(i, j)                                      (1 in exact arithmetic)
// h_s(x) over ALL n state rows, d = x - c_s with c_s the filter mean of step s: moments = 1: H = n columns, d; moments = 2:
// H = n (n + 3) / 2 columns, d and then the lower triangle by rows of d d'.  Centred at c_s the second moments do not cancel.
// Plain weighted moments: quaternion and angle rows get no special handling.  Nothing N x N is stored.
//
// The carry of a step is T [(L + 1) H][N]: slot l (rows l H .. (l + 1) H - 1) holds T^(l).  The pass reads the slots 0 .. L-1 of
// step t and writes the slots 1 .. L of step t + 1 (the other half of a ping-pong); the enter kernel writes slot 0.  Slots of steps
// before the first (s < 0) carry zeros, which the pass moves on as zeros; the host reports them as NaN.
//
// Kernels of one step t -> t + 1 (in stream order, after the family's prologue, which writes Xhat [NS + 1][N], log w_t last):
//   marginal_norm_pass_kernel<Term>, marginal_norm_merge_kernel   of rbpf_loc_marginal.hpp, unchanged, with logws_next = 0: D(j).
//   fixed_lag_pass_kernel<Term>   grid = (successor blocks of 256) x (predecessor chunks of forward_stats_chunk(N, M)) x (column
//                                 blocks of KB = kFixedLagKB).  A lane owns successor j and keeps its NS rows (load_next), D(j)
//                                 and KB + 1 accumulators in registers.  The predecessors come through LDS in tiles of
//                                 fixed_lag_tile(NS) entries of E = NS + 1 + KB doubles (the Xhat row, log w, this block's columns of
//                                 the carry, zeros past the last column), staged coalesced and read as broadcasts; the depth follows
//                                 the rule of forward_stats_tile, so that a tile never takes more than 32 KB.  Per pair
//                                 l = log w(i) - D(j) + logp with the CONSTANT bound -kBackwardSkip (a pair below -746 contributes
//                                 exactly 0), omega = exp(l), KB times acc[k] = fma(omega, col[k], acc[k]) and reach += omega.
//                                 l = -inf contributes nothing (what such a predecessor carries is never multiplied); a successor
//                                 with D = -inf takes nothing.  Every column block recomputes the term; block 0 stores reach.
//                                 Writes part [chunk][K + 1][M], reach in row K.
//   forward_stats_merge_kernel    of rbpf_loc_forwardstats.hpp, unchanged: plain sums in ascending chunk order -> slots 1 .. L of
//                                 step t + 1 and reach [M]; D(j) = -inf: zeros.
//   fixed_lag_reduce_kernel       one workgroup: out[k] = sum_j w(j) src[k][j] as strided partials and the tree of
//                                 marginal_tree_sum.  Called twice per step: on X[t+1] -> c_{t+1} (before the enter kernel), and on
//                                 the whole carry of step t + 1 and reach -> the page [(L + 1) H + 1]: est(0 .. L, t + 1), mass.
//   fixed_lag_enter_kernel        T0 of step t + 1 from X[t+1] and c_{t+1} into slot 0.  No all-pairs work.
// SUMMATION ORDER: fixed, a function of (N, M) only: ascending i inside a chunk (a chunk is whole tiles of every depth), ascending
// chunk in the merge, strided partials and the tree in the reducer.  No atomics.  A column's value depends neither on its place in
// the carry nor on L, moments or KB: every column goes through the same fma chain with the same omegas.
#pragma once
#include "../../include/rbpf.h"
#include "rbpf_internal.hpp"
#include "rbpf_loc_backward.hpp"
#include "rbpf_loc_marginal.hpp"
#include "rbpf_loc_forwardstats.hpp"

namespace rbpf {

#ifndef RBPF_FIXED_LAG_KB
#define RBPF_FIXED_LAG_KB 32                   // 16 in the tuning variant tools/fixed_lag_bench.py measures against; the product has this one
#endif
constexpr int kFixedLagKB = RBPF_FIXED_LAG_KB; // columns of the carry per workgroup: ONE value per build (profiles/fixed_lag_bench.json)
static_assert(kFixedLagKB == 16 || kFixedLagKB == 32, "KB is 16 or 32");
constexpr int kFixedLagMaxLag = 64;

constexpr int fixed_lag_columns(int n, int moments) { return moments == 2 ? n * (n + 3) / 2 : n; }       // H
// predecessors per LDS tile: at most 32 KB of [entry][NS + 1 + KB] doubles, the rule of forward_stats_tile
constexpr int fixed_lag_tile(int NS) { return (NS + 1 + kFixedLagKB) <= 16 ? 256 : (NS + 1 + kFixedLagKB) <= 32 ? 128 : 64; }

template <class Term>
struct FixedLagArgs {
  int N, M;                        // predecessors, successors (M = N outside the probes)
  int C, nchunks;                  // predecessor chunks, forward_stats_chunk(N, M)
  int K;                           // columns of the carry that move on (L H in a session)
  typename Term::Head head;        // the term's integers (.first is 0)
  const double* Xhat;              // [NS + 1][N], last row log w_t
  const double* xn_next;           // [rows][M]: the successors, particles of step t + 1
  const double* D;                 // [M]
  const double* tau;               // [K][N]: the slots 0 .. L-1 of step t
  double* part;                    // [nchunks][K + 1][M]
  Term term;
  template <class U>
  FixedLagArgs<U> with(const U& t) const { return {N, M, C, nchunks, K, head, Xhat, xn_next, D, tau, part, t}; }
};

template <class Term>
__global__ __launch_bounds__(kBackwardTile) void fixed_lag_pass_kernel(const FixedLagArgs<Term> a) {
  constexpr int NS = Term::NS;
  constexpr int S = NS + 1;
  constexpr int KB = kFixedLagKB;
  constexpr int E = S + KB;
  constexpr int TD = fixed_lag_tile(NS);
  static_assert(TD * E * sizeof(double) <= 32768, "a tile of the fixed-lag pass takes at most 32 KB");
  __shared__ double tile[TD * E];                // [predecessor][its Xhat row, log w, KB columns of the carry]
  const int tid = threadIdx.x;
  const int j = blockIdx.x * kBackwardTile + tid;
  const int jl = min(j, a.M - 1);          // lanes past the end recompute the last successor; nothing of theirs is stored
  const int c = blockIdx.y;
  const int k0 = blockIdx.z * KB;
  const int kc = min(KB, a.K - k0);        // columns of this block; the rest of the tile's KB are zeros
  const int i0 = c * a.C, i1 = min(a.N, i0 + a.C);
  double x[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) x[k] = a.term.load_next(a.head, a.xn_next, a.M, jl, k);
  const double dj = a.D[jl];
  const double d = dj > -INFINITY ? dj : INFINITY;      // no predecessor reaches j: every l is -inf, nothing is taken
  double acc[KB + 1];
#pragma unroll
  for (int k = 0; k <= KB; ++k) acc[k] = 0.0;
  for (int base = i0; base < i1; base += TD) {
    const int cnt = min(TD, i1 - base);
    __syncthreads();
    for (int q = tid; q < TD * E; q += kBackwardTile) {
      const int p = q % TD, r = q / TD;          // (TD is a power of two; lanes walk p: the rows of Xhat and the carry are read coalesced)
      if (p < cnt) {
        double v = 0.0;
        if (r < S) v = a.Xhat[(size_t)r * a.N + base + p];
        else if (r - S < kc) v = a.tau[(size_t)(k0 + r - S) * a.N + base + p];
        tile[p * E + r] = v;
      }
    }
    __syncthreads();
    for (int k = 0; k < cnt; ++k) {
      const double* h = tile + k * E;
      double l = h[NS] - d;
      if constexpr (Term::kSplit) {
        l += a.term.pair_near(a.head, h, x);
        if (l < -kBackwardSkip) continue;
        l += a.term.pair_far(a.head, h, x);
      } else {
        if (!a.term.pair(a.head, h, x, -kBackwardSkip, l)) continue;
      }
      if (l == -INFINITY) continue;
      const double om = exp(l);
      const double* col = h + S;
#pragma unroll
      for (int q = 0; q < KB; ++q) acc[q] = fma(om, col[q], acc[q]);
      acc[KB] += om;
    }
  }
  if (j < a.M) {
    double* out = a.part + (size_t)c * (a.K + 1) * a.M + j;
#pragma unroll
    for (int q = 0; q < KB; ++q)
      if (q < kc) out[(size_t)(k0 + q) * a.M] = acc[q];
    if (blockIdx.z == 0) out[(size_t)a.K * a.M] = acc[KB];
  }
}

// X [n][M] (the particles of a step), c [n] (their filter mean) -> T0 [H][M]: d = x - c, then (moments = 2) the lower triangle by
// rows of d d'
inline __global__ void fixed_lag_enter_kernel(int n, int moments, int M, const double* __restrict__ X, const double* __restrict__ c,
                                              double* __restrict__ T0) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= M) return;
  int k = n;
  for (int p = 0; p < n; ++p) {
    const double dp = X[(size_t)p * M + j] - c[p];
    T0[(size_t)p * M + j] = dp;
    if (moments == 2)
      for (int q = 0; q <= p; ++q) T0[(size_t)(k++) * M + j] = dp * (X[(size_t)q * M + j] - c[q]);
  }
}

// out[k] = sum_j w(j) src[k][j], k < K (src [K][ld]); mass_mode 1: out[K] = 1, 2: out[K] = sum_j w(j) reach(j).  One workgroup of
// 256: strided partials and the tree of marginal_tree_sum.
inline __global__ __launch_bounds__(256) void fixed_lag_reduce_kernel(int K, int M, size_t ld, const double* __restrict__ src,
                                                                      const double* __restrict__ reach, const double* __restrict__ w,
                                                                      int mass_mode, double* __restrict__ out) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  const int Kt = mass_mode == 2 ? K + 1 : K;
  for (int k = 0; k < Kt; ++k) {
    const double* s = k < K ? src + (size_t)k * ld : reach;
    double acc = 0.0;
    for (int j = tid; j < M; j += 256) acc = fma(w[j], s[j], acc);
    const double v = marginal_tree_sum(acc, red, tid);
    if (tid == 0) out[k] = v;
  }
  if (mass_mode == 1 && tid == 0) out[K] = 1.0;
}

// ---- host side -----------------------------------------------------------------------------------------------------------
constexpr int kFixedLagBuffers = 11;

// doubles of every buffer of a FixedLagCarry (rbpf_loc_state.hpp), in the order of the struct: K columns move on, H enter, P pages
// of K + H + 1 and P means of nN
inline void fixed_lag_counts(size_t nN, size_t rows, size_t K, size_t H, size_t N, size_t M, size_t P, size_t cnt[kFixedLagBuffers]) {
  cnt[0] = (rows + 1) * N;
  cnt[1] = cnt[2] = marginal_part_count(N, M);
  cnt[3] = cnt[4] = cnt[5] = M;
  cnt[6] = (size_t)forward_stats_chunks((int)N, (int)M) * (K + 1) * M;
  cnt[7] = 2 * (K + H) * std::max(N, M);
  cnt[8] = M;
  cnt[9] = std::max<size_t>(P, 1) * (K + H + 1);
  cnt[10] = std::max<size_t>(P, 1) * nN;
}

// what the carry of a run of T steps takes from the pool
inline size_t fixed_lag_bytes(size_t nN, size_t rows, size_t lag, size_t moments, size_t N, size_t T) {
  size_t cnt[kFixedLagBuffers], b = 0;
  const size_t H = (size_t)fixed_lag_columns((int)nN, (int)moments);
  fixed_lag_counts(nN, rows, lag * H, H, N, N, T, cnt);
  for (size_t v : cnt) b += v;
  return b * sizeof(double);
}

inline int fixed_lag_check_lag(int lag, int moments) {
  if (lag < 1 || lag > kFixedLagMaxLag) { set_error("lag must be in 1 .. " + std::to_string(kFixedLagMaxLag)); return RBPF_ERR_INVALID_ARG; }
  if (moments != 1 && moments != 2) { set_error("moments must be 1 (means) or 2 (means and covariances)"); return RBPF_ERR_INVALID_ARG; }
  return RBPF_OK;
}

// all or nothing; the carry (zeros: the slots of steps before the first) and the zeros are written in stream s
inline int fixed_lag_take(FixedLagCarry& f, DevicePool& pool, int nN, int rows, int K, int H, int N, int M, int P, hipStream_t s) {
  size_t cnt[kFixedLagBuffers];
  fixed_lag_counts((size_t)nN, (size_t)rows, (size_t)K, (size_t)H, (size_t)N, (size_t)M, (size_t)P, cnt);
  f = FixedLagCarry();
  f.pool = &pool; f.nN = nN; f.rows = rows; f.K = K; f.H = H;
  double** slot[kFixedLagBuffers] = {&f.Xhat, &f.pm, &f.ps, &f.zero, &f.D, &f.cj, &f.part, &f.T, &f.reach, &f.pages, &f.cs};
  int st = RBPF_OK;
  for (int k = 0; k < kFixedLagBuffers && st == RBPF_OK; ++k) st = pool.alloc(slot[k], cnt[k]);
  if (st == RBPF_OK) {
    hipError_t e = hipMemsetAsync(f.zero, 0, cnt[3] * sizeof(double), s);
    if (e == hipSuccess) e = hipMemsetAsync(f.T, 0, cnt[7] * sizeof(double), s);
    if (e == hipSuccess) e = hipMemsetAsync(f.pages, 0, cnt[9] * sizeof(double), s);
    if (e == hipSuccess) e = hipMemsetAsync(f.cs, 0, cnt[10] * sizeof(double), s);
    if (e != hipSuccess) st = hip_fail(e, "clearing the carry of the fixed-lag smoother", __FILE__, __LINE__);
  }
  if (st != RBPF_OK) { f.release(); return st; }
  f.alive = true;
  return RBPF_OK;
}

// the sizes and buffers of a step into the norm pass's and the carry pass's arguments (head, xn_next, tau and term are the caller's)
template <class Term>
void fixed_lag_set(const FixedLagCarry& f, int N, int M, MarginalArgs<Term>& a, FixedLagArgs<Term>& b) {
  marginal_set_sizes(a, N, M);
  a.Xhat = f.Xhat; a.cj = f.cj; a.part_m = f.pm; a.part_s = f.ps;
  b.N = N; b.M = M; b.C = forward_stats_chunk(N, M); b.nchunks = forward_stats_chunks(N, M); b.K = f.K;
  b.Xhat = f.Xhat; b.D = f.D; b.part = f.part;
}

// A step enters: c = the filter mean of X [nN][M] under w, T0 into slot 0 of T_step [K + H][M]; then the page of the step: est of
// every slot and the mass (reach null: the first step, mass = 1).
inline hipError_t fixed_lag_launch_enter(const FixedLagCarry& f, int moments, int M, const double* X, const double* w, double* T_step,
                                         const double* reach, double* c, double* page, hipStream_t s) {
  hipLaunchKernelGGL(fixed_lag_reduce_kernel, dim3(1), dim3(256), 0, s, f.nN, M, (size_t)M, X, (const double*)nullptr, w, 0, c);
  hipLaunchKernelGGL(fixed_lag_enter_kernel, dim3((M + 255) / 256), dim3(256), 0, s, f.nN, moments, M, X, (const double*)c, T_step);
  hipLaunchKernelGGL(fixed_lag_reduce_kernel, dim3(1), dim3(256), 0, s, f.K + f.H, M, (size_t)M, (const double*)T_step, reach, w, reach ? 2 : 1, page);
  return hipGetLastError();
}

// norm pass + merge (D) + carry pass + merge + mean + enter + reducer of one step, in stream order: b.tau (the slots 0 .. L-1 of
// step t) -> T_next (all slots of step t + 1), reach, c_next, page; X_next [nN][M], w_next [M]: the filter's particles and weights
// of step t + 1
template <class Term>
hipError_t fixed_lag_launch_step(const MarginalArgs<Term>& a, const FixedLagArgs<Term>& b, const FixedLagCarry& f, int moments,
                                 const double* X_next, const double* w_next, double* T_next, double* c_next, double* page, hipStream_t s) {
  const int bx = (a.M + kBackwardTile - 1) / kBackwardTile;
  const int bz = (b.K + kFixedLagKB - 1) / kFixedLagKB;
  hipLaunchKernelGGL((marginal_norm_pass_kernel<Term>), dim3(bx, a.nchunks), dim3(kBackwardTile), 0, s, a);
  hipLaunchKernelGGL(marginal_norm_merge_kernel, dim3((a.M + 255) / 256), dim3(256), 0, s, a.M, a.nchunks, a.part_m, a.part_s, (const double*)f.zero,
                     f.D, f.cj);
  hipLaunchKernelGGL((fixed_lag_pass_kernel<Term>), dim3(bx, b.nchunks, bz), dim3(kBackwardTile), 0, s, b);
  hipLaunchKernelGGL(forward_stats_merge_kernel, dim3((b.M + 255) / 256), dim3(256), 0, s, b.M, b.K + 1, b.nchunks, (const double*)b.part,
                     (const double*)f.D, T_next + (size_t)f.H * b.M, f.reach);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return fixed_lag_launch_enter(f, moments, b.M, X_next, w_next, T_next, f.reach, c_next, page, s);
}

// pages [Td][K + H + 1] and means [Td][nN] of the steps entered -> the caller's arrays (NULL outputs are skipped); the stream is idle
inline int fixed_lag_copy_out(const FixedLagCarry& f, double* pages, double* cs) {
  if (pages) HIPCHK(hipMemcpy(pages, f.pages, (size_t)f.entered * (f.K + f.H + 1) * sizeof(double), hipMemcpyDeviceToHost));
  if (cs) HIPCHK(hipMemcpy(cs, f.cs, (size_t)f.entered * f.nN * sizeof(double), hipMemcpyDeviceToHost));
  return RBPF_OK;
}

// the carry was built with this lag and these moments, or: reset first
inline int fixed_lag_same(const FixedLagCarry& f, int lag, int moments, const char* reset) {
  if (f.lag == lag && f.moments == moments) return RBPF_OK;
  set_error("the carry of the fixed-lag smoother was built with lag = " + std::to_string(f.lag) + ", moments = " + std::to_string(f.moments) +
            " (" + reset + " first)");
  return RBPF_ERR_STATE;
}

}  // namespace rbpf
