// The two-slice (pairwise) smoothed moments of the transition residual, once for every map: with the marginal smoothing weights of
// rbpf_loc_marginal.hpp at hand, the joint smoothing weight of predecessor i at step t and successor j at step t + 1 is
//     xi_t(i, j) = w_t(i) p(X[t+1][:, j] | X[t][:, i]) w_{t+1|T}(j) / D_t(j)                    (sums to 1 over all pairs)
// and what a calibration of the transition noise needs of it are the moments of the term's UN-WHITENED residual r_ij,
//     S_t = sum_ij xi_t(i, j) r_ij r_ij',     m_t = sum_ij xi_t(i, j) r_ij,     pair_mass_t = sum_ij xi_t(i, j)
// (S_t: the E-step of EM for the noise covariance; m_t: the smoothed odometry bias; pair_mass_t: 1 in exact arithmetic).  The N x N
// matrix xi never exists: one more all-pairs pass reduces every pair into K = NR (NR + 3) / 2 + 1 numbers on the fly.  In the log domain
//     log xi_t(i, j) = log w_t(i) + (c(j) - log mass_t) + logp(j | i),       c(j) = log w_{t+1|T}(j) - D_t(j)
// c and mass_t are what the marginal step of t left behind: the pass runs after that step's marginal_normalise_kernel.
//
// A TERM (rbpf_loc_backward.hpp) gives the residual through one more member next to pair / pair_near / pair_far:
//     term.pair_res(head, h, x, bound, l, r)   the arithmetic of pair (or pair_near, the test, pair_far), the skip test in the same
//                                              place; false: the pair lies below `bound`; otherwise l is bit for bit what pair
//                                              gives and r [Term::NR] the un-whitened residual in kernel order.
//
// Kernels of one step t (in stream order, after the marginal step's normalisation):
//   pair_stats_pass_kernel<Term>   the grid and tile of marginal_weight_pass_kernel: (predecessor blocks of 256) x (successor chunks
//                                  of backward_chunk_size(M, N)); a lane owns predecessor i and keeps its NS + 1 doubles of Xhat in
//                                  registers; the successors come through LDS as [successor][NS + 1], read as broadcasts, the last
//                                  entry staged as c(j) - log(mass_t) (-inf where c(j) is -inf or mass_t is 0).  Per pair
//                                  l = log w(i) + that entry, pair_res with the CONSTANT bound -kBackwardSkip (every xi <= 1: no
//                                  running maximum, no rescaling; a pair below -746 contributes exactly 0, so the skip stays exact),
//                                  xi = exp(l), then K fma into the lane's accumulators: the lower triangle of S by rows, m, the
//                                  mass.  l = -inf contributes nothing.  Lanes past the end recompute the last predecessor and
//                                  their accumulators are cleared before the sum.  After the loop the 256 lanes' accumulators are
//                                  summed through the tile's LDS, NS + 1 of them at a time, every one by the fixed tree of
//                                  marginal_tree_sum; one [K] vector per workgroup is written, nothing per lane.
//   pair_stats_reduce_kernel       one workgroup: the blocks x chunks partials of every one of the K numbers as strided partials
//                                  (lane k: workgroups k, k + 256, ..) and the same tree; writes S (both triangles), m and the mass
//                                  of page t, in kernel order.
// SUMMATION ORDER: fixed, a function of (N, M) only: ascending j inside a chunk, the tree over the lanes of a workgroup, the strided
// partials over the workgroups (chunk-major: workgroup = chunk * blocks + block) and the tree again.  No atomics.
#pragma once
#include "../../include/rbpf.h"
#include "rbpf_internal.hpp"
#include "rbpf_loc_backward.hpp"
#include "rbpf_loc_marginal.hpp"

namespace rbpf {

constexpr int pair_stats_count(int NR) { return NR * (NR + 3) / 2 + 1; }      // K: lower triangle of S, m, the mass
constexpr int pair_stats_page(int NR) { return NR * NR + NR + 1; }            // a page as the reducer writes it: S [NR x NR], m, the mass

template <class Term>
struct PairStatsArgs {
  int N, M;                        // predecessors, successors (M = N outside the probes)
  int Cw, nchunks_w;               // successor chunks, backward_chunk_size(M, N): the weight pass's
  typename Term::Head head;        // the term's integers (.first is 0)
  const double* Xhat;              // [NS + 1][N], last row log w_t
  const double* xn_next;           // [rows][M]: the successors, particles of step t + 1
  const double* cj;                // [M]: c(j)
  const double* mass;              // [1]: the step's mass, as marginal_normalise_kernel wrote it
  double* part;                    // [K][blocks * nchunks_w]: one vector per workgroup
  Term term;
  template <class U>
  PairStatsArgs<U> with(const U& t) const { return {N, M, Cw, nchunks_w, head, Xhat, xn_next, cj, mass, part, t}; }
};

template <class Term>
__global__ __launch_bounds__(kBackwardTile) void pair_stats_pass_kernel(const PairStatsArgs<Term> a) {
  constexpr int NS = Term::NS;
  constexpr int NR = Term::NR;
  constexpr int S = NS + 1;
  constexpr int K = pair_stats_count(NR);
  constexpr int TRI = NR * (NR + 1) / 2;
  __shared__ double tile[kBackwardTile * S];     // [successor][NS + 1]: its rows, c(j) - log(mass) last; then the lanes' accumulators
  const int tid = threadIdx.x;
  const int i = blockIdx.x * kBackwardTile + tid;
  const int il = min(i, a.N - 1);          // lanes past the end recompute the last predecessor; their sums are cleared below
  const int c = blockIdx.y;
  const int j0 = c * a.Cw, j1 = min(a.M, j0 + a.Cw);
  const double mass = *a.mass;
  const double lm = mass > 0.0 ? log(mass) : -INFINITY;
  double h[S];
#pragma unroll
  for (int r = 0; r < S; ++r) h[r] = a.Xhat[(size_t)r * a.N + il];
  double acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0.0;
  for (int base = j0; base < j1; base += kBackwardTile) {
    const int cnt = min(kBackwardTile, j1 - base);
    __syncthreads();
    if (tid < cnt) {
#pragma unroll
      for (int r = 0; r < NS; ++r) tile[tid * S + r] = a.term.load_next(a.head, a.xn_next, a.M, base + tid, r);
      const double cv = a.cj[base + tid];
      tile[tid * S + NS] = (cv > -INFINITY && lm > -INFINITY) ? cv - lm : -INFINITY;   // (mass = 0: nothing contributes, no NaN)
    }
    __syncthreads();
    for (int k = 0; k < cnt; ++k) {
      const double (&x)[NS] = *reinterpret_cast<const double (*)[NS]>(tile + k * S);
      double l = h[NS] + tile[k * S + NS];
      double r[NR];
      if (!a.term.pair_res(a.head, h, x, -kBackwardSkip, l, r)) continue;
      if (l == -INFINITY) continue;
      const double xi = exp(l);
#pragma unroll
      for (int p = 0; p < NR; ++p) {
        const double xr = xi * r[p];
#pragma unroll
        for (int q = 0; q <= p; ++q) acc[p * (p + 1) / 2 + q] = fma(xr, r[q], acc[p * (p + 1) / 2 + q]);
        acc[TRI + p] = fma(xi, r[p], acc[TRI + p]);
      }
      acc[K - 1] += xi;
    }
  }
  if (i >= a.N) {
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
  }
  // the workgroup's sums: S accumulators at a time through the tile ([value][lane]), each by the tree of marginal_tree_sum
  const size_t nwg = (size_t)gridDim.x * gridDim.y;
  const size_t wg = (size_t)c * gridDim.x + blockIdx.x;
#pragma unroll
  for (int b0 = 0; b0 < K; b0 += S) {
    const int nb = (K - b0) < S ? (K - b0) : S;
    __syncthreads();
#pragma unroll
    for (int v = 0; v < S; ++v)
      if (b0 + v < K) tile[v * kBackwardTile + tid] = acc[b0 + v];
    __syncthreads();
    for (int sh = 7; sh >= 0; --sh) {
      const int off = 1 << sh;
      for (int q = tid; q < nb * off; q += kBackwardTile) {
        const int v = q >> sh, p = q & (off - 1);
        tile[v * kBackwardTile + p] += tile[v * kBackwardTile + p + off];
      }
      __syncthreads();
    }
    if (tid < nb) a.part[(size_t)(b0 + tid) * nwg + wg] = tile[tid * kBackwardTile];
  }
}

// part [K][nwg] -> out [NR * NR + NR + 1]: S [NR x NR] (both triangles), m [NR], the mass; kernel order.  One workgroup of 256.
inline __global__ __launch_bounds__(256) void pair_stats_reduce_kernel(int NR, int nwg, const double* __restrict__ part, double* __restrict__ out) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  const int tri = NR * (NR + 1) / 2, K = tri + NR + 1;
  int p = 0, q = 0;                              // (row, column) of value k while k < tri
  for (int k = 0; k < K; ++k) {
    double acc = 0.0;
    for (int g = tid; g < nwg; g += 256) acc += part[(size_t)k * nwg + g];
    const double v = marginal_tree_sum(acc, red, tid);
    if (tid == 0) {
      if (k < tri) { out[p + NR * q] = v; out[q + NR * p] = v; }
      else out[NR * NR + (k - tri)] = v;
    }
    if (k < tri && ++q > p) { ++p; q = 0; }
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------
template <class Term>
void pair_stats_set_sizes(PairStatsArgs<Term>& a, int N, int M) {
  a.N = N; a.M = M;
  a.Cw = backward_chunk_size(M, N); a.nchunks_w = (M + a.Cw - 1) / a.Cw;
}

// workgroups of the pass = vectors in `part`
inline size_t pair_stats_groups(size_t N, size_t M) {
  const size_t Cw = (size_t)backward_chunk_size((int)M, (int)N);
  return (N + kBackwardTile - 1) / kBackwardTile * ((M + Cw - 1) / Cw);
}

// pass + reduce of one step, in stream order: page [pair_stats_page(NR)]
template <class Term>
hipError_t pair_stats_launch_step(const PairStatsArgs<Term>& a, double* page, hipStream_t s) {
  const int blocks = (a.N + kBackwardTile - 1) / kBackwardTile;
  hipLaunchKernelGGL((pair_stats_pass_kernel<Term>), dim3(blocks, a.nchunks_w), dim3(kBackwardTile), 0, s, a);
  hipLaunchKernelGGL(pair_stats_reduce_kernel, dim3(1), dim3(256), 0, s, (int)Term::NR, blocks * a.nchunks_w, a.part, page);
  return hipGetLastError();
}

// What a statistics pass keeps in a BackwardWorkspace next to the marginal pass's buffers (take_pair_stats): pstat [K][workgroups] the
// workgroups' vectors, stat [T - 1][NR * NR + NR + 1] the pages.
inline size_t pair_stats_bytes(size_t nN, size_t rows, size_t n_res, size_t N, size_t T) {
  return marginal_bytes(nN, rows, N, T) +
         ((size_t)pair_stats_count((int)n_res) * pair_stats_groups(N, N) + (T - 1) * (size_t)pair_stats_page((int)n_res)) * sizeof(double);
}

inline int pair_stats_take(BackwardWorkspace& ws, DevicePool& pool, int nN, int rows, int n_res, int N, int T) {
  return ws.take_pair_stats(pool, (size_t)(rows + 1) * N, marginal_part_count((size_t)N, (size_t)N), (size_t)3 * N, (size_t)T * N,
                            (size_t)(nN + nN * nN + 2) * T, (size_t)pair_stats_count(n_res) * pair_stats_groups((size_t)N, (size_t)N),
                            (size_t)(T - 1) * pair_stats_page(n_res));
}

// the pages of a pass -> the caller's S [n x n x (T-1)], m [n x (T-1)], pair_mass [T-1] (NULL outputs are skipped); perm (may be
// null: the identity): kernel residual k is residual perm[k] of the caller
inline int pair_stats_copy_out(const BackwardWorkspace& ws, int n, int T, const int* perm, double* S, double* m, double* pair_mass) {
  if (T < 2 || (!S && !m && !pair_mass)) return RBPF_OK;
  const size_t pg = (size_t)pair_stats_page(n);
  std::vector<double> h(pg * (T - 1));
  HIPCHK(hipMemcpy(h.data(), ws.stat, h.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (int t = 0; t + 1 < T; ++t) {
    const double* src = h.data() + pg * t;
    for (int b = 0; b < n; ++b) {
      const int pb = perm ? perm[b] : b;
      if (m) m[(size_t)n * t + pb] = src[(size_t)n * n + b];
      if (S)
        for (int a = 0; a < n; ++a) S[(size_t)n * n * t + (perm ? perm[a] : a) + (size_t)n * pb] = src[a + (size_t)n * b];
    }
    if (pair_mass) pair_mass[t] = src[(size_t)n * n + n];
  }
  return RBPF_OK;
}

}  // namespace rbpf
