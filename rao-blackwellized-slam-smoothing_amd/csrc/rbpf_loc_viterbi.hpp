// The MAP trajectory of the localisation filters, once for every map: MAP sequence estimation over the stored particles (Godsill,
// Doucet & West 2001), a Viterbi recursion whose states at step t are the N stored particles of a localisation context
// (keep_history = 1, trace = 1):
//     delta_0(j)     = log w_0(j)
//     delta_{t+1}(j) = log w_{t+1}(j) + max_i [ delta_t(i) + logp(X[t+1][:, j] | X[t][:, i]) ],   psi_{t+1}(j) = the arg max
//     i_{T-1} = arg max_j delta_{T-1}(j),   i_t = psi_{t+1}(i_{t+1}),   x_map[:, t] = X[t][:, i_t],   score = delta_{T-1}(i_{T-1})
// Among equal candidates the LOWEST index wins, at every max.  log w_t stands in for log g(y_t | x_t): the filter resamples at every
// step, so the normalised weights are the likelihoods up to one constant per step, which moves no arg max.  logp is a TERM of
// rbpf_loc_backward.hpp (BsTerm, GsTerm<NR, ANG, QP>), with one more member:
//     term.load_next(head, xn, ld, j, k)   row k of the NS rows of successor j that logp reads, from particles held [rows][ld]
// The predecessors come from the family's prologue as Xhat [NS + 1][N]; its last row (log w there) is overwritten with delta_t.
//
// Kernels of one step t -> t + 1 after the prologue (all in stream order):
//   viterbi_pass_kernel<Term>   all pairs, max-plus.  The grid of backward_pass_kernel: (successor blocks of 256) x (particle chunks
//                               of backward_chunk_size); a lane owns successor j, keeps its NS rows in registers and a running
//                               (best, arg); the predecessors come in tiles of 256 through LDS as [particle][NS + 1] and are read
//                               as broadcasts, in ascending i, and only l > best updates: the lowest index wins.  No cross-lane
//                               operation.  Writes one (best, arg) per (chunk, j).
//   viterbi_merge_kernel        per j: the chunks in ascending c, strict >; delta_{t+1}(j) = log w_{t+1}(j) + best, psi = arg.  A
//                               successor whose delta is -inf (every candidate -inf, or w = 0) gets psi = 0.
//   viterbi_backtrack_kernel    one lane: the lowest arg max of delta_{T-1}, the walk through psi, the gather of x_map.
//
// THE SKIP IS EXACT.  Every part of logp is -z'z / 2 <= 0 and is accumulated monotonically, so a partial sum below the running best
// can never recover: the terms' own test runs with bound = best (the backward pass needs best - 746), and a skipped pair could
// not have changed (best, arg), ties included (a tie never updates).
#pragma once
#include "../../include/rbpf.h"
#include "rbpf_internal.hpp"
#include "rbpf_loc_backward.hpp"

namespace rbpf {

template <class Term>
struct ViterbiArgs {
  int N, M, C, nchunks;            // predecessors, successors (M = N outside the probes), chunk, chunks
  typename Term::Head head;        // the term's integers (.first is 0)
  const double* Xhat;              // [NS + 1][N], last row delta_t
  const double* xn_next;           // [rows][M]: the successors, particles of step t + 1
  double* part_best;               // [nchunks][M]
  int* part_arg;                   // [nchunks][M]
  Term term;
  template <class U>
  ViterbiArgs<U> with(const U& t) const { return {N, M, C, nchunks, head, Xhat, xn_next, part_best, part_arg, t}; }
};

template <class Term>
__global__ __launch_bounds__(kBackwardTile) void viterbi_pass_kernel(const ViterbiArgs<Term> a) {
  constexpr int NS = Term::NS;
  constexpr int S = NS + 1;
  __shared__ double tile[kBackwardTile * S];     // [particle][NS + 1]
  const int tid = threadIdx.x;
  const int j = blockIdx.x * kBackwardTile + tid;
  const int jl = min(j, a.M - 1);          // lanes past the end recompute the last successor; nothing of theirs is stored
  const int c = blockIdx.y;
  const int i0 = c * a.C, i1 = min(a.N, i0 + a.C);
  double x[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) x[k] = a.term.load_next(a.head, a.xn_next, a.M, jl, k);
  double best = -INFINITY;
  int arg = 0;
  for (int base = i0; base < i1; base += kBackwardTile) {
    const int cnt = min(kBackwardTile, i1 - base);
    __syncthreads();
    if (tid < cnt) {
#pragma unroll
      for (int r = 0; r < S; ++r) tile[tid * S + r] = a.Xhat[(size_t)r * a.N + base + tid];
    }
    __syncthreads();
    for (int k = 0; k < cnt; ++k) {
      const double* h = tile + k * S;
      double l = h[NS];
      if constexpr (Term::kSplit) {
        l += a.term.pair_near(a.head, h, x);
        if (l < best) continue;
        l += a.term.pair_far(a.head, h, x);
      } else {
        if (!a.term.pair(a.head, h, x, best, l)) continue;
      }
      if (l > best) { best = l; arg = base + k; }
    }
  }
  if (j < a.M) {
    a.part_best[(size_t)c * a.M + j] = best;
    a.part_arg[(size_t)c * a.M + j] = arg;
  }
}

// w_next null (the probes): delta = best.
inline __global__ void viterbi_merge_kernel(int M, int nchunks, const double* __restrict__ part_best, const int* __restrict__ part_arg,
                                            const double* __restrict__ w_next, double* __restrict__ delta, int* __restrict__ psi) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= M) return;
  double best = -INFINITY;
  int arg = 0;
  for (int c = 0; c < nchunks; ++c) {
    const double b = part_best[(size_t)c * M + j];
    if (b > best) { best = b; arg = part_arg[(size_t)c * M + j]; }
  }
  double d = best;
  if (w_next) {
    const double wj = w_next[j];
    d = wj > 0.0 ? log(wj) + best : -INFINITY;
  }
  delta[j] = d;
  psi[j] = d > -INFINITY ? arg : 0;
}

// delta_0 = log w_0
inline __global__ void viterbi_init_kernel(int N, const double* __restrict__ w, double* __restrict__ delta) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const double wi = w[i];
  delta[i] = wi > 0.0 ? log(wi) : -INFINITY;
}

// X [T][nN][N], psi [T][N] (row 0 is not read), delta = delta_{T-1} -> x_map [T][nN], index [T], score [1]
inline __global__ void viterbi_backtrack_kernel(int N, int T, int nN, const double* __restrict__ X, const int* __restrict__ psi,
                                                const double* __restrict__ delta, double* __restrict__ x_map, int* __restrict__ index,
                                                double* __restrict__ score) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double best = delta[0];
  int i = 0;
  for (int j = 1; j < N; ++j)
    if (delta[j] > best) { best = delta[j]; i = j; }
  *score = best;
  for (int t = T - 1; t >= 0; --t) {
    index[t] = i;
    for (int r = 0; r < nN; ++r) x_map[(size_t)t * nN + r] = X[((size_t)t * nN + r) * N + i];
    if (t > 0) i = psi[(size_t)t * N + i];
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------
// delta_t over the last row of Xhat (the prologue wrote log w there) + all-pairs pass, in stream order
template <class Term>
hipError_t viterbi_launch_pass(const ViterbiArgs<Term>& a, const double* delta, double* Xhat, hipStream_t s) {
  const hipError_t e = hipMemcpyAsync(Xhat + (size_t)Term::NS * a.N, delta, (size_t)a.N * sizeof(double), hipMemcpyDeviceToDevice, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((viterbi_pass_kernel<Term>), dim3((a.M + kBackwardTile - 1) / kBackwardTile, a.nchunks), dim3(kBackwardTile), 0, s, a);
  return hipGetLastError();
}

inline hipError_t viterbi_launch_merge(int M, int nchunks, const double* part_best, const int* part_arg, const double* w_next, double* delta,
                                       int* psi, hipStream_t s) {
  hipLaunchKernelGGL(viterbi_merge_kernel, dim3((M + 255) / 256), dim3(256), 0, s, M, nchunks, part_best, part_arg, w_next, delta, psi);
  return hipGetLastError();
}

inline hipError_t viterbi_launch_init(int N, const double* w, double* delta, hipStream_t s) {
  hipLaunchKernelGGL(viterbi_init_kernel, dim3((N + 255) / 256), dim3(256), 0, s, N, w, delta);
  return hipGetLastError();
}

inline hipError_t viterbi_launch_backtrack(int N, int T, int nN, const double* X, const int* psi, const double* delta, double* x_map,
                                           int* index, double* score, hipStream_t s) {
  hipLaunchKernelGGL(viterbi_backtrack_kernel, dim3(1), dim3(64), 0, s, N, T, nN, X, psi, delta, x_map, index, score);
  return hipGetLastError();
}

// The buffers of a MAP pass in a BackwardWorkspace (rbpf_loc_state.hpp, take_map): Xhat [rows + 1][N]; pm, arg [nchunks][N] the chunk
// partials; u [2][N] two rows of delta (delta_t in row t & 1); idx = psi [T][N], then the path's index [T]; mean = x_map [T][nN],
// then the score.
inline size_t viterbi_bytes(size_t nN, size_t rows, size_t N, size_t T) {
  const size_t C = (size_t)backward_chunk_size((int)N, (int)N), nch = (N + C - 1) / C;
  return ((rows + 1) * N + nch * N + 2 * N + nN * T + 1) * sizeof(double) + (nch * N + T * N + T) * sizeof(int);
}

inline int viterbi_take(BackwardWorkspace& ws, DevicePool& pool, int nN, int rows, int N, int T) {
  const size_t C = (size_t)backward_chunk_size(N, N), nch = ((size_t)N + C - 1) / C;
  return ws.take_map(pool, (size_t)(rows + 1) * N, nch * N, (size_t)2 * N, (size_t)T * N + T, (size_t)nN * T + 1);
}

// what rbpf_loc_map_trajectory / rbpf_loc_generic_map_finish copy out: x_map [nN x T] column-major, index [T], score
inline int viterbi_copy_out(const BackwardWorkspace& ws, int nN, int N, int T, double* x_map, int32_t* index, double* score) {
  if (x_map) HIPCHK(hipMemcpy(x_map, ws.mean, (size_t)nN * T * sizeof(double), hipMemcpyDeviceToHost));
  if (index) HIPCHK(hipMemcpy(index, ws.idx + (size_t)T * N, (size_t)T * sizeof(int), hipMemcpyDeviceToHost));
  if (score) HIPCHK(hipMemcpy(score, ws.mean + (size_t)nN * T, sizeof(double), hipMemcpyDeviceToHost));
  return RBPF_OK;
}

}  // namespace rbpf
