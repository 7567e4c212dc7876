// The backward-simulation recursion of the localisation smoothers, once for every map (forward filter, backward simulation:
// Godsill, Doucet & West 2004).  M trajectories are drawn backwards through the stored particles and weights of a localisation
// context (keep_history = 1, trace = 1):
//     b[T-1][j] = sample(w[T-1], u[T-1][j]);   t = T-2 .. 0:  l_i = log w[t][i] + logp(xs[t+1][j] | X[t][:, i]),  b[t][j] = sample(p, u[t][j])
// with p the log-sum-exp normalisation of l (particleSmoother.m:232, :236-238, :241) and sample = #{i : cumsum(p)_i < u}
// (tools/sample.m:30-32).  What a map family brings is logp, as a TERM: a struct, passed by value inside the kernel arguments
// (its uniform data stay in SGPRs), with
//     Term::Head                        the integers behind the sizes in BackwardArgs, `head`: `first` (1: the draw of step T-1,
//                                       l_i = log w_i) and the term's own small integers (which rows of a state it reads), in the
//                                       order the term wants, so that the scalar loads that bring the sizes bring them too
//     Term::NS                          predicted rows per particle; the LDS tile pitch and the rows of Xhat are NS + 1, log w last
//     Term::kLocateBound                launch bound of the locate kernel
//     term.load_x(head, xs_next, j, k)  row k of the NS rows of trajectory j that logp reads
//     term.pair(head, h, x, bound, l)   l += logp of one pair, h = the particle's NS + 1 doubles; false: the pair lies below
//                                       `bound` = the running max - kBackwardSkip (l is then not final, and its exp is exactly 0
//                                       wherever the term puts its test)
//     Term::kSplit                      true: instead of pair the term gives logp in two parts, pair_near(head, h, x) and
//                                       pair_far(head, h, x), and the kernels put the test between them (a cheap part that decides
//                                       and a dear one: the dense-mag map's position and orientation terms)
//     Term::NR, term.pair_res(head, h, x, bound, l, r)   pair (or pair_near, the test, pair_far) that also leaves the NR un-whitened
//                                       residuals of a pair it does not skip in r, kernel order (rbpf_loc_pairstats.hpp,
//                                       rbpf_loc_forwardstats.hpp)
//     term.gather(head, X, N, idx, xs, j) xs[j] <- all rows of particle idx
// The terms are BsTerm (the dense-mag map, rbpf_loc_smooth.hip) and GsTerm<NR, ANG, QP> (a generic map's Gaussian transitions,
// with or without a quaternion block, rbpf_loc_generic_smooth.hip); each file also has the prologue that writes Xhat.
//
// Kernels of one step t after the prologue (all in stream order):
//   backward_pass_kernel<Term>    all pairs.  Grid = (trajectory blocks of 256) x (particle chunks of C); a lane owns one trajectory,
//                                 keeps its rows in registers and a running (max, sum) pair; the particles come in tiles of 256
//                                 through LDS as [particle][NS + 1] and are read as broadcasts (all lanes one address).  No
//                                 cross-lane operation.  Writes one (max, sum) per (chunk, j).
//   backward_locate_kernel<Term>  per j: merge the chunk partials, find the chunk that holds u * total, walk it with the SAME
//                                 term, gather xs[t][j].
//   backward_mean_kernel          traj_smooth_mean[:, t] = plain means over j of all rows (particleFilterLocalization.m:123).
//   backward_logp_kernel<Term>    logp of every pair: the one-step probes' second output.
//
// SUMMATION ORDER (fixed; the indices depend on nothing else):
//   * inside a chunk, particles in ascending i: (m, s) <- l_i: if l_i > m: s = s exp(m - l_i) + 1, m = l_i; else s += exp(l_i - m);
//   * M_j = max over the chunks' m_c;  P_c = P_{c-1} + s_c exp(m_c - M_j) in ascending c, P_{-1} = 0; total = P_last;
//   * c0 = first c with P_c >= u total;  walk: acc = P_{c0-1}; ascending i in chunk c0: acc += exp(l_i - M_j); the first i
//     with a non-zero term and acc >= u total is b.  A walk that reaches the end of its chunk without crossing (the walk's sum and
//     the chunk's rescaled partial differ by rounding) goes on, acc carried over, through the following chunks with s_c > 0; if
//     none crosses, b = the last particle with a non-zero term (the clamp of a draw past the last cdf edge), counted in the
//     context's clamped-draw flag like the filter's.  w_i = 0 gives l_i = -inf and a zero term: never selected.
//   * C = chunk_size(N, M) below: a function of the two sizes only.
//
// PHILOX COUNTERS: u[t][j] = first uniform of philox_uniform2(seed, slot = j, step = t, lane = 0x42530000, iter = 0).  The filter's
// draws use lanes 0 .. 3 (rbpf_device.hpp), so the two ranges are disjoint for the same seed.
#pragma once
#include "../../include/rbpf.h"
#include "rbpf_internal.hpp"
#include "rbpf_device.hpp"
#include "rbpf_ctx.hpp"
#include "rbpf_loc_state.hpp"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

namespace rbpf {

constexpr int kBackwardTile = 256;               // particles per LDS tile = threads per workgroup
constexpr int kBackwardMaxChunk = 2048;          // largest chunk (particles): the walk of the locate kernel is at most this long per chunk
constexpr int kBackwardMaxRows = 8;              // widest state (rows of xs) the mean kernel takes
constexpr uint32_t kBackwardPhiloxLane = 0x42530000u;
constexpr double kBackwardSkip = 746.0;          // exp(x) == 0 for x < -745.14

// chunk of the all-pairs pass: enough (trajectory block) x (chunk) workgroups to give every CU four, in whole tiles
inline int backward_chunk_size(int N, int M) {
  const int bx = (M + kBackwardTile - 1) / kBackwardTile;
  const int want = std::max(1, (1024 + bx - 1) / bx);
  int C = ((N + want - 1) / want + kBackwardTile - 1) / kBackwardTile * kBackwardTile;
  return std::min(std::max(C, kBackwardTile), kBackwardMaxChunk);
}

template <class Term>
struct BackwardArgs {
  int N, M, C, nchunks;
  typename Term::Head head;        // .first and the term's integers
  const double* Xhat;              // [NS + 1][N]
  const double* X;                 // [rows][N] particles of this step (gather)
  const double* xs_next;           // [M][rows]
  const double* u;                 // [M]
  double* part_m; double* part_s;  // [nchunks][M]
  int* index;                      // [M]
  double* xs;                      // [M][rows] or null
  int* clamped;                    // device counter
  Term term;
  // the same step with another term over the same Head (the dispatch of a family whose term type is chosen at run time)
  template <class U>
  BackwardArgs<U> with(const U& t) const { return {N, M, C, nchunks, head, Xhat, X, xs_next, u, part_m, part_s, index, xs, clamped, t}; }
};

template <class Term>
__global__ __launch_bounds__(kBackwardTile) void backward_pass_kernel(const BackwardArgs<Term> a) {
  constexpr int NS = Term::NS;
  constexpr int S = NS + 1;
  __shared__ double tile[kBackwardTile * S];     // [particle][NS + 1]
  const int tid = threadIdx.x;
  const int j = blockIdx.x * kBackwardTile + tid;
  const int jl = min(j, a.M - 1);          // lanes past the end recompute the last trajectory; nothing of theirs is stored
  const int c = blockIdx.y;
  const int i0 = c * a.C, i1 = min(a.N, i0 + a.C);
  double x[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) x[k] = a.head.first ? 0.0 : a.term.load_x(a.head, a.xs_next, jl, k);
  double m = -INFINITY, s = 0.0;
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
      if (!a.head.first) {
        if constexpr (Term::kSplit) {
          l += a.term.pair_near(a.head, h, x);
          if (l < m - kBackwardSkip) continue;
          l += a.term.pair_far(a.head, h, x);
        } else {
          if (!a.term.pair(a.head, h, x, m - kBackwardSkip, l)) continue;
        }
      }
      if (l == -INFINITY) continue;
      const double d = l - m;
      const double ex = exp(-fabs(d));
      if (d > 0.0) { s = s * ex + 1.0; m = l; }
      else s += ex;
    }
  }
  if (j < a.M) {
    a.part_m[(size_t)c * a.M + j] = m;
    a.part_s[(size_t)c * a.M + j] = s;
  }
}

template <class Term>
__global__ __launch_bounds__((Term::kLocateBound)) void backward_locate_kernel(const BackwardArgs<Term> a) {
  constexpr int NS = Term::NS;
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.M) return;
  double x[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) x[k] = a.head.first ? 0.0 : a.term.load_x(a.head, a.xs_next, j, k);
  double Mx = -INFINITY;
  for (int c = 0; c < a.nchunks; ++c) Mx = fmax(Mx, a.part_m[(size_t)c * a.M + j]);
  int idx = -1;
  if (Mx > -INFINITY) {
    double total = 0.0;
    for (int c = 0; c < a.nchunks; ++c) {
      const double sc = a.part_s[(size_t)c * a.M + j];
      if (sc > 0.0) total += sc * exp(a.part_m[(size_t)c * a.M + j] - Mx);
    }
    const double target = a.u[j] * total;
    double acc = 0.0;
    int c0 = 0;
    for (; c0 < a.nchunks; ++c0) {
      const double sc = a.part_s[(size_t)c0 * a.M + j];
      if (!(sc > 0.0)) continue;
      const double nxt = acc + sc * exp(a.part_m[(size_t)c0 * a.M + j] - Mx);
      if (nxt >= target) break;
      acc = nxt;
    }
    int last_nz = -1;
    for (int c = c0; c < a.nchunks && idx < 0; ++c) {
      if (!(a.part_s[(size_t)c * a.M + j] > 0.0)) continue;
      const int i0 = c * a.C, i1 = min(a.N, i0 + a.C);
      for (int i = i0; i < i1; ++i) {
        double h[NS + 1];
        h[NS] = a.Xhat[(size_t)NS * a.N + i];
        if (h[NS] == -INFINITY) continue;
        double l = h[NS];
        if (!a.head.first) {
#pragma unroll
          for (int r = 0; r < NS; ++r) h[r] = a.Xhat[(size_t)r * a.N + i];
          if constexpr (Term::kSplit) {
            l += a.term.pair_near(a.head, h, x);
            if (l < Mx - kBackwardSkip) continue;
            l += a.term.pair_far(a.head, h, x);
          } else {
            if (!a.term.pair(a.head, h, x, Mx - kBackwardSkip, l)) continue;
          }
        }
        const double term = exp(l - Mx);
        if (!(term > 0.0)) continue;
        last_nz = i;
        acc += term;
        if (acc >= target) { idx = i; break; }
      }
    }
    if (idx < 0) idx = last_nz;
    if (idx < 0 || !(acc >= target)) atomicAdd(a.clamped, 1);
  } else {
    atomicAdd(a.clamped, 1);
  }
  if (idx < 0) {                                   // no non-zero term at all: the last particle with a non-zero weight
    for (int i = a.N - 1; i >= 0 && idx < 0; --i)
      if (a.Xhat[(size_t)NS * a.N + i] > -INFINITY) idx = i;
    if (idx < 0) idx = a.N - 1;
  }
  a.index[j] = idx;
  if (a.xs) a.term.gather(a.head, a.X, a.N, idx, a.xs, j);
}

// logp of every pair, without log w: out [N x M] column-major (the probes' second output)
template <class Term>
__global__ void backward_logp_kernel(const BackwardArgs<Term> a, double* __restrict__ out) {
  constexpr int NS = Term::NS;
  const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= (size_t)a.N * a.M) return;
  const int i = (int)(q % a.N), j = (int)(q / a.N);
  double h[NS + 1], x[NS];
#pragma unroll
  for (int r = 0; r < NS; ++r) h[r] = a.Xhat[(size_t)r * a.N + i];
  h[NS] = 0.0;
#pragma unroll
  for (int k = 0; k < NS; ++k) x[k] = a.term.load_x(a.head, a.xs_next, j, k);
  double l = 0.0;
  if constexpr (Term::kSplit) l = a.term.pair_near(a.head, h, x) + a.term.pair_far(a.head, h, x);
  else a.term.pair(a.head, h, x, -INFINITY, l);
  out[q] = l;
}

// mean over the M trajectories of xs [M][nN] -> out [nN]: one workgroup, strided partial sums, then a fixed tree
inline __global__ __launch_bounds__(256) void backward_mean_kernel(int M, int nN, const double* __restrict__ xs, double* __restrict__ out) {
  __shared__ double red[kBackwardMaxRows][256];
  const int tid = threadIdx.x;
  double acc[kBackwardMaxRows];
#pragma unroll
  for (int r = 0; r < kBackwardMaxRows; ++r) acc[r] = 0.0;
  for (int j = tid; j < M; j += 256)
#pragma unroll
    for (int r = 0; r < kBackwardMaxRows; ++r)
      if (r < nN) acc[r] += xs[(size_t)j * nN + r];
#pragma unroll
  for (int r = 0; r < kBackwardMaxRows; ++r) red[r][tid] = acc[r];
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off)
#pragma unroll
      for (int r = 0; r < kBackwardMaxRows; ++r) red[r][tid] += red[r][tid + off];
    __syncthreads();
  }
  if (tid < nN) out[tid] = red[tid][0] / (double)M;
}

inline __global__ void backward_philox_kernel(unsigned long long seed, int T, int M, double* __restrict__ u) {
  const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= (size_t)T * M) return;
  double u0, u1;
  philox_uniform2(seed, (uint32_t)(q % M), (uint32_t)(q / M), kBackwardPhiloxLane, 0u, u0, u1);
  u[q] = u0;
}

// ---- host side -----------------------------------------------------------------------------------------------------------
// What every backward pass asks of the forward run before it touches the device's history: stored particles and weights, every
// step done, no degenerate step on record.  `reader` and `who` are how the entry point names itself in the two refusals.
// Selects the context's device and leaves its stream idle.
inline int backward_check_forward(rbpf_ctx* c, const char* reader, const char* who) {
  if (!c->opt.keep_history || !c->opt.trace) {
    set_error(std::string(reader) + " reads the stored particles and weights: create the context with keep_history = 1 and trace = 1");
    return RBPF_ERR_STATE;
  }
  if (c->t < c->T) { set_error(std::string(who) + ": " + std::to_string(c->t) + " of " + std::to_string(c->T) + " steps are done"); return RBPF_ERR_STATE; }
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  std::vector<double> lse((size_t)c->T);
  HIPCHK(hipMemcpy(lse.data(), c->loc->d_lse, lse.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (int t = 0; t < c->T; ++t)
    if (!(lse[t] > std::log(1e-12))) {
      set_error("the forward run recorded a degenerate step (t = " + std::to_string(t) + "): its weights are no filtering distribution");
      return RBPF_ERR_STATE;
    }
  return RBPF_OK;
}

// d_u [T][M] <- the caller's uniforms, or (u null) the Philox draws of `seed`
inline int backward_uniforms(const double* u, uint64_t seed, int T, int M, double* d_u, hipStream_t s) {
  hipError_t e;
  if (u) {
    e = hipMemcpy(d_u, u, (size_t)T * M * sizeof(double), hipMemcpyHostToDevice);
  } else {
    const size_t cnt = (size_t)T * M;
    hipLaunchKernelGGL(backward_philox_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, (unsigned long long)seed, T, M, d_u);
    e = hipGetLastError();
  }
  return e == hipSuccess ? RBPF_OK : hip_fail(e, "uniforms of the backward pass", __FILE__, __LINE__);
}

// all-pairs pass + locate of one step, in stream order (the family's prologue goes before it)
template <class Term>
hipError_t backward_launch_step(const BackwardArgs<Term>& a, hipStream_t s) {
  hipLaunchKernelGGL((backward_pass_kernel<Term>), dim3((a.M + kBackwardTile - 1) / kBackwardTile, a.nchunks), dim3(kBackwardTile), 0, s, a);
  hipLaunchKernelGGL((backward_locate_kernel<Term>), dim3((a.M + 63) / 64), dim3(64), 0, s, a);
  return hipGetLastError();
}

template <class Term>
hipError_t backward_launch_logp(const BackwardArgs<Term>& a, double* logp, hipStream_t s) {
  const size_t cnt = (size_t)a.N * a.M;
  hipLaunchKernelGGL((backward_logp_kernel<Term>), dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, a, logp);
  return hipGetLastError();
}

inline hipError_t backward_launch_mean(int M, int nN, const double* xs, double* out, hipStream_t s) {
  hipLaunchKernelGGL(backward_mean_kernel, dim3(1), dim3(256), 0, s, M, nN, xs, out);
  return hipGetLastError();
}

}  // namespace rbpf
