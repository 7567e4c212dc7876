// The marginal smoothing weights of the localisation filters, once for every map: forward filtering, backward smoothing (FFBSm,
// Doucet, Godsill & Andrieu 2000) over the stored particles X[t] and weights w[t] of a localisation context (keep_history = 1,
// trace = 1), all N of them at every step:
//     w_{T-1|T}(i) = w_{T-1}(i)
//     D_t(j)       = sum_l w_t(l) p(X[t+1][:, j] | X[t][:, l])                                  for every successor j
//     w_{t|T}(i)   = w_t(i) sum_j w_{t+1|T}(j) p(X[t+1][:, j] | X[t][:, i]) / D_t(j)            t = T-2 .. 0
// in the log domain, in fp64: with c(j) = log w_{t+1|T}(j) - D(j) (D the log of the sum above),
//     lws(i) = log sum_j exp(log w_t(i) + c(j) + logp(j | i)),   mass = sum_i exp(lws(i)),   log w_{t|T}(i) = lws(i) - log(mass)
// mass is 1 in exact arithmetic and is kept per step as a diagnostic.  A successor that carries no smoothed weight, or that no
// predecessor reaches (D = -inf), has c = -inf and passes nothing back; a particle with w = 0 gets lws = -inf, weight exactly 0.
// logp is a TERM of rbpf_loc_backward.hpp (BsTerm, GsTerm<NR, ANG, QP>) with the load_next of rbpf_loc_viterbi.hpp: the successors
// are particles, read where they lie ([rows][ld]).  The predecessors come from the family's prologue as Xhat [NS + 1][N], log w last.
//
// Kernels of one step t after the prologue (all in stream order):
//   marginal_norm_pass_kernel<Term>    D, all pairs.  The grid, LDS tile, (m, s) recurrence and skip of backward_pass_kernel:
//                                      (successor blocks of 256) x (predecessor chunks of backward_chunk_size(N, M)); a lane owns
//                                      successor j.  Writes one (m, s) per (chunk, j).
//   marginal_norm_merge_kernel         per j: Mx = max_c m_c, D(j) = Mx + log(sum_c s_c exp(m_c - Mx)) in ascending c,
//                                      c(j) = logws_next(j) - D(j), -inf where logws_next(j) or D(j) is -inf.
//   marginal_weight_pass_kernel<Term>  the transposed pass.  Grid = (predecessor blocks of 256) x (successor chunks of
//                                      backward_chunk_size(M, N)); a lane owns predecessor i and keeps its NS + 1 doubles of Xhat
//                                      in registers; the successors come in tiles of 256 through LDS as [successor][NS + 1], the
//                                      NS rows load_next gives and c(j) last, and are read as broadcasts (all lanes one address).
//                                      Per pair l = log w(i) + c(j), then the term (h = the lane's registers, x = the tile's row)
//                                      with bound m - kBackwardSkip, the same (m, s) recurrence in ascending j.  No cross-lane
//                                      operation.  Writes one (m, s) per (chunk, i).
//   marginal_weight_merge_kernel       per i: the chunks as in the norm merge -> lws(i), un-normalised.
//   marginal_normalise_kernel          one workgroup: mass = sum_i exp(lws(i)) as strided partials (lane k: i = k, k + 256, ..)
//                                      and a fixed tree, the way backward_mean_kernel sums; logws(i) = lws(i) - log(mass),
//                                      w_smooth(i) = exp of it.
//   marginal_moments_kernel            one workgroup per step: mean [nN] = sum_i w(i) X[:, i], cov [nN x nN] = sum_i w(i) (X[:, i] -
//                                      mean)(X[:, i] - mean)', ess = 1 / sum_i w(i)^2, the same strided partials and tree.  The
//                                      means are PLAIN weighted means of all rows, the way the filter's traj_mean treats them:
//                                      angle and quaternion rows get no special handling (no wrap, no renormalisation).
//
// THE SKIP IS EXACT in both passes: every part of logp is <= 0 and is added monotonically, so a partial sum below m - 746 has an
// exp of exactly 0.  SUMMATION ORDER: fixed, a function of (N, M) only -- ascending index inside a chunk, ascending chunk in the
// merges, strided partials and a fixed tree in the two one-workgroup kernels.
#pragma once
#include "../../include/rbpf.h"
#include "rbpf_internal.hpp"
#include "rbpf_loc_backward.hpp"

namespace rbpf {

template <class Term>
struct MarginalArgs {
  int N, M;                        // predecessors, successors (M = N outside the probes)
  int C, nchunks;                  // norm pass: predecessor chunks, backward_chunk_size(N, M)
  int Cw, nchunks_w;               // weight pass: successor chunks, backward_chunk_size(M, N)
  typename Term::Head head;        // the term's integers (.first is 0)
  const double* Xhat;              // [NS + 1][N], last row log w_t
  const double* xn_next;           // [rows][M]: the successors, particles of step t + 1
  const double* cj;                // [M]: c(j) (the weight pass)
  double* part_m; double* part_s;  // [nchunks][M] in the norm pass, [nchunks_w][N] in the weight pass
  Term term;
  template <class U>
  MarginalArgs<U> with(const U& t) const { return {N, M, C, nchunks, Cw, nchunks_w, head, Xhat, xn_next, cj, part_m, part_s, t}; }
};

template <class Term>
__global__ __launch_bounds__(kBackwardTile) void marginal_norm_pass_kernel(const MarginalArgs<Term> a) {
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
      if constexpr (Term::kSplit) {
        l += a.term.pair_near(a.head, h, x);
        if (l < m - kBackwardSkip) continue;
        l += a.term.pair_far(a.head, h, x);
      } else {
        if (!a.term.pair(a.head, h, x, m - kBackwardSkip, l)) continue;
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
__global__ __launch_bounds__(kBackwardTile) void marginal_weight_pass_kernel(const MarginalArgs<Term> a) {
  constexpr int NS = Term::NS;
  constexpr int S = NS + 1;
  __shared__ double tile[kBackwardTile * S];     // [successor][NS + 1]: its rows, c(j) last
  const int tid = threadIdx.x;
  const int i = blockIdx.x * kBackwardTile + tid;
  const int il = min(i, a.N - 1);          // lanes past the end recompute the last predecessor; nothing of theirs is stored
  const int c = blockIdx.y;
  const int j0 = c * a.Cw, j1 = min(a.M, j0 + a.Cw);
  double h[S];
#pragma unroll
  for (int r = 0; r < S; ++r) h[r] = a.Xhat[(size_t)r * a.N + il];
  double m = -INFINITY, s = 0.0;
  for (int base = j0; base < j1; base += kBackwardTile) {
    const int cnt = min(kBackwardTile, j1 - base);
    __syncthreads();
    if (tid < cnt) {
#pragma unroll
      for (int r = 0; r < NS; ++r) tile[tid * S + r] = a.term.load_next(a.head, a.xn_next, a.M, base + tid, r);
      tile[tid * S + NS] = a.cj[base + tid];
    }
    __syncthreads();
    for (int k = 0; k < cnt; ++k) {
      const double (&x)[NS] = *reinterpret_cast<const double (*)[NS]>(tile + k * S);
      double l = h[NS] + tile[k * S + NS];
      if constexpr (Term::kSplit) {
        l += a.term.pair_near(a.head, h, x);
        if (l < m - kBackwardSkip) continue;
        l += a.term.pair_far(a.head, h, x);
      } else {
        if (!a.term.pair(a.head, h, x, m - kBackwardSkip, l)) continue;
      }
      if (l == -INFINITY) continue;
      const double d = l - m;
      const double ex = exp(-fabs(d));
      if (d > 0.0) { s = s * ex + 1.0; m = l; }
      else s += ex;
    }
  }
  if (i < a.N) {
    a.part_m[(size_t)c * a.N + i] = m;
    a.part_s[(size_t)c * a.N + i] = s;
  }
}

// the chunks' (m, s) of one column -> the log of their sum, ascending c; -inf if every chunk is empty
__device__ __forceinline__ double marginal_merge_chunks(int n, int nchunks, int q, const double* __restrict__ part_m,
                                                        const double* __restrict__ part_s) {
  double Mx = -INFINITY;
  for (int c = 0; c < nchunks; ++c) Mx = fmax(Mx, part_m[(size_t)c * n + q]);
  if (!(Mx > -INFINITY)) return -INFINITY;
  double total = 0.0;
  for (int c = 0; c < nchunks; ++c) {
    const double sc = part_s[(size_t)c * n + q];
    if (sc > 0.0) total += sc * exp(part_m[(size_t)c * n + q] - Mx);
  }
  return Mx + log(total);
}

// D [M] may be null (only the probes keep it)
inline __global__ void marginal_norm_merge_kernel(int M, int nchunks, const double* __restrict__ part_m, const double* __restrict__ part_s,
                                                  const double* __restrict__ logws_next, double* __restrict__ D, double* __restrict__ cj) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= M) return;
  const double d = marginal_merge_chunks(M, nchunks, j, part_m, part_s);
  const double lw = logws_next[j];
  if (D) D[j] = d;
  cj[j] = (lw > -INFINITY && d > -INFINITY) ? lw - d : -INFINITY;
}

inline __global__ void marginal_weight_merge_kernel(int N, int nchunks, const double* __restrict__ part_m, const double* __restrict__ part_s,
                                                    double* __restrict__ lws) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  lws[i] = marginal_merge_chunks(N, nchunks, i, part_m, part_s);
}

// sum over the 256 lanes' values: a fixed tree (every lane calls it; the result is valid in every lane)
__device__ __forceinline__ double marginal_tree_sum(double v, double* red, int tid) {
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) red[tid] += red[tid + off];
    __syncthreads();
  }
  return red[0];
}

// lws [N] (un-normalised, overwritten) -> logws = lws - log(mass), w_smooth = exp(logws), *mass.  One workgroup of 256.
inline __global__ __launch_bounds__(256) void marginal_normalise_kernel(int N, double* __restrict__ lws, double* __restrict__ w_smooth,
                                                                        double* __restrict__ mass) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (int i = tid; i < N; i += 256) acc += exp(lws[i]);
  const double total = marginal_tree_sum(acc, red, tid);
  const double lm = log(total);
  for (int i = tid; i < N; i += 256) {
    const double l = lws[i];
    const double v = l > -INFINITY ? l - lm : -INFINITY;       // (total = 0: every lws is -inf, and stays)
    lws[i] = v;
    w_smooth[i] = exp(v);
  }
  if (tid == 0) *mass = total;
}

// the last step: logws = log w, w_smooth = w (bit for bit), mass = 1
inline __global__ void marginal_init_kernel(int N, const double* __restrict__ w, double* __restrict__ logws, double* __restrict__ w_smooth,
                                            double* __restrict__ mass) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) *mass = 1.0;
  if (i >= N) return;
  const double wi = w[i];
  logws[i] = wi > 0.0 ? log(wi) : -INFINITY;
  w_smooth[i] = wi;
}

// X [nN][N], w [N] (the smoothed weights of the step) -> mean [nN], cov [nN x nN], *ess.  One workgroup of 256; plain weighted
// moments of all rows (no special handling of angle or quaternion rows).
inline __global__ __launch_bounds__(256) void marginal_moments_kernel(int N, int nN, const double* __restrict__ X, const double* __restrict__ w,
                                                                      double* __restrict__ mean, double* __restrict__ cov, double* __restrict__ ess) {
  constexpr int R = kBackwardMaxRows;
  __shared__ double red[256];
  __shared__ double mu[R];
  const int tid = threadIdx.x;
  double acc[R], w2 = 0.0;
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = 0.0;
  for (int i = tid; i < N; i += 256) {
    const double wi = w[i];
    w2 = fma(wi, wi, w2);
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (r < nN) acc[r] = fma(wi, X[(size_t)r * N + i], acc[r]);
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (r < nN) {                                   // (nN is uniform: every lane takes the same branches)
      const double v = marginal_tree_sum(acc[r], red, tid);
      if (tid == 0) { mu[r] = v; mean[r] = v; }
    }
  }
  w2 = marginal_tree_sum(w2, red, tid);
  if (tid == 0) *ess = 1.0 / w2;
  __syncthreads();
  // the lower triangle, one column b at a time: acc[a] = sum w d_a d_b, a >= b
  for (int b = 0; b < nN; ++b) {
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.0;
    const double mb = mu[b];
    for (int i = tid; i < N; i += 256) {
      const double wd = w[i] * (X[(size_t)b * N + i] - mb);
#pragma unroll
      for (int r = 0; r < R; ++r)
        if (r >= b && r < nN) acc[r] = fma(wd, X[(size_t)r * N + i] - mu[r], acc[r]);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (r >= b && r < nN) {
        const double v = marginal_tree_sum(acc[r], red, tid);
        if (tid == 0) { cov[r + (size_t)nN * b] = v; cov[b + (size_t)nN * r] = v; }
      }
    }
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------
// norm pass + merge (c(j), and D where wanted) + weight pass + merge (lws, un-normalised) of one step, in stream order (the family's
// prologue goes before it); a.part_m / a.part_s hold max(nchunks M, nchunks_w N) doubles each
template <class Term>
hipError_t marginal_launch_step(const MarginalArgs<Term>& a, const double* logws_next, double* D, double* cj, double* lws, hipStream_t s) {
  hipLaunchKernelGGL((marginal_norm_pass_kernel<Term>), dim3((a.M + kBackwardTile - 1) / kBackwardTile, a.nchunks), dim3(kBackwardTile), 0, s, a);
  hipLaunchKernelGGL(marginal_norm_merge_kernel, dim3((a.M + 255) / 256), dim3(256), 0, s, a.M, a.nchunks, a.part_m, a.part_s, logws_next, D, cj);
  hipLaunchKernelGGL((marginal_weight_pass_kernel<Term>), dim3((a.N + kBackwardTile - 1) / kBackwardTile, a.nchunks_w), dim3(kBackwardTile), 0, s, a);
  hipLaunchKernelGGL(marginal_weight_merge_kernel, dim3((a.N + 255) / 256), dim3(256), 0, s, a.N, a.nchunks_w, a.part_m, a.part_s, lws);
  return hipGetLastError();
}

// the sizes of a step into the arguments
template <class Term>
void marginal_set_sizes(MarginalArgs<Term>& a, int N, int M) {
  a.N = N; a.M = M;
  a.C = backward_chunk_size(N, M); a.nchunks = (N + a.C - 1) / a.C;
  a.Cw = backward_chunk_size(M, N); a.nchunks_w = (M + a.Cw - 1) / a.Cw;
}

// doubles in each of part_m and part_s
inline size_t marginal_part_count(size_t N, size_t M) {
  const size_t C = (size_t)backward_chunk_size((int)N, (int)M), Cw = (size_t)backward_chunk_size((int)M, (int)N);
  return std::max((N + C - 1) / C * M, (M + Cw - 1) / Cw * N);
}

inline hipError_t marginal_launch_init(int N, const double* w, double* logws, double* w_smooth, double* mass, hipStream_t s) {
  hipLaunchKernelGGL(marginal_init_kernel, dim3((N + 255) / 256), dim3(256), 0, s, N, w, logws, w_smooth, mass);
  return hipGetLastError();
}

// lws (in place) -> logws, w_smooth, mass
inline hipError_t marginal_launch_normalise(int N, double* lws, double* w_smooth, double* mass, hipStream_t s) {
  hipLaunchKernelGGL(marginal_normalise_kernel, dim3(1), dim3(256), 0, s, N, lws, w_smooth, mass);
  return hipGetLastError();
}

inline hipError_t marginal_launch_moments(int N, int nN, const double* X, const double* w, double* mean, double* cov, double* ess, hipStream_t s) {
  hipLaunchKernelGGL(marginal_moments_kernel, dim3(1), dim3(256), 0, s, N, nN, X, w, mean, cov, ess);
  return hipGetLastError();
}

// The buffers of a marginal pass in a BackwardWorkspace (rbpf_loc_state.hpp, take_marginal): Xhat [rows + 1][N]; pm, ps [nchunks][N]
// the chunk partials of both passes (M = N: the two chunkings agree); u [3][N]: two rows of log w_{.|T} (step t in row t & 1) and
// c; xs = w_smooth [T][N]; mean = mean [T][nN], cov [T][nN][nN], ess [T], mass [T].
struct MarginalOut {
  double *mean, *cov, *ess, *mass;
};

inline MarginalOut marginal_out(const BackwardWorkspace& ws, int nN, int T) {
  MarginalOut o;
  o.mean = ws.mean;
  o.cov = o.mean + (size_t)nN * T;
  o.ess = o.cov + (size_t)nN * nN * T;
  o.mass = o.ess + T;
  return o;
}

inline size_t marginal_bytes(size_t nN, size_t rows, size_t N, size_t T) {
  return ((rows + 1) * N + 2 * marginal_part_count(N, N) + 3 * N + T * N + (nN + nN * nN + 2) * T) * sizeof(double);
}

inline int marginal_take(BackwardWorkspace& ws, DevicePool& pool, int nN, int rows, int N, int T) {
  return ws.take_marginal(pool, (size_t)(rows + 1) * N, marginal_part_count((size_t)N, (size_t)N), (size_t)3 * N, (size_t)T * N,
                          (size_t)(nN + nN * nN + 2) * T);
}

// the last step of a pass (the first thing it enqueues): log w_{T-1}, w_smooth, mass and the moments of step T-1
inline hipError_t marginal_launch_last(const BackwardWorkspace& ws, int nN, int N, int T, const double* X, const double* w, hipStream_t s) {
  const MarginalOut o = marginal_out(ws, nN, T);
  const int t = T - 1;
  double* wsm = ws.xs + (size_t)t * N;
  hipError_t e = marginal_launch_init(N, w + (size_t)t * N, ws.u + (size_t)(t & 1) * N, wsm, o.mass + t, s);
  if (e != hipSuccess) return e;
  return marginal_launch_moments(N, nN, X + (size_t)t * nN * N, wsm, o.mean + (size_t)t * nN, o.cov + (size_t)t * nN * nN, o.ess + t, s);
}

// what follows the passes of step t (lws of the step lies in row t & 1 of ws.u): normalise, moments
inline hipError_t marginal_launch_close_step(const BackwardWorkspace& ws, int nN, int N, int T, int t, const double* X, hipStream_t s) {
  const MarginalOut o = marginal_out(ws, nN, T);
  double* wsm = ws.xs + (size_t)t * N;
  hipError_t e = marginal_launch_normalise(N, ws.u + (size_t)(t & 1) * N, wsm, o.mass + t, s);
  if (e != hipSuccess) return e;
  return marginal_launch_moments(N, nN, X + (size_t)t * nN * N, wsm, o.mean + (size_t)t * nN, o.cov + (size_t)t * nN * nN, o.ess + t, s);
}

// what rbpf_loc_marginal_smooth / rbpf_loc_generic_marginal_finish copy out: w_smooth [N x T], mean [nN x T], cov [nN x nN x T]
// (all column-major), ess [T], mass [T]
inline int marginal_copy_out(const BackwardWorkspace& ws, int nN, int N, int T, double* w_smooth, double* mean, double* cov, double* ess,
                             double* mass) {
  const MarginalOut o = marginal_out(ws, nN, T);
  if (w_smooth) HIPCHK(hipMemcpy(w_smooth, ws.xs, (size_t)N * T * sizeof(double), hipMemcpyDeviceToHost));
  if (mean) HIPCHK(hipMemcpy(mean, o.mean, (size_t)nN * T * sizeof(double), hipMemcpyDeviceToHost));
  if (cov) HIPCHK(hipMemcpy(cov, o.cov, (size_t)nN * nN * T * sizeof(double), hipMemcpyDeviceToHost));
  if (ess) HIPCHK(hipMemcpy(ess, o.ess, (size_t)T * sizeof(double), hipMemcpyDeviceToHost));
  if (mass) HIPCHK(hipMemcpy(mass, o.mass, (size_t)T * sizeof(double), hipMemcpyDeviceToHost));
  return RBPF_OK;
}

}  // namespace rbpf
