// Rejection-sampling backward simulation for the localisation smoothers, once for every map (Douc, Garivier, Moulines & Olsson
// 2011; with the all-pairs pass as the fallback: Taghavi et al. 2013, Bunch & Godsill 2013).  The recursion of
// rbpf_loc_backward.hpp draws b[t][j] from p_i ~ w[t][i] exp(logp(xs[t+1][j] | X[t][:, i])) by an all-pairs pass.  Every term of
// this project has logp = -z'z / 2 <= 0, a bound that is attained, so the same law comes from
//     r = 0 .. R-1:  (u0, u1) = philox_uniform2(seed, slot = j, step = t, lane = 0x42530001, iter = r)
//                    i = #{k : cdf_k < u0 cdf_{N-1}},  cdf the inclusive prefix sums of w[t]            (proposal: the weights)
//                    accept iff logp(xs[t+1][j] | X[t][:, i]) >= log u1                                  (logp WITHOUT log w_i)
// the first accepted i being b[t][j]; a trajectory without an acceptance after R = max_tries tries is drawn by the all-pairs pass
// and locate kernel of rbpf_loc_backward.hpp with its uniform u[t][j] (lane 0x42530000, iter 0), an independent exact draw, so the
// law of every index is the backward kernel's for every R.  Step T-1 is the draw of rbpf_loc_backward.hpp.  R = 0 is that header's
// method bit for bit: the counters of u[t][j] and the sizes of the pass are the same.
//
// Kernels of one step t < T-1 after the family's prologue (all in stream order):
//   reject_cdf_local_kernel      first level of the cdf: blocks of 1024 weights, a lane owns 16 in a row, the 64 lane totals are
//   reject_cdf_offset_kernel     summed in lane order; second level: the block totals in block order.  CDF ORDER below.
//   reject_tries_kernel<Term>    a lane per trajectory, its NS rows in registers; per try: two uniforms, a binary search of the cdf
//                                (N doubles), the NS rows of the proposed particle from Xhat (no log w row), the term with
//                                bound = log u1.  No LDS, no cross-lane operation; a wave runs as long as its slowest lane.
//   reject_count_kernel,         compaction: flags (no acceptance) counted per block of 256 trajectories, the block counts scanned by
//   reject_offsets_kernel,       one workgroup (M' and the step's tries go to the counters), the flagged trajectories' successors and
//   reject_gather_kernel         uniforms gathered into M' rows in ascending j.
//   (M' is read back, 4 bytes)   then backward_pass_kernel / backward_locate_kernel on the M' rows with C = backward_chunk_size(N, M'):
//                                the SUMMATION ORDER of rbpf_loc_backward.hpp for those two sizes.  M' = 0 launches neither.
//   reject_commit_kernel<Term>   index[j] = the accepted particle, or the fallback's index of row pos[j]; term.gather.
//
// CDF ORDER (fixed by N alone): inside a lane's 16 weights left to right; lane totals left to right over the 64 lanes of a block;
// block totals left to right.  cdf_i = offset of the block + (offset of the lane + the lane's running sum).  A
// weight of 0 repeats its predecessor's cdf exactly, also across lanes and blocks, so such a particle is never proposed.
#pragma once
#include "rbpf_loc_backward.hpp"

namespace rbpf {

constexpr uint32_t kRejectPhiloxLane = 0x42530001u;
constexpr int kRejectMaxTries = 1 << 22;          // 256 trajectories' tries fit an int (reject_count_kernel)
constexpr int kRejectCdfBlock = 1024, kRejectCdfLane = 16;   // weights per block and per lane of the cdf's first level (64 lanes)

// doubles of each of part_m / part_s that the fallback pass may need: the largest nchunks(N, M') M' over M' <= M (a smaller M' has
// fewer trajectory blocks and so smaller chunks: more of them)
inline size_t reject_part_count(int N, int M) {
  size_t best = 0;
  for (int bx = 1; bx <= (M + kBackwardTile - 1) / kBackwardTile; ++bx) {
    const int Mp = std::min(M, bx * kBackwardTile);
    const int C = backward_chunk_size(N, Mp);
    best = std::max(best, (size_t)((N + C - 1) / C) * Mp);
  }
  return best;
}

inline size_t reject_cdf_blocks(int N) { return (size_t)(N + kRejectCdfBlock - 1) / kRejectCdfBlock; }

// bytes of a RejectWorkspace (rbpf_loc_state.hpp)
inline size_t reject_bytes(size_t N, size_t M, size_t rows, size_t T) {
  const size_t B = (M + kBackwardTile - 1) / kBackwardTile;
  return (N + reject_cdf_blocks((int)N) + M * rows + M) * sizeof(double) + (4 * M + B + T) * sizeof(int) + (B + T) * sizeof(long long);
}

inline __global__ __launch_bounds__(64) void reject_cdf_local_kernel(int N, const double* __restrict__ w, double* __restrict__ cdf, double* __restrict__ btot) {
  __shared__ double tot[64];
  const int tid = threadIdx.x;
  const int i0 = blockIdx.x * kRejectCdfBlock + tid * kRejectCdfLane;
  double run[kRejectCdfLane];
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < kRejectCdfLane; ++k) {
    s += (i0 + k < N) ? w[i0 + k] : 0.0;
    run[k] = s;
  }
  tot[tid] = s;
  __syncthreads();
  if (tid == 0) {
    double off = 0.0;
    for (int l = 0; l < 64; ++l) { const double v = tot[l]; tot[l] = off; off += v; }
    btot[blockIdx.x] = off;
  }
  __syncthreads();
  const double off = tot[tid];
#pragma unroll
  for (int k = 0; k < kRejectCdfLane; ++k)
    if (i0 + k < N) cdf[i0 + k] = off + run[k];
}

inline __global__ __launch_bounds__(64) void reject_cdf_offset_kernel(int N, const double* __restrict__ btot, double* __restrict__ cdf) {
  __shared__ double boff;
  const int tid = threadIdx.x;
  if (tid == 0) {
    double off = 0.0;
    for (int b = 0; b < (int)blockIdx.x; ++b) off += btot[b];
    boff = off;
  }
  __syncthreads();
  const double off = boff;
  for (int i = blockIdx.x * kRejectCdfBlock + tid; i < min(N, ((int)blockIdx.x + 1) * kRejectCdfBlock); i += 64) cdf[i] = off + cdf[i];
}

template <class Term>
struct RejectArgs {
  int N, M, R, step;
  typename Term::Head head;
  const double* Xhat;              // [NS + 1][N]; the log w row is not read
  const double* cdf;               // [N]
  const double* xs_next;           // [M][rows]
  const double* u_try;             // [R][M][2]: the probes' uniforms; null: the Philox draws of `seed`
  unsigned long long seed;
  int* acc; int* tries;            // [M]
  Term term;
};

template <class Term>
__global__ __launch_bounds__(kBackwardTile) void reject_tries_kernel(const RejectArgs<Term> a) {
  constexpr int NS = Term::NS;
  const int j = blockIdx.x * kBackwardTile + threadIdx.x;
  if (j >= a.M) return;
  double x[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) x[k] = a.term.load_x(a.head, a.xs_next, j, k);
  const double total = a.cdf[a.N - 1];
  int idx = -1, r = 0;
  while (r < a.R) {
    double u0, u1;
    if (a.u_try) {
      u0 = a.u_try[((size_t)r * a.M + j) * 2];
      u1 = a.u_try[((size_t)r * a.M + j) * 2 + 1];
    } else {
      philox_uniform2(a.seed, (uint32_t)j, (uint32_t)a.step, kRejectPhiloxLane, (uint32_t)r, u0, u1);
    }
    ++r;
    const double target = u0 * total;
    int lo = 0, hi = a.N - 1;                    // the first i with cdf_i >= target (a target past the last edge: N - 1)
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (a.cdf[mid] < target) lo = mid + 1;
      else hi = mid;
    }
    double h[NS + 1];
#pragma unroll
    for (int k = 0; k < NS; ++k) h[k] = a.Xhat[(size_t)k * a.N + lo];
    h[NS] = 0.0;
    const double bound = log(u1);
    double l = 0.0;
    bool ok;
    if constexpr (Term::kSplit) {
      l = a.term.pair_near(a.head, h, x);
      ok = l >= bound;
      if (ok) {
        l += a.term.pair_far(a.head, h, x);
        ok = l >= bound;
      }
    } else {
      ok = a.term.pair(a.head, h, x, bound, l) && l >= bound;
    }
    if (ok) { idx = lo; break; }
  }
  a.acc[j] = idx;
  a.tries[j] = r;
}

// Compaction, in three launches.  Blocks of 256 trajectories: the count of those without an acceptance and the tries of each block;
// one workgroup turns the block counts into offsets (thread k owns the blocks [k L, (k + 1) L), L = ceil(blocks / 1024)) and writes
// the step's two counters; then every block scans its own flags and gathers its rows behind its offset, ascending j throughout.
// Integer sums: any order gives the same result.
inline __global__ __launch_bounds__(kBackwardTile) void reject_count_kernel(int M, const int* __restrict__ acc, const int* __restrict__ tries,
                                                                           int* __restrict__ bcnt, long long* __restrict__ btries) {
  __shared__ int cnt[kBackwardTile];
  __shared__ int trs[kBackwardTile];                // 256 trajectories of at most kRejectMaxTries tries each fit an int
  const int tid = threadIdx.x;
  const int j = blockIdx.x * kBackwardTile + tid;
  cnt[tid] = j < M ? (acc[j] < 0) : 0;
  trs[tid] = j < M ? tries[j] : 0;
  __syncthreads();
  for (int off = kBackwardTile / 2; off > 0; off >>= 1) {
    if (tid < off) { cnt[tid] += cnt[tid + off]; trs[tid] += trs[tid + off]; }
    __syncthreads();
  }
  if (tid == 0) { bcnt[blockIdx.x] = cnt[0]; btries[blockIdx.x] = trs[0]; }
}

inline __global__ __launch_bounds__(1024) void reject_offsets_kernel(int B, int* __restrict__ bcnt, const long long* __restrict__ btries,
                                                                     int* __restrict__ n_fb, long long* __restrict__ n_tries) {
  __shared__ int cnt[1024];
  __shared__ long long trs[1024];
  const int tid = threadIdx.x;
  const int L = (B + 1023) / 1024;
  const int b0 = min(B, tid * L), b1 = min(B, b0 + L);
  int c = 0;
  long long s = 0;
  for (int b = b0; b < b1; ++b) { c += bcnt[b]; s += btries[b]; }
  cnt[tid] = c;
  trs[tid] = s;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int vc = tid >= off ? cnt[tid - off] : 0;
    const long long vs = tid >= off ? trs[tid - off] : 0;
    __syncthreads();
    cnt[tid] += vc;
    trs[tid] += vs;
    __syncthreads();
  }
  int p = cnt[tid] - c;
  for (int b = b0; b < b1; ++b) { const int v = bcnt[b]; bcnt[b] = p; p += v; }   // counts -> exclusive offsets, in place
  if (tid == 1023) {
    *n_fb = cnt[1023];
    *n_tries = trs[1023];
  }
}

inline __global__ __launch_bounds__(kBackwardTile) void reject_gather_kernel(int M, int nN, const int* __restrict__ acc, const int* __restrict__ boff,
                                                                            const double* __restrict__ xs_next, const double* __restrict__ u,
                                                                            int* __restrict__ pos, double* __restrict__ xs_c, double* __restrict__ u_c) {
  __shared__ int cnt[kBackwardTile];
  const int tid = threadIdx.x;
  const int j = blockIdx.x * kBackwardTile + tid;
  const int flag = j < M ? (acc[j] < 0) : 0;
  cnt[tid] = flag;
  __syncthreads();
  for (int off = 1; off < kBackwardTile; off <<= 1) {
    const int v = tid >= off ? cnt[tid - off] : 0;
    __syncthreads();
    cnt[tid] += v;
    __syncthreads();
  }
  if (j >= M) return;
  if (!flag) { pos[j] = -1; return; }
  const int p = boff[blockIdx.x] + cnt[tid] - 1;
  pos[j] = p;
  u_c[p] = u[j];
  for (int r = 0; r < nN; ++r) xs_c[(size_t)p * nN + r] = xs_next[(size_t)j * nN + r];
}

// a: the step's arguments over all M trajectories (index, xs, X, head, term)
template <class Term>
__global__ void reject_commit_kernel(const BackwardArgs<Term> a, const int* __restrict__ acc, const int* __restrict__ pos, const int* __restrict__ fb) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.M) return;
  const int got = acc[j];
  const int idx = got >= 0 ? got : fb[pos[j]];
  a.index[j] = idx;
  if (a.xs) a.term.gather(a.head, a.X, a.N, idx, a.xs, j);
}

// ---- host side -----------------------------------------------------------------------------------------------------------
inline hipError_t reject_launch_cdf(int N, const double* w, double* cdf, double* btot, hipStream_t s) {
  const unsigned B = (unsigned)reject_cdf_blocks(N);
  hipLaunchKernelGGL(reject_cdf_local_kernel, dim3(B), dim3(64), 0, s, N, w, cdf, btot);
  hipLaunchKernelGGL(reject_cdf_offset_kernel, dim3(B), dim3(64), 0, s, N, btot, cdf);
  return hipGetLastError();
}

// One step t < T-1 after the family's prologue.  a: the arguments of the all-pairs step over all M trajectories (nothing of it is
// launched at that size unless every trajectory falls back); w: the step's weights; rows: the rows of a state in xs_next;
// u_try: the probes' uniforms or null (then seed and step key the Philox draws); n_fb, n_tries: the step's two counters (device).
// Waits for the stream once, for M'.
template <class Term>
hipError_t reject_launch_step(const BackwardArgs<Term>& a, const RejectWorkspace& rw, const double* w, int rows, int max_tries, const double* u_try,
                              unsigned long long seed, int step, int* n_fb, long long* n_tries, hipStream_t s) {
  hipError_t e = reject_launch_cdf(a.N, w, rw.cdf, rw.btot, s);
  if (e != hipSuccess) return e;
  RejectArgs<Term> q{a.N, a.M, max_tries, step, a.head, a.Xhat, rw.cdf, a.xs_next, u_try, seed, rw.acc, rw.tries, a.term};
  hipLaunchKernelGGL((reject_tries_kernel<Term>), dim3((a.M + kBackwardTile - 1) / kBackwardTile), dim3(kBackwardTile), 0, s, q);
  const int B = (a.M + kBackwardTile - 1) / kBackwardTile;
  hipLaunchKernelGGL(reject_count_kernel, dim3(B), dim3(kBackwardTile), 0, s, a.M, rw.acc, rw.tries, rw.bcnt, rw.btries);
  hipLaunchKernelGGL(reject_offsets_kernel, dim3(1), dim3(1024), 0, s, B, rw.bcnt, rw.btries, n_fb, n_tries);
  hipLaunchKernelGGL(reject_gather_kernel, dim3(B), dim3(kBackwardTile), 0, s, a.M, rows, rw.acc, rw.bcnt, a.xs_next, a.u, rw.pos, rw.xs_c, rw.u_c);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  int Mp = 0;
  if ((e = hipMemcpyAsync(&Mp, n_fb, sizeof(int), hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
  if (Mp < 0 || Mp > a.M) return hipErrorUnknown;
  if (Mp > 0) {
    BackwardArgs<Term> b = a;
    b.M = Mp; b.C = backward_chunk_size(a.N, Mp); b.nchunks = (a.N + b.C - 1) / b.C;
    b.xs_next = rw.xs_c; b.u = rw.u_c; b.index = rw.fb; b.xs = nullptr;
    if ((e = backward_launch_step(b, s)) != hipSuccess) return e;
  }
  hipLaunchKernelGGL((reject_commit_kernel<Term>), dim3((a.M + 255) / 256), dim3(256), 0, s, a, rw.acc, rw.pos, rw.fb);
  return hipGetLastError();
}

}  // namespace rbpf
