// sparseFeatures = true branch of the reference (src/particleFilter.m:127-137,165-181) for ARBITRARY models whose handles are
// device code (RBPF_MODEL_GENERIC_SPARSE): the caller's measModel has already been evaluated for every particle at the
// particle's own map, [yhat, dy] = measModel(xn_i, xl_i), and this file does the rest of the EKF step -- innovation of the
// observed outputs, S, its Cholesky factor with the one jitter retry, the weight, and the update of mean and covariance.
//
// dy is dense: nothing is assumed about its non-zeros.  At the largest admitted shape (nLin = 96, n_y = 32) a particle costs
// about 1.6 Mflop and moves its covariance in and out (2 x 73.7 KB) plus 24.6 KB of Jacobian, so the step is one workgroup of
// four waves per particle with the covariance resident in LDS:
//
//   PH = P H'                 n x n x n_o, 4 x 4 register tiles, lanes along the rows of P (odd LDS row strides: no bank conflicts)
//   SS = H PH + R(ind, ind)   lower triangle
//   [cS; v'; W] = [SS; e'; PH] / cS'   ONE left-looking column sweep over the stacked rows, a thread per row and a barrier per
//                             column: the rows of SS give chol(SS), the row e gives v = cS \ e (particleFilter.m:149), the rows
//                             of PH give W = PH / cS'
//   logw = -sum(log(diag(cS))) - v'v / 2 - n_o log(2 pi) / 2                                                          (:150)
//   xl + W v,  P - W W'       = xl + K e, P - K SS K' of :181,197-198 with K = W / cS: the gain itself is formed after a jitter
//                             retry only, where :198 keeps the un-jittered SS and K SS K' = W W' - jitter K K'
//
// Vector loads and stores only; every sum runs in a fixed order, so results do not depend on the launch.
#include "../../include/rbpf.h"
#include "rbpf_internal.hpp"
#include "rbpf_sparse.hpp"

namespace rbpf {

constexpr int kSxThreads = 256;
constexpr int kSxMaxNy = 32;        // observed-output mask: one ballot of a wave's low lanes
constexpr int kSxMaxNLin = 96;      // n_y + 1 + nLin rows of the column sweep <= kSxThreads, and the LDS plan below

size_t sparse_ext_step_lds_bytes(int n, int d) {
  const size_t ldp = (size_t)n | 1, ldw = (size_t)d | 1;
  return ((size_t)n * ldp + (size_t)d * ldp + (size_t)n * ldw + ((size_t)d + 1) * ldw + (size_t)n + 2 * (size_t)d) * sizeof(double) +
         (size_t)d * sizeof(int);
}

// rows rq, rq + Q, rq + 2Q, rq + 3Q of a 4-row register tile, clamped into [0, lim): a clamped row is computed and not stored
__device__ __forceinline__ void tile4(int q, int Q, int lim, int (&r)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) r[i] = min(q + i * Q, lim - 1);
}

// Ps -= scale * V V' for V [n][ldw] with `no` columns: 4 x 4 register tiles, lanes along the columns of Ps.  Element (r, c) and its
// mirror image add the same products in the same order, so a symmetric Ps stays symmetric bit for bit.
__device__ __forceinline__ void sx_rank_update(double* Ps, const double* V, int n, int no, int ldp, int ldw, double scale, int tid) {
  const int RQ = (n + 3) >> 2;
  for (int item = tid; item < RQ * RQ; item += kSxThreads) {
    const int cq = item % RQ, rq = item / RQ;
    int r[4], c[4];
    tile4(rq, RQ, n, r);
    tile4(cq, RQ, n, c);
    double acc[4][4] = {};
#pragma unroll 4
    for (int b = 0; b < no; ++b) {
      double rv[4], cv[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) { rv[k] = V[r[k] * ldw + b]; cv[k] = V[c[k] * ldw + b]; }
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[k][j] = fma(rv[k], cv[j], acc[k][j]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (rq + k * RQ < n && cq + j * RQ < n) Ps[(rq + k * RQ) * ldp + cq + j * RQ] -= scale * acc[k][j];
  }
}

__global__ __launch_bounds__(kSxThreads, 1) void sparse_ext_step_kernel(const SparseExtStepArgs a) {
  extern __shared__ double sm[];
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int n = a.n, d = a.d, ldb = a.ldb;
  const int ldp = n | 1, ldw = d | 1;
  double* Ps = sm;                              // [n][ldp]    P, downdated in place
  double* Hs = Ps + (size_t)n * ldp;            // [d][ldp]    dy(ind,:), observed rows only
  double* W = Hs + (size_t)d * ldp;             // [n][ldw]    P dy(ind,:)', then W
  double* cS = W + (size_t)n * ldw;             // [d + 1][ldw] SS (lower), then chol(SS) below the diagonal; row n_o: e, then v
  double* xls = cS + (size_t)(d + 1) * ldw;     // [n]
  double* ev = xls + n;                         // [d] innovation of the observed outputs
  double* dg = ev + d;                          // [d] diag(cS)
  int* obs = reinterpret_cast<int*>(dg + d);    // [d] observed outputs, ascending

  // ind = ~isnan(y_t)  (:134), the same in every wave
  const bool seen = lane < d && !isnan(a.y[lane]);
  const unsigned long long mask = __ballot(seen);
  const int no = __popcll(mask);
  if (tid < 64 && seen) obs[__popcll(mask & ((1ull << lane) - 1ull))] = lane;

  const int anc = a.ai ? min(max(a.ai[i], 0), a.N - 1) : i;
  const double* P_src = a.Pb_old + (size_t)anc * a.Pb_old_stride;
  const double* xl_src = a.xl_g + (size_t)i * a.ldx;
  for (int q = tid; q < n; q += kSxThreads) xls[q] = xl_src[q];
  {
    const int half = ldb >> 1;                  // ldb is even: 16 bytes per lane, both elements in one row
    const double2* P2 = reinterpret_cast<const double2*>(P_src);
    for (int q = tid; q < n * half; q += kSxThreads) {
      const int r = q / half, c = 2 * (q - r * half);
      const double2 v = P2[q];
      Ps[r * ldp + c] = v.x;
      if (c + 1 < n) Ps[r * ldp + c + 1] = v.y;
    }
  }
  __syncthreads();

  bool ok = no > 0;
  double jit_used = 0.0;
  if (no > 0) {
    const double* dy_i = a.dy + (size_t)i * a.dy_sp;
    for (int q = tid; q < no * n; q += kSxThreads) {
      const int b = q / n, c = q - b * n;
      Hs[b * ldp + c] = dy_i[(size_t)obs[b] * a.dy_sr + c];
    }
    if (tid < no) ev[tid] = a.y[obs[tid]] - a.yhat[(size_t)i * a.yhat_si + (size_t)obs[tid] * a.yhat_sk];     // :131,135
    const int RQ = (n + 3) >> 2, BT = (no + 3) >> 2;
    // my row of the column sweep: SS rows (active from their diagonal on), the innovation, the rows of P dy'
    double* row = tid < no ? cS + (size_t)tid * ldw : tid == no ? cS + (size_t)no * ldw : W + (size_t)min(tid - no - 1, n - 1) * ldw;
    const bool has_row = tid <= no + n;
    for (int attempt = 0; attempt < 2; ++attempt) {                                      // :145-148
      const double jit = attempt ? a.jitter : 0.0;
      __syncthreads();
      for (int item = tid; item < RQ * BT; item += kSxThreads) {                         // P * dy(ind,:)'
        const int rq = item % RQ, b0 = (item / RQ) * 4;
        int r[4], b[4];
        tile4(rq, RQ, n, r);
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = min(b0 + j, no - 1);
        double acc[4][4] = {};
#pragma unroll 4
        for (int c = 0; c < n; ++c) {                    // (unrolled: one wave per SIMD, the LDS reads of four columns in flight)
          double pv[4], hv[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) { pv[k] = Ps[r[k] * ldp + c]; hv[k] = Hs[b[k] * ldp + c]; }
#pragma unroll
          for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[k][j] = fma(pv[k], hv[j], acc[k][j]);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (rq + k * RQ < n && b0 + j < no) W[(rq + k * RQ) * ldw + b0 + j] = acc[k][j];
      }
      __syncthreads();
      for (int q = tid; q < no * no; q += kSxThreads) {                                  // SS = dy*P*dy' + R, observed part (:132,136)
        const int aa = q / no, bb = q - aa * no;
        if (bb > aa) continue;
        double s = 0.0;
#pragma unroll 8
        for (int c = 0; c < n; ++c) s = fma(Hs[aa * ldp + c], W[c * ldw + bb], s);
        s += a.R[obs[aa] + (size_t)d * obs[bb]];
        cS[aa * ldw + bb] = (aa == bb) ? s + jit : s;
      }
      if (tid < no) cS[no * ldw + tid] = ev[tid];
      __syncthreads();
      ok = true;
      for (int j = 0; j < no; ++j) {
        // every thread forms the pivot itself (row j is final below its diagonal), so the verdict is uniform and one
        // barrier per column is enough; the diagonal of cS keeps SS(j,j), sqrt of the pivot goes to dg
        const double* Lj = cS + (size_t)j * ldw;
        const bool active = has_row && (tid >= no || tid >= j);
        double s = Lj[j], v = active ? row[j] : 0.0;
#pragma unroll 4
        for (int k = 0; k < j; ++k) {
          const double ljk = Lj[k];
          s -= ljk * ljk;
          if (active) v -= row[k] * ljk;
        }
        if (!(s > 0.0)) { ok = false; break; }
        const double ljj = sqrt(s);
        if (tid == j) dg[j] = ljj;
        else if (active) row[j] = v / ljj;
        __syncthreads();
      }
      if (ok) { jit_used = jit; break; }
    }
    if (tid == 0) {
      double lw;
      if (ok) {
        double sl = 0.0, q2 = 0.0;
        for (int r = 0; r < no; ++r) { const double v = cS[no * ldw + r]; sl += log(dg[r]); q2 += v * v; }
        lw = -sl - 0.5 * q2 - 0.5 * (double)no * 1.8378770664093453;                    // :150
      } else {
        atomicOr(a.status, 1);
        lw = nan("");
      }
      a.logw[i] = lw;
    }
  } else if (tid == 0) {
    a.logw[i] = 0.0;                            // nothing observed: empty innovation (:134-136)
  }

  if (ok) {                                     // uniform: else the gathered state and covariance pass through unchanged
    const double* vv = cS + (size_t)no * ldw;
    for (int r = tid; r < n; r += kSxThreads) {                                          // xl + K*e  (:197)
      double s = xls[r];
#pragma unroll 4
      for (int b = 0; b < no; ++b) s = fma(W[r * ldw + b], vv[b], s);
      xls[r] = s;
    }
    sx_rank_update(Ps, W, n, no, ldp, ldw, 1.0, tid);                                    // P - K*SS*K'  (:198) = P - W W' ...
    if (jit_used != 0.0) {
      // ... after a retry K = W / cS comes from chol(SS + jitter I) while :198 keeps the un-jittered SS:
      // K SS K' = W W' - jitter K K'.  The rare path: W becomes K in place, row by row, then one more update.
      __syncthreads();
      for (int r = tid; r < n; r += kSxThreads) {
        double* k = W + (size_t)r * ldw;
        for (int b2 = no - 1; b2 >= 0; --b2) {
          double v = k[b2];
          for (int q = b2 + 1; q < no; ++q) v -= cS[q * ldw + b2] * k[q];
          k[b2] = v / dg[b2];
        }
      }
      __syncthreads();
      sx_rank_update(Ps, W, n, no, ldp, ldw, -jit_used, tid);
    }
  }
  __syncthreads();
  double* xl_dst = a.xl_new + (size_t)i * a.ldx;
  for (int q = tid; q < a.ldx; q += kSxThreads) xl_dst[q] = q < n ? xls[q] : 0.0;
  {
    const int half = ldb >> 1;
    double2* P2 = reinterpret_cast<double2*>(a.Pb_new + (size_t)i * a.szB);
    for (int q = tid; q < n * half; q += kSxThreads) {
      const int r = q / half, c = 2 * (q - r * half);
      P2[q] = make_double2(Ps[r * ldp + c], c + 1 < n ? Ps[r * ldp + c + 1] : 0.0);
    }
  }
}

hipError_t launch_sparse_ext_step(const SparseExtStepArgs& a, hipStream_t s) {
  if (a.d < 1 || a.d > kSxMaxNy || a.n < 1 || a.n > kSxMaxNLin || (a.ldb & 1) || a.ldb < a.n || a.ldx < a.n) return hipErrorInvalidValue;
  const size_t lds = sparse_ext_step_lds_bytes(a.n, a.d);
  if (lds > 150 * 1024) return hipErrorInvalidValue;
  static std::atomic<uint64_t> attr{0};
  if (hipError_t e = lds_opt_in(reinterpret_cast<const void*>(&sparse_ext_step_kernel), 150 * 1024, attr)) return e;
  hipLaunchKernelGGL(sparse_ext_step_kernel, dim3(a.N), dim3(kSxThreads), lds, s, a);
  return hipGetLastError();
}

// xl(:,ai) of the step about to run (particleFilter.m:112) -> out [N][ldx]; ai == nullptr: slot i reads column i (stride ldx) or
// the one shared column (stride 0) of the initial states
__global__ void sparse_ext_gather_xl_kernel(int N, int ldx, const double* __restrict__ src, size_t src_stride,
                                            const int* __restrict__ ai, double* __restrict__ out) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (size_t)N * ldx) return;
  const int i = (int)(e / ldx), q = (int)(e - (size_t)i * ldx);
  const int anc = ai ? min(max(ai[i], 0), N - 1) : i;
  out[e] = src[(size_t)anc * src_stride + q];
}

hipError_t launch_sparse_ext_gather_xl(int N, int ldx, const double* src, size_t src_stride, const int* ai, double* out, hipStream_t s) {
  const size_t total = (size_t)N * ldx;
  hipLaunchKernelGGL(sparse_ext_gather_xl_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, N, ldx, src, src_stride, ai, out);
  return hipGetLastError();
}

// yhattraj(:,t) = yhat of the maximum-weight particle (particleFilter.m:201-203); iw_max is the normalisation kernel's
__global__ void sparse_ext_yhat_of_max_kernel(int d, const double* __restrict__ yhat, size_t si, size_t sk, const int* __restrict__ iw_max,
                                              double* __restrict__ out) {
  const int k = threadIdx.x;
  if (k < d) out[k] = yhat[(size_t)iw_max[0] * si + (size_t)k * sk];
}

hipError_t launch_sparse_ext_yhat_of_max(int d, const double* yhat, size_t si, size_t sk, const int* iw_max, double* out, hipStream_t s) {
  hipLaunchKernelGGL(sparse_ext_yhat_of_max_kernel, dim3(1), dim3(64), 0, s, d, yhat, si, sk, iw_max, out);
  return hipGetLastError();
}

}  // namespace rbpf
