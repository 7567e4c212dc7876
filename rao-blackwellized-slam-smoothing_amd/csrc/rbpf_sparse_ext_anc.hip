// Ancestor weights of the reference trajectory, sparseFeatures = true branch (src/particleSmoother.m:194-217), for ARBITRARY
// models whose handles are device code (RBPF_MODEL_GENERIC_SPARSE, rbpf_particle_smoother_sparse_device).  Particle i stacks
// the future observations -- the observed outputs of the times ti = t .. N_T-1, time-major, outputs ascending within a time --
// linearised at its own map of generation t - 1:
//     [yhat, dy] = measModel(xnk(:,ti), xl(:,i))                 (:206)   the caller's handle, batched over F N_P columns
//     e = (y(ti,:) - yhat)(ind),  D_i = dy(ind,:) stacked        (:207-210)
//     S_i = D_i P_i D_i' + blkdiag(R(ind,ind))                   (:211,215)
// and S_i, e go to the batched Cholesky of rbpf_smoother.hip (launch_chol mode 0, R == nullptr).  Three kernels:
//   replicate  the handle's operands of a chunk of F future times in device memory: column f N_P + i carries xnk(:,ti_f) and
//              the map of particle i
//   pack       the observed rows of the chunk's dy (any of the three layouts) -> D [N_P][M][n], y - yhat -> rhs [N_P][M]
//   build      S_i from D_i and P_i.  D is dense and differs per particle, so this is 2 M n (n + M / 2) flops a particle
//              against the M^3 / 3 of the factorisation behind it: one workgroup per particle, P_i resident in LDS on an odd row
//              stride (n = 96: 96 x 97 doubles = 74.5 KB), D_i streamed in 16-row tiles -- G = D_tile P into LDS, then the
//              tiles S[tile, ct <= tile] = G D(ct)' -- both products on the fp64 matrix cores (v_mfma_f64_16x16x4_f64:
//              A[l & 15][k = l >> 4], B[k = l >> 4][l & 15], result column l & 15, row (l >> 4) + 4 reg).  The factorisation
//              reads the 16 x 16 tiles on and below the diagonal only (chol_aug_elems, c64_diag_elems_fast, c64_strip_fast: loads of
//              other elements are masked by a select), so nothing above them is computed or written.
// Edges are zero-padded: M and n are arbitrary.  Every sum runs in a fixed order, so results do not depend on the chunking.
// Vector loads and stores only.
#include "../../include/rbpf.h"
#include "rbpf_internal.hpp"
#include "rbpf_sparse.hpp"

#include <algorithm>

namespace rbpf {

constexpr int kSbThreads = 256;          // four waves: one per SIMD
typedef double sb_v4d __attribute__((ext_vector_type(4)));

// ---- replicate ---------------------------------------------------------------------------------------------------------
// xn [nN x F N] column-major and xl [F N][ldx] of a chunk: times[f] the chunk's future times, xnk [T][nN], xl_bank [N][ldx]
__global__ void sparse_ext_replicate_kernel(int N, int F, int nN, int ldx, const int* __restrict__ times, const double* __restrict__ xnk,
                                            const double* __restrict__ xl_bank, double* __restrict__ xn, double* __restrict__ xl) {
  const size_t per = (size_t)N * ldx, total = (size_t)F * per, stride = (size_t)gridDim.x * blockDim.x;
  const size_t e0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (size_t e = e0; e < total; e += stride) xl[e] = xl_bank[e % per];
  const size_t pern = (size_t)N * nN;
  for (size_t e = e0; e < (size_t)F * pern; e += stride) xn[e] = xnk[(size_t)times[e / pern] * nN + e % nN];
}

hipError_t launch_sparse_ext_replicate(int N, int F, int nN, int ldx, const int* times, const double* xnk, const double* xl_bank,
                                       double* xn, double* xl, hipStream_t s) {
  const size_t total = (size_t)F * N * std::max(ldx, nN);
  const unsigned blocks = (unsigned)std::min<size_t>((total + 255) / 256, 65535u * 16u);
  hipLaunchKernelGGL(sparse_ext_replicate_kernel, dim3(blocks), dim3(256), 0, s, N, F, nN, ldx, times, xnk, xl_bank, xn, xl);
  return hipGetLastError();
}

// ---- pack --------------------------------------------------------------------------------------------------------------
// pairs [m0, m0 + Mc) of the step's M stacked observations are those of the chunk's F times (slot0: index of the chunk's first
// time in the table of observed times, time_slot[ti]: index of time ti in it).  Column col = f N + i of the handle's C = F N.
__global__ void sparse_ext_pack_kernel(SparseExtPackArgs a) {
  const size_t total = (size_t)a.N * a.Mc * a.n;
  const size_t C = (size_t)a.F * a.N;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(e % a.n);
    const size_t r = e / a.n;
    const int ml = (int)(r % a.Mc), i = (int)(r / a.Mc);
    const int ti = a.pair_t[a.m0 + ml], j = a.pair_j[a.m0 + ml];
    const size_t col = (size_t)(a.time_slot[ti] - a.slot0) * a.N + i;
    const size_t src = a.dy_layout == 0 ? col + C * ((size_t)j + (size_t)a.d * c) : (col * a.d + j) * (size_t)a.dy_ld + c;
    a.D[((size_t)i * a.M + a.m0 + ml) * a.n + c] = a.dy[src];
    if (c == 0) {
      const double yh = a.yhat[a.yhat_layout == 0 ? col + C * (size_t)j : col * a.d + j];
      a.rhs[(size_t)i * a.M + a.m0 + ml] = a.y[(size_t)ti * a.d + j] - yh;               // :207-208
    }
  }
}

hipError_t launch_sparse_ext_pack(const SparseExtPackArgs& a, hipStream_t s) {
  if (a.Mc <= 0) return hipSuccess;
  const size_t total = (size_t)a.N * a.Mc * a.n;
  const unsigned blocks = (unsigned)std::min<size_t>((total + 255) / 256, 65535u * 16u);
  hipLaunchKernelGGL(sparse_ext_pack_kernel, dim3(blocks), dim3(256), 0, s, a);
  return hipGetLastError();
}

// ---- build -------------------------------------------------------------------------------------------------------------
static __host__ __device__ inline int sb_np4(int n) { return (n + 3) & ~3; }
static __host__ __device__ inline int sb_n16(int n) { return (n + 15) & ~15; }

size_t sparse_ext_build_lds_bytes(int n, int M) {
  const size_t np4 = sb_np4(n), ldp = (size_t)sb_n16(n) + 1, ldd = np4 | 1, Mp = (size_t)(M + 15) & ~(size_t)15;
  return (np4 * ldp + 2 * 16 * ldd) * sizeof(double) + 2 * Mp * sizeof(int);
}

__global__ __launch_bounds__(kSbThreads, 1) void sparse_ext_build_kernel(const SparseExtBuildArgs a) {
  extern __shared__ double sm[];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n = a.n, M = a.M;
  const int np4 = sb_np4(n), n16 = sb_n16(n), ldp = n16 + 1, ldd = np4 | 1, Mp = (M + 15) & ~15;
  double* Ps = sm;                                   // [np4][ldp]  P, zero beyond n x n
  double* Dt = Ps + (size_t)np4 * ldp;               // [16][ldd]   the row tile of D, zero beyond its M x n
  double* Gs = Dt + 16 * ldd;                        // [16][ldd]   Dt * P
  int* pt = reinterpret_cast<int*>(Gs + 16 * ldd);   // [Mp] times of the stacked observations
  int* pj = pt + Mp;                                 // [Mp] their outputs
  const double* P_src = a.Pb + (size_t)p * a.szB;
  for (int q = tid; q < np4 * ldp; q += kSbThreads) {
    const int r = q / ldp, c = q - r * ldp;
    Ps[q] = (r < n && c < n) ? P_src[(size_t)r * a.ldb + c] : 0.0;
  }
  for (int q = tid; q < Mp; q += kSbThreads) {
    pt[q] = q < M ? a.pair_t[q] : -1 - q;            // (padding rows: never equal to another time, never stored)
    pj[q] = q < M ? a.pair_j[q] : 0;
  }
  const double* D = a.D + (size_t)p * a.szD;
  double* S = a.S + (size_t)p * M * M;
  const int lr = lane & 15, lk = lane >> 4;
  const int KS = np4 >> 2, CT = n16 >> 4, RT = Mp >> 4;
  for (int rt = 0; rt < RT; ++rt) {
    __syncthreads();                                 // the last tile's readers of Dt and Gs are done (and Ps is complete)
    for (int q = tid; q < 16 * np4; q += kSbThreads) {
      const int r = q / np4, c = q - r * np4, row = 16 * rt + r;
      Dt[r * ldd + c] = (row < M && c < n) ? D[(size_t)row * a.ldn + c] : 0.0;
    }
    __syncthreads();
    // G = Dt * P: wave wv forms the column tiles wv, wv + 4 (at most two for n <= 96: their chains interleave)
    for (int ct0 = wv; ct0 < CT; ct0 += 8) {
      const int ct1 = ct0 + 4;
      const bool two = ct1 < CT;
      sb_v4d g0 = {0.0, 0.0, 0.0, 0.0}, g1 = {0.0, 0.0, 0.0, 0.0};
      const double* pa = Dt + lr * ldd + lk;
      const double* pb0 = Ps + (size_t)lk * ldp + 16 * ct0 + lr;
      const double* pb1 = Ps + (size_t)lk * ldp + 16 * (two ? ct1 : ct0) + lr;
      for (int ks = 0; ks < KS; ++ks) {
        const double av = pa[4 * ks];
        g0 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, pb0[(size_t)4 * ks * ldp], g0, 0, 0, 0);
        g1 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, pb1[(size_t)4 * ks * ldp], g1, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {                  // result: row lk + 4 r of the tile, column lr of the column tile
        const int row = lk + 4 * r;
        if (16 * ct0 + lr < np4) Gs[row * ldd + 16 * ct0 + lr] = g0[r];
        if (two && 16 * ct1 + lr < np4) Gs[row * ldd + 16 * ct1 + lr] = g1[r];
      }
    }
    __syncthreads();
    // S(16 rt + ., 16 ct + .) for ct <= rt, formed transposed -- A = the rows of D of tile ct, B = G' -- so that a result
    // register holds 16 consecutive rows of one column of the column-major S
    const int ia = 16 * rt + lr;                     // row of S this lane stores
    const int ta = pt[ia], ja = pj[ia];
    for (int ct0 = wv; ct0 <= rt; ct0 += 8) {
      const int ct1 = ct0 + 4;
      const bool two = ct1 <= rt;
      const int b0 = 16 * ct0 + lr, b1 = 16 * (two ? ct1 : ct0) + lr;
      const double* d0 = D + (size_t)min(b0, M - 1) * a.ldn;
      const double* d1 = D + (size_t)min(b1, M - 1) * a.ldn;
      const bool v0 = b0 < M, v1 = b1 < M;
      const double* pg = Gs + lr * ldd + lk;
      sb_v4d s0 = {0.0, 0.0, 0.0, 0.0}, s1 = {0.0, 0.0, 0.0, 0.0};
      for (int ks = 0; ks < KS; ++ks) {
        const int k = 4 * ks + lk, kc = min(k, n - 1);
        const double x0 = d0[kc], x1 = d1[kc];       // unconditional loads at clamped indices
        const double gv = pg[4 * ks];
        s0 = __builtin_amdgcn_mfma_f64_16x16x4f64((v0 && k < n) ? x0 : 0.0, gv, s0, 0, 0, 0);
        s1 = __builtin_amdgcn_mfma_f64_16x16x4f64((v1 && k < n) ? x1 : 0.0, gv, s1, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int jb0 = 16 * ct0 + lk + 4 * r, jb1 = 16 * ct1 + lk + 4 * r;       // columns of S
        if (ia < M && jb0 < M) {
          double v = s0[r];
          if (pt[jb0] == ta) v += a.R[ja + a.d * pj[jb0]];                        // blkdiag(RS, R(ind,ind))  (:211)
          S[(size_t)ia + (size_t)M * jb0] = v;                                    // :215
        }
        if (two && ia < M && jb1 < M) {
          double v = s1[r];
          if (pt[jb1] == ta) v += a.R[ja + a.d * pj[jb1]];
          S[(size_t)ia + (size_t)M * jb1] = v;
        }
      }
    }
  }
}

hipError_t launch_sparse_ext_build(const SparseExtBuildArgs& a, int N, hipStream_t s) {
  if (a.M <= 0 || N <= 0) return hipSuccess;
  if (a.n < 1 || a.n > 96 || a.M > 1023 || a.d < 1 || a.ldb < a.n || a.ldn < a.n) return hipErrorInvalidValue;
  const size_t lds = sparse_ext_build_lds_bytes(a.n, a.M);
  if (lds > 150 * 1024) return hipErrorInvalidValue;
  static std::atomic<uint64_t> attr{0};
  if (hipError_t e = lds_opt_in(reinterpret_cast<const void*>(&sparse_ext_build_kernel), 150 * 1024, attr)) return e;
  hipLaunchKernelGGL(sparse_ext_build_kernel, dim3(N), dim3(kSbThreads), lds, s, a);
  return hipGetLastError();
}

}  // namespace rbpf
