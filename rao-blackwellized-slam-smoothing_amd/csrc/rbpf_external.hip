// Generic model family on the device (rbpf_filter_ancestors_device / rbpf_filter_step_device / device callbacks): the
// re-layouts between what a caller's handles read and write -- column-major states, Jacobians as measModel returns them --
// and what the step kernels consume (StepArgs::xn_ext SoA [nN][N], StepArgs::H_ext [N][d][ldx]).  Nothing here computes;
// the Jacobian pack is the one kernel with real bytes (2 N d nLin 8 B per step).
#include "rbpf_internal.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>

namespace rbpf {

// xn_anc[q + nN*i] = X[q][clamp(ai[i])] (ai == nullptr: i itself) for the slots i < count -- the ancestors' states in the
// callbacks' order (particleFilter.m:106-108; the smoothers' later iterations gather the N - 1 ordinary slots only,
// particleSmoother.m:132-137).  The clamp is generic_draw_propagate's.
__global__ void ext_gather_states_kernel(int count, int N, int nN, const double* __restrict__ soa, const int* __restrict__ ai,
                                         double* __restrict__ cm) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const int a = ai ? min(max(ai[i], 0), N - 1) : i;
  for (int q = 0; q < nN; ++q) cm[q + (size_t)nN * i] = soa[(size_t)q * N + a];
}

// soa[q][i] = cm[q + nN*i]
__global__ void ext_states_to_soa_kernel(int N, int nN, const double* __restrict__ cm, double* __restrict__ soa) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  for (int q = 0; q < nN; ++q) soa[(size_t)q * N + i] = cm[q + (size_t)nN * i];
}

// The smoothers' form of the kernel above: slot N - 1 is the conditioned reference trajectory (particleSmoother.m:242), so its
// column of cm -- which dynModel did not write -- is filled from xref [nN] here, before measModel reads cm.  xref == nullptr:
// every column is the handle's.
__global__ void ext_states_to_soa_ref_kernel(int N, int nN, double* __restrict__ cm, double* __restrict__ soa,
                                             const double* __restrict__ xref) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const bool ref = xref != nullptr && i == N - 1;
  for (int q = 0; q < nN; ++q) {
    const double v = ref ? xref[q] : cm[q + (size_t)nN * i];
    if (ref) cm[q + (size_t)nN * i] = v;
    soa[(size_t)q * N + i] = v;
  }
}

// MATLAB order dy(i, k, c) at i + N*(k + d*c)  ->  H[(i*d + k)*ldx + c]: a transpose of the (i, c) plane of every output
// row k.  One workgroup moves a tile of kPackTile particles x kPackTile coefficients through LDS: the loads run along i
// (contiguous in the source), the stores along c (contiguous in the destination).  The tile's rows are padded by one
// double, so the transposed read (lane l at row l: stride 65 doubles = 130 banks of 4 B) puts the 32 lanes of a half
// wave on 32 different bank pairs.  Columns nLin..ldx-1 of the destination are written as zeros.
constexpr int kPackTile = 64;
constexpr int kPackRows = 4;       // tile rows in flight per pass: 256 threads = kPackRows waves of 64

__global__ void __launch_bounds__(kPackTile * kPackRows)
ext_pack_dy_matlab_kernel(int N, int d, int n, int ldx, const double* __restrict__ dy, double* __restrict__ H) {
  __shared__ double tile[kPackTile][kPackTile + 1];      // [c][i]
  const int tx = threadIdx.x % kPackTile, ty = threadIdx.x / kPackTile;
  const int c0 = blockIdx.x * kPackTile, i0 = blockIdx.y * kPackTile, k = blockIdx.z;
  const int i_in = i0 + tx;
  for (int cl = ty; cl < kPackTile; cl += kPackRows) {
    const int c = c0 + cl;
    tile[cl][tx] = (i_in < N && c < n) ? dy[(size_t)i_in + (size_t)N * (k + (size_t)d * c)] : 0.0;
  }
  __syncthreads();
  const int c_out = c0 + tx;
  if (c_out >= ldx) return;
  for (int il = ty; il < kPackTile; il += kPackRows) {
    const int i = i0 + il;
    if (i < N) H[((size_t)i * d + k) * ldx + c_out] = tile[tx][il];
  }
}

// C-contiguous [N][d][nLin]  ->  the same rows on the ldx stride, zeros behind them.  One element of the destination per
// thread and pass: stores are contiguous over the whole buffer, loads contiguous within a row.
__global__ void ext_pack_dy_rows_kernel(size_t rows, int n, int ldx, const double* __restrict__ dy, double* __restrict__ H) {
  const size_t total = rows * (size_t)ldx;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const size_t r = e / (size_t)ldx;
    const int c = (int)(e - r * (size_t)ldx);
    H[e] = (c < n) ? dy[r * (size_t)n + c] : 0.0;
  }
}

// Pack and whiten in one pass (the refreshes of the information form, rbpf_smoother.hip::info_gram_product): G = W H written
// straight to its place, G[(i*d + a)*n + c] = sum_b W[a + d*b] dy(i, b, c), instead of the pack above followed by
// sweep_whiten_kernel's read-modify-write of the same rows.  The arithmetic is that kernel's, s = 0; for b ascending:
// s = fma(W[a + d*b], v[b], s), so the result equals the two-kernel path bit for bit.
//
// MATLAB order: the d outputs of one (i, c) pair lie rows * n doubles apart in the source, so a workgroup moves d planes of a
// tile through LDS.  The tile is kPackTile coefficients x kWhitenCols particles (32, not 64: three planes of [64][65] doubles
// would be 100 KB, one workgroup per CU; [3][64][33] is 50 KB and keeps three).  Loads run along i, 32 lanes on 256
// consecutive bytes per plane row; stores along c, 64 lanes on 512 consecutive bytes.  The row pad is the pack kernel's: an
// odd row stride in doubles (33 as 65) is 2 mod 32 in 4-byte banks, so the transposed read -- lane l at row l -- puts the 32
// lanes of a half wave on 32 different bank pairs.
constexpr int kWhitenCols = 32;

__global__ void __launch_bounds__(kPackTile * kPackRows)
ext_pack_whiten_matlab_kernel(int rows, int d, int n, const double* __restrict__ dy, const double* __restrict__ W,
                              double* __restrict__ G) {
  __shared__ double tile[3][kPackTile][kWhitenCols + 1];      // [b][c][i]
  const int c0 = blockIdx.x * kPackTile, i0 = blockIdx.y * kWhitenCols;
  {
    const int ix = threadIdx.x % kWhitenCols, cy = threadIdx.x / kWhitenCols;
    const int i_in = i0 + ix;
    for (int b = 0; b < d; ++b)
      for (int cl = cy; cl < kPackTile; cl += (kPackTile * kPackRows) / kWhitenCols) {
        const int c = c0 + cl;
        tile[b][cl][ix] = (i_in < rows && c < n) ? dy[(size_t)i_in + (size_t)rows * (b + (size_t)d * c)] : 0.0;
      }
  }
  __syncthreads();
  const int tx = threadIdx.x % kPackTile, ty = threadIdx.x / kPackTile;
  const int c_out = c0 + tx;
  if (c_out >= n) return;
  double w[9];                                                  // W(a, b) at a + 3 b, whatever d is: fixed indices, registers
#pragma unroll
  for (int b = 0; b < 3; ++b)
#pragma unroll
    for (int a = 0; a < 3; ++a) w[a + 3 * b] = (a < d && b < d) ? W[a + d * b] : 0.0;
  for (int il = ty; il < kWhitenCols; il += kPackRows) {
    const int i = i0 + il;
    if (i >= rows) break;
    double v[3];
#pragma unroll
    for (int b = 0; b < 3; ++b) v[b] = (b < d) ? tile[b][tx][il] : 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (a >= d) break;
      double s = 0.0;
#pragma unroll
      for (int b = 0; b < 3; ++b) if (b < d) s = fma(w[a + 3 * b], v[b], s);
      G[((size_t)i * d + a) * n + c_out] = s;
    }
  }
}

// Rows of H contiguous, row stride ld (C-contiguous: ld = n; the native layout's rows: ld = ldx): one (i, c) pair per thread
// and pass, loads and stores contiguous within a row.
__global__ void ext_pack_whiten_rows_kernel(size_t rows, int d, int n, int ld, const double* __restrict__ dy,
                                            const double* __restrict__ W, double* __restrict__ G) {
  const size_t total = rows * (size_t)n;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const size_t i = e / (size_t)n;
    const int c = (int)(e - i * (size_t)n);
    double v[3];
    for (int b = 0; b < d; ++b) v[b] = dy[(i * d + b) * (size_t)ld + c];
    for (int a = 0; a < d; ++a) {
      double s = 0.0;
      for (int b = 0; b < d; ++b) s = fma(W[a + d * b], v[b], s);
      G[(i * d + a) * (size_t)n + c] = s;
    }
  }
}

// rows of `n` doubles on the stride ld -> the same rows back to back (the native layout's rows without their pad)
__global__ void ext_compact_rows_kernel(size_t rows, int n, int ld, const double* __restrict__ src, double* __restrict__ dst) {
  const size_t total = rows * (size_t)n;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const size_t r = e / (size_t)n;
    dst[e] = src[r * (size_t)ld + (e - r * (size_t)n)];
  }
}

hipError_t launch_ext_gather_states(int N, int nN, const double* soa, const int* ai, double* cm, hipStream_t s) {
  hipLaunchKernelGGL(ext_gather_states_kernel, dim3((N + 255) / 256), dim3(256), 0, s, N, N, nN, soa, ai, cm);
  return hipGetLastError();
}

hipError_t launch_ext_gather_columns(int count, int N, int nN, const double* soa, const int* ai, double* cm, hipStream_t s) {
  if (count <= 0) return hipSuccess;
  hipLaunchKernelGGL(ext_gather_states_kernel, dim3((count + 255) / 256), dim3(256), 0, s, count, N, nN, soa, ai, cm);
  return hipGetLastError();
}

hipError_t launch_ext_states_to_soa_ref(int N, int nN, double* cm, double* soa, const double* xref, hipStream_t s) {
  hipLaunchKernelGGL(ext_states_to_soa_ref_kernel, dim3((N + 255) / 256), dim3(256), 0, s, N, nN, cm, soa, xref);
  return hipGetLastError();
}

hipError_t launch_ext_pack_whiten(int layout, int rows, int d, int n, int ld, const double* dy, const double* W, double* G,
                                  hipStream_t s) {
  if (d < 1 || d > 3) return hipErrorInvalidValue;   // tile[3], w[9], v[3] below: the refreshes of carried factors, n_y = 1 and 3 only
  if (rows <= 0) return hipSuccess;
  if (layout == 0) {
    const dim3 grid((n + kPackTile - 1) / kPackTile, (rows + kWhitenCols - 1) / kWhitenCols);
    hipLaunchKernelGGL(ext_pack_whiten_matlab_kernel, grid, dim3(kPackTile * kPackRows), 0, s, rows, d, n, dy, W, G);
  } else {
    const size_t total = (size_t)rows * n;
    const unsigned blocks = (unsigned)std::min<size_t>((total + 255) / 256, (size_t)1 << 20);
    hipLaunchKernelGGL(ext_pack_whiten_rows_kernel, dim3(blocks), dim3(256), 0, s, (size_t)rows, d, n, ld, dy, W, G);
  }
  return hipGetLastError();
}

hipError_t launch_ext_compact_rows(size_t rows, int n, int ld, const double* src, double* dst, hipStream_t s) {
  const size_t total = rows * (size_t)n;
  if (total == 0) return hipSuccess;
  const unsigned blocks = (unsigned)std::min<size_t>((total + 255) / 256, (size_t)1 << 20);
  hipLaunchKernelGGL(ext_compact_rows_kernel, dim3(blocks), dim3(256), 0, s, rows, n, ld, src, dst);
  return hipGetLastError();
}

hipError_t launch_ext_states_to_soa(int N, int nN, const double* cm, double* soa, hipStream_t s) {
  hipLaunchKernelGGL(ext_states_to_soa_kernel, dim3((N + 255) / 256), dim3(256), 0, s, N, nN, cm, soa);
  return hipGetLastError();
}

hipError_t launch_ext_pack_dy(int layout, int N, int d, int n, int ldx, const double* dy, double* H, hipStream_t s) {
  if (layout == 0) {
    const dim3 grid((ldx + kPackTile - 1) / kPackTile, (N + kPackTile - 1) / kPackTile, d);
    hipLaunchKernelGGL(ext_pack_dy_matlab_kernel, grid, dim3(kPackTile * kPackRows), 0, s, N, d, n, ldx, dy, H);
  } else {
    const size_t rows = (size_t)N * d, total = rows * (size_t)ldx;
    const unsigned blocks = (unsigned)std::min<size_t>((total + 255) / 256, (size_t)1 << 20);
    hipLaunchKernelGGL(ext_pack_dy_rows_kernel, dim3(blocks), dim3(256), 0, s, rows, n, ldx, dy, H);
  }
  return hipGetLastError();
}

}  // namespace rbpf
