// Generic model family on the device (rbpf_filter_ancestors_device / rbpf_filter_step_device / device callbacks): the
// re-layouts between what a caller's handles read and write -- column-major states, Jacobians as measModel returns them --
// and what the step kernels consume (StepArgs::xn_ext SoA [nN][N], StepArgs::H_ext [N][d][ldx]).  Nothing here computes;
// the Jacobian pack is the one kernel with real bytes (2 N d nLin 8 B per step).
#include "rbpf_internal.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>

namespace rbpf {

// xn_anc[q + nN*i] = X[q][clamp(ai[i])] (ai == nullptr: i itself) -- the ancestors' states in the callbacks' order
// (particleFilter.m:106-108).  The clamp is generic_draw_propagate's.
__global__ void ext_gather_states_kernel(int N, int nN, const double* __restrict__ soa, const int* __restrict__ ai,
                                         double* __restrict__ cm) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int a = ai ? min(max(ai[i], 0), N - 1) : i;
  for (int q = 0; q < nN; ++q) cm[q + (size_t)nN * i] = soa[(size_t)q * N + a];
}

// soa[q][i] = cm[q + nN*i]
__global__ void ext_states_to_soa_kernel(int N, int nN, const double* __restrict__ cm, double* __restrict__ soa) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  for (int q = 0; q < nN; ++q) soa[(size_t)q * N + i] = cm[q + (size_t)nN * i];
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

hipError_t launch_ext_gather_states(int N, int nN, const double* soa, const int* ai, double* cm, hipStream_t s) {
  hipLaunchKernelGGL(ext_gather_states_kernel, dim3((N + 255) / 256), dim3(256), 0, s, N, nN, soa, ai, cm);
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
