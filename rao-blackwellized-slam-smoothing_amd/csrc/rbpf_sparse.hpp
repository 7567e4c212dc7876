// sparseFeatures branch (examples/slam-sparse-visual): kernel arguments, see rbpf_sparse.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace rbpf {

struct SparseStepArgs {
  int N, t, n, d, nN, nw, ldx, ldb, propagate;
  size_t szB;
  double f, fp;                       // camera (measurement.m:46)
  const int* ai;                      // ancestors of this step (null: identity)
  const double* xn_old; size_t xn_old_stride; double* xn_new; size_t xn_new_stride;   // SoA [nN][stride]
  const double* xl_old; size_t xl_old_stride; double* xl_new;                         // [N][ldx]
  const double* Pb_old; size_t Pb_old_stride; double* Pb_new;                         // [N][n][ldb] row-major
  const double* y;                    // [d] outputs of this step, NaN = not observed
  const double* R;                    // [d x d] column-major
  const double* odo;                  // [nN]
  const double* Ssqrt;                // [nw x nw] element-wise sqrt(dt*Q)  (pfslam.m:81)
  int rng_mode, k_iter; unsigned long long seed; const double* Z;                     // replay normals [N][nw]
  const double* xref;                 // CPF-AS: state of slot N-1 (or null)
  double jitter;
  double* logw;
  int* status;
};

struct SparseAncArgs {
  int n, d, nN, ldx, ldb, M, off;
  size_t szB;
  double f, fp;
  const int* pair_t; const int* pair_j;     // observed (time, landmark) pairs of the whole run, time-major
  const double* xnk;                  // [T][nN] reference trajectory
  const double* y;                    // [T][d]
  const double* xl; const double* Pb; // particle banks (current generation)
  const double* R;                    // [d x d]
  double* rhs;                        // [N][M]
  double* S;                          // [N][M*M] column-major
};

// The same step for RBPF_MODEL_GENERIC_SPARSE (rbpf_sparse_ext.hip): measModel was evaluated by the caller's device code
struct SparseExtStepArgs {
  int N, n, d, ldx, ldb;
  size_t szB;
  const int* ai;                      // ancestors of this step (null: identity): whose covariance slot i starts from
  const double* xl_g;                 // [N][ldx] xl(:,ai), gathered before measModel ran (particleFilter.m:112)
  double* xl_new;                     // [N][ldx]
  const double* Pb_old; size_t Pb_old_stride; double* Pb_new;                         // [N][n][ldb] row-major
  const double* yhat; size_t yhat_si, yhat_sk;       // yhat(i, k) at i*si + k*sk
  const double* dy; size_t dy_sp; int dy_sr;         // dy(i, k, c) at i*sp + k*sr + c
  const double* y;                    // [d] outputs of this step, NaN = not observed
  const double* R;                    // [d x d] column-major
  double jitter;
  double* logw;
  int* status;
};

size_t sparse_ext_step_lds_bytes(int n, int d);
hipError_t launch_sparse_ext_step(const SparseExtStepArgs& a, hipStream_t s);
hipError_t launch_sparse_ext_gather_xl(int N, int ldx, const double* src, size_t src_stride, const int* ai, double* out, hipStream_t s);
hipError_t launch_sparse_ext_yhat_of_max(int d, const double* yhat, size_t si, size_t sk, const int* iw_max, double* out, hipStream_t s);

// Ancestor weights of the smoother for RBPF_MODEL_GENERIC_SPARSE (rbpf_sparse_ext_anc.hip)
struct SparseExtPackArgs {
  int N, F, n, d, M, m0, Mc;          // particles, future times of the chunk, nLin, n_y; pairs [m0, m0 + Mc) of the step's M
  int slot0;                          // index of the chunk's first time in the table of observed times
  const int* time_slot;               // [T] index of every time in that table
  const int* pair_t; const int* pair_j;     // the step's stacked (time, output) pairs
  const double* y;                    // [T][d]
  const double* yhat; int yhat_layout;      // of the handle's F N columns: 0 MATLAB order, 2 C-contiguous
  const double* dy; int dy_layout, dy_ld;   // 0 MATLAB order; 1 / 2: rows on the stride dy_ld
  double* D;                          // [N][M][n]
  double* rhs;                        // [N][M]
};

struct SparseExtBuildArgs {
  int n, M, d, ldb, ldn;
  size_t szB, szD;                    // doubles between two particles' P and D
  const double* Pb;                   // [N][n][ldb] row-major (symmetric)
  const double* D;                    // [N][M][ldn]
  const int* pair_t; const int* pair_j;     // [M] time and output of every stacked row
  const double* R;                    // [d x d] column-major
  double* S;                          // [N][M*M] column-major: the 16 x 16 tiles on and below the diagonal
};

hipError_t launch_sparse_ext_replicate(int N, int F, int nN, int ldx, const int* times, const double* xnk, const double* xl_bank,
                                       double* xn, double* xl, hipStream_t s);
hipError_t launch_sparse_ext_pack(const SparseExtPackArgs& a, hipStream_t s);
size_t sparse_ext_build_lds_bytes(int n, int M);
hipError_t launch_sparse_ext_build(const SparseExtBuildArgs& a, int N, hipStream_t s);

size_t sparse_step_lds_bytes(int n, int d);
hipError_t launch_sparse_step(const SparseStepArgs& a, hipStream_t s);
hipError_t launch_sparse_anc(const SparseAncArgs& a, int N, hipStream_t s);

}  // namespace rbpf
