// EKF comparison baseline of examples/slam-dense-mag (ekf_dense.m:67-102 with the closures measModel_ekf / dynModel_ekf of
// run_dense3D_magfield.m:281-299,310-316) on the device, batched over independent runs (data sets).
//
// One Gaussian state [position(3); orientation deviation(3); map(nLin = m + 3)], n = 6 + nLin, P [n x n] fp64 in full-square
// storage, one matrix per run, rewritten in place.  Two launches per time step, both batched over the B runs of the call:
//
//   ekf_gain_kernel    one workgroup per run.  With PH = Pp dy' (three columns) handed over by the previous update pass:
//                      SS = dy PH + R, its 3 x 3 Cholesky (one retry with jitter 1e-3, ekf_dense.m:83-86), xf = xp + PH (SS \ e),
//                      the relinearisation (:95-96), the trajectory rows, and U = M PH' with M = inv(SS) (M = inv(SSj) SS inv(SSj)
//                      after a jitter retry, which is what K SS K' of :91 amounts to).  Then the NEXT step's prediction
//                      (dynModel_ekf), its 6 x 6 block D = G Qt G' and its measurement Jacobian dy_next: basis-gradient rows from
//                      per-axis sin / cos tables in LDS, the Hessian contraction J3 in the same loop.
//   ekf_update_kernel  grid = row tiles x B, the hot path.  One pass over P:
//                          P(i,j) <- 0.5 (((P(i,j) + D(i,j)) - PH(i,:) U(:,j)) + ((P(j,i) + D(j,i)) - PH(j,:) U(:,i)))     (:91-92)
//                      and, in the same pass, PH_next(j,:) = sum_i P_new(i,j) dy_next(:,i) for the lines it holds.  P is symmetric
//                      bit for bit (both halves of the sum are evaluated by the same expression at the mirrored element), so the
//                      pass reads P(i,j) only: every element is read and written by the same thread, and a workgroup's lines
//                      need nothing from any other workgroup.  8 n^2 bytes read + 8 n^2 written per run and step.
//
// The prediction covariance Pp = Pf + G Qt G' (F = I) touches the leading 6 x 6 block only; it is never stored: the update pass
// adds D on the fly and the gain kernel adds D dy(:,1:6)' to the carried PH.  Reductions are shuffle butterflies and fixed-order
// sums over the four waves (no atomics), and nothing depends on a run's position in the batch: a run's results are bit-identical
// alone and batched.
#include "../../include/rbpf.h"
#include "rbpf_internal.hpp"
#include "rbpf_device.hpp"
#include "rbpf_ctx.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace rbpf {

constexpr int kEkfTile = 64;               // lines of P per update workgroup: 4 waves x 16 lines
constexpr int kEkfMaxNLin = 1151;          // the filter's own range of nLin
constexpr int kEkfSmall = 32;              // doubles of small per-run scratch in the gain kernel's LDS: M[9] g[3] q[4] Rnb[9]
constexpr int kEkfLdsLimit = 160 * 1024;

struct EkfRunDev {                         // per-run constants (device array [B])
  double L[3];                             // domain half-widths of the basis
  double lo[3], up[3];                     // LL of JacobianPhi3D (run_dense3D_magfield.m:292)
  int kmax[3], ktot;
  const int* NN;                           // [3][m] axis-major
};

struct EkfGainArgs {
  int n, m, T, t;                          // t = -1: only prepare step 0 (no gain, no prediction)
  int ktmax;                               // table pitch in LDS: largest ktot of the batch
  const EkfRunDev* runs;
  double* x;                               // [B][n] state: xp on entry, xp of the next step on exit
  double* q;                               // [B][4]
  double* dy;                              // [B][3][n] measurement Jacobian of the step about to be updated / of the next one
  double* yhat;                            // [B][3]
  double* D;                               // [B][2][36] G Qt G' of step t in slot t & 1 (column-major 6 x 6)
  const double* PHacc;                     // [B][3][n] Pf dy' carried by the previous update pass
  double* PH;                              // [B][3][n] Pp dy'
  double* U;                               // [B][3][n] M PH'
  const double* odo;                       // [B][T-1][7]
  const double* y;                         // [B][T][3]
  const double* R;                         // [B][9] column-major
  const double* Qt; int qt_pages;          // [pages][36] dt * Q
  double* xf_traj;                         // [B][T][n]
  double* qnb_traj;                        // [B][T][4]
  int* status;                             // [B] 0, or 1 + the first step whose SS failed both factorisations
};

struct EkfUpdArgs {
  int n;
  const double* Pin; size_t pin_stride;    // per-run strides in elements
  double* Pout; size_t pout_stride;
  const double* PH; const double* U; const double* dy;   // [B][3][n]
  const double* D; int dslot;              // null: no prediction block (the pass before step 0)
  double* PHacc;                           // [B][3][n] out
};

static size_t ekf_gain_lds_bytes(int n, int ktmax) { return ((size_t)n + 4 * (size_t)ktmax + 4 * 12 + kEkfSmall) * sizeof(double); }
static size_t ekf_update_lds_bytes(int n) { return ((size_t)9 * n + 36) * sizeof(double); }

// fixed-order sum over the workgroup's 256 threads of K values per thread; every thread gets the result
template <int K>
__device__ __forceinline__ void ekf_block_sum(double (&v)[K], double* red, int tid) {
  const int lane = tid & 63, wv = tid >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    v[k] = wave_sum(v[k]);
    if (lane == 0) red[wv * K + k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = (red[k] + red[K + k]) + (red[2 * K + k] + red[3 * K + k]);
  __syncthreads();
}

__global__ __launch_bounds__(256) void ekf_gain_kernel(const EkfGainArgs a) {
  extern __shared__ double sm[];
  const int b = blockIdx.x, tid = threadIdx.x, n = a.n, nl = a.n - 6, m = a.m, t = a.t, T = a.T;
  const EkfRunDev& run = a.runs[b];
  double* xs = sm;                         // [n]
  double* tS = xs + n;                     // basis tables on [-L, L] (tools/domain_cartesian_dx.m:146-170)
  double* tC = tS + a.ktmax;
  double* hS = tC + a.ktmax;               // Hessian tables on LL (tools/JacobianPhi3D.m:41-48)
  double* hC = hS + a.ktmax;
  double* red = hC + a.ktmax;              // [4][12]
  double* sM = red + 48;                   // [9]
  double* sg = sM + 9;                     // [3]
  double* sq = sg + 3;                     // [4]
  double* sR = sq + 4;                     // [9] Rnb, Rm[row * 3 + col]
  const size_t bn = (size_t)b * n, b3n = (size_t)b * 3 * n;
  double* dy = a.dy + b3n;
  for (int i = tid; i < n; i += 256) xs[i] = a.x[bn + i];
  if (tid < 4) sq[tid] = a.q[(size_t)b * 4 + tid];
  __syncthreads();

  if (t >= 0) {
    // ---- PH = Pp dy' = Pf dy' + D dy(:,1:6)' and SS = dy PH + R ---------------------------------------------------------
    const double* Dt = a.D + ((size_t)b * 2 + (t & 1)) * 36;
    const double* PHacc = a.PHacc + b3n;
    double* PH = a.PH + b3n;
    double* U = a.U + b3n;
    double ss[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) ss[k] = 0.0;
    for (int i = tid; i < n; i += 256) {
      double ph[3], d[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) { ph[c] = PHacc[(size_t)c * n + i]; d[c] = dy[(size_t)c * n + i]; }
      if (i < 6) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          double s = 0.0;
          for (int j = 0; j < 6; ++j) s = fma(Dt[i + 6 * j], dy[(size_t)c * n + j], s);
          ph[c] += s;
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) PH[(size_t)c * n + i] = ph[c];
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) ss[r + 3 * c] = fma(d[r], ph[c], ss[r + 3 * c]);
    }
    ekf_block_sum<9>(ss, red, tid);
    if (tid == 0) {
      double S[9], Sj[9], Lc[9], e[3], z[3], g[3], Si[9], M[9];
      for (int k = 0; k < 9; ++k) { S[k] = ss[k] + a.R[(size_t)b * 9 + k]; Sj[k] = S[k]; }
      bool jit = false;
      bool ok = chol_lower_small<3>(S, Lc);
      if (!ok) {                                                              // ekf_dense.m:83-86, jitter = 1e-3 (:58)
        jit = true;
        for (int k = 0; k < 3; ++k) Sj[k + 3 * k] = S[k + 3 * k] + 1e-3;
        ok = chol_lower_small<3>(Sj, Lc);
      }
      if (ok) {
        for (int k = 0; k < 3; ++k) e[k] = a.y[((size_t)b * T + t) * 3 + k] - a.yhat[(size_t)b * 3 + k];
        fwd_subst<3>(Lc, e, z);
        bwd_subst_T<3>(Lc, z, g);
        for (int c = 0; c < 3; ++c) {
          const double u[3] = {c == 0 ? 1.0 : 0.0, c == 1 ? 1.0 : 0.0, c == 2 ? 1.0 : 0.0};
          fwd_subst<3>(Lc, u, z);
          bwd_subst_T<3>(Lc, z, &Si[3 * c]);
        }
        if (jit) {                                                            // K SS K' with K = PH inv(SSj)
          double Tm[9];
          for (int c = 0; c < 3; ++c)
            for (int r = 0; r < 3; ++r) Tm[r + 3 * c] = Si[r] * S[3 * c] + Si[r + 3] * S[1 + 3 * c] + Si[r + 6] * S[2 + 3 * c];
          for (int c = 0; c < 3; ++c)
            for (int r = 0; r < 3; ++r) M[r + 3 * c] = Tm[r] * Si[3 * c] + Tm[r + 3] * Si[1 + 3 * c] + Tm[r + 6] * Si[2 + 3 * c];
        } else {
          for (int k = 0; k < 9; ++k) M[k] = Si[k];
        }
      } else {                                                                // the call fails; keep the state finite
        if (a.status[b] == 0) a.status[b] = t + 1;
        for (int k = 0; k < 9; ++k) M[k] = 0.0;
        for (int k = 0; k < 3; ++k) g[k] = 0.0;
      }
      for (int k = 0; k < 9; ++k) sM[k] = M[k];
      for (int k = 0; k < 3; ++k) sg[k] = g[k];
    }
    __syncthreads();
    // ---- xf = xp + PH (SS \ e), U = M PH' ----------------------------------------------------------------------------------
    for (int i = tid; i < n; i += 256) {
      double ph[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) ph[c] = PH[(size_t)c * n + i];             // this thread's own stores
#pragma unroll
      for (int r = 0; r < 3; ++r) U[(size_t)r * n + i] = fma(sM[r + 6], ph[2], fma(sM[r + 3], ph[1], sM[r] * ph[0]));
      xs[i] += fma(ph[2], sg[2], fma(ph[1], sg[1], ph[0] * sg[0]));           // :90
    }
    __syncthreads();
    if (tid == 0) {                                                           // :95-96
      const double phi[3] = {xs[3] / 2.0, xs[4] / 2.0, xs[5] / 2.0};
      double eq[4], qn[4];
      expq_dev(phi, eq);
      qleft_mul(eq, sq, qn);
      for (int k = 0; k < 4; ++k) { sq[k] = qn[k]; a.qnb_traj[((size_t)b * T + t) * 4 + k] = qn[k]; }
      xs[3] = 0.0; xs[4] = 0.0; xs[5] = 0.0;
    }
    __syncthreads();
    for (int i = tid; i < n; i += 256) a.xf_traj[((size_t)b * T + t) * n + i] = xs[i];
    __syncthreads();                                                          // the prediction below rewrites xs[0..2]
  }
  if (t + 1 >= T) return;

  // ---- the next step: dynModel_ekf (run_dense3D_magfield.m:310-316), D = G Qt G', measModel_ekf (:281-299) ---------------
  if (tid == 0) {
    double* Dn = a.D + ((size_t)b * 2 + ((t + 1) & 1)) * 36;
    if (t >= 0) {
      const double* odo = a.odo + ((size_t)b * (T - 1) + t) * 7;
      double qn[4];
      for (int k = 0; k < 3; ++k) xs[k] += odo[k];                            // :312
      qleft_mul(sq, odo + 3, qn);                                             // :313
      for (int k = 0; k < 4; ++k) sq[k] = qn[k];
    }
    quat2rmat_dev(sq, sR);
    if (t >= 0) {
      const double* Qt = a.Qt + (size_t)(a.qt_pages > 1 ? t : 0) * 36;
      double G[36], T1[36];                                                   // G(1:6,:) = blkdiag(I, Rnb), column-major (:315)
      for (int k = 0; k < 36; ++k) G[k] = 0.0;
      for (int k = 0; k < 3; ++k) G[k + 6 * k] = 1.0;
      for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) G[(3 + r) + 6 * (3 + c)] = sR[r * 3 + c];
      for (int c = 0; c < 6; ++c)
        for (int r = 0; r < 6; ++r) { double s = 0.0; for (int k = 0; k < 6; ++k) s += G[r + 6 * k] * Qt[k + 6 * c]; T1[r + 6 * c] = s; }
      for (int c = 0; c < 6; ++c)
        for (int r = 0; r < 6; ++r) { double s = 0.0; for (int k = 0; k < 6; ++k) s += T1[r + 6 * k] * G[c + 6 * k]; Dn[r + 6 * c] = s; }
    } else {
      for (int k = 0; k < 36; ++k) Dn[k] = 0.0;
    }
  }
  __syncthreads();
  const int kt = run.ktot;
  for (int e = tid; e < 2 * kt; e += 256) {
    const bool hess = e >= kt;
    int ax = 0, k = hess ? e - kt : e;
    const int qi = k;
    if (k >= run.kmax[0]) { k -= run.kmax[0]; ax = 1; if (k >= run.kmax[1]) { k -= run.kmax[1]; ax = 2; } }
    double s, c;
    if (!hess) {
      const double La = run.L[ax];
      sincos(RBPF_PI * (double)(k + 1) * (xs[ax] + La) / (2.0 * La), &s, &c);
      tS[qi] = s; tC[qi] = c;
    } else {
      const double ba = run.up[ax] - run.lo[ax];
      sincos(RBPF_PI * (double)(k + 1) * (xs[ax] - run.lo[ax]) / ba, &s, &c);
      hS[qi] = s; hC[qi] = c;
    }
  }
  __syncthreads();
  double Rm[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) Rm[k] = sR[k];
  const int base[3] = {0, run.kmax[0], run.kmax[0] + run.kmax[1]};
  double acc[9];                           // v = dPhi x(7:end) [3], then J3 (symmetric): xx xy xz yy yz zz
#pragma unroll
  for (int k = 0; k < 9; ++k) acc[k] = 0.0;
  for (int k = tid; k < nl; k += 256) {
    double g[3];
    const double xk = xs[6 + k];
    if (k < 3) {
      g[0] = (k == 0); g[1] = (k == 1); g[2] = (k == 2);
    } else {
      const int j = k - 3;
      int nn[3];
      double sv[3], cv[3], f[3], hs[3], hc[3];
#pragma unroll
      for (int ax = 0; ax < 3; ++ax) {
        nn[ax] = run.NN[(size_t)ax * m + j];
        const int qi = base[ax] + nn[ax] - 1;
        sv[ax] = tS[qi]; cv[ax] = tC[qi];
        const double ba = run.up[ax] - run.lo[ax];
        const double mult = 1.0 / sqrt(0.5 * ba);
        f[ax] = (RBPF_PI * (double)nn[ax]) / ba;
        hs[ax] = hS[qi] * mult; hc[ax] = hC[qi] * mult;
      }
#pragma unroll
      for (int di = 0; di < 3; ++di) {                                        // domain_cartesian_dx.m:146-170, evaluation order kept
        double v = 1.0;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
          const double La = run.L[ax];
          if (ax == di) v = v * RBPF_PI * (double)nn[ax] / (2.0 * La * sqrt(La)) * cv[ax];
          else v = v * 1.0 / sqrt(La) * sv[ax];
        }
        g[di] = v;
      }
      const double sss = hs[0] * hs[1] * hs[2];                               // JacobianPhi3D.m:50-58
      acc[3] = fma(-f[0] * f[0] * sss, xk, acc[3]);
      acc[4] = fma(f[0] * f[1] * hc[0] * hc[1] * hs[2], xk, acc[4]);
      acc[5] = fma(f[0] * f[2] * hc[0] * hs[1] * hc[2], xk, acc[5]);
      acc[6] = fma(-f[1] * f[1] * sss, xk, acc[6]);
      acc[7] = fma(f[1] * f[2] * hs[0] * hc[1] * hc[2], xk, acc[7]);
      acc[8] = fma(-f[2] * f[2] * sss, xk, acc[8]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      dy[(size_t)c * n + 6 + k] = Rm[0 * 3 + c] * g[0] + Rm[1 * 3 + c] * g[1] + Rm[2 * 3 + c] * g[2];   // :298
      acc[c] = fma(g[c], xk, acc[c]);
    }
  }
  ekf_block_sum<9>(acc, red, tid);
  if (tid == 0) {
    const double v[3] = {acc[0], acc[1], acc[2]};
    const double J3[9] = {acc[3], acc[4], acc[5], acc[4], acc[6], acc[7], acc[5], acc[7], acc[8]};   // column-major, symmetric
    double X[9];
    mcross_dev(v, X);
    for (int c = 0; c < 3; ++c) {
      a.yhat[(size_t)b * 3 + c] = Rm[0 * 3 + c] * v[0] + Rm[1 * 3 + c] * v[1] + Rm[2 * 3 + c] * v[2];                  // :290
      for (int col = 0; col < 3; ++col) {
        dy[(size_t)c * n + col] = Rm[0 * 3 + c] * J3[0 + 3 * col] + Rm[1 * 3 + c] * J3[1 + 3 * col] + Rm[2 * 3 + c] * J3[2 + 3 * col];   // :296
        dy[(size_t)c * n + 3 + col] = Rm[0 * 3 + c] * X[0 + 3 * col] + Rm[1 * 3 + c] * X[1 + 3 * col] + Rm[2 * 3 + c] * X[2 + 3 * col];  // :297
      }
    }
  }
  for (int i = tid; i < n; i += 256) a.x[bn + i] = xs[i];
  if (tid < 4) a.q[(size_t)b * 4 + tid] = sq[tid];
}

// line j of P = the n contiguous elements P(0..n-1, j); a wave takes the lines wv, wv + 4, ... of its tile, lane = row
__global__ __launch_bounds__(256) void ekf_update_kernel(const EkfUpdArgs a) {
  extern __shared__ double sm[];
  const int n = a.n, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  double* sPH = sm;                        // [3][n]
  double* sU = sPH + 3 * (size_t)n;
  double* sdy = sU + 3 * (size_t)n;
  double* sD = sdy + 3 * (size_t)n;        // [36]
  const size_t b3n = (size_t)b * 3 * n;
  for (int i = tid; i < 3 * n; i += 256) {
    sPH[i] = a.PH[b3n + i];
    sU[i] = a.U[b3n + i];
    sdy[i] = a.dy[b3n + i];
  }
  if (tid < 36) sD[tid] = a.D ? a.D[((size_t)b * 2 + a.dslot) * 36 + tid] : 0.0;
  __syncthreads();
  const double* Pin = a.Pin + (size_t)b * a.pin_stride;
  double* Pout = a.Pout + (size_t)b * a.pout_stride;
  const int j0 = blockIdx.x * kEkfTile;
  for (int lj = wv; lj < kEkfTile; lj += 4) {
    const int j = j0 + lj;
    if (j >= n) break;                     // the tail tile (wave-uniform)
    const double phj0 = sPH[j], phj1 = sPH[n + j], phj2 = sPH[2 * n + j];
    const double uj0 = sU[j], uj1 = sU[n + j], uj2 = sU[2 * n + j];
    const double* lin = Pin + (size_t)j * n;
    double* lout = Pout + (size_t)j * n;
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
    for (int i = lane; i < n; i += 64) {
      const double p = lin[i];
      double dij = 0.0, dji = 0.0;
      if (j < 6 && i < 6) { dij = sD[i + 6 * j]; dji = sD[j + 6 * i]; }
      // the two products are written out so that element (i, j)'s second half is element (j, i)'s first half bit for bit
      const double sa = fma(sPH[2 * n + i], uj2, fma(sPH[n + i], uj1, sPH[i] * uj0));
      const double sb = fma(phj2, sU[2 * n + i], fma(phj1, sU[n + i], phj0 * sU[i]));
      const double va = (p + dij) - sa, vb = (p + dji) - sb;
      const double pn = 0.5 * (va + vb);                                      // ekf_dense.m:91-92
      lout[i] = pn;
      acc0 = fma(pn, sdy[i], acc0);
      acc1 = fma(pn, sdy[n + i], acc1);
      acc2 = fma(pn, sdy[2 * n + i], acc2);
    }
    acc0 = wave_sum(acc0); acc1 = wave_sum(acc1); acc2 = wave_sum(acc2);
    if (lane == 0) {
      a.PHacc[b3n + j] = acc0;
      a.PHacc[b3n + n + j] = acc1;
      a.PHacc[b3n + 2 * (size_t)n + j] = acc2;
    }
  }
}

static hipError_t launch_ekf_gain(const EkfGainArgs& a, int B, hipStream_t s) {
  static std::atomic<uint64_t> done{0};
  const size_t lds = ekf_gain_lds_bytes(a.n, a.ktmax);
  hipError_t e;
  if ((e = lds_opt_in((const void*)ekf_gain_kernel, (int)lds, done)) != hipSuccess) return e;
  hipLaunchKernelGGL(ekf_gain_kernel, dim3(B), dim3(256), lds, s, a);
  return hipGetLastError();
}

static hipError_t launch_ekf_update(const EkfUpdArgs& a, int B, hipStream_t s) {
  static std::atomic<uint64_t> done{0};
  const size_t lds = ekf_update_lds_bytes(a.n);
  hipError_t e;
  if ((e = lds_opt_in((const void*)ekf_update_kernel, (int)lds, done)) != hipSuccess) return e;
  hipLaunchKernelGGL(ekf_update_kernel, dim3((a.n + kEkfTile - 1) / kEkfTile, B), dim3(256), lds, s, a);
  return hipGetLastError();
}

// ---- host side -----------------------------------------------------------------------------------------------------------
template <typename T>
static int ekf_size_ok(const T* p, const char* name) {
  if (!p) { set_error(std::string(name) + " is NULL"); return RBPF_ERR_INVALID_ARG; }
  if (p->struct_size != 0 && p->struct_size != (int32_t)sizeof(T)) {
    set_error(std::string(name) + ".struct_size = " + std::to_string(p->struct_size) + ", this library's has " + std::to_string(sizeof(T)) +
              " bytes: rebuild the binding against include/rbpf.h");
    return RBPF_ERR_INVALID_ARG;
  }
  return RBPF_OK;
}

static int ekf_validate(const rbpf_ekf_problem* p, const rbpf_options* opt) {
  RB_TRY(ekf_size_ok(p, "rbpf_ekf_problem"));
  RB_TRY(options_ok(opt));
  if (p->n_runs < 1 || p->N_T < 1) { set_error("rbpf_ekf_problem: n_runs and N_T must be >= 1"); return RBPF_ERR_INVALID_ARG; }
  if (p->n_runs > 65535) { set_error("rbpf_ekf_problem: more than 65535 runs in one call are not supported"); return RBPF_ERR_UNSUPPORTED; }
  if (!p->models) { set_error("rbpf_ekf_problem: models is NULL"); return RBPF_ERR_INVALID_ARG; }
  for (int b = 0; b < p->n_runs; ++b) {
    const rbpf_model* md = p->models[b];
    if (!md) { set_error("rbpf_ekf_problem: models[" + std::to_string(b) + "] is NULL"); return RBPF_ERR_INVALID_ARG; }
    if (md->kind != RBPF_MODEL_DENSE_MAG_6D) {
      set_error("rbpf_ekf_dense: the EKF baseline exists for the dense-mag family only (RBPF_MODEL_DENSE_MAG_6D; the reference has no "
                "EKF for the other families)");
      return RBPF_ERR_UNSUPPORTED;
    }
    if (md->m_basis != p->models[0]->m_basis) { set_error("rbpf_ekf_problem: every model of a batch must have the same m_basis"); return RBPF_ERR_INVALID_ARG; }
  }
  const int nl = p->models[0]->m_basis + 3;
  if (p->models[0]->m_basis < 1 || nl > kEkfMaxNLin) { set_error("rbpf_ekf_problem: nLin = m_basis + 3 must be in 4 .. 1151"); return RBPF_ERR_INVALID_ARG; }
  if (!p->y || !p->x0 || !p->q0 || !p->P0 || !p->R || !p->Q || !p->dt || !p->LL) { set_error("rbpf_ekf_problem: a required array is NULL"); return RBPF_ERR_INVALID_ARG; }
  if (p->N_T > 1 && (!p->odometry || p->odo_ld < p->N_T - 1)) { set_error("odometry must be [>= N_T-1 x 7] per run"); return RBPF_ERR_INVALID_ARG; }
  if (p->q_pages != 1 && p->q_pages < p->N_T - 1) { set_error("Q must have 1 or >= N_T-1 pages"); return RBPF_ERR_INVALID_ARG; }
  if (p->dt_len != 1 && p->dt_len < p->N_T - 1) { set_error("dt must have 1 or >= N_T-1 entries"); return RBPF_ERR_INVALID_ARG; }
  return RBPF_OK;
}

static int ekf_qt_pages(const rbpf_ekf_problem* p) { return (p->q_pages > 1 || p->dt_len > 1) ? std::max(p->N_T - 1, 1) : 1; }

static size_t ekf_bytes(const rbpf_ekf_problem* p) {
  const size_t B = p->n_runs, T = p->N_T, m = p->models[0]->m_basis, n = m + 9, n2 = n * n;
  size_t d = (p->keep_P ? B * n2 + B * T * n2 : B * n2);                      // P (and its history)
  d += B * (n + 4 + 3 * n + 3 + 72 + 9 * n);                                  // x, q, dy, yhat, D, PHacc / PH / U
  d += B * (std::max<size_t>(T - 1, 1) * 7 + T * 3 + 9) + (size_t)ekf_qt_pages(p) * 36;   // odometry, y, R, dt Q
  d += B * T * (n + 4);                                                       // trajectories
  return d * sizeof(double) + B * (sizeof(int) + sizeof(EkfRunDev) + 3 * m * sizeof(int));
}

static int ekf_run(const rbpf_ekf_problem* p, rbpf_ekf_out* out) {
  const int B = p->n_runs, T = p->N_T, m = p->models[0]->m_basis, n = m + 9;
  const size_t n2 = (size_t)n * n;
  // host-side packing and the checks that need the data
  std::vector<EkfRunDev> runs((size_t)B);
  std::vector<int> nn_all((size_t)B * 3 * m);
  int ktmax = 0;
  for (int b = 0; b < B; ++b) {
    ModelDev M;
    std::vector<int> nn;
    RB_TRY(fill_model_dev(p->models[b], 7, m + 3, 3, 6, 7, nullptr, 0.0, M, nn));
    EkfRunDev& r = runs[(size_t)b];
    for (int a = 0; a < 3; ++a) {
      r.L[a] = M.L[a]; r.kmax[a] = M.kmax[a];
      r.lo[a] = p->LL[(size_t)b * 6 + 2 * a]; r.up[a] = p->LL[(size_t)b * 6 + 2 * a + 1];
      if (!(r.up[a] > r.lo[a])) { set_error("rbpf_ekf_problem: LL must hold lower < upper bounds per axis"); return RBPF_ERR_INVALID_ARG; }
    }
    r.ktot = M.ktot; r.NN = nullptr;
    ktmax = std::max(ktmax, M.ktot);
    std::copy(nn.begin(), nn.end(), nn_all.begin() + (size_t)b * 3 * m);
  }
  if (std::max(ekf_gain_lds_bytes(n, ktmax), ekf_update_lds_bytes(n)) > (size_t)kEkfLdsLimit) {
    set_error("rbpf_ekf_dense: the per-axis index range of NN (" + std::to_string(ktmax) + " table entries) does not fit the gain kernel's LDS");
    return RBPF_ERR_UNSUPPORTED;
  }
  for (int b = 0; b < B; ++b) {                                               // the update pass reads P(i,j) for P(j,i)
    const double* P0 = p->P0 + (size_t)b * n2;
    for (int j = 0; j < n; ++j)
      for (int i = j + 1; i < n; ++i)
        if (P0[i + (size_t)n * j] != P0[j + (size_t)n * i]) { set_error("rbpf_ekf_problem: P0 must be symmetric (run " + std::to_string(b) + ")"); return RBPF_ERR_INVALID_ARG; }
  }
  const int pages = ekf_qt_pages(p);
  std::vector<double> Qt((size_t)pages * 36);
  for (int t = 0; t < pages; ++t)
    for (int k = 0; k < 36; ++k) Qt[(size_t)t * 36 + k] = p->dt[p->dt_len > 1 ? t : 0] * p->Q[(size_t)(p->q_pages > 1 ? t : 0) * 36 + k];
  const int To = std::max(T - 1, 1);
  std::vector<double> yy((size_t)B * T * 3), oo((size_t)B * To * 7, 0.0);
  for (int b = 0; b < B; ++b) {
    for (int t = 0; t < T; ++t) for (int k = 0; k < 3; ++k) yy[((size_t)b * T + t) * 3 + k] = p->y[(size_t)b * T * 3 + t + (size_t)T * k];
    for (int t = 0; t + 1 < T; ++t)
      for (int k = 0; k < 7; ++k) oo[((size_t)b * To + t) * 7 + k] = p->odometry[(size_t)b * p->odo_ld * 7 + t + (size_t)p->odo_ld * k];
  }

  if (!have_device()) { set_error("no HIP device: the device EKF has no CPU fallback"); return RBPF_ERR_NO_DEVICE; }
  {
    size_t fr = 0, tot = 0;
    HIPCHK(hipMemGetInfo(&fr, &tot));
    const size_t need = ekf_bytes(p);
    if (need > fr) {
      set_error("rbpf_ekf_dense: the workspace of " + std::to_string(need) + " bytes does not fit the device (" + std::to_string(fr) +
                " free)" + (p->keep_P ? ": keep_P = 1 holds n^2 N_T doubles per run" : ""));
      return RBPF_ERR_OUT_OF_MEMORY;
    }
  }
  DevicePool pool;                                                            // freed on every return below
  EkfRunDev* d_runs = nullptr;
  int *d_nn = nullptr, *d_status = nullptr;
  double *d_P = nullptr, *d_hist = nullptr, *d_x = nullptr, *d_q = nullptr, *d_dy = nullptr, *d_yhat = nullptr, *d_D = nullptr;
  double *d_PHacc = nullptr, *d_PH = nullptr, *d_U = nullptr, *d_odo = nullptr, *d_y = nullptr, *d_R = nullptr, *d_Qt = nullptr;
  double *d_xf = nullptr, *d_qnb = nullptr;
  RB_TRY(pool.upload(&d_nn, nn_all.data(), nn_all.size()));
  for (int b = 0; b < B; ++b) runs[(size_t)b].NN = d_nn + (size_t)b * 3 * m;
  RB_TRY(pool.upload(&d_runs, runs.data(), runs.size()));
  RB_TRY(pool.upload(&d_P, p->P0, (size_t)B * n2));
  if (p->keep_P) RB_TRY(pool.alloc(&d_hist, (size_t)B * T * n2));
  RB_TRY(pool.upload(&d_x, p->x0, (size_t)B * n));
  RB_TRY(pool.upload(&d_q, p->q0, (size_t)B * 4));
  RB_TRY(pool.alloc(&d_dy, (size_t)B * 3 * n));
  RB_TRY(pool.alloc(&d_yhat, (size_t)B * 3));
  RB_TRY(pool.alloc(&d_D, (size_t)B * 72));
  RB_TRY(pool.alloc(&d_PHacc, (size_t)B * 3 * n));
  RB_TRY(pool.alloc(&d_PH, (size_t)B * 3 * n));
  RB_TRY(pool.alloc(&d_U, (size_t)B * 3 * n));
  RB_TRY(pool.upload(&d_odo, oo.data(), oo.size()));
  RB_TRY(pool.upload(&d_y, yy.data(), yy.size()));
  RB_TRY(pool.upload(&d_R, p->R, (size_t)B * 9));
  RB_TRY(pool.upload(&d_Qt, Qt.data(), Qt.size()));
  RB_TRY(pool.alloc(&d_xf, (size_t)B * T * n));
  RB_TRY(pool.alloc(&d_qnb, (size_t)B * T * 4));
  RB_TRY(pool.alloc(&d_status, (size_t)B));
  HIPCHK(hipMemset(d_status, 0, (size_t)B * sizeof(int)));
  HIPCHK(hipMemset(d_D, 0, (size_t)B * 72 * sizeof(double)));
  HIPCHK(hipMemset(d_PH, 0, (size_t)B * 3 * n * sizeof(double)));
  HIPCHK(hipMemset(d_U, 0, (size_t)B * 3 * n * sizeof(double)));

  EkfGainArgs g;
  g.n = n; g.m = m; g.T = T; g.ktmax = ktmax; g.runs = d_runs;
  g.x = d_x; g.q = d_q; g.dy = d_dy; g.yhat = d_yhat; g.D = d_D; g.PHacc = d_PHacc; g.PH = d_PH; g.U = d_U;
  g.odo = d_odo; g.y = d_y; g.R = d_R; g.Qt = d_Qt; g.qt_pages = pages;
  g.xf_traj = d_xf; g.qnb_traj = d_qnb; g.status = d_status;
  EkfUpdArgs u;
  u.n = n; u.PH = d_PH; u.U = d_U; u.dy = d_dy; u.PHacc = d_PHacc;
  // before step 0: dy_0 from (x0, q0), then PH_0 = P0 dy_0' by an update pass with PH = U = 0 (it stores P0 back unchanged)
  g.t = -1;
  HIPCHK(launch_ekf_gain(g, B, 0));
  u.Pin = d_P; u.pin_stride = n2; u.Pout = d_P; u.pout_stride = n2; u.D = nullptr; u.dslot = 0;
  HIPCHK(launch_ekf_update(u, B, 0));
  for (int t = 0; t < T; ++t) {
    g.t = t;
    HIPCHK(launch_ekf_gain(g, B, 0));
    if (p->keep_P) {                                                          // page t-1 -> page t of the history [n x n x N_T x B]
      u.Pin = t == 0 ? d_P : d_hist + (size_t)(t - 1) * n2;
      u.pin_stride = t == 0 ? n2 : (size_t)T * n2;
      u.Pout = d_hist + (size_t)t * n2; u.pout_stride = (size_t)T * n2;
    }
    u.D = d_D; u.dslot = t & 1;
    HIPCHK(launch_ekf_update(u, B, 0));
  }
  HIPCHK(hipDeviceSynchronize());
  std::vector<int> status((size_t)B);
  HIPCHK(hipMemcpy(status.data(), d_status, (size_t)B * sizeof(int), hipMemcpyDeviceToHost));
  for (int b = 0; b < B; ++b)
    if (status[(size_t)b]) {
      set_error("rbpf_ekf_dense: run " + std::to_string(b) + ", step " + std::to_string(status[(size_t)b] - 1) +
                ": Cholesky of the innovation covariance failed twice (matrix must be positive definite)");
      return RBPF_ERR_CHOL_FAILED;
    }
  if (out->xf_traj) HIPCHK(hipMemcpy(out->xf_traj, d_xf, (size_t)B * T * n * sizeof(double), hipMemcpyDeviceToHost));
  if (out->qnb_traj) HIPCHK(hipMemcpy(out->qnb_traj, d_qnb, (size_t)B * T * 4 * sizeof(double), hipMemcpyDeviceToHost));
  if (out->Pf) HIPCHK(hipMemcpy(out->Pf, p->keep_P ? d_hist : d_P, (size_t)B * (p->keep_P ? T : 1) * n2 * sizeof(double), hipMemcpyDeviceToHost));
  return RBPF_OK;
}

}  // namespace rbpf

using namespace rbpf;

extern "C" {

int rbpf_ekf_workspace_bytes(const rbpf_ekf_problem* prob, const rbpf_options* opt, size_t* bytes) {
  if (!bytes) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  RB_TRY(ekf_validate(prob, opt));
  *bytes = ekf_bytes(prob);
  return RBPF_OK;
}

int rbpf_ekf_dense(const rbpf_ekf_problem* prob, const rbpf_options* opt, rbpf_ekf_out* out) {
  RB_TRY(ekf_validate(prob, opt));
  RB_TRY(ekf_size_ok(out, "rbpf_ekf_out"));
  return ekf_run(prob, out);
}

}  // extern "C"
