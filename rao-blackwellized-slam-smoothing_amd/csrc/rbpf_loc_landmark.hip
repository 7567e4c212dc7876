// Localisation in the fixed landmark map of an arbitrary device-code model: particleFilter.m:100-161 with the sparseFeatures
// branch of :127-137, xl = mean and P = V'V (V lower n x n, the DenseMagMap convention) the same for every particle and never
// updated (:163-204 left out).  The caller's measModel hands over yhat_i [n_y] and H_i = dy(i,:,:) [n_y x n]; with
// ind = ~isnan(y(t,:)), M = |ind| (the same for every particle of a step), per particle
//     e = y_t(ind)' - yhat_i(ind),   S = (V H_i(ind,:)')'(V H_i(ind,:)') + R(ind,ind),
//     logw = -sum log diag chol S - |chol(S) \ e|^2 / 2 - M log(2 pi) / 2                                      (:129-136,145-150)
// (the jitter retry of :145-148 cannot trigger: S is a Gram matrix plus a principal submatrix of a positive definite R, checked at
// creation).  mean is never read here: the prediction is the handle's.  Rows of yhat / dy of outputs that are not observed are
// never loaded.
//
// loc_landmark_weights_kernel<NRT, NCT, VEC> is the hot kernel, a sibling of loc_generic_weights_kernel (rbpf_loc_generic.hip) for
// n <= 96 = 16 NRT and M <= 32 = 16 NCT.  A workgroup of four waves serves kLmPB = 32 particles, a wave kLmPW = 8 of them one
// after the other, and nothing of a particle's arithmetic depends on the others or on where it stands in the launch:
//   * V goes to LDS once per workgroup, as the NRT (NRT + 1) / 2 tiles of 16 x 16 of its lower triangle (entries above the diagonal
//     and past n are zeros there), each tile in the A operand order of v_mfma_f64_16x16x4, so an operand is one conflict-free
//     ds_read_b64 of 64 consecutive doubles;
//   * Y = V H(ind,:)' [16 NRT x 16 NCT]: the observed rows are the columns, compacted (column m is output ind[m], the columns
//     from M on are zeros).  The B operand comes straight from memory: the four lanes that share a column read 4 consecutive doubles
//     each of one 128-byte piece of that row of the Jacobian (VEC: as one 32-byte load; rows that do not start on 32 bytes: four
//     8-byte loads), so a wave's load covers 16 whole pieces and every byte is read once; no LDS staging is needed, because which
//     k a lane supplies is free as long as A and B agree, and the V tiles are laid out to agree.  Row tile rt skips the k chunks right of its diagonal block.  Accumulators stay in registers;
//   * the Gram blocks with the accumulator trick of loc_generic_weights_kernel: register r of a finished result tile given as A and
//     B adds sum_k Y(4 r + k, i) Y(4 r + k, j) to a tile of Y'Y, no lane movement.  M > 16: tile 0 as A and tile 1 as B is the
//     off-diagonal block S(i, 16 + j);
//   * R(ind,ind) (pad: the identity, which adds log 1 = 0 and a zero residual) is added in the result map, where every lane keeps
//     its entries for the whole launch; S then passes through a wave-private LDS slab so that lane i holds row i, and the
//     Cholesky factor, the forward solve and the weight run right-looking in registers, columns broadcast by v_readlane.
#include "../../include/rbpf.h"
#include "rbpf_internal.hpp"
#include "rbpf_ctx.hpp"
#include "rbpf_loc_state.hpp"
#include "rbpf_timed_reps.hpp"
#include "rbpf_sparse.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

namespace rbpf {

constexpr int kLmMaxNy = 32, kLmMaxN = 96, kLmMaxNonlin = 8;
constexpr int kLmWaves = 4;                // waves per workgroup
constexpr int kLmPW = 8;                   // particles per wave
constexpr int kLmPB = kLmWaves * kLmPW;    // particles per workgroup
constexpr int kLmSP = 33;                  // row pitch of the S slab (doubles): lane i reads row i, 66 i mod 64 banks are distinct

struct LocLmArgs {
  int n, npart, ld, ny, M;       // nLin, particles, row stride of H in doubles, outputs, observed outputs (1 .. 32)
  const double* H;               // H_i(k, c) at H[((size_t)i * ny + k) * ld + c], c < n
  const double* yhat;            // yhat_i(k) at yhat[i * yhat_si + k * yhat_sk]
  size_t yhat_si, yhat_sk;
  const double* V;               // [n x n] column-major lower factor
  const double* R;               // [ny x ny] column-major
  const double* y;               // [ny]
  const int* ind;                // [32]: the observed outputs ascending, entries from M on are not read
  double* S;                     // [npart][M x M] column-major, H(ind,:) P H(ind,:)' before R is added, or null
  double* logw;                  // [npart] or null
};

typedef double lm_v4d __attribute__((ext_vector_type(4)));

__device__ __forceinline__ double lm_readlane(double v, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}

template <int NRT, int NCT, bool VEC>
__global__ __launch_bounds__(64 * kLmWaves) __attribute__((amdgpu_waves_per_eu(VEC ? 2 : 1))) void loc_landmark_weights_kernel(const LocLmArgs a) {
  constexpr int NT = NRT * (NRT + 1) / 2;  // tiles of the lower triangle; tile (rt, kt), kt <= rt, is number rt (rt + 1) / 2 + kt
  constexpr int MP = 16 * NCT;             // M padded
  __shared__ double Vt[NT * 256];          // tile element (ks, ak, ar) at ks 64 + ak 16 + ar: V(16 rt + ar, 16 kt + k(ks, ak))
  __shared__ double Sb[kLmWaves][MP * kLmSP];
  const int n = a.n, M = a.M;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int arow = lane & 15, ak = lane >> 4;            // MFMA operand maps: A row / B column = lane & 15, k slot = lane >> 4
  // the k that operand slot (ks, ak) of a 16-chunk stands for: a lane supplies 4 consecutive k, so that it reads 32 consecutive
  // bytes of its row (VEC: in one load).  One map for both ways of loading: the sums do not depend on how the operands arrive
  auto kof = [](int ks, int kq) { return 4 * kq + ks; };

  for (int idx = tid; idx < NT * 256; idx += 64 * kLmWaves) {
    const int tl = idx >> 8, el = idx & 255;
    int rt = 0;
    while ((rt + 1) * (rt + 2) / 2 <= tl) ++rt;
    const int kt = tl - rt * (rt + 1) / 2;
    const int row = 16 * rt + (el & 15), k = 16 * kt + kof(el >> 6, (el >> 4) & 3);
    const double v = a.V[(size_t)min(k, n - 1) * n + min(row, n - 1)];   // (clamped: the address is valid whether it is used or not)
    Vt[idx] = (k <= row && row < n) ? v : 0.0;
  }

  // column arow of column tile ct is output ind[16 ct + arow]; R(ind,ind) in the result map: entry (i, j) of a tile is in register
  // r of lane l with i = (l >> 4) + 4 r, j = l & 15.  Of the off-diagonal block the entry S(16 + j, i) of the lower triangle.
  int rowc[NCT];
  bool cok[NCT];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) {
    const int m = 16 * ct + arow;
    cok[ct] = m < M;
    rowc[ct] = a.ind[cok[ct] ? m : 0];
  }
  double Rd[NCT][4], Ro[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = ak + 4 * r;
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
      const int mi = 16 * ct + i;
      const int oi = a.ind[mi < M ? mi : 0];
      const double v = a.R[oi + (size_t)a.ny * rowc[ct]];
      Rd[ct][r] = (mi < M && cok[ct]) ? v : (i == arow ? 1.0 : 0.0);
    }
    if (NCT == 2) {
      const int oi = a.ind[i < M ? i : 0];
      const double v = a.R[rowc[NCT - 1] + (size_t)a.ny * oi];
      Ro[r] = (i < M && cok[NCT - 1]) ? v : 0.0;
    }
  }
  // the residual's row of lane i < M
  const bool eok = lane < M;
  const int erow = a.ind[eok ? lane : 0];
  const double ye = a.y[erow];
  __syncthreads();

  double* Sw = Sb[wv];
  const int pbase = blockIdx.x * kLmPB + wv * kLmPW;
  for (int pi = 0; pi < kLmPW; ++pi) {
    const int p = pbase + pi;                              // (wave-uniform)
    if (p >= a.npart) break;
    const double* hb[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) hb[ct] = a.H + ((size_t)p * a.ny + rowc[ct]) * (size_t)a.ld;
    const double yh = a.yhat[(size_t)p * a.yhat_si + (size_t)erow * a.yhat_sk];

    lm_v4d acc[NRT][NCT];
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt)
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) acc[rt][ct] = (lm_v4d){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kt = 0; kt < NRT; ++kt) {
      double b[NCT][4];
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) {
        if (VEC) {
          // (the load may reach up to 3 doubles past n, inside the row's stride: those are selected away, never summed)
          const int k4 = 16 * kt + 4 * ak;
          const lm_v4d h = *reinterpret_cast<const lm_v4d*>(hb[ct] + min(k4, ((n + 3) & ~3) - 4));
          const bool in = k4 < n;
          b[ct][0] = (cok[ct] && in) ? h.x : 0.0;
          b[ct][1] = (cok[ct] && in && k4 + 1 < n) ? h.y : 0.0;
          b[ct][2] = (cok[ct] && in && k4 + 2 < n) ? h.z : 0.0;
          b[ct][3] = (cok[ct] && in && k4 + 3 < n) ? h.w : 0.0;
        } else {
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) {
            const int k = 16 * kt + kof(ks, ak);
            const double h = hb[ct][min(k, n - 1)];
            b[ct][ks] = (cok[ct] && k < n) ? h : 0.0;
          }
        }
      }
#pragma unroll
      for (int rt = kt; rt < NRT; ++rt) {
        const double* At = Vt + (rt * (rt + 1) / 2 + kt) * 256 + lane;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const double av = At[ks * 64];
#pragma unroll
          for (int ct = 0; ct < NCT; ++ct) acc[rt][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, b[ct][ks], acc[rt][ct], 0, 0, 0);
        }
      }
    }

    // Gram tiles.  Result map: column = lane & 15, row = (lane >> 4) + 4 reg, so register r as both operands is
    // A(i, k) = Y(4 r + k, i), B(k, j) = Y(4 r + k, j)
    lm_v4d gd[NCT], go = (lm_v4d){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) gd[ct] = (lm_v4d){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) gd[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(acc[rt][ct][r], acc[rt][ct][r], gd[ct], 0, 0, 0);
        if (NCT == 2) go = __builtin_amdgcn_mfma_f64_16x16x4f64(acc[rt][0][r], acc[rt][NCT - 1][r], go, 0, 0, 0);
      }

    if (a.S) {                                             // (the probe's output; entries (r, c) and (c, r) are the same sums)
      double* So = a.S + (size_t)p * M * M;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = ak + 4 * r;
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
          if (16 * ct + i < M && cok[ct]) So[(16 * ct + i) + (size_t)M * (16 * ct + arow)] = gd[ct][r];
        if (NCT == 2 && i < M && cok[NCT - 1]) {
          So[i + (size_t)M * (16 + arow)] = go[r];
          So[(16 + arow) + (size_t)M * i] = go[r];
        }
      }
    }
    if (!a.logw) continue;

    // S + R into the slab's lower triangle, then row i to lane i
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = ak + 4 * r;
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) Sw[(16 * ct + i) * kLmSP + 16 * ct + arow] = gd[ct][r] + Rd[ct][r];
      if (NCT == 2) Sw[(16 + arow) * kLmSP + i] = go[r] + Ro[r];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int li = min(lane, MP - 1);
    double s[MP];
#pragma unroll
    for (int c = 0; c < MP; ++c) s[c] = Sw[li * kLmSP + c];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();

    // right-looking Cholesky of the MP x MP matrix, row li on the lane (entries right of the diagonal are never used), with the
    // forward solve z = chol(S) \ e carried along as one more column; every sum in the order of the column index.  The chain from
    // one column to the next is one reciprocal square root: lane j keeps its diagonal entry, and the logarithms are taken once,
    // on all lanes together, after the last column
    double e = eok ? ye - yh : 0.0;
    double zz = 0.0, dsave = 1.0;
#pragma unroll
    for (int j = 0; j < MP; ++j) {
      const double inv = rsqrt(lm_readlane(s[j], j));
      const double lij = s[j] * inv;                       // L(i, j) on the lanes i > j; on lane j: L(j, j)
      if (lane == j) dsave = lij;
      const double zj = lm_readlane(e, j) * inv;
      zz = fma(zj, zj, zz);
      e = fma(-lij, zj, e);
#pragma unroll
      for (int k = j + 1; k < MP; ++k) s[k] = fma(-lij, lm_readlane(lij, k), s[k]);
    }
    const double lg = log(dsave);
    double logdet = 0.0;
#pragma unroll
    for (int j = 0; j < MP; ++j) logdet += lm_readlane(lg, j);
    if (lane == 0) a.logw[p] = -logdet - 0.5 * zz - 0.5 * (double)M * 1.8378770664093454835606594728112;   // log(2 pi)
  }
}

template <int NRT, int NCT>
static hipError_t launch_lm2(const LocLmArgs& a, hipStream_t s) {
  // the 32-byte loads need rows that start on 32 bytes and a stride that holds n rounded up to 4
  const bool vec = a.ld % 4 == 0 && a.ld >= ((a.n + 3) & ~3) && (reinterpret_cast<uintptr_t>(a.H) & 31) == 0;
  const dim3 grid((a.npart + kLmPB - 1) / kLmPB), block(64 * kLmWaves);
  if (vec) hipLaunchKernelGGL((loc_landmark_weights_kernel<NRT, NCT, true>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((loc_landmark_weights_kernel<NRT, NCT, false>), grid, block, 0, s, a);
  return hipGetLastError();
}

template <int NCT>
static hipError_t launch_lm1(const LocLmArgs& a, hipStream_t s) {
  switch ((a.n + 15) / 16) {
    case 1: return launch_lm2<1, NCT>(a, s);
    case 2: return launch_lm2<2, NCT>(a, s);
    case 3: return launch_lm2<3, NCT>(a, s);
    case 4: return launch_lm2<4, NCT>(a, s);
    case 5: return launch_lm2<5, NCT>(a, s);
    case 6: return launch_lm2<6, NCT>(a, s);
    default: return hipErrorInvalidValue;
  }
}

// M = 0: every log-weight is 0 (the bytes of 0.0 are zeros); otherwise the kernel of ceil(n / 16) and ceil(M / 16)
static hipError_t launch_loc_landmark_weights(const LocLmArgs& a, hipStream_t s) {
  if (a.M == 0) return a.logw ? hipMemsetAsync(a.logw, 0, (size_t)a.npart * sizeof(double), s) : hipSuccess;
  if (a.M < 0 || a.M > kLmMaxNy || a.n < 1) return hipErrorInvalidValue;
  return a.M <= 16 ? launch_lm1<1>(a, s) : launch_lm1<2>(a, s);
}

// ---- host side -----------------------------------------------------------------------------------------------------------
static int lm_validate_sizes(int n_nonlin, int n_y, int n_lin) {
  if (n_nonlin < 1 || n_y < 1 || n_lin < 1) { set_error("n_nonlin, n_y and n_lin must be >= 1"); return RBPF_ERR_INVALID_ARG; }
  if (n_y > kLmMaxNy) { set_error("localisation in a landmark map is built for n_y from 1 to 32"); return RBPF_ERR_UNSUPPORTED; }
  if (n_lin > kLmMaxN) { set_error("localisation in a landmark map is built for n_lin from 1 to 96"); return RBPF_ERR_UNSUPPORTED; }
  if (n_nonlin > kLmMaxNonlin) { set_error("localisation in a landmark map is built for n_nonlin from 1 to 8"); return RBPF_ERR_UNSUPPORTED; }
  return RBPF_OK;
}

static int lm_ctx_ok(const rbpf_ctx* c) {
  if (!c->loc || !c->loc->landmark) { set_error("not a landmark-map localisation context (rbpf_loc_landmark_create)"); return RBPF_ERR_STATE; }
  return RBPF_OK;
}

// the observed outputs of y [d] (element k at y[k * stride]), ascending, into ind[32]; returns how many
static int lm_observed(const double* y, size_t stride, int d, int* ind) {
  int M = 0;
  for (int k = 0; k < kLmMaxNy; ++k) ind[k] = 0;
  for (int k = 0; k < d; ++k)
    if (!std::isnan(y[k * stride])) ind[M++] = k;
  return M;
}

}  // namespace rbpf

using namespace rbpf;

extern "C" {

int rbpf_loc_landmark_create(int32_t n_nonlin, int32_t n_y, int32_t n_lin, const double* mean, const double* V, const double* R,
                             int32_t N_P, int32_t N_T, const double* y, const double* x0_nonlin, int32_t x0_cols,
                             const rbpf_rng* rng, const rbpf_options* opt, rbpf_ctx** out) {
  if (!out) { set_error("ctx out pointer is NULL"); return RBPF_ERR_INVALID_ARG; }
  *out = nullptr;
  if (!mean || !V || !R || !y || !x0_nonlin || !rng) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  RB_TRY(lm_validate_sizes(n_nonlin, n_y, n_lin));
  RB_TRY(loc_generic_validate_run(N_P, N_T, x0_cols, rng, opt));
  RB_TRY(lg_validate_R(R, n_y));
  if (!have_device()) { set_error("no HIP device: the localisation filter has no CPU fallback"); return RBPF_ERR_NO_DEVICE; }
  rbpf_ctx* c = nullptr;
  RB_TRY(loc_generic_build(n_nonlin, n_y, n_lin, mean, V, R, N_P, N_T, y, x0_nonlin, x0_cols, rng, opt, &c));
  std::unique_ptr<rbpf_ctx, void (*)(rbpf_ctx*)> guard(c, [](rbpf_ctx* p) { ctx_free(p); });
  LocState* L = c->loc;
  const int N = N_P, T = N_T, n = n_lin, d = n_y, ldx = L->ldx;
  L->landmark = true;
  // the observed outputs of every step; the NaN of y never reach a sum, the device copy of y is read at observed rows only
  std::vector<int> ind((size_t)T * kLmMaxNy);
  L->n_obs.resize(T);
  for (int t = 0; t < T; ++t) L->n_obs[t] = lm_observed(y + t, (size_t)T, d, ind.data() + (size_t)t * kLmMaxNy);
  RB_TRY(L->pool.upload(&L->d_ind, ind.data(), ind.size()));
  {
    // xl for a sparse-feature measModel: the mean in every row, the pad zero; filled once, by the gather of the SLAM filter
    std::vector<double> row((size_t)ldx, 0.0);
    std::copy(mean, mean + n, row.begin());
    double* d_row = nullptr;
    RB_TRY(L->pool.upload(&d_row, row.data(), row.size()));
    RB_TRY(L->pool.alloc(&L->d_xl, (size_t)N * ldx));
    HIPCHK(launch_sparse_ext_gather_xl(N, ldx, d_row, 0, nullptr, L->d_xl, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    L->pool.release(d_row);
  }
  {
    std::vector<double> nans((size_t)T * d, std::numeric_limits<double>::quiet_NaN());
    RB_TRY(c->pool.upload(&c->d_yhattraj, nans.data(), nans.size()));
  }
  guard.release();
  *out = c;
  return RBPF_OK;
}

int rbpf_loc_landmark_map_device(rbpf_ctx* c, const double** xl_dev, int32_t* ldx) {
  if (!c || !xl_dev || !ldx) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  RB_TRY(lm_ctx_ok(c));
  *xl_dev = c->loc->d_xl;
  *ldx = c->loc->ldx;
  return RBPF_OK;
}

int rbpf_loc_landmark_step_device(rbpf_ctx* c, const double* xn_new_dev, const double* yhat_dev, int32_t yhat_layout,
                                  const double* dy_dev, int32_t dy_layout) {
  if (!c || !xn_new_dev || !yhat_dev || !dy_dev) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  if (yhat_layout != 0 && yhat_layout != 2) { set_error("yhat_layout must be 0 (MATLAB order) or 2 (C-contiguous)"); return RBPF_ERR_INVALID_ARG; }
  if (dy_layout < 0 || dy_layout > 2) { set_error("dy_layout must be 0 (MATLAB order), 1 (rows on the stride ldx) or 2 (C-contiguous)"); return RBPF_ERR_INVALID_ARG; }
  RB_TRY(lm_ctx_ok(c));
  LocState* L = c->loc;
  const int t = c->t, N = c->N, nN = L->nN, n = L->n, d = L->d;
  if (t >= c->T) { set_error("advance past N_T"); return RBPF_ERR_STATE; }
  if (t > 0 && L->drawn_step != t) { set_error("no ancestors drawn for this step (rbpf_loc_generic_ancestors_device first)"); return RBPF_ERR_STATE; }
  HIPCHK(hipSetDevice(c->device));
  const bool hist = c->opt.keep_history != 0;
  double* X_new = c->X + (size_t)(hist ? t : (t & 1)) * nN * N;
  HIPCHK(launch_ext_states_to_soa(N, nN, xn_new_dev, X_new, c->stream));
  LocLmArgs a;
  a.n = n; a.npart = N; a.ny = d; a.M = L->n_obs[t];
  if (dy_layout == 0) {                                   // the lines of one particle lie N_P doubles apart: pack them into rows first
    if (!L->d_H) RB_TRY(L->pool.alloc(&L->d_H, (size_t)N * d * L->ldx));
    HIPCHK(launch_ext_pack_dy(0, N, d, n, L->ldx, dy_dev, L->d_H, c->stream));
    a.H = L->d_H; a.ld = L->ldx;
  } else {
    a.H = dy_dev; a.ld = dy_layout == 1 ? L->ldx : n;
  }
  a.yhat = yhat_dev; a.yhat_si = yhat_layout == 0 ? 1 : (size_t)d; a.yhat_sk = yhat_layout == 0 ? (size_t)N : 1;
  a.V = L->d_V; a.R = L->d_R; a.y = c->d_y + (size_t)t * d; a.ind = L->d_ind + (size_t)t * kLmMaxNy;
  a.S = nullptr; a.logw = c->logw + (c->opt.trace ? (size_t)t * N : 0);
  HIPCHK(launch_loc_landmark_weights(a, c->stream));
  RB_TRY(loc_generic_normalise_step(c, X_new));
  HIPCHK(launch_sparse_ext_yhat_of_max(d, yhat_dev, a.yhat_si, a.yhat_sk, c->d_flags + 2, c->d_yhattraj + (size_t)t * d, c->stream));
  c->t = t + 1;
  if (!c->opt.on_step) return RBPF_OK;
  HIPCHK(hipStreamSynchronize(c->stream));              // the hook sees a finished step
  return ctx_call_on_step(c, t, false);
}

int rbpf_loc_landmark_yhattraj(rbpf_ctx* c, double* yhattraj) {
  if (!c || !yhattraj) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  RB_TRY(lm_ctx_ok(c));
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(yhattraj, c->d_yhattraj, (size_t)c->T * c->loc->d * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return RBPF_OK;
}

int rbpf_loc_landmark_weights(int32_t n_y, int32_t n_lin, int32_t n_p, const double* yhat, int32_t yhat_layout, const double* dy,
                              int32_t dy_layout, int32_t ldx, const double* V, const double* R, const double* y, double* S,
                              double* logw, int32_t reps, double* ms) {
  if (!yhat || !dy || !V || !R || !y) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  if (yhat_layout != 0 && yhat_layout != 2) { set_error("yhat_layout must be 0 (MATLAB order) or 2 (C-contiguous)"); return RBPF_ERR_INVALID_ARG; }
  if (dy_layout < 0 || dy_layout > 2) { set_error("dy_layout must be 0 (MATLAB order), 1 (rows on the stride ldx) or 2 (C-contiguous)"); return RBPF_ERR_INVALID_ARG; }
  RB_TRY(lm_validate_sizes(1, n_y, n_lin));
  if (n_p < 1 || n_p > kMaxParticles) { set_error("n_p must be in 1 .. 1048576"); return RBPF_ERR_INVALID_ARG; }
  if (dy_layout == 1 && ldx < n_lin) { set_error("ldx must be >= n_lin"); return RBPF_ERR_INVALID_ARG; }
  RB_TRY(lg_validate_R(R, n_y));
  if (!have_device()) { set_error("no HIP device"); return RBPF_ERR_NO_DEVICE; }
  const int n = n_lin, d = n_y, N = n_p;
  const int ld = dy_layout == 1 ? ldx : (dy_layout == 0 ? lg_ldx(n) : n);
  int ind[kLmMaxNy];
  const int M = lm_observed(y, 1, d, ind);
  DevicePool tmp;
  double *d_dy = nullptr, *d_H = nullptr, *d_yhat = nullptr, *d_V = nullptr, *d_R = nullptr, *d_y = nullptr, *d_S = nullptr, *d_logw = nullptr;
  int* d_ind = nullptr;
  RB_TRY(tmp.upload(&d_dy, dy, (size_t)N * d * (dy_layout == 1 ? ld : n)));
  RB_TRY(tmp.upload(&d_yhat, yhat, (size_t)N * d));
  RB_TRY(tmp.upload(&d_V, V, (size_t)n * n));
  RB_TRY(tmp.upload(&d_R, R, (size_t)d * d));
  RB_TRY(tmp.upload(&d_y, y, (size_t)d));
  RB_TRY(tmp.upload(&d_ind, (const int*)ind, (size_t)kLmMaxNy));
  RB_TRY(tmp.alloc(&d_S, (size_t)N * M * M));
  RB_TRY(tmp.alloc(&d_logw, (size_t)N));
  if (dy_layout == 0) {
    RB_TRY(tmp.alloc(&d_H, (size_t)N * d * ld));
    HIPCHK(launch_ext_pack_dy(0, N, d, n, ld, d_dy, d_H, 0));
  }
  LocLmArgs a;
  a.n = n; a.npart = N; a.ld = ld; a.ny = d; a.M = M; a.H = dy_layout == 0 ? d_H : d_dy;
  a.yhat = d_yhat; a.yhat_si = yhat_layout == 0 ? 1 : (size_t)d; a.yhat_sk = yhat_layout == 0 ? (size_t)N : 1;
  a.V = d_V; a.R = d_R; a.y = d_y; a.ind = d_ind; a.S = d_S; a.logw = d_logw;
  RB_TRY(timed_reps(reps, 0, [&] { return launch_loc_landmark_weights(a, 0); }, ms));
  if (S && M > 0) HIPCHK(hipMemcpy(S, d_S, (size_t)N * M * M * sizeof(double), hipMemcpyDeviceToHost));
  if (logw) HIPCHK(hipMemcpy(logw, d_logw, (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
  return RBPF_OK;
}

}  // extern "C"
