// Localisation in a fixed GP map (examples/mag-localization-mapping): particleFilterLocalization.m:84-132 with the closures of
// run_localization.m:241-281.  The particles carry 7 non-linear states and NO map state; the map posterior N(mean, V'V) is shared.
//
// loc_predict_kernel is the hot kernel.  One workgroup serves kLocPB = 64 particles = 192 columns (three gradient rows each):
//   * per-axis sin / cos tables of its particles in LDS (tools/domain_cartesian_dx.m:146-170, as basis_table_entry builds them);
//   * the gradient rows G_c(i) = row c of [e_c, d_c Phi(p_i)] generated from the tables in 16-deep k chunks into LDS, never
//     written to global memory; dEft = G mean as running dot products of the generating threads;
//   * var_c = |V G_c'|^2 on v_mfma_f64_16x16x4: Y = V G' in super-blocks of 128 rows (4 waves x 2 row tiles of 16 x 192, the
//     accumulators of a whole super-block live in registers), A operand = V read straight from global memory (lower triangle
//     only: the k chunks right of a row tile's diagonal block are skipped, entries above the diagonal masked), B operand = the
//     chunk in LDS.  The squares of a 16 x 16 result tile are summed after its full k sum.
// One pass over the lower triangle of V therefore serves 192 columns: 2 * 192 flop per 8-byte element = 48 flop / byte
// against L2 / Infinity Cache.  The chunks are regenerated once per super-block (4.5 x at n = 1003, ~10 % of the MFMA work).
#include "../../include/rbpf.h"
#include "rbpf_internal.hpp"
#include "rbpf_device.hpp"
#include "rbpf_ctx.hpp"
#include "rbpf_loc_state.hpp"
#include "rbpf_timed_reps.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace rbpf {

constexpr int kLocPB = 64;                 // particles per workgroup
constexpr int kLocCT = 3 * kLocPB / 16;    // column tiles of 16: column = c * 64 + particle
constexpr int kLocKC = 16;                 // k depth of a generated chunk
constexpr int kLocGS = 208;                // row pitch of a chunk in LDS (doubles): 416 dwords = 32 mod 64 banks, the four k rows of an operand read are conflict-free
constexpr int kLocRows = 128;              // rows of a super-block: 4 waves x 2 row tiles
constexpr int kLocRed = 4 * 3 * kLocPB;    // cross-wave reduction scratch (doubles)
constexpr int kLocMaxN = 1151;             // the library's largest nLin
constexpr int kLocLdsLimit = 160 * 1024;

struct LocArgs {
  ModelDev mdl;                  // kind, m, NN (axis-major, device), L, kmax, ktot
  int n, npart;
  const double* xn; size_t xn_cs, xn_ps;   // state c of particle p at xn[c * xn_cs + p * xn_ps]
  const double* mean;            // [n]
  const double* V;               // [n x n] column-major lower factor (kernel <true> only)
  const double* var_table;       // [npart x 3] column-major or null
  double sigma2;
  const double* y;               // [3]; null: no weights
  double* dEft; double* var;     // [3 x npart] or null
  double* logw;                  // [npart] or null
};

typedef double loc_v4d __attribute__((ext_vector_type(4)));

static size_t loc_lds_bytes(int ktot, bool with_v) {
  return ((size_t)2 * ktot * kLocPB + 2 * kLocRed + (with_v ? 2 * kLocKC * kLocGS : 0)) * sizeof(double);
}

// the three gradient entries of column k of [e_c, d_c Phi] for the particle whose tables are tS / tC (pitch kLocPB):
// H_column of rbpf_model_dev.hpp before the rotation, same order of evaluation
__device__ __forceinline__ void loc_grad(const ModelDev& M, int n, int k, const double* tS, const double* tC, double g[3]) {
  if (k >= n) { g[0] = 0.0; g[1] = 0.0; g[2] = 0.0; return; }
  if (k < 3) { g[0] = (k == 0); g[1] = (k == 1); g[2] = (k == 2); return; }
  const int j = k - 3;
  const int base[3] = {0, M.kmax[0], M.kmax[0] + M.kmax[1]};
  int nn[3];
  double sv[3], cv[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    nn[a] = M.NN[a * M.m + j];
    const int q = base[a] + nn[a] - 1;
    sv[a] = tS[q * kLocPB];
    cv[a] = tC[q * kLocPB];
  }
#pragma unroll
  for (int di = 0; di < 3; ++di) {
    double v = 1.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double La = M.L[a];
      if (a == di) v = v * RBPF_PI * (double)nn[a] / (2.0 * La * sqrt(La)) * cv[a];
      else v = v * 1.0 / sqrt(La) * sv[a];
    }
    g[di] = v;
  }
}

template <bool WITH_V>
__global__ __launch_bounds__(256) void loc_predict_kernel(const LocArgs a) {
  extern __shared__ double sm[];
  const ModelDev& M = a.mdl;
  const int kt = M.ktot, n = a.n;
  double* tabS = sm;                       // [kt][64]
  double* tabC = tabS + (size_t)kt * kLocPB;
  double* redE = tabC + (size_t)kt * kLocPB;   // [4][3][64] partial means
  double* redV = redE + kLocRed;           // [4][192] partial square sums
  double* Gb = redV + kLocRed;             // [2][16][kLocGS]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int slot = blockIdx.x * kLocPB + lane;
  const int sl = min(slot, a.npart - 1);   // lanes past the end recompute the last particle; nothing of theirs is stored

  // tables: lane = particle, wave = phase over the entries
  {
    double pos[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) pos[c] = a.xn[(size_t)c * a.xn_cs + (size_t)sl * a.xn_ps];
    for (int q = wv; q < kt; q += 4) {
      int ax = 0, k = q;
      if (k >= M.kmax[0]) { k -= M.kmax[0]; ax = 1; if (k >= M.kmax[1]) { k -= M.kmax[1]; ax = 2; } }
      const double La = M.L[ax];
      const double arg = RBPF_PI * (double)(k + 1) * (pos[ax] + La) / (2.0 * La);
      double s, c;
      sincos(arg, &s, &c);
      tabS[q * kLocPB + lane] = s;
      tabC[q * kLocPB + lane] = c;
    }
  }
  __syncthreads();
  const double* tS = tabS + lane;
  const double* tC = tabC + lane;

  double dE[3] = {0.0, 0.0, 0.0};
  if (!WITH_V) {
    for (int k = wv; k < n; k += 4) {
      double g[3];
      loc_grad(M, n, k, tS, tC, g);
      const double mk = a.mean[k];
#pragma unroll
      for (int c = 0; c < 3; ++c) dE[c] = fma(g[c], mk, dE[c]);
    }
  } else {
    double sq[kLocCT];
#pragma unroll
    for (int ct = 0; ct < kLocCT; ++ct) sq[ct] = 0.0;
    const int nsb = (n + kLocRows - 1) / kLocRows;
    const int arow = lane & 15, ak = lane >> 4;          // MFMA operand maps: A row / B column = lane & 15, k = lane >> 4
    int buf = 0;
    for (int sb = 0; sb < nsb; ++sb) {
      const bool last = (sb == nsb - 1);                 // the last super-block sees every k: the means are summed there
      const int kend = min(n, kLocRows * (sb + 1));
      const int nch = (kend + kLocKC - 1) / kLocKC;
      const int rt0 = sb * (kLocRows / 16) + wv * 2;     // this wave's first row tile
      const int row0 = rt0 * 16 + arow, row1 = row0 + 16;
      loc_v4d acc[2][kLocCT];
#pragma unroll
      for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int ct = 0; ct < kLocCT; ++ct) acc[x][ct] = (loc_v4d){0.0, 0.0, 0.0, 0.0};

      auto gen_chunk = [&](int kc, int b) {
        double* G = Gb + (size_t)b * kLocKC * kLocGS;
#pragma unroll
        for (int i = 0; i < kLocKC / 4; ++i) {
          const int kk = wv + 4 * i, k = kc * kLocKC + kk;
          double g[3];
          loc_grad(M, n, k, tS, tC, g);
#pragma unroll
          for (int c = 0; c < 3; ++c) G[kk * kLocGS + c * kLocPB + lane] = g[c];
          if (last && k < n) {
            const double mk = a.mean[k];
#pragma unroll
            for (int c = 0; c < 3; ++c) dE[c] = fma(g[c], mk, dE[c]);
          }
        }
      };
      // A operands of chunk kc: V(row, k) for k <= row < n, zero elsewhere (upper triangle, padding); the address is clamped
      auto load_a = [&](int kc, double av[4][2]) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const int k = kc * kLocKC + ks * 4 + ak;
          const int kcl = min(k, n - 1);
          const bool ok0 = (k <= row0) && (row0 < n), ok1 = (k <= row1) && (row1 < n);
          const double v0 = a.V[(size_t)kcl * n + min(row0, n - 1)];
          const double v1 = a.V[(size_t)kcl * n + min(row1, n - 1)];
          av[ks][0] = ok0 ? v0 : 0.0;
          av[ks][1] = ok1 ? v1 : 0.0;
        }
      };

      double a_cur[4][2], a_nxt[4][2];
      gen_chunk(0, buf);
      load_a(0, a_cur);
      __syncthreads();
      for (int kc = 0; kc < nch; ++kc) {
        const bool more = kc + 1 < nch;
        if (more) { load_a(kc + 1, a_nxt); gen_chunk(kc + 1, buf ^ 1); }
        // row tile x holds non-zeros of this chunk iff kc <= its tile index (wave-uniform)
        const bool act0 = (kc <= rt0) && (rt0 * 16 < n), act1 = (kc <= rt0 + 1) && ((rt0 + 1) * 16 < n);
        if (act1) {                                       // act0 implies act1 inside the matrix except past the last row
          const double* G = Gb + (size_t)buf * kLocKC * kLocGS + ak * kLocGS + arow;
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
            for (int ct = 0; ct < kLocCT; ++ct) {
              const double b = G[ks * 4 * kLocGS + ct * 16];
              if (act0) acc[0][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a_cur[ks][0], b, acc[0][ct], 0, 0, 0);
              acc[1][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a_cur[ks][1], b, acc[1][ct], 0, 0, 0);
            }
          }
        } else if (act0) {
          const double* G = Gb + (size_t)buf * kLocKC * kLocGS + ak * kLocGS + arow;
#pragma unroll
          for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int ct = 0; ct < kLocCT; ++ct)
              acc[0][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a_cur[ks][0], G[ks * 4 * kLocGS + ct * 16], acc[0][ct], 0, 0, 0);
        }
        __syncthreads();
        buf ^= 1;
        if (more) {
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) { a_cur[ks][0] = a_nxt[ks][0]; a_cur[ks][1] = a_nxt[ks][1]; }
        }
      }
      // the k sums of this super-block's tiles are complete: accumulate their squares (result map: col = lane & 15, rows 4 reg + lane >> 4)
#pragma unroll
      for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int ct = 0; ct < kLocCT; ++ct) {
          const loc_v4d v = acc[x][ct];
          sq[ct] += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
        }
    }
#pragma unroll
    for (int ct = 0; ct < kLocCT; ++ct) {
      double s = sq[ct];
      s += __shfl_xor(s, 16, 64);
      s += __shfl_xor(s, 32, 64);
      if (lane < 16) redV[wv * (3 * kLocPB) + ct * 16 + lane] = s;
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) redE[(wv * 3 + c) * kLocPB + lane] = dE[c];
  __syncthreads();
  if (tid >= kLocPB || slot >= a.npart) return;
  double e[3], var[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    e[c] = (redE[(0 * 3 + c) * kLocPB + lane] + redE[(1 * 3 + c) * kLocPB + lane]) + (redE[(2 * 3 + c) * kLocPB + lane] + redE[(3 * 3 + c) * kLocPB + lane]);
    if (WITH_V) {
      const int col = c * kLocPB + lane;
      var[c] = (redV[col] + redV[3 * kLocPB + col]) + (redV[2 * 3 * kLocPB + col] + redV[3 * 3 * kLocPB + col]);
    } else if (a.var_table) {
      var[c] = a.var_table[(size_t)c * a.npart + slot];
    }
    if (a.dEft) a.dEft[(size_t)slot * 3 + c] = e[c];
    if (a.var && WITH_V) a.var[(size_t)slot * 3 + c] = var[c];
  }
  if (!a.y || !a.logw) return;
  // run_localization.m:265-270: w = sum_c normpdf(y_c, (Rnb' dEft')_c, sqrt(var_c + sigma2)), here as a log-sum-exp
  double q[4], Rm[9], l[3];
#pragma unroll
  for (int c = 0; c < 4; ++c) q[c] = a.xn[(size_t)(3 + c) * a.xn_cs + (size_t)slot * a.xn_ps];
  quat2rmat_dev(q, Rm);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double mu = Rm[0 * 3 + k] * e[0] + Rm[1 * 3 + k] * e[1] + Rm[2 * 3 + k] * e[2];
    const double s2 = var[k] + a.sigma2;
    const double r = a.y[k] - mu;
    l[k] = -0.5 * (r * r / s2) - 0.5 * log(s2) - 0.918938533204672741780329736406;    // log(sqrt(2 pi))
  }
  const double mx = fmax(l[0], fmax(l[1], l[2]));
  a.logw[slot] = (mx == -INFINITY || mx != mx) ? mx : mx + log(exp(l[0] - mx) + exp(l[1] - mx) + exp(l[2] - mx));
}

static hipError_t launch_loc_predict(const LocArgs& a, hipStream_t s) {
  static std::atomic<uint64_t> done_v{0}, done_t{0};
  const bool with_v = a.V != nullptr;
  const size_t lds = loc_lds_bytes(a.mdl.ktot, with_v);
  const int nb = (a.npart + kLocPB - 1) / kLocPB;
  hipError_t e;
  if (with_v) {
    if ((e = lds_opt_in((const void*)loc_predict_kernel<true>, (int)lds, done_v)) != hipSuccess) return e;
    hipLaunchKernelGGL((loc_predict_kernel<true>), dim3(nb), dim3(256), lds, s, a);
  } else {
    if ((e = lds_opt_in((const void*)loc_predict_kernel<false>, (int)lds, done_t)) != hipSuccess) return e;
    hipLaunchKernelGGL((loc_predict_kernel<false>), dim3(nb), dim3(256), lds, s, a);
  }
  return hipGetLastError();
}

// ---- dynModel of run_localization.m:274-281 ------------------------------------------------------------------------------
// S: 6 x 6 column-major, S(r, c) = sqrt(dt Q(r, c)) element-wise on the two diagonal 3 x 3 blocks (full blocks, not factors)
__device__ inline void loc_dyn_model_dev(const double x[7], const double* odo, const double* S, const double z[6], double xp[7]) {
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    double s = 0.0;
    for (int c = 0; c < 3; ++c) s += S[r + 6 * c] * z[c];
    xp[r] = x[r] + odo[r] + s;                                                                   // :277
  }
  double phi[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    double s = 0.0;
    for (int c = 0; c < 3; ++c) s += S[(3 + r) + 6 * (3 + c)] * z[3 + c];
    phi[r] = s;
  }
  double eq[4];
  expq_dev(phi, eq);
  // qRight(q) * dq  (tools/qRight.m:29-34: [q0 -qv'; qv q0 I - [qv x]])
  const double* q = &x[3];
  const double p[4] = {odo[3], odo[4], odo[5], odo[6]};
  double r4[4];
  r4[0] = q[0] * p[0] + (-q[1]) * p[1] + (-q[2]) * p[2] + (-q[3]) * p[3];
  r4[1] = q[1] * p[0] + q[0] * p[1] + q[3] * p[2] + (-q[2]) * p[3];
  r4[2] = q[2] * p[0] + (-q[3]) * p[1] + q[0] * p[2] + q[1] * p[3];
  r4[3] = q[3] * p[0] + q[2] * p[1] + (-q[1]) * p[2] + q[0] * p[3];
  qleft_mul(r4, eq, &xp[3]);                                                                     // :278-279
}

struct LocPropArgs {
  int N, t;
  const int* ai;                 // [N] ancestors
  const double* X_old; double* X_new;   // SoA [7][N]
  const double* odo; const double* S;
  int rng_mode; const double* Z; unsigned long long seed;
};

__global__ void loc_propagate_kernel(const LocPropArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.N) return;
  const int anc = min(max(a.ai[i], 0), a.N - 1);
  double x[7], xp[7], z[6];
#pragma unroll
  for (int c = 0; c < 7; ++c) x[c] = a.X_old[(size_t)c * a.N + anc];
  if (a.rng_mode == RBPF_RNG_REPLAY) {
#pragma unroll
    for (int k = 0; k < 6; ++k) z[k] = a.Z[(size_t)i * 6 + k];
  } else {
    philox_normals(a.seed, i, a.t, 0, 6, z);
  }
  loc_dyn_model_dev(x, a.odo, a.S, z, xp);
#pragma unroll
  for (int c = 0; c < 7; ++c) a.X_new[(size_t)c * a.N + i] = xp[c];
}

__global__ void loc_dyn_model_kernel(int np, const double* __restrict__ xn, const double* __restrict__ odo, const double* __restrict__ S,
                                     const double* __restrict__ z, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= np) return;
  double x[7], xp[7], zz[6];
  for (int c = 0; c < 7; ++c) x[c] = xn[(size_t)i * 7 + c];
  for (int k = 0; k < 6; ++k) zz[k] = z[(size_t)i * 6 + k];
  loc_dyn_model_dev(x, odo, S, zz, xp);
  for (int c = 0; c < 7; ++c) out[(size_t)i * 7 + c] = xp[c];
}

// x0 [7 x cols] (AoS, cols = 1 or N) -> X[0] SoA
__global__ void loc_fill_x0_kernel(int N, int cols, const double* __restrict__ x0, double* __restrict__ X0) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  for (int c = 0; c < 7; ++c) X0[(size_t)c * N + i] = x0[(size_t)(cols > 1 ? i : 0) * 7 + c];
}

// ---- host side -----------------------------------------------------------------------------------------------------------
void loc_free(rbpf_ctx* c) {
  if (!c || !c->loc) return;
  LocState* L = c->loc;
  delete L;
  c->loc = nullptr;
}

template <typename T>
static int loc_size_ok(const T* p, const char* name) {
  if (!p) { set_error(std::string(name) + " is NULL"); return RBPF_ERR_INVALID_ARG; }
  if (p->struct_size != 0 && p->struct_size != (int32_t)sizeof(T)) {
    set_error(std::string(name) + ".struct_size = " + std::to_string(p->struct_size) + ", this library's has " + std::to_string(sizeof(T)) +
              " bytes: rebuild the binding against include/rbpf.h");
    return RBPF_ERR_INVALID_ARG;
  }
  return RBPF_OK;
}

// filter = true: exactly one of V / var_table; false (rbpf_loc_predict): V optional, var_table not read
static int loc_validate_map(const rbpf_loc_map* map, bool filter) {
  RB_TRY(loc_size_ok(map, "rbpf_loc_map"));
  if (map->m_basis < 1 || map->m_basis + 3 > kLocMaxN) { set_error("rbpf_loc_map: n = m_basis + 3 must be in 4 .. 1151"); return RBPF_ERR_INVALID_ARG; }
  if (!map->NN || !map->mean) { set_error("rbpf_loc_map: NN / mean is NULL"); return RBPF_ERR_INVALID_ARG; }
  if (filter && ((map->V != nullptr) == (map->var_table != nullptr))) { set_error("rbpf_loc_map: exactly one of V and var_table must be set"); return RBPF_ERR_INVALID_ARG; }
  if (!(map->sigma2 >= 0.0)) { set_error("rbpf_loc_map: sigma2 must be >= 0"); return RBPF_ERR_INVALID_ARG; }
  return RBPF_OK;
}

static int loc_validate_problem(const rbpf_loc_problem* p) {
  RB_TRY(loc_size_ok(p, "rbpf_loc_problem"));
  if (p->N_P < 1 || p->N_T < 1) { set_error("N_P and N_T must be >= 1"); return RBPF_ERR_INVALID_ARG; }
  if (p->N_P > kMaxParticles) { set_error("N_P above 1048576 is not supported"); return RBPF_ERR_UNSUPPORTED; }
  if (!p->y || !p->x0_nonlin || !p->Q || !p->dt) { set_error("a required problem array is NULL"); return RBPF_ERR_INVALID_ARG; }
  if (p->N_T > 1 && (!p->odometry || p->odo_ld < p->N_T - 1)) { set_error("odometry must be [>= N_T-1 x 7]"); return RBPF_ERR_INVALID_ARG; }
  if (p->x0_cols != 1 && p->x0_cols != p->N_P) { set_error("x0_nonlin must be 7 x 1 or 7 x N_P"); return RBPF_ERR_INVALID_ARG; }
  if (p->q_pages != 1 && p->q_pages < p->N_T - 1) { set_error("Q must have 1 or >= N_T-1 pages"); return RBPF_ERR_INVALID_ARG; }
  if (p->dt_len != 1 && p->dt_len < p->N_T - 1) { set_error("dt must have 1 or >= N_T-1 entries"); return RBPF_ERR_INVALID_ARG; }
  return RBPF_OK;
}

int loc_validate_options(const rbpf_options* o) {
  RB_TRY(options_ok(o));
  if (!o) return RBPF_OK;
  if (o->fix_p_mean || o->lazy_depth || o->inplace || o->storage || o->chol_variant || o->chol_refresh || o->exchange_capacity ||
      o->n_devices || o->device_ids || o->info_rebuild) {
    set_error("localisation reads keep_history, trace and on_step only: every other option must be zero (sharding is not implemented)");
    return RBPF_ERR_UNSUPPORTED;
  }
  return RBPF_OK;
}

// element-wise sqrt(dt Q) of the two diagonal blocks, per page (run_localization.m:277,279)
static int loc_noise_pages(const rbpf_loc_problem* p, std::vector<double>& S, int& pages) {
  const bool varying = p->q_pages > 1 || p->dt_len > 1;
  pages = varying ? std::max(p->N_T - 1, 1) : 1;
  S.assign((size_t)pages * 36, 0.0);
  for (int t = 0; t < pages; ++t) {
    const double dt = p->dt[p->dt_len > 1 ? t : 0];
    const double* Q = p->Q + (size_t)(p->q_pages > 1 ? t : 0) * 36;
    for (int b = 0; b < 2; ++b)
      for (int c = 0; c < 3; ++c)
        for (int r = 0; r < 3; ++r) {
          const int q = (3 * b + r) + 6 * (3 * b + c);
          const double v = dt * Q[q];
          if (!(v >= 0.0)) { set_error("dt * Q has a negative entry in a diagonal block: the element-wise sqrt of dynModel would be complex"); return RBPF_ERR_INVALID_ARG; }
          S[(size_t)t * 36 + q] = std::sqrt(v);
        }
  }
  return RBPF_OK;
}

// ModelDev of the map's basis; nn: axis-major copy of NN for the device
static int loc_model_dev(const rbpf_loc_map* map, ModelDev& M, std::vector<int>& nn) {
  rbpf_model md;
  std::memset(&md, 0, sizeof(md));
  md.kind = RBPF_MODEL_DENSE_MAG_6D; md.m_basis = map->m_basis; md.dim = 3; md.NN = map->NN;
  for (int a = 0; a < 3; ++a) md.L[a] = map->L[a];
  RB_TRY(fill_model_dev(&md, 7, map->m_basis + 3, 3, 6, 7, nullptr, 0.0, M, nn));
  if (loc_lds_bytes(M.ktot, true) > (size_t)kLocLdsLimit) {
    set_error("rbpf_loc_map: the per-axis index range of NN (" + std::to_string(M.ktot) + " table entries per particle) exceeds the 96 the prediction kernel keeps in LDS");
    return RBPF_ERR_UNSUPPORTED;
  }
  return RBPF_OK;
}

static size_t loc_bytes(const rbpf_loc_map* map, const rbpf_loc_problem* p, const rbpf_options* opt, const rbpf_rng* rng) {
  const size_t N = p->N_P, T = p->N_T, n = map->m_basis + 3;
  const bool hist = opt && opt->keep_history, trace = opt && opt->trace;
  size_t b = (hist ? T : 2) * 7 * N * sizeof(double) + (hist ? T : 1) * N * sizeof(int);
  b += ((trace ? 2 * T : 2) + 1) * N * sizeof(double);
  b += (n + (map->V ? n * n : 0) + (map->var_table ? 3 * N : 0) + (size_t)3 * map->m_basis) * sizeof(double);
  b += (resample_scratch_doubles((int)N) + 15 * T + 36 * T + 7 * (size_t)p->x0_cols) * sizeof(double);
  if (rng && rng->mode == RBPF_RNG_REPLAY) b += 7 * N * (T > 1 ? T - 1 : 0) * sizeof(double);
  return b;
}

static int loc_step(rbpf_ctx* c) {
  LocState* L = c->loc;
  const int t = c->t, N = c->N, T = c->T;
  if (t >= T) { set_error("advance past N_T"); return RBPF_ERR_STATE; }
  const bool hist = c->opt.keep_history != 0;
  int* A_t = c->A + (hist ? (size_t)t * N : 0);
  double* X_new = c->X + (size_t)(hist ? t : (t & 1)) * 7 * N;
  const double* X_old = (t == 0) ? X_new : c->X + (size_t)(hist ? t - 1 : ((t - 1) & 1)) * 7 * N;
  const size_t tr = c->opt.trace ? (size_t)t * N : 0;
  if (t == 0) {
    hipLaunchKernelGGL(loc_fill_x0_kernel, dim3((N + 255) / 256), dim3(256), 0, c->stream, N, L->x0_cols, L->d_x0, X_new);
    HIPCHK(hipGetLastError());
  } else {
    // ai(i) = sample(w) for every slot (particleFilterLocalization.m:93): approximate search on the parallel prefix, exact re-draw
    // against the strict cumsum when a uniform falls within rounding of a bin edge (tools/sample.m:30-32 stays bit-exact)
    SearchArgs s;
    s.N = N; s.n_draw = N; s.t = t; s.wc = c->wc; s.rng_mode = c->rng_mode; s.k_iter = 0;
    s.U = c->d_U ? c->d_U + (size_t)(t - 1) * N : nullptr;
    s.seed = c->seed; s.ai = A_t; s.overflow = c->d_flags + 1;
    s.approx = 1; s.ambiguous = c->d_flags + 4; s.w = c->w + (c->opt.trace ? (size_t)(t - 1) * N : 0); s.wc_exact = c->wc;
    if (N > kSingleWgResampleMaxN) s.scan_depth = (N + 1023) / 1024 + 32;
    HIPCHK(launch_search(s, c->stream));
    HIPCHK(launch_resample_fixup(s, c->stream));
    LocPropArgs pa;
    pa.N = N; pa.t = t; pa.ai = A_t; pa.X_old = X_old; pa.X_new = X_new;
    pa.odo = c->d_odo + (size_t)(t - 1) * 7;
    pa.S = L->d_S + (size_t)(L->s_pages > 1 ? t - 1 : 0) * 36;
    pa.rng_mode = c->rng_mode; pa.seed = c->seed;
    pa.Z = c->d_Z ? c->d_Z + (size_t)(t - 1) * N * 6 : nullptr;
    hipLaunchKernelGGL(loc_propagate_kernel, dim3((N + 255) / 256), dim3(256), 0, c->stream, pa);
    HIPCHK(hipGetLastError());
  }
  LocArgs a;
  a.mdl = c->mdl; a.n = L->n; a.npart = N;
  a.xn = X_new; a.xn_cs = (size_t)N; a.xn_ps = 1;
  a.mean = L->d_mean; a.V = L->d_V; a.var_table = L->d_vartab; a.sigma2 = L->sigma2;
  a.y = c->d_y + (size_t)t * 3; a.dEft = nullptr; a.var = nullptr; a.logw = c->logw + tr;
  HIPCHK(launch_loc_predict(a, c->stream));
  NormArgs nm;
  nm.N = N; nm.nN = 7; nm.t = t; nm.logw = c->logw + tr; nm.w = c->w + tr; nm.wc = c->wc; nm.xn = X_new;
  nm.traj_max = c->traj_max + (size_t)t * 7; nm.traj_mean = c->traj_mean + (size_t)t * 7;
  nm.iw_max = c->d_flags + 2; nm.lse_out = L->d_lse + t;
  nm.parallel_scan = 1;
  if (N > kSingleWgResampleMaxN) {
    HIPCHK(launch_resample_pipeline(nm, nullptr, nullptr, nullptr, nullptr, c->d_rs, c->stream));
    HIPCHK(launch_resample_lse(N, c->d_rs, L->d_lse + t, c->stream));
  } else {
    HIPCHK(launch_normalise_scan(nm, c->stream));
  }
  c->t = t + 1;
  return RBPF_OK;
}

}  // namespace rbpf

using namespace rbpf;

extern "C" {

int rbpf_loc_workspace_bytes(const rbpf_loc_map* map, const rbpf_loc_problem* prob, const rbpf_options* opt, size_t* bytes) {
  if (!bytes) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  RB_TRY(loc_validate_map(map, true));
  RB_TRY(loc_validate_problem(prob));
  RB_TRY(loc_validate_options(opt));
  *bytes = loc_bytes(map, prob, opt, nullptr);
  return RBPF_OK;
}

int rbpf_loc_create(const rbpf_loc_map* map, const rbpf_loc_problem* prob, const rbpf_rng* rng, const rbpf_options* opt,
                    rbpf_ctx** out) {
  if (!out) { set_error("ctx out pointer is NULL"); return RBPF_ERR_INVALID_ARG; }
  *out = nullptr;
  RB_TRY(loc_validate_map(map, true));
  RB_TRY(loc_validate_problem(prob));
  RB_TRY(loc_validate_options(opt));
  if (!rng) { set_error("rng is NULL"); return RBPF_ERR_INVALID_ARG; }
  const int N = prob->N_P, T = prob->N_T, n = map->m_basis + 3;
  if (rng->mode == RBPF_RNG_REPLAY && T > 1 && (!rng->U || !rng->Z)) { set_error("replay rng needs U and Z"); return RBPF_ERR_INVALID_ARG; }
  if (rng->mode != RBPF_RNG_REPLAY && rng->mode != RBPF_RNG_PHILOX) { set_error("unknown rng mode"); return RBPF_ERR_INVALID_ARG; }
  std::vector<double> S;
  int s_pages = 1;
  RB_TRY(loc_noise_pages(prob, S, s_pages));
  ModelDev M;
  std::vector<int> nn;
  RB_TRY(loc_model_dev(map, M, nn));
  if (!have_device()) { set_error("no HIP device: the localisation filter has no CPU fallback"); return RBPF_ERR_NO_DEVICE; }

  rbpf_ctx* c = new rbpf_ctx();
  LocState* L = new LocState();
  c->loc = L;
  std::memset(&c->opt, 0, sizeof(c->opt));
  if (opt) c->opt = *opt;
  c->N = N; c->T = T; c->mdl = M; c->rng_mode = rng->mode; c->seed = rng->seed;
  L->n = n; L->sigma2 = map->sigma2; L->s_pages = s_pages; L->x0_cols = prob->x0_cols;
  c->h_dt.assign(prob->dt, prob->dt + (prob->dt_len > 1 ? T - 1 : 1));   // (the running statistics scale S by 1 / dt)
  c->dt_len = (int)c->h_dt.size();
  const bool hist = c->opt.keep_history != 0, trace = c->opt.trace != 0;
  std::unique_ptr<rbpf_ctx, void (*)(rbpf_ctx*)> guard(c, [](rbpf_ctx* p) { ctx_free(p); });
  HIPCHK(hipGetDevice(&c->device));
  HIPCHK(hipStreamCreate(&c->stream));
  RB_TRY(c->pool.upload(&c->d_NN, nn.data(), nn.size()));
  c->mdl.NN = c->d_NN;
  RB_TRY(L->pool.upload(&L->d_mean, map->mean, (size_t)n));
  if (map->V) RB_TRY(L->pool.upload(&L->d_V, map->V, (size_t)n * n));
  if (map->var_table) RB_TRY(L->pool.upload(&L->d_vartab, map->var_table, (size_t)3 * N));
  RB_TRY(L->pool.upload(&L->d_S, S.data(), S.size()));
  RB_TRY(L->pool.upload(&L->d_x0, prob->x0_nonlin, (size_t)7 * prob->x0_cols));
  {
    // y [N_T x 3] column-major -> [t][3]; odometry [ld x 7] -> [t][7]
    std::vector<double> yy((size_t)T * 3), oo((size_t)std::max(T - 1, 1) * 7, 0.0);
    for (int t = 0; t < T; ++t) for (int k = 0; k < 3; ++k) yy[(size_t)t * 3 + k] = prob->y[t + (size_t)T * k];
    for (int t = 0; t + 1 < T; ++t) for (int k = 0; k < 7; ++k) oo[(size_t)t * 7 + k] = prob->odometry[t + (size_t)prob->odo_ld * k];
    RB_TRY(c->pool.upload(&c->d_y, yy.data(), yy.size()));
    RB_TRY(c->pool.upload(&c->d_odo, oo.data(), oo.size()));
  }
  if (rng->mode == RBPF_RNG_REPLAY && T > 1) {
    RB_TRY(c->pool.upload(&c->d_U, rng->U, (size_t)N * (T - 1)));
    RB_TRY(c->pool.upload(&c->d_Z, rng->Z, (size_t)6 * N * (T - 1)));
  }
  RB_TRY(c->pool.alloc(&c->X, (size_t)(hist ? T : 2) * 7 * N));
  RB_TRY(c->pool.alloc(&c->A, (size_t)(hist ? T : 1) * N));
  HIPCHK(hipMemset(c->A, 0, (size_t)(hist ? T : 1) * N * sizeof(int)));
  RB_TRY(c->pool.alloc(&c->logw, (size_t)(trace ? T : 1) * N));
  RB_TRY(c->pool.alloc(&c->w, (size_t)(trace ? T : 1) * N));
  RB_TRY(c->pool.alloc(&c->wc, (size_t)N));
  RB_TRY(c->pool.alloc(&c->traj_max, (size_t)T * 7));
  RB_TRY(c->pool.alloc(&c->traj_mean, (size_t)T * 7));
  RB_TRY(L->pool.alloc(&L->d_lse, (size_t)T));
  RB_TRY(c->pool.alloc(&c->d_flags, 16));
  HIPCHK(hipMemset(c->d_flags, 0, 16 * sizeof(int)));
  RB_TRY(c->pool.alloc(&c->d_rs, resample_scratch_doubles(N)));
  guard.release();
  *out = c;
  return RBPF_OK;
}

int rbpf_loc_advance(rbpf_ctx* c, int32_t n_steps) {
  if (!c || !c->loc) { set_error("not a localisation context"); return RBPF_ERR_INVALID_ARG; }
  if (c->loc->generic) { set_error("a generic localisation context is driven step by step (rbpf_loc_generic_step_device): its handles are the caller's"); return RBPF_ERR_STATE; }
  HIPCHK(hipSetDevice(c->device));
  for (int s = 0; s < n_steps; ++s) {
    RB_TRY(loc_step(c));
    RB_TRY(ctx_call_on_step(c, c->t - 1, false));       // particleFilterLocalization.m:129-131
  }
  return RBPF_OK;
}

int rbpf_loc_finish(rbpf_ctx* c, rbpf_loc_out* o) {
  if (!c || !c->loc) { set_error("not a localisation context"); return RBPF_ERR_INVALID_ARG; }
  RB_TRY(loc_size_ok(o, "rbpf_loc_out"));
  HIPCHK(hipSetDevice(c->device));
  const int N = c->N, Td = c->t, nN = c->loc->nN;
  const bool hist = c->opt.keep_history != 0, trace = c->opt.trace != 0;
  if ((o->trace_logw || o->trace_w) && !trace) { set_error("trace_logw / trace_w need rbpf_options.trace"); return RBPF_ERR_STATE; }
  if ((o->trace_ai || o->xn_traj) && !hist) { set_error("trace_ai / xn_traj need rbpf_options.keep_history"); return RBPF_ERR_STATE; }
  HIPCHK(hipStreamSynchronize(c->stream));
  RB_TRY(ctx_check_flags(c));
  o->first_degenerate_step = -1;
  if (Td == 0) return RBPF_OK;
  std::vector<double> lse((size_t)Td);
  HIPCHK(hipMemcpy(lse.data(), c->loc->d_lse, (size_t)Td * sizeof(double), hipMemcpyDeviceToHost));
  for (int t = 0; t < Td; ++t)
    if (!(lse[t] > std::log(1e-12))) { o->first_degenerate_step = t; break; }                    // sum(w) <= 1e-12 (:113)
  if (o->log_sum_w) std::memcpy(o->log_sum_w, lse.data(), (size_t)Td * sizeof(double));
  if (o->traj_max) HIPCHK(hipMemcpy(o->traj_max, c->traj_max, (size_t)Td * nN * sizeof(double), hipMemcpyDeviceToHost));
  if (o->traj_mean) HIPCHK(hipMemcpy(o->traj_mean, c->traj_mean, (size_t)Td * nN * sizeof(double), hipMemcpyDeviceToHost));
  if (o->trace_logw) HIPCHK(hipMemcpy(o->trace_logw, c->logw, (size_t)Td * N * sizeof(double), hipMemcpyDeviceToHost));
  if (o->trace_w) HIPCHK(hipMemcpy(o->trace_w, c->w, (size_t)Td * N * sizeof(double), hipMemcpyDeviceToHost));
  if (o->trace_ai) HIPCHK(hipMemcpy(o->trace_ai, c->A, (size_t)Td * N * sizeof(int), hipMemcpyDeviceToHost));
  const double* X_last = c->X + (size_t)(hist ? Td - 1 : ((Td - 1) & 1)) * nN * N;
  if (o->final_xn || o->xn_traj) {
    DevicePool tmp;
    double* d_tmp = nullptr;
    const size_t cnt = (size_t)nN * N * (o->xn_traj ? Td : 1);
    RB_TRY(tmp.alloc(&d_tmp, cnt));
    if (o->final_xn) {
      HIPCHK(launch_transpose_soa(N, nN, X_last, d_tmp, c->stream));
      HIPCHK(hipStreamSynchronize(c->stream));
      HIPCHK(hipMemcpy(o->final_xn, d_tmp, (size_t)nN * N * sizeof(double), hipMemcpyDeviceToHost));
    }
    if (o->xn_traj) {
      // xn_traj(:,:,1:t-1) = xn_traj(:,ai,1:t-1) of every step (:101-104) = every slot's path through the ancestor table
      HIPCHK(launch_backtrace(N, nN, Td, c->X, c->A, nullptr, N, d_tmp, c->stream, 0));
      HIPCHK(hipStreamSynchronize(c->stream));
      HIPCHK(hipMemcpy(o->xn_traj, d_tmp, cnt * sizeof(double), hipMemcpyDeviceToHost));
    }
  }
  return RBPF_OK;
}

int rbpf_particle_filter_localization(const rbpf_loc_map* map, const rbpf_loc_problem* prob, const rbpf_rng* rng,
                                      const rbpf_options* opt, rbpf_loc_out* out) {
  rbpf_ctx* c = nullptr;
  int s = rbpf_loc_create(map, prob, rng, opt, &c);
  if (s != RBPF_OK) return s;
  s = rbpf_loc_advance(c, prob->N_T);
  if (s == RBPF_OK) s = rbpf_loc_finish(c, out);
  rbpf_destroy(c);
  return s;
}

int rbpf_loc_predict(const rbpf_loc_map* map, int32_t n_pred, const double* xn, double* dEft, double* var, int32_t reps, double* ms) {
  RB_TRY(loc_validate_map(map, false));
  if (!xn || n_pred < 1 || (!dEft && !var)) { set_error("bad argument"); return RBPF_ERR_INVALID_ARG; }
  if (var && !map->V) { set_error("rbpf_loc_predict: var needs map->V"); return RBPF_ERR_INVALID_ARG; }
  ModelDev M;
  std::vector<int> nn;
  RB_TRY(loc_model_dev(map, M, nn));
  if (!have_device()) { set_error("no HIP device"); return RBPF_ERR_NO_DEVICE; }
  const int n = map->m_basis + 3;
  DevicePool tmp;
  int* d_nn = nullptr;
  double *d_xn = nullptr, *d_mean = nullptr, *d_V = nullptr, *d_E = nullptr, *d_var = nullptr;
  RB_TRY(tmp.upload(&d_nn, nn.data(), nn.size()));
  RB_TRY(tmp.upload(&d_xn, xn, (size_t)7 * n_pred));
  RB_TRY(tmp.upload(&d_mean, map->mean, (size_t)n));
  if (map->V && var) RB_TRY(tmp.upload(&d_V, map->V, (size_t)n * n));
  RB_TRY(tmp.alloc(&d_E, (size_t)3 * n_pred));
  RB_TRY(tmp.alloc(&d_var, (size_t)3 * n_pred));
  LocArgs a;
  a.mdl = M; a.mdl.NN = d_nn; a.n = n; a.npart = n_pred;
  a.xn = d_xn; a.xn_cs = 1; a.xn_ps = 7;
  a.mean = d_mean; a.V = d_V; a.var_table = nullptr; a.sigma2 = map->sigma2; a.y = nullptr; a.logw = nullptr;
  a.dEft = d_E; a.var = d_var;
  RB_TRY(timed_reps(reps, 0, [&] { return launch_loc_predict(a, 0); }, ms));
  if (dEft) HIPCHK(hipMemcpy(dEft, d_E, (size_t)3 * n_pred * sizeof(double), hipMemcpyDeviceToHost));
  if (var) HIPCHK(hipMemcpy(var, d_var, (size_t)3 * n_pred * sizeof(double), hipMemcpyDeviceToHost));
  return RBPF_OK;
}

int rbpf_loc_dyn_model(int32_t n_p, const double* xn, const double* odo, double dt, const double* Q, const double* z, double* xn_next) {
  if (!xn || !odo || !Q || !z || !xn_next || n_p < 1) { set_error("bad argument"); return RBPF_ERR_INVALID_ARG; }
  rbpf_loc_problem p;
  std::memset(&p, 0, sizeof(p));
  p.N_T = 2; p.q_pages = 1; p.dt_len = 1; p.Q = Q; p.dt = &dt;
  std::vector<double> S;
  int pages = 1;
  RB_TRY(loc_noise_pages(&p, S, pages));
  if (!have_device()) { set_error("no HIP device"); return RBPF_ERR_NO_DEVICE; }
  DevicePool tmp;
  double *d_x = nullptr, *d_o = nullptr, *d_S = nullptr, *d_z = nullptr, *d_out = nullptr;
  RB_TRY(tmp.upload(&d_x, xn, (size_t)7 * n_p));
  RB_TRY(tmp.upload(&d_o, odo, (size_t)7));
  RB_TRY(tmp.upload(&d_S, S.data(), (size_t)36));
  RB_TRY(tmp.upload(&d_z, z, (size_t)6 * n_p));
  RB_TRY(tmp.alloc(&d_out, (size_t)7 * n_p));
  hipLaunchKernelGGL(loc_dyn_model_kernel, dim3((n_p + 63) / 64), dim3(64), 0, 0, n_p, d_x, d_o, d_S, d_z, d_out);
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(xn_next, d_out, (size_t)7 * n_p * sizeof(double), hipMemcpyDeviceToHost));
  return RBPF_OK;
}

}  // extern "C"
