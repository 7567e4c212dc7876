// Localisation in the fixed map of an arbitrary device-code model: particleFilter.m:100-161 with xl, P the same for every particle
// and never updated (:163-204 left out).  The map posterior is N(mean, V'V), V lower n x n (the DenseMagMap convention); the
// caller's measModel hands over H_i = dy(i,:,:) [n_y x n], and per particle
//     e = y_t' - H_i mean,   S = (V H_i')'(V H_i') + R,   logw = -sum log diag chol S - |chol(S) \ e|^2 / 2 - n_y log(2 pi) / 2
// (:139-150; the jitter retry of :145-148 cannot trigger: S is a Gram matrix plus a positive definite R, checked at creation).
//
// loc_generic_weights_kernel<NY> is the hot kernel, a sibling of loc_predict_kernel (rbpf_loc.hip).  One workgroup serves
// kLgCT = 8 column tiles of 16; a tile carries floor(16 / NY) particles, particle q of a tile in its columns q NY .. q NY + NY - 1
// (the columns past them are zero), so every particle's columns lie inside one tile:
//   * Y = V H' on v_mfma_f64_16x16x4 in super-blocks of 128 rows (4 waves x 2 row tiles of 16 x 128, accumulators in registers),
//     A operand = V read straight from global memory (lower triangle only: the k chunks right of a row tile's diagonal block are
//     skipped, entries above the diagonal masked), B operand = a 16-deep k chunk of the H rows staged in LDS; the chunks are
//     loaded from memory by all 256 threads, which also accumulate H mean (in the last super-block, the one that sees every k);
//   * the Gram blocks: a finished 16 x 16 result tile has its column on the lane and its rows on (lane >> 4) + 4 reg, which is the
//     operand map of the same instruction with k = lane >> 4 -- register r of the tile, given as A AND B, adds
//     sum_k Y(4 r + k, i) Y(4 r + k, j) to a 16 x 16 tile of Y'Y.  Four more MFMAs per result tile therefore sum its whole Gram
//     tile, with no lane movement and no LDS; the diagonal NY x NY blocks of that tile are the particles' H P H'.  One Gram
//     accumulator per column tile lives across the super-blocks; the four waves' partial sums meet in LDS at the end;
//   * one thread per particle adds R, factors the NY x NY matrix in registers and writes the log-weight.  Y never leaves the CU.
#include "../../include/rbpf.h"
#include "rbpf_internal.hpp"
#include "rbpf_ctx.hpp"
#include "rbpf_loc_state.hpp"
#include "rbpf_timed_reps.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace rbpf {

constexpr int kLgCT = 8;                   // column tiles of 16 per workgroup
constexpr int kLgCols = 16 * kLgCT;
constexpr int kLgKC = 16;                  // k depth of a staged chunk
constexpr int kLgGS = 144;                 // row pitch of a chunk in LDS (doubles): 288 dwords = 32 mod 64 banks, the four k rows of an operand read are conflict-free
constexpr int kLgRows = 128;               // rows of a super-block: 4 waves x 2 row tiles
constexpr int kLgRed = 128;                // Gram entries kept per (wave, column tile): floor(16 / NY) NY^2 <= 128
constexpr int kLgMaxN = 1151;              // the library's largest nLin
constexpr int kLgMaxNy = 8, kLgMaxNonlin = 8;

struct LocGenArgs {
  int n, npart, ld;              // nLin, particles, row stride of H in doubles
  const double* H;               // H_i(k, c) at H[((size_t)i * NY + k) * ld + c], c < n (what lies behind column n is never read)
  const double* mean;            // [n]
  const double* V;               // [n x n] column-major lower factor
  const double* R;               // [NY x NY] column-major
  const double* y;               // [NY]
  double* yhat;                  // [npart][NY] or null
  double* S;                     // [npart][NY x NY] column-major, H P H' before R is added, or null
  double* logw;                  // [npart] or null
};

typedef double lg_v4d __attribute__((ext_vector_type(4)));

template <int NY>
__global__ __launch_bounds__(256) void loc_generic_weights_kernel(const LocGenArgs a) {
  constexpr int PPT = 16 / NY;             // particles per column tile
  constexpr int PB = kLgCT * PPT;          // particles per workgroup
  constexpr int BLK = NY * NY;
  static_assert(PPT * BLK <= kLgRed, "Gram scratch");
  static_assert(4 * kLgCT * kLgRed <= 2 * kLgKC * kLgGS, "the Gram scratch reuses the chunk buffers");
  __shared__ double Gb[2 * kLgKC * kLgGS]; // [2][16][kLgGS] chunks; after the last chunk: [4][kLgCT][kLgRed] partial Gram blocks
  __shared__ double redE[kLgCols];         // H mean per column
  const int n = a.n;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int p0 = blockIdx.x * PB;

  // staging map: thread = (k offset skk, column scg of every tile); column scg of tile j is output row sk of particle p0 + j PPT + sq
  const int skk = tid & 15, scg = tid >> 4;
  const int sq = scg / NY, sk = scg - sq * NY;
  const bool scol = sq < PPT;
  const double* hrow[kLgCT];
  bool hok[kLgCT];
#pragma unroll
  for (int j = 0; j < kLgCT; ++j) {
    const int p = p0 + j * PPT + sq;
    hok[j] = scol && p < a.npart;
    hrow[j] = a.H + ((size_t)min(p, a.npart - 1) * NY + sk) * (size_t)a.ld;   // (clamped: the address is valid whether it is read or not)
  }
  double dE[kLgCT];
#pragma unroll
  for (int j = 0; j < kLgCT; ++j) dE[j] = 0.0;

  lg_v4d gram[kLgCT];
#pragma unroll
  for (int ct = 0; ct < kLgCT; ++ct) gram[ct] = (lg_v4d){0.0, 0.0, 0.0, 0.0};

  const int nsb = (n + kLgRows - 1) / kLgRows;
  const int arow = lane & 15, ak = lane >> 4;            // MFMA operand maps: A row / B column = lane & 15, k = lane >> 4
  int buf = 0;
  for (int sb = 0; sb < nsb; ++sb) {
    const bool last = (sb == nsb - 1);                   // the last super-block sees every k: the means are summed there
    const int kend = min(n, kLgRows * (sb + 1));
    const int nch = (kend + kLgKC - 1) / kLgKC;
    const int rt0 = sb * (kLgRows / 16) + wv * 2;        // this wave's first row tile
    const int row0 = rt0 * 16 + arow, row1 = row0 + 16;
    lg_v4d acc[2][kLgCT];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int ct = 0; ct < kLgCT; ++ct) acc[x][ct] = (lg_v4d){0.0, 0.0, 0.0, 0.0};

    // chunk kc of the H rows into buffer b: G[kk][column]; columns without a particle and k >= n are zeros
    auto load_chunk = [&](int kc, int b) {
      double* G = Gb + (size_t)b * kLgKC * kLgGS + skk * kLgGS + scg;
      const int k = kc * kLgKC + skk;
      const bool kok = k < n;
      const int kcl = min(k, n - 1);
      const double mk = (last && kok) ? a.mean[kcl] : 0.0;
#pragma unroll
      for (int j = 0; j < kLgCT; ++j) {
        const double h = hrow[j][kcl];
        const double v = (kok && hok[j]) ? h : 0.0;
        G[j * 16] = v;
        if (last) dE[j] = fma(v, mk, dE[j]);
      }
    };
    // A operands of chunk kc: V(row, k) for k <= row < n, zero elsewhere (upper triangle, padding); the address is clamped
    auto load_a = [&](int kc, double av[4][2]) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const int k = kc * kLgKC + ks * 4 + ak;
        const int kcl = min(k, n - 1);
        const bool ok0 = (k <= row0) && (row0 < n), ok1 = (k <= row1) && (row1 < n);
        const double v0 = a.V[(size_t)kcl * n + min(row0, n - 1)];
        const double v1 = a.V[(size_t)kcl * n + min(row1, n - 1)];
        av[ks][0] = ok0 ? v0 : 0.0;
        av[ks][1] = ok1 ? v1 : 0.0;
      }
    };

    double a_cur[4][2], a_nxt[4][2];
    load_chunk(0, buf);
    load_a(0, a_cur);
    __syncthreads();
    for (int kc = 0; kc < nch; ++kc) {
      const bool more = kc + 1 < nch;
      if (more) { load_a(kc + 1, a_nxt); load_chunk(kc + 1, buf ^ 1); }
      // row tile x holds non-zeros of this chunk iff kc <= its tile index (wave-uniform)
      const bool act0 = (kc <= rt0) && (rt0 * 16 < n), act1 = (kc <= rt0 + 1) && ((rt0 + 1) * 16 < n);
      if (act1) {                                         // act0 implies act1 inside the matrix except past the last row
        const double* G = Gb + (size_t)buf * kLgKC * kLgGS + ak * kLgGS + arow;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
          for (int ct = 0; ct < kLgCT; ++ct) {
            const double b = G[ks * 4 * kLgGS + ct * 16];
            if (act0) acc[0][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a_cur[ks][0], b, acc[0][ct], 0, 0, 0);
            acc[1][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a_cur[ks][1], b, acc[1][ct], 0, 0, 0);
          }
        }
      } else if (act0) {
        const double* G = Gb + (size_t)buf * kLgKC * kLgGS + ak * kLgGS + arow;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
          for (int ct = 0; ct < kLgCT; ++ct)
            acc[0][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a_cur[ks][0], G[ks * 4 * kLgGS + ct * 16], acc[0][ct], 0, 0, 0);
      }
      __syncthreads();
      buf ^= 1;
      if (more) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) { a_cur[ks][0] = a_nxt[ks][0]; a_cur[ks][1] = a_nxt[ks][1]; }
      }
    }
    // the k sums of this super-block's tiles are complete.  Result map: column = lane & 15, row = (lane >> 4) + 4 reg, so
    // register r as both operands is A(i, k) = Y(4 r + k, i), B(k, j) = Y(4 r + k, j): the tile's rows 4 r .. 4 r + 3 of Y'Y
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int ct = 0; ct < kLgCT; ++ct) {
        const lg_v4d v = acc[x][ct];
        gram[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(v.x, v.x, gram[ct], 0, 0, 0);
        gram[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(v.y, v.y, gram[ct], 0, 0, 0);
        gram[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(v.z, v.z, gram[ct], 0, 0, 0);
        gram[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(v.w, v.w, gram[ct], 0, 0, 0);
      }
  }

  // (the chunk loop ended with a barrier: nobody reads Gb any more.)  The diagonal NY x NY blocks of every wave's Gram tiles:
  // entry (i, j) of a tile is in register r of lane l with i = (l >> 4) + 4 r, j = l & 15
  double* red = Gb;
#pragma unroll
  for (int ct = 0; ct < kLgCT; ++ct) {
    const double g[4] = {gram[ct].x, gram[ct].y, gram[ct].z, gram[ct].w};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = ak + 4 * r, j = arow;
      const int qi = i / NY, qj = j / NY;
      if (qi == qj && qi < PPT) red[(wv * kLgCT + ct) * kLgRed + qi * BLK + (i - qi * NY) + NY * (j - qj * NY)] = g[r];
    }
  }
  // H mean: the 16 k offsets of a column are 16 consecutive lanes
#pragma unroll
  for (int j = 0; j < kLgCT; ++j) {
    double s = dE[j];
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    s += __shfl_xor(s, 8, 64);
    if (skk == 0) redE[j * 16 + scg] = s;
  }
  __syncthreads();

  // one thread per particle: S = Gram + R, its Cholesky factor, the solve and the weight -- all in registers
  if (tid >= PB) return;
  const int ct = tid / PPT, q = tid - ct * PPT;
  const int slot = p0 + tid;
  if (slot >= a.npart) return;
  // (only the lower triangle is kept: entries (r, c) and (c, r) of a Gram tile are the same products summed in the same order)
  double S[NY][NY], e[NY];
#pragma unroll
  for (int c = 0; c < NY; ++c)
#pragma unroll
    for (int r = c; r < NY; ++r) {
      const int o = ct * kLgRed + q * BLK + r + NY * c;
      const double v = (red[o] + red[kLgCT * kLgRed + o]) + (red[2 * kLgCT * kLgRed + o] + red[3 * kLgCT * kLgRed + o]);
      S[r][c] = v;
      if (a.S) { a.S[(size_t)slot * BLK + r + NY * c] = v; a.S[(size_t)slot * BLK + c + NY * r] = v; }
    }
#pragma unroll
  for (int k = 0; k < NY; ++k) e[k] = redE[ct * 16 + q * NY + k];
  if (a.yhat) {
#pragma unroll
    for (int k = 0; k < NY; ++k) a.yhat[(size_t)slot * NY + k] = e[k];
  }
  if (!a.logw) return;
#pragma unroll
  for (int k = 0; k < NY; ++k) e[k] = a.y[k] - e[k];
  // lower Cholesky factor of S + R, column by column, on the lower triangle (particleFilter.m:139-143)
  double logdet = 0.0;
#pragma unroll
  for (int j = 0; j < NY; ++j) {
    double s = S[j][j] + a.R[j + NY * j];
#pragma unroll
    for (int k = 0; k < j; ++k) s = fma(-S[j][k], S[j][k], s);
    const double dj = sqrt(s);
    logdet += log(dj);
    S[j][j] = dj;
    const double inv = 1.0 / dj;
#pragma unroll
    for (int i = j + 1; i < NY; ++i) {
      double v = S[i][j] + a.R[i + NY * j];
#pragma unroll
      for (int k = 0; k < j; ++k) v = fma(-S[i][k], S[j][k], v);
      S[i][j] = v * inv;
    }
  }
  double zz = 0.0;
#pragma unroll
  for (int i = 0; i < NY; ++i) {                          // z = chol(S) \ e (:150)
    double v = e[i];
#pragma unroll
    for (int k = 0; k < i; ++k) v = fma(-S[i][k], e[k], v);
    v = v / S[i][i];
    e[i] = v;
    zz = fma(v, v, zz);
  }
  a.logw[slot] = -logdet - 0.5 * zz - 0.5 * (double)NY * 1.8378770664093454835606594728112;   // log(2 pi)
}

template <int NY>
static hipError_t launch_lg(const LocGenArgs& a, hipStream_t s) {
  constexpr int PB = kLgCT * (16 / NY);
  hipLaunchKernelGGL((loc_generic_weights_kernel<NY>), dim3((a.npart + PB - 1) / PB), dim3(256), 0, s, a);
  return hipGetLastError();
}

static hipError_t launch_loc_generic_weights(int ny, const LocGenArgs& a, hipStream_t s) {
  switch (ny) {
    case 1: return launch_lg<1>(a, s);
    case 2: return launch_lg<2>(a, s);
    case 3: return launch_lg<3>(a, s);
    case 4: return launch_lg<4>(a, s);
    case 5: return launch_lg<5>(a, s);
    case 6: return launch_lg<6>(a, s);
    case 7: return launch_lg<7>(a, s);
    case 8: return launch_lg<8>(a, s);
    default: return hipErrorInvalidValue;
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------
int lg_ldx(int n) { return (n + 15) / 16 * 16; }   // row stride of the native layout: rows start on 128-byte lines

static int lg_validate_sizes(int n_nonlin, int n_y, int n_lin) {
  if (n_nonlin < 1 || n_y < 1 || n_lin < 1) { set_error("n_nonlin, n_y and n_lin must be >= 1"); return RBPF_ERR_INVALID_ARG; }
  if (n_y > kLgMaxNy) { set_error("localisation in a generic map is built for n_y from 1 to 8"); return RBPF_ERR_UNSUPPORTED; }
  if (n_lin > kLgMaxN) { set_error("localisation in a generic map is built for n_lin from 1 to 1151"); return RBPF_ERR_UNSUPPORTED; }
  if (n_nonlin > kLgMaxNonlin) { set_error("localisation in a generic map is built for n_nonlin from 1 to 8"); return RBPF_ERR_UNSUPPORTED; }
  return RBPF_OK;
}

// (a principal submatrix of a positive definite matrix is positive definite: for a landmark map this one check covers every set
// of observed outputs)
int lg_validate_R(const double* R, int d) {
  std::vector<double> Lr((size_t)d * d);            // sized by d: the landmark map's n_y goes past kLgMaxNy
  if (!chol_lower_host(R, d, d, Lr.data(), d)) { set_error("R must be positive definite"); return RBPF_ERR_CHOL_FAILED; }
  return RBPF_OK;
}

static int lg_ctx_ok(const rbpf_ctx* c) {
  if (!c->loc || !c->loc->generic) { set_error("not a generic localisation context (rbpf_loc_generic_create)"); return RBPF_ERR_STATE; }
  return RBPF_OK;
}

}  // namespace rbpf

using namespace rbpf;

extern "C" {

int rbpf_loc_generic_create(int32_t n_nonlin, int32_t n_y, int32_t n_lin, const double* mean, const double* V, const double* R,
                            int32_t N_P, int32_t N_T, const double* y, const double* x0_nonlin, int32_t x0_cols,
                            const rbpf_rng* rng, const rbpf_options* opt, rbpf_ctx** out) {
  if (!out) { set_error("ctx out pointer is NULL"); return RBPF_ERR_INVALID_ARG; }
  *out = nullptr;
  if (!mean || !V || !R || !y || !x0_nonlin || !rng) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  RB_TRY(lg_validate_sizes(n_nonlin, n_y, n_lin));
  RB_TRY(loc_generic_validate_run(N_P, N_T, x0_cols, rng, opt));
  RB_TRY(lg_validate_R(R, n_y));
  if (!have_device()) { set_error("no HIP device: the localisation filter has no CPU fallback"); return RBPF_ERR_NO_DEVICE; }
  return loc_generic_build(n_nonlin, n_y, n_lin, mean, V, R, N_P, N_T, y, x0_nonlin, x0_cols, rng, opt, out);
}

}  // extern "C"

// what every generic localisation context checks of its run (rbpf_loc_generic_create, rbpf_loc_landmark_create)
int rbpf::loc_generic_validate_run(int N_P, int N_T, int x0_cols, const rbpf_rng* rng, const rbpf_options* opt) {
  if (N_P < 1 || N_T < 1) { set_error("N_P and N_T must be >= 1"); return RBPF_ERR_INVALID_ARG; }
  if (N_P > kMaxParticles) { set_error("N_P above 1048576 is not supported"); return RBPF_ERR_UNSUPPORTED; }
  if (x0_cols != 1 && x0_cols != N_P) { set_error("x0_nonlin must be n_nonlin x 1 or n_nonlin x N_P"); return RBPF_ERR_INVALID_ARG; }
  RB_TRY(loc_validate_options(opt));
  if (rng->mode != RBPF_RNG_REPLAY && rng->mode != RBPF_RNG_PHILOX) { set_error("unknown rng mode"); return RBPF_ERR_INVALID_ARG; }
  if (rng->mode == RBPF_RNG_REPLAY && N_T > 1 && !rng->U) { set_error("replay rng needs U (the handle draws its own normals: Z is not read)"); return RBPF_ERR_INVALID_ARG; }
  return RBPF_OK;
}

// the context of validated arguments: the map, the measurements and the arrays of the filter's steps
int rbpf::loc_generic_build(int n_nonlin, int n_y, int n_lin, const double* mean, const double* V, const double* R, int N_P, int N_T,
                            const double* y, const double* x0_nonlin, int x0_cols, const rbpf_rng* rng, const rbpf_options* opt,
                            rbpf_ctx** out) {
  const int N = N_P, T = N_T, n = n_lin, d = n_y, nN = n_nonlin;
  rbpf_ctx* c = new rbpf_ctx();
  LocState* L = new LocState();
  c->loc = L;
  std::memset(&c->opt, 0, sizeof(c->opt));
  if (opt) c->opt = *opt;
  std::memset(&c->mdl, 0, sizeof(c->mdl));                // kind 0: no model family's entry point takes this context
  c->mdl.nN = nN; c->mdl.n = n; c->mdl.d = d;
  c->N = N; c->T = T; c->rng_mode = rng->mode; c->seed = rng->seed;
  L->generic = true; L->n = n; L->nN = nN; L->d = d; L->ldx = lg_ldx(n); L->x0_cols = x0_cols;
  const bool hist = c->opt.keep_history != 0, trace = c->opt.trace != 0;
  std::unique_ptr<rbpf_ctx, void (*)(rbpf_ctx*)> guard(c, [](rbpf_ctx* p) { ctx_free(p); });
  HIPCHK(hipGetDevice(&c->device));
  HIPCHK(hipStreamCreate(&c->stream));
  RB_TRY(L->pool.upload(&L->d_mean, mean, (size_t)n));
  RB_TRY(L->pool.upload(&L->d_V, V, (size_t)n * n));
  RB_TRY(L->pool.upload(&L->d_R, R, (size_t)d * d));
  {
    // y [N_T x n_y] column-major -> [t][n_y]; x0 repeated to [n_nonlin x N_P] (particleFilter.m:55-59)
    std::vector<double> yy((size_t)T * d), xx((size_t)nN * N);
    for (int t = 0; t < T; ++t) for (int k = 0; k < d; ++k) yy[(size_t)t * d + k] = y[t + (size_t)T * k];
    for (int i = 0; i < N; ++i) for (int q = 0; q < nN; ++q) xx[q + (size_t)nN * i] = x0_nonlin[q + (size_t)nN * (x0_cols > 1 ? i : 0)];
    RB_TRY(c->pool.upload(&c->d_y, yy.data(), yy.size()));
    RB_TRY(c->pool.upload(&c->d_xn_anc, xx.data(), xx.size()));
  }
  if (rng->mode == RBPF_RNG_REPLAY && T > 1) RB_TRY(c->pool.upload(&c->d_U, rng->U, (size_t)N * (T - 1)));
  RB_TRY(c->pool.alloc(&c->X, (size_t)(hist ? T : 2) * nN * N));
  RB_TRY(c->pool.alloc(&c->A, (size_t)(hist ? T : 1) * N));
  HIPCHK(hipMemset(c->A, 0, (size_t)(hist ? T : 1) * N * sizeof(int)));
  RB_TRY(c->pool.alloc(&c->logw, (size_t)(trace ? T : 1) * N));
  RB_TRY(c->pool.alloc(&c->w, (size_t)(trace ? T : 1) * N));
  RB_TRY(c->pool.alloc(&c->wc, (size_t)N));
  RB_TRY(c->pool.alloc(&c->traj_max, (size_t)T * nN));
  RB_TRY(c->pool.alloc(&c->traj_mean, (size_t)T * nN));
  RB_TRY(L->pool.alloc(&L->d_lse, (size_t)T));
  RB_TRY(c->pool.alloc(&c->d_flags, 16));
  HIPCHK(hipMemset(c->d_flags, 0, 16 * sizeof(int)));
  RB_TRY(c->pool.alloc(&c->d_rs, resample_scratch_doubles(N)));
  guard.release();
  *out = c;
  return RBPF_OK;
}

// after the log-weights of step c->t: normalisation, the cdf for the next draw, traj_max / traj_mean, log(sum(w))
int rbpf::loc_generic_normalise_step(rbpf_ctx* c, const double* X_new) {
  LocState* L = c->loc;
  const int t = c->t, N = c->N, nN = L->nN;
  const size_t tr = c->opt.trace ? (size_t)t * N : 0;
  NormArgs nm;
  nm.N = N; nm.nN = nN; nm.t = t; nm.logw = c->logw + tr; nm.w = c->w + tr; nm.wc = c->wc; nm.xn = X_new;
  nm.traj_max = c->traj_max + (size_t)t * nN; nm.traj_mean = c->traj_mean + (size_t)t * nN;
  nm.iw_max = c->d_flags + 2; nm.lse_out = L->d_lse + t;
  nm.parallel_scan = 1;
  if (N > kSingleWgResampleMaxN) {
    HIPCHK(launch_resample_pipeline(nm, nullptr, nullptr, nullptr, nullptr, c->d_rs, c->stream));
    HIPCHK(launch_resample_lse(N, c->d_rs, L->d_lse + t, c->stream));
  } else {
    HIPCHK(launch_normalise_scan(nm, c->stream));
  }
  return RBPF_OK;
}

extern "C" {

int rbpf_loc_generic_layout(const rbpf_ctx* c, int32_t* ldx) {
  if (!c || !ldx) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  RB_TRY(lg_ctx_ok(c));
  *ldx = c->loc->ldx;
  return RBPF_OK;
}

int rbpf_loc_generic_ancestors_device(rbpf_ctx* c, const int32_t** ai_dev, const double** xn_anc_dev) {
  if (!c || !ai_dev || !xn_anc_dev) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  RB_TRY(lg_ctx_ok(c));
  LocState* L = c->loc;
  const int t = c->t, N = c->N, nN = L->nN;
  if (t >= c->T) { set_error("advance past N_T"); return RBPF_ERR_STATE; }
  *xn_anc_dev = c->d_xn_anc;
  if (t == 0) { *ai_dev = nullptr; return RBPF_OK; }      // the initial states, as uploaded
  HIPCHK(hipSetDevice(c->device));
  const bool hist = c->opt.keep_history != 0;
  int* A_t = c->A + (hist ? (size_t)t * N : 0);
  *ai_dev = A_t;
  if (L->drawn_step == t) return RBPF_OK;
  // ai(i) = sample(w) for every slot (particleFilter.m:106), as loc_step draws them
  SearchArgs s;
  s.N = N; s.n_draw = N; s.t = t; s.wc = c->wc; s.rng_mode = c->rng_mode; s.k_iter = 0;
  s.U = c->d_U ? c->d_U + (size_t)(t - 1) * N : nullptr;
  s.seed = c->seed; s.ai = A_t; s.overflow = c->d_flags + 1;
  s.approx = 1; s.ambiguous = c->d_flags + 4; s.w = c->w + (c->opt.trace ? (size_t)(t - 1) * N : 0); s.wc_exact = c->wc;
  if (N > kSingleWgResampleMaxN) s.scan_depth = (N + 1023) / 1024 + 32;
  HIPCHK(launch_search(s, c->stream));
  HIPCHK(launch_resample_fixup(s, c->stream));
  const double* X_old = c->X + (size_t)(hist ? t - 1 : ((t - 1) & 1)) * nN * N;
  HIPCHK(launch_ext_gather_states(N, nN, X_old, A_t, c->d_xn_anc, c->stream));
  L->drawn_step = t;
  return RBPF_OK;
}

int rbpf_loc_generic_step_device(rbpf_ctx* c, const double* xn_new_dev, const double* dy_dev, int32_t dy_layout) {
  if (!c || !xn_new_dev || !dy_dev) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  if (dy_layout < 0 || dy_layout > 2) { set_error("dy_layout must be 0 (MATLAB order), 1 (native) or 2 (C-contiguous)"); return RBPF_ERR_INVALID_ARG; }
  RB_TRY(lg_ctx_ok(c));
  LocState* L = c->loc;
  if (L->landmark) { set_error("a landmark-map context takes its steps through rbpf_loc_landmark_step_device"); return RBPF_ERR_STATE; }
  const int t = c->t, N = c->N, nN = L->nN, n = L->n, d = L->d;
  if (t >= c->T) { set_error("advance past N_T"); return RBPF_ERR_STATE; }
  if (t > 0 && L->drawn_step != t) { set_error("no ancestors drawn for this step (rbpf_loc_generic_ancestors_device first)"); return RBPF_ERR_STATE; }
  HIPCHK(hipSetDevice(c->device));
  const bool hist = c->opt.keep_history != 0;
  double* X_new = c->X + (size_t)(hist ? t : (t & 1)) * nN * N;
  const size_t tr = c->opt.trace ? (size_t)t * N : 0;
  HIPCHK(launch_ext_states_to_soa(N, nN, xn_new_dev, X_new, c->stream));
  LocGenArgs a;
  a.n = n; a.npart = N;
  if (dy_layout == 0) {                                   // the lines of one particle lie N_P doubles apart: pack them into rows first
    if (!L->d_H) RB_TRY(L->pool.alloc(&L->d_H, (size_t)N * d * L->ldx));
    HIPCHK(launch_ext_pack_dy(0, N, d, n, L->ldx, dy_dev, L->d_H, c->stream));
    a.H = L->d_H; a.ld = L->ldx;
  } else {
    a.H = dy_dev; a.ld = dy_layout == 1 ? L->ldx : n;
  }
  a.mean = L->d_mean; a.V = L->d_V; a.R = L->d_R; a.y = c->d_y + (size_t)t * d;
  a.yhat = nullptr; a.S = nullptr; a.logw = c->logw + tr;
  HIPCHK(launch_loc_generic_weights(d, a, c->stream));
  RB_TRY(loc_generic_normalise_step(c, X_new));
  c->t = t + 1;
  if (!c->opt.on_step) return RBPF_OK;
  HIPCHK(hipStreamSynchronize(c->stream));              // the hook sees a finished step
  return ctx_call_on_step(c, t, false);
}

int rbpf_loc_generic_weights(int32_t n_y, int32_t n_lin, int32_t n_p, const double* dy, int32_t dy_layout, int32_t ldx,
                             const double* mean, const double* V, const double* R, const double* y, double* yhat, double* S,
                             double* logw, int32_t reps, double* ms) {
  if (!dy || !mean || !V || !R || !y) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  if (dy_layout < 0 || dy_layout > 2) { set_error("dy_layout must be 0 (MATLAB order), 1 (rows on the stride ldx) or 2 (C-contiguous)"); return RBPF_ERR_INVALID_ARG; }
  RB_TRY(lg_validate_sizes(1, n_y, n_lin));
  if (n_p < 1 || n_p > kMaxParticles) { set_error("n_p must be in 1 .. 1048576"); return RBPF_ERR_INVALID_ARG; }
  if (dy_layout == 1 && ldx < n_lin) { set_error("ldx must be >= n_lin"); return RBPF_ERR_INVALID_ARG; }
  RB_TRY(lg_validate_R(R, n_y));
  if (!have_device()) { set_error("no HIP device"); return RBPF_ERR_NO_DEVICE; }
  const int n = n_lin, d = n_y, N = n_p;
  const int ld = dy_layout == 1 ? ldx : (dy_layout == 0 ? lg_ldx(n) : n);
  DevicePool tmp;
  double *d_dy = nullptr, *d_H = nullptr, *d_mean = nullptr, *d_V = nullptr, *d_R = nullptr, *d_y = nullptr;
  double *d_yhat = nullptr, *d_S = nullptr, *d_logw = nullptr;
  RB_TRY(tmp.upload(&d_dy, dy, (size_t)N * d * (dy_layout == 1 ? ld : n)));
  RB_TRY(tmp.upload(&d_mean, mean, (size_t)n));
  RB_TRY(tmp.upload(&d_V, V, (size_t)n * n));
  RB_TRY(tmp.upload(&d_R, R, (size_t)d * d));
  RB_TRY(tmp.upload(&d_y, y, (size_t)d));
  RB_TRY(tmp.alloc(&d_yhat, (size_t)N * d));
  RB_TRY(tmp.alloc(&d_S, (size_t)N * d * d));
  RB_TRY(tmp.alloc(&d_logw, (size_t)N));
  if (dy_layout == 0) {
    RB_TRY(tmp.alloc(&d_H, (size_t)N * d * ld));
    HIPCHK(launch_ext_pack_dy(0, N, d, n, ld, d_dy, d_H, 0));
  }
  LocGenArgs a;
  a.n = n; a.npart = N; a.ld = ld; a.H = dy_layout == 0 ? d_H : d_dy;
  a.mean = d_mean; a.V = d_V; a.R = d_R; a.y = d_y; a.yhat = d_yhat; a.S = d_S; a.logw = d_logw;
  RB_TRY(timed_reps(reps, 0, [&] { return launch_loc_generic_weights(d, a, 0); }, ms));
  if (yhat) HIPCHK(hipMemcpy(yhat, d_yhat, (size_t)N * d * sizeof(double), hipMemcpyDeviceToHost));
  if (S) HIPCHK(hipMemcpy(S, d_S, (size_t)N * d * d * sizeof(double), hipMemcpyDeviceToHost));
  if (logw) HIPCHK(hipMemcpy(logw, d_logw, (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
  return RBPF_OK;
}

}  // extern "C"
