// Backward-simulation smoother for localisation in a fixed map (forward filter, backward simulation: Godsill, Doucet & West 2004).
// In a fixed map the state (pos3 + quat4) is Markov, so M trajectories are drawn backwards through the stored forward particles
// X [T][7][N] and weights w [T][N] of a localisation context (keep_history = 1, trace = 1):
//     b[T-1][j] = sample(w[T-1], u[T-1][j]);   t = T-2 .. 0:  l_i = log w[t][i] + logp(xs[t+1][j] | X[t][:, i]),  b[t][j] = sample(p, u[t][j])
// with p the log-sum-exp normalisation of l (particleSmoother.m:232, :236-238, :241) and sample = #{i : cumsum(p)_i < u}
// (tools/sample.m:30-32).  logp is the density of dynModel as it draws (run_localization.m:274-281), constants omitted:
//     a_i = qRight(q_i) dq,  e = qLeft(qInv(a_i)) q~,  phi = logq(e),  r = [p~ - (p_i + dx(1:3)); phi],  z = blkdiag(S_pos, S_rot) \ r,  logp = -z'z / 2
// logq(e) = acos(e0) e_v / sin(acos(e0)) after the sign flip of tools/logq.m:26-28 is evaluated as atan2(|e_v|, e0) e_v / |e_v|: the
// same value for a unit e, without the cancellation of acos near 1.
//
// The recursion, its kernels, the SUMMATION ORDER and the PHILOX COUNTERS are those of rbpf_loc_backward.hpp; this file brings the
// dense-mag map's part of a step:
//   bs_prologue_kernel   Xhat[t][:, i] = (p_i + dx(1:3), a_i, log w_i): 8 doubles per particle, SoA, shared by all M trajectories.
//   BsTerm               logp of one pair: the position term, then the orientation term.  A pair whose log w + position term alone
//                        lies more than 746 below the running max skips its orientation term: its exp is exactly 0.
// The MAP trajectory (rbpf_loc_map_trajectory, the recursion and kernels of rbpf_loc_viterbi.hpp) runs on the same prologue and term,
// and so do the marginal smoothing weights (rbpf_loc_marginal_smooth, rbpf_loc_marginal.hpp), backward simulation by rejection
// sampling (rbpf_loc_backward_simulate_reject, rbpf_loc_reject.hpp) and the two-slice statistics of the transition residual
// (rbpf_loc_pair_stats_smooth, rbpf_loc_pairstats.hpp: BsTerm::pair_res hands out r = [p~ - (p_i + dx); phi]).
// The running statistics (rbpf_loc_forward_stats_update, rbpf_loc_forwardstats.hpp) walk the stored steps FORWARDS on the same
// prologue and term and keep their carry in the context (LocState::fs) between calls.
// The fixed-lag smoother (rbpf_loc_fixed_lag_update, rbpf_loc_fixedlag.hpp) does the same with the moments of the last `lag` states
// (LocState::fl).
#include "../../include/rbpf.h"
#include "rbpf_internal.hpp"
#include "rbpf_device.hpp"
#include "rbpf_ctx.hpp"
#include "rbpf_loc_state.hpp"
#include "rbpf_loc_backward.hpp"
#include "rbpf_loc_viterbi.hpp"
#include "rbpf_loc_marginal.hpp"
#include "rbpf_loc_pairstats.hpp"
#include "rbpf_loc_forwardstats.hpp"
#include "rbpf_loc_fixedlag.hpp"
#include "rbpf_loc_reject.hpp"
#include "rbpf_timed_reps.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace rbpf {

struct BsNoise { double ip[9], ir[9]; };   // inv(S_pos), inv(S_rot), row-major

__global__ void bs_prologue_kernel(int N, const double* __restrict__ xn, size_t cs, size_t ps, const double* __restrict__ w,
                                   const double* __restrict__ odo, double* __restrict__ Xhat) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  double q[4];
#pragma unroll
  for (int c = 0; c < 3; ++c) Xhat[(size_t)c * N + i] = xn[(size_t)c * cs + (size_t)i * ps] + odo[c];
#pragma unroll
  for (int c = 0; c < 4; ++c) q[c] = xn[(size_t)(3 + c) * cs + (size_t)i * ps];
  const double p[4] = {odo[3], odo[4], odo[5], odo[6]};
  // qRight(q) dq (tools/qRight.m:29-34), as loc_dyn_model_dev
  Xhat[(size_t)3 * N + i] = q[0] * p[0] + (-q[1]) * p[1] + (-q[2]) * p[2] + (-q[3]) * p[3];
  Xhat[(size_t)4 * N + i] = q[1] * p[0] + q[0] * p[1] + q[3] * p[2] + (-q[2]) * p[3];
  Xhat[(size_t)5 * N + i] = q[2] * p[0] + (-q[3]) * p[1] + q[0] * p[2] + q[1] * p[3];
  Xhat[(size_t)6 * N + i] = q[3] * p[0] + q[2] * p[1] + (-q[1]) * p[2] + q[0] * p[3];
  const double wi = w[i];
  Xhat[(size_t)7 * N + i] = wi > 0.0 ? log(wi) : -INFINITY;
}

// -z_pos'z_pos / 2 of one pair; h: the particle's 8 doubles (predicted position, a, log w), x: the trajectory's state; r (may be
// null): the un-whitened residual p~ - (p_i + dx), 3 doubles
__device__ __forceinline__ double bs_pos_term(const BsNoise& nz, const double* h, const double x[7], double* r = nullptr) {
  const double r0 = x[0] - h[0], r1 = x[1] - h[1], r2 = x[2] - h[2];
  if (r) { r[0] = r0; r[1] = r1; r[2] = r2; }
  const double z0 = nz.ip[0] * r0 + nz.ip[1] * r1 + nz.ip[2] * r2;
  const double z1 = nz.ip[3] * r0 + nz.ip[4] * r1 + nz.ip[5] * r2;
  const double z2 = nz.ip[6] * r0 + nz.ip[7] * r1 + nz.ip[8] * r2;
  return -0.5 * (z0 * z0 + z1 * z1 + z2 * z2);
}

// r (may be null): the un-whitened residual phi, 3 doubles
__device__ __forceinline__ double bs_rot_term(const BsNoise& nz, const double* h, const double x[7], double* r = nullptr) {
  // e = qLeft(qInv(a)) q~ (tools/qLeft.m:30-35, qInv.m:27-31)
  const double a0 = h[3], a1 = -h[4], a2 = -h[5], a3 = -h[6];
  double e0 = a0 * x[3] + (-a1) * x[4] + (-a2) * x[5] + (-a3) * x[6];
  double e1 = a1 * x[3] + a0 * x[4] + (-a3) * x[5] + a2 * x[6];
  double e2 = a2 * x[3] + a3 * x[4] + a0 * x[5] + (-a1) * x[6];
  double e3 = a3 * x[3] + (-a2) * x[4] + a1 * x[5] + a0 * x[6];
  if (e0 < 0.0) { e0 = -e0; e1 = -e1; e2 = -e2; e3 = -e3; }                       // tools/logq.m:26-28
  const double nv = sqrt(e1 * e1 + e2 * e2 + e3 * e3);
  const double f = (nv == 0.0) ? 1.0 : atan2(nv, e0) / nv;
  const double p0 = f * e1, p1 = f * e2, p2 = f * e3;
  if (r) { r[0] = p0; r[1] = p1; r[2] = p2; }
  const double z0 = nz.ir[0] * p0 + nz.ir[1] * p1 + nz.ir[2] * p2;
  const double z1 = nz.ir[3] * p0 + nz.ir[4] * p1 + nz.ir[5] * p2;
  const double z2 = nz.ir[6] * p0 + nz.ir[7] * p1 + nz.ir[8] * p2;
  return -0.5 * (z0 * z0 + z1 * z1 + z2 * z2);
}

// the dense-mag map's term: h = (predicted position, a, log w), x = the trajectory's state, all 7 rows
struct BsTerm {
  struct Head { int first; };                 // no integers of its own: all 7 rows, always
  static constexpr int NS = 7;
  static constexpr int NR = 6;                // residuals: [p~ - (p_i + dx); phi]
  static constexpr int kLocateBound = 1024;   // the default
  BsNoise nz;
  __device__ __forceinline__ double load_x(Head, const double* xs_next, int j, int k) const { return xs_next[(size_t)j * 7 + k]; }
  __device__ __forceinline__ double load_next(Head, const double* xn, int ld, int j, int k) const { return xn[(size_t)k * ld + j]; }   // particles [7][ld]
  static constexpr bool kSplit = true;        // the skip test sits between the two terms
  __device__ __forceinline__ double pair_near(Head, const double* h, const double (&x)[7]) const { return bs_pos_term(nz, h, x); }
  __device__ __forceinline__ double pair_far(Head, const double* h, const double (&x)[7]) const { return bs_rot_term(nz, h, x); }
  // pair_near, the test, pair_far; r: the un-whitened residual (rbpf_loc_pairstats.hpp)
  __device__ __forceinline__ bool pair_res(Head, const double* h, const double (&x)[7], double bound, double& l, double (&r)[6]) const {
    l += bs_pos_term(nz, h, x, r);
    if (l < bound) return false;
    l += bs_rot_term(nz, h, x, r + 3);
    return true;
  }
  __device__ __forceinline__ void gather(Head, const double* X, int N, int idx, double* xs, int j) const {
#pragma unroll
    for (int r = 0; r < 7; ++r) xs[(size_t)j * 7 + r] = X[(size_t)r * N + idx];
  }
};

// ---- host side -----------------------------------------------------------------------------------------------------------
static bool bs_inv3(const double* S, int ld, double* inv) {   // S column-major with leading dimension ld -> inv row-major
  const double a = S[0], b = S[ld], c = S[2 * ld], d = S[1], e = S[1 + ld], f = S[1 + 2 * ld], g = S[2], h = S[2 + ld], i = S[2 + 2 * ld];
  const double det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
  double scale = 0.0;
  for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) scale = std::max(scale, std::fabs(S[r + ld * k]));
  if (!(std::fabs(det) > 1e-12 * scale * scale * scale) || !std::isfinite(det)) return false;
  const double adj[9] = {e * i - f * h, c * h - b * i, b * f - c * e, f * g - d * i, a * i - c * g, c * d - a * f,
                         d * h - e * g, b * g - a * h, a * e - b * d};
  for (int k = 0; k < 9; ++k) inv[k] = adj[k] / det;
  return true;
}

// S: 6 x 6 column-major element-wise sqrt(dt Q) of the diagonal blocks (loc_noise_pages)
static int bs_noise(const double* S, BsNoise& nz) {
  if (!bs_inv3(S, 6, nz.ip) || !bs_inv3(S + 3 + 6 * 3, 6, nz.ir)) {
    set_error("a diagonal block of the element-wise sqrt(dt Q) is singular: the transition density of dynModel does not exist");
    return RBPF_ERR_INVALID_ARG;
  }
  return RBPF_OK;
}

static size_t bs_bytes(size_t N, size_t T, size_t M, bool full_xs) {
  const size_t nch = (N + backward_chunk_size((int)N, (int)M) - 1) / backward_chunk_size((int)N, (int)M);
  return (8 * N + 2 * nch * M + T * M + (full_xs ? T : 2) * 7 * M + 7 * T) * sizeof(double) + T * M * sizeof(int);
}

// prologue + all-pairs pass + locate of one step, in stream order
static hipError_t bs_launch_step(const BackwardArgs<BsTerm>& a, const double* xn, size_t cs, size_t ps, const double* w, const double* odo,
                                 double* Xhat, hipStream_t s) {
  hipLaunchKernelGGL(bs_prologue_kernel, dim3((a.N + 255) / 256), dim3(256), 0, s, a.N, xn, cs, ps, w, odo, Xhat);
  return backward_launch_step(a, s);
}

// prologue + delta over its log w + max-plus pass + merge of one MAP step: (best, arg) of every successor into delta_next / psi_next
static hipError_t bs_launch_map_step(const ViterbiArgs<BsTerm>& a, const double* xn, size_t cs, size_t ps, const double* w, const double* odo,
                                     const double* delta, double* Xhat, const double* w_next, double* delta_next, int* psi_next, hipStream_t s) {
  hipLaunchKernelGGL(bs_prologue_kernel, dim3((a.N + 255) / 256), dim3(256), 0, s, a.N, xn, cs, ps, w, odo, Xhat);
  const hipError_t e = viterbi_launch_pass(a, delta, Xhat, s);
  if (e != hipSuccess) return e;
  return viterbi_launch_merge(a.M, a.nchunks, a.part_best, a.part_arg, w_next, delta_next, psi_next, s);
}

// prologue + the two all-pairs passes and their merges of one marginal-smoothing step (rbpf_loc_marginal.hpp): c(j), D where wanted,
// and the un-normalised lws
static hipError_t bs_launch_marginal_step(const MarginalArgs<BsTerm>& a, const double* xn, size_t cs, size_t ps, const double* w, const double* odo,
                                          double* Xhat, const double* logws_next, double* D, double* cj, double* lws, hipStream_t s) {
  hipLaunchKernelGGL(bs_prologue_kernel, dim3((a.N + 255) / 256), dim3(256), 0, s, a.N, xn, cs, ps, w, odo, Xhat);
  return marginal_launch_step(a, logws_next, D, cj, lws, s);
}

}  // namespace rbpf

using namespace rbpf;

extern "C" {

int rbpf_loc_backward_workspace_bytes(int32_t N_P, int32_t N_T, int32_t n_traj, size_t* bytes) {
  if (!bytes) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  if (N_P < 1 || N_T < 1 || n_traj < 1) { set_error("N_P, N_T and n_traj must be >= 1"); return RBPF_ERR_INVALID_ARG; }
  if (N_P > kMaxParticles) { set_error("N_P above 1048576 is not supported"); return RBPF_ERR_UNSUPPORTED; }
  *bytes = bs_bytes((size_t)N_P, (size_t)N_T, (size_t)n_traj, true);
  return RBPF_OK;
}

int rbpf_loc_history(rbpf_ctx* c, double* xn_fwd) {
  if (!c || !c->loc) { set_error("not a localisation context"); return RBPF_ERR_INVALID_ARG; }
  if (!xn_fwd) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  if (!c->opt.keep_history) { set_error("rbpf_loc_history needs rbpf_options.keep_history"); return RBPF_ERR_STATE; }
  HIPCHK(hipSetDevice(c->device));
  const int N = c->N, Td = c->t, nN = c->loc->nN;
  if (Td == 0) return RBPF_OK;
  DevicePool tmp;
  double* d_tmp = nullptr;
  RB_TRY(tmp.alloc(&d_tmp, (size_t)nN * N * Td));
  for (int t = 0; t < Td; ++t) HIPCHK(launch_transpose_soa(N, nN, c->X + (size_t)t * nN * N, d_tmp + (size_t)t * nN * N, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpy(xn_fwd, d_tmp, (size_t)nN * N * Td * sizeof(double), hipMemcpyDeviceToHost));
  return RBPF_OK;
}

// rbpf_loc_backward_simulate (max_tries = -1: every step is the all-pairs pass) and rbpf_loc_backward_simulate_reject (max_tries >= 0:
// steps N_T-2 .. 0 by rbpf_loc_reject.hpp); `who` is how the entry point names itself in its refusals
static int bs_simulate(rbpf_ctx* c, int32_t n_traj, const double* u, uint64_t seed, int max_tries, double* xs_traj, int32_t* index,
                       double* traj_smooth_mean, int32_t* n_fallback, int64_t* n_tries, const char* who) {
  if (!c || !c->loc) { set_error("not a localisation context"); return RBPF_ERR_INVALID_ARG; }
  if (c->loc->generic) {
    set_error("backward simulation needs the transition density of dynModel: a generic map's dynModel is a sampler (its handles carry no density)");
    return RBPF_ERR_UNSUPPORTED;
  }
  if (n_traj < 1) { set_error("n_traj must be >= 1"); return RBPF_ERR_INVALID_ARG; }
  RB_TRY(backward_check_forward(c, who, who));
  LocState* L = c->loc;
  const int N = c->N, T = c->T, M = n_traj;
  const bool reject = max_tries >= 0;
  std::vector<BsNoise> nz((size_t)L->s_pages);
  {
    std::vector<double> S((size_t)L->s_pages * 36);
    HIPCHK(hipMemcpy(S.data(), L->d_S, S.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int p = 0; p < (T > 1 ? L->s_pages : 0); ++p) RB_TRY(bs_noise(S.data() + (size_t)p * 36, nz[p]));
  }
  const int C = backward_chunk_size(N, M), nch = (N + C - 1) / C;
  const bool full_xs = xs_traj != nullptr;
  // workspace from the context's pool, handed back on every way out
  BackwardWorkspace ws;
  BackwardWorkspaceGuard lease(ws);
  RB_TRY(ws.take(c->pool, (size_t)8 * N, reject ? reject_part_count(N, M) : (size_t)nch * M, (size_t)T * M, (size_t)(full_xs ? T : 2) * 7 * M,
                 (size_t)7 * T));
  RejectWorkspace rw;
  RejectWorkspaceGuard reject_lease(rw);
  if (reject) {
    RB_TRY(rw.take(c->pool, (size_t)N, reject_cdf_blocks(N), (size_t)M, 7, (size_t)T));
    HIPCHK(hipMemsetAsync(rw.n_fb, 0, (size_t)T * sizeof(int), c->stream));
    HIPCHK(hipMemsetAsync(rw.n_tries, 0, (size_t)T * sizeof(long long), c->stream));
  }
  RB_TRY(backward_uniforms(u, seed, T, M, ws.u, c->stream));
  auto slab = [&](int t) { return ws.xs + (size_t)(full_xs ? t : (t & 1)) * 7 * M; };
  for (int t = T - 1; t >= 0; --t) {
    BackwardArgs<BsTerm> a;
    a.N = N; a.M = M; a.C = C; a.nchunks = nch; a.head.first = (t == T - 1);
    a.Xhat = ws.Xhat; a.X = c->X + (size_t)t * 7 * N;
    a.xs_next = a.head.first ? nullptr : slab(t + 1);
    a.u = ws.u + (size_t)t * M; a.part_m = ws.pm; a.part_s = ws.ps;
    a.index = ws.idx + (size_t)t * M; a.xs = slab(t); a.clamped = c->d_flags + 1;
    if (!a.head.first) a.term.nz = nz[L->s_pages > 1 ? t : 0];
    else std::memset(&a.term.nz, 0, sizeof(a.term.nz));
    const double* odo = c->d_odo + (size_t)(a.head.first ? 0 : t) * 7;          // the draw of step T-1 reads log w only
    if (reject && !a.head.first) {
      hipLaunchKernelGGL(bs_prologue_kernel, dim3((N + 255) / 256), dim3(256), 0, c->stream, N, a.X, (size_t)N, (size_t)1, c->w + (size_t)t * N, odo, ws.Xhat);
      HIPCHK(reject_launch_step(a, rw, c->w + (size_t)t * N, 7, max_tries, nullptr, seed, t, rw.n_fb + t, rw.n_tries + t, c->stream));
    } else {
      HIPCHK(bs_launch_step(a, a.X, (size_t)N, 1, c->w + (size_t)t * N, odo, ws.Xhat, c->stream));
    }
    if (traj_smooth_mean) HIPCHK(backward_launch_mean(M, 7, slab(t), ws.mean + (size_t)t * 7, c->stream));
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  RB_TRY(ctx_check_flags(c));
  if (reject && n_fallback) HIPCHK(hipMemcpy(n_fallback, rw.n_fb, (size_t)T * sizeof(int), hipMemcpyDeviceToHost));
  if (reject && n_tries) HIPCHK(hipMemcpy(n_tries, rw.n_tries, (size_t)T * sizeof(long long), hipMemcpyDeviceToHost));
  if (xs_traj) HIPCHK(hipMemcpy(xs_traj, ws.xs, (size_t)7 * M * T * sizeof(double), hipMemcpyDeviceToHost));
  if (index) HIPCHK(hipMemcpy(index, ws.idx, (size_t)M * T * sizeof(int), hipMemcpyDeviceToHost));
  if (traj_smooth_mean) HIPCHK(hipMemcpy(traj_smooth_mean, ws.mean, (size_t)7 * T * sizeof(double), hipMemcpyDeviceToHost));
  return RBPF_OK;
}

int rbpf_loc_backward_simulate(rbpf_ctx* c, int32_t n_traj, const double* u, uint64_t seed, double* xs_traj, int32_t* index,
                               double* traj_smooth_mean) {
  return bs_simulate(c, n_traj, u, seed, -1, xs_traj, index, traj_smooth_mean, nullptr, nullptr, "rbpf_loc_backward_simulate");
}

int rbpf_loc_backward_reject_workspace_bytes(int32_t N_P, int32_t N_T, int32_t n_traj, size_t* bytes) {
  RB_TRY(rbpf_loc_backward_workspace_bytes(N_P, N_T, n_traj, bytes));
  const size_t nch = ((size_t)N_P + backward_chunk_size(N_P, n_traj) - 1) / backward_chunk_size(N_P, n_traj);
  *bytes += 2 * (reject_part_count(N_P, n_traj) - nch * (size_t)n_traj) * sizeof(double) + reject_bytes((size_t)N_P, (size_t)n_traj, 7, (size_t)N_T);
  return RBPF_OK;
}

int rbpf_loc_backward_simulate_reject(rbpf_ctx* c, int32_t n_traj, uint64_t seed, int32_t max_tries, double* xs_traj, int32_t* index,
                                      double* traj_smooth_mean, int32_t* n_fallback, int64_t* n_tries) {
  if (max_tries < 0 || max_tries > kRejectMaxTries) { set_error("max_tries must be in 0 .. 4194304"); return RBPF_ERR_INVALID_ARG; }
  return bs_simulate(c, n_traj, nullptr, seed, max_tries, xs_traj, index, traj_smooth_mean, n_fallback, n_tries, "rbpf_loc_backward_simulate_reject");
}

int rbpf_loc_backward_reject_step(int32_t N, int32_t M, const double* xn, const double* w, const double* xs_next, const double* odo, double dt,
                                  const double* Q, const double* u_try, const double* u, int32_t R, int32_t* index, int32_t* accepted_at,
                                  int32_t reps, double* ms) {
  if (!xn || !w || !xs_next || !odo || !Q || !u || !index) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  if (N < 1 || M < 1) { set_error("N and M must be >= 1"); return RBPF_ERR_INVALID_ARG; }
  if (R < 0 || R > kRejectMaxTries) { set_error("max_tries must be in 0 .. 4194304"); return RBPF_ERR_INVALID_ARG; }
  if (N > kMaxParticles) { set_error("N above 1048576 is not supported"); return RBPF_ERR_UNSUPPORTED; }
  double S[36];
  for (int q = 0; q < 36; ++q) S[q] = 0.0;
  for (int b = 0; b < 2; ++b)
    for (int cc = 0; cc < 3; ++cc)
      for (int r = 0; r < 3; ++r) {
        const int q = (3 * b + r) + 6 * (3 * b + cc);
        const double v = dt * Q[q];
        if (!(v >= 0.0)) { set_error("dt * Q has a negative entry in a diagonal block: the element-wise sqrt of dynModel would be complex"); return RBPF_ERR_INVALID_ARG; }
        S[q] = std::sqrt(v);
      }
  BackwardArgs<BsTerm> a;
  RB_TRY(bs_noise(S, a.term.nz));
  if (!have_device()) { set_error("no HIP device: the backward pass has no CPU fallback"); return RBPF_ERR_NO_DEVICE; }
  DevicePool tmp;
  RejectWorkspace rw;
  RejectWorkspaceGuard lease(rw);
  double *d_xn = nullptr, *d_w = nullptr, *d_xs = nullptr, *d_odo = nullptr, *d_u = nullptr, *d_ut = nullptr, *d_Xhat = nullptr, *d_pm = nullptr,
         *d_ps = nullptr;
  int *d_idx = nullptr, *d_clamped = nullptr;
  const size_t np = reject_part_count(N, M);
  RB_TRY(tmp.upload(&d_xn, xn, (size_t)7 * N));
  RB_TRY(tmp.upload(&d_w, w, (size_t)N));
  RB_TRY(tmp.upload(&d_xs, xs_next, (size_t)7 * M));
  RB_TRY(tmp.upload(&d_odo, odo, (size_t)7));
  RB_TRY(tmp.upload(&d_u, u, (size_t)M));
  if (R > 0 && u_try) RB_TRY(tmp.upload(&d_ut, u_try, (size_t)2 * M * R));   // (null: the device generator, seed 0, step 0)
  RB_TRY(tmp.alloc(&d_Xhat, (size_t)8 * N));
  RB_TRY(tmp.alloc(&d_pm, np));
  RB_TRY(tmp.alloc(&d_ps, np));
  RB_TRY(tmp.alloc(&d_idx, (size_t)M));
  RB_TRY(tmp.alloc(&d_clamped, (size_t)1));
  RB_TRY(rw.take(tmp, (size_t)N, reject_cdf_blocks(N), (size_t)M, 7, 1));
  HIPCHK(hipMemset(d_clamped, 0, sizeof(int)));
  a.N = N; a.M = M; a.C = backward_chunk_size(N, M); a.nchunks = (N + a.C - 1) / a.C; a.head.first = 0;
  a.Xhat = d_Xhat; a.X = nullptr; a.xs_next = d_xs; a.u = d_u; a.part_m = d_pm; a.part_s = d_ps; a.index = d_idx; a.xs = nullptr;
  a.clamped = d_clamped;
  RB_TRY(timed_reps(reps, 0, [&] {
    hipLaunchKernelGGL(bs_prologue_kernel, dim3((N + 255) / 256), dim3(256), 0, 0, N, d_xn, (size_t)1, (size_t)7, d_w, d_odo, d_Xhat);
    return reject_launch_step(a, rw, d_w, 7, R, d_ut, 0ull, 0, rw.n_fb, rw.n_tries, 0);
  }, ms));
  HIPCHK(hipMemcpy(index, d_idx, (size_t)M * sizeof(int), hipMemcpyDeviceToHost));
  if (accepted_at) {
    std::vector<int> acc((size_t)M), tr((size_t)M);
    HIPCHK(hipMemcpy(acc.data(), rw.acc, (size_t)M * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(tr.data(), rw.tries, (size_t)M * sizeof(int), hipMemcpyDeviceToHost));
    for (int j = 0; j < M; ++j) accepted_at[j] = acc[j] >= 0 ? tr[j] - 1 : -1;
  }
  return RBPF_OK;
}

int rbpf_loc_backward_step(int32_t N, int32_t M, const double* xn, const double* w, const double* xs_next, const double* odo, double dt,
                           const double* Q, const double* u, int32_t* index, double* logp, int32_t reps, double* ms) {
  if (!xn || !w || !xs_next || !odo || !Q || !u || !index) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  if (N < 1 || M < 1) { set_error("N and M must be >= 1"); return RBPF_ERR_INVALID_ARG; }
  if (N > kMaxParticles) { set_error("N above 1048576 is not supported"); return RBPF_ERR_UNSUPPORTED; }
  double S[36];
  for (int q = 0; q < 36; ++q) S[q] = 0.0;
  for (int b = 0; b < 2; ++b)
    for (int cc = 0; cc < 3; ++cc)
      for (int r = 0; r < 3; ++r) {
        const int q = (3 * b + r) + 6 * (3 * b + cc);
        const double v = dt * Q[q];
        if (!(v >= 0.0)) { set_error("dt * Q has a negative entry in a diagonal block: the element-wise sqrt of dynModel would be complex"); return RBPF_ERR_INVALID_ARG; }
        S[q] = std::sqrt(v);
      }
  BackwardArgs<BsTerm> a;
  RB_TRY(bs_noise(S, a.term.nz));
  if (!have_device()) { set_error("no HIP device: the backward pass has no CPU fallback"); return RBPF_ERR_NO_DEVICE; }
  const int C = backward_chunk_size(N, M), nch = (N + C - 1) / C;
  DevicePool tmp;
  double *d_xn = nullptr, *d_w = nullptr, *d_xs = nullptr, *d_odo = nullptr, *d_u = nullptr, *d_Xhat = nullptr, *d_pm = nullptr,
         *d_ps = nullptr, *d_lp = nullptr;
  int *d_idx = nullptr, *d_clamped = nullptr;
  RB_TRY(tmp.upload(&d_xn, xn, (size_t)7 * N));
  RB_TRY(tmp.upload(&d_w, w, (size_t)N));
  RB_TRY(tmp.upload(&d_xs, xs_next, (size_t)7 * M));
  RB_TRY(tmp.upload(&d_odo, odo, (size_t)7));
  RB_TRY(tmp.upload(&d_u, u, (size_t)M));
  RB_TRY(tmp.alloc(&d_Xhat, (size_t)8 * N));
  RB_TRY(tmp.alloc(&d_pm, (size_t)nch * M));
  RB_TRY(tmp.alloc(&d_ps, (size_t)nch * M));
  RB_TRY(tmp.alloc(&d_idx, (size_t)M));
  RB_TRY(tmp.alloc(&d_clamped, (size_t)1));
  HIPCHK(hipMemset(d_clamped, 0, sizeof(int)));
  if (logp) RB_TRY(tmp.alloc(&d_lp, (size_t)N * M));
  a.N = N; a.M = M; a.C = C; a.nchunks = nch; a.head.first = 0;
  a.Xhat = d_Xhat; a.X = nullptr; a.xs_next = d_xs; a.u = d_u; a.part_m = d_pm; a.part_s = d_ps; a.index = d_idx; a.xs = nullptr;
  a.clamped = d_clamped;
  RB_TRY(timed_reps(reps, 0, [&] { return bs_launch_step(a, d_xn, 1, 7, d_w, d_odo, d_Xhat, 0); }, ms));
  if (logp) HIPCHK(backward_launch_logp(a, d_lp, 0));
  HIPCHK(hipMemcpy(index, d_idx, (size_t)M * sizeof(int), hipMemcpyDeviceToHost));
  if (logp) HIPCHK(hipMemcpy(logp, d_lp, (size_t)N * M * sizeof(double), hipMemcpyDeviceToHost));
  return RBPF_OK;
}

int rbpf_loc_map_workspace_bytes(int32_t N_P, int32_t N_T, size_t* bytes) {
  if (!bytes) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  if (N_P < 1 || N_T < 1) { set_error("N_P and N_T must be >= 1"); return RBPF_ERR_INVALID_ARG; }
  if (N_P > kMaxParticles) { set_error("N_P above 1048576 is not supported"); return RBPF_ERR_UNSUPPORTED; }
  *bytes = viterbi_bytes(7, 7, (size_t)N_P, (size_t)N_T);
  return RBPF_OK;
}

int rbpf_loc_map_trajectory(rbpf_ctx* c, double* x_map, int32_t* index, double* score) {
  if (!c || !c->loc) { set_error("not a localisation context"); return RBPF_ERR_INVALID_ARG; }
  if (c->loc->generic) {
    set_error("the MAP trajectory needs the transition density of dynModel: a generic map's dynModel is a sampler (its handles carry no density)");
    return RBPF_ERR_UNSUPPORTED;
  }
  RB_TRY(backward_check_forward(c, "rbpf_loc_map_trajectory", "rbpf_loc_map_trajectory"));
  LocState* L = c->loc;
  const int N = c->N, T = c->T;
  std::vector<BsNoise> nz((size_t)L->s_pages);
  {
    std::vector<double> S((size_t)L->s_pages * 36);
    HIPCHK(hipMemcpy(S.data(), L->d_S, S.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int p = 0; p < (T > 1 ? L->s_pages : 0); ++p) RB_TRY(bs_noise(S.data() + (size_t)p * 36, nz[p]));
  }
  const int C = backward_chunk_size(N, N), nch = (N + C - 1) / C;
  BackwardWorkspace ws;
  BackwardWorkspaceGuard lease(ws);
  RB_TRY(viterbi_take(ws, c->pool, 7, 7, N, T));
  HIPCHK(viterbi_launch_init(N, c->w, ws.u, c->stream));
  for (int t = 0; t + 1 < T; ++t) {
    ViterbiArgs<BsTerm> a;
    a.N = N; a.M = N; a.C = C; a.nchunks = nch; a.head.first = 0;
    a.Xhat = ws.Xhat; a.xn_next = c->X + (size_t)(t + 1) * 7 * N; a.part_best = ws.pm; a.part_arg = ws.arg;
    a.term.nz = nz[L->s_pages > 1 ? t : 0];
    HIPCHK(bs_launch_map_step(a, c->X + (size_t)t * 7 * N, (size_t)N, 1, c->w + (size_t)t * N, c->d_odo + (size_t)t * 7,
                              ws.u + (size_t)(t & 1) * N, ws.Xhat, c->w + (size_t)(t + 1) * N, ws.u + (size_t)((t + 1) & 1) * N,
                              ws.idx + (size_t)(t + 1) * N, c->stream));
  }
  HIPCHK(viterbi_launch_backtrack(N, T, 7, c->X, ws.idx, ws.u + (size_t)((T - 1) & 1) * N, ws.mean, ws.idx + (size_t)T * N,
                                  ws.mean + (size_t)7 * T, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  RB_TRY(ctx_check_flags(c));
  return viterbi_copy_out(ws, 7, N, T, x_map, index, score);
}

int rbpf_loc_map_step(int32_t N, int32_t M, const double* xn, const double* delta, const double* xs_next, const double* odo, double dt,
                      const double* Q, double* best, int32_t* arg, int32_t reps, double* ms) {
  if (!xn || !delta || !xs_next || !odo || !Q || !best || !arg) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  if (N < 1 || M < 1) { set_error("N and M must be >= 1"); return RBPF_ERR_INVALID_ARG; }
  if (N > kMaxParticles || M > kMaxParticles) { set_error("N or M above 1048576 is not supported"); return RBPF_ERR_UNSUPPORTED; }
  double S[36];
  for (int q = 0; q < 36; ++q) S[q] = 0.0;
  for (int b = 0; b < 2; ++b)
    for (int cc = 0; cc < 3; ++cc)
      for (int r = 0; r < 3; ++r) {
        const int q = (3 * b + r) + 6 * (3 * b + cc);
        const double v = dt * Q[q];
        if (!(v >= 0.0)) { set_error("dt * Q has a negative entry in a diagonal block: the element-wise sqrt of dynModel would be complex"); return RBPF_ERR_INVALID_ARG; }
        S[q] = std::sqrt(v);
      }
  ViterbiArgs<BsTerm> a;
  RB_TRY(bs_noise(S, a.term.nz));
  if (!have_device()) { set_error("no HIP device: the MAP pass has no CPU fallback"); return RBPF_ERR_NO_DEVICE; }
  const int C = backward_chunk_size(N, M), nch = (N + C - 1) / C;
  std::vector<double> xt((size_t)7 * M);                                  // the successors as the history holds them: [7][M]
  for (int j = 0; j < M; ++j)
    for (int r = 0; r < 7; ++r) xt[(size_t)r * M + j] = xs_next[(size_t)j * 7 + r];
  DevicePool tmp;
  double *d_xn = nullptr, *d_delta = nullptr, *d_xs = nullptr, *d_odo = nullptr, *d_Xhat = nullptr, *d_pb = nullptr, *d_best = nullptr;
  int *d_pa = nullptr, *d_arg = nullptr;
  RB_TRY(tmp.upload(&d_xn, xn, (size_t)7 * N));
  RB_TRY(tmp.upload(&d_delta, delta, (size_t)N));
  RB_TRY(tmp.upload(&d_xs, xt.data(), (size_t)7 * M));
  RB_TRY(tmp.upload(&d_odo, odo, (size_t)7));
  RB_TRY(tmp.alloc(&d_Xhat, (size_t)8 * N));
  RB_TRY(tmp.alloc(&d_pb, (size_t)nch * M));
  RB_TRY(tmp.alloc(&d_pa, (size_t)nch * M));
  RB_TRY(tmp.alloc(&d_best, (size_t)M));
  RB_TRY(tmp.alloc(&d_arg, (size_t)M));
  a.N = N; a.M = M; a.C = C; a.nchunks = nch; a.head.first = 0;
  a.Xhat = d_Xhat; a.xn_next = d_xs; a.part_best = d_pb; a.part_arg = d_pa;
  // (the prologue's last row is overwritten with delta: what it reads as w does not matter)
  RB_TRY(timed_reps(reps, 0, [&] { return bs_launch_map_step(a, d_xn, 1, 7, d_delta, d_odo, d_delta, d_Xhat, nullptr, d_best, d_arg, 0); }, ms));
  HIPCHK(hipMemcpy(best, d_best, (size_t)M * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(arg, d_arg, (size_t)M * sizeof(int), hipMemcpyDeviceToHost));
  return RBPF_OK;
}

int rbpf_loc_marginal_workspace_bytes(int32_t N_P, int32_t N_T, size_t* bytes) {
  if (!bytes) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  if (N_P < 1 || N_T < 1) { set_error("N_P and N_T must be >= 1"); return RBPF_ERR_INVALID_ARG; }
  if (N_P > kMaxParticles) { set_error("N_P above 1048576 is not supported"); return RBPF_ERR_UNSUPPORTED; }
  *bytes = marginal_bytes(7, 7, (size_t)N_P, (size_t)N_T);
  return RBPF_OK;
}

// rbpf_loc_marginal_smooth (stats = false) and rbpf_loc_pair_stats_smooth (stats = true: after every step's normalisation the
// statistics pass of rbpf_loc_pairstats.hpp on the same Xhat, c and mass); `who` and `what` are how the entry point names itself
static int bs_marginal(rbpf_ctx* c, bool stats, double* w_smooth, double* mean, double* cov, double* ess, double* mass, double* S, double* m,
                       double* pair_mass, const char* who, const char* what) {
  if (!c || !c->loc) { set_error("not a localisation context"); return RBPF_ERR_INVALID_ARG; }
  if (c->loc->generic) {
    set_error(std::string(what) + " the transition density of dynModel: a generic map's dynModel is a sampler (its handles carry no density)");
    return RBPF_ERR_UNSUPPORTED;
  }
  RB_TRY(backward_check_forward(c, who, who));
  LocState* L = c->loc;
  const int N = c->N, T = c->T;
  std::vector<BsNoise> nz((size_t)L->s_pages);
  {
    std::vector<double> Sq((size_t)L->s_pages * 36);
    HIPCHK(hipMemcpy(Sq.data(), L->d_S, Sq.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int p = 0; p < (T > 1 ? L->s_pages : 0); ++p) RB_TRY(bs_noise(Sq.data() + (size_t)p * 36, nz[p]));
  }
  BackwardWorkspace ws;
  BackwardWorkspaceGuard lease(ws);
  RB_TRY(stats ? pair_stats_take(ws, c->pool, 7, 7, BsTerm::NR, N, T) : marginal_take(ws, c->pool, 7, 7, N, T));
  HIPCHK(marginal_launch_last(ws, 7, N, T, c->X, c->w, c->stream));
  for (int t = T - 2; t >= 0; --t) {
    MarginalArgs<BsTerm> a;
    marginal_set_sizes(a, N, N);
    a.head.first = 0;
    a.Xhat = ws.Xhat; a.xn_next = c->X + (size_t)(t + 1) * 7 * N; a.cj = ws.u + (size_t)2 * N; a.part_m = ws.pm; a.part_s = ws.ps;
    a.term.nz = nz[L->s_pages > 1 ? t : 0];
    HIPCHK(bs_launch_marginal_step(a, c->X + (size_t)t * 7 * N, (size_t)N, 1, c->w + (size_t)t * N, c->d_odo + (size_t)t * 7, ws.Xhat,
                                   ws.u + (size_t)((t + 1) & 1) * N, nullptr, ws.u + (size_t)2 * N, ws.u + (size_t)(t & 1) * N, c->stream));
    HIPCHK(marginal_launch_close_step(ws, 7, N, T, t, c->X, c->stream));
    if (stats) {
      PairStatsArgs<BsTerm> b;
      pair_stats_set_sizes(b, N, N);
      b.head = a.head; b.Xhat = a.Xhat; b.xn_next = a.xn_next; b.cj = a.cj; b.mass = marginal_out(ws, 7, T).mass + t; b.part = ws.pstat;
      b.term = a.term;
      HIPCHK(pair_stats_launch_step(b, ws.stat + (size_t)t * pair_stats_page(BsTerm::NR), c->stream));
    }
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  RB_TRY(ctx_check_flags(c));
  RB_TRY(marginal_copy_out(ws, 7, N, T, w_smooth, mean, cov, ess, mass));
  return stats ? pair_stats_copy_out(ws, BsTerm::NR, T, nullptr, S, m, pair_mass) : RBPF_OK;
}

int rbpf_loc_marginal_smooth(rbpf_ctx* c, double* w_smooth, double* mean, double* cov, double* ess, double* mass) {
  return bs_marginal(c, false, w_smooth, mean, cov, ess, mass, nullptr, nullptr, nullptr, "rbpf_loc_marginal_smooth", "marginal smoothing needs");
}

int rbpf_loc_pair_stats_workspace_bytes(int32_t N_P, int32_t N_T, size_t* bytes) {
  RB_TRY(rbpf_loc_marginal_workspace_bytes(N_P, N_T, bytes));
  *bytes = pair_stats_bytes(7, 7, BsTerm::NR, (size_t)N_P, (size_t)N_T);
  return RBPF_OK;
}

int rbpf_loc_pair_stats_smooth(rbpf_ctx* c, double* w_smooth, double* mean, double* cov, double* ess, double* mass, double* S, double* m,
                               double* pair_mass) {
  return bs_marginal(c, true, w_smooth, mean, cov, ess, mass, S, m, pair_mass, "rbpf_loc_pair_stats_smooth", "the transition statistics need");
}

// rbpf_loc_marginal_step (S, m and pair_mass null) and rbpf_loc_pair_stats_step: the marginal step, and behind it the normalisation
// of a copy of lws (the probes return lws un-normalised) and the statistics pass
static int bs_marginal_probe(int32_t N, int32_t M, const double* xn, const double* logw, const double* xs_next, const double* logws_next,
                             const double* odo, double dt, const double* Q, double* D, double* lws, bool stats, double* S, double* m,
                             double* pair_mass, int32_t reps, double* ms) {
  if (!xn || !logw || !xs_next || !logws_next || !odo || !Q || !D || !lws) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  if (stats && (!S || !m || !pair_mass)) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  if (N < 1 || M < 1) { set_error("N and M must be >= 1"); return RBPF_ERR_INVALID_ARG; }
  if (N > kMaxParticles || M > kMaxParticles) { set_error("N or M above 1048576 is not supported"); return RBPF_ERR_UNSUPPORTED; }
  double Sq[36];
  for (int q = 0; q < 36; ++q) Sq[q] = 0.0;
  for (int b = 0; b < 2; ++b)
    for (int cc = 0; cc < 3; ++cc)
      for (int r = 0; r < 3; ++r) {
        const int q = (3 * b + r) + 6 * (3 * b + cc);
        const double v = dt * Q[q];
        if (!(v >= 0.0)) { set_error("dt * Q has a negative entry in a diagonal block: the element-wise sqrt of dynModel would be complex"); return RBPF_ERR_INVALID_ARG; }
        Sq[q] = std::sqrt(v);
      }
  MarginalArgs<BsTerm> a;
  RB_TRY(bs_noise(Sq, a.term.nz));
  if (!have_device()) { set_error("no HIP device: the marginal pass has no CPU fallback"); return RBPF_ERR_NO_DEVICE; }
  marginal_set_sizes(a, N, M);
  std::vector<double> xt((size_t)7 * M);                                  // the successors as the history holds them: [7][M]
  for (int j = 0; j < M; ++j)
    for (int r = 0; r < 7; ++r) xt[(size_t)r * M + j] = xs_next[(size_t)j * 7 + r];
  DevicePool tmp;
  double *d_xn = nullptr, *d_lw = nullptr, *d_xs = nullptr, *d_lwn = nullptr, *d_odo = nullptr, *d_Xhat = nullptr, *d_pm = nullptr,
         *d_ps = nullptr, *d_D = nullptr, *d_c = nullptr, *d_lws = nullptr, *d_nrm = nullptr, *d_part = nullptr, *d_page = nullptr;
  const size_t np = marginal_part_count((size_t)N, (size_t)M);
  RB_TRY(tmp.upload(&d_xn, xn, (size_t)7 * N));
  RB_TRY(tmp.upload(&d_lw, logw, (size_t)N));
  RB_TRY(tmp.upload(&d_xs, xt.data(), (size_t)7 * M));
  RB_TRY(tmp.upload(&d_lwn, logws_next, (size_t)M));
  RB_TRY(tmp.upload(&d_odo, odo, (size_t)7));
  RB_TRY(tmp.alloc(&d_Xhat, (size_t)8 * N));
  RB_TRY(tmp.alloc(&d_pm, np));
  RB_TRY(tmp.alloc(&d_ps, np));
  RB_TRY(tmp.alloc(&d_D, (size_t)M));
  RB_TRY(tmp.alloc(&d_c, (size_t)M));
  RB_TRY(tmp.alloc(&d_lws, (size_t)N));
  a.head.first = 0;
  a.Xhat = d_Xhat; a.xn_next = d_xs; a.cj = d_c; a.part_m = d_pm; a.part_s = d_ps;
  PairStatsArgs<BsTerm> b;
  if (stats) {
    RB_TRY(tmp.alloc(&d_nrm, (size_t)2 * N + 1));                        // the normalised copy of lws, its weights, the mass
    RB_TRY(tmp.alloc(&d_part, (size_t)pair_stats_count(BsTerm::NR) * pair_stats_groups((size_t)N, (size_t)M)));
    RB_TRY(tmp.alloc(&d_page, (size_t)pair_stats_page(BsTerm::NR)));
    pair_stats_set_sizes(b, N, M);
    b.head = a.head; b.Xhat = d_Xhat; b.xn_next = d_xs; b.cj = d_c; b.mass = d_nrm + (size_t)2 * N; b.part = d_part; b.term = a.term;
  }
  RB_TRY(timed_reps(reps, 0, [&] {
    hipLaunchKernelGGL(bs_prologue_kernel, dim3((N + 255) / 256), dim3(256), 0, 0, N, d_xn, (size_t)1, (size_t)7, d_lw, d_odo, d_Xhat);
    // the caller's log w over the prologue's last row (what it read as w does not matter)
    hipError_t e = hipMemcpyAsync(d_Xhat + (size_t)7 * N, d_lw, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, 0);
    if (e != hipSuccess) return e;
    e = marginal_launch_step(a, d_lwn, d_D, d_c, d_lws, 0);
    if (e != hipSuccess || !stats) return e;
    e = hipMemcpyAsync(d_nrm, d_lws, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, 0);
    if (e != hipSuccess) return e;
    e = marginal_launch_normalise(N, d_nrm, d_nrm + N, d_nrm + (size_t)2 * N, 0);
    if (e != hipSuccess) return e;
    return pair_stats_launch_step(b, d_page, 0);
  }, ms));
  HIPCHK(hipMemcpy(D, d_D, (size_t)M * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(lws, d_lws, (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
  if (stats) {
    BackwardWorkspace view;
    view.stat = d_page;
    RB_TRY(pair_stats_copy_out(view, BsTerm::NR, 2, nullptr, S, m, pair_mass));
  }
  return RBPF_OK;
}

int rbpf_loc_marginal_step(int32_t N, int32_t M, const double* xn, const double* logw, const double* xs_next, const double* logws_next,
                           const double* odo, double dt, const double* Q, double* D, double* lws, int32_t reps, double* ms) {
  return bs_marginal_probe(N, M, xn, logw, xs_next, logws_next, odo, dt, Q, D, lws, false, nullptr, nullptr, nullptr, reps, ms);
}

int rbpf_loc_pair_stats_step(int32_t N, int32_t M, const double* xn, const double* logw, const double* xs_next, const double* logws_next,
                             const double* odo, double dt, const double* Q, double* D, double* lws, double* S, double* m, double* pair_mass,
                             int32_t reps, double* ms) {
  return bs_marginal_probe(N, M, xn, logw, xs_next, logws_next, odo, dt, Q, D, lws, true, S, m, pair_mass, reps, ms);
}

// ---- the running two-slice statistics (rbpf_loc_forwardstats.hpp) ------------------------------------------------------------
int rbpf_loc_forward_stats_workspace_bytes(int32_t N_P, int32_t N_T, size_t* bytes) {
  RB_TRY(rbpf_loc_marginal_workspace_bytes(N_P, N_T, bytes));           // its argument checks
  *bytes = forward_stats_bytes(7, BsTerm::NR, (size_t)N_P, (size_t)N_T);
  return RBPF_OK;
}

int rbpf_loc_forward_stats_reset(rbpf_ctx* c) {
  if (!c || !c->loc) { set_error("not a localisation context"); return RBPF_ERR_INVALID_ARG; }
  if (c->loc->generic) { set_error("a generic localisation context has rbpf_loc_generic_forward_stats_reset"); return RBPF_ERR_INVALID_ARG; }
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->loc->fs.release();
  return RBPF_OK;
}

int rbpf_loc_forward_stats_update(rbpf_ctx* c, double* S_run, double* m_run, double* mass_run, double* tau_S, double* tau_m) {
  if (!c || !c->loc) { set_error("not a localisation context"); return RBPF_ERR_INVALID_ARG; }
  if (c->loc->generic) {
    set_error("the running statistics need the transition density of dynModel: a generic map's dynModel is a sampler (its handles carry no density)");
    return RBPF_ERR_UNSUPPORTED;
  }
  RB_TRY(forward_stats_check_forward(c, "rbpf_loc_forward_stats_update"));
  LocState* L = c->loc;
  ForwardCarry& f = L->fs;
  const int N = c->N, T = c->T, Td = c->t;
  std::vector<BsNoise> nz((size_t)L->s_pages);
  {
    std::vector<double> Sq((size_t)L->s_pages * 36);
    HIPCHK(hipMemcpy(Sq.data(), L->d_S, Sq.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int p = 0; p < L->s_pages; ++p) RB_TRY(bs_noise(Sq.data() + (size_t)p * 36, nz[p]));
  }
  for (int t = f.alive ? f.folded : 0; t + 1 < Td; ++t)
    if (!(c->h_dt[c->dt_len > 1 ? t : 0] > 0.0)) { set_error("dt of step " + std::to_string(t) + " is not positive: S / dt does not exist"); return RBPF_ERR_INVALID_ARG; }
  if (!f.alive) RB_TRY(forward_stats_take(f, c->pool, 7, 7, BsTerm::NR, N, N, T - 1, c->stream));
  constexpr size_t KF = (size_t)forward_stats_carry(BsTerm::NR);
  for (int t = f.folded; t + 1 < Td; ++t) {
    MarginalArgs<BsTerm> a;
    ForwardStatsArgs<BsTerm> b;
    forward_stats_set(f, N, N, a, b);
    a.head.first = 0; b.head = a.head;
    a.xn_next = b.xn_next = c->X + (size_t)(t + 1) * 7 * N;
    a.term.nz = b.term.nz = nz[L->s_pages > 1 ? t : 0];
    b.tau = f.tau + (size_t)f.cur * KF * N;
    b.s_scale = 1.0 / c->h_dt[c->dt_len > 1 ? t : 0];
    hipLaunchKernelGGL(bs_prologue_kernel, dim3((N + 255) / 256), dim3(256), 0, c->stream, N, c->X + (size_t)t * 7 * N, (size_t)N, (size_t)1,
                       c->w + (size_t)t * N, c->d_odo + (size_t)t * 7, f.Xhat);
    HIPCHK(forward_stats_launch_step(a, b, f.zero, f.D, f.cj, f.tau + (size_t)(f.cur ^ 1) * KF * N, f.reach, c->w + (size_t)(t + 1) * N,
                                     f.pages + (size_t)t * pair_stats_page(BsTerm::NR), c->stream));
    f.cur ^= 1;
    f.folded = t + 1;
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  RB_TRY(ctx_check_flags(c));
  return forward_stats_copy_out(f, N, nullptr, S_run, m_run, mass_run, tau_S, tau_m);
}

// One step on the caller's arrays, the kernel-level probe
int rbpf_loc_forward_stats_step(int32_t N, int32_t M, const double* xn, const double* logw, const double* xs_next, const double* tau_S,
                                const double* tau_m, const double* odo, double dt, const double* Q, double* D, double* tau_S_next,
                                double* tau_m_next, double* reach, int32_t reps, double* ms) {
  if (!xn || !logw || !xs_next || !tau_S || !tau_m || !odo || !Q || !D || !tau_S_next || !tau_m_next || !reach) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  if (N < 1 || M < 1) { set_error("N and M must be >= 1"); return RBPF_ERR_INVALID_ARG; }
  if (N > kMaxParticles || M > kMaxParticles) { set_error("N or M above 1048576 is not supported"); return RBPF_ERR_UNSUPPORTED; }
  if (!(dt > 0.0)) { set_error("dt must be positive"); return RBPF_ERR_INVALID_ARG; }
  double Sq[36];
  for (int q = 0; q < 36; ++q) Sq[q] = 0.0;
  for (int b = 0; b < 2; ++b)
    for (int cc = 0; cc < 3; ++cc)
      for (int r = 0; r < 3; ++r) {
        const int q = (3 * b + r) + 6 * (3 * b + cc);
        const double v = dt * Q[q];
        if (!(v >= 0.0)) { set_error("dt * Q has a negative entry in a diagonal block: the element-wise sqrt of dynModel would be complex"); return RBPF_ERR_INVALID_ARG; }
        Sq[q] = std::sqrt(v);
      }
  MarginalArgs<BsTerm> a;
  ForwardStatsArgs<BsTerm> b;
  RB_TRY(bs_noise(Sq, a.term.nz));
  if (!have_device()) { set_error("no HIP device: the running statistics have no CPU fallback"); return RBPF_ERR_NO_DEVICE; }
  constexpr int NR = BsTerm::NR;
  constexpr size_t KF = (size_t)forward_stats_carry(NR);
  const size_t ld = (size_t)std::max(N, M);
  std::vector<double> xt((size_t)7 * M), tk(KF * N);                      // the successors as the history holds them: [7][M]
  for (int j = 0; j < M; ++j)
    for (int r = 0; r < 7; ++r) xt[(size_t)r * M + j] = xs_next[(size_t)j * 7 + r];
  forward_stats_pack(NR, N, nullptr, tau_S, tau_m, tk.data());
  DevicePool tmp;
  ForwardCarry f;
  RB_TRY(forward_stats_take(f, tmp, 7, 7, NR, N, M, 1, 0));
  double *d_xn = nullptr, *d_lw = nullptr, *d_xs = nullptr, *d_odo = nullptr, *d_wn = nullptr;
  RB_TRY(tmp.upload(&d_xn, xn, (size_t)7 * N));
  RB_TRY(tmp.upload(&d_lw, logw, (size_t)N));
  RB_TRY(tmp.upload(&d_xs, xt.data(), (size_t)7 * M));
  RB_TRY(tmp.upload(&d_odo, odo, (size_t)7));
  RB_TRY(tmp.alloc(&d_wn, (size_t)M));
  HIPCHK(hipMemcpy(f.tau, tk.data(), tk.size() * sizeof(double), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(forward_stats_fill_kernel, dim3((M + 255) / 256), dim3(256), 0, 0, M, 1.0 / M, d_wn);   // (the reducer's weights: uniform)
  forward_stats_set(f, N, M, a, b);
  a.head.first = 0; b.head = a.head;
  a.xn_next = b.xn_next = d_xs;
  b.term = a.term; b.tau = f.tau; b.s_scale = 1.0 / dt;
  double* tau_next = f.tau + KF * ld;
  RB_TRY(timed_reps(reps, 0, [&] {
    hipLaunchKernelGGL(bs_prologue_kernel, dim3((N + 255) / 256), dim3(256), 0, 0, N, d_xn, (size_t)1, (size_t)7, d_lw, d_odo, f.Xhat);
    // the caller's log w over the prologue's last row (what it read as w does not matter)
    const hipError_t e = hipMemcpyAsync(f.Xhat + (size_t)7 * N, d_lw, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, 0);
    if (e != hipSuccess) return e;
    return forward_stats_launch_step(a, b, f.zero, f.D, f.cj, tau_next, f.reach, d_wn, f.pages, 0);
  }, ms));
  std::vector<double> tn(KF * M);
  HIPCHK(hipMemcpy(D, f.D, (size_t)M * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(reach, f.reach, (size_t)M * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(tn.data(), tau_next, tn.size() * sizeof(double), hipMemcpyDeviceToHost));
  forward_stats_unpack(NR, M, nullptr, tn.data(), tau_S_next, tau_m_next);
  return RBPF_OK;
}

// ---- the fixed-lag smoother (rbpf_loc_fixedlag.hpp) ------------------------------------------------------------------------------
int rbpf_loc_fixed_lag_workspace_bytes(int32_t N_P, int32_t N_T, int32_t lag, int32_t moments, size_t* bytes) {
  RB_TRY(rbpf_loc_marginal_workspace_bytes(N_P, N_T, bytes));           // its argument checks
  RB_TRY(fixed_lag_check_lag(lag, moments));
  *bytes = fixed_lag_bytes(7, 7, (size_t)lag, (size_t)moments, (size_t)N_P, (size_t)N_T);
  return RBPF_OK;
}

int rbpf_loc_fixed_lag_reset(rbpf_ctx* c) {
  if (!c || !c->loc) { set_error("not a localisation context"); return RBPF_ERR_INVALID_ARG; }
  if (c->loc->generic) { set_error("a generic localisation context has rbpf_loc_generic_fixed_lag_reset"); return RBPF_ERR_INVALID_ARG; }
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->loc->fl.release();
  return RBPF_OK;
}

int rbpf_loc_fixed_lag_update(rbpf_ctx* c, int32_t lag, int32_t moments, double* pages, double* means) {
  if (!c || !c->loc) { set_error("not a localisation context"); return RBPF_ERR_INVALID_ARG; }
  if (c->loc->generic) {
    set_error("the fixed-lag smoother needs the transition density of dynModel: a generic map's dynModel is a sampler (its handles carry no density)");
    return RBPF_ERR_UNSUPPORTED;
  }
  RB_TRY(fixed_lag_check_lag(lag, moments));
  RB_TRY(forward_stats_check_forward(c, "rbpf_loc_fixed_lag_update"));
  LocState* L = c->loc;
  FixedLagCarry& f = L->fl;
  if (f.alive) RB_TRY(fixed_lag_same(f, lag, moments, "rbpf_loc_fixed_lag_reset"));
  const int N = c->N, T = c->T, Td = c->t;
  std::vector<BsNoise> nz((size_t)L->s_pages);
  {
    std::vector<double> Sq((size_t)L->s_pages * 36);
    HIPCHK(hipMemcpy(Sq.data(), L->d_S, Sq.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int p = 0; p < L->s_pages; ++p) RB_TRY(bs_noise(Sq.data() + (size_t)p * 36, nz[p]));
  }
  if (!f.alive) {
    const int H = fixed_lag_columns(7, moments);
    RB_TRY(fixed_lag_take(f, c->pool, 7, 7, lag * H, H, N, N, T, c->stream));
    f.lag = lag; f.moments = moments;
  }
  const size_t half = (size_t)(f.K + f.H) * N, page = (size_t)f.K + f.H + 1;
  if (f.entered == 0) {
    HIPCHK(fixed_lag_launch_enter(f, moments, N, c->X, c->w, f.T + (size_t)f.cur * half, nullptr, f.cs, f.pages, c->stream));
    f.entered = 1;
  }
  for (int t = f.entered - 1; t + 1 < Td; ++t) {
    MarginalArgs<BsTerm> a;
    FixedLagArgs<BsTerm> b;
    fixed_lag_set(f, N, N, a, b);
    a.head.first = 0; b.head = a.head;
    a.xn_next = b.xn_next = c->X + (size_t)(t + 1) * 7 * N;
    a.term.nz = b.term.nz = nz[L->s_pages > 1 ? t : 0];
    b.tau = f.T + (size_t)f.cur * half;
    hipLaunchKernelGGL(bs_prologue_kernel, dim3((N + 255) / 256), dim3(256), 0, c->stream, N, c->X + (size_t)t * 7 * N, (size_t)N, (size_t)1,
                       c->w + (size_t)t * N, c->d_odo + (size_t)t * 7, f.Xhat);
    HIPCHK(fixed_lag_launch_step(a, b, f, moments, c->X + (size_t)(t + 1) * 7 * N, c->w + (size_t)(t + 1) * N, f.T + (size_t)(f.cur ^ 1) * half,
                                 f.cs + (size_t)(t + 1) * 7, f.pages + (size_t)(t + 1) * page, c->stream));
    f.cur ^= 1;
    f.entered = t + 2;
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  RB_TRY(ctx_check_flags(c));
  return fixed_lag_copy_out(f, pages, means);
}

// One step on the caller's arrays, the kernel-level probe
int rbpf_loc_fixed_lag_step(int32_t N, int32_t M, int32_t K, int32_t moments, const double* xn, const double* logw, const double* xs_next,
                            const double* tau, const double* odo, double dt, const double* Q, double* D, double* tau_next, double* reach,
                            int32_t reps, double* ms) {
  if (!xn || !logw || !xs_next || !tau || !odo || !Q || !D || !tau_next || !reach) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  if (N < 1 || M < 1 || K < 1) { set_error("N, M and K must be >= 1"); return RBPF_ERR_INVALID_ARG; }
  if (N > kMaxParticles || M > kMaxParticles || K > kFixedLagMaxLag * fixed_lag_columns(kBackwardMaxRows, 2)) { set_error("N or M above 1048576 or K above 64 x 44 is not supported"); return RBPF_ERR_UNSUPPORTED; }
  RB_TRY(fixed_lag_check_lag(1, moments));
  if (!(dt > 0.0)) { set_error("dt must be positive"); return RBPF_ERR_INVALID_ARG; }
  double Sq[36];
  for (int q = 0; q < 36; ++q) Sq[q] = 0.0;
  for (int b = 0; b < 2; ++b)
    for (int cc = 0; cc < 3; ++cc)
      for (int r = 0; r < 3; ++r) {
        const int q = (3 * b + r) + 6 * (3 * b + cc);
        const double v = dt * Q[q];
        if (!(v >= 0.0)) { set_error("dt * Q has a negative entry in a diagonal block: the element-wise sqrt of dynModel would be complex"); return RBPF_ERR_INVALID_ARG; }
        Sq[q] = std::sqrt(v);
      }
  MarginalArgs<BsTerm> a;
  FixedLagArgs<BsTerm> b;
  RB_TRY(bs_noise(Sq, a.term.nz));
  if (!have_device()) { set_error("no HIP device: the fixed-lag smoother has no CPU fallback"); return RBPF_ERR_NO_DEVICE; }
  const int H = fixed_lag_columns(7, moments);
  const size_t ld = (size_t)std::max(N, M);
  std::vector<double> xt((size_t)7 * M);                                  // the successors as the history holds them: [7][M]
  for (int j = 0; j < M; ++j)
    for (int r = 0; r < 7; ++r) xt[(size_t)r * M + j] = xs_next[(size_t)j * 7 + r];
  DevicePool tmp;
  FixedLagCarry f;
  RB_TRY(fixed_lag_take(f, tmp, 7, 7, K, H, N, M, 1, 0));
  double *d_xn = nullptr, *d_lw = nullptr, *d_xs = nullptr, *d_odo = nullptr, *d_wn = nullptr;
  RB_TRY(tmp.upload(&d_xn, xn, (size_t)7 * N));
  RB_TRY(tmp.upload(&d_lw, logw, (size_t)N));
  RB_TRY(tmp.upload(&d_xs, xt.data(), (size_t)7 * M));
  RB_TRY(tmp.upload(&d_odo, odo, (size_t)7));
  RB_TRY(tmp.alloc(&d_wn, (size_t)M));
  HIPCHK(hipMemcpy(f.T, tau, (size_t)K * N * sizeof(double), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(forward_stats_fill_kernel, dim3((M + 255) / 256), dim3(256), 0, 0, M, 1.0 / M, d_wn);   // (the reducer's weights: uniform)
  fixed_lag_set(f, N, M, a, b);
  a.head.first = 0; b.head = a.head;
  a.xn_next = b.xn_next = d_xs;
  b.term = a.term; b.tau = f.T;
  double* T_next = f.T + (size_t)(K + H) * ld;
  RB_TRY(timed_reps(reps, 0, [&] {
    hipLaunchKernelGGL(bs_prologue_kernel, dim3((N + 255) / 256), dim3(256), 0, 0, N, d_xn, (size_t)1, (size_t)7, d_lw, d_odo, f.Xhat);
    // the caller's log w over the prologue's last row (what it read as w does not matter)
    const hipError_t e = hipMemcpyAsync(f.Xhat + (size_t)7 * N, d_lw, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, 0);
    if (e != hipSuccess) return e;
    return fixed_lag_launch_step(a, b, f, moments, d_xs, d_wn, T_next, f.cs, f.pages, 0);
  }, ms));
  HIPCHK(hipMemcpy(D, f.D, (size_t)M * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(reach, f.reach, (size_t)M * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(tau_next, T_next + (size_t)H * M, (size_t)K * M * sizeof(double), hipMemcpyDeviceToHost));
  return RBPF_OK;
}

}  // extern "C"
