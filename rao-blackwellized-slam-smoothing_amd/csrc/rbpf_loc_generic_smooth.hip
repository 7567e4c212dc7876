// Backward-simulation smoother in the fixed map of a generic device-code model (forward filter, backward simulation: Godsill,
// Doucet & West 2004), for a dynModel that is a drift plus Gaussian noise on some rows of the state:
//     x'[rows] = mean(x) + L z,   L L' = cov,   z ~ N(0, I)
// The recursion is that of rbpf_loc_backward.hpp on the stored particles X [T][n_nonlin][N] and weights w [T][N] of a generic
// localisation context (keep_history = 1, trace = 1):
//     b[T-1][j] = sample(w[T-1], u[T-1][j]);   t = T-2 .. 0:  l_i = log w[t][i] + logp(xs[t+1][j] | X[t][:, i]),  b[t][j] = sample(p, u[t][j])
// with the density, constants omitted (particleSmoother.m:181-182),
//     r = wrap(x'[rows] - mu_i),   z = L \ r = W r,   logp = -z'z / 2,        wrap(r) = r - 2 pi rint(r / (2 pi)) on the angle rows
// mu_i = mean(X[t][:, i]) comes from the caller's device code, one call per step with N columns: the pass is driven step by step
// (begin / particles_device / step_device / finish), as the forward filter of such a context is.  W = inv(L) is lower triangular,
// inverted on the host in fp64, and travels in the kernel arguments (n_res (n_res + 1) / 2 values, uniform: SGPRs).
//
// The recursion's kernels, the SUMMATION ORDER and the PHILOX COUNTERS are those of rbpf_loc_backward.hpp; this file brings a
// Gaussian transition's part of a step:
//   gs_prologue_kernel        Xhat[t] = (mu rows .., log w_i): n_res + 1 doubles per particle, SoA, shared by all M trajectories.
//                             (gs_prologue_pose_kernel: the n_sel rows of mu in kernel order, see POSE STATES below.)
//   GsTerm<NR, ANG, QP>       logp of one pair (gs_term, gs_pose_term: explicit fma throughout, no contraction is left to the
//                             compiler, so the pass and the locate walk see the SAME terms).  A lane keeps the trajectory's selected
//                             rows only; the gather takes all n_nonlin rows.  The partial sums of z_k^2 only lower l, so after the
//                             first NR / 2 rows of W a pair more than 746 below the running max skips the rest: its exp is exactly 0,
//                             wherever the test sits.
//
// POSE STATES (rbpf_loc_generic_backward_pose_*): four of the selected rows may be a unit quaternion (q0 .. q3, scalar first), whose
// noise multiplies the predicted quaternion mu_q on the right (run_dense3D_magfield.m:202-203, run_localization.m:274-281).  In
// the block's place the residual has the three entries
//     e = qInv(mu_q) (x) x'_q,   e <- -e if e0 < 0,   phi = atan2(|e_v|, e0) e_v / |e_v|   (phi = 0 if |e_v| = 0)
// = logq(e) of tools/logq.m for a unit e, in the form of rbpf_loc_smooth.hip.  n_sel = n_res + 1 rows are selected, Xhat and the
// LDS tile hold n_sel + 1 doubles per particle.  KERNEL ORDER: the plain rows first, in the caller's order, the block last; the
// host permutes rows, the angle bits, the rows of mu (in the prologue) and cov (symmetrically, before the factorisation) to it --
// z'z does not depend on the order.  W is lower triangular, so the plain rows of z are final before the block is touched, and the
// skip test sits there, after all NP plain rows and before the quaternion product and atan2 (NP = 0: no test).  The template
// parameter QP of the term is NP with a block and -1 without one; with -1 the pair is gs_term.
//
// THE MAP TRAJECTORY (rbpf_loc_generic_map_*): the Viterbi recursion of rbpf_loc_viterbi.hpp on the same prologues, terms, layout and
// factorisation, driven forwards in time (begin / particles_device / step_device for t = 0 .. N_T-2 / finish).
//
// THE MARGINAL SMOOTHING WEIGHTS (rbpf_loc_generic_marginal_*): the recursion of rbpf_loc_marginal.hpp on the same prologues, terms,
// layout and factorisation, driven backwards in time (begin / particles_device / step_device for t = N_T-2 .. 0 / finish).
//
// THE TWO-SLICE STATISTICS (rbpf_loc_generic_pair_stats_*): the marginal pass, and behind every step's normalisation the pass of
// rbpf_loc_pairstats.hpp on the same Xhat, c and mass; GsTerm::pair_res hands out the un-whitened residual in kernel order, and the
// host puts S and m back into the caller's order (LocGenLayout::perm) when it copies out.
//
// THE RUNNING STATISTICS (rbpf_loc_generic_forward_stats_*): the forward-only recursion of rbpf_loc_forwardstats.hpp on the same
// prologues and terms, driven FORWARDS in time from the first pair of steps not yet folded in (begin / particles_device / step_device
// / finish); its carry stays in the context (LocState::fs) between calls, and only between begin and finish does it count as an open
// pass.
//
// THE FIXED-LAG SMOOTHER (rbpf_loc_generic_fixed_lag_*): the recursion of rbpf_loc_fixedlag.hpp driven the same way, FORWARDS; its
// carry is LocState::fl, and between begin and finish it counts as one more kind of open pass.
//
// REJECTION SAMPLING (rbpf_loc_generic_backward_reject_begin): the pass that rbpf_loc_reject.hpp puts in front of the all-pairs pass
// at steps N_T-2 .. 0, on the same prologues and terms, driven by the same particles_device / step_device / finish.
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

constexpr int kGsMaxRes = 8, kGsMaxNonlin = kBackwardMaxRows;
constexpr double kGsTwoPi = 6.283185307179586476925286766559;

struct GsW { double w[kGsMaxRes * (kGsMaxRes + 1) / 2]; };   // W = inv(L), lower: W(k, c) at w[k (k + 1) / 2 + c], c <= k

// what every instantiation of the term carries (uniform: SGPRs): the integers that BackwardArgs keeps behind the sizes, and W
struct GsHead {
  int nN;                          // rows of a state
  int first;                       // 1: the draw of step T-1, l_i = log w_i
  unsigned angle_mask;             // bit k: residual row k is an angle
  int rows[kGsMaxRes];             // the state rows that carry noise
};
struct GsData {
  typedef GsHead Head;
  GsW W;
};

__global__ void gs_prologue_kernel(int N, int NR, const double* __restrict__ mu, const double* __restrict__ w, double* __restrict__ Xhat) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  for (int k = 0; k < NR; ++k) Xhat[(size_t)k * N + i] = mu ? mu[(size_t)k * N + i] : 0.0;
  const double wi = w[i];
  Xhat[(size_t)NR * N + i] = wi > 0.0 ? log(wi) : -INFINITY;
}

// l <- l - z'z / 2 of one pair; h: the particle's NR + 1 doubles (predicted rows, log w), x: the trajectory's selected rows.
// false: after NR / 2 rows the pair already lies below `bound` (l is then not final).  Every product-sum is an explicit fma.
// rout (may be null): where a pair that is not skipped leaves its un-whitened residual r, NR doubles (pair_res).
template <int NR, bool ANG>
__device__ __forceinline__ bool gs_term(const GsW& W, unsigned amask, const double* h, const double (&x)[NR], double bound, double& l,
                                        double* rout = nullptr) {
  constexpr int KT = NR / 2;
  double r[NR];
#pragma unroll
  for (int k = 0; k < NR; ++k) {
    double d = x[k] - h[k];
    if (ANG && ((amask >> k) & 1u)) d = fma(-kGsTwoPi, rint(d / kGsTwoPi), d);
    r[k] = d;
  }
  double q = 0.0;
#pragma unroll
  for (int k = 0; k < NR; ++k) {
    double z = W.w[k * (k + 1) / 2] * r[0];
#pragma unroll
    for (int c = 1; c <= k; ++c) z = fma(W.w[k * (k + 1) / 2 + c], r[c], z);
    q = fma(z, z, q);
    if (k + 1 == KT && fma(-0.5, q, l) < bound) return false;
  }
  l = fma(-0.5, q, l);
  if (rout) {
#pragma unroll
    for (int k = 0; k < NR; ++k) rout[k] = r[k];
  }
  return true;
}

struct GsSrc { int s[kGsMaxRes]; };        // kernel row k of Xhat is row s[k] of the caller's mu

// the prologue of a transition with a quaternion block: NS = n_sel rows of mu, taken in kernel order
__global__ void gs_prologue_pose_kernel(int N, int NS, GsSrc src, const double* __restrict__ mu, const double* __restrict__ w,
                                        double* __restrict__ Xhat) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  for (int k = 0; k < NS; ++k) Xhat[(size_t)k * N + i] = mu ? mu[(size_t)src.s[k] * N + i] : 0.0;
  const double wi = w[i];
  Xhat[(size_t)NS * N + i] = wi > 0.0 ? log(wi) : -INFINITY;
}

// gs_term with a quaternion block behind NP plain rows: h = (NP predicted plain rows, the predicted unit quaternion, log w),
// x = the trajectory's NP plain rows and its quaternion; NR = NP + 3 residuals.  false: the plain rows alone put the pair below
// `bound` (NP >= 1 only).  Every product-sum is an explicit fma; e = qLeft(qInv(mu_q)) x_q (tools/qLeft.m:30-35, qInv.m:27-31)
// is summed left to right, as bs_rot_term writes it.
// rout (may be null): where a pair that is not skipped leaves its un-whitened residual in kernel order, the block's phi last.
template <int NP, bool ANG>
__device__ __forceinline__ bool gs_pose_term(const GsW& W, unsigned amask, const double* h, const double (&x)[NP + 4], double bound, double& l,
                                             double* rout = nullptr) {
  constexpr int NR = NP + 3;
  double r[NR];
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    double d = x[k] - h[k];
    if (ANG && ((amask >> k) & 1u)) d = fma(-kGsTwoPi, rint(d / kGsTwoPi), d);
    r[k] = d;
  }
  double q = 0.0;
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    double z = W.w[k * (k + 1) / 2] * r[0];
#pragma unroll
    for (int c = 1; c <= k; ++c) z = fma(W.w[k * (k + 1) / 2 + c], r[c], z);
    q = fma(z, z, q);
  }
  if (NP >= 1 && fma(-0.5, q, l) < bound) return false;
  const double a0 = h[NP], a1 = -h[NP + 1], a2 = -h[NP + 2], a3 = -h[NP + 3];
  const double x0 = x[NP], x1 = x[NP + 1], x2 = x[NP + 2], x3 = x[NP + 3];
  double e0 = fma(-a3, x3, fma(-a2, x2, fma(-a1, x1, a0 * x0)));
  double e1 = fma(a2, x3, fma(-a3, x2, fma(a0, x1, a1 * x0)));
  double e2 = fma(-a1, x3, fma(a0, x2, fma(a3, x1, a2 * x0)));
  double e3 = fma(a0, x3, fma(a1, x2, fma(-a2, x1, a3 * x0)));
  if (e0 < 0.0) { e0 = -e0; e1 = -e1; e2 = -e2; e3 = -e3; }                       // tools/logq.m:26-28
  const double nv = sqrt(fma(e3, e3, fma(e2, e2, e1 * e1)));
  const double f = (nv == 0.0) ? 1.0 : atan2(nv, e0) / nv;
  r[NP] = f * e1; r[NP + 1] = f * e2; r[NP + 2] = f * e3;
#pragma unroll
  for (int k = NP; k < NR; ++k) {
    double z = W.w[k * (k + 1) / 2] * r[0];
#pragma unroll
    for (int c = 1; c <= k; ++c) z = fma(W.w[k * (k + 1) / 2 + c], r[c], z);
    q = fma(z, z, q);
  }
  l = fma(-0.5, q, l);
  if (rout) {
#pragma unroll
    for (int k = 0; k < NR; ++k) rout[k] = r[k];
  }
  return true;
}

// QP < 0: NR selected rows and gs_term; QP = NP >= 0: a quaternion block behind NP plain rows (NR = NP + 3, NR + 1 selected rows)
// kLocateBound: the locate kernel is launched with 64 threads; stating that for the block's instantiations lifts the 128-VGPR cap
// of the default bound (1024), under which NP = 4 spilled 12 bytes; without a block the default stays.
template <int NRES, bool ANG, int QP = -1>
struct GsTerm : GsData {
  static constexpr int NR = NRES;             // residuals
  static constexpr int NS = QP < 0 ? NR : NR + 1;
  static constexpr int kLocateBound = QP < 0 ? 1024 : 64;
  __device__ __forceinline__ double load_x(const GsHead& y, const double* xs_next, int j, int k) const { return xs_next[(size_t)j * y.nN + y.rows[k]]; }
  __device__ __forceinline__ double load_next(const GsHead& y, const double* xn, int ld, int j, int k) const { return xn[(size_t)y.rows[k] * ld + j]; }   // particles [nN][ld]
  static constexpr bool kSplit = false;       // gs_term and gs_pose_term hold their own test
  __device__ __forceinline__ bool pair(const GsHead& y, const double* h, const double (&x)[NS], double bound, double& l) const {
    if constexpr (QP < 0) return gs_term<NR, ANG>(W, y.angle_mask, h, x, bound, l);
    else return gs_pose_term<QP, ANG>(W, y.angle_mask, h, x, bound, l);
  }
  // pair, and the un-whitened residual in kernel order (rbpf_loc_pairstats.hpp)
  __device__ __forceinline__ bool pair_res(const GsHead& y, const double* h, const double (&x)[NS], double bound, double& l, double (&r)[NR]) const {
    if constexpr (QP < 0) return gs_term<NR, ANG>(W, y.angle_mask, h, x, bound, l, r);
    else return gs_pose_term<QP, ANG>(W, y.angle_mask, h, x, bound, l, r);
  }
  __device__ __forceinline__ void gather(const GsHead& y, const double* X, int N, int idx, double* xs, int j) const {
    for (int r = 0; r < y.nN; ++r) xs[(size_t)j * y.nN + r] = X[(size_t)r * N + idx];
  }
};

typedef BackwardArgs<GsData> GsArgs;

// ---- host side -----------------------------------------------------------------------------------------------------------
// The term type of a layout is chosen at run time: gs_pick calls f(GsTag<GsTerm<NR, ANG, QP>>()) for it, f a generic lambda
// that builds the kernel arguments with that term and launches.
template <class T>
struct GsTag { typedef T Term; };

template <int NR, class F>
static hipError_t gs_pick_ang(unsigned angle_mask, F&& f) {
  return angle_mask ? f(GsTag<GsTerm<NR, true>>()) : f(GsTag<GsTerm<NR, false>>());
}

// a quaternion block behind NP plain rows; an angle row is one of those
template <int NP, class F>
static hipError_t gs_pick_pose(unsigned angle_mask, F&& f) {
  if constexpr (NP > 0) {
    if (angle_mask) return f(GsTag<GsTerm<NP + 3, true, NP>>());
  }
  return f(GsTag<GsTerm<NP + 3, false, NP>>());
}

template <class F>
static hipError_t gs_pick(const LocGenLayout& y, unsigned angle_mask, F&& f) {
  if (y.n_plain >= 0) {
    switch (y.n_plain) {
      case 0: return gs_pick_pose<0>(angle_mask, f);
      case 1: return gs_pick_pose<1>(angle_mask, f);
      case 2: return gs_pick_pose<2>(angle_mask, f);
      case 3: return gs_pick_pose<3>(angle_mask, f);
      case 4: return gs_pick_pose<4>(angle_mask, f);
      default: return hipErrorInvalidValue;
    }
  }
  switch (y.n_res) {
    case 1: return gs_pick_ang<1>(angle_mask, f);
    case 2: return gs_pick_ang<2>(angle_mask, f);
    case 3: return gs_pick_ang<3>(angle_mask, f);
    case 4: return gs_pick_ang<4>(angle_mask, f);
    case 5: return gs_pick_ang<5>(angle_mask, f);
    case 6: return gs_pick_ang<6>(angle_mask, f);
    case 7: return gs_pick_ang<7>(angle_mask, f);
    case 8: return gs_pick_ang<8>(angle_mask, f);
    default: return hipErrorInvalidValue;
  }
}

// all-pairs pass + locate of one step (logp == null), or the logp kernel, in stream order
static hipError_t gs_launch(const LocGenLayout& y, const GsArgs& a, double* logp, hipStream_t s) {
  return gs_pick(y, a.head.angle_mask, [&](auto tag) {
    const auto b = a.with(typename decltype(tag)::Term{a.term});
    return logp ? backward_launch_logp(b, logp, s) : backward_launch_step(b, s);
  });
}

static void gs_launch_prologue(const LocGenLayout& y, int N, const double* mu, const double* w, double* Xhat, hipStream_t s) {
  if (y.n_plain >= 0) {
    GsSrc src;
    for (int k = 0; k < kGsMaxRes; ++k) src.s[k] = y.src[k];
    hipLaunchKernelGGL(gs_prologue_pose_kernel, dim3((N + 255) / 256), dim3(256), 0, s, N, y.n_sel, src, mu, w, Xhat);
  } else {
    hipLaunchKernelGGL(gs_prologue_kernel, dim3((N + 255) / 256), dim3(256), 0, s, N, y.n_res, mu, w, Xhat);
  }
}

// prologue + pass + locate of one step
static hipError_t gs_launch_step(const LocGenLayout& y, const GsArgs& a, const double* mu, const double* w, double* Xhat, hipStream_t s) {
  gs_launch_prologue(y, a.N, mu, w, Xhat, s);
  return gs_launch(y, a, nullptr, s);
}

typedef ViterbiArgs<GsData> GvArgs;

// prologue + delta over its log w + max-plus pass + merge of one MAP step (rbpf_loc_viterbi.hpp)
static hipError_t gs_launch_map_step(const LocGenLayout& y, const GvArgs& a, const double* mu, const double* w, const double* delta, double* Xhat,
                                     const double* w_next, double* delta_next, int* psi_next, hipStream_t s) {
  gs_launch_prologue(y, a.N, mu, w, Xhat, s);
  const hipError_t e = gs_pick(y, a.head.angle_mask, [&](auto tag) {
    return viterbi_launch_pass(a.with(typename decltype(tag)::Term{a.term}), delta, Xhat, s);
  });
  if (e != hipSuccess) return e;
  return viterbi_launch_merge(a.M, a.nchunks, a.part_best, a.part_arg, w_next, delta_next, psi_next, s);
}

typedef MarginalArgs<GsData> GmArgs;

// prologue (logw: the caller's log w over its last row, the probes) + the two all-pairs passes and their merges of one
// marginal-smoothing step (rbpf_loc_marginal.hpp)
static hipError_t gs_launch_marginal_step(const LocGenLayout& y, const GmArgs& a, const double* mu, const double* w, const double* logw, double* Xhat,
                                          const double* logws_next, double* D, double* cj, double* lws, hipStream_t s) {
  gs_launch_prologue(y, a.N, mu, w, Xhat, s);
  if (logw) {
    const hipError_t e = hipMemcpyAsync(Xhat + (size_t)y.n_sel * a.N, logw, (size_t)a.N * sizeof(double), hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return e;
  }
  return gs_pick(y, a.head.angle_mask, [&](auto tag) {
    return marginal_launch_step(a.with(typename decltype(tag)::Term{a.term}), logws_next, D, cj, lws, s);
  });
}

typedef PairStatsArgs<GsData> GpArgs;

// the statistics pass's arguments on what a marginal step's hold (rbpf_loc_pairstats.hpp)
static GpArgs gs_pair_stats_args(const GmArgs& a, const double* mass, double* part) {
  GpArgs b;
  std::memset(&b, 0, sizeof(b));
  pair_stats_set_sizes(b, a.N, a.M);
  b.head = a.head; b.Xhat = a.Xhat; b.xn_next = a.xn_next; b.cj = a.cj; b.mass = mass; b.part = part; b.term = a.term;
  return b;
}

// statistics pass + reduce of one step, after the marginal step's normalisation
static hipError_t gs_launch_pair_stats(const LocGenLayout& y, const GpArgs& a, double* page, hipStream_t s) {
  return gs_pick(y, a.head.angle_mask, [&](auto tag) {
    return pair_stats_launch_step(a.with(typename decltype(tag)::Term{a.term}), page, s);
  });
}

static int gs_validate_rows(int n_nonlin, int n_res, const int32_t* rows, uint32_t angle_mask) {
  if (n_nonlin < 1 || n_nonlin > kGsMaxNonlin) { set_error("n_nonlin must be in 1 .. 8"); return RBPF_ERR_INVALID_ARG; }
  if (n_res < 1 || n_res > kGsMaxRes) { set_error("n_res (the rows that carry noise) must be in 1 .. 8"); return RBPF_ERR_INVALID_ARG; }
  if (!rows) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  unsigned seen = 0;
  for (int k = 0; k < n_res; ++k) {
    if (rows[k] < 0 || rows[k] >= n_nonlin) { set_error("rows[" + std::to_string(k) + "] = " + std::to_string(rows[k]) + " is no row of the n_nonlin = " + std::to_string(n_nonlin) + " state"); return RBPF_ERR_INVALID_ARG; }
    if (seen & (1u << rows[k])) { set_error("rows names row " + std::to_string(rows[k]) + " twice"); return RBPF_ERR_INVALID_ARG; }
    seen |= 1u << rows[k];
  }
  if (angle_mask >> n_res) { set_error("angle_mask has a bit at or above n_res: an angle row must be one of rows"); return RBPF_ERR_INVALID_ARG; }
  return RBPF_OK;
}

// validates (rows [n_sel], angle_mask over the positions in rows, quat_pos = the position of q0 in rows or -1) and lays them out
// for the kernels
static int gs_layout(int n_nonlin, int n_sel, const int32_t* rows, uint32_t angle_mask, int quat_pos, LocGenLayout& y) {
  y = LocGenLayout();
  if (quat_pos == -1) {
    RB_TRY(gs_validate_rows(n_nonlin, n_sel, rows, angle_mask));
    y.n_sel = y.n_res = n_sel; y.angle_mask = angle_mask;
    for (int k = 0; k < n_sel; ++k) y.rows[k] = rows[k];
    return RBPF_OK;
  }
  if (n_sel - 1 > kGsMaxRes) { set_error("n_res = n_sel - 1 = " + std::to_string(n_sel - 1) + " residuals: n_res must be in 1 .. 8"); return RBPF_ERR_INVALID_ARG; }
  if (quat_pos < -1 || quat_pos >= n_sel) { set_error("quat_pos = " + std::to_string(quat_pos) + ": the quaternion block is not inside rows (positions 0 .. n_sel-1, or -1 for none)"); return RBPF_ERR_INVALID_ARG; }
  if (quat_pos + 4 > n_sel) { set_error("the quaternion block (positions " + std::to_string(quat_pos) + " .. " + std::to_string(quat_pos + 3) + " of rows) runs past n_sel = " + std::to_string(n_sel)); return RBPF_ERR_INVALID_ARG; }
  RB_TRY(gs_validate_rows(n_nonlin, n_sel, rows, angle_mask));        // (n_sel <= 8 from here on: the rows are distinct)
  if (angle_mask & (0xFu << quat_pos)) { set_error("angle_mask marks a row of the quaternion block: its residual is logq, not a wrapped difference"); return RBPF_ERR_INVALID_ARG; }
  y.n_sel = n_sel; y.n_res = n_sel - 1; y.n_plain = n_sel - 4;
  int k = 0;
  for (int p = 0; p < n_sel; ++p) {
    if (p >= quat_pos && p < quat_pos + 4) continue;
    y.rows[k] = rows[p]; y.src[k] = p; y.perm[k] = p < quat_pos ? p : p - 1;
    if ((angle_mask >> p) & 1u) y.angle_mask |= 1u << k;
    ++k;
  }
  for (int q = 0; q < 4; ++q) { y.rows[k + q] = rows[quat_pos + q]; y.src[k + q] = quat_pos + q; }
  for (int q = 0; q < 3; ++q) y.perm[k + q] = quat_pos + q;
  return RBPF_OK;
}

// cov [n x n] column-major (lower triangle read) -> W = inv(chol(cov, 'lower')), packed by rows
static int gs_factor(const double* cov, int n, GsW& W, const std::string& where) {
  double L[kGsMaxRes * kGsMaxRes];
  for (int q = 0; q < n * n; ++q)
    if (!std::isfinite(cov[q])) { set_error("cov" + where + " has a non-finite entry"); return RBPF_ERR_CHOL_FAILED; }
  if (!chol_lower_host(cov, n, n, L, n)) {
    set_error("cov" + where + " is not positive definite: the transition density does not exist");
    return RBPF_ERR_CHOL_FAILED;
  }
  std::memset(&W, 0, sizeof(W));
  for (int j = 0; j < n; ++j) {
    W.w[j * (j + 1) / 2 + j] = 1.0 / L[j + n * j];
    for (int i = j + 1; i < n; ++i) {
      double s = 0.0;
      for (int k = j; k < i; ++k) s += L[i + n * k] * W.w[k * (k + 1) / 2 + j];
      W.w[i * (i + 1) / 2 + j] = -s / L[i + n * i];
    }
  }
  return RBPF_OK;
}

// gs_factor of cov in kernel order: cov_k(a, b) = cov(perm[a], perm[b]), the symmetric permutation (z'z is the same quadratic form)
static int gs_factor_layout(const double* cov, const LocGenLayout& y, GsW& W, const std::string& where) {
  if (y.n_plain < 0) return gs_factor(cov, y.n_res, W, where);
  const int n = y.n_res;
  double P[kGsMaxRes * kGsMaxRes];
  for (int b = 0; b < n; ++b)
    for (int a = b; a < n; ++a) {                  // the caller's lower triangle is the one read
      const int i = std::max(y.perm[a], y.perm[b]), j = std::min(y.perm[a], y.perm[b]);
      P[a + n * b] = P[b + n * a] = cov[i + n * j];
    }
  return gs_factor(P, n, W, where);
}

// NR: the rows of mu (n_res, or n_sel with a quaternion block); Xhat has one more
static size_t gs_bytes(size_t nN, size_t NR, size_t N, size_t T, size_t M) {
  const size_t C = (size_t)backward_chunk_size((int)N, (int)M), nch = (N + C - 1) / C;
  return ((NR + 1) * N + 2 * nch * M + T * M + T * nN * M + nN * T) * sizeof(double) + T * M * sizeof(int);
}

static int gs_ctx_ok(const rbpf_ctx* c) {
  if (!c || !c->loc) { set_error("not a localisation context"); return RBPF_ERR_INVALID_ARG; }
  if (!c->loc->generic) { set_error("not a generic localisation context (rbpf_loc_generic_create): the dense-mag map has rbpf_loc_backward_simulate"); return RBPF_ERR_INVALID_ARG; }
  return RBPF_OK;
}

// prologue + the rejection step of rbpf_loc_reject.hpp (waits for the stream once)
static hipError_t gs_launch_reject_step(const LocGenLayout& y, const GsArgs& a, const RejectWorkspace& rw, const double* mu, const double* w,
                                        double* Xhat, int max_tries, const double* u_try, unsigned long long seed, int step, int* n_fb,
                                        long long* n_tries, hipStream_t s) {
  gs_launch_prologue(y, a.N, mu, w, Xhat, s);
  return gs_pick(y, a.head.angle_mask, [&](auto tag) {
    return reject_launch_step(a.with(typename decltype(tag)::Term{a.term}), rw, w, a.head.nN, max_tries, u_try, seed, step, n_fb, n_tries, s);
  });
}

static const char* const kFlOpen = "a fixed-lag stepping is open on this context (rbpf_loc_generic_fixed_lag_finish first)";
static const char* const kFsOpen = "a running-statistics stepping is open on this context (rbpf_loc_generic_forward_stats_finish first)";

static void gs_release(rbpf_ctx* c) {
  c->loc->gb.rw.release();
  c->loc->gb.ws.release();
  c->loc->gb = LocGenBackward();
}

}  // namespace rbpf

using namespace rbpf;

extern "C" {

int rbpf_loc_generic_backward_workspace_bytes(int32_t n_nonlin, int32_t n_res, int32_t N_P, int32_t N_T, int32_t n_traj, size_t* bytes) {
  if (!bytes) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  if (n_nonlin < 1 || n_nonlin > kGsMaxNonlin || n_res < 1 || n_res > kGsMaxRes || n_res > n_nonlin) {
    set_error("n_nonlin must be in 1 .. 8 and n_res in 1 .. n_nonlin");
    return RBPF_ERR_INVALID_ARG;
  }
  if (N_P < 1 || N_T < 1 || n_traj < 1) { set_error("N_P, N_T and n_traj must be >= 1"); return RBPF_ERR_INVALID_ARG; }
  if (N_P > kMaxParticles) { set_error("N_P above 1048576 is not supported"); return RBPF_ERR_UNSUPPORTED; }
  *bytes = gs_bytes((size_t)n_nonlin, (size_t)n_res, (size_t)N_P, (size_t)N_T, (size_t)n_traj);
  return RBPF_OK;
}

int rbpf_loc_generic_backward_pose_workspace_bytes(int32_t n_nonlin, int32_t n_sel, int32_t quat_pos, int32_t N_P, int32_t N_T,
                                                   int32_t n_traj, size_t* bytes) {
  if (quat_pos == -1) return rbpf_loc_generic_backward_workspace_bytes(n_nonlin, n_sel, N_P, N_T, n_traj, bytes);
  if (!bytes) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  if (n_nonlin < 4 || n_nonlin > kGsMaxNonlin || n_sel < 4 || n_sel > n_nonlin || quat_pos < 0 || quat_pos + 4 > n_sel) {
    set_error("with a quaternion block n_nonlin must be in 4 .. 8, n_sel in 4 .. n_nonlin and the block inside the n_sel rows");
    return RBPF_ERR_INVALID_ARG;
  }
  if (N_P < 1 || N_T < 1 || n_traj < 1) { set_error("N_P, N_T and n_traj must be >= 1"); return RBPF_ERR_INVALID_ARG; }
  if (N_P > kMaxParticles) { set_error("N_P above 1048576 is not supported"); return RBPF_ERR_UNSUPPORTED; }
  *bytes = gs_bytes((size_t)n_nonlin, (size_t)n_sel, (size_t)N_P, (size_t)N_T, (size_t)n_traj);
  return RBPF_OK;
}

int rbpf_loc_generic_backward_begin(rbpf_ctx* c, int32_t n_traj, const double* u, uint64_t seed, int32_t n_res, const int32_t* rows,
                                    uint32_t angle_mask) {
  return rbpf_loc_generic_backward_pose_begin(c, n_traj, u, seed, n_res, rows, angle_mask, -1);
}

// rbpf_loc_generic_backward_pose_begin (max_tries = -1) and rbpf_loc_generic_backward_reject_begin (max_tries >= 0)
static int gs_begin(rbpf_ctx* c, int32_t n_traj, const double* u, uint64_t seed, int max_tries, int32_t n_sel, const int32_t* rows,
                    uint32_t angle_mask, int32_t quat_pos, const char* who) {
  RB_TRY(gs_ctx_ok(c));
  LocState* L = c->loc;
  if (n_traj < 1) { set_error("n_traj must be >= 1"); return RBPF_ERR_INVALID_ARG; }
  LocGenLayout lay;
  RB_TRY(gs_layout(L->nN, n_sel, rows, angle_mask, quat_pos, lay));
  if (L->gb.open) { set_error("a backward pass is open on this context (rbpf_loc_generic_backward_finish first)"); return RBPF_ERR_STATE; }
  if (L->gv.open) { set_error("a MAP pass is open on this context (rbpf_loc_generic_map_finish first)"); return RBPF_ERR_STATE; }
  if (L->gm.open) { set_error("a marginal pass is open on this context (rbpf_loc_generic_marginal_finish first)"); return RBPF_ERR_STATE; }
  if (L->gp.open) { set_error("a statistics pass is open on this context (rbpf_loc_generic_pair_stats_finish first)"); return RBPF_ERR_STATE; }
  if (L->fs.open) { set_error(kFsOpen); return RBPF_ERR_STATE; }
  if (L->fl.open) { set_error(kFlOpen); return RBPF_ERR_STATE; }
  RB_TRY(backward_check_forward(c, "backward simulation", who));
  const int N = c->N, T = c->T, M = n_traj, nN = L->nN;
  LocGenBackward& g = L->gb;
  g.M = M; g.lay = lay;
  g.C = backward_chunk_size(N, M); g.nch = (N + g.C - 1) / g.C;
  g.reject = max_tries >= 0; g.max_tries = std::max(max_tries, 0); g.seed = seed;
  int s = g.ws.take(c->pool, (size_t)(lay.n_sel + 1) * N, g.reject ? reject_part_count(N, M) : (size_t)g.nch * M, (size_t)T * M, (size_t)T * nN * M,
                    (size_t)nN * T);
  if (s == RBPF_OK && g.reject) {
    L->reject_n_fb.clear();
    L->reject_n_tries.clear();
    s = g.rw.take(c->pool, (size_t)N, reject_cdf_blocks(N), (size_t)M, (size_t)nN, (size_t)T);
    if (s == RBPF_OK) {
      hipError_t e = hipMemsetAsync(g.rw.n_fb, 0, (size_t)T * sizeof(int), c->stream);
      if (e == hipSuccess) e = hipMemsetAsync(g.rw.n_tries, 0, (size_t)T * sizeof(long long), c->stream);
      if (e != hipSuccess) s = hip_fail(e, "counters of the rejection pass", __FILE__, __LINE__);
    }
  }
  if (s == RBPF_OK) s = backward_uniforms(u, seed, T, M, g.ws.u, c->stream);
  if (s != RBPF_OK) { gs_release(c); return s; }
  g.t = T - 1;
  g.open = true;
  return RBPF_OK;
}

int rbpf_loc_generic_backward_pose_begin(rbpf_ctx* c, int32_t n_traj, const double* u, uint64_t seed, int32_t n_sel, const int32_t* rows,
                                         uint32_t angle_mask, int32_t quat_pos) {
  return gs_begin(c, n_traj, u, seed, -1, n_sel, rows, angle_mask, quat_pos, "rbpf_loc_generic_backward_begin");
}

int rbpf_loc_generic_backward_reject_begin(rbpf_ctx* c, int32_t n_traj, uint64_t seed, int32_t max_tries, int32_t n_sel, const int32_t* rows,
                                           uint32_t angle_mask, int32_t quat_pos) {
  if (max_tries < 0 || max_tries > kRejectMaxTries) { set_error("max_tries must be in 0 .. 4194304"); return RBPF_ERR_INVALID_ARG; }
  return gs_begin(c, n_traj, nullptr, seed, max_tries, n_sel, rows, angle_mask, quat_pos, "rbpf_loc_generic_backward_reject_begin");
}

int rbpf_loc_generic_backward_reject_stats(rbpf_ctx* c, int32_t* n_fallback, int64_t* n_tries) {
  RB_TRY(gs_ctx_ok(c));
  const LocState* L = c->loc;
  if (L->reject_n_fb.empty()) { set_error("no rejection pass has finished on this context (rbpf_loc_generic_backward_reject_begin .. _finish first)"); return RBPF_ERR_STATE; }
  for (size_t t = 0; t < L->reject_n_fb.size(); ++t) {
    if (n_fallback) n_fallback[t] = L->reject_n_fb[t];
    if (n_tries) n_tries[t] = L->reject_n_tries[t];
  }
  return RBPF_OK;
}

int rbpf_loc_generic_backward_reject_workspace_bytes(int32_t n_nonlin, int32_t n_sel, int32_t quat_pos, int32_t N_P, int32_t N_T, int32_t n_traj,
                                                     size_t* bytes) {
  RB_TRY(rbpf_loc_generic_backward_pose_workspace_bytes(n_nonlin, n_sel, quat_pos, N_P, N_T, n_traj, bytes));
  const size_t nch = ((size_t)N_P + backward_chunk_size(N_P, n_traj) - 1) / backward_chunk_size(N_P, n_traj);
  *bytes += 2 * (reject_part_count(N_P, n_traj) - nch * (size_t)n_traj) * sizeof(double) +
            reject_bytes((size_t)N_P, (size_t)n_traj, (size_t)n_nonlin, (size_t)N_T);
  return RBPF_OK;
}

int rbpf_loc_generic_backward_particles_device(rbpf_ctx* c, int32_t* t, const double** xn_dev) {
  RB_TRY(gs_ctx_ok(c));
  if (!t || !xn_dev) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  const LocGenBackward& g = c->loc->gb;
  if (!g.open) { set_error("no backward pass is open (rbpf_loc_generic_backward_begin first)"); return RBPF_ERR_STATE; }
  if (g.t < 0) { set_error("every step of the backward pass is done (rbpf_loc_generic_backward_finish)"); return RBPF_ERR_STATE; }
  *t = g.t;
  *xn_dev = c->X + (size_t)g.t * c->loc->nN * c->N;
  return RBPF_OK;
}

int rbpf_loc_generic_backward_step_device(rbpf_ctx* c, const double* mu_dev, const double* cov) {
  RB_TRY(gs_ctx_ok(c));
  LocState* L = c->loc;
  LocGenBackward& g = L->gb;
  if (!g.open) { set_error("no backward pass is open (rbpf_loc_generic_backward_begin first)"); return RBPF_ERR_STATE; }
  if (g.t < 0) { set_error("every step of the backward pass is done (rbpf_loc_generic_backward_finish)"); return RBPF_ERR_STATE; }
  const int N = c->N, T = c->T, M = g.M, nN = L->nN, t = g.t;
  GsArgs a;
  std::memset(&a, 0, sizeof(a));
  a.head.first = (t == T - 1);
  if (!a.head.first) {
    if (!mu_dev || !cov) { set_error("NULL argument (mu_dev and cov may be NULL at step N_T-1 only)"); return RBPF_ERR_INVALID_ARG; }
    RB_TRY(gs_factor_layout(cov, g.lay, a.term.W, " of step " + std::to_string(t)));
  }
  HIPCHK(hipSetDevice(c->device));
  a.N = N; a.M = M; a.C = g.C; a.nchunks = g.nch; a.head.nN = nN; a.head.angle_mask = g.lay.angle_mask;
  for (int k = 0; k < g.lay.n_sel; ++k) a.head.rows[k] = g.lay.rows[k];
  a.Xhat = g.ws.Xhat; a.X = c->X + (size_t)t * nN * N;
  a.xs_next = a.head.first ? nullptr : g.ws.xs + (size_t)(t + 1) * nN * M;
  a.u = g.ws.u + (size_t)t * M; a.part_m = g.ws.pm; a.part_s = g.ws.ps;
  a.index = g.ws.idx + (size_t)t * M; a.xs = g.ws.xs + (size_t)t * nN * M; a.clamped = c->d_flags + 1;
  if (g.reject && !a.head.first)
    HIPCHK(gs_launch_reject_step(g.lay, a, g.rw, mu_dev, c->w + (size_t)t * N, g.ws.Xhat, g.max_tries, nullptr, g.seed, t, g.rw.n_fb + t,
                                 g.rw.n_tries + t, c->stream));
  else
    HIPCHK(gs_launch_step(g.lay, a, a.head.first ? nullptr : mu_dev, c->w + (size_t)t * N, g.ws.Xhat, c->stream));
  HIPCHK(backward_launch_mean(M, nN, a.xs, g.ws.mean + (size_t)t * nN, c->stream));
  g.t = t - 1;
  return RBPF_OK;
}

int rbpf_loc_generic_backward_finish(rbpf_ctx* c, double* xs_traj, int32_t* index, double* traj_smooth_mean) {
  RB_TRY(gs_ctx_ok(c));
  LocState* L = c->loc;
  LocGenBackward& g = L->gb;
  if (!g.open) { set_error("no backward pass is open (rbpf_loc_generic_backward_begin first)"); return RBPF_ERR_STATE; }
  const int T = c->T, M = g.M, nN = L->nN, t_next = g.t;
  const bool reject = g.reject;
  BackwardWorkspace ws = g.ws;
  RejectWorkspace rw = g.rw;
  g = LocGenBackward();                                                  // the pass is closed whichever way this returns,
  BackwardWorkspaceGuard lease(ws);                                      // and its workspace goes back
  RejectWorkspaceGuard reject_lease(rw);
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (t_next >= 0) {
    if (!xs_traj && !index && !traj_smooth_mean) return RBPF_OK;         // the way out of a pass that was given up
    set_error("rbpf_loc_generic_backward_finish: steps " + std::to_string(t_next) + " .. 0 of the backward pass were not run");
    return RBPF_ERR_STATE;
  }
  RB_TRY(ctx_check_flags(c));
  if (reject) {
    std::vector<int> nf((size_t)T);
    std::vector<long long> nt((size_t)T);
    HIPCHK(hipMemcpy(nf.data(), rw.n_fb, (size_t)T * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(nt.data(), rw.n_tries, (size_t)T * sizeof(long long), hipMemcpyDeviceToHost));
    L->reject_n_fb.swap(nf);
    L->reject_n_tries.swap(nt);
  }
  if (xs_traj) HIPCHK(hipMemcpy(xs_traj, ws.xs, (size_t)nN * M * T * sizeof(double), hipMemcpyDeviceToHost));
  if (index) HIPCHK(hipMemcpy(index, ws.idx, (size_t)M * T * sizeof(int), hipMemcpyDeviceToHost));
  if (traj_smooth_mean) HIPCHK(hipMemcpy(traj_smooth_mean, ws.mean, (size_t)nN * T * sizeof(double), hipMemcpyDeviceToHost));
  return RBPF_OK;
}

int rbpf_loc_generic_backward_step(int32_t N, int32_t M, int32_t n_nonlin, int32_t n_res, const int32_t* rows, uint32_t angle_mask,
                                   const double* mu, const double* w, const double* xs_next, const double* cov, const double* u,
                                   int32_t* index, double* logp, int32_t reps, double* ms) {
  return rbpf_loc_generic_backward_pose_step(N, M, n_nonlin, n_res, rows, angle_mask, -1, mu, w, xs_next, cov, u, index, logp, reps, ms);
}

int rbpf_loc_generic_backward_pose_step(int32_t N, int32_t M, int32_t n_nonlin, int32_t n_sel, const int32_t* rows, uint32_t angle_mask,
                                        int32_t quat_pos, const double* mu, const double* w, const double* xs_next, const double* cov,
                                        const double* u, int32_t* index, double* logp, int32_t reps, double* ms) {
  if (!mu || !w || !xs_next || !cov || !u || !index || !rows) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  if (N < 1 || M < 1) { set_error("N and M must be >= 1"); return RBPF_ERR_INVALID_ARG; }
  if (N > kMaxParticles) { set_error("N above 1048576 is not supported"); return RBPF_ERR_UNSUPPORTED; }
  LocGenLayout lay;
  RB_TRY(gs_layout(n_nonlin, n_sel, rows, angle_mask, quat_pos, lay));
  GsArgs a;
  std::memset(&a, 0, sizeof(a));
  RB_TRY(gs_factor_layout(cov, lay, a.term.W, ""));
  if (!have_device()) { set_error("no HIP device: the backward pass has no CPU fallback"); return RBPF_ERR_NO_DEVICE; }
  const int C = backward_chunk_size(N, M), nch = (N + C - 1) / C;
  DevicePool tmp;
  double *d_mu = nullptr, *d_w = nullptr, *d_xs = nullptr, *d_u = nullptr, *d_Xhat = nullptr, *d_pm = nullptr, *d_ps = nullptr, *d_lp = nullptr;
  int *d_idx = nullptr, *d_clamped = nullptr;
  RB_TRY(tmp.upload(&d_mu, mu, (size_t)lay.n_sel * N));
  RB_TRY(tmp.upload(&d_w, w, (size_t)N));
  RB_TRY(tmp.upload(&d_xs, xs_next, (size_t)n_nonlin * M));
  RB_TRY(tmp.upload(&d_u, u, (size_t)M));
  RB_TRY(tmp.alloc(&d_Xhat, (size_t)(lay.n_sel + 1) * N));
  RB_TRY(tmp.alloc(&d_pm, (size_t)nch * M));
  RB_TRY(tmp.alloc(&d_ps, (size_t)nch * M));
  RB_TRY(tmp.alloc(&d_idx, (size_t)M));
  RB_TRY(tmp.alloc(&d_clamped, (size_t)1));
  HIPCHK(hipMemset(d_clamped, 0, sizeof(int)));
  if (logp) RB_TRY(tmp.alloc(&d_lp, (size_t)N * M));
  a.N = N; a.M = M; a.C = C; a.nchunks = nch; a.head.nN = n_nonlin; a.head.first = 0; a.head.angle_mask = lay.angle_mask;
  for (int k = 0; k < lay.n_sel; ++k) a.head.rows[k] = lay.rows[k];
  a.Xhat = d_Xhat; a.X = nullptr; a.xs_next = d_xs; a.u = d_u; a.part_m = d_pm; a.part_s = d_ps; a.index = d_idx; a.xs = nullptr;
  a.clamped = d_clamped;
  RB_TRY(timed_reps(reps, 0, [&] { return gs_launch_step(lay, a, d_mu, d_w, d_Xhat, 0); }, ms));
  if (logp) HIPCHK(gs_launch(lay, a, d_lp, 0));
  HIPCHK(hipMemcpy(index, d_idx, (size_t)M * sizeof(int), hipMemcpyDeviceToHost));
  if (logp) HIPCHK(hipMemcpy(logp, d_lp, (size_t)N * M * sizeof(double), hipMemcpyDeviceToHost));
  return RBPF_OK;
}

int rbpf_loc_generic_backward_reject_step(int32_t N, int32_t M, int32_t n_nonlin, int32_t n_sel, const int32_t* rows, uint32_t angle_mask,
                                          int32_t quat_pos, const double* mu, const double* w, const double* xs_next, const double* cov,
                                          const double* u_try, const double* u, int32_t R, int32_t* index, int32_t* accepted_at, int32_t reps,
                                          double* ms) {
  if (!mu || !w || !xs_next || !cov || !u || !index || !rows) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  if (N < 1 || M < 1) { set_error("N and M must be >= 1"); return RBPF_ERR_INVALID_ARG; }
  if (R < 0 || R > kRejectMaxTries) { set_error("max_tries must be in 0 .. 4194304"); return RBPF_ERR_INVALID_ARG; }
  if (N > kMaxParticles) { set_error("N above 1048576 is not supported"); return RBPF_ERR_UNSUPPORTED; }
  LocGenLayout lay;
  RB_TRY(gs_layout(n_nonlin, n_sel, rows, angle_mask, quat_pos, lay));
  GsArgs a;
  std::memset(&a, 0, sizeof(a));
  RB_TRY(gs_factor_layout(cov, lay, a.term.W, ""));
  if (!have_device()) { set_error("no HIP device: the backward pass has no CPU fallback"); return RBPF_ERR_NO_DEVICE; }
  DevicePool tmp;
  RejectWorkspace rw;
  RejectWorkspaceGuard lease(rw);
  double *d_mu = nullptr, *d_w = nullptr, *d_xs = nullptr, *d_u = nullptr, *d_ut = nullptr, *d_Xhat = nullptr, *d_pm = nullptr, *d_ps = nullptr;
  int *d_idx = nullptr, *d_clamped = nullptr;
  const size_t np = reject_part_count(N, M);
  RB_TRY(tmp.upload(&d_mu, mu, (size_t)lay.n_sel * N));
  RB_TRY(tmp.upload(&d_w, w, (size_t)N));
  RB_TRY(tmp.upload(&d_xs, xs_next, (size_t)n_nonlin * M));
  RB_TRY(tmp.upload(&d_u, u, (size_t)M));
  if (R > 0 && u_try) RB_TRY(tmp.upload(&d_ut, u_try, (size_t)2 * M * R));   // (null: the device generator, seed 0, step 0)
  RB_TRY(tmp.alloc(&d_Xhat, (size_t)(lay.n_sel + 1) * N));
  RB_TRY(tmp.alloc(&d_pm, np));
  RB_TRY(tmp.alloc(&d_ps, np));
  RB_TRY(tmp.alloc(&d_idx, (size_t)M));
  RB_TRY(tmp.alloc(&d_clamped, (size_t)1));
  RB_TRY(rw.take(tmp, (size_t)N, reject_cdf_blocks(N), (size_t)M, (size_t)n_nonlin, 1));
  HIPCHK(hipMemset(d_clamped, 0, sizeof(int)));
  a.N = N; a.M = M; a.C = backward_chunk_size(N, M); a.nchunks = (N + a.C - 1) / a.C;
  a.head.nN = n_nonlin; a.head.first = 0; a.head.angle_mask = lay.angle_mask;
  for (int k = 0; k < lay.n_sel; ++k) a.head.rows[k] = lay.rows[k];
  a.Xhat = d_Xhat; a.X = nullptr; a.xs_next = d_xs; a.u = d_u; a.part_m = d_pm; a.part_s = d_ps; a.index = d_idx; a.xs = nullptr;
  a.clamped = d_clamped;
  RB_TRY(timed_reps(reps, 0, [&] { return gs_launch_reject_step(lay, a, rw, d_mu, d_w, d_Xhat, R, d_ut, 0ull, 0, rw.n_fb, rw.n_tries, 0); }, ms));
  HIPCHK(hipMemcpy(index, d_idx, (size_t)M * sizeof(int), hipMemcpyDeviceToHost));
  if (accepted_at) {
    std::vector<int> acc((size_t)M), tr((size_t)M);
    HIPCHK(hipMemcpy(acc.data(), rw.acc, (size_t)M * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(tr.data(), rw.tries, (size_t)M * sizeof(int), hipMemcpyDeviceToHost));
    for (int j = 0; j < M; ++j) accepted_at[j] = acc[j] >= 0 ? tr[j] - 1 : -1;
  }
  return RBPF_OK;
}

// ---- the MAP trajectory ---------------------------------------------------------------------------------------------------
int rbpf_loc_generic_map_workspace_bytes(int32_t n_nonlin, int32_t n_sel, int32_t quat_pos, int32_t N_P, int32_t N_T, size_t* bytes) {
  if (!bytes) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  if (quat_pos == -1) {
    if (n_nonlin < 1 || n_nonlin > kGsMaxNonlin || n_sel < 1 || n_sel > kGsMaxRes || n_sel > n_nonlin) {
      set_error("n_nonlin must be in 1 .. 8 and n_res in 1 .. n_nonlin");
      return RBPF_ERR_INVALID_ARG;
    }
  } else if (n_nonlin < 4 || n_nonlin > kGsMaxNonlin || n_sel < 4 || n_sel > n_nonlin || quat_pos < 0 || quat_pos + 4 > n_sel) {
    set_error("with a quaternion block n_nonlin must be in 4 .. 8, n_sel in 4 .. n_nonlin and the block inside the n_sel rows");
    return RBPF_ERR_INVALID_ARG;
  }
  if (N_P < 1 || N_T < 1) { set_error("N_P and N_T must be >= 1"); return RBPF_ERR_INVALID_ARG; }
  if (N_P > kMaxParticles) { set_error("N_P above 1048576 is not supported"); return RBPF_ERR_UNSUPPORTED; }
  *bytes = viterbi_bytes((size_t)n_nonlin, (size_t)n_sel, (size_t)N_P, (size_t)N_T);
  return RBPF_OK;
}

int rbpf_loc_generic_map_begin(rbpf_ctx* c, int32_t n_sel, const int32_t* rows, uint32_t angle_mask, int32_t quat_pos) {
  RB_TRY(gs_ctx_ok(c));
  LocState* L = c->loc;
  LocGenLayout lay;
  RB_TRY(gs_layout(L->nN, n_sel, rows, angle_mask, quat_pos, lay));
  if (L->gv.open) { set_error("a MAP pass is open on this context (rbpf_loc_generic_map_finish first)"); return RBPF_ERR_STATE; }
  if (L->gb.open) { set_error("a backward pass is open on this context (rbpf_loc_generic_backward_finish first)"); return RBPF_ERR_STATE; }
  if (L->gm.open) { set_error("a marginal pass is open on this context (rbpf_loc_generic_marginal_finish first)"); return RBPF_ERR_STATE; }
  if (L->gp.open) { set_error("a statistics pass is open on this context (rbpf_loc_generic_pair_stats_finish first)"); return RBPF_ERR_STATE; }
  if (L->fs.open) { set_error(kFsOpen); return RBPF_ERR_STATE; }
  if (L->fl.open) { set_error(kFlOpen); return RBPF_ERR_STATE; }
  RB_TRY(backward_check_forward(c, "the MAP trajectory", "rbpf_loc_generic_map_begin"));
  const int N = c->N, T = c->T;
  LocGenBackward& g = L->gv;
  g.M = N; g.lay = lay;
  g.C = backward_chunk_size(N, N); g.nch = (N + g.C - 1) / g.C;
  int s = viterbi_take(g.ws, c->pool, L->nN, lay.n_sel, N, T);
  if (s == RBPF_OK) {
    const hipError_t e = viterbi_launch_init(N, c->w, g.ws.u, c->stream);
    if (e != hipSuccess) s = hip_fail(e, "delta of step 0", __FILE__, __LINE__);
  }
  if (s != RBPF_OK) { g.ws.release(); g = LocGenBackward(); return s; }
  g.t = 0;
  g.open = true;
  return RBPF_OK;
}

int rbpf_loc_generic_map_particles_device(rbpf_ctx* c, int32_t* t, const double** xn_dev) {
  RB_TRY(gs_ctx_ok(c));
  if (!t || !xn_dev) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  const LocGenBackward& g = c->loc->gv;
  if (!g.open) { set_error("no MAP pass is open (rbpf_loc_generic_map_begin first)"); return RBPF_ERR_STATE; }
  if (g.t + 1 >= c->T) { set_error("every step of the MAP pass is done (rbpf_loc_generic_map_finish)"); return RBPF_ERR_STATE; }
  *t = g.t;
  *xn_dev = c->X + (size_t)g.t * c->loc->nN * c->N;
  return RBPF_OK;
}

int rbpf_loc_generic_map_step_device(rbpf_ctx* c, const double* mu_dev, const double* cov) {
  RB_TRY(gs_ctx_ok(c));
  LocState* L = c->loc;
  LocGenBackward& g = L->gv;
  if (!g.open) { set_error("no MAP pass is open (rbpf_loc_generic_map_begin first)"); return RBPF_ERR_STATE; }
  if (g.t + 1 >= c->T) { set_error("every step of the MAP pass is done (rbpf_loc_generic_map_finish)"); return RBPF_ERR_STATE; }
  if (!mu_dev || !cov) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  const int N = c->N, nN = L->nN, t = g.t;
  GvArgs a;
  std::memset(&a, 0, sizeof(a));
  RB_TRY(gs_factor_layout(cov, g.lay, a.term.W, " of step " + std::to_string(t)));
  HIPCHK(hipSetDevice(c->device));
  a.N = N; a.M = N; a.C = g.C; a.nchunks = g.nch; a.head.nN = nN; a.head.angle_mask = g.lay.angle_mask;
  for (int k = 0; k < g.lay.n_sel; ++k) a.head.rows[k] = g.lay.rows[k];
  a.Xhat = g.ws.Xhat; a.xn_next = c->X + (size_t)(t + 1) * nN * N; a.part_best = g.ws.pm; a.part_arg = g.ws.arg;
  HIPCHK(gs_launch_map_step(g.lay, a, mu_dev, c->w + (size_t)t * N, g.ws.u + (size_t)(t & 1) * N, g.ws.Xhat, c->w + (size_t)(t + 1) * N,
                            g.ws.u + (size_t)((t + 1) & 1) * N, g.ws.idx + (size_t)(t + 1) * N, c->stream));
  g.t = t + 1;
  return RBPF_OK;
}

int rbpf_loc_generic_map_finish(rbpf_ctx* c, double* x_map, int32_t* index, double* score) {
  RB_TRY(gs_ctx_ok(c));
  LocState* L = c->loc;
  LocGenBackward& g = L->gv;
  if (!g.open) { set_error("no MAP pass is open (rbpf_loc_generic_map_begin first)"); return RBPF_ERR_STATE; }
  const int N = c->N, T = c->T, nN = L->nN, t_next = g.t;
  BackwardWorkspace ws = g.ws;
  g = LocGenBackward();                                                  // the pass is closed whichever way this returns,
  BackwardWorkspaceGuard lease(ws);                                      // and its workspace goes back
  HIPCHK(hipSetDevice(c->device));
  if (t_next + 1 < T) {
    HIPCHK(hipStreamSynchronize(c->stream));
    if (!x_map && !index && !score) return RBPF_OK;                      // the way out of a pass that was given up
    set_error("rbpf_loc_generic_map_finish: steps " + std::to_string(t_next) + " .. " + std::to_string(T - 2) + " of the MAP pass were not run");
    return RBPF_ERR_STATE;
  }
  const hipError_t e = viterbi_launch_backtrack(N, T, nN, c->X, ws.idx, ws.u + (size_t)((T - 1) & 1) * N, ws.mean, ws.idx + (size_t)T * N,
                                                ws.mean + (size_t)nN * T, c->stream);
  const hipError_t e2 = hipStreamSynchronize(c->stream);                 // (waited for whichever way this returns: the workspace goes back)
  HIPCHK(e);
  HIPCHK(e2);
  RB_TRY(ctx_check_flags(c));
  return viterbi_copy_out(ws, nN, N, T, x_map, index, score);
}

int rbpf_loc_generic_map_step(int32_t N, int32_t M, int32_t n_nonlin, int32_t n_sel, const int32_t* rows, uint32_t angle_mask, int32_t quat_pos,
                              const double* mu, const double* delta, const double* xs_next, const double* cov, double* best, int32_t* arg,
                              int32_t reps, double* ms) {
  if (!mu || !delta || !xs_next || !cov || !best || !arg || !rows) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  if (N < 1 || M < 1) { set_error("N and M must be >= 1"); return RBPF_ERR_INVALID_ARG; }
  if (N > kMaxParticles || M > kMaxParticles) { set_error("N or M above 1048576 is not supported"); return RBPF_ERR_UNSUPPORTED; }
  LocGenLayout lay;
  RB_TRY(gs_layout(n_nonlin, n_sel, rows, angle_mask, quat_pos, lay));
  GvArgs a;
  std::memset(&a, 0, sizeof(a));
  RB_TRY(gs_factor_layout(cov, lay, a.term.W, ""));
  if (!have_device()) { set_error("no HIP device: the MAP pass has no CPU fallback"); return RBPF_ERR_NO_DEVICE; }
  const int C = backward_chunk_size(N, M), nch = (N + C - 1) / C;
  std::vector<double> xt((size_t)n_nonlin * M);                           // the successors as the history holds them: [n_nonlin][M]
  for (int j = 0; j < M; ++j)
    for (int r = 0; r < n_nonlin; ++r) xt[(size_t)r * M + j] = xs_next[(size_t)j * n_nonlin + r];
  DevicePool tmp;
  double *d_mu = nullptr, *d_delta = nullptr, *d_xs = nullptr, *d_Xhat = nullptr, *d_pb = nullptr, *d_best = nullptr;
  int *d_pa = nullptr, *d_arg = nullptr;
  RB_TRY(tmp.upload(&d_mu, mu, (size_t)lay.n_sel * N));
  RB_TRY(tmp.upload(&d_delta, delta, (size_t)N));
  RB_TRY(tmp.upload(&d_xs, xt.data(), (size_t)n_nonlin * M));
  RB_TRY(tmp.alloc(&d_Xhat, (size_t)(lay.n_sel + 1) * N));
  RB_TRY(tmp.alloc(&d_pb, (size_t)nch * M));
  RB_TRY(tmp.alloc(&d_pa, (size_t)nch * M));
  RB_TRY(tmp.alloc(&d_best, (size_t)M));
  RB_TRY(tmp.alloc(&d_arg, (size_t)M));
  a.N = N; a.M = M; a.C = C; a.nchunks = nch; a.head.nN = n_nonlin; a.head.first = 0; a.head.angle_mask = lay.angle_mask;
  for (int k = 0; k < lay.n_sel; ++k) a.head.rows[k] = lay.rows[k];
  a.Xhat = d_Xhat; a.xn_next = d_xs; a.part_best = d_pb; a.part_arg = d_pa;
  // (the prologue's last row is overwritten with delta: what it reads as w does not matter)
  RB_TRY(timed_reps(reps, 0, [&] { return gs_launch_map_step(lay, a, d_mu, d_delta, d_delta, d_Xhat, nullptr, d_best, d_arg, 0); }, ms));
  HIPCHK(hipMemcpy(best, d_best, (size_t)M * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(arg, d_arg, (size_t)M * sizeof(int), hipMemcpyDeviceToHost));
  return RBPF_OK;
}

// ---- the marginal smoothing weights ------------------------------------------------------------------------------------------
int rbpf_loc_generic_marginal_workspace_bytes(int32_t n_nonlin, int32_t n_sel, int32_t quat_pos, int32_t N_P, int32_t N_T, size_t* bytes) {
  if (!bytes) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  size_t unused = 0;
  RB_TRY(rbpf_loc_generic_map_workspace_bytes(n_nonlin, n_sel, quat_pos, N_P, N_T, &unused));   // the argument checks of the MAP pass
  *bytes = marginal_bytes((size_t)n_nonlin, (size_t)n_sel, (size_t)N_P, (size_t)N_T);
  return RBPF_OK;
}

// The marginal pass (rbpf_loc_generic_marginal_*) and the statistics pass (rbpf_loc_generic_pair_stats_*: the same steps, and after
// every step's normalisation the pass of rbpf_loc_pairstats.hpp) share their entry points' bodies; a kind says which slot of LocState
// holds the open pass and how the family names itself.
struct GmKind {
  LocGenBackward LocState::*slot;
  bool stats;
  const char* noun;                // "a <noun> pass is open"
  const char* fam;                 // the entry points' common prefix
  const char* reader;              // how backward_check_forward names the reader
};
static const GmKind kGmMarginal = {&LocState::gm, false, "marginal", "rbpf_loc_generic_marginal", "marginal smoothing"};
static const GmKind kGmStats = {&LocState::gp, true, "statistics", "rbpf_loc_generic_pair_stats", "the transition statistics"};

static int gm_not_open(const GmKind& k) {
  set_error(std::string("no ") + k.noun + " pass is open (" + k.fam + "_begin first)");
  return RBPF_ERR_STATE;
}
static int gm_all_done(const GmKind& k) {
  set_error(std::string("every step of the ") + k.noun + " pass is done (" + k.fam + "_finish)");
  return RBPF_ERR_STATE;
}

static int gm_begin(const GmKind& k, rbpf_ctx* c, int32_t n_sel, const int32_t* rows, uint32_t angle_mask, int32_t quat_pos) {
  RB_TRY(gs_ctx_ok(c));
  LocState* L = c->loc;
  LocGenLayout lay;
  RB_TRY(gs_layout(L->nN, n_sel, rows, angle_mask, quat_pos, lay));
  if (L->gm.open) { set_error("a marginal pass is open on this context (rbpf_loc_generic_marginal_finish first)"); return RBPF_ERR_STATE; }
  if (L->gp.open) { set_error("a statistics pass is open on this context (rbpf_loc_generic_pair_stats_finish first)"); return RBPF_ERR_STATE; }
  if (L->fs.open) { set_error(kFsOpen); return RBPF_ERR_STATE; }
  if (L->fl.open) { set_error(kFlOpen); return RBPF_ERR_STATE; }
  if (L->gb.open) { set_error("a backward pass is open on this context (rbpf_loc_generic_backward_finish first)"); return RBPF_ERR_STATE; }
  if (L->gv.open) { set_error("a MAP pass is open on this context (rbpf_loc_generic_map_finish first)"); return RBPF_ERR_STATE; }
  RB_TRY(backward_check_forward(c, k.reader, (std::string(k.fam) + "_begin").c_str()));
  const int N = c->N, T = c->T;
  LocGenBackward& g = L->*k.slot;
  g.M = N; g.lay = lay;                                                  // (the chunking of both passes: marginal_set_sizes, per step)
  int s = k.stats ? pair_stats_take(g.ws, c->pool, L->nN, lay.n_sel, lay.n_res, N, T) : marginal_take(g.ws, c->pool, L->nN, lay.n_sel, N, T);
  if (s == RBPF_OK) {
    const hipError_t e = marginal_launch_last(g.ws, L->nN, N, T, c->X, c->w, c->stream);
    if (e != hipSuccess) s = hip_fail(e, "the last step of the marginal pass", __FILE__, __LINE__);
  }
  if (s != RBPF_OK) { g.ws.release(); g = LocGenBackward(); return s; }
  g.t = T - 2;
  g.open = true;
  return RBPF_OK;
}

static int gm_particles_device(const GmKind& k, rbpf_ctx* c, int32_t* t, const double** xn_dev) {
  RB_TRY(gs_ctx_ok(c));
  if (!t || !xn_dev) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  const LocGenBackward& g = c->loc->*k.slot;
  if (!g.open) return gm_not_open(k);
  if (g.t < 0) return gm_all_done(k);
  *t = g.t;
  *xn_dev = c->X + (size_t)g.t * c->loc->nN * c->N;
  return RBPF_OK;
}

static int gm_step_device(const GmKind& k, rbpf_ctx* c, const double* mu_dev, const double* cov) {
  RB_TRY(gs_ctx_ok(c));
  LocState* L = c->loc;
  LocGenBackward& g = L->*k.slot;
  if (!g.open) return gm_not_open(k);
  if (g.t < 0) return gm_all_done(k);
  if (!mu_dev || !cov) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  const int N = c->N, T = c->T, nN = L->nN, t = g.t;
  GmArgs a;
  std::memset(&a, 0, sizeof(a));
  RB_TRY(gs_factor_layout(cov, g.lay, a.term.W, " of step " + std::to_string(t)));
  HIPCHK(hipSetDevice(c->device));
  marginal_set_sizes(a, N, N);
  a.head.nN = nN; a.head.angle_mask = g.lay.angle_mask;
  for (int q = 0; q < g.lay.n_sel; ++q) a.head.rows[q] = g.lay.rows[q];
  a.Xhat = g.ws.Xhat; a.xn_next = c->X + (size_t)(t + 1) * nN * N; a.cj = g.ws.u + (size_t)2 * N; a.part_m = g.ws.pm; a.part_s = g.ws.ps;
  HIPCHK(gs_launch_marginal_step(g.lay, a, mu_dev, c->w + (size_t)t * N, nullptr, g.ws.Xhat, g.ws.u + (size_t)((t + 1) & 1) * N, nullptr,
                                 g.ws.u + (size_t)2 * N, g.ws.u + (size_t)(t & 1) * N, c->stream));
  HIPCHK(marginal_launch_close_step(g.ws, nN, N, T, t, c->X, c->stream));
  if (k.stats)
    HIPCHK(gs_launch_pair_stats(g.lay, gs_pair_stats_args(a, marginal_out(g.ws, nN, T).mass + t, g.ws.pstat),
                                g.ws.stat + (size_t)t * pair_stats_page(g.lay.n_res), c->stream));
  g.t = t - 1;
  return RBPF_OK;
}

static int gm_finish(const GmKind& k, rbpf_ctx* c, double* w_smooth, double* mean, double* cov, double* ess, double* mass, double* S, double* m,
                     double* pair_mass) {
  RB_TRY(gs_ctx_ok(c));
  LocState* L = c->loc;
  LocGenBackward& g = L->*k.slot;
  if (!g.open) return gm_not_open(k);
  const int N = c->N, T = c->T, nN = L->nN, t_next = g.t;
  const LocGenLayout lay = g.lay;
  BackwardWorkspace ws = g.ws;
  g = LocGenBackward();                                                  // the pass is closed whichever way this returns,
  BackwardWorkspaceGuard lease(ws);                                      // and its workspace goes back
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (t_next >= 0) {
    if (!w_smooth && !mean && !cov && !ess && !mass && !S && !m && !pair_mass) return RBPF_OK;     // the way out of a pass that was given up
    set_error(std::string(k.fam) + "_finish: steps " + std::to_string(t_next) + " .. 0 of the " + k.noun + " pass were not run");
    return RBPF_ERR_STATE;
  }
  RB_TRY(ctx_check_flags(c));
  RB_TRY(marginal_copy_out(ws, nN, N, T, w_smooth, mean, cov, ess, mass));
  return k.stats ? pair_stats_copy_out(ws, lay.n_res, T, lay.perm, S, m, pair_mass) : RBPF_OK;
}

// rbpf_loc_generic_marginal_step (S, m, pair_mass null) and rbpf_loc_generic_pair_stats_step
static int gm_probe(int32_t N, int32_t M, int32_t n_nonlin, int32_t n_sel, const int32_t* rows, uint32_t angle_mask, int32_t quat_pos,
                    const double* mu, const double* logw, const double* xs_next, const double* logws_next, const double* cov, double* D,
                    double* lws, bool stats, double* S, double* m, double* pair_mass, int32_t reps, double* ms) {
  if (!mu || !logw || !xs_next || !logws_next || !cov || !D || !lws || !rows) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  if (stats && (!S || !m || !pair_mass)) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  if (N < 1 || M < 1) { set_error("N and M must be >= 1"); return RBPF_ERR_INVALID_ARG; }
  if (N > kMaxParticles || M > kMaxParticles) { set_error("N or M above 1048576 is not supported"); return RBPF_ERR_UNSUPPORTED; }
  LocGenLayout lay;
  RB_TRY(gs_layout(n_nonlin, n_sel, rows, angle_mask, quat_pos, lay));
  GmArgs a;
  std::memset(&a, 0, sizeof(a));
  RB_TRY(gs_factor_layout(cov, lay, a.term.W, ""));
  if (!have_device()) { set_error("no HIP device: the marginal pass has no CPU fallback"); return RBPF_ERR_NO_DEVICE; }
  marginal_set_sizes(a, N, M);
  std::vector<double> xt((size_t)n_nonlin * M);                           // the successors as the history holds them: [n_nonlin][M]
  for (int j = 0; j < M; ++j)
    for (int r = 0; r < n_nonlin; ++r) xt[(size_t)r * M + j] = xs_next[(size_t)j * n_nonlin + r];
  const size_t np = marginal_part_count((size_t)N, (size_t)M);
  DevicePool tmp;
  double *d_mu = nullptr, *d_lw = nullptr, *d_xs = nullptr, *d_lwn = nullptr, *d_Xhat = nullptr, *d_pm = nullptr, *d_ps = nullptr, *d_D = nullptr,
         *d_c = nullptr, *d_lws = nullptr, *d_nrm = nullptr, *d_part = nullptr, *d_page = nullptr;
  RB_TRY(tmp.upload(&d_mu, mu, (size_t)lay.n_sel * N));
  RB_TRY(tmp.upload(&d_lw, logw, (size_t)N));
  RB_TRY(tmp.upload(&d_xs, xt.data(), (size_t)n_nonlin * M));
  RB_TRY(tmp.upload(&d_lwn, logws_next, (size_t)M));
  RB_TRY(tmp.alloc(&d_Xhat, (size_t)(lay.n_sel + 1) * N));
  RB_TRY(tmp.alloc(&d_pm, np));
  RB_TRY(tmp.alloc(&d_ps, np));
  RB_TRY(tmp.alloc(&d_D, (size_t)M));
  RB_TRY(tmp.alloc(&d_c, (size_t)M));
  RB_TRY(tmp.alloc(&d_lws, (size_t)N));
  if (stats) {
    RB_TRY(tmp.alloc(&d_nrm, (size_t)2 * N + 1));                        // the normalised copy of lws, its weights, the mass
    RB_TRY(tmp.alloc(&d_part, (size_t)pair_stats_count(lay.n_res) * pair_stats_groups((size_t)N, (size_t)M)));
    RB_TRY(tmp.alloc(&d_page, (size_t)pair_stats_page(lay.n_res)));
  }
  a.head.nN = n_nonlin; a.head.first = 0; a.head.angle_mask = lay.angle_mask;
  for (int k = 0; k < lay.n_sel; ++k) a.head.rows[k] = lay.rows[k];
  a.Xhat = d_Xhat; a.xn_next = d_xs; a.cj = d_c; a.part_m = d_pm; a.part_s = d_ps;
  // (the prologue's last row is overwritten with the caller's log w: what it reads as w does not matter)
  RB_TRY(timed_reps(reps, 0, [&] {
    hipError_t e = gs_launch_marginal_step(lay, a, d_mu, d_lw, d_lw, d_Xhat, d_lwn, d_D, d_c, d_lws, 0);
    if (e != hipSuccess || !stats) return e;
    e = hipMemcpyAsync(d_nrm, d_lws, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, 0);
    if (e != hipSuccess) return e;
    e = marginal_launch_normalise(N, d_nrm, d_nrm + N, d_nrm + (size_t)2 * N, 0);
    if (e != hipSuccess) return e;
    return gs_launch_pair_stats(lay, gs_pair_stats_args(a, d_nrm + (size_t)2 * N, d_part), d_page, 0);
  }, ms));
  HIPCHK(hipMemcpy(D, d_D, (size_t)M * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(lws, d_lws, (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
  if (stats) {
    BackwardWorkspace view;
    view.stat = d_page;
    RB_TRY(pair_stats_copy_out(view, lay.n_res, 2, lay.perm, S, m, pair_mass));
  }
  return RBPF_OK;
}

int rbpf_loc_generic_marginal_begin(rbpf_ctx* c, int32_t n_sel, const int32_t* rows, uint32_t angle_mask, int32_t quat_pos) {
  return gm_begin(kGmMarginal, c, n_sel, rows, angle_mask, quat_pos);
}

int rbpf_loc_generic_marginal_particles_device(rbpf_ctx* c, int32_t* t, const double** xn_dev) { return gm_particles_device(kGmMarginal, c, t, xn_dev); }

int rbpf_loc_generic_marginal_step_device(rbpf_ctx* c, const double* mu_dev, const double* cov) { return gm_step_device(kGmMarginal, c, mu_dev, cov); }

int rbpf_loc_generic_marginal_finish(rbpf_ctx* c, double* w_smooth, double* mean, double* cov, double* ess, double* mass) {
  return gm_finish(kGmMarginal, c, w_smooth, mean, cov, ess, mass, nullptr, nullptr, nullptr);
}

int rbpf_loc_generic_marginal_step(int32_t N, int32_t M, int32_t n_nonlin, int32_t n_sel, const int32_t* rows, uint32_t angle_mask,
                                   int32_t quat_pos, const double* mu, const double* logw, const double* xs_next, const double* logws_next,
                                   const double* cov, double* D, double* lws, int32_t reps, double* ms) {
  return gm_probe(N, M, n_nonlin, n_sel, rows, angle_mask, quat_pos, mu, logw, xs_next, logws_next, cov, D, lws, false, nullptr, nullptr, nullptr,
                  reps, ms);
}

// ---- the two-slice statistics of the transition residual ---------------------------------------------------------------------
int rbpf_loc_generic_pair_stats_workspace_bytes(int32_t n_nonlin, int32_t n_sel, int32_t quat_pos, int32_t N_P, int32_t N_T, size_t* bytes) {
  RB_TRY(rbpf_loc_generic_marginal_workspace_bytes(n_nonlin, n_sel, quat_pos, N_P, N_T, bytes));   // its argument checks
  *bytes = pair_stats_bytes((size_t)n_nonlin, (size_t)n_sel, (size_t)(quat_pos == -1 ? n_sel : n_sel - 1), (size_t)N_P, (size_t)N_T);
  return RBPF_OK;
}

int rbpf_loc_generic_pair_stats_begin(rbpf_ctx* c, int32_t n_sel, const int32_t* rows, uint32_t angle_mask, int32_t quat_pos) {
  return gm_begin(kGmStats, c, n_sel, rows, angle_mask, quat_pos);
}

int rbpf_loc_generic_pair_stats_particles_device(rbpf_ctx* c, int32_t* t, const double** xn_dev) { return gm_particles_device(kGmStats, c, t, xn_dev); }

int rbpf_loc_generic_pair_stats_step_device(rbpf_ctx* c, const double* mu_dev, const double* cov) { return gm_step_device(kGmStats, c, mu_dev, cov); }

int rbpf_loc_generic_pair_stats_finish(rbpf_ctx* c, double* w_smooth, double* mean, double* cov, double* ess, double* mass, double* S, double* m,
                                       double* pair_mass) {
  return gm_finish(kGmStats, c, w_smooth, mean, cov, ess, mass, S, m, pair_mass);
}

int rbpf_loc_generic_pair_stats_step(int32_t N, int32_t M, int32_t n_nonlin, int32_t n_sel, const int32_t* rows, uint32_t angle_mask,
                                     int32_t quat_pos, const double* mu, const double* logw, const double* xs_next, const double* logws_next,
                                     const double* cov, double* D, double* lws, double* S, double* m, double* pair_mass, int32_t reps,
                                     double* ms) {
  return gm_probe(N, M, n_nonlin, n_sel, rows, angle_mask, quat_pos, mu, logw, xs_next, logws_next, cov, D, lws, true, S, m, pair_mass, reps, ms);
}

// ---- the running two-slice statistics (rbpf_loc_forwardstats.hpp) ------------------------------------------------------------
typedef ForwardStatsArgs<GsData> GfArgs;

static hipError_t gs_launch_forward_stats(const LocGenLayout& y, const GmArgs& a, const GfArgs& b, const double* mu, const double* w,
                                          const double* logw, const ForwardCarry& f, double* tau_next, const double* w_next, double* page,
                                          hipStream_t s) {
  gs_launch_prologue(y, a.N, mu, w, f.Xhat, s);
  if (logw) {
    const hipError_t e = hipMemcpyAsync(f.Xhat + (size_t)y.n_sel * a.N, logw, (size_t)a.N * sizeof(double), hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return e;
  }
  return gs_pick(y, a.head.angle_mask, [&](auto tag) {
    typedef typename decltype(tag)::Term Term;
    return forward_stats_launch_step(a.with(Term{a.term}), b.with(Term{b.term}), f.zero, f.D, f.cj, tau_next, f.reach, w_next, page, s);
  });
}

// the head, the sizes and the buffers of a step (xn_next, tau, s_scale and the term's W are the caller's)
static void gs_forward_stats_args(const ForwardCarry& f, const LocGenLayout& lay, int nN, int N, int M, GmArgs& a, GfArgs& b) {
  std::memset(&b, 0, sizeof(b));
  forward_stats_set(f, N, M, a, b);
  a.head.nN = nN; a.head.first = 0; a.head.angle_mask = lay.angle_mask;
  for (int q = 0; q < lay.n_sel; ++q) a.head.rows[q] = lay.rows[q];
  b.head = a.head; b.term = a.term;
}

static bool gs_same_layout(const LocGenLayout& p, const LocGenLayout& q) {
  if (p.n_sel != q.n_sel || p.n_res != q.n_res || p.n_plain != q.n_plain || p.angle_mask != q.angle_mask) return false;
  for (int k = 0; k < 8; ++k)
    if (p.rows[k] != q.rows[k] || p.src[k] != q.src[k] || p.perm[k] != q.perm[k]) return false;
  return true;
}

static int gf_not_open() {
  set_error("no running-statistics stepping is open (rbpf_loc_generic_forward_stats_begin first)");
  return RBPF_ERR_STATE;
}

int rbpf_loc_generic_forward_stats_workspace_bytes(int32_t n_nonlin, int32_t n_sel, int32_t quat_pos, int32_t N_P, int32_t N_T, size_t* bytes) {
  RB_TRY(rbpf_loc_generic_marginal_workspace_bytes(n_nonlin, n_sel, quat_pos, N_P, N_T, bytes));   // its argument checks
  *bytes = forward_stats_bytes((size_t)n_sel, (size_t)(quat_pos == -1 ? n_sel : n_sel - 1), (size_t)N_P, (size_t)N_T);
  return RBPF_OK;
}

int rbpf_loc_generic_forward_stats_reset(rbpf_ctx* c) {
  RB_TRY(gs_ctx_ok(c));
  if (c->loc->fs.open) { set_error(kFsOpen); return RBPF_ERR_STATE; }
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->loc->fs.release();
  return RBPF_OK;
}

int rbpf_loc_generic_forward_stats_begin(rbpf_ctx* c, int32_t n_sel, const int32_t* rows, uint32_t angle_mask, int32_t quat_pos) {
  RB_TRY(gs_ctx_ok(c));
  LocState* L = c->loc;
  LocGenLayout lay;
  RB_TRY(gs_layout(L->nN, n_sel, rows, angle_mask, quat_pos, lay));
  if (L->fs.open) { set_error(kFsOpen); return RBPF_ERR_STATE; }
  if (L->fl.open) { set_error(kFlOpen); return RBPF_ERR_STATE; }
  if (L->gm.open) { set_error("a marginal pass is open on this context (rbpf_loc_generic_marginal_finish first)"); return RBPF_ERR_STATE; }
  if (L->gp.open) { set_error("a statistics pass is open on this context (rbpf_loc_generic_pair_stats_finish first)"); return RBPF_ERR_STATE; }
  if (L->gb.open) { set_error("a backward pass is open on this context (rbpf_loc_generic_backward_finish first)"); return RBPF_ERR_STATE; }
  if (L->gv.open) { set_error("a MAP pass is open on this context (rbpf_loc_generic_map_finish first)"); return RBPF_ERR_STATE; }
  RB_TRY(forward_stats_check_forward(c, "rbpf_loc_generic_forward_stats_begin"));
  ForwardCarry& f = L->fs;
  if (f.alive && !gs_same_layout(f.lay, lay)) {
    set_error("the carry of the running statistics was built with other rows (rbpf_loc_generic_forward_stats_reset first)");
    return RBPF_ERR_STATE;
  }
  if (!f.alive) {
    RB_TRY(forward_stats_take(f, c->pool, L->nN, lay.n_sel, lay.n_res, c->N, c->N, c->T - 1, c->stream));
    f.lay = lay;
  }
  f.open = true;
  return RBPF_OK;
}

int rbpf_loc_generic_forward_stats_particles_device(rbpf_ctx* c, int32_t* t, const double** xn_dev) {
  RB_TRY(gs_ctx_ok(c));
  if (!t || !xn_dev) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  const ForwardCarry& f = c->loc->fs;
  if (!f.open) return gf_not_open();
  if (f.folded + 1 >= c->t) { set_error("every stored pair of steps is folded in (rbpf_loc_generic_forward_stats_finish)"); return RBPF_ERR_STATE; }
  *t = f.folded;
  *xn_dev = c->X + (size_t)f.folded * c->loc->nN * c->N;
  return RBPF_OK;
}

int rbpf_loc_generic_forward_stats_step_device(rbpf_ctx* c, const double* mu_dev, const double* cov, double s_scale) {
  RB_TRY(gs_ctx_ok(c));
  LocState* L = c->loc;
  ForwardCarry& f = L->fs;
  if (!f.open) return gf_not_open();
  if (f.folded + 1 >= c->t) { set_error("every stored pair of steps is folded in (rbpf_loc_generic_forward_stats_finish)"); return RBPF_ERR_STATE; }
  if (!mu_dev || !cov) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  if (!(s_scale >= 0.0) || !std::isfinite(s_scale)) { set_error("s_scale (1 / dt of the step) must be finite and >= 0"); return RBPF_ERR_INVALID_ARG; }
  const int N = c->N, nN = L->nN, t = f.folded;
  const size_t KF = (size_t)forward_stats_carry(f.n_res);
  GmArgs a;
  GfArgs b;
  std::memset(&a, 0, sizeof(a));
  RB_TRY(gs_factor_layout(cov, f.lay, a.term.W, " of step " + std::to_string(t)));
  HIPCHK(hipSetDevice(c->device));
  gs_forward_stats_args(f, f.lay, nN, N, N, a, b);
  a.xn_next = b.xn_next = c->X + (size_t)(t + 1) * nN * N;
  b.tau = f.tau + (size_t)f.cur * KF * N; b.s_scale = s_scale;
  HIPCHK(gs_launch_forward_stats(f.lay, a, b, mu_dev, c->w + (size_t)t * N, nullptr, f, f.tau + (size_t)(f.cur ^ 1) * KF * N,
                                 c->w + (size_t)(t + 1) * N, f.pages + (size_t)t * pair_stats_page(f.n_res), c->stream));
  f.cur ^= 1;
  f.folded = t + 1;
  return RBPF_OK;
}

int rbpf_loc_generic_forward_stats_finish(rbpf_ctx* c, double* S_run, double* m_run, double* mass_run, double* tau_S, double* tau_m) {
  RB_TRY(gs_ctx_ok(c));
  ForwardCarry& f = c->loc->fs;
  if (!f.open) return gf_not_open();
  f.open = false;                                                        // the stepping is closed whichever way this returns; the carry stays
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (f.folded + 1 < c->t) {
    if (!S_run && !m_run && !mass_run && !tau_S && !tau_m) return RBPF_OK;     // the way out of a stepping that was given up
    set_error("rbpf_loc_generic_forward_stats_finish: the pairs of steps from " + std::to_string(f.folded) + " on were not folded in");
    return RBPF_ERR_STATE;
  }
  RB_TRY(ctx_check_flags(c));
  return forward_stats_copy_out(f, c->N, f.lay.perm, S_run, m_run, mass_run, tau_S, tau_m);
}

int rbpf_loc_generic_forward_stats_step(int32_t N, int32_t M, int32_t n_nonlin, int32_t n_sel, const int32_t* rows, uint32_t angle_mask,
                                        int32_t quat_pos, const double* mu, const double* logw, const double* xs_next, const double* tau_S,
                                        const double* tau_m, const double* cov, double s_scale, double* D, double* tau_S_next,
                                        double* tau_m_next, double* reach, int32_t reps, double* ms) {
  if (!mu || !logw || !xs_next || !tau_S || !tau_m || !cov || !D || !tau_S_next || !tau_m_next || !reach || !rows) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  if (N < 1 || M < 1) { set_error("N and M must be >= 1"); return RBPF_ERR_INVALID_ARG; }
  if (N > kMaxParticles || M > kMaxParticles) { set_error("N or M above 1048576 is not supported"); return RBPF_ERR_UNSUPPORTED; }
  if (!(s_scale >= 0.0) || !std::isfinite(s_scale)) { set_error("s_scale (1 / dt of the step) must be finite and >= 0"); return RBPF_ERR_INVALID_ARG; }
  LocGenLayout lay;
  RB_TRY(gs_layout(n_nonlin, n_sel, rows, angle_mask, quat_pos, lay));
  GmArgs a;
  GfArgs b;
  std::memset(&a, 0, sizeof(a));
  RB_TRY(gs_factor_layout(cov, lay, a.term.W, ""));
  if (!have_device()) { set_error("no HIP device: the running statistics have no CPU fallback"); return RBPF_ERR_NO_DEVICE; }
  const int NR = lay.n_res;
  const size_t KF = (size_t)forward_stats_carry(NR), ld = (size_t)std::max(N, M);
  std::vector<double> xt((size_t)n_nonlin * M), tk(KF * N);               // the successors as the history holds them: [n_nonlin][M]
  for (int j = 0; j < M; ++j)
    for (int r = 0; r < n_nonlin; ++r) xt[(size_t)r * M + j] = xs_next[(size_t)j * n_nonlin + r];
  forward_stats_pack(NR, N, lay.perm, tau_S, tau_m, tk.data());
  DevicePool tmp;
  ForwardCarry f;
  RB_TRY(forward_stats_take(f, tmp, n_nonlin, lay.n_sel, NR, N, M, 1, 0));
  double *d_mu = nullptr, *d_lw = nullptr, *d_xs = nullptr, *d_wn = nullptr;
  RB_TRY(tmp.upload(&d_mu, mu, (size_t)lay.n_sel * N));
  RB_TRY(tmp.upload(&d_lw, logw, (size_t)N));
  RB_TRY(tmp.upload(&d_xs, xt.data(), (size_t)n_nonlin * M));
  RB_TRY(tmp.alloc(&d_wn, (size_t)M));
  HIPCHK(hipMemcpy(f.tau, tk.data(), tk.size() * sizeof(double), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(forward_stats_fill_kernel, dim3((M + 255) / 256), dim3(256), 0, 0, M, 1.0 / M, d_wn);   // (the reducer's weights: uniform)
  gs_forward_stats_args(f, lay, n_nonlin, N, M, a, b);
  a.xn_next = b.xn_next = d_xs;
  b.tau = f.tau; b.s_scale = s_scale;
  double* tau_next = f.tau + KF * ld;
  // (the prologue's last row is overwritten with the caller's log w: what it reads as w does not matter)
  RB_TRY(timed_reps(reps, 0, [&] { return gs_launch_forward_stats(lay, a, b, d_mu, d_lw, d_lw, f, tau_next, d_wn, f.pages, 0); }, ms));
  std::vector<double> tn(KF * M);
  HIPCHK(hipMemcpy(D, f.D, (size_t)M * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(reach, f.reach, (size_t)M * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(tn.data(), tau_next, tn.size() * sizeof(double), hipMemcpyDeviceToHost));
  forward_stats_unpack(NR, M, lay.perm, tn.data(), tau_S_next, tau_m_next);
  return RBPF_OK;
}

// ---- the fixed-lag smoother (rbpf_loc_fixedlag.hpp) ------------------------------------------------------------------------------
typedef FixedLagArgs<GsData> GlArgs;

static hipError_t gs_launch_fixed_lag(const LocGenLayout& y, const GmArgs& a, const GlArgs& b, const double* mu, const double* w,
                                      const double* logw, const FixedLagCarry& f, int moments, const double* X_next, const double* w_next,
                                      double* T_next, double* c_next, double* page, hipStream_t s) {
  gs_launch_prologue(y, a.N, mu, w, f.Xhat, s);
  if (logw) {
    const hipError_t e = hipMemcpyAsync(f.Xhat + (size_t)y.n_sel * a.N, logw, (size_t)a.N * sizeof(double), hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return e;
  }
  return gs_pick(y, a.head.angle_mask, [&](auto tag) {
    typedef typename decltype(tag)::Term Term;
    return fixed_lag_launch_step(a.with(Term{a.term}), b.with(Term{b.term}), f, moments, X_next, w_next, T_next, c_next, page, s);
  });
}

// the head, the sizes and the buffers of a step (xn_next, tau and the term's W are the caller's)
static void gs_fixed_lag_args(const FixedLagCarry& f, const LocGenLayout& lay, int nN, int N, int M, GmArgs& a, GlArgs& b) {
  std::memset(&b, 0, sizeof(b));
  fixed_lag_set(f, N, M, a, b);
  a.head.nN = nN; a.head.first = 0; a.head.angle_mask = lay.angle_mask;
  for (int q = 0; q < lay.n_sel; ++q) a.head.rows[q] = lay.rows[q];
  b.head = a.head; b.term = a.term;
}

static int gl_not_open() {
  set_error("no fixed-lag stepping is open (rbpf_loc_generic_fixed_lag_begin first)");
  return RBPF_ERR_STATE;
}

int rbpf_loc_generic_fixed_lag_workspace_bytes(int32_t n_nonlin, int32_t n_sel, int32_t quat_pos, int32_t N_P, int32_t N_T, int32_t lag,
                                               int32_t moments, size_t* bytes) {
  RB_TRY(rbpf_loc_generic_marginal_workspace_bytes(n_nonlin, n_sel, quat_pos, N_P, N_T, bytes));   // its argument checks
  RB_TRY(fixed_lag_check_lag(lag, moments));
  *bytes = fixed_lag_bytes((size_t)n_nonlin, (size_t)n_sel, (size_t)lag, (size_t)moments, (size_t)N_P, (size_t)N_T);
  return RBPF_OK;
}

int rbpf_loc_generic_fixed_lag_reset(rbpf_ctx* c) {
  RB_TRY(gs_ctx_ok(c));
  if (c->loc->fl.open) { set_error(kFlOpen); return RBPF_ERR_STATE; }
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->loc->fl.release();
  return RBPF_OK;
}

int rbpf_loc_generic_fixed_lag_begin(rbpf_ctx* c, int32_t n_sel, const int32_t* rows, uint32_t angle_mask, int32_t quat_pos, int32_t lag,
                                     int32_t moments) {
  RB_TRY(gs_ctx_ok(c));
  LocState* L = c->loc;
  LocGenLayout lay;
  RB_TRY(gs_layout(L->nN, n_sel, rows, angle_mask, quat_pos, lay));
  RB_TRY(fixed_lag_check_lag(lag, moments));
  if (L->fl.open) { set_error(kFlOpen); return RBPF_ERR_STATE; }
  if (L->fs.open) { set_error(kFsOpen); return RBPF_ERR_STATE; }
  if (L->gm.open) { set_error("a marginal pass is open on this context (rbpf_loc_generic_marginal_finish first)"); return RBPF_ERR_STATE; }
  if (L->gp.open) { set_error("a statistics pass is open on this context (rbpf_loc_generic_pair_stats_finish first)"); return RBPF_ERR_STATE; }
  if (L->gb.open) { set_error("a backward pass is open on this context (rbpf_loc_generic_backward_finish first)"); return RBPF_ERR_STATE; }
  if (L->gv.open) { set_error("a MAP pass is open on this context (rbpf_loc_generic_map_finish first)"); return RBPF_ERR_STATE; }
  RB_TRY(forward_stats_check_forward(c, "rbpf_loc_generic_fixed_lag_begin"));
  FixedLagCarry& f = L->fl;
  if (f.alive) {
    RB_TRY(fixed_lag_same(f, lag, moments, "rbpf_loc_generic_fixed_lag_reset"));
    if (!gs_same_layout(f.lay, lay)) {
      set_error("the carry of the fixed-lag smoother was built with other rows (rbpf_loc_generic_fixed_lag_reset first)");
      return RBPF_ERR_STATE;
    }
  } else {
    const int H = fixed_lag_columns(L->nN, moments);
    RB_TRY(fixed_lag_take(f, c->pool, L->nN, lay.n_sel, lag * H, H, c->N, c->N, c->T, c->stream));
    f.lay = lay; f.lag = lag; f.moments = moments;
  }
  if (f.entered == 0) {                                                  // step 0 enters: no all-pairs work
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(fixed_lag_launch_enter(f, moments, c->N, c->X, c->w, f.T + (size_t)f.cur * (f.K + f.H) * c->N, nullptr, f.cs, f.pages, c->stream));
    f.entered = 1;
  }
  f.open = true;
  return RBPF_OK;
}

int rbpf_loc_generic_fixed_lag_particles_device(rbpf_ctx* c, int32_t* t, const double** xn_dev) {
  RB_TRY(gs_ctx_ok(c));
  if (!t || !xn_dev) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  const FixedLagCarry& f = c->loc->fl;
  if (!f.open) return gl_not_open();
  if (f.entered >= c->t) { set_error("every stored step is folded in (rbpf_loc_generic_fixed_lag_finish)"); return RBPF_ERR_STATE; }
  *t = f.entered - 1;
  *xn_dev = c->X + (size_t)(f.entered - 1) * c->loc->nN * c->N;
  return RBPF_OK;
}

int rbpf_loc_generic_fixed_lag_step_device(rbpf_ctx* c, const double* mu_dev, const double* cov) {
  RB_TRY(gs_ctx_ok(c));
  LocState* L = c->loc;
  FixedLagCarry& f = L->fl;
  if (!f.open) return gl_not_open();
  if (f.entered >= c->t) { set_error("every stored step is folded in (rbpf_loc_generic_fixed_lag_finish)"); return RBPF_ERR_STATE; }
  if (!mu_dev || !cov) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  const int N = c->N, nN = L->nN, t = f.entered - 1;
  const size_t half = (size_t)(f.K + f.H) * N, page = (size_t)f.K + f.H + 1;
  GmArgs a;
  GlArgs b;
  std::memset(&a, 0, sizeof(a));
  RB_TRY(gs_factor_layout(cov, f.lay, a.term.W, " of step " + std::to_string(t)));
  HIPCHK(hipSetDevice(c->device));
  gs_fixed_lag_args(f, f.lay, nN, N, N, a, b);
  a.xn_next = b.xn_next = c->X + (size_t)(t + 1) * nN * N;
  b.tau = f.T + (size_t)f.cur * half;
  HIPCHK(gs_launch_fixed_lag(f.lay, a, b, mu_dev, c->w + (size_t)t * N, nullptr, f, f.moments, c->X + (size_t)(t + 1) * nN * N,
                             c->w + (size_t)(t + 1) * N, f.T + (size_t)(f.cur ^ 1) * half, f.cs + (size_t)(t + 1) * nN,
                             f.pages + (size_t)(t + 1) * page, c->stream));
  f.cur ^= 1;
  f.entered = t + 2;
  return RBPF_OK;
}

int rbpf_loc_generic_fixed_lag_finish(rbpf_ctx* c, double* pages, double* means) {
  RB_TRY(gs_ctx_ok(c));
  FixedLagCarry& f = c->loc->fl;
  if (!f.open) return gl_not_open();
  f.open = false;                                                        // the stepping is closed whichever way this returns; the carry stays
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (f.entered < c->t) {
    if (!pages && !means) return RBPF_OK;                                // the way out of a stepping that was given up
    set_error("rbpf_loc_generic_fixed_lag_finish: the steps from " + std::to_string(f.entered) + " on were not folded in");
    return RBPF_ERR_STATE;
  }
  RB_TRY(ctx_check_flags(c));
  return fixed_lag_copy_out(f, pages, means);
}

int rbpf_loc_generic_fixed_lag_step(int32_t N, int32_t M, int32_t K, int32_t moments, int32_t n_nonlin, int32_t n_sel, const int32_t* rows,
                                    uint32_t angle_mask, int32_t quat_pos, const double* mu, const double* logw, const double* xs_next,
                                    const double* tau, const double* cov, double* D, double* tau_next, double* reach, int32_t reps,
                                    double* ms) {
  if (!mu || !logw || !xs_next || !tau || !cov || !D || !tau_next || !reach || !rows) { set_error("NULL argument"); return RBPF_ERR_INVALID_ARG; }
  if (N < 1 || M < 1 || K < 1) { set_error("N, M and K must be >= 1"); return RBPF_ERR_INVALID_ARG; }
  if (N > kMaxParticles || M > kMaxParticles || K > kFixedLagMaxLag * fixed_lag_columns(kBackwardMaxRows, 2)) { set_error("N or M above 1048576 or K above 64 x 44 is not supported"); return RBPF_ERR_UNSUPPORTED; }
  RB_TRY(fixed_lag_check_lag(1, moments));
  LocGenLayout lay;
  RB_TRY(gs_layout(n_nonlin, n_sel, rows, angle_mask, quat_pos, lay));
  GmArgs a;
  GlArgs b;
  std::memset(&a, 0, sizeof(a));
  RB_TRY(gs_factor_layout(cov, lay, a.term.W, ""));
  if (!have_device()) { set_error("no HIP device: the fixed-lag smoother has no CPU fallback"); return RBPF_ERR_NO_DEVICE; }
  const int H = fixed_lag_columns(n_nonlin, moments);
  const size_t ld = (size_t)std::max(N, M);
  std::vector<double> xt((size_t)n_nonlin * M);                           // the successors as the history holds them: [n_nonlin][M]
  for (int j = 0; j < M; ++j)
    for (int r = 0; r < n_nonlin; ++r) xt[(size_t)r * M + j] = xs_next[(size_t)j * n_nonlin + r];
  DevicePool tmp;
  FixedLagCarry f;
  RB_TRY(fixed_lag_take(f, tmp, n_nonlin, lay.n_sel, K, H, N, M, 1, 0));
  double *d_mu = nullptr, *d_lw = nullptr, *d_xs = nullptr, *d_wn = nullptr;
  RB_TRY(tmp.upload(&d_mu, mu, (size_t)lay.n_sel * N));
  RB_TRY(tmp.upload(&d_lw, logw, (size_t)N));
  RB_TRY(tmp.upload(&d_xs, xt.data(), (size_t)n_nonlin * M));
  RB_TRY(tmp.alloc(&d_wn, (size_t)M));
  HIPCHK(hipMemcpy(f.T, tau, (size_t)K * N * sizeof(double), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(forward_stats_fill_kernel, dim3((M + 255) / 256), dim3(256), 0, 0, M, 1.0 / M, d_wn);   // (the reducer's weights: uniform)
  gs_fixed_lag_args(f, lay, n_nonlin, N, M, a, b);
  a.xn_next = b.xn_next = d_xs;
  b.tau = f.T;
  double* T_next = f.T + (size_t)(K + H) * ld;
  // (the prologue's last row is overwritten with the caller's log w: what it reads as w does not matter)
  RB_TRY(timed_reps(reps, 0, [&] { return gs_launch_fixed_lag(lay, a, b, d_mu, d_lw, d_lw, f, moments, d_xs, d_wn, T_next, f.cs, f.pages, 0); }, ms));
  HIPCHK(hipMemcpy(D, f.D, (size_t)M * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(reach, f.reach, (size_t)M * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(tau_next, T_next + (size_t)H * M, (size_t)K * M * sizeof(double), hipMemcpyDeviceToHost));
  return RBPF_OK;
}

}  // extern "C"
