// State of a localisation context (rbpf_ctx::loc), shared by the filter (rbpf_loc.hip), the backward-simulation smoother
// (rbpf_loc_smooth.hip) and localisation in the map of a generic device-code model (rbpf_loc_generic.hip), dense or of landmarks
// (rbpf_loc_landmark.hip).
#pragma once
#include "../../include/rbpf.h"
#include "rbpf_devmem.hpp"

#include <vector>

namespace rbpf {

// How the selected rows of a transition reach the kernels.  With a quaternion block (rbpf_loc_generic_backward_pose_*) the KERNEL
// ORDER is the plain rows in the caller's order, then q0 .. q3; without one it is the caller's order and both maps are the identity.
struct LocGenLayout {
  int n_sel = 0;                   // selected state rows = rows of mu; n_res + 1 with a block
  int n_res = 0;                   // residuals = order of cov
  int n_plain = -1;                // with a block: the plain rows before it in kernel order, 0 .. 4; -1: no block
  int rows[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // state rows, kernel order
  unsigned angle_mask = 0;         // bit k: kernel row k is an angle
  int src[8] = {0, 1, 2, 3, 4, 5, 6, 7};    // kernel row k is row src[k] of the caller's mu
  int perm[8] = {0, 1, 2, 3, 4, 5, 6, 7};   // kernel residual k is residual perm[k] of the caller's cov
};

// The device buffers of a backward-simulation pass (rbpf_loc_backward.hpp), leased from a pool (rbpf_ctx::pool) and handed back by
// release().  It is plain data with no destructor (LocGenBackward keeps one across calls); a scope that must hand it back on every
// way out holds a BackwardWorkspaceGuard on it.
struct BackwardWorkspace {
  DevicePool* pool = nullptr;
  double *Xhat = nullptr;          // [rows + 1][N]
  double *pm = nullptr, *ps = nullptr;   // [nchunks][M] each: n_part
  double *u = nullptr;             // [T][M]: n_draws
  double *xs = nullptr, *mean = nullptr;
  int* idx = nullptr;              // [T][M]: n_draws
  int* arg = nullptr;              // a MAP pass only (take_map)
  double *pstat = nullptr, *stat = nullptr;   // a statistics pass only (take_pair_stats)
  // all or nothing: a failed allocation hands back what was taken before it
  int take(DevicePool& from, size_t n_Xhat, size_t n_part, size_t n_draws, size_t n_xs, size_t n_mean) {
    pool = &from;
    int s = from.alloc(&Xhat, n_Xhat);
    if (s == RBPF_OK) s = from.alloc(&pm, n_part);
    if (s == RBPF_OK) s = from.alloc(&ps, n_part);
    if (s == RBPF_OK) s = from.alloc(&u, n_draws);
    if (s == RBPF_OK) s = from.alloc(&xs, n_xs);
    if (s == RBPF_OK) s = from.alloc(&mean, n_mean);
    if (s == RBPF_OK) s = from.alloc(&idx, n_draws);
    if (s != RBPF_OK) release();
    return s;
  }
  // the buffers of a MAP pass (rbpf_loc_viterbi.hpp) in the same fields: pm and arg [n_part] the chunk partials (best, arg max),
  // u [n_delta] two rows of delta, idx [n_psi] psi and the path's index, mean [n_xmap] x_map and the score; ps and xs stay null
  int take_map(DevicePool& from, size_t n_Xhat, size_t n_part, size_t n_delta, size_t n_psi, size_t n_xmap) {
    pool = &from;
    int s = from.alloc(&Xhat, n_Xhat);
    if (s == RBPF_OK) s = from.alloc(&pm, n_part);
    if (s == RBPF_OK) s = from.alloc(&arg, n_part);
    if (s == RBPF_OK) s = from.alloc(&u, n_delta);
    if (s == RBPF_OK) s = from.alloc(&idx, n_psi);
    if (s == RBPF_OK) s = from.alloc(&mean, n_xmap);
    if (s != RBPF_OK) release();
    return s;
  }
  // the buffers of a marginal-smoothing pass (rbpf_loc_marginal.hpp) in the same fields: pm and ps [n_part] the chunk partials of both
  // passes, u [n_lw] two rows of log w_{.|T} and c, xs [n_w] w_smooth, mean [n_out] mean, cov, ess and mass of every step; idx and
  // arg stay null
  int take_marginal(DevicePool& from, size_t n_Xhat, size_t n_part, size_t n_lw, size_t n_w, size_t n_out) {
    pool = &from;
    int s = from.alloc(&Xhat, n_Xhat);
    if (s == RBPF_OK) s = from.alloc(&pm, n_part);
    if (s == RBPF_OK) s = from.alloc(&ps, n_part);
    if (s == RBPF_OK) s = from.alloc(&u, n_lw);
    if (s == RBPF_OK) s = from.alloc(&xs, n_w);
    if (s == RBPF_OK) s = from.alloc(&mean, n_out);
    if (s != RBPF_OK) release();
    return s;
  }
  // the buffers of a two-slice statistics pass (rbpf_loc_pairstats.hpp): those of a marginal pass, pstat [n_pstat] the workgroups'
  // vectors of the statistics pass and stat [n_stat] its pages (S, m and the pair mass of every pair of steps)
  int take_pair_stats(DevicePool& from, size_t n_Xhat, size_t n_part, size_t n_lw, size_t n_w, size_t n_out, size_t n_pstat, size_t n_stat) {
    int s = take_marginal(from, n_Xhat, n_part, n_lw, n_w, n_out);
    if (s == RBPF_OK) s = from.alloc(&pstat, n_pstat);
    if (s == RBPF_OK) s = from.alloc(&stat, n_stat);
    if (s != RBPF_OK) release();
    return s;
  }
  void release() {
    if (pool)
      for (void* p : {(void*)Xhat, (void*)pm, (void*)ps, (void*)u, (void*)xs, (void*)mean, (void*)idx, (void*)arg, (void*)pstat, (void*)stat})
        pool->release(p);
    *this = BackwardWorkspace();
  }
};

struct BackwardWorkspaceGuard {
  BackwardWorkspace& ws;
  explicit BackwardWorkspaceGuard(BackwardWorkspace& w) : ws(w) {}
  BackwardWorkspaceGuard(const BackwardWorkspaceGuard&) = delete;
  BackwardWorkspaceGuard& operator=(const BackwardWorkspaceGuard&) = delete;
  ~BackwardWorkspaceGuard() { ws.release(); }
};

// What rejection-sampling backward simulation (rbpf_loc_reject.hpp) keeps next to a BackwardWorkspace, leased and handed back the
// same way: the cdf of a step's weights, what the tries left per trajectory, and the compacted rows of the trajectories that fall
// back to the all-pairs pass.  (The chunk partials of that pass are the BackwardWorkspace's pm / ps, sized by reject_part_count.)
struct RejectWorkspace {
  DevicePool* pool = nullptr;
  double *cdf = nullptr, *btot = nullptr;   // [N] inclusive prefix sums of w[t]; [blocks] the totals of their first level
  double *xs_c = nullptr, *u_c = nullptr;   // [M][rows], [M]: successors and uniforms of the trajectories that fall back, ascending j
  int *acc = nullptr, *tries = nullptr;     // [M]: the accepted particle or -1; tries made
  int *pos = nullptr, *fb = nullptr;        // [M]: row of trajectory j among the compacted ones or -1; the fallback's index per row
  int* bcnt = nullptr;                      // [ceil(M / 256)]: trajectories without an acceptance per block of 256, then their offsets
  long long* btries = nullptr;              // [ceil(M / 256)]: tries per block
  int *n_fb = nullptr;                      // [T]: M' of every step (step T-1: 0)
  long long* n_tries = nullptr;             // [T]: tries of every step, summed over the trajectories
  int take(DevicePool& from, size_t N, size_t n_blocks, size_t M, size_t rows, size_t T) {
    pool = &from;
    int s = from.alloc(&cdf, N);
    if (s == RBPF_OK) s = from.alloc(&btot, n_blocks);
    if (s == RBPF_OK) s = from.alloc(&xs_c, M * rows);
    if (s == RBPF_OK) s = from.alloc(&u_c, M);
    if (s == RBPF_OK) s = from.alloc(&acc, M);
    if (s == RBPF_OK) s = from.alloc(&tries, M);
    if (s == RBPF_OK) s = from.alloc(&pos, M);
    if (s == RBPF_OK) s = from.alloc(&fb, M);
    if (s == RBPF_OK) s = from.alloc(&bcnt, (M + 255) / 256);
    if (s == RBPF_OK) s = from.alloc(&btries, (M + 255) / 256);
    if (s == RBPF_OK) s = from.alloc(&n_fb, T);
    if (s == RBPF_OK) s = from.alloc(&n_tries, T);
    if (s != RBPF_OK) release();
    return s;
  }
  void release() {
    if (pool)
      for (void* p : {(void*)cdf, (void*)btot, (void*)xs_c, (void*)u_c, (void*)acc, (void*)tries, (void*)pos, (void*)fb, (void*)bcnt, (void*)btries, (void*)n_fb, (void*)n_tries})
        pool->release(p);
    *this = RejectWorkspace();
  }
};

struct RejectWorkspaceGuard {
  RejectWorkspace& ws;
  explicit RejectWorkspaceGuard(RejectWorkspace& w) : ws(w) {}
  RejectWorkspaceGuard(const RejectWorkspaceGuard&) = delete;
  RejectWorkspaceGuard& operator=(const RejectWorkspaceGuard&) = delete;
  ~RejectWorkspaceGuard() { ws.release(); }
};

// An open backward-simulation pass over a generic map (rbpf_loc_generic_backward_begin .. _finish, rbpf_loc_generic_smooth.hip): the
// workspace is taken from rbpf_ctx::pool at begin and handed back at finish (or with the context).  An open MAP pass
// (rbpf_loc_generic_map_begin .. _finish) and an open marginal-smoothing pass (rbpf_loc_generic_marginal_begin .. _finish) are kept
// in the same form.
struct LocGenBackward {
  bool open = false;
  int M = 0, C = 0, nch = 0;
  int t = -1;                      // the step the next rbpf_loc_generic_backward_step_device processes; -1: all done
  LocGenLayout lay;
  BackwardWorkspace ws;
  // rbpf_loc_generic_backward_reject_begin: steps N_T-2 .. 0 try max_tries proposals per trajectory before the all-pairs pass
  bool reject = false;
  int max_tries = 0;
  unsigned long long seed = 0;
  RejectWorkspace rw;
};

// The device buffers of the running statistics' carry (rbpf_loc_forwardstats.hpp).  Persistent state of a localisation context
// (LocState::fs): taken from rbpf_ctx::pool at the first call, kept across calls and further steps of the filter, handed back by the
// reset entry points (and with the context).  The probes build one on a pool of their own.
//   Xhat [rows + 1][N]; pm, ps [marginal_part_count(N, M)] the norm pass's chunk partials; zero [M] zeros (logws_next of the norm
//   merge); D [M]; cj [M] (what the norm merge writes next to D, not read); part [nchunks][KF + 1][M]; tau [2][KF][max(N, M)] the
//   carry, ping-pong; reach [M]; pages [P][NR * NR + NR + 1].
struct ForwardCarry {
  DevicePool* pool = nullptr;
  bool alive = false;
  bool open = false;               // generic family: between _begin and _finish
  int folded = 0;                  // pairs of steps (t, t + 1), t = 0 .. folded - 1, are in the carry
  int cur = 0;                     // which half of tau holds the carry of step `folded`
  int nN = 0, rows = 0, n_res = 0;
  LocGenLayout lay;                // generic family
  double *Xhat = nullptr, *pm = nullptr, *ps = nullptr, *zero = nullptr, *D = nullptr, *cj = nullptr, *part = nullptr, *tau = nullptr,
         *reach = nullptr, *pages = nullptr;
  void release() {
    if (pool)
      for (void* p : {(void*)Xhat, (void*)pm, (void*)ps, (void*)zero, (void*)D, (void*)cj, (void*)part, (void*)tau, (void*)reach, (void*)pages})
        pool->release(p);
    *this = ForwardCarry();
  }
};

// The device buffers of the fixed-lag smoother's carry (rbpf_loc_fixedlag.hpp).  Persistent state of a localisation context
// (LocState::fl) with the life cycle of ForwardCarry; the probes build one on a pool of their own.
//   Xhat, pm, ps, zero, D, cj as in ForwardCarry; part [nchunks][K + 1][M]; T [2][K + H][max(N, M)] the carry, ping-pong: slot l of
//   a step in the rows l H .. (l + 1) H - 1; reach [M]; pages [P][K + H + 1]: est of every slot and the mass; cs [P][nN]: the filter
//   mean of every step entered.  K = lag H columns move on in a pass, H enter.
struct FixedLagCarry {
  DevicePool* pool = nullptr;
  bool alive = false;
  bool open = false;               // generic family: between _begin and _finish
  int entered = 0;                 // the steps 0 .. entered - 1 are in the carry and have their page
  int cur = 0;                     // which half of T holds the carry of step entered - 1
  int nN = 0, rows = 0, lag = 0, moments = 0, K = 0, H = 0;
  LocGenLayout lay;                // generic family
  double *Xhat = nullptr, *pm = nullptr, *ps = nullptr, *zero = nullptr, *D = nullptr, *cj = nullptr, *part = nullptr, *T = nullptr,
         *reach = nullptr, *pages = nullptr, *cs = nullptr;
  void release() {
    if (pool)
      for (void* p : {(void*)Xhat, (void*)pm, (void*)ps, (void*)zero, (void*)D, (void*)cj, (void*)part, (void*)T, (void*)reach, (void*)pages, (void*)cs})
        pool->release(p);
    *this = FixedLagCarry();
  }
};

struct LocState {
  DevicePool pool;                 // owns the device buffers below; the context-level arrays of a localisation session are in rbpf_ctx::pool
  int n = 0;
  int nN = 7;                      // width of the non-linear state: 7 (pos3 + quat4) in the dense-mag map, the model's in a generic one
  double sigma2 = 0.0;
  double *d_mean = nullptr, *d_V = nullptr, *d_vartab = nullptr, *d_S = nullptr, *d_lse = nullptr, *d_x0 = nullptr;
  int s_pages = 1, x0_cols = 1;
  // generic map (rbpf_loc_generic_create): the caller's handles produce states and Jacobians, the context is driven step by step
  bool generic = false;
  int d = 3;                       // n_y
  int ldx = 0;                     // row stride of the native dy layout
  int drawn_step = -1;             // step whose ancestors rbpf_loc_generic_ancestors_device has drawn
  double *d_R = nullptr;           // [n_y x n_y]
  double *d_H = nullptr;           // [N][n_y][ldx] rows packed from dy layout 0 (allocated on first use)
  LocGenBackward gb;               // backward simulation with a Gaussian transition density
  std::vector<int> reject_n_fb;    // [N_T] of the last finished rejection pass (rbpf_loc_generic_backward_reject_stats); empty: none
  std::vector<long long> reject_n_tries;
  LocGenBackward gv;               // the MAP trajectory with one (rbpf_loc_generic_map_begin .. _finish): t counts up, M = N_P; never open with gb
  LocGenBackward gm;               // marginal smoothing with one (rbpf_loc_generic_marginal_begin .. _finish): t counts down from N_T-2, M = N_P; never open with gb or gv
  LocGenBackward gp;               // two-slice statistics with one (rbpf_loc_generic_pair_stats_begin .. _finish): as gm; never open with gb, gv or gm
  ForwardCarry fs;                 // the running statistics' carry (rbpf_loc_forward_stats_*, rbpf_loc_generic_forward_stats_*); while fs.open: a fifth kind of open pass
  FixedLagCarry fl;                // the fixed-lag smoother's carry (rbpf_loc_fixed_lag_*, rbpf_loc_generic_fixed_lag_*); while fl.open: a sixth kind of open pass
  // landmark map (rbpf_loc_landmark_create): the handle's yhat is the prediction and the outputs observed at a step are selected
  bool landmark = false;
  int *d_ind = nullptr;            // [N_T][32]: the observed outputs of every step, ascending
  std::vector<int> n_obs;          // [N_T]: how many there are
  double *d_xl = nullptr;          // [N_P][ldx]: every row the map's mean, what a sparse-feature measModel takes as xl
};

// of rbpf_options a localisation context reads keep_history, trace and on_step only
int loc_validate_options(const rbpf_options* o);

// pieces of rbpf_loc_generic_create / rbpf_loc_generic_step_device that a landmark-map context shares (rbpf_loc_generic.hip)
int loc_generic_validate_run(int N_P, int N_T, int x0_cols, const rbpf_rng* rng, const rbpf_options* opt);
int loc_generic_build(int n_nonlin, int n_y, int n_lin, const double* mean, const double* V, const double* R, int N_P, int N_T,
                      const double* y, const double* x0_nonlin, int x0_cols, const rbpf_rng* rng, const rbpf_options* opt, rbpf_ctx** out);
int loc_generic_normalise_step(rbpf_ctx* c, const double* X_new);
int lg_ldx(int n);                                 // row stride of the native dy layout: rows start on 128-byte lines
int lg_validate_R(const double* R, int d);         // R [d x d] is positive definite (any d: the landmark map's goes up to 32)

}  // namespace rbpf
