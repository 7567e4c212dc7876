// Device-resident context shared by the filter and smoother host code.
#pragma once
#include "../../include/rbpf.h"
#include "rbpf_internal.hpp"
#include "rbpf_devmem.hpp"

#include <memory>
#include <string>
#include <utility>
#include <vector>

namespace rbpf {

void set_error(const std::string& s);
int hip_fail(hipError_t e, const char* what, const char* file, int line);

#define HIPCHK(expr)                                                          \
  do {                                                                        \
    hipError_t _e = (expr);                                                   \
    if (_e != hipSuccess) return ::rbpf::hip_fail(_e, #expr, __FILE__, __LINE__); \
  } while (0)
#define RB_TRY(x) do { int _s = (x); if (_s != RBPF_OK) return _s; } while (0)

inline bool have_device() {
  int n = 0;
  return hipGetDeviceCount(&n) == hipSuccess && n > 0;
}
// lower Cholesky factor of the leading n x n of A (column-major, leading dimensions lda / ldl); false: not positive definite
bool chol_lower_host(const double* A, int n, int lda, double* Lc, int ldl);

struct SmootherState;   // rbpf_smoother.hip
struct ShardState;      // rbpf_shard.hip
struct LocState;        // rbpf_loc.hip

// the handles of rbpf_particle_smoother_sparse_device (the generic sparse family's smoother) on their way into a context
struct SparseSmootherHandles {
  rbpf_sparse_dyn_fn dyn_model; rbpf_sparse_meas_fn meas_model; rbpf_sparse_dyn_res_norm_fn dyn_res_norm; void* user;
  int yhat_layout, dy_layout, max_future;
};

// extra capacity requested by the sharded filter
struct CreateExtras {
  size_t bank_extra = 0;   // particles appended to every bank (recv region of remote ancestors)
  size_t rng_slots = 0;    // slots per step in the replay buffers (global particle count); 0: N_P
};

// information-form per-step buffers handed to the step kernel
struct InfoStep {
  const double* ivec_old; size_t ivec_old_stride; double* ivec_new;
  const double* hld_old; size_t hld_old_stride; double* hld_new;
  double* qf_new; double* Hb_new;
};

}  // namespace rbpf

struct rbpf_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  rbpf::DevicePool pool;    // owns every device buffer below (Pt[1] / Pb[1] of a single-bank session alias bank 0)
  rbpf::ModelDev mdl;
  rbpf::Layout lay;
  rbpf::Layout lay_low;     // same HBM layout, 2 x 2 wave decomposition (lazy variants with >= 3 pending sets)
  rbpf_options opt;
  int N = 0, T = 0;
  bool smoother = false;
  int N_K = 1;
  int rng_mode = 0;
  unsigned long long seed = 0;
  int chol_pages = 1;
  int x0_lin_cols = 1;
  // constants
  int* d_NN = nullptr;
  double *d_y = nullptr, *d_odo = nullptr, *d_cholQ = nullptr, *d_cholQfull = nullptr;
  double *d_x0l = nullptr, *d_P0t = nullptr, *d_P0b = nullptr;
  double* d_R = nullptr;    // sparse-visual family: R [d x d]
  double *d_U = nullptr, *d_Z = nullptr;
  std::vector<double> h_x0n, h_P0, h_x0l, h_R, h_y, h_Ufin;
  // particle banks (ping-pong)
  double* Pt[2] = {nullptr, nullptr};
  double* Pb[2] = {nullptr, nullptr};
  double* F[2] = {nullptr, nullptr};
  double* xl[2] = {nullptr, nullptr};
  int cur = 0;              // bank holding the stored covariances
  int xcur = 0;             // bank holding the means (== cur unless the multi-step lazy update is on)
  // multi-step lazy update (filter fast path)
  int lazy_depth = 1;
  double* Fb[rbpf::kMaxSets + 1] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // factor-set banks
  int* fidx[2] = {nullptr, nullptr};   // [lazy_depth+1][N] entry tables, ping-pong
  int* base[2] = {nullptr, nullptr};   // [N] stored-matrix slot of every lineage, ping-pong
  int tcur = 0;
  // generic model family: host-evaluated states / Jacobians of the step about to run (consumed by ctx_step)
  double *d_xn_ext = nullptr, *d_H_ext = nullptr;
  const double *ext_xn = nullptr, *ext_H = nullptr;
  rbpf_callbacks cb = {nullptr, nullptr, nullptr, nullptr};   // the model's handles (copied at create; all null: caller-driven)
  bool has_cb = false;
  // generic family on the device: callbacks that take device pointers (rbpf_filter_set_device_callbacks), their dy layout,
  // and the buffers handed to them or to the caller -- ancestors' states and new states [nN x N] column-major, the staging
  // buffer of dy layouts 0 / 2 [N][d][n].  Allocated on first use.
  rbpf_callbacks dev_cb = {nullptr, nullptr, nullptr, nullptr};
  bool has_dev_cb = false;
  int dev_dy_layout = 0;
  double *d_xn_anc = nullptr, *d_xn_cm = nullptr, *d_dy_stage = nullptr;
  // generic sparse family (RBPF_MODEL_GENERIC_SPARSE): xl(:,ai) of the step about to run [N][ldx] and the step it was gathered
  // for, yhat of every step's maximum-weight particle [T][d]
  double *d_xl_g = nullptr, *d_yhattraj = nullptr;
  int gathered_step = -1;
  // ... in the smoother (rbpf_particle_smoother_sparse_device): the measModel callback, which rbpf_callbacks cannot carry (dyn_model
  // and dyn_res_norm are dev_cb's), the layouts of its results and the largest number of future times per call (0: automatic)
  rbpf_sparse_meas_fn sparse_meas = nullptr;
  void* sparse_user = nullptr;
  int sparse_yhat_layout = 2, sparse_dy_layout = 2, sparse_max_future = 0;
  std::vector<double> h_xn;      // generic family: states of the last step [nN x N] column-major (host evaluates dynModel)
  std::vector<double> h_xn_new, h_dy;   // scratch of the callbacks
  std::vector<int> h_ai;
  std::vector<double> h_odo, h_Q, h_dt;  // host copies for the callbacks' per-step arguments
  int q_pages = 1, dt_len = 1;
  bool cholQfull_ok = true;      // chol(dt*Q,'lower') of the full matrix exists (default additive dynResNorm needs it)
  int drawn_step = -1;           // step whose ordinary ancestors were already drawn by generic_draw_propagate
  bool fp32 = false;        // the covariance banks hold float (rbpf_options.storage = 1)
  bool inplace = false;     // single covariance bank, rewritten in place at every flush (rbpf_options.inplace)
  int* d_ip = nullptr;      // [8][N] in-place flush plan: destination entry, phase, scratch
  bool share_inplace = false;   // single bank + block-lower storage at eight / sixteen tile rows: the children of one parent store ONE flushed matrix (launch_share_inplace_plan)
  // shared flush (filter, ping-pong banks, symmetric storage at eight tile rows): one child per parent stores the flushed matrix
  bool share_flush = false;
  int* d_share = nullptr;                       // [3][N]: smallest child per parent, destination entry, phase (1 = writer)
  double* d_strip_ws = nullptr; size_t strip_ws_stride = 0;   // symmetric storage at sixteen tile rows: the step kernel's column strips ([N][stride])
  unsigned long long* d_share_writers = nullptr;   // writers of the timed shared flushes (device counter)
  long long share_flush_particles = 0;          // particles of the timed shared flushes (N per flush step)
  long long one_launch_flushes = 0;             // shared flush steps issued as one launch (rbpf_filter_one_launch_flushes)
  // timed launches: reads of stored matrices counted per particle (nominal) and per DISTINCT matrix (device counter)
  int* d_distinct_mark = nullptr; size_t distinct_keys = 0; unsigned long long* d_distinct_counter = nullptr;
  long long distinct_nominal = 0; int distinct_epoch = 0;
  // history
  int hist_slabs = 2;
  double* X = nullptr;      // [slabs][nN][N]
  int* A = nullptr;         // [T or 1][N]
  double *logw = nullptr, *w = nullptr, *wc = nullptr;
  double *traj_max = nullptr, *traj_mean = nullptr;
  double* d_scal = nullptr;
  int* d_flags = nullptr;   // [0] status bits, [1] clamped draws, [2] iw_max, [3] scratch, [4] flagged draws of the search, [5] strict recomputations (rbpf_filter_resample_fallbacks)
  int t = 0;
  int overflow_draws = 0;
  bool timing_on = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
  double sched_bytes = 0.0;  // bytes the timed launches had to move (rbpf_timing.scheduled_bytes_per_launch)
  rbpf::SmootherState* sm = nullptr;
  rbpf::ShardState* sh = nullptr;
  rbpf::LocState* loc = nullptr;   // localisation in a fixed map (rbpf_loc_*): the map and the per-step noise factors
  double* d_rs = nullptr;    // scratch of the multi-workgroup resample pipeline
  double* d_unext = nullptr; // [N] Philox resampling uniforms of the next step (written by propagate_kernel)
  int* d_pre_i = nullptr;   // [N][kPreInts]  per-workgroup descriptors of the step kernel
  double* d_pre_d = nullptr; // [N][kPreDoubles]
  int* d_order = nullptr;   // [N] processing order of the next step (ancestor-sorted)
  int* d_counts = nullptr;  // [2N] counting-sort scratch
  int ready_step = -1;      // step whose ancestors (and order) were already drawn by the fused resample kernel
  bool fuse_resample = false;
  bool sort_steps = false;  // smoothers: process every step in ancestor order too (the filter's fused resample kernel does it there)
  int order_step = -1;      // step d_order was computed for by ctx_step (smoothers)
  size_t bank_cap = 0;      // particles per bank incl. the recv region
  size_t rng_slots = 0;     // slots per step in d_U / d_Z
};

namespace rbpf {

int fill_model_dev(const rbpf_model* model, int nN, int n, int d, int nw, int nodo, const double* R, double jitter,
                   ModelDev& M, std::vector<int>& nn_axis_major);
int ctx_create(const rbpf_model* model, const rbpf_problem* prob, const rbpf_rng* rng, const rbpf_options* opt,
               bool smoother, int N_K, rbpf_ctx** out, const CreateExtras* ex = nullptr,
               const rbpf_callbacks* device_callbacks = nullptr, int dy_layout = 0,    // device_callbacks: rbpf_particle_smoother_device
               const SparseSmootherHandles* sparse_handles = nullptr);                 // rbpf_particle_smoother_sparse_device
int ctx_reset(rbpf_ctx* c);
void ctx_free(rbpf_ctx* c);
int ctx_step(rbpf_ctx* c, int k_iter, const double* xref_t, int n_draw, const InfoStep* info);
int ctx_check_flags(rbpf_ctx* c);
// generic family with callbacks (rbpf_model.callbacks): ordinary ancestors of the step about to run + dynModel on the
// host for slots [0, n_draw); then (generic_finish_inputs) the reference slot, measModel and the upload
int generic_draw_propagate(rbpf_ctx* c, int k_iter, int n_draw);
int generic_finish_inputs(rbpf_ctx* c, const double* xref_host);
// the same two halves with device callbacks (rbpf_particle_smoother_device): everything stays on the device, in stream order
int device_draw_propagate(rbpf_ctx* c, int k_iter, int n_draw);
int device_finish_inputs(rbpf_ctx* c, const double* xref_dev);
// generic sparse family: xl(:,ai) of the step about to run into d_xl_g, and the step itself on the caller's (or the callback's)
// yhat / dy (rbpf_filter_step_sparse_device; the smoother's states are already in the history slab: states_done)
int sparse_ext_gather_xl(rbpf_ctx* c);
int sparse_ext_ctx_step(rbpf_ctx* c, int k_iter, const double* xn_new_dev, bool states_done, const double* yhat_dev, int yhat_layout,
                        const double* dy_dev, int dy_layout);
// The context whose device callbacks are being called on this thread by a one-shot entry point (rbpf_particle_smoother_device),
// null otherwise: the callbacks have no other way to the stream they must enqueue on (rbpf_stream_get(NULL, ...)) and to the
// row stride of the native dy layout (rbpf_filter_external_layout(NULL, ...)).
rbpf_ctx* callback_context();
void set_callback_context(rbpf_ctx* c);
int ctx_call_on_step(rbpf_ctx* c, int t, bool is_smoother);
void ctx_account_launch(rbpf_ctx* c, const StepArgs& a);
int ctx_arm_distinct(rbpf_ctx* c, StepArgs& a, size_t keys);

// Schedule of the multi-step lazy update (lazy_depth = C; C = 1 is the plain schedule, one pending set rewritten every step): with
// t steps done the sets produced at steps t-ell .. t-1 are pending, set q in factor bank bank(q) of the C + 1; the step that finds
// C of them rewrites the stored matrices (`flush`), and every step leaves its own set in self_bank().
struct LazySched {
  int ell, first, B;
  bool flush;
  int bank(int q) const { return (first + q) % B; }
  int self_bank() const { return (first + ell) % B; }
};
// the sets pending FOR step t: what it applies
inline LazySched lazy_for_step(int lazy_depth, int t) {
  const int C = lazy_depth, ell = (t == 0) ? 0 : ((t - 1) % C) + 1;
  return {ell, t - ell, C + 1, t == 0 || ell == C};
}
// the sets pending AFTER the last finished step, c->t - 1: what unpacking or packing the state as it stands has to apply
inline LazySched lazy_after_last_step(const rbpf_ctx* c) { return lazy_for_step(c->lazy_depth, c->t); }
// ... and where they are: set q of particle j is entry fidx[q][j] of fset[q] (N: particles of this context's banks)
struct PendingSets { int n; const double* fset[kMaxSets]; const int* fidx[kMaxSets]; };
inline PendingSets ctx_pending_sets(const rbpf_ctx* c, int N) {
  const LazySched sc = lazy_after_last_step(c);
  PendingSets p{};
  p.n = sc.ell;
  for (int q = 0; q < sc.ell; ++q) { p.fset[q] = c->Fb[sc.bank(q)]; p.fidx[q] = c->fidx[c->tcur] + (size_t)sc.bank(q) * N; }
  return p;
}

// The shared flush (the children of one parent store ONE copy of their identical flushed matrix): the layouts whose step kernel
// has the writer / reader variants, and the steps that can use them.
bool layout_shares_flush(const Layout& L);
bool step_shares_flush(const StepArgs& a);

// What ctx_step (one GPU) and shard_step_impl (one rank of a sharded session) have in common.
struct StepBanks { int ob, nb, xo, xn, told, tnew; bool flush; };   // covariance / mean / index-table banks read (old) and written (new) by a step
// Everything of step t's StepArgs that does not depend on where the particles' states and ancestors live (N: local particles).
StepBanks ctx_step_args(rbpf_ctx* c, int t, int k_iter, const double* xref_t, const InfoStep* info, int N, StepArgs& a);
enum class FlushMode {
  Plain,            // one launch
  Shared,           // writers (phase 1), then their read-only siblings (phase 0)
  InPlace,          // single bank: phases 0, 1
  InPlaceShared     // single bank, shared: readers (phase 0), then phases 1 and 2
};
// The step launches after launch_propagate (timed when timing_on) and the commit of the banks and of t.
int ctx_launch_step(rbpf_ctx* c, StepArgs& a, const StepBanks& bk, FlushMode mode);
int ctx_unpack(rbpf_ctx* c, const int* d_index, int count, double* d_out);
void smoother_free(rbpf_ctx* c);
// in-library multi-device driver (rbpf_multi.hip): rbpf_options.n_devices
// rbpf_options.struct_size (ABI 9): a caller compiled against another layout is refused before any field is trusted
inline int options_ok(const rbpf_options* o) {
  if (!o || o->struct_size == 0 || o->struct_size == (int32_t)sizeof(rbpf_options)) return RBPF_OK;
  set_error("rbpf_options.struct_size = " + std::to_string(o->struct_size) + ", this library's rbpf_options has " + std::to_string(sizeof(rbpf_options)) +
            " bytes (ABI " + std::to_string(RBPF_ABI_VERSION) + "): rebuild the binding against include/rbpf.h");
  return RBPF_ERR_INVALID_ARG;
}
// the K rbpf_options.chol_refresh stands for (rbpf_chol_refresh_resolve; rbpf_smoother.hip)
int resolve_chol_refresh(int model_kind, int n, int d, int requested);
// is there a from-scratch factorisation kernel for the information form's n x n matrices with d pending rows kept in LDS?
// (rbpf_smoother.hip: the 64-column kernel while its LDS fits, else the 16-column kernel up to 64 row tiles)
bool info_chol_variant_fits(int n, int d);
// an explicit kernel choice (chol_variant) names the kernel of the from-scratch factorisation: with chol_refresh left at 0
// (automatic) it selects that factorisation at every step
inline int effective_chol_refresh(const rbpf_options& o) { return (o.chol_refresh == 0 && o.chol_variant != 0) ? 1 : o.chol_refresh; }
inline bool wants_multi(const rbpf_options* o) { return o && (o->n_devices > 1 || (o->n_devices == 1 && o->device_ids)); }
int multi_particle_filter(const rbpf_model* model, const rbpf_problem* prob, const rbpf_rng* rng, const rbpf_options* opt,
                          rbpf_filter_out* out);
int multi_particle_smoother(const rbpf_model* model, const rbpf_problem* prob, const rbpf_rng* rng, const rbpf_options* opt,
                            int32_t N_K, int32_t info_form, rbpf_smoother_out* out);
void shard_free(rbpf_ctx* c);
void loc_free(rbpf_ctx* c);

}  // namespace rbpf
