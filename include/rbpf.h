/*
 * rbpf.h -- C ABI of the MI355X-native Rao-Blackwellized particle filter / smoother.
 *
 * This is the drop-in boundary for the hot path of manonkok/Rao-Blackwellized-SLAM-smoothing.
 * The reference has no FFI layer of its own (it is pure MATLAB); the boundary *is* the three
 * MATLAB function signatures
 *     src/particleFilter.m:1-3, src/particleSmoother.m:1-2,
 *     src/particleSmootherInformationForm.m:1-2
 * and their callback contracts.  A MEX gateway (matlab/rbpf_mex.cpp) binds
 * exactly the entry points declared here; on machines without MATLAB the same ABI is driven by
 * the Python ctypes host mirror in rao-blackwellized-slam-smoothing_amd/.
 *
 * Conventions
 *   - All host matrices are MATLAB column-major fp64, caller-owned, never mutated.
 *   - Function handles cannot cross the boundary; the dynModel / measModel / dynResNorm closures
 *     of the example runners are described by an `rbpf_model` descriptor (family id + constants).
 *   - MATLAB's global RNG stream is replaced by an `rbpf_rng` block: replay buffers (seed-exact
 *     parity runs) or a (seed) pair for the device Philox4x32-10 generator (throughput runs).
 *   - Every function returns an rbpf_status; RBPF_OK == 0.  No global state; a context is bound
 *     to the HIP device that was current when it was created and owns one stream.
 *   - Particle / time indices in trace outputs are 0-based.
 */
#ifndef RBPF_H_
#define RBPF_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RBPF_ABI_VERSION 9   /* 9 (r05): rbpf_options starts with `struct_size` (checked by every entry point that takes options), lost
                              * `family_products` (r04's family GEMM was measured slower and removed), gained `info_rebuild`, and
                              * chol_refresh = 0 now means "automatic"; rbpf_probe_family_pht is gone, rbpf_chol_refresh_resolve is new */

typedef enum {
  RBPF_OK = 0,
  RBPF_ERR_INVALID_ARG = 1,
  RBPF_ERR_UNSUPPORTED = 2,     /* model family / option not implemented on the device path        */
  RBPF_ERR_HIP = 3,             /* a HIP runtime call failed (rbpf_last_error has the text)         */
  RBPF_ERR_NO_DEVICE = 4,       /* no gfx950 device visible: the product path has NO CPU fallback   */
  RBPF_ERR_OUT_OF_MEMORY = 5,
  RBPF_ERR_CHOL_FAILED = 6,     /* second Cholesky failure: MATLAB would throw                      *
                                 * (particleFilter.m:147, particleSmootherInformationForm.m:228-231) */
  RBPF_ERR_STATE = 7,           /* call sequence error (e.g. advance past N_T)                      */
  RBPF_ERR_CALLBACK = 8         /* a host callback (model handle / on_step hook) returned non-zero   */
} rbpf_status;

/* Model families = the closures defined in the reference's example runners. */
typedef enum {
  /* examples/slam-dense-mag/run_dense3D_magfield.m: dynModel :301-308, measModel :265-279,
   * dynResNorm :202-203.  nNonLin=7 (pos3+quat4), ny=3, nw=6, n_odo=7, nLin=m+3.             */
  RBPF_MODEL_DENSE_MAG_6D = 1,
  /* examples/slam-dense-radio/run_dense2D_withHeading.m: dynModel :75-76, dynResNorm :77,
   * measModel :168.  nNonLin=3 (x,y,heading), ny=1, nw=1, n_odo=3, nLin=m.                    */
  RBPF_MODEL_DENSE_RADIO_2DH = 2,
  /* examples/slam-sparse-visual: dynModel pfslam.m:81 (xn + dx' + sqrt(dt*Q)*randn, element-wise sqrt), measModel
   * pfslam.m:82 -> measurement.m:32-84 (1-D pinhole camera, point landmarks), dynResNorm = [] (psslam.m:119).
   * sparseFeatures = true: per-particle EKF linearisation, NaN in y = not observed (particleFilter.m:127-137,
   * 165-181).  nNonLin=3 (x,y,heading), ny = m_basis landmarks, nw=3, n_odo=3, nLin = 2*m_basis.              */
  RBPF_MODEL_SPARSE_VISUAL_2D = 3,
  /* Arbitrary dense model (any dynModel / measModel handles, sparseFeatures = false): the caller evaluates the handles
   * itself -- dynModel per particle (particleFilter.m:108), measModel on the whole batch (:124) -- and hands states and
   * Jacobians to rbpf_filter_step_external; everything else of the step (weights, normalisation, resampling, Kalman
   * update, ancestry) runs on the device.  The slow path behind unrecognised handles.
   * Measurement width: with host callbacks (rbpf_model.callbacks != NULL; the MEX gateway) n_y must be 1 or 3 -- a known
   * limit of the slow path.  Without them (callbacks == NULL: rbpf_filter_step_external, the device entry points
   * rbpf_filter_ancestors_device / rbpf_filter_step_device / rbpf_filter_set_device_callbacks, and
   * rbpf_particle_smoother_device) every n_y from 1 to 8 runs, on one GPU.  At n_y other than 1 and 3 the covariances are
   * fp64 full squares rewritten every step and the ancestor weights are factorised from scratch: storage != 0,
   * lazy_depth >= 2, inplace, chol_refresh > 1 and info_rebuild return RBPF_ERR_UNSUPPORTED before any device memory is
   * taken (chol_refresh = 0 resolves to 1), as does an nLin whose step-kernel LDS plan exceeds 160 KB (DESIGN.md has the
   * admitted nLin per n_y; n_y = 8: nLin <= 383 and 512..639, the filter also 1024..1117), and a smoother whose nLin x nLin
   * ancestor-weight factorisation has no kernel that fits (n_y = 7 at nLin >= 1024).                                  */
  RBPF_MODEL_GENERIC_DENSE = 4,
  /* Arbitrary model with sparseFeatures = true (particleFilter.m:127-137,165-181): [yhat, dy] = measModel(xn_i, xl_i) is
   * linearised per particle at the particle's own map and NaN in y marks an output that was not observed.  The caller's
   * device code evaluates both handles; the library hands it the resampled linear states and runs the EKF step
   * (rbpf_filter_sparse_gathered_device / rbpf_filter_step_sparse_device below).  The filter on one GPU only.
   * rbpf_model.callbacks must be NULL (RBPF_ERR_INVALID_ARG); m_basis, dim, NN, L, cam are not read.
   * Admitted: n_y 1 .. 32, n_lin 1 .. 96 (the border-only bank layout; the step kernel's LDS plan stays within 150 KB),
   * n_nonlin and n_w <= 8.  Anything larger, storage != 0, lazy_depth >= 2, inplace, n_devices and the smoothers return
   * RBPF_ERR_UNSUPPORTED with a message that names the rule, before any device memory is taken.                           */
  RBPF_MODEL_GENERIC_SPARSE = 5
} rbpf_model_kind;

/* Host callbacks of the generic family = the reference's handle contracts, batched over columns so that a binding
 * makes one call per step (the MEX gateway: one mexCallMATLAB each).  All matrices column-major.
 * A non-zero return aborts the run with RBPF_ERR_CALLBACK.
 *   dyn_model    xn_new(:,j) = dynModel(xn_anc(:,j), odometry(t,:), dt(t), Q(:,:,t)) for j = 0..n_cols-1, in this order
 *                (the handle draws its own random numbers: particleFilter.m:108, particleSmoother.m:134-136); t is the
 *                0-based row of odometry (= MATLAB's t-1)
 *   meas_model   dy = measModel(xn [n_nonlin x n_cols]) -> [n_cols x n_y x n_lin] ([n_cols x n_lin] memory for
 *                n_y = 1), particleFilter.m:124, particleSmoother.m:120
 *   dyn_res_norm e_dyn(:,j) = dynResNorm(xnk_t, xn(:,j), odometry(t,:), dt(t), Q(:,:,t))' [n_w x n_cols]
 *                (particleSmoother.m:178-180); NULL = isempty(dynResNorm): the additive default (:175-177) on the device */
typedef struct {
  int (*dyn_model)(void* user, int32_t t, int32_t n_cols, const double* xn_anc, double* xn_new);
  int (*meas_model)(void* user, int32_t n_cols, const double* xn, double* dy);
  int (*dyn_res_norm)(void* user, int32_t t, int32_t n_cols, const double* xnk_t, const double* xn, double* e_dyn);
  void* user;
} rbpf_callbacks;

typedef struct {
  int32_t kind;          /* rbpf_model_kind                                                     */
  int32_t m_basis;       /* number of basis functions m (tools/domain_cartesian_dx.m:43)        */
  int32_t dim;           /* input dimension of the basis (3 for dense-mag, 2 for dense-radio)   */
  int32_t use_dyn_res_norm; /* 1: model's dynResNorm handle; 0: additive default                *
                             * (particleSmoother.m:175-177, isempty(dynResNorm))                */
  const int32_t* NN;     /* [m x dim] column-major index table NN (domain_cartesian_dx.m:36-43); NULL for   *
                          * RBPF_MODEL_SPARSE_VISUAL_2D                                                       */
  double L[3];           /* domain half-widths (domain_cartesian_dx.m:27-29)                    */
  double cam[3];         /* RBPF_MODEL_SPARSE_VISUAL_2D: f, fp, fw (load_data.m:58-60)          */
  const rbpf_callbacks* callbacks; /* RBPF_MODEL_GENERIC_DENSE: the handles (one-shot entry points and            *
                                    * rbpf_filter_advance call them every step); NULL: the caller drives the       *
                                    * filter itself with rbpf_filter_ancestors / rbpf_filter_step_external          */
} rbpf_model;

typedef struct {
  int32_t N_P;           /* particles                                                           */
  int32_t N_T;           /* time steps = size(y,1)                                              */
  int32_t n_nonlin;      /* size(x0_nonLin,1)                                                   */
  int32_t n_lin;         /* size(x0_lin,1)                                                      */
  int32_t n_y;           /* size(y,2)                                                           */
  int32_t n_w;           /* size(Q,1)                                                           */
  int32_t n_odo;         /* size(odometry,2)                                                    */
  int32_t x0_lin_cols;   /* 1 or N_P          (particleFilter.m:60-64)                          */
  int32_t q_pages;       /* size(Q,3): 1 or >= N_T-1   (particleFilter.m:75-77)                 */
  int32_t dt_len;        /* 1 or >= N_T-1              (particleFilter.m:80-82)                 */
  const double* odometry;/* [>=N_T-1 x n_odo], leading dimension odo_ld                         */
  int32_t odo_ld;
  const double* y;       /* [N_T x n_y]                                                         */
  const double* x0_nonlin;/* [n_nonlin]                                                         */
  const double* x0_lin;  /* [n_lin x x0_lin_cols]                                               */
  const double* P0_lin;  /* [n_lin x n_lin]                                                     */
  const double* Q;       /* [n_w x n_w x q_pages]                                               */
  const double* R;       /* [n_y x n_y]                                                         */
  const double* dt;      /* [dt_len]                                                            */
} rbpf_problem;

typedef enum { RBPF_RNG_REPLAY = 0, RBPF_RNG_PHILOX = 1 } rbpf_rng_mode;

typedef struct {
  int32_t mode;          /* rbpf_rng_mode                                                       */
  int32_t n_iter;        /* pages available in the replay buffers (1 for the filter, N_K)       */
  /* Replay buffers (RBPF_RNG_REPLAY), drawn by the caller in the reference's call order:
   *   U [N_P x (N_T-1) x n_iter]      the `rand` of tools/sample.m:31 for slot i at step t
   *                                   (for smoother iterations k>1 slot N_P-1 holds the single
   *                                   rand of particleSmoother.m:241)
   *   Z [n_w x N_P x (N_T-1) x n_iter] the randn's consumed by dynModel for slot i at step t
   *   Ufin [n_iter]                   the rand of `ak = sample(w)` (particleSmoother.m:346)    */
  const double* U;
  const double* Z;
  const double* Ufin;
  uint64_t seed;         /* RBPF_RNG_PHILOX: key of the counter-based device generator          */
} rbpf_rng;

typedef struct rbpf_ctx rbpf_ctx;      /* opaque filter / smoother context (device-resident state) */

/* Per-step hook = the reference's makePlots call sites: after every time step of the filter
 * (src/particleFilter.m:215-217: makePlots(xn,xl_max,P_max,traj_max,yhattraj,xn_traj,traj_mean,xl,P)) and after every
 * iteration of the smoothers (src/particleSmoother.m:360-362: makePlots(xnk,xlk,k,XNK,XLK,PK)).  Filter: `ctx` is
 * valid inside the callback for rbpf_filter_finish(ctx, &partial), which returns any of the outputs / final_* banks
 * as of step t.  Smoothers: iteration k's pages of the caller's XNK / XLK / PK buffers are complete when it runs.
 * A non-zero return aborts with RBPF_ERR_CALLBACK.                                                                */
typedef struct {
  rbpf_ctx* ctx;         /* filter only (NULL for the smoothers)                                */
  int32_t t;             /* filter: 0-based time step just finished; smoother: 0-based iteration */
  int32_t is_smoother;
} rbpf_view;
typedef int (*rbpf_on_step_fn)(const rbpf_view* view, void* user);

typedef struct {
  int32_t struct_size;   /* = sizeof(rbpf_options) of the caller's build (rbpf_abi_sizeof(3) at run time): an entry  *
                          * point handed options of another size returns RBPF_ERR_INVALID_ARG instead of reading past the caller's     *
                          * struct.  0 is accepted from callers that zero the struct and fill fields by name (C designated             *
                          * initialisers) -- they were compiled against this header by construction                                    */
  int32_t keep_history;  /* 1: keep xn history + ancestor table (needed for traj_sample_iwmax,  *
                          *    xn_traj and every smoother); 0: ping-pong only                   */
  int32_t trace;         /* 1: record per-step logw / w / ancestor indices (tests)              */
  int32_t fix_p_mean;    /* 0: reproduce quirk Q3 (particleFilter.m:228-230 overwrites P_mean);  *
                          * 1: accumulate it over the particles (the evident intent)            */
  int32_t lazy_depth;    /* filter and information-form smoother: C >= 2 keeps up to C pending rank-n_y downdates on the    *
                          * fly and rewrites the stored covariances every C-th step only (C-1 read-only steps in         *
                          * between); 0/1: rewrite every step.  Results agree to rounding (same algebra).  max 4 (filter; *
                          * 8 on symmetric storage, storage = 2) / 3 (information form, also in the sharded smoother); ignored  *
                          * by the covariance-form smoother                                                                  */
  double jitter;         /* <=0: reference default (1e-3 filter :89, 1e-2 smoothers :70)        */
  int32_t inplace;       /* filter (and, on request only, the information-form smoother) with lazy_depth >= 2: keep ONE covariance bank and rewrite it in place at    *
                          * every flush (the first child of a stored matrix overwrites it after its siblings    *
                          * were written to dead slots) instead of ping-pong banks -- halves the memory, same    *
                          * results bit for bit.  0: automatic (when two banks do not fit the device), 1: on,    *
                          * -1: off.  On block-lower storage (eight / sixteen tile rows; elsewhere the per-child  *
                          * in-place flush) the single bank keeps                                                *
                          * the shared flush: one writer per parent with children, the first writer of a stored  *
                          * matrix overwrites it in place after its readers (results to rounding, as two banks). */
  int32_t storage;       /* 0 = the covariance banks hold fp64 (the reference's precision); 1 = fp32 STORAGE of the banks, for the  *
                          * filter of a dense model with n_y = 3 (dense-mag, also sharded, or a generic model;       *
                          * BASELINE.json configs[4]): half the HBM traffic and memory, all                          *
                          * arithmetic and every other state stay fp64.  Results then agree with the fp64 run to     *
                          * ~1e-6 relative per step (not to 1e-9) and resampling indices may differ.                 *
                          * 2 = fp64, SYMMETRIC storage: particleFilter.m:198 keeps P_i symmetric up to rounding, so only the   *
                          * lower block triangle (64 x 64 tiles) + the border rows are kept -- 0.5625 n^2 elements at nLin =   *
                          * 515, i.e. 0.56 x the HBM traffic and memory of storage 0; read-only steps of lazy_depth apply the  *
                          * pending sets as P H' - KS (K' H') instead of element-wise.  Same algebra: results within 1e-9 of  *
                          * storage 0 (P(r,c) and P(c,r), which differ by rounding in the reference's plain form, are one     *
                          * stored value).  Dense models with n_y = 3 and 256 <= n_lin <= 1151 (4 to 16 tile rows of 64, the     *
                          * core rows 64 * floor(n_lin / 128) * 2): the filter, single-GPU and sharded, lazy_depth <= 4 off     *
                          * eight tile rows; both smoothers at 256 <= n_lin <= 767 (single-GPU; sharded at 256..383 and          *
                          * 512..639 only); the smoothers are refused from n_lin = 768 on.  n_y = 1                               *
                          * with n_lin = 128 (dense-radio; two tile rows: 0.75 x the bytes): filter and both smoothers.  The     *
                          * generic (host-callback) family takes the same sizes as the built-in ones.  RBPF_ERR_UNSUPPORTED      *
                          * elsewhere.                                                                                          *
                          * 3 = fp32 tiles of the lower block triangle (storage 1's rounding on storage 2's layout: 0.28 x the   *
                          * bytes of storage 0): the filter with n_y = 3 and 384 <= n_lin <= 1151 (not at four tile rows),      *
                          * lazy_depth <= 4.                                                                                    */
  int32_t chol_variant;  /* smoothers: kernel of the ancestor-weight factorisation (particleSmoother.m:221,                   *
                          * particleSmootherInformationForm.m:228).  0: by matrix size (default); 16 / 64 / 648 / 644 / 1 /             *
                          * (a non-zero value with chol_refresh = 0 selects the from-scratch factorisation, chol_refresh = 1)           *
                          * 10-14 as the `variant` of rbpf_chol_weights.  Same arithmetic, results to rounding (tests).                */
  int32_t chol_refresh;  /* information-form smoother, the ancestor-weight factorisation chol(Imat_i + ImatAddt) of                    *
                          * particleSmootherInformationForm.m:224-236.                                                                 *
                          * K > 1: CARRY the factor along every lineage -- per step n_y rank-1 updates (the particle's own           *
                          * H' R^-1 H, :334) and n_y rank-1 downdates (the reference trajectory's term leaving ImatAddt, :194-201)    *
                          * of the ancestor's factor, O(n^2) instead of n^3 / 3, the forward solve carried as an augmented row --     *
                          * and refactorise every K-th step from Imat rebuilt along the state history (recognised families; the       *
                          * information matrices are then only materialised at those steps).  Same algebra, different arithmetic:     *
                          * every ancestor index and trajectory draw identical, ancestor probabilities within 2e-9 absolute, outputs *
                          * within 1e-9 of the from-scratch factorisation (measured 8.8e-10 over T = 3000 at nLin = 515;             *
                          * tests/test_gpu_chol_carry.py, test_gpu_r05_parity.py).  nLin <= 575, n_y = 1 or 3; also in *
                          * the sharded smoother (rbpf_shard_smoother_refresh_*).  K >= N_T - 1 never refactorises after the first    *
                          * step: no information matrix is stored (or, sharded, exchanged) at all -- see info_rebuild; 256 < K <       *
                          * N_T - 1 (single device only) rebuilds the matrices from the origin at every refresh likewise, since a        *
                          * window that long would need N_P x K x n_y x n_lin doubles of Jacobians.                                      *
                          * 1: factorise from scratch at every step, the reference's own arithmetic.                                  *
                          * 0 (default): AUTOMATIC = 32 where the carried factors apply and pay (recognised dense family, 128 <=      *
                          * nLin <= 575), 1 elsewhere; rbpf_chol_refresh_resolve tells which.                                        *
                          * Failure behaviour of K > 1: the reference's retry of a failed chol (:228-231) is unusable as written      *
                          * (quirk Q4), so a failed factorisation is an error either way; a carried DOWNDATE that loses definiteness  *
                          * sets status bit 2, the particle's ancestor log-weight becomes NaN and the run ends with                    *
                          * RBPF_ERR_CHOL_FAILED when the iteration's flags are checked.  Use chol_refresh = 1 where near-singular     *
                          * Imat + ImatAddt are expected.                                                                              */
  int32_t exchange_capacity; /* sharded sessions: particle records one rank can send / receive per time step (buffers are  *
                          * sized from it, identically on every rank; received records persist for lazy_depth steps).       *
                          * > 0: a hard limit -- a step that needs more fails on EVERY rank with RBPF_ERR_OUT_OF_MEMORY before   *
                          * any collective is issued (the plan is replicated).  0: start at min(N_local, max(256, N_local /    *
                          * 16)) and GROW on demand: every rank reaches the same verdict from the replicated plan and enlarges *
                          * its buffers by the same rule without communicating (rbpf_shard_views_get then returns the new      *
                          * pointers / capacities; received records of the running lazy cycle are kept).  < 0: start at        *
                          * |exchange_capacity| and grow likewise.                                                              */
  rbpf_on_step_fn on_step; /* NULL: no hook                                                       */
  void* on_step_user;
  int32_t n_devices;     /* rbpf_particle_filter / rbpf_particle_smoother(info_form = 1) only.  0 / 1 with device_ids == NULL: one  *
                          * GPU (the current device).  W > 1: the N_P particles are sharded over W GPUs of this node INSIDE the   *
                          * library -- one host thread per device runs the sharded step loop (rbpf_shard_* below) and the library  *
                          * issues the collectives itself over RCCL (ncclCommInitAll; all-gather of the forward bank + grouped     *
                          * send / recv of the migrating particle records, on each context's stream), so a single host process   *
                          * (a MATLAB session behind the MEX gateway: particleSmootherInformationForm.m is one call) reaches all  *
                          * GPUs.  N_P must be a multiple of W; recognised dense model families; results equal the single-GPU run *
                          * (bit for bit without lazy_depth, 1e-9 with it), every reference output incl. xn_traj; no traces / final banks. */
  const int32_t* device_ids; /* [n_devices] HIP device of every rank, NULL = 0 .. n_devices-1.  A device named more than once makes *
                          * its ranks share that GPU over a host-staged transport (no RCCL) -- how a one-GPU machine exercises the  *
                          * multi-rank loop; n_devices = 1 with device_ids set runs the loop with a world of one.                  */
  int32_t info_rebuild;  /* information-form smoother with carried factors (chol_refresh = K > 1), single device: 0 = the information    *
                          * matrices are materialised at every refresh (two banks of N_P matrices; a refresh walks back K generations).   *
                          * 1 = NONE is stored: every refresh rebuilds them from the initial matrix along the WHOLE ancestral path --    *
                          * Imat_i = Imat0 + sum of H' R^-1 H over the path, :334's terms in another order of summation -- chunk by chunk  *
                          * (4096 particles x 32 generations at a time).  2.3 MB per particle less at nLin = 515: with inplace = 1 the     *
                          * state is 3.6 MB per particle and the metric's N_P = 65 536 fits one 288 GB GPU.  The cost of a refresh grows   *
                          * with t: choose K in the hundreds (K >= N_T - 1 never refreshes and implies this mode).  Same tolerance as      *
                          * chol_refresh (tests/test_gpu_chol_carry.py, test_gpu_r05_parity.py).                                          */
} rbpf_options;

/* Outputs of particleFilter (src/particleFilter.m:1,26-34).  NULL pointers are skipped. */
typedef struct {
  double* traj_max;          /* [n_nonlin x N_T]                                                */
  double* traj_mean;         /* [n_nonlin x N_T]                                                */
  double* xl_max;            /* [n_lin]                                                         */
  double* xl_mean;           /* [n_lin]                                                         */
  double* P_max;             /* [n_lin x n_lin]                                                 */
  double* P_mean;            /* [n_lin x n_lin]                                                 */
  double* traj_sample_iwmax; /* [n_nonlin x N_T]   (needs keep_history)                         */
  double* xn_traj;           /* [n_nonlin x N_P x N_T] (needs keep_history)                     */
  /* extras (not reference outputs; used by the parity tests) */
  double* trace_logw;        /* [N_P x N_T]        (needs trace)                                */
  double* trace_w;           /* [N_P x N_T]        (needs trace)                                */
  int32_t* trace_ai;         /* [N_P x N_T] 0-based, column 0 unused (needs trace)              */
  double* final_xn;          /* [n_nonlin x N_P]                                                */
  double* final_xl;          /* [n_lin x N_P]                                                   */
  double* final_P;           /* [n_lin x n_lin x N_P]                                           */
  int32_t* iw_max;           /* [1] 0-based index of the maximum-weight particle at t = N_T     */
} rbpf_filter_out;

/* Outputs of particleSmoother / particleSmootherInformationForm (particleSmoother.m:1,27-30). */
typedef struct {
  double* XNK;               /* [n_nonlin x N_T x N_K]                                          */
  double* XLK;               /* [n_lin x N_K]                                                   */
  double* PK;                /* [n_lin x n_lin x N_K]                                           */
  /* extras for the parity tests (need trace) */
  double* trace_logw;        /* [N_P x N_T x N_K]                                               */
  double* trace_w;           /* [N_P x N_T x N_K]                                               */
  int32_t* trace_ai;         /* [N_P x N_T x N_K] 0-based                                       */
  double* trace_paNt;        /* [N_P x N_T x N_K] ancestor probabilities AI(:,t) (:240)         */
  int32_t* trace_ak;         /* [N_K] 0-based                                                   */
} rbpf_smoother_out;

/* Timing of the dominant kernel (the fused resample-gather + weight + Kalman-update stream kernel),
 * measured with HIP events on the context's own stream.                                           */
typedef struct {
  double stream_kernel_ms;   /* sum of launch durations since the last reset                     */
  int64_t stream_kernel_launches;
  double algorithmic_bytes_per_launch; /* N_P * (2 n^2 + 2 n + 2 nNonLin) * 8         */
  double scheduled_bytes_per_launch;   /* mean over the timed launches of the bytes this run's schedule has to move:      *
                                        * per particle one read of the stored covariance, one write of it only when the  *
                                        * launch rewrites it (every lazy_depth-th step), the pending rank-n_y factor sets *
                                        * it applies (2 n n_y each) and writes (one), the mean and the non-linear state   *
                                        * in and out.  <= algorithmic; the roofline fraction is quoted on this figure     */
} rbpf_timing;

/* ---- library ---------------------------------------------------------------------------------- */
int rbpf_abi_version(void);
/* sizeof of the library's own view of an interface struct -- a binding in another language (ctypes, MEX, a MATLAB loadlibrary
 * prototype file) compares its mirror against it once at load time.  which: 0 rbpf_model, 1 rbpf_problem, 2 rbpf_rng, 3 rbpf_options,
 * 4 rbpf_filter_out, 5 rbpf_smoother_out, 6 rbpf_timing, 7 rbpf_callbacks, 8 rbpf_view, 9 rbpf_loc_map, 10 rbpf_loc_problem,
 * 11 rbpf_loc_out; -1 for any other value.                                                                                  */
int rbpf_abi_sizeof(int32_t which);
const char* rbpf_status_string(int status);
/* Thread-local text of the last error raised on this thread (HIP error string, argument name). */
const char* rbpf_last_error(void);
/* Number of visible gfx950 devices (0 when none; never touches a device).                        */
int rbpf_device_count(void);
/* Bytes of device memory this process's sessions and calls own right now: back to its earlier value once they are destroyed /
 * have returned, successfully or not (a leak check that does not depend on what else runs on the device).                   */
int64_t rbpf_device_bytes_live(void);

/* ---- one-shot entry points: what the MEX gateway binds ----------------------------------------- */
/* Replaces src/particleFilter.m:1-3 for the recognised model families (dense branch).             */
int rbpf_particle_filter(const rbpf_model* model, const rbpf_problem* prob, const rbpf_rng* rng,
                         const rbpf_options* opt, rbpf_filter_out* out);
/* Replaces src/particleSmoother.m:1-2 (info_form = 0) and
 * src/particleSmootherInformationForm.m:1-2 (info_form = 1).                                      */
int rbpf_particle_smoother(const rbpf_model* model, const rbpf_problem* prob, const rbpf_rng* rng,
                           const rbpf_options* opt, int32_t N_K, int32_t info_form,
                           rbpf_smoother_out* out);

/* Both smoothers for a generic model whose handles are device code (an addition to ABI 9: no struct changed).  model->kind is
 * RBPF_MODEL_GENERIC_DENSE and model->callbacks NULL; device_callbacks are called in the reference's order with DEVICE pointers,
 * valid in stream order on the context's stream (the callbacks enqueue there, or synchronise themselves):
 *   dyn_model(user, t, n_cols, xn_anc, xn_new)   once per step t >= 1: n_cols = N_P in iteration 0, N_P - 1 (the ordinary slots,
 *                in slot order, particleSmoother.m:132-137) afterwards; both [n_nonlin x n_cols] column-major
 *   dyn_res_norm(user, t, N_P, xnk_t, xn, e_dyn)  iterations k >= 1, steps t >= 1: xn [n_nonlin x N_P] the states of generation
 *                t - 1, e_dyn [n_w x N_P] column-major; NULL: the additive default on the device (needs n_w == n_nonlin)
 *   meas_model(user, n_cols, xn, dy)              n_cols = N_P once per step; N_T once per iteration k >= 1 (the reference
 *                trajectory, :120); with carried factors (chol_refresh > 1) any number of columns at a refresh, where the
 *                information matrices are rebuilt from the state history through it -- so it must be a pure function of xn.
 *                dy in dy_layout (rbpf_filter_step_device) for n_cols rows; layout 1: rows on the stride ldx >= n_lin, the
 *                per-step call writes the step kernels' own buffer, every other call a staging buffer.
 * Between two steps of an iteration no state, Jacobian or residual crosses to the host and the library adds no host
 * synchronisation to those of the built-in families' smoother.  With device callbacks chol_refresh > 1 never stores or copies a
 * per-particle information matrix between refreshes, and info_rebuild = 1, chol_refresh >= N_T - 1 and inplace = 1 are
 * available as for the built-in families (chol_refresh = 0 still resolves to 1 for a generic model).  One GPU:
 * rbpf_options.n_devices is RBPF_ERR_UNSUPPORTED.  n_y from 1 to 8; at n_y other than 1 and 3 both forms run with the
 * from-scratch factorisation only (chol_refresh <= 1) on fp64 full squares: see RBPF_MODEL_GENERIC_DENSE.                 */
int rbpf_particle_smoother_device(const rbpf_model* model, const rbpf_problem* prob, const rbpf_rng* rng,
                                  const rbpf_options* opt, int32_t N_K, int32_t info_form,
                                  const rbpf_callbacks* device_callbacks, int32_t dy_layout, rbpf_smoother_out* out);

/* The covariance-form smoother's sparseFeatures branch (src/particleSmoother.m:194-217,267-277,306-321) for an ARBITRARY model whose
 * handles are device code (an addition to ABI 9: no struct changed).  model->kind is RBPF_MODEL_GENERIC_SPARSE and
 * model->callbacks NULL; rbpf_callbacks.meas_model cannot carry xl and yhat, so the three callbacks and `user` are plain arguments.
 * They are called in the reference's order with DEVICE pointers, valid in stream order on the context's stream
 * (rbpf_stream_get(NULL, ...) inside a callback; the callbacks enqueue there, or synchronise themselves):
 *   dyn_model(user, t, n_cols, xn_anc, xn_new)    as for rbpf_particle_smoother_device: once per step t >= 1, n_cols = N_P in
 *                iteration 0, N_P - 1 (the ordinary slots, in slot order, :132-137) afterwards
 *   dyn_res_norm(user, t, N_P, xnk_t, xn, e_dyn)  as for rbpf_particle_smoother_device; NULL: the additive default on the device
 *                (:175-177, needs n_w == n_nonlin)
 *   meas_model(user, n_cols, xn, xl, ldx, yhat, dy)  [yhat, dy] = measModel(xn, xl) for n_cols columns: xn [n_nonlin x n_cols]
 *                column-major, xl [n_cols][ldx] (row c: the map column c is linearised at; columns n_lin..ldx-1 zero), results
 *                into yhat / dy, library buffers for n_cols columns in yhat_layout / dy_layout.  It must be a PURE function of
 *                its arguments and accept any n_cols:
 *                  n_cols = N_P once per step: xl the maps after the resampling gather, the reference slot's sampled map
 *                      included (:243), as rbpf_filter_sparse_gathered_device hands them to the filter's caller;
 *                  n_cols = F N_P at the steps t >= 1 of the iterations k >= 1, for the ancestor weights (:194-217): a chunk of F
 *                      future times ti_f of t .. N_T-1; column f N_P + i carries xn = xnk(:,ti_f) and xl = xl(:,i) of generation
 *                      t - 1 -- the map BEFORE the resampling gather, the one :206 linearises at -- both materialised in device
 *                      memory by the library.  Times without an observed output are skipped (the handle is pure: the
 *                      reference's call for them has no effect).
 *                Rows of yhat / dy that belong to outputs not observed at that time are never read.  dy is dense.
 *   yhat_layout / dy_layout  as in rbpf_filter_step_sparse_device with N_P replaced by n_cols: yhat 0 (MATLAB order, yhat(c,k) at
 *                c + n_cols k) or 2 (C-contiguous); dy 0 (MATLAB order, dy(c,k,q) at c + n_cols (k + n_y q)), 2 (C-contiguous) or
 *                1 (rows on the stride ldx, [n_cols][n_y][ldx]).
 *   max_future_per_call  the largest F; 0: chosen so that the chunk's staging buffers (dy: F N_P n_y n_lin doubles, and the
 *                replicated xl) stay within 256 MB.
 * Per particle the stacked future observations give D [M x n_lin] (time-major, outputs ascending within a time), e = y - yhat
 * and S = D P D' + blkdiag(R(ind,ind)) (:207-215), formed on the fp64 matrix cores (rbpf_sparse_ext_anc.hip), then the batched
 * Cholesky with the one jitter retry (:221-229; jitter 1e-2, :70).  The step itself is rbpf_filter_step_sparse_device's.  Between two
 * steps nothing crosses to the host and the library adds no host synchronisation to those of the built-in sparse smoother.
 * Refused before anything touches a device: NULL arguments (dyn_res_norm and user may be NULL), N_K < 1, unknown layouts, a model
 * of another kind or with callbacks (RBPF_ERR_INVALID_ARG); rbpf_options.n_devices, storage other than 0, lazy_depth >= 2,
 * inplace, n_y > 32, n_lin > 96, more than 1023 stacked future observations at step 1 (RBPF_ERR_UNSUPPORTED).  The largest
 * workspace is S, N_P M^2 doubles with M the observations after step 0.  Not available: the information form (the reference
 * returns nothing for sparseFeatures, particleSmootherInformationForm.m:77-80), host closures, sharding, the MEX gateway.   */
typedef int (*rbpf_sparse_dyn_fn)(void* user, int32_t t, int32_t n_cols, const double* xn_anc, double* xn_new);
typedef int (*rbpf_sparse_meas_fn)(void* user, int32_t n_cols, const double* xn, const double* xl, int32_t ldx, double* yhat, double* dy);
typedef int (*rbpf_sparse_dyn_res_norm_fn)(void* user, int32_t t, int32_t n_cols, const double* xnk_t, const double* xn, double* e_dyn);
int rbpf_particle_smoother_sparse_device(const rbpf_model* model, const rbpf_problem* prob, const rbpf_rng* rng,
                                         const rbpf_options* opt, int32_t N_K, rbpf_sparse_dyn_fn dyn_model,
                                         rbpf_sparse_meas_fn meas_model, rbpf_sparse_dyn_res_norm_fn dyn_res_norm, void* user,
                                         int32_t yhat_layout, int32_t dy_layout, int32_t max_future_per_call,
                                         rbpf_smoother_out* out);
/* Per-step timing of that smoother's ancestor weights, for tools/sparse_device_smoother_bench.py: enable = 1 makes every later
 * call in this process put HIP events around the build kernel and around the batched factorisation of every step with future
 * observations (read once per iteration, where the library waits for the stream anyway); 0 switches it off.  The non-NULL outputs
 * receive the totals accumulated since the last call -- milliseconds in the build kernel, in the factorisation, and the number of
 * timed steps -- and the totals are reset.  Never touches a device.                                                       */
int rbpf_sparse_smoother_timing(int32_t enable, double* build_ms, double* chol_ms, int64_t* steps);

/* ---- resident-state API (what bench.py times: inputs already in HBM) --------------------------- */
/* Uploads model, problem and RNG block to the current device and allocates the particle banks.    */
int rbpf_filter_create(const rbpf_model* model, const rbpf_problem* prob, const rbpf_rng* rng,
                       const rbpf_options* opt, rbpf_ctx** ctx);
/* Bytes of device memory a context for this problem needs (no device access).                     */
int rbpf_filter_workspace_bytes(const rbpf_model* model, const rbpf_problem* prob,
                                const rbpf_options* opt, size_t* bytes);
/* Enqueue `n_steps` time steps (particleFilter.m:100-218) on the context stream; asynchronous.    */
int rbpf_filter_advance(rbpf_ctx* ctx, int32_t n_steps);
/* Rewind to t = 0 (re-initialises weights / states: particleFilter.m:52-67); asynchronous.        */
int rbpf_filter_reset(rbpf_ctx* ctx);
/* Block until the stream is idle; reports a deferred RBPF_ERR_CHOL_FAILED.                        */
int rbpf_sync(rbpf_ctx* ctx);
/* Final extraction (particleFilter.m:220-233) + download of the requested outputs.                */
int rbpf_filter_finish(rbpf_ctx* ctx, rbpf_filter_out* out);
/* Current step index (number of steps processed).                                                 */
int rbpf_filter_tell(const rbpf_ctx* ctx, int32_t* t);
/* The covariance-bank schedule the context chose (rbpf_options.inplace = 0 is automatic): banks = 1 (single bank
 * rewritten in place at every flush) or 2 (ping-pong banks); shared_flush = 1 when a flush step writes one matrix
 * per parent for all its children (two banks, block-lower storage).  What particleFilter.m:112-113's gather became. */
int rbpf_filter_schedule(const rbpf_ctx* ctx, int32_t* banks, int32_t* shared_flush);
/* Shared flush steps since the context was created that ran as ONE launch (writers and read-only siblings in one grid:
 * two banks, fp64 tiles at eight tile rows, 2-4 pending sets); the other shared flushes took two launches.  Filter and
 * sharded-filter contexts.                                                                          */
int rbpf_filter_one_launch_flushes(const rbpf_ctx* ctx, int64_t* n);
/* Resampling steps since the context was created whose ancestors were recomputed with the strict left-to-right cumsum
 * (tools/sample.m:30): the search runs on a parallel prefix sum and certifies every draw by a rounding bound; one draw inside
 * the bound of a bin edge sends the whole step through the strict sum.  Waits for the context's stream, changes nothing.   */
int rbpf_filter_resample_fallbacks(rbpf_ctx* ctx, int64_t* n);
/* Generic model family (RBPF_MODEL_GENERIC_DENSE), one time step at a time:
 *   t = 0:  rbpf_filter_step_external(ctx, xn0, measModel(xn0))
 *   t > 0:  rbpf_filter_ancestors(ctx, ai, xn_prev); xn(:,i) = dynModel(xn_prev(:,ai(i)+1), ...); 
 *           rbpf_filter_step_external(ctx, xn, measModel(xn))
 * ai [N_P] 0-based ancestors of the step about to run (drawn by the previous step), xn_prev [n_nonlin x N_P] the
 * states of the last step; xn_new [n_nonlin x N_P]; dy [N_P x n_y x n_lin] exactly as measModel returns it
 * ([N_P x n_lin] memory for n_y = 1).                                                                       */
int rbpf_filter_ancestors(rbpf_ctx* ctx, int32_t* ai, double* xn_prev);
int rbpf_filter_step_external(rbpf_ctx* ctx, const double* xn_new, const double* dy);
/* The generic family with handles that live on the device: the same step, but states and Jacobians are read from and
 * handed out in DEVICE memory, in stream order on rbpf_stream_get(ctx); between two steps nothing crosses to the host
 * and the library does not synchronise with it.  All four entry points take a filter context of the generic family
 * created with rbpf_model.callbacks == NULL (any other context: RBPF_ERR_STATE; NULL arguments and an unknown dy_layout:
 * RBPF_ERR_INVALID_ARG, before anything touches a device).
 *   dy_layout 0  MATLAB order as measModel returns it, dy(i,k,c) at i + N_P*(k + n_y*c)
 *             2  C-contiguous [N_P][n_y][n_lin], unpadded
 *             1  the native layout of the step kernels, H[(i*n_y + k)*ldx + c] with the row stride ldx >= n_lin of
 *                rbpf_filter_external_layout, consumed in place: the caller leaves columns n_lin..ldx-1 zero
 * Layouts 0 and 2 are packed into the native one by a kernel (one read and one write of the Jacobians).
 *   rbpf_filter_ancestors_device  as rbpf_filter_ancestors (RBPF_ERR_STATE before the first step and after the last):
 *        *ai_dev [N_P] the 0-based ancestors of the step about to run, *xn_anc_dev [n_nonlin x N_P] column-major their
 *        states, xn_anc(q,i) = xn_{t-1}(q, ai(i)).  Both are owned by the context and valid in stream order until the next
 *        step call.
 *   rbpf_filter_step_device       as rbpf_filter_step_external at every t; xn_new_dev [n_nonlin x N_P] column-major.
 *        Returns without waiting unless an on_step hook is set (then: synchronise, call the hook).
 *   rbpf_filter_set_device_callbacks  from now on rbpf_filter_advance drives the context with these callbacks and hands
 *        them device pointers: dyn_model(user, t, N_P, xn_anc_dev, xn_new_dev), meas_model(user, N_P, xn_dev, dy_dev) with
 *        dy_dev in dy_layout -- layout 1: the context's own Jacobian buffer (its pad zeroed here, once), 0 / 2: a staging
 *        buffer of the context.  The callbacks enqueue on rbpf_stream_get(ctx) or synchronise themselves; a non-zero
 *        return is RBPF_ERR_CALLBACK; dyn_res_norm is ignored.
 * n_y from 1 to 8 (see RBPF_MODEL_GENERIC_DENSE for what the widths other than 1 and 3 run with); every layout above is
 * written for any of them.  rbpf_filter_external_layout and rbpf_filter_ancestors_device also serve a context of
 * RBPF_MODEL_GENERIC_SPARSE (below), unchanged.                                                                         */
int rbpf_filter_external_layout(const rbpf_ctx* ctx, int32_t* ldx);
int rbpf_filter_ancestors_device(rbpf_ctx* ctx, const int32_t** ai_dev, const double** xn_anc_dev);
int rbpf_filter_step_device(rbpf_ctx* ctx, const double* xn_new_dev, const double* dy_dev, int32_t dy_layout);
int rbpf_filter_set_device_callbacks(rbpf_ctx* ctx, const rbpf_callbacks* callbacks, int32_t dy_layout);
/* The sparseFeatures branch with handles that live on the device (RBPF_MODEL_GENERIC_SPARSE; any other context:
 * RBPF_ERR_STATE, NULL arguments and unknown layouts: RBPF_ERR_INVALID_ARG before anything touches a device).  One step, in
 * stream order on rbpf_stream_get(ctx), nothing crosses to the host:
 *   t > 0:  rbpf_filter_ancestors_device(ctx, &ai, &xn_anc);  xn = dynModel(xn_anc, ...)        (t = 0: xn = x0_nonlin repeated)
 *           rbpf_filter_sparse_gathered_device(ctx, &xl, &ldx)
 *           [yhat, dy] = measModel(xn, xl)                                                       one call for all particles
 *           rbpf_filter_step_sparse_device(ctx, xn, yhat, yhat_layout, dy, dy_layout)
 *   rbpf_filter_sparse_gathered_device  *xl_dev [N_P][ldx]: row i holds xl(:,ai(i)) of the step about to run
 *        (particleFilter.m:112), columns n_lin..ldx-1 zero; at t = 0 the initial linear states (x0_lin n x 1 repeated, or
 *        n x N_P).  Owned by the context, valid in stream order until the next step call.  RBPF_ERR_STATE after the last step.
 *   rbpf_filter_step_sparse_device  xn_new_dev [n_nonlin x N_P] column-major.
 *        yhat_layout 0: yhat(i,k) at i + N_P*k (MATLAB order); 2: C-contiguous [N_P][n_y].
 *        dy_layout 0: dy(i,k,c) at i + N_P*(k + n_y*c) (MATLAB order, packed by a kernel first); 2: C-contiguous
 *        [N_P][n_y][n_lin]; 1: rows on the stride ldx, [N_P][n_y][ldx].  dy is dense: no structure is assumed.
 *        Rows of yhat / dy that belong to outputs not observed at this step (NaN in y) are not read by the step; they may hold
 *        anything.  Per particle: e = (y - yhat)(ind), S = dy(ind,:) P dy(ind,:)' + R(ind,ind), chol with the one jitter retry
 *        of particleFilter.m:145-148 (a second failure: RBPF_ERR_CHOL_FAILED at the next rbpf_sync / rbpf_filter_finish), the
 *        weight (:150), xl + K e and P - K S K' (:181,197-198); nothing observed: weight 0, state carried over.  Then the
 *        weights are normalised and the next ancestors drawn as for every other family.  Returns without waiting unless an
 *        on_step hook is set.  rbpf_filter_advance and device callbacks are not available for this kind (RBPF_ERR_STATE).
 *   rbpf_filter_sparse_yhattraj  yhattraj [n_y x N_T] column-major (particleFilter.m:94,201-203): column t is the whole yhat
 *        of step t's maximum-weight particle as the caller handed it in, NaN for steps not yet run.  Waits for the stream.    */
int rbpf_filter_sparse_gathered_device(rbpf_ctx* ctx, const double** xl_dev, int32_t* ldx);
int rbpf_filter_step_sparse_device(rbpf_ctx* ctx, const double* xn_new_dev, const double* yhat_dev, int32_t yhat_layout,
                                   const double* dy_dev, int32_t dy_layout);
int rbpf_filter_sparse_yhattraj(rbpf_ctx* ctx, double* yhattraj);
/* Enable (1) / disable (0) per-launch HIP-event timing of the stream kernel; read / reset it.     */
int rbpf_timing_enable(rbpf_ctx* ctx, int32_t on);
int rbpf_timing_read(rbpf_ctx* ctx, rbpf_timing* out, int32_t reset);
int rbpf_destroy(rbpf_ctx* ctx);

/* ---- particle-sharded filter (one process per GPU) ----------------------------------
 * The global filter has N = world * N_P logical slots.  A logical slot keeps its identity (RNG stream,
 * position in every output) but its particle may live on any rank: children are computed on the rank
 * that already holds their ancestor's map state ("owner computes") and only the load-imbalance excess
 * migrates.  Every rank always holds exactly N_P particles in physical slots 0..N_P-1.  The collectives
 * stay outside the library (torch.distributed over RCCL in multigpu.py); the library exposes the device
 * buffers and the kernels between them.  Per time step t >= 1 the host side does
 *   all_gather(fwd_local -> fwd_gather)                 log-weights + non-linear states, physical order
 *   rbpf_shard_normalise_search(ctx, perm, ai_host)     permute to logical order; global w / cumsum /
 *                                                       ancestors -- identical on every rank
 *   (host) placement of the new generation + exchange plan from the replicated ancestor vector
 *   rbpf_shard_pack(ctx, idx, count)                    ancestors another rank needs -> send records
 *   all_to_all_single(send_rec -> recv_rec)
 *   rbpf_shard_step(ctx, anc_bank, slot_ids)            fused step kernel for my N_P physical slots
 * and after the last step one more gather + rbpf_shard_normalise_search(ctx, perm, NULL).            */
typedef struct {
  int32_t rank, world, N_local, N_global, n_nonlin;
  size_t record_doubles;       /* doubles per exchanged particle record [Pt | Pb | F | xl]            */
  size_t recv_capacity;        /* records the receive buffer can hold                                */
  size_t send_capacity;        /* records the send buffer can hold                                   */
  double* fwd_local;           /* [fwd_rows][N_local]: rows xn, then logw (step kernel output); the sharded smoother
                                * appends one row, the measurement part of my particles' ancestor log-weights        */
  double* fwd_gather;          /* [world][fwd_rows][N_local] all_gather target                        */
  double* send_rec;            /* [send_capacity][record_doubles]                                     */
  double* recv_rec;            /* [recv_capacity][record_doubles]                                     */
  int32_t fwd_rows;            /* n_nonlin + 1 (filter) / n_nonlin + 2 (smoother)                     */
} rbpf_shard_views;

int rbpf_shard_create(const rbpf_model* model, const rbpf_problem* prob, const rbpf_rng* rng,
                      const rbpf_options* opt, int32_t rank, int32_t world, rbpf_ctx** ctx);
int rbpf_shard_views_get(rbpf_ctx* ctx, rbpf_shard_views* out);
/* After the gather: bring the forward bank into logical order (phys_of_logical_host [N_global]:
 * rank*N_local + physical index of each logical slot; NULL = identity), normalise the global weights,
 * cumsum, trajectory summaries of the step just finished; if ai_host != NULL also draw the ancestors of
 * ALL N_global logical slots (0-based logical ids; the same vector on every rank) into ai_host.
 * Synchronises the stream.                                                                          */
int rbpf_shard_normalise_search(rbpf_ctx* ctx, const int32_t* phys_of_logical_host, int32_t* ai_host);
/* Gather `count` local particles (physical indices idx_host, in send order) into send_rec.           */
int rbpf_shard_pack(rbpf_ctx* ctx, const int32_t* idx_host, int32_t count);
/* One fused step for my N_local physical slots.  slot_ids_host [N_local]: logical id of each physical
 * slot of the NEW generation; anc_bank_host [N_local]: where its ancestor's map state is (< N_local:
 * physical slot of the old local bank, >= N_local: N_local + record index in recv_rec).  Both NULL at
 * t = 0 (identity placement: logical slot rank*N_local + p at physical slot p).                      */
int rbpf_shard_step(rbpf_ctx* ctx, const int32_t* anc_bank_host, const int32_t* slot_ids_host);
/* Device-side planner (the production path): placement of the new generation + exchange plan from the
  * ancestors drawn by the last rbpf_shard_normalise_search, entirely on the device.  counts_host
 * [2*world+2] receives the records to send to / receive from every rank, the number of migrating
 * children, and the first record of recv_rec this step's exchange must write to (records persist across
 * the read-only steps of a lazy cycle).  Afterwards rbpf_shard_pack(ctx, NULL, n_send), rbpf_shard_step(ctx, NULL, NULL) and
 * rbpf_shard_normalise_search(ctx, NULL, ...) use the device plan.                                      */
int rbpf_shard_plan(rbpf_ctx* ctx, int64_t* counts_host);
/* rbpf_shard_normalise_search(ctx, NULL, draw) + rbpf_shard_plan(ctx, counts) in one call (what the production loop
 * uses): the ancestors are not copied to the host and the stream is synchronised once.                        */
int rbpf_shard_normalise_plan(rbpf_ctx* ctx, int64_t* counts_host);
/* Test hook: this rank's view of the current device plan.                                             */
int rbpf_shard_plan_read(rbpf_ctx* ctx, int32_t* slot_ids, int32_t* anc_bank, int32_t* send_idx,
                         int32_t n_send, int32_t* new_gid);
/* traj_max / traj_mean [n_nonlin x N_T] of the steps normalised so far (identical on every rank).     */
int rbpf_shard_trajectories(rbpf_ctx* ctx, double* traj_max, double* traj_mean);
/* xn_traj [n_nonlin x N_global x t] of the steps finished so far (particleFilter.m:117-118: every logical slot's path traced
 * back through the ancestor table; needs keep_history).  The state history and the ancestor table are replicated (they come with
 * the all-gather of the forward bank), so any one rank returns the whole array.                                              */
int rbpf_shard_xn_traj(rbpf_ctx* ctx, double* xn_traj);
/* The HIP stream a context enqueues on (hipStream_t).  A caller that issues its collectives on this stream
 * (torch.cuda.ExternalStream) needs no host synchronisation between the library calls and the collectives.      */
/* ctx == NULL inside a device callback of rbpf_particle_smoother_device (on the thread that made the call): the stream of the
 * context that is calling back, which the caller never sees; likewise rbpf_filter_external_layout(NULL, &ldx) there.  NULL
 * anywhere else stays RBPF_ERR_INVALID_ARG.                                                                                 */
int rbpf_stream_get(rbpf_ctx* ctx, void** hip_stream);
/* on = 1: rbpf_shard_pack / rbpf_shard_step / rbpf_shard_smoother_step return without synchronising the stream (the caller's
 * collectives are ordered behind them on the same stream); on = 0 (default): they synchronise (host / gloo transports).    */
int rbpf_shard_set_async(rbpf_ctx* ctx, int32_t on);
/* Final extraction of the sharded filter (particleFilter.m:220-233), after the last step was gathered and normalised.
 * phase 0: iw_max (logical index, identical on every rank); xl_max [n], P_max [n x n] written by the rank that holds that
 *          particle and zero-filled elsewhere; xl_mean [n] = this rank's share of sum_i w_i xl_i; traj_sample_iwmax
 *          [n_nonlin x N_T] (needs keep_history; identical on every rank).  The caller sum-reduces xl_max, P_max, xl_mean.
 * phase 1: xl_mean is INPUT (the reduced mean); P_mean [n x n] = quirk Q3's last-particle term w_N (P_N + (xl_mean - xl_N)
 *          (xl_mean - xl_N)') written by the rank that holds logical slot N - 1, zero elsewhere (the caller sum-reduces it).
 * NULL outputs are skipped.                                                                                          */
int rbpf_shard_finish(rbpf_ctx* ctx, int32_t phase, double* xl_max, double* P_max, double* xl_mean, double* P_mean,
                      double* traj_sample_iwmax, int32_t* iw_max);
/* Test hook: replace the ancestors drawn for the next step (ai [N_global], logical ids) before rbpf_shard_plan.        */
int rbpf_shard_set_ancestors(rbpf_ctx* ctx, const int32_t* ai);

/* ---- particle-sharded information-form smoother ---------------------------------
 * particleSmootherInformationForm.m with the N = world * N_P particles of every CPF-AS iteration sharded like the
 * filter above.  The extra information-form state (ivec, Imat, halfLogDetP) travels in the particle records.
 * The measurement part of the ancestor weights of the reference trajectory (:205-236: one n x n factorisation per particle, or
 * one sweep over its carried factor) is computed on the rank that holds each particle, BEFORE the all_gather of the forward
 * bank, whose extra row carries it along (one collective per step instead of two); log w and the dynResNorm part are added
 * for all N particles from the gathered bank, identically on every rank, then normalised and sampled.  Results equal the
 * single-GPU rbpf_particle_smoother(info_form = 1) with N particles bit for bit.  Per iteration k the host side does
 *   rbpf_shard_smoother_begin(ctx, k)
 *   t = 0: rbpf_shard_smoother_step(ctx)
 *   t > 0: k > 0 (no refresh due): rbpf_shard_smoother_anc_weights(ctx)
 *          all_gather(fwd_local -> fwd_gather); rbpf_shard_smoother_normalise(ctx, 1)
 *          k > 0: rbpf_shard_smoother_anc_sample(ctx, 0)
 *                 (refresh steps of the carried factors: the refresh sequence below, all_gather(anc_local -> anc_gather),
 *                  rbpf_shard_smoother_anc_sample(ctx, 1))
 *          rbpf_shard_plan; rbpf_shard_pack; all_to_all_single(send_rec -> recv_rec); rbpf_shard_smoother_step(ctx)
 *   all_gather; rbpf_shard_smoother_normalise(ctx, 0); rbpf_shard_smoother_end(ctx, ...)                       */
typedef struct {
  double* anc_local;           /* [N_local] measurement part of my particles' ancestor log-weights (physical order): the
                                * last row of fwd_local                                                    */
  double* anc_gather;          /* [world][N_local] all_gather target of anc_local on its own (refresh steps) */
  /* carried factors (chol_refresh > 1): base matrices exchanged at a refresh, [refresh_capacity][matrix_doubles]; NULL / 0
   * otherwise                                                                                                */
  double* refresh_send;
  double* refresh_recv;
  int64_t refresh_capacity;
  int64_t matrix_doubles;      /* n_lin * n_lin                                                            */
} rbpf_shard_smoother_views;

int rbpf_shard_smoother_create(const rbpf_model* model, const rbpf_problem* prob, const rbpf_rng* rng,
                               const rbpf_options* opt, int32_t N_K, int32_t rank, int32_t world, rbpf_ctx** ctx);
int rbpf_shard_smoother_views_get(rbpf_ctx* ctx, rbpf_shard_smoother_views* out);
/* Start of iteration k (0-based): rewind; k > 0: H along the reference trajectory + suffix sums (:120,:132-146). */
int rbpf_shard_smoother_begin(rbpf_ctx* ctx, int32_t k);
/* Global weights of the finished step; want_draw: ancestors of the ordinary slots of the next one (:160-166).   */
int rbpf_shard_smoother_normalise(rbpf_ctx* ctx, int32_t want_draw);
/* k > 0, t > 0, before the gather: measurement part of my particles' ancestor log-weights -> anc_local (:205-236). */
int rbpf_shard_smoother_anc_weights(rbpf_ctx* ctx);
/* After gather + normalise: add log w and the dynResNorm part (:175-182,232) for all N particles, normalise (:243-245) and
 * draw ai(N_P) (:248).  separate_gather: 0 = the measurement parts came with the forward bank, 1 = they are in anc_gather. */
int rbpf_shard_smoother_anc_sample(rbpf_ctx* ctx, int32_t separate_gather);
/* Carried ancestor-weight factors in the sharded smoother (rbpf_options.chol_refresh = K > 1, lazy_depth as usual): between
 * refreshes rbpf_shard_smoother_anc_weights runs one up/down-date sweep per particle over its ancestor's factor, which migrates
 * inside the particle records in place of Imat.  At the steps t = 1 and (t - 1) % K == 0 of an iteration k > 0 the factors are
 * refreshed INSTEAD of rbpf_shard_smoother_anc_weights:
 *   rbpf_shard_smoother_refresh_begin(ctx, owner_now, base_loc)   both [N_global] int32, identical on every rank:
 *        owner_now[j] = rank * N_local + slot of logical slot j's particle, base_loc[j] = the same for the ancestor its
 *        information matrix is rebuilt from (-1: the common initial matrix, nothing to fetch)
 *   the host mirror derives the fetch plan from the two tables (multigpu.plan_refresh: unique (destination, matrix) pairs),
 *   rbpf_shard_smoother_refresh_pack(ctx, slots, count); all_to_all_single(refresh_send -> refresh_recv);
 *   rbpf_shard_smoother_refresh_end(ctx, base_index, n_recv)      base_index [N_local]: bank slot or N_local + position in
 *        refresh_recv
 * (after the gather and normalise of the finished step: the walk reads the state history), then all_gather(anc_local ->
 * anc_gather) and rbpf_shard_smoother_anc_sample(ctx, 1).                                           */
 /* (the plan: rbpf_plan_refresh below -- the one implementation both multi-GPU drivers use) */
int rbpf_shard_smoother_refresh_begin(rbpf_ctx* ctx, int32_t* owner_now, int32_t* base_loc);
/* Fetch plan of one refresh for `rank`, from the two replicated tables (host arithmetic only, no device access): rank q sends
 * rank r each matrix some particle on r needs, once (siblings share it), ordered by (destination, source, slot).  send_slots
 * [<= send_capacity] bank slots to pack, concatenated per destination (*n_send of them); send_counts / recv_counts [world] of
 * this rank; send_totals / recv_totals [world]: every rank's totals (capacity check, identical on all ranks); base_index
 * [n_local]: a slot of the own bank, or n_local + position in refresh_recv.  Used by the in-library driver (rbpf_options.
 * n_devices) and by multigpu.ShardedSmootherSession alike; multigpu.plan_refresh (numpy) is its specification in the tests. */
int rbpf_plan_refresh(const int32_t* owner_now, const int32_t* base_loc, int32_t N_global, int32_t n_local, int32_t world,
                      int32_t rank, int32_t* send_slots, int32_t send_capacity, int32_t* n_send, int64_t* send_counts,
                      int64_t* recv_counts, int64_t* send_totals, int64_t* recv_totals, int32_t* base_index);
/* Before refresh_pack, when the plan's largest per-rank total exceeds rbpf_shard_smoother_views.refresh_capacity: every rank
 * (the plan is replicated) enlarges its refresh buffers to hold `count` matrices -- rbpf_shard_smoother_views_get then returns the
 * new pointers / capacity -- unless rbpf_options.exchange_capacity > 0 made the capacity a hard limit (RBPF_ERR_OUT_OF_MEMORY).  */
int rbpf_shard_smoother_refresh_reserve(rbpf_ctx* ctx, int64_t count);
int rbpf_shard_smoother_refresh_pack(rbpf_ctx* ctx, const int32_t* slots, int32_t count);
int rbpf_shard_smoother_refresh_end(rbpf_ctx* ctx, const int32_t* base_index, int32_t n_recv);
/* One information-form time step of my particles (:256-335), using the plan of rbpf_shard_plan for t > 0.        */
int rbpf_shard_smoother_step(rbpf_ctx* ctx);
/* End of iteration (:346-354): ak = sample(w), new reference trajectory -> XNK_k [n_nonlin x N_T] (every rank);
 * XLK_k [n_lin], PK_k [n_lin x n_lin] are filled by the rank that holds particle ak (*owner_rank), zero elsewhere. */
int rbpf_shard_smoother_end(rbpf_ctx* ctx, double* XNK_k, double* XLK_k, double* PK_k, int32_t* ak,
                            int32_t* owner_rank);

/* ---- helper kernels exposed for parity tests (a5-a8, a19 of SURVEY 8a) ------------------------- */
/* The uniforms / normals the Philox generator hands to slot i at step t of iteration k, in replay
 * layout (U [N_P x (N_T-1)], Z [n_w x N_P x (N_T-1)]), so a replay run can reproduce a Philox run. */
int rbpf_philox_fill(uint64_t seed, int32_t k_iter, int32_t N_P, int32_t N_T, int32_t n_w,
                     double* U, double* Z, double* Ufin);
/* measModel of the family evaluated on the device: xn [n_nonlin x Npred] -> dy stored as
 * [n_y x n_lin x Npred] (i.e. H_i contiguous per particle).  run_dense3D_magfield.m:265-279.      */
int rbpf_meas_model(const rbpf_model* model, int32_t n_nonlin, int32_t n_pred, const double* xn,
                    double* dy);
/* dynModel with injected normals: xn [n_nonlin x Np], odo [n_odo], cholQ from (dt,Q),
 * z [n_w x Np] -> xn_next [n_nonlin x Np].  run_dense3D_magfield.m:301-308.                       */
int rbpf_dyn_model(const rbpf_model* model, int32_t n_nonlin, int32_t n_w, int32_t n_odo,
                   int32_t n_p, const double* xn, const double* odo, double dt, const double* Q,
                   const double* z, double* xn_next);
/* dynResNorm: eDyn [n_w x Np] for reference state xnk_t against xn [n_nonlin x Np]
 * (run_dense3D_magfield.m:202-203; default additive form when model->use_dyn_res_norm == 0).      */
int rbpf_dyn_res_norm(const rbpf_model* model, int32_t n_nonlin, int32_t n_w, int32_t n_odo,
                      int32_t n_p, const double* xnk_t, const double* xn, const double* odo,
                      double dt, const double* Q, double* e_dyn);
/* tools/sample.m:30-32 applied to n_draws uniforms: ind[j] = sum(cumsum(w) < u[j]) (0-based,
 * clamped to N-1).                                                                                */
int rbpf_sample(int32_t N, const double* w, int32_t n_draws, const double* u, int32_t* ind);
/* tools/JacobianPhi3D.m:29-64: x [3 x Np] -> J [3 x 3 x m x Np].                                  */
int rbpf_jacobian_phi3d(const rbpf_model* model, int32_t n_p, const double* x,
                        const double* lower, const double* upper, double* J);
/* particleSmoother.m:221-229 for a batch of matrices: cS = chol(S,'lower') (one retry with S + jitter*I),
 * v = cS \ e, logw[b] = -sum(log(diag(cS))) - v'v/2 - M/2*log(2*pi).  S [batch][M x M] column-major (lower
 * triangle read), e [batch][M].  variant 0: automatic kernel choice; 16: the 16-column kernel; 64 / 648 / 644: the
 * 64-column kernel (waves by size / 8 / 4); 1: the register-resident kernel in its default shape (64 <= M <= 143, information
 * form only; two waves per matrix); 11 / 12 / 14: the same with one / two / four waves per matrix (14: the r02 kernel); 10: one
 * wave per matrix, left-looking on register tiles (the next block column's loads in flight during a column's work).
 * variant + 1000: the information-form loaders and expression of particleSmootherInformationForm.m:224-236 with
 * ImatAddt = ivecAddt = 0, i.e. logw[b] = -sum(log(diag(cI))) + v'v/2 and no retry.  reps >= 1 repeats the launch;
 * *ms (may be NULL) = mean kernel time (HIP events).  *status (may be NULL): bit 1 set when a factorisation failed
 * (its logw is NaN).                                                                               */
int rbpf_chol_weights(int32_t M, int32_t batch, const double* S, const double* e, double jitter,
                      int32_t variant, int32_t reps, double* logw, int32_t* status, double* ms);
/* What rbpf_options.chol_refresh = `requested` means for an information-form smoother of this model family and size: the K in
 * use (> 1: carried factors refreshed every K-th step; 1: from-scratch factorisation every step).  The multi-rank drivers need it
 * to issue the refresh exchange at the right steps.                                                                          */
int32_t rbpf_chol_refresh_resolve(int32_t model_kind, int32_t n_lin, int32_t n_y, int32_t requested);
/* The sweep kernel of the carried factors (rbpf_options.chol_refresh) on its own, for the kernel-level parity test and the
 * bench: ONE augmented factor L [(n+1) x (n+1)] column-major lower = [chol(A) 0; z' *], z = chol(A) \ b, replicated `batch`
 * times; U, V [d x n] column-major (row a = update / downdate vector a), eta [d] = the entry both vectors carry in the augmented
 * row.  Result (copy 0): L_out (same layout) = the factor of A + U'U - V'V with the row (L_out \ (b + U' eta - V' eta))', and
 * *logw = -sum(log(diag(L_out))) + z_out' z_out / 2 (particleSmootherInformationForm.m:234-236 without the qf / halfLogDetP
 * terms).  d = 1 or 3, n <= 575.  *status bit 1: a downdate lost definiteness.  reps / *ms as in rbpf_chol_weights.        */
int rbpf_chol_sweep_probe(int32_t n, int32_t d, int32_t batch, const double* L, const double* U, const double* V,
                          const double* eta, int32_t reps, double* L_out, double* logw, int32_t* status, double* ms);
/* The pack-and-whiten kernel of the refreshes behind rbpf_particle_smoother_device on its own, for the kernel-level test:
 * dy_host [rows x d x n] in dy_layout 0 (MATLAB order, dy(i, k, c) at i + rows * (k + d * c)) or 2 (C-contiguous), W_host
 * [d x d] column-major; G_host [rows][d][n] receives G(i, a, c) = sum_b W(a, b) dy(i, b, c), accumulated as s = 0; for b
 * ascending: s = fma(W(a, b), dy(i, b, c), s).  fused = 1: one kernel, from the layout straight to G; fused = 0: the pack kernel
 * followed by the whitening kernel the built-in families' refreshes run -- the same bits.  d = 1 or 3.                      */
int rbpf_ext_pack_whiten_probe(int32_t dy_layout, int32_t rows, int32_t d, int32_t n, const double* dy_host,
                               const double* W_host, int32_t fused, double* G_host);
/* The build kernel of rbpf_particle_smoother_sparse_device's ancestor weights on its own, for the kernel-level test and the
 * bench, on caller-supplied DEVICE arrays: P_dev [N][n][n] (symmetric), D_dev [N][M][n] row-major, pair_t_dev / pair_j_dev [M] the
 * time and the output (0 .. d-1) of every stacked row, R_dev [d x d] column-major; S_dev [N][M*M] column-major receives
 * S_i(a, b) = (D_i P_i D_i')(a, b) + (pair_t[a] == pair_t[b] ? R(pair_j[a], pair_j[b]) : 0) in the 16 x 16 tiles on and below the
 * diagonal (what the batched Cholesky reads); the tiles above are not written.  n <= 96, M <= 1023.  Runs on the null stream and
 * waits for it; reps >= 1 repeats the launch, *ms (may be NULL) = mean kernel time (HIP events).                           */
int rbpf_sparse_ext_build_probe(int32_t N, int32_t n, int32_t M, int32_t d, const double* P_dev, const double* D_dev,
                                const int32_t* pair_t_dev, const int32_t* pair_j_dev, const double* R_dev, int32_t reps,
                                double* S_dev, double* ms);
/* Quaternion helpers of tools/ on the device, batched over n columns, for the parity tests:
 *   op 0  expq, scalar branch   tools/expq.m:22-31  (flip when q0 < 0)          in [3 x n]      -> out [4 x n]
 *   op 1  expq, batched branch  tools/expq.m:33-37  (flip when q0 <= 0)         in [3 x n]      -> out [4 x n]
 *   op 2  logq, scalar branch   tools/logq.m:25-30  (flip when q0 < 0)          in [4 x n]      -> out [3 x n]
 *   op 3  logq, batched branch  tools/logq.m:32-35  (flip when q0 <= 0)         in [4 x n]      -> out [3 x n]
 *   op 4  qLeft                 tools/qLeft.m:30-40                              in [4 x n]      -> out [4 x 4 x n]
 *   op 5  qRight                tools/qRight.m:29-39                             in [4 x n]      -> out [4 x 4 x n]
 *   op 6  qInv                  tools/qInv.m:27-31                               in [4 x n]      -> out [4 x n]
 *   op 7  quat2rmat             tools/quat2rmat.m:27-40                          in [4 x n]      -> out [3 x 3 x n]
 *   op 8  mcross                tools/mcross.m:33-42                             in [3 x n]      -> out [3 x 3 x n]
 * q0 > 1 by rounding is clamped before acos (quirk Q7).                                                             */
int rbpf_quat_helpers(int32_t op, int32_t n, const double* in, double* out);
/* The wave-level reduction of the symmetric-storage step kernel (rbpf_step_sym.hip: v_permlane32_swap / v_permlane16_swap
 * folds + DPP row rotations) on its own, for the kernel-level test: in [4][64] (four values per lane of one wave64) -> out [4],
 * out[v] = sum over the 64 lanes of in[v][.] in the kernel's fixed association order.                                    */
int rbpf_probe_wave_reduce(const double* in, double* out);
/* The wave sums of the step kernel's body, four per register butterfly, beside the xor butterfly they replace: one wave64 sums
 * nv (1 .. 36) vectors, in [nv][64] -> out_ref [nv] by the xor butterfly through LDS, out_packed [nv] by the packed form.  The two
 * agree bit for bit (same lane pairs at every stage).                                                                   */
int rbpf_probe_wave_sums_packed(int32_t nv, const double* in, double* out_ref, double* out_packed);

/* ---- localisation in a fixed GP map (examples/mag-localization-mapping) --------------------------
 * particleFilterLocalization.m:84-132 with the closures of run_localization.m:241-281: a particle filter over the
 * 7 non-linear states (pos3 + quat4) that carries no map state.  The map is a posterior N(mean, P) over the n = m + 3
 * coefficients of the dense-mag basis, handed over as the mean and a lower-triangular factor V with V'V = P.  Per step and
 * particle i, with G_c(i) = row c of [e_c, d_c Phi(p_i)]:
 *     dEft(i,c) = G_c(i) mean,   var(i,c) = |V G_c(i)'|^2   (or var_table(i,c), the reference's literal reading: quirk Q10),
 *     w(i) = sum_c normpdf(y_t(c), (Rnb_i' dEft(i,:)')(c), sqrt(var(i,c) + sigma2))       -- a SUM of three densities
 * dynModel (:274-281): pos + dx + sqrt(dt Q(1:3,1:3)) randn(3,1) with the ELEMENT-WISE square root, orientation
 * qLeft(qRight(q) dq) expq(sqrt(dt Q(4:6,4:6)) randn(3,1)).  R of the reference signature is not used (:19).
 * These structs are additions to ABI 9: each starts with its own struct_size (0 is accepted as in rbpf_options). */
typedef struct {
  int32_t struct_size;       /* sizeof(rbpf_loc_map) = rbpf_abi_sizeof(9)                                */
  int32_t m_basis;           /* m; n = m + 3, 4 <= n <= 1151                                             */
  const int32_t* NN;         /* [m x 3] column-major index table (domain_cartesian_dx.m:36-43)           */
  double L[3];               /* domain half-widths                                                       */
  const double* mean;        /* [n] posterior mean (`foo`, run_localization.m:151)                       */
  const double* V;           /* [n x n] column-major, lower triangle read: V'V = P.  May be NULL         */
  double sigma2;             /* measurement noise variance (theta(4))                                    */
  const double* var_table;   /* [N_P x 3] column-major: slot i uses row i (run_localization.m:261-263,270). May be NULL; *
                              * exactly one of V / var_table is set for the filter entry points          */
} rbpf_loc_map;

typedef struct {
  int32_t struct_size;       /* sizeof(rbpf_loc_problem) = rbpf_abi_sizeof(10)                           */
  int32_t N_P, N_T;          /* particles; time steps = size(y,1)                                        */
  int32_t x0_cols;           /* 1 or N_P   (particleFilterLocalization.m:55-59)                          */
  int32_t q_pages;           /* 1 or >= N_T-1  (:66-68)                                                  */
  int32_t dt_len;            /* 1 or >= N_T-1  (:71-73)                                                  */
  int32_t odo_ld;            /* leading dimension of odometry                                            */
  const double* odometry;    /* [>= N_T-1 x 7]                                                           */
  const double* y;           /* [N_T x 3]                                                                */
  const double* x0_nonlin;   /* [7 x x0_cols]                                                            */
  const double* Q;           /* [6 x 6 x q_pages]                                                        */
  const double* dt;          /* [dt_len]                                                                 */
} rbpf_loc_problem;

/* Outputs of particleFilterLocalization (:1, :25-26) as of the last finished step (T_done columns are filled).  NULL
 * pointers are skipped.                                                                                  */
typedef struct {
  int32_t struct_size;       /* sizeof(rbpf_loc_out) = rbpf_abi_sizeof(11)                               */
  int32_t first_degenerate_step; /* OUT: -1, or the first 0-based t with sum(w) <= 1e-12 (:113-115)      */
  double* traj_max;          /* [7 x N_T]                                                                */
  double* traj_mean;         /* [7 x N_T] (quaternion rows included, not renormalised: :123)             */
  /* extras */
  double* trace_logw;        /* [N_P x N_T] log of the unnormalised weights (needs trace)                */
  double* trace_w;           /* [N_P x N_T] (needs trace)                                                */
  int32_t* trace_ai;         /* [N_P x N_T] 0-based, column 0 unused (needs keep_history)                */
  double* final_xn;          /* [7 x N_P]                                                                */
  double* xn_traj;           /* [7 x N_P x N_T] (needs keep_history): :101-104, traced back on request   */
  double* log_sum_w;         /* [N_T] log(sum(w)) before the normalisation of :118                       */
} rbpf_loc_out;

/* One shot.  Of `opt` only struct_size, keep_history, trace, on_step / on_step_user are read (jitter is ignored); any
 * other non-zero field is RBPF_ERR_UNSUPPORTED (n_devices > 1 included).  on_step: view->ctx is valid for rbpf_loc_finish. */
int rbpf_particle_filter_localization(const rbpf_loc_map* map, const rbpf_loc_problem* prob, const rbpf_rng* rng,
                                      const rbpf_options* opt, rbpf_loc_out* out);
/* Resident form: rbpf_sync, rbpf_filter_tell and rbpf_destroy work on the context.                      */
int rbpf_loc_create(const rbpf_loc_map* map, const rbpf_loc_problem* prob, const rbpf_rng* rng, const rbpf_options* opt,
                    rbpf_ctx** ctx);
int rbpf_loc_advance(rbpf_ctx* ctx, int32_t n_steps);
int rbpf_loc_finish(rbpf_ctx* ctx, rbpf_loc_out* out);
/* Bytes of device memory such a context needs (no device access).                                       */
int rbpf_loc_workspace_bytes(const rbpf_loc_map* map, const rbpf_loc_problem* prob, const rbpf_options* opt, size_t* bytes);
/* The prediction kernel on its own: xn [7 x n_pred] -> dEft [3 x n_pred], var [3 x n_pred] (var and map->V may be NULL:
 * means only; map->var_table is not read).  reps >= 1 repeats the launch; *ms (may be NULL) = median kernel time.       */
int rbpf_loc_predict(const rbpf_loc_map* map, int32_t n_pred, const double* xn, double* dEft, double* var, int32_t reps,
                     double* ms);
/* dynModel of run_localization.m:274-281 with injected normals: xn [7 x n_p], odo [7], z [6 x n_p] -> xn_next [7 x n_p]. */
int rbpf_loc_dyn_model(int32_t n_p, const double* xn, const double* odo, double dt, const double* Q, const double* z,
                       double* xn_next);

/* ---- backward-simulation smoother for localisation in a fixed map --------------------------------
 * Forward filter, backward simulation (Godsill, Doucet & West 2004).  In a fixed map the state (pos3 + quat4) is Markov, so
 * n_traj trajectories are drawn backwards through the forward particles X [7 x N_P x N_T] (as propagated) and normalised weights
 * w of a localisation context created with keep_history = 1 and trace = 1, all N_T steps done:
 *     b(j, N_T) = sample(w(:, N_T));   t = N_T-1 .. 1:  l(i) = log(w(i, t)) + logp(xs(:, j, t+1) | X(:, i, t)),  b(j, t) = sample(p)
 * with p the log-sum-exp normalisation of l (particleSmoother.m:232, :236-238, :241).  logp is the density of dynModel
 * (run_localization.m:274-281) as it draws, constants omitted (particleSmoother.m:181-182), with odometry row t, dt(t), Q(:,:,t):
 *     a = qRight(q_i) dq,  e = qLeft(qInv(a)) q~,  phi = logq(e),  r = [p~ - p_i - dx(1:3); phi],
 *     z = blkdiag(S_pos, S_rot) \ r  (S = sqrt(dt Q) element-wise on the diagonal blocks),  logp = -z'z / 2.
 * A singular S block is RBPF_ERR_INVALID_ARG.  w(i) = 0 is never selected.  A draw past the last cdf edge is clamped to the
 * last particle with a non-zero term and counted with the filter's clamped draws.
 * u [N_T x n_traj], row t = step t (u[t * n_traj + j]), uniforms in (0, 1]; NULL: Philox4x32-10 keyed by `seed` on the counters
 * (slot = j, step = t, lane = 0x42530000, iter = 0), first uniform -- disjoint from the filter's lanes 0 .. 4.  The generator's
 * uniforms are (a + 0.5) 2^-53 of a 53-bit a, rounded as doubles: they lie in (0, 1] (1.0 when all 53 bits are set).
 * Outputs (NULL pointers are skipped): xs_traj [7 x n_traj x N_T], index [n_traj x N_T] 0-based, traj_smooth_mean [7 x N_T] (plain
 * means over the trajectories of all 7 rows, as particleFilterLocalization.m:123).  The workspace comes from the context's pool
 * and is returned before the call returns.  RBPF_ERR_STATE: steps missing, no keep_history / trace, or a degenerate forward step;
 * RBPF_ERR_INVALID_ARG: not a localisation context, n_traj < 1.  The context stays usable after a refusal.                     */
int rbpf_loc_backward_simulate(rbpf_ctx* ctx, int32_t n_traj, const double* u, uint64_t seed, double* xs_traj, int32_t* index,
                               double* traj_smooth_mean);
/* The forward particles as propagated, NOT traced back: xn_fwd [7 x N_P x T_done] (needs keep_history).                       */
int rbpf_loc_history(rbpf_ctx* ctx, double* xn_fwd);
/* Bytes of device memory rbpf_loc_backward_simulate takes from the pool while it runs (no device access).                     */
int rbpf_loc_backward_workspace_bytes(int32_t N_P, int32_t N_T, int32_t n_traj, size_t* bytes);
/* One backward step on the caller's arrays, the kernel-level probe: xn [7 x N], w [N], xs_next [7 x M], odo [7], Q [6 x 6],
 * u [M] -> index [M]; logp [N x M] column-major (may be NULL) = the transition log densities without log(w).  reps >= 1 repeats
 * the step's launches; *ms (may be NULL) = median time of one step.                                                            */
int rbpf_loc_backward_step(int32_t N, int32_t M, const double* xn, const double* w, const double* xs_next, const double* odo,
                           double dt, const double* Q, const double* u, int32_t* index, double* logp, int32_t reps, double* ms);

/* ---- the MAP trajectory of a localisation run ------------------------------------------------------
 * MAP sequence estimation over the stored particles (Godsill, Doucet & West 2001): the one path through the forward particles
 * X [7 x N_P x N_T] (as propagated) of a context created with keep_history = 1 and trace = 1, all N_T steps done, that maximises
 * the joint of states and measurements.  A Viterbi recursion whose states at step t are the N_P particles:
 *     delta(j, 1)   = log(w(j, 1))
 *     delta(j, t+1) = log(w(j, t+1)) + max_i [ delta(i, t) + logp(X(:, j, t+1) | X(:, i, t)) ],   psi(j, t+1) = the arg max
 *     i(N_T) = arg max_j delta(j, N_T),   i(t) = psi(i(t+1), t+1),   x_map(:, t) = X(:, i(t), t),   score = delta(i(N_T), N_T)
 * with logp the density of rbpf_loc_backward_simulate and odometry row t, dt(t), Q(:,:,t).  Among equal candidates the lowest
 * index wins, at every max.  log(w) stands in for the measurement likelihood: the filter resamples at every step, so the normalised
 * weights are the likelihoods up to one constant per step; score is the log joint up to constants that do not depend on the path
 * (those, and the normaliser of the transition density).  A particle with w = 0, or one no predecessor reaches, has delta = -inf
 * and psi = 0.  In a fixed map the state is Markov, so the recursion is exact over particle paths.
 * Outputs (NULL pointers are skipped): x_map [7 x N_T], index [N_T] 0-based, *score.  The workspace (psi as int32 [N_T][N_P], two
 * rows of delta, the chunk partials, the predicted particles) comes from the context's pool and is returned before the call
 * returns.  Refusals as rbpf_loc_backward_simulate: RBPF_ERR_STATE for steps missing, no keep_history / trace or a degenerate
 * forward step, RBPF_ERR_UNSUPPORTED for a generic context (rbpf_loc_generic_map_* below).  The context stays usable.            */
int rbpf_loc_map_trajectory(rbpf_ctx* ctx, double* x_map, int32_t* index, double* score);
/* Bytes of device memory rbpf_loc_map_trajectory takes from the pool while it runs (no device access).                          */
int rbpf_loc_map_workspace_bytes(int32_t N_P, int32_t N_T, size_t* bytes);
/* One step of the recursion on the caller's arrays, the kernel-level probe: xn [7 x N], delta [N] (-inf allowed), xs_next [7 x M]
 * (the successors), odo [7], Q [6 x 6] -> best [M] = max_i [delta(i) + logp(xs_next(:, j) | xn(:, i))] and arg [M] its lowest arg
 * max, 0 where best = -inf.  reps >= 1 repeats the step's launches; *ms (may be NULL) = median time of one step.                */
int rbpf_loc_map_step(int32_t N, int32_t M, const double* xn, const double* delta, const double* xs_next, const double* odo, double dt,
                      const double* Q, double* best, int32_t* arg, int32_t reps, double* ms);

/* ---- the marginal smoothing weights of a localisation run -------------------------------------------
 * Forward filtering, backward smoothing (FFBSm, Doucet, Godsill & Andrieu 2000) over the forward particles X [7 x N_P x N_T] (as
 * propagated) and weights w of a context created with keep_history = 1 and trace = 1, all N_T steps done: the smoothed weight
 * of EVERY stored particle,
 *     ws(i, N_T) = w(i, N_T)
 *     D(j, t)    = sum_l w(l, t) p(X(:, j, t+1) | X(:, l, t))
 *     ws(i, t)   = w(i, t) sum_j ws(j, t+1) p(X(:, j, t+1) | X(:, i, t)) / D(j, t)              t = N_T-1 .. 1
 * with p the density of rbpf_loc_backward_simulate and odometry row t, dt(t), Q(:,:,t).  Deterministic: no uniforms, no n_traj.
 * All sums run in the log domain in fp64, in a fixed order that depends on N_P only; every step is normalised by its
 * mass(t) = sum_i ws(i, t) before normalisation, 1 in exact arithmetic and returned as a diagnostic (mass(N_T) = 1).  A particle
 * with w = 0 has ws = 0 exactly and passes nothing back; a successor that no predecessor reaches passes nothing back either (its
 * share shows as mass < 1).  ws(:, N_T) is w(:, N_T) bit for bit.
 * Outputs (NULL pointers are skipped): w_smooth [N_P x N_T], mean [7 x N_T] = sum_i ws(i, t) X(:, i, t), cov [7 x 7 x N_T] the
 * weighted second central moment about that mean, ess [N_T] = 1 / sum_i ws(i, t)^2, mass [N_T].  The means are PLAIN weighted
 * means of all 7 rows, the way the filter's traj_mean treats them: the quaternion rows get no special handling.  The workspace
 * comes from the context's pool and is returned before the call returns.  Refusals as rbpf_loc_map_trajectory.                   */
int rbpf_loc_marginal_smooth(rbpf_ctx* ctx, double* w_smooth, double* mean, double* cov, double* ess, double* mass);
/* Bytes of device memory rbpf_loc_marginal_smooth takes from the pool while it runs (no device access).                          */
int rbpf_loc_marginal_workspace_bytes(int32_t N_P, int32_t N_T, size_t* bytes);
/* One step of the recursion on the caller's arrays, the kernel-level probe: xn [7 x N], logw [N] = log w(:, t), xs_next [7 x M]
 * (the successors), logws_next [M] = log ws(:, t+1) (-inf allowed in both), odo [7], Q [6 x 6] -> D [M] = log sum_l exp(logw(l) +
 * logp(xs_next(:, j) | xn(:, l))) and lws [N] = log of the un-normalised ws(:, t); -inf where nothing contributes.  reps >= 1
 * repeats the step's launches; *ms (may be NULL) = median time of one step.                                                     */
int rbpf_loc_marginal_step(int32_t N, int32_t M, const double* xn, const double* logw, const double* xs_next, const double* logws_next,
                           const double* odo, double dt, const double* Q, double* D, double* lws, int32_t reps, double* ms);

/* ---- the two-slice statistics of the transition residual of a localisation run ----------------------
 * rbpf_loc_marginal_smooth, and with its weights the pairwise (two-slice) smoothed moments of the transition residual: with
 *     xi(i, j, t) = w(i, t) p(X(:, j, t+1) | X(:, i, t)) ws(j, t+1) / D(j, t)                  (sums to 1 over all pairs)
 * and r(i, j) = [p~ - (p_i + dx(1:3)); phi] the UN-WHITENED residual of rbpf_loc_backward_simulate's density (before S_pos and
 * S_rot divide it),
 *     S(:, :, t) = sum_ij xi r r',     m(:, t) = sum_ij xi r,     pair_mass(t) = sum_ij xi                       t = 1 .. N_T-1
 * page t belongs to the pair of steps (t, t+1).  S is the E-step of EM for the transition noise (its mean over t, divided by
 * dt(t), estimates the covariance per unit time), m the smoothed odometry bias, pair_mass 1 in exact arithmetic.  xi is never
 * stored: one more all-pairs pass per step reduces every pair on the fly, in fp64, in a summation order fixed by N_P; a pair whose
 * log xi lies below -746 contributes exactly 0.
 * Outputs (NULL pointers are skipped): the five of rbpf_loc_marginal_smooth, bit for bit what it returns, then S [6 x 6 x (N_T-1)],
 * m [6 x (N_T-1)], pair_mass [N_T-1].  Refusals as rbpf_loc_marginal_smooth.                                                     */
int rbpf_loc_pair_stats_smooth(rbpf_ctx* ctx, double* w_smooth, double* mean, double* cov, double* ess, double* mass, double* S, double* m,
                               double* pair_mass);
/* Bytes of device memory rbpf_loc_pair_stats_smooth takes from the pool while it runs (no device access).                        */
int rbpf_loc_pair_stats_workspace_bytes(int32_t N_P, int32_t N_T, size_t* bytes);
/* One step on the caller's arrays, the kernel-level probe: the arguments and the outputs D, lws of rbpf_loc_marginal_step, then
 * S [6 x 6], m [6], pair_mass [1] of that step (computed with the step's own mass = sum_i exp(lws(i))).  *ms = median time of
 * the marginal step, the normalisation and the statistics pass together.                                                       */
int rbpf_loc_pair_stats_step(int32_t N, int32_t M, const double* xn, const double* logw, const double* xs_next, const double* logws_next,
                             const double* odo, double dt, const double* Q, double* D, double* lws, double* S, double* m, double* pair_mass,
                             int32_t reps, double* ms);

/* ---- running two-slice statistics of a localisation run: forward-only smoothing -----------------------
 * The forward-only form of FFBSm for an additive functional (Del Moral, Doucet & Singh 2010): what rbpf_loc_pair_stats_smooth
 * gives after the run, accumulated over the steps and available WHILE the run goes on, at one all-pairs step per new time step.
 * Every particle carries tau(:, i, t), the conditional expectation of the functional accumulated so far:
 *     D(j)          = log sum_i w(i, t) p(X(:, j, t+1) | X(:, i, t))
 *     omega(i, j)   = w(i, t) p(X(:, j, t+1) | X(:, i, t)) / exp(D(j))                  (sums to 1 over i)
 *     tau(j, t+1)   = sum_i omega(i, j) (tau(i, t) + s(i, j)),     tau(:, 1) = 0,     s = [r r' / dt(t); r]
 *     S_run(:, :, k), m_run(:, k) = sum_j w(j, k+1) tau(j, k+1),     mass_run(k) = sum_j w(j, k+1) sum_i omega(i, j)     (= 1)
 * r the un-whitened residual of rbpf_loc_pair_stats_smooth.  Page k (k = 1 .. T_done-1) is the FFBSm estimate of
 * sum_{s<=k} E[r r'/dt(s) | y(1:k+1)] and sum_{s<=k} E[r | y(1:k+1)] from the steps 1 .. k+1 only; once every step is done the last
 * page equals sum_t S(:, :, t) / dt(t) and sum_t m(:, t) of rbpf_loc_pair_stats_smooth (the same estimator, another order of sums).
 * THE CARRY IS PERSISTENT STATE OF THE CONTEXT: tau [27 x N_P] (twice), the pages [N_T-1][43], the number of pairs of steps folded
 * in and the kernels' workspace are taken from the context's pool at the first call, kept across calls and across further
 * rbpf_loc_advance, and handed back by rbpf_loc_forward_stats_reset or rbpf_destroy.  A call folds in every stored pair of steps
 * (t, t+1) not yet folded, ascending; not every step has to be done, but at least 2, and keep_history = 1 and trace = 1.  The other
 * passes run beside a living carry as before.  Fixed summation order (a function of N_P), fp64, no atomics; a pair whose log omega
 * lies below -746 contributes exactly 0.
 * Outputs (NULL pointers are skipped): S_run [6 x 6 x (T_done-1)], m_run [6 x (T_done-1)], mass_run [T_done-1] (all pages, T_done =
 * the steps done), tau_S [6 x 6 x N_P] (both triangles) and tau_m [6 x N_P], the carry of the latest step.                        */
int rbpf_loc_forward_stats_update(rbpf_ctx* ctx, double* S_run, double* m_run, double* mass_run, double* tau_S, double* tau_m);
/* Hands the carry back to the pool; the next update starts again at the first pair of steps.  No carry: nothing happens.         */
int rbpf_loc_forward_stats_reset(rbpf_ctx* ctx);
/* Bytes of device memory the carry holds while it lives (no device access).  With rows = 7, n_res = 6, KF = n_res (n_res + 3) / 2,
 * C = max(256, ceil(ceil(N_P / max(1, ceil(1024 / ceil(N_P / 256)))) / 256) * 256) and nchunks = ceil(N_P / C), in doubles:
 *   (rows + 1) N_P                        the predecessors of a step
 * + 2 P,  P = what rbpf_loc_marginal_workspace_bytes counts per array of chunk partials (the normaliser pass's)
 * + 4 N_P                                 zeros, D, what the normaliser's merge writes next to D, reach
 * + nchunks (KF + 1) N_P                  the carry pass's chunk partials
 * + 2 KF N_P                              tau, ping-pong
 * + max(N_T - 1, 1) (n_res^2 + n_res + 1) the pages.                                                                              */
int rbpf_loc_forward_stats_workspace_bytes(int32_t N_P, int32_t N_T, size_t* bytes);
/* One step on the caller's arrays, the kernel-level probe: xn [7 x N], logw [N], xs_next [7 x M], odo [7], dt, Q as
 * rbpf_loc_marginal_step; tau_S [6 x 6 x N] (the lower triangle is read), tau_m [6 x N] the incoming carry -> D [M], tau_S_next
 * [6 x 6 x M], tau_m_next [6 x M], reach [M] = sum_i omega(i, j).  *ms = median time of the normaliser pass, the carry pass, its
 * merge and the reducer together (the reducer with uniform weights).                                                             */
int rbpf_loc_forward_stats_step(int32_t N, int32_t M, const double* xn, const double* logw, const double* xs_next, const double* tau_S,
                                const double* tau_m, const double* odo, double dt, const double* Q, double* D, double* tau_S_next,
                                double* tau_m_next, double* reach, int32_t reps, double* ms);

/* ---- fixed-lag smoothing of the state: forward-only, while the run goes on -------------------------------
 * E[x(s) | y(1 : s+lag)] and its covariance for every step s, at one all-pairs pass per new time step whatever the lag: the
 * forward-only form of FFBSm (the estimator of rbpf_loc_marginal_smooth) for the per-step functionals of the last `lag` steps.
 * With D and omega as at rbpf_loc_forward_stats_update, n = 7 state rows, c(:, s) the filter mean of step s and d = x - c(:, s),
 *     h(s)(x)        = d                                  (moments = 1, H = n columns)
 *                    = [d; lower triangle by rows of d d'] (moments = 2, H = n (n + 3) / 2 columns)
 *     T0(i, t)       = h(t)(X(:, i, t))
 *     T(l)(j, t+1)   = sum_i omega(i, j) T(l-1)(i, t),     l = 1 .. lag                (one pass over lag H columns)
 *     est(l, t+1)    = sum_j w(j, t+1) T(l)(j, t+1)  =  E[h(t+1-l)(x(t+1-l)) | y(1 : t+1)],     l = 0 .. lag
 *     mass(t+1)      = sum_j w(j, t+1) sum_i omega(i, j)                                (= 1)
 * est(l, t) is the FFBSm estimate from the steps up to t alone: what rbpf_loc_marginal_smooth gives for step t-l on a run that
 * ended at t, in another order of sums.  mean = c + E[d], cov = E[d d'] - E[d] E[d]': centred at the filter mean, nothing cancels.
 * Plain weighted moments of all rows: quaternion rows get no special handling.  Lags that reach before the first step carry zeros.
 * THE CARRY IS PERSISTENT STATE OF THE CONTEXT, with the life cycle of the running statistics' (and beside it, if both live): taken
 * from the context's pool at the first call, which fixes lag (1 .. 64) and moments; kept across calls and further
 * rbpf_loc_advance; handed back by rbpf_loc_fixed_lag_reset or rbpf_destroy.  A call with another lag or moments is refused
 * (RBPF_ERR_STATE: reset first).  A call folds in every stored step not yet folded, ascending; keep_history = 1, trace = 1 and at
 * least 2 steps done (not every step).  Fixed summation order (a function of N_P), fp64, no atomics; a column's value depends
 * neither on lag nor on moments nor on its place in the carry; a pair whose log omega lies below -746 contributes exactly 0.
 * Outputs (NULL pointers are skipped), T_done = the steps done: pages [((lag + 1) H + 1) x T_done], column t: est(0 .. lag, t)
 * (H values each, 0 where t - l < 0), then mass(t) (mass(1) = 1); means [7 x T_done] = c.                                          */
int rbpf_loc_fixed_lag_update(rbpf_ctx* ctx, int32_t lag, int32_t moments, double* pages, double* means);
/* Hands the carry back to the pool; the next update starts again at the first step.  No carry: nothing happens.                    */
int rbpf_loc_fixed_lag_reset(rbpf_ctx* ctx);
/* Bytes of device memory the carry holds while it lives (no device access).  With rows = n = 7, H as above, K = lag H, and C,
 * nchunks, P as at rbpf_loc_forward_stats_workspace_bytes, in doubles:
 *   (rows + 1) N_P                        the predecessors of a step
 * + 2 P                                   the normaliser pass's chunk partials
 * + 4 N_P                                 zeros, D, what the normaliser's merge writes next to D, reach
 * + nchunks (K + 1) N_P                   the carry pass's chunk partials
 * + 2 (K + H) N_P                         the carry, ping-pong
 * + N_T (K + H + 1)                       the pages
 * + N_T n                                 the filter means.                                                                       */
int rbpf_loc_fixed_lag_workspace_bytes(int32_t N_P, int32_t N_T, int32_t lag, int32_t moments, size_t* bytes);
/* One pass on the caller's arrays, the kernel-level probe: xn, logw, xs_next, odo, dt, Q as rbpf_loc_marginal_step; tau [K][N]
 * (column k contiguous over the particles), any K >= 1, the incoming columns -> D [M], tau_next [K][M], reach [M] = sum_i omega(i,
 * j).  *ms = median time of the normaliser pass and its merge, the carry pass, its merge, the enter kernel (with `moments`, on the
 * successors) and the reducers together (uniform weights); the outputs do not depend on moments.                                   */
int rbpf_loc_fixed_lag_step(int32_t N, int32_t M, int32_t K, int32_t moments, const double* xn, const double* logw, const double* xs_next,
                            const double* tau, const double* odo, double dt, const double* Q, double* D, double* tau_next, double* reach,
                            int32_t reps, double* ms);

/* ---- localisation in the fixed map of a generic device-code model --------------------------------
 * particleFilter.m:100-161 with the map frozen: xl = mean and P = V'V (V lower n_lin x n_lin, column-major, lower triangle read:
 * the rbpf_loc_map convention) are the same for every particle and never updated (:163-204 are left out).  The model is the
 * caller's device code, as for rbpf_filter_step_device: per step, with dy(i,:,:) = H_i [n_y x n_lin] from the caller's measModel,
 *     e_i = y_t' - H_i mean,   S_i = H_i P H_i' + R,   logw_i = -sum log diag chol S_i - |chol(S_i) \ e_i|^2 / 2 - n_y log(2 pi) / 2
 * (:139-150, a proper Gaussian; the jitter retry of :145-148 is left out: S_i is a Gram matrix plus R, and an R that is not
 * positive definite is RBPF_ERR_CHOL_FAILED at creation).  Normalisation, traj_max / traj_mean, the ancestors ai(i) = sample(w) on
 * the library's uniforms, xn_traj and log(sum(w)) are those of rbpf_loc_create's filter; dynModel draws its own normals (rng->Z is
 * not read).  n_y 1 .. 8, n_lin 1 .. 1151, n_nonlin 1 .. 8 (above: RBPF_ERR_UNSUPPORTED).  No new struct: the scalars and arrays
 * below, rbpf_rng, rbpf_options (keep_history, trace, on_step are read, any other non-zero field is RBPF_ERR_UNSUPPORTED) and
 * rbpf_loc_out, whose 7 rows are n_nonlin rows for such a context.  NULL arguments and bad sizes are refused before any device
 * is touched; without a device: RBPF_ERR_NO_DEVICE.
 *   rbpf_loc_generic_create   mean [n_lin], V, R [n_y x n_y] column-major, y [N_T x n_y] column-major, x0_nonlin
 *        [n_nonlin x x0_cols], x0_cols 1 or N_P.  rbpf_loc_finish, rbpf_loc_history, rbpf_filter_tell, rbpf_sync, rbpf_stream_get and
 *        rbpf_destroy work on the context; rbpf_loc_advance is RBPF_ERR_STATE (the handles are the caller's) and
 *        rbpf_loc_backward_simulate RBPF_ERR_UNSUPPORTED (it needs dynModel's transition density; a generic dynModel is a sampler).
 *        A caller that can state the density as Gaussian in a wrapped difference has the rbpf_loc_generic_backward_* entry points
 *        below; without one the refusal is the open end.
 *   rbpf_loc_generic_layout   ldx >= n_lin, the row stride of dy layout 1.
 *   rbpf_loc_generic_ancestors_device   before every step, in stream order on rbpf_stream_get(ctx): *xn_anc_dev
 *        [n_nonlin x N_P] column-major = the states of the resampled ancestors, xn_{t-1}(:, ai(i)), and *ai_dev [N_P] the 0-based
 *        ancestors; at t = 0 the initial states (x0_nonlin repeated) and *ai_dev = NULL.  Owned by the context, valid until the
 *        next step call.  RBPF_ERR_STATE after the last step.
 *   rbpf_loc_generic_step_device   xn_new_dev [n_nonlin x N_P] column-major = dynModel(xn_anc, ...) (t = 0: xn_anc itself),
 *        dy_dev = measModel(xn_new) in dy_layout 0 (MATLAB order, dy(i,k,c) at i + N_P*(k + n_y*c), packed by a kernel first),
 *        2 (C-contiguous [N_P][n_y][n_lin]) or 1 ([N_P][n_y][ldx] rows, consumed in place; columns n_lin .. ldx-1 are never
 *        read and may hold anything).  RBPF_ERR_STATE at t >= 1 without the ancestors call.  Returns without waiting unless an
 *        on_step hook is set (then: synchronise, call the hook; view->ctx is valid for rbpf_loc_finish).
 *   rbpf_loc_generic_weights   the weight kernel on its own, host arrays: dy for n_p particles in dy_layout (ldx: the row stride
 *        of layout 1, otherwise ignored), y [n_y] -> yhat [n_y x n_p] = H_i mean, S [n_y x n_y x n_p] = H_i P H_i' (before R is
 *        added), logw [n_p]; NULL outputs are skipped.  reps >= 1 repeats the launch; *ms (may be NULL) = median kernel time by
 *        device events.                                                                                                          */
int rbpf_loc_generic_create(int32_t n_nonlin, int32_t n_y, int32_t n_lin, const double* mean, const double* V, const double* R,
                            int32_t N_P, int32_t N_T, const double* y, const double* x0_nonlin, int32_t x0_cols,
                            const rbpf_rng* rng, const rbpf_options* opt, rbpf_ctx** ctx);
int rbpf_loc_generic_layout(const rbpf_ctx* ctx, int32_t* ldx);
int rbpf_loc_generic_ancestors_device(rbpf_ctx* ctx, const int32_t** ai_dev, const double** xn_anc_dev);
int rbpf_loc_generic_step_device(rbpf_ctx* ctx, const double* xn_new_dev, const double* dy_dev, int32_t dy_layout);
int rbpf_loc_generic_weights(int32_t n_y, int32_t n_lin, int32_t n_p, const double* dy, int32_t dy_layout, int32_t ldx,
                             const double* mean, const double* V, const double* R, const double* y, double* yhat, double* S,
                             double* logw, int32_t reps, double* ms);

/* ---- backward simulation in the fixed map of a generic device-code model: Gaussian transitions ----
 * The recursion of rbpf_loc_backward_simulate on a context of rbpf_loc_generic_create (keep_history = 1, trace = 1, every step
 * done, no degenerate forward step), for a dynModel that is a drift plus Gaussian noise on n_res of the n_nonlin rows:
 *     r = wrap(x'(rows) - mu_i),   z = L \ r  (L L' = cov, lower),   logp = -z'z / 2        (constants omitted, particleSmoother.m:181-182)
 * rows [n_res] 0-based, distinct, each < n_nonlin, n_res 1 .. 8; rows not listed take no part in the density.  Bit k of angle_mask
 * marks residual row k (state row rows[k]) as an angle: wrap(r) = r - 2 pi rint(r / (2 pi)), 2 pi the fp64 constant, applied before L.
 * mu_i = mean(X(:, i, t)) is the caller's device code, so the pass is driven step by step, t = N_T-1 .. 0:
 *   rbpf_loc_generic_backward_begin   takes the workspace from the context's pool; u [N_T x n_traj] (row t = step t) or NULL: Philox
 *        keyed by `seed` on the counters of rbpf_loc_backward_simulate.  RBPF_ERR_STATE: a pass is open already, steps missing, no
 *        keep_history / trace, a degenerate forward step.
 *   rbpf_loc_generic_backward_particles_device   *t = the step the next step call processes, *xn_dev = its stored particles
 *        [n_nonlin][N_P] (rows contiguous over the particles: a C-contiguous (n_nonlin, N_P) array), library memory, read only.
 *   rbpf_loc_generic_backward_step_device   mu_dev [n_res][N_P] on rbpf_stream_get(ctx), cov [n_res x n_res] on the host (symmetric;
 *        the lower triangle is read); both may be NULL at t = N_T-1, whose draw reads log w only.  With odometry row t, dt(t),
 *        Q(:,:,t): the arguments dynModel got when it made step t+1.  A cov that is not positive definite: RBPF_ERR_CHOL_FAILED, the
 *        step named, before anything is launched.  Enqueues prologue, all-pairs pass, locate and mean without waiting.
 *   rbpf_loc_generic_backward_finish   synchronises, copies out (NULL outputs are skipped) xs_traj [n_nonlin x n_traj x N_T],
 *        index [n_traj x N_T] 0-based, traj_smooth_mean [n_nonlin x N_T] (plain means of all rows) and returns the workspace.  With
 *        steps left undone it returns the workspace all the same: RBPF_OK when every output is NULL (the way out after a failed
 *        handle), RBPF_ERR_STATE otherwise.  rbpf_destroy releases an open pass too.
 *   rbpf_loc_generic_backward_workspace_bytes   what begin takes from the pool (no device access).
 *   rbpf_loc_generic_backward_step   one step on host arrays, the kernel-level probe: mu [n_res][N], w [N], xs_next [n_nonlin x M]
 *        column-major, cov [n_res x n_res], u [M] -> index [M]; logp [N x M] column-major (may be NULL) without log(w).  reps >= 1
 *        repeats the step's launches; *ms (may be NULL) = median time of one step by device events.
 * RBPF_ERR_STATE out of order (step without begin, begin twice, a step after the last); NULL arguments and bad sizes are
 * RBPF_ERR_INVALID_ARG before any device is touched; without a device RBPF_ERR_NO_DEVICE; the context stays usable after any
 * refusal.  rbpf_loc_backward_simulate keeps refusing a generic context.  Not built: densities that are neither Gaussian in a wrapped
 * difference nor the pose family below, n_res > 8, sharding.                                                                   */
int rbpf_loc_generic_backward_begin(rbpf_ctx* ctx, int32_t n_traj, const double* u, uint64_t seed, int32_t n_res, const int32_t* rows,
                                    uint32_t angle_mask);
int rbpf_loc_generic_backward_particles_device(rbpf_ctx* ctx, int32_t* t, const double** xn_dev);
int rbpf_loc_generic_backward_step_device(rbpf_ctx* ctx, const double* mu_dev, const double* cov);
int rbpf_loc_generic_backward_finish(rbpf_ctx* ctx, double* xs_traj, int32_t* index, double* traj_smooth_mean);
int rbpf_loc_generic_backward_workspace_bytes(int32_t n_nonlin, int32_t n_res, int32_t N_P, int32_t N_T, int32_t n_traj, size_t* bytes);
int rbpf_loc_generic_backward_step(int32_t N, int32_t M, int32_t n_nonlin, int32_t n_res, const int32_t* rows, uint32_t angle_mask,
                                   const double* mu, const double* w, const double* xs_next, const double* cov, const double* u,
                                   int32_t* index, double* logp, int32_t reps, double* ms);

/* ---- ... for pose states: a unit quaternion among the selected rows ----
 * The same pass for a dynModel whose state holds a unit quaternion (q0, q1, q2, q3), scalar first (tools/q*.m), with the noise
 * multiplied on the RIGHT of the predicted quaternion: x'_q = mu_q (x) expq(noise) (run_dense3D_magfield.m:202-203,
 * run_localization.m:274-281).  rows [n_sel] names the selected state rows, the four of the block adjacent and in order at
 * positions quat_pos .. quat_pos+3 of rows; the residual has n_res = n_sel - 1 entries, the block's place taken by three:
 *     e = qInv(mu_q) (x) x'_q,   e <- -e if e0 < 0 (tools/logq.m:26-28),   phi = atan2(|e_v|, e0) e_v / |e_v|,  0 if |e_v| = 0
 * (= logq(e) for a unit e), the other rows x'(rows[k]) - mu_k, wrapped where bit k of angle_mask is set: the bits index POSITIONS in
 * rows.  mu_dev / mu is [n_sel][N_P]: its block rows are the predicted unit quaternion, composed with the odometry by the caller.
 * cov [n_res x n_res] is in the caller's residual order (rows before the block, the block's three, rows behind it); the library
 * evaluates the residual with the plain rows first and the block last and permutes cov symmetrically on the host to that order.
 *   rbpf_loc_generic_backward_pose_begin   as _begin; then _particles_device, _step_device (mu_dev [n_sel][N_P]) and _finish as above.
 *   rbpf_loc_generic_backward_pose_workspace_bytes   what it takes from the pool: Xhat has n_sel + 1 rows.
 *   rbpf_loc_generic_backward_pose_step   the probe, mu [n_sel][N].
 * With quat_pos = -1 the three are rbpf_loc_generic_backward_begin / _workspace_bytes / _step (n_sel = n_res), result for result.
 * RBPF_ERR_INVALID_ARG, each with its message: a block that is not inside rows (quat_pos < -1 or >= n_sel), one that runs past
 * n_sel, one that overlaps an angle bit, n_sel - 1 > 8.  One block, 0 .. 4 plain rows (n_sel 4 .. 8).  Not built: noise multiplied
 * on the left, two blocks, noise through a non-square G.                                                                         */
int rbpf_loc_generic_backward_pose_begin(rbpf_ctx* ctx, int32_t n_traj, const double* u, uint64_t seed, int32_t n_sel, const int32_t* rows,
                                         uint32_t angle_mask, int32_t quat_pos);
int rbpf_loc_generic_backward_pose_workspace_bytes(int32_t n_nonlin, int32_t n_sel, int32_t quat_pos, int32_t N_P, int32_t N_T,
                                                   int32_t n_traj, size_t* bytes);
int rbpf_loc_generic_backward_pose_step(int32_t N, int32_t M, int32_t n_nonlin, int32_t n_sel, const int32_t* rows, uint32_t angle_mask,
                                        int32_t quat_pos, const double* mu, const double* w, const double* xs_next, const double* cov,
                                        const double* u, int32_t* index, double* logp, int32_t reps, double* ms);

/* ---- the MAP trajectory in the fixed map of a generic device-code model ----
 * The recursion of rbpf_loc_map_trajectory on a context of rbpf_loc_generic_create or rbpf_loc_landmark_create (the pass never reads
 * the map), with the transition density of rbpf_loc_generic_backward_pose_begin: n_sel, rows, angle_mask, quat_pos as there,
 * quat_pos = -1 for a density without a quaternion block (n_sel = n_res).  It runs FORWARDS in time, t = 0 .. N_T-2:
 *   rbpf_loc_generic_map_begin   takes the workspace from the context's pool and enqueues delta of step 0.  The argument checks
 *        of _pose_begin; RBPF_ERR_STATE: a MAP pass or a backward pass is open (the two cannot be open at once; _backward_begin
 *        refuses likewise while a MAP pass is open), steps missing, no keep_history / trace, a degenerate forward step.
 *   rbpf_loc_generic_map_particles_device   *t = the step the next step call processes, *xn_dev = its stored particles
 *        [n_nonlin][N_P], library memory, read only.
 *   rbpf_loc_generic_map_step_device   mu_dev [n_sel][N_P] = mean of the particles of step t on rbpf_stream_get(ctx), cov
 *        [n_res x n_res] on the host, with odometry row t, dt(t), Q(:,:,t): what the backward pass gets for the same t.  A cov that
 *        is not positive definite: RBPF_ERR_CHOL_FAILED, the step named, before anything is launched.  Enqueues prologue, all-pairs
 *        pass and merge (delta and psi of step t+1) without waiting.
 *   rbpf_loc_generic_map_finish   backtracks, synchronises, copies out (NULL outputs are skipped) x_map [n_nonlin x N_T], index
 *        [N_T] 0-based, *score, and returns the workspace.  With steps left undone it returns the workspace all the same: RBPF_OK
 *        when every output is NULL (the way out after a failed handle), RBPF_ERR_STATE otherwise.  rbpf_destroy releases an open
 *        pass too.
 *   rbpf_loc_generic_map_workspace_bytes   what begin takes from the pool (no device access): Xhat has n_sel + 1 rows.
 *   rbpf_loc_generic_map_step   one step on host arrays, the kernel-level probe: mu [n_sel][N], delta [N], xs_next [n_nonlin x M]
 *        column-major, cov [n_res x n_res] -> best [M], arg [M] as rbpf_loc_map_step.
 * RBPF_ERR_STATE out of order (step without begin, begin twice, a step after the last); the context stays usable after any
 * refusal.  Not built: sharding, host closures, N-best paths, other successors than the N_P particles outside the probe.           */
int rbpf_loc_generic_map_begin(rbpf_ctx* ctx, int32_t n_sel, const int32_t* rows, uint32_t angle_mask, int32_t quat_pos);
int rbpf_loc_generic_map_particles_device(rbpf_ctx* ctx, int32_t* t, const double** xn_dev);
int rbpf_loc_generic_map_step_device(rbpf_ctx* ctx, const double* mu_dev, const double* cov);
int rbpf_loc_generic_map_finish(rbpf_ctx* ctx, double* x_map, int32_t* index, double* score);
int rbpf_loc_generic_map_workspace_bytes(int32_t n_nonlin, int32_t n_sel, int32_t quat_pos, int32_t N_P, int32_t N_T, size_t* bytes);
int rbpf_loc_generic_map_step(int32_t N, int32_t M, int32_t n_nonlin, int32_t n_sel, const int32_t* rows, uint32_t angle_mask,
                              int32_t quat_pos, const double* mu, const double* delta, const double* xs_next, const double* cov,
                              double* best, int32_t* arg, int32_t reps, double* ms);

/* ---- the marginal smoothing weights in the fixed map of a generic device-code model ----
 * The recursion of rbpf_loc_marginal_smooth on a context of rbpf_loc_generic_create or rbpf_loc_landmark_create (the pass never
 * reads the map), with the transition density of rbpf_loc_generic_backward_pose_begin: n_sel, rows, angle_mask, quat_pos as there,
 * quat_pos = -1 for a density without a quaternion block.  It runs BACKWARDS in time, t = N_T-2 .. 0, as the backward pass does:
 *   rbpf_loc_generic_marginal_begin   takes the workspace from the context's pool and enqueues step N_T-1 (ws = w, its moments).
 *        The argument checks of _pose_begin; RBPF_ERR_STATE: a marginal, MAP or backward pass is open (only one of the three can
 *        be open at once; _backward_begin and _map_begin refuse likewise while a marginal pass is open), steps missing, no
 *        keep_history / trace, a degenerate forward step.
 *   rbpf_loc_generic_marginal_particles_device   *t = the step the next step call processes, *xn_dev = its stored particles
 *        [n_nonlin][N_P], library memory, read only.
 *   rbpf_loc_generic_marginal_step_device   mu_dev [n_sel][N_P] = mean of the particles of step t on rbpf_stream_get(ctx), cov
 *        [n_res x n_res] on the host, with odometry row t, dt(t), Q(:,:,t).  A cov that is not positive definite:
 *        RBPF_ERR_CHOL_FAILED, the step named, before anything is launched.  Enqueues prologue, the two all-pairs passes, their
 *        merges, the normalisation and the moments of step t without waiting.
 *   rbpf_loc_generic_marginal_finish   synchronises, copies out (NULL outputs are skipped) w_smooth [N_P x N_T], mean [n_nonlin x
 *        N_T], cov [n_nonlin x n_nonlin x N_T], ess [N_T], mass [N_T], and returns the workspace.  With steps left undone it
 *        returns the workspace all the same: RBPF_OK when every output is NULL (the way out after a failed handle), RBPF_ERR_STATE
 *        otherwise.  rbpf_destroy releases an open pass too.  mean and cov are plain weighted moments of all n_nonlin rows: angle
 *        and quaternion rows get no special handling.
 *   rbpf_loc_generic_marginal_workspace_bytes   what begin takes from the pool (no device access): Xhat has n_sel + 1 rows.
 *   rbpf_loc_generic_marginal_step   one step on host arrays, the kernel-level probe: mu [n_sel][N], logw [N], xs_next [n_nonlin x
 *        M] column-major, logws_next [M], cov [n_res x n_res] -> D [M], lws [N] as rbpf_loc_marginal_step.
 * RBPF_ERR_STATE out of order; the context stays usable after any refusal.  Not built: sharding, host closures, other
 * successors than the N_P particles outside the probe, sub-quadratic approximations.  (The two-slice moments of the transition
 * residual: rbpf_loc_generic_pair_stats_* below.)                                                                                 */
int rbpf_loc_generic_marginal_begin(rbpf_ctx* ctx, int32_t n_sel, const int32_t* rows, uint32_t angle_mask, int32_t quat_pos);
int rbpf_loc_generic_marginal_particles_device(rbpf_ctx* ctx, int32_t* t, const double** xn_dev);
int rbpf_loc_generic_marginal_step_device(rbpf_ctx* ctx, const double* mu_dev, const double* cov);
int rbpf_loc_generic_marginal_finish(rbpf_ctx* ctx, double* w_smooth, double* mean, double* cov, double* ess, double* mass);
int rbpf_loc_generic_marginal_workspace_bytes(int32_t n_nonlin, int32_t n_sel, int32_t quat_pos, int32_t N_P, int32_t N_T, size_t* bytes);
int rbpf_loc_generic_marginal_step(int32_t N, int32_t M, int32_t n_nonlin, int32_t n_sel, const int32_t* rows, uint32_t angle_mask,
                                   int32_t quat_pos, const double* mu, const double* logw, const double* xs_next, const double* logws_next,
                                   const double* cov, double* D, double* lws, int32_t reps, double* ms);

/* ---- the two-slice statistics of the transition residual in the fixed map of a generic device-code model ----
 * The statistics of rbpf_loc_pair_stats_smooth on a context of rbpf_loc_generic_create or rbpf_loc_landmark_create, driven exactly
 * as the rbpf_loc_generic_marginal_* family is (same arguments, checks and refusals; a statistics pass counts as a fourth kind of
 * pass, and only one of the four can be open at once).  r is the un-whitened residual of rbpf_loc_generic_backward_pose_begin's
 * density: a wrapped difference on plain and angle rows, logq of the quaternion error in a block.  _finish returns the five outputs
 * of _marginal_finish and S [n_res x n_res x (N_T-1)], m [n_res x (N_T-1)], pair_mass [N_T-1] in the CALLER's residual order (the
 * order of cov).  _step is the probe: the arguments of rbpf_loc_generic_marginal_step, then S [n_res x n_res], m [n_res],
 * pair_mass [1].                                                                                                                */
int rbpf_loc_generic_pair_stats_begin(rbpf_ctx* ctx, int32_t n_sel, const int32_t* rows, uint32_t angle_mask, int32_t quat_pos);
int rbpf_loc_generic_pair_stats_particles_device(rbpf_ctx* ctx, int32_t* t, const double** xn_dev);
int rbpf_loc_generic_pair_stats_step_device(rbpf_ctx* ctx, const double* mu_dev, const double* cov);
int rbpf_loc_generic_pair_stats_finish(rbpf_ctx* ctx, double* w_smooth, double* mean, double* cov, double* ess, double* mass, double* S,
                                       double* m, double* pair_mass);
int rbpf_loc_generic_pair_stats_workspace_bytes(int32_t n_nonlin, int32_t n_sel, int32_t quat_pos, int32_t N_P, int32_t N_T, size_t* bytes);
int rbpf_loc_generic_pair_stats_step(int32_t N, int32_t M, int32_t n_nonlin, int32_t n_sel, const int32_t* rows, uint32_t angle_mask,
                                     int32_t quat_pos, const double* mu, const double* logw, const double* xs_next, const double* logws_next,
                                     const double* cov, double* D, double* lws, double* S, double* m, double* pair_mass, int32_t reps,
                                     double* ms);

/* ---- running two-slice statistics in the fixed map of a generic device-code model ----------------------
 * The statistics of rbpf_loc_forward_stats_update on a context of rbpf_loc_generic_create or rbpf_loc_landmark_create, driven as
 * the rbpf_loc_generic_pair_stats_* family is (same rows, angle_mask, quat_pos, checks; mu and cov for every step; the library names
 * the step), but FORWARDS: the steps ascend from the first pair not yet folded in, t = folded .. T_done-2, and not every step of
 * the run has to be done (at least 2).  _step_device takes s_scale = 1 / dt(t) next to cov: what the S part of the functional is
 * scaled by (the library does not know dt).  The carry is persistent state of the context as in the dense-mag map; _begin takes it
 * at the first call, and with other rows than the carry was built with it is refused (RBPF_ERR_STATE: _reset first).  Between _begin
 * and _finish the stepping counts as a fifth kind of open pass: only one of the five can be open at once.  _finish closes the
 * stepping and keeps the carry: with every stored pair folded it returns S_run [n_res x n_res x (T_done-1)], m_run [n_res x
 * (T_done-1)], mass_run [T_done-1], tau_S [n_res x n_res x N_P], tau_m [n_res x N_P] in the CALLER's residual order (NULL pointers
 * are skipped); with pairs left (a handle failed) it refuses unless every pointer is NULL, and the carry stays where the last
 * complete step put it: a later _begin resumes there.  _reset (not while the stepping is open) hands the carry back.
 * _workspace_bytes: the sum stated at rbpf_loc_forward_stats_workspace_bytes with rows = n_sel and n_res = n_sel (n_sel - 1 with a
 * quaternion block).  _step is the probe: the arguments of rbpf_loc_generic_marginal_step without logws_next, the incoming carry
 * and s_scale -> D [M], tau_S_next [n_res x n_res x M], tau_m_next [n_res x M], reach [M].                                          */
int rbpf_loc_generic_forward_stats_begin(rbpf_ctx* ctx, int32_t n_sel, const int32_t* rows, uint32_t angle_mask, int32_t quat_pos);
int rbpf_loc_generic_forward_stats_particles_device(rbpf_ctx* ctx, int32_t* t, const double** xn_dev);
int rbpf_loc_generic_forward_stats_step_device(rbpf_ctx* ctx, const double* mu_dev, const double* cov, double s_scale);
int rbpf_loc_generic_forward_stats_finish(rbpf_ctx* ctx, double* S_run, double* m_run, double* mass_run, double* tau_S, double* tau_m);
int rbpf_loc_generic_forward_stats_reset(rbpf_ctx* ctx);
int rbpf_loc_generic_forward_stats_workspace_bytes(int32_t n_nonlin, int32_t n_sel, int32_t quat_pos, int32_t N_P, int32_t N_T, size_t* bytes);
int rbpf_loc_generic_forward_stats_step(int32_t N, int32_t M, int32_t n_nonlin, int32_t n_sel, const int32_t* rows, uint32_t angle_mask,
                                        int32_t quat_pos, const double* mu, const double* logw, const double* xs_next, const double* tau_S,
                                        const double* tau_m, const double* cov, double s_scale, double* D, double* tau_S_next,
                                        double* tau_m_next, double* reach, int32_t reps, double* ms);

/* ---- fixed-lag smoothing in the fixed map of a generic device-code model --------------------------------
 * The estimates of rbpf_loc_fixed_lag_update on a context of rbpf_loc_generic_create or rbpf_loc_landmark_create, over all n =
 * n_nonlin state rows, driven as the rbpf_loc_generic_forward_stats_* family is: FORWARDS, t = (steps folded) - 1 .. T_done-2, mu
 * and cov for every step, the library names the step; not every step of the run has to be done (at least 2).  _begin takes the
 * carry at the first call, which fixes lag, moments and the rows; with others it is refused (RBPF_ERR_STATE: _reset first).
 * Between _begin and _finish the stepping counts as a sixth kind of open pass: only one of the six can be open at once.  _finish
 * closes the stepping and keeps the carry: with every stored step folded it returns pages and means [n_nonlin x T_done] as
 * rbpf_loc_fixed_lag_update does (NULL pointers are skipped); with steps left (a handle failed) it refuses unless both pointers are
 * NULL, and the carry stays where the last complete step put it: a later _begin resumes there.  _reset (not while the stepping is
 * open) hands the carry back.  _workspace_bytes: the sum stated at rbpf_loc_fixed_lag_workspace_bytes with rows = n_sel and n =
 * n_nonlin.  _step is the probe: the arguments of rbpf_loc_generic_marginal_step without logws_next, K, moments and tau [K][N] ->
 * D [M], tau_next [K][M], reach [M].                                                                                              */
int rbpf_loc_generic_fixed_lag_begin(rbpf_ctx* ctx, int32_t n_sel, const int32_t* rows, uint32_t angle_mask, int32_t quat_pos, int32_t lag,
                                     int32_t moments);
int rbpf_loc_generic_fixed_lag_particles_device(rbpf_ctx* ctx, int32_t* t, const double** xn_dev);
int rbpf_loc_generic_fixed_lag_step_device(rbpf_ctx* ctx, const double* mu_dev, const double* cov);
int rbpf_loc_generic_fixed_lag_finish(rbpf_ctx* ctx, double* pages, double* means);
int rbpf_loc_generic_fixed_lag_reset(rbpf_ctx* ctx);
int rbpf_loc_generic_fixed_lag_workspace_bytes(int32_t n_nonlin, int32_t n_sel, int32_t quat_pos, int32_t N_P, int32_t N_T, int32_t lag,
                                               int32_t moments, size_t* bytes);
int rbpf_loc_generic_fixed_lag_step(int32_t N, int32_t M, int32_t K, int32_t moments, int32_t n_nonlin, int32_t n_sel, const int32_t* rows,
                                    uint32_t angle_mask, int32_t quat_pos, const double* mu, const double* logw, const double* xs_next,
                                    const double* tau, const double* cov, double* D, double* tau_next, double* reach, int32_t reps,
                                    double* ms);

/* ---- backward simulation by rejection sampling, in every fixed map -----------------------------------
 * The law of rbpf_loc_backward_simulate / rbpf_loc_generic_backward_*, drawn without the all-pairs pass where a proposal is
 * accepted (Douc, Garivier, Moulines & Olsson 2011): every transition density here has logp = -z'z / 2 <= 0.  Step N_T-1 is the
 * draw of the all-pairs calls.  For t = N_T-2 .. 0 and trajectory j, tries r = 0 .. max_tries-1:
 *     (u0, u1) = Philox(seed; slot = j, step = t, lane = 0x42530001, iter = r),  i = #{k : cdf_k < u0 cdf_{N-1}} (cdf: the inclusive
 *     prefix sums of w[t], fp64, in an order fixed by N_P),  accept iff logp(xs[t+1][j] | X[t][:, i]) >= log u1  (no log w_i: the
 *     weights are the proposal);  the first accepted i is index[t][j].
 * Trajectories without an acceptance are drawn by the all-pairs pass with their uniform of the all-pairs calls (lane 0x42530000),
 * compacted in ascending j into M' rows, with the chunk size and summation order of (N_P, M'); M' comes to the host once per step.
 * The law of every index is the backward kernel's for every max_tries; max_tries = 0 gives the arrays of the all-pairs calls with
 * the same seed bit for bit.  The device generator only: the probes take uniforms.  Refusals as the all-pairs calls, and
 * max_tries outside 0 .. 4194304 is RBPF_ERR_INVALID_ARG.
 *   rbpf_loc_backward_simulate_reject   the dense-mag map; outputs as rbpf_loc_backward_simulate, and (either may be NULL)
 *        n_fallback [N_T] = M' of every step and n_tries [N_T] = the tries of every step summed over the trajectories (both 0 at
 *        step N_T-1).
 *   rbpf_loc_generic_backward_reject_begin   opens the pass on a generic or landmark-map context; rbpf_loc_generic_backward_
 *        particles_device / _step_device / _finish drive it as they drive rbpf_loc_generic_backward_pose_begin's (each _step_device
 *        below N_T-1 waits for the stream once).  rbpf_loc_generic_backward_reject_stats: the two counters of the last pass that
 *        _finish closed with every step done (RBPF_ERR_STATE if there is none).
 *   *_reject_workspace_bytes   device bytes of a pass (no device access).
 *   rbpf_loc_backward_reject_step, rbpf_loc_generic_backward_reject_step   one step on host arrays, the kernel-level probes: the
 *        arguments of rbpf_loc_backward_step / rbpf_loc_generic_backward_pose_step without logp, and u_try [R][M][2] (try r of
 *        trajectory j: u0 at [r][j][0], u1 at [r][j][1]; NULL: the device generator's draws of seed 0 at step 0, for timing runs
 *        whose R x M uniforms would not fit a host array), u [M] the fallback's uniforms, R = max_tries ->
 *        index [M], accepted_at [M] (the try that was accepted, -1: fallback; may be NULL); ms: median over reps of the whole step. */
int rbpf_loc_backward_simulate_reject(rbpf_ctx* ctx, int32_t n_traj, uint64_t seed, int32_t max_tries, double* xs_traj, int32_t* index,
                                      double* traj_smooth_mean, int32_t* n_fallback, int64_t* n_tries);
int rbpf_loc_backward_reject_workspace_bytes(int32_t N_P, int32_t N_T, int32_t n_traj, size_t* bytes);
int rbpf_loc_backward_reject_step(int32_t N, int32_t M, const double* xn, const double* w, const double* xs_next, const double* odo, double dt,
                                  const double* Q, const double* u_try, const double* u, int32_t R, int32_t* index, int32_t* accepted_at,
                                  int32_t reps, double* ms);
int rbpf_loc_generic_backward_reject_begin(rbpf_ctx* ctx, int32_t n_traj, uint64_t seed, int32_t max_tries, int32_t n_sel, const int32_t* rows,
                                           uint32_t angle_mask, int32_t quat_pos);
int rbpf_loc_generic_backward_reject_stats(rbpf_ctx* ctx, int32_t* n_fallback, int64_t* n_tries);
int rbpf_loc_generic_backward_reject_workspace_bytes(int32_t n_nonlin, int32_t n_sel, int32_t quat_pos, int32_t N_P, int32_t N_T, int32_t n_traj,
                                                     size_t* bytes);
int rbpf_loc_generic_backward_reject_step(int32_t N, int32_t M, int32_t n_nonlin, int32_t n_sel, const int32_t* rows, uint32_t angle_mask,
                                          int32_t quat_pos, const double* mu, const double* w, const double* xs_next, const double* cov,
                                          const double* u_try, const double* u, int32_t R, int32_t* index, int32_t* accepted_at, int32_t reps,
                                          double* ms);

/* ---- localisation in the fixed landmark map of a generic device-code model ------------------------
 * The frozen-map filter above for a model of the sparseFeatures branch (particleFilter.m:100-161 with :127-137): the map posterior
 * N(mean, V'V), V lower, is shared by all particles and never updated, and the caller's measModel(xn, xl) returns the prediction
 * yhat_i [n_y] (nonlinear in the map) next to H_i = dy(i,:,:) [n_y x n_lin].  Per step t, ind = ~isnan(y(t,:)), M = |ind|:
 *     e_i = y_t(ind)' - yhat_i(ind),   S_i = H_i(ind,:) P H_i(ind,:)' + R(ind,ind),
 *     logw_i = -sum log diag chol S_i - |chol(S_i) \ e_i|^2 / 2 - M log(2 pi) / 2                          (:129-136,145-150)
 * mean is not read by the weight kernel.  Rows of yhat / dy that belong to outputs not observed at a step are never read; they may
 * hold anything, NaN included.  M = 0: every log-weight is 0, the weights 1 / N_P.  The jitter retry of :145-148 is left out: S_i is
 * a Gram matrix plus a principal submatrix of R, and an R that is not symmetric positive definite is RBPF_ERR_CHOL_FAILED at
 * creation.  Everything after the weights is the generic localisation context's.  n_y 1 .. 32, n_lin 1 .. 96, n_nonlin 1 .. 8 (the
 * limits of the SLAM branch; above: RBPF_ERR_UNSUPPORTED); one GPU, fp64.  NULL arguments and bad sizes are RBPF_ERR_INVALID_ARG
 * before any device is touched; without a device: RBPF_ERR_NO_DEVICE.
 *   rbpf_loc_landmark_create   arguments as rbpf_loc_generic_create; y [N_T x n_y] column-major, NaN = not observed.  The context is
 *        a generic localisation context: rbpf_loc_finish, rbpf_loc_history, rbpf_filter_tell, rbpf_sync, rbpf_stream_get,
 *        rbpf_destroy, rbpf_loc_generic_layout, rbpf_loc_generic_ancestors_device and all of rbpf_loc_generic_backward_* work on it
 *        unchanged; rbpf_loc_advance is RBPF_ERR_STATE, rbpf_loc_backward_simulate RBPF_ERR_UNSUPPORTED, options other than
 *        keep_history, trace, on_step RBPF_ERR_UNSUPPORTED, and rbpf_loc_generic_step_device RBPF_ERR_STATE (it has no yhat).
 *   rbpf_loc_landmark_map_device   *xl_dev [N_P][ldx]: every row = mean, columns n_lin .. ldx-1 zero: the shape
 *        rbpf_filter_sparse_gathered_device hands out, so a handle written for the SLAM filter runs unchanged.  Owned by the
 *        context, constant for its life.
 *   rbpf_loc_landmark_step_device   xn_new_dev as in rbpf_loc_generic_step_device; yhat / dy layouts as in
 *        rbpf_filter_step_sparse_device: yhat 0 (yhat(i,k) at i + N_P*k) or 2 ([N_P][n_y]); dy 0 (MATLAB order, packed by a kernel
 *        first), 1 ([N_P][n_y][ldx] rows; what stands in columns n_lin .. ldx-1 never enters a result) or 2 ([N_P][n_y][n_lin]).
 *        RBPF_ERR_STATE at t >= 1 without rbpf_loc_generic_ancestors_device, and after the last step.  Returns without waiting
 *        unless an on_step hook is set.
 *   rbpf_loc_landmark_yhattraj   yhattraj [n_y x N_T] column-major: column t is the whole yhat of step t's maximum-weight particle
 *        as the caller handed it in, NaN for steps not yet run.  Waits for the stream.
 *   rbpf_loc_landmark_weights   the weight kernel on its own, host arrays: yhat and dy for n_p particles in their layouts (ldx: the
 *        row stride of dy layout 1, otherwise ignored), y [n_y] with NaN = not observed -> S [M x M x n_p] column-major =
 *        H_i(ind,:) P H_i(ind,:)' in ascending output order, before R is added, logw [n_p]; NULL outputs are skipped.  reps >= 1
 *        repeats the launch; *ms (may be NULL) = median kernel time by device events.
 * Not built: host closures, the MEX gateway, sharding, n_lin > 96, n_y > 32.                                                      */
int rbpf_loc_landmark_create(int32_t n_nonlin, int32_t n_y, int32_t n_lin, const double* mean, const double* V, const double* R,
                             int32_t N_P, int32_t N_T, const double* y, const double* x0_nonlin, int32_t x0_cols,
                             const rbpf_rng* rng, const rbpf_options* opt, rbpf_ctx** ctx);
int rbpf_loc_landmark_map_device(rbpf_ctx* ctx, const double** xl_dev, int32_t* ldx);
int rbpf_loc_landmark_step_device(rbpf_ctx* ctx, const double* xn_new_dev, const double* yhat_dev, int32_t yhat_layout,
                                  const double* dy_dev, int32_t dy_layout);
int rbpf_loc_landmark_yhattraj(rbpf_ctx* ctx, double* yhattraj);
int rbpf_loc_landmark_weights(int32_t n_y, int32_t n_lin, int32_t n_p, const double* yhat, int32_t yhat_layout, const double* dy,
                              int32_t dy_layout, int32_t ldx, const double* V, const double* R, const double* y, double* S,
                              double* logw, int32_t reps, double* ms);

/* ---- the EKF comparison baseline of examples/slam-dense-mag, batched over data sets ---------------
 * ekf_dense.m:41-102 with the closures measModel_ekf / dynModel_ekf of run_dense3D_magfield.m:281-299,310-316, on the device:
 * one Gaussian state [position(3); orientation deviation(3); map(nLin = m_basis + 3)], n = 6 + nLin, per run.  The n_runs runs
 * of a call are independent (the Monte-Carlo protocol of main.m:37-57 has 80) and a run's results are bit-identical alone and
 * at any position of a batch.  Arrays carry the run as their slowest axis; within a run the conventions of rbpf_problem hold.
 * These structs are additions to ABI 9: each starts with its own struct_size (0 is accepted as in rbpf_options).            */
typedef struct {
  int32_t struct_size;       /* sizeof(rbpf_ekf_problem) = rbpf_abi_sizeof(12)                           */
  int32_t n_runs;            /* B >= 1                                                                   */
  int32_t N_T;               /* time steps = size(y,1), the same for every run                           */
  int32_t q_pages;           /* 1 or >= N_T-1  (ekf_dense.m:47-49)                                       */
  int32_t dt_len;            /* 1 or >= N_T-1  (:52-54)                                                  */
  int32_t odo_ld;            /* leading dimension of each run's odometry                                 */
  int32_t keep_P;            /* 0: rbpf_ekf_out.Pf is the final covariance; 1: the covariance of every step */
  const rbpf_model* const* models; /* [n_runs] dense-mag models with one m_basis; pointers may repeat    */
  const double* odometry;    /* [odo_ld x 7 x n_runs], odo_ld >= N_T-1                                   */
  const double* y;           /* [N_T x 3 x n_runs]                                                       */
  const double* x0;          /* [n x n_runs]                                                             */
  const double* q0;          /* [4 x n_runs]                                                             */
  const double* P0;          /* [n x n x n_runs], symmetric                                              */
  const double* R;           /* [3 x 3 x n_runs]                                                         */
  const double* LL;          /* [2 x 3 x n_runs] domain bounds (lower; upper) handed to JacobianPhi3D (:292) */
  const double* Q;           /* [6 x 6 x q_pages], shared by the runs                                    */
  const double* dt;          /* [dt_len], shared by the runs                                             */
} rbpf_ekf_problem;

/* NULL pointers are skipped. */
typedef struct {
  int32_t struct_size;       /* sizeof(rbpf_ekf_out) = rbpf_abi_sizeof(13)                               */
  int32_t reserved;
  double* xf_traj;           /* [n x N_T x n_runs]                                                       */
  double* qnb_traj;          /* [4 x N_T x n_runs]                                                       */
  double* Pf;                /* keep_P = 0: [n x n x n_runs]; keep_P = 1: Pf_traj [n x n x N_T x n_runs]  */
} rbpf_ekf_out;

/* One shot.  Of `opt` (may be NULL) only struct_size is read.  A model of another family: RBPF_ERR_UNSUPPORTED; models of
 * different m_basis, nLin outside 4 .. 1151 or an unsymmetric P0: RBPF_ERR_INVALID_ARG; a workspace that does not fit the
 * device: RBPF_ERR_OUT_OF_MEMORY before anything is launched; an innovation covariance that fails its factorisation with and
 * without the jitter of ekf_dense.m:83-86 in any run: RBPF_ERR_CHOL_FAILED (no output is written).                          */
int rbpf_ekf_dense(const rbpf_ekf_problem* prob, const rbpf_options* opt, rbpf_ekf_out* out);
/* Bytes of device memory such a call needs, the keep_P = 1 history included (no device access).                             */
int rbpf_ekf_workspace_bytes(const rbpf_ekf_problem* prob, const rbpf_options* opt, size_t* bytes);

#ifdef __cplusplus
}
#endif
#endif /* RBPF_H_ */
