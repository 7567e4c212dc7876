"""Host-side mirror of the reference's MATLAB interface, driving the HIP library through the C ABI.

The reference's estimators are MATLAB functions taking function handles:

    particleFilter(dynModel,measModel,odometry,y,x0_nonLin,x0_lin,P0_lin,Q,R,N_P,dt,sparseFeatures,makePlots)
        (src/particleFilter.m:1-3)
    particleSmoother(dynModel,measModel,dynResNorm,odometry,y,x0_nonLin,x0_lin,P0_lin,Q,R,N_P,N_K,dt,
        sparseFeatures,makePlots)                                     (src/particleSmoother.m:1-2)
    particleSmootherInformationForm(... same ...)   (src/particleSmootherInformationForm.m:1-2)

MATLAB is not available on the build / GPU machines, so this module keeps the same names, argument
order and meaning in Python.  Handles cannot cross the C ABI; the closures of the example runners are
represented by model-family objects (`DenseMagModel`, `DenseRadioModel`) whose bound methods
`dynModel` / `measModel` / `dynResNorm` are *recognised* by the estimators (exactly what the MATLAB
wrappers in matlab/ do with func2str) and turned into an `rbpf_model` descriptor.  All arithmetic of
the hot path runs in the HIP kernels; nothing here computes filter results on the CPU and nothing
imports oracle/.

MATLAB's global RNG stream (`rand` in tools/sample.m:31, `randn` inside dynModel) is replaced by an
explicit `rng=` keyword: `ReplayRNG(U, Z, Ufin)` (seed-exact parity) or `PhiloxRNG(seed)` (device
counter-based generator, the default).
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np

from . import _ffi
from ._ffi import RBPFError, check, load_library


# ------------------------------------------------------------------------------------------------
# basis set-up (host logic, once per run): tools/domain_cartesian_dx.m:26-51
# ------------------------------------------------------------------------------------------------
def domain_cartesian_dx(m: int, d: int, LL):
    """Index selection of the reduced-rank GP basis.  Returns (L, NN): half-widths [d] and the
    m x d table of the m smallest Dirichlet-Laplacian eigen-indices (stable ascending sort,
    first axis slowest in the enumeration -- tools/domain_cartesian_dx.m:33-43,195-216)."""
    LL = np.atleast_2d(np.asarray(LL, dtype=np.float64))
    L = (LL.max(axis=0) - LL.min(axis=0)) / 2.0 if LL.shape[0] > 1 else LL.ravel().copy()
    if L.size != d:
        raise ValueError("LL must have d columns")
    counts = np.ceil(m ** (1.0 / d) * L / L.min()).astype(np.int64)
    axes = [np.arange(1, c + 1, dtype=np.int64) for c in counts]
    grid = np.stack([g.ravel() for g in np.meshgrid(*axes, indexing="ij")], axis=1)
    lam = eigenval(grid, L)
    order = np.argsort(lam, kind="stable")[:m]
    return L, grid[order].astype(np.int32)


def eigenval(NN, L):
    """tools/domain_cartesian_dx.m:40."""
    return np.sum((np.pi * np.asarray(NN, dtype=np.float64) / (2.0 * np.asarray(L, dtype=np.float64))) ** 2, axis=1)


# ------------------------------------------------------------------------------------------------
# model families
# ------------------------------------------------------------------------------------------------
class _Handle:
    """Stands in for a MATLAB function handle of a recognised model family."""

    def __init__(self, model, role):
        self.model = model
        self.role = role

    def __call__(self, *args):
        return self.model._evaluate(self.role, *args)

    def __repr__(self):
        return f"<{type(self.model).__name__}.{self.role} handle>"


class _ModelFamily:
    kind = 0
    nNonLin = 0
    ny = 0
    nw = 0
    n_odo = 0
    dim = 0

    def __init__(self, NN, L):
        self.NN = np.ascontiguousarray(np.asarray(NN, dtype=np.int32))
        self.L = np.asarray(L, dtype=np.float64).ravel().copy()
        if self.NN.ndim != 2 or self.NN.shape[1] != self.dim or self.L.size != self.dim:
            raise ValueError(f"NN must be m x {self.dim} and L length {self.dim}")
        self.dynModel = _Handle(self, "dynModel")
        self.measModel = _Handle(self, "measModel")
        self.dynResNorm = _Handle(self, "dynResNorm")

    @property
    def m(self):
        return self.NN.shape[0]

    def descriptor(self, use_dyn_res_norm=True):
        d = _ffi.rbpf_model()
        d.kind = self.kind
        d.m_basis = self.m
        d.dim = self.dim
        d.use_dyn_res_norm = 1 if use_dyn_res_norm else 0
        self._nn_f = np.asfortranarray(self.NN)                 # [m x dim] column-major, kept alive
        d.NN = self._nn_f.ctypes.data_as(_ffi.c_int32_p)
        for a in range(3):
            d.L[a] = float(self.L[a]) if a < self.dim else 0.0
        return d

    # Device evaluation of the closures (used when a handle is *called* from Python, e.g. by
    # data-generation code or tests).  Randomness is injected as the last argument of dynModel.
    def _evaluate(self, role, *args):
        lib = load_library()
        if role == "measModel":
            xn = np.asfortranarray(np.asarray(args[0], dtype=np.float64).reshape(self.nNonLin, -1))
            npred = xn.shape[1]
            dy = np.empty((self.ny, self.nLin, npred), dtype=np.float64, order="F")
            check(lib.rbpf_meas_model(C.byref(self.descriptor()), self.nNonLin, npred, _dp(xn), _dp(dy)))
            out = np.transpose(dy, (2, 0, 1))                   # [Npred x ny x nLin] as in the reference
            return out[:, 0, :] if self.ny == 1 else out        # 2-D for ny = 1 (run_dense2D_withHeading.m:168)
        if role == "dynModel":
            xn, dx, dt, Q, z = args
            xn = np.asfortranarray(np.asarray(xn, dtype=np.float64).reshape(self.nNonLin, -1))
            npar = xn.shape[1]
            z = np.asfortranarray(np.asarray(z, dtype=np.float64).reshape(self.nw, npar))
            dx = np.ascontiguousarray(np.asarray(dx, dtype=np.float64).ravel())
            Q = np.asfortranarray(np.asarray(Q, dtype=np.float64).reshape(self.nw, self.nw))
            out = np.empty_like(xn)
            check(lib.rbpf_dyn_model(C.byref(self.descriptor()), self.nNonLin, self.nw, self.n_odo, npar, _dp(xn),
                                     _dp(dx), float(dt), _dp(Q), _dp(z), _dp(out)))
            return out[:, 0] if npar == 1 else out
        if role == "dynResNorm":
            xnk, xni, dx, dt, Q = args
            xni = np.asfortranarray(np.asarray(xni, dtype=np.float64).reshape(self.nNonLin, -1))
            npar = xni.shape[1]
            xnk = np.ascontiguousarray(np.asarray(xnk, dtype=np.float64).ravel())
            dx = np.ascontiguousarray(np.asarray(dx, dtype=np.float64).ravel())
            Q = np.asfortranarray(np.asarray(Q, dtype=np.float64).reshape(self.nw, self.nw))
            out = np.empty((self.nw, npar), dtype=np.float64, order="F")
            check(lib.rbpf_dyn_res_norm(C.byref(self.descriptor()), self.nNonLin, self.nw, self.n_odo, npar, _dp(xnk),
                                        _dp(xni), _dp(dx), float(dt), _dp(Q), _dp(out)))
            return out[:, 0] if npar == 1 else out
        raise ValueError(role)


class DenseMagModel(_ModelFamily):
    """examples/slam-dense-mag/run_dense3D_magfield.m: 6-D pose + curl-free 3-D field.
    dynModel :301-308, measModel :265-279, dynResNorm :202-203."""
    kind = _ffi.RBPF_MODEL_DENSE_MAG_6D
    nNonLin, ny, nw, n_odo, dim = 7, 3, 6, 7, 3

    @property
    def nLin(self):
        return self.m + 3

    def JacobianPhi3D(self, x, lower, upper):
        """tools/JacobianPhi3D.m:29-64 on the device: x [3 x Np] -> J [3 x 3 x m x Np]."""
        lib = load_library()
        x = np.asfortranarray(np.asarray(x, dtype=np.float64).reshape(3, -1))
        lo = np.ascontiguousarray(np.asarray(lower, dtype=np.float64).ravel())
        up = np.ascontiguousarray(np.asarray(upper, dtype=np.float64).ravel())
        J = np.empty((3, 3, self.m, x.shape[1]), dtype=np.float64, order="F")
        check(lib.rbpf_jacobian_phi3d(C.byref(self.descriptor()), x.shape[1], _dp(x), _dp(lo), _dp(up), _dp(J)))
        return J


class DenseRadioModel(_ModelFamily):
    """examples/slam-dense-radio/run_dense2D_withHeading.m: planar position + heading, scalar field.
    dynModel :75-76, dynResNorm :77, measModel :168."""
    kind = _ffi.RBPF_MODEL_DENSE_RADIO_2DH
    nNonLin, ny, nw, n_odo, dim = 3, 1, 1, 3, 2

    @property
    def nLin(self):
        return self.m


class SparseVisualModel(_ModelFamily):
    """examples/slam-sparse-visual: planar pose (x, y, heading), nLand point landmarks seen by a 1-D pinhole camera.
    dynModel pfslam.m:81 (xn + dx' + sqrt(dt*Q)*randn, element-wise sqrt), measModel pfslam.m:82 ->
    measurement.m:32-84 ([yhat, dy] = measModel(xn_i, xl_i)), dynResNorm = [] (psslam.m:118-119).
    Runs with sparseFeatures=true (per-particle EKF linearisation, NaN in y = not observed)."""
    kind = _ffi.RBPF_MODEL_SPARSE_VISUAL_2D
    nNonLin, nw, n_odo, dim = 3, 3, 3, 2
    sparse = True

    def __init__(self, nLand, f=1.5, fp=0.0, fw=1.0):                         # camera: load_data.m:58-60
        self.nLand, self.f, self.fp, self.fw = int(nLand), float(f), float(fp), float(fw)
        self.NN = np.zeros((self.nLand, 2), dtype=np.int32)
        self.L = np.ones(2)
        self.dynModel = _Handle(self, "dynModel")
        self.measModel = _Handle(self, "measModel")
        self.dynResNorm = None                                                # psslam.m passes []

    @property
    def m(self):
        return self.nLand

    @property
    def ny(self):
        return self.nLand

    @property
    def nLin(self):
        return 2 * self.nLand

    def descriptor(self, use_dyn_res_norm=False):
        d = _ffi.rbpf_model()
        d.kind, d.m_basis, d.dim, d.use_dyn_res_norm = self.kind, self.nLand, 2, 0
        d.NN = None
        d.cam[0], d.cam[1], d.cam[2] = self.f, self.fp, self.fw
        return d

    def _evaluate(self, role, *args):
        raise RBPFError(_ffi.RBPF_ERR_UNSUPPORTED, "the sparse-visual closures are only evaluated inside the estimators")


class GenericDenseModel:
    """Descriptor behind arbitrary (unrecognised) dynModel / measModel / dynResNorm callables with sparseFeatures = false.
    The handles cross the C ABI as `rbpf_callbacks` (include/rbpf.h): the library calls back once per step with the
    ancestors' states of all ordinary slots (dynModel, evaluated here column by column in slot order exactly as
    particleFilter.m:104-109 / particleSmoother.m:132-137 do) and once with the whole batch (measModel, :124); the
    smoothers additionally call dynResNorm for all particles (particleSmoother.m:178-180) and measModel along the
    reference trajectory (:120).  Everything else of every step stays on the device (RBPF_MODEL_GENERIC_DENSE).  The slow
    path: one host round trip per step."""
    kind = _ffi.RBPF_MODEL_GENERIC_DENSE
    sparse = False

    def __init__(self, nNonLin, nLin, ny, nw, n_odo, dynModel=None, measModel=None, dynResNorm=None, odometry=None, Q=None,
                 dt=None):
        self.nNonLin, self.nLin, self.ny, self.nw, self.n_odo = int(nNonLin), int(nLin), int(ny), int(nw), int(n_odo)
        self._dyn, self._meas, self._drn = dynModel, measModel, dynResNorm
        self._odo, self._Q, self._dt = odometry, Q, dt
        self.error = None                                   # first exception raised inside a callback
        self._cb = None

    def _Qt(self, t):
        return self._Q[:, :, t if self._Q.shape[2] > 1 else 0]

    def _dtt(self, t):
        return float(self._dt[t if self._dt.size > 1 else 0])

    def _make_callbacks(self):
        nN, n, d, nw = self.nNonLin, self.nLin, self.ny, self.nw

        def dyn(_user, t, n_cols, xn_anc, xn_new):
            try:
                A = np.ctypeslib.as_array(xn_anc, shape=(n_cols * nN,)).reshape(n_cols, nN)
                out = np.ctypeslib.as_array(xn_new, shape=(n_cols * nN,)).reshape(n_cols, nN)
                Qt, dtt, odo = self._Qt(t), self._dtt(t), self._odo[t, :]
                for i in range(n_cols):                                                   # particleFilter.m:104-109
                    out[i, :] = np.asarray(self._dyn(A[i].copy(), odo, dtt, Qt), dtype=np.float64).ravel()
                return 0
            except Exception as exc:                                                      # noqa: BLE001
                self.error = self.error or exc
                return 1

        def meas(_user, n_cols, xn, dy):
            try:
                X = np.ctypeslib.as_array(xn, shape=(n_cols * nN,)).reshape(n_cols, nN).T   # [nN x n_cols]
                v = np.asarray(self._meas(np.asfortranarray(X)), dtype=np.float64)            # particleFilter.m:124
                if v.ndim == 2:
                    v = v.reshape(n_cols, 1, n)
                if v.shape != (n_cols, d, n):
                    raise ValueError(f"measModel returned shape {v.shape}, expected {(n_cols, d, n)}")
                np.ctypeslib.as_array(dy, shape=(n_cols * d * n,))[:] = np.asfortranarray(v).ravel(order="F")
                return 0
            except Exception as exc:                                                      # noqa: BLE001
                self.error = self.error or exc
                return 1

        def drn(_user, t, n_cols, xnk_t, xn, e_dyn):
            try:
                xk = np.ctypeslib.as_array(xnk_t, shape=(nN,)).copy()
                X = np.ctypeslib.as_array(xn, shape=(n_cols * nN,)).reshape(n_cols, nN)
                out = np.ctypeslib.as_array(e_dyn, shape=(n_cols * nw,)).reshape(n_cols, nw)
                Qt, dtt, odo = self._Qt(t), self._dtt(t), self._odo[t, :]
                for i in range(n_cols):                                                   # particleSmoother.m:178-180
                    e = np.asarray(self._drn(xk, X[i].copy(), odo, dtt, Qt), dtype=np.float64).ravel()
                    if e.size != nw:
                        raise ValueError(f"dynResNorm returned {e.size} values, expected size(Q,1) = {nw}")
                    out[i, :] = e
                return 0
            except Exception as exc:                                                      # noqa: BLE001
                self.error = self.error or exc
                return 1

        cb = _ffi.rbpf_callbacks()
        self._fns = (_ffi.DYN_MODEL_FN(dyn), _ffi.MEAS_MODEL_FN(meas),
                     _ffi.DYN_RES_NORM_FN(drn) if self._drn is not None else _ffi.DYN_RES_NORM_FN())
        cb.dyn_model, cb.meas_model, cb.dyn_res_norm = self._fns
        cb.user = None
        return cb

    def descriptor(self, use_dyn_res_norm=False):
        d = _ffi.rbpf_model()
        d.kind, d.m_basis, d.dim, d.use_dyn_res_norm = self.kind, self.nLin, 0, 0
        d.NN = None
        if self._dyn is not None:
            self._cb = self._make_callbacks()               # kept alive by the model object
            d.callbacks = C.pointer(self._cb)
        return d


class GenericSparseModel:
    """Descriptor behind a DeviceSparseHandles / DeviceSparseSmootherHandles object: an arbitrary model with sparseFeatures = true, sized from the problem arrays
    (RBPF_MODEL_GENERIC_SPARSE).  It carries no handles -- the binding drives the steps -- only the sizes and the per-step arguments
    of dynModel.  Admitted: ny <= 32, nLin <= 96, nNonLin and nw <= 8; the filter (DeviceSparseHandles) and the covariance-form
    smoother (DeviceSparseSmootherHandles) on one GPU, fp64 storage."""
    kind = _ffi.RBPF_MODEL_GENERIC_SPARSE
    sparse = True

    def __init__(self, nNonLin, nLin, ny, nw, n_odo, odometry=None, Q=None, dt=None):
        self.nNonLin, self.nLin, self.ny, self.nw, self.n_odo = int(nNonLin), int(nLin), int(ny), int(nw), int(n_odo)
        self._odo, self._Q, self._dt = odometry, Q, dt
        self.error = None

    def descriptor(self, use_dyn_res_norm=False):
        d = _ffi.rbpf_model()
        d.kind, d.m_basis, d.dim, d.use_dyn_res_norm = self.kind, self.nLin, 0, 0
        d.NN = None
        return d


class DeviceHandles:
    """An arbitrary (unrecognised) dense model whose handles are device code: batched callables on torch float64 tensors of
    the library's device,

        xn_new (n_nonlin, N_P) = dynModel(xn_anc (n_nonlin, N_P), dx (n_odo,), dt, Q (n_w, n_w))   -- draws its own random numbers
        dy (N_P, n_y, nLin)    = measModel(xn (n_nonlin, N_P))            ((N_P, nLin) is accepted for n_y = 1)

    handed to particleFilter / FilterSession in place of the handle pair.  They run inside torch.cuda.stream(the library's
    stream); xn_anc and xn are views of library memory.  Between two steps nothing is copied to the host and nothing waits
    for it (rbpf_filter_ancestors_device / rbpf_filter_step_device).

    dy_layout=None (default): the binding drives the filter step by step and looks at the strides of every returned dy --
    MATLAB-order strides (1, N_P, N_P n_y) are packed by the transpose kernel (layout 0), a C-contiguous tensor by the row
    copy (layout 2), the native view filled in place is consumed where it is (layout 1, see native_out); anything else costs
    one contiguous() and goes the way of layout 2.
    dy_layout=0 / 1 / 2: the handles are registered as device callbacks (rbpf_filter_set_device_callbacks) and
    rbpf_filter_advance runs the steps; measModel's result is copied into the library's buffer of that layout unless it is
    that buffer.
    native_out=True: measModel is called as measModel(xn, out) with `out` (N_P, n_y, nLin) a view of the buffer the step
    kernels will read (strides (n_y ldx, ldx, 1) by default); filling it and returning it saves the pack kernel."""

    def __init__(self, dynModel, measModel, dy_layout=None, native_out=False):
        if not (callable(dynModel) and callable(measModel)):
            raise RBPFError(_ffi.RBPF_ERR_INVALID_ARG, "dynModel / measModel must be callable")
        if dy_layout not in (None, 0, 1, 2):
            raise RBPFError(_ffi.RBPF_ERR_INVALID_ARG, "dy_layout must be None, 0 (MATLAB order), 1 (native) or 2 (C-contiguous)")
        self.dynModel, self.measModel = dynModel, measModel
        self.dy_layout, self.native_out = dy_layout, bool(native_out)


class DeviceSmootherHandles(DeviceHandles):
    """Device handles for particleSmoother / particleSmootherInformationForm (and, as its base class, for the filter): batched
    callables on torch float64 tensors of the library's device, run inside torch.cuda.stream(the library's stream), handed in
    place of the three handles -- the object as dynModel, None as measModel and dynResNorm.  Between two steps of an iteration
    no state, Jacobian or residual is copied to the host and nothing waits for it (rbpf_particle_smoother_device).

    A filter handle is written for exactly N_P columns; the smoothers' contract is wider, hence the separate class:

        xn_new (n_nonlin, n_cols) = dynModel(xn_anc (n_nonlin, n_cols), dx (n_odo,), dt, Q (n_w, n_w))
            n_cols = N_P in iteration 0, N_P - 1 at the steps t >= 1 of later iterations: the ordinary slots, in slot order
            (particleSmoother.m:132-137).  Draws its own random numbers.  Called once per step, N_T - 1 times per iteration.
        dy (n_cols, n_y, nLin) = measModel(xn (n_nonlin, n_cols))            ((n_cols, nLin) is accepted for n_y = 1)
            must be a PURE function of xn.  n_cols = N_P once per step; N_T once per iteration k >= 1, for the reference
            trajectory (particleSmoother.m:120); with chol_refresh > 1, any chunk size at a refresh, where the information
            matrices are rebuilt from the state history through it.
        e (n_w, N_P) = dynResNorm(xnk_t (n_nonlin,), xn (n_nonlin, N_P), dx, dt, Q)
            the reference's handle (particleSmoother.m:178-180) batched over the particles of generation t - 1.  None: the
            additive default (:175-177) on the device, as for host handles; it needs n_w == n_nonlin.

    dy_layout 0 / 1 / 2 mean what they mean for the filter (DeviceHandles): the layout of the library buffer measModel's result
    is copied into unless it is that buffer.  native_out=True: measModel(xn, out) with `out` (n_cols, n_y, nLin) a view of that
    buffer; with dy_layout=1 its strides are (n_y ldx, ldx, 1) in EVERY call -- the per-step call fills the buffer the step
    kernels read, the others a staging buffer that a copy kernel compacts.
    A handle that raises, or returns a wrong shape, dtype or device, surfaces as that exception; the library stays usable.
    One GPU (no n_devices), dense features only."""

    def __init__(self, dynModel, measModel, dynResNorm=None, dy_layout=0, native_out=False):
        if dy_layout not in (0, 1, 2):
            raise RBPFError(_ffi.RBPF_ERR_INVALID_ARG, "dy_layout must be 0 (MATLAB order), 1 (native) or 2 (C-contiguous)")
        super().__init__(dynModel, measModel, dy_layout=dy_layout, native_out=native_out)
        if not _is_empty_handle(dynResNorm) and not callable(dynResNorm):
            raise RBPFError(_ffi.RBPF_ERR_INVALID_ARG, "dynResNorm must be callable or None")
        self.dynResNorm = None if _is_empty_handle(dynResNorm) else dynResNorm


class DeviceSparseHandles(DeviceHandles):
    """An arbitrary model with sparseFeatures = true (particleFilter.m:127-137,165-181) whose handles are device code: batched
    callables on torch float64 tensors of the library's device, run inside torch.cuda.stream(the library's stream),

        xn_new (n_nonlin, N_P)               = dynModel(xn_anc (n_nonlin, N_P), dx (n_odo,), dt, Q (n_w, n_w))   -- draws its own random numbers
        yhat (N_P, n_y), dy (N_P, n_y, nLin) = measModel(xn (n_nonlin, N_P), xl (N_P, nLin))

    handed to particleFilter(handles, None, ..., sparseFeatures=True) or FilterSession in place of the handle pair.  xl is a view of
    library memory: the linear states after the resampling gather, xl(:,ai) (:112); row i is the map measModel linearises
    particle i at.  measModel is called once per step (the reference's second call at :167 is at the same point).  NaN in y marks
    an output that was not observed: the rows of yhat / dy that belong to such outputs are never read by the step and may hold
    anything, NaN included; dy is dense, no structure is assumed.
    The layouts are read off the strides of what measModel returns: dy C-contiguous or in MATLAB order (strides
    (1, N_P, N_P n_y), packed by a kernel first), yhat contiguous or transposed; anything else costs one contiguous().
    extras=True adds yhattraj (n_y, N_T): every step's yhat of the maximum-weight particle (:201-203).
    n_y <= 32, nLin <= 96, n_nonlin and n_w <= 8; the filter on one GPU with fp64 storage.  Not taken by the smoothers (a filter
    handle is written for exactly N_P columns: particleSmoother takes a DeviceSparseSmootherHandles, whose contract is wider), by
    sharded sessions, with sparseFeatures=False, or with lazy_depth / inplace / another storage (see GenericSparseModel).
    A handle that raises, or returns a wrong shape, dtype or device, surfaces as that exception; the library stays usable."""

    def __init__(self, dynModel, measModel):
        super().__init__(dynModel, measModel)


class DeviceSparseSmootherHandles(DeviceSparseHandles):
    """Device handles for particleSmoother(..., sparseFeatures=True) with an arbitrary model (particleSmoother.m:194-217,267-277,
    306-321), and, as its base class, for the filter: batched callables on torch float64 tensors of the library's device, run inside
    torch.cuda.stream(the library's stream), handed in place of the three handles -- the object as dynModel, None as measModel and
    dynResNorm.  Between two steps of an iteration nothing is copied to the host and nothing waits for it
    (rbpf_particle_smoother_sparse_device).

        xn_new (n_nonlin, C) = dynModel(xn_anc (n_nonlin, C), dx (n_odo,), dt, Q (n_w, n_w))
            C = N_P in iteration 0, N_P - 1 at the steps t >= 1 of later iterations: the ordinary slots, in slot order (:132-137).
            Draws its own random numbers.
        yhat (C, n_y), dy (C, n_y, nLin) = measModel(xn (n_nonlin, C), xl (C, nLin))
            must be a PURE function of its arguments and accept any C.  C = N_P once per step: xl the gathered maps as in the filter,
            the reference slot's sampled map included (:243).  C = F N_P at the steps t >= 1 of the iterations k >= 1, for the
            ancestor weights: F is a chunk of the future times ti of t .. N_T-1 that have an observed output; column f N_P + i carries
            xn = xnk(:,ti_f) and xl row = xl(:,i) of generation t - 1, the map before the resampling gather (the one :206 linearises
            at).  Rows of yhat / dy of outputs not observed at that time are never read; dy is dense, no structure is assumed.
        e (n_w, N_P) = dynResNorm(xnk_t (n_nonlin,), xn (n_nonlin, N_P), dx, dt, Q), or None
            exactly DeviceSmootherHandles' contract; None: the additive default (:175-177) on the device, needs n_w == n_nonlin.

    future_chunk: the largest F per call.  None: as many future times as keep the chunk's staging buffers (dy, F N_P n_y nLin
    doubles, and the replicated xl) within 256 MB; an integer >= 1 forces it.  The results do not depend on it, bit for bit.
    The layouts are read off the strides of what measModel returns, as for DeviceSparseHandles, once, in a call with C = N_P at the
    initial states before the run: dy C-contiguous, in MATLAB order (strides (1, C, C n_y)) or rows on a wider stride (a slice
    [:, :, :nLin]); yhat contiguous or transposed.  The library's buffers then have that layout, and every result is copied into them.
    One GPU, fp64 storage; n_y <= 32, nLin <= 96 and at most 1023 observed outputs after step 0.  Not built: the information form
    (the reference's returns nothing for sparseFeatures: use particleSmoother), host closures, sharding, the MEX gateway."""

    def __init__(self, dynModel, measModel, dynResNorm=None, future_chunk=None):
        super().__init__(dynModel, measModel)
        if not _is_empty_handle(dynResNorm) and not callable(dynResNorm):
            raise RBPFError(_ffi.RBPF_ERR_INVALID_ARG, "dynResNorm must be callable or None")
        if future_chunk is not None and (isinstance(future_chunk, bool) or not isinstance(future_chunk, (int, np.integer)) or future_chunk < 1):
            raise RBPFError(_ffi.RBPF_ERR_INVALID_ARG, "future_chunk must be None (automatic) or an integer >= 1")
        self.dynResNorm = None if _is_empty_handle(dynResNorm) else dynResNorm
        self.future_chunk = None if future_chunk is None else int(future_chunk)


def _refuse_device_handles(what, *handles):
    if any(isinstance(h, DeviceHandles) for h in handles):
        raise RBPFError(_ffi.RBPF_ERR_UNSUPPORTED, "DeviceHandles are not supported by %s: the filter on one GPU only "
                                                   "(particleFilter, FilterSession); the smoothers take a "
                                                   "DeviceSmootherHandles as dynModel, whose handles accept any number of columns" % what)


class _DeviceSmootherCallbacks:
    """The rbpf_callbacks of a DeviceSmootherHandles object: the ctypes wrappers of _DeviceDriver._register with views of the
    passed pointers sized by n_cols, plus dynResNorm.  The stream and the native row stride are the calling context's, asked
    for inside the first callback (the one-shot entry point creates the context itself)."""

    def __init__(self, lib, handles, model, prob):
        import torch
        from .multigpu import _view
        self.torch, self._view = torch, _view
        self.lib, self.h = lib, handles
        self.nN, self.n, self.d, self.nw, self.N = model.nNonLin, model.nLin, model.ny, model.nw, prob.N_P
        self.layout = int(handles.dy_layout)
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.odo = torch.as_tensor(np.ascontiguousarray(model._odo), device=self.device)
        self.Q = torch.as_tensor(np.ascontiguousarray(np.moveaxis(model._Q, 2, 0)), device=self.device)     # [pages][nw][nw]
        self.dt = model._dt
        self.error = None
        self.stream = None
        self.ldx = 0
        torch.cuda.current_stream(self.device).synchronize()           # the constants above, before the library's stream reads them

        def guarded(fn):
            def call(*a):
                try:
                    self._enter()
                    with torch.cuda.stream(self.stream):
                        fn(*a)
                    return 0
                except Exception as exc:                                                  # noqa: BLE001
                    self.error = self.error or exc
                    return 1
            return call

        cb = _ffi.rbpf_callbacks()
        self._fns = (_ffi.DYN_MODEL_FN(guarded(self._dyn)), _ffi.MEAS_MODEL_FN(guarded(self._meas)),
                     _ffi.DYN_RES_NORM_FN(guarded(self._drn)) if handles.dynResNorm is not None else _ffi.DYN_RES_NORM_FN())
        cb.dyn_model, cb.meas_model, cb.dyn_res_norm = self._fns
        cb.user = None
        self.cb = cb

    def _enter(self):
        if self.stream is None:
            sp, ldx = C.c_void_p(), C.c_int32(0)
            check(self.lib.rbpf_stream_get(None, C.byref(sp)))
            check(self.lib.rbpf_filter_external_layout(None, C.byref(ldx)))
            self.stream, self.ldx = self.torch.cuda.ExternalStream(sp.value, device=self.device), ldx.value

    def _args(self, t):
        return self.odo[t], float(self.dt[t if self.dt.size > 1 else 0]), self.Q[t if self.Q.shape[0] > 1 else 0]

    def _checked(self, what, x, shape):
        if tuple(x.shape) != shape or x.dtype != self.torch.float64 or not x.is_cuda:
            raise ValueError(f"{what} returned {tuple(x.shape)} {x.dtype} on {x.device}, expected a float64 device tensor of "
                             f"shape {shape}")
        return x

    def _dyn(self, _user, t, n_cols, xn_anc, xn_new):
        anc = self._view(self.torch, xn_anc, (n_cols, self.nN), self.device).t()
        xn = self._checked("dynModel", self.h.dynModel(anc, *self._args(t)), (self.nN, n_cols))
        self._view(self.torch, xn_new, (n_cols, self.nN), self.device).t().copy_(xn)

    def _drn(self, _user, t, n_cols, xnk_t, xn, e_dyn):
        xk = self._view(self.torch, xnk_t, (self.nN,), self.device)
        X = self._view(self.torch, xn, (n_cols, self.nN), self.device).t()
        e = self._checked("dynResNorm", self.h.dynResNorm(xk, X, *self._args(t)), (self.nw, n_cols))
        self._view(self.torch, e_dyn, (n_cols, self.nw), self.device).t().copy_(e)

    def _meas(self, _user, n_cols, xn, dy_p):
        n, d = self.n, self.d
        if self.layout == 0:
            target = self._view(self.torch, dy_p, (n, d, n_cols), self.device).permute(2, 1, 0)
        elif self.layout == 1:
            target = self._view(self.torch, dy_p, (n_cols, d, self.ldx), self.device)[:, :, :n]
        else:
            target = self._view(self.torch, dy_p, (n_cols, d, n), self.device)
        X = self._view(self.torch, xn, (n_cols, self.nN), self.device).t()
        dy = self.h.measModel(X, target) if self.h.native_out else self.h.measModel(X)
        if dy.dim() == 2 and d == 1:
            dy = dy.unsqueeze(1)
        self._checked("measModel", dy, (n_cols, d, n))
        if not _DeviceDriver._same(dy, target):
            target.copy_(dy)


class _SparseSmootherCallbacks(_DeviceSmootherCallbacks):
    """The callbacks of a DeviceSparseSmootherHandles object for rbpf_particle_smoother_sparse_device: dynModel and dynResNorm as
    for DeviceSmootherHandles; measModel takes the maps and returns (yhat, dy), copied into the library's buffers of the layouts
    read off its strides in one call at the initial states (C = N_P) before the run."""

    def __init__(self, lib, handles, model, prob):
        import torch
        from .multigpu import _view
        self.torch, self._view = torch, _view
        self.lib, self.h = lib, handles
        self.nN, self.n, self.d, self.nw, self.N = model.nNonLin, model.nLin, model.ny, model.nw, prob.N_P
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.odo = torch.as_tensor(np.ascontiguousarray(model._odo), device=self.device)
        self.Q = torch.as_tensor(np.ascontiguousarray(np.moveaxis(model._Q, 2, 0)), device=self.device)     # [pages][nw][nw]
        self.dt = model._dt
        self.error = None
        self.stream = None
        self.ldx = 0
        self.future = 0 if handles.future_chunk is None else int(handles.future_chunk)
        x0 = torch.as_tensor(prob.x0n, device=self.device).repeat(self.N, 1).t()
        xl0 = torch.as_tensor(np.ascontiguousarray(prob.x0l.T), device=self.device)
        yhat, dy = self._meas_sparse(x0, xl0.expand(self.N, self.n).contiguous() if xl0.shape[0] == 1 else xl0, self.N)
        self.yhat_layout = 0 if (not yhat.is_contiguous() and yhat.t().is_contiguous()) else 2
        if dy.is_contiguous():
            self.dy_layout = 2
        elif dy.permute(2, 1, 0).is_contiguous():
            self.dy_layout = 0
        else:                                             # rows on a wider stride: the library's buffer has its own, ldx
            self.dy_layout = 1 if (dy.stride(2) == 1 and dy.stride(0) == self.d * dy.stride(1)) else 2
        del yhat, dy
        torch.cuda.current_stream(self.device).synchronize()           # the constants above, before the library's stream reads them

        def guarded(fn):
            def call(*a):
                try:
                    self._enter()
                    with torch.cuda.stream(self.stream):
                        fn(*a)
                    return 0
                except Exception as exc:                                                  # noqa: BLE001
                    self.error = self.error or exc
                    return 1
            return call

        self._fns = (_ffi.DYN_MODEL_FN(guarded(self._dyn)), _ffi.SPARSE_MEAS_MODEL_FN(guarded(self._meas)),
                     _ffi.DYN_RES_NORM_FN(guarded(self._drn)) if handles.dynResNorm is not None else _ffi.DYN_RES_NORM_FN())

    def _meas_sparse(self, xn, xl, n_cols):
        torch = self.torch
        out = self.h.measModel(xn, xl)
        if not (isinstance(out, (tuple, list)) and len(out) == 2 and all(torch.is_tensor(v) for v in out)):
            raise ValueError("measModel must return (yhat, dy), two device tensors")
        self._checked("measModel (yhat)", out[0], (n_cols, self.d))
        self._checked("measModel (dy)", out[1], (n_cols, self.d, self.n))
        return out

    def _meas(self, _user, n_cols, xn, xl, ldx, yhat_p, dy_p):
        n, d = self.n, self.d
        X = self._view(self.torch, xn, (n_cols, self.nN), self.device).t()
        XL = self._view(self.torch, xl, (n_cols, ldx), self.device)[:, :n]
        yhat, dy = self._meas_sparse(X, XL, n_cols)
        if self.yhat_layout == 0:
            self._view(self.torch, yhat_p, (d, n_cols), self.device).t().copy_(yhat)
        else:
            self._view(self.torch, yhat_p, (n_cols, d), self.device).copy_(yhat)
        if self.dy_layout == 0:
            target = self._view(self.torch, dy_p, (n, d, n_cols), self.device).permute(2, 1, 0)
        elif self.dy_layout == 1:
            target = self._view(self.torch, dy_p, (n_cols, d, ldx), self.device)[:, :, :n]
        else:
            target = self._view(self.torch, dy_p, (n_cols, d, n), self.device)
        target.copy_(dy)


class _DeviceDriver:
    """Runs the steps of a generic-family filter context with DeviceHandles (see there)."""

    def __init__(self, lib, ctx, handles, model, prob):
        self._setup(lib, ctx, handles, (model.nNonLin, model.nLin, model.ny, prob.N_P, prob.N_T), lib.rbpf_filter_external_layout, model)
        self.x0 = self.torch.as_tensor(prob.x0n, device=self.device).repeat(self.N, 1)                       # particleFilter.m:59
        self.torch.cuda.current_stream(self.device).synchronize()      # the constants above, before the library's stream reads them
        if handles.dy_layout is not None:
            self._register(int(handles.dy_layout))

    def _setup(self, lib, ctx, handles, sizes, layout_fn, args):
        """The context's stream and native row stride (layout_fn), and the handles' per-step arguments (args._odo, ._Q, ._dt) as
        device constants; the caller synchronises before the library's stream reads them."""
        import torch
        from .multigpu import _view
        self.torch, self._view = torch, _view
        self.lib, self.ctx, self.h = lib, ctx, handles
        self.nN, self.n, self.d, self.N, self.T = sizes
        self.device = torch.device("cuda", torch.cuda.current_device())
        sp = C.c_void_p()
        check(lib.rbpf_stream_get(ctx, C.byref(sp)))
        self.stream = torch.cuda.ExternalStream(sp.value, device=self.device)
        ldx = C.c_int32(0)
        check(layout_fn(ctx, C.byref(ldx)))
        self.ldx = ldx.value
        self.odo = torch.as_tensor(np.ascontiguousarray(args._odo), device=self.device)
        self.Q = torch.as_tensor(np.ascontiguousarray(np.moveaxis(args._Q, 2, 0)), device=self.device)      # [pages][nw][nw]
        self.dt = args._dt
        self.error = None
        self._keep = None
        self._native = None
        self._cb = None

    # -- the handles ------------------------------------------------------------------------------------
    def _dyn(self, t, xn_anc):
        Q = self.Q[t if self.Q.shape[0] > 1 else 0]
        xn = self.h.dynModel(xn_anc, self.odo[t], float(self.dt[t if self.dt.size > 1 else 0]), Q)
        if tuple(xn.shape) != (self.nN, self.N) or xn.dtype != self.torch.float64 or not xn.is_cuda:
            raise ValueError(f"dynModel returned {tuple(xn.shape)} {xn.dtype} on {xn.device}, expected a float64 device tensor of "
                             f"shape {(self.nN, self.N)}")
        return xn

    def _meas(self, xn, out):
        dy = self.h.measModel(xn, out) if self.h.native_out else self.h.measModel(xn)
        if dy.dim() == 2 and self.d == 1:
            dy = dy.unsqueeze(1)
        if tuple(dy.shape) != (self.N, self.d, self.n) or dy.dtype != self.torch.float64 or not dy.is_cuda:
            raise ValueError(f"measModel returned {tuple(dy.shape)} {dy.dtype} on {dy.device}, expected a float64 device tensor of "
                             f"shape {(self.N, self.d, self.n)}")
        return dy

    @staticmethod
    def _same(a, b):
        return b is not None and a.data_ptr() == b.data_ptr() and a.stride() == b.stride()

    def _dy_view(self, ptr, layout):
        """(N, n_y, nLin) view of a dy buffer of the C ABI's layout 0 / 1 / 2."""
        N, d, n = self.N, self.d, self.n
        if layout == 0:
            return self._view(self.torch, ptr, (n, d, N), self.device).permute(2, 1, 0)
        if layout == 1:
            return self._view(self.torch, ptr, (N, d, self.ldx), self.device)[:, :, :n]
        return self._view(self.torch, ptr, (N, d, n), self.device)

    # -- caller-driven: one step at a time, the layout of every dy read off its strides --------------------
    def _step(self, t):
        torch, lib = self.torch, self.lib
        with torch.cuda.stream(self.stream):
            if t == 0:
                xn_cm = self.x0
            else:
                ai, anc = C.c_void_p(), C.c_void_p()
                check(lib.rbpf_filter_ancestors_device(self.ctx, C.byref(ai), C.byref(anc)))
                xn = self._dyn(t - 1, self._view(torch, anc, (self.N, self.nN), self.device).t())
                xn_cm = xn.t().contiguous()                               # [n_nonlin x N_P] column-major (no copy if it is)
            out = self._native_out()
            dy, layout = self._layout_of(self._meas(xn_cm.t(), out), out)
            self._keep = (xn_cm, dy)                                      # read in stream order by the step just enqueued
            check(lib.rbpf_filter_step_device(self.ctx, C.c_void_p(xn_cm.data_ptr()), C.c_void_p(dy.data_ptr()), layout))

    def _native_out(self):
        """The (N, n_y, nLin) view of the native buffer a native_out measModel fills, or None."""
        if not self.h.native_out:
            return None
        if self._native is None:
            self._native = self.torch.zeros((self.N, self.d, self.ldx), dtype=self.torch.float64, device=self.device)
        return self._native[:, :, :self.n]

    def _layout_of(self, dy, out):
        """(dy, dy_layout of the C ABI) read off the strides of what measModel returned; anything else costs one contiguous()."""
        if self._same(dy, out):
            return dy, 1
        if dy.is_contiguous():
            return dy, 2
        if dy.permute(2, 1, 0).is_contiguous():
            return dy, 0
        return dy.contiguous(), 2

    # -- device callbacks: rbpf_filter_advance runs the steps ---------------------------------------------
    def _register(self, layout):
        torch = self.torch

        def dyn(_user, t, n_cols, xn_anc, xn_new):
            try:
                with torch.cuda.stream(self.stream):
                    anc = self._view(torch, xn_anc, (n_cols, self.nN), self.device).t()
                    self._view(torch, xn_new, (n_cols, self.nN), self.device).t().copy_(self._dyn(t, anc))
                return 0
            except Exception as exc:                                                      # noqa: BLE001
                self.error = self.error or exc
                return 1

        def meas(_user, n_cols, xn, dy_p):
            try:
                with torch.cuda.stream(self.stream):
                    target = self._dy_view(dy_p, layout)
                    dy = self._meas(self._view(torch, xn, (n_cols, self.nN), self.device).t(), target)
                    if not self._same(dy, target):
                        target.copy_(dy)
                return 0
            except Exception as exc:                                                      # noqa: BLE001
                self.error = self.error or exc
                return 1

        cb = _ffi.rbpf_callbacks()
        self._fns = (_ffi.DYN_MODEL_FN(dyn), _ffi.MEAS_MODEL_FN(meas))
        cb.dyn_model, cb.meas_model = self._fns
        cb.user = None
        self._cb = cb
        check(self.lib.rbpf_filter_set_device_callbacks(self.ctx, C.byref(cb), layout))

    def advance(self, n_steps):
        try:
            if self._cb is not None:
                check(self.lib.rbpf_filter_advance(self.ctx, int(n_steps)))
                return
            t0 = C.c_int32(0)
            check(self.lib.rbpf_filter_tell(self.ctx, C.byref(t0)))
            if t0.value + int(n_steps) > self.T:
                raise RBPFError(_ffi.RBPF_ERR_STATE, "advance past N_T")
            for t in range(t0.value, t0.value + int(n_steps)):
                self._step(t)
        except RBPFError as exc:
            if exc.status == _ffi.RBPF_ERR_CALLBACK and self.error is not None:
                raise self.error from exc
            raise


class _SparseDeviceDriver(_DeviceDriver):
    """Runs the steps of a generic sparse filter context with DeviceSparseHandles (see there)."""

    def _meas_sparse(self, xn, xl):
        torch = self.torch
        out = self.h.measModel(xn, xl)
        if not (isinstance(out, (tuple, list)) and len(out) == 2 and all(torch.is_tensor(v) for v in out)):
            raise ValueError("measModel must return (yhat, dy), two device tensors")
        for what, v, shape in (("yhat", out[0], (self.N, self.d)), ("dy", out[1], (self.N, self.d, self.n))):
            if tuple(v.shape) != shape or v.dtype != torch.float64 or not v.is_cuda:
                raise ValueError(f"measModel returned {what} {tuple(v.shape)} {v.dtype} on {v.device}, expected a float64 device "
                                 f"tensor of shape {shape}")
        return out

    @staticmethod
    def _layouts(yhat, dy):
        """(yhat, yhat_layout, dy, dy_layout) of the C ABI read off the strides; anything else costs one contiguous()."""
        if yhat.is_contiguous():
            yl = 2
        elif yhat.t().is_contiguous():
            yl = 0
        else:
            yhat, yl = yhat.contiguous(), 2
        if dy.is_contiguous():
            dl = 2
        elif dy.permute(2, 1, 0).is_contiguous():
            dl = 0
        else:
            dy, dl = dy.contiguous(), 2
        return yhat, yl, dy, dl

    def _step(self, t):
        torch, lib = self.torch, self.lib
        with torch.cuda.stream(self.stream):
            if t == 0:
                xn_cm = self.x0
            else:
                ai, anc = C.c_void_p(), C.c_void_p()
                check(lib.rbpf_filter_ancestors_device(self.ctx, C.byref(ai), C.byref(anc)))
                xn = self._dyn(t - 1, self._view(torch, anc, (self.N, self.nN), self.device).t())
                xn_cm = xn.t().contiguous()                               # [n_nonlin x N_P] column-major (no copy if it is)
            xlp, ldx = C.c_void_p(), C.c_int32(0)
            check(lib.rbpf_filter_sparse_gathered_device(self.ctx, C.byref(xlp), C.byref(ldx)))
            xl = self._view(torch, xlp, (self.N, ldx.value), self.device)[:, :self.n]       # xl(:,ai), particleFilter.m:112
            yhat, yl, dy, dl = self._layouts(*self._meas_sparse(xn_cm.t(), xl))
            self._keep = (xn_cm, yhat, dy)                                # read in stream order by the step just enqueued
            check(lib.rbpf_filter_step_sparse_device(self.ctx, C.c_void_p(xn_cm.data_ptr()), C.c_void_p(yhat.data_ptr()), yl,
                                                     C.c_void_p(dy.data_ptr()), dl))

    def yhattraj(self):
        out = np.empty((self.d, self.T), order="F")
        check(self.lib.rbpf_filter_sparse_yhattraj(self.ctx, _dp(out)))
        return out


def dense_mag_prior(m, LL, theta):
    """GP prior of run_dense3D_magfield.m:83-107,122-131 -> (model, x0_lin, P0_lin, R)."""
    L, NN = domain_cartesian_dx(m, 3, LL)
    lam = eigenval(NN, L)
    linSigma2, lengthScale, magnSigma2, sigma2 = (float(t) for t in np.asarray(theta).ravel())
    Sse = magnSigma2 * math.sqrt(2 * math.pi) ** 3 * lengthScale ** 3 * np.exp(-lam * lengthScale ** 2 / 2)
    k = np.concatenate(([linSigma2] * 3, Sse))
    return DenseMagModel(NN, L), np.zeros(m + 3), np.diag(k), sigma2 * np.eye(3)


def dense_radio_prior(m, LL, theta):
    """run_dense2D_withHeading.m:107-128,137-146 -> (model, x0_lin, P0_lin, R)."""
    L, NN = domain_cartesian_dx(m, 2, LL)
    lam = eigenval(NN, L)
    lengthScale, magnSigma2, sigma2 = (float(t) for t in np.asarray(theta).ravel())
    k = magnSigma2 * math.sqrt(2 * math.pi) ** 2 * lengthScale ** 2 * np.exp(-lam * lengthScale ** 2 / 2)
    return DenseRadioModel(NN, L), np.zeros(m), np.diag(k), sigma2 * np.eye(1)


# ------------------------------------------------------------------------------------------------
# RNG blocks
# ------------------------------------------------------------------------------------------------
@dataclass
class PhiloxRNG:
    """Device Philox4x32-10 stream keyed by `seed` (throughput runs)."""
    seed: int = 1

    def replay(self, N_P, N_T, nw, n_iter=1):
        """The exact uniforms / normals the device generator uses, as a ReplayRNG."""
        lib = load_library()
        U = np.empty((n_iter, max(N_T - 1, 0), N_P))
        Z = np.empty((n_iter, max(N_T - 1, 0), N_P, nw))
        Ufin = np.empty(n_iter)
        for k in range(n_iter):
            uf = C.c_double(0.0)
            check(lib.rbpf_philox_fill(C.c_uint64(self.seed), k, N_P, N_T, nw, _dp(U[k]), _dp(Z[k]), C.byref(uf)))
            Ufin[k] = uf.value
        return ReplayRNG(U, Z, Ufin)

    def backward_uniforms(self, n_traj, N_T):
        """The uniforms u [N_T x n_traj] rbpf_loc_backward_simulate draws from this seed: Philox4x32-10 on the counters
        (slot = j, step = t, lane = 0x42530000, iter = 0), first uniform (53 bits).  Computed on the host, bit for bit."""
        M32 = np.uint64(0xFFFFFFFF)
        t, j = np.meshgrid(np.arange(int(N_T), dtype=np.uint64), np.arange(int(n_traj), dtype=np.uint64), indexing="ij")
        c = [j, t, np.full_like(j, 0x42530000), np.zeros_like(j)]
        k0, k1 = np.uint64(int(self.seed) & 0xFFFFFFFF), np.uint64((int(self.seed) >> 32) & 0xFFFFFFFF)
        for _ in range(10):
            p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
            c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
            k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
        a = ((c[0] << np.uint64(32)) | c[1]) >> np.uint64(11)
        return (a.astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)


class ReplayRNG:
    """Pre-drawn random numbers in the reference's call order.
    U [n_iter, N_T-1, N_P], Z [n_iter, N_T-1, N_P, nw], Ufin [n_iter] (see include/rbpf.h); Uback [N_T, N_S]: the backward
    uniforms of particleSmootherLocalization (row t = step t)."""

    def __init__(self, U, Z, Ufin=None, Uback=None):
        self.Uback = None if Uback is None else np.ascontiguousarray(np.asarray(Uback, dtype=np.float64))   # particleSmootherLocalization: u [N_T x N_S]
        self.U = np.ascontiguousarray(np.asarray(U, dtype=np.float64))
        self.Z = np.ascontiguousarray(np.asarray(Z, dtype=np.float64))
        if self.U.ndim == 2:
            self.U = self.U[None]
        if self.Z.ndim == 3:
            self.Z = self.Z[None]
        self.Ufin = None if Ufin is None else np.ascontiguousarray(np.asarray(Ufin, dtype=np.float64).ravel())


def _rng_block(rng, N_P, N_T, nw, n_iter):
    blk = _ffi.rbpf_rng()
    if rng is None:
        rng = PhiloxRNG(1)
    if isinstance(rng, PhiloxRNG):
        blk.mode = _ffi.RBPF_RNG_PHILOX
        blk.n_iter = n_iter
        blk.seed = int(rng.seed)
        return blk, rng
    if not isinstance(rng, ReplayRNG):
        raise TypeError("rng must be PhiloxRNG or ReplayRNG")
    if N_T > 1:
        if rng.U.shape[0] < n_iter or rng.U.shape[1:] != (N_T - 1, N_P):
            raise ValueError(f"ReplayRNG.U must be [{n_iter}, {N_T - 1}, {N_P}]")
        if rng.Z.shape[0] < n_iter or rng.Z.shape[1:] != (N_T - 1, N_P, nw):
            raise ValueError(f"ReplayRNG.Z must be [{n_iter}, {N_T - 1}, {N_P}, {nw}]")
    blk.mode = _ffi.RBPF_RNG_REPLAY
    blk.n_iter = rng.U.shape[0]
    blk.U = _dp(rng.U)
    blk.Z = _dp(rng.Z)
    if rng.Ufin is not None:
        blk.Ufin = _dp(rng.Ufin)
    return blk, rng


def _dp(a):
    return a.ctypes.data_as(_ffi.c_double_p)


def _ip(a):
    return a.ctypes.data_as(_ffi.c_int32_p)


# ------------------------------------------------------------------------------------------------
# problem marshalling
# ------------------------------------------------------------------------------------------------
class _Problem:
    def __init__(self, model, odometry, y, x0_nonLin, x0_lin, P0_lin, Q, R, N_P, dt):
        y = np.asarray(y, dtype=np.float64)
        if y.ndim == 1:
            y = y.reshape(-1, 1)
        self.N_T, self.ny = y.shape
        self.N_P = int(N_P)
        self.y = np.asfortranarray(y)
        odo = np.asarray(odometry, dtype=np.float64)
        if odo.ndim == 1:
            odo = odo.reshape(1, -1)
        self.odo = np.asfortranarray(odo)
        self.x0n = np.ascontiguousarray(np.asarray(x0_nonLin, dtype=np.float64).ravel())
        x0l = np.asarray(x0_lin, dtype=np.float64)
        if x0l.ndim == 1:
            x0l = x0l.reshape(-1, 1)
        self.x0l = np.asfortranarray(x0l)
        self.P0 = np.asfortranarray(np.asarray(P0_lin, dtype=np.float64))
        Q = np.asarray(Q, dtype=np.float64)
        if Q.ndim == 0:
            Q = Q.reshape(1, 1)
        if Q.ndim == 2:
            Q = Q[:, :, None]
        self.Q = np.asfortranarray(Q)
        self.R = np.asfortranarray(np.atleast_2d(np.asarray(R, dtype=np.float64)))
        self.dt = np.ascontiguousarray(np.atleast_1d(np.asarray(dt, dtype=np.float64)).ravel())
        n = self.x0l.shape[0]
        if self.x0n.size != model.nNonLin or n != model.nLin or self.ny != model.ny:
            raise ValueError("state / measurement sizes do not match the model family")
        if self.P0.shape != (n, n) or self.R.shape != (self.ny, self.ny):
            raise ValueError("P0_lin / R shape mismatch")
        if self.Q.shape[0] != model.nw or self.Q.shape[1] != model.nw:
            raise ValueError("Q shape mismatch")
        if self.N_T > 1 and (self.odo.shape[0] < self.N_T - 1 or self.odo.shape[1] != model.n_odo):
            raise ValueError("odometry must be [>=N_T-1 x n_odo]")
        p = _ffi.rbpf_problem()
        p.N_P, p.N_T = self.N_P, self.N_T
        p.n_nonlin, p.n_lin, p.n_y, p.n_w, p.n_odo = model.nNonLin, n, self.ny, model.nw, model.n_odo
        p.x0_lin_cols = self.x0l.shape[1]
        p.q_pages = self.Q.shape[2]
        p.dt_len = self.dt.size
        p.odometry = _dp(self.odo)
        p.odo_ld = self.odo.shape[0]
        p.y, p.x0_nonlin, p.x0_lin, p.P0_lin = _dp(self.y), _dp(self.x0n), _dp(self.x0l), _dp(self.P0)
        p.Q, p.R, p.dt = _dp(self.Q), _dp(self.R), _dp(self.dt)
        self.c = p


def _storage_code(storage):
    """rbpf_options.storage: "fp64" (default, the reference's precision), "fp32" storage of the covariance banks, or
    "fp64sym" (fp64, lower block triangle only: particleFilter.m:198 keeps the covariances symmetric), or "fp32sym" (the lower block
    triangle in fp32; arithmetic stays fp64)."""
    if storage in ("fp64", 0, None):
        return 0
    if storage in ("fp32", 1):
        return 1
    if storage in ("fp64sym", "sym", 2):
        return 2
    if storage in ("fp32sym", 3):
        return 3
    raise ValueError("storage must be 'fp64', 'fp32', 'fp64sym' or 'fp32sym'")


def _check_sparse_flag(model, sparseFeatures):
    """sparseFeatures selects the measModel calling convention (particleFilter.m:123-129): it has to match the family."""
    if bool(sparseFeatures) != bool(getattr(model, "sparse", False)):
        raise RBPFError(_ffi.RBPF_ERR_INVALID_ARG,
                        "sparseFeatures=%s does not match the measurement model of %s" % (bool(sparseFeatures), type(model).__name__))


def _is_empty_handle(h):
    return h is None or (isinstance(h, (list, tuple)) and len(h) == 0)


def _recognise(dynModel, measModel, dynResNorm=None):
    """Map handles to a model family (the MATLAB wrappers do the same on functions(h)).  Returns (model, use_dynResNorm);
    model is None when the handles belong to no known family -- the generic (host-callback) family then takes them."""
    mdl = getattr(dynModel, "model", None)
    if not isinstance(mdl, _ModelFamily) or getattr(measModel, "model", None) is not mdl:
        if isinstance(mdl, _ModelFamily) or isinstance(getattr(measModel, "model", None), _ModelFamily):
            raise RBPFError(_ffi.RBPF_ERR_UNSUPPORTED, "dynModel and measModel are handles of different model families")
        if not (callable(dynModel) and callable(measModel)):
            raise RBPFError(_ffi.RBPF_ERR_INVALID_ARG, "dynModel / measModel must be callable")
        return None, not _is_empty_handle(dynResNorm)
    use_drn = True
    if _is_empty_handle(dynResNorm):
        use_drn = False                                       # isempty(dynResNorm), particleSmoother.m:175
    elif getattr(dynResNorm, "model", None) is not mdl:
        raise RBPFError(_ffi.RBPF_ERR_UNSUPPORTED, "dynResNorm is not the model family's handle")
    return mdl, use_drn


def _device_handles(dynModel, measModel):
    """The DeviceHandles object given in place of the handle pair (as dynModel, measModel None or the same object), or None."""
    if not isinstance(dynModel, DeviceHandles) and not isinstance(measModel, DeviceHandles):
        return None
    if not isinstance(dynModel, DeviceHandles) or (measModel is not None and measModel is not dynModel):
        raise RBPFError(_ffi.RBPF_ERR_INVALID_ARG, "DeviceHandles replace the handle pair: pass the object as dynModel and None "
                                                   "(or the same object) as measModel")
    return dynModel


def _generic_model(dynModel, measModel, dynResNorm, odometry, y, x0_nonLin, x0_lin, Q, dt, sparse=False):
    """GenericDenseModel for arbitrary callables (sparse=True: GenericSparseModel for DeviceSparseHandles), sized from the problem
    arrays."""
    y2 = np.asarray(y, dtype=np.float64)
    y2 = y2.reshape(-1, 1) if y2.ndim == 1 else y2
    Qa = np.asarray(Q, dtype=np.float64)
    Qa = Qa.reshape(1, 1) if Qa.ndim == 0 else Qa
    Q3 = Qa[:, :, None] if Qa.ndim == 2 else Qa
    x0l = np.asarray(x0_lin, dtype=np.float64)
    odo = np.asarray(odometry, dtype=np.float64)
    odo = odo.reshape(1, -1) if odo.ndim == 1 else odo
    dtv = np.atleast_1d(np.asarray(dt, dtype=np.float64)).ravel()
    if sparse:
        return GenericSparseModel(np.asarray(x0_nonLin).size, x0l.shape[0], y2.shape[1], Q3.shape[0], odo.shape[1], odo, Q3, dtv)
    return GenericDenseModel(np.asarray(x0_nonLin).size, x0l.shape[0], y2.shape[1], Q3.shape[0], odo.shape[1], dynModel, measModel,
                             None if _is_empty_handle(dynResNorm) else dynResNorm, odo, Q3, dtv)


def _raise_callback_error(model, exc):
    """A Python exception inside a handle surfaces as RBPF_ERR_CALLBACK from the library: re-raise the original."""
    if isinstance(exc, RBPFError) and exc.status == _ffi.RBPF_ERR_CALLBACK and getattr(model, "error", None) is not None:
        raise model.error from exc
    raise exc


# ------------------------------------------------------------------------------------------------
# the three estimators
# ------------------------------------------------------------------------------------------------
def particleFilter(dynModel, measModel, odometry, y, x0_nonLin, x0_lin, P0_lin, Q, R, N_P, dt,
                   sparseFeatures=False, makePlots: Optional[Callable] = None, *, rng=None, trace=False,
                   want_xn_traj=True, extras=False, lazy_depth=0, inplace=0, storage="fp64", fix_p_mean=False, n_devices=0,
                   device_ids=None):
    """Mirror of src/particleFilter.m:1-3.  Returns the reference's 8 outputs
    (traj_max, traj_mean, xl_max, xl_mean, P_max, P_mean, traj_sample_iwmax, xn_traj); with
    extras=True a 9th element (dict of traces / final particle banks) is appended.

    Handles of a recognised family (DenseMagModel / DenseRadioModel / SparseVisualModel) run entirely in the HIP kernels.
    Any other pair of callables takes the generic family: the reference's calling conventions (particleFilter.m:108,124)
        xn_new [nN] = dynModel(xn_i [nN], odometry(t-1,:), dt(t-1), Q(:,:,t-1))      -- draws its own random numbers
        dy [N x ny x nLin] (or [N x nLin] for ny = 1) = measModel(xn [nN x N])
    evaluated on the host through `rbpf_callbacks`; resampling uniforms still come from `rng` (the normals of a ReplayRNG
    are not used: dynModel owns its randomness, as in the reference).
    A DeviceHandles object as dynModel (measModel None) keeps such a model on the device: batched handles on torch tensors, no
    host round trip (see DeviceHandles; one GPU, no n_devices).
    makePlots is called after every step with the reference's nine arguments (particleFilter.m:215-217) through the
    library's on_step hook.
    n_devices = W > 1 (rbpf_options.n_devices): the library shards the N_P particles over W GPUs itself -- one host thread per
    device, RCCL collectives -- and returns the reference's eight outputs (xn_traj from the replicated state history; None with
    want_xn_traj=False); device_ids names the HIP devices
    (a device named twice makes its ranks share it over a host-staged transport: tests on one GPU)."""
    handles = _device_handles(dynModel, measModel)
    if handles is not None:                                   # device code: no host callbacks, the binding drives the context
        if int(n_devices) > 1 or (int(n_devices) == 1 and device_ids is not None):
            _refuse_device_handles("sharded sessions (n_devices)", handles)
        dynModel = measModel = None
        model = None
    else:
        model, _ = _recognise(dynModel, measModel, model_dyn_res_norm(dynModel))
    generic = model is None
    if generic:
        if isinstance(handles, DeviceSparseHandles):
            if not sparseFeatures:
                raise RBPFError(_ffi.RBPF_ERR_INVALID_ARG, "DeviceSparseHandles need sparseFeatures=True: their measModel returns "
                                                           "(yhat, dy) at every particle's own map")
        elif sparseFeatures:
            raise RBPFError(_ffi.RBPF_ERR_UNSUPPORTED, "sparseFeatures=true is implemented for the sparse-visual family only")
        model = _generic_model(dynModel, measModel, None, odometry, y, x0_nonLin, x0_lin, Q, dt, sparse=bool(sparseFeatures))
    _check_sparse_flag(model, sparseFeatures)
    lib = load_library()
    prob = _Problem(model, odometry, y, x0_nonLin, x0_lin, P0_lin, Q, R, N_P, dt)
    nN, n, N, T = model.nNonLin, model.nLin, prob.N_P, prob.N_T
    if generic and isinstance(rng, ReplayRNG) and (rng.Z is None or rng.Z.size == 0):
        rng = ReplayRNG(rng.U, np.zeros(rng.U.shape + (model.nw,)), rng.Ufin)
    blk, _keep = _rng_block(rng, N, T, model.nw, 1)
    opt = _ffi.rbpf_options(keep_history=1, trace=1 if (trace or extras) else 0, fix_p_mean=1 if fix_p_mean else 0,
                            lazy_depth=int(lazy_depth), jitter=0.0, inplace=int(inplace),
                            storage=_storage_code(storage))
    mdesc = model.descriptor()
    multi = int(n_devices) > 1 or (int(n_devices) == 1 and device_ids is not None)
    if multi:
        if extras or makePlots is not None:
            raise RBPFError(_ffi.RBPF_ERR_UNSUPPORTED, "n_devices: traces / final banks / makePlots are not available in the sharded filter")
        ids = None
        if device_ids is not None:
            ids = (C.c_int32 * int(n_devices))(*[int(v) for v in device_ids])
            opt.device_ids = C.cast(ids, C.POINTER(C.c_int32))
        opt.n_devices = int(n_devices)
        o = _ffi.rbpf_filter_out()
        b = dict(traj_max=np.full((nN, T), np.nan, order="F"), traj_mean=np.full((nN, T), np.nan, order="F"), xl_max=np.empty(n),
                 P_max=np.empty((n, n), order="F"), xl_mean=np.empty(n), P_mean=np.empty((n, n), order="F"),
                 traj_sample_iwmax=np.empty((nN, T), order="F"), iw_max=np.zeros(1, dtype=np.int32))
        if want_xn_traj:
            b["xn_traj"] = np.empty((nN, N, T), order="F")
        for k, v in b.items():
            setattr(o, k, _ip(v) if v.dtype == np.int32 else _dp(v))
        check(lib.rbpf_particle_filter(C.byref(mdesc), C.byref(prob.c), C.byref(blk), C.byref(opt), C.byref(o)))
        return (b["traj_max"], b["traj_mean"], b["xl_max"], b["xl_mean"], b["P_max"], b["P_mean"], b["traj_sample_iwmax"],
                b.get("xn_traj"))

    def alloc_out(Tdone, full):
        o = _ffi.rbpf_filter_out()
        bufs = dict(traj_max=np.empty((nN, T), order="F"), traj_mean=np.empty((nN, T), order="F"),
                    xl_max=np.empty(n), P_max=np.empty((n, n), order="F"))
        if full:
            bufs.update(xl_mean=np.empty(n), P_mean=np.empty((n, n), order="F"),
                        traj_sample_iwmax=np.empty((nN, Tdone), order="F"))
        if full and want_xn_traj or (not full):
            bufs["xn_traj"] = np.empty((nN, N, Tdone), order="F")
        if (extras and full) or not full:
            bufs["final_xn"] = np.empty((nN, N), order="F")
            bufs["final_xl"] = np.empty((n, N), order="F")
            bufs["final_P"] = np.empty((n, n, N), order="F")
        if extras and full:
            bufs["trace_logw"] = np.empty((N, Tdone), order="F")
            bufs["trace_w"] = np.empty((N, Tdone), order="F")
            bufs["trace_ai"] = np.empty((N, Tdone), dtype=np.int32, order="F")
        bufs["iw_max"] = np.zeros(1, dtype=np.int32)
        for k, v in bufs.items():
            setattr(o, k, _ip(v) if v.dtype == np.int32 else _dp(v))
        return o, bufs

    hook_error = []
    hook = None
    if makePlots is not None:
        def on_step(view_p, _user):
            # the plot hook wants the particle cloud after every step (particleFilter.m:215-217)
            try:
                v = view_p.contents
                t = int(v.t)
                o, b = alloc_out(t + 1, full=False)
                check(lib.rbpf_filter_finish(C.c_void_p(v.ctx), C.byref(o)))
                yhattraj = np.full((prob.ny, T), np.nan)
                xn_traj = np.zeros((nN, N, T))
                xn_traj[:, :, :t + 1] = b["xn_traj"]
                makePlots(b["final_xn"], b["xl_max"], b["P_max"], b["traj_max"], yhattraj, xn_traj, b["traj_mean"],
                          b["final_xl"], b["final_P"])
                return 0
            except Exception as exc:                                                      # noqa: BLE001
                hook_error.append(exc)
                return 1
        hook = _ffi.ON_STEP_FN(on_step)
        opt.on_step = hook

    ctx = C.c_void_p()
    check(lib.rbpf_filter_create(C.byref(mdesc), C.byref(prob.c), C.byref(blk), C.byref(opt), C.byref(ctx)))
    try:
        try:
            if handles is not None:
                driver = (_SparseDeviceDriver if model.sparse else _DeviceDriver)(lib, ctx, handles, model, prob)    # (alive until the context is gone: it owns what the last step reads)
                driver.advance(T)
            else:
                check(lib.rbpf_filter_advance(ctx, T))
        except RBPFError as exc:
            if exc.status == _ffi.RBPF_ERR_CALLBACK and hook_error:
                raise hook_error[0] from exc
            _raise_callback_error(model, exc)
        o, b = alloc_out(T, full=True)
        check(lib.rbpf_filter_finish(ctx, C.byref(o)))
        n_fallbacks = C.c_int64(0)
        yhattraj = None
        if extras:
            check(lib.rbpf_filter_resample_fallbacks(ctx, C.byref(n_fallbacks)))
            if isinstance(handles, DeviceSparseHandles):
                yhattraj = driver.yhattraj()
    finally:
        lib.rbpf_destroy(ctx)
    xn_traj = b.get("xn_traj")
    res = (b["traj_max"], b["traj_mean"], b["xl_max"], b["xl_mean"], b["P_max"], b["P_mean"],
           b["traj_sample_iwmax"], xn_traj)
    if extras:
        ex = dict(logw=b["trace_logw"].T.copy(), w=b["trace_w"].T.copy(), ai=b["trace_ai"].T.copy(),
                  xn=b["final_xn"], xl=b["final_xl"], P=b["final_P"], iw_max=int(b["iw_max"][0]),
                  resample_fallbacks=int(n_fallbacks.value))
        if yhattraj is not None:
            ex["yhattraj"] = yhattraj
        return res + (ex,)
    return res


def particle_filter_external(dynModel, measModel, odometry, y, x0_nonLin, x0_lin, P0_lin, Q, R, N_P, dt, rng=None):
    """The caller-driven form of the generic family (what a binding without callback support would do): one host round trip
    per step through rbpf_filter_ancestors / rbpf_filter_step_external.  Same results as particleFilter with the same
    callables; returns (traj_max, traj_mean, xl_max, P_max)."""
    lib = load_library()
    model = _generic_model(None, None, None, odometry, y, x0_nonLin, x0_lin, Q, dt)
    prob = _Problem(model, odometry, y, x0_nonLin, x0_lin, P0_lin, Q, R, N_P, dt)
    nN, n, N, T, d = model.nNonLin, model.nLin, prob.N_P, prob.N_T, model.ny
    if isinstance(rng, ReplayRNG) and (rng.Z is None or rng.Z.size == 0):
        rng = ReplayRNG(rng.U, np.zeros(rng.U.shape + (model.nw,)), rng.Ufin)
    blk, _keep = _rng_block(rng, N, T, model.nw, 1)
    opt = _ffi.rbpf_options(keep_history=1, trace=0, fix_p_mean=0, lazy_depth=0, jitter=0.0)
    mdesc = model.descriptor()
    ctx = C.c_void_p()
    check(lib.rbpf_filter_create(C.byref(mdesc), C.byref(prob.c), C.byref(blk), C.byref(opt), C.byref(ctx)))
    try:
        xn = np.asfortranarray(np.repeat(np.asarray(x0_nonLin, dtype=np.float64).reshape(-1, 1), N, axis=1))   # :59
        ai = np.zeros(N, dtype=np.int32)
        xprev = np.empty((nN, N), order="F")
        for t in range(T):
            if t > 0:
                check(lib.rbpf_filter_ancestors(ctx, _ip(ai), _dp(xprev)))
                xn = np.empty((nN, N), order="F")
                for i in range(N):                                                    # :104-109
                    xn[:, i] = np.asarray(dynModel(xprev[:, ai[i]].copy(), model._odo[t - 1, :], model._dtt(t - 1), model._Qt(t - 1)),
                                          dtype=np.float64).ravel()
            dy = np.asarray(measModel(xn), dtype=np.float64)                           # :124
            if dy.ndim == 2:
                dy = dy.reshape(N, 1, n)
            check(lib.rbpf_filter_step_external(ctx, _dp(np.asfortranarray(xn)), _dp(np.asfortranarray(dy))))
        o = _ffi.rbpf_filter_out()
        b = dict(traj_max=np.empty((nN, T), order="F"), traj_mean=np.empty((nN, T), order="F"), xl_max=np.empty(n),
                 P_max=np.empty((n, n), order="F"))
        for k, v in b.items():
            setattr(o, k, _dp(v))
        check(lib.rbpf_filter_finish(ctx, C.byref(o)))
    finally:
        lib.rbpf_destroy(ctx)
    return b["traj_max"], b["traj_mean"], b["xl_max"], b["P_max"]


def model_dyn_res_norm(dynModel):
    mdl = getattr(dynModel, "model", None)
    return mdl.dynResNorm if isinstance(mdl, _ModelFamily) else None


def _refuse_sparse_smoother(model, y, lazy_depth, inplace, storage):
    """The refusals of rbpf_particle_smoother_sparse_device that depend on the options and the sizes, made here as well: the binding
    calls measModel once before the run (the layouts), and a refused run calls no handle."""
    who = "generic sparse family (sparseFeatures = true with device handles): "
    if _storage_code(storage) != 0:
        raise RBPFError(_ffi.RBPF_ERR_UNSUPPORTED, who + "options.storage must be 0 (fp64 full squares)")
    if int(lazy_depth) >= 2:
        raise RBPFError(_ffi.RBPF_ERR_UNSUPPORTED, who + "lazy_depth >= 2 is not supported (the EKF update rewrites every covariance "
                                                         "at every step)")
    if int(inplace) > 0:
        raise RBPFError(_ffi.RBPF_ERR_UNSUPPORTED, who + "inplace = 1 is not supported (one covariance bank needs lazy_depth >= 2)")
    if not 1 <= model.ny <= 32:
        raise RBPFError(_ffi.RBPF_ERR_UNSUPPORTED, "generic sparse family: n_y must be 1 .. 32")
    if not 1 <= model.nLin <= 96:
        raise RBPFError(_ffi.RBPF_ERR_UNSUPPORTED, "generic sparse family: nLin must be 1 .. 96 (the border-only bank layout)")
    y2 = np.asarray(y, dtype=np.float64)
    y2 = y2.reshape(-1, 1) if y2.ndim == 1 else y2
    if int(np.count_nonzero(~np.isnan(y2[1:]))) > 1023:
        raise RBPFError(_ffi.RBPF_ERR_UNSUPPORTED, "sparse smoother: more than 1023 future observations (particleSmoother.m:197-212 "
                                                   "stacks them all)")


def _smoother(info_form, dynModel, measModel, dynResNorm, odometry, y, x0_nonLin, x0_lin, P0_lin, Q, R, N_P, N_K, dt,
              sparseFeatures, makePlots, rng, extras, chol_variant=0, lazy_depth=0, chol_refresh=0, n_devices=0, device_ids=None,
              storage="fp64", exchange_capacity=0, inplace=0, info_rebuild=0):
    handles = dynModel if isinstance(dynModel, (DeviceSmootherHandles, DeviceSparseSmootherHandles)) else None
    sparse_handles = isinstance(handles, DeviceSparseSmootherHandles)
    if handles is None:
        _refuse_device_handles("the smoothers", dynModel, measModel, dynResNorm)
    elif sparse_handles:                                      # sparseFeatures = true with device code (see DeviceSparseSmootherHandles)
        if (measModel is not None and measModel is not handles) or not (_is_empty_handle(dynResNorm) or dynResNorm is handles):
            raise RBPFError(_ffi.RBPF_ERR_INVALID_ARG, "DeviceSparseSmootherHandles replace the three handles: pass the object as "
                                                       "dynModel and None as measModel and dynResNorm")
        if info_form:
            # particleSmootherInformationForm.m:77-80 prints and returns with outputs unassigned (oracle quirk Q5)
            raise RBPFError(_ffi.RBPF_ERR_UNSUPPORTED, "DeviceSparseSmootherHandles: the information form has only been implemented for "
                                                       "dense features (the reference's returns nothing for sparseFeatures): use "
                                                       "particleSmoother")
        if not sparseFeatures:
            raise RBPFError(_ffi.RBPF_ERR_INVALID_ARG, "DeviceSparseSmootherHandles need sparseFeatures=True: their measModel returns "
                                                       "(yhat, dy) at every particle's own map")
        if int(n_devices) > 1 or (int(n_devices) == 1 and device_ids is not None):
            raise RBPFError(_ffi.RBPF_ERR_UNSUPPORTED, "DeviceSparseSmootherHandles are not supported by sharded sessions (n_devices): "
                                                       "the sparseFeatures branch is not sharded")
        dynModel = measModel = dynResNorm = None
    else:                                                     # device code: no host callbacks (see DeviceSmootherHandles)
        if (measModel is not None and measModel is not handles) or not (_is_empty_handle(dynResNorm) or dynResNorm is handles):
            raise RBPFError(_ffi.RBPF_ERR_INVALID_ARG, "DeviceSmootherHandles replace the three handles: pass the object as "
                                                       "dynModel and None as measModel and dynResNorm")
        if int(n_devices) > 1 or (int(n_devices) == 1 and device_ids is not None):
            raise RBPFError(_ffi.RBPF_ERR_UNSUPPORTED, "DeviceSmootherHandles are not supported by sharded sessions (n_devices): "
                                                       "the smoothers with device handles run on one GPU only")
        if sparseFeatures:
            raise RBPFError(_ffi.RBPF_ERR_UNSUPPORTED, "DeviceSmootherHandles: sparseFeatures=true is implemented for the "
                                                       "sparse-visual family only")
        dynModel = measModel = dynResNorm = None
    if sparseFeatures:
        if info_form:
            # particleSmootherInformationForm.m:77-80 prints and returns with outputs unassigned
            raise RBPFError(_ffi.RBPF_ERR_UNSUPPORTED, "This code has only been implemented for dense features")
    model, use_drn = (None, False) if handles is not None else _recognise(dynModel, measModel, dynResNorm)
    if sparse_handles:
        model = _generic_model(None, None, None, odometry, y, x0_nonLin, x0_lin, Q, dt, sparse=True)
        _refuse_sparse_smoother(model, y, lazy_depth, inplace, storage)      # what the library would refuse, before a handle is called
    if model is None:
        # arbitrary handles (particleSmoother.m:134-136,175-180,264 accept any): the generic family through callbacks
        if sparseFeatures:
            raise RBPFError(_ffi.RBPF_ERR_UNSUPPORTED, "sparseFeatures=true is implemented for the sparse-visual family only")
        model = _generic_model(dynModel, measModel, dynResNorm, odometry, y, x0_nonLin, x0_lin, Q, dt)
    _check_sparse_flag(model, sparseFeatures)
    lib = load_library()
    prob = _Problem(model, odometry, y, x0_nonLin, x0_lin, P0_lin, Q, R, N_P, dt)
    N_K = int(N_K)
    nN, n, N, T = model.nNonLin, model.nLin, prob.N_P, prob.N_T
    if isinstance(model, (GenericDenseModel, GenericSparseModel)) and isinstance(rng, ReplayRNG) and (rng.Z is None or rng.Z.size == 0):
        rng = ReplayRNG(rng.U, np.zeros(rng.U.shape + (model.nw,)), rng.Ufin)
    blk, _keep = _rng_block(rng, prob.N_P, prob.N_T, model.nw, N_K)
    opt = _ffi.rbpf_options(keep_history=1, trace=1 if extras else 0, fix_p_mean=0, lazy_depth=int(lazy_depth), jitter=0.0,
                            chol_variant=int(chol_variant), chol_refresh=int(chol_refresh), storage=_storage_code(storage),
                            inplace=int(inplace), info_rebuild=int(info_rebuild))
    if int(n_devices) > 1 or (int(n_devices) == 1 and device_ids is not None):
        if extras:
            raise RBPFError(_ffi.RBPF_ERR_UNSUPPORTED, "n_devices: traces are not gathered from the sharded smoother")
        opt.n_devices = int(n_devices)
        opt.exchange_capacity = int(exchange_capacity)
        if device_ids is not None:
            _ids = (C.c_int32 * int(n_devices))(*[int(v) for v in device_ids])
            opt.device_ids = C.cast(_ids, C.POINTER(C.c_int32))
    mdesc = model.descriptor(use_dyn_res_norm=use_drn)
    o = _ffi.rbpf_smoother_out()
    b = dict(XNK=np.full((nN, T, N_K), np.nan, order="F"), XLK=np.full((n, N_K), np.nan, order="F"),
             PK=np.full((n, n, N_K), np.nan, order="F"))
    if extras:
        b.update(trace_logw=np.empty((N, T, N_K), order="F"), trace_w=np.empty((N, T, N_K), order="F"),
                 trace_ai=np.zeros((N, T, N_K), dtype=np.int32, order="F"),
                 trace_paNt=np.full((N, T, N_K), np.nan, order="F"), trace_ak=np.zeros(N_K, dtype=np.int32))
    for k, v in b.items():
        setattr(o, k, _ip(v) if v.dtype == np.int32 else _dp(v))
    hook_error = []
    if makePlots is not None:
        def on_iter(view_p, _user):                            # particleSmoother.m:360-362, after every iteration
            try:
                k = int(view_p.contents.t)
                makePlots(b["XNK"][:, :, k], b["XLK"][:, k], k, b["XNK"], b["XLK"], b["PK"])
                return 0
            except Exception as exc:                                                      # noqa: BLE001
                hook_error.append(exc)
                return 1
        hook = _ffi.ON_STEP_FN(on_iter)
        opt.on_step = hook
    driver = None
    try:
        if sparse_handles:
            driver = _SparseSmootherCallbacks(lib, handles, model, prob)
            check(lib.rbpf_particle_smoother_sparse_device(C.byref(mdesc), C.byref(prob.c), C.byref(blk), C.byref(opt), N_K,
                                                           driver._fns[0], driver._fns[1], driver._fns[2], None,
                                                           driver.yhat_layout, driver.dy_layout, driver.future, C.byref(o)))
        elif handles is not None:
            driver = _DeviceSmootherCallbacks(lib, handles, model, prob)
            check(lib.rbpf_particle_smoother_device(C.byref(mdesc), C.byref(prob.c), C.byref(blk), C.byref(opt), N_K,
                                                    1 if info_form else 0, C.byref(driver.cb), driver.layout, C.byref(o)))
        else:
            check(lib.rbpf_particle_smoother(C.byref(mdesc), C.byref(prob.c), C.byref(blk), C.byref(opt), N_K,
                                             1 if info_form else 0, C.byref(o)))
    except RBPFError as exc:
        if exc.status == _ffi.RBPF_ERR_CALLBACK and hook_error:
            raise hook_error[0] from exc
        _raise_callback_error(driver if driver is not None else model, exc)
    res = (b["XNK"], b["XLK"], b["PK"])
    if extras:
        ex = dict(logw=np.transpose(b["trace_logw"], (2, 1, 0)).copy(), w=np.transpose(b["trace_w"], (2, 1, 0)).copy(),
                  ai=np.transpose(b["trace_ai"], (2, 1, 0)).copy(), paNt=np.transpose(b["trace_paNt"], (2, 1, 0)).copy(),
                  ak=b["trace_ak"])
        return res + (ex,)
    return res


def particleSmoother(dynModel, measModel, dynResNorm, odometry, y, x0_nonLin, x0_lin, P0_lin, Q, R, N_P, N_K, dt,
                     sparseFeatures=False, makePlots=None, *, rng=None, extras=False, chol_variant=0, storage="fp64",
                     lazy_depth=0, inplace=0, n_devices=0, device_ids=None):
    """Mirror of src/particleSmoother.m:1-2 (covariance-form ancestor weights) -> (XNK, XLK, PK).
    sparseFeatures=True runs for the sparse-visual family, and for ANY model whose handles are device code: a
    DeviceSparseSmootherHandles object as dynModel (see there).  The covariance form rewrites every covariance at every step, so
    lazy_depth is ignored and inplace refused; n_devices is what it is for particleSmootherInformationForm."""
    return _smoother(False, dynModel, measModel, dynResNorm, odometry, y, x0_nonLin, x0_lin, P0_lin, Q, R, N_P, N_K,
                     dt, sparseFeatures, makePlots, rng, extras, chol_variant, lazy_depth=lazy_depth, n_devices=n_devices,
                     device_ids=device_ids, storage=storage, inplace=inplace)


def particleSmootherInformationForm(dynModel, measModel, dynResNorm, odometry, y, x0_nonLin, x0_lin, P0_lin, Q, R,
                                    N_P, N_K, dt, sparseFeatures=False, makePlots=None, *, rng=None, extras=False,
                                    chol_variant=0, lazy_depth=0, chol_refresh=0, n_devices=0, device_ids=None, storage="fp64",
                                    exchange_capacity=0, inplace=0, info_rebuild=0):
    """Mirror of src/particleSmootherInformationForm.m:1-2 -> (XNK, XLK, PK).  lazy_depth = C >= 2 (max 3): the stored
    covariances are rewritten every C-th step only (same algebra as :331 every step, results to rounding).
    chol_refresh (rbpf_options.chol_refresh) = K > 1: the ancestor-weight factors (:228) are carried along the lineages by rank-1
    up/down-dates and recomputed every K-th step (every index identical, ancestor probabilities within 2e-9, outputs 1e-9 of the
    from-scratch factorisation); 1: chol(Imat_i + ImatAddt) from scratch at every step, the reference's own arithmetic; 0 (default):
    automatic -- K = 32 for the recognised dense families from nLin = 128 on, 1 elsewhere (`chol_refresh_in_use` tells).
    info_rebuild = 1 (rbpf_options.info_rebuild): no information matrix is stored -- every refresh rebuilds them from the initial
    matrix along the whole ancestral path, chunk by chunk (choose K in the hundreds; K >= N_T - 1 never refreshes and implies it);
    together with inplace = 1 (one covariance bank rewritten in place; needs lazy_depth >= 2) the state is 3.6 MB per particle at
    nLin = 515 -- the metric's N_P = 65 536 on one 288 GB GPU.
    n_devices = W > 1: the particles of every iteration are sharded over W GPUs inside the library (rbpf_options.n_devices)."""
    return _smoother(True, dynModel, measModel, dynResNorm, odometry, y, x0_nonLin, x0_lin, P0_lin, Q, R, N_P, N_K,
                     dt, sparseFeatures, makePlots, rng, extras, chol_variant, lazy_depth, chol_refresh, n_devices, device_ids, storage,
                     exchange_capacity, inplace, info_rebuild)


def chol_refresh_in_use(model, chol_refresh=0):
    """The K rbpf_options.chol_refresh = `chol_refresh` stands for with this model (rbpf_chol_refresh_resolve): > 1 carried
    ancestor-weight factors refreshed every K-th step, 1 the from-scratch factorisation of every step."""
    lib = load_library()
    return int(lib.rbpf_chol_refresh_resolve(int(model.descriptor().kind), int(model.nLin), int(model.ny), int(chol_refresh)))


def sample(w, u):
    """tools/sample.m:30-32 on the device for a batch of uniforms; returns 0-based indices."""
    lib = load_library()
    w = np.ascontiguousarray(np.asarray(w, dtype=np.float64).ravel())
    u = np.ascontiguousarray(np.atleast_1d(np.asarray(u, dtype=np.float64)).ravel())
    ind = np.empty(u.size, dtype=np.int32)
    check(lib.rbpf_sample(w.size, _dp(w), u.size, _dp(u), _ip(ind)))
    return ind


_QUAT_OPS = dict(expq=(0, 3, (4,)), expq_batched=(1, 3, (4,)), logq=(2, 4, (3,)), logq_batched=(3, 4, (3,)),
                 qLeft=(4, 4, (4, 4)), qRight=(5, 4, (4, 4)), qInv=(6, 4, (4,)), quat2rmat=(7, 4, (3, 3)), mcross=(8, 3, (3, 3)))


def quat_helper(name, x):
    """tools/{expq,logq,qLeft,qRight,qInv,quat2rmat,mcross}.m on the device for a batch: x [n x 3] or [n x 4] (rows, as the
    reference's batched branches take them) -> [n x 4] / [n x 3] / [n x 4 x 4] / [n x 3 x 3].  `expq` / `logq` are the scalar
    branches (sign flip on q0 < 0), `*_batched` the batched ones (flip on q0 <= 0, quirk Q7)."""
    op, nin, oshape = _QUAT_OPS[name]
    lib = load_library()
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1, nin))
    n = x.shape[0]
    out = np.empty((n,) + oshape[::-1], dtype=np.float64)          # column-major per item
    check(lib.rbpf_quat_helpers(op, n, _dp(x), _dp(out)))
    return np.transpose(out, (0, 2, 1)).copy() if len(oshape) == 2 else out


def chol_weights(S, e, jitter=0.0, variant=0, reps=1, info_form=False):
    """particleSmoother.m:221-229 for a batch: S [B, M, M] (symmetric; the lower triangle is read), e [B, M] ->
    (logw [B], status, mean kernel ms).  variant 0 / 16 / 64 selects the factorisation kernel (648 / 644: the 64-column kernel
    with 8 / 4 waves; 649: 8 waves, wave 0 forming the early diagonal blocks itself; 128: the 128-column kernel, information form and M >= 432 only; 1: the register-resident kernel,
    information form and 64 <= M <= 143 only).  info_form: the
    information-form loaders and expression of particleSmootherInformationForm.m:224-236 with ImatAddt = ivecAddt = 0:
    logw = -sum(log(diag(cI))) + v'v/2, no retry."""
    lib = load_library()
    S = np.ascontiguousarray(np.asarray(S, dtype=np.float64))
    e = np.ascontiguousarray(np.asarray(e, dtype=np.float64))
    B, M = e.shape
    assert S.shape == (B, M, M)
    St = np.ascontiguousarray(np.transpose(S, (0, 2, 1)))                  # column-major per matrix
    logw = np.empty(B, dtype=np.float64)
    status = np.zeros(1, dtype=np.int32)
    ms = np.zeros(1, dtype=np.float64)
    check(lib.rbpf_chol_weights(M, B, _dp(St), _dp(e), float(jitter), int(variant) + (1000 if info_form else 0), int(reps),
                                _dp(logw), _ip(status), _dp(ms)))
    return logw, int(status[0]), float(ms[0])


def chol_sweep_probe(L, U, V, eta, batch=1, reps=1):
    """The sweep kernel of the carried ancestor-weight factors (rbpf_options.chol_refresh) on its own: L [(n+1) x (n+1)] lower,
    the augmented factor [chol(A) 0; z' *]; U, V [d x n] update / downdate vectors (rows); eta [d] their entry in the augmented
    row.  Returns (L_out, logw, status, mean kernel ms): the factor of A + U'U - V'V with the carried row, and
    -sum(log(diag)) + z'z/2.  `batch` copies are swept (timing); copy 0 is returned."""
    lib = load_library()
    L = np.asfortranarray(np.asarray(L, dtype=np.float64))
    U = np.asfortranarray(np.asarray(U, dtype=np.float64))
    V = np.asfortranarray(np.asarray(V, dtype=np.float64))
    eta = np.ascontiguousarray(np.asarray(eta, dtype=np.float64))
    d, n = U.shape
    assert L.shape == (n + 1, n + 1) and V.shape == (d, n) and eta.shape == (d,)
    Lo = np.zeros((n + 1, n + 1), order="F")
    logw = np.zeros(1)
    status = np.zeros(1, dtype=np.int32)
    ms = np.zeros(1)
    check(lib.rbpf_chol_sweep_probe(n, d, int(batch), _dp(L), _dp(U), _dp(V), _dp(eta), int(reps), _dp(Lo), _dp(logw), _ip(status), _dp(ms)))
    return Lo, float(logw[0]), int(status[0]), float(ms[0])


def pack_whiten_probe(dy, W, dy_layout=0, fused=True):
    """rbpf_ext_pack_whiten_probe: G (rows, n_y, nLin) = W @ dy[i] for dy (rows, n_y, nLin), handed to the device in dy_layout 0
    (MATLAB order) or 2 (C-contiguous).  fused=True: the pack-and-whiten kernel of the refreshes with device handles; False: the
    pack kernel followed by the whitening kernel of the built-in families' refreshes -- the same bits."""
    lib = load_library()
    dy = np.asarray(dy, dtype=np.float64)
    rows, d, n = dy.shape
    W = np.asfortranarray(np.asarray(W, dtype=np.float64))
    assert W.shape == (d, d)
    mem = np.asfortranarray(dy) if int(dy_layout) == 0 else np.ascontiguousarray(dy)
    G = np.empty((rows, d, n))
    check(lib.rbpf_ext_pack_whiten_probe(int(dy_layout), rows, d, n, _dp(mem), _dp(W), 1 if fused else 0, _dp(G)))
    return G


def sparse_smoother_timing(enable):
    """Switch the per-step HIP-event timing of particleSmoother with DeviceSparseSmootherHandles on or off
    (rbpf_sparse_smoother_timing) and return the totals since the last call: dict(build_ms, chol_ms, steps) -- milliseconds in the
    build kernel and in the batched factorisation of the ancestor weights, and the number of timed steps."""
    lib = load_library()
    b, f, n = C.c_double(0.0), C.c_double(0.0), C.c_int64(0)
    check(lib.rbpf_sparse_smoother_timing(1 if enable else 0, C.byref(b), C.byref(f), C.byref(n)))
    return dict(build_ms=float(b.value), chol_ms=float(f.value), steps=int(n.value))


def sparse_ext_build_probe(P, D, pair_t, pair_j, R, reps=1, out=None):
    """The build kernel of the sparse smoother with device handles on its own (rbpf_sparse_ext_build_probe), on torch device tensors:
    P (N, n, n) symmetric, D (N, M, n), pair_t / pair_j (M,) int32 -- the time and the output of every stacked row -- and R (d, d)
    -> (S (N, M, M) with S[i, a, b] = (D_i P_i D_i')(a, b) + (pair_t[a] == pair_t[b]) R[pair_j[a], pair_j[b]] in the 16 x 16 tiles on
    and below the diagonal, mean kernel time in ms).  The tiles above the diagonal are not written: they keep what `out`
    (N, M, M), viewed as the kernel's column-major matrices, held (NaN when out is None)."""
    import torch
    lib = load_library()
    N, M, n = (int(v) for v in D.shape)
    d = int(R.shape[0])
    f64 = dict(dtype=torch.float64, device=D.device)
    Pc, Dc = P.to(**f64).contiguous(), D.to(**f64).contiguous()
    Rc = R.to(**f64).t().contiguous()                                  # column-major
    pt = pair_t.to(dtype=torch.int32, device=D.device).contiguous()
    pj = pair_j.to(dtype=torch.int32, device=D.device).contiguous()
    if tuple(Pc.shape) != (N, n, n) or tuple(pt.shape) != (M,) or tuple(pj.shape) != (M,) or tuple(R.shape) != (d, d):
        raise ValueError("P (N, n, n), D (N, M, n), pair_t / pair_j (M,), R (d, d)")
    S = torch.full((N, M, M), float("nan"), **f64) if out is None else out     # [i][b][a]: column-major matrices
    torch.cuda.synchronize(D.device)                                   # the kernel runs on the null stream
    ms = C.c_double(0.0)
    check(lib.rbpf_sparse_ext_build_probe(N, n, M, d, C.c_void_p(Pc.data_ptr()), C.c_void_p(Dc.data_ptr()), C.c_void_p(pt.data_ptr()),
                                          C.c_void_p(pj.data_ptr()), C.c_void_p(Rc.data_ptr()), int(reps), C.c_void_p(S.data_ptr()),
                                          C.byref(ms)))
    return S.transpose(1, 2), float(ms.value)


# ------------------------------------------------------------------------------------------------
# resident-state driver used by bench.py (inputs already in HBM when the timed region starts)
# ------------------------------------------------------------------------------------------------
class FilterSession:
    """Thin RAII wrapper over rbpf_filter_create / advance / sync / timing / destroy."""

    def __init__(self, model, odometry, y, x0_nonLin, x0_lin, P0_lin, Q, R, N_P, dt, rng=None, keep_history=False,
                 trace=False, lazy_depth=0, inplace=0, storage="fp64"):
        self.lib = load_library()
        handles = model if isinstance(model, DeviceHandles) else None
        if handles is not None:                                # device code in place of a model: the generic family, caller-driven
            model = _generic_model(None, None, None, odometry, y, x0_nonLin, x0_lin, Q, dt,
                                   sparse=isinstance(handles, DeviceSparseHandles))
            if isinstance(rng, ReplayRNG) and (rng.Z is None or rng.Z.size == 0):
                rng = ReplayRNG(rng.U, np.zeros(rng.U.shape + (model.nw,)), rng.Ufin)
        self.model = model
        self._driver = None
        self.prob = _Problem(model, odometry, y, x0_nonLin, x0_lin, P0_lin, Q, R, N_P, dt)
        self.blk, self._rng = _rng_block(rng, self.prob.N_P, self.prob.N_T, model.nw, 1)
        self.opt = _ffi.rbpf_options(keep_history=1 if keep_history else 0, trace=1 if trace else 0, fix_p_mean=0,
                                     lazy_depth=int(lazy_depth), jitter=0.0, inplace=int(inplace),
                                     storage=_storage_code(storage))
        self.mdesc = model.descriptor()
        self.ctx = C.c_void_p()
        check(self.lib.rbpf_filter_create(C.byref(self.mdesc), C.byref(self.prob.c), C.byref(self.blk),
                                          C.byref(self.opt), C.byref(self.ctx)))
        if handles is not None:
            try:
                self._driver = (_SparseDeviceDriver if model.sparse else _DeviceDriver)(self.lib, self.ctx, handles, model, self.prob)
            except Exception:
                self.close()
                raise

    def advance(self, n_steps):
        if self._driver is not None:
            return self._driver.advance(n_steps)
        check(self.lib.rbpf_filter_advance(self.ctx, int(n_steps)))

    def reset(self):
        check(self.lib.rbpf_filter_reset(self.ctx))

    def sync(self):
        check(self.lib.rbpf_sync(self.ctx))

    def tell(self):
        t = C.c_int32(0)
        check(self.lib.rbpf_filter_tell(self.ctx, C.byref(t)))
        return t.value

    def schedule(self):
        """(banks, shared_flush) the context chose (rbpf_filter_schedule)."""
        b, sf = C.c_int32(0), C.c_int32(0)
        check(self.lib.rbpf_filter_schedule(self.ctx, C.byref(b), C.byref(sf)))
        return b.value, bool(sf.value)

    @property
    def banks(self):
        return self.schedule()[0]

    def one_launch_flushes(self):
        """Shared flush steps so far that ran as one launch (rbpf_filter_one_launch_flushes)."""
        n = C.c_int64(0)
        check(self.lib.rbpf_filter_one_launch_flushes(self.ctx, C.byref(n)))
        return n.value

    def resample_fallbacks(self):
        """Resampling steps so far that were recomputed with the strict cumsum (rbpf_filter_resample_fallbacks)."""
        n = C.c_int64(0)
        check(self.lib.rbpf_filter_resample_fallbacks(self.ctx, C.byref(n)))
        return n.value

    def timing(self, enable=None, reset=False):
        if enable is not None:
            check(self.lib.rbpf_timing_enable(self.ctx, 1 if enable else 0))
            return None
        tm = _ffi.rbpf_timing()
        check(self.lib.rbpf_timing_read(self.ctx, C.byref(tm), 1 if reset else 0))
        return dict(ms=tm.stream_kernel_ms, launches=tm.stream_kernel_launches,
                    bytes_per_launch=tm.algorithmic_bytes_per_launch,
                    scheduled_bytes_per_launch=tm.scheduled_bytes_per_launch)

    def finish(self, want=("traj_max", "traj_mean", "xl_max", "P_max")):
        """Any subset of the reference's outputs (particleFilter.m:220-233) and of the extras of rbpf_filter_out, as of the
        last finished step.  trace_* need trace=True, traj_sample_iwmax / xn_traj / trace_ai need keep_history=True; yhattraj
        (n_y, N_T) is kept for DeviceSparseHandles only."""
        m = self.model
        nN, n, N, T, Td = m.nNonLin, m.nLin, self.prob.N_P, self.prob.N_T, self.tell()
        shapes = dict(traj_max=(nN, T), traj_mean=(nN, T), xl_max=(n,), xl_mean=(n,), P_max=(n, n), P_mean=(n, n),
                      traj_sample_iwmax=(nN, Td), xn_traj=(nN, N, Td), trace_logw=(N, Td), trace_w=(N, Td), trace_ai=(N, Td),
                      final_xn=(nN, N), final_xl=(n, N), final_P=(n, n, N))
        o = _ffi.rbpf_filter_out()
        b = {}
        for k in want:
            if k == "yhattraj":
                continue
            b[k] = np.empty(shapes[k], dtype=np.int32 if k == "trace_ai" else np.float64, order="F")
            setattr(o, k, _ip(b[k]) if k == "trace_ai" else _dp(b[k]))
        b["iw_max"] = np.zeros(1, dtype=np.int32)
        o.iw_max = _ip(b["iw_max"])
        check(self.lib.rbpf_filter_finish(self.ctx, C.byref(o)))
        if "yhattraj" in want:
            if not isinstance(self._driver, _SparseDeviceDriver):
                raise RBPFError(_ffi.RBPF_ERR_STATE, "yhattraj is kept for DeviceSparseHandles only")
            b["yhattraj"] = self._driver.yhattraj()
        return b

    def close(self):
        if self.ctx:
            self.lib.rbpf_destroy(self.ctx)
            self.ctx = C.c_void_p()
        self._driver = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


# ------------------------------------------------------------------------------------------------
# localisation in a fixed GP map: examples/mag-localization-mapping
# ------------------------------------------------------------------------------------------------
def _grad_rows(NN, L, x):
    """Rows of [e_c, d_c Phi(x)] for c = x, y, z: three [N x (m + 3)] arrays (run_localization.m:135-142; per-axis tables
    instead of tools/domain_cartesian_dx.m:146-170's m x d loops, same products)."""
    NN = np.asarray(NN, dtype=np.int64)
    L = np.asarray(L, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    S, Cc, D = [], [], []
    for a in range(3):
        arg = np.pi * NN[None, :, a] * (x[:, a:a + 1] + L[a]) / (2.0 * L[a])
        S.append(1.0 / math.sqrt(L[a]) * np.sin(arg))
        Cc.append(np.pi * NN[None, :, a] / (2.0 * L[a] * math.sqrt(L[a])) * np.cos(arg))
    N, m = x.shape[0], NN.shape[0]
    rows = []
    for c in range(3):
        v = np.ones((N, m))
        for a in range(3):
            v = v * (Cc[a] if a == c else S[a])
        lin = np.zeros((N, 3))
        lin[:, c] = 1.0
        rows.append(np.hstack((lin, v)))
    return rows


def _lower_factor(P):
    """V lower with V'V = P (symmetrised first): the transposed Cholesky factor of the index-reversed matrix, reversed back.
    ValueError when P is not positive definite."""
    P = np.asarray(P, dtype=np.float64)
    P = 0.5 * (P + P.T)
    try:
        Cr = np.linalg.cholesky(P[::-1, ::-1])
    except np.linalg.LinAlgError as exc:
        raise ValueError("P is not positive definite") from exc
    return Cr.T[::-1, ::-1]


class DenseMagMap:
    """A fixed map of the dense-mag family: the posterior N(mean, V'V) over the m + 3 basis coefficients, as the SLAM filter /
    smoothers return it (xl_max, P_max / XLK, PK) or as the batch regression of run_localization.m:134-151 computes it.  Its
    `dynModel` / `measModel` are the closures of run_localization.m:274-281 / :241-272 and are recognised by
    particleFilterLocalization.

    var_points=None: every particle gets the predictive variance at its own position (the evident intent of :261-263).
    var_points=[>= N_P x 3]: the reference's literal behaviour (quirk Q10): the variances at those points are computed once on
    the device and particle slot i uses row i."""

    def __init__(self, model, mean, V, sigma2, var_points=None):
        if not isinstance(model, DenseMagModel):
            raise TypeError("DenseMagMap needs a DenseMagModel")
        self.model = model
        n = model.nLin
        self.mean = np.ascontiguousarray(np.asarray(mean, dtype=np.float64).ravel())
        self.V = np.asfortranarray(np.tril(np.asarray(V, dtype=np.float64)))
        self.sigma2 = float(sigma2)
        if self.mean.size != n or self.V.shape != (n, n):
            raise ValueError("mean must be [m + 3] and V [(m + 3) x (m + 3)]")
        self.var_points = None if var_points is None else np.asarray(var_points, dtype=np.float64).reshape(-1, 3)
        self._var_table = None
        self.dynModel = _Handle(self, "dynModel")
        self.measModel = _Handle(self, "measModel")

    @classmethod
    def from_posterior(cls, model, xl, P, sigma2, var_points=None):
        """From a map posterior (mean xl, covariance P).  V = lower factor with V'V = P: the transposed Cholesky factor of the
        index-reversed matrix, reversed back."""
        return cls(model, xl, _lower_factor(P), sigma2, var_points)

    @classmethod
    def from_data(cls, model, x, y, theta, var_points=None):
        """Batch GP regression of run_localization.m:119-151: x [N x 3] positions (domain coordinates), y [N x 3] field
        measurements in the navigation frame, theta = (linSigma2, lengthScale, magnSigma2, sigma2)."""
        linSigma2, lengthScale, magnSigma2, sigma2 = (float(t) for t in np.asarray(theta).ravel())
        lam = eigenval(model.NN, model.L)
        k = np.concatenate(([linSigma2] * 3, magnSigma2 * math.sqrt(2 * math.pi) ** 3 * lengthScale ** 3 * np.exp(-lam * lengthScale ** 2 / 2)))
        Phi = np.vstack(_grad_rows(model.NN, model.L, x))                                   # :145
        y = np.asarray(y, dtype=np.float64).reshape(-1, 3)
        Phiy = Phi.T @ y.reshape(-1, order="F")                                              # :147
        Lc = np.linalg.cholesky(Phi.T @ Phi + np.diag(sigma2 / k))                           # :150
        import scipy.linalg as sla
        foo = sla.solve_triangular(Lc.T, sla.solve_triangular(Lc, Phiy, lower=True), lower=False)   # :151
        V = math.sqrt(sigma2) * sla.solve_triangular(Lc, np.eye(Lc.shape[0]), lower=True)   # dVarft = sigma2 |L \ g|^2 (:261)
        return cls(model, foo, V, sigma2, var_points)

    def _map_struct(self, table=None, with_V=True):
        mp = _ffi.rbpf_loc_map()
        mp.m_basis = self.model.m
        self._nn_f = np.asfortranarray(self.model.NN)
        mp.NN = _ip(self._nn_f)
        for a in range(3):
            mp.L[a] = float(self.model.L[a])
        mp.mean = _dp(self.mean)
        mp.sigma2 = self.sigma2
        if table is not None:
            mp.var_table = _dp(table)
        elif with_V:
            mp.V = _dp(self.V)
        return mp

    def predict(self, xn, reps=1, want_var=True):
        """The prediction kernel on its own (rbpf_loc_predict): xn [7 x n_pred] (or [3 x n_pred] positions) ->
        (dEft [n_pred x 3], var [n_pred x 3], median kernel ms)."""
        lib = load_library()
        xn = np.asarray(xn, dtype=np.float64)
        if xn.shape[0] == 3:
            xn = np.vstack((xn.reshape(3, -1), np.tile(np.array([[1.0], [0.0], [0.0], [0.0]]), (1, xn.reshape(3, -1).shape[1]))))
        xn = np.asfortranarray(xn.reshape(7, -1))
        npred = xn.shape[1]
        dE = np.empty((3, npred), order="F")
        var = np.empty((3, npred), order="F") if want_var else None
        ms = C.c_double(0.0)
        mp = self._map_struct(with_V=want_var)
        check(lib.rbpf_loc_predict(C.byref(mp), npred, _dp(xn), _dp(dE), _dp(var) if want_var else None, int(reps), C.byref(ms)))
        return dE.T.copy(), (var.T.copy() if want_var else None), ms.value

    def _loc_map(self, N_P):
        """rbpf_loc_map for a run with N_P particles (the variance table of var_points is computed here, once)."""
        if self.var_points is None:
            return self._map_struct()
        if self.var_points.shape[0] < N_P:
            raise ValueError(f"var_points has {self.var_points.shape[0]} rows, fewer than N_P = {N_P} (index out of bounds in the reference)")
        _, var, _ = self.predict(self.var_points[:N_P].T)
        self._var_table = np.asfortranarray(var)                                            # [N_P x 3]
        return self._map_struct(table=self._var_table)

    def _evaluate(self, role, *args):
        if role == "dynModel":
            xn, dx, dt, Q, z = args
            lib = load_library()
            xn = np.asfortranarray(np.asarray(xn, dtype=np.float64).reshape(7, -1))
            npar = xn.shape[1]
            z = np.asfortranarray(np.asarray(z, dtype=np.float64).reshape(6, npar))
            dx = np.ascontiguousarray(np.asarray(dx, dtype=np.float64).ravel())
            Q = np.asfortranarray(np.asarray(Q, dtype=np.float64).reshape(6, 6))
            out = np.empty_like(xn)
            check(lib.rbpf_loc_dyn_model(npar, _dp(xn), _dp(dx), float(dt), _dp(Q), _dp(z), _dp(out)))
            return out[:, 0] if npar == 1 else out
        raise RBPFError(_ffi.RBPF_ERR_UNSUPPORTED, "the localisation measModel is only evaluated inside particleFilterLocalization")


class _LocProblem:
    def __init__(self, odometry, y, x0_nonLin, Q, N_P, dt):
        y = np.asarray(y, dtype=np.float64)
        self.N_T, self.N_P = y.shape[0], int(N_P)
        if y.ndim != 2 or y.shape[1] != 3:
            raise ValueError("y must be [N_T x 3]")
        self.y = np.asfortranarray(y)
        odo = np.asarray(odometry, dtype=np.float64)
        self.odo = np.asfortranarray(odo.reshape(1, -1) if odo.ndim == 1 else odo)
        x0 = np.asarray(x0_nonLin, dtype=np.float64)
        self.x0 = np.asfortranarray(x0.reshape(7, -1))
        if self.x0.shape[1] not in (1, self.N_P):
            raise ValueError("x0_nonLin must be [7] or [7 x N_P]")
        Q = np.asarray(Q, dtype=np.float64)
        self.Q = np.asfortranarray(Q[:, :, None] if Q.ndim == 2 else Q)
        self.dt = np.ascontiguousarray(np.atleast_1d(np.asarray(dt, dtype=np.float64)).ravel())
        if self.Q.shape[:2] != (6, 6):
            raise ValueError("Q must be [6 x 6] or [6 x 6 x >= N_T-1]")
        if self.N_T > 1 and (self.odo.shape[0] < self.N_T - 1 or self.odo.shape[1] != 7):
            raise ValueError("odometry must be [>= N_T-1 x 7]")
        p = _ffi.rbpf_loc_problem()
        p.N_P, p.N_T, p.x0_cols, p.q_pages, p.dt_len = self.N_P, self.N_T, self.x0.shape[1], self.Q.shape[2], self.dt.size
        p.odo_ld = self.odo.shape[0]
        p.odometry, p.y, p.x0_nonlin, p.Q, p.dt = _dp(self.odo), _dp(self.y), _dp(self.x0), _dp(self.Q), _dp(self.dt)
        self.c = p


def _recognise_map(dynModel, measModel):
    if isinstance(dynModel, DeviceTransition) or isinstance(measModel, DeviceTransition):
        raise RBPFError(_ffi.RBPF_ERR_UNSUPPORTED, "a DeviceTransition states the density of a DeviceMap's dynModel (DeviceMap(..., transition=...)): "
                        "it is no handle, and the dense-mag map has its own transition density")
    mp = getattr(dynModel, "model", None)
    if not isinstance(mp, DenseMagMap) or getattr(measModel, "model", None) is not mp:
        raise RBPFError(_ffi.RBPF_ERR_UNSUPPORTED, "particleFilterLocalization runs the handles of a DenseMagMap, or a DeviceMap as dynModel; a host-callback "
                        "family for arbitrary localisation handles is not implemented")
    return mp


def device_map_weights(dy, mean, V, R, y, dy_layout=2, ldx=None, pad=0.0, reps=1):
    """rbpf_loc_generic_weights, the kernel-level probe of localisation in a generic map: dy [N x n_y x nLin] (the Jacobians of N
    particles), mean [nLin], V [nLin x nLin] lower with V'V = P, R [n_y x n_y], y [n_y] ->
    (yhat [N x n_y] = H_i mean, S [N x n_y x n_y] = H_i P H_i' before R is added, logw [N], median kernel ms over `reps` launches).
    dy_layout: the memory layout dy is handed to the library in -- 0 MATLAB order, 2 C-contiguous, 1 rows on the stride ldx
    (default: the next multiple of 16), the columns behind nLin filled with `pad` (the kernel does not read them)."""
    lib = load_library()
    dy = np.asarray(dy, dtype=np.float64)
    if dy.ndim != 3:
        raise ValueError("dy must be [N x n_y x nLin]")
    N, d, n = dy.shape
    if dy_layout == 0:
        buf = np.asfortranarray(dy)
    elif dy_layout == 1:
        ldx = (n + 15) // 16 * 16 if ldx is None else int(ldx)
        buf = np.full((N, d, max(ldx, n)), float(pad))
        buf[:, :, :n] = dy
    else:
        buf = np.ascontiguousarray(dy)
    mean = np.ascontiguousarray(np.asarray(mean, dtype=np.float64).ravel())
    V = np.asfortranarray(np.tril(np.asarray(V, dtype=np.float64)))
    R = np.asfortranarray(np.asarray(R, dtype=np.float64).reshape(d, d))
    y = np.ascontiguousarray(np.asarray(y, dtype=np.float64).ravel())
    if mean.size != n or V.shape != (n, n) or y.size != d:
        raise ValueError("mean must be [nLin], V [nLin x nLin] and y [n_y]")
    yhat, S, logw = np.empty((N, d)), np.empty((N, d, d)), np.empty(N)
    ms = C.c_double(0.0)
    check(lib.rbpf_loc_generic_weights(d, n, N, _dp(buf), int(dy_layout), int(ldx or 0), _dp(mean), _dp(V), _dp(R), _dp(y), _dp(yhat),
                                       _dp(S), _dp(logw), int(reps), C.byref(ms)))
    return yhat, S, logw, ms.value


class DeviceTransition:
    """The transition density of a DeviceHandles dynModel as it draws, for backward simulation in a DeviceMap: a drift plus Gaussian
    noise on some rows of the state,

        x'[rows] = mean(x) + L z,  L L' = cov:    r = wrap(x'[rows] - mean(x)),   z = L \\ r,   logp = -z'z / 2

    (constants omitted, particleSmoother.m:181-182).
    mean(xn (n_nonlin, N_P), dx, dt, Q) -> (n_res, N_P): torch float64 on the library's device and stream, the predicted rows; it
        must be pure.  Called once per backward step t = N_T-2 .. 0 with the stored forward particles of step t (a view of library
        memory: do not write to it) and odometry[t], dt[t], Q[:,:,t] -- the arguments the forward dynModel got when it made step
        t+1.
    rows: the indices of the n_nonlin state that carry noise (default: all), n_res = len(rows) in 1 .. 8, distinct.  Rows that are
        not listed take NO part in the density, as in the reference's dense-radio dynResNorm (heading only): a trajectory is then
        extended backwards whatever those rows of the candidate particles are.
    angle_rows: a subset of rows whose residual is wrapped, r <- r - 2 pi rint(r / (2 pi)).
    cov(dt, Q) -> (n_res, n_res): a host callable on numpy arrays (default: dt * Q, which needs n_w == n_res), evaluated once per
        step page and factorised on the host; one that is not positive definite is refused before any kernel runs.
    quat_rows: four state rows (q0, q1, q2, q3) that hold a unit quaternion, scalar first (the reference's tools/q*.m), for a pose
        state whose rotation noise multiplies the predicted quaternion on the right, x'_q = mu_q (x) expq(noise)
        (run_dense3D_magfield.m:202-203, run_localization.m:274-281).  All four must be in rows, adjacent there and in that order,
        none in angle_rows; one block at most.  With n_sel = len(rows) in 4 .. 8, mean returns (n_sel, N_P): its four block rows are
        the predicted UNIT quaternion, composed with the odometry by the handle (q (x) dq or dq (x) q).  The residual then has
        n_res = n_sel - 1 entries: the plain rows' differences, and in the block's place the three of

            e = qInv(mu_q) (x) x'_q,   e <- -e if e0 < 0,   phi = atan2(|e_v|, e0) e_v / |e_v|   (0 if |e_v| = 0)

        = logq(e) of tools/logq.m for a unit e.  cov(dt, Q) is (n_res, n_res) in that order.  Not built: noise multiplied on the
        left, two blocks, noise through a non-square G."""

    def __init__(self, mean, cov=None, rows=None, angle_rows=(), quat_rows=None):
        if not callable(mean) or (cov is not None and not callable(cov)):
            raise TypeError("mean must be callable, cov callable or None")
        self.mean, self.cov = mean, cov
        self.rows = None if rows is None else tuple(int(r) for r in rows)
        self.angle_rows = tuple(int(r) for r in angle_rows)
        self.quat_rows = None if quat_rows is None else tuple(int(r) for r in quat_rows)

    def resolve(self, n_nonlin):
        """(rows, angle_mask) for a state of n_nonlin rows, bit k of the mask marks rows[k]; with quat_rows
        (rows, angle_mask, quat_pos), quat_pos the position of q0 in rows: what rbpf_loc_generic_backward_pose_begin takes."""
        rows, mask = _transition_rows(n_nonlin, self.rows, self.angle_rows)
        if self.quat_rows is None:
            return rows, mask
        return rows, mask, _quat_position(rows, self.angle_rows, self.quat_rows)

    def layout(self, n_nonlin):
        """(rows, angle_mask, quat_pos, n_res): quat_pos = -1 and n_res = len(rows) without a block, n_res = len(rows) - 1 with one."""
        r = self.resolve(n_nonlin)
        return (r[0], r[1], -1, len(r[0])) if len(r) == 2 else (r[0], r[1], r[2], len(r[0]) - 1)

    def covariance(self, dt, Q, n_res):
        """cov(dt, Q) as a Fortran-ordered [n_res x n_res] array, shape checked."""
        Q = np.asarray(Q, dtype=np.float64)
        if self.cov is None:
            if Q.shape != (n_res, n_res):
                raise RBPFError(_ffi.RBPF_ERR_INVALID_ARG, f"the default cov = dt * Q needs n_w == n_res: Q is {Q.shape[0]} x {Q.shape[1]} and "
                                                           f"{n_res} rows carry noise (give DeviceTransition a cov(dt, Q))")
            c = float(dt) * Q
        else:
            c = np.asarray(self.cov(float(dt), Q), dtype=np.float64)
            c = c.reshape(1, 1) if c.ndim == 0 else c
        if c.shape != (n_res, n_res):
            raise RBPFError(_ffi.RBPF_ERR_INVALID_ARG, f"cov(dt, Q) returned {c.shape}, expected {(n_res, n_res)}")
        return np.asfortranarray(c)


def _transition_rows(n_nonlin, rows, angle_rows):
    rows = tuple(range(int(n_nonlin))) if rows is None else tuple(int(r) for r in rows)
    if not 1 <= len(rows) <= 8:
        raise RBPFError(_ffi.RBPF_ERR_INVALID_ARG, "n_res (the rows that carry noise) must be in 1 .. 8")
    if len(set(rows)) != len(rows) or min(rows) < 0 or max(rows) >= int(n_nonlin):
        raise RBPFError(_ffi.RBPF_ERR_INVALID_ARG, f"rows {rows} must be distinct rows of the n_nonlin = {int(n_nonlin)} state")
    mask = 0
    for r in angle_rows:
        if int(r) not in rows:
            raise RBPFError(_ffi.RBPF_ERR_INVALID_ARG, f"angle row {int(r)} is not one of rows {rows}")
        mask |= 1 << rows.index(int(r))
    return rows, mask


def _quat_position(rows, angle_rows, quat_rows):
    """The position of q0 in rows; the block must lie in rows, adjacent and in order, and hold no angle row."""
    rows, quat_rows = tuple(int(r) for r in rows), tuple(int(r) for r in quat_rows)
    if len(quat_rows) != 4 or len(set(quat_rows)) != 4:
        raise RBPFError(_ffi.RBPF_ERR_INVALID_ARG, f"quat_rows {quat_rows} must name four distinct rows (q0, q1, q2, q3): one block")
    if any(q not in rows for q in quat_rows):
        raise RBPFError(_ffi.RBPF_ERR_INVALID_ARG, f"quat_rows {quat_rows} must all be among rows {rows}")
    pos = rows.index(quat_rows[0])
    if rows[pos:pos + 4] != quat_rows:
        raise RBPFError(_ffi.RBPF_ERR_INVALID_ARG, f"quat_rows {quat_rows} must be adjacent in rows {rows}, in the order q0, q1, q2, q3")
    if any(int(a) in quat_rows for a in angle_rows):
        raise RBPFError(_ffi.RBPF_ERR_INVALID_ARG, f"a row of the quaternion block {quat_rows} cannot be an angle row")
    return pos


def device_map_backward_workspace_bytes(n_nonlin, n_res, N_P, N_T, n_traj, quat_pos=-1):
    """rbpf_loc_generic_backward_workspace_bytes (no device access).  quat_pos >= 0: a transition with a quaternion block at that
    position of rows (rbpf_loc_generic_backward_pose_workspace_bytes); the second argument is then n_sel = len(rows) = n_res + 1."""
    lib = load_library()
    nbytes = C.c_size_t(0)
    if int(quat_pos) == -1:
        check(lib.rbpf_loc_generic_backward_workspace_bytes(int(n_nonlin), int(n_res), int(N_P), int(N_T), int(n_traj), C.byref(nbytes)))
    else:
        check(lib.rbpf_loc_generic_backward_pose_workspace_bytes(int(n_nonlin), int(n_res), int(quat_pos), int(N_P), int(N_T), int(n_traj),
                                                                 C.byref(nbytes)))
    return int(nbytes.value)


def _transition_probe_args(mu, xs_next, cov, rows, angle_rows, quat_rows):
    """The arrays and integers the one-step probes of a Gaussian transition share: (mu [n_sel x N] C-contiguous, xs_next
    [n_nonlin x M] Fortran-ordered, cov [n_res x n_res], rows (int32), angle_mask, quat_pos or -1)."""
    mu = np.asarray(mu, dtype=np.float64)
    mu = np.ascontiguousarray(mu.reshape(1, -1) if mu.ndim == 1 else mu)
    xs_next = np.asarray(xs_next, dtype=np.float64)
    xs_next = np.asfortranarray(xs_next.reshape(1, -1) if xs_next.ndim == 1 else xs_next)
    n_sel = mu.shape[0]
    n_res = n_sel if quat_rows is None else n_sel - 1
    nN = xs_next.shape[0]
    cov = np.asarray(cov, dtype=np.float64)
    cov = cov.reshape(1, 1) if cov.ndim == 0 else cov
    if cov.shape != (n_res, n_res):
        raise RBPFError(_ffi.RBPF_ERR_INVALID_ARG, f"cov is {cov.shape}, expected {(n_res, n_res)}")
    cov = np.asfortranarray(cov)
    if rows is None:
        rows_a, mask = np.arange(nN, dtype=np.int32), 0
        for r in angle_rows:
            if not 0 <= int(r) < nN:
                raise RBPFError(_ffi.RBPF_ERR_INVALID_ARG, f"angle row {int(r)} is not one of rows")
            mask |= 1 << int(r)
        if nN != n_sel:
            raise RBPFError(_ffi.RBPF_ERR_INVALID_ARG, f"mu has {n_sel} rows and xs_next {nN}: name the rows that carry noise")
    else:                                                         # (the library checks them: duplicates, range)
        rows_a = np.ascontiguousarray(np.asarray(rows, dtype=np.int32).ravel())
        if rows_a.size != n_sel:
            raise RBPFError(_ffi.RBPF_ERR_INVALID_ARG, f"mu has {n_sel} rows and rows names {rows_a.size}")
        mask = 0
        for r in angle_rows:
            pos = np.nonzero(rows_a == int(r))[0]
            if pos.size == 0:
                raise RBPFError(_ffi.RBPF_ERR_INVALID_ARG, f"angle row {int(r)} is not one of rows {tuple(rows_a.tolist())}")
            mask |= 1 << int(pos[0])
    qpos = -1 if quat_rows is None else _quat_position(rows_a.tolist(), angle_rows, quat_rows)
    return mu, xs_next, cov, rows_a, mask, qpos


def device_map_backward_step(mu, w, xs_next, cov, u, rows=None, angle_rows=(), want_logp=False, reps=1, quat_rows=None):
    """rbpf_loc_generic_backward_step, the kernel-level probe: one backward step with a Gaussian transition on the caller's arrays.
    mu [n_res x N] (the predicted rows of every particle), w [N], xs_next [n_nonlin x M], cov [n_res x n_res], u [M]; rows (default:
    all n_nonlin = n_res rows) and angle_rows as in DeviceTransition -> (index [M], logp [N x M] or None, median ms of one step).
    quat_rows as in DeviceTransition (rbpf_loc_generic_backward_pose_step): mu is then [n_sel x N], n_sel = len(rows) = n_res + 1, its
    block rows the predicted unit quaternion."""
    lib = load_library()
    mu, xs_next, cov, rows_a, mask, qpos = _transition_probe_args(mu, xs_next, cov, rows, angle_rows, quat_rows)
    (n_sel, N), (nN, M) = mu.shape, xs_next.shape
    w = np.ascontiguousarray(np.asarray(w, dtype=np.float64).ravel())
    u = np.ascontiguousarray(np.asarray(u, dtype=np.float64).ravel())
    if w.size != N or u.size != M:
        raise ValueError("w must be [N] and u [M]")
    index = np.zeros(M, dtype=np.int32)
    logp = np.empty((N, M), order="F") if want_logp else None
    ms = C.c_double(0.0)
    if quat_rows is None:
        check(lib.rbpf_loc_generic_backward_step(N, M, nN, n_sel, _ip(rows_a), mask, _dp(mu), _dp(w), _dp(xs_next), _dp(cov), _dp(u), _ip(index),
                                                 _dp(logp) if want_logp else None, int(reps), C.byref(ms)))
    else:
        check(lib.rbpf_loc_generic_backward_pose_step(N, M, nN, n_sel, _ip(rows_a), mask, qpos, _dp(mu), _dp(w), _dp(xs_next), _dp(cov), _dp(u),
                                                      _ip(index), _dp(logp) if want_logp else None, int(reps), C.byref(ms)))
    return index, logp, ms.value


def device_map_backward_reject_step(mu, w, xs_next, cov, u_try, u, rows=None, angle_rows=(), reps=1, quat_rows=None):
    """rbpf_loc_generic_backward_reject_step, the kernel-level probe: one step of backward simulation by rejection sampling with a
    Gaussian transition on the caller's arrays.  mu, w, xs_next, cov, rows, angle_rows and quat_rows as device_map_backward_step;
    u_try [R x M x 2]: the uniforms (u0, u1) of try r of trajectory j, R = max_tries (R = 0: an empty array); u [M]: the fallback's
    uniforms -> (index [M], accepted_at [M]: the try that was accepted or -1 for a trajectory the all-pairs pass drew, median ms)."""
    lib = load_library()
    mu, xs_next, cov, rows_a, mask, qpos = _transition_probe_args(mu, xs_next, cov, rows, angle_rows, quat_rows)
    (n_sel, N), (nN, M) = mu.shape, xs_next.shape
    w = np.ascontiguousarray(np.asarray(w, dtype=np.float64).ravel())
    u = np.ascontiguousarray(np.asarray(u, dtype=np.float64).ravel())
    if w.size != N or u.size != M:
        raise ValueError("w must be [N] and u [M]")
    u_try, R = _reject_uniforms(u_try, M)
    index, acc = np.zeros(M, dtype=np.int32), np.zeros(M, dtype=np.int32)
    ms = C.c_double(0.0)
    check(lib.rbpf_loc_generic_backward_reject_step(N, M, nN, n_sel, _ip(rows_a), mask, -1 if quat_rows is None else qpos, _dp(mu), _dp(w),
                                                    _dp(xs_next), _dp(cov), _dp(u_try) if u_try is not None else None, _dp(u), R, _ip(index), _ip(acc), int(reps),
                                                    C.byref(ms)))
    return index, acc, ms.value


def device_map_map_step(mu, delta, xs_next, cov, rows=None, angle_rows=(), reps=1, quat_rows=None):
    """rbpf_loc_generic_map_step, the kernel-level probe: one step of the MAP recursion with a Gaussian transition on the caller's
    arrays.  mu [n_sel x N], delta [N] (-inf allowed), xs_next [n_nonlin x M] (the successors), cov [n_res x n_res]; rows, angle_rows
    and quat_rows as in device_map_backward_step -> (best [M] = max_i [delta_i + logp(xs_next[:, j] | i)], arg [M] the lowest arg max,
    0 where best is -inf, median ms of one step)."""
    lib = load_library()
    mu, xs_next, cov, rows_a, mask, qpos = _transition_probe_args(mu, xs_next, cov, rows, angle_rows, quat_rows)
    (n_sel, N), (nN, M) = mu.shape, xs_next.shape
    delta = np.ascontiguousarray(np.asarray(delta, dtype=np.float64).ravel())
    if delta.size != N:
        raise ValueError("delta must be [N]")
    best, arg = np.empty(M), np.zeros(M, dtype=np.int32)
    ms = C.c_double(0.0)
    check(lib.rbpf_loc_generic_map_step(N, M, nN, n_sel, _ip(rows_a), mask, qpos, _dp(mu), _dp(delta), _dp(xs_next), _dp(cov), _dp(best),
                                        _ip(arg), int(reps), C.byref(ms)))
    return best, arg, ms.value


def device_map_map_workspace_bytes(n_nonlin, n_sel, N_P, N_T, quat_pos=-1):
    """rbpf_loc_generic_map_workspace_bytes (no device access): n_sel = len(rows), quat_pos the position of a quaternion block in
    rows or -1."""
    lib = load_library()
    nbytes = C.c_size_t(0)
    check(lib.rbpf_loc_generic_map_workspace_bytes(int(n_nonlin), int(n_sel), int(quat_pos), int(N_P), int(N_T), C.byref(nbytes)))
    return int(nbytes.value)


def device_map_marginal_step(mu, logw, xs_next, logws_next, cov, rows=None, angle_rows=(), quat_rows=None, reps=1):
    """rbpf_loc_generic_marginal_step, the kernel-level probe: one step of the marginal-smoothing recursion with a Gaussian transition
    on the caller's arrays.  mu [n_sel x N], logw [N] = log w_t, xs_next [n_nonlin x M] (the successors), logws_next [M] =
    log w_{t+1|T} (-inf allowed in both), cov [n_res x n_res]; rows, angle_rows and quat_rows as in device_map_backward_step ->
    (D [M], lws [N] un-normalised, median ms of one step)."""
    lib = load_library()
    mu, xs_next, cov, rows_a, mask, qpos = _transition_probe_args(mu, xs_next, cov, rows, angle_rows, quat_rows)
    (n_sel, N), (nN, M) = mu.shape, xs_next.shape
    logw = np.ascontiguousarray(np.asarray(logw, dtype=np.float64).ravel())
    logws_next = np.ascontiguousarray(np.asarray(logws_next, dtype=np.float64).ravel())
    if logw.size != N or logws_next.size != M:
        raise ValueError("logw must be [N] and logws_next [M]")
    D, lws = np.empty(M), np.empty(N)
    ms = C.c_double(0.0)
    check(lib.rbpf_loc_generic_marginal_step(N, M, nN, n_sel, _ip(rows_a), mask, qpos, _dp(mu), _dp(logw), _dp(xs_next), _dp(logws_next),
                                             _dp(cov), _dp(D), _dp(lws), int(reps), C.byref(ms)))
    return D, lws, ms.value


def device_map_marginal_workspace_bytes(n_nonlin, n_sel, N_P, N_T, quat_pos=-1):
    """rbpf_loc_generic_marginal_workspace_bytes (no device access): n_sel = len(rows), quat_pos the position of a quaternion block
    in rows or -1."""
    lib = load_library()
    nbytes = C.c_size_t(0)
    check(lib.rbpf_loc_generic_marginal_workspace_bytes(int(n_nonlin), int(n_sel), int(quat_pos), int(N_P), int(N_T), C.byref(nbytes)))
    return int(nbytes.value)


def device_map_pair_stats_step(mu, logw, xs_next, logws_next, cov, rows=None, angle_rows=(), quat_rows=None, reps=1):
    """rbpf_loc_generic_pair_stats_step, the kernel-level probe: device_map_marginal_step, and behind it the two-slice statistics of
    that step with its own mass -> (D [M], lws [N] un-normalised, S [n_res x n_res], m [n_res], pair_mass, median ms of the marginal
    step, the normalisation and the statistics pass together).  S and m are in the order of cov."""
    lib = load_library()
    mu, xs_next, cov, rows_a, mask, qpos = _transition_probe_args(mu, xs_next, cov, rows, angle_rows, quat_rows)
    (n_sel, N), (nN, M) = mu.shape, xs_next.shape
    n = cov.shape[0]
    logw = np.ascontiguousarray(np.asarray(logw, dtype=np.float64).ravel())
    logws_next = np.ascontiguousarray(np.asarray(logws_next, dtype=np.float64).ravel())
    if logw.size != N or logws_next.size != M:
        raise ValueError("logw must be [N] and logws_next [M]")
    D, lws, S, m, pm = np.empty(M), np.empty(N), np.empty((n, n), order="F"), np.empty(n), np.empty(1)
    ms = C.c_double(0.0)
    check(lib.rbpf_loc_generic_pair_stats_step(N, M, nN, n_sel, _ip(rows_a), mask, qpos, _dp(mu), _dp(logw), _dp(xs_next), _dp(logws_next),
                                               _dp(cov), _dp(D), _dp(lws), _dp(S), _dp(m), _dp(pm), int(reps), C.byref(ms)))
    return D, lws, S, m, float(pm[0]), ms.value


def device_map_pair_stats_workspace_bytes(n_nonlin, n_sel, N_P, N_T, quat_pos=-1):
    """rbpf_loc_generic_pair_stats_workspace_bytes (no device access): n_sel = len(rows), quat_pos the position of a quaternion block
    in rows or -1."""
    lib = load_library()
    nbytes = C.c_size_t(0)
    check(lib.rbpf_loc_generic_pair_stats_workspace_bytes(int(n_nonlin), int(n_sel), int(quat_pos), int(N_P), int(N_T), C.byref(nbytes)))
    return int(nbytes.value)


def device_map_forward_stats_step(mu, logw, xs_next, tau_S, tau_m, cov, rows=None, angle_rows=(), quat_rows=None, s_scale=1.0, reps=1):
    """rbpf_loc_generic_forward_stats_step, the kernel-level probe: one step of the running two-slice statistics with a Gaussian
    transition on the caller's arrays.  mu, logw, xs_next, cov, rows, angle_rows and quat_rows as in device_map_marginal_step;
    tau_S [n_res x n_res x N] (the lower triangle is read) and tau_m [n_res x N] the incoming carry in the order of cov; s_scale =
    1 / dt of the step -> (D [M], tau_S_next [n_res x n_res x M], tau_m_next [n_res x M], reach [M] = sum_i omega(i, j), median ms
    of the normaliser pass, the carry pass, its merge and the reducer together)."""
    lib = load_library()
    mu, xs_next, cov, rows_a, mask, qpos = _transition_probe_args(mu, xs_next, cov, rows, angle_rows, quat_rows)
    (n_sel, N), (nN, M) = mu.shape, xs_next.shape
    n = cov.shape[0]
    logw = np.ascontiguousarray(np.asarray(logw, dtype=np.float64).ravel())
    tau_S = np.asfortranarray(np.asarray(tau_S, dtype=np.float64).reshape(n, n, -1))
    tau_m = np.asfortranarray(np.asarray(tau_m, dtype=np.float64).reshape(n, -1))
    if logw.size != N or tau_S.shape[2] != N or tau_m.shape[1] != N:
        raise ValueError("logw must be [N], tau_S [n_res x n_res x N] and tau_m [n_res x N]")
    D, tS, tm, reach = np.empty(M), np.empty((n, n, M), order="F"), np.empty((n, M), order="F"), np.empty(M)
    ms = C.c_double(0.0)
    check(lib.rbpf_loc_generic_forward_stats_step(N, M, nN, n_sel, _ip(rows_a), mask, qpos, _dp(mu), _dp(logw), _dp(xs_next), _dp(tau_S),
                                                  _dp(tau_m), _dp(cov), float(s_scale), _dp(D), _dp(tS), _dp(tm), _dp(reach), int(reps),
                                                  C.byref(ms)))
    return D, tS, tm, reach, ms.value


def device_map_forward_stats_workspace_bytes(n_nonlin, n_sel, N_P, N_T, quat_pos=-1):
    """rbpf_loc_generic_forward_stats_workspace_bytes (no device access): what the carry of the running statistics holds while it
    lives; n_sel = len(rows), quat_pos the position of a quaternion block in rows or -1."""
    lib = load_library()
    nbytes = C.c_size_t(0)
    check(lib.rbpf_loc_generic_forward_stats_workspace_bytes(int(n_nonlin), int(n_sel), int(quat_pos), int(N_P), int(N_T), C.byref(nbytes)))
    return int(nbytes.value)


def device_map_fixed_lag_step(mu, logw, xs_next, tau, cov, rows=None, angle_rows=(), quat_rows=None, moments=1, reps=1):
    """rbpf_loc_generic_fixed_lag_step, the kernel-level probe: one pass of the fixed-lag smoother with a Gaussian transition on the
    caller's arrays.  mu, logw, xs_next, cov, rows, angle_rows and quat_rows as in device_map_marginal_step; tau [K x N], any
    K >= 1, the incoming columns of the carry -> (D [M], tau_next [K x M], reach [M] = sum_i omega(i, j), median ms of the
    normaliser pass, the carry pass, its merge, the enter kernel (with `moments`) and the reducers together)."""
    lib = load_library()
    mu, xs_next, cov, rows_a, mask, qpos = _transition_probe_args(mu, xs_next, cov, rows, angle_rows, quat_rows)
    (n_sel, N), (nN, M) = mu.shape, xs_next.shape
    logw = np.ascontiguousarray(np.asarray(logw, dtype=np.float64).ravel())
    tau = np.asarray(tau, dtype=np.float64)
    tau = np.ascontiguousarray(tau.reshape(1, -1) if tau.ndim == 1 else tau)
    K = tau.shape[0]
    if logw.size != N or tau.shape != (K, N):
        raise ValueError("logw must be [N] and tau [K x N]")
    D, tn, reach = np.empty(M), np.empty((K, M)), np.empty(M)
    ms = C.c_double(0.0)
    check(lib.rbpf_loc_generic_fixed_lag_step(N, M, K, int(moments), nN, n_sel, _ip(rows_a), mask, qpos, _dp(mu), _dp(logw), _dp(xs_next),
                                              _dp(tau), _dp(cov), _dp(D), _dp(tn), _dp(reach), int(reps), C.byref(ms)))
    return D, tn, reach, ms.value


def device_map_fixed_lag_workspace_bytes(n_nonlin, n_sel, N_P, N_T, lag, moments=1, quat_pos=-1):
    """rbpf_loc_generic_fixed_lag_workspace_bytes (no device access): what the carry of the fixed-lag smoother holds while it lives;
    n_sel = len(rows), quat_pos the position of a quaternion block in rows or -1."""
    lib = load_library()
    nbytes = C.c_size_t(0)
    check(lib.rbpf_loc_generic_fixed_lag_workspace_bytes(int(n_nonlin), int(n_sel), int(quat_pos), int(N_P), int(N_T), int(lag), int(moments),
                                                         C.byref(nbytes)))
    return int(nbytes.value)


def fixed_lag_assemble(pages, means, lag, moments):
    """The estimates of LocalizationSession.fixed_lag_estimates from what the library keeps, in plain numpy: pages
    [((lag + 1) H + 1) x Td] (column t: est(l, t) for l = 0 .. lag, H values each, then mass(t)) and means [n x Td] (c_s, the filter
    mean of step s), H = n (moments = 1) or n (n + 3) / 2 (moments = 2: d, then the lower triangle by rows of d d') ->
    dict(mean [n x Td], lag_of [Td], by_lag [n x (lag + 1) x Td], mass [Td][, cov [n x n x Td]]).  mean = c + E[d],
    cov = E[d d'] - E[d] E[d]'; column s takes lag_of[s] = min(lag, Td - 1 - s) from page s + lag_of[s]; NaN where t - l < 0."""
    means = np.asarray(means, dtype=np.float64)
    pages = np.asarray(pages, dtype=np.float64)
    n, Td = means.shape
    lag, moments = int(lag), int(moments)
    H = n if moments == 1 else n * (n + 3) // 2
    if moments not in (1, 2) or lag < 1 or pages.shape != ((lag + 1) * H + 1, Td):
        raise ValueError(f"pages must be [((lag + 1) H + 1) x Td] = {((lag + 1) * H + 1, Td)} with lag >= 1 and moments 1 or 2")
    est = pages[:-1].reshape(lag + 1, H, Td)
    by_lag = np.full((n, lag + 1, Td), np.nan)
    for l in range(min(lag, Td - 1) + 1):
        by_lag[:, l, l:] = means[:, :Td - l] + est[l, :n, l:]
    s = np.arange(Td)
    lag_of = np.minimum(lag, Td - 1 - s).astype(np.int64)
    out = dict(mean=np.asfortranarray(by_lag[:, lag_of, s + lag_of]), lag_of=lag_of, by_lag=np.asfortranarray(by_lag), mass=pages[-1].copy())
    if moments == 2:
        e = est[lag_of, :, s + lag_of].T                                  # [H x Td]: the page column s takes
        cov = np.empty((n, n, Td), order="F")
        k = n
        for p_ in range(n):
            for q in range(p_ + 1):
                cov[p_, q] = cov[q, p_] = e[k] - e[p_] * e[q]
                k += 1
        out["cov"] = cov
    return out


class DeviceMap:
    """A fixed map of an arbitrary model whose handles are device code: the posterior N(mean, V'V) over the nLin linear states, V
    lower (the DenseMagMap convention), as a SLAM filter or smoother run with the same DeviceHandles returns it (xl_max, P_max /
    XLK, PK: from_posterior), and the measurement noise R [n_y x n_y], symmetric positive definite.  Handed to
    particleFilterLocalization(device_map, None, ...) or LocalizationSession, it localises a run in that map: the RBPF with the map
    frozen (particleFilter.m:100-161 with xl, P shared by all particles and never updated),

        e_i = y_t' - H_i mean,   S_i = H_i P H_i' + R,   logw_i = -sum log diag chol S_i - |chol(S_i) \\ e_i|^2 / 2 - n_y log(2 pi) / 2

    with H_i = dy(i,:,:) of handles.measModel(xn), called once per step with N_P columns; handles.dynModel draws its own random
    numbers, as for DeviceHandles.  The layout of every dy is read off its strides (MATLAB-order strides, C-contiguous, or the native
    view of a native_out handle, consumed in place); handles.dy_layout is not used.  n_y 1 .. 8, nLin 1 .. 1151, n_nonlin 1 .. 8; one
    GPU.  transition: a DeviceTransition, the density of handles.dynModel as it draws (a drift plus Gaussian noise on some rows of
    the state); with one, LocalizationSession.backward_simulate and particleSmootherLocalization draw smoothed trajectories in this
    map; a 3-D pose state (position + unit quaternion) states its rotation rows as the transition's quat_rows.  Without a transition
    they refuse (they need dynModel's transition density; a generic dynModel is a sampler).  Not built: densities outside that family
    (rotation noise multiplied on the left, two quaternion blocks, noise through a non-square G), host closures, sharding.  The map
    of a sparseFeatures model: DeviceLandmarkMap."""

    _create = "rbpf_loc_generic_create"

    def __init__(self, handles, mean, V, R, transition=None):
        if transition is not None and not isinstance(transition, DeviceTransition):
            raise TypeError("transition must be a DeviceTransition")
        self.transition = transition
        self._check_handles(handles)
        self.handles = handles
        self.mean = np.ascontiguousarray(np.asarray(mean, dtype=np.float64).ravel())
        n = self.mean.size
        self.V = np.asfortranarray(np.tril(np.asarray(V, dtype=np.float64)))
        R = np.asarray(R, dtype=np.float64)
        self.R = np.asfortranarray(R.reshape(1, 1) if R.ndim == 0 else R)
        if self.V.shape != (n, n):
            raise ValueError("mean must be [nLin] and V [nLin x nLin]")
        if self.R.ndim != 2 or self.R.shape[0] != self.R.shape[1]:
            raise ValueError("R must be [n_y x n_y]")

    @staticmethod
    def _check_handles(handles):
        if not isinstance(handles, DeviceHandles):
            raise TypeError("DeviceMap needs a DeviceHandles object")
        if isinstance(handles, DeviceSparseHandles):
            raise RBPFError(_ffi.RBPF_ERR_UNSUPPORTED, "DeviceMap is built for dense models: a DeviceSparseHandles measModel predicts "
                                                       "from the map it is handed; DeviceLandmarkMap localises in a landmark map")

    def _driver(self, lib, ctx, prob):
        return _DeviceMapDriver(lib, ctx, self, prob)

    @property
    def nLin(self):
        return self.mean.size

    @property
    def ny(self):
        return self.R.shape[0]

    @classmethod
    def from_posterior(cls, handles, xl, P, R, transition=None):
        """From a map posterior (mean xl, covariance P), factored as DenseMagMap.from_posterior factors it."""
        return cls(handles, xl, _lower_factor(P), R, transition=transition)

    def predict(self, xn, reps=1):
        """The map's prediction at the states xn [n_nonlin x n_pred] (numpy or a device tensor), through the weight kernel on its
        own: (yhat [n_pred x n_y] = H mean, cov [n_pred x n_y x n_y] = H P H', without R).  measModel is called once, with n_pred
        columns."""
        import torch
        lib = load_library()
        if lib.rbpf_device_count() < 1:
            raise RBPFError(_ffi.RBPF_ERR_NO_DEVICE, "no HIP device: the localisation filter has no CPU fallback")
        device = torch.device("cuda", torch.cuda.current_device())
        xn = torch.as_tensor(xn, dtype=torch.float64, device=device)
        xn = xn.reshape(-1, 1) if xn.dim() == 1 else xn
        npred, d, n = xn.shape[1], self.ny, self.nLin
        if self.handles.native_out:
            dy = self.handles.measModel(xn, torch.zeros((npred, d, (n + 15) // 16 * 16), dtype=torch.float64, device=device)[:, :, :n])
        else:
            dy = self.handles.measModel(xn)
        if dy.dim() == 2 and d == 1:
            dy = dy.unsqueeze(1)
        if tuple(dy.shape) != (npred, d, n) or dy.dtype != torch.float64 or not dy.is_cuda:
            raise ValueError(f"measModel returned {tuple(dy.shape)} {dy.dtype} on {dy.device}, expected a float64 device tensor of "
                             f"shape {(npred, d, n)}")
        yhat, S, _, _ = device_map_weights(dy.cpu().numpy(), self.mean, self.V, self.R, np.zeros(d), reps=reps)
        return yhat, S


class _DeviceMapProblem:
    """The problem arrays of a localisation run in a DeviceMap, sized from the map and the arrays themselves."""

    def __init__(self, mp, odometry, y, x0_nonLin, Q, N_P, dt):
        y = np.asarray(y, dtype=np.float64)
        y = y.reshape(-1, 1) if y.ndim == 1 else y
        self.N_T, self.N_P, self.ny = y.shape[0], int(N_P), mp.ny
        if y.ndim != 2 or y.shape[1] != mp.ny:
            raise ValueError(f"y must be [N_T x {mp.ny}]")
        self.y = np.asfortranarray(y)
        x0 = np.asarray(x0_nonLin, dtype=np.float64)
        self.x0 = np.asfortranarray(x0.reshape(-1, 1) if x0.ndim == 1 else x0)
        self.nNonLin = self.x0.shape[0]
        if self.x0.shape[1] not in (1, self.N_P):
            raise ValueError("x0_nonLin must be [n_nonlin] or [n_nonlin x N_P]")
        odo = np.asarray(odometry, dtype=np.float64)
        self._odo = odo.reshape(1, -1) if odo.ndim == 1 else odo
        Qa = np.asarray(Q, dtype=np.float64)
        Qa = Qa.reshape(1, 1) if Qa.ndim == 0 else Qa
        self._Q = Qa[:, :, None] if Qa.ndim == 2 else Qa
        self._dt = np.atleast_1d(np.asarray(dt, dtype=np.float64)).ravel()
        if self.N_T > 1 and (self._odo.shape[0] < self.N_T - 1 or (self._Q.shape[2] > 1 and self._Q.shape[2] < self.N_T - 1)
                             or (self._dt.size > 1 and self._dt.size < self.N_T - 1)):
            raise ValueError("odometry must have >= N_T-1 rows, Q and dt one or >= N_T-1 pages / entries")


def _loc_generic_states(driver, t):
    """The states of step t of a generic localisation context, [n_nonlin x N_P] column-major, on the driver's stream: the resampled
    ancestors through dynModel (t = 0: the initial states)."""
    ai, anc = C.c_void_p(), C.c_void_p()
    check(driver.lib.rbpf_loc_generic_ancestors_device(driver.ctx, C.byref(ai), C.byref(anc)))
    xn_cm = driver._view(driver.torch, anc, (driver.N, driver.nN), driver.device)
    if t > 0:
        xn_cm = driver._dyn(t - 1, xn_cm.t()).t().contiguous()
    return xn_cm


class _DeviceMapDriver(_DeviceDriver):
    """Runs the steps of a generic localisation context (rbpf_loc_generic_create) with the handles of a DeviceMap: the pair
    rbpf_loc_generic_ancestors_device / rbpf_loc_generic_step_device, the layout of every dy read off its strides."""

    def __init__(self, lib, ctx, mp, prob):                       # (the initial states are the context's; handles.dy_layout is not used)
        self._setup(lib, ctx, mp.handles, (prob.nNonLin, mp.nLin, mp.ny, prob.N_P, prob.N_T), lib.rbpf_loc_generic_layout, prob)
        self.torch.cuda.current_stream(self.device).synchronize()      # the constants, before the library's stream reads them

    def _step(self, t):
        torch, lib = self.torch, self.lib
        with torch.cuda.stream(self.stream):
            xn_cm = _loc_generic_states(self, t)
            out = self._native_out()
            dy, layout = self._layout_of(self._meas(xn_cm.t(), out), out)
            self._keep = (xn_cm, dy)                                      # read in stream order by the step just enqueued
            check(lib.rbpf_loc_generic_step_device(self.ctx, C.c_void_p(xn_cm.data_ptr()), C.c_void_p(dy.data_ptr()), layout))


class _LandmarkMapDriver(_SparseDeviceDriver):
    """Runs the steps of a landmark-map localisation context (rbpf_loc_landmark_create) with the DeviceSparseHandles of a
    DeviceLandmarkMap: measModel(xn, xl) with xl the context's rows of the map's mean."""

    def __init__(self, lib, ctx, mp, prob):
        self._setup(lib, ctx, mp.handles, (prob.nNonLin, mp.nLin, mp.ny, prob.N_P, prob.N_T), lib.rbpf_loc_generic_layout, prob)
        xlp, ldx = C.c_void_p(), C.c_int32(0)
        check(lib.rbpf_loc_landmark_map_device(ctx, C.byref(xlp), C.byref(ldx)))
        self.xl = self._view(self.torch, xlp, (self.N, ldx.value), self.device)[:, :self.n]
        self.torch.cuda.current_stream(self.device).synchronize()      # the constants, before the library's stream reads them

    def _step(self, t):
        torch, lib = self.torch, self.lib
        with torch.cuda.stream(self.stream):
            xn_cm = _loc_generic_states(self, t)
            yhat, yl, dy, dl = self._layouts(*self._meas_sparse(xn_cm.t(), self.xl))
            self._keep = (xn_cm, yhat, dy)                                # read in stream order by the step just enqueued
            check(lib.rbpf_loc_landmark_step_device(self.ctx, C.c_void_p(xn_cm.data_ptr()), C.c_void_p(yhat.data_ptr()), yl,
                                                    C.c_void_p(dy.data_ptr()), dl))

    def yhattraj(self):
        out = np.empty((self.d, self.T), order="F")
        check(self.lib.rbpf_loc_landmark_yhattraj(self.ctx, _dp(out)))
        return out


def landmark_map_weights(yhat, dy, V, R, y, yhat_layout=2, dy_layout=2, ldx=None, pad=0.0, reps=1):
    """rbpf_loc_landmark_weights, the kernel-level probe of localisation in a landmark map: yhat [N x n_y], dy [N x n_y x nLin] (the
    handle's outputs for N particles), V [nLin x nLin] lower with V'V = P, R [n_y x n_y], y [n_y] with NaN = not observed ->
    (S [N x M x M] = H_i(ind,:) P H_i(ind,:)' before R is added, logw [N], median kernel ms over `reps` launches), M the number of
    observed outputs.  yhat_layout 0 / 2 and dy_layout 0 / 1 / 2: the memory layouts the arrays are handed over in; in dy layout 1
    the columns behind nLin (row stride ldx, default the next multiple of 16) are filled with `pad`."""
    lib = load_library()
    dy = np.asarray(dy, dtype=np.float64)
    if dy.ndim != 3:
        raise ValueError("dy must be [N x n_y x nLin]")
    N, d, n = dy.shape
    yhat = np.asarray(yhat, dtype=np.float64)
    if yhat.shape != (N, d):
        raise ValueError("yhat must be [N x n_y]")
    ybuf = np.asfortranarray(yhat) if yhat_layout == 0 else np.ascontiguousarray(yhat)
    if dy_layout == 0:
        buf = np.asfortranarray(dy)
    elif dy_layout == 1:
        ldx = (n + 15) // 16 * 16 if ldx is None else int(ldx)
        buf = np.full((N, d, max(ldx, n)), float(pad))
        buf[:, :, :n] = dy
    else:
        buf = np.ascontiguousarray(dy)
    V = np.asfortranarray(np.asarray(V, dtype=np.float64))
    R = np.asfortranarray(np.asarray(R, dtype=np.float64).reshape(d, d))
    y = np.ascontiguousarray(np.asarray(y, dtype=np.float64).ravel())
    if V.shape != (n, n) or y.size != d:
        raise ValueError("V must be [nLin x nLin] and y [n_y]")
    M = int(np.count_nonzero(~np.isnan(y)))
    S, logw = np.empty((N, M, M)), np.empty(N)
    ms = C.c_double(0.0)
    check(lib.rbpf_loc_landmark_weights(d, n, N, _dp(ybuf), int(yhat_layout), _dp(buf), int(dy_layout), int(ldx or 0), _dp(V), _dp(R),
                                        _dp(y), _dp(S), _dp(logw), int(reps), C.byref(ms)))
    return S, logw, ms.value


class DeviceLandmarkMap(DeviceMap):
    """A fixed landmark map of a sparseFeatures model whose handles are device code: the posterior N(mean, V'V) over the nLin
    linear states, V lower, as the SLAM filter or smoother run with the same DeviceSparseHandles returns it (xl_max, P_max / XLK,
    PK: from_posterior), and R [n_y x n_y], symmetric positive definite.  Accepted wherever a DeviceMap is
    (particleFilterLocalization(landmark_map, None, ...), LocalizationSession, and with a DeviceTransition backward_simulate and
    particleSmootherLocalization); the recursion is particleFilter.m:100-161 with the sparseFeatures branch of :127-137 and the map
    frozen: per step, with ind the outputs whose y is not NaN and M their number,

        e_i = y_t(ind)' - yhat_i(ind),   S_i = H_i(ind,:) P H_i(ind,:)' + R(ind,ind),
        logw_i = -sum log diag chol S_i - |chol(S_i) \\ e_i|^2 / 2 - M log(2 pi) / 2

    with (yhat, dy) = handles.measModel(xn, xl), called once per step with N_P columns and xl [N_P x nLin] the map's mean in every
    row (the view the SLAM filter hands its handle, so the handle runs unchanged); rows of yhat / dy of outputs not observed may
    hold anything.  Nothing observed: equal weights.  extras gains yhattraj [n_y x N_T], the handle's yhat of every step's
    maximum-weight particle.  n_y 1 .. 32, nLin 1 .. 96, n_nonlin 1 .. 8; one GPU.  Not built: host closures, the MEX gateway,
    sharding (n_devices is refused), nLin > 96, n_y > 32."""

    _create = "rbpf_loc_landmark_create"

    @staticmethod
    def _check_handles(handles):
        if not isinstance(handles, DeviceHandles):
            raise TypeError("DeviceLandmarkMap needs a DeviceSparseHandles object")
        if not isinstance(handles, DeviceSparseHandles):
            raise RBPFError(_ffi.RBPF_ERR_UNSUPPORTED, "DeviceLandmarkMap is built for sparseFeatures models (DeviceSparseHandles: "
                                                       "measModel(xn, xl) -> (yhat, dy)); DeviceMap localises in the map of a dense model")

    def _driver(self, lib, ctx, prob):
        return _LandmarkMapDriver(lib, ctx, self, prob)

    def predict(self, xn, reps=1):
        """The map's prediction at the states xn [n_nonlin x n_pred] (numpy or a device tensor) with every output treated as
        observed: (yhat [n_pred x n_y], the handle's, cov [n_pred x n_y x n_y] = H P H' without R, through the weight kernel on
        its own).  measModel is called once, with n_pred columns."""
        import torch
        lib = load_library()
        if lib.rbpf_device_count() < 1:
            raise RBPFError(_ffi.RBPF_ERR_NO_DEVICE, "no HIP device: the localisation filter has no CPU fallback")
        device = torch.device("cuda", torch.cuda.current_device())
        xn = torch.as_tensor(xn, dtype=torch.float64, device=device)
        xn = xn.reshape(-1, 1) if xn.dim() == 1 else xn
        npred, d, n = xn.shape[1], self.ny, self.nLin
        xl = torch.as_tensor(self.mean, device=device).repeat(npred, 1)
        out = self.handles.measModel(xn, xl)
        if not (isinstance(out, (tuple, list)) and len(out) == 2 and all(torch.is_tensor(v) for v in out)):
            raise ValueError("measModel must return (yhat, dy), two device tensors")
        yhat, dy = out
        if tuple(yhat.shape) != (npred, d) or tuple(dy.shape) != (npred, d, n) or yhat.dtype != torch.float64 or dy.dtype != torch.float64:
            raise ValueError(f"measModel returned yhat {tuple(yhat.shape)} {yhat.dtype} and dy {tuple(dy.shape)} {dy.dtype}, expected "
                             f"float64 tensors of shape {(npred, d)} and {(npred, d, n)}")
        yhat = yhat.cpu().numpy()
        S, _, _ = landmark_map_weights(yhat, dy.cpu().numpy(), self.V, self.R, np.zeros(d), reps=reps)
        return yhat, S


def _device_map(dynModel, measModel):
    """The DeviceMap given in place of the handle pair (as dynModel, measModel None or the same object), or None."""
    if not isinstance(dynModel, DeviceMap) and not isinstance(measModel, DeviceMap):
        return None
    if not isinstance(dynModel, DeviceMap) or (measModel is not None and measModel is not dynModel):
        raise RBPFError(_ffi.RBPF_ERR_INVALID_ARG, "a DeviceMap replaces the handle pair: pass the object as dynModel and None "
                                                   "(or the same object) as measModel")
    return dynModel


_NO_BACKWARD_IN_DEVICE_MAP = ("backward simulation needs the transition density of dynModel: the dynModel of a DeviceMap is a "
                              "sampler that draws its own random numbers (its handles carry no density)")


def _device_map_create(lib, mp, prob, rng, opt):
    """rbpf_loc_generic_create (rbpf_loc_landmark_create for a landmark map) -> (ctx, what must stay alive with it)."""
    if isinstance(rng, ReplayRNG):                                # the handles draw their own normals: Z is not read
        rng = ReplayRNG(rng.U, np.zeros(rng.U.shape + (1,)))
    blk, keep = _rng_block(rng, prob.N_P, prob.N_T, 1, 1)
    ctx = C.c_void_p()
    check(getattr(lib, mp._create)(prob.nNonLin, mp.ny, mp.nLin, _dp(mp.mean), _dp(mp.V), _dp(mp.R), prob.N_P, prob.N_T, _dp(prob.y),
                                      _dp(prob.x0), prob.x0.shape[1], C.byref(blk), C.byref(opt), C.byref(ctx)))
    return ctx, (blk, keep)


def _loc_out(N, T, Td, extras, hist=True, trace=True, nN=7):
    o = _ffi.rbpf_loc_out()
    b = dict(traj_max=np.full((nN, T), np.nan, order="F"), traj_mean=np.full((nN, T), np.nan, order="F"))
    if extras:
        b.update(final_xn=np.empty((nN, N), order="F"), log_sum_w=np.empty(Td))
        if trace:
            b.update(trace_logw=np.empty((N, Td), order="F"), trace_w=np.empty((N, Td), order="F"))
        if hist:
            b.update(trace_ai=np.zeros((N, Td), dtype=np.int32, order="F"), xn_traj=np.empty((nN, N, Td), order="F"))
    for k, v in b.items():
        setattr(o, k, _ip(v) if v.dtype == np.int32 else _dp(v))
    return o, b


def particleFilterLocalization(dynModel, measModel, odometry, y, x0_nonLin, Q, R, N_P, dt, makePlots=None, *, rng=None,
                               extras=False, n_devices=0, lazy_depth=0):
    """Mirror of examples/mag-localization-mapping/particleFilterLocalization.m:1-2 -> (traj_max, traj_mean[, extras]).
    dynModel / measModel are the handles of a DenseMagMap; R is accepted and not used (:19).  makePlots(xn, traj_max, yhattraj,
    xn_traj, traj_mean) is called after every step (:129-131).  A step whose weights sum to <= 1e-12 raises a RuntimeWarning
    with the reference's text (:113-115) and the run carries on.
    A DeviceMap as dynModel (measModel None) localises in the fixed map of an arbitrary device-code model (see DeviceMap): the same
    outputs with n_nonlin rows in place of 7, yhattraj [n_y x N_T]; R is accepted and not used there either (the map's R counts).
    A DeviceLandmarkMap likewise, for a sparseFeatures model (see there): makePlots gets the handle's yhattraj, extras gains it."""
    import warnings
    dmap = _device_map(dynModel, measModel)
    if dmap is not None:
        return _device_map_localization(dmap, odometry, y, x0_nonLin, Q, N_P, dt, makePlots, rng, extras, n_devices, lazy_depth)
    mp = _recognise_map(dynModel, measModel)
    lib = load_library()
    prob = _LocProblem(odometry, y, x0_nonLin, Q, N_P, dt)
    N, T = prob.N_P, prob.N_T
    if lib.rbpf_device_count() < 1:
        raise RBPFError(_ffi.RBPF_ERR_NO_DEVICE, "no HIP device: the localisation filter has no CPU fallback")
    opt = _ffi.rbpf_options(keep_history=1, trace=1 if extras else 0, n_devices=int(n_devices), lazy_depth=int(lazy_depth))
    if opt.n_devices or opt.lazy_depth:
        mstruct = mp._map_struct()                                   # refused by the library before anything is computed
    else:
        mstruct = mp._loc_map(N)
    blk, _keep = _rng_block(rng, N, T, 6, 1)
    hook_error = []
    if makePlots is not None:
        def on_step(view_p, _user):
            try:
                v = view_p.contents
                t = int(v.t)
                o, b = _loc_out(N, T, t + 1, True, trace=False)
                check(lib.rbpf_loc_finish(C.c_void_p(v.ctx), C.byref(o)))
                xn_traj = np.zeros((7, N, T))
                xn_traj[:, :, :t + 1] = b["xn_traj"]
                makePlots(b["final_xn"], b["traj_max"], np.full((3, T), np.nan), xn_traj, b["traj_mean"])
                return 0
            except Exception as exc:                                                      # noqa: BLE001
                hook_error.append(exc)
                return 1
        hook = _ffi.ON_STEP_FN(on_step)
        opt.on_step = hook
    ctx = C.c_void_p()
    check(lib.rbpf_loc_create(C.byref(mstruct), C.byref(prob.c), C.byref(blk), C.byref(opt), C.byref(ctx)))
    try:
        try:
            check(lib.rbpf_loc_advance(ctx, T))
        except RBPFError as exc:
            if exc.status == _ffi.RBPF_ERR_CALLBACK and hook_error:
                raise hook_error[0] from exc
            raise
        o, b = _loc_out(N, T, T, extras)
        check(lib.rbpf_loc_finish(ctx, C.byref(o)))
    finally:
        lib.rbpf_destroy(ctx)
    if o.first_degenerate_step >= 0:
        warnings.warn(f"Weights filter close to zero at t={o.first_degenerate_step + 1} !!!", RuntimeWarning, stacklevel=2)
    if extras:
        ex = dict(logw=b["trace_logw"].T.copy(), w=b["trace_w"].T.copy(), ai=b["trace_ai"].T.copy(), xn=b["final_xn"],
                  xn_traj=b["xn_traj"], log_sum_w=b["log_sum_w"], first_degenerate_step=int(o.first_degenerate_step))
        return b["traj_max"], b["traj_mean"], ex
    return b["traj_max"], b["traj_mean"]


def _device_map_localization(mp, odometry, y, x0_nonLin, Q, N_P, dt, makePlots, rng, extras, n_devices, lazy_depth):
    """particleFilterLocalization in a DeviceMap: the binding drives a generic localisation context with the map's handles."""
    import warnings
    lib = load_library()
    prob = _DeviceMapProblem(mp, odometry, y, x0_nonLin, Q, N_P, dt)
    N, T, nN = prob.N_P, prob.N_T, prob.nNonLin
    landmark = isinstance(mp, DeviceLandmarkMap)                  # its driver keeps the handle's yhat of every step's best particle
    if lib.rbpf_device_count() < 1:
        raise RBPFError(_ffi.RBPF_ERR_NO_DEVICE, "no HIP device: the localisation filter has no CPU fallback")
    opt = _ffi.rbpf_options(keep_history=1, trace=1 if extras else 0, n_devices=int(n_devices), lazy_depth=int(lazy_depth))
    hook_error = []
    if makePlots is not None:
        def on_step(view_p, _user):
            try:
                v = view_p.contents
                t = int(v.t)
                o, b = _loc_out(N, T, t + 1, True, trace=False, nN=nN)
                check(lib.rbpf_loc_finish(C.c_void_p(v.ctx), C.byref(o)))
                xn_traj = np.zeros((nN, N, T))
                xn_traj[:, :, :t + 1] = b["xn_traj"]
                yhattraj = driver.yhattraj() if landmark else np.full((prob.ny, T), np.nan)
                makePlots(b["final_xn"], b["traj_max"], yhattraj, xn_traj, b["traj_mean"])
                return 0
            except Exception as exc:                                                      # noqa: BLE001
                hook_error.append(exc)
                return 1
        hook = _ffi.ON_STEP_FN(on_step)
        opt.on_step = hook
    ctx, _keep = _device_map_create(lib, mp, prob, rng, opt)      # (n_devices / lazy_depth: refused here, before anything is computed)
    try:
        try:
            driver = mp._driver(lib, ctx, prob)                    # (alive until the context is gone: it owns what the last step reads)
            driver.advance(T)
        except RBPFError as exc:
            if exc.status == _ffi.RBPF_ERR_CALLBACK and hook_error:
                raise hook_error[0] from exc
            raise
        o, b = _loc_out(N, T, T, extras, nN=nN)
        check(lib.rbpf_loc_finish(ctx, C.byref(o)))
        yhattraj = driver.yhattraj() if landmark and extras else None
    finally:
        lib.rbpf_destroy(ctx)
    if o.first_degenerate_step >= 0:
        warnings.warn(f"Weights filter close to zero at t={o.first_degenerate_step + 1} !!!", RuntimeWarning, stacklevel=3)
    if extras:
        ex = dict(logw=b["trace_logw"].T.copy(), w=b["trace_w"].T.copy(), ai=b["trace_ai"].T.copy(), xn=b["final_xn"],
                  xn_traj=b["xn_traj"], log_sum_w=b["log_sum_w"], first_degenerate_step=int(o.first_degenerate_step))
        if landmark:
            ex["yhattraj"] = yhattraj
        return b["traj_max"], b["traj_mean"], ex
    return b["traj_max"], b["traj_mean"]


def loc_workspace_bytes(map_struct, prob_struct, opt=None):
    """rbpf_loc_workspace_bytes (no device access)."""
    lib = load_library()
    nbytes = C.c_size_t(0)
    check(lib.rbpf_loc_workspace_bytes(C.byref(map_struct), C.byref(prob_struct), C.byref(opt) if opt is not None else None,
                                       C.byref(nbytes)))
    return int(nbytes.value)


class LocalizationSession:
    """rbpf_loc_create / advance / sync / finish / destroy: the counterpart of FilterSession for the localisation filter."""

    def __init__(self, loc_map, odometry, y, x0_nonLin, Q, N_P, dt, rng=None, keep_history=False, trace=False):
        self.lib = load_library()
        self.map = loc_map
        self.opt = _ffi.rbpf_options(keep_history=1 if keep_history else 0, trace=1 if trace else 0)
        self.hist = bool(keep_history)
        self.ctx = C.c_void_p()
        self.driver = None
        if isinstance(loc_map, DeviceMap):                        # a generic map: the binding drives the context with the map's handles
            self.prob = _DeviceMapProblem(loc_map, odometry, y, x0_nonLin, Q, N_P, dt)
            self.nN = self.prob.nNonLin
            self.ctx, self._rng = _device_map_create(self.lib, loc_map, self.prob, rng, self.opt)
            try:
                self.driver = loc_map._driver(self.lib, self.ctx, self.prob)
            except Exception:
                self.close()
                raise
            return
        self.nN = 7
        self.prob = _LocProblem(odometry, y, x0_nonLin, Q, N_P, dt)
        self.mstruct = loc_map._loc_map(self.prob.N_P)
        self.blk, self._rng = _rng_block(rng, self.prob.N_P, self.prob.N_T, 6, 1)
        check(self.lib.rbpf_loc_create(C.byref(self.mstruct), C.byref(self.prob.c), C.byref(self.blk), C.byref(self.opt),
                                       C.byref(self.ctx)))

    def advance(self, n_steps):
        if self.driver is not None:
            self.driver.advance(n_steps)
            return
        check(self.lib.rbpf_loc_advance(self.ctx, int(n_steps)))

    def sync(self):
        check(self.lib.rbpf_sync(self.ctx))

    def tell(self):
        t = C.c_int32(0)
        check(self.lib.rbpf_filter_tell(self.ctx, C.byref(t)))
        return t.value

    def finish(self, extras=False):
        o, b = _loc_out(self.prob.N_P, self.prob.N_T, self.tell(), extras, self.hist, bool(self.opt.trace), nN=self.nN)
        check(self.lib.rbpf_loc_finish(self.ctx, C.byref(o)))
        b["first_degenerate_step"] = int(o.first_degenerate_step)
        if extras and isinstance(self.driver, _LandmarkMapDriver):
            b["yhattraj"] = self.driver.yhattraj()
        return b

    def history(self):
        """rbpf_loc_history: the forward particles as propagated, NOT traced back, [7 x N_P x T_done] (needs keep_history;
        n_nonlin rows in a DeviceMap)."""
        X = np.empty((self.nN, self.prob.N_P, self.tell()), order="F")
        check(self.lib.rbpf_loc_history(self.ctx, _dp(X)))
        return X

    def backward_simulate(self, n_traj, rng=None, want=("xs_traj", "index", "traj_smooth_mean"), method="all_pairs", max_tries=None):
        """rbpf_loc_backward_simulate: n_traj trajectories drawn backwards through the stored particles (keep_history and trace,
        every step done).  rng: None / PhiloxRNG(seed): the device generator (PhiloxRNG.backward_uniforms(n_traj, N_T) are its
        draws); an array u [N_T x n_traj] of uniforms in (0, 1]: replay.  Returns a dict of the arrays named in `want`:
        xs_traj [7 x n_traj x N_T], index [n_traj x N_T] (0-based), traj_smooth_mean [7 x N_T].  In a DeviceMap: n_nonlin rows in
        place of 7, with the map's DeviceTransition (rbpf_loc_generic_backward_*); without one the call is refused.
        method="rejection" (rbpf_loc_backward_simulate_reject, rbpf_loc_generic_backward_reject_begin): the same law, steps N_T-2 .. 0
        by up to max_tries proposals from the weights per trajectory, accepted against the transition density, before the all-pairs
        pass draws the trajectories that are left; rng is None or a PhiloxRNG, and `want` may name n_fallback [N_T] (trajectories
        left to the all-pairs pass at every step) and n_tries [N_T] (int64, tries summed over the trajectories).  max_tries = 0 gives
        the arrays of method="all_pairs" with the same seed bit for bit.  max_tries=None is reject_default_max_tries(N_P, n_traj)."""
        if method not in ("all_pairs", "rejection"):
            raise ValueError(f"unknown method {method!r}: 'all_pairs' or 'rejection'")
        reject = method == "rejection"
        if not reject and max_tries is not None:
            raise ValueError("max_tries belongs to method='rejection'")
        if self.driver is not None and self.map.transition is None:
            raise RBPFError(_ffi.RBPF_ERR_UNSUPPORTED, _NO_BACKWARD_IN_DEVICE_MAP)
        M, T = int(n_traj), self.prob.N_T
        seed, u = 0, None
        if rng is None:
            rng = PhiloxRNG(1)
        if isinstance(rng, PhiloxRNG):
            seed = int(rng.seed)
        elif reject:
            raise ValueError("method='rejection' draws its tries on the device: rng must be None or a PhiloxRNG; uniforms are replayed by the "
                             "probes loc_backward_reject_step and device_map_backward_reject_step")
        else:
            u = np.ascontiguousarray(np.asarray(rng, dtype=np.float64))
            if M >= 1 and u.shape != (T, M):
                raise ValueError(f"u must be [{T} x {M}] (row t = step t)")
        if reject:
            max_tries = reject_default_max_tries(self.prob.N_P, M) if max_tries is None else int(max_tries)
            if max_tries < 0:
                raise ValueError("max_tries must be >= 0")
        unknown = set(want) - ({"xs_traj", "index", "traj_smooth_mean"} | ({"n_fallback", "n_tries"} if reject else set()))
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        Mb = max(M, 0)
        b = {}
        if "xs_traj" in want:
            b["xs_traj"] = np.empty((self.nN, Mb, T), order="F")
        if "index" in want:
            b["index"] = np.zeros((Mb, T), dtype=np.int32, order="F")
        if "traj_smooth_mean" in want:
            b["traj_smooth_mean"] = np.empty((self.nN, T), order="F")
        if "n_fallback" in want:
            b["n_fallback"] = np.zeros(T, dtype=np.int32)
        if "n_tries" in want:
            b["n_tries"] = np.zeros(T, dtype=np.int64)
        if self.driver is not None:
            self._backward_in_device_map(M, u, seed, b, max_tries if reject else None)
            return b
        if reject:
            check(self.lib.rbpf_loc_backward_simulate_reject(self.ctx, M, C.c_uint64(seed), max_tries,
                                                             _dp(b["xs_traj"]) if "xs_traj" in b else None,
                                                             _ip(b["index"]) if "index" in b else None,
                                                             _dp(b["traj_smooth_mean"]) if "traj_smooth_mean" in b else None,
                                                             _ip(b["n_fallback"]) if "n_fallback" in b else None,
                                                             b["n_tries"].ctypes.data_as(C.POINTER(C.c_int64)) if "n_tries" in b else None))
            return b
        check(self.lib.rbpf_loc_backward_simulate(self.ctx, M, _dp(u) if u is not None else None, C.c_uint64(seed),
                                                  _dp(b["xs_traj"]) if "xs_traj" in b else None,
                                                  _ip(b["index"]) if "index" in b else None,
                                                  _dp(b["traj_smooth_mean"]) if "traj_smooth_mean" in b else None))
        return b

    def _transition_pages(self):
        """What a pass with the map's DeviceTransition needs before it begins: (rows, angle_mask, quat_pos, n_sel = the rows of mu
        (n_res + 1 with a quaternion block), covs, page).  covs[(page of dt, page of Q)] = cov(dt, Q), one per distinct page of steps
        0 .. N_T-2, each checked here, before any kernel runs."""
        tr, prob = self.map.transition, self.prob
        rows, mask, qpos, n_res = tr.layout(self.nN)
        page = lambda a, t: t if a > 1 else 0                                                     # noqa: E731
        covs = {}
        for t in range(prob.N_T - 1):
            key = (page(prob._dt.size, t), page(prob._Q.shape[2], t))
            if key not in covs:
                c = tr.covariance(prob._dt[key[0]], prob._Q[:, :, key[1]], n_res)
                try:
                    if not np.all(np.isfinite(c)):
                        raise np.linalg.LinAlgError
                    np.linalg.cholesky(c)
                except np.linalg.LinAlgError:
                    raise RBPFError(_ffi.RBPF_ERR_CHOL_FAILED, f"cov(dt, Q) of step {t} is not positive definite: the transition density "
                                                               "does not exist") from None
                covs[key] = c
        return np.asarray(rows, dtype=np.int32), mask, qpos, len(rows), covs, page

    def _backward_in_device_map(self, M, u, seed, b, max_tries=None):
        """The backward pass with the map's DeviceTransition: the covariance pages on the host first, then begin, one
        particles_device / mean handle / step_device per step in stream order, finish (also the way out of a failed handle).
        max_tries: None, or the tries of method="rejection" (rbpf_loc_generic_backward_reject_begin; the same steps drive it)."""
        lib, drv, tr, prob = self.lib, self.driver, self.map.transition, self.prob
        torch, T, N, nN = drv.torch, prob.N_T, prob.N_P, self.nN
        rows_a, mask, qpos, n_sel, covs, page = self._transition_pages()
        if max_tries is None:
            check(lib.rbpf_loc_generic_backward_pose_begin(self.ctx, M, _dp(u) if u is not None else None, C.c_uint64(seed), n_sel, _ip(rows_a),
                                                           mask, qpos))
        else:
            check(lib.rbpf_loc_generic_backward_reject_begin(self.ctx, M, C.c_uint64(seed), int(max_tries), n_sel, _ip(rows_a), mask, qpos))
        try:
            with torch.cuda.stream(drv.stream):
                for _ in range(T):
                    t, xn = C.c_int32(0), C.c_void_p()
                    check(lib.rbpf_loc_generic_backward_particles_device(self.ctx, C.byref(t), C.byref(xn)))
                    t = t.value
                    if t == T - 1:                                # this draw reads log w only
                        check(lib.rbpf_loc_generic_backward_step_device(self.ctx, None, None))
                        continue
                    X = drv._view(torch, xn, (nN, N), drv.device)
                    Q = drv.Q[page(drv.Q.shape[0], t)]
                    mu = tr.mean(X, drv.odo[t], float(drv.dt[page(drv.dt.size, t)]), Q)
                    if not torch.is_tensor(mu) or tuple(mu.shape) != (n_sel, N) or mu.dtype != torch.float64 or not mu.is_cuda:
                        what = f"{tuple(mu.shape)} {mu.dtype} on {mu.device}" if torch.is_tensor(mu) else type(mu).__name__
                        raise ValueError(f"mean returned {what}, expected a float64 device tensor of shape {(n_sel, N)}")
                    mu = mu.contiguous()
                    self._keep_mu = mu                            # read in stream order by the step just enqueued
                    check(lib.rbpf_loc_generic_backward_step_device(self.ctx, C.c_void_p(mu.data_ptr()),
                                                                    _dp(covs[(page(prob._dt.size, t), page(prob._Q.shape[2], t))])))
        except BaseException:
            lib.rbpf_loc_generic_backward_finish(self.ctx, None, None, None)
            self._keep_mu = None
            raise
        try:
            check(lib.rbpf_loc_generic_backward_finish(self.ctx, _dp(b["xs_traj"]) if "xs_traj" in b else None,
                                                       _ip(b["index"]) if "index" in b else None,
                                                       _dp(b["traj_smooth_mean"]) if "traj_smooth_mean" in b else None))
            if "n_fallback" in b or "n_tries" in b:
                check(lib.rbpf_loc_generic_backward_reject_stats(self.ctx, _ip(b["n_fallback"]) if "n_fallback" in b else None,
                                                                 b["n_tries"].ctypes.data_as(C.POINTER(C.c_int64)) if "n_tries" in b else None))
        finally:
            self._keep_mu = None

    def map_trajectory(self, want=("x_map", "index", "score")):
        """rbpf_loc_map_trajectory: the MAP trajectory over the stored particles (keep_history and trace, every step done), a Viterbi
        recursion whose states at step t are the N_P particles (Godsill, Doucet & West 2001).  Returns a dict of what `want` names:
        x_map [7 x N_T] (one stored particle per step), index [N_T] (0-based, which one) and score = delta_{T-1}(i_{T-1}), the log
        joint of the path and the measurements up to constants that do not depend on the path.  Among equal candidates the lowest
        index wins.  In a DeviceMap: n_nonlin rows in place of 7, with the map's DeviceTransition (rbpf_loc_generic_map_*); without
        one the call is refused."""
        if self.driver is not None and self.map.transition is None:
            raise RBPFError(_ffi.RBPF_ERR_UNSUPPORTED, _NO_BACKWARD_IN_DEVICE_MAP)
        unknown = set(want) - {"x_map", "index", "score"}
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        T = self.prob.N_T
        x_map = np.empty((self.nN, T), order="F") if "x_map" in want else None
        index = np.zeros(T, dtype=np.int32) if "index" in want else None
        score = C.c_double(0.0)
        outs = (_dp(x_map) if x_map is not None else None, _ip(index) if index is not None else None,
                C.byref(score) if "score" in want else None)
        if self.driver is not None:
            self._map_in_device_map(outs)
        else:
            check(self.lib.rbpf_loc_map_trajectory(self.ctx, *outs))
        b = {}
        if x_map is not None:
            b["x_map"] = x_map
        if index is not None:
            b["index"] = index
        if "score" in want:
            b["score"] = float(score.value)
        return b

    def _map_in_device_map(self, outs):
        """The MAP pass with the map's DeviceTransition: the covariance pages on the host first, then begin, one particles_device /
        mean handle / step_device per step t = 0 .. N_T-2 in stream order, finish (also the way out of a failed handle)."""
        self._stepped_pass_in_device_map("map", outs)

    def _stepped_pass_in_device_map(self, family, outs):
        """A pass of rbpf_loc_generic_<family>_* (map: t = 0 .. N_T-2; marginal and pair_stats: t = N_T-2 .. 0) whose every step takes
        the `mean` handle's mu and cov(dt, Q); the library names the step."""
        lib, drv, tr, prob = self.lib, self.driver, self.map.transition, self.prob
        torch, T, N, nN = drv.torch, prob.N_T, prob.N_P, self.nN
        begin, particles, step, finish = (getattr(lib, f"rbpf_loc_generic_{family}_{f}")
                                          for f in ("begin", "particles_device", "step_device", "finish"))
        rows_a, mask, qpos, n_sel, covs, page = self._transition_pages()
        check(begin(self.ctx, n_sel, _ip(rows_a), mask, qpos))
        try:
            with torch.cuda.stream(drv.stream):
                for _ in range(T - 1):
                    t, xn = C.c_int32(0), C.c_void_p()
                    check(particles(self.ctx, C.byref(t), C.byref(xn)))
                    t = t.value
                    X = drv._view(torch, xn, (nN, N), drv.device)
                    Q = drv.Q[page(drv.Q.shape[0], t)]
                    mu = tr.mean(X, drv.odo[t], float(drv.dt[page(drv.dt.size, t)]), Q)
                    if not torch.is_tensor(mu) or tuple(mu.shape) != (n_sel, N) or mu.dtype != torch.float64 or not mu.is_cuda:
                        what = f"{tuple(mu.shape)} {mu.dtype} on {mu.device}" if torch.is_tensor(mu) else type(mu).__name__
                        raise ValueError(f"mean returned {what}, expected a float64 device tensor of shape {(n_sel, N)}")
                    mu = mu.contiguous()
                    self._keep_mu = mu                            # read in stream order by the step just enqueued
                    check(step(self.ctx, C.c_void_p(mu.data_ptr()), _dp(covs[(page(prob._dt.size, t), page(prob._Q.shape[2], t))])))
        except BaseException:
            finish(self.ctx, *([None] * len(outs)))
            self._keep_mu = None
            raise
        try:
            check(finish(self.ctx, *outs))
        finally:
            self._keep_mu = None

    def smoothed_marginals(self, want=("w_smooth", "mean", "ess")):
        """rbpf_loc_marginal_smooth: the marginal smoothing weights of EVERY stored particle (keep_history and trace, every step done),
        forward filtering backward smoothing (Doucet, Godsill & Andrieu 2000): deterministic, no uniforms, no n_traj.  Returns a dict
        of what `want` names: w_smooth [N_P x N_T] (column N_T-1 is the filter's last weights bit for bit), mean [7 x N_T] and cov
        [7 x 7 x N_T] (plain weighted moments of all rows: quaternion and angle rows get no special handling), ess [N_T] =
        1 / sum w_smooth^2 and mass [N_T], the sum of a step's weights before its normalisation (1 in exact arithmetic).  In a
        DeviceMap: n_nonlin rows in place of 7, with the map's DeviceTransition (rbpf_loc_generic_marginal_*); without one the call
        is refused."""
        if self.driver is not None and self.map.transition is None:
            raise RBPFError(_ffi.RBPF_ERR_UNSUPPORTED, _NO_BACKWARD_IN_DEVICE_MAP)
        unknown = set(want) - {"w_smooth", "mean", "cov", "ess", "mass"}
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        T, N, nN = self.prob.N_T, self.prob.N_P, self.nN
        shapes = dict(w_smooth=(N, T), mean=(nN, T), cov=(nN, nN, T), ess=(T,), mass=(T,))
        b = {k: np.empty(shapes[k], order="F") for k in ("w_smooth", "mean", "cov", "ess", "mass") if k in want}
        outs = tuple(_dp(b[k]) if k in b else None for k in ("w_smooth", "mean", "cov", "ess", "mass"))
        if self.driver is not None:
            self._stepped_pass_in_device_map("marginal", outs)
        else:
            check(self.lib.rbpf_loc_marginal_smooth(self.ctx, *outs))
        return b

    def transition_statistics(self, want=("S", "m", "pair_mass", "w_smooth", "mean")):
        """rbpf_loc_pair_stats_smooth: the marginal smoother, and with its weights the two-slice (pairwise) smoothed moments of the
        transition residual (keep_history and trace, every step done).  With xi_t(i, j) = w_t(i) p(X[t+1][:, j] | X[t][:, i])
        w_{t+1|T}(j) / D_t(j), which sums to 1 over all pairs, and r_ij the UN-WHITENED residual of the transition density
        ([p~ - (p_i + dx); phi] in a DenseMagMap; in a DeviceMap the wrapped differences and logq of the quaternion error, in the
        order of the DeviceTransition's cov), returns a dict of what `want` names: S [n_res x n_res x (N_T-1)] = sum_ij xi r r',
        m [n_res x (N_T-1)] = sum_ij xi r, pair_mass [N_T-1] = sum_ij xi (1 in exact arithmetic); page t belongs to the steps
        (t, t+1).  The outputs of smoothed_marginals (w_smooth, mean, cov, ess, mass) may be named too and are bit for bit what it
        returns.  xi is never stored.  transition_noise_estimate turns S (and m) into an estimate of Q.  In a DeviceMap without a
        DeviceTransition the call is refused."""
        if self.driver is not None and self.map.transition is None:
            raise RBPFError(_ffi.RBPF_ERR_UNSUPPORTED, _NO_BACKWARD_IN_DEVICE_MAP)
        names = ("w_smooth", "mean", "cov", "ess", "mass", "S", "m", "pair_mass")
        unknown = set(want) - set(names)
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        T, N, nN = self.prob.N_T, self.prob.N_P, self.nN
        n_res = 6 if self.driver is None else self.map.transition.layout(nN)[3]
        shapes = dict(w_smooth=(N, T), mean=(nN, T), cov=(nN, nN, T), ess=(T,), mass=(T,), S=(n_res, n_res, T - 1), m=(n_res, T - 1),
                      pair_mass=(T - 1,))
        b = {k: np.empty(shapes[k], order="F") for k in names if k in want}
        outs = tuple(_dp(b[k]) if k in b else None for k in names)
        if self.driver is not None:
            self._stepped_pass_in_device_map("pair_stats", outs)
        else:
            check(self.lib.rbpf_loc_pair_stats_smooth(self.ctx, *outs))
        return b

    def running_statistics(self, want=("S_run", "m_run")):
        """rbpf_loc_forward_stats_update: the two-slice statistics of transition_statistics, accumulated over the steps and available
        WHILE the run goes on -- the forward-only form of FFBSm for an additive functional (Del Moral, Doucet & Singh 2010).  Needs
        keep_history and trace and at least 2 steps done, NOT every step.  Returns a dict of what `want` names, with P = tell() - 1:
        S_run [n_res x n_res x P] and m_run [n_res x P], page k the FFBSm estimate from the steps 0 .. k+1 alone of
        sum_{s<=k} E[r r' / dt_s] and sum_{s<=k} E[r] (r as in transition_statistics); mass_run [P] (1 in exact arithmetic);
        tau_S [n_res x n_res x N_P] and tau_m [n_res x N_P], the per-particle carry of the latest step.  Once every step is done the
        last page equals sum_t S_t / dt_t and sum_t m_t of transition_statistics.  The carry is kept in the session: a call folds
        in only the pairs of steps stored since the last one (one all-pairs step each), and holds its device memory until
        reset_running_statistics() or close().  In a DeviceMap the `mean` handle is called once per newly folded step, ascending;
        without a DeviceTransition the call is refused.  running_noise_estimate turns the pages into a running estimate of Q."""
        if self.driver is not None and self.map.transition is None:
            raise RBPFError(_ffi.RBPF_ERR_UNSUPPORTED, _NO_BACKWARD_IN_DEVICE_MAP)
        names = ("S_run", "m_run", "mass_run", "tau_S", "tau_m")
        unknown = set(want) - set(names)
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        N, nN, P = self.prob.N_P, self.nN, max(self.tell() - 1, 0)
        n_res = 6 if self.driver is None else self.map.transition.layout(nN)[3]
        shapes = dict(S_run=(n_res, n_res, P), m_run=(n_res, P), mass_run=(P,), tau_S=(n_res, n_res, N), tau_m=(n_res, N))
        b = {k: np.empty(shapes[k], order="F") for k in names if k in want}
        outs = tuple(_dp(b[k]) if k in b else None for k in names)
        if self.driver is not None:
            self._forward_pass_in_device_map(outs)
        else:
            check(self.lib.rbpf_loc_forward_stats_update(self.ctx, *outs))
        return b

    def reset_running_statistics(self):
        """rbpf_loc_forward_stats_reset: hands the carry of running_statistics back; the next call starts again at the first step."""
        if self.driver is not None:
            check(self.lib.rbpf_loc_generic_forward_stats_reset(self.ctx))
        else:
            check(self.lib.rbpf_loc_forward_stats_reset(self.ctx))

    def _forward_pass_in_device_map(self, outs):
        """The forward variant of _stepped_pass_in_device_map for rbpf_loc_generic_forward_stats_*: the steps ascend from the first
        pair not yet folded in to tell() - 2, every one with the `mean` handle's mu, cov(dt, Q) and 1 / dt.  A failed handle closes
        the stepping and leaves the carry where the last complete step put it."""
        lib, drv, tr, prob = self.lib, self.driver, self.map.transition, self.prob
        torch, N, nN = drv.torch, prob.N_P, self.nN
        rows_a, mask, qpos, n_sel, covs, page = self._transition_pages()
        check(lib.rbpf_loc_generic_forward_stats_begin(self.ctx, n_sel, _ip(rows_a), mask, qpos))
        try:
            with torch.cuda.stream(drv.stream):
                while True:
                    t, xn = C.c_int32(0), C.c_void_p()
                    st = lib.rbpf_loc_generic_forward_stats_particles_device(self.ctx, C.byref(t), C.byref(xn))
                    if st == _ffi.RBPF_ERR_STATE:                 # (the stepping is open: every stored pair is folded in)
                        break
                    check(st)
                    t = t.value
                    X = drv._view(torch, xn, (nN, N), drv.device)
                    Q = drv.Q[page(drv.Q.shape[0], t)]
                    dt = float(drv.dt[page(drv.dt.size, t)])
                    mu = tr.mean(X, drv.odo[t], dt, Q)
                    if not torch.is_tensor(mu) or tuple(mu.shape) != (n_sel, N) or mu.dtype != torch.float64 or not mu.is_cuda:
                        what = f"{tuple(mu.shape)} {mu.dtype} on {mu.device}" if torch.is_tensor(mu) else type(mu).__name__
                        raise ValueError(f"mean returned {what}, expected a float64 device tensor of shape {(n_sel, N)}")
                    if not dt > 0.0:
                        raise ValueError(f"dt of step {t} is not positive: S / dt does not exist")
                    mu = mu.contiguous()
                    self._keep_mu = mu                            # read in stream order by the step just enqueued
                    check(lib.rbpf_loc_generic_forward_stats_step_device(self.ctx, C.c_void_p(mu.data_ptr()),
                                                                         _dp(covs[(page(prob._dt.size, t), page(prob._Q.shape[2], t))]), 1.0 / dt))
        except BaseException:
            lib.rbpf_loc_generic_forward_stats_finish(self.ctx, None, None, None, None, None)
            self._keep_mu = None
            raise
        try:
            check(lib.rbpf_loc_generic_forward_stats_finish(self.ctx, *outs))
        finally:
            self._keep_mu = None

    def fixed_lag_estimates(self, lag, want=("mean",)):
        """rbpf_loc_fixed_lag_update: the state with a fixed delay, E[x_s | y_{0:s+lag}] and its covariance, available WHILE the run
        goes on at one all-pairs pass per new time step whatever the lag -- the forward-only form of FFBSm (the estimator of
        smoothed_marginals) for the moments of the last `lag` states.  Needs keep_history and trace and at least 2 steps done, NOT
        every step.  Returns a dict of what `want` names, with Td = tell() and n the state rows (plain weighted moments of all of
        them: quaternion and angle rows get no special handling):
          mean [n x Td]              column s: E[x_s | y_{0:min(s+lag, Td-1)}]
          cov [n x n x Td]           its covariance; naming it at the first call makes the carry hold second moments (moments = 2)
          lag_of [Td]                the lag actually applied: `lag` except in the last `lag` columns
          by_lag [n x (lag+1) x Td]  E[x_{t-l} | y_{0:t}] at [:, l, t], NaN where t - l < 0
          mass [Td]                  1 in exact arithmetic, mass[0] = 1
        Columns with lag_of == lag are final and bit-identical in every later call; the others are provisional.  The carry is kept
        in the session: a call folds in only the steps stored since the last one, and holds its device memory until
        reset_fixed_lag() or close().  Another lag, or cov after a first call without it, is refused: reset_fixed_lag() first.  In a
        DeviceMap the `mean` handle is called once per newly folded step, ascending; without a DeviceTransition the call is
        refused."""
        if self.driver is not None and self.map.transition is None:
            raise RBPFError(_ffi.RBPF_ERR_UNSUPPORTED, _NO_BACKWARD_IN_DEVICE_MAP)
        names = ("mean", "cov", "lag_of", "by_lag", "mass")
        unknown = set(want) - set(names)
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        lag = int(lag)
        held = getattr(self, "_fixed_lag", None)
        moments = 2 if "cov" in want or (held is not None and held == (lag, 2)) else 1
        n, Td = self.nN, self.tell()
        H = n if moments == 1 else n * (n + 3) // 2
        pages, means = np.empty(((max(lag, 0) + 1) * H + 1, Td), order="F"), np.empty((n, Td), order="F")
        if self.driver is not None:
            self._fixed_lag_pass_in_device_map(lag, moments, (_dp(pages), _dp(means)))
        else:
            check(self.lib.rbpf_loc_fixed_lag_update(self.ctx, lag, moments, _dp(pages), _dp(means)))
        self._fixed_lag = (lag, moments)
        out = fixed_lag_assemble(pages, means, lag, moments)
        return {k: out[k] for k in names if k in want}

    def reset_fixed_lag(self):
        """rbpf_loc_fixed_lag_reset: hands the carry of fixed_lag_estimates back; the next call starts again at the first step and
        may name another lag."""
        if self.driver is not None:
            check(self.lib.rbpf_loc_generic_fixed_lag_reset(self.ctx))
        else:
            check(self.lib.rbpf_loc_fixed_lag_reset(self.ctx))
        self._fixed_lag = None

    def _fixed_lag_pass_in_device_map(self, lag, moments, outs):
        """_forward_pass_in_device_map for rbpf_loc_generic_fixed_lag_*: the steps ascend from the last one folded in to tell() - 2,
        every one with the `mean` handle's mu and cov(dt, Q).  A failed handle closes the stepping and leaves the carry where the
        last complete step put it."""
        lib, drv, tr, prob = self.lib, self.driver, self.map.transition, self.prob
        torch, N, nN = drv.torch, prob.N_P, self.nN
        rows_a, mask, qpos, n_sel, covs, page = self._transition_pages()
        check(lib.rbpf_loc_generic_fixed_lag_begin(self.ctx, n_sel, _ip(rows_a), mask, qpos, lag, moments))
        try:
            with torch.cuda.stream(drv.stream):
                while True:
                    t, xn = C.c_int32(0), C.c_void_p()
                    st = lib.rbpf_loc_generic_fixed_lag_particles_device(self.ctx, C.byref(t), C.byref(xn))
                    if st == _ffi.RBPF_ERR_STATE:                 # (the stepping is open: every stored step is folded in)
                        break
                    check(st)
                    t = t.value
                    X = drv._view(torch, xn, (nN, N), drv.device)
                    Q = drv.Q[page(drv.Q.shape[0], t)]
                    dt = float(drv.dt[page(drv.dt.size, t)])
                    mu = tr.mean(X, drv.odo[t], dt, Q)
                    if not torch.is_tensor(mu) or tuple(mu.shape) != (n_sel, N) or mu.dtype != torch.float64 or not mu.is_cuda:
                        what = f"{tuple(mu.shape)} {mu.dtype} on {mu.device}" if torch.is_tensor(mu) else type(mu).__name__
                        raise ValueError(f"mean returned {what}, expected a float64 device tensor of shape {(n_sel, N)}")
                    mu = mu.contiguous()
                    self._keep_mu = mu                            # read in stream order by the step just enqueued
                    check(lib.rbpf_loc_generic_fixed_lag_step_device(self.ctx, C.c_void_p(mu.data_ptr()),
                                                                     _dp(covs[(page(prob._dt.size, t), page(prob._Q.shape[2], t))])))
        except BaseException:
            lib.rbpf_loc_generic_fixed_lag_finish(self.ctx, None, None)
            self._keep_mu = None
            raise
        try:
            check(lib.rbpf_loc_generic_fixed_lag_finish(self.ctx, *outs))
        finally:
            self._keep_mu = None

    def close(self):
        if self.ctx:
            self.lib.rbpf_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def loc_map_workspace_bytes(N_P, N_T):
    """rbpf_loc_map_workspace_bytes (no device access)."""
    lib = load_library()
    nbytes = C.c_size_t(0)
    check(lib.rbpf_loc_map_workspace_bytes(int(N_P), int(N_T), C.byref(nbytes)))
    return int(nbytes.value)


def loc_map_step(xn, delta, xs_next, odo, dt, Q, reps=1):
    """rbpf_loc_map_step, the kernel-level probe: one step of the MAP recursion on the caller's arrays.  xn [7 x N], delta [N],
    xs_next [7 x M] (the successors), odo [7], Q [6 x 6] -> (best [M], arg [M], median ms of one step)."""
    lib = load_library()
    xn = np.asfortranarray(np.asarray(xn, dtype=np.float64).reshape(7, -1))
    xs_next = np.asfortranarray(np.asarray(xs_next, dtype=np.float64).reshape(7, -1))
    N, M = xn.shape[1], xs_next.shape[1]
    delta = np.ascontiguousarray(np.asarray(delta, dtype=np.float64).ravel())
    odo = np.ascontiguousarray(np.asarray(odo, dtype=np.float64).ravel())
    Q = np.asfortranarray(np.asarray(Q, dtype=np.float64).reshape(6, 6))
    if delta.size != N or odo.size != 7:
        raise ValueError("delta must be [N] and odo [7]")
    best, arg = np.empty(M), np.zeros(M, dtype=np.int32)
    ms = C.c_double(0.0)
    check(lib.rbpf_loc_map_step(N, M, _dp(xn), _dp(delta), _dp(xs_next), _dp(odo), float(dt), _dp(Q), _dp(best), _ip(arg), int(reps), C.byref(ms)))
    return best, arg, ms.value


def particleMapLocalization(dynModel, measModel, odometry, y, x0_nonLin, Q, R, N_P, dt, *, rng=None, extras=False):
    """The MAP trajectory of localisation in a fixed map: particleFilterLocalization, then MAP sequence estimation over its stored
    particles (LocalizationSession.map_trajectory) -> (x_map [7 x N_T], score[, extras]).  dynModel / measModel, R and rng as
    particleSmootherLocalization takes them: the handles of a DenseMagMap, or a DeviceMap with a DeviceTransition as dynModel
    (measModel None), n_nonlin rows in place of 7.  extras: the filter's outputs (traj_max, traj_mean, first_degenerate_step, ...)
    and `index` [N_T], the particle of every step."""
    import warnings
    mp = _device_map(dynModel, measModel)
    if mp is not None and mp.transition is None:
        raise RBPFError(_ffi.RBPF_ERR_UNSUPPORTED, "particleMapLocalization: " + _NO_BACKWARD_IN_DEVICE_MAP)
    if mp is None:
        mp = _recognise_map(dynModel, measModel)
    with LocalizationSession(mp, odometry, y, x0_nonLin, Q, N_P, dt, rng=rng, keep_history=True, trace=True) as s:
        s.advance(s.prob.N_T)
        fwd = s.finish(extras=extras)
        if fwd["first_degenerate_step"] >= 0:
            warnings.warn(f"Weights filter close to zero at t={fwd['first_degenerate_step'] + 1} !!!", RuntimeWarning, stacklevel=2)
        out = s.map_trajectory()
    if extras:
        fwd["index"] = out["index"]
        return out["x_map"], out["score"], fwd
    return out["x_map"], out["score"]


def loc_marginal_workspace_bytes(N_P, N_T):
    """rbpf_loc_marginal_workspace_bytes (no device access)."""
    lib = load_library()
    nbytes = C.c_size_t(0)
    check(lib.rbpf_loc_marginal_workspace_bytes(int(N_P), int(N_T), C.byref(nbytes)))
    return int(nbytes.value)


def loc_marginal_step(xn, logw, xs_next, logws_next, odo, dt, Q, reps=1):
    """rbpf_loc_marginal_step, the kernel-level probe: one step of the marginal-smoothing recursion on the caller's arrays.  xn
    [7 x N], logw [N] = log w_t, xs_next [7 x M] (the successors), logws_next [M] = log w_{t+1|T} (-inf allowed in both), odo [7],
    Q [6 x 6] -> (D [M] = log sum_l w_t(l) p(j | l), lws [N] = log of the un-normalised w_{t|T}, median ms of one step)."""
    lib = load_library()
    xn = np.asfortranarray(np.asarray(xn, dtype=np.float64).reshape(7, -1))
    xs_next = np.asfortranarray(np.asarray(xs_next, dtype=np.float64).reshape(7, -1))
    N, M = xn.shape[1], xs_next.shape[1]
    logw = np.ascontiguousarray(np.asarray(logw, dtype=np.float64).ravel())
    logws_next = np.ascontiguousarray(np.asarray(logws_next, dtype=np.float64).ravel())
    odo = np.ascontiguousarray(np.asarray(odo, dtype=np.float64).ravel())
    Q = np.asfortranarray(np.asarray(Q, dtype=np.float64).reshape(6, 6))
    if logw.size != N or logws_next.size != M or odo.size != 7:
        raise ValueError("logw must be [N], logws_next [M] and odo [7]")
    D, lws = np.empty(M), np.empty(N)
    ms = C.c_double(0.0)
    check(lib.rbpf_loc_marginal_step(N, M, _dp(xn), _dp(logw), _dp(xs_next), _dp(logws_next), _dp(odo), float(dt), _dp(Q), _dp(D), _dp(lws),
                                     int(reps), C.byref(ms)))
    return D, lws, ms.value


def particleMarginalSmootherLocalization(dynModel, measModel, odometry, y, x0_nonLin, Q, R, N_P, dt, *, rng=None, extras=False):
    """The marginal smoother of localisation in a fixed map: particleFilterLocalization, then the marginal smoothing weights of its
    stored particles (LocalizationSession.smoothed_marginals) -> (traj_marginal_mean [7 x N_T], w_smooth [N_P x N_T][, extras]).
    dynModel / measModel, R and rng as particleMapLocalization takes them: the handles of a DenseMagMap, or a DeviceMap with a
    DeviceTransition as dynModel (measModel None), n_nonlin rows in place of 7.  extras: the filter's outputs (traj_max, traj_mean,
    first_degenerate_step, ...) and `cov`, `ess`, `mass` of every step."""
    import warnings
    mp = _device_map(dynModel, measModel)
    if mp is not None and mp.transition is None:
        raise RBPFError(_ffi.RBPF_ERR_UNSUPPORTED, "particleMarginalSmootherLocalization: " + _NO_BACKWARD_IN_DEVICE_MAP)
    if mp is None:
        mp = _recognise_map(dynModel, measModel)
    with LocalizationSession(mp, odometry, y, x0_nonLin, Q, N_P, dt, rng=rng, keep_history=True, trace=True) as s:
        s.advance(s.prob.N_T)
        fwd = s.finish(extras=extras)
        if fwd["first_degenerate_step"] >= 0:
            warnings.warn(f"Weights filter close to zero at t={fwd['first_degenerate_step'] + 1} !!!", RuntimeWarning, stacklevel=2)
        out = s.smoothed_marginals(want=("w_smooth", "mean", "cov", "ess", "mass") if extras else ("w_smooth", "mean"))
    if extras:
        fwd.update(cov=out["cov"], ess=out["ess"], mass=out["mass"])
        return out["mean"], out["w_smooth"], fwd
    return out["mean"], out["w_smooth"]


def loc_pair_stats_workspace_bytes(N_P, N_T):
    """rbpf_loc_pair_stats_workspace_bytes (no device access)."""
    lib = load_library()
    nbytes = C.c_size_t(0)
    check(lib.rbpf_loc_pair_stats_workspace_bytes(int(N_P), int(N_T), C.byref(nbytes)))
    return int(nbytes.value)


def loc_pair_stats_step(xn, logw, xs_next, logws_next, odo, dt, Q, reps=1):
    """rbpf_loc_pair_stats_step, the kernel-level probe: loc_marginal_step, and behind it the two-slice statistics of that step with
    its own mass -> (D [M], lws [N] un-normalised, S [6 x 6], m [6], pair_mass, median ms of the marginal step, the normalisation and
    the statistics pass together)."""
    lib = load_library()
    xn = np.asfortranarray(np.asarray(xn, dtype=np.float64).reshape(7, -1))
    xs_next = np.asfortranarray(np.asarray(xs_next, dtype=np.float64).reshape(7, -1))
    N, M = xn.shape[1], xs_next.shape[1]
    logw = np.ascontiguousarray(np.asarray(logw, dtype=np.float64).ravel())
    logws_next = np.ascontiguousarray(np.asarray(logws_next, dtype=np.float64).ravel())
    odo = np.ascontiguousarray(np.asarray(odo, dtype=np.float64).ravel())
    Q = np.asfortranarray(np.asarray(Q, dtype=np.float64).reshape(6, 6))
    if logw.size != N or logws_next.size != M or odo.size != 7:
        raise ValueError("logw must be [N], logws_next [M] and odo [7]")
    D, lws, S, m, pm = np.empty(M), np.empty(N), np.empty((6, 6), order="F"), np.empty(6), np.empty(1)
    ms = C.c_double(0.0)
    check(lib.rbpf_loc_pair_stats_step(N, M, _dp(xn), _dp(logw), _dp(xs_next), _dp(logws_next), _dp(odo), float(dt), _dp(Q), _dp(D), _dp(lws),
                                       _dp(S), _dp(m), _dp(pm), int(reps), C.byref(ms)))
    return D, lws, S, m, float(pm[0]), ms.value


def particleTransitionStatisticsLocalization(dynModel, measModel, odometry, y, x0_nonLin, Q, R, N_P, dt, *, rng=None, extras=False):
    """The two-slice statistics of localisation in a fixed map: particleFilterLocalization, then LocalizationSession.transition_statistics
    on its stored particles -> (S [n_res x n_res x (N_T-1)], m [n_res x (N_T-1)], pair_mass [N_T-1][, extras]).  dynModel / measModel, R
    and rng as particleMarginalSmootherLocalization takes them.  extras: the filter's outputs and `w_smooth`, `mean`, `cov`, `ess`,
    `mass` of the marginal smoother."""
    import warnings
    mp = _device_map(dynModel, measModel)
    if mp is not None and mp.transition is None:
        raise RBPFError(_ffi.RBPF_ERR_UNSUPPORTED, "particleTransitionStatisticsLocalization: " + _NO_BACKWARD_IN_DEVICE_MAP)
    if mp is None:
        mp = _recognise_map(dynModel, measModel)
    with LocalizationSession(mp, odometry, y, x0_nonLin, Q, N_P, dt, rng=rng, keep_history=True, trace=True) as s:
        s.advance(s.prob.N_T)
        fwd = s.finish(extras=extras)
        if fwd["first_degenerate_step"] >= 0:
            warnings.warn(f"Weights filter close to zero at t={fwd['first_degenerate_step'] + 1} !!!", RuntimeWarning, stacklevel=2)
        stats = ("S", "m", "pair_mass")
        out = s.transition_statistics(want=stats + (("w_smooth", "mean", "cov", "ess", "mass") if extras else ()))
    if extras:
        fwd.update({k: v for k, v in out.items() if k not in stats})
        return out["S"], out["m"], out["pair_mass"], fwd
    return out["S"], out["m"], out["pair_mass"]


def transition_noise_estimate(S, dt, m=None):
    """The M-step of EM for a transition noise of the form cov(dt, Q) = dt Q, from the statistics of
    LocalizationSession.transition_statistics, in plain numpy: S [n x n x P] (page t: the steps (t, t+1)), dt a scalar or [P] (or
    longer: the first P entries are read, the way the passes read dt) ->
        Q_hat = mean_t S_t / dt_t                                       (m None)
        (Q_hat, bias) = (mean_t (S_t - m_t m_t') / dt_t, mean_t m_t)    (m [n x P]: the centred form, and the mean smoothed
                                                                         residual: the odometry bias per step)
    For a DeviceTransition whose cov(dt, Q) is dt Q on the residual rows this is the maximiser of the expected complete-data
    likelihood under the smoothing weights of the current Q.  In a DenseMagMap it estimates the covariance per unit time of the
    residual [p~ - (p + dx); phi], of which the two diagonal 3 x 3 blocks mean something: the map's dynModel draws its noise with
    the ELEMENT-WISE sqrt(dt Q) of those two blocks of Q as factors S_pos and S_rot, so what it realises is S_pos S_pos' and
    S_rot S_rot', equal to dt Q for diagonal blocks only -- compare the estimate's blocks with those products over dt.  The
    off-diagonal block (position against orientation) is a diagnostic: the model has none."""
    S = np.asarray(S, dtype=np.float64)
    if S.ndim == 2:
        S = S[:, :, None]
    n, P = S.shape[0], S.shape[2]
    if S.shape[1] != n or P < 1:
        raise ValueError("S must be [n x n x P] with P >= 1")
    dt = np.atleast_1d(np.asarray(dt, dtype=np.float64)).ravel()
    dt = np.full(P, dt[0]) if dt.size == 1 else dt[:P]
    if dt.size != P or not np.all(dt > 0.0):
        raise ValueError("dt must be a positive scalar or hold one positive entry per page of S")
    if m is None:
        return np.mean(S / dt[None, None, :], axis=2)
    m = np.asarray(m, dtype=np.float64).reshape(n, -1)
    if m.shape[1] != P:
        raise ValueError("m must be [n x P]")
    return np.mean((S - m[:, None, :] * m[None, :, :]) / dt[None, None, :], axis=2), np.mean(m, axis=1)


def loc_forward_stats_workspace_bytes(N_P, N_T):
    """rbpf_loc_forward_stats_workspace_bytes (no device access): what the carry of the running statistics holds while it lives."""
    lib = load_library()
    nbytes = C.c_size_t(0)
    check(lib.rbpf_loc_forward_stats_workspace_bytes(int(N_P), int(N_T), C.byref(nbytes)))
    return int(nbytes.value)


def loc_forward_stats_step(xn, logw, xs_next, tau_S, tau_m, odo, dt, Q, reps=1):
    """rbpf_loc_forward_stats_step, the kernel-level probe: one step of the running two-slice statistics in the dense-mag map on the
    caller's arrays.  xn [7 x N], logw [N], xs_next [7 x M], odo [7], dt, Q as loc_marginal_step; tau_S [6 x 6 x N] (the lower
    triangle is read) and tau_m [6 x N] the incoming carry -> (D [M], tau_S_next [6 x 6 x M], tau_m_next [6 x M], reach [M] =
    sum_i omega(i, j), median ms of the normaliser pass, the carry pass, its merge and the reducer together)."""
    lib = load_library()
    xn = np.asfortranarray(np.asarray(xn, dtype=np.float64).reshape(7, -1))
    xs_next = np.asfortranarray(np.asarray(xs_next, dtype=np.float64).reshape(7, -1))
    N, M = xn.shape[1], xs_next.shape[1]
    logw = np.ascontiguousarray(np.asarray(logw, dtype=np.float64).ravel())
    odo = np.ascontiguousarray(np.asarray(odo, dtype=np.float64).ravel())
    Q = np.asfortranarray(np.asarray(Q, dtype=np.float64).reshape(6, 6))
    tau_S = np.asfortranarray(np.asarray(tau_S, dtype=np.float64).reshape(6, 6, -1))
    tau_m = np.asfortranarray(np.asarray(tau_m, dtype=np.float64).reshape(6, -1))
    if logw.size != N or odo.size != 7 or tau_S.shape[2] != N or tau_m.shape[1] != N:
        raise ValueError("logw must be [N], odo [7], tau_S [6 x 6 x N] and tau_m [6 x N]")
    D, tS, tm, reach = np.empty(M), np.empty((6, 6, M), order="F"), np.empty((6, M), order="F"), np.empty(M)
    ms = C.c_double(0.0)
    check(lib.rbpf_loc_forward_stats_step(N, M, _dp(xn), _dp(logw), _dp(xs_next), _dp(tau_S), _dp(tau_m), _dp(odo), float(dt), _dp(Q), _dp(D),
                                          _dp(tS), _dp(tm), _dp(reach), int(reps), C.byref(ms)))
    return D, tS, tm, reach, ms.value


def particleRunningStatisticsLocalization(dynModel, measModel, odometry, y, x0_nonLin, Q, R, N_P, dt, *, rng=None, every=1, extras=False):
    """The running two-slice statistics of localisation in a fixed map: the filter of particleFilterLocalization, and
    LocalizationSession.running_statistics folded in every `every` steps while it runs -> (S_run [n_res x n_res x (N_T-1)],
    m_run [n_res x (N_T-1)], mass_run [N_T-1][, extras]).  The pages do not depend on `every`.  dynModel / measModel, R and rng as
    particleTransitionStatisticsLocalization takes them.  extras: the filter's outputs and `tau_S`, `tau_m` of the last step."""
    import warnings
    mp = _device_map(dynModel, measModel)
    if mp is not None and mp.transition is None:
        raise RBPFError(_ffi.RBPF_ERR_UNSUPPORTED, "particleRunningStatisticsLocalization: " + _NO_BACKWARD_IN_DEVICE_MAP)
    if mp is None:
        mp = _recognise_map(dynModel, measModel)
    every = max(int(every), 1)
    with LocalizationSession(mp, odometry, y, x0_nonLin, Q, N_P, dt, rng=rng, keep_history=True, trace=True) as s:
        T = s.prob.N_T
        while s.tell() < T:
            s.advance(min(every, T - s.tell()))
            if 2 <= s.tell() < T:
                s.running_statistics(want=())
        fwd = s.finish(extras=extras)
        if fwd["first_degenerate_step"] >= 0:
            warnings.warn(f"Weights filter close to zero at t={fwd['first_degenerate_step'] + 1} !!!", RuntimeWarning, stacklevel=2)
        out = s.running_statistics(want=("S_run", "m_run", "mass_run") + (("tau_S", "tau_m") if extras else ()))
    if extras:
        fwd.update(tau_S=out["tau_S"], tau_m=out["tau_m"])
        return out["S_run"], out["m_run"], out["mass_run"], fwd
    return out["S_run"], out["m_run"], out["mass_run"]


def running_noise_estimate(S_run, m_run=None):
    """The running M-step for a transition noise of the form cov(dt, Q) = dt Q, from the pages of
    LocalizationSession.running_statistics, in plain numpy: S_run [n x n x P] (page k: the steps 0 .. k+1, already divided by dt
    step by step) ->
        Q_hat[:, :, k] = S_run[:, :, k] / (k + 1)                        (m_run None)
        (Q_hat, bias), bias[:, k] = m_run[:, k] / (k + 1)                (m_run [n x P]: the running smoothed odometry bias per step)
    Page k is what transition_noise_estimate would give (un-centred) on a run that ended at step k+1.  The caveat of
    transition_noise_estimate holds: in a DenseMagMap this estimates the covariance per unit time of the residual
    [p~ - (p + dx); phi], of which the two diagonal 3 x 3 blocks mean something -- the map's dynModel draws its noise with the
    ELEMENT-WISE sqrt(dt Q) of those blocks as factors S_pos and S_rot, so what it realises is S_pos S_pos' and S_rot S_rot', equal to
    dt Q for diagonal blocks only; the off-diagonal block is a diagnostic."""
    S = np.asarray(S_run, dtype=np.float64)
    if S.ndim == 2:
        S = S[:, :, None]
    n, P = S.shape[0], S.shape[2]
    if S.shape[1] != n or P < 1:
        raise ValueError("S_run must be [n x n x P] with P >= 1")
    k1 = np.arange(1, P + 1, dtype=np.float64)
    if m_run is None:
        return S / k1[None, None, :]
    m = np.asarray(m_run, dtype=np.float64).reshape(n, -1)
    if m.shape[1] != P:
        raise ValueError("m_run must be [n x P]")
    return S / k1[None, None, :], m / k1[None, :]


def loc_fixed_lag_workspace_bytes(N_P, N_T, lag, moments=1):
    """rbpf_loc_fixed_lag_workspace_bytes (no device access): what the carry of the fixed-lag smoother holds while it lives."""
    lib = load_library()
    nbytes = C.c_size_t(0)
    check(lib.rbpf_loc_fixed_lag_workspace_bytes(int(N_P), int(N_T), int(lag), int(moments), C.byref(nbytes)))
    return int(nbytes.value)


def loc_fixed_lag_step(xn, logw, xs_next, tau, odo, dt, Q, moments=1, reps=1):
    """rbpf_loc_fixed_lag_step, the kernel-level probe: one pass of the fixed-lag smoother in the dense-mag map on the caller's
    arrays.  xn [7 x N], logw [N], xs_next [7 x M], odo [7], dt, Q as loc_marginal_step; tau [K x N], any K >= 1, the incoming
    columns of the carry -> (D [M], tau_next [K x M], reach [M] = sum_i omega(i, j), median ms of the normaliser pass, the carry
    pass, its merge, the enter kernel (with `moments`) and the reducers together)."""
    lib = load_library()
    xn = np.asfortranarray(np.asarray(xn, dtype=np.float64).reshape(7, -1))
    xs_next = np.asfortranarray(np.asarray(xs_next, dtype=np.float64).reshape(7, -1))
    N, M = xn.shape[1], xs_next.shape[1]
    logw = np.ascontiguousarray(np.asarray(logw, dtype=np.float64).ravel())
    odo = np.ascontiguousarray(np.asarray(odo, dtype=np.float64).ravel())
    Q = np.asfortranarray(np.asarray(Q, dtype=np.float64).reshape(6, 6))
    tau = np.asarray(tau, dtype=np.float64)
    tau = np.ascontiguousarray(tau.reshape(1, -1) if tau.ndim == 1 else tau)
    K = tau.shape[0]
    if logw.size != N or odo.size != 7 or tau.shape != (K, N):
        raise ValueError("logw must be [N], odo [7] and tau [K x N]")
    D, tn, reach = np.empty(M), np.empty((K, M)), np.empty(M)
    ms = C.c_double(0.0)
    check(lib.rbpf_loc_fixed_lag_step(N, M, K, int(moments), _dp(xn), _dp(logw), _dp(xs_next), _dp(tau), _dp(odo), float(dt), _dp(Q), _dp(D),
                                      _dp(tn), _dp(reach), int(reps), C.byref(ms)))
    return D, tn, reach, ms.value


def particleFixedLagSmootherLocalization(dynModel, measModel, odometry, y, x0_nonLin, Q, R, N_P, dt, lag, *, rng=None, every=1, extras=False):
    """The fixed-lag smoother of localisation in a fixed map: the filter of particleFilterLocalization, and
    LocalizationSession.fixed_lag_estimates folded in every `every` steps while it runs -> (mean [n x N_T], cov [n x n x N_T],
    lag_of [N_T][, extras]); column s is E[x_s | y_{0:min(s+lag, N_T-1)}] and its covariance.  The estimates do not depend on
    `every`.  dynModel / measModel, R and rng as particleRunningStatisticsLocalization takes them.  extras: the filter's outputs and
    `by_lag`, `mass`."""
    import warnings
    mp = _device_map(dynModel, measModel)
    if mp is not None and mp.transition is None:
        raise RBPFError(_ffi.RBPF_ERR_UNSUPPORTED, "particleFixedLagSmootherLocalization: " + _NO_BACKWARD_IN_DEVICE_MAP)
    if mp is None:
        mp = _recognise_map(dynModel, measModel)
    every = max(int(every), 1)
    with LocalizationSession(mp, odometry, y, x0_nonLin, Q, N_P, dt, rng=rng, keep_history=True, trace=True) as s:
        T = s.prob.N_T
        while s.tell() < T:
            s.advance(min(every, T - s.tell()))
            if 2 <= s.tell() < T:
                s.fixed_lag_estimates(lag, want=("cov",))
        fwd = s.finish(extras=extras)
        if fwd["first_degenerate_step"] >= 0:
            warnings.warn(f"Weights filter close to zero at t={fwd['first_degenerate_step'] + 1} !!!", RuntimeWarning, stacklevel=2)
        out = s.fixed_lag_estimates(lag, want=("mean", "cov", "lag_of") + (("by_lag", "mass") if extras else ()))
    if extras:
        fwd.update(by_lag=out["by_lag"], mass=out["mass"])
        return out["mean"], out["cov"], out["lag_of"], fwd
    return out["mean"], out["cov"], out["lag_of"]


def loc_backward_workspace_bytes(N_P, N_T, n_traj):
    """rbpf_loc_backward_workspace_bytes (no device access)."""
    lib = load_library()
    nbytes = C.c_size_t(0)
    check(lib.rbpf_loc_backward_workspace_bytes(int(N_P), int(N_T), int(n_traj), C.byref(nbytes)))
    return int(nbytes.value)


def loc_backward_step(xn, w, xs_next, odo, dt, Q, u, want_logp=False, reps=1):
    """rbpf_loc_backward_step, the kernel-level probe: one backward step on the caller's arrays.  xn [7 x N], w [N],
    xs_next [7 x M], odo [7], Q [6 x 6], u [M] -> (index [M], logp [N x M] or None, median ms of one step)."""
    lib = load_library()
    xn = np.asfortranarray(np.asarray(xn, dtype=np.float64).reshape(7, -1))
    xs_next = np.asfortranarray(np.asarray(xs_next, dtype=np.float64).reshape(7, -1))
    N, M = xn.shape[1], xs_next.shape[1]
    w = np.ascontiguousarray(np.asarray(w, dtype=np.float64).ravel())
    u = np.ascontiguousarray(np.asarray(u, dtype=np.float64).ravel())
    odo = np.ascontiguousarray(np.asarray(odo, dtype=np.float64).ravel())
    Q = np.asfortranarray(np.asarray(Q, dtype=np.float64).reshape(6, 6))
    if w.size != N or u.size != M or odo.size != 7:
        raise ValueError("w must be [N], u [M] and odo [7]")
    index = np.zeros(M, dtype=np.int32)
    logp = np.empty((N, M), order="F") if want_logp else None
    ms = C.c_double(0.0)
    check(lib.rbpf_loc_backward_step(N, M, _dp(xn), _dp(w), _dp(xs_next), _dp(odo), float(dt), _dp(Q), _dp(u), _ip(index),
                                     _dp(logp) if want_logp else None, int(reps), C.byref(ms)))
    return index, logp, ms.value


# What tools/loc_reject_bench.py measured on an MI355X at N = M = 65 536 in the dense-mag map (profiles/loc_reject_bench.json): the
# all-pairs step over one round of tries of a run whose every try is rejected.  None: not measured, max_tries is then mandatory.
REJECT_R_STAR = 5183.0                         # t_pass = 20.65 ms over t_try = 3.98 us
REJECT_R_STAR_SIZE = 65536


def reject_default_max_tries(N_P, n_traj, r_star=None):
    """max_tries of method="rejection" where the caller gives none.  A trajectory should never spend more on tries than its fallback
    costs: at N_P = n_traj = 65 536 that is R* = t_pass / t_try tries, and the default there is the largest power of two not above
    R*.  A round of tries is paced by the latency of its dependent loads and costs the same at every size, while the all-pairs step
    grows with N_P x n_traj, so below that size the bound is scaled by N_P n_traj / 65 536^2 (0: every trajectory goes to the
    all-pairs pass); above it the measured value stands."""
    r_star = REJECT_R_STAR if r_star is None else r_star
    if r_star is None:
        raise ValueError("method='rejection' has no measured default for max_tries on this build (tools/loc_reject_bench.py has not run): "
                         "pass max_tries explicitly")
    r = float(r_star) * min(1.0, float(N_P) * float(n_traj) / float(REJECT_R_STAR_SIZE) ** 2)
    return 0 if r < 1.0 else int(2 ** int(np.floor(np.log2(r))))


def loc_backward_reject_workspace_bytes(N_P, N_T, n_traj):
    """rbpf_loc_backward_reject_workspace_bytes (no device access)."""
    lib = load_library()
    nbytes = C.c_size_t(0)
    check(lib.rbpf_loc_backward_reject_workspace_bytes(int(N_P), int(N_T), int(n_traj), C.byref(nbytes)))
    return int(nbytes.value)


def _reject_uniforms(u_try, M):
    """u_try [R x M x 2] (C order: try, trajectory, (u0, u1)) -> (the contiguous array, R); an int R: (None, R), the device
    generator's draws of seed 0 at step 0 (timing runs)."""
    if isinstance(u_try, (int, np.integer)):
        if u_try < 0:
            raise ValueError("max_tries must be >= 0")
        return None, int(u_try)
    u_try = np.ascontiguousarray(np.asarray(u_try, dtype=np.float64))
    if u_try.size == 0:
        return None, 0
    if u_try.ndim != 3 or u_try.shape[1:] != (M, 2):
        raise ValueError(f"u_try must be [R x {M} x 2]")
    return u_try, u_try.shape[0]


def loc_backward_reject_step(xn, w, xs_next, odo, dt, Q, u_try, u, reps=1):
    """rbpf_loc_backward_reject_step, the kernel-level probe: one step of backward simulation by rejection sampling on the caller's
    arrays.  xn [7 x N], w [N], xs_next [7 x M], odo [7], Q [6 x 6] as loc_backward_step; u_try [R x M x 2]: the uniforms (u0, u1) of
    try r of trajectory j, R = max_tries (R = 0: an empty array; an int R: the device generator's draws, for timing); u [M]: the
    fallback's uniforms -> (index [M], accepted_at [M]: the try that was accepted or -1 for a trajectory the all-pairs pass drew,
    median ms of one step)."""
    lib = load_library()
    xn = np.asfortranarray(np.asarray(xn, dtype=np.float64).reshape(7, -1))
    xs_next = np.asfortranarray(np.asarray(xs_next, dtype=np.float64).reshape(7, -1))
    N, M = xn.shape[1], xs_next.shape[1]
    w = np.ascontiguousarray(np.asarray(w, dtype=np.float64).ravel())
    u = np.ascontiguousarray(np.asarray(u, dtype=np.float64).ravel())
    odo = np.ascontiguousarray(np.asarray(odo, dtype=np.float64).ravel())
    Q = np.asfortranarray(np.asarray(Q, dtype=np.float64).reshape(6, 6))
    if w.size != N or u.size != M or odo.size != 7:
        raise ValueError("w must be [N], u [M] and odo [7]")
    u_try, R = _reject_uniforms(u_try, M)
    index, acc = np.zeros(M, dtype=np.int32), np.zeros(M, dtype=np.int32)
    ms = C.c_double(0.0)
    check(lib.rbpf_loc_backward_reject_step(N, M, _dp(xn), _dp(w), _dp(xs_next), _dp(odo), float(dt), _dp(Q), _dp(u_try) if u_try is not None else None, _dp(u),
                                            R, _ip(index), _ip(acc), int(reps), C.byref(ms)))
    return index, acc, ms.value


def particleSmootherLocalization(dynModel, measModel, odometry, y, x0_nonLin, Q, R, N_P, N_S, dt, *, rng=None, extras=False, method="all_pairs",
                                 max_tries=None):
    """Forward filter, backward simulation for localisation in a fixed map: particleFilterLocalization, then N_S trajectories drawn
    backwards through its particles -> (xs_traj [7 x N_S x N_T], traj_smooth_mean [7 x N_T][, extras]).  dynModel / measModel are
    the handles of a DenseMagMap, R is accepted and not used, as there; or a DeviceMap with a DeviceTransition as dynModel (measModel
    None): n_nonlin rows in place of 7.  rng: PhiloxRNG (one seed keys the filter's and the
    backward draws, on disjoint counters) or ReplayRNG(U, Z, Uback=u) with the backward uniforms u [N_T x N_S].
    extras: the filter's outputs (traj_max, traj_mean, first_degenerate_step, ...) and the drawn `index` [N_S x N_T].
    method, max_tries: as LocalizationSession.backward_simulate; method="rejection" takes a PhiloxRNG or None, and extras then hold
    n_fallback and n_tries [N_T] too."""
    import warnings
    if method not in ("all_pairs", "rejection"):
        raise ValueError(f"unknown method {method!r}: 'all_pairs' or 'rejection'")
    if method == "rejection" and isinstance(rng, ReplayRNG):
        raise ValueError("method='rejection' draws its tries on the device: rng must be None or a PhiloxRNG; uniforms are replayed by the "
                         "probes loc_backward_reject_step and device_map_backward_reject_step")
    mp = _device_map(dynModel, measModel)
    if mp is not None and mp.transition is None:
        raise RBPFError(_ffi.RBPF_ERR_UNSUPPORTED, "particleSmootherLocalization: " + _NO_BACKWARD_IN_DEVICE_MAP)
    if mp is None:
        mp = _recognise_map(dynModel, measModel)
    if isinstance(rng, ReplayRNG):
        if rng.Uback is None:
            raise ValueError("a ReplayRNG needs Uback [N_T x N_S] to replay the backward draws")
        back = rng.Uback
    else:
        back = rng
    with LocalizationSession(mp, odometry, y, x0_nonLin, Q, N_P, dt, rng=rng, keep_history=True, trace=True) as s:
        s.advance(s.prob.N_T)
        fwd = s.finish(extras=extras)
        if fwd["first_degenerate_step"] >= 0:
            warnings.warn(f"Weights filter close to zero at t={fwd['first_degenerate_step'] + 1} !!!", RuntimeWarning, stacklevel=2)
        if method == "rejection":
            out = s.backward_simulate(N_S, rng=back, want=("xs_traj", "index", "traj_smooth_mean", "n_fallback", "n_tries"), method=method,
                                      max_tries=max_tries)
        else:
            out = s.backward_simulate(N_S, rng=back, max_tries=max_tries)
    if extras:
        if method == "rejection":
            fwd["n_fallback"], fwd["n_tries"] = out["n_fallback"], out["n_tries"]
        fwd["index"] = out["index"]
        return out["xs_traj"], out["traj_smooth_mean"], fwd
    return out["xs_traj"], out["traj_smooth_mean"]
