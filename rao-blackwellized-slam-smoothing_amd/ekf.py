"""EKF comparison baseline of examples/slam-dense-mag (ekf_dense.m:41-102 with the closures measModel_ekf / dynModel_ekf
of run_dense3D_magfield.m:281-299,310-316) -- SURVEY 8 (f3).

One Gaussian state [position(3); orientation deviation(3); map(m+3)], serial in time, so the recursion stays on the
host (numpy); the two pieces that touch the reduced-rank basis run through the device helper kernels of the C ABI:
the rotated basis gradient `Rnb' * dPhi` (rbpf_meas_model) and the basis Hessian (rbpf_jacobian_phi3d).

`ekf_dense_device` / `ekf_dense_batch` run the same recursion on the device (rbpf_ekf_dense, csrc/rbpf_ekf.hip): two kernels
per time step, batched over independent runs -- the 80 runs of the Monte-Carlo protocol (main.m:37-57) are one call."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import RBPFError, RBPF_ERR_CHOL_FAILED, check, load_library


def _qleft(q):
    q0, q1, q2, q3 = q
    return np.array([[q0, -q1, -q2, -q3], [q1, q0, -q3, q2], [q2, q3, q0, -q1], [q3, -q2, q1, q0]])     # tools/qLeft.m:30-35


def _expq(phi):
    mag = float(np.sqrt(phi @ phi))                                          # tools/expq.m:22-31
    den = mag + (1.0 if mag == 0.0 else 0.0)
    eq = np.concatenate(([np.cos(mag)], phi / den * np.sin(mag)))
    return -eq if eq[0] < 0 else eq


def _quat2rmat(q):
    q0, q1, q2, q3 = q                                                       # tools/quat2rmat.m:27-33
    return np.array([[q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, 2 * q1 * q2 - 2 * q0 * q3, 2 * q1 * q3 + 2 * q0 * q2],
                     [2 * q1 * q2 + 2 * q0 * q3, q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3, 2 * q2 * q3 - 2 * q0 * q1],
                     [2 * q1 * q3 - 2 * q0 * q2, 2 * q2 * q3 + 2 * q0 * q1, q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3]])


def _mcross(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])                         # tools/mcross.m:33-37


def _chol_jitter(SS, jitter):
    try:
        return np.linalg.cholesky(SS)
    except np.linalg.LinAlgError:
        try:
            return np.linalg.cholesky(SS + jitter * np.eye(SS.shape[0]))                                 # ekf_dense.m:84-86
        except np.linalg.LinAlgError as exc:
            raise RBPFError(RBPF_ERR_CHOL_FAILED, "matrix must be positive definite") from exc


def measModel_ekf(model, LL, x, q):
    """run_dense3D_magfield.m:281-299 -> (yhat [3], dy [3 x (6 + nLin)])."""
    LL = np.asarray(LL, dtype=np.float64)
    xn = np.concatenate((x[0:3], q))
    RtdPhi = model.measModel(xn)[0]                                          # Rnb' * dPhi  [3 x nLin]  (device)
    Rnb = _quat2rmat(q)
    yhat = RtdPhi @ x[6:]                                                    # :290
    J = model.JacobianPhi3D(x[0:3], LL[0], LL[1])[:, :, :, 0]                # [3 x 3 x m]  (device), :292-294
    J3 = np.tensordot(J, x[9:], axes=([2], [0]))
    dy = np.zeros((3, RtdPhi.shape[1] + 6))
    dy[:, 0:3] = Rnb.T @ J3                                                  # :296
    dy[:, 3:6] = Rnb.T @ _mcross(Rnb @ yhat)                                 # :297  (dPhi*x(7:end) = Rnb * yhat)
    dy[:, 6:] = RtdPhi                                                       # :298
    return yhat, dy


def ekf_dense(model, LL, odometry, y, x0, q0, P0, Q, R, dt):
    """ekf_dense.m:41-102 for a DenseMagModel family object -> (xf_traj, qnb_traj, Pf_traj)."""
    y = np.atleast_2d(np.asarray(y, dtype=np.float64))
    odometry = np.atleast_2d(np.asarray(odometry, dtype=np.float64))
    xf = np.asarray(x0, dtype=np.float64).ravel().copy()
    Pf = np.asarray(P0, dtype=np.float64).copy()
    q_nb = np.asarray(q0, dtype=np.float64).ravel().copy()
    R = np.atleast_2d(np.asarray(R, dtype=np.float64))
    nS, N_T = xf.size, y.shape[0]
    Q = np.asarray(Q, dtype=np.float64)
    Qp = Q if Q.ndim == 3 else np.repeat(Q[:, :, None], max(N_T - 1, 1), axis=2)                         # :47-49
    dtv = np.atleast_1d(np.asarray(dt, dtype=np.float64)).ravel()
    if dtv.size == 1:
        dtv = dtv[0] * np.ones(max(N_T - 1, 1))                                                          # :52-54
    xf_traj, Pf_traj, qnb_traj = np.full((nS, N_T), np.nan), np.full((nS, nS, N_T), np.nan), np.full((4, N_T), np.nan)
    xp, Pp = xf, Pf
    for t in range(N_T):
        if t != 0:                                                           # :69-74 with dynModel_ekf :310-316
            dx = odometry[t - 1, :]
            xp = xf.copy()
            xp[0:3] = xf[0:3] + dx[0:3]
            q_nb = _qleft(q_nb) @ dx[3:7]
            G = np.zeros((nS, 6))
            G[0:3, 0:3] = np.eye(3)
            G[3:6, 3:6] = _quat2rmat(q_nb)
            Pp = Pf + G @ (dtv[t - 1] * Qp[:, :, t - 1]) @ G.T               # F = I
        yhat, dy = measModel_ekf(model, LL, xp, q_nb)                        # :78
        e = y[t, :] - yhat
        SS = dy @ Pp @ dy.T + R
        cS = _chol_jitter(SS, 1e-3)
        Mx = np.linalg.solve(cS, dy).T
        Mx = np.linalg.solve(cS.T, Mx.T).T
        K = Pp @ Mx                                                          # :87
        xf = xp + K @ e
        Pf = Pp - K @ SS @ K.T
        Pf = 0.5 * (Pf + Pf.T)                                               # :92
        q_nb = _qleft(_expq(xf[3:6] / 2.0)) @ q_nb                           # :95
        xf[3:6] = 0.0
        xf_traj[:, t], Pf_traj[:, :, t], qnb_traj[:, t] = xf, Pf, q_nb
    return xf_traj, qnb_traj, Pf_traj


def _dp(a):
    return a.ctypes.data_as(_ffi.c_double_p)


def ekf_dense_batch(models, LLs, odometry, y, x0, q0, P0, Q, R, dt, keep_P=False):
    """B independent runs of ekf_dense.m:41-102 in one device call (rbpf_ekf_dense).  `models`: B DenseMagModel objects of one
    basis size (the same object may repeat); LLs [B x 2 x 3], odometry [B x N_T-1 x 7], y [B x N_T x 3], x0 [B x n], q0 [B x 4],
    P0 [B x n x n] (symmetric), R [B x 3 x 3] or one [3 x 3] for all; Q [6 x 6] or [6 x 6 x N_T-1] and dt (scalar or vector)
    are shared.  -> (xf_traj [B x n x N_T], qnb_traj [B x 4 x N_T], Pf [B x n x n], or Pf_traj [B x n x n x N_T] with keep_P).
    A run's results are bit-identical alone and at any position of a batch."""
    lib = load_library()
    models = list(models)
    B = len(models)
    y = np.asarray(y, dtype=np.float64)
    if B < 1 or y.ndim != 3 or y.shape[0] != B or y.shape[2] != 3:
        raise ValueError("y must be [B x N_T x 3] with one model per run")
    N_T = y.shape[1]
    To = max(N_T - 1, 1)
    odo = np.zeros((B, 7, To))                                               # per run [To x 7] column-major
    if N_T > 1:
        odometry = np.asarray(odometry, dtype=np.float64).reshape(B, -1, 7)
        if odometry.shape[1] < N_T - 1:
            raise ValueError("odometry must be [B x >= N_T-1 x 7]")
        odo[:, :, :N_T - 1] = np.transpose(odometry[:, :N_T - 1, :], (0, 2, 1))
    yy = np.ascontiguousarray(np.transpose(y, (0, 2, 1)))
    x0 = np.ascontiguousarray(np.asarray(x0, dtype=np.float64).reshape(B, -1))
    n = x0.shape[1]
    q0 = np.ascontiguousarray(np.asarray(q0, dtype=np.float64).reshape(B, 4))
    P0 = np.ascontiguousarray(np.transpose(np.asarray(P0, dtype=np.float64).reshape(B, n, n), (0, 2, 1)))
    R = np.asarray(R, dtype=np.float64)
    R = np.ascontiguousarray(np.transpose(np.broadcast_to(R, (B, 3, 3)), (0, 2, 1)))
    LL = np.ascontiguousarray(np.transpose(np.asarray(LLs, dtype=np.float64).reshape(B, 2, 3), (0, 2, 1)))
    Q = np.asarray(Q, dtype=np.float64)
    Qp = np.ascontiguousarray(np.transpose(Q.reshape(6, 6, -1), (2, 1, 0)))   # pages of [6 x 6] column-major
    dtv = np.ascontiguousarray(np.atleast_1d(np.asarray(dt, dtype=np.float64)).ravel())
    by_id = {}                                                               # a model object that repeats is one descriptor
    for mdl in models:
        if id(mdl) not in by_id:
            by_id[id(mdl)] = mdl.descriptor() if hasattr(mdl, "descriptor") else mdl
    descs = [by_id[id(mdl)] for mdl in models]
    for mdl, d in zip(models, descs):
        if not isinstance(d, _ffi.rbpf_model):
            raise TypeError(f"{type(mdl).__name__} is not a model family object")
    if descs[0].kind == _ffi.RBPF_MODEL_DENSE_MAG_6D and n != descs[0].m_basis + 9:    # the library sizes every array by models[0]
        raise ValueError(f"x0 has {n} states, the first model has {descs[0].m_basis + 9}")
    ptrs = (C.POINTER(_ffi.rbpf_model) * B)(*[C.pointer(d) for d in descs])
    prob = _ffi.rbpf_ekf_problem(n_runs=B, N_T=N_T, q_pages=Qp.shape[0], dt_len=dtv.size, odo_ld=To, keep_P=1 if keep_P else 0)
    prob.struct_size = C.sizeof(_ffi.rbpf_ekf_problem)
    prob.models = ptrs
    prob.odometry, prob.y, prob.x0, prob.q0, prob.P0 = _dp(odo), _dp(yy), _dp(x0), _dp(q0), _dp(P0)
    prob.R, prob.LL, prob.Q, prob.dt = _dp(R), _dp(LL), _dp(Qp), _dp(dtv)
    xf = np.empty((B, N_T, n))
    qnb = np.empty((B, N_T, 4))
    Pf = np.empty((B, N_T, n, n) if keep_P else (B, n, n))
    out = _ffi.rbpf_ekf_out(xf_traj=_dp(xf), qnb_traj=_dp(qnb), Pf=_dp(Pf))
    out.struct_size = C.sizeof(_ffi.rbpf_ekf_out)
    check(lib.rbpf_ekf_dense(C.byref(prob), None, C.byref(out)))
    Pf = np.transpose(Pf, (0, 3, 2, 1)) if keep_P else np.transpose(Pf, (0, 2, 1))
    return np.transpose(xf, (0, 2, 1)), np.transpose(qnb, (0, 2, 1)), Pf


def ekf_workspace_bytes(model, n_runs, N_T, keep_P=False):
    """Device bytes an `ekf_dense_batch` call of that shape needs (rbpf_ekf_workspace_bytes; no device access)."""
    lib = load_library()
    d = model.descriptor()
    ptrs = (C.POINTER(_ffi.rbpf_model) * n_runs)(*[C.pointer(d)] * n_runs)
    one = np.zeros(36)
    prob = _ffi.rbpf_ekf_problem(n_runs=n_runs, N_T=N_T, q_pages=1, dt_len=1, odo_ld=max(N_T - 1, 1), keep_P=1 if keep_P else 0)
    prob.struct_size = C.sizeof(_ffi.rbpf_ekf_problem)
    prob.models = ptrs
    for f in ("odometry", "y", "x0", "q0", "P0", "R", "LL", "Q", "dt"):
        setattr(prob, f, _dp(one))                                           # only their presence is checked
    nbytes = C.c_size_t(0)
    check(lib.rbpf_ekf_workspace_bytes(C.byref(prob), None, C.byref(nbytes)))
    return int(nbytes.value)


def ekf_dense_device(model, LL, odometry, y, x0, q0, P0, Q, R, dt, keep_P=True):
    """`ekf_dense` on the device: same arguments, same (xf_traj, qnb_traj, Pf_traj); with keep_P=False the third element is the
    final covariance [n x n] only (at the metric's horizon the history is n^2 N_T doubles)."""
    y = np.atleast_2d(np.asarray(y, dtype=np.float64))
    odometry = np.atleast_2d(np.asarray(odometry, dtype=np.float64))
    xf, qnb, Pf = ekf_dense_batch([model], np.asarray(LL, dtype=np.float64)[None], odometry[None], y[None],
                                  np.asarray(x0, dtype=np.float64).ravel()[None], np.asarray(q0, dtype=np.float64).ravel()[None],
                                  np.asarray(P0, dtype=np.float64)[None], Q, np.atleast_2d(np.asarray(R, dtype=np.float64)), dt, keep_P=keep_P)
    return xf[0], qnb[0], Pf[0]
