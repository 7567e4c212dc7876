"""Checker of the localisation filter: a restatement of examples/mag-localization-mapping/particleFilterLocalization.m:51-132
and of the two closures of run_localization.m (measModel :241-272, dynModel :274-281, batch map :134-151), on top of the oracle's
primitives (oracle/rbpf_oracle.py).  Randomness is injected in the reference's call order: U[t-1, i] is the `rand` of
`ai(i) = sample(w)` (:93), Z[t-1, i, :] the six `randn` of dynModel for slot i (:277 position, :279 orientation).

`dtype=np.longdouble` runs the same statements in extended precision on the same fp64 inputs (the oracle's primitives are fp64
only, so that mode uses the dtype-generic twins below; tests/test_localization_cpu.py checks the twins against the primitives
bit for bit in fp64).  That makes the restatement its own arbiter: |fp64 - long double| is the reference's own rounding error.

Nothing in the package imports this file.
"""
import math

import numpy as np

import rbpf_oracle as O


# ---- dtype-generic twins of the oracle's primitives (same expressions, same order) -------------------------------------------
def _eigenfun_dx(NN, x, di, L, dtype):
    NN = np.asarray(NN, dtype=dtype)
    x = np.asarray(x, dtype=dtype)
    L = np.asarray(L, dtype=dtype)
    pi = dtype(np.pi)
    v = np.ones((x.shape[0], NN.shape[0]), dtype=dtype)
    for j in range(NN.shape[1]):
        arg = pi * NN[None, :, j] * (x[:, j:j + 1] + L[j]) / (dtype(2.0) * L[j])
        if j == di:
            v = v * pi * NN[None, :, j] / (dtype(2.0) * L[j] * np.sqrt(L[j])) * np.cos(arg)
        else:
            v = v * dtype(1.0) / np.sqrt(L[j]) * np.sin(arg)
    return v


def _quat2rmat(q):
    q0, q1, q2, q3 = q
    return np.array([
        [q0 ** 2 + q1 ** 2 - q2 ** 2 - q3 ** 2, 2 * q1 * q2 - 2 * q0 * q3, 2 * q1 * q3 + 2 * q0 * q2],
        [2 * q1 * q2 + 2 * q0 * q3, q0 ** 2 - q1 ** 2 + q2 ** 2 - q3 ** 2, 2 * q2 * q3 - 2 * q0 * q1],
        [2 * q1 * q3 - 2 * q0 * q2, 2 * q2 * q3 + 2 * q0 * q1, q0 ** 2 - q1 ** 2 - q2 ** 2 + q3 ** 2]], dtype=q.dtype)


def _mcross(v):
    z = v.dtype.type(0.0)
    return np.array([[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]], dtype=v.dtype)


def _qLeft(q):
    M = np.empty((4, 4), dtype=q.dtype)
    M[0, 0] = q[0]
    M[0, 1:] = -q[1:4]
    M[1:, 0] = q[1:4]
    M[1:, 1:] = q[0] * np.eye(3, dtype=q.dtype) + _mcross(q[1:4])
    return M


def _qRight(q):
    M = np.empty((4, 4), dtype=q.dtype)
    M[0, 0] = q[0]
    M[0, 1:] = -q[1:4]
    M[1:, 0] = q[1:4]
    M[1:, 1:] = q[0] * np.eye(3, dtype=q.dtype) - _mcross(q[1:4])
    return M


def _expq(phi):
    mag = np.sqrt(phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2])
    nphi = phi / (mag + (phi.dtype.type(1.0) if mag == 0 else phi.dtype.type(0.0)))
    eq = np.concatenate(([np.cos(mag)], nphi * np.sin(mag))).astype(phi.dtype)
    return -eq if eq[0] < 0 else eq


def _sample(w, u):
    return int(np.sum(np.cumsum(w) < u))


def _prims(dtype):
    """(eigenfun_dx, quat2rmat, qLeft, qRight, expq, sample): the oracle's own in fp64, the twins otherwise."""
    if dtype is np.float64:
        return (lambda NN, x, di, L: O.eigenfun_dx(NN, x, di, L)), O.quat2rmat, O.qLeft, O.qRight, O.expq, O.sample
    return (lambda NN, x, di, L: _eigenfun_dx(NN, x, di, L, dtype)), _quat2rmat, _qLeft, _qRight, _expq, _sample


# ---- the map -----------------------------------------------------------------------------------------------------------------
def grad_rows(NN, L, pos, dtype=np.float64):
    """dPhix, dPhiy, dPhiz of run_localization.m:245-250 (= :135-142): [N x (m + 3)] each."""
    efdx = _prims(dtype)[0]
    pos = np.asarray(pos, dtype=dtype).reshape(-1, 3)
    N = pos.shape[0]
    rows = []
    for c in range(3):
        lin = np.zeros((N, 3), dtype=dtype)
        lin[:, c] = 1
        rows.append(np.hstack((lin, np.asarray(efdx(NN, pos, c, L), dtype=dtype))))
    return rows


def prior_k(NN, L, theta):
    """run_localization.m:119-132."""
    linSigma2, lengthScale, magnSigma2, _ = (float(t) for t in theta)
    lam = O.eigenval(np.asarray(NN, dtype=np.float64), np.asarray(L, dtype=np.float64))
    Sse = magnSigma2 * math.sqrt(2 * math.pi) ** 3 * lengthScale ** 3 * np.exp(-lam * lengthScale ** 2 / 2)
    return np.concatenate(([linSigma2] * 3, Sse))


def map_from_data(NN, L, x, y, theta):
    """run_localization.m:134-151 -> (foo, Lc, V) with V = sqrt(sigma2) inv(Lc): dVarft(g) = sigma2 |Lc \\ g|^2 = |V g|^2 (:261)."""
    sigma2 = float(theta[3])
    k = prior_k(NN, L, theta)
    Phi = np.vstack(grad_rows(NN, L, x))
    Phiy = Phi.T @ np.asarray(y, dtype=np.float64).reshape(-1, order="F")
    Lc = np.linalg.cholesky(Phi.T @ Phi + np.diag(sigma2 / k))
    foo = np.linalg.solve(Lc.T, np.linalg.solve(Lc, Phiy))
    V = np.tril(math.sqrt(sigma2) * np.linalg.inv(Lc))
    return foo, Lc, V


def predict(NN, L, mean, pos, V=None, P=None, dtype=np.float64):
    """dEft [N x 3] (:260) and the predictive variances [N x 3] at `pos` (:261-263 evaluated there): |V g|^2, or g' P g when the
    covariance itself is given."""
    rows = grad_rows(NN, L, pos, dtype)
    mean = np.asarray(mean, dtype=dtype)
    dE = np.column_stack([r @ mean for r in rows])
    var = None
    if V is not None:
        Vt = np.asarray(V, dtype=dtype).T
        var = np.column_stack([np.sum((r @ Vt) ** 2, axis=1) for r in rows])
    elif P is not None:
        Pd = np.asarray(P, dtype=dtype)
        var = np.column_stack([np.sum((r @ Pd) * r, axis=1) for r in rows])
    return dE, var


# ---- the closures ------------------------------------------------------------------------------------------------------------
def dyn_model(xn, dx, dt, Q, z, dtype=np.float64):
    """run_localization.m:274-281; z = the six randn values in call order.  sqrt is element-wise."""
    _, _, qLeft, qRight, expq, _ = _prims(dtype)
    xn = np.asarray(xn, dtype=dtype).ravel()
    dx = np.asarray(dx, dtype=dtype).ravel()
    Q = np.asarray(Q, dtype=dtype)
    z = np.asarray(z, dtype=dtype).ravel()
    dt = dtype(dt)
    pos = xn[0:3] + dx[0:3] + np.sqrt(dt * Q[0:3, 0:3]) @ z[0:3]                              # :277
    e = np.asarray(expq(np.sqrt(dt * Q[3:6, 3:6]) @ z[3:6]), dtype=dtype)
    quat = np.asarray(qLeft(np.asarray(qRight(xn[3:7]), dtype=dtype) @ dx[3:7]), dtype=dtype) @ e          # :278-279
    return np.concatenate((pos, quat))


def meas_model(yt, xn, dE, var, sigma2, dtype=np.float64):
    """run_localization.m:265-271: w(i) = sum(normpdf(yt, (Rnb_i' dEft(i,:)')', sqrt(dVarft(i,:) + sigma2)))."""
    quat2rmat = _prims(dtype)[1]
    yt = np.asarray(yt, dtype=dtype).ravel()
    N = xn.shape[1]
    w = np.empty(N, dtype=dtype)
    s2pi = np.sqrt(dtype(2.0) * dtype(np.pi))
    for i in range(N):
        Rnb = np.asarray(quat2rmat(xn[3:7, i]), dtype=dtype)
        mu = Rnb.T @ dE[i, :]
        s = np.sqrt(var[i, :] + dtype(sigma2))
        w[i] = np.sum(np.exp(-dtype(0.5) * ((yt - mu) / s) ** 2) / (s * s2pi))
    return w


# ---- the estimator -----------------------------------------------------------------------------------------------------------
def particleFilterLocalization(NN, L, mean, sigma2, odometry, y, x0_nonLin, Q, N_P, dt, U, Z, V=None, P=None, var_points=None,
                               dtype=np.float64):
    """particleFilterLocalization.m:51-132.  var_points=None: variances at the particles (the evident intent); an array of
    points: the reference's literal reading (run_localization.m:261-263: variances at those points, indexed by the slot).
    Returns dict(traj_max, traj_mean [7 x N_T], ai [N_T x N_P] 0-based, w [N_T x N_P], log_sum_w [N_T], xn_traj [7 x N_P x N_T],
    degenerate [N_T] bool)."""
    sample = _prims(dtype)[5]
    y = np.asarray(y, dtype=np.float64)
    N_T = y.shape[0]
    odometry = np.asarray(odometry, dtype=np.float64)
    x0 = np.asarray(x0_nonLin, dtype=dtype)
    w = np.full(N_P, dtype(1.0) / dtype(N_P), dtype=dtype)                                   # :52
    xn = x0.reshape(7, -1).copy() if x0.ndim > 1 and x0.shape[1] > 1 else np.repeat(x0.reshape(7, 1), N_P, axis=1)   # :55-59
    Q = np.asarray(Q, dtype=np.float64)
    if Q.ndim == 2:
        Q = np.repeat(Q[:, :, None], N_T, axis=2)                                              # :66-68
    dt = np.atleast_1d(np.asarray(dt, dtype=np.float64)).ravel()
    if dt.size == 1:
        dt = dt[0] * np.ones(N_T)                                                              # :71-73
    traj_max = np.full((7, N_T), np.nan, dtype=dtype)
    traj_mean = np.full((7, N_T), np.nan, dtype=dtype)
    xn_traj = np.zeros((7, N_P, N_T), dtype=dtype)
    xn_traj[:, :, 0] = xn
    AI = np.zeros((N_T, N_P), dtype=np.int64)
    W = np.zeros((N_T, N_P), dtype=dtype)
    lsw = np.zeros(N_T, dtype=dtype)
    degenerate = np.zeros(N_T, dtype=bool)
    var_tab = None
    if var_points is not None:
        var_tab = predict(NN, L, mean, np.asarray(var_points)[:, 0:3], V=V, P=P, dtype=dtype)[1]
    for t in range(N_T):
        xn_ = xn.copy()                                                                        # :87
        if t != 0:
            ai = np.zeros(N_P, dtype=np.int64)
            for i in range(N_P):
                ai[i] = sample(w, U[t - 1, i])                                                 # :93
                xn[:, i] = dyn_model(xn_[:, ai[i]], odometry[t - 1, :], dt[t - 1], Q[:, :, t - 1], Z[t - 1, i, :], dtype)   # :95
            AI[t] = ai
            xn_traj[:, :, t] = xn                                                              # :102
            xn_traj[:, :, :t] = xn_traj[:, ai, :t]                                             # :103
        if var_tab is None:
            dE, var = predict(NN, L, mean, xn[0:3, :].T, V=V, P=P, dtype=dtype)
        else:
            dE, var = predict(NN, L, mean, xn[0:3, :].T, dtype=dtype)[0], var_tab[:N_P]        # dVarft(i,:) by slot (:270)
        w = meas_model(y[t, :], xn, dE, var, sigma2, dtype)                                    # :110
        sw = np.sum(w)
        degenerate[t] = bool(sw <= 1e-12)                                                      # :113-115
        lsw[t] = np.log(sw)
        w = w / sw                                                                             # :118
        iw_max = int(np.argmax(w))                                                             # :121 (first maximum)
        traj_max[:, t] = xn[:, iw_max]                                                         # :122
        traj_mean[:, t] = np.sum(xn * w, axis=1)                                               # :123
        W[t] = w
    return dict(traj_max=traj_max, traj_mean=traj_mean, ai=AI, w=W, log_sum_w=lsw, xn_traj=xn_traj, degenerate=degenerate)


# ---- seeded problem instances ------------------------------------------------------------------------------------------------
def loc_case(N_P, N_T, m, seed=1, global_init=False, table=False, dt=0.01):
    """A synthetic instance from the oracle's generators: a bean_6D run gives the field, the training path (map by batch
    regression, run_localization.m:134-151) and the path to localise.  global_init: x0 [7 x N_P] with positions uniform over the
    training path's bounding box (:156-160).  table: var_points = N_P points of a grid over the box (the reference's xt, :103-106)."""
    import cases
    d = O.generate_bean_6D(N_T, cases.Q_MAG, cases.THETA_MAG, dt, seed=seed, m_sim=300)
    L, NN = O.domain_cartesian_dx(m, 3, d["LL"])
    rs = np.random.RandomState(seed + 500)
    # training data: the true path with the field measured in the navigation frame (y rotated back by the true attitude)
    pos = np.asarray(d["pos"], dtype=np.float64).T.copy()                                     # [N_T x 3]
    quat = np.asarray(d["quat"], dtype=np.float64).reshape(-1, 4)
    y_nav = np.stack([O.quat2rmat(quat[t]) @ d["y"][t] for t in range(N_T)])
    foo, Lc, V = map_from_data(NN, L, pos, y_nav, cases.THETA_MAG)
    x0 = np.asarray(d["initState"], dtype=np.float64).ravel()
    if global_init:
        lo, hi = pos.min(axis=0), pos.max(axis=0)
        x0 = np.repeat(x0.reshape(7, 1), N_P, axis=1)
        x0[0, :] = lo[0] + (hi[0] - lo[0]) * rs.random_sample(N_P)
        x0[1, :] = lo[1] + (hi[1] - lo[1]) * rs.random_sample(N_P)
    var_points = None
    if table:
        g = int(math.ceil(math.sqrt(N_P)))
        X1, X2 = np.meshgrid(np.linspace(-L[0], L[0], g), np.linspace(-L[1], L[1], g))
        var_points = np.column_stack((X1.ravel(), X2.ravel(), np.zeros(g * g)))[:N_P]
    U = rs.random_sample((max(N_T - 1, 0), N_P))
    Z = rs.standard_normal((max(N_T - 1, 0), N_P, 6))
    return dict(NN=NN, L=L, mean=foo, V=V, Lc=Lc, sigma2=float(cases.THETA_MAG[3]), theta=cases.THETA_MAG, odometry=d["dx"], y=d["y"],
                x0_nonLin=x0, Q=cases.Q_MAG, N_P=N_P, dt=dt, U=U, Z=Z, var_points=var_points, train_x=pos, train_y=y_nav, m=m, LL=d["LL"])


def run_case(c, dtype=np.float64, **kw):
    return particleFilterLocalization(c["NN"], c["L"], c["mean"], c["sigma2"], c["odometry"], c["y"], c["x0_nonLin"], c["Q"], c["N_P"],
                                      c["dt"], c["U"], c["Z"], V=c["V"], var_points=c["var_points"], dtype=dtype, **kw)
