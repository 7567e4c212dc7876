"""Checker of the backward-simulation smoother for localisation in a fixed map (forward filter, backward simulation: Godsill,
Doucet & West 2004): a restatement of the recursion in numpy on the primitives of tests/localization_ref.py.

    b[T-1][j] = sample(w[T-1], u[T-1][j])
    t = T-2 .. 0:  l_i = log w[t][i] + logp(xs[t+1][j] | X[t][:, i]),  p = exp(l - lse(l))   (particleSmoother.m:232, :236-238)
                   b[t][j] = sample(p, u[t][j])                                               (:241, tools/sample.m:30-32)

logp is the density of the localisation dynModel (run_localization.m:274-281) as it draws, constants omitted
(particleSmoother.m:181-182): with a = qRight(q_i) dq, e = qLeft(qInv(a)) q~, phi = logq(e) (tools/logq.m:26-30),
r = [p~ - p_i - dx(1:3); phi], z = blkdiag(S_pos, S_rot) \\ r with S = sqrt(dt Q) element-wise, logp = -z'z / 2.

Everything is vectorised over the particles i; `dtype=np.longdouble` runs the same statements in extended precision on the same
fp64 inputs.  Every draw reports its margin (distance from u to the nearest cdf edge, in long double) and
eps_ref = max |cdf_fp64 - cdf_longdouble|: the restatement is its own arbiter.

Nothing in the package imports this file.
"""
import numpy as np

import localization_ref as R


def qright_mul(q, p):
    """qRight(q) p (tools/qRight.m:29-34) for q [4 x N], p [4]: rows summed left to right."""
    return np.stack((q[0] * p[0] + (-q[1]) * p[1] + (-q[2]) * p[2] + (-q[3]) * p[3],
                     q[1] * p[0] + q[0] * p[1] + q[3] * p[2] + (-q[2]) * p[3],
                     q[2] * p[0] + (-q[3]) * p[1] + q[0] * p[2] + q[1] * p[3],
                     q[3] * p[0] + q[2] * p[1] + (-q[1]) * p[2] + q[0] * p[3]))


def qleft_mul(q, p):
    """qLeft(q) p (tools/qLeft.m:30-35) for q [4 x N], p [4]."""
    return np.stack((q[0] * p[0] + (-q[1]) * p[1] + (-q[2]) * p[2] + (-q[3]) * p[3],
                     q[1] * p[0] + q[0] * p[1] + (-q[3]) * p[2] + q[2] * p[3],
                     q[2] * p[0] + q[3] * p[1] + q[0] * p[2] + (-q[1]) * p[3],
                     q[3] * p[0] + (-q[2]) * p[1] + q[1] * p[2] + q[0] * p[3]))


def qinv(q):
    """tools/qInv.m:27-31."""
    return np.stack((q[0], -q[1], -q[2], -q[3]))


def logq(q):
    """tools/logq.m:26-30 for q [4 x N], sign flip included; q0 > 1 by rounding is clamped (MATLAB's acos would go complex)."""
    q = np.where(q[0] < 0, -q, q)
    na = np.arccos(np.minimum(q[0], q.dtype.type(1.0)))
    return na * q[1:4] / (np.sin(na) + (na == 0))


def inv3(A):
    """Inverse of a 3 x 3 matrix by its adjugate (np.linalg has no long double)."""
    a, b, c, d, e, f, g, h, i = A.ravel()
    adj = np.array([[e * i - f * h, c * h - b * i, b * f - c * e],
                    [f * g - d * i, a * i - c * g, c * d - a * f],
                    [d * h - e * g, b * g - a * h, a * e - b * d]], dtype=A.dtype)
    det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)
    if det == 0:
        raise ValueError("singular noise block")
    return adj / det


def noise_inverses(dt, Q, dtype=np.float64):
    """inv(S_pos), inv(S_rot) with S = sqrt(dt Q) element-wise on the diagonal blocks (run_localization.m:277, :279)."""
    Q = np.asarray(Q, dtype=dtype)
    dt = dtype(dt)
    return inv3(np.sqrt(dt * Q[0:3, 0:3])), inv3(np.sqrt(dt * Q[3:6, 3:6]))


def residual(xt, X, dx, dt, Q, dtype=np.float64):
    """z [6 x N]: the six normals dynModel would have needed to move particle i of X [7 x N] to xt [7]."""
    xt = np.asarray(xt, dtype=dtype).ravel()
    X = np.asarray(X, dtype=dtype).reshape(7, -1)
    dx = np.asarray(dx, dtype=dtype).ravel()
    Sp, Sr = noise_inverses(dt, Q, dtype)
    a = qright_mul(X[3:7], dx[3:7])
    phi = logq(qleft_mul(qinv(a), xt[3:7]))
    r = xt[0:3, None] - X[0:3] - dx[0:3, None]
    return np.vstack((Sp @ r, Sr @ phi))


def logp(xt, X, dx, dt, Q, dtype=np.float64):
    """[N] log transition densities xt | X[:, i], constants omitted."""
    z = residual(xt, X, dx, dt, Q, dtype)
    return -dtype(0.5) * np.sum(z * z, axis=0)


def backward_cdf(logw_plus_logp):
    """particleSmoother.m:236-238 then the cumsum of tools/sample.m:30."""
    l = logw_plus_logp
    c = np.max(l)
    lse = c + np.log(np.sum(np.exp(l - c)))
    return np.cumsum(np.exp(l - lse))


def _log_weights(w, dtype):
    w = np.asarray(w, dtype=dtype)
    with np.errstate(divide="ignore"):
        return np.log(w)


def _draw(cdf64, cdf_ld, u):
    """(index by the fp64 cdf, index by the long-double cdf, margin, eps_ref) for the uniforms u [M] against one cdf."""
    u = np.asarray(u, dtype=np.float64)
    idx = np.sum(cdf64[None, :] < u[:, None], axis=1)
    idx_ld = np.sum(cdf_ld[None, :] < u.astype(np.longdouble)[:, None], axis=1)
    margin = np.min(np.abs(cdf_ld[None, :] - u.astype(np.longdouble)[:, None]), axis=1)
    eps = np.max(np.abs(cdf64.astype(np.longdouble) - cdf_ld))
    return idx, idx_ld, margin, np.full(u.shape, eps, dtype=np.longdouble)


def backward_step(X, w, xs_next, odo, dt, Q, u):
    """One backward step on the caller's arrays: X [7 x N], w [N], xs_next [7 x M], u [M].
    Returns dict(index, index_ld [M], margin, eps_ref [M] (long double), logp, logp_ld [N x M])."""
    X = np.asarray(X, dtype=np.float64).reshape(7, -1)
    xs_next = np.asarray(xs_next, dtype=np.float64).reshape(7, -1)
    M = xs_next.shape[1]
    u = np.asarray(u, dtype=np.float64).ravel()
    out = dict(index=np.zeros(M, dtype=np.int64), index_ld=np.zeros(M, dtype=np.int64), margin=np.zeros(M, dtype=np.longdouble),
               eps_ref=np.zeros(M, dtype=np.longdouble), logp=np.zeros((X.shape[1], M)), logp_ld=np.zeros((X.shape[1], M), dtype=np.longdouble))
    lw, lw_ld = _log_weights(w, np.float64), _log_weights(w, np.longdouble)
    for j in range(M):
        lp = logp(xs_next[:, j], X, odo, dt, Q)
        lp_ld = logp(xs_next[:, j], X, odo, dt, Q, np.longdouble)
        i, i_ld, mg, ep = _draw(backward_cdf(lw + lp), backward_cdf(lw_ld + lp_ld), u[j:j + 1])
        out["index"][j], out["index_ld"][j], out["margin"][j], out["eps_ref"][j] = i[0], i_ld[0], mg[0], ep[0]
        out["logp"][:, j], out["logp_ld"][:, j] = lp, lp_ld
    return out


def backward_simulate(X, W, odometry, Q, dt, u):
    """The whole recursion on forward arrays X [T x 7 x N] (as propagated), W [T x N] (normalised), u [T x M].
    Returns dict(index, index_ld [T x M], xs_traj [7 x M x T], traj_smooth_mean [7 x T], margin, eps_ref [T x M] (long double),
    logp_rel: the largest distance of the fp64 from the long-double logp over all steps, relative to the largest |logp|).
    xs[t+1][j] is one of the N particles of step t + 1, so a step computes at most N distinct cdfs whatever M is."""
    X = np.asarray(X, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    u = np.asarray(u, dtype=np.float64)
    T, _, N = X.shape
    M = u.shape[1]
    odometry = np.asarray(odometry, dtype=np.float64)
    Q = np.asarray(Q, dtype=np.float64)
    Q = np.repeat(Q[:, :, None], T, axis=2) if Q.ndim == 2 else Q
    dt = np.atleast_1d(np.asarray(dt, dtype=np.float64)).ravel()
    dt = dt[0] * np.ones(T) if dt.size == 1 else dt
    index = np.zeros((T, M), dtype=np.int64)
    index_ld = np.zeros((T, M), dtype=np.int64)
    margin = np.zeros((T, M), dtype=np.longdouble)
    eps_ref = np.zeros((T, M), dtype=np.longdouble)
    index[T - 1], index_ld[T - 1], margin[T - 1], eps_ref[T - 1] = _draw(np.cumsum(W[T - 1]), np.cumsum(W[T - 1].astype(np.longdouble)), u[T - 1])
    err, scale = 0.0, 0.0
    for t in range(T - 2, -1, -1):
        lw, lw_ld = _log_weights(W[t], np.float64), _log_weights(W[t], np.longdouble)
        for b in np.unique(index[t + 1]):
            js = np.nonzero(index[t + 1] == b)[0]
            lp = logp(X[t + 1][:, b], X[t], odometry[t], dt[t], Q[:, :, t])
            lp_ld = logp(X[t + 1][:, b], X[t], odometry[t], dt[t], Q[:, :, t], np.longdouble)
            err, scale = max(err, float(np.max(np.abs(lp - lp_ld)))), max(scale, float(np.max(np.abs(lp_ld))))
            index[t, js], index_ld[t, js], margin[t, js], eps_ref[t, js] = _draw(backward_cdf(lw + lp), backward_cdf(lw_ld + lp_ld), u[t, js])
    xs = np.stack([X[t][:, index[t]] for t in range(T)], axis=2)
    return dict(index=index, index_ld=index_ld, xs_traj=xs, traj_smooth_mean=np.mean(xs, axis=1), margin=margin, eps_ref=eps_ref,
                logp_rel=err / max(scale, 1e-300))


def ffbsm_marginals(X, W, odometry, Q, dt, dtype=np.longdouble):
    """The O(N^2) forward-filter backward-smoother marginal weights, directly:
    w_{t|T}(i) = w_t(i) sum_k w_{t+1|T}(k) f(x_{t+1}^k | x_t^i) / sum_l w_t(l) f(x_{t+1}^k | x_t^l)."""
    X = np.asarray(X, dtype=np.float64)
    T, _, N = X.shape
    Ws = np.zeros((T, N), dtype=dtype)
    Ws[T - 1] = np.asarray(W[T - 1], dtype=dtype)
    for t in range(T - 2, -1, -1):
        F = np.stack([np.exp(logp(X[t + 1][:, k], X[t], odometry[t], dt, Q, dtype)) for k in range(N)], axis=1)   # F[i, k]
        wt = np.asarray(W[t], dtype=dtype)
        den = wt @ F
        Ws[t] = wt * (F @ (Ws[t + 1] / den))
    return Ws


def forward_arrays(c, ref=None):
    """The forward particles as propagated, X [T x 7 x N], and the normalised weights W [T x N] of the restatement's filter on the
    case c (localization_ref.run_case returns the traced-back xn_traj only: the particles are rebuilt from its ancestors)."""
    ref = ref if ref is not None else R.run_case(c)
    T, N = ref["w"].shape
    x0 = np.asarray(c["x0_nonLin"], dtype=np.float64)
    X = np.zeros((T, 7, N))
    X[0] = x0.reshape(7, -1) if x0.ndim > 1 and x0.shape[1] > 1 else np.repeat(x0.reshape(7, 1), N, axis=1)
    for t in range(1, T):
        for i in range(N):
            X[t][:, i] = R.dyn_model(X[t - 1][:, ref["ai"][t, i]], c["odometry"][t - 1], c["dt"], c["Q"], c["Z"][t - 1, i, :])
    return X, np.asarray(ref["w"], dtype=np.float64)


# ---- the committed cases: the CPU test checks the margin condition on exactly what the GPU tests run -------------------------
PROBE_LOGP_SHAPES = [(1, 1), (70, 5), (257, 65)]
PROBE_INDEX_SHAPES = [(64, 64), (70, 1), (1, 3), (4100, 130)]
FULL_RUNS = [(70, 8, 33, False), (70, 8, 33, True), (257, 6, 1, False)]       # (N_P, N_T, M, global_init), m = 13 maps
U_SEED = 4242


def probe_case(N, M, seed=7):
    """Inputs of one backward step: N particles scattered like a filter's cloud after a few steps, M states of the next step
    drawn by dynModel from random particles.  N = 70: a Q with full diagonal blocks (the element-wise square root is then no
    factor of anything, the 3 x 3 inverses are full); otherwise the examples' diagonal Q.  From N = 64 on the first and the last
    ten weights are exact zeros."""
    import cases
    rs = np.random.RandomState(1000 * seed + N + 7 * M)
    dt = 0.01
    if N == 70:
        d = np.sqrt(np.diag(cases.Q_MAG) * (0.5 + rs.random_sample(6)))
        Q = np.outer(d, d) * (0.2 + 0.8 * np.eye(6))
    else:
        Q = cases.Q_MAG
    spread = 2.0 * np.sqrt(dt * np.diag(Q))
    X = np.zeros((7, N))
    X[0:3] = np.array([[1.5], [-0.7], [0.3]]) + spread[0:3, None] * rs.standard_normal((3, N))
    q0 = R._expq(0.4 * rs.standard_normal(3))
    for i in range(N):
        X[3:7, i] = R._qLeft(q0) @ R._expq(spread[3:6] * rs.standard_normal(3))
    dx = np.concatenate((0.05 * rs.standard_normal(3), R._expq(0.02 * rs.standard_normal(3))))
    w = rs.random_sample(N) + 0.05
    if N >= 64:
        w[:10] = 0.0
        w[-10:] = 0.0
    w /= w.sum()
    live = np.nonzero(w > 0)[0]
    xs_next = np.column_stack([R.dyn_model(X[:, live[rs.randint(live.size)]], dx, dt, Q, rs.standard_normal(6)) for _ in range(M)])
    return dict(X=X, w=w, xs_next=xs_next, odo=dx, dt=dt, Q=Q, u=rs.random_sample(M))


def full_run_uniforms(N_T, M):
    return np.random.RandomState(U_SEED).random_sample((N_T, M))
