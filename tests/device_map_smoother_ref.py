"""Checker of the backward-simulation smoother in a DeviceMap with a Gaussian transition density (rbpf.DeviceTransition): the
recursion of tests/localization_smoother_ref.py,

    b[T-1][j] = sample(w[T-1], u[T-1][j])
    t = T-2 .. 0:  l_i = log w[t][i] + logp(xs[t+1][j] | X[t][:, i]),  p = exp(l - lse(l)),  b[t][j] = sample(p, u[t][j])

with the density of a dynModel that is a drift plus Gaussian noise on the state rows `rows`, constants omitted
(particleSmoother.m:181-182):

    r = wrap(x'[rows] - mu_i),   z = L \\ r  (L = chol(cov, 'lower')),   logp = -z'z / 2,     wrap(r) = r - 2 pi rint(r / (2 pi))

on the angle rows, 2 pi the fp64 constant.  mu_i [n_res] is what the model's `mean` handle returned for particle i, a float64
array: the checker starts from it, as the kernels do.  z by forward substitution with device_map_ref.chol / forward.  Everything
is vectorised over the particles; `dtype=np.longdouble` runs the same statements in extended precision on the same fp64 inputs.
Every draw reports its margin and eps_ref (localization_smoother_ref._draw): the restatement is its own arbiter.

The committed cases are four models, each x' = post(drift(x, dx) + Gn chol(dt Q) z), post wrapping the angle rows of the STATE
into [-pi, pi]:
  A  generic_model.GenericModel, n_w = n_nonlin = 3: mean = drift, cov = G (dt Q) G', a full 3 x 3 with a full factor.
  B  an 8-state additive model, n_res = 8, x' = x + dx + chol(dt Q) z with a full random SPD Q: the default cov = dt Q.
  C  the dense-radio motion model: 2-D position + heading, noise on the heading only (rows = (2,), angle_rows = (2,), n_res = 1), Q
     in pages (one value per step); the true heading passes +-pi during the run.
  D  n_nonlin = 4, rows = (0, 1, 3), angle_rows = (3,), a coupled 3 x 3 cov; row 2 moves without noise and takes no part.
The angle residuals of every committed input lie within a few standard deviations of 0 mod 2 pi, never near +-pi, where the fp64
and the long-double wrap could round to different branches (a property of the density, not of a kernel).

Nothing in the package imports this file."""
import numpy as np

import device_map_ref as dm
import generic_model as gm
import generic_ny_cases as gc
import rbpf_oracle as O
from localization_smoother_ref import _draw, _log_weights, backward_cdf

LD = np.longdouble
TWO_PI = np.float64(2.0 * np.pi)


def wrap(r, dtype=np.float64):
    two_pi = dtype(TWO_PI)
    return r - two_pi * np.rint(r / two_pi)


def residual(xt, mu, cov, rows, angle_rows=(), dtype=np.float64):
    """z [n_res x N]: the normals the sampler would have needed to move particle i (predicted rows mu[:, i]) to xt [n_nonlin]."""
    rows = tuple(rows)
    xt = np.asarray(xt, dtype=np.float64).astype(dtype).ravel()
    mu = np.asarray(mu, dtype=np.float64).astype(dtype).reshape(len(rows), -1)
    r = xt[list(rows), None] - mu
    for a in angle_rows:
        k = rows.index(a)
        r[k] = wrap(r[k], dtype)
    L = dm.chol(np.asarray(cov, dtype=np.float64).astype(dtype).reshape(len(rows), len(rows)))
    return dm.forward(L, r)


def logp(xt, mu, cov, rows, angle_rows=(), dtype=np.float64):
    """[N] log transition densities xt | particle i, constants omitted."""
    z = residual(xt, mu, cov, rows, angle_rows, dtype)
    return -dtype(0.5) * np.sum(z * z, axis=0)


def backward_step(mu, w, xs_next, cov, u, rows, angle_rows=()):
    """One backward step on the caller's arrays: mu [n_res x N], w [N], xs_next [n_nonlin x M], u [M].
    Returns dict(index, index_ld [M], margin, eps_ref [M] (long double), logp, logp_ld [N x M])."""
    mu = np.asarray(mu, dtype=np.float64).reshape(len(rows), -1)
    xs_next = np.asarray(xs_next, dtype=np.float64)
    N, M = mu.shape[1], xs_next.shape[1]
    u = np.asarray(u, dtype=np.float64).ravel()
    out = dict(index=np.zeros(M, dtype=np.int64), index_ld=np.zeros(M, dtype=np.int64), margin=np.zeros(M, dtype=LD),
               eps_ref=np.zeros(M, dtype=LD), logp=np.zeros((N, M)), logp_ld=np.zeros((N, M), dtype=LD))
    lw, lw_ld = _log_weights(w, np.float64), _log_weights(w, LD)
    for j in range(M):
        lp = logp(xs_next[:, j], mu, cov, rows, angle_rows)
        lp_ld = logp(xs_next[:, j], mu, cov, rows, angle_rows, LD)
        i, i_ld, mg, ep = _draw(backward_cdf(lw + lp), backward_cdf(lw_ld + lp_ld), u[j:j + 1])
        out["index"][j], out["index_ld"][j], out["margin"][j], out["eps_ref"][j] = i[0], i_ld[0], mg[0], ep[0]
        out["logp"][:, j], out["logp_ld"][:, j] = lp, lp_ld
    return out


def backward_simulate(X, W, mus, covs, u, rows, angle_rows=()):
    """The whole recursion on forward arrays X [T x n_nonlin x N] (as propagated), W [T x N] (normalised), the handle's results
    mus[t] [n_res x N] and the covariances covs[t] for t = 0 .. T-2, u [T x M].  Returns dict(index, index_ld [T x M],
    xs_traj [n_nonlin x M x T], traj_smooth_mean [n_nonlin x T], margin, eps_ref [T x M] (long double), logp_rel)."""
    X, W, u = np.asarray(X, dtype=np.float64), np.asarray(W, dtype=np.float64), np.asarray(u, dtype=np.float64)
    T, _, N = X.shape
    M = u.shape[1]
    index, index_ld = np.zeros((T, M), dtype=np.int64), np.zeros((T, M), dtype=np.int64)
    margin, eps_ref = np.zeros((T, M), dtype=LD), np.zeros((T, M), dtype=LD)
    index[T - 1], index_ld[T - 1], margin[T - 1], eps_ref[T - 1] = _draw(np.cumsum(W[T - 1]), np.cumsum(W[T - 1].astype(LD)), u[T - 1])
    err, scale = 0.0, 0.0
    for t in range(T - 2, -1, -1):
        lw, lw_ld = _log_weights(W[t], np.float64), _log_weights(W[t], LD)
        for b in np.unique(index[t + 1]):
            js = np.nonzero(index[t + 1] == b)[0]
            lp = logp(X[t + 1][:, b], mus[t], covs[t], rows, angle_rows)
            lp_ld = logp(X[t + 1][:, b], mus[t], covs[t], rows, angle_rows, LD)
            err, scale = max(err, float(np.max(np.abs(lp - lp_ld)))), max(scale, float(np.max(np.abs(lp_ld))))
            index[t, js], index_ld[t, js], margin[t, js], eps_ref[t, js] = _draw(backward_cdf(lw + lp), backward_cdf(lw_ld + lp_ld), u[t, js])
    xs = np.stack([X[t][:, index[t]] for t in range(T)], axis=2)
    return dict(index=index, index_ld=index_ld, xs_traj=xs, traj_smooth_mean=np.mean(xs, axis=1), margin=margin, eps_ref=eps_ref,
                logp_rel=err / max(scale, 1e-300))


def ffbsm_marginals(X, W, mus, covs, rows, angle_rows=(), dtype=LD):
    """The O(N^2) forward-filter backward-smoother marginal weights, directly (localization_smoother_ref.ffbsm_marginals)."""
    X = np.asarray(X, dtype=np.float64)
    T, _, N = X.shape
    Ws = np.zeros((T, N), dtype=dtype)
    Ws[T - 1] = np.asarray(W[T - 1], dtype=dtype)
    for t in range(T - 2, -1, -1):
        F = np.stack([np.exp(logp(X[t + 1][:, k], mus[t], covs[t], rows, angle_rows, dtype)) for k in range(N)], axis=1)   # F[i, k]
        wt = np.asarray(W[t], dtype=dtype)
        Ws[t] = wt * (F @ (Ws[t + 1] / (wt @ F)))
    return Ws


# ---- the four models ---------------------------------------------------------------------------------------------------------
class Case:
    """A model (measurement side: a generic_model.GenericModel), its problem p (generic_ny_cases plus the map of device_map_ref.case)
    and the statement of its transition: rows, angle_rows, drift(x [n_nonlin x N], dx) -> [n_nonlin x N], Gn [n_nonlin x n_w]."""

    def __init__(self, name, m, p, rows, angle_rows, drift, Gn, default_cov=False):
        self.name, self.m, self.p, self.rows, self.angle_rows, self.drift, self.Gn = name, m, p, tuple(rows), tuple(angle_rows), drift, Gn
        self.default_cov = default_cov                                    # cov = dt Q is the transition's default
        self.nN, self.n_res = m.nNonLin, len(self.rows)
        Q = np.asarray(p["Q"], dtype=np.float64)
        self.Qp = Q[:, :, None] if Q.ndim == 2 else Q
        self.dt = np.atleast_1d(np.asarray(p["dt"], dtype=np.float64)).ravel()

    def Q(self, t):
        return self.Qp[:, :, t if self.Qp.shape[2] > 1 else 0]

    def dtt(self, t):
        return float(self.dt[t if self.dt.size > 1 else 0])

    def cov_of(self, dt, Q):
        """The host callable of the DeviceTransition."""
        Gr = self.Gn[list(self.rows)]
        return Gr @ (dt * np.atleast_2d(Q)) @ Gr.T

    def cov(self, t):
        return self.cov_of(self.dtt(t), self.Q(t))

    def mean(self, x, t):
        return self.drift(np.asarray(x, dtype=np.float64), self.p["odometry"][t])[list(self.rows)]

    def post(self, x):
        for a in self.angle_rows:
            x[a] = wrap(x[a])
        return x

    def dyn(self, x, t, z):
        """x [n_nonlin x N], z [N x n_w] -> the states of step t + 1."""
        Lq = np.linalg.cholesky(np.atleast_2d(self.dtt(t) * self.Q(t)))
        return self.post(self.drift(x, self.p["odometry"][t]) + self.Gn @ (Lq @ z.T))


def _rot_drift(x, dx):
    """Dense-radio motion: the odometry's planar step turned by the heading, the heading advanced by dx(3)."""
    c, s = np.cos(x[2]), np.sin(x[2])
    return np.stack((x[0] + c * dx[0] - s * dx[1], x[1] + s * dx[0] + c * dx[1], x[2] + dx[2]))


def _simulate_y(c, seed):
    """The map (mean, V) of device_map_ref.case and y along a true path of the case's own dynModel."""
    m, p = c.m, c.p
    rs = np.random.RandomState(4000 + seed)
    n, d, nN = m.nLin, m.ny, m.nNonLin
    p["mean"] = p["x0_lin"] + 0.05 * rs.standard_normal(n)
    p["V"] = np.tril(rs.standard_normal((n, n))) * np.sqrt(0.1 / n)
    xl_true = p["mean"] + p["V"].T @ rs.standard_normal(n)
    Lr = np.linalg.cholesky(p["R"])
    x = np.asarray(p["x0_nonLin"], dtype=np.float64).reshape(nN, 1).copy()
    T = p["y"].shape[0]
    y = np.zeros((T, d))
    for t in range(T):
        if t > 0:
            x = c.dyn(x, t - 1, rs.standard_normal((1, m.nw)))
        y[t] = m.measModel(x)[0] @ xl_true + Lr @ rs.standard_normal(d)
    p["y"] = y


_CASES = {}


def case(name, N_P, N_T, seed=3):
    """Model A, B, C or D at (N_P, N_T), built once."""
    key = (name, N_P, N_T, seed)
    if key in _CASES:
        return _CASES[key]
    rs = np.random.RandomState(7000 + seed + ord(name))
    if name == "A":
        m, p = gc.case((3, 3, 3, 2, 17), N_P, N_T, seed=seed)
        drift = lambda x, dx: x + m.bend * np.sin(x) + (m.A @ dx)[:, None]                     # noqa: E731
        c = Case(name, m, p, (0, 1, 2), (), drift, m.G)
    elif name == "B":
        m, p = gc.case((8, 8, 8, 3, 21), N_P, N_T, seed=seed, additive=True)
        B = rs.standard_normal((8, 8))
        p["Q"] = 0.02 * (B @ B.T) / 8.0 + 0.01 * np.eye(8)
        drift = lambda x, dx: x + (m.A @ dx)[:, None]                                           # noqa: E731
        c = Case(name, m, p, range(8), (), drift, m.G, default_cov=True)
    elif name == "C":
        m, p = gc.case((3, 1, 3, 2, 15), N_P, N_T, seed=seed)
        p["Q"] = rs.uniform(0.05, 0.15, (1, 1, max(N_T - 1, 1)))                                # one value per step
        p["dt"] = 0.1
        p["x0_nonLin"] = np.array([0.4, -0.2, 3.0])
        p["odometry"] = np.column_stack((0.2 * np.ones(max(N_T - 1, 1)), 0.05 * rs.standard_normal(max(N_T - 1, 1)), 0.1 * np.ones(max(N_T - 1, 1))))
        p["Z"] = np.random.RandomState(7100 + seed).standard_normal((1, max(N_T - 1, 0), N_P, 1))
        c = Case(name, m, p, (2,), (2,), _rot_drift, np.array([[0.0], [0.0], [1.0]]))
    elif name == "D":
        m, p = gc.case((4, 3, 4, 3, 19), N_P, N_T, seed=seed)
        Cc = np.eye(3) + 0.4 * rs.standard_normal((3, 3))                                       # couples the three noisy rows
        Gn = np.zeros((4, 3))
        Gn[[0, 1, 3]] = Cc
        p["x0_nonLin"] = np.array([0.3, -0.5, 0.2, 3.05])
        p["odometry"][:, :] = 0.3 * rs.standard_normal(p["odometry"].shape)
        A = m.A.copy()
        A[3] = 0.0
        A[3, 3] = 1.0
        p["odometry"][:, 3] = 0.06                                                              # the heading climbs through pi
        drift = lambda x, dx: x + 0.1 * np.sin(x) * np.array([1.0, 1.0, 1.0, 0.0])[:, None] + (A @ dx)[:, None]    # noqa: E731
        c = Case(name, m, p, (0, 1, 3), (3,), drift, Gn)
        c.A = A
    else:
        raise KeyError(name)
    _simulate_y(c, seed)
    _CASES[key] = c
    return c


def forward_arrays(c, dtype=np.float64):
    """The restatement's forward pass of device_map_ref.run with the case's own dynModel: the particles as propagated
    X [T x n_nonlin x N], the normalised weights W [T x N] and the ancestors ai [T x N]."""
    m, p = c.m, c.p
    N, T, nN = p["N_P"], p["y"].shape[0], c.nN
    U, Z = p["U"][0], p["Z"][0]
    sample = O.sample if dtype is np.float64 else dm._sample_ld
    xn = np.repeat(np.asarray(p["x0_nonLin"], dtype=np.float64).reshape(nN, 1), N, axis=1)
    X, W, AI = np.zeros((T, nN, N)), np.zeros((T, N), dtype=dtype), np.zeros((T, N), dtype=np.int64)
    w = np.full(N, dtype(1.0) / dtype(N), dtype=dtype)
    for t in range(T):
        if t != 0:
            AI[t] = [sample(w, U[t - 1, i]) for i in range(N)]
            xn = c.dyn(xn[:, AI[t]], t - 1, Z[t - 1])
        X[t] = xn
        _, _, logw = dm.weights(m.measModel(xn), p["mean"], p["V"], p["R"], p["y"][t], dtype)
        e = np.exp(logw - np.max(logw))
        w = e / np.sum(e)
        W[t] = w
    return X, W, AI


def transition_arrays(c, X):
    """(mus, covs) of steps 0 .. T-2 on the forward particles X."""
    T = X.shape[0]
    return [c.mean(X[t], t) for t in range(T - 1)], [c.cov(t) for t in range(T - 1)]


# ---- the committed cases: the CPU test checks the margin condition on exactly what the GPU tests run -------------------------
PROBE_LOGP_SHAPES = [(1, 1), (70, 5), (257, 65)]
PROBE_INDEX_SHAPES = [(64, 64), (70, 1), (1, 3), (4100, 130)]
PROBE_LOGP_CASES = [("A", N, M) for N, M in PROBE_LOGP_SHAPES] + [("B", 257, 65), ("C", 70, 5), ("D", 70, 5)]
PROBE_INDEX_CASES = [("A", N, M) for N, M in PROBE_INDEX_SHAPES] + [("B", 4100, 130), ("C", 64, 64), ("D", 64, 64)]
FULL_RUNS = [("A", 70, 8, 33), ("B", 40, 5, 33), ("C", 257, 6, 1), ("D", 65, 6, 17)]          # (model, N_P, N_T, n_traj)
U_SEED = 4242

_PROBES = {}


def probe_case(name, N, M, seed=7):
    """Inputs of one backward step of model `name`: N particles scattered two standard deviations of the transition noise around
    a centre (the angle rows around 3.1: part of the cloud has wrapped to -pi), mu their predicted rows, M states of the next
    step drawn by the model's dynModel from random live particles.  From N = 64 on the first and the last ten weights are exact
    zeros.  Built once per (name, N, M)."""
    key = (name, N, M, seed)
    if key in _PROBES:
        return _PROBES[key]
    c = case(name, 8, 4)
    rs = np.random.RandomState(1000 * seed + N + 7 * M + ord(name))
    cov = c.cov(1)
    Lc = np.linalg.cholesky(cov)
    X = rs.uniform(-1.0, 1.0, (c.nN, 1)) + 0.1 * rs.standard_normal((c.nN, N))
    X[list(c.rows)] = rs.uniform(-1.0, 1.0, (c.n_res, 1)) + 2.0 * (Lc @ rs.standard_normal((c.n_res, N)))
    for a in c.angle_rows:
        X[a] += 3.1 - np.mean(X[a])
    X = c.post(X)
    w = rs.random_sample(N) + 0.05
    if N >= 64:
        w[:10] = 0.0
        w[-10:] = 0.0
    w /= w.sum()
    live = np.nonzero(w > 0)[0]
    pick = live[rs.randint(live.size, size=M)]
    xs_next = c.dyn(X[:, pick], 1, rs.standard_normal((M, c.m.nw)))
    out = dict(case=c, X=X, mu=c.mean(X, 1), w=w, xs_next=xs_next, cov=cov, u=rs.random_sample(M), rows=c.rows, angle_rows=c.angle_rows)
    _PROBES[key] = out
    return out


_PROBE_REFS = {}


def probe_reference(name, N, M):
    """backward_step of probe_case(name, N, M), computed once and shared."""
    key = (name, N, M)
    if key not in _PROBE_REFS:
        p = probe_case(name, N, M)
        _PROBE_REFS[key] = backward_step(p["mu"], p["w"], p["xs_next"], p["cov"], p["u"], p["rows"], p["angle_rows"])
    return _PROBE_REFS[key]


def full_run_uniforms(N_T, M):
    return np.random.RandomState(U_SEED).random_sample((N_T, M))
