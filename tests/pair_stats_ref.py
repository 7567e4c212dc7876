"""Checker of the two-slice (pairwise) smoothed moments of the transition residual (LocalizationSession.transition_statistics,
csrc/rbpf_loc_pairstats.hpp): a restatement in numpy, every sum in np.longdouble,

    xi_t(i, j)  = exp(log w_t(i) + c_t(j) + logp(X[t+1][:, j] | X[t][:, i]) - log(mass_t))           (sums to 1 over all pairs)
    S_t = sum_ij xi_t(i, j) r_ij r_ij',     m_t = sum_ij xi_t(i, j) r_ij,     pair_mass_t = sum_ij xi_t(i, j)

D, c, lws and mass_t = sum_i exp(lws(i)) come from marginal_smoother_ref.step, logp from the matrices that file's probes carry.  The
UN-WHITENED residual r_ij is taken from the three families' own checkers, not restated:
    the dense-mag map     localization_smoother_ref.residual gives z = [inv(S_pos) r_pos; inv(S_rot) phi]; r = [S_pos z_pos; S_rot z_rot]
                          with S = the element-wise sqrt(dt Q) of the diagonal blocks, in long double
    Gaussian transitions  device_map_smoother_ref.residual gives z = L \\ r, L = chol(cov); r = L z
    a quaternion block    pose_transition_ref.residual_vector gives r, in the caller's residual order
A successor is handled at a time (r [n_res x N]): the N x M x n_res tensor is never formed.
tests/test_pair_stats_cpu.py checks this restatement's xi against the two-slice marginals of the backward-simulation path law.

Nothing in the package imports this file."""
import numpy as np

import device_map_ref as dm
import device_map_smoother_ref as S
import localization_smoother_ref as LS
import map_trajectory_ref as V
import marginal_smoother_ref as G
import pose_transition_ref as P

LD = np.longdouble


# ---- the un-whitened residuals: r_of(j) -> [n_res x N], long double -----------------------------------------------------------
def r_mag(xs_next, X, odo, dt, Q):
    Qd = np.asarray(Q, dtype=np.float64).astype(LD)
    Sp, Sr = np.sqrt(LD(dt) * Qd[0:3, 0:3]), np.sqrt(LD(dt) * Qd[3:6, 3:6])

    def r_of(j):
        z = LS.residual(xs_next[:, j], X, odo, dt, Q, LD)
        return np.vstack((Sp @ z[0:3], Sr @ z[3:6]))
    return r_of


def r_gauss(xs_next, mu, cov, rows, angle_rows=()):
    n = len(tuple(rows))
    L = dm.chol(np.asarray(cov, dtype=np.float64).astype(LD).reshape(n, n))
    return lambda j: L @ S.residual(xs_next[:, j], mu, cov, rows, angle_rows, LD)


def r_pose(xs_next, mu, rows, angle_rows, quat_rows):
    return lambda j: P.residual_vector(xs_next[:, j], mu, rows, angle_rows, quat_rows, LD)


def r_of_probe(p):
    """The residuals of (possibly modified) probe inputs of marginal_smoother_ref.probe / .sweep."""
    if p["kind"] == "mag":
        return r_mag(p["xs_next"], p["X"], p["odo"], p["dt"], p["Q"])
    if p["quat_rows"] is not None:
        return r_pose(p["xs_next"], p["mu"], p["rows"], p["angle_rows"], p["quat_rows"])
    return r_gauss(p["xs_next"], p["mu"], p["cov"], p["rows"], p["angle_rows"])


def r_of_case(c, xs_next, mu, cov):
    """For a device_map_smoother_ref.Case or a pose_transition_ref.PoseCase."""
    if getattr(c, "quat_rows", None):
        return r_pose(xs_next, mu, c.rows, c.angle_rows, c.quat_rows)
    return r_gauss(xs_next, mu, cov, c.rows, c.angle_rows)


# ---- xi and its moments ----------------------------------------------------------------------------------------------------
def log_mass(lws):
    """log sum_i exp(lws(i)); -inf if every entry is -inf."""
    return G.lse(np.asarray(lws, dtype=LD), axis=0)


def xi_column(logw, cj, lp_j, lmass):
    """xi(:, j) [N] long double; exactly 0 where log w(i) or c(j) is -inf or the mass is 0."""
    logw = np.asarray(logw, dtype=LD)
    if not (cj > -np.inf and lmass > -np.inf):
        return np.zeros(logw.shape, dtype=LD)
    live = logw > -np.inf
    out = np.zeros(logw.shape, dtype=LD)
    out[live] = np.exp(logw[live] + LD(cj) + np.asarray(lp_j, dtype=LD)[live] - LD(lmass))
    return out


def xi_matrix(logw, c, lp, lmass):
    """xi [N x M] (tiny problems only)."""
    return np.stack([xi_column(logw, c[j], lp[:, j], lmass) for j in range(len(c))], axis=1)


def moments(logw, c, lp, lmass, r_of):
    """(S [n x n], m [n], pair_mass), long double, one successor at a time."""
    S_, m_, pm = None, None, LD(0.0)
    for j in range(len(c)):
        r = r_of(j)
        if S_ is None:
            S_, m_ = np.zeros((r.shape[0], r.shape[0]), dtype=LD), np.zeros(r.shape[0], dtype=LD)
        xi = xi_column(logw, c[j], lp[:, j], lmass)
        if not np.any(xi > 0):
            continue
        rx = r * xi[None, :]
        S_ += rx @ r.T
        m_ += np.sum(rx, axis=1)
        pm += np.sum(xi)
    return S_, m_, pm


def step(logw, lp, logws_next, r_of):
    """One step: marginal_smoother_ref.step, the step's own mass, the moments -> dict(D, c, lws, mass, S, m, pair_mass)."""
    D, c, lws = G.step(logw, lp, logws_next)
    lmass = log_mass(lws)
    S_, m_, pm = moments(logw, c, lp, lmass, r_of)
    return dict(D=D, c=c, lws=lws, mass=np.exp(lmass), S=S_, m=m_, pair_mass=pm)


def recursion(X, W, lp_of, r_of_t):
    """marginal_smoother_ref.recursion and the moments of every pair of steps: lp_of(t) -> [N x N], r_of_t(t) -> r_of.  Adds S
    [T-1 x n x n], m [T-1 x n], pair_mass [T-1] to its dict."""
    lps = {}

    def lp_cached(t):
        if t not in lps:
            lps[t] = lp_of(t)
        return lps[t]
    res = G.recursion(X, W, lp_cached)
    T = X.shape[0]
    Ss, ms, pms = [], [], []
    for t in range(T - 1):
        logw = V.log_weights(W[t])
        D, lwn = res["D"][t], res["logws"][t + 1]
        ok = (lwn > -np.inf) & (D > -np.inf)
        c = np.where(ok, np.where(ok, lwn, LD(0.0)) - np.where(ok, D, LD(0.0)), LD(-np.inf))
        S_, m_, pm = moments(logw, c, lp_cached(t), np.log(res["mass"][t]), r_of_t(t))
        Ss.append(S_), ms.append(m_), pms.append(pm)
    res.update(S=np.stack(Ss), m=np.stack(ms), pair_mass=np.array(pms, dtype=LD))
    return res


def path_law_pairs(lw, lps):
    """The two-slice marginals of the backward-simulation path law by enumeration of all N^T paths (the path law of
    marginal_smoother_ref.path_law_marginals): lw [T x N] log weights, lps[t] [N x N] -> (one [T x N], two [T-1 x N x N]), long double."""
    import itertools
    T, N = lw.shape
    w = np.exp(np.asarray(lw, dtype=LD))
    B = []
    for t in range(T - 1):
        F = w[t][:, None] * np.exp(np.asarray(lps[t], dtype=LD))           # F[i, j] = w_t(i) p(j | i)
        B.append(F / np.sum(F, axis=0, keepdims=True))
    one, two = np.zeros((T, N), dtype=LD), np.zeros((max(T - 1, 0), N, N), dtype=LD)
    for path in itertools.product(range(N), repeat=T):
        p = w[T - 1, path[T - 1]]
        for t in range(T - 1):
            p = p * B[t][path[t], path[t + 1]]
        for t in range(T):
            one[t, path[t]] += p
        for t in range(T - 1):
            two[t, path[t], path[t + 1]] += p
    return one, two


# ---- the three families on forward arrays -------------------------------------------------------------------------------------
def run_mag(c, X, W):
    T = X.shape[0]
    dt, Q = V.pages(c, T)
    return recursion(X, W, lambda t: V.lp_mag(X[t + 1], X[t], c["odometry"][t], dt[t], Q[:, :, t]),
                     lambda t: r_mag(X[t + 1], X[t], c["odometry"][t], dt[t], Q[:, :, t]))


def run_case(c, X, W, mus=None):
    ref_mus, covs = S.transition_arrays(c, X)
    mus = ref_mus if mus is None else mus
    return recursion(X, W, lambda t: V.lp_case(c, X[t + 1], mus[t], covs[t]), lambda t: r_of_case(c, X[t + 1], mus[t], covs[t]))


def run_landmark(p, X, W):
    cov = p["dt"] * np.atleast_2d(np.asarray(p["Q"], dtype=np.float64))
    mu = lambda t: X[t] + np.asarray(p["odometry"][t], dtype=np.float64).reshape(3, 1)      # noqa: E731
    return recursion(X, W, lambda t: V.lp_gauss(X[t + 1], mu(t), cov, (0, 1, 2)), lambda t: r_gauss(X[t + 1], mu(t), cov, (0, 1, 2)))


# ---- the committed cases ---------------------------------------------------------------------------------------------------
PROBE_SHAPES = G.PROBE_SHAPES
PROBE_FAMILIES = G.PROBE_FAMILIES
FULL_RUNS = G.FULL_RUNS
# more than 256 workgroups in the statistics pass (17 predecessor blocks x 17 successor chunks): the reducer's strided loop; for the
# cheapest Gaussian family only (C: n_res = 1), so that the long-double reference stays affordable
BIG = ("C", 4352, 4352)

_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _with_moments(p):
    p = dict(p)
    lmass = log_mass(p["lws"])
    p["mass"] = np.exp(lmass)
    p["S"], p["m"], p["pair_mass"] = moments(p["logw"], p["c"], p["lp"], lmass, r_of_probe(p))
    return p


def probe(family, N, M):
    """marginal_smoother_ref.probe(family, N, M) with mass, S, m, pair_mass of the restatement; computed once."""
    return _once(("probe", family, N, M), lambda: _with_moments(G.probe(family, N, M)))


def sweep(name):
    """marginal_smoother_ref.sweep(name) (layout `name` of transition_sweep_ref, 300 x 70) with the restatement's moments, S and m in
    the caller's residual order."""
    return _once(("sweep", name), lambda: _with_moments(G.sweep(name)))


def groups(N, M):
    """(predecessor blocks, successor chunks) of the statistics pass: its workgroups."""
    return (N + 255) // 256, G.chunks(M, N)[1]
