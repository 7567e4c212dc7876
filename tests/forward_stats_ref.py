"""Checker of the running two-slice statistics (LocalizationSession.running_statistics, csrc/rbpf_loc_forwardstats.hpp): the
forward-only form of FFBSm for an additive functional (Del Moral, Doucet & Singh 2010) restated in numpy, every sum in np.longdouble,

    D_t(j)       = log sum_i w_t(i) p(X[t+1][:, j] | X[t][:, i])                      (marginal_smoother_ref.step, logws_next = 0)
    omega(i, j)  = exp(log w_t(i) + logp(j | i) - D_t(j))                             (sums to 1 over i)
    tau_{t+1}(j) = sum_i omega(i, j) (tau_t(i) + s_t(i, j)),   tau_0 = 0,   s_t = [r r' s_scale; r],   s_scale = 1 / dt_t
    est_{t+1}    = sum_j w_{t+1}(j) tau_{t+1}(j),              mass_{t+1} = sum_j w_{t+1}(j) sum_i omega(i, j)

The un-whitened residual r_ij comes from pair_stats_ref.r_of_probe / r_of_case (which take it from the three families' checkers);
it is not restated here.  tau is kept as (tau_S [n x n x N], tau_m [n x N]) in the caller's residual order.  A successor is handled
at a time: nothing N x M x n is formed.

Nothing in the package imports this file."""
import numpy as np

import device_map_smoother_ref as S
import map_trajectory_ref as V
import marginal_smoother_ref as G
import pair_stats_ref as PS

LD = np.longdouble


def step(logw, lp, tau, r_of, s_scale):
    """One step: logw [N], lp [N x M], tau = (tau_S [n x n x N], tau_m [n x N]), r_of(j) -> [n x N] -> dict(D [M], tau_S [n x n x M],
    tau_m [n x M], reach [M]), long double.  A predecessor with log w = -inf contributes exactly nothing; a successor that no
    predecessor reaches (D = -inf) gets tau = 0 and reach = 0."""
    logw, lp = np.asarray(logw, dtype=LD), np.asarray(lp, dtype=LD)
    tS, tm = np.asarray(tau[0], dtype=LD), np.asarray(tau[1], dtype=LD)
    N, M = lp.shape
    n = tm.shape[0]
    D = G.step(logw, lp, np.zeros(M))[0]
    oS, om, reach = np.zeros((n, n, M), dtype=LD), np.zeros((n, M), dtype=LD), np.zeros(M, dtype=LD)
    for j in range(M):
        live = np.nonzero((logw > -np.inf) & (lp[:, j] > -np.inf))[0]
        if not (D[j] > -np.inf) or live.size == 0:
            continue
        w = np.exp(logw[live] + lp[live, j] - D[j])
        r = np.asarray(r_of(j), dtype=LD)[:, live]
        rw = r * w[None, :]
        oS[:, :, j] = np.sum(tS[:, :, live] * w[None, None, :], axis=2) + LD(s_scale) * (rw @ r.T)
        om[:, j] = np.sum(tm[:, live] * w[None, :], axis=1) + np.sum(rw, axis=1)
        reach[j] = np.sum(w)
    return dict(D=D, tau_S=oS, tau_m=om, reach=reach)


def estimate(w_next, res):
    """(S [n x n], m [n], mass) = sum_j w_next(j) (tau_S(:, :, j), tau_m(:, j), reach(j)), long double."""
    w = np.asarray(w_next, dtype=np.float64).astype(LD)
    return np.sum(res["tau_S"] * w[None, None, :], axis=2), np.sum(res["tau_m"] * w[None, :], axis=1), np.sum(res["reach"] * w)


def recursion(X, W, lp_of, r_of_t, dt):
    """The whole recursion on forward arrays X [T x n_state x N] and W [T x N]: lp_of(t) -> [N x N], r_of_t(t) -> r_of, dt [>= T-1].
    Returns dict(S_run [T-1 x n x n], m_run [T-1 x n], mass_run [T-1], D [T-1 x N], reach [T-1 x N], taus [T-1]: (tau_S, tau_m)
    after every step), long double."""
    X, W = np.asarray(X, dtype=np.float64), np.asarray(W, dtype=np.float64)
    T, N = W.shape
    tau, out = None, dict(S_run=[], m_run=[], mass_run=[], D=[], reach=[], taus=[])
    for t in range(T - 1):
        r_of = r_of_t(t)
        if tau is None:
            n = np.asarray(r_of(0)).shape[0]
            tau = (np.zeros((n, n, N), dtype=LD), np.zeros((n, N), dtype=LD))
        res = step(V.log_weights(W[t]), lp_of(t), tau, r_of, LD(1.0) / LD(dt[t]))
        tau = (res["tau_S"], res["tau_m"])
        S_, m_, mass = estimate(W[t + 1], res)
        out["S_run"].append(S_), out["m_run"].append(m_), out["mass_run"].append(mass)
        out["D"].append(res["D"]), out["reach"].append(res["reach"]), out["taus"].append(tau)
    for k in ("S_run", "m_run", "D", "reach"):
        out[k] = np.stack(out[k])
    out["mass_run"] = np.array(out["mass_run"], dtype=LD)
    return out


def steps_dt(dt, T):
    """dt of the steps 0 .. T-2 from a scalar or an array of at least T-1 entries."""
    dt = np.atleast_1d(np.asarray(dt, dtype=np.float64)).ravel()
    return np.full(max(T - 1, 1), dt[0]) if dt.size == 1 else dt[:T - 1]


# ---- the three families on forward arrays -------------------------------------------------------------------------------------
def run_mag(c, X, W):
    T = X.shape[0]
    dt, Q = V.pages(c, T)
    return recursion(X, W, lambda t: V.lp_mag(X[t + 1], X[t], c["odometry"][t], dt[t], Q[:, :, t]),
                     lambda t: PS.r_mag(X[t + 1], X[t], c["odometry"][t], dt[t], Q[:, :, t]), dt)


def run_case(c, X, W, mus=None):
    ref_mus, covs = S.transition_arrays(c, X)
    mus = ref_mus if mus is None else mus
    return recursion(X, W, lambda t: V.lp_case(c, X[t + 1], mus[t], covs[t]), lambda t: PS.r_of_case(c, X[t + 1], mus[t], covs[t]),
                     steps_dt(c.p["dt"], X.shape[0]))


def run_landmark(p, X, W):
    cov = p["dt"] * np.atleast_2d(np.asarray(p["Q"], dtype=np.float64))
    mu = lambda t: X[t] + np.asarray(p["odometry"][t], dtype=np.float64).reshape(3, 1)      # noqa: E731
    return recursion(X, W, lambda t: V.lp_gauss(X[t + 1], mu(t), cov, (0, 1, 2)), lambda t: PS.r_gauss(X[t + 1], mu(t), cov, (0, 1, 2)),
                     steps_dt(p["dt"], X.shape[0]))


# ---- the committed cases ---------------------------------------------------------------------------------------------------
# marginal_smoother_ref's shapes but its largest: 300 x 70 (a ragged successor block; 300 predecessors are two chunks of 256, the last
# tile partial at every tile depth), 513 x 257 (two successor blocks, three chunks), 1 x 5, 1 x 1; and 600 x 520: three chunks x three
# blocks, the cheapest shape with several of both (2304 x 2304 would cost the long-double restatement sixteen times as much)
PROBE_SHAPES = [s for s in G.PROBE_SHAPES if s != (2304, 2304)] + [(600, 520)]
PROBE_FAMILIES = G.PROBE_FAMILIES
FULL_RUNS = G.FULL_RUNS

_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def chunks(N, M):
    """(chunk size, chunks) of the carry pass's own rule, forward_stats_chunk(N, M): backward_chunk_size without its cap of 2048."""
    bx = (M + 255) // 256
    want = max(1, (1024 + bx - 1) // bx)
    C = max(((N + want - 1) // want + 255) // 256 * 256, 256)
    return C, (N + C - 1) // C


def carry(n, N, seed):
    """A seeded non-zero incoming carry: tau_S [n x n x N] symmetric, tau_m [n x N]."""
    rs = np.random.RandomState(seed)
    A = rs.standard_normal((n, n, N))
    return np.asfortranarray(A + A.transpose(1, 0, 2)), np.asfortranarray(rs.standard_normal((n, N)))


def scale_of(p):
    """s_scale of a probe: 1 / dt in the dense-mag map (its entry point takes dt), 0.7 elsewhere."""
    return 1.0 / float(p["dt"]) if p["kind"] == "mag" else 0.7


def _with_step(p, seed):
    p = dict(p)
    n = 6 if p["kind"] == "mag" else np.asarray(p["cov"]).shape[0]
    p["tau_S"], p["tau_m"] = carry(n, len(p["logw"]), seed)
    p["s_scale"] = scale_of(p)
    p["fs"] = step(p["logw"], p["lp"], (p["tau_S"], p["tau_m"]), PS.r_of_probe(p), p["s_scale"])
    return p


def probe(family, N, M):
    """marginal_smoother_ref.probe(family, N, M) with a seeded incoming carry, s_scale and the restatement's step in `fs`; once."""
    return _once(("probe", family, N, M), lambda: _with_step(G.probe(family, N, M), 31 + N + 3 * M + sum(map(ord, family))))


def sweep(name):
    """marginal_smoother_ref.sweep(name) (layout `name` of transition_sweep_ref, 300 x 70) the same way, in the caller's order."""
    return _once(("sweep", name), lambda: _with_step(G.sweep(name), 57 + sum(map(ord, name))))
