"""Checker of the fixed-lag smoother (LocalizationSession.fixed_lag_estimates, csrc/rbpf_loc_fixedlag.hpp) restated in numpy, every sum
in np.longdouble, twice:

  direct()     the DEFINITION: for every horizon t the backward FFBSm recursion of marginal_smoother_ref on the steps 0 .. t alone,
               and est(l, t) = sum_i w_{t-l | t}(i) h_{t-l}(X[t-l][:, i]) -- the moments of step t - l under the smoothed weights
               of a run that ended at t.  Nothing of the forward recursion is used.
  recursion()  the forward-only recursion under test:
                   T0_t(i)          = h_t(X[t][:, i])
                   T^(l)_{t+1}(j)   = sum_i omega_t(i, j) T^(l-1)_t(i),   l = 1 .. L        (step())
                   est(l, t+1)      = sum_j w_{t+1}(j) T^(l)_{t+1}(j),    mass(t+1) = sum_j w_{t+1}(j) sum_i omega_t(i, j)
               omega_t(i, j) = exp(log w_t(i) + logp(j | i) - D_t(j)), D from marginal_smoother_ref.step with logws_next = 0.

h_s(x) over all n state rows, d = x - c_s, c_s the filter mean of step s: moments = 1: d [n]; moments = 2: d, then the lower triangle
by rows of d d' [n (n + 3) / 2].  lp comes from the three families' checkers through marginal_smoother_ref / map_trajectory_ref; the
probe and sweep inputs are forward_stats_ref's (marginal_smoother_ref's with a seeded carry).

Nothing in the package imports this file."""
import numpy as np

import device_map_smoother_ref as S
import forward_stats_ref as FS
import map_trajectory_ref as V
import marginal_smoother_ref as G

LD = np.longdouble
KB = 32                                                                    # kFixedLagKB of csrc/rbpf_loc_fixedlag.hpp


def columns(n, moments):
    return n if moments == 1 else n * (n + 3) // 2


def h_of(X, c, moments):
    """X [n x N] (fp64), c [n] -> h [H x N], long double."""
    d = np.asarray(X, dtype=np.float64).astype(LD) - np.asarray(c, dtype=LD)[:, None]
    if moments == 1:
        return d
    n = d.shape[0]
    return np.vstack([d] + [d[p] * d[q] for p in range(n) for q in range(p + 1)])


def filter_mean(X, w):
    return np.asarray(X, dtype=np.float64).astype(LD) @ np.asarray(w, dtype=np.float64).astype(LD)


def step(logw, lp, tau):
    """The shift of one step: logw [N], lp [N x M], tau [K x N] -> dict(D [M], tau [K x M], reach [M]), long double.  A predecessor
    with log w = -inf contributes exactly nothing, whatever it carries; a successor that no predecessor reaches (D = -inf) gets
    zeros."""
    logw, lp, tau = np.asarray(logw, dtype=LD), np.asarray(lp, dtype=LD), np.atleast_2d(np.asarray(tau, dtype=LD))
    N, M = lp.shape
    D = G.step(logw, lp, np.zeros(M))[0]
    out, reach = np.zeros((tau.shape[0], M), dtype=LD), np.zeros(M, dtype=LD)
    for j in range(M):
        live = np.nonzero((logw > -np.inf) & (lp[:, j] > -np.inf))[0]
        if not (D[j] > -np.inf) or live.size == 0:
            continue
        w = np.exp(logw[live] + lp[live, j] - D[j])
        out[:, j] = tau[:, live] @ w
        reach[j] = np.sum(w)
    return dict(D=D, tau=out, reach=reach)


def _empty(T, n, lag, moments):
    H = columns(n, moments)
    return dict(est=np.full((T, lag + 1, H), np.nan, dtype=LD), c=np.zeros((T, n), dtype=LD), mass=np.ones(T, dtype=LD),
                sd=np.zeros(T))


def _centres(X, W, out, c=None):
    for s in range(X.shape[0]):
        out["c"][s] = filter_mean(X[s], W[s]) if c is None else np.asarray(c, dtype=np.float64)[s].astype(LD)
        out["sd"][s] = float(np.max(np.abs(X[s].astype(LD) - out["c"][s][:, None])))


def direct(X, W, lp_of, lag, moments, c=None):
    """The definition on forward arrays X [T x n x N], W [T x N]; lp_of(t) -> [N x N]; c [T x n]: the centres to use instead of the
    restatement's own filter means (the device's, which are fp64 numbers: a centre is a constant of the functional).  Returns dict(est [T x (lag+1) x H] (NaN where
    t - l < 0), c [T x n], mass (ones), sd [T] = max |X[s] - c_s|), long double."""
    X, W = np.asarray(X, dtype=np.float64), np.asarray(W, dtype=np.float64)
    T, n, N = X.shape
    out = _empty(T, n, lag, moments)
    _centres(X, W, out, c)
    lps = {}

    def lp_once(t):
        if t not in lps:
            lps[t] = lp_of(t)
        return lps[t]
    for t in range(T):
        ws = G.recursion(X[:t + 1], W[:t + 1], lp_once)["w_smooth"]       # w_{s | t}, s = 0 .. t
        for l in range(min(lag, t) + 1):
            s = t - l
            out["est"][t, l] = h_of(X[s], out["c"][s], moments) @ ws[s]
    return out


def recursion(X, W, lp_of, lag, moments, c=None):
    """The forward-only recursion on the same arrays, the same dict; mass from the recursion, D [T-1 x N] and reach [T-1 x N] too."""
    X, W = np.asarray(X, dtype=np.float64), np.asarray(W, dtype=np.float64)
    T, n, N = X.shape
    H = columns(n, moments)
    out = _empty(T, n, lag, moments)
    _centres(X, W, out, c)
    out["D"], out["reach"] = [], []
    slots = [h_of(X[0], out["c"][0], moments)]                            # slots[l] = T^(l) of the current step
    out["est"][0, 0] = slots[0] @ W[0].astype(LD)
    for t in range(T - 1):
        keep = slots[:lag]
        res = step(V.log_weights(W[t]), lp_of(t), np.vstack(keep))
        moved = [res["tau"][k * H:(k + 1) * H] for k in range(len(keep))]
        slots = [h_of(X[t + 1], out["c"][t + 1], moments)] + moved
        w = W[t + 1].astype(LD)
        for l, Tl in enumerate(slots):
            out["est"][t + 1, l] = Tl @ w
        out["mass"][t + 1] = np.sum(res["reach"] * w)
        out["D"].append(res["D"]), out["reach"].append(res["reach"])
    return out


def moments_of(ref, l, t):
    """(mean [n], cov [n x n] or None) of step t - l at horizon t from a direct() / recursion() result."""
    e = ref["est"][t, l]
    n = ref["c"].shape[1]
    mean = ref["c"][t - l] + e[:n]
    if e.size == n:
        return mean, None
    cov, k = np.zeros((n, n), dtype=LD), n
    for p in range(n):
        for q in range(p + 1):
            cov[p, q] = cov[q, p] = e[k] - e[p] * e[q]
            k += 1
    return mean, cov


# ---- the three families on forward arrays -------------------------------------------------------------------------------------
def lp_mag(c, X):
    dt, Q = V.pages(c, X.shape[0])
    return lambda t: V.lp_mag(X[t + 1], X[t], c["odometry"][t], dt[t], Q[:, :, t])


def lp_case(c, X, mus=None):
    ref_mus, covs = S.transition_arrays(c, X)
    mus = ref_mus if mus is None else mus
    return lambda t: V.lp_case(c, X[t + 1], mus[t], covs[t])


def lp_landmark(p, X):
    cov = p["dt"] * np.atleast_2d(np.asarray(p["Q"], dtype=np.float64))
    return lambda t: V.lp_gauss(X[t + 1], X[t] + np.asarray(p["odometry"][t], dtype=np.float64).reshape(3, 1), cov, (0, 1, 2))


def run_mag(c, X, W, lag, moments, how=direct, centres=None):
    return how(X, W, lp_mag(c, X), lag, moments, centres)


def run_case(c, X, W, lag, moments, mus=None, how=direct, centres=None):
    return how(X, W, lp_case(c, X, mus), lag, moments, centres)


def run_landmark(p, X, W, lag, moments, how=direct, centres=None):
    return how(X, W, lp_landmark(p, X), lag, moments, centres)


def run_full(kind, c, X, W, lag, moments, mus=None, how=direct, centres=None):
    if kind == "mag":
        return run_mag(c, X, W, lag, moments, how, centres)
    if kind == "landmark":
        return run_landmark(c, X, W, lag, moments, how, centres)
    return run_case(c, X, W, lag, moments, mus, how, centres)


# ---- the committed cases ---------------------------------------------------------------------------------------------------
PROBE_SHAPES = FS.PROBE_SHAPES
PROBE_FAMILIES = FS.PROBE_FAMILIES
FULL_RUNS = FS.FULL_RUNS
chunks = FS.chunks                                                         # the pass's own rule: forward_stats_chunk(N, M)

_CACHE = {}


def tau_of(K, N, seed):
    """A seeded incoming carry [K x N]."""
    return np.random.RandomState(seed).standard_normal((K, N))


def probe(family, N, M, K):
    """forward_stats_ref.probe(family, N, M) with a seeded carry of K columns in `tau` and the restatement's step in `fl`; once."""
    key = ("probe", family, N, M, K)
    if key not in _CACHE:
        p = dict(FS.probe(family, N, M))
        p["tau"] = tau_of(K, N, 131 + N + 3 * M + 7 * K + sum(map(ord, family)))
        p["fl"] = step(p["logw"], p["lp"], p["tau"])
        _CACHE[key] = p
    return _CACHE[key]


def sweep(name, K=3):
    key = ("sweep", name, K)
    if key not in _CACHE:
        p = dict(FS.sweep(name))
        p["tau"] = tau_of(K, len(p["logw"]), 257 + sum(map(ord, name)))
        p["fl"] = step(p["logw"], p["lp"], p["tau"])
        _CACHE[key] = p
    return _CACHE[key]
