"""Checker of the marginal smoothing weights of the localisation filters (forward filtering, backward smoothing: Doucet, Godsill &
Andrieu 2000): a restatement in numpy, every sum in np.longdouble and in the log domain,

    w_{T-1|T}(i) = w_{T-1}(i)
    D_t(j)       = log sum_l w_t(l) p(X[t+1][:, j] | X[t][:, l])
    c_t(j)       = log w_{t+1|T}(j) - D_t(j)            (-inf where log w_{t+1|T}(j) or D_t(j) is -inf: nothing is passed back)
    lws_t(i)     = log w_t(i) + log sum_j exp(c_t(j) + logp(X[t+1][:, j] | X[t][:, i]))
    mass_t       = sum_i exp(lws_t(i)),      log w_{t|T}(i) = lws_t(i) - log(mass_t)

logp is taken from the checkers of the three map families through tests/map_trajectory_ref.py (lp_mag, lp_gauss, lp_pose, lp_case),
not restated; the probe inputs are those of map_trajectory_ref.probe (its `delta` serves as log w_t) and of the 25 layouts of
tests/transition_sweep_ref.py, with seeded log w_{t+1|T} drawn here.  tests/test_marginal_smoother_cpu.py checks this restatement
against the marginals of the backward-simulation path law, enumerated over all paths.

Nothing in the package imports this file."""
import numpy as np

import map_trajectory_ref as V
import transition_sweep_ref as TS

LD = np.longdouble
NEG = LD(-np.inf)


def lse(a, axis):
    """log sum exp along `axis` in long double; -inf where every entry is -inf."""
    a = np.asarray(a, dtype=LD)
    m = np.max(a, axis=axis, keepdims=True)
    fin = m > -np.inf
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.sum(np.where(fin, np.exp(a - np.where(fin, m, LD(0.0))), LD(0.0)), axis=axis, keepdims=True)
        out = np.where(fin, m + np.log(np.where(fin, s, LD(1.0))), NEG)
    return np.squeeze(out, axis=axis)


def step(logw, lp, logws_next):
    """One backward step: logw [N], lp [N x M] (lp[i, j] = logp(successor j | predecessor i)), logws_next [M] -> (D [M], c [M],
    lws [N] un-normalised), long double."""
    logw, lp, logws_next = np.asarray(logw, dtype=LD), np.asarray(lp, dtype=LD), np.asarray(logws_next, dtype=LD)
    D = lse(logw[:, None] + lp, axis=0)
    ok = (logws_next > -np.inf) & (D > -np.inf)
    with np.errstate(invalid="ignore"):
        c = np.where(ok, np.where(ok, logws_next, LD(0.0)) - np.where(ok, D, LD(0.0)), NEG)
    lws = lse(logw[:, None] + c[None, :] + lp, axis=1)
    return D, c, lws


def moments(X, w):
    """X [n x N], w [N] -> (mean [n], cov [n x n], ess), plain weighted moments in long double."""
    X, w = np.asarray(X, dtype=np.float64).astype(LD), np.asarray(w, dtype=LD)
    mean = X @ w
    d = X - mean[:, None]
    return mean, (d * w[None, :]) @ d.T, LD(1.0) / np.sum(w * w)


def recursion(X, W, lp_of):
    """The whole recursion on forward arrays X [T x n x N] and W [T x N]; lp_of(t) -> [N x N] long double, lp[i, j] =
    logp(X[t+1][:, j] | X[t][:, i]).  Returns dict(logws [T x N], w_smooth [T x N], mass [T], mean [T x n], cov [T x n x n],
    ess [T], D [T-1 x N]), long double."""
    X, W = np.asarray(X, dtype=np.float64), np.asarray(W, dtype=np.float64)
    T, n, N = X.shape
    logws, mass = np.zeros((T, N), dtype=LD), np.ones(T, dtype=LD)
    Ds = np.zeros((max(T - 1, 0), N), dtype=LD)
    logws[T - 1] = V.log_weights(W[T - 1])
    for t in range(T - 2, -1, -1):
        Ds[t], _, lws = step(V.log_weights(W[t]), lp_of(t), logws[t + 1])
        with np.errstate(divide="ignore"):
            mass[t] = np.sum(np.exp(lws))
            logws[t] = np.where(lws > -np.inf, lws - np.log(mass[t]), NEG)
    w_smooth = np.exp(logws)
    w_smooth[T - 1] = W[T - 1]
    mean, cov, ess = np.zeros((T, n), dtype=LD), np.zeros((T, n, n), dtype=LD), np.zeros(T, dtype=LD)
    for t in range(T):
        mean[t], cov[t], ess[t] = moments(X[t], w_smooth[t])
    return dict(logws=logws, w_smooth=w_smooth, mass=mass, mean=mean, cov=cov, ess=ess, D=Ds)


def path_law_marginals(lw, lps):
    """The marginals of the backward-simulation path law by enumeration of all N^T paths, in the linear domain:
    P(path) = w_{T-1}(i_{T-1}) prod_t w_t(i_t) p(i_{t+1} | i_t) / D_t(i_{t+1}),  D_t(j) = sum_l w_t(l) p(j | l).
    lw [T x N] log weights, lps[t] [N x N] -> [T x N] long double."""
    import itertools
    T, N = lw.shape
    w = np.exp(np.asarray(lw, dtype=LD))
    B = []
    for t in range(T - 1):
        F = w[t][:, None] * np.exp(np.asarray(lps[t], dtype=LD))           # F[i, j] = w_t(i) p(j | i)
        B.append(F / np.sum(F, axis=0, keepdims=True))
    out = np.zeros((T, N), dtype=LD)
    for path in itertools.product(range(N), repeat=T):
        p = w[T - 1, path[T - 1]]
        for t in range(T - 1):
            p = p * B[t][path[t], path[t + 1]]
        for t in range(T):
            out[t, path[t]] += p
    return out


def run_mag(c, X, W):
    T = X.shape[0]
    dt, Q = V.pages(c, T)
    return recursion(X, W, lambda t: V.lp_mag(X[t + 1], X[t], c["odometry"][t], dt[t], Q[:, :, t]))


def run_case(c, X, W, mus=None):
    """A Case / PoseCase on forward arrays; mus[t]: what the `mean` handle returned (default: the case's own statement)."""
    import device_map_smoother_ref as S
    ref_mus, covs = S.transition_arrays(c, X)
    mus = ref_mus if mus is None else mus
    return recursion(X, W, lambda t: V.lp_case(c, X[t + 1], mus[t], covs[t]))


def run_landmark(p, X, W):
    cov = p["dt"] * np.atleast_2d(np.asarray(p["Q"], dtype=np.float64))
    return recursion(X, W, lambda t: V.lp_gauss(X[t + 1], X[t] + np.asarray(p["odometry"][t], dtype=np.float64).reshape(3, 1), cov, (0, 1, 2)))


# ---- the committed cases ---------------------------------------------------------------------------------------------------
# map_trajectory_ref's shapes (300 x 70: two predecessor chunks and a ragged last tile; 513 x 257: two successor chunks; M != N),
# one pair alone, and nine chunks of 256 in both passes
PROBE_SHAPES = list(V.PROBE_SHAPES) + [(1, 1), (2304, 2304)]
PROBE_FAMILIES = V.PROBE_FAMILIES
FULL_RUNS = V.FULL_RUNS

_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def next_weights(seed, M):
    """Seeded log w_{t+1|T} [M]: normalised weights spread over a few units; from M = 64 on entries 3 and M - 2 are -inf."""
    rs = np.random.RandomState(seed)
    w = rs.random_sample(M) + 0.05
    with np.errstate(divide="ignore"):
        lw = np.log(w / np.sum(w)) - 3.0 * rs.random_sample(M)
    if M >= 64:
        lw[3] = -np.inf
        lw[M - 2] = -np.inf
    return lw


def probe(family, N, M):
    """map_trajectory_ref.probe(family, N, M) (inputs, `lp`) with logw = its delta, a seeded logws_next, and the restatement's
    D, c, lws; computed once."""
    def make():
        p = dict(V.probe(family, N, M))
        p["logw"] = p["delta"]
        p["logws_next"] = next_weights(4211 + N + 13 * M + sum(map(ord, family)), M)
        p["D"], p["c"], p["lws"] = step(p["logw"], p["lp"], p["logws_next"])
        return p
    return _once(("probe", family, N, M), make)


def sweep(name):
    """The base inputs of layout `name` of transition_sweep_ref (300 x 70) as a probe: dict(kind, mu, xs_next, cov, rows, angle_rows,
    quat_rows, logw = log w, logws_next, lp, D, c, lws)."""
    def make():
        q = TS.inputs(name)
        p = dict(kind="generic", **TS.probe_args(q))
        p["logw"] = q["delta"]
        p["lp"] = TS.reference(name)["logp_ld"]
        p["logws_next"] = next_weights(977 + TS.NAMES.index(name), TS.M)
        p["D"], p["c"], p["lws"] = step(p["logw"], p["lp"], p["logws_next"])
        return p
    return _once(("sweep", name), make)


def lp_of_probe(p):
    """The long-double logp matrix of (possibly modified) probe inputs."""
    if p["kind"] == "mag":
        return V.lp_mag(p["xs_next"], p["X"], p["odo"], p["dt"], p["Q"])
    if p["quat_rows"] is not None:
        return V.lp_pose(p["xs_next"], p["mu"], p["cov"], p["rows"], p["angle_rows"], p["quat_rows"])
    return V.lp_gauss(p["xs_next"], p["mu"], p["cov"], p["rows"], p["angle_rows"])


def chunks(N, M):
    """(chunk size, chunks) of backward_chunk_size(N, M): the N side in chunks, the M side in blocks of 256."""
    bx = (M + 255) // 256
    want = max(1, (1024 + bx - 1) // bx)
    C = min(max(((N + want - 1) // want + 255) // 256 * 256, 256), 2048)
    return C, (N + C - 1) // C

