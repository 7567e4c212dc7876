"""Checker of the MAP trajectory of the localisation filters (MAP sequence estimation over the stored particles: Godsill, Doucet &
West 2001): a restatement of the Viterbi recursion in numpy, scores in np.longdouble,

    delta_0(j)     = log w_0(j)
    delta_{t+1}(j) = log w_{t+1}(j) + max_i [ delta_t(i) + logp(X[t+1][:, j] | X[t][:, i]) ],   psi_{t+1}(j) = the arg max
    i_{T-1} = arg max_j delta_{T-1}(j),   i_t = psi_{t+1}(i_{t+1}),   score = delta_{T-1}(i_{T-1})

the lowest index among equals at every max (np.argmax), psi = 0 where delta = -inf.  logp is taken from the checkers of the three
map families, not restated: localization_smoother_ref.logp (the dense-mag map), device_map_smoother_ref.logp (Gaussian transitions)
and pose_transition_ref.logp (a quaternion block), each evaluated in long double on the fp64 inputs.

THE NEAR-BEST SET.  For every (t, j) the restatement also returns {i : s_i >= best - tau}, tau = 2e-9 max(1, |best|): twice the
project's 1e-9 tolerance, applied to delta.  Two candidates can change order on the device only when they are closer than that, so
the device's arg must lie inside the set and equal it where the set is a singleton.  THE CAP: in every committed case at most 1 % of
the (t, j) entries have a near-best set with more than one DISTINCT particle (bit-identical predecessor columns with equal delta
count as one: an exact tie, which the lowest-index rule decides the same way everywhere), and no entry on the restatement's own
optimal path, the last arg max included, is such an entry.  tests/test_map_trajectory_cpu.py asserts it on the restatement's
forward pass of every case, the GPU tests assert it again on the device's own forward arrays.

Nothing in the package imports this file."""
import numpy as np

import device_map_smoother_ref as S
import localization_ref as R
import localization_smoother_ref as LS
import pose_transition_ref as P

LD = np.longdouble
TAU = 2e-9


def log_weights(w):
    w = np.asarray(w, dtype=np.float64).astype(LD)
    with np.errstate(divide="ignore"):
        return np.log(w)


def step(delta, lp):
    """One max-plus step: delta [N] and lp [N x M] (long double) -> (best [M], arg [M], near: a list of M index arrays)."""
    with np.errstate(invalid="ignore"):
        s = np.asarray(delta, dtype=LD)[:, None] + np.asarray(lp, dtype=LD)
        best = np.max(s, axis=0)
        arg = np.where(best > -np.inf, np.argmax(s, axis=0), 0)
        tau = LD(TAU) * np.maximum(LD(1.0), np.abs(best))
        bound = np.where(best > -np.inf, best - tau, -np.inf)
        near = [np.nonzero(s[:, j] >= bound[j])[0] for j in range(s.shape[1])]
    return best, arg.astype(np.int64), near


def _distinct(cols):
    """How many distinct columns an array has, bit for bit."""
    return len({c.tobytes() for c in np.ascontiguousarray(cols.T)})


def recursion(X, W, lp_of):
    """The whole recursion on forward arrays X [T x n x N] (as propagated) and W [T x N] (normalised); lp_of(t) -> [N x N] long
    double, lp[i, j] = logp(X[t+1][:, j] | X[t][:, i]).  Returns dict(delta [T x N], psi [T x N], path [T], score, near {(t, j):
    indices i of step t-1}, multi [T x N] bool: the near-best set of (t, j) holds more than one distinct particle, frac: their share
    of the (t, j) entries, t >= 1, on_path: such an entry lies on the optimal path (the last arg max included))."""
    X, W = np.asarray(X, dtype=np.float64), np.asarray(W, dtype=np.float64)
    T, _, N = X.shape
    delta, psi = np.zeros((T, N), dtype=LD), np.zeros((T, N), dtype=np.int64)
    multi, near = np.zeros((T, N), dtype=bool), {}
    delta[0] = log_weights(W[0])
    for t in range(T - 1):
        best, arg, nr = step(delta[t], lp_of(t))
        with np.errstate(invalid="ignore"):
            delta[t + 1] = np.where(best > -np.inf, log_weights(W[t + 1]) + best, -np.inf)
        psi[t + 1] = np.where(delta[t + 1] > -np.inf, arg, 0)
        hi = delta[t].astype(np.float64)                                   # delta_t as two doubles: equal pairs = equal long doubles
        lo = np.where(np.isfinite(hi), delta[t] - np.where(np.isfinite(hi), hi, 0.0), 0.0).astype(np.float64)
        key = np.vstack((X[t], hi[None], lo[None]))
        for j in range(N):
            near[(t + 1, j)] = nr[j]
            multi[t + 1, j] = nr[j].size > 1 and _distinct(key[:, nr[j]]) > 1
    path = np.zeros(T, dtype=np.int64)
    path[T - 1] = int(np.argmax(delta[T - 1]))
    for t in range(T - 1, 0, -1):
        path[t - 1] = psi[t, path[t]]
    score = delta[T - 1, path[T - 1]]
    last = np.nonzero(delta[T - 1] >= score - LD(TAU) * max(LD(1.0), abs(score)))[0]
    on_path = bool(last.size > 1 or any(multi[t, path[t]] for t in range(1, T)))
    return dict(delta=delta, psi=psi, path=path, score=score, near=near, multi=multi, frac=float(np.mean(multi[1:])) if T > 1 else 0.0,
                on_path=on_path)


def brute_force(lw, lps):
    """The best of all N^T paths by enumeration: lw [T x N] log weights, lps[t] [N x N] -> (path, score), the sums in the order of
    the recursion."""
    import itertools
    T, N = lw.shape
    best, arg = None, None
    for path in itertools.product(range(N), repeat=T):
        s = lw[0, path[0]]
        for t in range(T - 1):
            s = lw[t + 1, path[t + 1]] + (s + lps[t][path[t], path[t + 1]])
        if best is None or s > best:
            best, arg = s, path
    return np.array(arg, dtype=np.int64), best


# ---- logp of the three families, as [N x M] long-double matrices ---------------------------------------------------------------
def lp_mag(xs_next, X, odo, dt, Q):
    return np.stack([LS.logp(xs_next[:, j], X, odo, dt, Q, LD) for j in range(xs_next.shape[1])], axis=1)


def lp_gauss(xs_next, mu, cov, rows, angle_rows=()):
    return np.stack([S.logp(xs_next[:, j], mu, cov, rows, angle_rows, LD) for j in range(xs_next.shape[1])], axis=1)


def lp_pose(xs_next, mu, cov, rows, angle_rows, quat_rows):
    return np.stack([P.logp(xs_next[:, j], mu, cov, rows, angle_rows, quat_rows, LD) for j in range(xs_next.shape[1])], axis=1)


def lp_case(c, xs_next, mu, cov):
    """logp for a device_map_smoother_ref.Case or a pose_transition_ref.PoseCase."""
    if getattr(c, "quat_rows", None):
        return lp_pose(xs_next, mu, cov, c.rows, c.angle_rows, c.quat_rows)
    return lp_gauss(xs_next, mu, cov, c.rows, c.angle_rows)


def pages(c, T):
    """(dt [T], Q [6 x 6 x T]) of a dense-mag case, as particleFilterLocalization.m:66-73 expands them."""
    Q = np.asarray(c["Q"], dtype=np.float64)
    Q = np.repeat(Q[:, :, None], T, axis=2) if Q.ndim == 2 else Q
    dt = np.atleast_1d(np.asarray(c["dt"], dtype=np.float64)).ravel()
    return (dt[0] * np.ones(T) if dt.size == 1 else dt), Q


def run_mag(c, X, W):
    T = X.shape[0]
    dt, Q = pages(c, T)
    return recursion(X, W, lambda t: lp_mag(X[t + 1], X[t], c["odometry"][t], dt[t], Q[:, :, t]))


def run_case(c, X, W, mus=None):
    """A Case / PoseCase on forward arrays; mus[t]: what the `mean` handle returned (default: the case's own statement)."""
    ref_mus, covs = S.transition_arrays(c, X)
    mus = ref_mus if mus is None else mus
    return recursion(X, W, lambda t: lp_case(c, X[t + 1], mus[t], covs[t]))


def run_landmark(p, X, W):
    """A landmark_map_ref problem with the additive transition of its dynModel: mean = x + odometry[t], cov = dt Q, all three rows."""
    cov = p["dt"] * np.atleast_2d(np.asarray(p["Q"], dtype=np.float64))
    return recursion(X, W, lambda t: lp_gauss(X[t + 1], X[t] + np.asarray(p["odometry"][t], dtype=np.float64).reshape(3, 1), cov, (0, 1, 2)))


# ---- forward passes of the restatements ------------------------------------------------------------------------------------
def forward_mag(c):
    """localization_smoother_ref.forward_arrays for a case whose dt and Q may come in pages."""
    ref = R.run_case(c)
    T, N = ref["w"].shape
    dt, Q = pages(c, T)
    x0 = np.asarray(c["x0_nonLin"], dtype=np.float64)
    X = np.zeros((T, 7, N))
    X[0] = x0.reshape(7, -1) if x0.ndim > 1 and x0.shape[1] > 1 else np.repeat(x0.reshape(7, 1), N, axis=1)
    for t in range(1, T):
        for i in range(N):
            X[t][:, i] = R.dyn_model(X[t - 1][:, ref["ai"][t, i]], c["odometry"][t - 1], dt[t - 1], Q[:, :, t - 1], c["Z"][t - 1, i, :])
    return X, np.asarray(ref["w"], dtype=np.float64)


def forward_landmark(p):
    import landmark_map_ref as lm
    ref = lm.run(p)
    T, N = ref["w"].shape
    X = np.zeros((T, 3, N))
    X[0] = np.repeat(np.asarray(p["x0_nonLin"], dtype=np.float64).reshape(3, 1), N, axis=1)
    Z = p["rng"].Z[0]
    for t in range(1, T):
        X[t] = lm.dyn(p, X[t - 1][:, ref["ai"][t]], t - 1, Z[t - 1])
    return X, np.asarray(ref["w"], dtype=np.float64)


# ---- the committed cases ---------------------------------------------------------------------------------------------------
N_P, N_T = 300, 7
PROBE_SHAPES = [(300, 70), (513, 257), (1, 5)]            # (300, 70): two chunks and a partial tile
# mag: BsTerm; C, D, B: GsTerm at n_res = 1 (an angle row), 3 (one angle row), 8; pose0 / pose3 / pose4: a block behind 0, 3, 4 plain rows
PROBE_FAMILIES = ("mag", "C", "D", "B", "pose0", "pose3", "pose4")
# (kind, name): the full runs.  mag_pages: dt and Q in pages, one per step.  Every DeviceMap case starts from one x0 column: step 0
# ties in every entry.
FULL_RUNS = [("mag", "plain"), ("mag", "pages"), ("gauss", "A"), ("gauss", "D"), ("pose", "E"), ("landmark", "ro")]
LANDMARK = ("ro", 6, N_P, N_T, 2)                          # (kind, landmarks, N_P, N_T, seed) of landmark_map_ref.case

_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def pose_probe(n_plain, N, M, seed=11):
    """Inputs of one step for a quaternion block behind n_plain plain rows (all rows selected, the block last; with 4 plain rows,
    row 1 is an angle near pi): N predecessors two standard deviations of the noise around a centre, mu their predicted rows, M
    successors drawn from random predecessors."""
    rs = np.random.RandomState(1000 * seed + 31 * n_plain + N + 7 * M)
    n_res, nN = n_plain + 3, n_plain + 4
    cov = P._spd(rs, np.concatenate((0.15 * np.ones(n_plain), 0.04 * np.ones(3))))
    Lc = np.linalg.cholesky(cov)
    rows, quat_rows = tuple(range(nN)), tuple(range(n_plain, nN))
    angle_rows = (1,) if n_plain == 4 else ()
    n = 2.0 * (Lc @ rs.standard_normal((n_res, N)))
    mu = np.zeros((nN, N))
    mu[:n_plain] = rs.uniform(-1.0, 1.0, (n_plain, 1)) + n[:n_plain]
    for a in angle_rows:
        mu[a] = S.wrap(mu[a] + 3.1 - np.mean(mu[a]))
    mu[n_plain:] = P.qmul(P.expq(0.4 * rs.standard_normal(3)).reshape(4, 1) * np.ones((1, N)), P.expq(n[n_plain:]))
    pick = rs.randint(N, size=M)
    z = Lc @ rs.standard_normal((n_res, M))
    xs = np.zeros((nN, M))
    xs[:n_plain] = mu[:n_plain, pick] + z[:n_plain]
    for a in angle_rows:
        xs[a] = S.wrap(xs[a])
    xs[n_plain:] = P.qmul(mu[n_plain:, pick], P.expq(z[n_plain:]))
    return dict(mu=mu, xs_next=xs, cov=cov, rows=rows, angle_rows=angle_rows, quat_rows=quat_rows)


def probe(family, N, M):
    """Inputs of one step of `family` and the restatement's answer, computed once: dict(args for the probe wrapper, delta, best, arg,
    near).  delta = log w minus a random spread of a few units; from N = 64 on the first and the last ten are -inf (w = 0)."""
    def make():
        rs = np.random.RandomState(977 + N + 7 * M + sum(map(ord, family)))
        if family == "mag":
            p = LS.probe_case(N, M)
            w = p["w"]
            lp = lp_mag(p["xs_next"], p["X"], p["odo"], p["dt"], p["Q"])
            out = dict(kind="mag", X=p["X"], xs_next=p["xs_next"], odo=p["odo"], dt=p["dt"], Q=p["Q"])
        elif family.startswith("pose"):
            p = pose_probe(int(family[4:]), N, M)
            w = rs.random_sample(N) + 0.05
            if N >= 64:
                w[:10] = 0.0
                w[-10:] = 0.0
            lp = lp_pose(p["xs_next"], p["mu"], p["cov"], p["rows"], p["angle_rows"], p["quat_rows"])
            out = dict(kind="generic", **p)
        else:
            p = S.probe_case(family, N, M)
            w = p["w"]
            lp = lp_gauss(p["xs_next"], p["mu"], p["cov"], p["rows"], p["angle_rows"])
            out = dict(kind="generic", mu=p["mu"], xs_next=p["xs_next"], cov=p["cov"], rows=p["rows"], angle_rows=p["angle_rows"], quat_rows=None)
        with np.errstate(divide="ignore"):
            delta = np.log(w / np.sum(w)) - 3.0 * rs.random_sample(N)
        out["delta"] = delta
        out["lp"] = lp
        out["best"], out["arg"], out["near"] = step(delta, lp)
        return out
    return _once(("probe", family, N, M), make)


def mag_case(name):
    def make():
        c = dict(R.loc_case(N_P, N_T, 13))
        if name == "pages":
            rs = np.random.RandomState(88)
            c["dt"] = 0.01 * rs.uniform(0.7, 1.4, N_T)
            c["Q"] = np.stack([np.asarray(c["Q"]) * f for f in rs.uniform(0.6, 1.6, N_T)], axis=2)
        return c
    return _once(("mag", name), make)


def landmark_case():
    import landmark_map_ref as lm
    kind, L, N, T, seed = LANDMARK
    return _once(("landmark",), lambda: lm.case(kind, L, N, T, seed))


def full_case(kind, name):
    if kind == "mag":
        return mag_case(name)
    if kind == "gauss":
        return S.case(name, N_P, N_T)
    if kind == "pose":
        return P.case(name, N_P, N_T)
    return landmark_case()


def full_reference(kind, name):
    """The restatement's own forward pass of a committed case and its recursion: (X, W, result), computed once."""
    def make():
        c = full_case(kind, name)
        if kind == "mag":
            X, W = forward_mag(c)
            return X, W, run_mag(c, X, W)
        if kind == "landmark":
            X, W = forward_landmark(c)
            return X, W, run_landmark(c, X, W)
        X, W, _ = S.forward_arrays(c)
        return X, W, run_case(c, X, W)
    return _once(("ref", kind, name), make)


def cap_ok(res):
    """The cap: at most 1 % of the entries near-tied between distinct particles, none of them on the optimal path."""
    return res["frac"] <= 0.01 and not res["on_path"]
