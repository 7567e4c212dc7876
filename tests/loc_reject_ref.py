"""Checker of backward simulation by rejection sampling (csrc/rbpf_loc_reject.hpp; Douc, Garivier, Moulines & Olsson 2011, with the
all-pairs pass as the fallback): a restatement in numpy on the logp and the draw of the three families' existing checkers.

    step T-1:      b[T-1][j] = sample(w[T-1], u[T-1][j])                                          (the existing draw)
    t = T-2 .. 0:  tries r = 0 .. R-1:  (u0, u1) = philox_ref.uniform2(seed, slot = j, step = t, lane = 0x42530001, iter = r)
                                        i = #{k : cdf_k < u0 cdf_{N-1}},  cdf = cumsum(w[t]) strictly left to right
                                        accept iff logp(xs[t+1][j] | X[t][:, i]) >= log u1        (logp without log w_i)
                   the first accepted i is b[t][j]; without one after R tries the existing restatement's draw with u[t][j]
                   (lane 0x42530000, iter 0): l = log w + logp, p = exp(l - lse(l)), sample(p, u)

Every statement runs in fp64 and in long double on the same fp64 inputs, and every decision reports its MARGIN next to the error it
must outweigh -- the restatement is its own arbiter:
    proposal   distance of u0 cdf_{N-1} (long double) from the nearest long-double cdf edge, against eps = max |cdf64 - cdf_ld| plus
               the distance of the two targets (localization_smoother_ref._draw measures its draws the same way);
    accept     |log u1 - logp_ld| of the proposed pair against the step's largest |logp64 - logp_ld| over all pairs;
    fallback   the margin and eps_ref of localization_smoother_ref._draw.
A fixture `holds` when every margin is at least 100 x its error measure and the fp64 and the long-double decisions agree everywhere
(conditions()); the GPU tests then compare every index, none left out.

n_fallback[t] = trajectories without an acceptance, n_tries[t] = tries made, summed over the trajectories; both 0 at step T-1.

Nothing in the package imports this file."""
import numpy as np

import localization_smoother_ref as LS
import philox_ref
import pose_transition_ref as P
import transition_sweep_ref as TS
from localization_smoother_ref import _draw, _log_weights, backward_cdf

LD = np.longdouble
REJECT_LANE = 0x42530001
FACTOR = 100.0                                 # every margin >= FACTOR x its error measure


# ---- one step ------------------------------------------------------------------------------------------------------------------
def step(lp64, lp_ld, w, u_try, u):
    """One step on logp matrices [N x M] (fp64 and long double), w [N], u_try(r, j) -> (u0, u1) for r < R (a callable with attribute
    R, or an array [R x M x 2]), u [M] the fallback's uniforms.  Returns dict(index, index_ld, accepted_at, accepted_at_ld [M],
    n_fallback, n_tries, prop = (margin, eps) and acc = (margin, err) over all tries made, fb = (margin, eps) over the fallback
    draws; long double)."""
    if not callable(u_try):
        arr = np.asarray(u_try, dtype=np.float64)
        R = arr.shape[0] if arr.size else 0
        draw = lambda r, j: (arr[r, j, 0], arr[r, j, 1])                                            # noqa: E731
    else:
        R, draw = u_try.R, u_try
    w = np.asarray(w, dtype=np.float64)
    N, M = lp64.shape
    cdf64, cdf_ld = np.cumsum(w), np.cumsum(w.astype(LD))
    eps_cdf = np.max(np.abs(cdf64.astype(LD) - cdf_ld))
    err_lp = np.max(np.abs(lp64.astype(LD) - lp_ld))
    lw, lw_ld = _log_weights(w, np.float64), _log_weights(w, LD)
    index, index_ld = np.zeros(M, dtype=np.int64), np.zeros(M, dtype=np.int64)
    acc, acc_ld = np.full(M, -1, dtype=np.int64), np.full(M, -1, dtype=np.int64)
    prop, accm, fb = [], [], []
    n_tries = 0
    for j in range(M):
        for r in range(R):
            if acc[j] >= 0 and acc_ld[j] >= 0:
                break
            u0, u1 = draw(r, j)
            t64, t_ld = np.float64(u0) * cdf64[-1], LD(u0) * cdf_ld[-1]
            i, i_ld = min(int(np.sum(cdf64 < t64)), N - 1), min(int(np.sum(cdf_ld < t_ld)), N - 1)
            prop.append((np.min(np.abs(cdf_ld - t_ld)), eps_cdf + abs(LD(t64) - t_ld)))
            b64, b_ld = np.log(np.float64(u1)), np.log(LD(u1))
            accm.append((abs(b_ld - lp_ld[i_ld, j]), err_lp))
            if acc[j] < 0:
                n_tries += 1
                if lp64[i, j] >= b64:
                    acc[j], index[j] = r, i
            if acc_ld[j] < 0 and lp_ld[i_ld, j] >= b_ld:
                acc_ld[j], index_ld[j] = r, i_ld
        if acc[j] < 0 or acc_ld[j] < 0:
            d = _draw(backward_cdf(lw + lp64[:, j]), backward_cdf(lw_ld + lp_ld[:, j]), np.asarray(u[j:j + 1], dtype=np.float64))
            if acc[j] < 0:
                index[j] = d[0][0]
            if acc_ld[j] < 0:
                index_ld[j] = d[1][0]
            fb.append((d[2][0], d[3][0]))
    pack = lambda v: (np.array([a for a, _ in v], dtype=LD), np.array([b for _, b in v], dtype=LD))   # noqa: E731
    return dict(index=index, index_ld=index_ld, accepted_at=acc, accepted_at_ld=acc_ld, n_fallback=int(np.sum(acc < 0)), n_tries=n_tries,
                prop=pack(prop), acc=pack(accm), fb=pack(fb))


def conditions(res):
    """(holds, worst): every margin >= FACTOR x its error measure and the fp64 and long-double decisions agree everywhere; worst = the
    smallest margin / error over all decisions (inf if there is none)."""
    worst = np.inf
    ok = bool(np.array_equal(res["index"], res["index_ld"]) and np.array_equal(res["accepted_at"], res["accepted_at_ld"]))
    for key in ("prop", "acc", "fb"):
        m, e = res[key]
        if m.size:
            ratio = float(np.min(m / np.maximum(e, LD(1e-300))))
            worst = min(worst, ratio)
            ok = ok and bool(np.all(m >= FACTOR * e))
    return ok, worst


def shares(res):
    """(share of trajectories that accepted, share that fell back)."""
    M = res["accepted_at"].size
    return float(np.sum(res["accepted_at"] >= 0)) / M, float(np.sum(res["accepted_at"] < 0)) / M


class PhiloxTries:
    """u_try of a session: the uniforms of (seed, slot = j, step = t, lane 0x42530001, iter = r), drawn as they are asked for."""

    def __init__(self, seed, t, R):
        self.seed, self.t, self.R = int(seed), int(t), int(R)

    def __call__(self, r, j):
        return philox_ref.uniform2(self.seed, j, self.t, REJECT_LANE, r)


def backward_uniforms(seed, T, M):
    """u [T x M] of the existing draws: first uniform of (slot = j, step = t, lane 0x42530000, iter 0)."""
    return np.array([[philox_ref.uniform2(seed, j, t, philox_ref.BACKWARD_LANE, 0)[0] for j in range(M)] for t in range(T)])


# ---- logp matrices of the three families, fp64 and long double -----------------------------------------------------------------
def lp_mag(xs_next, X, odo, dt, Q):
    f = lambda dtype: np.stack([LS.logp(xs_next[:, j], X, odo, dt, Q, dtype) for j in range(xs_next.shape[1])], axis=1)   # noqa: E731
    return f(np.float64), f(LD)


def lp_generic(xs_next, mu, cov, rows, angle_rows=(), quat_rows=None):
    f = lambda dtype: np.stack([P.logp(xs_next[:, j], mu, cov, rows, angle_rows, quat_rows, dtype)           # noqa: E731
                                for j in range(xs_next.shape[1])], axis=1)
    return f(np.float64), f(LD)


# ---- the whole recursion -------------------------------------------------------------------------------------------------------
def simulate(X, W, lp_of, seed, R, M):
    """The recursion on forward arrays X [T x n x N] (as propagated) and W [T x N] with the device generator of `seed`;
    lp_of(t, cols) -> (lp64, lp_ld) [N x len(cols)]: logp of the particles cols of step t + 1 given every particle of step t.
    Returns dict(index, index_ld [T x M], n_fallback, n_tries [T], steps: the step() results of t = 0 .. T-2, first: (margin, eps_ref)
    of the draw of step T-1)."""
    X, W = np.asarray(X, dtype=np.float64), np.asarray(W, dtype=np.float64)
    T, _, N = X.shape
    u = backward_uniforms(seed, T, M)
    index, index_ld = np.zeros((T, M), dtype=np.int64), np.zeros((T, M), dtype=np.int64)
    n_fb, n_tr = np.zeros(T, dtype=np.int64), np.zeros(T, dtype=np.int64)
    index[T - 1], index_ld[T - 1], mg, ep = _draw(np.cumsum(W[T - 1]), np.cumsum(W[T - 1].astype(LD)), u[T - 1])
    steps = [None] * (T - 1)
    for t in range(T - 2, -1, -1):
        cols, inv = np.unique(index[t + 1], return_inverse=True)
        a, b = lp_of(t, cols)
        res = step(a[:, inv], b[:, inv], W[t], PhiloxTries(seed, t, R), u[t])
        index[t], index_ld[t], n_fb[t], n_tr[t], steps[t] = res["index"], res["index_ld"], res["n_fallback"], res["n_tries"], res
    return dict(index=index, index_ld=index_ld, n_fallback=n_fb, n_tries=n_tr, steps=steps, first=(mg, ep), u=u)


def simulate_holds(sim):
    ok = bool(np.array_equal(sim["index"], sim["index_ld"]) and np.all(sim["first"][0] >= FACTOR * sim["first"][1]))
    worst = np.inf
    for res in sim["steps"]:
        o, w = conditions(res)
        ok, worst = ok and o, min(worst, w)
    return ok, worst


# ---- the committed fixtures: the CPU test checks the conditions on exactly what the GPU tests run ------------------------------
MIXED_R = 16
MAG_SHAPE = (300, 700)                         # neither a multiple of 64 or 256; M' crosses a 256 boundary
SWEEP_SHAPE = (70, 130)
SPREAD = 0.5                                   # the cloud lies this many transition standard deviations around its centre
SESSION = dict(N_P=300, N_T=5, R=16, seed=11, n_traj=(130, 700))

_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _tries(rs, R, M):
    return rs.random_sample((R, M, 2))


def mag_fixture(N=MAG_SHAPE[0], M=MAG_SHAPE[1], spread=SPREAD, seed=5):
    """Dense-mag inputs of one step: N particles `spread` transition standard deviations around a centre, M successors drawn by
    dynModel from random live particles; the first and the last ten weights are exact zeros."""
    def make():
        import cases
        import localization_ref as R
        rs = np.random.RandomState(9000 + 13 * seed + N + 7 * M)
        dt, Q = 0.01, cases.Q_MAG
        sd = spread * np.sqrt(dt * np.diag(Q))
        X = np.zeros((7, N))
        X[0:3] = np.array([[1.5], [-0.7], [0.3]]) + sd[0:3, None] * rs.standard_normal((3, N))
        q0 = R._expq(0.4 * rs.standard_normal(3))
        for i in range(N):
            X[3:7, i] = R._qLeft(q0) @ R._expq(sd[3:6] * rs.standard_normal(3))
        dx = np.concatenate((0.05 * rs.standard_normal(3), R._expq(0.02 * rs.standard_normal(3))))
        w = rs.random_sample(N) + 0.05
        w[:10] = 0.0
        w[-10:] = 0.0
        w /= w.sum()
        live = np.nonzero(w > 0)[0]
        xs = np.column_stack([R.dyn_model(X[:, live[rs.randint(live.size)]], dx, dt, Q, rs.standard_normal(6)) for _ in range(M)])
        return dict(kind="mag", key=("mag", N, M, spread, seed), X=X, w=w, xs_next=xs, odo=dx, dt=dt, Q=Q, u=rs.random_sample(M),
                    u_try=_tries(rs, MIXED_R, M))
    return _once(("mag", N, M, spread, seed), make)


def sweep_fixture(name, N=SWEEP_SHAPE[0], M=SWEEP_SHAPE[1], spread=SPREAD, R=None, seed=0):
    """One step in the layout `name` of transition_sweep_ref (rows, angle rows, the block's place, decoys in the rows that are not
    selected, predecessors on an angle row offset by whole turns) at another size and spread: predecessors `spread` transition
    standard deviations around a centre, successors drawn from random live predecessors with one transition's noise.  R tries;
    None: the number at which half of the trajectories of this fixture have accepted (at least 1), from its own uniforms."""
    def make():
        l = TS.layout(name)
        rs = np.random.RandomState(TS.SEED + 7 + 101 * TS.NAMES.index(name) + N + 7 * M + 1009 * seed)
        pos = l.residual_positions()
        kind = ["quat" if p == l.qpos else "angle" if l.rows[p] in l.angle_rows else "plain" for p in pos]
        span = dict(plain=(0.04, 0.08), angle=(0.025, 0.035), quat=(0.012, 0.018))
        while True:
            cov = P._spd(rs, np.array([rs.uniform(*span[k]) for k in kind]))
            cov = 0.5 * (cov + cov.T)
            if np.linalg.cond(cov) < 1e3:
                break
        Lc = np.linalg.cholesky(cov)
        w = rs.random_sample(N) + 0.05
        w[:10] = 0.0
        w[-10:] = 0.0
        w /= w.sum()
        live = np.nonzero(w > 0)[0]
        pick = live[rs.randint(live.size, size=M)]
        n_pred = spread * (Lc @ rs.standard_normal((l.n_res, N)))
        n_succ = n_pred[:, pick] + Lc @ rs.standard_normal((l.n_res, M))
        mu = np.zeros((l.n_sel, N))
        xs = rs.choice([-1.0, 1.0], (TS.N_NONLIN, M)) * rs.uniform(1e3, 2e3, (TS.N_NONLIN, M))      # the decoys
        k = 0
        while k < l.n_res:
            p = pos[k]
            if kind[k] == "quat":
                qc = P.expq(0.4 * rs.standard_normal(3)).reshape(4, 1)
                mu[p:p + 4] = P.qmul(qc * np.ones((1, N)), P.expq(n_pred[k:k + 3]))
                xs[list(l.quat_rows)] = P.qmul(qc * np.ones((1, M)), P.expq(n_succ[k:k + 3]))
                k += 3
                continue
            if kind[k] == "angle":
                mu[p] = 3.1 + n_pred[k] + TS.S.TWO_PI * rs.randint(-3, 4, N)
                xs[l.rows[p]] = TS.S.wrap(3.1 + n_succ[k])
            else:
                c = rs.uniform(-1.0, 1.0)
                mu[p], xs[l.rows[p]] = c + n_pred[k], c + n_succ[k]
            k += 1
        out = dict(kind="generic", key=("sweep", name, N, M, spread, R, seed), layout=l, mu=mu, xs_next=xs, cov=cov, w=w, u=rs.random_sample(M), **l.args())
        u_try = _tries(rs, 64, M)
        if R is None:
            full = step(*lp_generic(xs, mu, cov, l.rows, l.angle_rows, l.quat_rows), w, u_try, out["u"])
            at = np.sort(np.where(full["accepted_at"] >= 0, full["accepted_at"], 64))
            out["u_try"] = u_try[:max(1, min(64, int(at[M // 2]) + 1))]
        else:
            out["u_try"] = u_try[:R]
        return out
    return _once(("sweep", name, N, M, spread, R, seed), make)


def nothing_falls_back_fixture():
    """Gaussian term, n_res = 1, the cloud 0.25 standard deviations wide, R = 64, 300 successors (two trajectory blocks).  A successor
    three standard deviations out is accepted with probability 0.01 per try, so about one in 230 successors outlasts 64 tries: the
    seed is one whose 300 do not (asserted on the reference by the CPU test)."""
    return sweep_fixture("g1", 300, 300, 0.25, 64, seed=2)


def logp_of(p):
    if p["kind"] == "mag":
        return lp_mag(p["xs_next"], p["X"], p["odo"], p["dt"], p["Q"])
    return lp_generic(p["xs_next"], p["mu"], p["cov"], p["rows"], p["angle_rows"], p["quat_rows"])


def reference(p):
    """step() of a fixture; a committed fixture (one with a `key`) is computed once and shared."""
    make = lambda: step(*logp_of(p), p["w"], p["u_try"], p["u"])                                    # noqa: E731
    return _once(("ref",) + p["key"], make) if "key" in p else make()


FAR = 10.0                                     # at least 125 standard deviations of every row it is used on: logp < -7800


def far_successor(p, j):
    """The fixture with successor j moved so far from every particle, along a row that is neither an angle nor in the block, that the
    exp of every pair is 0 and every try is rejected."""
    q = {k: v for k, v in p.items() if k != "key"}
    xs = p["xs_next"].copy()
    if p["kind"] == "mag":
        xs[0, j] += FAR
    else:
        l = p["layout"]
        xs[[r for r in l.plain if r not in l.angle_rows][0], j] += FAR
    q["xs_next"] = xs
    return q


# ---- full sessions: the three map classes at (N_P, N_T) of SESSION ---------------------------------------------------------------
SESSION_KINDS = ("mag", "gauss", "landmark")   # DenseMagMap; a DeviceMap, model D (n_res = 3, one angle row); a DeviceLandmarkMap (3 plain rows)


def session_case(kind):
    def make():
        import device_map_smoother_ref as S
        N, T = SESSION["N_P"], SESSION["N_T"]
        if kind == "mag":
            import localization_ref as R
            return dict(R.loc_case(N, T, 13))
        if kind == "gauss":
            return S.case("D", N, T)
        import landmark_map_ref as lm
        return lm.case("ro", 6, N, T, 2)
    return _once(("session", kind), make)


def session_forward(kind):
    """The restatement's own forward pass (X [T x n x N], W [T x N]) of a session case."""
    def make():
        import device_map_smoother_ref as S
        import map_trajectory_ref as V
        c = session_case(kind)
        if kind == "mag":
            return V.forward_mag(c)
        if kind == "landmark":
            return V.forward_landmark(c)
        return S.forward_arrays(c)[:2]
    return _once(("forward", kind), make)


def session_lp(kind, X, mus=None):
    """lp_of of simulate() for a session case on forward arrays X; mus[t]: what the `mean` handle returned (gauss; default: the
    case's own statement)."""
    import device_map_smoother_ref as S
    import map_trajectory_ref as V
    c = session_case(kind)
    T = X.shape[0]
    if kind == "mag":
        dt, Q = V.pages(c, T)
        return lambda t, cols: lp_mag(X[t + 1][:, cols], X[t], c["odometry"][t], dt[t], Q[:, :, t])
    if kind == "landmark":
        cov = c["dt"] * np.atleast_2d(np.asarray(c["Q"], dtype=np.float64))
        return lambda t, cols: lp_generic(X[t + 1][:, cols], X[t] + np.asarray(c["odometry"][t], dtype=np.float64).reshape(3, 1), cov, (0, 1, 2))
    ref_mus, covs = S.transition_arrays(c, X)
    mus = ref_mus if mus is None else mus
    return lambda t, cols: lp_generic(X[t + 1][:, cols], mus[t], covs[t], c.rows, c.angle_rows, None)
