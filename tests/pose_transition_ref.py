"""Checker of the backward-simulation smoother in a DeviceMap for pose states (rbpf.DeviceTransition(..., quat_rows=...)): the
recursion and the draws of tests/device_map_smoother_ref.py with the density of a state that holds a unit quaternion (q0 .. q3,
scalar first) whose noise multiplies the predicted quaternion on the right (run_dense3D_magfield.m:202-203,
run_localization.m:274-281), constants omitted:

    r = [wrap(x'[plain rows] - mu) ; phi],   e = qInv(mu_q) (x) x'_q,   e <- -e if e0 < 0 (tools/logq.m:26-28),
    phi = atan2(|e_v|, e0) e_v / |e_v|  (0 if |e_v| = 0),      z = L \\ r  (L = chol(cov, 'lower')),   logp = -z'z / 2

The residual is in the CALLER's order: the rows in the order of `rows`, the three entries of phi in the place of the four block
rows; cov is n_res x n_res in that order, n_res = len(rows) - 1.  mu [n_sel x N] is what the model's `mean` handle returned, its
block rows the predicted unit quaternion.  logq_acos is the literal form of tools/logq.m; the atan2 form has the same value for a
unit e without the cancellation of acos near 1.  Everything is vectorised over the particles; `dtype=np.longdouble` runs the same
statements in extended precision on the same fp64 inputs.  _draw, backward_cdf, Case, forward_arrays and transition_arrays are
those of device_map_smoother_ref.

The committed cases are three models, each x' = post(plain rows of drift(x, dx) + noise ; drift_q (x) expq(noise_phi)) with the
noise chol(cov) z in residual order:
  E  n_nonlin = 7, position 0..2 and quaternion 3..6, rows all, n_res = 6: the state of the reference's 3-D examples.  Q is a full
     6 x 6 SPD matrix that couples position and rotation; cov = dt Q is the transition's default.  mu_q = qRight(q) dq.
  F  n_nonlin = 4, the quaternion alone, n_res = 3: no plain row precedes the block.  mu_q = q (x) dq.
  G  n_nonlin = 8, rows = (4, 0, 1, 2, 3, 6), quat_rows = (0, 1, 2, 3), angle_rows = (6,), n_res = 5: the block is not last in the
     caller's order, the heading (row 6) passes +-pi during the run, rows 5 and 7 move without noise and take no part, and cov is
     coupled through a custom cov(dt, Q) = C (dt Q) C'.
Every committed input keeps |phi| < 1 rad (tests/test_pose_transition_cpu.py asserts it): e0 > cos(1) stays far from the branch at
0, where fp64 and long double could flip differently -- a property of the density, not of a kernel.

Nothing in the package imports this file."""
import numpy as np

import device_map_ref as dm
import generic_ny_cases as gc
from device_map_smoother_ref import (Case, _draw, _log_weights, _simulate_y, backward_cdf, forward_arrays,  # noqa: F401
                                     transition_arrays, wrap)

LD = np.longdouble


# ---- quaternions (tools/q*.m), [4 x ...] arrays of any float dtype --------------------------------------------------------
def qmul(a, b):
    """a (x) b = qLeft(a) b (tools/qLeft.m:30-35), rows summed left to right."""
    return np.stack((a[0] * b[0] + (-a[1]) * b[1] + (-a[2]) * b[2] + (-a[3]) * b[3],
                     a[1] * b[0] + a[0] * b[1] + (-a[3]) * b[2] + a[2] * b[3],
                     a[2] * b[0] + a[3] * b[1] + a[0] * b[2] + (-a[1]) * b[3],
                     a[3] * b[0] + (-a[2]) * b[1] + a[1] * b[2] + a[0] * b[3]))


def qinv(q):
    """tools/qInv.m:27-31."""
    return np.stack((q[0], -q[1], -q[2], -q[3]))


def expq(v):
    """tools/expq.m for v [3 x ...]: (cos |v|, sin |v| v / |v|)."""
    v = np.asarray(v)
    a = np.sqrt(np.sum(v * v, axis=0))
    return np.concatenate((np.cos(a)[None], (np.sin(a) / np.where(a > 0, a, 1.0))[None] * v))


def logq_atan2(e):
    """The form the kernels use: sign flip, then atan2(|e_v|, e0) e_v / |e_v|, 0 where |e_v| = 0."""
    e = np.where(e[0] < 0, -e, e)
    nv = np.sqrt(e[1] * e[1] + e[2] * e[2] + e[3] * e[3])
    f = np.where(nv == 0, e.dtype.type(1.0), np.arctan2(nv, e[0]) / np.where(nv == 0, e.dtype.type(1.0), nv))
    return f * e[1:4]


def logq_acos(e):
    """tools/logq.m:26-30, literally; e0 > 1 by rounding is clamped (MATLAB's acos would go complex)."""
    e = np.where(e[0] < 0, -e, e)
    na = np.arccos(np.minimum(e[0], e.dtype.type(1.0)))
    return na * e[1:4] / (np.sin(na) + (na == 0))


# ---- the density ----------------------------------------------------------------------------------------------------------
def residual_vector(xt, mu, rows, angle_rows=(), quat_rows=None, dtype=np.float64, logq=logq_atan2):
    """r [n_res x N] in the caller's residual order for xt [n_nonlin] against the predicted rows mu [n_sel x N]."""
    rows = tuple(rows)
    xt = np.asarray(xt, dtype=np.float64).astype(dtype).ravel()
    mu = np.asarray(mu, dtype=np.float64).astype(dtype).reshape(len(rows), -1)
    quat_rows = tuple(quat_rows) if quat_rows is not None else ()
    qpos = rows.index(quat_rows[0]) if quat_rows else -1
    assert not quat_rows or rows[qpos:qpos + 4] == quat_rows
    out = []
    for pos, r in enumerate(rows):
        if pos == qpos:
            e = qmul(qinv(mu[qpos:qpos + 4]), xt[list(quat_rows), None] * np.ones((1, mu.shape[1]), dtype=dtype))
            out.extend(logq(e))
        elif r in quat_rows:
            continue
        else:
            d = xt[r] - mu[pos]
            out.append(wrap(d, dtype) if r in angle_rows else d)
    return np.stack(out)


def logp(xt, mu, cov, rows, angle_rows=(), quat_rows=None, dtype=np.float64, logq=logq_atan2):
    """[N] log transition densities xt | particle i, constants omitted."""
    r = residual_vector(xt, mu, rows, angle_rows, quat_rows, dtype, logq)
    n = r.shape[0]
    z = dm.forward(dm.chol(np.asarray(cov, dtype=np.float64).astype(dtype).reshape(n, n)), r)
    return -dtype(0.5) * np.sum(z * z, axis=0)


def max_phi(xs_next, mu, rows, quat_rows):
    """The largest |phi| over all pairs (particle, trajectory)."""
    qpos = tuple(rows).index(quat_rows[0])
    worst = 0.0
    for j in range(np.asarray(xs_next).shape[1]):
        r = residual_vector(xs_next[:, j], mu, rows, (), quat_rows)[qpos:qpos + 3]
        worst = max(worst, float(np.max(np.sqrt(np.sum(r * r, axis=0)))))
    return worst


def backward_step(mu, w, xs_next, cov, u, rows, angle_rows=(), quat_rows=None):
    """device_map_smoother_ref.backward_step with this density: mu [n_sel x N], w [N], xs_next [n_nonlin x M], u [M]."""
    mu = np.asarray(mu, dtype=np.float64).reshape(len(rows), -1)
    xs_next = np.asarray(xs_next, dtype=np.float64)
    N, M = mu.shape[1], xs_next.shape[1]
    u = np.asarray(u, dtype=np.float64).ravel()
    out = dict(index=np.zeros(M, dtype=np.int64), index_ld=np.zeros(M, dtype=np.int64), margin=np.zeros(M, dtype=LD),
               eps_ref=np.zeros(M, dtype=LD), logp=np.zeros((N, M)), logp_ld=np.zeros((N, M), dtype=LD))
    lw, lw_ld = _log_weights(w, np.float64), _log_weights(w, LD)
    for j in range(M):
        lp = logp(xs_next[:, j], mu, cov, rows, angle_rows, quat_rows)
        lp_ld = logp(xs_next[:, j], mu, cov, rows, angle_rows, quat_rows, LD)
        i, i_ld, mg, ep = _draw(backward_cdf(lw + lp), backward_cdf(lw_ld + lp_ld), u[j:j + 1])
        out["index"][j], out["index_ld"][j], out["margin"][j], out["eps_ref"][j] = i[0], i_ld[0], mg[0], ep[0]
        out["logp"][:, j], out["logp_ld"][:, j] = lp, lp_ld
    return out


def backward_simulate(X, W, mus, covs, u, rows, angle_rows=(), quat_rows=None):
    """device_map_smoother_ref.backward_simulate with this density; also max_phi, the largest |phi| of any pair it evaluated."""
    X, W, u = np.asarray(X, dtype=np.float64), np.asarray(W, dtype=np.float64), np.asarray(u, dtype=np.float64)
    T, _, N = X.shape
    M = u.shape[1]
    index, index_ld = np.zeros((T, M), dtype=np.int64), np.zeros((T, M), dtype=np.int64)
    margin, eps_ref = np.zeros((T, M), dtype=LD), np.zeros((T, M), dtype=LD)
    index[T - 1], index_ld[T - 1], margin[T - 1], eps_ref[T - 1] = _draw(np.cumsum(W[T - 1]), np.cumsum(W[T - 1].astype(LD)), u[T - 1])
    err, scale, phi = 0.0, 0.0, 0.0
    for t in range(T - 2, -1, -1):
        lw, lw_ld = _log_weights(W[t], np.float64), _log_weights(W[t], LD)
        for b in np.unique(index[t + 1]):
            js = np.nonzero(index[t + 1] == b)[0]
            lp = logp(X[t + 1][:, b], mus[t], covs[t], rows, angle_rows, quat_rows)
            lp_ld = logp(X[t + 1][:, b], mus[t], covs[t], rows, angle_rows, quat_rows, LD)
            err, scale = max(err, float(np.max(np.abs(lp - lp_ld)))), max(scale, float(np.max(np.abs(lp_ld))))
            phi = max(phi, max_phi(X[t + 1][:, b:b + 1], mus[t], rows, quat_rows))
            index[t, js], index_ld[t, js], margin[t, js], eps_ref[t, js] = _draw(backward_cdf(lw + lp), backward_cdf(lw_ld + lp_ld), u[t, js])
    xs = np.stack([X[t][:, index[t]] for t in range(T)], axis=2)
    return dict(index=index, index_ld=index_ld, xs_traj=xs, traj_smooth_mean=np.mean(xs, axis=1), margin=margin, eps_ref=eps_ref,
                logp_rel=err / max(scale, 1e-300), max_phi=phi)


# ---- the three models -------------------------------------------------------------------------------------------------------
class PoseCase(Case):
    """A device_map_smoother_ref.Case whose selected rows hold a quaternion block: drift(x [n_nonlin x N], dx) -> [n_nonlin x N] with
    the predicted unit quaternion in the block rows; cov_fn(dt, Q) -> [n_res x n_res] in residual order (None: dt Q)."""

    def __init__(self, name, m, p, rows, angle_rows, quat_rows, drift, cov_fn=None):
        super().__init__(name, m, p, rows, angle_rows, drift, None, default_cov=cov_fn is None)
        self.quat_rows = tuple(quat_rows)
        self.qpos = self.rows.index(self.quat_rows[0])
        self.n_sel, self.n_res = len(self.rows), len(self.rows) - 1
        self.cov_fn = cov_fn
        assert m.nw == self.n_res

    def cov_of(self, dt, Q):
        """The host callable of the DeviceTransition."""
        return dt * np.atleast_2d(Q) if self.cov_fn is None else self.cov_fn(dt, np.atleast_2d(Q))

    def mean(self, x, t):
        return self.drift(np.asarray(x, dtype=np.float64), self.p["odometry"][t])[list(self.rows)]

    def dyn(self, x, t, z):
        """x [n_nonlin x N], z [N x n_res] -> the states of step t + 1: x'_q = mu_q (x) expq(noise)."""
        mu = self.drift(np.asarray(x, dtype=np.float64), self.p["odometry"][t])
        n = np.linalg.cholesky(self.cov(t)) @ z.T
        out, k, q = mu.copy(), 0, list(self.quat_rows)
        for pos, r in enumerate(self.rows):
            if pos == self.qpos:
                out[q] = qmul(mu[q], expq(n[k:k + 3]))
                k += 3
            elif r not in self.quat_rows:
                out[r] = mu[r] + n[k]
                k += 1
        return self.post(out)


def _spd(rs, sd):
    """D (B B' / n + I) D / 2: a full SPD matrix with standard deviations about sd."""
    n = len(sd)
    B = rs.standard_normal((n, n))
    return np.diag(sd) @ (0.5 * (B @ B.T) / n + 0.5 * np.eye(n)) @ np.diag(sd)


def drift_E(x, dx):
    """Position + dx(1:3); qRight(q) dq = dq (x) q, the composition of run_localization.m."""
    dq = np.asarray(dx[3:7], dtype=np.float64).reshape(4, 1) * np.ones((1, x.shape[1]))
    return np.concatenate((x[0:3] + np.asarray(dx[0:3]).reshape(3, 1), qmul(dq, x[3:7])))


def drift_F(x, dx):
    return qmul(x, np.asarray(dx, dtype=np.float64).reshape(4, 1) * np.ones((1, x.shape[1])))


def drift_G(x, dx):
    """q (x) dq on rows 0..3; row 4 bends, rows 5 and 7 move without noise, row 6 is a heading that advances by dx(7)."""
    dq = np.asarray(dx[0:4], dtype=np.float64).reshape(4, 1) * np.ones((1, x.shape[1]))
    return np.concatenate((qmul(x[0:4], dq), np.stack((x[4] + 0.1 * np.sin(x[4]) + dx[4], x[5] + dx[5], x[6] + dx[6],
                                                        x[7] + 0.1 * np.sin(x[5]) + dx[7]))))


_CASES = {}


def case(name, N_P, N_T, seed=3):
    """Model E, F or G at (N_P, N_T), built once."""
    key = (name, N_P, N_T, seed)
    if key in _CASES:
        return _CASES[key]
    rs = np.random.RandomState(7000 + seed + ord(name))
    T1 = max(N_T - 1, 1)
    q0 = expq(np.array([0.2, -0.3, 0.1]))
    dq = expq(0.05 * rs.standard_normal((3, T1))).T                                             # [T1 x 4]
    if name == "E":
        m, p = gc.case((7, 6, 7, 3, 17), N_P, N_T, seed=seed)
        p["Q"] = _spd(rs, np.array([0.15, 0.15, 0.15, 0.03, 0.03, 0.03]))
        p["x0_nonLin"] = np.concatenate(([0.3, -0.5, 0.2], q0))
        p["odometry"] = np.column_stack((0.3 * rs.standard_normal((T1, 3)), dq))
        c = PoseCase(name, m, p, range(7), (), (3, 4, 5, 6), drift_E)
    elif name == "F":
        m, p = gc.case((4, 3, 4, 2, 15), N_P, N_T, seed=seed)
        p["Q"] = _spd(rs, np.array([0.04, 0.04, 0.04]))
        p["x0_nonLin"] = q0
        p["odometry"] = dq
        c = PoseCase(name, m, p, range(4), (), (0, 1, 2, 3), drift_F)
    elif name == "G":
        m, p = gc.case((8, 5, 8, 3, 19), N_P, N_T, seed=seed)
        p["Q"] = np.diag(rs.uniform(0.01, 0.04, 5))
        Cc = np.diag([1.0, 0.25, 0.25, 0.25, 0.3]) @ (np.eye(5) + 0.4 * rs.standard_normal((5, 5)))   # couples all five residuals
        p["x0_nonLin"] = np.concatenate((q0, [0.3, -0.5, 3.05, 0.2]))
        odo = np.column_stack((dq, 0.3 * rs.standard_normal((T1, 4))))
        odo[:, 6] = 0.06                                                                        # the heading climbs through pi
        p["odometry"] = odo
        c = PoseCase(name, m, p, (4, 0, 1, 2, 3, 6), (6,), (0, 1, 2, 3), drift_G, cov_fn=lambda dt, Q: Cc @ (dt * Q) @ Cc.T)
    else:
        raise KeyError(name)
    _simulate_y(c, seed)
    _CASES[key] = c
    return c


# ---- the committed cases: the CPU test checks the margin condition on exactly what the GPU tests run -------------------------
PROBE_LOGP_SHAPES = [(1, 1), (70, 5), (257, 65)]
PROBE_INDEX_SHAPES = [(64, 64), (70, 1), (1, 3), (4100, 130)]
MODELS = ("E", "F", "G")
PROBE_LOGP_CASES = [(name, N, M) for name in MODELS for N, M in PROBE_LOGP_SHAPES]
PROBE_INDEX_CASES = [(name, N, M) for name in MODELS for N, M in PROBE_INDEX_SHAPES]
FULL_RUNS = [("E", 70, 8, 33), ("E", 257, 6, 1), ("F", 40, 5, 33), ("G", 65, 6, 17)]          # (model, N_P, N_T, n_traj)
U_SEED = 4242

_PROBES = {}


def probe_case(name, N, M, seed=7):
    """Inputs of one backward step of model `name`, as device_map_smoother_ref.probe_case: N particles scattered two standard
    deviations of the transition noise around a centre (the quaternion: centre (x) expq(2 noise); the angle rows around 3.1), mu
    their predicted rows, M states of the next step drawn by the model's dynModel from random live particles.  From N = 64 on the
    first and the last ten weights are exact zeros.  Built once per (name, N, M)."""
    key = (name, N, M, seed)
    if key in _PROBES:
        return _PROBES[key]
    c = case(name, 8, 4)
    rs = np.random.RandomState(1000 * seed + N + 7 * M + ord(name))
    cov = c.cov(1)
    n = 2.0 * (np.linalg.cholesky(cov) @ rs.standard_normal((c.n_res, N)))
    X = rs.uniform(-1.0, 1.0, (c.nN, 1)) + 0.1 * rs.standard_normal((c.nN, N))
    k, q = 0, list(c.quat_rows)
    for pos, r in enumerate(c.rows):
        if pos == c.qpos:
            X[q] = qmul(expq(0.4 * rs.standard_normal(3)).reshape(4, 1) * np.ones((1, N)), expq(n[k:k + 3]))
            k += 3
        elif r not in c.quat_rows:
            X[r] = rs.uniform(-1.0, 1.0) + n[k]
            k += 1
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
    xs_next = c.dyn(X[:, pick], 1, rs.standard_normal((M, c.n_res)))
    out = dict(case=c, X=X, mu=c.mean(X, 1), w=w, xs_next=xs_next, cov=cov, u=rs.random_sample(M), rows=c.rows, angle_rows=c.angle_rows,
               quat_rows=c.quat_rows)
    _PROBES[key] = out
    return out


_PROBE_REFS = {}


def probe_reference(name, N, M):
    """backward_step of probe_case(name, N, M), computed once and shared."""
    key = (name, N, M)
    if key not in _PROBE_REFS:
        p = probe_case(name, N, M)
        _PROBE_REFS[key] = backward_step(p["mu"], p["w"], p["xs_next"], p["cov"], p["u"], p["rows"], p["angle_rows"], p["quat_rows"])
    return _PROBE_REFS[key]


def full_run_uniforms(N_T, M):
    return np.random.RandomState(U_SEED).random_sample((N_T, M))


# ---- the dense-mag inputs in model E's form: ties this checker to tests/localization_smoother_ref.py -------------------------
ROWS_E = tuple(range(7))
QUAT_E = (3, 4, 5, 6)


def dense_mag_as_pose(p):
    """(mu [7 x N], cov [6 x 6]) of localization_smoother_ref.probe_case(...) = p: mu = (p + dx_pos, qRight(q) dq) and
    cov = blkdiag(S_pos S_pos', S_rot S_rot') with S = sqrt(dt Q) element-wise on the diagonal blocks, the factor that file
    whitens with -- for the examples' diagonal Q this is blkdiag(dt Q(1:3,1:3), dt Q(4:6,4:6)) exactly."""
    import localization_smoother_ref as LS
    X, dx, dt, Q = p["X"], p["odo"], p["dt"], np.asarray(p["Q"], dtype=np.float64)
    mu = np.concatenate((X[0:3] + dx[0:3, None], LS.qright_mul(X[3:7], dx[3:7])))
    cov = np.zeros((6, 6))
    for s in (slice(0, 3), slice(3, 6)):
        Sb = np.sqrt(dt * Q[s, s])
        cov[s, s] = dt * Q[s, s] if np.all(Q[s, s] == np.diag(np.diag(Q[s, s]))) else Sb @ Sb.T
    return mu, cov
