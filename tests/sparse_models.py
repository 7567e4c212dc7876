"""Models for the sparseFeatures = true branch (src/particleFilter.m:127-137,165-181) beyond the reference's pinhole camera, as
objects oracle/rbpf_oracle.py:particleFilter(model, ..., sparseFeatures=True) takes:

    dynModel(xn, dx, dt, Q, z) -> (xn_new, _)          z: the normals of this call, replayed from ReplayRNG.Z
    measModel(xn_i, xl_i)      -> (yhat [ny], dy [ny x nLin])

and seeded problem instances built on them (the dict layout of tests/cases.py).  The torch twins are in
tests/sparse_models_torch.py.

RangeBearingModel   planar pose (x, y, heading), L point landmarks (mx, my interleaved in xl); per landmark the range and the
                    bearing relative to the heading: ny = 2 L, nLin = 2 L.  `coupling` adds a fixed linear term G xl to yhat (G
                    dense, seeded), so that no entry of the Jacobian is zero: a step kernel that assumed the block structure of
                    the physical part would be found out.
RangeOnly3DModel    position (x, y, z), L beacons in 3-D (xl = L x 3), the ranges only: ny = L, nLin = 3 L."""
import numpy as np

import rbpf_oracle as O


class _AdditiveDyn:
    nNonLin = 3
    nw = 3
    sparse = True
    dynResNorm = None

    def dynModel(self, xn, dx, dt, Q, z):
        """xn + dx' + chol(dt*Q, 'lower') * randn(3, 1)"""
        Lq = np.linalg.cholesky(dt * np.atleast_2d(np.asarray(Q, dtype=np.float64)))
        return np.asarray(xn, dtype=np.float64).ravel() + np.asarray(dx, dtype=np.float64).ravel() + Lq @ np.asarray(z, dtype=np.float64).ravel(), None


class RangeBearingModel(_AdditiveDyn):
    def __init__(self, L, coupling=0.02, seed=0):
        self.L = int(L)
        self.G = coupling * np.random.RandomState(1000 + seed).standard_normal((2 * self.L, 2 * self.L))

    @property
    def ny(self):
        return 2 * self.L

    @property
    def nLin(self):
        return 2 * self.L

    def measModel(self, xn, xl):
        xn = np.asarray(xn, dtype=np.float64).ravel()
        xl = np.asarray(xl, dtype=np.float64).ravel()
        m = xl.reshape(-1, 2)
        dx, dy_ = m[:, 0] - xn[0], m[:, 1] - xn[1]
        r2 = dx * dx + dy_ * dy_
        r = np.sqrt(r2)
        yhat = np.empty(2 * self.L)
        yhat[0::2] = r
        yhat[1::2] = np.arctan2(dy_, dx) - xn[2]
        J = np.zeros((2 * self.L, 2 * self.L))
        j = np.arange(self.L)
        J[2 * j, 2 * j] = dx / r
        J[2 * j, 2 * j + 1] = dy_ / r
        J[2 * j + 1, 2 * j] = -dy_ / r2
        J[2 * j + 1, 2 * j + 1] = dx / r2
        return yhat + self.G @ xl, J + self.G


class RangeOnly3DModel(_AdditiveDyn):
    def __init__(self, L):
        self.L = int(L)

    @property
    def ny(self):
        return self.L

    @property
    def nLin(self):
        return 3 * self.L

    def measModel(self, xn, xl):
        xn = np.asarray(xn, dtype=np.float64).ravel()
        dlt = np.asarray(xl, dtype=np.float64).reshape(-1, 3) - xn[None, :]
        r = np.sqrt(np.sum(dlt * dlt, axis=1))
        J = np.zeros((self.L, 3 * self.L))
        j = np.arange(self.L)
        for a in range(3):
            J[j, 3 * j + a] = dlt[:, a] / r
        return r, J


Q_RB = np.diag([0.05 ** 2, 0.05 ** 2, 0.01 ** 2])


def range_bearing_case(L, N_P, N_T, seed=1, pattern=None):
    """A vehicle driving along +x with the landmarks AHEAD of the whole path (bearings stay inside +-1 rad: the reference does
    not wrap innovations).  y has whole landmarks missing at some steps and single components at others; `pattern` = list of
    per-step strings overrides that for the first steps: "none" (every output NaN), "last" (only the last output observed),
    "all"."""
    rs = np.random.RandomState(seed)
    model = RangeBearingModel(L, seed=seed)
    mp = np.vstack((rs.uniform(5.0, 9.0, L), rs.uniform(-3.0, 3.0, L)))
    th = 0.02 * np.cumsum(rs.standard_normal(N_T))
    p = np.vstack((0.1 * np.arange(N_T), 0.03 * np.cumsum(rs.standard_normal(N_T))))
    xl_true = mp.T.reshape(-1)
    sig = np.tile([0.1, 0.02], L)
    y = np.empty((N_T, 2 * L))
    for t in range(N_T):
        y[t] = model.measModel(np.array([p[0, t], p[1, t], th[t]]), xl_true)[0] + sig * rs.standard_normal(2 * L)
        if t % 3 == 1:                                            # whole landmarks missing
            gone = rs.random_sample(L) < 0.4
            y[t, np.repeat(gone, 2)] = np.nan
        elif t % 3 == 2:                                          # single components missing
            y[t, rs.random_sample(2 * L) < 0.3] = np.nan
    for t, what in enumerate(pattern or []):
        y[t] = model.measModel(np.array([p[0, t], p[1, t], th[t]]), xl_true)[0] + sig * rs.standard_normal(2 * L)
        if what == "none":
            y[t, :] = np.nan
        elif what == "last":
            y[t, :-1] = np.nan
    u = np.vstack((np.diff(p, axis=1), np.diff(th)[None, :])).T + 0.01 * rs.standard_normal((N_T - 1, 3))
    x0_lin = xl_true[:, None] + 0.3 * rs.standard_normal((2 * L, N_P))
    rng = O.ReplayRNG.draw(seed + 500, 1, N_T, N_P, 3)
    return dict(kind="sparse", model=model, odometry=u, y=y, x0_nonLin=np.array([p[0, 0], p[1, 0], th[0]]), x0_lin=x0_lin,
                P0_lin=1.0 ** 2 * np.eye(2 * L), Q=Q_RB, R=np.diag(sig ** 2), N_P=N_P, dt=1.0, rng=rng, N_K=1)


def range_only_case(L, N_P, N_T, seed=1):
    """A vehicle among L beacons in 3-D, ranges only; x0_lin is n x 1 (every particle starts from the same map).  Some ranges
    are missing at every step but the first."""
    rs = np.random.RandomState(seed)
    model = RangeOnly3DModel(L)
    beacons = rs.uniform(-8.0, 8.0, (L, 3)) + np.array([0.0, 0.0, 12.0])
    p = np.cumsum(np.vstack((np.zeros(3), 0.2 * rs.standard_normal((N_T - 1, 3)))), axis=0)
    xl_true = beacons.reshape(-1)
    y = np.empty((N_T, L))
    for t in range(N_T):
        y[t] = model.measModel(p[t], xl_true)[0] + 0.05 * rs.standard_normal(L)
        if t > 0:
            y[t, rs.random_sample(L) < 0.25] = np.nan
    u = np.diff(p, axis=0) + 0.01 * rs.standard_normal((N_T - 1, 3))
    x0_lin = xl_true + 0.2 * rs.standard_normal(3 * L)
    rng = O.ReplayRNG.draw(seed + 600, 1, N_T, N_P, 3)
    return dict(kind="sparse", model=model, odometry=u, y=y, x0_nonLin=p[0].copy(), x0_lin=x0_lin, P0_lin=0.5 ** 2 * np.eye(3 * L),
                Q=np.diag([0.03 ** 2] * 3), R=0.05 ** 2 * np.eye(L), N_P=N_P, dt=1.0, rng=rng, N_K=1)
