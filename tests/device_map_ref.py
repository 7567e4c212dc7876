"""Localisation in the fixed map of a generic model, restated in numpy: particleFilter.m:100-161 with xl = mean and P = V'V the
same for every particle and never updated (:163-204 left out).  Per step and particle i, with H_i = measModel(xn_i) [n_y x nLin],

    e_i = y_t' - H_i mean,   S_i = (V H_i')'(V H_i') + R,   logw_i = -sum log diag chol S_i - |chol(S_i) \\ e_i|^2 / 2 - n_y log(2 pi) / 2

(:139-150), then the normalisation, traj_max / traj_mean, ai(i) = sample(w) on the replayed uniforms U, xn = dynModel(xn_(ai)) on the
replayed normals Z of generic_model.problem, and xn_traj through the ancestor table.  Runs in float64 and in np.longdouble (the
handles' Jacobians and states are rounded to float64 in both, as the device is handed them; the draws are rbpf_oracle.sample in
float64 and its long-double twin otherwise).

The problems are generic_ny_cases.case (a full R) with the map mean = x0_lin + small noise and V a random lower factor scaled so
that H P H' is of R's order; y is simulated from that map along a true path.  Shared by tests/test_device_map_cpu.py and
tests/test_gpu_device_map.py."""
import numpy as np

import generic_ny_cases as gc
import rbpf_oracle as O

LD = np.longdouble


def chol(A):
    """Lower Cholesky factor in the dtype of A, one column at a time."""
    A = np.array(A)
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        d = np.sqrt(A[j, j] - L[j, :j] @ L[j, :j])
        L[j, j] = d
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - L[i, :j] @ L[j, :j]) / d
    return L


def forward(L, b):
    x = np.zeros_like(b)
    for i in range(L.shape[0]):
        x[i] = (b[i] - L[i, :i] @ x[:i]) / L[i, i]
    return x


def weights(H, mean, V, R, y, dtype=np.float64):
    """H [N x n_y x nLin] -> (yhat [N x n_y], S [N x n_y x n_y] before R is added, logw [N]) in `dtype`."""
    H = np.asarray(H, dtype=np.float64).astype(dtype)
    N, d, n = H.shape
    V = np.tril(np.asarray(V, dtype=np.float64)).astype(dtype)
    mean, R, y = (np.asarray(a, dtype=np.float64).astype(dtype) for a in (mean, R, y))
    Y = (H.reshape(N * d, n) @ V.T).reshape(N, d, n)                      # row (i, k) = V H_i(k, :)'
    S = np.einsum("iar,ibr->iab", Y, Y)
    yhat = (H.reshape(N * d, n) @ mean).reshape(N, d)
    logw = np.zeros(N, dtype=dtype)
    c = dtype(0.5) * dtype(d) * np.log(dtype(2.0) * dtype(np.pi))
    for i in range(N):
        L = chol(S[i] + R.reshape(d, d))
        z = forward(L, y.ravel() - yhat[i])
        logw[i] = -np.sum(np.log(np.diag(L))) - dtype(0.5) * (z @ z) - c
    return yhat, S, logw


def _sample_ld(w, u):
    return int(np.sum(np.cumsum(np.asarray(w, dtype=LD).ravel()) < LD(u)))


class Model:
    """generic_model.GenericModel's handles batched over the particles, evaluated in float64 (what a device handle returns)."""

    def __init__(self, m, p):
        self.m = m
        Q = np.asarray(p["Q"], dtype=np.float64)
        self.Lq = np.linalg.cholesky(np.atleast_2d(p["dt"] * Q))

    def dyn(self, xn, dx, z):
        """xn [n_nonlin x N], z [N x n_w] -> [n_nonlin x N]"""
        m = self.m
        return xn + m.bend * np.sin(xn) + (m.A @ dx)[:, None] + m.G @ (self.Lq @ z.T)

    def meas(self, xn):
        return self.m.measModel(xn)


def case(shape, N_P, N_T, seed=3, x0_cols=1):
    """(model, problem): generic_ny_cases.case with the map (mean, V), y simulated from it, and x0_nonLin as one column or N_P."""
    m, p = gc.case(shape, N_P, N_T, seed=seed)
    rs = np.random.RandomState(4000 + seed)
    n, d, nN = m.nLin, m.ny, m.nNonLin
    p["mean"] = p["x0_lin"] + 0.05 * rs.standard_normal(n)
    p["V"] = np.tril(rs.standard_normal((n, n))) * np.sqrt(0.1 / n)         # |V h|^2 ~ 0.1 / n * n / 2 * |h|^2 ~ 0.03: R's order
    xl_true = p["mean"] + p["V"].T @ rs.standard_normal(n)
    mdl = Model(m, p)
    Lr = np.linalg.cholesky(p["R"])
    x = np.asarray(p["x0_nonLin"], dtype=np.float64).reshape(nN, 1)
    y = np.zeros((N_T, d))
    for t in range(N_T):
        if t > 0:
            x = mdl.dyn(x, p["odometry"][t - 1], rs.standard_normal((1, m.nw)))
        y[t] = mdl.meas(x)[0] @ xl_true + Lr @ rs.standard_normal(d)
    p["y"] = y
    if x0_cols > 1:
        p["x0_nonLin"] = p["x0_nonLin"].reshape(nN, 1) + 0.1 * rs.standard_normal((nN, N_P))
    return m, p


def run(m, p, dtype=np.float64):
    """-> dict(ai [N_T x N_P] 0-based, logw, w [N_T x N_P], log_sum_w [N_T], traj_max, traj_mean [n_nonlin x N_T],
    xn_traj [n_nonlin x N_P x N_T], degenerate [N_T])."""
    N, T, nN = p["N_P"], p["y"].shape[0], m.nNonLin
    mdl = Model(m, p)
    sample = O.sample if dtype is np.float64 else _sample_ld
    U, Z = p["U"][0], p["Z"][0]
    x0 = np.asarray(p["x0_nonLin"], dtype=np.float64)
    xn = x0.reshape(nN, -1).copy() if x0.ndim > 1 and x0.shape[1] > 1 else np.repeat(x0.reshape(nN, 1), N, axis=1)
    w = np.full(N, dtype(1.0) / dtype(N), dtype=dtype)
    out = dict(ai=np.zeros((T, N), dtype=np.int64), logw=np.zeros((T, N), dtype=dtype), w=np.zeros((T, N), dtype=dtype),
               log_sum_w=np.zeros(T, dtype=dtype), traj_max=np.zeros((nN, T)), traj_mean=np.zeros((nN, T), dtype=dtype),
               xn_traj=np.zeros((nN, N, T)), degenerate=np.zeros(T, dtype=bool))
    out["xn_traj"][:, :, 0] = xn
    for t in range(T):
        if t != 0:
            ai = np.array([sample(w, U[t - 1, i]) for i in range(N)], dtype=np.int64)        # particleFilter.m:106
            xn = mdl.dyn(xn[:, ai], p["odometry"][t - 1], Z[t - 1])                            # :108
            out["ai"][t] = ai
            out["xn_traj"][:, :, t] = xn
            out["xn_traj"][:, :, :t] = out["xn_traj"][:, ai, :t]
        _, _, logw = weights(mdl.meas(xn), p["mean"], p["V"], p["R"], p["y"][t], dtype)
        mx = np.max(logw)
        e = np.exp(logw - mx)
        lse = mx + np.log(np.sum(e))
        w = e / np.sum(e)
        out["logw"][t], out["w"][t], out["log_sum_w"][t] = logw, w, lse
        out["degenerate"][t] = bool(lse <= np.log(1e-12))
        out["traj_max"][:, t] = xn[:, int(np.argmax(w))]
        out["traj_mean"][:, t] = np.sum(xn.astype(dtype) * w, axis=1)
    return out


# The full-run cases of the GPU tests: (shape, N_P, N_T, seed, x0_cols).  tests/test_device_map_cpu.py asserts that the float64 and
# the long-double run draw identical ancestors in every one of them: no draw sits on a bin edge.
FULL_RUNS = [
    ((3, 3, 3, 2, 64), 257, 8, 3, 1),
    ((3, 2, 3, 4, 129), 65, 6, 3, 65),
    ((4, 3, 4, 5, 200), 40, 5, 3, 1),
    ((3, 3, 3, 8, 65), 129, 6, 3, 1),
]

_RUNS = {}


def full_run(i):
    """(model, problem, float64 run) of FULL_RUNS[i], computed once."""
    if i not in _RUNS:
        shape, N, T, seed, cols = FULL_RUNS[i]
        m, p = case(shape, N, T, seed=seed, x0_cols=cols)
        _RUNS[i] = (m, p, run(m, p))
    return _RUNS[i]
