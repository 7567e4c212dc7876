"""Localisation in the fixed landmark map of a sparseFeatures model, restated in numpy: particleFilter.m:100-161 with the branch of
:127-137, xl = mean and P = V'V the same for every particle and never updated (:163-204 left out).  Per step t, with
ind = ~isnan(y(t,:)), M = |ind|, and per particle i, with (yhat_i, H_i) = measModel(xn_i, mean),

    e = y_t(ind)' - yhat_i(ind),   S = (V H_i(ind,:)')'(V H_i(ind,:)') + R(ind,ind),
    logw_i = -sum log diag chol S - |chol(S) \\ e|^2 / 2 - M log(2 pi) / 2                                  (:129-136,145-150)

(M = 0: logw = 0), then the normalisation, traj_max / traj_mean, ai(i) = sample(w) on the replayed uniforms, xn = dynModel(xn_(ai)) on
the replayed normals, xn_traj through the ancestor table, and yhattraj(:,t) = the whole yhat of step t's maximum-weight particle.
Runs in float64 and in np.longdouble: the handles' outputs and the states are float64 in both, as the device is handed them; the
draws are rbpf_oracle.sample in float64 and its long-double twin otherwise.  The factorisation and the solve are
device_map_ref.chol / forward.

The problems are sparse_models.range_bearing_case / range_only_case (y with NaN patterns) with the map mean = column 0 of the
case's x0_lin and V = tril(randn) sqrt(0.02 / nLin) from a seeded stream.  Shared by tests/test_landmark_map_cpu.py and
tests/test_gpu_landmark_map.py; nothing in the package imports it."""
import numpy as np

import device_map_ref as dm
import generic_ny_cases as gc
import rbpf_oracle as O
import sparse_models as sm

LD = np.longdouble


def weights(yhat, H, V, R, y, dtype=np.float64):
    """yhat [N x n_y], H [N x n_y x nLin], y [n_y] with NaN = not observed -> (S [N x M x M] before R is added, logw [N]) in `dtype`.
    Rows of yhat / H of unobserved outputs are selected away before anything is computed."""
    y = np.asarray(y, dtype=np.float64).ravel()
    ind = np.flatnonzero(~np.isnan(y))
    M = ind.size
    N = np.asarray(H).shape[0]
    if M == 0:
        return np.zeros((N, 0, 0), dtype=dtype), np.zeros(N, dtype=dtype)
    H = np.asarray(H, dtype=np.float64)[:, ind, :].astype(dtype)
    n = H.shape[2]
    V = np.tril(np.asarray(V, dtype=np.float64)).astype(dtype)
    R = np.asarray(R, dtype=np.float64).reshape(y.size, y.size)[np.ix_(ind, ind)].astype(dtype)
    e = y[ind].astype(dtype)[None, :] - np.asarray(yhat, dtype=np.float64)[:, ind].astype(dtype)
    Y = (H.reshape(N * M, n) @ V.T).reshape(N, M, n)                      # row (i, k) = V H_i(ind_k, :)'
    S = np.einsum("iar,ibr->iab", Y, Y)
    logw = np.zeros(N, dtype=dtype)
    c = dtype(0.5) * dtype(M) * np.log(dtype(2.0) * dtype(np.pi))
    for i in range(N):
        L = dm.chol(S[i] + R)
        z = dm.forward(L, e[i])
        logw[i] = -np.sum(np.log(np.diag(L))) - dtype(0.5) * (z @ z) - c
    return S, logw


def meas(model, xn, mean):
    """The numpy model's measModel over the particles: xn [n_nonlin x N] -> (yhat [N x n_y], H [N x n_y x nLin])."""
    out = [model.measModel(xn[:, i], mean) for i in range(xn.shape[1])]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def dyn(p, xn, t, z):
    """sparse_models._AdditiveDyn.dynModel over the particles, in the operation order of its torch twin: xn [3 x N], z [N x 3]."""
    Lq = np.linalg.cholesky(p["dt"] * np.atleast_2d(np.asarray(p["Q"], dtype=np.float64)))
    return xn + np.asarray(p["odometry"][t], dtype=np.float64).reshape(-1, 1) + Lq @ z.T


def case(kind, L, N_P, N_T, seed, R_full=False, pattern=None):
    """The problem dict of sparse_models with the map (mean, V) added; kind "rb" (range and bearing) or "ro" (ranges in 3-D)."""
    p = sm.range_bearing_case(L, N_P, N_T, seed=seed, pattern=pattern) if kind == "rb" else sm.range_only_case(L, N_P, N_T, seed=seed)
    x0 = np.asarray(p["x0_lin"], dtype=np.float64)
    p["mean"] = (x0[:, 0] if x0.ndim == 2 else x0).copy()
    n = p["mean"].size
    p["V"] = np.tril(np.random.RandomState(7000 + seed).standard_normal((n, n))) * np.sqrt(0.02 / n)
    if R_full:
        p["R"] = gc.full_R(p["model"].ny, seed)
    return p


def run(p, dtype=np.float64):
    """-> dict(ai [N_T x N_P] 0-based, logw, w [N_T x N_P], log_sum_w [N_T], traj_max, traj_mean [3 x N_T], xn_traj [3 x N_P x N_T],
    yhattraj [n_y x N_T], iw_max [N_T], n_obs [N_T], ess [N_T], degenerate [N_T])."""
    model = p["model"]
    N, T, nN, d = p["N_P"], p["y"].shape[0], 3, p["y"].shape[1]
    sample = O.sample if dtype is np.float64 else dm._sample_ld
    U, Z = p["rng"].U[0], p["rng"].Z[0]
    xn = np.repeat(np.asarray(p["x0_nonLin"], dtype=np.float64).reshape(nN, 1), N, axis=1)
    w = np.full(N, dtype(1.0) / dtype(N), dtype=dtype)
    out = dict(ai=np.zeros((T, N), dtype=np.int64), logw=np.zeros((T, N), dtype=dtype), w=np.zeros((T, N), dtype=dtype),
               log_sum_w=np.zeros(T, dtype=dtype), traj_max=np.zeros((nN, T)), traj_mean=np.zeros((nN, T), dtype=dtype),
               xn_traj=np.zeros((nN, N, T)), yhattraj=np.zeros((d, T)), iw_max=np.zeros(T, dtype=np.int64),
               n_obs=np.zeros(T, dtype=np.int64), ess=np.zeros(T), degenerate=np.zeros(T, dtype=bool))
    out["xn_traj"][:, :, 0] = xn
    for t in range(T):
        if t != 0:
            ai = np.array([sample(w, U[t - 1, i]) for i in range(N)], dtype=np.int64)        # particleFilter.m:106
            xn = dyn(p, xn[:, ai], t - 1, Z[t - 1])                                            # :108
            out["ai"][t] = ai
            out["xn_traj"][:, :, t] = xn
            out["xn_traj"][:, :, :t] = out["xn_traj"][:, ai, :t]
        yhat, H = meas(model, xn, p["mean"])
        _, logw = weights(yhat, H, p["V"], p["R"], p["y"][t], dtype)
        mx = np.max(logw)
        e = np.exp(logw - mx)
        lse = mx + np.log(np.sum(e))
        w = e / np.sum(e)
        iw = int(np.argmax(w))
        out["logw"][t], out["w"][t], out["log_sum_w"][t] = logw, w, lse
        out["degenerate"][t] = bool(lse <= np.log(1e-12))
        out["traj_max"][:, t] = xn[:, iw]
        out["traj_mean"][:, t] = np.sum(xn.astype(dtype) * w, axis=1)
        out["yhattraj"][:, t], out["iw_max"][t] = yhat[iw], iw
        out["n_obs"][t] = int(np.count_nonzero(~np.isnan(p["y"][t])))
        out["ess"][t] = float(1.0 / np.sum(w.astype(np.float64) ** 2))
    return out


# The full-run cases of the GPU tests: (kind, landmarks L, N_P, N_T, seed, full R, pattern of the first steps).  They cover
# (n_y, nLin) = (32, 32), (6, 6), (32, 96), (17, 51), (16, 16); the last one has a full R, a step with nothing observed and one with
# only the last output (n_y, nLin = 10, 10).  tests/test_landmark_map_cpu.py asserts that the float64 and the long-double run draw
# identical ancestors in every one of them: no draw sits on a bin edge.
FULL_RUNS = [
    ("rb", 16, 65, 7, 1, False, None),
    ("rb", 3, 129, 8, 2, False, None),
    ("ro", 32, 40, 6, 1, False, None),
    ("ro", 17, 257, 6, 3, False, None),
    ("rb", 8, 64, 9, 4, False, None),
    ("rb", 5, 48, 6, 5, True, ["all", "none", "last"]),
]


def run_id(i):
    kind, L = FULL_RUNS[i][:2]
    return "%s_L%d" % (kind, L)


_RUNS = {}


def full_run(i):
    """(problem, float64 run) of FULL_RUNS[i], computed once."""
    if i not in _RUNS:
        kind, L, N, T, seed, R_full, pattern = FULL_RUNS[i]
        p = case(kind, L, N, T, seed, R_full=R_full, pattern=pattern)
        _RUNS[i] = (p, run(p))
    return _RUNS[i]
