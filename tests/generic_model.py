"""A synthetic conditionally linear-Gaussian model family of any size the generic (host-callback) family takes, its
device-side handles, and an extended-precision known answer for its no-noise limit.

  dynModel     x' = x + 0.1 sin(x) + A dx + G chol(dt Q, 'lower') z          A: n_nonlin x n_odo, G: n_nonlin x n_w
  measModel    H(x)[k, j] = c_kj cos(omega_j . x + phi_kj)                   [N x n_y x nLin], as particleFilter.m:124 reads it
  dynResNorm   chol(dt Q)^-1 G^+ (x' - x - 0.1 sin(x) - A dx)                  (n_w values, particleSmoother.m:178-180)

A, G, omega_j, c and phi are fixed by the seed; nothing in the library knows the family, so the device runs it through
RBPF_MODEL_GENERIC_DENSE.  Used by tests/test_gpu_generic_shapes.py (against the numpy oracle and the known answer) and
tests/test_oracle_generic_kat.py (the oracle against the known answer, on the CPU)."""
import numpy as np


class GenericModel:
    """Oracle-side model object (the attributes and methods oracle/rbpf_oracle.py reads).  noise=False: dynModel ignores its
    normals, so every particle follows one deterministic path (the known-answer tests)."""

    def __init__(self, n_nonlin, n_w, n_odo, n_y, nLin, seed=0, noise=True, additive=False):
        rs = np.random.RandomState(1000 + seed)
        self.nNonLin, self.nw, self.n_odo, self.ny, self.nLin = n_nonlin, n_w, n_odo, n_y, nLin
        self.noise, self.additive = noise, additive
        if additive:                       # the additive default of an empty dynResNorm: x' = x + dx + chol(dt Q) z exactly
            assert n_w == n_nonlin == n_odo
            self.A, self.G, self.bend = np.eye(n_nonlin), np.eye(n_nonlin), 0.0
        else:
            self.A = rs.standard_normal((n_nonlin, n_odo)) / np.sqrt(n_odo)
            self.G = rs.standard_normal((n_nonlin, n_w)) / np.sqrt(n_w) + np.eye(n_nonlin, n_w)
            self.bend = 0.1
        self.Gpinv = np.linalg.pinv(self.G)
        self.omega = rs.standard_normal((nLin, n_nonlin))
        self.c = rs.uniform(0.5, 1.5, (n_y, nLin)) * rs.choice((-1.0, 1.0), (n_y, nLin)) / np.sqrt(nLin)
        self.phi = rs.uniform(0.0, 2.0 * np.pi, (n_y, nLin))

    def drift(self, xn, dx):
        xn = np.asarray(xn, dtype=np.float64).ravel()
        return xn + self.bend * np.sin(xn) + self.A @ np.asarray(dx, dtype=np.float64).ravel()

    def dynModel(self, xn, dx, dt, Q, z):
        x = self.drift(xn, dx)
        if self.noise:
            x = x + self.G @ (np.linalg.cholesky(np.atleast_2d(dt * Q)) @ np.asarray(z, dtype=np.float64).ravel())
        return x, None

    def measModel(self, xn):
        """xn [n_nonlin] or [n_nonlin x N] -> dy [N x n_y x nLin]."""
        X = np.asarray(xn, dtype=np.float64).reshape(self.nNonLin, -1)
        arg = (self.omega @ X).T                                        # [N x nLin]
        return self.c[None] * np.cos(arg[:, None, :] + self.phi[None])

    def dynResNorm(self, xnkt, xni, dx, dt, Q):
        r = self.Gpinv @ (np.asarray(xnkt, dtype=np.float64).ravel() - self.drift(xni, dx))
        Lq = np.linalg.cholesky(np.atleast_2d(dt * Q))
        return np.linalg.solve(Lq, r)


def problem(model, N_P, N_T, N_K=1, seed=0, dt=1.0):
    """Problem data with y simulated from the model (a true path, a true map drawn from the prior, measurement noise), P0
    diagonal, R SPD (with off-diagonal terms for n_y = 3), and the replayed random numbers of the reference's call order."""
    rs = np.random.RandomState(2000 + seed)
    nN, nw, nodo, ny, n = model.nNonLin, model.nw, model.n_odo, model.ny, model.nLin
    Q = np.diag(rs.uniform(0.01, 0.04, nw))
    if ny == 3:
        B = rs.standard_normal((3, 3))
        R = 0.01 * (B @ B.T) + 0.02 * np.eye(3)
    else:
        R = 0.03 * np.eye(ny)
    P0 = np.diag(rs.uniform(0.5, 1.5, n))
    x0_lin = 0.3 * rs.standard_normal(n)
    x0_nonLin = rs.uniform(-1.0, 1.0, nN)
    odometry = 0.3 * rs.standard_normal((max(N_T - 1, 1), nodo))
    xl_true = x0_lin + np.sqrt(np.diag(P0)) * rs.standard_normal(n)
    Lr = np.linalg.cholesky(R)
    x = x0_nonLin.copy()
    y = np.zeros((N_T, ny))
    for t in range(N_T):
        if t > 0:
            x = model.dynModel(x, odometry[t - 1], dt, Q, rs.standard_normal(nw))[0]
        y[t] = model.measModel(x)[0] @ xl_true + Lr @ rs.standard_normal(ny)
    U = rs.random_sample((N_K, max(N_T - 1, 0), N_P))
    Z = rs.standard_normal((N_K, max(N_T - 1, 0), N_P, nw))
    Ufin = rs.random_sample(N_K)
    return dict(odometry=odometry, y=y, x0_nonLin=x0_nonLin, x0_lin=x0_lin, P0_lin=P0, Q=Q, R=R, N_P=N_P, N_K=N_K, dt=dt,
                U=U, Z=Z, Ufin=Ufin)


def handles(model, p, use_dynResNorm=True):
    """Device-side handles: plain closures the library does not recognise.  dynModel replays the normals Z in the reference's
    call order -- per step slots 0..N_P-1 in the filter and in smoother iteration k = 0, slots 0..N_P-2 in later iterations
    (particleFilter.m:104-109, particleSmoother.m:132-137,149-152) -- so it draws what the oracle's dynModel is handed."""
    Z, N_P, N_T = p["Z"], p["N_P"], p["y"].shape[0]
    state = {"k": 0, "t": 0, "i": 0, "calls": 0}

    def dynModel(xn, dx, dt, Q):
        k, t, i = state["k"], state["t"], state["i"]
        out = model.dynModel(xn, dx, dt, Q, Z[k, t, i])[0]
        state["calls"] += 1
        i += 1
        if i == (N_P if k == 0 else N_P - 1):
            i, t = 0, t + 1
            if t == N_T - 1:
                t, k = 0, k + 1
        state.update(k=k, t=t, i=i)
        return out

    drn = (lambda xnk, xni, dx, dt, Q: model.dynResNorm(xnk, xni, dx, dt, Q)) if use_dynResNorm else []
    return dynModel, (lambda xn: model.measModel(xn)), drn, state


# ------------------------------------------------------------------------------------------------
# extended-precision known answer of the no-noise model
# ------------------------------------------------------------------------------------------------
LD = np.longdouble


def chol_ld(A):
    """Lower Cholesky factor in long double (numpy's linalg has none): right-looking, one column at a time."""
    A = np.array(A, dtype=LD)
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        d = np.sqrt(A[j, j])
        L[j, j] = d
        L[j + 1:, j] = A[j + 1:, j] / d
        A[j + 1:, j + 1:] -= np.outer(L[j + 1:, j], L[j + 1:, j])
    return L


def forward_ld(L, B):
    """L \\ B in long double, row by row."""
    X = np.zeros(B.shape, dtype=LD)
    for i in range(L.shape[0]):
        X[i] = (B[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def batch_posterior(model, p, path):
    """Known answer of a no-noise run along `path` [n_nonlin x T] (the path every particle followed): the T sequential Kalman
    updates of particleFilter.m:184-198 equal the batch posterior of all n_y T measurements with Phi = the stacked H_t,
        P_T = P0 - V'V,  xl_T = x0 + V'w,  V = L \\ (Phi P0),  w = L \\ (y - Phi x0),  L L' = C = Phi P0 Phi' + kron(I_T, R)
    (= (P0^-1 + sum_t H_t' R^-1 H_t)^-1 and P_T (P0^-1 x0 + sum_t H_t' R^-1 y_t) by the Woodbury identity), and the sum over t
    of the unnormalised log-weights (:139-150) is the log marginal likelihood log N(y; Phi x0, C).  Everything after the fp64
    H_t the device is handed is in long double.  Also returns kappa = cond_2(C), which the tolerances are built from."""
    T, ny, n = p["y"].shape[0], model.ny, model.nLin
    Phi = model.measModel(path).reshape(T * ny, n)                       # time-major rows: [H_0; H_1; ...]
    PhiL = Phi.astype(LD)
    p0 = np.diag(p["P0_lin"]).astype(LD)
    assert np.all(p["P0_lin"] == np.diag(np.diag(p["P0_lin"])))
    PhiP0 = PhiL * p0[None, :]
    C = PhiP0 @ PhiL.T
    R = p["R"].astype(LD)
    for t in range(T):
        C[t * ny:(t + 1) * ny, t * ny:(t + 1) * ny] += R
    L = chol_ld(C)
    x0 = np.asarray(p["x0_lin"], dtype=np.float64).ravel().astype(LD)
    r = p["y"].reshape(-1).astype(LD) - PhiL @ x0
    w = forward_ld(L, r[:, None])[:, 0]
    V = forward_ld(L, PhiP0)
    P = -(V.T @ V)
    P[np.diag_indices(n)] += p0
    xl = x0 + V.T @ w
    M = T * ny
    loglik = -0.5 * (w @ w) - np.sum(np.log(np.diag(L))) - LD(0.5) * M * np.log(LD(2.0) * LD(np.pi))
    ev = np.linalg.eigvalsh(C.astype(np.float64))
    return dict(xl=xl, P=P, loglik=loglik, kappa=float(ev[-1] / ev[0]), M=M, P0max=float(np.max(p0)))


def path_of(model, p):
    """The deterministic path of a no-noise model from x0_nonLin [n_nonlin x T]."""
    T = p["y"].shape[0]
    X = np.zeros((model.nNonLin, T))
    X[:, 0] = p["x0_nonLin"]
    for t in range(1, T):
        X[:, t] = model.dynModel(X[:, t - 1], p["odometry"][t - 1], p["dt"], p["Q"], None)[0]
    return X


_KAT = {}


def kat_case(shape, N_P, N_T, seed=1):
    """(model, problem, known answer) of the no-noise model at shape = (n_nonlin, n_w, n_odo, n_y, nLin); the long-double
    answer is computed once per shape and length."""
    key = (tuple(shape), N_T, seed)
    if key not in _KAT:
        m = GenericModel(*shape, seed=seed, noise=False)
        p0 = problem(m, 1, N_T, seed=seed)
        _KAT[key] = (m, p0, batch_posterior(m, p0, path_of(m, p0)))
    m, p0, ref = _KAT[key]
    rs = np.random.RandomState(seed)
    p = dict(p0, N_P=N_P, U=rs.random_sample((1, N_T - 1, N_P)), Z=np.zeros((1, N_T - 1, N_P, m.nw)), Ufin=None)
    return m, p, ref


def kat_tolerance(ref, T):
    """Bounds for an fp64 run against the long-double answer, from the problem's conditioning.  The filter performs, one
    measurement block at a time, the solve with C that the batch form does at once; a backward-stable solve of an M x M
    system loses at most about M u kappa(C) (u = 2^-53) relative to the scale of its data, and the sequential form adds one
    rounding of P per step (T u).  So, with a safety factor of 8:
        |P - P_T| <= 8 (M kappa + T) u max|P0|          (P_T = P0 - V'V: its errors are on the scale of P0)
        |xl - xl_T| <= 8 (M kappa + T) u (max|xl_T| + max|x0 - xl_T|)
        |sum_t logw_t - loglik| <= 8 (M kappa + T) u (|loglik| + M)     (w'w and log det C, each to M u kappa relative)."""
    u = 2.0 ** -53
    return 8.0 * (ref["M"] * ref["kappa"] + T) * u
