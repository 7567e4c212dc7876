"""The device EKF's schedule (csrc/rbpf_ekf.hip), restated in numpy, against the oracle's ekf_dense -- no device needed.

The device does not evaluate ekf_dense.m:87-92 literally.  Per step it
  * never forms Pp = Pf + G Qt G': the 6 x 6 block D = G Qt G' is added on the fly;
  * updates with Pf = Pp - PH M PH', PH = Pp dy', M = inv(SS) (inv(SSj) SS inv(SSj) after a jitter retry) instead of K SS K';
  * carries PH: the update pass of step t accumulates Pf_t dy_{t+1}' while it writes Pf_t, and step t + 1 adds D dy(:,1:6)'.
`schedule` below does exactly that (with numpy's sums in place of the kernels' reduction trees) and must stay within 1e-12 of
the oracle (relative to the largest magnitude of each output, as the project's EKF tolerance is stated) at the shapes of the
GPU tests up to m = 253.

Measured here at n = 49, 70, 134 and 262: 1.5e-15 .. 1.9e-15 on xf_traj, <= 5e-22 on qnb_traj, 3.5e-16 .. 5.9e-16 on Pf_traj.
(In numpy the carried product and a product in a pass of its own are the same expression P @ dy.T; what the restatement
checks of the carried form is the algebra -- the block correction and which P and dy each product sees.  The kernels' own
summation order is covered by the GPU tests.)"""
import numpy as np
import pytest

import cases
import rbpf_oracle as O

TOL = 1e-12
SHAPES = [(40, 14, 8), (61, 14, 5), (125, 40, 3), (253, 24, 2)]               # (m, N_T, seed) of tests/test_gpu_ekf_device.py


def ekf_inputs(c):
    """x0, q0, P0 as run_dense3D_magfield.m:248-250 builds them (tests/test_gpu_helpers.py::test_ekf_baseline_matches_oracle)."""
    n = c["m"] + 3
    x0 = np.concatenate((c["x0_nonLin"][0:3], np.zeros(3), np.asarray(c["x0_lin"]).ravel()))
    P0 = np.zeros((6 + n, 6 + n))
    P0[6:, 6:] = c["P0_lin"]
    return x0, c["x0_nonLin"][3:7], P0


def schedule(model, LL, odometry, y, x0, q0, P0, Q, R, dt):
    y, odometry = np.atleast_2d(y), np.atleast_2d(odometry)
    N_T, n = y.shape[0], x0.size
    Qp, dtv = O._expand_Q_dt(Q, dt, N_T)
    x, q, P = x0.copy(), q0.copy(), P0.copy()
    xf_traj, qnb_traj, Pf_traj = np.zeros((n, N_T)), np.zeros((4, N_T)), np.zeros((n, n, N_T))
    D = np.zeros((6, 6))
    yhat, dy = O.measModel_ekf(model, LL, x, q)
    PHacc = P @ dy.T                                                          # the pass before step 0
    for t in range(N_T):
        PH = PHacc.copy()
        PH[0:6] += D @ dy[:, 0:6].T
        SS = dy @ PH + R
        try:
            cS, jit = np.linalg.cholesky(SS), False
        except np.linalg.LinAlgError:
            cS, jit = O._chol_lower_with_jitter(SS, 1e-3), True
        Si = np.linalg.solve(cS.T, np.linalg.solve(cS, np.eye(3)))
        M = Si @ SS @ Si if jit else Si
        x = x + PH @ np.linalg.solve(cS.T, np.linalg.solve(cS, y[t] - yhat))
        U = M @ PH.T
        q = O.qLeft(O.expq(x[3:6] / 2.0)) @ q
        x[3:6] = 0.0
        xf_traj[:, t], qnb_traj[:, t] = x, q
        Pd = P.copy()
        Pd[0:6, 0:6] += D
        A = Pd - PH @ U
        P = 0.5 * (A + A.T)
        Pf_traj[:, :, t] = P
        if t + 1 < N_T:
            x, q, _, G = O.dynModel_ekf(x, q, odometry[t])
            D = G[0:6] @ (dtv[t] * Qp[:, :, t]) @ G[0:6].T
            yhat, dy = O.measModel_ekf(model, LL, x, q)
            PHacc = P @ dy.T                                                  # accumulated by the update pass of step t
    return xf_traj, qnb_traj, Pf_traj


def distances(got, ref):
    return [float(np.max(np.abs(g - r)) / max(1.0, float(np.max(np.abs(r))))) for g, r in zip(got, ref)]


@pytest.mark.parametrize("m,N_T,seed", SHAPES)
def test_device_schedule_matches_oracle(m, N_T, seed):
    c = cases.mag_case(4, N_T, m, seed=seed)
    x0, q0, P0 = ekf_inputs(c)
    args = (c["model"], c["LL"], c["odometry"], c["y"], x0, q0, P0, c["Q"], c["R"], c["dt"])
    ref = O.ekf_dense(*args)
    dist = distances(schedule(*args), ref)
    print(f"n = {m + 9}: schedule - oracle {dist}")
    assert max(dist) <= TOL


def test_device_schedule_takes_the_jitter_branch():
    """P0 = 0, Q = 0, R = -5e-4 I: every step fails the first factorisation and passes the second (ekf_dense.m:83-86); P stays
    zero and the oracle finite.  R = -I fails both."""
    c = cases.mag_case(4, 14, 40, seed=8)
    x0, q0, P0 = ekf_inputs(c)
    args = (c["model"], c["LL"], c["odometry"], c["y"], x0, q0, np.zeros_like(P0), np.zeros((6, 6)))
    ref = O.ekf_dense(*args, -5e-4 * np.eye(3), c["dt"])
    assert all(np.isfinite(r).all() for r in ref) and not ref[2].any()
    got = schedule(*args, -5e-4 * np.eye(3), c["dt"])
    assert max(distances(got, ref)) <= TOL
    with pytest.raises(O.CholeskyFailure):
        O.ekf_dense(*args, -np.eye(3), c["dt"])
    with pytest.raises(O.CholeskyFailure):
        schedule(*args, -np.eye(3), c["dt"])
