"""CPU: the restatement of the running two-slice statistics (tests/forward_stats_ref.py) against the offline statistics
(tests/pair_stats_ref.py): at the last step the forward-only recursion gives sum_t S_t / dt_t and sum_t m_t, the same estimator in
another order of sums; -inf weights; running_noise_estimate; the new ABI symbols, the workspace sizes stated in include/rbpf.h and the
ABI version."""
import os
import re

import numpy as np
import pytest

import device_map_smoother_ref as S
import forward_stats_ref as FS
import localization_ref as R
import map_trajectory_ref as V
import pair_stats_ref as PS
import pose_transition_ref as P

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, T = 24, 6


def _small(kind):
    """(X [T x n x N], W [T x N], lp_of, r_of_t, dt [T-1]) of one case of a family at N = 24, N_T = 6, on the restatement's forward
    pass: the dense-mag map, a Gaussian case with an angle row (D), a pose case (E)."""
    if kind == "mag":
        c = R.loc_case(N, T, 13)
        X, W = V.forward_mag(c)
        dt, Q = V.pages(c, T)
        return (X, W, lambda t: V.lp_mag(X[t + 1], X[t], c["odometry"][t], dt[t], Q[:, :, t]),
                lambda t: PS.r_mag(X[t + 1], X[t], c["odometry"][t], dt[t], Q[:, :, t]), dt[:T - 1])
    c = S.case("D", N, T) if kind == "gauss" else P.case("E", N, T)
    X, W, _ = S.forward_arrays(c)
    mus, covs = S.transition_arrays(c, X)
    return (X, W, lambda t: V.lp_case(c, X[t + 1], mus[t], covs[t]), lambda t: PS.r_of_case(c, X[t + 1], mus[t], covs[t]),
            FS.steps_dt(c.p["dt"], T))


@pytest.mark.parametrize("kind", ["mag", "gauss", "pose"])
def test_the_last_page_is_the_sum_of_the_offline_statistics(kind):
    X, W, lp_of, r_of_t, dt = _small(kind)
    assert X.shape[0] == T and W.shape == (T, N) and N <= 40
    fwd = FS.recursion(X, W, lp_of, r_of_t, dt)
    off = PS.recursion(X, W, lp_of, r_of_t)
    want_S = sum(off["S"][t] / LD(dt[t]) for t in range(T - 1))
    want_m = sum(off["m"][t] for t in range(T - 1))
    sS = float(np.max(np.abs(want_S)))
    sm = float(np.sqrt(np.max(np.diag(want_S))))
    eS = float(np.max(np.abs(fwd["S_run"][-1] - want_S))) / sS
    em = float(np.max(np.abs(fwd["m_run"][-1] - want_m))) / sm
    ep = float(np.max(np.abs(fwd["mass_run"] - 1.0)))
    er = float(np.max(np.abs(fwd["reach"] - 1.0)))
    print(f"{kind}: last page against the offline sums: S {eS:.2e} of {sS:.3g}, m {em:.2e} of {sm:.3g}; |mass_run - 1| {ep:.2e}, |reach - 1| {er:.2e}")
    tol = 1e-15 * (T - 1)
    assert fwd["S_run"].dtype == LD and eS <= tol and em <= tol and ep <= tol and er <= tol
    # page 0 is one offline step of a run that ended at step 1: w_{1|1} = w_1
    D, c, lws = FS.G.step(V.log_weights(W[0]), lp_of(0), V.log_weights(W[1]))
    S0, m0, pm0 = PS.moments(V.log_weights(W[0]), c, lp_of(0), PS.log_mass(lws), r_of_t(0))
    assert float(np.max(np.abs(fwd["S_run"][0] - S0 / LD(dt[0])))) <= tol * float(np.max(np.abs(S0 / LD(dt[0]))))
    assert float(np.max(np.abs(fwd["m_run"][0] - m0))) <= tol * float(np.sqrt(np.max(np.diag(S0))))


def test_minus_infinity_weights_contribute_exactly_nothing():
    rs = np.random.RandomState(5)
    n, Np, M = 3, 9, 5
    X = rs.standard_normal((2, 3, Np))
    cov = 0.5 * np.eye(3)
    xs = X[1][:, :M]
    lp = V.lp_gauss(xs, X[0], cov, (0, 1, 2))
    logw = np.log(rs.random_sample(Np) + 0.1)
    dead = [2, 7]
    logw[dead] = -np.inf
    tS, tm = FS.carry(n, Np, 3)
    a = FS.step(logw, lp, (tS, tm), PS.r_gauss(xs, X[0], cov, (0, 1, 2)), 0.7)
    # whatever the dead predecessors carry and wherever they lie: bit for bit the same
    tS2, tm2, X2 = tS.copy(), tm.copy(), X.copy()
    tS2[:, :, dead], tm2[:, dead], X2[0][:, dead] = 1e300, -1e300, 1e150
    b = FS.step(logw, V.lp_gauss(xs, X2[0], cov, (0, 1, 2)), (tS2, tm2), PS.r_gauss(xs, X2[0], cov, (0, 1, 2)), 0.7)
    for k in ("D", "tau_S", "tau_m", "reach"):
        np.testing.assert_array_equal(a[k], b[k])
    # ... and the answer of the inputs without them
    keep = [i for i in range(Np) if i not in dead]
    c = FS.step(logw[keep], lp[keep], (tS[:, :, keep], tm[:, keep]), PS.r_gauss(xs, X[0][:, keep], cov, (0, 1, 2)), 0.7)
    for k in ("D", "tau_S", "tau_m", "reach"):
        assert float(np.max(np.abs(a[k] - c[k]))) <= 1e-17 * 10
    assert float(np.max(np.abs(a["reach"] - 1.0))) <= 1e-17 * 10
    # every predecessor dead: D = -inf, tau = 0 and reach = 0, no NaN
    z = FS.step(np.full(Np, -np.inf), lp, (tS, tm), PS.r_gauss(xs, X[0], cov, (0, 1, 2)), 0.7)
    assert np.all(z["D"] == -np.inf) and np.all(z["tau_S"] == 0) and np.all(z["tau_m"] == 0) and np.all(z["reach"] == 0)
    # s_scale = 0 and no m part to add would leave the plain omega-average of the incoming carry: check the S part
    q = FS.step(logw, lp, (tS, tm), PS.r_gauss(xs, X[0], cov, (0, 1, 2)), 0.0)
    live = np.nonzero(logw > -np.inf)[0]
    for j in range(M):
        w = np.exp(np.asarray(logw, dtype=LD)[live] + lp[live, j] - q["D"][j])
        assert float(np.max(np.abs(q["tau_S"][:, :, j] - np.sum(tS[:, :, live] * w[None, None, :], axis=2)))) <= 1e-17 * 10


def test_running_noise_estimate(rbpf):
    rs = np.random.RandomState(3)
    n, Pg = 3, 5
    Q = np.array([[2.0, 0.3, 0.0], [0.3, 1.0, 0.1], [0.0, 0.1, 0.5]])
    S_run = np.stack([(k + 1) * Q for k in range(Pg)], axis=2)            # exact statistics of a known Q give it back on every page
    np.testing.assert_allclose(rbpf.running_noise_estimate(S_run), np.repeat(Q[:, :, None], Pg, axis=2), rtol=1e-15)
    m_run = rs.standard_normal((n, Pg))
    Qh, bias = rbpf.running_noise_estimate(S_run, m_run)
    np.testing.assert_allclose(bias, m_run / np.arange(1, Pg + 1)[None, :], rtol=1e-15)
    np.testing.assert_allclose(Qh[:, :, 3], Q, rtol=1e-15)
    np.testing.assert_allclose(rbpf.running_noise_estimate(Q), Q[:, :, None], rtol=1e-15)          # one page as a matrix
    # the last page is transition_noise_estimate's answer (un-centred) for the same run
    dt = rs.uniform(0.5, 2.0, Pg)
    A = rs.standard_normal((n, n, Pg))
    S_t = np.einsum("abt,cbt->act", A, A)
    run = np.cumsum(S_t / dt[None, None, :], axis=2)
    np.testing.assert_allclose(rbpf.running_noise_estimate(run)[:, :, -1], rbpf.transition_noise_estimate(S_t, dt), rtol=1e-13)
    for bad in (lambda: rbpf.running_noise_estimate(np.zeros((2, 3, 4))), lambda: rbpf.running_noise_estimate(S_run, m_run[:, :2])):
        with pytest.raises(ValueError):
            bad()
    assert "ELEMENT-WISE" in rbpf.running_noise_estimate.__doc__          # the dense-mag caveat of transition_noise_estimate


NEW_SYMBOLS = ["rbpf_loc_forward_stats_update", "rbpf_loc_forward_stats_reset", "rbpf_loc_forward_stats_workspace_bytes",
               "rbpf_loc_forward_stats_step", "rbpf_loc_generic_forward_stats_begin", "rbpf_loc_generic_forward_stats_particles_device",
               "rbpf_loc_generic_forward_stats_step_device", "rbpf_loc_generic_forward_stats_finish", "rbpf_loc_generic_forward_stats_reset",
               "rbpf_loc_generic_forward_stats_workspace_bytes", "rbpf_loc_generic_forward_stats_step"]


def test_the_new_symbols_are_declared_exported_and_bound(rbpf):
    lib = rbpf.load_library()
    src = open(os.path.join(ROOT, "include", "rbpf.h")).read()
    import importlib
    ffi = importlib.import_module(rbpf.__name__ + "._ffi")
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint " + name + r"\(", src), name
        assert name in ffi.EXPORTS and getattr(lib, name).argtypes is not None, name
    for name in ("particleRunningStatisticsLocalization", "loc_forward_stats_step", "device_map_forward_stats_step", "running_noise_estimate",
                 "loc_forward_stats_workspace_bytes", "device_map_forward_stats_workspace_bytes"):
        assert callable(getattr(rbpf, name))
    assert hasattr(rbpf.LocalizationSession, "running_statistics") and hasattr(rbpf.LocalizationSession, "reset_running_statistics")


def test_the_abi_version_stays_9(rbpf):
    assert rbpf.load_library().rbpf_abi_version() == 9
    assert re.search(r"#define\s+RBPF_ABI_VERSION\s+9\b", open(os.path.join(ROOT, "include", "rbpf.h")).read())


@pytest.mark.parametrize("N_P,N_T", [(1, 1), (300, 7), (513, 2), (4352, 3), (8192, 6), (65536, 100)])
def test_workspace_bytes(rbpf, N_P, N_T):
    """The sum stated at rbpf_loc_forward_stats_workspace_bytes in include/rbpf.h."""
    def stated(nN, rows, n_res, marginal_bytes):
        KF = n_res * (n_res + 3) // 2
        # P from the marginal pass's own statement: ((rows + 1) N + 2 P + 3 N + T N + (nN + nN^2 + 2) T) doubles
        P2 = marginal_bytes // 8 - ((rows + 1) * N_P + 3 * N_P + N_T * N_P + (nN + nN * nN + 2) * N_T)
        nch = FS.chunks(N_P, N_P)[1]
        return 8 * ((rows + 1) * N_P + P2 + 4 * N_P + nch * (KF + 1) * N_P + 2 * KF * N_P + max(N_T - 1, 1) * (n_res * n_res + n_res + 1))
    assert FS.chunks(300, 70) == (256, 2) and FS.chunks(513, 257) == (256, 3) and FS.chunks(600, 520) == (256, 3) and FS.chunks(1, 5) == (256, 1)
    assert FS.chunks(65536, 65536) == (16384, 4) and FS.chunks(8192, 8192) == (256, 32)       # no cap of 2048: four chunks at 65 536
    assert rbpf.loc_forward_stats_workspace_bytes(N_P, N_T) == stated(7, 7, 6, rbpf.loc_marginal_workspace_bytes(N_P, N_T))
    for nN, n_sel, qpos, n_res in ((3, 1, -1, 1), (8, 8, -1, 8), (8, 6, 1, 5), (7, 7, 3, 6), (4, 4, 0, 3)):
        assert rbpf.device_map_forward_stats_workspace_bytes(nN, n_sel, N_P, N_T, quat_pos=qpos) == \
            stated(nN, n_sel, n_res, rbpf.device_map_marginal_workspace_bytes(nN, n_sel, N_P, N_T, quat_pos=qpos))
    for bad in (lambda: rbpf.loc_forward_stats_workspace_bytes(0, N_T), lambda: rbpf.loc_forward_stats_workspace_bytes(N_P, 0),
                lambda: rbpf.device_map_forward_stats_workspace_bytes(3, 4, N_P, N_T),
                lambda: rbpf.device_map_forward_stats_workspace_bytes(8, 6, N_P, N_T, quat_pos=3)):
        with pytest.raises(rbpf.RBPFError) as ei:
            bad()
        assert ei.value.status == rbpf.RBPF_ERR_INVALID_ARG
