"""Localisation in a fixed GP map on the device against the restatement (tests/localization_ref.py) on replayed random streams.

Tolerance: the project's own, 1e-9 relative to the largest magnitude of the quantity; ancestor indices exact.  Every full-run
case is one for which the fp64 and the long-double restatement draw identical ancestors at every step (asserted here; for the
m = 1000 cases the long-double ancestors are stored under tests/golden/, computing them takes one to five minutes each).

Measured on the MI355X: the restatement's own error e_ref = |fp64 - long double| on the weights is 6e-15 .. 3e-14 relative in
these cases, the device's distance from the fp64 restatement 2e-15 .. 3e-14 (weights), <= 1.2e-15 (trajectories), <= 7e-15
(log sum w); rbpf_loc_predict alone is within 9e-16 at every n.  The 1e-9 bound was not widened."""
import os
import warnings

import numpy as np
import pytest

import cases
import localization_ref as R
import rbpf_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-9
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want)) / max(float(np.max(np.abs(want))), 1e-300))


def _device_map(rbpf, c, **kw):
    model = rbpf.DenseMagModel(c["NN"], c["L"])
    return rbpf.DenseMagMap(model, c["mean"], c["V"], c["sigma2"], **kw)


def _run_device(rbpf, c, mp, rng=None, **kw):
    rng = rng if rng is not None else rbpf.ReplayRNG(c["U"], c["Z"])
    return rbpf.particleFilterLocalization(mp.dynModel, mp.measModel, c["odometry"], c["y"], c["x0_nonLin"], c["Q"], np.eye(3),
                                           c["N_P"], c["dt"], rng=rng, extras=True, **kw)


def _compare(out, ref):
    tmax, tmean, ex = out
    np.testing.assert_array_equal(ex["ai"][1:], ref["ai"][1:])
    figures = dict(w=_rel(ex["w"], ref["w"]), traj_max=_rel(tmax, ref["traj_max"]), traj_mean=_rel(tmean, ref["traj_mean"]),
                   xn_traj=_rel(ex["xn_traj"], ref["xn_traj"]), log_sum_w=_rel(ex["log_sum_w"], ref["log_sum_w"]))
    print("relative distances device - restatement:", figures)
    for k, v in figures.items():
        assert v < TOL, (k, v)
    assert ex["first_degenerate_step"] == -1 and not ref["degenerate"].any()


@pytest.mark.parametrize("n", [4, 16, 133, 515, 1003, 1151])
def test_predict_kernel_means_and_variances(rbpf, n):
    m = n - 3
    rs = np.random.RandomState(n)
    L, NN = O.domain_cartesian_dx(m, 3, np.array([[-9.0, -7.0, -2.5], [9.0, 7.0, 2.5]]))
    V = np.tril(rs.standard_normal((n, n))) / np.sqrt(n)
    mean = rs.standard_normal(n)
    mp = rbpf.DenseMagMap(rbpf.DenseMagModel(NN, L), mean, V, 1.0)
    for n_pred in (1, 63, 64, 65, 1000):
        pos = np.column_stack([rs.uniform(-L[a], L[a], n_pred) for a in range(3)])
        dE, var, _ = mp.predict(pos.T)
        dE_ref, var_ref = R.predict(NN, L, mean, pos, V=V)
        e1, e2 = _rel(dE, dE_ref), _rel(var, var_ref)
        print(f"n = {n}, n_pred = {n_pred}: dEft {e1:.2e}, var {e2:.2e}")
        assert e1 < TOL and e2 < TOL
        dE2, none, _ = mp.predict(pos.T, want_var=False)                 # table mode of the kernel: means only
        assert none is None and _rel(dE2, dE_ref) < TOL


def test_dyn_model_against_the_restatement(rbpf):
    c = R.loc_case(8, 6, 13, seed=2)
    mp = _device_map(rbpf, c)
    rs = np.random.RandomState(5)
    npar = 37
    q = rs.standard_normal((4, npar))
    q /= np.linalg.norm(q, axis=0)
    xn = np.vstack((rs.standard_normal((3, npar)), q))
    for trial in range(3):                                                # a time-varying Q and dt: three different pages
        A = rs.random_sample((6, 6))
        Q = A @ A.T * 10.0 ** (-trial)                                    # positive entries, full diagonal blocks
        dt = 0.01 * (trial + 1)
        dx = np.concatenate((rs.standard_normal(3), O.expq(0.2 * rs.standard_normal(3))))
        z = rs.standard_normal((6, npar))
        got = mp.dynModel(xn, dx, dt, Q, z)
        want = np.column_stack([R.dyn_model(xn[:, i], dx, dt, Q, z[:, i]) for i in range(npar)])
        assert _rel(got, want) < TOL
    Qneg = np.eye(6)
    Qneg[0, 1] = Qneg[1, 0] = -0.1                                        # MATLAB's sqrt would go complex
    with pytest.raises(rbpf.RBPFError) as ei:
        mp.dynModel(xn, dx, 0.1, Qneg, z)
    assert ei.value.status == rbpf.RBPF_ERR_INVALID_ARG


@pytest.mark.parametrize("variant", ["own", "table", "glob"])
@pytest.mark.parametrize("N_P,N_T,m", [(64, 40, 13), (256, 30, 130), (1000, 20, 1000)])
def test_full_run_matches_the_restatement(rbpf, N_P, N_T, m, variant):
    c = R.loc_case(N_P, N_T, m, seed=1, table=variant == "table", global_init=variant == "glob")
    ref = R.run_case(c)
    if m >= 1000:
        ai_ld = np.load(os.path.join(GOLDEN, f"loc_ai_longdouble_{variant}_{N_P}_{N_T}_{m}_seed1.npy"))
    else:
        ai_ld = R.run_case(c, dtype=np.longdouble)["ai"]
    np.testing.assert_array_equal(ref["ai"], ai_ld)                       # the condition on the case: no draw on a bin edge
    mp = _device_map(rbpf, c, var_points=c["var_points"])
    _compare(_run_device(rbpf, c, mp), ref)


def test_time_varying_noise_and_step(rbpf):
    c = R.loc_case(48, 12, 13, seed=4)
    rs = np.random.RandomState(9)
    T = c["y"].shape[0]
    Q = np.repeat(cases.Q_MAG[:, :, None], T, axis=2) * (0.5 + rs.random_sample(T))[None, None, :]
    Q[0, 1, :] = Q[1, 0, :] = 0.1 * Q[0, 0, :]
    c["Q"], c["dt"] = Q, 0.01 * (0.5 + rs.random_sample(T))
    ref = R.run_case(c)
    np.testing.assert_array_equal(ref["ai"], R.run_case(c, dtype=np.longdouble)["ai"])
    _compare(_run_device(rbpf, c, _device_map(rbpf, c)), ref)


def test_map_from_the_device_slam_filter(rbpf):
    s = cases.mag_case(N_P=32, N_T=12, m=130, seed=3)
    mdl, x0, P0, Rm = cases.device_model(rbpf, s)
    out = rbpf.particleFilter(mdl.dynModel, mdl.measModel, s["odometry"], s["y"], s["x0_nonLin"], x0, P0, s["Q"], Rm, s["N_P"],
                              s["dt"], rng=cases.device_rng(rbpf, s))
    xl_max, P_max = out[2], out[4]
    sigma2 = float(s["theta"][3])
    mp = rbpf.DenseMagMap.from_posterior(mdl, xl_max, P_max, sigma2)
    N_P, T = 128, s["y"].shape[0]
    rs = np.random.RandomState(77)
    U, Z = rs.random_sample((T - 1, N_P)), rs.standard_normal((T - 1, N_P, 6))
    Psym = 0.5 * (P_max + P_max.T)
    kw = dict(P=Psym)
    args = (mdl.NN, mdl.L, xl_max, sigma2, s["odometry"], s["y"], s["x0_nonLin"], s["Q"], N_P, s["dt"], U, Z)
    ref = R.particleFilterLocalization(*args, **kw)
    np.testing.assert_array_equal(ref["ai"], R.particleFilterLocalization(*args, dtype=np.longdouble, **kw)["ai"])
    got = rbpf.particleFilterLocalization(mp.dynModel, mp.measModel, s["odometry"], s["y"], s["x0_nonLin"], s["Q"], Rm, N_P, s["dt"],
                                          rng=rbpf.ReplayRNG(U, Z), extras=True)
    _compare(got, ref)


def test_philox_run_equals_its_replay(rbpf):
    c = R.loc_case(300, 10, 40, seed=6)
    mp = _device_map(rbpf, c)
    a = _run_device(rbpf, c, mp, rng=rbpf.PhiloxRNG(11))
    rep = rbpf.PhiloxRNG(11).replay(c["N_P"], c["y"].shape[0], 6)
    b = _run_device(rbpf, c, mp, rng=rbpf.ReplayRNG(rep.U[0], rep.Z[0]))
    for x, y in ((a[0], b[0]), (a[1], b[1]), (a[2]["w"], b[2]["w"]), (a[2]["ai"], b[2]["ai"]), (a[2]["xn_traj"], b[2]["xn_traj"])):
        np.testing.assert_array_equal(x, y)
    other = _run_device(rbpf, c, mp, rng=rbpf.PhiloxRNG(12))
    assert not np.array_equal(other[2]["ai"], a[2]["ai"])


def test_large_particle_count_uses_the_multi_workgroup_normalisation(rbpf):
    """N_P above the single-workgroup limit of the normalisation: same numbers as the restatement's first steps."""
    c = R.loc_case(9000, 3, 13, seed=8)
    ref = R.run_case(c)
    _compare(_run_device(rbpf, c, _device_map(rbpf, c)), ref)


def test_degenerate_weights_warn_and_carry_on(rbpf):
    c = R.loc_case(64, 8, 13, seed=1)
    c["y"] = c["y"].copy()
    c["y"][0, :] += 1e3 * np.sqrt(c["sigma2"] + 650.0)                    # 1e3 sigma of the widest predictive density
    mp = _device_map(rbpf, c)
    with pytest.warns(RuntimeWarning, match="Weights filter close to zero at t=1"):
        tmax, tmean, ex = _run_device(rbpf, c, mp)
    assert ex["first_degenerate_step"] == 0
    assert np.all(np.isfinite(ex["w"])) and np.all(np.isfinite(tmean))
    assert np.allclose(ex["w"].sum(axis=1), 1.0, atol=1e-12)


def test_make_plots_hook(rbpf):
    c = R.loc_case(32, 6, 13, seed=1)
    mp = _device_map(rbpf, c)
    calls = []

    def makePlots(xn, traj_max, yhattraj, xn_traj, traj_mean):
        calls.append((xn.shape, traj_max.shape, yhattraj.shape, xn_traj.shape, traj_mean.shape,
                      int(np.sum(~np.isnan(traj_max[0, :])))))

    with warnings.catch_warnings():
        warnings.simplefilter("error")
        rbpf.particleFilterLocalization(mp.dynModel, mp.measModel, c["odometry"], c["y"], c["x0_nonLin"], c["Q"], np.eye(3), c["N_P"],
                                        c["dt"], makePlots, rng=rbpf.ReplayRNG(c["U"], c["Z"]))
    T = c["y"].shape[0]
    assert len(calls) == T
    for t, call in enumerate(calls):
        assert call == ((7, 32), (7, T), (3, T), (7, 32, T), (7, T), t + 1)   # run_localization.m:287: sum(~isnan(traj_max(1,:)))


def test_session_advances_in_pieces(rbpf):
    c = R.loc_case(64, 10, 13, seed=1)
    mp = _device_map(rbpf, c)
    whole = _run_device(rbpf, c, mp)
    with rbpf.LocalizationSession(mp, c["odometry"], c["y"], c["x0_nonLin"], c["Q"], c["N_P"], c["dt"],
                                  rng=rbpf.ReplayRNG(c["U"], c["Z"])) as s:
        s.advance(4)
        s.sync()
        assert s.tell() == 4
        s.advance(6)
        b = s.finish()
    np.testing.assert_array_equal(b["traj_mean"], whole[1])
    np.testing.assert_array_equal(b["traj_max"], whole[0])


def test_refusals(rbpf):
    c = R.loc_case(16, 4, 13, seed=1)
    mp = _device_map(rbpf, c)
    slam = rbpf.DenseMagModel(c["NN"], c["L"])
    rng = rbpf.ReplayRNG(c["U"], c["Z"])
    args = (c["odometry"], c["y"], c["x0_nonLin"], c["Q"], np.eye(3), c["N_P"], c["dt"])
    for dyn, meas in ((lambda *a: None, lambda *a: None), (slam.dynModel, slam.measModel), (mp.dynModel, slam.measModel)):
        with pytest.raises(rbpf.RBPFError) as ei:
            rbpf.particleFilterLocalization(dyn, meas, *args, rng=rng)
        assert ei.value.status == rbpf.RBPF_ERR_UNSUPPORTED
    for kw in (dict(n_devices=2), dict(lazy_depth=2)):
        with pytest.raises(rbpf.RBPFError) as ei:
            rbpf.particleFilterLocalization(mp.dynModel, mp.measModel, *args, rng=rng, **kw)
        assert ei.value.status == rbpf.RBPF_ERR_UNSUPPORTED
    short = _device_map(rbpf, c, var_points=np.zeros((c["N_P"] - 1, 3)))
    with pytest.raises(ValueError):
        rbpf.particleFilterLocalization(short.dynModel, short.measModel, *args, rng=rng)
