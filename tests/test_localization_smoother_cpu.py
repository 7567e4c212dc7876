"""Backward-simulation smoother for localisation, the parts that need no device: the checker itself
(tests/localization_smoother_ref.py), the margin condition on every case the GPU tests run, and the refusals that come before
any device is touched.

Measured (fp64 against long double, this file): eps_ref = max |cdf_fp64 - cdf_longdouble| is at most 5.1e-12 on the committed
cases (probe 64 x 64), the smallest margin of any draw 7.0e-6 (full run 70 x 8 x 33); logp agrees to 7.9e-13 relative to the largest
|logp| of a case or better.  logq's acos near 1 costs nothing here: acos(e0) / sin(acos(e0)) is 1 + O(angle^2), so the error of
the angle itself cancels."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import localization_ref as R
import localization_smoother_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rbpf_loc_backward_simulate", "rbpf_loc_history", "rbpf_loc_backward_workspace_bytes", "rbpf_loc_backward_step"]


def test_vectorised_quaternion_products_are_the_primitives():
    rs = np.random.RandomState(3)
    q = rs.standard_normal((4, 9))
    q /= np.linalg.norm(q, axis=0)
    p = rs.standard_normal(4)
    for dtype in (np.float64, np.longdouble):
        qd, pd = q.astype(dtype), p.astype(dtype)
        for i in range(q.shape[1]):
            assert np.max(np.abs(S.qright_mul(qd, pd)[:, i] - R._qRight(qd[:, i]) @ pd)) < 1e-15
            assert np.max(np.abs(S.qleft_mul(qd, pd)[:, i] - R._qLeft(qd[:, i]) @ pd)) < 1e-15
    import rbpf_oracle as O
    for i in range(q.shape[1]):
        assert np.max(np.abs(S.logq(q[:, i:i + 1])[:, 0] - O.logq(q[:, i]))) < 1e-15


def test_logp_inverts_the_dyn_model():
    """x' = dyn_model(x, dx, dt, Q, z) with a diagonal Q: the residual is z again."""
    import cases
    rs = np.random.RandomState(5)
    worst = 0.0
    for trial in range(20):
        q = rs.standard_normal(4)
        q /= np.linalg.norm(q)
        x = np.concatenate((3.0 * rs.standard_normal(3), q))
        dx = np.concatenate((0.1 * rs.standard_normal(3), R._expq(0.05 * rs.standard_normal(3))))
        Q = cases.Q_MAG if trial % 2 else np.diag(rs.random_sample(6) + 0.1)
        dt = 0.01 * (1 + trial)
        z = rs.standard_normal(6)
        xp = R.dyn_model(x, dx, dt, Q, z)
        got = S.residual(xp, x.reshape(7, 1), dx, dt, Q)[:, 0]
        worst = max(worst, float(np.max(np.abs(got - z))))
        assert abs(S.logp(xp, x.reshape(7, 1), dx, dt, Q)[0] + 0.5 * z @ z) < 1e-9
    print("largest |residual - z|:", worst)
    assert worst < 1e-10


def test_backward_simulation_frequencies_match_the_ffbsm_marginals():
    """Known answer: over M = 20000 draws the index frequencies at every (t, i) agree with the O(N^2) smoothing marginals within
    five binomial standard deviations (+ 1 / M).  The seed is fixed, so the outcome is deterministic."""
    c = R.loc_case(30, 6, 13)
    X, W = S.forward_arrays(c)
    T, N = W.shape
    M = 20000
    u = np.random.RandomState(99).random_sample((T, M))
    out = S.backward_simulate(X, W, c["odometry"], c["Q"], c["dt"], u)
    p = np.asarray(S.ffbsm_marginals(X, W, c["odometry"], c["Q"], c["dt"]), dtype=np.float64)
    assert np.max(np.abs(p.sum(axis=1) - 1.0)) < 1e-12
    f = np.stack([np.bincount(out["index"][t], minlength=N) for t in range(T)]) / M
    bound = 5.0 * np.sqrt(p * (1.0 - p) / M) + 1.0 / M
    print("largest |f - p| / bound:", float(np.max(np.abs(f - p) / bound)))
    assert np.all(np.abs(f - p) <= bound)
    print("largest |p_smooth - w_filter|:", float(np.max(np.abs(p - W))))
    assert np.max(np.abs(p[1:T - 1] - W[1:T - 1])) > 20.0 / M             # smoothing moved the marginals: the filter's weights would fail


def _check_margins(name, margin, eps_ref, logp_rel):
    print(f"{name}: min margin {float(np.min(margin)):.3e}, eps_ref {float(np.max(eps_ref)):.3e}, logp fp64 vs long double {logp_rel:.3e}")
    assert np.all(margin >= 100.0 * eps_ref)                               # every draw: none is excluded
    assert logp_rel <= 1e-10


@pytest.mark.parametrize("N,M", S.PROBE_LOGP_SHAPES + S.PROBE_INDEX_SHAPES)
def test_margin_condition_of_the_probe_cases(N, M):
    p = S.probe_case(N, M)
    o = S.backward_step(p["X"], p["w"], p["xs_next"], p["odo"], p["dt"], p["Q"], p["u"])
    rel = float(np.max(np.abs(o["logp"] - o["logp_ld"])) / np.max(np.abs(o["logp_ld"])))
    _check_margins(f"probe {N} x {M}", o["margin"], o["eps_ref"], rel)
    np.testing.assert_array_equal(o["index"], o["index_ld"])
    assert np.all(p["w"][o["index"]] > 0)


@pytest.mark.parametrize("N_P,N_T,M,glob", S.FULL_RUNS)
def test_margin_condition_of_the_full_runs(N_P, N_T, M, glob):
    """On the restatement's own forward pass (the device's differs from it by rounding; the GPU test repeats the check on the
    device's arrays)."""
    c = R.loc_case(N_P, N_T, 13, global_init=glob)
    X, W = S.forward_arrays(c)
    o = S.backward_simulate(X, W, c["odometry"], c["Q"], c["dt"], S.full_run_uniforms(N_T, M))
    _check_margins(f"full run {N_P} x {N_T} x {M} glob={glob}", o["margin"], o["eps_ref"], o["logp_rel"])
    np.testing.assert_array_equal(o["index"], o["index_ld"])
    np.testing.assert_array_equal(o["index"][N_T - 1], [R._sample(W[N_T - 1], uu) for uu in S.full_run_uniforms(N_T, M)[N_T - 1]])


def test_prototypes_exports_and_refusals_before_any_device(rbpf):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rbpf.h")).read(), flags=re.S)
    lib = rbpf.load_library()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in rbpf.EXPORTS and hasattr(lib, name)
    assert lib.rbpf_abi_version() == 9 and lib.rbpf_abi_sizeof(14) == -1
    nbytes = C.c_size_t(0)
    assert lib.rbpf_loc_backward_workspace_bytes(70, 8, 33, C.byref(nbytes)) == rbpf.RBPF_OK and nbytes.value > 8 * 8 * 70
    small = nbytes.value
    assert rbpf.loc_backward_workspace_bytes(70, 8, 66) > small
    for bad in ((0, 8, 33), (70, 0, 33), (70, 8, 0)):
        assert lib.rbpf_loc_backward_workspace_bytes(*bad, C.byref(nbytes)) == rbpf.RBPF_ERR_INVALID_ARG
    assert lib.rbpf_loc_backward_simulate(None, 4, None, 1, None, None, None) == rbpf.RBPF_ERR_INVALID_ARG
    assert b"localisation" in lib.rbpf_last_error()
    assert lib.rbpf_loc_history(None, None) == rbpf.RBPF_ERR_INVALID_ARG
    p = S.probe_case(70, 5)
    Q = np.eye(6)
    Q[3:6, 3:6] = 1.0                                                      # sqrt element-wise: a rank-one block
    with pytest.raises(rbpf.RBPFError) as ei:
        rbpf.loc_backward_step(p["X"], p["w"], p["xs_next"], p["odo"], p["dt"], Q, p["u"])
    assert ei.value.status == rbpf.RBPF_ERR_INVALID_ARG and "singular" in str(ei.value)
    Q = np.eye(6)
    Q[0, 1] = Q[1, 0] = -0.1
    with pytest.raises(rbpf.RBPFError) as ei:
        rbpf.loc_backward_step(p["X"], p["w"], p["xs_next"], p["odo"], p["dt"], Q, p["u"])
    assert ei.value.status == rbpf.RBPF_ERR_INVALID_ARG


def test_philox_backward_uniforms_are_uniforms(rbpf):
    u = rbpf.PhiloxRNG(11).backward_uniforms(1000, 7)
    assert u.shape == (7, 1000) and np.all(u > 0) and np.all(u < 1) and abs(u.mean() - 0.5) < 0.02
    assert not np.array_equal(u, rbpf.PhiloxRNG(12).backward_uniforms(1000, 7))
    np.testing.assert_array_equal(u[:, :10], rbpf.PhiloxRNG(11).backward_uniforms(10, 7))    # counter-based: column j is its own


def test_one_shot_recognises_the_handles_of_a_map_only(rbpf):
    c = R.loc_case(8, 3, 13)
    slam = rbpf.DenseMagModel(c["NN"], c["L"])
    mp = rbpf.DenseMagMap(slam, c["mean"], c["V"], c["sigma2"])
    args = (c["odometry"], c["y"], c["x0_nonLin"], c["Q"], np.eye(3), c["N_P"], 4, c["dt"])
    for dyn, meas in ((lambda *a: None, lambda *a: None), (slam.dynModel, slam.measModel), (mp.dynModel, slam.measModel)):
        with pytest.raises(rbpf.RBPFError) as ei:
            rbpf.particleSmootherLocalization(dyn, meas, *args)
        assert ei.value.status == rbpf.RBPF_ERR_UNSUPPORTED
    with pytest.raises(ValueError):                                        # a replayed forward pass needs the backward uniforms too
        rbpf.particleSmootherLocalization(mp.dynModel, mp.measModel, *args, rng=rbpf.ReplayRNG(c["U"], c["Z"]))
