"""Backward-simulation smoother for localisation on the device against the restatement (tests/localization_smoother_ref.py).

Tolerances: logp and the smoothed mean 1e-9 relative to the largest magnitude of the quantity (the project's own); indices exact.
Every case here satisfies the margin condition (every draw at least 100 eps_ref away from a cdf edge, eps_ref = the restatement's
own |fp64 - long double| on the cdf): tests/test_localization_smoother_cpu.py asserts it for the probes and for the full runs on
the restatement's forward pass, the full-run test below asserts it again on the device's own forward arrays."""
import ctypes as C

import numpy as np
import pytest

import cases
import localization_ref as R
import localization_smoother_ref as S

pytestmark = pytest.mark.gpu

TOL = 1e-9


def _rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want)) / max(float(np.max(np.abs(want))), 1e-300))


def _live(rbpf):
    return int(rbpf.load_library().rbpf_device_bytes_live())


def _map(rbpf, c):
    return rbpf.DenseMagMap(rbpf.DenseMagModel(c["NN"], c["L"]), c["mean"], c["V"], c["sigma2"])


def _session(rbpf, c, **kw):
    kw.setdefault("keep_history", True)
    kw.setdefault("trace", True)
    kw.setdefault("rng", rbpf.ReplayRNG(c["U"], c["Z"]))
    return rbpf.LocalizationSession(_map(rbpf, c), c["odometry"], c["y"], c["x0_nonLin"], c["Q"], c["N_P"], c["dt"], **kw)


@pytest.fixture(scope="module")
def small_case():
    return R.loc_case(70, 8, 13)


@pytest.mark.parametrize("N,M", S.PROBE_LOGP_SHAPES)
def test_probe_logp(rbpf, N, M):
    p = S.probe_case(N, M)
    _, logp, _ = rbpf.loc_backward_step(p["X"], p["w"], p["xs_next"], p["odo"], p["dt"], p["Q"], p["u"], want_logp=True)
    want = np.column_stack([S.logp(p["xs_next"][:, j], p["X"], p["odo"], p["dt"], p["Q"], np.longdouble) for j in range(M)])
    err = _rel(logp, want)
    print(f"logp {N} x {M}: device vs long double {err:.2e}")
    assert logp.shape == (N, M) and err < TOL


@pytest.mark.parametrize("N,M", S.PROBE_INDEX_SHAPES)
def test_probe_indices(rbpf, N, M):
    p = S.probe_case(N, M)
    want = S.backward_step(p["X"], p["w"], p["xs_next"], p["odo"], p["dt"], p["Q"], p["u"])
    index, _, _ = rbpf.loc_backward_step(p["X"], p["w"], p["xs_next"], p["odo"], p["dt"], p["Q"], p["u"])
    np.testing.assert_array_equal(index, want["index"])
    if N > 2048:
        assert want["index"].max() >= 2048                                # beyond the largest chunk: not the first one
    for u in (2.0 ** -60, 1.0 - 2.0 ** -53):
        index, _, _ = rbpf.loc_backward_step(p["X"], p["w"], p["xs_next"], p["odo"], p["dt"], p["Q"], np.full(M, u))
        assert np.all(index >= 0) and np.all(index < N) and np.all(p["w"][index] > 0)


@pytest.mark.parametrize("N_P,N_T,M,glob", S.FULL_RUNS)
def test_full_run(rbpf, N_P, N_T, M, glob):
    c = R.loc_case(N_P, N_T, 13, global_init=glob)
    u = S.full_run_uniforms(N_T, M)
    with _session(rbpf, c) as s:
        s.advance(N_T)
        fwd = s.finish(extras=True)
        xn_fwd = s.history()
        out = s.backward_simulate(M, rng=u)
    assert fwd["first_degenerate_step"] == -1
    X = np.ascontiguousarray(np.transpose(xn_fwd, (2, 0, 1)))            # [T x 7 x N], the device's own forward particles
    W = np.ascontiguousarray(fwd["trace_w"].T)
    np.testing.assert_array_equal(X[N_T - 1], fwd["final_xn"])
    want = S.backward_simulate(X, W, c["odometry"], c["Q"], c["dt"], u)
    print(f"min margin {float(want['margin'].min()):.3e}, eps_ref {float(want['eps_ref'].max()):.3e}, logp fp64 vs long double {want['logp_rel']:.3e}")
    assert np.all(want["margin"] >= 100.0 * want["eps_ref"]) and want["logp_rel"] <= 1e-10
    np.testing.assert_array_equal(out["index"].T, want["index"])
    gathered = np.stack([X[t][:, out["index"][:, t]] for t in range(N_T)], axis=2)
    np.testing.assert_array_equal(out["xs_traj"], gathered)
    err = _rel(out["traj_smooth_mean"], want["traj_smooth_mean"])
    print(f"traj_smooth_mean: {err:.2e}")
    assert err < TOL
    np.testing.assert_array_equal(out["index"][:, N_T - 1], [R._sample(W[N_T - 1], uu) for uu in u[N_T - 1]])


def test_one_shot_equals_the_session_and_repeats(rbpf, small_case):
    c = small_case
    T, M = c["y"].shape[0], 9
    u = np.random.RandomState(3).random_sample((T, M))
    mp = _map(rbpf, c)
    xs, mean, ex = rbpf.particleSmootherLocalization(mp.dynModel, mp.measModel, c["odometry"], c["y"], c["x0_nonLin"], c["Q"], np.eye(3),
                                                     c["N_P"], M, c["dt"], rng=rbpf.ReplayRNG(c["U"], c["Z"], Uback=u), extras=True)
    with _session(rbpf, c) as s:
        s.advance(T)
        a = s.backward_simulate(M, rng=u)
        b = s.backward_simulate(M, rng=u)
        only = s.backward_simulate(M, rng=u, want=("index",))
    for k in ("xs_traj", "index", "traj_smooth_mean"):
        np.testing.assert_array_equal(a[k], b[k])
    np.testing.assert_array_equal(only["index"], a["index"])
    assert set(only) == {"index"}
    np.testing.assert_array_equal(xs, a["xs_traj"])
    np.testing.assert_array_equal(mean, a["traj_smooth_mean"])
    np.testing.assert_array_equal(ex["index"], a["index"])


def test_philox_seed_equals_the_replay_of_its_uniforms(rbpf, small_case):
    c = small_case
    T, M = c["y"].shape[0], 40
    with _session(rbpf, c) as s:
        s.advance(T)
        a = s.backward_simulate(M, rng=rbpf.PhiloxRNG(11))
        b = s.backward_simulate(M, rng=rbpf.PhiloxRNG(11).backward_uniforms(M, T))
        other = s.backward_simulate(M, rng=rbpf.PhiloxRNG(12))
    for k in ("xs_traj", "index", "traj_smooth_mean"):
        np.testing.assert_array_equal(a[k], b[k])
    assert not np.array_equal(other["index"], a["index"])


def test_refusals_leave_the_session_usable(rbpf, small_case):
    c = small_case
    T, M = c["y"].shape[0], 5
    lib = rbpf.load_library()
    u = np.random.RandomState(4).random_sample((T, M))
    with _session(rbpf, c) as s:
        s.advance(3)
        with pytest.raises(rbpf.RBPFError) as ei:                          # steps missing
            s.backward_simulate(M, rng=u)
        assert ei.value.status == rbpf.RBPF_ERR_STATE
        s.advance(T - 3)
        for n_traj in (0, -2):
            with pytest.raises(rbpf.RBPFError) as ei:
                s.backward_simulate(n_traj, rng=rbpf.PhiloxRNG(1))
            assert ei.value.status == rbpf.RBPF_ERR_INVALID_ARG
        fin = s.finish()
        good = s.backward_simulate(M, rng=u)
    assert np.all(np.isfinite(fin["traj_mean"])) and np.all(good["index"] >= 0) and np.all(good["index"] < c["N_P"])
    for kw in (dict(keep_history=False, trace=True), dict(keep_history=True, trace=False), dict(keep_history=False, trace=False)):
        with _session(rbpf, c, **kw) as s:
            s.advance(T)
            with pytest.raises(rbpf.RBPFError) as ei:
                s.backward_simulate(M, rng=u)
            assert ei.value.status == rbpf.RBPF_ERR_STATE
            assert np.all(np.isfinite(s.finish()["traj_mean"]))
    bad = dict(c)
    bad["y"] = c["y"].copy()
    bad["y"][2, :] += 1e3 * np.sqrt(c["sigma2"] + 650.0)                  # a degenerate step (as tests/test_gpu_localization.py)
    with _session(rbpf, bad) as s:
        s.advance(T)
        with pytest.raises(rbpf.RBPFError) as ei:
            s.backward_simulate(M, rng=u)
        assert ei.value.status == rbpf.RBPF_ERR_STATE and "degenerate" in str(ei.value)
        assert s.finish()["first_degenerate_step"] == 2
    # not a localisation context
    m = cases.mag_case(N_P=8, N_T=3, m=13, seed=1)
    mdl, x0, P0, Rm = cases.device_model(rbpf, m)
    f = rbpf.FilterSession(mdl, m["odometry"], m["y"], m["x0_nonLin"], x0, P0, m["Q"], Rm, m["N_P"], m["dt"], rng=cases.device_rng(rbpf, m))
    try:
        f.advance(3)
        idx = np.zeros((M, 3), dtype=np.int32)
        assert lib.rbpf_loc_backward_simulate(f.ctx, M, None, 1, None, idx.ctypes.data_as(C.POINTER(C.c_int32)), None) == rbpf.RBPF_ERR_INVALID_ARG
        assert lib.rbpf_loc_history(f.ctx, None) == rbpf.RBPF_ERR_INVALID_ARG
        f.sync()
    finally:
        f.close()


def test_pool_books_return_after_backward_simulate(rbpf, small_case):
    c = small_case
    T, M = c["y"].shape[0], 33
    base = _live(rbpf)
    with _session(rbpf, c) as s:
        s.advance(T)
        s.sync()
        before = _live(rbpf)
        assert before > base
        out = s.backward_simulate(M, rng=rbpf.PhiloxRNG(5))
        assert _live(rbpf) == before
        with pytest.raises(rbpf.RBPFError):
            s.backward_simulate(0)
        assert _live(rbpf) == before
        s.history()
        assert _live(rbpf) == before
    assert _live(rbpf) == base and np.all(np.isfinite(out["xs_traj"]))
    assert rbpf.loc_backward_workspace_bytes(c["N_P"], T, M) >= 8 * (8 * c["N_P"] + 7 * M * T)
