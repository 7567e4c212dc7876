"""GPU: localisation in the fixed map of a generic device-code model (rbpf.DeviceMap) against the numpy restatement
(tests/device_map_ref.py) on replayed random streams.

Tolerance: the project's standing one (tests/test_gpu_localization.py), 1e-9 relative to the largest magnitude of the quantity;
ancestor indices exact.  Every full-run case is one for which the float64 and the long-double restatement draw identical
ancestors at every step (asserted in tests/test_device_map_cpu.py).  The measured distances are printed.

Measured on the MI355X: the weight kernel alone is within 1e-15 (yhat), 1.4e-15 (S) and 7e-14 (logw, at nLin = 1 .. 17 where S is
worst conditioned; 9e-16 from nLin = 63 on) of the float64 restatement; the full runs within 2.7e-15 (weights), 5.1e-16
(trajectories) and 4.2e-16 (log sum w); the restatement's own error |fp64 - long double| on the weights is 5e-16 .. 1.5e-15; the
step-0 log-weights equal the SLAM filter's to 2e-16.  The 1e-9 bound was not widened."""
import warnings

import numpy as np
import pytest

import device_map_ref as dm
import generic_ny_cases as gc

pytestmark = pytest.mark.gpu

TOL = 1e-9


def _rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want)) / max(float(np.max(np.abs(want))), 1e-300))


def _torch():
    import torch
    return torch


def _device():
    torch = _torch()
    return torch.device("cuda", torch.cuda.current_device())


# ------------------------------------------------------------------------------------------------
# 1. the weight kernel alone
# ------------------------------------------------------------------------------------------------
_KERNEL_INPUTS = {}


def _kernel_inputs(d, n, N):
    """(H, mean, V, R, y) and the float64 restatement's (yhat, S, logw); built once per shape."""
    key = (d, n, N)
    if key not in _KERNEL_INPUTS:
        rs = np.random.RandomState(7 * d + 13 * n + N)
        H = rs.standard_normal((N, d, n)) / np.sqrt(n)
        V = np.tril(rs.standard_normal((n, n))) / np.sqrt(n)
        mean, y, R = rs.standard_normal(n), rs.standard_normal(d), gc.full_R(d, 1)
        _KERNEL_INPUTS[key] = (H, mean, V, R, y) + dm.weights(H, mean, V, R, y)
    return _KERNEL_INPUTS[key]


def _check_kernel(rbpf, d, n, N, worst, **kw):
    H, mean, V, R, y, yhat_ref, S_ref, logw_ref = _kernel_inputs(d, n, N)
    yhat, S, logw, _ = rbpf.device_map_weights(H, mean, V, R, y, **kw)
    assert np.all(np.isfinite(yhat)) and np.all(np.isfinite(S)) and np.all(np.isfinite(logw))
    e = (_rel(yhat, yhat_ref), _rel(S, S_ref), _rel(logw, logw_ref))
    assert max(e) < TOL, (d, n, N, kw, e)
    for k in range(3):
        worst[k] = max(worst[k], e[k])


@pytest.mark.parametrize("d", range(1, 9))
def test_weight_kernel_at_every_width_and_particle_count(rbpf, d):
    """Tiles and packing: particle counts around one column tile, one workgroup and several, at nLin below and above a k chunk."""
    worst = [0.0, 0.0, 0.0]
    for N in (1, 2, 15, 16, 17, 63, 64, 65, 257):
        for n in (1, 5, 17):
            _check_kernel(rbpf, d, n, N, worst)
    print(f"n_y = {d}: worst relative distance yhat {worst[0]:.2e}, S {worst[1]:.2e}, logw {worst[2]:.2e}")


@pytest.mark.parametrize("n", [3, 4, 15, 16, 63, 64, 65, 129, 515, 1151])
def test_weight_kernel_at_every_chunk_and_super_block_boundary(rbpf, n):
    worst = [0.0, 0.0, 0.0]
    for d in (1, 3, 5, 8):
        for N in (17, 65):
            _check_kernel(rbpf, d, n, N, worst)
    print(f"nLin = {n}: worst relative distance yhat {worst[0]:.2e}, S {worst[1]:.2e}, logw {worst[2]:.2e}")


@pytest.mark.parametrize("d,n,N", [(3, 129, 65), (7, 64, 17)])
@pytest.mark.parametrize("layout", [0, 1, 2])
def test_weight_kernel_in_each_dy_layout(rbpf, d, n, N, layout):
    worst = [0.0, 0.0, 0.0]
    _check_kernel(rbpf, d, n, N, worst, dy_layout=layout)
    if layout == 1:
        _check_kernel(rbpf, d, n, N, worst, dy_layout=1, ldx=n + 5)       # a stride that is no multiple of anything
    print(f"layout {layout}: worst relative distance yhat {worst[0]:.2e}, S {worst[1]:.2e}, logw {worst[2]:.2e}")


def test_the_pad_of_the_native_layout_is_not_read_into_a_sum(rbpf):
    worst = [0.0, 0.0, 0.0]
    for d, n, N in ((3, 129, 65), (5, 17, 17), (8, 1, 2)):
        _check_kernel(rbpf, d, n, N, worst, dy_layout=1, pad=np.nan)
        _check_kernel(rbpf, d, n, N, worst, dy_layout=1, ldx=n + 31, pad=np.nan)


# ------------------------------------------------------------------------------------------------
# 2. full runs
# ------------------------------------------------------------------------------------------------
_TORCH_MODELS = {}


def _torch_model(key, m, p):
    if key not in _TORCH_MODELS:
        import generic_model_torch as gmt
        _TORCH_MODELS[key] = gmt.TorchGenericModel(m, p, _device())
        _torch().cuda.synchronize()
    tm = _TORCH_MODELS[key]
    tm.reset()
    return tm


def _loc_args(p):
    return (p["odometry"], p["y"], p["x0_nonLin"], p["Q"], p["R"], p["N_P"], p["dt"])


def _map(rbpf, tm, p, **kw):
    return rbpf.DeviceMap(rbpf.DeviceHandles(tm.dynModel, tm.measModel, **kw), p["mean"], p["V"], p["R"])


def _compare(tmax, tmean, ex, ref):
    np.testing.assert_array_equal(ex["ai"][1:], ref["ai"][1:])
    figures = dict(w=_rel(ex["w"], ref["w"]), logw=_rel(ex["logw"], ref["logw"]), traj_max=_rel(tmax, ref["traj_max"]),
                   traj_mean=_rel(tmean, ref["traj_mean"]), xn_traj=_rel(ex["xn_traj"], ref["xn_traj"]),
                   log_sum_w=_rel(ex["log_sum_w"], ref["log_sum_w"]))
    print("relative distances device - restatement:", figures)
    for k, v in figures.items():
        assert v < TOL, (k, v)
    assert ex["first_degenerate_step"] == -1 and not ref["degenerate"].any()


@pytest.mark.parametrize("i", range(len(dm.FULL_RUNS)), ids=lambda i: "ny%d_n%d" % dm.FULL_RUNS[i][0][3:5])
def test_full_run_matches_the_restatement_one_shot_and_in_a_session(rbpf, i):
    m, p, ref = dm.full_run(i)
    T = p["y"].shape[0]
    tm = _torch_model(i, m, p)
    base = rbpf.load_library().rbpf_device_bytes_live()
    tmax, tmean, ex = rbpf.particleFilterLocalization(_map(rbpf, tm, p), None, *_loc_args(p), rng=rbpf.ReplayRNG(p["U"], p["Z"]), extras=True)
    assert tm.calls == T - 1
    _compare(tmax, tmean, ex, ref)
    tm.reset()
    with rbpf.LocalizationSession(_map(rbpf, tm, p), p["odometry"], p["y"], p["x0_nonLin"], p["Q"], p["N_P"], p["dt"],
                                  rng=rbpf.ReplayRNG(p["U"], p["Z"]), keep_history=True, trace=True) as s:
        s.advance(2)
        s.sync()
        assert s.tell() == 2
        s.advance(T - 2)
        b = s.finish(extras=True)
        X = s.history()
    for k, want in (("traj_max", tmax), ("traj_mean", tmean), ("trace_w", ex["w"].T), ("trace_ai", ex["ai"].T), ("xn_traj", ex["xn_traj"]),
                    ("log_sum_w", ex["log_sum_w"])):
        np.testing.assert_array_equal(b[k], want, err_msg=k)                 # two advance calls: equal arrays
    np.testing.assert_array_equal(X[:, :, -1], ex["xn"])
    assert rbpf.load_library().rbpf_device_bytes_live() == base


@pytest.mark.parametrize("kw", [dict(), dict(native_out=True), "matlab"], ids=["c_contiguous", "native_out", "matlab_strides"])
def test_full_run_in_each_dy_layout(rbpf, kw):
    """The binding reads the layout off the strides of what measModel returns: the same run on each of the three routes."""
    m, p, ref = dm.full_run(1)
    tm = _torch_model(1, m, p)
    if kw == "matlab":
        meas = lambda xn: tm.measModel(xn).permute(2, 1, 0).contiguous().permute(2, 1, 0)     # noqa: E731
        mp = rbpf.DeviceMap(rbpf.DeviceHandles(tm.dynModel, meas), p["mean"], p["V"], p["R"])
    elif kw:
        def meas(xn, out):
            out.copy_(tm.measModel(xn))
            return out
        mp = rbpf.DeviceMap(rbpf.DeviceHandles(tm.dynModel, meas, native_out=True), p["mean"], p["V"], p["R"])
    else:
        mp = _map(rbpf, tm, p)
    _compare(*rbpf.particleFilterLocalization(mp, None, *_loc_args(p), rng=rbpf.ReplayRNG(p["U"], p["Z"]), extras=True), ref)


def test_predict_matches_the_restatement(rbpf):
    m, p, _ = dm.full_run(0)
    tm = _torch_model(0, m, p)
    xn = np.random.RandomState(1).uniform(-1, 1, (m.nNonLin, 37))
    yhat, cov = _map(rbpf, tm, p).predict(xn)
    yhat_ref, S_ref, _ = dm.weights(m.measModel(xn), p["mean"], p["V"], p["R"], np.zeros(m.ny))
    assert yhat.shape == (37, m.ny) and cov.shape == (37, m.ny, m.ny)
    assert _rel(yhat, yhat_ref) < TOL and _rel(cov, S_ref) < TOL


# ------------------------------------------------------------------------------------------------
# 3. against code that already exists: the map set to the prior, step 0 of the SLAM filter
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 3, 3, 3, 64), (3, 3, 3, 6, 130)], ids=["ny3", "ny6"])
def test_step_0_equals_the_slam_filter_when_the_map_is_the_prior(rbpf, shape):
    N, T = 32, 3
    m, p = gc.case(shape, N, T)
    import generic_model_torch as gmt
    tm = gmt.TorchGenericModel(m, p, _device())
    _torch().cuda.synchronize()
    rng = rbpf.ReplayRNG(p["U"], p["Z"], p["Ufin"])
    h = rbpf.DeviceHandles(tm.dynModel, tm.measModel)
    slam = rbpf.particleFilter(h, None, p["odometry"], p["y"], p["x0_nonLin"], p["x0_lin"], p["P0_lin"], p["Q"], p["R"], N, p["dt"],
                               rng=rng, extras=True)[8]
    tm.reset()
    mp = rbpf.DeviceMap.from_posterior(h, p["x0_lin"], p["P0_lin"], p["R"])
    _, _, ex = rbpf.particleFilterLocalization(mp, None, *_loc_args(p), rng=rng, extras=True)
    e = _rel(ex["logw"][0], slam["logw"][0])
    print("step-0 log-weights, DeviceMap at the prior against particleFilter:", e)
    assert e < TOL


# ------------------------------------------------------------------------------------------------
# 4. round trip at toy size: map with the SLAM filter, localise in that map
# ------------------------------------------------------------------------------------------------
def test_round_trip_slam_then_localise(rbpf):
    N, T = 128, 12
    m, p = gc.case((3, 3, 3, 3, 64), N, T)
    import generic_model_torch as gmt
    tm = gmt.TorchGenericModel(m, p, _device())
    _torch().cuda.synchronize()
    lib = rbpf.load_library()
    base = lib.rbpf_device_bytes_live()
    rng = rbpf.ReplayRNG(p["U"], p["Z"], p["Ufin"])
    h = rbpf.DeviceHandles(tm.dynModel, tm.measModel)
    out = rbpf.particleFilter(h, None, p["odometry"], p["y"], p["x0_nonLin"], p["x0_lin"], p["P0_lin"], p["Q"], p["R"], N, p["dt"], rng=rng)
    xl_max, P_max = out[2], out[4]
    tm.reset()
    mp = rbpf.DeviceMap.from_posterior(h, xl_max, P_max, p["R"])
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                    # no degenerate-weights warning
        tmax, tmean, ex = rbpf.particleFilterLocalization(mp, None, *_loc_args(p), rng=rng, extras=True)
    assert ex["first_degenerate_step"] == -1
    assert np.all(np.isfinite(ex["w"])) and np.all(np.isfinite(ex["logw"])) and np.all(np.isfinite(tmean))
    np.testing.assert_allclose(ex["w"].sum(axis=1), 1.0, rtol=1e-12)
    assert lib.rbpf_device_bytes_live() == base


# ------------------------------------------------------------------------------------------------
# 5. makePlots
# ------------------------------------------------------------------------------------------------
def test_make_plots_gets_the_five_arguments_and_its_exception_surfaces(rbpf):
    m, p, _ = dm.full_run(2)
    N, T, nN, d = p["N_P"], p["y"].shape[0], m.nNonLin, m.ny
    tm = _torch_model(2, m, p)
    calls = []

    def plots(*a):
        calls.append([np.asarray(x).shape for x in a])

    rbpf.particleFilterLocalization(_map(rbpf, tm, p), None, *_loc_args(p), makePlots=plots, rng=rbpf.ReplayRNG(p["U"], p["Z"]))
    assert calls == [[(nN, N), (nN, T), (d, T), (nN, N, T), (nN, T)]] * T

    class Boom(Exception):
        pass

    def bad(*a):
        raise Boom()

    tm.reset()
    base = rbpf.load_library().rbpf_device_bytes_live()
    with pytest.raises(Boom):
        rbpf.particleFilterLocalization(_map(rbpf, tm, p), None, *_loc_args(p), makePlots=bad, rng=rbpf.ReplayRNG(p["U"], p["Z"]))
    assert rbpf.load_library().rbpf_device_bytes_live() == base


# ------------------------------------------------------------------------------------------------
# 6. refusals on the device leave nothing behind
# ------------------------------------------------------------------------------------------------
def test_refusals_leave_no_memory_behind_and_a_valid_run_works_afterwards(rbpf):
    torch = _torch()
    m, p, ref = dm.full_run(2)
    N, T = p["N_P"], p["y"].shape[0]
    tm = _torch_model(2, m, p)
    lib = rbpf.load_library()
    base = lib.rbpf_device_bytes_live()
    rng = rbpf.ReplayRNG(p["U"], p["Z"])
    for kw in (dict(n_devices=2), dict(lazy_depth=2)):
        with pytest.raises(rbpf.RBPFError) as ei:
            rbpf.particleFilterLocalization(_map(rbpf, tm, p), None, *_loc_args(p), rng=rng, **kw)
        assert ei.value.status == rbpf.RBPF_ERR_UNSUPPORTED
        assert lib.rbpf_device_bytes_live() == base
    with pytest.raises(rbpf.RBPFError) as ei:
        rbpf.particleSmootherLocalization(_map(rbpf, tm, p), None, *_loc_args(p)[:6], 8, p["dt"], rng=rng)
    assert ei.value.status == rbpf.RBPF_ERR_UNSUPPORTED and "transition density" in str(ei.value)
    with rbpf.LocalizationSession(_map(rbpf, tm, p), p["odometry"], p["y"], p["x0_nonLin"], p["Q"], N, p["dt"], rng=rng,
                                  keep_history=True, trace=True) as s:
        s.advance(T)
        with pytest.raises(rbpf.RBPFError) as ei:
            s.backward_simulate(4)
        assert ei.value.status == rbpf.RBPF_ERR_UNSUPPORTED and "transition density" in str(ei.value)
        st = lib.rbpf_loc_backward_simulate(s.ctx, 4, None, 1, None, None, None)          # the library itself refuses too
        assert st == rbpf.RBPF_ERR_UNSUPPORTED and b"transition density" in lib.rbpf_last_error()
        assert lib.rbpf_loc_advance(s.ctx, 1) == rbpf.RBPF_ERR_STATE
    assert lib.rbpf_device_bytes_live() == base
    for meas in (lambda xn: tm.measModel(xn)[:, :, :-1], lambda xn: tm.measModel(xn).to(torch.float32)):
        tm.reset()
        bad = rbpf.DeviceMap(rbpf.DeviceHandles(tm.dynModel, meas), p["mean"], p["V"], p["R"])
        with pytest.raises(ValueError):
            rbpf.particleFilterLocalization(bad, None, *_loc_args(p), rng=rng)
        assert lib.rbpf_device_bytes_live() == base
    tm.reset()
    _compare(*rbpf.particleFilterLocalization(_map(rbpf, tm, p), None, *_loc_args(p), rng=rng, extras=True), ref)
    assert lib.rbpf_device_bytes_live() == base
