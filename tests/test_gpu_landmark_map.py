"""GPU: localisation in the fixed landmark map of a sparseFeatures device-code model (rbpf.DeviceLandmarkMap, rbpf_loc_landmark_*)
against the numpy restatement (tests/landmark_map_ref.py) on replayed random streams.

Tolerance: the project's standing one (tests/test_gpu_localization.py, tests/test_gpu_device_map.py), 1e-9 relative to the largest
magnitude of the quantity; ancestors, indices, xn_traj and traj_max exact.  Every full-run case is one for which the float64 and
the long-double restatement draw identical ancestors at every step (asserted in tests/test_landmark_map_cpu.py).  The measured
distances are printed.

Measured on the MI355X: the weight kernel alone is within 8.1e-16 (S) and 1.2e-14 (logw, at nLin = 3 where S is worst conditioned;
5.2e-15 at n_y = 32, 2.2e-15 at (32, 96)) of the float64 restatement, and bit-identical across the layouts, the pads, the poison
values and the launches it is asked to be; the six full runs within 1.2e-13 (weights), 1.2e-14 (log-weights), 3.9e-15 (traj_mean)
and 1.9e-15 (log sum w), with ancestors, xn_traj and traj_max exact; the restatement's own error |fp64 - long double| is 5.9e-16 ..
9.5e-15 on the weights and at most 2.8e-14 on the log-weights; the step-0 log-weights equal the SLAM filter's to 1.9e-15; the
backward draws have a margin of 8.2e-5 against a reference error of 6.3e-16; the round trip localises to a mean position error of
0.169 where dead reckoning on the same odometry gives 0.360.  The 1e-9 bound was not widened."""
import warnings

import numpy as np
import pytest

import device_map_smoother_ref as S
import generic_ny_cases as gc
import landmark_map_ref as lm
import rbpf_oracle as O
import sparse_models as sm

pytestmark = pytest.mark.gpu

TOL = 1e-9
PB = 32                                                                   # particles per workgroup of the weight kernel


def _rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if want.size == 0:
        return 0.0
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
MASKS = {
    "all": lambda d: np.ones(d, dtype=bool),
    "first": lambda d: np.arange(d) == 0,
    "last": lambda d: np.arange(d) == d - 1,
    "alternating": lambda d: np.arange(d) % 2 == 0,
    "sixteen": lambda d: np.isin(np.arange(d), np.r_[0:5, 9:17, 29:32]),
    "seventeen": lambda d: np.isin(np.arange(d), np.r_[0:5, 9:17, 28:32]),
    "none": lambda d: np.zeros(d, dtype=bool),
}
_KERNEL_INPUTS = {}


def _kernel_inputs(d, n, N, mask="all", R_seed=1):
    """(yhat, H, V, R, y) and the float64 restatement's (S, logw); built once per shape and mask."""
    key = (d, n, N, mask, R_seed)
    if key not in _KERNEL_INPUTS:
        rs = np.random.RandomState(7 * d + 13 * n + N)
        H = rs.standard_normal((N, d, n)) / np.sqrt(n)
        V = np.tril(rs.standard_normal((n, n))) / np.sqrt(n)
        yhat, y, R = rs.standard_normal((N, d)), rs.standard_normal(d), gc.full_R(d, R_seed)
        y[~MASKS[mask](d)] = np.nan
        _KERNEL_INPUTS[key] = (yhat, H, V, R, y) + lm.weights(yhat, H, V, R, y)
    return _KERNEL_INPUTS[key]


def _check_kernel(rbpf, d, n, N, worst, mask="all", R_seed=1, **kw):
    yhat, H, V, R, y, S_ref, logw_ref = _kernel_inputs(d, n, N, mask, R_seed)
    Sg, logw, _ = rbpf.landmark_map_weights(yhat, H, V, R, y, **kw)
    assert Sg.shape == S_ref.shape and np.all(np.isfinite(Sg)) and np.all(np.isfinite(logw))
    e = (_rel(Sg, S_ref), _rel(logw, logw_ref))
    assert max(e) < TOL, (d, n, N, mask, kw, e)
    for k in range(2):
        worst[k] = max(worst[k], e[k])
    return Sg, logw


@pytest.mark.parametrize("d", [1, 2, 15, 16, 17, 31, 32])
def test_weight_kernel_at_every_width(rbpf, d):
    worst = [0.0, 0.0]
    for n, N in ((17, 17), (40, 33)):
        _check_kernel(rbpf, d, n, N, worst)
    print(f"n_y = {d}: worst relative distance S {worst[0]:.2e}, logw {worst[1]:.2e}")


@pytest.mark.parametrize("mask", ["first", "last", "alternating", "sixteen", "seventeen", "none"])
def test_weight_kernel_with_some_outputs_observed(rbpf, mask):
    worst = [0.0, 0.0]
    M = int(MASKS[mask](32).sum())
    assert M == dict(first=1, last=1, alternating=16, sixteen=16, seventeen=17, none=0)[mask]
    for n, N in ((33, 17), (96, 33)):
        Sg, logw = _check_kernel(rbpf, 32, n, N, worst, mask=mask)
        assert Sg.shape == (N, M, M)
        if mask == "none":
            np.testing.assert_array_equal(logw, np.zeros(N))
    print(f"mask {mask}: worst relative distance S {worst[0]:.2e}, logw {worst[1]:.2e}")


@pytest.mark.parametrize("n", [1, 3, 15, 16, 17, 63, 64, 65, 95, 96])
def test_weight_kernel_at_every_tile_boundary_of_nlin(rbpf, n):
    worst = [0.0, 0.0]
    for d in (5, 32):
        _check_kernel(rbpf, d, n, 33, worst)
    print(f"nLin = {n}: worst relative distance S {worst[0]:.2e}, logw {worst[1]:.2e}")


@pytest.mark.parametrize("d,n", [(5, 33), (32, 96), (20, 40)])
def test_a_particles_result_does_not_depend_on_the_launch(rbpf, d, n):
    """Particle counts around one workgroup, and each particle alone against the same particle inside a launch of 257."""
    worst = [0.0, 0.0]
    yhat, H, V, R, y, _, _ = _kernel_inputs(d, n, 257)
    S_all, logw_all = _check_kernel(rbpf, d, n, 257, worst)
    for N in (1, 2, PB - 1, PB, PB + 1):
        _check_kernel(rbpf, d, n, N, worst)
        Sg, logw, _ = rbpf.landmark_map_weights(yhat[:N], H[:N], V, R, y)             # the first N of the 257: bit for bit
        np.testing.assert_array_equal(Sg, S_all[:N])
        np.testing.assert_array_equal(logw, logw_all[:N])
    for i in (0, 31, 32, 100, 255, 256):
        Sg, logw, _ = rbpf.landmark_map_weights(yhat[i:i + 1], H[i:i + 1], V, R, y)
        np.testing.assert_array_equal(Sg[0], S_all[i])
        np.testing.assert_array_equal(logw[0], logw_all[i])
    print(f"(n_y, nLin) = ({d}, {n}): worst relative distance S {worst[0]:.2e}, logw {worst[1]:.2e}")


@pytest.mark.parametrize("mask", ["alternating", "seventeen", "last"])
def test_unobserved_rows_are_never_read_into_a_sum(rbpf, mask):
    d, n, N = 32, 65, 33
    yhat, H, V, R, y, S_ref, logw_ref = _kernel_inputs(d, n, N, mask)
    gone = np.isnan(y)
    results = []
    for poison in (np.nan, 1e300, 0.0):
        yh, Hp = yhat.copy(), H.copy()
        yh[:, gone], Hp[:, gone, :] = poison, poison
        for layouts in (dict(), dict(yhat_layout=0, dy_layout=0), dict(dy_layout=1)):
            results.append(rbpf.landmark_map_weights(yh, Hp, V, R, y, **layouts)[:2])
    for Sg, logw in results:
        np.testing.assert_array_equal(Sg, results[0][0])
        np.testing.assert_array_equal(logw, results[0][1])
    assert _rel(results[0][0], S_ref) < TOL and _rel(results[0][1], logw_ref) < TOL


def test_the_pad_of_dy_layout_1_never_enters_a_result(rbpf):
    worst = [0.0, 0.0]
    for d, n, N in ((7, 33, 17), (32, 95, 33), (5, 1, 2), (32, 96, 17)):
        base = _check_kernel(rbpf, d, n, N, worst, dy_layout=1)
        for kw in (dict(pad=np.nan), dict(ldx=n + 31, pad=np.nan), dict(ldx=n + 5, pad=np.nan), dict(ldx=n, pad=np.nan)):
            Sg, logw = _check_kernel(rbpf, d, n, N, worst, dy_layout=1, **kw)
            np.testing.assert_array_equal(Sg, base[0])
            np.testing.assert_array_equal(logw, base[1])


@pytest.mark.parametrize("d,n,N", [(7, 33, 17), (32, 96, 65)])
@pytest.mark.parametrize("yl", [0, 2])
@pytest.mark.parametrize("dl", [0, 1, 2])
def test_weight_kernel_in_each_pair_of_layouts(rbpf, d, n, N, yl, dl):
    worst = [0.0, 0.0]
    base = _check_kernel(rbpf, d, n, N, worst)
    Sg, logw = _check_kernel(rbpf, d, n, N, worst, yhat_layout=yl, dy_layout=dl)
    np.testing.assert_array_equal(Sg, base[0])                            # one arithmetic, whichever way the operands arrive
    np.testing.assert_array_equal(logw, base[1])
    Sg, logw = _check_kernel(rbpf, d, n, N, worst, mask="alternating" if d == 32 else "last", yhat_layout=yl, dy_layout=dl)


def test_a_full_r_and_garbage_above_the_diagonal_of_v(rbpf):
    worst = [0.0, 0.0]
    for d, n, N, mask in ((17, 51, 33, "all"), (32, 96, 17, "seventeen"), (6, 6, 5, "all")):
        base = _check_kernel(rbpf, d, n, N, worst, mask=mask, R_seed=2)
        yhat, H, V, R, y, _, _ = _kernel_inputs(d, n, N, mask, 2)
        assert np.count_nonzero(R) == d * d                               # no zero in R
        Vg = V.copy()
        Vg[np.triu_indices(n, 1)] = np.nan
        Sg, logw, _ = rbpf.landmark_map_weights(yhat, H, Vg, R, y)
        np.testing.assert_array_equal(Sg, base[0])
        np.testing.assert_array_equal(logw, base[1])
    print(f"full R: worst relative distance S {worst[0]:.2e}, logw {worst[1]:.2e}")


# ------------------------------------------------------------------------------------------------
# 2. full runs
# ------------------------------------------------------------------------------------------------
TWIN_MODES = [dict(), dict(nan_unobserved=True), dict(dy_mode="matlab", yhat_mode="t"), dict(dy_mode="slice", nan_unobserved=True),
              dict(yhat_mode="t"), dict(dy_mode="matlab", nan_unobserved=True)]


class Twin:
    """The torch twin of a case's model (sparse_models_torch.twin_of), recording the yhat of every measModel call."""

    def __init__(self, p, **kw):
        import sparse_models_torch as smt
        self.tw = smt.twin_of(p["model"], p, _device(), **kw)
        _torch().cuda.synchronize()
        self.yhats = []

    def reset(self):
        self.tw.reset()
        self.yhats = []

    def dynModel(self, xn, dx, dt, Q):
        return self.tw.dynModel(xn, dx, dt, Q)

    def measModel(self, xn, xl):
        yhat, dy = self.tw.measModel(xn, xl)
        self.yhats.append(yhat.detach().cpu().numpy().copy())
        return yhat, dy

    def drift(self, xn, dx, dt, Q):
        return xn + dx.reshape(-1, 1)


def _loc_args(p):
    return (p["odometry"], p["y"], p["x0_nonLin"], p["Q"], p["R"], p["N_P"], p["dt"])


def _rng(rbpf, p):
    return rbpf.ReplayRNG(p["rng"].U, p["rng"].Z)


def _map(rbpf, tw, p, transition=None):
    return rbpf.DeviceLandmarkMap(rbpf.DeviceSparseHandles(tw.dynModel, tw.measModel), p["mean"], p["V"], p["R"], transition=transition)


def _run(rbpf, tw, p, **kw):
    tw.reset()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                   # (the reference's warning where the weights sum to little)
        return rbpf.particleFilterLocalization(_map(rbpf, tw, p), None, *_loc_args(p), rng=_rng(rbpf, p), extras=True, **kw)


def _compare(tw, tmax, tmean, ex, p, ref):
    np.testing.assert_array_equal(ex["ai"][1:], ref["ai"][1:])
    np.testing.assert_array_equal(ex["xn_traj"], ref["xn_traj"])
    np.testing.assert_array_equal(tmax, ref["traj_max"])
    figures = dict(w=_rel(ex["w"], ref["w"]), logw=_rel(ex["logw"], ref["logw"]), traj_mean=_rel(tmean, ref["traj_mean"]),
                   log_sum_w=_rel(ex["log_sum_w"], ref["log_sum_w"]))
    print("relative distances device - restatement:", figures)
    for k, v in figures.items():
        assert v < TOL, (k, v)
    first = np.flatnonzero(ref["degenerate"])
    assert ex["first_degenerate_step"] == (int(first[0]) if first.size else -1)
    T = p["y"].shape[0]
    assert ex["yhattraj"].shape == (p["y"].shape[1], T) and len(tw.yhats) == T
    for t in range(T):                                                    # the handle's own output, NaN rows included
        np.testing.assert_array_equal(ex["yhattraj"][:, t], tw.yhats[t][int(np.argmax(ex["w"][t]))])
        seen = ~np.isnan(p["y"][t])
        assert _rel(ex["yhattraj"][seen, t], ref["yhattraj"][seen, t]) < TOL


@pytest.mark.parametrize("i", range(len(lm.FULL_RUNS)), ids=lm.run_id)
def test_full_run_matches_the_restatement_one_shot_and_in_a_session(rbpf, i):
    p, ref = lm.full_run(i)
    T = p["y"].shape[0]
    tw = Twin(p, **TWIN_MODES[i])
    base = rbpf.load_library().rbpf_device_bytes_live()
    tmax, tmean, ex = _run(rbpf, tw, p)
    assert tw.tw.dyn_calls == T - 1 and tw.tw.meas_calls == T
    _compare(tw, tmax, tmean, ex, p, ref)
    if i == 5:                                                            # nothing observed at step 1: equal weights
        np.testing.assert_array_equal(ex["logw"][1], np.zeros(p["N_P"]))
        assert np.ptp(ex["w"][1]) == 0.0 and abs(ex["w"][1][0] * p["N_P"] - 1.0) <= 4 * np.finfo(float).eps
        assert abs(ex["log_sum_w"][1] - np.log(p["N_P"])) <= 1e-14
    tw.reset()
    with rbpf.LocalizationSession(_map(rbpf, tw, p), p["odometry"], p["y"], p["x0_nonLin"], p["Q"], p["N_P"], p["dt"],
                                  rng=_rng(rbpf, p), keep_history=True, trace=True) as s:
        s.advance(2)
        s.sync()
        assert s.tell() == 2
        s.advance(T - 2)
        b = s.finish(extras=True)
        X = s.history()
    for k, want in (("traj_max", tmax), ("traj_mean", tmean), ("trace_w", ex["w"].T), ("trace_logw", ex["logw"].T), ("trace_ai", ex["ai"].T),
                    ("xn_traj", ex["xn_traj"]), ("log_sum_w", ex["log_sum_w"]), ("yhattraj", ex["yhattraj"])):
        np.testing.assert_array_equal(b[k], want, err_msg=k)                 # two advance calls: equal arrays
    np.testing.assert_array_equal(X[:, :, -1], ex["xn"])
    assert rbpf.load_library().rbpf_device_bytes_live() == base


def test_predict_matches_the_restatement(rbpf):
    p, _ = lm.full_run(3)
    tw = Twin(p)
    xn = np.asarray(p["x0_nonLin"]).reshape(3, 1) + np.random.RandomState(1).uniform(-0.3, 0.3, (3, 37))
    yhat, cov = _map(rbpf, tw, p).predict(xn)
    d = p["model"].ny
    yhat_ref, H = lm.meas(p["model"], xn, p["mean"])
    S_ref, _ = lm.weights(yhat_ref, H, p["V"], p["R"], np.zeros(d))
    assert yhat.shape == (37, d) and cov.shape == (37, d, d)
    assert _rel(yhat, yhat_ref) < TOL and _rel(cov, S_ref) < TOL


# ------------------------------------------------------------------------------------------------
# 3. against code that already exists: the map set to the prior, step 0 of the SLAM filter
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,L,pattern", [("rb", 8, None), ("rb", 3, ["last"]), ("ro", 17, None)], ids=["range_bearing", "last_output_only", "range_only"])
def test_step_0_equals_the_slam_filter_when_the_map_is_the_prior(rbpf, kind, L, pattern):
    N, T = 32, 3
    p = lm.case(kind, L, N, T, seed=2, pattern=pattern)
    x0 = np.asarray(p["x0_nonLin"], dtype=np.float64).reshape(3, 1) + 0.05 * np.random.RandomState(5).standard_normal((3, N))
    tw = Twin(p)
    h = rbpf.DeviceSparseHandles(tw.dynModel, tw.measModel)
    P0 = p["V"].T @ p["V"]
    # (the SLAM filter takes one initial state: spread the particles through the first step's states instead -- step 0 of both
    # filters weighs x0 repeated, so compare there, and at spread states through the probe)
    slam = rbpf.particleFilter(h, None, p["odometry"], p["y"], p["x0_nonLin"], p["mean"], P0, p["Q"], p["R"], N, p["dt"], True,
                               rng=rbpf.ReplayRNG(p["rng"].U, p["rng"].Z, p["rng"].Ufin), extras=True)[8]
    tw.reset()
    mp = _map(rbpf, tw, p)                                               # (V itself: V'V of a random V is too close to singular to factor again)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        _, _, ex = rbpf.particleFilterLocalization(mp, None, *_loc_args(p), rng=_rng(rbpf, p), extras=True)
    e = _rel(ex["logw"][0], slam["logw"][0])
    print("step-0 log-weights, DeviceLandmarkMap at the prior against particleFilter:", e)
    assert e < TOL
    yhat, H = lm.meas(p["model"], x0, p["mean"])
    _, logw, _ = rbpf.landmark_map_weights(yhat, H, mp.V, p["R"], p["y"][0])
    want = np.array([O._sparse_logw(p["model"], p["y"][0], x0[:, i], p["mean"], P0, p["R"], 1e-3) for i in range(N)])
    assert _rel(logw, want) < TOL


# ------------------------------------------------------------------------------------------------
# 4. round trip at toy size: map with the SLAM filter, localise a second run in that map
# ------------------------------------------------------------------------------------------------
def _second_run(p, L, seed, N_P, N_T):
    """A later drive through the world of sparse_models.range_bearing_case(L, ., ., seed): the same landmarks (the case's first
    draws), another path, and an odometry that drifts sideways, so dead reckoning leaves the path."""
    rs0 = np.random.RandomState(seed)
    xl_true = np.vstack((rs0.uniform(5.0, 9.0, L), rs0.uniform(-3.0, 3.0, L))).T.reshape(-1)
    rs = np.random.RandomState(seed + 77)
    th = 0.02 * np.cumsum(rs.standard_normal(N_T))
    path = np.vstack((0.1 * np.arange(N_T), 0.03 * np.cumsum(rs.standard_normal(N_T))))
    sig = np.tile([0.1, 0.02], L)
    y = np.array([p["model"].measModel(np.array([path[0, t], path[1, t], th[t]]), xl_true)[0] + sig * rs.standard_normal(2 * L) for t in range(N_T)])
    y[2, 1::2] = np.nan
    y[5, :4] = np.nan
    u = np.vstack((np.diff(path, axis=1), np.diff(th)[None, :])).T + np.array([0.0, 0.06, 0.0]) + 0.02 * rs.standard_normal((N_T - 1, 3))
    truth = np.vstack((path, th[None, :]))
    q = dict(p, odometry=u, y=y, x0_nonLin=truth[:, 0].copy(), Q=np.diag([0.08 ** 2, 0.08 ** 2, 0.02 ** 2]), N_P=N_P,
             rng=O.ReplayRNG.draw(seed + 900, 1, N_T, N_P, 3))
    return q, truth


def test_round_trip_slam_then_localise_a_second_run(rbpf):
    L, N, T, seed = 8, 128, 12, 6
    c = sm.range_bearing_case(L, N, T, seed=seed)
    tw = Twin(c)
    lib = rbpf.load_library()
    base = lib.rbpf_device_bytes_live()
    h = rbpf.DeviceSparseHandles(tw.dynModel, tw.measModel)
    out = rbpf.particleFilter(h, None, c["odometry"], c["y"], c["x0_nonLin"], c["x0_lin"], c["P0_lin"], c["Q"], c["R"], N, c["dt"], True,
                              rng=rbpf.ReplayRNG(c["rng"].U, c["rng"].Z, c["rng"].Ufin))
    xl_max, P_max = out[2], out[4]
    q, truth = _second_run(c, L, seed, 256, 14)
    tw2 = Twin(q)
    mp = rbpf.DeviceLandmarkMap.from_posterior(rbpf.DeviceSparseHandles(tw2.dynModel, tw2.measModel), xl_max, P_max, c["R"])
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                    # no degenerate-weights warning
        tmax, tmean, ex = rbpf.particleFilterLocalization(mp, None, *_loc_args(q), rng=_rng(rbpf, q), extras=True)
    assert ex["first_degenerate_step"] == -1
    assert np.all(np.isfinite(ex["w"])) and np.all(np.isfinite(ex["logw"])) and np.all(np.isfinite(tmean)) and np.all(np.isfinite(tmax))
    np.testing.assert_allclose(ex["w"].sum(axis=1), 1.0, rtol=1e-12)
    dead = truth[:, :1] + np.hstack((np.zeros((3, 1)), np.cumsum(q["odometry"].T, axis=1)))
    err = lambda x: float(np.mean(np.hypot(x[0] - truth[0], x[1] - truth[1])))                # noqa: E731
    print(f"mean position error: localisation {err(tmean):.3f}, dead reckoning on the same odometry {err(dead):.3f}")
    assert err(tmean) <= err(dead)
    assert lib.rbpf_device_bytes_live() == base


# ------------------------------------------------------------------------------------------------
# 5. backward simulation: the pass never reads the map
# ------------------------------------------------------------------------------------------------
def test_backward_simulation_with_a_transition_matches_the_restatement(rbpf):
    p, _ = lm.full_run(4)
    N, T, M = p["N_P"], p["y"].shape[0], 7
    tw = Twin(p)
    tr = rbpf.DeviceTransition(tw.drift, rows=(0, 1, 2))
    u = S.full_run_uniforms(T, M)
    tw.reset()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        with rbpf.LocalizationSession(_map(rbpf, tw, p, tr), p["odometry"], p["y"], p["x0_nonLin"], p["Q"], N, p["dt"], rng=_rng(rbpf, p),
                                      keep_history=True, trace=True) as s:
            s.advance(T)
            fwd = s.finish(extras=True)
            xn_fwd = s.history()
            out = s.backward_simulate(M, rng=u)
    assert fwd["first_degenerate_step"] == -1
    X = np.ascontiguousarray(np.transpose(xn_fwd, (2, 0, 1)))
    W = np.ascontiguousarray(fwd["trace_w"].T)
    mus = [X[t] + np.asarray(p["odometry"][t], dtype=np.float64).reshape(3, 1) for t in range(T - 1)]
    covs = [p["dt"] * np.asarray(p["Q"], dtype=np.float64)] * (T - 1)
    want = S.backward_simulate(X, W, mus, covs, u, (0, 1, 2), ())
    print(f"min margin {float(want['margin'].min()):.3e}, eps_ref {float(want['eps_ref'].max()):.3e}")
    assert np.all(want["margin"] >= 100.0 * want["eps_ref"])
    np.testing.assert_array_equal(want["index"], want["index_ld"])
    np.testing.assert_array_equal(out["index"].T, want["index"])
    np.testing.assert_array_equal(out["xs_traj"], np.stack([X[t][:, out["index"][:, t]] for t in range(T)], axis=2))
    assert _rel(out["traj_smooth_mean"], want["traj_smooth_mean"]) < TOL
    tw.reset()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        xs, mean, ex = rbpf.particleSmootherLocalization(_map(rbpf, tw, p, tr), None, *_loc_args(p)[:6], M, p["dt"],
                                                         rng=rbpf.ReplayRNG(p["rng"].U, p["rng"].Z, Uback=u), extras=True)
    assert xs.shape == (3, M, T) and mean.shape == (3, T) and ex["index"].shape == (M, T)      # the shapes of a DeviceMap
    np.testing.assert_array_equal(xs, out["xs_traj"])
    np.testing.assert_array_equal(ex["index"], out["index"])


# ------------------------------------------------------------------------------------------------
# 6. makePlots
# ------------------------------------------------------------------------------------------------
def test_make_plots_gets_the_five_arguments_and_its_exception_surfaces(rbpf):
    p, ref = lm.full_run(1)
    N, T, d = p["N_P"], p["y"].shape[0], p["model"].ny
    tw = Twin(p)
    calls, seen = [], []

    def plots(*a):
        calls.append([np.asarray(x).shape for x in a])
        seen.append(np.array(a[2]))

    _run(rbpf, tw, p, makePlots=plots)
    assert calls == [[(3, N), (3, T), (d, T), (3, N, T), (3, T)]] * T
    for t in range(T):                                                    # yhattraj: filled up to the step, NaN behind it
        assert np.all(np.isnan(seen[t][:, t + 1:])) and np.all(np.isfinite(seen[t][:, :t + 1]))

    class Boom(Exception):
        pass

    def bad(*a):
        raise Boom()

    base = rbpf.load_library().rbpf_device_bytes_live()
    with pytest.raises(Boom):
        _run(rbpf, tw, p, makePlots=bad)
    assert rbpf.load_library().rbpf_device_bytes_live() == base


# ------------------------------------------------------------------------------------------------
# 7. refusals and failing handles leave nothing behind
# ------------------------------------------------------------------------------------------------
def test_refusals_and_failing_handles_leave_no_memory_behind_and_a_valid_run_works_afterwards(rbpf):
    torch = _torch()
    p, ref = lm.full_run(1)
    N, T = p["N_P"], p["y"].shape[0]
    tw = Twin(p)
    lib = rbpf.load_library()
    base = lib.rbpf_device_bytes_live()
    for kw in (dict(n_devices=2), dict(lazy_depth=2)):
        with pytest.raises(rbpf.RBPFError) as ei:
            rbpf.particleFilterLocalization(_map(rbpf, tw, p), None, *_loc_args(p), rng=_rng(rbpf, p), **kw)
        assert ei.value.status == rbpf.RBPF_ERR_UNSUPPORTED
        assert lib.rbpf_device_bytes_live() == base
    with pytest.raises(rbpf.RBPFError) as ei:
        rbpf.particleSmootherLocalization(_map(rbpf, tw, p), None, *_loc_args(p)[:6], 8, p["dt"], rng=_rng(rbpf, p))
    assert ei.value.status == rbpf.RBPF_ERR_UNSUPPORTED and "transition density" in str(ei.value)
    tw.reset()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        with rbpf.LocalizationSession(_map(rbpf, tw, p), p["odometry"], p["y"], p["x0_nonLin"], p["Q"], N, p["dt"], rng=_rng(rbpf, p),
                                      keep_history=True, trace=True) as s:
            s.advance(1)
            xn = torch.zeros((3, N), dtype=torch.float64, device=_device())
            yh = torch.zeros((N, p["model"].ny), dtype=torch.float64, device=_device())
            dy = torch.zeros((N, p["model"].ny, p["model"].nLin), dtype=torch.float64, device=_device())
            torch.cuda.synchronize()
            step = lambda: lib.rbpf_loc_landmark_step_device(s.ctx, xn.data_ptr(), yh.data_ptr(), 2, dy.data_ptr(), 2)   # noqa: E731
            assert step() == rbpf.RBPF_ERR_STATE and b"ancestors" in lib.rbpf_last_error()      # t = 1 without the ancestors call
            assert lib.rbpf_loc_generic_step_device(s.ctx, xn.data_ptr(), dy.data_ptr(), 2) == rbpf.RBPF_ERR_STATE
            s.advance(T - 1)
            assert step() == rbpf.RBPF_ERR_STATE                           # after the last step
            with pytest.raises(rbpf.RBPFError) as ei:
                s.backward_simulate(4)
            assert ei.value.status == rbpf.RBPF_ERR_UNSUPPORTED and "transition density" in str(ei.value)
            st = lib.rbpf_loc_backward_simulate(s.ctx, 4, None, 1, None, None, None)          # the library itself refuses too
            assert st == rbpf.RBPF_ERR_UNSUPPORTED and b"transition density" in lib.rbpf_last_error()
            assert lib.rbpf_loc_advance(s.ctx, 1) == rbpf.RBPF_ERR_STATE
    assert lib.rbpf_device_bytes_live() == base

    class Boom(Exception):
        pass

    def raises(xn, xl):
        raise Boom()

    bad_handles = [(raises, Boom),
                   (lambda xn, xl: tuple(v[:, :-1] for v in tw.tw.measModel(xn, xl)), ValueError),
                   (lambda xn, xl: (tw.tw.measModel(xn, xl)[0].to(torch.float32), tw.tw.measModel(xn, xl)[1]), ValueError),
                   (lambda xn, xl: tw.tw.measModel(xn, xl)[1], ValueError)]
    for meas, exc in bad_handles:
        tw.reset()
        bad = rbpf.DeviceLandmarkMap(rbpf.DeviceSparseHandles(tw.dynModel, meas), p["mean"], p["V"], p["R"])
        with pytest.raises(exc):
            rbpf.particleFilterLocalization(bad, None, *_loc_args(p), rng=_rng(rbpf, p))
        assert lib.rbpf_device_bytes_live() == base
    _compare(tw, *_run(rbpf, tw, p), p, ref)
    assert lib.rbpf_device_bytes_live() == base
