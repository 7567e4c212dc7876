"""The EKF baseline on the device (rbpf_ekf_dense: ekf.ekf_dense_device / ekf_dense_batch) against the oracle's ekf_dense.

Tolerance: the project's own for this estimator (tests/test_gpu_helpers.py::test_ekf_baseline_matches_oracle),
max|got - ref| <= 1e-9 max(1, max|ref|) for each of xf_traj, qnb_traj, Pf_traj.  Where the issue asks for equality (a run alone
against the same run in a batch, keep_P on and off) the comparison is bit for bit."""
import functools
import importlib

import numpy as np
import pytest

import cases
import rbpf_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-9
#          m   N_T seed
PARITY = [(40, 14, 8),       # n = 49: one partial row tile
          (61, 14, 5),       # n = 70: one full tile + 6 tail rows
          (125, 40, 3),      # n = 134: tail past 128; 40 steps of carried PH
          (253, 24, 2),      # n = 262
          (512, 6, 1)]       # n = 521: the protocol's size


@pytest.fixture(scope="module")
def ekf(rbpf):
    return importlib.import_module(rbpf.__name__ + ".ekf")


def _inputs(c):
    n = c["m"] + 3                                                              # run_dense3D_magfield.m:248-250
    x0 = np.concatenate((c["x0_nonLin"][0:3], np.zeros(3), np.asarray(c["x0_lin"]).ravel()))
    P0 = np.zeros((6 + n, 6 + n))
    P0[6:, 6:] = c["P0_lin"]
    return x0, c["x0_nonLin"][3:7], P0


@functools.lru_cache(maxsize=None)
def _case(m, N_T, seed):
    c = cases.mag_case(4, N_T, m, seed=seed)
    x0, q0, P0 = _inputs(c)
    ref = O.ekf_dense(c["model"], c["LL"], c["odometry"], c["y"], x0, q0, P0, c["Q"], c["R"], c["dt"])
    for r in ref:
        r.setflags(write=False)
    return c, x0, q0, P0, ref


def _check(got, ref, what=""):
    dist = [float(np.max(np.abs(g - r)) / max(1.0, float(np.max(np.abs(r))))) for g, r in zip(got, ref)]
    print(f"{what} device - oracle (xf_traj, qnb_traj, Pf): {dist}")
    for g, r in zip(got, ref):
        assert g.shape == r.shape
    assert max(dist) <= TOL, dist


def _live(rbpf):
    return int(rbpf.load_library().rbpf_device_bytes_live())


@pytest.mark.parametrize("m,N_T,seed", PARITY)
def test_device_ekf_matches_oracle(rbpf, ekf, m, N_T, seed):
    c, x0, q0, P0, ref = _case(m, N_T, seed)
    mdl, _, _, R = cases.device_model(rbpf, c)
    got = ekf.ekf_dense_device(mdl, c["LL"], c["odometry"], c["y"], x0, q0, P0, c["Q"], R, c["dt"], keep_P=True)
    _check(got, ref, f"n = {m + 9}, N_T = {N_T}:")
    assert np.array_equal(got[2], np.transpose(got[2], (1, 0, 2)))             # the update keeps P symmetric bit for bit


def test_time_varying_Q_and_dt(rbpf, ekf):
    c, x0, q0, P0, _ = _case(61, 14, 5)
    N_T = c["y"].shape[0]
    scale = 0.5 + np.arange(N_T - 1) % 4                                       # a different Q on every page
    Q = c["Q"][:, :, None] * scale[None, None, :]
    dt = c["dt"] * (1.0 + 0.25 * (np.arange(N_T - 1) % 3))
    ref = O.ekf_dense(c["model"], c["LL"], c["odometry"], c["y"], x0, q0, P0, Q, c["R"], dt)
    mdl, _, _, R = cases.device_model(rbpf, c)
    _check(ekf.ekf_dense_device(mdl, c["LL"], c["odometry"], c["y"], x0, q0, P0, Q, R, dt), ref, "Q pages, dt vector:")


def test_batch_is_bit_identical_to_single_runs(rbpf, ekf):
    """B = 5 at m = 61: three seeds = three models with their own LL; two more runs share the first model, with the
    magnetometer disturbances 1 and 10 on the second body axis (run_dense3D_magfield.m:81)."""
    runs = []
    shared = None
    for seed, off in ((5, 0.0), (6, 0.0), (7, 0.0), (5, 1.0), (5, 10.0)):
        c, x0, q0, P0, ref = _case(61, 14, seed)
        y = c["y"] + np.array([0.0, off, 0.0])
        if off:
            ref = O.ekf_dense(c["model"], c["LL"], c["odometry"], y, x0, q0, P0, c["Q"], c["R"], c["dt"])
        mdl, _, _, R = cases.device_model(rbpf, c)
        if seed == 5:
            shared = shared or mdl
            mdl = shared                                                       # the same object: the model pointers repeat
        runs.append(dict(c=c, mdl=mdl, y=y, x0=x0, q0=q0, P0=P0, R=R, ref=ref))

    def batch(rs):
        return ekf.ekf_dense_batch([r["mdl"] for r in rs], np.stack([r["c"]["LL"] for r in rs]), np.stack([r["c"]["odometry"] for r in rs]),
                                   np.stack([r["y"] for r in rs]), np.stack([r["x0"] for r in rs]), np.stack([r["q0"] for r in rs]),
                                   np.stack([r["P0"] for r in rs]), rs[0]["c"]["Q"], np.stack([r["R"] for r in rs]), rs[0]["c"]["dt"], keep_P=True)

    fwd, rev = batch(runs), batch(runs[::-1])
    for b, r in enumerate(runs):
        got = tuple(o[b] for o in fwd)
        _check(got, r["ref"], f"run {b} of the batch:")
        alone = ekf.ekf_dense_device(r["mdl"], r["c"]["LL"], r["c"]["odometry"], r["y"], r["x0"], r["q0"], r["P0"], r["c"]["Q"], r["R"],
                                     r["c"]["dt"], keep_P=True)
        for g, a_, v in zip(got, alone, rev):
            assert np.array_equal(g, a_)
            assert np.array_equal(g, v[len(runs) - 1 - b])


def test_keep_P_false_returns_the_last_page(rbpf, ekf):
    c, x0, q0, P0, _ = _case(61, 14, 5)
    mdl, _, _, R = cases.device_model(rbpf, c)
    args = (mdl, c["LL"], c["odometry"], c["y"], x0, q0, P0, c["Q"], R, c["dt"])
    xf1, q1, P1 = ekf.ekf_dense_device(*args, keep_P=True)
    xf0, q0_, Pl = ekf.ekf_dense_device(*args, keep_P=False)
    assert Pl.shape == (x0.size, x0.size)
    assert np.array_equal(Pl, P1[:, :, -1]) and np.array_equal(xf0, xf1) and np.array_equal(q0_, q1)


def test_jitter_branch_and_second_failure(rbpf, ekf):
    """P0 = 0, Q = 0, R = -5e-4 I: every step fails the first factorisation and passes the retry with jitter 1e-3
    (ekf_dense.m:83-86); R = -I fails both: CholeskyFailure in the oracle, RBPF_ERR_CHOL_FAILED on the device."""
    c, x0, q0, P0, _ = _case(40, 14, 8)
    mdl = cases.device_model(rbpf, c)[0]
    Z, Q0 = np.zeros_like(P0), np.zeros((6, 6))
    ref = O.ekf_dense(c["model"], c["LL"], c["odometry"], c["y"], x0, q0, Z, Q0, -5e-4 * np.eye(3), c["dt"])
    assert all(np.isfinite(r).all() for r in ref)
    _check(ekf.ekf_dense_device(mdl, c["LL"], c["odometry"], c["y"], x0, q0, Z, Q0, -5e-4 * np.eye(3), c["dt"]), ref, "jitter branch:")
    with pytest.raises(O.CholeskyFailure):
        O.ekf_dense(c["model"], c["LL"], c["odometry"], c["y"], x0, q0, Z, Q0, -np.eye(3), c["dt"])
    live = _live(rbpf)
    with pytest.raises(rbpf.RBPFError) as ei:
        ekf.ekf_dense_device(mdl, c["LL"], c["odometry"], c["y"], x0, q0, Z, Q0, -np.eye(3), c["dt"])
    assert ei.value.status == rbpf.RBPF_ERR_CHOL_FAILED
    assert _live(rbpf) == live


def test_refusals_and_device_memory(rbpf, ekf):
    c, x0, q0, P0, _ = _case(61, 14, 5)
    mdl, _, _, R = cases.device_model(rbpf, c)
    live = _live(rbpf)
    ekf.ekf_dense_device(mdl, c["LL"], c["odometry"], c["y"], x0, q0, P0, c["Q"], R, c["dt"], keep_P=False)
    assert _live(rbpf) == live
    radio = rbpf.DenseRadioModel(np.ones((8, 2), dtype=np.int32), [1.0, 1.0])
    with pytest.raises(rbpf.RBPFError) as ei:
        ekf.ekf_dense_device(radio, c["LL"], c["odometry"], c["y"], x0, q0, P0, c["Q"], R, c["dt"])
    assert ei.value.status == rbpf.RBPF_ERR_UNSUPPORTED and "dense-mag" in str(ei.value)
    assert _live(rbpf) == live
    c2 = _case(40, 14, 8)[0]
    other = cases.device_model(rbpf, c2)[0]
    two = lambda a: np.stack([a, a])                                           # noqa: E731
    with pytest.raises(rbpf.RBPFError) as ei:
        ekf.ekf_dense_batch([mdl, other], two(c["LL"]), two(c["odometry"]), two(c["y"]), two(x0), two(q0), two(P0), c["Q"], R, c["dt"])
    assert ei.value.status == rbpf.RBPF_ERR_INVALID_ARG
    assert _live(rbpf) == live


def test_device_ekf_matches_the_host_path(rbpf, ekf):
    """ekf.ekf_dense (host recursion over the helper kernels, what the tools run by default) and the device recursion."""
    c, x0, q0, P0, _ = _case(40, 14, 8)
    mdl, _, _, R = cases.device_model(rbpf, c)
    args = (mdl, c["LL"], c["odometry"], c["y"], x0, q0, P0, c["Q"], R, c["dt"])
    _check(ekf.ekf_dense_device(*args), ekf.ekf_dense(*args), "device - host path:")


def test_protocol_tool_with_the_device_ekf(rbpf):
    """tools/boxplot_mag.py ekf="device" (the levels of a simulation in one ekf_dense_batch call) against its default host path,
    on a small instance.  The tool rounds its RMSEs to 1e-4 m, and trajectories that agree to 1e-9 give RMSEs that agree far
    below that, so the rounded figures may differ by one unit of the last place at most."""
    import os
    import sys
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import boxplot_mag
    kw = dict(n_sim=1, N_K=1, N_P=8, m=40, N_T=16, levels=(0.0, 10.0))
    host, dev = boxplot_mag.run_protocol(**kw), boxplot_mag.run_protocol(ekf="device", **kw)
    assert host["ekf"] == "host" and dev["ekf"] == "device"
    for rh, rd in zip(host["table"], dev["table"]):
        assert np.max(np.abs(np.asarray(rh["ekf"]) - np.asarray(rd["ekf"]))) <= 1.0001e-4
