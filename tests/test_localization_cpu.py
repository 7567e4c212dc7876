"""Localisation in a fixed GP map, the parts that need no device: the checker itself (tests/localization_ref.py), the workspace
query, the refusals and the host-side validation."""
import ctypes as C

import numpy as np
import pytest

import localization_ref as R
import rbpf_oracle as O


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(float(np.max(np.abs(b))), 1e-300))


def test_restatement_map_is_the_batch_gp_posterior():
    c = R.loc_case(8, 12, 40, seed=3)
    NN, L, theta = c["NN"], c["L"], c["theta"]
    sigma2 = float(theta[3])
    Phi = np.vstack(R.grad_rows(NN, L, c["train_x"]))
    k = R.prior_k(NN, L, theta)
    # independently: the normal equations of the regression, solved without the Cholesky factor
    A = Phi.T @ Phi + np.diag(sigma2 / k)
    mean = np.linalg.solve(A, Phi.T @ c["train_y"].reshape(-1, order="F"))
    P = sigma2 * np.linalg.inv(A)
    assert _rel(c["mean"], mean) < 1e-12
    rs = np.random.RandomState(0)
    pts = np.column_stack([rs.uniform(-L[a], L[a], 9) for a in range(3)])
    for g in R.grad_rows(NN, L, pts):
        vg = np.sum((g @ c["V"].T) ** 2, axis=1)
        gPg = np.sum((g @ P) * g, axis=1)
        assert _rel(vg, gPg) < 1e-12
    assert np.array_equal(c["V"], np.tril(c["V"]))
    assert _rel(c["V"].T @ c["V"], P) < 1e-12


def test_dtype_generic_twins_equal_the_oracle_primitives_in_fp64():
    rs = np.random.RandomState(1)
    L, NN = O.domain_cartesian_dx(30, 3, np.array([[-3.0, -2.0, -1.0], [3.0, 2.0, 1.0]]))
    x = np.column_stack([rs.uniform(-L[a], L[a], 5) for a in range(3)])
    for di in range(3):
        assert np.array_equal(R._eigenfun_dx(NN, x, di, L, np.float64), O.eigenfun_dx(NN, x, di, L))
    q = rs.standard_normal(4)
    q /= np.linalg.norm(q)
    assert np.array_equal(R._quat2rmat(q), O.quat2rmat(q))
    assert np.array_equal(R._qLeft(q), O.qLeft(q))
    assert np.array_equal(R._qRight(q), O.qRight(q))
    for phi in (rs.standard_normal(3), np.zeros(3), np.array([2.0, 0.0, 0.0])):
        assert np.array_equal(R._expq(phi), O.expq(phi))
    w = rs.random_sample(50)
    w /= w.sum()
    for u in rs.random_sample(20):
        assert R._sample(w, u) == O.sample(w, u)


def test_restatement_dyn_model_is_not_the_slam_closure():
    """(dq (x) q) (x) e with the element-wise square root -- against q (x) (dq (x) e) with Cholesky factors."""
    rs = np.random.RandomState(2)
    q = rs.standard_normal(4)
    q /= np.linalg.norm(q)
    dq = O.expq(0.3 * rs.standard_normal(3))
    xn = np.concatenate((rs.standard_normal(3), q))
    dx = np.concatenate((rs.standard_normal(3), dq))
    Q = np.diag([0.1, 0.2, 0.3, 0.01, 0.02, 0.03])
    Q[0, 1] = Q[1, 0] = 0.05
    z = rs.standard_normal(6)
    out = R.dyn_model(xn, dx, 0.5, Q, z)
    e = O.expq(np.sqrt(0.5 * Q[3:6, 3:6]) @ z[3:6])
    assert np.allclose(out[3:7], O.qLeft(O.qLeft(dq) @ q) @ e, atol=1e-15)
    assert np.allclose(out[0:3], xn[0:3] + dx[0:3] + np.sqrt(0.5 * Q[0:3, 0:3]) @ z[0:3], atol=1e-15)
    slam = O.DenseMagModel(NN=np.zeros((1, 3)), L=np.ones(3)).dynModel(xn, dx, 0.5, Q, z)[0]
    assert not np.allclose(out, slam, atol=1e-6)


def _structs(rbpf, n, N_P, N_T=10, V=True, table=False):
    import importlib
    ffi = importlib.import_module("rao-blackwellized-slam-smoothing_amd._ffi")
    m = n - 3
    keep = dict(NN=np.ones((max(m, 1), 3), dtype=np.int32, order="F"), mean=np.zeros(n), V=np.eye(n, order="F"),
                tab=np.ones((N_P, 3), order="F"), odo=np.zeros((N_T, 7), order="F"), y=np.zeros((N_T, 3), order="F"),
                x0=np.array([0, 0, 0, 1.0, 0, 0, 0]), Q=np.eye(6, order="F"), dt=np.ones(1))
    dp = lambda a: a.ctypes.data_as(ffi.c_double_p)                                    # noqa: E731
    mp = ffi.rbpf_loc_map()
    mp.m_basis = m
    mp.NN = keep["NN"].ctypes.data_as(ffi.c_int32_p)
    mp.L[0] = mp.L[1] = mp.L[2] = 1.0
    mp.mean, mp.sigma2 = dp(keep["mean"]), 1.0
    if V:
        mp.V = dp(keep["V"])
    if table:
        mp.var_table = dp(keep["tab"])
    pr = ffi.rbpf_loc_problem()
    pr.N_P, pr.N_T, pr.x0_cols, pr.q_pages, pr.dt_len, pr.odo_ld = N_P, N_T, 1, 1, 1, N_T
    pr.odometry, pr.y, pr.x0_nonlin, pr.Q, pr.dt = dp(keep["odo"]), dp(keep["y"]), dp(keep["x0"]), dp(keep["Q"]), dp(keep["dt"])
    return ffi, mp, pr, keep


def test_workspace_bytes_need_no_device_and_hold_no_per_particle_basis_array(rbpf):
    ffi, mp, pr, keep = _structs(rbpf, 1003, 4096)
    opt = ffi.rbpf_options(keep_history=0, trace=0)
    b1 = rbpf.loc_workspace_bytes(mp, pr, opt)
    pr.N_P = 65536
    b2 = rbpf.loc_workspace_bytes(mp, pr, opt)
    pr.N_P = 2 * 65536
    b3 = rbpf.loc_workspace_bytes(mp, pr, opt)
    slope = (b2 - b1) / (65536 - 4096)
    assert 0 < slope < 1024, slope                                  # an N_P x n array would be 8 KB per particle at n = 1003
    assert abs((b3 - b2) / 65536 - slope) < 1.0                     # linear in N_P
    assert b1 >= 1003 * 1003 * 8                                    # the shared factor is there once


def test_workspace_bytes_refusals(rbpf):
    lib = rbpf.load_library()
    nbytes = C.c_size_t(0)

    def status(mp, pr, opt=None):
        return lib.rbpf_loc_workspace_bytes(C.byref(mp), C.byref(pr), C.byref(opt) if opt is not None else None, C.byref(nbytes))

    ffi, mp, pr, keep = _structs(rbpf, 133, 64)
    assert status(mp, pr) == rbpf.RBPF_OK
    mp.struct_size = C.sizeof(ffi.rbpf_loc_map) - 8                 # a binding built against another layout
    assert status(mp, pr) == rbpf.RBPF_ERR_INVALID_ARG
    ffi, mp, pr, keep = _structs(rbpf, 133, 64)
    pr.struct_size = C.sizeof(ffi.rbpf_loc_problem) + 8
    assert status(mp, pr) == rbpf.RBPF_ERR_INVALID_ARG
    ffi, mp, pr, keep = _structs(rbpf, 133, 64, V=True, table=True)  # both set
    assert status(mp, pr) == rbpf.RBPF_ERR_INVALID_ARG
    ffi, mp, pr, keep = _structs(rbpf, 133, 64, V=False, table=False)  # both NULL
    assert status(mp, pr) == rbpf.RBPF_ERR_INVALID_ARG
    ffi, mp, pr, keep = _structs(rbpf, 133, 64, V=False, table=True)
    assert status(mp, pr) == rbpf.RBPF_OK
    ffi, mp, pr, keep = _structs(rbpf, 1152, 64)                    # n > 1151
    assert status(mp, pr) == rbpf.RBPF_ERR_INVALID_ARG
    ffi, mp, pr, keep = _structs(rbpf, 1151, 64)
    assert status(mp, pr) == rbpf.RBPF_OK
    ffi, mp, pr, keep = _structs(rbpf, 133, 64)
    opt = ffi.rbpf_options(struct_size=C.sizeof(ffi.rbpf_options) - 8)
    assert status(mp, pr, opt) == rbpf.RBPF_ERR_INVALID_ARG
    assert status(mp, pr, ffi.rbpf_options(n_devices=2)) == rbpf.RBPF_ERR_UNSUPPORTED
    assert lib.rbpf_abi_sizeof(9) == C.sizeof(ffi.rbpf_loc_map)
    assert lib.rbpf_abi_sizeof(10) == C.sizeof(ffi.rbpf_loc_problem)
    assert lib.rbpf_abi_sizeof(11) == C.sizeof(ffi.rbpf_loc_out)


def _small_map(rbpf, m=13, var_points=None):
    c = R.loc_case(8, 6, m, seed=2)
    model = rbpf.DenseMagModel(c["NN"], c["L"])
    return c, model, rbpf.DenseMagMap(model, c["mean"], c["V"], c["sigma2"], var_points=var_points)


def test_no_cpu_fallback_without_a_device(rbpf):
    if rbpf.device_count() > 0:
        pytest.skip("a device is visible: the refusal cannot be observed here")
    c, model, mp = _small_map(rbpf)
    with pytest.raises(rbpf.RBPFError) as ei:
        rbpf.particleFilterLocalization(mp.dynModel, mp.measModel, c["odometry"], c["y"], c["x0_nonLin"], c["Q"], np.eye(3), c["N_P"],
                                        c["dt"], rng=rbpf.ReplayRNG(c["U"], c["Z"]))
    assert ei.value.status == rbpf.RBPF_ERR_NO_DEVICE


def test_from_posterior_rejects_an_indefinite_covariance(rbpf):
    c, model, _ = _small_map(rbpf)
    n = model.nLin
    P = np.eye(n)
    P[2, 2] = -1.0
    with pytest.raises(ValueError):
        rbpf.DenseMagMap.from_posterior(model, np.zeros(n), P, 1.0)
    good = c["V"].T @ c["V"]
    mp = rbpf.DenseMagMap.from_posterior(model, c["mean"], good, c["sigma2"])
    assert np.array_equal(mp.V, np.tril(mp.V))
    assert _rel(mp.V.T @ mp.V, good) < 1e-12


def test_from_data_equals_the_restatement(rbpf):
    c, model, _ = _small_map(rbpf, m=40)
    mp = rbpf.DenseMagMap.from_data(model, c["train_x"], c["train_y"], c["theta"])
    assert _rel(mp.mean, c["mean"]) < 1e-10
    assert _rel(mp.V.T @ mp.V, c["V"].T @ c["V"]) < 1e-10


def test_too_few_var_points_is_a_value_error(rbpf):
    c, model, mp = _small_map(rbpf, var_points=np.zeros((c_n := 5, 3)))
    assert c_n < c["N_P"]
    with pytest.raises(ValueError):
        mp._loc_map(c["N_P"])
    if rbpf.device_count() == 0:
        with pytest.raises((ValueError, rbpf.RBPFError)) as ei:
            rbpf.particleFilterLocalization(mp.dynModel, mp.measModel, c["odometry"], c["y"], c["x0_nonLin"], c["Q"], np.eye(3),
                                            c["N_P"], c["dt"], rng=rbpf.ReplayRNG(c["U"], c["Z"]))
        assert isinstance(ei.value, ValueError) or ei.value.status == rbpf.RBPF_ERR_NO_DEVICE


def test_unrecognised_handles_are_refused_before_anything_runs(rbpf):
    c, model, mp = _small_map(rbpf)
    with pytest.raises(rbpf.RBPFError) as ei:
        rbpf.particleFilterLocalization(lambda *a: None, lambda *a: None, c["odometry"], c["y"], c["x0_nonLin"], c["Q"], np.eye(3),
                                        c["N_P"], c["dt"])
    assert ei.value.status == rbpf.RBPF_ERR_UNSUPPORTED
