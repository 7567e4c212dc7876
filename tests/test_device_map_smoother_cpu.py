"""Backward simulation in a DeviceMap with a Gaussian transition density (rbpf.DeviceTransition), the parts that need no device: the
checker itself (tests/device_map_smoother_ref.py), the margin condition on every case the GPU tests run (every draw, none
excluded), and the prototypes, exports and refusals that come before any device is touched.

The checker-only tests pass with or without the feature: they validate the committed inputs.  Bounds: the density against the
sampler 1e-12 relative in fp64 (forward substitution of an n_res <= 8 system of condition < 1e3: a few hundred eps); a 2 pi k shift
of an angle row 1e-9 relative (the shift costs eps * 2 pi k absolute in r, amplified by |z| / sd); the known answers five binomial
standard deviations + 1 / M, the form of tests/test_localization_smoother_cpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import device_map_ref as dm
import device_map_smoother_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rbpf_loc_generic_backward_begin", "rbpf_loc_generic_backward_particles_device", "rbpf_loc_generic_backward_step_device",
       "rbpf_loc_generic_backward_finish", "rbpf_loc_generic_backward_workspace_bytes", "rbpf_loc_generic_backward_step"]


def _never(*a):
    raise AssertionError("a handle was called")


# ------------------------------------------------------------------------------------------------
# 1. the checker
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B", "D"])
def test_the_density_inverts_the_sampler(name):
    """At x' = mean(x) + L z on the selected rows, logp = -z'z / 2; adding 2 pi k to an angle row of x' leaves it where it is."""
    c = S.case(name, 8, 4)
    rs = np.random.RandomState(5 + ord(name))
    worst, worst_shift = 0.0, 0.0
    for trial in range(20):
        t = trial % 3
        x = rs.uniform(-2.0, 2.0, (c.nN, 1))
        z = rs.standard_normal(c.n_res)
        cov = c.cov(t)
        xp = c.drift(x, c.p["odometry"][t])[:, 0]
        xp[list(c.rows)] = c.mean(x, t)[:, 0] + np.linalg.cholesky(cov) @ z
        want = -0.5 * z @ z
        got = S.logp(xp, c.mean(x, t), cov, c.rows, c.angle_rows)[0]
        worst = max(worst, abs(got - want) / abs(want))
        for a in c.angle_rows:
            for k in (-2, 1, 3):
                shifted = xp.copy()
                shifted[a] += 2.0 * np.pi * k
                worst_shift = max(worst_shift, abs(S.logp(shifted, c.mean(x, t), cov, c.rows, c.angle_rows)[0] - got) / abs(got))
    print(f"model {name}: largest |logp + z'z/2| / |z'z/2| {worst:.2e}, under a 2 pi k shift {worst_shift:.2e}")
    assert worst < 1e-12
    assert worst_shift < 1e-9


def test_model_a_density_is_what_its_own_dyn_res_norm_gives():
    """-z'z / 2 with z = chol(G dt Q G') \\ r equals -|Lq^-1 G^-1 r|^2 / 2: the two factors of one covariance."""
    c = S.case("A", 8, 4)
    m, p = c.m, c.p
    rs = np.random.RandomState(11)
    for trial in range(10):
        x, xp = rs.uniform(-1, 1, (3, 1)), rs.uniform(-1, 1, 3)
        e = m.dynResNorm(xp, x[:, 0], p["odometry"][0], p["dt"], p["Q"])
        got = S.logp(xp, c.mean(x, 0), c.cov(0), c.rows)[0]
        assert abs(got + 0.5 * e @ e) < 1e-11 * abs(got)


def test_the_forward_pass_of_model_a_is_device_map_refs():
    c = S.case("A", 70, 8)
    X, W, AI = S.forward_arrays(c)
    ref = dm.run(c.m, c.p)
    np.testing.assert_array_equal(AI, ref["ai"])
    np.testing.assert_array_equal(W, ref["w"])
    np.testing.assert_array_equal(X[-1], ref["xn_traj"][:, :, -1])


def _known_answer(name, angle_rows_used):
    c = S.case(name, 30, 6)
    X, W, _ = S.forward_arrays(c)
    T, N = W.shape
    M = 20000
    mus, covs = S.transition_arrays(c, X)
    u = np.random.RandomState(99).random_sample((T, M))
    out = S.backward_simulate(X, W, mus, covs, u, c.rows, angle_rows_used)
    p = np.asarray(S.ffbsm_marginals(X, W, mus, covs, c.rows, c.angle_rows), dtype=np.float64)   # the true density: wrapped
    assert np.max(np.abs(p.sum(axis=1) - 1.0)) < 1e-12
    f = np.stack([np.bincount(out["index"][t], minlength=N) for t in range(T)]) / M
    bound = 5.0 * np.sqrt(p * (1.0 - p) / M) + 1.0 / M
    print(f"model {name}, angle rows {angle_rows_used}: largest |f - p| / bound:", float(np.max(np.abs(f - p) / bound)))
    return f, p, bound, W, M, X


def test_backward_simulation_frequencies_match_the_ffbsm_marginals():
    f, p, bound, W, M, _ = _known_answer("A", ())
    T = W.shape[0]
    assert np.all(np.abs(f - p) <= bound)
    print("largest |p_smooth - w_filter|:", float(np.max(np.abs(p - W))))
    assert np.max(np.abs(p[1:T - 1] - W[1:T - 1])) > 20.0 / M             # smoothing moved the marginals: the filter's weights would fail


def test_known_answer_with_an_angle_row_and_a_run_that_ignores_the_wrap_fails_it():
    f, p, bound, W, M, X = _known_answer("C", (2,))
    T = W.shape[0]
    assert np.all(np.abs(f - p) <= bound)
    assert np.max(np.abs(p[1:T - 1] - W[1:T - 1])) > 20.0 / M
    assert X[:, 2].max() > 3.0 and X[:, 2].min() < -3.0                   # the cloud straddles +-pi
    f_unwrapped, _, _, _, _, _ = _known_answer("C", ())
    assert not np.all(np.abs(f_unwrapped - p) <= bound)                   # the unwrapped density draws from another distribution


def _check_margins(name, margin, eps_ref, logp_rel):
    print(f"{name}: min margin {float(np.min(margin)):.3e}, eps_ref {float(np.max(eps_ref)):.3e}, logp fp64 vs long double {logp_rel:.3e}")
    assert np.all(margin >= 100.0 * eps_ref)                               # every draw: the cap on excluded draws is zero
    assert logp_rel <= 1e-10


@pytest.mark.parametrize("name,N,M", S.PROBE_LOGP_CASES + S.PROBE_INDEX_CASES)
def test_margin_condition_of_the_probe_cases(name, N, M):
    p = S.probe_case(name, N, M)
    o = S.probe_reference(name, N, M)
    rel = float(np.max(np.abs(o["logp"] - o["logp_ld"])) / np.max(np.abs(o["logp_ld"])))
    _check_margins(f"probe {name} {N} x {M}", o["margin"], o["eps_ref"], rel)
    np.testing.assert_array_equal(o["index"], o["index_ld"])
    assert np.all(p["w"][o["index"]] > 0)
    if N > 2048:
        assert o["index"].max() >= 2048                                    # beyond the largest chunk: not the first one
    for a in p["angle_rows"]:                                              # the angle residuals: a few sd from 0 mod 2 pi, never near +-pi
        k = p["rows"].index(a)
        r = S.wrap(p["xs_next"][a][None, :] - p["mu"][k][:, None])
        assert np.max(np.abs(r)) < 2.0
        if N >= 64:
            assert np.max(np.abs(p["xs_next"][a][None, :] - p["mu"][k][:, None])) > 6.0      # ... and the wrap is exercised


@pytest.mark.parametrize("name,N_P,N_T,M", S.FULL_RUNS)
def test_margin_condition_of_the_full_runs(name, N_P, N_T, M):
    """On the restatement's own forward pass (the device's differs from it by rounding; the GPU test repeats the check on the
    device's arrays)."""
    c = S.case(name, N_P, N_T)
    X, W, AI = S.forward_arrays(c)
    _, W_ld, AI_ld = S.forward_arrays(c, np.longdouble)
    np.testing.assert_array_equal(AI, AI_ld)                               # the forward draws sit on no bin edge either
    assert len(np.unique(AI[1:])) > 1
    mus, covs = S.transition_arrays(c, X)
    u = S.full_run_uniforms(N_T, M)
    o = S.backward_simulate(X, W, mus, covs, u, c.rows, c.angle_rows)
    _check_margins(f"full run {name} {N_P} x {N_T} x {M}", o["margin"], o["eps_ref"], o["logp_rel"])
    np.testing.assert_array_equal(o["index"], o["index_ld"])
    import rbpf_oracle as O
    np.testing.assert_array_equal(o["index"][N_T - 1], [O.sample(W[N_T - 1], uu) for uu in u[N_T - 1]])
    if name in ("C", "D"):
        a = c.angle_rows[0]
        assert X[:, a].max() > 3.0 and X[:, a].min() < -3.0               # the heading passes +-pi during the run


# ------------------------------------------------------------------------------------------------
# 2. the library and the binding, before any device
# ------------------------------------------------------------------------------------------------
def test_prototypes_and_exports(rbpf):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rbpf.h")).read(), flags=re.S)
    lib = rbpf.load_library()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in rbpf.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None, name
    assert lib.rbpf_abi_version() == 9 and lib.rbpf_abi_sizeof(14) == -1
    for name in ("DeviceTransition", "device_map_backward_step", "device_map_backward_workspace_bytes"):
        assert hasattr(rbpf, name), name


def test_workspace_bytes(rbpf):
    lib = rbpf.load_library()
    nbytes = C.c_size_t(0)
    nN, nr, N, T, M = 4, 3, 4100, 6, 130
    assert lib.rbpf_loc_generic_backward_workspace_bytes(nN, nr, N, T, M, C.byref(nbytes)) == rbpf.RBPF_OK
    nch = 3                                                                # at least ceil(N / 2048) chunks of partials
    assert nbytes.value >= 8 * ((nr + 1) * N + 2 * nch * M + T * M + nN * M * T + nN * T) + 4 * M * T
    assert rbpf.device_map_backward_workspace_bytes(nN, nr, N, T, 2 * M) > nbytes.value
    for bad in ((0, 1, 8, 3, 4), (9, 1, 8, 3, 4), (4, 0, 8, 3, 4), (4, 9, 8, 3, 4), (4, 5, 8, 3, 4), (4, 3, 0, 3, 4), (4, 3, 8, 0, 4), (4, 3, 8, 3, 0)):
        assert lib.rbpf_loc_generic_backward_workspace_bytes(*bad, C.byref(nbytes)) == rbpf.RBPF_ERR_INVALID_ARG, bad
    assert lib.rbpf_loc_generic_backward_workspace_bytes(nN, nr, N, T, M, None) == rbpf.RBPF_ERR_INVALID_ARG


def test_null_contexts_are_refused(rbpf):
    lib = rbpf.load_library()
    rows = (C.c_int32 * 3)(0, 1, 2)
    t, xn = C.c_int32(0), C.c_void_p()
    assert lib.rbpf_loc_generic_backward_begin(None, 4, None, 1, 3, rows, 0) == rbpf.RBPF_ERR_INVALID_ARG
    assert b"localisation" in lib.rbpf_last_error()
    assert lib.rbpf_loc_generic_backward_particles_device(None, C.byref(t), C.byref(xn)) == rbpf.RBPF_ERR_INVALID_ARG
    assert lib.rbpf_loc_generic_backward_step_device(None, None, None) == rbpf.RBPF_ERR_INVALID_ARG
    assert lib.rbpf_loc_generic_backward_finish(None, None, None, None) == rbpf.RBPF_ERR_INVALID_ARG


def _probe_status(rbpf, p, **kw):
    a = dict(mu=p["mu"], w=p["w"], xs_next=p["xs_next"], cov=p["cov"], u=p["u"], rows=p["rows"], angle_rows=p["angle_rows"])
    a.update(kw)
    with pytest.raises(rbpf.RBPFError) as ei:
        rbpf.device_map_backward_step(**a)
    return ei.value


def test_the_probe_refuses_bad_arguments_before_any_device(rbpf):
    lib = rbpf.load_library()
    p = S.probe_case("D", 70, 5)
    for kw in (dict(rows=(0, 1, 1)), dict(rows=(0, 1, 4)), dict(rows=(0, 1, -1)), dict(angle_rows=(2,)), dict(rows=(0, 1)),
               dict(cov=np.eye(2)), dict(cov=np.eye(4)), dict(rows=None)):
        assert _probe_status(rbpf, p, **kw).status == rbpf.RBPF_ERR_INVALID_ARG, kw
    bad = np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    e = _probe_status(rbpf, p, cov=bad)
    assert e.status == rbpf.RBPF_ERR_CHOL_FAILED and "positive definite" in str(e)
    assert _probe_status(rbpf, p, cov=np.full((3, 3), np.nan)).status == rbpf.RBPF_ERR_CHOL_FAILED
    # the C entry point itself: NULL arguments, n_res outside 1 .. 8, a mask bit that names no row
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))                                      # noqa: E731
    mu, w, xs, cov, u = (np.ascontiguousarray(p[k]) for k in ("mu", "w", "xs_next", "cov", "u"))
    xs = np.asfortranarray(xs)
    rows = (C.c_int32 * 9)(0, 1, 3, 2, 0, 0, 0, 0, 0)
    idx = (C.c_int32 * 5)()
    call = lambda **kw: lib.rbpf_loc_generic_backward_step(*[kw.get(k, v) for k, v in (                                    # noqa: E731
        ("N", 70), ("M", 5), ("nN", 4), ("nr", 3), ("rows", rows), ("mask", 4), ("mu", dp(mu)), ("w", dp(w)), ("xs", dp(xs)), ("cov", dp(cov)),
        ("u", dp(u)), ("index", idx), ("logp", None), ("reps", 1), ("ms", None))])
    for k in ("rows", "mu", "w", "xs", "cov", "u", "index"):
        assert call(**{k: None}) == rbpf.RBPF_ERR_INVALID_ARG, k
    dup, far, neg = (C.c_int32 * 3)(0, 1, 1), (C.c_int32 * 3)(0, 1, 4), (C.c_int32 * 3)(0, -1, 2)
    for kw in (dict(nr=0), dict(nr=9), dict(N=0), dict(M=0), dict(nN=0), dict(nN=9), dict(mask=8), dict(rows=dup, mask=0),
               dict(rows=far, mask=0), dict(rows=neg, mask=0)):
        assert call(**kw) == rbpf.RBPF_ERR_INVALID_ARG, kw
    if rbpf.device_count() == 0:
        assert call() == rbpf.RBPF_ERR_NO_DEVICE
        with pytest.raises(rbpf.RBPFError) as ei:
            rbpf.device_map_backward_step(p["mu"], p["w"], p["xs_next"], p["cov"], p["u"], rows=p["rows"], angle_rows=p["angle_rows"])
        assert ei.value.status == rbpf.RBPF_ERR_NO_DEVICE


def test_device_transition_states_rows_and_covariance(rbpf):
    tr = rbpf.DeviceTransition(_never)
    assert tr.resolve(5) == ((0, 1, 2, 3, 4), 0)
    tr = rbpf.DeviceTransition(_never, rows=(0, 1, 3), angle_rows=(3,))
    assert tr.resolve(4) == ((0, 1, 3), 4)                                 # bit k marks rows[k]
    for kw, nN in ((dict(rows=(0, 0)), 3), (dict(rows=(0, 3)), 3), (dict(rows=(-1,)), 3), (dict(rows=()), 3), (dict(), 9),
                   (dict(rows=(0, 1), angle_rows=(2,)), 3)):
        with pytest.raises(rbpf.RBPFError) as ei:
            rbpf.DeviceTransition(_never, **kw).resolve(nN)
        assert ei.value.status == rbpf.RBPF_ERR_INVALID_ARG, kw
    # the default cov = dt Q needs n_w == n_res, and says so
    Q = np.diag([1.0, 2.0])
    np.testing.assert_array_equal(rbpf.DeviceTransition(_never).covariance(0.5, Q, 2), 0.5 * Q)
    with pytest.raises(rbpf.RBPFError) as ei:
        rbpf.DeviceTransition(_never).covariance(0.5, Q, 3)
    assert ei.value.status == rbpf.RBPF_ERR_INVALID_ARG and "n_w == n_res" in str(ei.value)
    with pytest.raises(rbpf.RBPFError) as ei:                              # a cov of the wrong shape
        rbpf.DeviceTransition(_never, cov=lambda dt, Q: np.eye(2)).covariance(0.5, Q, 3)
    assert ei.value.status == rbpf.RBPF_ERR_INVALID_ARG
    c = S.case("D", 8, 4)
    got = rbpf.DeviceTransition(_never, cov=c.cov_of, rows=c.rows, angle_rows=c.angle_rows).covariance(c.dtt(0), c.Q(0), 3)
    np.testing.assert_array_equal(got, c.cov(0))
    with pytest.raises(TypeError):
        rbpf.DeviceTransition(None)


def test_a_device_map_takes_a_transition_and_a_dense_mag_map_does_not(rbpf):
    m, p = dm.case((3, 3, 3, 2, 5), 4, 3)
    h = rbpf.DeviceHandles(_never, _never)
    tr = rbpf.DeviceTransition(_never)
    assert rbpf.DeviceMap(h, p["mean"], p["V"], p["R"], transition=tr).transition is tr
    assert rbpf.DeviceMap(h, p["mean"], p["V"], p["R"]).transition is None
    assert rbpf.DeviceMap.from_posterior(h, p["mean"], p["V"].T @ p["V"] + 0.1 * np.eye(5), p["R"], transition=tr).transition is tr
    with pytest.raises(TypeError):
        rbpf.DeviceMap(h, p["mean"], p["V"], p["R"], transition=_never)
    import localization_ref as R
    c = R.loc_case(8, 3, 13)
    mag = rbpf.DenseMagMap(rbpf.DenseMagModel(c["NN"], c["L"]), c["mean"], c["V"], c["sigma2"])
    args = (c["odometry"], c["y"], c["x0_nonLin"], c["Q"], np.eye(3), c["N_P"], 4, c["dt"])
    for dyn, meas in ((mag.dynModel, tr), (tr, mag.measModel), (tr, None)):
        with pytest.raises(rbpf.RBPFError) as ei:
            rbpf.particleSmootherLocalization(dyn, meas, *args)
        assert ei.value.status == rbpf.RBPF_ERR_UNSUPPORTED and "DeviceTransition" in str(ei.value)


def test_without_a_device_the_smoother_raises_no_device(rbpf):
    if rbpf.device_count() > 0:
        pytest.skip("a GPU is visible")
    m, p = dm.case((3, 3, 3, 2, 5), 4, 3)
    mp = rbpf.DeviceMap(rbpf.DeviceHandles(_never, _never), p["mean"], p["V"], p["R"], transition=rbpf.DeviceTransition(_never))
    with pytest.raises(rbpf.RBPFError) as ei:
        rbpf.particleSmootherLocalization(mp, None, p["odometry"], p["y"], p["x0_nonLin"], p["Q"], p["R"], p["N_P"], 4, p["dt"])
    assert ei.value.status == rbpf.RBPF_ERR_NO_DEVICE
