"""Localisation in the fixed landmark map of a sparseFeatures device-code model (rbpf.DeviceLandmarkMap, rbpf_loc_landmark_*):
everything that holds without a device -- the prototypes, the unchanged ABI, the refusals that come before any device is touched,
the factorisation of from_posterior, the checker checked against the oracle's sparseFeatures filter, and the condition on the GPU
tests' full-run cases (tests/landmark_map_ref.py): the float64 and the long-double restatement draw identical ancestors at every
step, so "indices exact" is a fair demand of the device."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import generic_ny_cases as gc
import landmark_map_ref as lm
import rbpf_oracle as O
from test_generic_device_cpu import ABI9_SIZES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rbpf_loc_landmark_create", "rbpf_loc_landmark_map_device", "rbpf_loc_landmark_step_device", "rbpf_loc_landmark_yhattraj",
       "rbpf_loc_landmark_weights"]


def _ffi(rbpf):
    return importlib.import_module(rbpf.__name__ + "._ffi")


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _never(*a):
    raise AssertionError("a handle was called")


def test_prototypes_are_declared_exported_and_mirrored(rbpf):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rbpf.h")).read(), flags=re.S)
    lib = rbpf.load_library()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in rbpf.EXPORTS
        assert getattr(lib, name).argtypes is not None, name
    assert hasattr(rbpf, "DeviceLandmarkMap") and hasattr(rbpf, "landmark_map_weights")
    assert issubclass(rbpf.DeviceLandmarkMap, rbpf.DeviceMap)             # accepted wherever a DeviceMap is


def test_abi_is_9_and_no_struct_changed_size(rbpf):
    lib = rbpf.load_library()
    assert lib.rbpf_abi_version() == 9
    assert [lib.rbpf_abi_sizeof(w) for w in range(len(ABI9_SIZES))] == ABI9_SIZES
    assert lib.rbpf_abi_sizeof(len(ABI9_SIZES)) == -1


class _Args:
    """Valid arguments of rbpf_loc_landmark_create at (n_nonlin, n_y, n_lin) = (3, 4, 6), N_P = 4, N_T = 3; fields are replaced per test."""

    def __init__(self, rbpf, **kw):
        ffi = _ffi(rbpf)
        self.nN, self.d, self.n, self.N, self.T, self.cols = 3, 4, 6, 4, 3, 1
        self.mean, self.V, self.R = np.zeros(6), np.asfortranarray(np.eye(6)), None
        self.y, self.x0 = np.zeros((3, 4), order="F"), np.zeros((3, 1), order="F")
        self.y[1, 2] = np.nan
        self.U = np.full((1, 2, 4), 0.5)
        self.rng = ffi.rbpf_rng()
        self.rng.mode, self.rng.n_iter, self.rng.U = ffi.RBPF_RNG_REPLAY, 1, _dp(self.U)
        self.opt = ffi.rbpf_options(keep_history=1)
        self.null = set()
        for k, v in kw.items():
            setattr(self, k, v)
        if self.R is None:
            self.R = np.asfortranarray(gc.full_R(max(self.d, 1), 1))

    def call(self, lib):
        ctx = C.c_void_p()
        p = lambda name: None if name in self.null else _dp(getattr(self, name))              # noqa: E731
        st = lib.rbpf_loc_landmark_create(self.nN, self.d, self.n, p("mean"), p("V"), p("R"), self.N, self.T, p("y"), p("x0"), self.cols,
                                          None if "rng" in self.null else C.byref(self.rng), C.byref(self.opt),
                                          None if "ctx" in self.null else C.byref(ctx))
        assert not ctx.value or st == 0
        if ctx.value:
            lib.rbpf_destroy(ctx)
        return st


def _weights_args(rbpf, **kw):
    a = dict(d=4, n=6, N=5, yhat=_dp(np.zeros((5, 4))), yl=2, dy=_dp(np.zeros((5, 4, 6))), dl=2, ldx=0, V=_dp(np.asfortranarray(np.eye(6))),
             R=_dp(np.asfortranarray(gc.full_R(4, 1))), y=_dp(np.zeros(4)), logw=_dp(np.zeros(5)))
    a.update(kw)
    return (a["d"], a["n"], a["N"], a["yhat"], a["yl"], a["dy"], a["dl"], a["ldx"], a["V"], a["R"], a["y"], None, a["logw"], 1, None)


def test_null_arguments_are_invalid_before_a_device_is_needed(rbpf):
    lib = rbpf.load_library()
    for name in ("mean", "V", "R", "y", "x0", "rng", "ctx"):
        assert _Args(rbpf, null={name}).call(lib) == rbpf.RBPF_ERR_INVALID_ARG, name
    ldx, p1 = C.c_int32(0), C.c_void_p()
    out = np.zeros(16)
    assert lib.rbpf_loc_landmark_map_device(None, C.byref(p1), C.byref(ldx)) == rbpf.RBPF_ERR_INVALID_ARG
    assert lib.rbpf_loc_landmark_step_device(None, None, None, 2, None, 2) == rbpf.RBPF_ERR_INVALID_ARG
    assert lib.rbpf_loc_landmark_yhattraj(None, _dp(out)) == rbpf.RBPF_ERR_INVALID_ARG
    for kw in (dict(yhat=None), dict(dy=None), dict(V=None), dict(R=None), dict(y=None), dict(yl=1), dict(yl=3), dict(dl=3), dict(dl=-1),
               dict(N=0), dict(d=0), dict(n=0), dict(dl=1, ldx=5)):
        assert lib.rbpf_loc_landmark_weights(*_weights_args(rbpf, **kw)) == rbpf.RBPF_ERR_INVALID_ARG, kw
    for kw in (dict(d=33), dict(n=97)):
        assert lib.rbpf_loc_landmark_weights(*_weights_args(rbpf, **kw)) == rbpf.RBPF_ERR_UNSUPPORTED, kw


@pytest.mark.parametrize("field,value", [("d", 0), ("d", 33), ("n", 0), ("n", 97), ("nN", 0), ("nN", 9), ("N", 0), ("T", 0), ("cols", 2)])
def test_sizes_out_of_range_are_refused(rbpf, field, value):
    st = _Args(rbpf, **{field: value}).call(rbpf.load_library())
    assert st == (rbpf.RBPF_ERR_UNSUPPORTED if value in (33, 97, 9) else rbpf.RBPF_ERR_INVALID_ARG)


def test_an_r_that_is_not_positive_definite_is_refused_at_creation(rbpf):
    lib = rbpf.load_library()
    R = np.asfortranarray(gc.full_R(4, 1))
    R[0, 1] = R[1, 0] = 1.0                                               # symmetric, indefinite
    assert _Args(rbpf, R=R).call(lib) == rbpf.RBPF_ERR_CHOL_FAILED
    assert b"R must be positive definite" in lib.rbpf_last_error()
    assert lib.rbpf_loc_landmark_weights(*_weights_args(rbpf, R=_dp(R))) == rbpf.RBPF_ERR_CHOL_FAILED


@pytest.mark.parametrize("field", ["lazy_depth", "n_devices", "inplace", "storage", "fix_p_mean", "chol_refresh"])
def test_foreign_options_are_unsupported(rbpf, field):
    a = _Args(rbpf)
    setattr(a.opt, field, 2)
    assert a.call(rbpf.load_library()) == rbpf.RBPF_ERR_UNSUPPORTED


def test_constructor_validation_and_the_two_cross_refusals(rbpf):
    n = 6
    hs, hd = rbpf.DeviceSparseHandles(_never, _never), rbpf.DeviceHandles(_never, _never)
    mp = rbpf.DeviceLandmarkMap(hs, np.zeros(n), np.eye(n), np.eye(4))
    assert mp.nLin == n and mp.ny == 4 and mp.transition is None
    assert rbpf.DeviceLandmarkMap(rbpf.DeviceSparseSmootherHandles(_never, _never), np.zeros(n), np.eye(n), 0.5).ny == 1
    with pytest.raises(TypeError):
        rbpf.DeviceLandmarkMap(object(), np.zeros(n), np.eye(n), np.eye(4))
    with pytest.raises(TypeError):
        rbpf.DeviceLandmarkMap(hs, np.zeros(n), np.eye(n), np.eye(4), transition=object())
    with pytest.raises(ValueError):
        rbpf.DeviceLandmarkMap(hs, np.zeros(n), np.eye(n + 1), np.eye(4))
    with pytest.raises(ValueError):
        rbpf.DeviceLandmarkMap(hs, np.zeros(n), np.eye(n), np.zeros((4, 3)))
    with pytest.raises(rbpf.RBPFError) as ei:
        rbpf.DeviceLandmarkMap(hd, np.zeros(n), np.eye(n), np.eye(4))
    assert ei.value.status == rbpf.RBPF_ERR_UNSUPPORTED and "DeviceMap" in str(ei.value).replace("DeviceLandmarkMap", "")
    with pytest.raises(rbpf.RBPFError) as ei:
        rbpf.DeviceMap(hs, np.zeros(n), np.eye(n), np.eye(4))
    assert ei.value.status == rbpf.RBPF_ERR_UNSUPPORTED and "DeviceLandmarkMap" in str(ei.value)


def test_from_posterior_factors_p_and_refuses_an_indefinite_one(rbpf):
    rs = np.random.RandomState(0)
    n = 23
    B = rs.standard_normal((n, n))
    P = B @ B.T / n + 0.1 * np.eye(n)
    hs = rbpf.DeviceSparseHandles(_never, _never)
    mp = rbpf.DeviceLandmarkMap.from_posterior(hs, rs.standard_normal(n), P, gc.full_R(3, 1))
    assert isinstance(mp, rbpf.DeviceLandmarkMap)
    assert np.array_equal(mp.V, np.tril(mp.V)) and mp.nLin == n and mp.ny == 3
    assert np.max(np.abs(mp.V.T @ mp.V - P)) <= 1e-12 * np.max(np.abs(P))
    dense = rbpf.DeviceMap.from_posterior(rbpf.DeviceHandles(_never, _never), np.zeros(n), P, np.eye(3))
    np.testing.assert_array_equal(dense.V, mp.V)                          # one factorisation, shared
    P[0, 0] = -1.0
    with pytest.raises(ValueError):
        rbpf.DeviceLandmarkMap.from_posterior(hs, np.zeros(n), P, np.eye(3))


def _small_map(rbpf, transition=None):
    p = lm.case("rb", 2, 4, 3, 1)
    return p, rbpf.DeviceLandmarkMap(rbpf.DeviceSparseHandles(_never, _never), p["mean"], p["V"], p["R"], transition=transition)


def test_without_a_device_every_entry_point_says_no_device(rbpf):
    lib = rbpf.load_library()
    if rbpf.device_count() > 0:                                           # with one, the same calls are served
        assert _Args(rbpf).call(lib) == rbpf.RBPF_OK
        assert lib.rbpf_loc_landmark_weights(*_weights_args(rbpf)) == rbpf.RBPF_OK
        return
    p, mp = _small_map(rbpf)
    with pytest.raises(rbpf.RBPFError) as ei:
        rbpf.particleFilterLocalization(mp, None, p["odometry"], p["y"], p["x0_nonLin"], p["Q"], p["R"], p["N_P"], p["dt"])
    assert ei.value.status == rbpf.RBPF_ERR_NO_DEVICE
    assert _Args(rbpf).call(lib) == rbpf.RBPF_ERR_NO_DEVICE
    assert lib.rbpf_loc_landmark_weights(*_weights_args(rbpf)) == rbpf.RBPF_ERR_NO_DEVICE
    with pytest.raises(rbpf.RBPFError) as ei:
        rbpf.landmark_map_weights(np.zeros((4, 2)), np.zeros((4, 2, 5)), np.eye(5), np.eye(2), np.zeros(2))
    assert ei.value.status == rbpf.RBPF_ERR_NO_DEVICE
    with pytest.raises(rbpf.RBPFError) as ei:
        mp.predict(np.zeros((3, 2)))
    assert ei.value.status == rbpf.RBPF_ERR_NO_DEVICE


def test_smoothing_in_a_landmark_map_without_a_transition_is_refused_with_the_reason(rbpf):
    p, mp = _small_map(rbpf)
    with pytest.raises(rbpf.RBPFError) as ei:
        rbpf.particleSmootherLocalization(mp, None, p["odometry"], p["y"], p["x0_nonLin"], p["Q"], p["R"], p["N_P"], 4, p["dt"])
    assert ei.value.status == rbpf.RBPF_ERR_UNSUPPORTED and "transition density" in str(ei.value)
    with pytest.raises(rbpf.RBPFError) as ei:                             # a mixed pair
        rbpf.particleFilterLocalization(mp, _never, p["odometry"], p["y"], p["x0_nonLin"], p["Q"], p["R"], p["N_P"], p["dt"])
    assert ei.value.status == rbpf.RBPF_ERR_INVALID_ARG


def test_the_restatement_equals_the_dense_formula_on_the_observed_rows():
    """weights() against H(ind,:) P H(ind,:)' + R(ind,ind) formed directly and numpy's own Cholesky, with NaN in the rows left out."""
    rs = np.random.RandomState(2)
    N, d, n = 7, 5, 11
    H, V, yhat, y = rs.standard_normal((N, d, n)), np.tril(rs.standard_normal((n, n))), rs.standard_normal((N, d)), rs.standard_normal(d)
    R = gc.full_R(d, 2)
    y[[1, 3]] = np.nan
    H[:, [1, 3], :] = np.nan
    yhat[:, [1, 3]] = np.nan
    S, logw = lm.weights(yhat, H, V, R, y)
    ind = [0, 2, 4]
    P = V.T @ V
    for i in range(N):
        Hi = H[i][ind]
        Si = Hi @ P @ Hi.T
        assert np.max(np.abs(S[i] - Si)) < 1e-12 * np.max(np.abs(Si))
        L = np.linalg.cholesky(Si + R[np.ix_(ind, ind)])
        z = np.linalg.solve(L, y[ind] - yhat[i][ind])
        want = -np.sum(np.log(np.diag(L))) - 0.5 * z @ z - 0.5 * 3 * np.log(2 * np.pi)
        assert abs(logw[i] - want) < 1e-11 * abs(want)
    S0, logw0 = lm.weights(yhat, H, V, R, np.full(d, np.nan))
    assert S0.shape == (N, 0, 0) and np.array_equal(logw0, np.zeros(N))


@pytest.mark.parametrize("kind,L,pattern", [("rb", 3, None), ("rb", 3, ["last"]), ("rb", 2, ["none"]), ("ro", 4, None)],
                         ids=["range_bearing", "only_the_last_output", "nothing_observed", "range_only"])
def test_step_0_of_the_restatement_equals_the_oracles_sparse_filter_at_the_prior(kind, L, pattern):
    """An independent check of the checker: with x0_lin = mean for every particle and P0_lin = V'V, step 0 of
    rbpf_oracle.particleFilter(..., sparseFeatures=True) weighs the particles as the frozen-map recursion does.  (The initial
    states are spread first, or every particle would carry the same weight.)"""
    N = 12
    p = lm.case(kind, L, N, 2, seed=1, pattern=pattern)
    model, V = p["model"], p["V"]
    ref = O.particleFilter(model, p["odometry"], p["y"][:1], p["x0_nonLin"], p["mean"], V.T @ V, p["Q"], p["R"], N, p["dt"], p["rng"],
                           sparseFeatures=True, trace=True)
    xn = np.repeat(np.asarray(p["x0_nonLin"], dtype=np.float64).reshape(3, 1), N, axis=1)
    yhat, H = lm.meas(model, xn, p["mean"])
    _, logw = lm.weights(yhat, H, V, p["R"], p["y"][0])
    want = ref["trace"]["logw"][0]
    print("step-0 log-weights, restatement against the oracle:", float(np.max(np.abs(logw - want))))
    assert np.max(np.abs(logw - want)) <= 1e-9 * max(float(np.max(np.abs(want))), 1e-300)
    # and with particles that differ: the oracle's per-particle weight function on spread states
    xs = xn + 0.05 * np.random.RandomState(3).standard_normal(xn.shape)
    yhat, H = lm.meas(model, xs, p["mean"])
    _, logw = lm.weights(yhat, H, V, p["R"], p["y"][0])
    want = np.array([O._sparse_logw(model, p["y"][0], xs[:, i], p["mean"], V.T @ V, p["R"], 1e-3) for i in range(N)])
    assert np.max(np.abs(logw - want)) <= 1e-9 * max(float(np.max(np.abs(want))), 1e-300)


@pytest.mark.parametrize("i", range(len(lm.FULL_RUNS)), ids=lm.run_id)
def test_float64_and_long_double_draw_the_same_ancestors(i):
    p, ref = lm.full_run(i)
    ld = lm.run(p, dtype=np.longdouble)
    np.testing.assert_array_equal(ref["ai"], ld["ai"])
    np.testing.assert_array_equal(ref["iw_max"], ld["iw_max"])
    np.testing.assert_array_equal(ref["degenerate"], ld["degenerate"])    # (the sum of the weights is small where 32 outputs are seen)
    assert len(np.unique(ref["ai"][1:])) > 1                                # the draws are not trivial
    e_w = float(np.max(np.abs(ref["w"] - ld["w"].astype(np.float64))) / np.max(ref["w"]))
    e_l = float(np.max(np.abs(ref["logw"] - ld["logw"].astype(np.float64))))
    print(f"restatement's own error |fp64 - long double|: weights {e_w:.2e} (relative), log-weights {e_l:.2e}; observed outputs "
          f"{ref['n_obs'].min()} .. {ref['n_obs'].max()}; effective sample size >= {ref['ess'].min():.1f}")
    assert e_w < 1e-10
