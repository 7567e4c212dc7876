"""GPU: the sparseFeatures = true branch (src/particleFilter.m:127-137,165-181) with arbitrary models whose handles are device
code -- rbpf.DeviceSparseHandles, RBPF_MODEL_GENERIC_SPARSE -- against oracle/rbpf_oracle.py:particleFilter(model, ...,
sparseFeatures=True).  The numpy side of every model is in tests/sparse_models.py (the pinhole camera: the oracle's own
SparseVisualModel), its torch twin in tests/sparse_models_torch.py.  The standard of tests/test_gpu_sparse.py applies: resampling
indices exact, everything else 1e-9 relative."""
import functools
import importlib

import numpy as np
import pytest

import cases
import sparse_models as sm
from test_gpu_sparse import RTOL, check_filter, rel

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


def _device():
    torch = _torch()
    return torch.device("cuda", torch.cuda.current_device())


def _twin(c, **kw):
    smt = importlib.import_module("sparse_models_torch")
    return smt.twin_of(c["model"], c, _device(), **kw)


def _args(c):
    return (c["odometry"], c["y"], c["x0_nonLin"], c["x0_lin"], c["P0_lin"], c["Q"], c["R"], c["N_P"], c["dt"])


def run(rbpf, c, twin=None, **kw):
    tw = twin if twin is not None else _twin(c)
    return rbpf.particleFilter(rbpf.DeviceSparseHandles(tw.dynModel, tw.measModel), None, *_args(c), True,
                               rng=cases.device_rng(rbpf, c), extras=True, **kw)


@functools.lru_cache(maxsize=None)
def case(name):
    """(problem, oracle result), computed once and shared."""
    kind, *a = name.split(":")
    a = [int(v) for v in a]
    if kind == "pinhole":
        c = cases.sparse_case(a[0], a[1], a[2], seed=5)
    elif kind == "rb":
        c = sm.range_bearing_case(a[0], a[1], a[2], seed=3)
    elif kind == "ro":
        c = sm.range_only_case(a[0], a[1], a[2], seed=4)
    elif kind == "patterns":
        c = sm.range_bearing_case(3, 7, 6, seed=7, pattern=["all", "none", "last", "all"])
    elif kind == "jitter":
        c = sm.range_bearing_case(3, 6, 5, seed=12)
        c = dict(c, P0_lin=c["P0_lin"] * 1e-9, R=-2e-4 * np.eye(6))
    return c, cases.oracle_filter(c)


def check(ref, out, rows=None):
    check_filter(ref, out)
    got, want = out[8]["yhattraj"], ref["yhattraj"]
    assert got.shape == want.shape
    if rows is not None:
        got, want = got[rows], want[rows]
    assert rel(got, want) <= RTOL, "yhattraj"


def assert_same(a, b, skip=()):
    """Two runs of the product, bit for bit: the eight outputs and every extra."""
    for k in range(8):
        np.testing.assert_array_equal(a[k], b[k])
    for key in a[8]:
        if key not in skip:
            np.testing.assert_array_equal(a[8][key], b[8][key], err_msg=key)


# ---- 1. the pinhole twin against the oracle's own model ----------------------------------------------------------------
@pytest.mark.parametrize("N_P,N_T,nLand", [(12, 10, 6), (7, 9, 3), (40, 14, 20)])
def test_pinhole_twin_matches_oracle(rbpf, N_P, N_T, nLand):
    c, ref = case(f"pinhole:{N_P}:{N_T}:{nLand}")
    assert np.asarray(c["x0_lin"]).shape == (2 * nLand, N_P)                   # x0_lin n x N_P
    assert np.all(np.isnan(c["y"][N_T // 2]))
    check(ref, run(rbpf, c))


# ---- 2. range-bearing landmarks ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,N_P,N_T", [(3, 7, 8), (16, 9, 6)])
def test_range_bearing_matches_oracle(rbpf, L, N_P, N_T):
    c, ref = case(f"rb:{L}:{N_P}:{N_T}")
    gone = np.isnan(c["y"]).reshape(N_T, L, 2)
    assert np.any(gone[:, :, 0] & gone[:, :, 1]) and np.any(gone[:, :, 0] ^ gone[:, :, 1])      # whole landmarks / single components
    assert c["model"].ny == 2 * L and c["model"].nLin == 2 * L
    check(ref, run(rbpf, c))


# ---- 3. range-only 3-D beacons at the largest admitted shape ---------------------------------------------------------------
def test_range_only_at_the_largest_shape_matches_oracle(rbpf):
    c, ref = case("ro:32:5:4")
    assert c["model"].ny == 32 and c["model"].nLin == 96 and np.asarray(c["x0_lin"]).ndim == 1   # x0_lin n x 1
    check(ref, run(rbpf, c))


# ---- 4. observation patterns -------------------------------------------------------------------------------------------
def test_observation_patterns_match_oracle(rbpf):
    c, ref = case("patterns")
    seen = ~np.isnan(c["y"])
    assert seen[0].all() and not seen[1].any() and seen[2].tolist() == [False] * 5 + [True] and seen[3].all()
    out = run(rbpf, c)
    check(ref, out)
    w = out[8]["w"][1]                                                        # nothing observed: uniform, exp(-log(N_P)) (:154-156)
    assert np.ptp(w) == 0.0 and abs(w[0] * c["N_P"] - 1.0) <= 4 * np.finfo(float).eps
    np.testing.assert_array_equal(out[8]["logw"][1], np.zeros(c["N_P"]))


def test_a_step_without_observations_carries_the_state_over(rbpf):
    c, _ = case("patterns")
    tw = _twin(c)
    want = ("final_xl", "final_P", "trace_ai")
    with rbpf.FilterSession(rbpf.DeviceSparseHandles(tw.dynModel, tw.measModel), *_args(c), rng=cases.device_rng(rbpf, c),
                            keep_history=True, trace=True) as s:
        s.advance(1)
        before = s.finish(want)
        s.advance(1)                                                          # y[1] is all NaN
        after = s.finish(want)
    ai = after["trace_ai"][:, 1]
    np.testing.assert_array_equal(after["final_xl"], before["final_xl"][:, ai])
    np.testing.assert_array_equal(after["final_P"], before["final_P"][:, :, ai])


def test_unobserved_rows_are_never_read(rbpf):
    """A twin that writes NaN into every unobserved row of yhat and dy gives the results of the twin that computes them."""
    c, ref = case("patterns")
    base = run(rbpf, c)
    nans = run(rbpf, c, twin=_twin(c, nan_unobserved=True))
    assert_same(base, nans, skip=("yhattraj",))
    seen = ~np.isnan(c["y"]).T                                                # [n_y x N_T]
    np.testing.assert_array_equal(nans[8]["yhattraj"][seen], base[8]["yhattraj"][seen])
    assert np.all(np.isnan(nans[8]["yhattraj"][~seen]))
    assert rel(nans[8]["yhattraj"][seen], ref["yhattraj"][seen]) <= RTOL


# ---- 5. layouts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dy_mode,yhat_mode", [("matlab", "c"), ("slice", "c"), ("c", "t"), ("matlab", "t"), ("slice", "t")])
def test_layouts_are_bit_identical(rbpf, dy_mode, yhat_mode):
    c, ref = case("rb:3:7:8")
    tw = _twin(c, dy_mode=dy_mode, yhat_mode=yhat_mode)
    torch = _torch()
    xl = torch.zeros(c["N_P"], 6, dtype=torch.float64, device=_device()) + 5.0
    yhat, dy = tw.measModel(torch.zeros(3, c["N_P"], dtype=torch.float64, device=_device()), xl)
    tw.reset()
    N, d = c["N_P"], 6
    assert dy.stride() == {"c": (d * d, d, 1), "matlab": (1, N, N * d), "slice": (d * (d + 3), d + 3, 1)}[dy_mode]   # (nLin = n_y here)
    assert yhat.stride() == ((1, N) if yhat_mode == "t" else (d, 1))
    out = run(rbpf, c, twin=tw)
    assert_same(out, run(rbpf, c))
    check(ref, out)


# ---- 6. sessions -----------------------------------------------------------------------------------------------------------
def test_session_windows_equal_one_call(rbpf):
    c, ref = case("rb:3:7:8")
    one = run(rbpf, c)
    tw = _twin(c)
    want = ("traj_max", "traj_mean", "xl_max", "xl_mean", "P_max", "P_mean", "traj_sample_iwmax", "xn_traj", "trace_logw", "trace_w",
            "trace_ai", "final_xn", "final_xl", "final_P", "yhattraj")
    with rbpf.FilterSession(rbpf.DeviceSparseHandles(tw.dynModel, tw.measModel), *_args(c), rng=cases.device_rng(rbpf, c),
                            keep_history=True, trace=True) as s:
        for w in (1, 3, 8 - 4):
            s.advance(w)
        assert s.tell() == 8
        b = s.finish(want)
    for k, key in enumerate(want[:8]):
        np.testing.assert_array_equal(b[key], one[k], err_msg=key)
    ex = one[8]
    np.testing.assert_array_equal(b["trace_logw"].T, ex["logw"])
    np.testing.assert_array_equal(b["trace_w"].T, ex["w"])
    np.testing.assert_array_equal(b["trace_ai"].T, ex["ai"])
    for key, name in (("final_xn", "xn"), ("final_xl", "xl"), ("final_P", "P"), ("yhattraj", "yhattraj")):
        np.testing.assert_array_equal(b[key], ex[name], err_msg=key)
    assert int(b["iw_max"][0]) == ex["iw_max"] == ref["iw_max"]


# ---- 7. jitter retry: the construction of tests/test_gpu_edge_cases.py carries over ----------------------------------------
def test_jitter_retry_path_matches_oracle(rbpf):
    """S = dy P dy' + R not positive definite on the first try -> chol(S + 1e-3 I) (particleFilter.m:145-148); the downdate still
    uses the un-jittered S (:198).  Tolerances of the dense test."""
    c, ref = case("jitter")
    ex = run(rbpf, c)[8]
    np.testing.assert_array_equal(ex["ai"][1:], ref["trace"]["ai"][1:])
    assert rel(ex["w"], ref["trace"]["w"]) <= RTOL
    assert rel(ex["P"], ref["trace"]["P"]) <= 1e-8
    assert rel(ex["xl"], ref["trace"]["xl"]) <= 1e-8


def test_second_cholesky_failure_is_an_error(rbpf):
    c, _ = case("rb:3:7:8")
    c = dict(c, P0_lin=c["P0_lin"] * 1e-9, R=-1.0 * np.eye(6))
    with pytest.raises(rbpf.RBPFError) as ei:
        run(rbpf, c)
    assert ei.value.status == rbpf.RBPF_ERR_CHOL_FAILED


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------
def _dummy(n, d, N=4, T=3):
    """A problem of the given sizes whose handles must never be called."""
    return (np.zeros((T - 1, 3)), np.zeros((T, d)), np.zeros(3), np.zeros(n), np.eye(n), 0.01 * np.eye(3), np.eye(d), N, 1.0)


def _never(*a):
    raise AssertionError("a refused run called a handle")


def _raises_at_second_call(tw):
    def meas(xn, xl):
        if tw.meas_calls == 1:
            raise RuntimeError("boom in measModel")
        return tw.measModel(xn, xl)
    return meas


def _wrong_shape(tw):
    return lambda xn, xl: tuple(v[:-1] for v in tw.measModel(xn, xl))


def _float32(tw):
    return lambda xn, xl: tuple(v.float() for v in tw.measModel(xn, xl))


REFUSALS = {
    # name: (arguments or None = the valid problem, keywords, expected exception, status, words of the message)
    "n_y=33": (_dummy(66, 33), {}, "RBPF_ERR_UNSUPPORTED", "n_y must be 1 .. 32"),
    "nLin=97": (_dummy(97, 4), {}, "RBPF_ERR_UNSUPPORTED", "nLin must be 1 .. 96"),
    "fp32": (None, dict(storage="fp32"), "RBPF_ERR_UNSUPPORTED", "storage"),
    "lazy_depth=2": (None, dict(lazy_depth=2), "RBPF_ERR_UNSUPPORTED", "lazy_depth"),
    "inplace=1": (None, dict(inplace=1), "RBPF_ERR_UNSUPPORTED", "inplace"),
    "n_devices=2": (None, dict(n_devices=2), "RBPF_ERR_UNSUPPORTED", "n_devices"),
    "sparseFeatures=False": (None, dict(sparse=False), "RBPF_ERR_INVALID_ARG", "sparseFeatures"),
}


@pytest.mark.parametrize("name", list(REFUSALS) + ["particleSmoother", "particleSmootherInformationForm", "raises", "wrong shape",
                                                   "float32"])
def test_refusals_leave_nothing_behind(rbpf, name):
    c, ref = case("rb:3:7:8")
    lib = rbpf.load_library()
    good = run(rbpf, c)
    _torch().cuda.synchronize()
    base = int(lib.rbpf_device_bytes_live())
    tw = _twin(c)
    if name in REFUSALS:
        args, kw, status, words = REFUSALS[name]
        kw = dict(kw)
        sparse = kw.pop("sparse", True)
        handles = rbpf.DeviceSparseHandles(_never, _never) if args is not None else rbpf.DeviceSparseHandles(tw.dynModel, tw.measModel)
        with pytest.raises(rbpf.RBPFError) as ei:
            rbpf.particleFilter(handles, None, *(args or _args(c)), sparse, rng=rbpf.PhiloxRNG(1) if args is not None else cases.device_rng(rbpf, c), **kw)
        assert ei.value.status == getattr(rbpf, status) and words in str(ei.value), str(ei.value)
        assert tw.dyn_calls == 0 and tw.meas_calls == 0
    elif name.startswith("particleSmoother"):
        handles = rbpf.DeviceSparseHandles(tw.dynModel, tw.measModel)
        with pytest.raises(rbpf.RBPFError) as ei:
            getattr(rbpf, name)(handles, None, None, *_args(c)[:8], 2, c["dt"], True, rng=cases.device_rng(rbpf, c))
        assert ei.value.status == rbpf.RBPF_ERR_UNSUPPORTED and "smoother" in str(ei.value)
        assert tw.meas_calls == 0
    else:
        meas, exc, words = {"raises": (_raises_at_second_call(tw), RuntimeError, "boom in measModel"),
                            "wrong shape": (_wrong_shape(tw), ValueError, "expected a float64 device tensor of shape"),
                            "float32": (_float32(tw), ValueError, "torch.float32")}[name]
        with pytest.raises(exc, match=words):
            rbpf.particleFilter(rbpf.DeviceSparseHandles(tw.dynModel, meas), None, *_args(c), True, rng=cases.device_rng(rbpf, c))
    _torch().cuda.synchronize()
    assert int(lib.rbpf_device_bytes_live()) == base
    assert_same(run(rbpf, c), good)                                           # a valid run afterwards
    assert int(lib.rbpf_device_bytes_live()) == base


def test_plain_device_handles_stay_refused_with_sparse_features(rbpf):
    c, _ = case("rb:3:7:8")
    tw = _twin(c)
    with pytest.raises(rbpf.RBPFError, match="sparse-visual family only") as ei:
        rbpf.particleFilter(rbpf.DeviceHandles(tw.dynModel, tw.measModel), None, *_args(c), True, rng=cases.device_rng(rbpf, c))
    assert ei.value.status == rbpf.RBPF_ERR_UNSUPPORTED
