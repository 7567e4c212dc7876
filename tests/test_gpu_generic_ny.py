"""GPU: generic device-code models (no host callbacks) at every measurement width from 1 to 8 -- rbpf.DeviceHandles under
both drivers and every dy layout, rbpf.particle_filter_external, rbpf.DeviceSmootherHandles in both smoother forms --
against the numpy oracle (tests/test_oracle_generic_ny_kat.py pins the oracle itself at these widths), against the
extended-precision batch posterior, and the refusals of what these widths do not have.

Every problem carries a full SPD R (tests/generic_ny_cases.py).  Tolerances are the project's standing ones
(tests/test_gpu_filter.check_filter, tests/test_gpu_smoother.check: indices exact, values 1e-9 relative) and
generic_model.kat_tolerance for the known answer."""
import ctypes as C
import importlib

import numpy as np
import pytest

import generic_model as gm
import generic_ny_cases as gc
import test_gpu_filter as tf
import test_gpu_generic_device as gd
import test_gpu_generic_shapes as gs
import test_gpu_smoother as ts

pytestmark = pytest.mark.gpu

_CASES = {}


def _torch():
    import torch
    return torch


def _device():
    torch = _torch()
    return torch.device("cuda", torch.cuda.current_device())


def _case(shape, N, T):
    """(numpy model, problem with a full R, torch model); built once."""
    key = (shape, N, T)
    if key not in _CASES:
        import generic_model_torch as gmt
        m, p = gc.case(shape, N, T)
        tm = gmt.TorchGenericModel(m, p, _device())
        _torch().cuda.synchronize()
        _CASES[key] = (m, p, tm)
    return _CASES[key]


def _filter_args(p):
    return (p["odometry"], p["y"], p["x0_nonLin"], p["x0_lin"], p["P0_lin"], p["Q"], p["R"], p["N_P"], p["dt"])


def _rng(rbpf, p):
    return rbpf.ReplayRNG(p["U"], p["Z"], p["Ufin"])


# ------------------------------------------------------------------------------------------------
# filter parity against the oracle
# ------------------------------------------------------------------------------------------------
# (n_nonlin, n_w, n_odo, n_y, nLin).  (3, 3, 3, 4, 384): three row chunks per wave; its LDS plan is 90 KB and is admitted.
FILTER_SHAPES = [
    (2, 2, 2, 2, 1),          # every linear matrix 1 x 1, H wider than tall
    (3, 3, 3, 2, 64),         # no core chunk, all border rows
    (3, 2, 3, 4, 129),        # one core chunk and one border row
    (4, 3, 4, 5, 200),        # 72 border rows
    (3, 3, 3, 6, 130),
    (2, 2, 2, 7, 64),
    (3, 3, 3, 8, 7),          # nLin < n_y
    (3, 3, 3, 8, 256),        # two core chunks (the blocked variant: the plain plan is above its threshold)
    (3, 3, 3, 4, 384),        # three chunks per wave, CPL = 3
]


@pytest.mark.parametrize("shape", FILTER_SHAPES, ids=lambda s: "ny%d_n%d" % (s[3], s[4]))
def test_device_handles_match_the_oracle_at_any_width(rbpf, shape):
    N, T = 8, 8
    m, p, tm = _case(shape, N, T)
    tm.reset()
    out = rbpf.particleFilter(rbpf.DeviceHandles(tm.dynModel, tm.measModel), None, *_filter_args(p), rng=_rng(rbpf, p), extras=True)
    assert tm.calls == T - 1
    tf.check_filter(gs.oracle_run("filter", m, p), out)


def test_the_caller_driven_host_form_matches_the_oracle_at_n_y_4(rbpf):
    """rbpf.particle_filter_external (rbpf_filter_ancestors / rbpf_filter_step_external): a model without callbacks whose
    handles run on the host, one round trip per step."""
    m, p, _ = _case((3, 2, 3, 4, 129), 8, 8)
    dyn, meas, _, state = gm.handles(m, p)
    traj_max, traj_mean, xl_max, P_max = rbpf.particle_filter_external(dyn, meas, *_filter_args(p), rng=_rng(rbpf, p))
    ref = gs.oracle_run("filter", m, p)
    for got, want in ((traj_max, ref["traj_max"]), (traj_mean, ref["traj_mean"]), (xl_max, ref["xl_max"]), (P_max, ref["P_max"])):
        assert tf.rel(got, want) <= tf.RTOL


# ------------------------------------------------------------------------------------------------
# both drivers, every dy layout, native_out: the library sees the same bits on every route
# ------------------------------------------------------------------------------------------------
def _device_run(rbpf, m, p, tm, layout, drive):
    """tests/test_gpu_generic_device.device_run on a case of this file: device callbacks under rbpf_filter_advance
    ("callbacks") or the pair rbpf_filter_ancestors_device / rbpf_filter_step_device ("pair"), dy handed over in `layout`."""
    torch = _torch()
    ffi = importlib.import_module(rbpf.__name__ + "._ffi")
    T = p["y"].shape[0]
    s = gd._session(rbpf, gd._plain_model(rbpf, m), p, {})
    try:
        h = gd._Harness(rbpf, m, p, tm).on_library_stream(s)
        lib = s.lib
        if drive == "callbacks":
            def dyn(_user, t, n_cols, xn_anc, xn_new):
                try:
                    with torch.cuda.stream(h.stream):
                        h.states(xn_new).copy_(h.dyn(t, h.states(xn_anc)))
                    return 0
                except Exception as exc:                                          # noqa: BLE001
                    h.error = h.error or exc
                    return 1

            def meas(_user, n_cols, xn, dy):
                try:
                    with torch.cuda.stream(h.stream):
                        h.dy_target(dy, layout).copy_(tm.measModel(h.states(xn)))
                    return 0
                except Exception as exc:                                          # noqa: BLE001
                    h.error = h.error or exc
                    return 1

            cb = ffi.rbpf_callbacks()
            fns = (ffi.DYN_MODEL_FN(dyn), ffi.MEAS_MODEL_FN(meas))
            cb.dyn_model, cb.meas_model = fns
            assert lib.rbpf_filter_set_device_callbacks(s.ctx, C.byref(cb), layout) == 0, lib.rbpf_last_error()
            s.advance(T)
            assert h.error is None, h.error
        else:
            keep = []
            for t in range(T):
                with torch.cuda.stream(h.stream):
                    if t == 0:
                        xn_cm = h.x0
                    else:
                        ai, anc = C.c_void_p(), C.c_void_p()
                        assert lib.rbpf_filter_ancestors_device(s.ctx, C.byref(ai), C.byref(anc)) == 0, lib.rbpf_last_error()
                        xn_cm = h.dyn(t - 1, h.states(anc)).t().contiguous()
                    dy = tm.measModel(xn_cm.t())
                    if layout == 0:
                        buf = dy.permute(2, 1, 0).contiguous()
                    elif layout == 1:
                        buf = torch.zeros((h.N, h.d, h.ldx), dtype=torch.float64, device=h.dev)
                        buf[:, :, :h.n].copy_(dy)
                    else:
                        buf = dy.contiguous()
                    keep.append((xn_cm, buf))
                    assert lib.rbpf_filter_step_device(s.ctx, C.c_void_p(xn_cm.data_ptr()), C.c_void_p(buf.data_ptr()), layout) == 0, \
                        lib.rbpf_last_error()
        return gd._finish(s)
    finally:
        s.close()


def _native_run(rbpf, m, p, tm, dy_layout):
    """rbpf.DeviceHandles with native_out: measModel fills the (N, n_y, nLin) view of the buffer the step kernel reads."""
    seen = []

    def meas(xn, out):
        seen.append(out.stride())
        out.copy_(tm.measModel(xn))
        return out

    tm.reset()
    s = gd._session(rbpf, rbpf.DeviceHandles(tm.dynModel, meas, dy_layout=dy_layout, native_out=True), p, {})
    try:
        s.advance(p["y"].shape[0])
        got = gd._finish(s)
    finally:
        s.close()
    for st in seen:
        assert st[2] == 1 and st[1] >= m.nLin and st[1] % 2 == 0 and st[0] == m.ny * st[1]
    return got


@pytest.mark.parametrize("shape,N", [((3, 2, 3, 4, 129), 70), ((3, 3, 3, 8, 256), 10)], ids=["ny4_n129_N70", "ny8_n256_N10"])
def test_both_drivers_and_every_dy_layout_give_the_same_bits(rbpf, shape, N):
    """N_P and nLin on and off the 64 x 64 tiles of the pack kernel, at n_y = 4 and 8."""
    T = 6
    m, p, tm = _case(shape, N, T)
    want = _device_run(rbpf, m, p, tm, 0, "callbacks")
    assert np.all(np.isfinite(want["P_max"])) and np.all(np.isfinite(want["trace_w"]))
    for drive in ("callbacks", "pair"):
        for layout in (0, 1, 2):
            if (drive, layout) != ("callbacks", 0):
                gd.assert_same(_device_run(rbpf, m, p, tm, layout, drive), want)
    gd.assert_same(_native_run(rbpf, m, p, tm, None), want)          # caller-driven, the native view read off the strides
    gd.assert_same(_native_run(rbpf, m, p, tm, 1), want)             # device callbacks, layout 1 filled in place


# ------------------------------------------------------------------------------------------------
# extended-precision known answer (no oracle)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(gc.KAT, key=lambda s: s[3]), ids=lambda s: "ny%d_n%d" % (s[3], s[4]))
def test_device_kalman_recursion_equals_the_long_double_batch_posterior_at_any_width(rbpf, shape):
    """The loop of tests/test_gpu_generic_shapes.py's test of the same name, through DeviceHandles: no process noise, so every
    particle's final xl and P are the batch posterior and its summed log-weights the log marginal likelihood."""
    import generic_model_torch as gmt
    N_P, N_T = 4, gc.KAT[shape]
    m, p, _ = gc.kat_case(shape, N_P, N_T)
    tm = gmt.TorchGenericModel(m, p, _device())
    _torch().cuda.synchronize()
    out = rbpf.particleFilter(rbpf.DeviceHandles(tm.dynModel, tm.measModel), None, *_filter_args(p), rng=_rng(rbpf, p), extras=True)
    xn_traj, ex = out[7], out[8]
    # every particle followed one path; the answer is built, in long double, from the H_t of THAT path (torch's sin on the device
    # and numpy's differ by rounding, which the recursion x' = x + 0.1 sin(x) + A dx carries along: a sanity bound only)
    path = np.ascontiguousarray(xn_traj[:, 0, :])
    np.testing.assert_array_equal(xn_traj, np.repeat(path[:, None, :], N_P, axis=1))
    assert np.max(np.abs(path - gm.path_of(m, p))) <= 1e-9
    ref = gm.batch_posterior(m, p, path)
    logw = np.asarray(ex["logw"])
    logw = logw if logw.shape[0] == N_P else logw.T
    tol = gc.check_kat(ref, p, N_T, lambda i: ex["xl"][:, i], lambda i: ex["P"][:, :, i], lambda i: logw[i], N_P)
    print("kat", shape, "tol %.3g kappa %.4g" % (tol, ref["kappa"]))


# ------------------------------------------------------------------------------------------------
# smoothers
# ------------------------------------------------------------------------------------------------
# (shape, N_P, N_T, additive model with dynResNorm = None, forms)
SMOOTHER_CASES = {
    "ny2_n16_additive": ((3, 3, 3, 2, 16), 8, 6, True, ("cov", "info")),
    "ny4_n129_drn": ((3, 2, 3, 4, 129), 7, 6, False, ("cov", "info")),          # n_w < n_nonlin: needs the dynResNorm handle
    "ny8_n65": ((3, 3, 3, 8, 65), 6, 5, False, ("cov", "info")),
    "ny5_n200_packed": ((4, 3, 4, 5, 200), 6, 5, False, ("info",)),           # nLin >= 176: packed information matrices
    "ny7_n1024": ((3, 3, 3, 7, 1024), 4, 3, False, ()),                       # refused: no factorisation kernel takes Imat (LDS 160.3 KB, 65 row tiles)
    "ny8_n640": ((3, 3, 3, 8, 640), 4, 3, False, ()),                         # refused: the information form's LDS plan is 184 KB
}
SMOOTHER_RUNS = [(name, form) for name in SMOOTHER_CASES for form in SMOOTHER_CASES[name][4]]
_SM = {}


def _smoother_case(name):
    if name not in _SM:
        import generic_model_torch_smoother as gms
        shape, N, T, additive, _ = SMOOTHER_CASES[name]
        m, p = gc.case(shape, N, T, N_K=2, additive=additive)
        tm = gms.TorchSmootherModel(m, p, _device())
        _torch().cuda.synchronize()
        _SM[name] = (m, p, tm, additive)
    return _SM[name]


def _smooth(rbpf, name, form, **kw):
    m, p, tm, additive = _smoother_case(name)
    tm.reset()
    handles = rbpf.DeviceSmootherHandles(tm.dynModel, tm.measModel, None if additive else tm.dynResNorm)
    f = rbpf.particleSmootherInformationForm if form == "info" else rbpf.particleSmoother
    args = (p["odometry"], p["y"], p["x0_nonLin"], p["x0_lin"], p["P0_lin"], p["Q"], p["R"], p["N_P"], p["N_K"], p["dt"])
    return f(handles, None, None, *args, rng=_rng(rbpf, p), extras=True, **kw)


@pytest.mark.parametrize("name,form", SMOOTHER_RUNS)
def test_device_smoother_handles_match_the_oracle_at_any_width(rbpf, name, form):
    m, p, tm, additive = _smoother_case(name)
    lib = rbpf.load_library()
    base = int(lib.rbpf_device_bytes_live())
    out = _smooth(rbpf, name, form)
    ts.check(gs.oracle_run(form, m, p, use_dynResNorm=not additive), out, p["N_K"])
    assert int(lib.rbpf_device_bytes_live()) == base
    # chol_refresh = 0 resolves to 1 for such a model: the same arrays.  The information form only: the covariance form has no
    # carried factors, and rbpf.particleSmoother takes no chol_refresh argument to compare under.
    if form == "info":
        again = _smooth(rbpf, name, form, chol_refresh=1)
        for a, b in zip(out[:3], again[:3]):
            np.testing.assert_array_equal(a, b)
        for k in ("ai", "w", "logw", "paNt", "ak"):
            np.testing.assert_array_equal(out[3][k], again[3][k], err_msg=k)


# ------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------
def _valid_run(rbpf):
    """A small n_y = 4 filter run: the library is usable after a refusal."""
    m, p, tm = _case((3, 2, 3, 4, 16), 4, 3)
    tm.reset()
    out = rbpf.particleFilter(rbpf.DeviceHandles(tm.dynModel, tm.measModel), None, *_filter_args(p), rng=_rng(rbpf, p), extras=True)
    tf.check_filter(gs.oracle_run("filter", m, p), out)


def _refused_filter(rbpf, shape, **kw):
    m, p, tm = _case(shape, 4, 3)
    tm.reset()
    return lambda: rbpf.particleFilter(rbpf.DeviceHandles(tm.dynModel, tm.measModel), None, *_filter_args(p), rng=_rng(rbpf, p), **kw)


REFUSALS = {
    "n_y_9": ("filter", (3, 3, 3, 9, 16), {}, "1 .. 8"),
    "n_y_0": ("filter", (3, 3, 3, 0, 16), {}, "1 .. 8"),
    "lazy_depth_2": ("filter", (3, 2, 3, 4, 129), dict(lazy_depth=2), "lazy_depth"),
    "lazy_depth_4": ("filter", (3, 3, 3, 8, 256), dict(lazy_depth=4), "lazy_depth"),
    "storage_fp32": ("filter", (3, 3, 3, 4, 384), dict(storage="fp32"), "storage"),
    "storage_fp64sym": ("filter", (3, 3, 3, 4, 384), dict(storage="fp64sym"), "storage"),
    "storage_fp32sym": ("filter", (3, 3, 3, 4, 384), dict(storage="fp32sym"), "storage"),
    "inplace": ("filter", (3, 2, 3, 4, 129), dict(inplace=1), "inplace"),
    "lds_plan": ("filter", (3, 3, 3, 8, 1151), {}, "LDS"),
    "chol_refresh_5": ("info", "ny4_n129_drn", dict(chol_refresh=5), "chol_refresh"),
    "info_rebuild": ("info", "ny4_n129_drn", dict(info_rebuild=1), "info_rebuild"),
    "lds_plan_information_form": ("info", "ny8_n640", {}, "LDS"),
    "no_factorisation_kernel_information_form": ("info", "ny7_n1024", {}, "factorisation"),
    "no_factorisation_kernel_covariance_form": ("cov", "ny7_n1024", {}, "factorisation"),
}


@pytest.mark.parametrize("which", sorted(REFUSALS))
def test_what_the_new_widths_do_not_have_is_refused(rbpf, which):
    """RBPF_ERR_UNSUPPORTED with a message that names the rule, no device memory left behind, and a valid n_y = 4 run in the
    same process afterwards."""
    kind, what, kw, word = REFUSALS[which]
    lib = rbpf.load_library()
    _valid_run(rbpf)                                                       # (builds and caches what the run after the refusal needs)
    base = int(lib.rbpf_device_bytes_live())
    if kind == "filter":
        call = _refused_filter(rbpf, what, **kw)
    else:
        call = lambda: _smooth(rbpf, what, kind, **kw)                     # noqa: E731
    msg = gs._refused(rbpf, call)
    assert word in msg, msg
    assert int(lib.rbpf_device_bytes_live()) == base
    _valid_run(rbpf)
    assert int(lib.rbpf_device_bytes_live()) == base


def test_host_closures_at_n_y_2_are_still_refused(rbpf):
    """The host-callback route (rbpf_model.callbacks) keeps n_y in {1, 3}."""
    m, p = gc.case((3, 3, 3, 2, 16), 4, 3)
    msg = gs._refused(rbpf, lambda: gs.device_filter(rbpf, m, p))
    assert "1 or 3" in msg, msg
    _valid_run(rbpf)
