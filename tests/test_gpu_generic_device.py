"""GPU: the generic family with handles on the device (rbpf_filter_ancestors_device / rbpf_filter_step_device /
rbpf_filter_set_device_callbacks, rbpf.DeviceHandles).

* Device path == host-callback path, bit for bit.  Both evaluate the handles with the same torch computation on the device
  (tests/generic_model_torch.py); the host path copies its results to the host and lets the library transpose and upload
  them, the device path leaves them where they are and lets the kernels of rbpf_external.hip re-lay them.  The library sees
  identical bits either way, so every output is compared with assert_array_equal -- at every dy layout (0 MATLAB order,
  1 native, 2 C-contiguous) and with both drivers (device callbacks under rbpf_filter_advance, and the caller-driven pair).
  The shapes put N_P and nLin on and off the 64 x 64 tiles of the pack kernel: nLin = 1, 2, 64, 129, 256, 383, 639 and
  N_P = 1, 8, 10, 70.  The test never synchronises between two steps.
* Oracle parity of rbpf.particleFilter(DeviceHandles(...)) against oracle/rbpf_oracle.py, with the project's tolerances
  (indices exact, values 1e-9: tests/test_gpu_filter.check_filter); torch's cos differs from numpy's by rounding only.
* Session windows, makePlots, the refusals, and the library's books of device memory."""
import ctypes as C
import importlib

import numpy as np
import pytest

import cases
import test_gpu_filter as tf
import test_gpu_generic_shapes as gs

pytestmark = pytest.mark.gpu

OUTPUTS = ("trace_ai", "trace_w", "trace_logw", "final_xl", "final_P", "traj_max", "traj_mean", "xl_max", "P_max")

# (n_nonlin, n_w, n_odo, n_y, nLin), N_P, N_T, FilterSession options
CONFIGS = {
    "scalar": ((1, 1, 1, 1, 1), 8, 8, {}),
    "wide_h": ((2, 2, 2, 3, 2), 8, 8, {}),
    "two_tile_edges": ((5, 2, 4, 1, 129), 70, 8, {}),
    "two_tile_edges_lazy3": ((5, 2, 4, 1, 129), 70, 8, dict(lazy_depth=3)),
    "sym256_lazy4": ((4, 3, 4, 3, 256), 70, 7, dict(storage="fp64sym", lazy_depth=4, inplace=0)),
    "sym256_lazy4_inplace": ((4, 3, 4, 3, 256), 70, 7, dict(storage="fp64sym", lazy_depth=4, inplace=1)),
    "sym383": ((3, 3, 3, 3, 383), 10, 7, dict(storage="fp64sym")),
    "fp32sym639": ((6, 4, 6, 3, 639), 8, 7, dict(storage="fp32sym")),
    "one_particle": ((3, 3, 3, 3, 64), 1, 7, {}),
}

_CASES, _HOST = {}, {}


def _torch():
    import torch
    return torch


def _case(shape, N, T):
    """(numpy model, problem, torch model) of a shape; built once."""
    key = (shape, N, T)
    if key not in _CASES:
        import generic_model_torch as gmt
        torch = _torch()
        m, p = gs.case(shape, N, T)
        tm = gmt.TorchGenericModel(m, p, torch.device("cuda", torch.cuda.current_device()))
        torch.cuda.synchronize()                                          # the constants, before any other stream reads them
        _CASES[key] = (m, p, tm)
    return _CASES[key]


def _session(rbpf, model, p, opts):
    return rbpf.FilterSession(model, p["odometry"], p["y"], p["x0_nonLin"], p["x0_lin"], p["P0_lin"], p["Q"], p["R"], p["N_P"],
                              p["dt"], rng=rbpf.ReplayRNG(p["U"], p["Z"], p["Ufin"]), keep_history=True, trace=True, **opts)


def _plain_model(rbpf, m):
    return rbpf.GenericDenseModel(m.nNonLin, m.nLin, m.ny, m.nw, m.n_odo)      # no handles: rbpf_model.callbacks == NULL


class _Harness:
    """What the callbacks and the caller-driven loop of one run share: the torch model, the problem's constants on the device,
    the library's stream, views of library memory."""

    def __init__(self, rbpf, m, p, tm):
        torch = _torch()
        self.torch, self.m, self.p, self.tm = torch, m, p, tm
        self.view = importlib.import_module(rbpf.__name__ + ".multigpu")._view
        self.dev = tm.device
        self.N, self.T = p["N_P"], p["y"].shape[0]
        self.nN, self.n, self.d = m.nNonLin, m.nLin, m.ny
        f = dict(dtype=torch.float64, device=self.dev)
        self.odo, self.Q, self.dt = torch.as_tensor(p["odometry"], **f), torch.as_tensor(p["Q"], **f), float(p["dt"])
        self.x0 = torch.as_tensor(np.asarray(p["x0_nonLin"], dtype=np.float64), **f).repeat(self.N, 1)
        torch.cuda.synchronize()
        tm.reset()
        self.error = None

    def on_library_stream(self, s):
        self.s, self.lib = s, s.lib
        sp = C.c_void_p()
        assert self.lib.rbpf_stream_get(self.s.ctx, C.byref(sp)) == 0
        ldx = C.c_int32(0)
        assert self.lib.rbpf_filter_external_layout(self.s.ctx, C.byref(ldx)) == 0
        self.ldx = ldx.value
        assert self.ldx >= self.n
        self.stream = self.torch.cuda.ExternalStream(sp.value, device=self.dev)
        return self

    def states(self, ptr):
        return self.view(self.torch, ptr, (self.N, self.nN), self.dev).t()         # [n_nonlin x N] column-major

    def dy_target(self, ptr, layout):
        N, d, n = self.N, self.d, self.n
        if layout == 0:
            return self.view(self.torch, ptr, (n, d, N), self.dev).permute(2, 1, 0)
        if layout == 1:
            return self.view(self.torch, ptr, (N, d, self.ldx), self.dev)[:, :, :n]
        return self.view(self.torch, ptr, (N, d, n), self.dev)

    def dyn(self, t, anc):
        return self.tm.dynModel(anc, self.odo[t], self.dt, self.Q)


def _host_model(rbpf, m, h):
    """The host-callback family with BATCHED host handles: the torch computation of the device path, copied to the host."""
    ffi = importlib.import_module(rbpf.__name__ + "._ffi")
    torch = h.torch

    class Model(rbpf.GenericDenseModel):
        def _make_callbacks(self):
            nN, n, d, N = h.nN, h.n, h.d, h.N

            def dyn(_user, t, n_cols, xn_anc, xn_new):
                try:
                    A = np.ctypeslib.as_array(xn_anc, shape=(n_cols * nN,)).reshape(n_cols, nN)
                    x = h.dyn(t, torch.as_tensor(A.copy(), device=h.dev).t())
                    np.ctypeslib.as_array(xn_new, shape=(n_cols * nN,))[:] = x.t().contiguous().cpu().numpy().ravel()
                    return 0
                except Exception as exc:                                          # noqa: BLE001
                    h.error = h.error or exc
                    return 1

            def meas(_user, n_cols, xn, dy):
                try:
                    X = np.ctypeslib.as_array(xn, shape=(n_cols * nN,)).reshape(n_cols, nN)
                    v = h.tm.measModel(torch.as_tensor(X.copy(), device=h.dev).t()).cpu().numpy()
                    assert v.shape == (N, d, n)
                    np.ctypeslib.as_array(dy, shape=(n_cols * d * n,))[:] = v.ravel(order="F")
                    return 0
                except Exception as exc:                                          # noqa: BLE001
                    h.error = h.error or exc
                    return 1

            cb = ffi.rbpf_callbacks()
            self._fns = (ffi.DYN_MODEL_FN(dyn), ffi.MEAS_MODEL_FN(meas))
            cb.dyn_model, cb.meas_model = self._fns
            cb.user = None
            return cb

    return Model(m.nNonLin, m.nLin, m.ny, m.nw, m.n_odo, dynModel=True, measModel=True)


def _finish(s):
    s.sync()
    return s.finish(want=OUTPUTS)


def host_run(rbpf, name):
    """The host-callback path of a configuration: the reference of the bit-for-bit comparisons.  Computed once, never changed."""
    if name not in _HOST:
        shape, N, T, opts = CONFIGS[name]
        m, p, tm = _case(shape, N, T)
        h = _Harness(rbpf, m, p, tm)
        s = _session(rbpf, _host_model(rbpf, m, h), p, opts)
        try:
            s.advance(T)
            assert h.error is None, h.error
            out = _finish(s)
        finally:
            s.close()
        for v in out.values():
            v.setflags(write=False)
        _HOST[name] = out
    return _HOST[name]


def device_run(rbpf, name, layout, drive, before=None):
    """drive "callbacks": rbpf_filter_set_device_callbacks + rbpf_filter_advance; "pair": rbpf_filter_ancestors_device /
    rbpf_filter_step_device, step by step.  No synchronisation between the steps.  before(h): refusals to provoke first."""
    shape, N, T, opts = CONFIGS[name]
    m, p, tm = _case(shape, N, T)
    torch = _torch()
    ffi = importlib.import_module(rbpf.__name__ + "._ffi")
    s = _session(rbpf, _plain_model(rbpf, m), p, opts)
    try:
        h = _Harness(rbpf, m, p, tm).on_library_stream(s)
        lib = s.lib
        if before is not None:
            before(h)
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
                        assert ai.value and anc.value
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
        return _finish(s)
    finally:
        s.close()


def assert_same(got, want):
    np.testing.assert_array_equal(got["trace_ai"][:, 1:], want["trace_ai"][:, 1:])
    for k in OUTPUTS[1:]:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


# ------------------------------------------------------------------------------------------------
# device path == host path, bit for bit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_device_path_equals_host_path_bit_for_bit(rbpf, name, layout):
    want = host_run(rbpf, name)
    assert np.all(np.isfinite(want["P_max"])) and np.all(np.isfinite(want["trace_w"]))
    for drive in ("callbacks", "pair"):
        assert_same(device_run(rbpf, name, layout, drive), want)


# ------------------------------------------------------------------------------------------------
# the public interface: rbpf.DeviceHandles
# ------------------------------------------------------------------------------------------------
def _filter_args(p):
    return (p["odometry"], p["y"], p["x0_nonLin"], p["x0_lin"], p["P0_lin"], p["Q"], p["R"], p["N_P"], p["dt"])


@pytest.mark.parametrize("name,dy_layout", [("two_tile_edges", None), ("two_tile_edges", 0), ("sym256_lazy4", None), ("sym256_lazy4", 1)])
def test_device_handles_match_the_oracle(rbpf, name, dy_layout):
    """Independent of the host path: particleFilter(DeviceHandles) against the numpy oracle."""
    shape, N, T, opts = CONFIGS[name]
    m, p, tm = _case(shape, N, T)
    tm.reset()
    handles = rbpf.DeviceHandles(tm.dynModel, tm.measModel, dy_layout=dy_layout)
    out = rbpf.particleFilter(handles, None, *_filter_args(p), rng=rbpf.ReplayRNG(p["U"], p["Z"], p["Ufin"]), extras=True, **opts)
    assert tm.calls == T - 1
    tf.check_filter(gs.oracle_run("filter", m, p), out)


@pytest.mark.parametrize("how", ["matlab_strides", "native_out", "odd_strides"])
def test_the_binding_reads_the_layout_off_the_strides(rbpf, how):
    """MATLAB-order strides, the native view filled in place and a tensor of neither kind all give the bits of the host path."""
    name = "two_tile_edges"
    shape, N, T, opts = CONFIGS[name]
    m, p, tm = _case(shape, N, T)
    torch = _torch()
    seen = []
    if how == "matlab_strides":
        def meas(xn):
            dy = tm.measModel(xn).permute(2, 1, 0).contiguous().permute(2, 1, 0)
            seen.append((dy.is_contiguous(), dy.permute(2, 1, 0).is_contiguous(), dy.stride(0), dy.stride(2)))
            return dy
        handles = rbpf.DeviceHandles(tm.dynModel, meas)
    elif how == "native_out":
        def meas(xn, out):
            seen.append(out.stride())
            out.copy_(tm.measModel(xn))
            return out
        handles = rbpf.DeviceHandles(tm.dynModel, meas, native_out=True)
    else:
        def meas(xn):
            wide = torch.zeros((N, m.ny, 2 * m.nLin), dtype=torch.float64, device=xn.device)
            wide[:, :, ::2] = tm.measModel(xn)
            seen.append(wide[:, :, ::2].stride())
            return wide[:, :, ::2]
        handles = rbpf.DeviceHandles(tm.dynModel, meas)
    tm.reset()
    s = _session(rbpf, handles, p, opts)
    try:
        s.advance(T)
        got = _finish(s)
    finally:
        s.close()
    assert len(seen) == T
    if how == "matlab_strides":
        assert seen[0] == (False, True, 1, N * m.ny)                      # (the stride of a dimension of size 1 is arbitrary)
    elif how == "native_out":
        assert seen[0][2] == 1 and seen[0][1] >= m.nLin and seen[0][0] == m.ny * seen[0][1]
    assert_same(got, host_run(rbpf, name))


def test_session_windows(rbpf):
    """advance(3) followed by advance(4) equals advance(7)."""
    shape, N, T, opts = CONFIGS["sym383"]
    m, p, tm = _case(shape, N, T)
    assert T == 7
    outs = []
    for windows in ((3, 4), (7,)):
        tm.reset()
        s = _session(rbpf, rbpf.DeviceHandles(tm.dynModel, tm.measModel), p, opts)
        try:
            for w in windows:
                s.advance(w)
            assert s.tell() == 7
            outs.append(_finish(s))
        finally:
            s.close()
    assert_same(outs[0], outs[1])
    assert_same(outs[0], host_run(rbpf, "sym383"))


def test_make_plots_is_called_once_per_step(rbpf):
    """The reference's nine arguments (particleFilter.m:215-217) after every step, through the on_step hook."""
    shape, N, T, opts = CONFIGS["wide_h"]
    m, p, tm = _case(shape, N, T)
    calls = []

    def makePlots(*a):
        assert len(a) == 9
        xn, xl_max, P_max, traj_max, yhattraj, xn_traj, traj_mean, xl, P = a
        assert xn.shape == (m.nNonLin, N) and xl.shape == (m.nLin, N) and P.shape == (m.nLin, m.nLin, N)
        assert np.all(np.isfinite(xn)) and np.all(np.isfinite(P))
        calls.append(xn.copy())

    for dy_layout in (None, 2):
        calls.clear()
        tm.reset()
        out = rbpf.particleFilter(rbpf.DeviceHandles(tm.dynModel, tm.measModel, dy_layout=dy_layout), None, *_filter_args(p),
                                  rng=rbpf.ReplayRNG(p["U"], p["Z"], p["Ufin"]), makePlots=makePlots, extras=True, **opts)
        assert len(calls) == T
        np.testing.assert_array_equal(calls[-1], out[8]["xn"])


# ------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(rbpf):
    name = "wide_h"
    ffi = importlib.import_module(rbpf.__name__ + "._ffi")
    ok_cb = ffi.rbpf_callbacks()
    keep = (ffi.DYN_MODEL_FN(lambda *a: 0), ffi.MEAS_MODEL_FN(lambda *a: 0))
    ok_cb.dyn_model, ok_cb.meas_model = keep

    def refusals(h):
        lib, ctx = h.lib, h.s.ctx
        ai, anc = C.c_void_p(), C.c_void_p()
        some = C.c_void_p(h.x0.data_ptr())
        assert lib.rbpf_filter_ancestors_device(ctx, C.byref(ai), C.byref(anc)) == rbpf.RBPF_ERR_STATE      # before the first step
        assert lib.rbpf_filter_step_device(ctx, some, some, 7) == rbpf.RBPF_ERR_INVALID_ARG
        assert lib.rbpf_filter_set_device_callbacks(ctx, C.byref(ok_cb), 7) == rbpf.RBPF_ERR_INVALID_ARG
        assert lib.rbpf_filter_step_device(ctx, None, some, 0) == rbpf.RBPF_ERR_INVALID_ARG
        assert h.s.tell() == 0

    want = host_run(rbpf, name)
    for drive in ("pair", "callbacks"):
        assert_same(device_run(rbpf, name, 0, drive, before=refusals), want)

    # a dense-mag context is not of the generic family; afterwards it advances as usual
    c = cases.mag_case(N_P=8, N_T=4, m=16, seed=2)
    mdl, x0, P0, R = cases.device_model(rbpf, c)
    s = rbpf.FilterSession(mdl, c["odometry"], c["y"], c["x0_nonLin"], x0, P0, c["Q"], R, c["N_P"], c["dt"], rng=cases.device_rng(rbpf, c))
    try:
        torch = _torch()
        some = torch.zeros(4096, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        ptr, ldx = C.c_void_p(some.data_ptr()), C.c_int32(0)
        assert s.lib.rbpf_filter_step_device(s.ctx, ptr, ptr, 0) == rbpf.RBPF_ERR_STATE
        assert s.lib.rbpf_filter_external_layout(s.ctx, C.byref(ldx)) == rbpf.RBPF_ERR_STATE
        assert s.lib.rbpf_filter_set_device_callbacks(s.ctx, C.byref(ok_cb), 0) == rbpf.RBPF_ERR_STATE
        s.advance(4)
        s.sync()
        assert np.all(np.isfinite(s.finish()["P_max"]))
    finally:
        s.close()

    # a context created with host callbacks keeps them; afterwards it advances as usual
    shape, N, T, opts = CONFIGS[name]
    m, p, tm = _case(shape, N, T)
    h = _Harness(rbpf, m, p, tm)
    s = _session(rbpf, _host_model(rbpf, m, h), p, opts)
    try:
        assert s.lib.rbpf_filter_set_device_callbacks(s.ctx, C.byref(ok_cb), 0) == rbpf.RBPF_ERR_STATE
        ai, anc = C.c_void_p(), C.c_void_p()
        assert s.lib.rbpf_filter_ancestors_device(s.ctx, C.byref(ai), C.byref(anc)) == rbpf.RBPF_ERR_STATE
        s.advance(T)
        assert h.error is None, h.error
        assert_same(_finish(s), want)
    finally:
        s.close()


@pytest.mark.parametrize("smoother", ["particleSmoother", "particleSmootherInformationForm"])
def test_device_handles_are_refused_by_the_smoothers(rbpf, smoother):
    shape, N, T, opts = CONFIGS["wide_h"]
    m, p, tm = _case(shape, N, T)
    tm.reset()
    handles = rbpf.DeviceHandles(tm.dynModel, tm.measModel)
    with pytest.raises(rbpf.RBPFError) as ei:
        getattr(rbpf, smoother)(handles, None, None, *_filter_args(p)[:8], 2, p["dt"], rng=rbpf.ReplayRNG(p["U"], p["Z"], p["Ufin"]))
    assert ei.value.status == rbpf.RBPF_ERR_UNSUPPORTED and "smoother" in str(ei.value)
    assert tm.calls == 0
    # ... and the filter takes the same object afterwards
    out = rbpf.particleFilter(handles, None, *_filter_args(p), rng=rbpf.ReplayRNG(p["U"], p["Z"], p["Ufin"]))
    assert np.all(np.isfinite(out[4]))


# ------------------------------------------------------------------------------------------------
# device memory
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dy_layout", [None, 0, 1, 2])
def test_every_byte_comes_back(rbpf, dy_layout):
    """rbpf_device_bytes_live() after the session is closed, the staging buffer of layouts 0 / 2 included."""
    shape, N, T, opts = CONFIGS["two_tile_edges"]
    m, p, tm = _case(shape, N, T)
    lib = rbpf.load_library()
    base = int(lib.rbpf_device_bytes_live())
    plain = _session(rbpf, _plain_model(rbpf, m), p, opts)
    try:
        without = int(lib.rbpf_device_bytes_live())
    finally:
        plain.close()
    assert int(lib.rbpf_device_bytes_live()) == base
    tm.reset()
    s = _session(rbpf, rbpf.DeviceHandles(tm.dynModel, tm.measModel, dy_layout=dy_layout), p, opts)
    try:
        s.advance(T)
        s.sync()
        during = int(lib.rbpf_device_bytes_live())
        assert np.all(np.isfinite(s.finish()["P_max"]))
    finally:
        s.close()
    states = 2 * m.nNonLin * N * 8                                       # ancestors' states and new states, column-major
    stage = N * m.ny * m.nLin * 8 if dy_layout in (0, 2) else 0
    if dy_layout is None:
        assert during - without == states // 2                            # the caller-driven pair: the ancestors' states only
    else:
        assert during - without == states + stage
    assert int(lib.rbpf_device_bytes_live()) == base
