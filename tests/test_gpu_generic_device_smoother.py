"""GPU: both smoothers on a generic model whose handles are device code (rbpf.DeviceSmootherHandles,
rbpf_particle_smoother_device).

* Device path == host-callback path, bit for bit.  Both evaluate the handles with the same torch computation on the device
  (tests/generic_model_torch_smoother.py); the host path copies results to the host and lets the library transpose and upload
  them, the device path leaves them where they are.  The library sees identical bits, so every output and every trace is
  compared with assert_array_equal, at every dy layout.
* Oracle parity (oracle/rbpf_oracle.py) with the project's tolerances (tests/test_gpu_smoother.check: indices exact, values
  1e-9 relative), from scratch and with the information matrices rebuilt through the device measModel at the refreshes of the
  carried factors (windows, the rebuild from the origin, the refresh-free mode, one covariance bank).
* The call contract, errors, refusals and the library's books of device memory."""
import importlib

import numpy as np
import pytest

import test_gpu_generic_shapes as gs
import test_gpu_smoother as ts

pytestmark = pytest.mark.gpu

TRACES = ("ai", "w", "logw", "paNt", "ak")

# (n_nonlin, n_w, n_odo, n_y, nLin), N_P, N_T, N_K, additive model with dynResNorm = None, options of the information form
CASES = {
    "scalar": ((1, 1, 1, 1, 1), 8, 8, 3, True, {}),                       # every matrix 1 x 1, the additive default on the device
    "n_w_below_n_nonlin": ((2, 1, 3, 1, 5), 7, 6, 3, False, {}),            # needs a dynResNorm handle
    "pack_tile_tails": ((3, 3, 3, 3, 130), 9, 7, 2, False, {}),             # tails of the 64-wide pack tiles both ways, N_T != N_P
    "n_t_equals_n_p": ((2, 1, 3, 1, 5), 8, 8, 2, False, {}),                # the reference call and the step call: same n_cols
    "cov65": ((3, 3, 3, 3, 65), 6, 5, 2, False, {}),
    "block_lower259": ((3, 3, 3, 3, 259), 6, 5, 2, False, dict(storage="fp64sym", lazy_depth=2)),
}
BOTH_FORMS = ("scalar", "n_w_below_n_nonlin", "pack_tile_tails", "n_t_equals_n_p")
RUNS = [(name, form) for name in BOTH_FORMS for form in ("cov", "info")] + [("cov65", "cov"), ("block_lower259", "info")]

_CASES, _HOST = {}, {}


def _torch():
    import torch
    return torch


def _case(name, N_T=None):
    """(numpy model, problem, torch model) of a case; built once."""
    key = (name, N_T)
    if key not in _CASES:
        import generic_model_torch_smoother as gms
        torch = _torch()
        shape, N, T, N_K, additive, _ = CASES[name]
        m, p = gs.case(shape, N, N_T or T, N_K=N_K, additive=additive)
        tm = gms.TorchSmootherModel(m, p, torch.device("cuda", torch.cuda.current_device()))
        torch.cuda.synchronize()                                          # the constants, before any other stream reads them
        _CASES[key] = (m, p, tm, additive)
    return _CASES[key]


def _args(p):
    return (p["odometry"], p["y"], p["x0_nonLin"], p["x0_lin"], p["P0_lin"], p["Q"], p["R"], p["N_P"], p["N_K"], p["dt"])


def _run(rbpf, form, first, p, **kw):
    f = rbpf.particleSmootherInformationForm if form == "info" else rbpf.particleSmoother
    return f(first, None, None, *_args(p), rng=rbpf.ReplayRNG(p["U"], p["Z"], p["Ufin"]), extras=True, **kw)


def _handles(rbpf, tm, additive, dy_layout=0, **kw):
    tm.reset()
    return rbpf.DeviceSmootherHandles(tm.dynModel, tm.measModel, None if additive else tm.dynResNorm, dy_layout=dy_layout, **kw)


def _options(name, form, **kw):
    return dict(CASES[name][5], chol_refresh=1, **kw) if form == "info" else {}


def _host_model(rbpf, m, p, tm, additive):
    """The host-callback family with BATCHED host handles: the torch computation of the device path, copied to the host."""
    ffi = importlib.import_module(rbpf.__name__ + "._ffi")
    torch = _torch()
    dev = tm.device
    f = dict(dtype=torch.float64, device=dev)
    odo, Q, dt = torch.as_tensor(p["odometry"], **f), torch.as_tensor(p["Q"], **f), float(p["dt"])
    torch.cuda.synchronize()

    class Model(rbpf.GenericDenseModel):
        def _make_callbacks(self):
            nN, n, d, nw = m.nNonLin, m.nLin, m.ny, m.nw

            def guarded(fn):
                def call(*a):
                    try:
                        fn(*a)
                        return 0
                    except Exception as exc:                                      # noqa: BLE001
                        self.error = self.error or exc
                        return 1
                return call

            def on_device(ptr, n_cols):
                return torch.as_tensor(np.ctypeslib.as_array(ptr, shape=(n_cols * nN,)).reshape(n_cols, nN).copy(), device=dev).t()

            def dyn(_user, t, n_cols, xn_anc, xn_new):
                x = tm.dynModel(on_device(xn_anc, n_cols), odo[t], dt, Q)
                np.ctypeslib.as_array(xn_new, shape=(n_cols * nN,))[:] = x.t().contiguous().cpu().numpy().ravel()

            def meas(_user, n_cols, xn, dy):
                v = tm.measModel(on_device(xn, n_cols)).cpu().numpy()
                assert v.shape == (n_cols, d, n)
                np.ctypeslib.as_array(dy, shape=(n_cols * d * n,))[:] = v.ravel(order="F")

            def drn(_user, t, n_cols, xnk_t, xn, e_dyn):
                xk = torch.as_tensor(np.ctypeslib.as_array(xnk_t, shape=(nN,)).copy(), device=dev)
                e = tm.dynResNorm(xk, on_device(xn, n_cols), odo[t], dt, Q)
                np.ctypeslib.as_array(e_dyn, shape=(n_cols * nw,))[:] = e.t().contiguous().cpu().numpy().ravel()

            cb = ffi.rbpf_callbacks()
            self._fns = (ffi.DYN_MODEL_FN(guarded(dyn)), ffi.MEAS_MODEL_FN(guarded(meas)),
                         ffi.DYN_RES_NORM_FN() if additive else ffi.DYN_RES_NORM_FN(guarded(drn)))
            cb.dyn_model, cb.meas_model, cb.dyn_res_norm = self._fns
            cb.user = None
            return cb

    return Model(m.nNonLin, m.nLin, m.ny, m.nw, m.n_odo, dynModel=True, measModel=True)


def host_run(rbpf, name, form):
    """The host-callback path of a run: the reference of the bit-for-bit comparisons.  Computed once, never changed.
    The smoothers build their GenericDenseModel themselves from the callables they are given, so the model with the batched
    callbacks is put in through the factory they call (host._generic_model) for the length of this one call."""
    if (name, form) not in _HOST:
        host = importlib.import_module(rbpf.__name__ + ".host")
        m, p, tm, additive = _case(name)
        tm.reset()
        model = _host_model(rbpf, m, p, tm, additive)
        unrecognised = lambda *a: None                                    # noqa: E731  (never called: the model's callbacks are)
        f = rbpf.particleSmootherInformationForm if form == "info" else rbpf.particleSmoother
        factory = host._generic_model
        host._generic_model = lambda *a: model
        try:
            out = f(unrecognised, unrecognised, None if additive else unrecognised, *_args(p),
                    rng=rbpf.ReplayRNG(p["U"], p["Z"], p["Ufin"]), extras=True, **_options(name, form))
        finally:
            host._generic_model = factory
        assert model.error is None, model.error
        for v in out[:3] + tuple(out[3].values()):
            v.setflags(write=False)
        _HOST[(name, form)] = out
    return _HOST[(name, form)]


def assert_same(got, want):
    for a, b, k in zip(got[:3], want[:3], ("XNK", "XLK", "PK")):
        np.testing.assert_array_equal(a, b, err_msg=k)
    for k in TRACES:
        np.testing.assert_array_equal(got[3][k], want[3][k], err_msg=k)


# ------------------------------------------------------------------------------------------------
# device path == host path, bit for bit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("name,form", RUNS)
def test_device_path_equals_host_path_bit_for_bit(rbpf, name, form, layout):
    want = host_run(rbpf, name, form)
    assert np.all(np.isfinite(want[2])) and np.all(np.isfinite(want[3]["w"]))
    m, p, tm, additive = _case(name)
    lib = rbpf.load_library()
    base = int(lib.rbpf_device_bytes_live())
    got = _run(rbpf, form, _handles(rbpf, tm, additive, dy_layout=layout), p, **_options(name, form))
    assert_same(got, want)
    assert int(lib.rbpf_device_bytes_live()) == base


def test_native_out_is_handed_the_row_stride_in_every_call(rbpf):
    """dy_layout = 1 with native_out: the per-step call, the call along the reference trajectory and the compaction copy."""
    name, form = "pack_tile_tails", "info"
    m, p, tm, additive = _case(name)
    seen = []

    def meas(xn, out):
        seen.append((tuple(out.shape), out.stride()))
        out.copy_(tm.measModel(xn))
        return out

    tm.reset()
    handles = rbpf.DeviceSmootherHandles(tm.dynModel, meas, tm.dynResNorm, dy_layout=1, native_out=True)
    got = _run(rbpf, form, handles, p, **_options(name, form))
    assert_same(got, host_run(rbpf, name, form))
    N, T = p["N_P"], p["y"].shape[0]
    assert {s[0][0] for s in seen} == {N, T}
    for shape, stride in seen:
        assert stride[2] == 1 and stride[1] >= m.nLin and stride[1] % 2 == 0 and stride[0] == m.ny * stride[1]


# ------------------------------------------------------------------------------------------------
# against the numpy oracle
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["cov", "info"])
@pytest.mark.parametrize("name", ["pack_tile_tails", "n_w_below_n_nonlin"])
def test_device_handles_match_the_oracle(rbpf, name, form):
    m, p, tm, additive = _case(name)
    out = _run(rbpf, form, _handles(rbpf, tm, additive), p, **_options(name, form))
    ts.check(gs.oracle_run(form, m, p), out, p["N_K"])


REBUILT = {
    "window2": dict(chol_refresh=2),
    "window3": dict(chol_refresh=3),                                       # 7 steps: windows of 3, 3 and 1 generations
    "refresh_free": dict(chol_refresh=1000),
    "from_the_origin": dict(chol_refresh=3, info_rebuild=1),
}


@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("mode", sorted(REBUILT))
def test_information_matrices_rebuilt_through_the_device_meas_model(rbpf, mode, layout):
    """(3, 3, 3, 3, 130), N_P = 9, N_T = 8: carried factors whose refreshes rebuild the information matrices from the state
    history by calling measModel on it -- modes a host-callback model is refused or has no equivalent of."""
    m, p, tm, additive = _case("pack_tile_tails", N_T=8)
    lib = rbpf.load_library()
    base = int(lib.rbpf_device_bytes_live())
    out = _run(rbpf, "info", _handles(rbpf, tm, additive, dy_layout=layout), p, **REBUILT[mode])
    N, T, K = p["N_P"], 8, p["N_K"]
    assert tm.count("meas") > K * T + (K - 1), "no refresh called measModel"
    ts.check(gs.oracle_run("info", m, p), out, K)
    assert int(lib.rbpf_device_bytes_live()) == base


def _peak_bytes_run(rbpf, name, **kw):
    """A run whose measModel reads rbpf_device_bytes_live() at every call (every buffer of the run is allocated by then)."""
    m, p, tm, additive = _case(name)
    lib = rbpf.load_library()
    peak = [0]

    def meas(xn):
        peak[0] = max(peak[0], int(lib.rbpf_device_bytes_live()))
        return tm.measModel(xn)

    tm.reset()
    out = _run(rbpf, "info", rbpf.DeviceSmootherHandles(tm.dynModel, meas, tm.dynResNorm), p, **dict(CASES[name][5], **kw))
    return out, peak[0], (m, p)


_PEAKS = {}


def _peak(rbpf, **kw):
    """(outputs, peak of rbpf_device_bytes_live() above its value before the run) of the block-lower case on one covariance bank."""
    key = tuple(sorted(kw.items()))
    if key not in _PEAKS:
        base = int(rbpf.load_library().rbpf_device_bytes_live())
        out, peak, _ = _peak_bytes_run(rbpf, "block_lower259", inplace=1, **kw)
        assert int(rbpf.load_library().rbpf_device_bytes_live()) == base
        _PEAKS[key] = (out, peak - base)
    return _PEAKS[key]


def test_refresh_free_on_one_covariance_bank_matches_the_oracle(rbpf):
    """(3, 3, 3, 3, 259) on block-lower storage, lazy_depth = 2, inplace = 1, chol_refresh = 1000."""
    m, p, tm, additive = _case("block_lower259")
    out, _ = _peak(rbpf, chol_refresh=1000)
    ts.check(gs.oracle_run("info", m, p), out, p["N_K"])


def test_refresh_free_stores_no_information_matrix(rbpf):
    """The same run against chol_refresh = 3, whose windowed refreshes keep two banks of N_P information matrices besides the
    carried factors: the refresh-free run holds one chunk of them while it factorises and nothing else of that size, so its
    peak is lower by more than one bank (N_P packed block-lower matrices: 256 * 17 * 18 / 2 doubles each at nLin = 259)."""
    N = CASES["block_lower259"][1]
    _, free = _peak(rbpf, chol_refresh=1000)
    _, window = _peak(rbpf, chol_refresh=3)
    print("peak bytes live: chol_refresh=1000 %d, chol_refresh=3 %d" % (free, window))
    assert window - free > 0.5 * N * 39168 * 8


def test_refresh_free_peak_is_below_the_from_scratch_run(rbpf):
    """The check as the issue of this feature states it: the peak of rbpf_device_bytes_live() with chol_refresh = 1000 below that
    of the same run with chol_refresh = 1.

    Per particle at nLin = 259 the from-scratch run keeps two banks of packed information matrices (39 168 doubles each) and a
    factor workspace (272 * 272 = 73 984): 152 320 doubles.  The refresh-free run keeps two banks of factors in the sweep
    layout (43 032 each) and, per particle of a CHUNK, a matrix, a workspace and the staged Jacobians (about 119 400 with
    N_T - 1 = 4 generations): with the chunk a quarter of the particles at the most (here 2 of 6) that is 86 064 + 39 800
    doubles.  A chunk of all N_P particles, as below N_P = 4096 before, would make it 205 464 and the check fail."""
    _, free = _peak(rbpf, chol_refresh=1000)
    _, scratch = _peak(rbpf, chol_refresh=1)
    print("peak bytes live: chol_refresh=1000 %d, chol_refresh=1 %d" % (free, scratch))
    assert free < scratch


# ------------------------------------------------------------------------------------------------
# the call contract
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["cov", "info"])
def test_call_contract(rbpf, form):
    name = "n_w_below_n_nonlin"
    m, p, tm, additive = _case(name)
    N, T, K = p["N_P"], p["y"].shape[0], p["N_K"]
    seen = []

    def makePlots(xnk, xlk, k, XNK, XLK, PK):
        assert xnk.shape == (m.nNonLin, T) and xlk.shape == (m.nLin,) and np.all(np.isfinite(xnk))
        seen.append(k)

    _run(rbpf, form, _handles(rbpf, tm, additive), p, makePlots=makePlots, **_options(name, form))
    assert tm.columns("dyn") == [N] * (T - 1) + [N - 1] * ((K - 1) * (T - 1))
    assert tm.count("dyn") == K * (T - 1)
    assert tm.count("meas") == K * T + (K - 1)
    assert sorted(tm.columns("meas")) == sorted([N] * (K * T) + [T] * (K - 1))
    assert tm.columns("drn") == [N] * ((K - 1) * (T - 1))
    assert seen == list(range(K))


# ------------------------------------------------------------------------------------------------
# errors, refusals, memory
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["cov", "info"])
def test_a_dyn_model_that_ignores_n_cols_raises_and_leaves_the_library_usable(rbpf, form):
    name = "n_w_below_n_nonlin"
    m, p, tm, additive = _case(name)
    torch = _torch()
    N = p["N_P"]
    lib = rbpf.load_library()
    base = int(lib.rbpf_device_bytes_live())

    def filter_only(xn, dx, dt, Q):                       # written for the filter: always N_P columns
        if xn.shape[1] == N:
            return tm.dynModel(xn, dx, dt, Q)
        tm.calls += 1
        return torch.zeros((m.nNonLin, N), dtype=torch.float64, device=xn.device)

    tm.reset()
    handles = rbpf.DeviceSmootherHandles(filter_only, tm.measModel, tm.dynResNorm)
    with pytest.raises(ValueError) as ei:
        _run(rbpf, form, handles, p, **_options(name, form))
    assert "dynModel" in str(ei.value)
    assert int(lib.rbpf_device_bytes_live()) == base
    tm.reset()
    out = rbpf.particleFilter(handles, None, *_args(p)[:8], p["dt"], rng=rbpf.ReplayRNG(p["U"], p["Z"], p["Ufin"]))
    assert np.all(np.isfinite(out[4]))
    assert int(lib.rbpf_device_bytes_live()) == base


@pytest.mark.parametrize("bad", ["shape", "dtype", "device", "raises"])
def test_a_bad_meas_model_surfaces_as_its_exception(rbpf, bad):
    name = "n_w_below_n_nonlin"
    m, p, tm, additive = _case(name)
    torch = _torch()
    lib = rbpf.load_library()
    base = int(lib.rbpf_device_bytes_live())

    def meas(xn):
        dy = tm.measModel(xn)
        if bad == "shape":
            return dy[:, :, :-1]
        if bad == "dtype":
            return dy.to(torch.float32)
        if bad == "device":
            return dy.cpu()
        raise KeyError("measModel broke")

    tm.reset()
    with pytest.raises(KeyError if bad == "raises" else ValueError):
        _run(rbpf, "info", rbpf.DeviceSmootherHandles(tm.dynModel, meas, tm.dynResNorm), p, chol_refresh=1)
    assert int(lib.rbpf_device_bytes_live()) == base


def test_refusals(rbpf):
    name = "n_w_below_n_nonlin"
    m, p, tm, additive = _case(name)
    for kw in (dict(n_devices=2), dict(sparseFeatures=True)):
        tm.reset()
        with pytest.raises(rbpf.RBPFError) as ei:
            _run(rbpf, "info", _handles(rbpf, tm, additive), p, **kw)
        assert ei.value.status == rbpf.RBPF_ERR_UNSUPPORTED, ei.value
        assert tm.calls == 0 and not tm.log
    tm.reset()
    with pytest.raises(rbpf.RBPFError) as ei:
        _run(rbpf, "cov", _handles(rbpf, tm, additive), p, sparseFeatures=True)
    assert ei.value.status == rbpf.RBPF_ERR_UNSUPPORTED and not tm.log
    # the C entry point on its own: n_devices, and a model that carries host callbacks
    ffi = importlib.import_module(rbpf.__name__ + "._ffi")
    host = importlib.import_module(rbpf.__name__ + ".host")
    model = host._generic_model(None, None, None, p["odometry"], p["y"], p["x0_nonLin"], p["x0_lin"], p["Q"], p["dt"])
    prob = host._Problem(model, p["odometry"], p["y"], p["x0_nonLin"], p["x0_lin"], p["P0_lin"], p["Q"], p["R"], p["N_P"], p["dt"])
    blk, _keep = host._rng_block(rbpf.ReplayRNG(p["U"], p["Z"], p["Ufin"]), prob.N_P, prob.N_T, model.nw, p["N_K"])
    import ctypes as C
    cb = ffi.rbpf_callbacks()
    keep = (ffi.DYN_MODEL_FN(lambda *a: 1), ffi.MEAS_MODEL_FN(lambda *a: 1), ffi.DYN_RES_NORM_FN(lambda *a: 1))
    cb.dyn_model, cb.meas_model, cb.dyn_res_norm = keep
    out = ffi.rbpf_smoother_out()
    lib = rbpf.load_library()
    mdesc = model.descriptor()
    opt = ffi.rbpf_options(keep_history=1, n_devices=2)
    a = (C.byref(mdesc), C.byref(prob.c), C.byref(blk))
    assert lib.rbpf_particle_smoother_device(*a, C.byref(opt), 2, 1, C.byref(cb), 0, C.byref(out)) == rbpf.RBPF_ERR_UNSUPPORTED
    assert b"one GPU" in lib.rbpf_last_error()
    opt = ffi.rbpf_options(keep_history=1)
    assert lib.rbpf_particle_smoother_device(*a, C.byref(opt), 2, 1, C.byref(cb), 7, C.byref(out)) == rbpf.RBPF_ERR_INVALID_ARG
    assert lib.rbpf_particle_smoother_device(*a, C.byref(opt), 2, 1, None, 0, C.byref(out)) == rbpf.RBPF_ERR_INVALID_ARG
    # a callback that fails is RBPF_ERR_CALLBACK, and every byte comes back
    base = int(lib.rbpf_device_bytes_live())
    assert lib.rbpf_particle_smoother_device(*a, C.byref(opt), 2, 1, C.byref(cb), 0, C.byref(out)) == rbpf.RBPF_ERR_CALLBACK
    assert int(lib.rbpf_device_bytes_live()) == base
