"""GPU: backward simulation in a DeviceMap with a Gaussian transition density (rbpf.DeviceTransition, rbpf_loc_generic_backward_*)
against the restatement (tests/device_map_smoother_ref.py).

Tolerances: logp and the smoothed mean 1e-9 relative to the largest magnitude of the quantity, the TOL of
tests/test_gpu_localization_smoother.py (the same arithmetic class: fp64 products and sums of at most 8 terms); indices exact.
Every case satisfies the margin condition (every draw at least 100 eps_ref away from a cdf edge): tests/test_device_map_smoother_cpu.py
asserts it for the probes and for the full runs on the restatement's forward pass, the full-run test below asserts it again on the
device's own forward arrays and on what the device's `mean` handle returned."""
import ctypes as C

import numpy as np
import pytest

import device_map_smoother_ref as S
import rbpf_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-9


def _rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want)) / max(float(np.max(np.abs(want))), 1e-300))


def _live(rbpf):
    return int(rbpf.load_library().rbpf_device_bytes_live())


# ------------------------------------------------------------------------------------------------
# 1. the probe
# ------------------------------------------------------------------------------------------------
def _probe(rbpf, p, **kw):
    a = dict(mu=p["mu"], w=p["w"], xs_next=p["xs_next"], cov=p["cov"], u=p["u"], rows=p["rows"], angle_rows=p["angle_rows"])
    a.update(kw)
    return rbpf.device_map_backward_step(**a)


@pytest.mark.parametrize("name,N,M", S.PROBE_LOGP_CASES)
def test_probe_logp(rbpf, name, N, M):
    p = S.probe_case(name, N, M)
    _, logp, _ = _probe(rbpf, p, want_logp=True)
    want = S.probe_reference(name, N, M)["logp_ld"]
    err = _rel(logp, want)
    print(f"logp {name} {N} x {M}: device vs long double {err:.2e}")
    assert logp.shape == (N, M) and err < TOL


@pytest.mark.parametrize("name,N,M", S.PROBE_INDEX_CASES)
def test_probe_indices(rbpf, name, N, M):
    p = S.probe_case(name, N, M)
    want = S.probe_reference(name, N, M)
    index, _, _ = _probe(rbpf, p)
    np.testing.assert_array_equal(index, want["index"])
    if N > 2048:
        assert want["index"].max() >= 2048                                # beyond the largest chunk: not the first one
    for u in (2.0 ** -60, 1.0 - 2.0 ** -53):
        index, _, _ = _probe(rbpf, p, u=np.full(M, u))
        assert np.all(index >= 0) and np.all(index < N) and np.all(p["w"][index] > 0)


def test_probe_with_default_rows_equals_the_named_ones(rbpf):
    p = S.probe_case("A", 70, 5)
    a, la, _ = _probe(rbpf, p, want_logp=True)
    b, lb, _ = _probe(rbpf, p, rows=None, want_logp=True)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(la, lb)


# ------------------------------------------------------------------------------------------------
# 2. full runs: torch handles
# ------------------------------------------------------------------------------------------------
class Handles:
    """The device-code side of a device_map_smoother_ref.Case: dynModel (replaying Z, as generic_model_torch does), measModel and the
    transition's `mean`, which records what it returned (mus[t], in the order t = N_T-2 .. 0) for the checker."""

    def __init__(self, c):
        import torch
        import generic_model_torch as gmt
        self.torch, self.c = torch, c
        dev = torch.device("cuda", torch.cuda.current_device())
        f = dict(dtype=torch.float64, device=dev)
        self.tm = gmt.TorchGenericModel(c.m, c.p, dev)
        self.Gn = torch.as_tensor(c.Gn, **f)
        self.A = torch.as_tensor(getattr(c, "A", c.m.A), **f)
        self.sin_mask = torch.as_tensor([1.0, 1.0, 1.0, 0.0], **f).reshape(4, 1)
        T1 = max(c.p["y"].shape[0] - 1, 1)
        self.Lq = [torch.as_tensor(np.linalg.cholesky(np.atleast_2d(c.dtt(t) * c.Q(t))), **f) for t in range(T1)]
        self.rows = list(c.rows)
        self.fail_at = None
        self.returns = None
        torch.cuda.synchronize()
        self.reset()

    def reset(self):
        self.tm.reset()
        self.calls, self.mean_calls, self.mus = 0, 0, []

    def wrap(self, x):
        return x - float(S.TWO_PI) * self.torch.round(x / float(S.TWO_PI))

    def drift(self, xn, dx):
        torch, name = self.torch, self.c.name
        if name == "A":
            return xn + self.tm.bend * torch.sin(xn) + self.tm.A @ dx.reshape(-1, 1)
        if name == "B":
            return xn + self.A @ dx.reshape(-1, 1)
        if name == "C":
            co, si = torch.cos(xn[2]), torch.sin(xn[2])
            return torch.stack((xn[0] + co * dx[0] - si * dx[1], xn[1] + si * dx[0] + co * dx[1], xn[2] + dx[2]))
        return xn + 0.1 * torch.sin(xn) * self.sin_mask + self.A @ dx.reshape(-1, 1)

    def dynModel(self, xn, dx, dt, Q):
        if self.c.name == "A":                                            # the handles of tests/generic_model_torch.py
            return self.tm.dynModel(xn, dx, dt, Q)
        t = self.calls
        self.calls += 1
        x = self.drift(xn, dx) + self.Gn @ (self.Lq[t] @ self.tm.Z[t].t())
        for a in self.c.angle_rows:
            x[a] = self.wrap(x[a])
        return x

    def measModel(self, xn):
        return self.tm.measModel(xn)

    def mean(self, xn, dx, dt, Q):
        self.mean_calls += 1
        if self.fail_at == self.mean_calls:
            raise Boom()
        mu = self.drift(xn, dx)[self.rows]
        self.mus.append(mu.detach().cpu().numpy().copy())
        if self.returns == "float32":
            return mu.to(self.torch.float32)
        if self.returns == "shape":
            return mu[:, :-1]
        return mu

    def transition(self, rbpf):
        c = self.c
        return rbpf.DeviceTransition(self.mean, None if c.default_cov else c.cov_of, None if c.n_res == c.nN else c.rows, c.angle_rows)

    def map(self, rbpf, transition=True):
        p = self.c.p
        return rbpf.DeviceMap(rbpf.DeviceHandles(self.dynModel, self.measModel), p["mean"], p["V"], p["R"],
                              transition=self.transition(rbpf) if transition else None)

    def session(self, rbpf, **kw):
        p = self.c.p
        kw.setdefault("keep_history", True)
        kw.setdefault("trace", True)
        kw.setdefault("rng", rbpf.ReplayRNG(p["U"], p["Z"]))
        self.reset()
        mp = self.map(rbpf, kw.pop("transition", True))
        return rbpf.LocalizationSession(mp, p["odometry"], p["y"], p["x0_nonLin"], p["Q"], p["N_P"],
                                        p["dt"], **kw)


class Boom(Exception):
    pass


_HANDLES = {}


def _handles(name, N_P, N_T):
    key = (name, N_P, N_T)
    if key not in _HANDLES:
        _HANDLES[key] = Handles(S.case(name, N_P, N_T))
    h = _HANDLES[key]
    h.fail_at, h.returns = None, None
    h.reset()
    return h


@pytest.fixture()
def small():
    return _handles("D", 65, 6)


@pytest.mark.parametrize("name,N_P,N_T,M", S.FULL_RUNS)
def test_full_run(rbpf, name, N_P, N_T, M):
    h = _handles(name, N_P, N_T)
    c = h.c
    u = S.full_run_uniforms(N_T, M)
    with h.session(rbpf) as s:
        s.advance(N_T)
        fwd = s.finish(extras=True)
        xn_fwd = s.history()
        out = s.backward_simulate(M, rng=u)
    assert fwd["first_degenerate_step"] == -1
    assert h.mean_calls == N_T - 1                                        # once per backward step t = N_T-2 .. 0
    X = np.ascontiguousarray(np.transpose(xn_fwd, (2, 0, 1)))            # [T x n_nonlin x N], the device's own forward particles
    W = np.ascontiguousarray(fwd["trace_w"].T)
    np.testing.assert_array_equal(X[N_T - 1], fwd["final_xn"])
    mus = h.mus[::-1]                                                     # what the handle returned, mus[t]
    ref_mus, covs = S.transition_arrays(c, X)
    assert max(_rel(a, b) for a, b in zip(mus, ref_mus)) < 1e-13          # the torch handle is the numpy statement
    want = S.backward_simulate(X, W, mus, covs, u, c.rows, c.angle_rows)
    print(f"min margin {float(want['margin'].min()):.3e}, eps_ref {float(want['eps_ref'].max()):.3e}, logp fp64 vs long double {want['logp_rel']:.3e}")
    assert np.all(want["margin"] >= 100.0 * want["eps_ref"]) and want["logp_rel"] <= 1e-10
    np.testing.assert_array_equal(want["index"], want["index_ld"])
    assert out["xs_traj"].shape == (c.nN, M, N_T) and out["index"].shape == (M, N_T) and out["traj_smooth_mean"].shape == (c.nN, N_T)
    np.testing.assert_array_equal(out["index"].T, want["index"])
    gathered = np.stack([X[t][:, out["index"][:, t]] for t in range(N_T)], axis=2)
    np.testing.assert_array_equal(out["xs_traj"], gathered)
    err = _rel(out["traj_smooth_mean"], want["traj_smooth_mean"])
    print(f"traj_smooth_mean: {err:.2e}")
    assert err < TOL
    np.testing.assert_array_equal(out["index"][:, N_T - 1], [O.sample(W[N_T - 1], uu) for uu in u[N_T - 1]])


def test_one_shot_equals_the_session_and_repeats(rbpf, small):
    h, p = small, small.c.p
    T, M = p["y"].shape[0], 9
    u = np.random.RandomState(3).random_sample((T, M))
    xs, mean, ex = rbpf.particleSmootherLocalization(h.map(rbpf), None, p["odometry"], p["y"], p["x0_nonLin"], p["Q"], p["R"], p["N_P"], M,
                                                     p["dt"], rng=rbpf.ReplayRNG(p["U"], p["Z"], Uback=u), extras=True)
    with h.session(rbpf) as s:
        s.advance(T)
        a = s.backward_simulate(M, rng=u)
        b = s.backward_simulate(M, rng=u)
        only = s.backward_simulate(M, rng=u, want=("index",))
    for k in ("xs_traj", "index", "traj_smooth_mean"):
        np.testing.assert_array_equal(a[k], b[k])
    np.testing.assert_array_equal(only["index"], a["index"])
    assert set(only) == {"index"}
    np.testing.assert_array_equal(xs, a["xs_traj"])
    np.testing.assert_array_equal(mean, a["traj_smooth_mean"])
    np.testing.assert_array_equal(ex["index"], a["index"])
    assert len(np.unique(a["index"][:, 0])) > 1


def test_philox_seed_equals_the_replay_of_its_uniforms(rbpf, small):
    h = small
    T, M = h.c.p["y"].shape[0], 40
    with h.session(rbpf) as s:
        s.advance(T)
        a = s.backward_simulate(M, rng=rbpf.PhiloxRNG(11))
        b = s.backward_simulate(M, rng=rbpf.PhiloxRNG(11).backward_uniforms(M, T))
        other = s.backward_simulate(M, rng=rbpf.PhiloxRNG(12))
    for k in ("xs_traj", "index", "traj_smooth_mean"):
        np.testing.assert_array_equal(a[k], b[k])
    assert not np.array_equal(other["index"], a["index"])


def test_refusals_and_recovery(rbpf, small):
    h = small
    T, M = h.c.p["y"].shape[0], 5
    lib = rbpf.load_library()
    u = np.random.RandomState(4).random_sample((T, M))
    with h.session(rbpf) as s:
        s.advance(3)
        with pytest.raises(rbpf.RBPFError) as ei:                          # steps missing
            s.backward_simulate(M, rng=u)
        assert ei.value.status == rbpf.RBPF_ERR_STATE
        s.advance(T - 3)
        s.sync()
        before = _live(rbpf)
        for n_traj in (0, -2):
            with pytest.raises(rbpf.RBPFError) as ei:
                s.backward_simulate(n_traj, rng=rbpf.PhiloxRNG(1))
            assert ei.value.status == rbpf.RBPF_ERR_INVALID_ARG
        good = s.backward_simulate(M, rng=u)
        assert _live(rbpf) == before                                       # the pool books return after a good call
        # a handle that raises at the third step surfaces as that exception; nothing stays behind
        h.mean_calls, h.fail_at = 0, 3
        with pytest.raises(Boom):
            s.backward_simulate(M, rng=u)
        assert _live(rbpf) == before
        h.fail_at = None
        for bad in ("float32", "shape"):
            h.returns = bad
            with pytest.raises(ValueError):
                s.backward_simulate(M, rng=u)
            assert _live(rbpf) == before
        h.returns = None
        again = s.backward_simulate(M, rng=u)
        for k in ("xs_traj", "index", "traj_smooth_mean"):
            np.testing.assert_array_equal(again[k], good[k])
        # out of order at the C ABI
        rows = (C.c_int32 * 3)(*h.c.rows)
        t, xn = C.c_int32(0), C.c_void_p()
        assert lib.rbpf_loc_generic_backward_step_device(s.ctx, None, None) == rbpf.RBPF_ERR_STATE
        assert lib.rbpf_loc_generic_backward_particles_device(s.ctx, C.byref(t), C.byref(xn)) == rbpf.RBPF_ERR_STATE
        assert lib.rbpf_loc_generic_backward_finish(s.ctx, None, None, None) == rbpf.RBPF_ERR_STATE
        assert lib.rbpf_loc_generic_backward_begin(s.ctx, M, None, 1, 3, rows, 4) == rbpf.RBPF_OK
        assert _live(rbpf) > before
        assert lib.rbpf_loc_generic_backward_begin(s.ctx, M, None, 1, 3, rows, 4) == rbpf.RBPF_ERR_STATE
        assert lib.rbpf_loc_generic_backward_particles_device(s.ctx, C.byref(t), C.byref(xn)) == rbpf.RBPF_OK and t.value == T - 1 and xn.value
        assert lib.rbpf_loc_generic_backward_step_device(s.ctx, None, None) == rbpf.RBPF_OK        # the draw of step N_T-1
        assert lib.rbpf_loc_generic_backward_step_device(s.ctx, None, None) == rbpf.RBPF_ERR_INVALID_ARG   # later steps need mu and cov
        idx = np.zeros((M, T), dtype=np.int32, order="F")
        assert lib.rbpf_loc_generic_backward_finish(s.ctx, None, idx.ctypes.data_as(C.POINTER(C.c_int32)), None) == rbpf.RBPF_ERR_STATE
        assert _live(rbpf) == before                                       # ... and the workspace is back all the same
        st = lib.rbpf_loc_backward_simulate(s.ctx, 4, None, 1, None, None, None)                  # the dense-mag entry point keeps refusing
        assert st == rbpf.RBPF_ERR_UNSUPPORTED and b"transition density" in lib.rbpf_last_error()
        assert np.all(np.isfinite(s.finish()["traj_mean"]))
        final = s.backward_simulate(M, rng=u)
    np.testing.assert_array_equal(final["index"], good["index"])
    base = _live(rbpf)
    with h.session(rbpf) as s:                                             # rbpf_destroy releases an open pass too
        s.advance(T)
        assert lib.rbpf_loc_generic_backward_begin(s.ctx, M, None, 1, 3, (C.c_int32 * 3)(*h.c.rows), 4) == rbpf.RBPF_OK
    assert _live(rbpf) == base
    for kw in (dict(keep_history=False, trace=True), dict(keep_history=True, trace=False), dict(keep_history=False, trace=False)):
        with h.session(rbpf, **kw) as s:
            s.advance(T)
            with pytest.raises(rbpf.RBPFError) as ei:
                s.backward_simulate(M, rng=u)
            assert ei.value.status == rbpf.RBPF_ERR_STATE
            assert np.all(np.isfinite(s.finish()["traj_mean"]))


def test_a_cov_that_is_not_positive_definite_is_refused_with_the_step(rbpf, small):
    h, p = small, small.c.p
    T = p["y"].shape[0]
    tr = rbpf.DeviceTransition(h.mean, lambda dt, Q: np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]]), h.c.rows, h.c.angle_rows)
    mp = rbpf.DeviceMap(rbpf.DeviceHandles(h.dynModel, h.measModel), p["mean"], p["V"], p["R"], transition=tr)
    h.reset()
    with rbpf.LocalizationSession(mp, p["odometry"], p["y"], p["x0_nonLin"], p["Q"], p["N_P"], p["dt"], rng=rbpf.ReplayRNG(p["U"], p["Z"]),
                                  keep_history=True, trace=True) as s:
        s.advance(T)
        s.sync()
        before = _live(rbpf)
        with pytest.raises(rbpf.RBPFError) as ei:
            s.backward_simulate(4)
        assert ei.value.status == rbpf.RBPF_ERR_CHOL_FAILED and "step 0" in str(ei.value)
        assert h.mean_calls == 0 and _live(rbpf) == before                 # before any kernel or handle ran


def test_a_device_map_without_a_transition_still_refuses(rbpf, small):
    h, p = small, small.c.p
    T = p["y"].shape[0]
    base = _live(rbpf)
    with h.session(rbpf, transition=False) as s:
        s.advance(T)
        with pytest.raises(rbpf.RBPFError) as ei:
            s.backward_simulate(4)
        assert ei.value.status == rbpf.RBPF_ERR_UNSUPPORTED and "transition density" in str(ei.value)
    h.reset()
    with pytest.raises(rbpf.RBPFError) as ei:
        rbpf.particleSmootherLocalization(h.map(rbpf, transition=False), None, p["odometry"], p["y"], p["x0_nonLin"], p["Q"], p["R"], p["N_P"], 4,
                                          p["dt"], rng=rbpf.ReplayRNG(p["U"], p["Z"], Uback=np.full((T, 4), 0.5)))
    assert ei.value.status == rbpf.RBPF_ERR_UNSUPPORTED and "transition density" in str(ei.value)
    assert _live(rbpf) == base
