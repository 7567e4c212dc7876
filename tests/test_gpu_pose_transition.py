"""GPU: backward simulation in a DeviceMap for pose states (rbpf.DeviceTransition(..., quat_rows=...),
rbpf_loc_generic_backward_pose_*) against the restatement (tests/pose_transition_ref.py).

Tolerances: logp and the smoothed mean 1e-9 relative to the largest magnitude of the quantity, the TOL of
tests/test_gpu_device_map_smoother.py (fp64 products and sums of at most 8 terms, one sqrt, one atan2, one division); indices exact.
Every committed case satisfies the margin condition (every draw at least 100 eps_ref away from a cdf edge):
tests/test_pose_transition_cpu.py asserts it for the probes and for the full runs on the restatement's forward pass, the full-run
test below asserts it again on the device's own forward arrays and on what the device's `mean` handle returned.  No index is
excluded anywhere."""
import numpy as np
import pytest

import localization_smoother_ref as LS
import pose_transition_ref as P
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
    a = dict(mu=p["mu"], w=p["w"], xs_next=p["xs_next"], cov=p["cov"], u=p["u"], rows=p["rows"], angle_rows=p["angle_rows"],
             quat_rows=p["quat_rows"])
    a.update(kw)
    return rbpf.device_map_backward_step(**a)


@pytest.mark.parametrize("name,N,M", P.PROBE_LOGP_CASES)
def test_probe_logp(rbpf, name, N, M):
    p = P.probe_case(name, N, M)
    _, logp, _ = _probe(rbpf, p, want_logp=True)
    want = P.probe_reference(name, N, M)["logp_ld"]
    err = _rel(logp, want)
    print(f"logp {name} {N} x {M}: device vs long double {err:.2e}")
    assert logp.shape == (N, M) and err <= TOL


@pytest.mark.parametrize("name,N,M", P.PROBE_INDEX_CASES)
def test_probe_indices(rbpf, name, N, M):
    p = P.probe_case(name, N, M)
    want = P.probe_reference(name, N, M)
    index, _, _ = _probe(rbpf, p)
    np.testing.assert_array_equal(index, want["index"])                    # every draw
    if N > 2048:
        assert want["index"].max() >= 2048                                 # beyond the largest chunk: not the first one
    for u in (2.0 ** -60, 1.0 - 2.0 ** -53):
        index, _, _ = _probe(rbpf, p, u=np.full(M, u))
        assert np.all(index >= 0) and np.all(index < N) and np.all(p["w"][index] > 0)


@pytest.mark.parametrize("name", P.MODELS)
def test_antipodal_invariance(rbpf, name):
    """q and -q are one rotation: negating the quaternion of every second particle's mu and of every second trajectory changes no
    bit of logp (the negation is exact, every product of e changes sign with it, and the flip e <- -e restores e) and no index."""
    p = P.probe_case(name, 70, 5)
    c = p["case"]
    a, la, _ = _probe(rbpf, p, want_logp=True)
    mu, xs = p["mu"].copy(), p["xs_next"].copy()
    mu[c.qpos:c.qpos + 4, ::2] *= -1.0
    xs[np.ix_(list(c.quat_rows), range(1, xs.shape[1], 2))] *= -1.0
    b, lb, _ = _probe(rbpf, p, mu=mu, xs_next=xs, want_logp=True)
    np.testing.assert_array_equal(la, lb)
    np.testing.assert_array_equal(a, b)
    assert np.all(np.isfinite(la))


def test_zero_rotation(rbpf):
    """A particle and a trajectory that both hold the identity quaternion: e = (1, 0, 0, 0), |e_v| = 0, phi = 0 exactly and logp is
    finite.  Model F (no plain row): logp = 0 exactly.  Model E: the residual is [r_pos; 0], so logp = -|L \\ [r_pos; 0]|^2 / 2, the
    plain-row part, stated here on its own in long double (no quaternion arithmetic); rounding relative to |logp| as TOL."""
    one = np.array([1.0, 0.0, 0.0, 0.0])
    p = P.probe_case("F", 70, 5)
    mu, xs = p["mu"].copy(), p["xs_next"].copy()
    mu[:, 3], xs[:, 2] = one, one
    _, lp, _ = _probe(rbpf, p, mu=mu, xs_next=xs, want_logp=True)
    assert np.all(np.isfinite(lp)) and lp[3, 2] == 0.0
    p = P.probe_case("E", 70, 5)
    mu, xs = p["mu"].copy(), p["xs_next"].copy()
    mu[3:7, 3], xs[3:7, 2] = one, one
    _, lp, _ = _probe(rbpf, p, mu=mu, xs_next=xs, want_logp=True)
    r = np.concatenate((xs[0:3, 2] - mu[0:3, 3], np.zeros(3))).astype(np.longdouble)
    z = P.dm.forward(P.dm.chol(p["cov"].astype(np.longdouble)), r[:, None])
    want = float(-0.5 * np.sum(z * z))
    assert np.all(np.isfinite(lp)) and want < 0.0
    assert abs(lp[3, 2] - want) <= TOL * abs(want)


def test_pairs_far_below_the_running_maximum_are_skipped_without_a_trace(rbpf):
    """Half of the particles moved 60 standard deviations away in position: -z'z / 2 of their plain rows alone lies more than 746
    below the maximum, the pass and the walk leave them before the quaternion product, and their exp is 0 in the restatement too.
    The indices equal the restatement's at every draw (its margin condition asserted here, on these inputs)."""
    p = P.probe_case("E", 64, 64)
    mu = p["mu"].copy()
    mu[0:3, 1::2] += 60.0 * np.sqrt(np.diag(p["cov"])[0:3, None])
    want = P.backward_step(mu, p["w"], p["xs_next"], p["cov"], p["u"], p["rows"], p["angle_rows"], p["quat_rows"])
    assert np.all(want["margin"] >= 100.0 * want["eps_ref"])
    np.testing.assert_array_equal(want["index"], want["index_ld"])
    assert np.max(want["logp_ld"][1::2] - np.max(want["logp_ld"], axis=0)[None, :]) < -800.0
    index, _, _ = _probe(rbpf, p, mu=mu)
    np.testing.assert_array_equal(index, want["index"])
    assert np.all(index % 2 == 0)


def test_agreement_with_the_built_in_kernel_on_dense_mag_inputs(rbpf):
    """The inputs of tests/localization_smoother_ref.py in model E's form (mu = (p + dx_pos, qRight(q) dq), cov = blkdiag(dt Q(1:3,1:3),
    dt Q(4:6,4:6))): logp within TOL of rbpf.loc_backward_step's, the indices those of this file's checker at every draw."""
    p = LS.probe_case(257, 65)
    mu, cov = P.dense_mag_as_pose(p)
    _, built_in, _ = rbpf.loc_backward_step(p["X"], p["w"], p["xs_next"], p["odo"], p["dt"], p["Q"], p["u"], want_logp=True)
    _, lp, _ = rbpf.device_map_backward_step(mu, p["w"], p["xs_next"], cov, p["u"], quat_rows=P.QUAT_E, want_logp=True)
    err = _rel(lp, built_in)
    print(f"logp, pose kernel vs built-in dense-mag kernel: {err:.2e}")
    assert err <= TOL
    for N, M in ((64, 64), (4100, 130)):
        p = LS.probe_case(N, M)
        mu, cov = P.dense_mag_as_pose(p)
        want = P.backward_step(mu, p["w"], p["xs_next"], cov, p["u"], P.ROWS_E, (), P.QUAT_E)
        assert np.all(want["margin"] >= 100.0 * want["eps_ref"])
        np.testing.assert_array_equal(want["index"], want["index_ld"])
        index, _, _ = rbpf.device_map_backward_step(mu, p["w"], p["xs_next"], cov, p["u"], quat_rows=P.QUAT_E)
        np.testing.assert_array_equal(index, want["index"])


# ------------------------------------------------------------------------------------------------
# 2. full runs: torch handles
# ------------------------------------------------------------------------------------------------
class Handles:
    """The device-code side of a pose_transition_ref.PoseCase: dynModel (replaying Z), measModel and the transition's `mean`, which
    records what it returned (mus[t], in the order t = N_T-2 .. 0) for the checker."""

    def __init__(self, c):
        import torch
        import generic_model_torch as gmt
        self.torch, self.c = torch, c
        dev = torch.device("cuda", torch.cuda.current_device())
        self.f = dict(dtype=torch.float64, device=dev)
        self.tm = gmt.TorchGenericModel(c.m, c.p, dev)
        T1 = max(c.p["y"].shape[0] - 1, 1)
        self.Lc = [torch.as_tensor(np.linalg.cholesky(c.cov(t)), **self.f) for t in range(T1)]
        self.rows, self.q = list(c.rows), list(c.quat_rows)
        self.returns = None
        torch.cuda.synchronize()
        self.reset()

    def reset(self):
        self.tm.reset()
        self.calls, self.mean_calls, self.mus = 0, 0, []

    def qmul(self, a, b):
        return self.torch.stack((a[0] * b[0] + (-a[1]) * b[1] + (-a[2]) * b[2] + (-a[3]) * b[3],
                                 a[1] * b[0] + a[0] * b[1] + (-a[3]) * b[2] + a[2] * b[3],
                                 a[2] * b[0] + a[3] * b[1] + a[0] * b[2] + (-a[1]) * b[3],
                                 a[3] * b[0] + (-a[2]) * b[1] + a[1] * b[2] + a[0] * b[3]))

    def expq(self, v):
        torch = self.torch
        a = torch.sqrt(torch.sum(v * v, dim=0))
        return torch.cat((torch.cos(a)[None], (torch.sin(a) / torch.where(a > 0, a, torch.ones_like(a)))[None] * v))

    def drift(self, xn, dx):
        torch, name = self.torch, self.c.name
        ones = torch.ones((1, xn.shape[1]), **self.f)
        if name == "E":
            return torch.cat((xn[0:3] + dx[0:3].reshape(3, 1), self.qmul(dx[3:7].reshape(4, 1) * ones, xn[3:7])))
        if name == "F":
            return self.qmul(xn, dx.reshape(4, 1) * ones)
        return torch.cat((self.qmul(xn[0:4], dx[0:4].reshape(4, 1) * ones),
                          torch.stack((xn[4] + 0.1 * torch.sin(xn[4]) + dx[4], xn[5] + dx[5], xn[6] + dx[6],
                                       xn[7] + 0.1 * torch.sin(xn[5]) + dx[7]))))

    def dynModel(self, xn, dx, dt, Q):
        c, t = self.c, self.calls
        self.calls += 1
        mu = self.drift(xn, dx)
        n = self.Lc[t] @ self.tm.Z[t].t()
        out, k = mu.clone(), 0
        for pos, r in enumerate(c.rows):
            if pos == c.qpos:
                out[self.q] = self.qmul(mu[self.q], self.expq(n[k:k + 3]))
                k += 3
            elif r not in c.quat_rows:
                out[r] = mu[r] + n[k]
                k += 1
        for a in c.angle_rows:
            out[a] = out[a] - 2.0 * np.pi * self.torch.round(out[a] / (2.0 * np.pi))
        return out

    def measModel(self, xn):
        return self.tm.measModel(xn)

    def mean(self, xn, dx, dt, Q):
        self.mean_calls += 1
        mu = self.drift(xn, dx)[self.rows]
        self.mus.append(mu.detach().cpu().numpy().copy())
        if self.returns == "n_res rows":                                  # the residual's count where the selected rows are due
            return mu[:-1]
        return mu

    def transition(self, rbpf):
        c = self.c
        return rbpf.DeviceTransition(self.mean, None if c.default_cov else c.cov_of, None if c.n_sel == c.nN else c.rows, c.angle_rows,
                                     quat_rows=c.quat_rows)

    def map(self, rbpf):
        p = self.c.p
        return rbpf.DeviceMap(rbpf.DeviceHandles(self.dynModel, self.measModel), p["mean"], p["V"], p["R"], transition=self.transition(rbpf))

    def session(self, rbpf):
        p = self.c.p
        self.reset()
        return rbpf.LocalizationSession(self.map(rbpf), p["odometry"], p["y"], p["x0_nonLin"], p["Q"], p["N_P"], p["dt"], keep_history=True,
                                        trace=True, rng=rbpf.ReplayRNG(p["U"], p["Z"]))


_HANDLES = {}


def _handles(name, N_P, N_T):
    key = (name, N_P, N_T)
    if key not in _HANDLES:
        _HANDLES[key] = Handles(P.case(name, N_P, N_T))
    h = _HANDLES[key]
    h.returns = None
    h.reset()
    return h


@pytest.fixture()
def small():
    return _handles("G", 65, 6)


@pytest.mark.parametrize("name,N_P,N_T,M", P.FULL_RUNS)
def test_full_run(rbpf, name, N_P, N_T, M):
    h = _handles(name, N_P, N_T)
    c = h.c
    u = P.full_run_uniforms(N_T, M)
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
    ref_mus, covs = P.transition_arrays(c, X)
    assert all(m.shape == (c.n_sel, N_P) for m in mus)
    assert max(_rel(a, b) for a, b in zip(mus, ref_mus)) < 1e-13          # the torch handle is the numpy statement
    want = P.backward_simulate(X, W, mus, covs, u, c.rows, c.angle_rows, c.quat_rows)
    print(f"min margin {float(want['margin'].min()):.3e}, eps_ref {float(want['eps_ref'].max()):.3e}, logp fp64 vs long double "
          f"{want['logp_rel']:.3e}, largest |phi| {want['max_phi']:.3f}")
    assert np.all(want["margin"] >= 100.0 * want["eps_ref"]) and want["logp_rel"] <= 1e-10 and want["max_phi"] < 1.0
    np.testing.assert_array_equal(want["index"], want["index_ld"])
    assert out["xs_traj"].shape == (c.nN, M, N_T) and out["index"].shape == (M, N_T) and out["traj_smooth_mean"].shape == (c.nN, N_T)
    np.testing.assert_array_equal(out["index"].T, want["index"])
    gathered = np.stack([X[t][:, out["index"][:, t]] for t in range(N_T)], axis=2)
    np.testing.assert_array_equal(out["xs_traj"], gathered)
    err = _rel(out["traj_smooth_mean"], want["traj_smooth_mean"])
    print(f"traj_smooth_mean: {err:.2e}")
    assert err < TOL
    np.testing.assert_array_equal(out["index"][:, N_T - 1], [O.sample(W[N_T - 1], uu) for uu in u[N_T - 1]])
    if M > 1:
        assert len(np.unique(out["index"][:, 0])) > 1


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
    for k in ("xs_traj", "index", "traj_smooth_mean"):
        np.testing.assert_array_equal(a[k], b[k])
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


def test_a_mean_of_the_wrong_shape_is_refused_and_the_session_recovers(rbpf, small):
    h = small
    T, M = h.c.p["y"].shape[0], 5
    u = np.random.RandomState(4).random_sample((T, M))
    with h.session(rbpf) as s:
        s.advance(T)
        s.sync()
        before = _live(rbpf)
        good = s.backward_simulate(M, rng=u)
        assert _live(rbpf) == before
        h.returns = "n_res rows"
        with pytest.raises(ValueError) as ei:
            s.backward_simulate(M, rng=u)
        assert str((h.c.n_sel, h.c.p["N_P"])) in str(ei.value)             # the shape that is due is named
        assert _live(rbpf) == before                                       # nothing stays behind
        h.returns = None
        again = s.backward_simulate(M, rng=u)
    for k in ("xs_traj", "index", "traj_smooth_mean"):
        np.testing.assert_array_equal(again[k], good[k])
