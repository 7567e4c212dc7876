"""GPU: the MAP trajectory of the localisation filters (LocalizationSession.map_trajectory, rbpf_loc_map_*, rbpf_loc_generic_map_*)
against the restatement (tests/map_trajectory_ref.py: long-double scores, logp from the three families' checkers).

Tolerances: best and score 1e-9 max(1, |value|), the project's own for this arithmetic class (fp64 products and sums of at most 8
terms per pair, one sum per step).  Indices: the device's arg must lie in the restatement's near-best set (all candidates within
2e-9 max(1, |best|) of the best) and equal it where the set is a singleton; the full runs satisfy the cap (at most 1 % of the
(t, j) entries near-tied between distinct particles, none on the optimal path), asserted on the device's own forward arrays, and
their index must then equal the restatement's path."""
import ctypes as C
import warnings

import numpy as np
import pytest

import map_trajectory_ref as V

pytestmark = pytest.mark.gpu

TOL = 1e-9


def _live(rbpf):
    return int(rbpf.load_library().rbpf_device_bytes_live())


# ------------------------------------------------------------------------------------------------
# 1. the probes
# ------------------------------------------------------------------------------------------------
def _probe(rbpf, p, **kw):
    a = dict(p)
    a.update(kw)
    if a["kind"] == "mag":
        best, arg, _ = rbpf.loc_map_step(a["X"], a["delta"], a["xs_next"], a["odo"], a["dt"], a["Q"])
    else:
        best, arg, _ = rbpf.device_map_map_step(a["mu"], a["delta"], a["xs_next"], a["cov"], rows=a["rows"], angle_rows=a["angle_rows"],
                                                quat_rows=a["quat_rows"])
    return best, arg


def _lp(p):
    """The long-double logp matrix of (possibly modified) probe inputs."""
    if p["kind"] == "mag":
        return V.lp_mag(p["xs_next"], p["X"], p["odo"], p["dt"], p["Q"])
    if p["quat_rows"] is not None:
        return V.lp_pose(p["xs_next"], p["mu"], p["cov"], p["rows"], p["angle_rows"], p["quat_rows"])
    return V.lp_gauss(p["xs_next"], p["mu"], p["cov"], p["rows"], p["angle_rows"])


def _check_step(best, arg, want_best, want_near):
    wb = want_best.astype(np.float64)
    fin = np.isfinite(wb)
    np.testing.assert_array_equal(best[~fin], wb[~fin])
    err = float(np.max(np.abs(best[fin].astype(np.longdouble) - want_best[fin]) / np.maximum(1.0, np.abs(want_best[fin])))) if fin.any() else 0.0
    single = sum(n.size == 1 for n in want_near)
    print(f"best: device vs long double {err:.2e}; {single} of {len(want_near)} near-best sets are singletons")
    assert err < TOL
    for j, n in enumerate(want_near):
        assert arg[j] in n, (j, arg[j], n)                                # (a singleton: equal to it)


@pytest.mark.parametrize("family", V.PROBE_FAMILIES)
@pytest.mark.parametrize("N,M", V.PROBE_SHAPES)
def test_probe(rbpf, family, N, M):
    p = V.probe(family, N, M)
    best, arg = _probe(rbpf, p)
    assert best.shape == (M,) and arg.shape == (M,)
    _check_step(best, arg, p["best"], p["near"])


def _pred_key(p):
    return "X" if p["kind"] == "mag" else "mu"


@pytest.mark.parametrize("family", ["mag", "D", "pose3"])
def test_exact_ties_and_minus_infinity(rbpf, family):
    N, M = 300, 70                                                        # chunks [0, 256) and [256, 300)
    p = dict(V.probe(family, N, M))
    k = _pred_key(p)
    pred, delta = p[k].copy(), p["delta"].copy()
    pred[:, 280] = pred[:, 3]                                             # bit-identical, equal delta, in different chunks, dominant
    delta[3] = delta[280] = 1e5
    delta[7] = -np.inf
    pred[:, 7] = pred[:, 3]
    best, arg = _probe(rbpf, p, **{k: pred, "delta": delta})
    np.testing.assert_array_equal(arg, np.full(M, 3))
    want, _, _ = V.step(delta, _lp(dict(p, **{k: pred})))
    assert float(np.max(np.abs(best - want.astype(np.float64)) / np.abs(want.astype(np.float64)))) < TOL
    # without the dominant pair: a column with delta = -inf is never chosen, whatever its logp
    delta = p["delta"].copy()
    delta[3] = -np.inf
    pred = p[k].copy()
    best, arg = _probe(rbpf, p, **{k: pred, "delta": delta})
    assert not np.any(arg == 3) and not np.any(np.isin(arg, np.nonzero(delta == -np.inf)[0]))
    b2, a2, near = V.step(delta, p["lp"])
    _check_step(best, arg, b2, near)
    best, arg = _probe(rbpf, p, delta=np.full(N, -np.inf))
    assert np.all(best == -np.inf) and np.all(arg == 0)


def test_pruning_leaves_a_pair_decided_by_the_quaternion_alone(rbpf):
    """The plain rows are equal across the predecessors, delta too; the successors carry the LAST predecessor's predicted quaternion
    (phi = 0 there), cov is block diagonal: the best predecessor is the last one, and every earlier running best was passed by the
    block alone, after the plain rows' skip test."""
    N, M = 300, 70
    p = dict(V.probe("pose3", N, M))
    mu, xs, cov = p["mu"].copy(), p["xs_next"].copy(), p["cov"].copy()
    mu[:3] = mu[:3, :1]
    xs[3:] = mu[3:, N - 1:N]
    cov[:3, 3:] = 0.0
    cov[3:, :3] = 0.0
    p.update(mu=mu, xs_next=xs, cov=cov, delta=np.zeros(N))
    best, arg = _probe(rbpf, p)
    want, want_arg, near = V.step(p["delta"], _lp(p))
    assert np.all(want_arg == N - 1) and all(n.size == 1 for n in near)
    np.testing.assert_array_equal(arg, want_arg)
    _check_step(best, arg, want, near)


# ------------------------------------------------------------------------------------------------
# 2. full runs
# ------------------------------------------------------------------------------------------------
class _Mag:
    def __init__(self, rbpf, c):
        self.rbpf, self.c = rbpf, c

    def session(self, **kw):
        rbpf, c = self.rbpf, self.c
        kw.setdefault("keep_history", True)
        kw.setdefault("trace", True)
        mp = rbpf.DenseMagMap(rbpf.DenseMagModel(c["NN"], c["L"]), c["mean"], c["V"], c["sigma2"])
        return rbpf.LocalizationSession(mp, c["odometry"], c["y"], c["x0_nonLin"], c["Q"], c["N_P"], c["dt"], rng=rbpf.ReplayRNG(c["U"], c["Z"]), **kw)

    def keep(self):
        pass

    def reference(self, X, W):
        return V.run_mag(self.c, X, W)


class _Handled:
    """A DeviceMap case with the torch handles of the backward-simulation tests: the checker takes what `mean` returned."""

    def __init__(self, rbpf, kind, name):
        if kind == "gauss":
            import test_gpu_device_map_smoother as G
        else:
            import test_gpu_pose_transition as G
        self.rbpf, self.h = rbpf, G._handles(name, V.N_P, V.N_T)
        self.c = self.h.c

    def session(self, **kw):
        return self.h.session(self.rbpf, **kw)

    def keep(self):
        assert self.h.mean_calls == V.N_T - 1                             # once per step t = 0 .. N_T-2, in that order
        self.mus = list(self.h.mus)

    def reference(self, X, W):
        return V.run_case(self.c, X, W, mus=self.mus)


class _Landmark:
    def __init__(self, rbpf):
        import test_gpu_landmark_map as G
        self.rbpf, self.G, self.p = rbpf, G, V.landmark_case()
        self.tw = G.Twin(self.p)

    def session(self, **kw):
        rbpf, p = self.rbpf, self.p
        kw.setdefault("keep_history", True)
        kw.setdefault("trace", True)
        self.tw.reset()
        tr = rbpf.DeviceTransition(self.tw.drift, rows=(0, 1, 2))
        return rbpf.LocalizationSession(self.G._map(rbpf, self.tw, p, tr), p["odometry"], p["y"], p["x0_nonLin"], p["Q"], p["N_P"], p["dt"],
                                        rng=self.G._rng(rbpf, p), **kw)

    def keep(self):
        pass

    def reference(self, X, W):
        return V.run_landmark(self.p, X, W)


def _runner(rbpf, kind, name):
    if kind == "mag":
        return _Mag(rbpf, V.mag_case(name))
    if kind == "landmark":
        return _Landmark(rbpf)
    return _Handled(rbpf, kind, name)


@pytest.mark.parametrize("kind,name", V.FULL_RUNS)
def test_full_run(rbpf, kind, name):
    r = _runner(rbpf, kind, name)
    N, T = V.N_P, V.N_T
    base = _live(rbpf)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        with r.session() as s:
            s.advance(T)
            fwd = s.finish(extras=True)
            xn_fwd = s.history()
            s.sync()
            before = _live(rbpf)
            out = s.map_trajectory()
            assert _live(rbpf) == before                                  # the workspace went back to the pool
            r.keep()                                                      # (what the `mean` handle returned, for the checker)
            again = s.map_trajectory(want=("index",))
    assert _live(rbpf) == base
    assert fwd["first_degenerate_step"] == -1
    X = np.ascontiguousarray(np.transpose(xn_fwd, (2, 0, 1)))            # [T x n x N], the device's own forward particles
    W = np.ascontiguousarray(fwd["trace_w"].T)
    nN = X.shape[1]
    res = r.reference(X, W)
    print(f"{kind} {name}: near-tied entries {res['frac']:.4%}, on the path {res['on_path']}, score {float(res['score']):.9f} "
          f"(device {out['score']:.9f}), path {res['path'].tolist()}")
    assert V.cap_ok(res)                                                  # the cap, on the device's own forward arrays
    assert out["x_map"].shape == (nN, T) and out["index"].shape == (T,) and out["index"].dtype == np.int32
    np.testing.assert_array_equal(out["index"], res["path"])
    np.testing.assert_array_equal(out["x_map"], np.stack([X[t][:, out["index"][t]] for t in range(T)], axis=1))
    assert abs(out["score"] - float(res["score"])) <= TOL * max(1.0, abs(float(res["score"])))
    assert set(again) == {"index"}
    np.testing.assert_array_equal(again["index"], out["index"])
    if np.all(X[0] == X[0][:, :1]):                                       # one x0 column: step 0 ties in every entry
        assert np.all(W[0] == W[0][0]) and out["index"][0] == 0
    else:
        assert kind == "mag"
    assert len(np.unique(out["index"][1:])) > 1


def test_step_zero_ties_are_decided_by_the_lowest_index(rbpf):
    """x0_cols = 1: every particle of step 0 is the same state with the same weight, so psi of step 1 ties in every entry."""
    r = _runner(rbpf, "gauss", "D")
    with r.session() as s:
        s.advance(V.N_T)
        fwd = s.finish(extras=True)
        X0 = s.history()[:, :, 0]
        out = s.map_trajectory()
    assert np.all(X0 == X0[:, :1]) and np.ptp(fwd["trace_w"][:, 0]) == 0.0
    assert out["index"][0] == 0 and out["index"][1] != 0


def test_one_shot_equals_the_session(rbpf):
    c = V.mag_case("pages")                                               # dt and Q in pages
    r = _Mag(rbpf, c)
    with r.session() as s:
        s.advance(V.N_T)
        a = s.map_trajectory()
    mp = rbpf.DenseMagMap(rbpf.DenseMagModel(c["NN"], c["L"]), c["mean"], c["V"], c["sigma2"])
    x_map, score, ex = rbpf.particleMapLocalization(mp.dynModel, mp.measModel, c["odometry"], c["y"], c["x0_nonLin"], c["Q"], np.eye(3), c["N_P"],
                                                    c["dt"], rng=rbpf.ReplayRNG(c["U"], c["Z"]), extras=True)
    np.testing.assert_array_equal(x_map, a["x_map"])
    np.testing.assert_array_equal(ex["index"], a["index"])
    assert score == a["score"] and ex["traj_max"].shape == (7, V.N_T)
    h = _runner(rbpf, "pose", "E")
    with h.session() as s:
        s.advance(V.N_T)
        b = s.map_trajectory()
    p = h.c.p
    h.h.reset()
    x_map, score = rbpf.particleMapLocalization(h.h.map(rbpf), None, p["odometry"], p["y"], p["x0_nonLin"], p["Q"], p["R"], p["N_P"], p["dt"],
                                                rng=rbpf.ReplayRNG(p["U"], p["Z"]))
    np.testing.assert_array_equal(x_map, b["x_map"])
    assert score == b["score"]


# ------------------------------------------------------------------------------------------------
# 3. refusals
# ------------------------------------------------------------------------------------------------
def _refused(rbpf, fn, status, text):
    before = _live(rbpf)
    with pytest.raises(rbpf.RBPFError) as ei:
        fn()
    assert ei.value.status == status and text in str(ei.value), str(ei.value)
    assert _live(rbpf) == before


def test_refusals_of_the_dense_mag_entry_point(rbpf):
    c = V.mag_case("plain")
    r = _Mag(rbpf, c)
    T = V.N_T
    for kw in (dict(keep_history=False, trace=True), dict(keep_history=True, trace=False)):
        with r.session(**kw) as s:
            s.advance(T)
            s.sync()
            _refused(rbpf, s.map_trajectory, rbpf.RBPF_ERR_STATE, "keep_history = 1 and trace = 1")
    with r.session() as s:
        s.advance(3)
        s.sync()
        _refused(rbpf, s.map_trajectory, rbpf.RBPF_ERR_STATE, "3 of 7 steps are done")
        with pytest.raises(ValueError):
            s.map_trajectory(want=("xs_traj",))
        s.advance(T - 3)
        good = s.map_trajectory()
    # a degenerate forward step: measurements far outside the map's field
    d = dict(c)
    d["y"] = np.asarray(c["y"]).copy()
    d["y"][4, :] += 1e3 * np.sqrt(c["sigma2"] + 650.0)                    # (as tests/test_gpu_localization_smoother.py)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        with _Mag(rbpf, d).session() as s:
            s.advance(T)
            s.sync()
            _refused(rbpf, s.map_trajectory, rbpf.RBPF_ERR_STATE, "degenerate step (t = 4)")
    with r.session() as s:                                                # a valid run in the same process afterwards
        s.advance(T)
        again = s.map_trajectory()
    np.testing.assert_array_equal(again["index"], good["index"])
    assert again["score"] == good["score"]


def test_refusals_of_the_generic_entry_points(rbpf):
    r = _runner(rbpf, "gauss", "D")
    h, lib, T = r.h, rbpf.load_library(), V.N_T
    rows = (C.c_int32 * 3)(*h.c.rows)
    mask = 4                                                              # rows[2] = state row 3 is the angle
    base = _live(rbpf)
    with r.session(transition=False) as s:                                # a DeviceMap without a transition
        s.advance(T)
        s.sync()
        _refused(rbpf, s.map_trajectory, rbpf.RBPF_ERR_UNSUPPORTED, "transition density")
    h.reset()
    p = h.c.p
    _refused(rbpf, lambda: rbpf.particleMapLocalization(h.map(rbpf, transition=False), None, p["odometry"], p["y"], p["x0_nonLin"], p["Q"], p["R"],
                                                         p["N_P"], p["dt"], rng=rbpf.ReplayRNG(p["U"], p["Z"])),
             rbpf.RBPF_ERR_UNSUPPORTED, "transition density")
    for kw in (dict(keep_history=False, trace=True), dict(keep_history=True, trace=False)):
        with r.session(**kw) as s:
            s.advance(T)
            s.sync()
            _refused(rbpf, s.map_trajectory, rbpf.RBPF_ERR_STATE, "keep_history = 1 and trace = 1")
    with r.session() as s:
        s.advance(2)
        s.sync()
        _refused(rbpf, s.map_trajectory, rbpf.RBPF_ERR_STATE, "2 of 7 steps are done")
        s.advance(T - 2)
        s.sync()
        before = _live(rbpf)
        good = s.map_trajectory()
        t, xn = C.c_int32(0), C.c_void_p()
        # out of order at the C ABI
        assert lib.rbpf_loc_generic_map_step_device(s.ctx, None, None) == rbpf.RBPF_ERR_STATE and b"no MAP pass is open" in lib.rbpf_last_error()
        assert lib.rbpf_loc_generic_map_particles_device(s.ctx, C.byref(t), C.byref(xn)) == rbpf.RBPF_ERR_STATE
        assert lib.rbpf_loc_generic_map_finish(s.ctx, None, None, None) == rbpf.RBPF_ERR_STATE
        assert lib.rbpf_loc_generic_map_begin(s.ctx, 3, rows, mask, 0) == rbpf.RBPF_ERR_INVALID_ARG          # a block that runs past n_sel
        assert lib.rbpf_loc_generic_map_begin(s.ctx, 3, rows, 8, -1) == rbpf.RBPF_ERR_INVALID_ARG            # an angle bit above n_sel
        assert _live(rbpf) == before
        assert lib.rbpf_loc_generic_map_begin(s.ctx, 3, rows, mask, -1) == rbpf.RBPF_OK
        assert _live(rbpf) == before + rbpf.device_map_map_workspace_bytes(4, 3, V.N_P, T)
        assert lib.rbpf_loc_generic_map_begin(s.ctx, 3, rows, mask, -1) == rbpf.RBPF_ERR_STATE and b"a MAP pass is open" in lib.rbpf_last_error()
        st = lib.rbpf_loc_generic_backward_begin(s.ctx, 4, None, 1, 3, rows, mask)                            # nor a backward pass beside it
        assert st == rbpf.RBPF_ERR_STATE and b"a MAP pass is open" in lib.rbpf_last_error()
        assert lib.rbpf_loc_generic_map_particles_device(s.ctx, C.byref(t), C.byref(xn)) == rbpf.RBPF_OK and t.value == 0 and xn.value
        assert lib.rbpf_loc_generic_map_step_device(s.ctx, None, None) == rbpf.RBPF_ERR_INVALID_ARG           # every step needs mu and cov
        bad = np.asfortranarray(np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]]))
        st = lib.rbpf_loc_generic_map_step_device(s.ctx, xn, bad.ctypes.data_as(C.POINTER(C.c_double)))      # refused before mu is read
        assert st == rbpf.RBPF_ERR_CHOL_FAILED and b"step 0" in lib.rbpf_last_error()
        idx = np.zeros(T, dtype=np.int32)
        assert lib.rbpf_loc_generic_map_finish(s.ctx, None, idx.ctypes.data_as(C.POINTER(C.c_int32)), None) == rbpf.RBPF_ERR_STATE
        assert b"steps 0 .. 5" in lib.rbpf_last_error()
        assert _live(rbpf) == before                                      # ... and the workspace is back all the same
        # a MAP pass cannot begin while a backward pass is open
        assert lib.rbpf_loc_generic_backward_begin(s.ctx, 4, None, 1, 3, rows, mask) == rbpf.RBPF_OK
        assert lib.rbpf_loc_generic_map_begin(s.ctx, 3, rows, mask, -1) == rbpf.RBPF_ERR_STATE and b"a backward pass is open" in lib.rbpf_last_error()
        assert lib.rbpf_loc_generic_backward_finish(s.ctx, None, None, None) == rbpf.RBPF_OK
        assert _live(rbpf) == before
        st = lib.rbpf_loc_map_trajectory(s.ctx, None, None, None)                                             # the dense-mag entry point refuses
        assert st == rbpf.RBPF_ERR_UNSUPPORTED and b"transition density" in lib.rbpf_last_error()
        # a cov that is not positive definite, through the binding: before any handle or kernel runs
        tr = s.map.transition
        s.map.transition = rbpf.DeviceTransition(h.mean, lambda dt, Q: bad, h.c.rows, h.c.angle_rows)
        calls = h.mean_calls
        _refused(rbpf, s.map_trajectory, rbpf.RBPF_ERR_CHOL_FAILED, "step 0")
        assert h.mean_calls == calls
        s.map.transition = tr
        # a handle that raises at its third call surfaces as that exception; nothing stays behind
        import test_gpu_device_map_smoother as G
        h.mean_calls, h.fail_at = 0, 3
        with pytest.raises(G.Boom):
            s.map_trajectory()
        assert _live(rbpf) == before
        h.fail_at = None
        again = s.map_trajectory()                                        # a valid run afterwards
        np.testing.assert_array_equal(again["index"], good["index"])
        np.testing.assert_array_equal(again["x_map"], good["x_map"])
        assert again["score"] == good["score"]
    with r.session() as s:                                                # rbpf_destroy releases an open pass too
        s.advance(T)
        assert lib.rbpf_loc_generic_map_begin(s.ctx, 3, rows, mask, -1) == rbpf.RBPF_OK
    assert _live(rbpf) == base
