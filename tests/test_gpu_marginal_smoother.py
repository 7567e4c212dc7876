"""GPU: the marginal smoothing weights of the localisation filters (LocalizationSession.smoothed_marginals, rbpf_loc_marginal_*,
rbpf_loc_generic_marginal_*) against the restatement (tests/marginal_smoother_ref.py: every sum in long double and in the log
domain, logp from the three families' checkers).

Tolerances.  The probes' D and lws: 1e-9 max(1, largest finite |value| of that output), the project's own for this arithmetic
class (fp64 products and sums of at most 8 terms per pair, one log-sum-exp per output); -inf is reproduced exactly.  Full runs: the
log-weights of step t within (T - 1 - t) 1e-9 max(1, largest finite |log-weight| of the step) -- errors add in the log domain, one
backward step at a time -- compared where the restatement's log-weight is above -700 (below that exp leaves the normal range of
fp64 and w_smooth, a weight, cannot carry it: there the device's weight must be below exp(-699)); mean, cov and ess within 1e-9
of the largest magnitude of the quantity; |mass - 1| < 1e-9; column N_T-1 of w_smooth is the filter's last weights bit for bit.

Measured on an MI355X: the probes' largest error 9.0e-13 of their scale (the dense-mag term, whose logp carries an atan2; the
Gaussian and pose terms stay below 1e-15); full runs: log-weights at most 1.3e-14 per backward step, mean, cov and ess at most
4.8e-15, |mass - 1| at most 8.9e-16."""
import ctypes as C
import warnings

import numpy as np
import pytest

import map_trajectory_ref as V
import marginal_smoother_ref as G
import transition_sweep_ref as TS

pytestmark = pytest.mark.gpu

TOL = 1e-9
LD = np.longdouble


def _live(rbpf):
    return int(rbpf.load_library().rbpf_device_bytes_live())


# ------------------------------------------------------------------------------------------------
# 1. the probes
# ------------------------------------------------------------------------------------------------
def _probe(rbpf, p, **kw):
    a = dict(p)
    a.update(kw)
    if a["kind"] == "mag":
        D, lws, _ = rbpf.loc_marginal_step(a["X"], a["logw"], a["xs_next"], a["logws_next"], a["odo"], a["dt"], a["Q"])
    else:
        D, lws, _ = rbpf.device_map_marginal_step(a["mu"], a["logw"], a["xs_next"], a["logws_next"], a["cov"], rows=a["rows"],
                                                  angle_rows=a["angle_rows"], quat_rows=a["quat_rows"])
    return D, lws


def _check(got, want, what):
    """-inf exactly; the rest within TOL max(1, largest finite |want|)."""
    w64 = want.astype(np.float64)
    fin = np.isfinite(w64)
    np.testing.assert_array_equal(got[~fin], w64[~fin])
    assert np.all(np.isfinite(got[fin]))
    if not fin.any():
        return 0.0
    scale = max(1.0, float(np.max(np.abs(w64[fin]))))
    err = float(np.max(np.abs(got[fin].astype(LD) - want[fin]))) / scale
    print(f"{what}: device vs long double {err:.2e} of max(1, {scale:.3g}); {int((~fin).sum())} entries -inf")
    assert err < TOL
    return err


def _check_step(rbpf, p, **kw):
    D, lws = _probe(rbpf, p, **kw)
    q = dict(p)
    q.update(kw)
    if kw:
        lp = G.lp_of_probe(q) if set(kw) - {"logw", "logws_next"} else p["lp"]
        wD, _, wl = G.step(q["logw"], lp, q["logws_next"])
    else:
        wD, wl = p["D"], p["lws"]
    assert D.shape == wD.shape and lws.shape == wl.shape
    _check(D, wD, "D")
    _check(lws, wl, "lws")
    return D, lws


@pytest.mark.parametrize("family", G.PROBE_FAMILIES)
@pytest.mark.parametrize("N,M", G.PROBE_SHAPES)
def test_probe(rbpf, family, N, M):
    _check_step(rbpf, G.probe(family, N, M))


@pytest.mark.parametrize("name", TS.NAMES)
def test_every_term_instantiation(rbpf, name):
    _check_step(rbpf, G.sweep(name))


def _pred_key(p):
    return "X" if p["kind"] == "mag" else "mu"


@pytest.mark.parametrize("family", ["mag", "D", "pose3"])
def test_minus_infinity_on_both_sides(rbpf, family):
    N, M = 300, 70
    p = G.probe(family, N, M)
    logw, lwn = p["logw"].copy(), p["logws_next"].copy()
    logw[[40, 255, 256]] = -np.inf                                        # next to the chunk boundary of the norm pass too
    lwn[[0, 20, 69]] = -np.inf
    D, lws = _check_step(rbpf, p, logw=logw, logws_next=lwn)
    np.testing.assert_array_equal(lws == -np.inf, logw == -np.inf)        # a predecessor with w = 0: weight 0
    assert np.all(np.isfinite(D))
    # those i contribute nothing to D, those j nothing to lws: the answers of the inputs without them
    keep_i, keep_j = np.nonzero(logw > -np.inf)[0], np.nonzero(lwn > -np.inf)[0]
    k = _pred_key(p)
    D2, lws2 = _probe(rbpf, p, **{k: p[k][:, keep_i], "logw": logw[keep_i], "xs_next": p["xs_next"][:, keep_j], "logws_next": lwn[keep_j]})
    wD, _, wl = G.step(logw[keep_i], p["lp"][np.ix_(keep_i, keep_j)], lwn[keep_j])
    _check(D2, wD, "D without them")
    _check(lws2, wl, "lws without them")
    _check(D[keep_j], wD, "D, live successors")
    _check(lws[keep_i], wl, "lws, live predecessors")
    # nothing comes back from a step whose smoothed weights are all 0
    D3, lws3 = _probe(rbpf, p, logws_next=np.full(M, -np.inf))
    assert np.all(lws3 == -np.inf)
    _check(D3, p["D"], "D")
    D4, lws4 = _probe(rbpf, p, logw=np.full(N, -np.inf))
    assert np.all(D4 == -np.inf) and np.all(lws4 == -np.inf)


@pytest.mark.parametrize("family,N,M", [("mag", 300, 70), ("D", 300, 70), ("pose3", 300, 70), ("mag", 513, 257), ("pose3", 513, 257)])
def test_a_dominant_pair_and_its_duplicate(rbpf, family, N, M):
    """A successor 1e5 above the rest with a bit-identical duplicate, and the same among the predecessors: everything else falls to
    the skip (746 below the running max) or vanishes through exp.  At 300 x 70 the two predecessors lie in different chunks of the
    norm pass ([0, 256), [256, 300)); at 513 x 257 the two successors lie in different chunks of the weight pass ([0, 256), [256])."""
    assert G.chunks(N, M)[1] >= 2 and (M < 257 or G.chunks(M, N) == (256, 2))
    p = G.probe(family, N, M)
    k = _pred_key(p)
    pred, logw, xs, lwn = p[k].copy(), p["logw"].copy(), p["xs_next"].copy(), p["logws_next"].copy()
    i0, i1 = 30, N - 20                                                   # both live; i1 >= 256
    j0, j1 = 5, M - 1
    pred[:, i1] = pred[:, i0]
    logw[i0] = logw[i1] = 1e5
    xs[:, j1] = xs[:, j0]
    lwn[j0] = lwn[j1] = 1e5
    _check_step(rbpf, p, **{k: pred, "logw": logw, "xs_next": xs, "logws_next": lwn})
    _check_step(rbpf, p, **{k: pred, "logw": logw})                        # the predecessors alone
    _check_step(rbpf, p, xs_next=xs, logws_next=lwn)                      # the successors alone


def test_pruning_leaves_a_pair_decided_by_the_quaternion_alone(rbpf):
    """The plain rows are equal across the predecessors, log w too; the successors carry the LAST predecessor's predicted quaternion
    (phi = 0 there), cov is block diagonal: every running max of the norm pass was passed by the block alone, after the plain rows'
    skip test, and the last predecessor carries nearly all of every D."""
    N, M = 300, 70
    p = dict(G.probe("pose3", N, M))
    mu, xs, cov = p["mu"].copy(), p["xs_next"].copy(), p["cov"].copy()
    mu[:3] = mu[:3, :1]
    xs[3:] = mu[3:, N - 1:N]
    cov[:3, 3:] = 0.0
    cov[3:, :3] = 0.0
    logw = np.zeros(N)
    p.update(mu=mu, xs_next=xs, cov=cov, logw=logw)
    lp = G.lp_of_probe(p)
    assert np.all(np.argmax(lp, axis=0) == N - 1)
    wD, _, wl = G.step(logw, lp, p["logws_next"])
    D, lws = _probe(rbpf, p)
    _check(D, wD, "D")
    _check(lws, wl, "lws")
    assert int(np.argmax(lws)) == N - 1


# ------------------------------------------------------------------------------------------------
# 2. full runs
# ------------------------------------------------------------------------------------------------
def _runner(rbpf, kind, name):
    import test_gpu_map_trajectory as MT                                  # the sessions of the MAP tests: same cases, same handles
    return MT._runner(rbpf, kind, name)


def _reference(r, kind, X, W):
    if kind == "mag":
        return G.run_mag(r.c, X, W)
    if kind == "landmark":
        return G.run_landmark(r.p, X, W)
    assert r.h.mean_calls == V.N_T - 1                                    # once per step, t = N_T-2 .. 0
    return G.run_case(r.c, X, W, mus=list(r.h.mus)[::-1])


def _rel(got, want):
    want64 = np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(np.asarray(got, dtype=LD) - want))) / float(np.max(np.abs(want64)))


ALL = ("w_smooth", "mean", "cov", "ess", "mass")


@pytest.mark.parametrize("kind,name", G.FULL_RUNS)
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
            out = s.smoothed_marginals(want=ALL)
            assert _live(rbpf) == before                                  # the workspace went back to the pool
            X = np.ascontiguousarray(np.transpose(xn_fwd, (2, 0, 1)))    # [T x n x N], the device's own forward particles
            W = np.ascontiguousarray(fwd["trace_w"].T)
            res = _reference(r, kind, X, W)                               # (with what the `mean` handle returned)
            again = s.smoothed_marginals(want=ALL)
            default = s.smoothed_marginals()
    assert _live(rbpf) == base
    assert fwd["first_degenerate_step"] == -1
    nN = X.shape[1]
    assert out["w_smooth"].shape == (N, T) and out["mean"].shape == (nN, T) and out["cov"].shape == (nN, nN, T)
    assert out["ess"].shape == (T,) and out["mass"].shape == (T,)
    ws = out["w_smooth"]
    np.testing.assert_array_equal(ws[:, T - 1], W[T - 1])                 # bit for bit
    assert np.all(ws[W.T == 0.0] == 0.0) and np.all(ws >= 0.0)            # zero weights in the filter: exactly 0
    worst = 0.0
    for t in range(T - 1):
        want = res["logws"][t]
        w64 = want.astype(np.float64)
        big = w64 > -700.0
        assert big.any() and np.all(ws[~big, t] < np.exp(-699.0))
        assert np.all(ws[big, t] > 0.0)
        scale = max(1.0, float(np.max(np.abs(w64[big]))))
        err = float(np.max(np.abs(np.log(ws[big, t]).astype(LD) - want[big]))) / scale
        worst = max(worst, err / (T - 1 - t))
        assert err <= (T - 1 - t) * TOL, (t, err)
    e_mean, e_cov, e_ess = _rel(out["mean"].T, res["mean"]), _rel(np.transpose(out["cov"], (2, 0, 1)), res["cov"]), _rel(out["ess"], res["ess"])
    e_mass = float(np.max(np.abs(out["mass"] - 1.0)))
    print(f"{kind} {name}: log-weights {worst:.2e} per backward step, mean {e_mean:.2e}, cov {e_cov:.2e}, ess {e_ess:.2e}, |mass - 1| {e_mass:.2e}; "
          f"ess from {float(np.min(out['ess'])):.1f} to {float(np.max(out['ess'])):.1f}, filter's {1.0 / float(np.max(np.sum(W * W, axis=1))):.1f} at least")
    assert e_mean <= TOL and e_cov <= TOL and e_ess <= TOL and e_mass < TOL
    assert out["mass"][T - 1] == 1.0
    assert float(np.max(np.abs(ws[:, :T - 1] - W[:T - 1].T))) > 1e-6      # smoothed, not the filter's weights again
    for k in ALL:                                                         # two calls in a row: bit-identical
        np.testing.assert_array_equal(again[k], out[k])
    assert set(default) == {"w_smooth", "mean", "ess"}
    for k in default:
        np.testing.assert_array_equal(default[k], out[k])


def test_the_other_smoothers_are_left_as_they_were(rbpf):
    for kind, name in (("mag", "pages"), ("pose", "E")):
        r = _runner(rbpf, kind, name)
        with r.session() as s:
            s.advance(V.N_T)
            bs0 = s.backward_simulate(16, rng=rbpf.PhiloxRNG(5))
            mt0 = s.map_trajectory()
            s.smoothed_marginals()
            bs1 = s.backward_simulate(16, rng=rbpf.PhiloxRNG(5))
            mt1 = s.map_trajectory()
        for k in bs0:
            np.testing.assert_array_equal(bs1[k], bs0[k])
        for k in ("x_map", "index"):
            np.testing.assert_array_equal(mt1[k], mt0[k])
        assert mt1["score"] == mt0["score"]


def test_one_shot_equals_the_session(rbpf):
    c = V.mag_case("pages")                                               # dt and Q in pages
    r = _runner(rbpf, "mag", "pages")
    with r.session() as s:
        s.advance(V.N_T)
        a = s.smoothed_marginals(want=ALL)
    mp = rbpf.DenseMagMap(rbpf.DenseMagModel(c["NN"], c["L"]), c["mean"], c["V"], c["sigma2"])
    mean, w_smooth, ex = rbpf.particleMarginalSmootherLocalization(mp.dynModel, mp.measModel, c["odometry"], c["y"], c["x0_nonLin"], c["Q"], np.eye(3),
                                                                   c["N_P"], c["dt"], rng=rbpf.ReplayRNG(c["U"], c["Z"]), extras=True)
    np.testing.assert_array_equal(mean, a["mean"])
    np.testing.assert_array_equal(w_smooth, a["w_smooth"])
    for k in ("cov", "ess", "mass"):
        np.testing.assert_array_equal(ex[k], a[k])
    assert ex["traj_max"].shape == (7, V.N_T)
    h = _runner(rbpf, "pose", "E")
    with h.session() as s:
        s.advance(V.N_T)
        b = s.smoothed_marginals()
    p = h.c.p
    h.h.reset()
    mean, w_smooth = rbpf.particleMarginalSmootherLocalization(h.h.map(rbpf), None, p["odometry"], p["y"], p["x0_nonLin"], p["Q"], p["R"], p["N_P"],
                                                               p["dt"], rng=rbpf.ReplayRNG(p["U"], p["Z"]))
    np.testing.assert_array_equal(mean, b["mean"])
    np.testing.assert_array_equal(w_smooth, b["w_smooth"])


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
    r = _runner(rbpf, "mag", "plain")
    T = V.N_T
    for kw in (dict(keep_history=False, trace=True), dict(keep_history=True, trace=False)):
        with r.session(**kw) as s:
            s.advance(T)
            s.sync()
            _refused(rbpf, s.smoothed_marginals, rbpf.RBPF_ERR_STATE, "keep_history = 1 and trace = 1")
    with r.session() as s:
        s.advance(3)
        s.sync()
        _refused(rbpf, s.smoothed_marginals, rbpf.RBPF_ERR_STATE, "3 of 7 steps are done")
        with pytest.raises(ValueError):
            s.smoothed_marginals(want=("x_map",))
        s.advance(T - 3)
        good = s.smoothed_marginals()
    # a degenerate forward step: measurements far outside the map's field
    d = dict(c)
    d["y"] = np.asarray(c["y"]).copy()
    d["y"][4, :] += 1e3 * np.sqrt(c["sigma2"] + 650.0)                    # (as tests/test_gpu_localization_smoother.py)
    import test_gpu_map_trajectory as MT
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        with MT._Mag(rbpf, d).session() as s:
            s.advance(T)
            s.sync()
            _refused(rbpf, s.smoothed_marginals, rbpf.RBPF_ERR_STATE, "degenerate step (t = 4)")
    with r.session() as s:                                                # a valid run in the same process afterwards
        s.advance(T)
        again = s.smoothed_marginals()
    for k in good:
        np.testing.assert_array_equal(again[k], good[k])


def test_refusals_of_the_generic_entry_points(rbpf):
    r = _runner(rbpf, "gauss", "D")
    h, lib, T = r.h, rbpf.load_library(), V.N_T
    rows = (C.c_int32 * 3)(*h.c.rows)
    mask = 4                                                              # rows[2] = state row 3 is the angle
    none5 = (None,) * 5
    base = _live(rbpf)
    with r.session(transition=False) as s:                                # a DeviceMap without a transition
        s.advance(T)
        s.sync()
        _refused(rbpf, s.smoothed_marginals, rbpf.RBPF_ERR_UNSUPPORTED, "transition density")
    h.reset()
    p = h.c.p
    _refused(rbpf, lambda: rbpf.particleMarginalSmootherLocalization(h.map(rbpf, transition=False), None, p["odometry"], p["y"], p["x0_nonLin"],
                                                                      p["Q"], p["R"], p["N_P"], p["dt"], rng=rbpf.ReplayRNG(p["U"], p["Z"])),
             rbpf.RBPF_ERR_UNSUPPORTED, "transition density")
    for kw in (dict(keep_history=False, trace=True), dict(keep_history=True, trace=False)):
        with r.session(**kw) as s:
            s.advance(T)
            s.sync()
            _refused(rbpf, s.smoothed_marginals, rbpf.RBPF_ERR_STATE, "keep_history = 1 and trace = 1")
    with r.session() as s:
        s.advance(2)
        s.sync()
        _refused(rbpf, s.smoothed_marginals, rbpf.RBPF_ERR_STATE, "2 of 7 steps are done")
        s.advance(T - 2)
        s.sync()
        before = _live(rbpf)
        good = s.smoothed_marginals(want=ALL)
        t, xn = C.c_int32(0), C.c_void_p()
        # out of order at the C ABI
        assert lib.rbpf_loc_generic_marginal_step_device(s.ctx, None, None) == rbpf.RBPF_ERR_STATE and b"no marginal pass is open" in lib.rbpf_last_error()
        assert lib.rbpf_loc_generic_marginal_particles_device(s.ctx, C.byref(t), C.byref(xn)) == rbpf.RBPF_ERR_STATE
        assert lib.rbpf_loc_generic_marginal_finish(s.ctx, *none5) == rbpf.RBPF_ERR_STATE
        assert lib.rbpf_loc_generic_marginal_begin(s.ctx, 3, rows, mask, 0) == rbpf.RBPF_ERR_INVALID_ARG     # a block that runs past n_sel
        assert lib.rbpf_loc_generic_marginal_begin(s.ctx, 3, rows, 8, -1) == rbpf.RBPF_ERR_INVALID_ARG       # an angle bit above n_sel
        assert _live(rbpf) == before
        assert lib.rbpf_loc_generic_marginal_begin(s.ctx, 3, rows, mask, -1) == rbpf.RBPF_OK
        assert _live(rbpf) == before + rbpf.device_map_marginal_workspace_bytes(4, 3, V.N_P, T)
        assert lib.rbpf_loc_generic_marginal_begin(s.ctx, 3, rows, mask, -1) == rbpf.RBPF_ERR_STATE and b"a marginal pass is open" in lib.rbpf_last_error()
        st = lib.rbpf_loc_generic_backward_begin(s.ctx, 4, None, 1, 3, rows, mask)                            # nor a backward pass beside it
        assert st == rbpf.RBPF_ERR_STATE and b"a marginal pass is open" in lib.rbpf_last_error()
        st = lib.rbpf_loc_generic_map_begin(s.ctx, 3, rows, mask, -1)                                         # nor a MAP pass
        assert st == rbpf.RBPF_ERR_STATE and b"a marginal pass is open" in lib.rbpf_last_error()
        assert lib.rbpf_loc_generic_marginal_particles_device(s.ctx, C.byref(t), C.byref(xn)) == rbpf.RBPF_OK and t.value == T - 2 and xn.value
        assert lib.rbpf_loc_generic_marginal_step_device(s.ctx, None, None) == rbpf.RBPF_ERR_INVALID_ARG      # every step needs mu and cov
        bad = np.asfortranarray(np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]]))
        st = lib.rbpf_loc_generic_marginal_step_device(s.ctx, xn, bad.ctypes.data_as(C.POINTER(C.c_double)))  # refused before mu is read
        assert st == rbpf.RBPF_ERR_CHOL_FAILED and b"step 5" in lib.rbpf_last_error()
        ess = np.zeros(T)
        assert lib.rbpf_loc_generic_marginal_finish(s.ctx, None, None, None, ess.ctypes.data_as(C.POINTER(C.c_double)), None) == rbpf.RBPF_ERR_STATE
        assert b"steps 5 .. 0" in lib.rbpf_last_error()
        assert _live(rbpf) == before                                      # ... and the workspace is back all the same
        # a marginal pass cannot begin while a backward or a MAP pass is open
        assert lib.rbpf_loc_generic_backward_begin(s.ctx, 4, None, 1, 3, rows, mask) == rbpf.RBPF_OK
        assert lib.rbpf_loc_generic_marginal_begin(s.ctx, 3, rows, mask, -1) == rbpf.RBPF_ERR_STATE and b"a backward pass is open" in lib.rbpf_last_error()
        assert lib.rbpf_loc_generic_backward_finish(s.ctx, None, None, None) == rbpf.RBPF_OK
        assert lib.rbpf_loc_generic_map_begin(s.ctx, 3, rows, mask, -1) == rbpf.RBPF_OK
        assert lib.rbpf_loc_generic_marginal_begin(s.ctx, 3, rows, mask, -1) == rbpf.RBPF_ERR_STATE and b"a MAP pass is open" in lib.rbpf_last_error()
        assert lib.rbpf_loc_generic_map_finish(s.ctx, None, None, None) == rbpf.RBPF_OK
        assert _live(rbpf) == before
        st = lib.rbpf_loc_marginal_smooth(s.ctx, *none5)                                                      # the dense-mag entry point refuses
        assert st == rbpf.RBPF_ERR_UNSUPPORTED and b"transition density" in lib.rbpf_last_error()
        # a cov that is not positive definite, through the binding: before any handle or kernel runs
        tr = s.map.transition
        s.map.transition = rbpf.DeviceTransition(h.mean, lambda dt, Q: bad, h.c.rows, h.c.angle_rows)
        calls = h.mean_calls
        _refused(rbpf, s.smoothed_marginals, rbpf.RBPF_ERR_CHOL_FAILED, "step 0")
        assert h.mean_calls == calls
        s.map.transition = tr
        # a `mean` handle that returns the wrong shape, and one that raises at its third call: nothing stays behind
        h.returns = "shape"
        with pytest.raises(ValueError, match="mean returned"):
            s.smoothed_marginals()
        assert _live(rbpf) == before
        h.returns = None
        import test_gpu_device_map_smoother as GS
        h.mean_calls, h.fail_at = 0, 3
        with pytest.raises(GS.Boom):
            s.smoothed_marginals()
        assert _live(rbpf) == before
        h.fail_at = None
        again = s.smoothed_marginals(want=ALL)                            # a valid run afterwards
        for k in ALL:
            np.testing.assert_array_equal(again[k], good[k])
    with r.session() as s:                                                # rbpf_destroy releases an open pass too
        s.advance(T)
        assert lib.rbpf_loc_generic_marginal_begin(s.ctx, 3, rows, mask, -1) == rbpf.RBPF_OK
    assert _live(rbpf) == base
