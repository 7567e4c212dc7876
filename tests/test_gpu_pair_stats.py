"""GPU: the two-slice statistics of the transition residual (LocalizationSession.transition_statistics, rbpf_loc_pair_stats_*,
rbpf_loc_generic_pair_stats_*, csrc/rbpf_loc_pairstats.hpp) against the restatement (tests/pair_stats_ref.py: every sum in long
double, the residuals from the three families' checkers, D, c and lws from marginal_smoother_ref.step).

Tolerances (TOL = 1e-9, the project's class for this arithmetic, as tests/test_gpu_marginal_smoother.py): S within TOL of max |S_ref| of
the page; m within TOL of sqrt(max diag S_ref), the natural scale of m, which may cancel to nearly 0; |pair_mass - 1| < TOL wherever
the step's mass is positive (pair_mass exactly 0 where it is 0).  In full runs page t gets the factor (N_T - 1 - t) that the
log-weights get: xi_t is built on log w_{t+1|T}, whose error grows by one backward step at a time.  D and lws of the statistics probes
are those of the marginal probes bit for bit, and w_smooth, mean, cov, ess, mass of transition_statistics those of smoothed_marginals:
the same kernels produce them.

The probe shapes are the smallest at which the pass can go wrong: 300 x 70 (a ragged last block, whose lanes past the end must add
zero; one chunk), 513 x 257 (two successor chunks, three predecessor blocks), 1 x 5 and 1 x 1, 2304 x 2304 (9 x 9 workgroups) and, for
the cheapest Gaussian family only, 4352 x 4352 (17 x 17 = 289 workgroups: more than the reducer's 256 lanes).

The dominant pair of test_a_dominant_pair_and_its_duplicate lies 600 above the rest, not the 1e5 of the marginal tests: the
statistics need the step's mass = sum_i exp(lws(i)) inside fp64, as the mass of a session's step always is (its weights are normalised).

Measured on an MI355X: the probes' largest errors S 6.6e-13, m 2.6e-13, |pair_mass - 1| 2.1e-13 of their scales, all three in the
dominant-pair cases of the dense-mag term (log xi is a difference of numbers near 600 there, and its logp carries an atan2; the
dense-mag term's plain probes reach 3.5e-13, the Gaussian and pose terms 1.3e-13 in a dominant-pair case); full runs: per backward step S at most 3.1e-15, m 3.1e-15, |pair_mass - 1| 4.4e-16."""
import ctypes as C
import warnings

import numpy as np
import pytest

import map_trajectory_ref as V
import marginal_smoother_ref as G
import pair_stats_ref as PS
import transition_sweep_ref as TS

pytestmark = pytest.mark.gpu

TOL = 1e-9
LD = np.longdouble


def _live(rbpf):
    return int(rbpf.load_library().rbpf_device_bytes_live())


# ------------------------------------------------------------------------------------------------
# 1. the probes
# ------------------------------------------------------------------------------------------------
def _probe(rbpf, p, stats=True, **kw):
    a = dict(p)
    a.update(kw)
    if a["kind"] == "mag":
        f = rbpf.loc_pair_stats_step if stats else rbpf.loc_marginal_step
        return f(a["X"], a["logw"], a["xs_next"], a["logws_next"], a["odo"], a["dt"], a["Q"])[:-1]
    f = rbpf.device_map_pair_stats_step if stats else rbpf.device_map_marginal_step
    return f(a["mu"], a["logw"], a["xs_next"], a["logws_next"], a["cov"], rows=a["rows"], angle_rows=a["angle_rows"], quat_rows=a["quat_rows"])[:-1]


def _check_moments(S, m, pm, want, what, factor=1.0):
    """S, m, pair_mass of one page against the restatement's (a dict with S, m, pair_mass, mass); returns the three errors."""
    wS, wm = np.asarray(want["S"], dtype=LD), np.asarray(want["m"], dtype=LD)
    assert S.shape == wS.shape and m.shape == wm.shape
    assert np.all(np.isfinite(S)) and np.all(np.isfinite(m)) and np.isfinite(pm)
    np.testing.assert_array_equal(S, S.T)                                  # both triangles are written from one sum
    if not float(want["mass"]) > 0.0:
        assert np.all(S == 0.0) and np.all(m == 0.0) and pm == 0.0
        print(f"{what}: mass 0, everything exactly 0")
        return 0.0, 0.0, 0.0
    sS = float(np.max(np.abs(wS)))
    sm = float(np.sqrt(np.max(np.diag(wS))))
    eS = float(np.max(np.abs(S.astype(LD) - wS))) / sS
    em = float(np.max(np.abs(m.astype(LD) - wm))) / sm
    ep = abs(float(pm) - 1.0)
    print(f"{what}: S {eS:.2e} of {sS:.3g}, m {em:.2e} of {sm:.3g}, |pair_mass - 1| {ep:.2e} (restatement's {abs(float(want['pair_mass']) - 1.0):.1e})")
    assert eS <= factor * TOL and em <= factor * TOL and ep < factor * TOL
    return eS, em, ep


def _check_step(rbpf, p, what, **kw):
    """The statistics probe on p (with kw over its inputs) against the restatement of the same inputs."""
    D, lws, S, m, pm = _probe(rbpf, p, **kw)
    if kw:
        q = dict(p)
        q.update(kw)
        lp = G.lp_of_probe(q) if set(kw) - {"logw", "logws_next"} else p["lp"]
        want = PS.step(q["logw"], lp, q["logws_next"], PS.r_of_probe(q))
    else:
        want = p
    D0, lws0 = _probe(rbpf, p, stats=False, **kw)
    np.testing.assert_array_equal(D, D0)                                   # the marginal step's kernels, bit for bit
    np.testing.assert_array_equal(lws, lws0)
    _check_moments(S, m, pm, want, what)
    return S, m, pm, want


@pytest.mark.parametrize("family", PS.PROBE_FAMILIES)
@pytest.mark.parametrize("N,M", PS.PROBE_SHAPES)
def test_probe(rbpf, family, N, M):
    _check_step(rbpf, PS.probe(family, N, M), f"{family} {N} x {M}")


def test_more_workgroups_than_the_reducer_has_lanes(rbpf):
    family, N, M = PS.BIG
    assert PS.groups(N, M) == (17, 17)
    _check_step(rbpf, PS.probe(family, N, M), f"{family} {N} x {M}")


@pytest.mark.parametrize("name", TS.NAMES)
def test_every_term_instantiation(rbpf, name):
    """S and m in the CALLER's residual order: a wrong un-permutation behind a quaternion block shows here."""
    _check_step(rbpf, PS.sweep(name), name)


def _pred_key(p):
    return "X" if p["kind"] == "mag" else "mu"


@pytest.mark.parametrize("family", ["mag", "D", "pose3"])
def test_minus_infinity_on_both_sides(rbpf, family):
    N, M = 300, 70
    p = PS.probe(family, N, M)
    logw, lwn = p["logw"].copy(), p["logws_next"].copy()
    logw[[40, 255, 256]] = -np.inf                                        # next to the block boundary of the pass too
    lwn[[0, 20, 69]] = -np.inf
    S, m, pm, want = _check_step(rbpf, p, f"{family}, -inf on both sides", logw=logw, logws_next=lwn)
    # those i and those j carry no pair: the answers of the inputs without them
    keep_i, keep_j = np.nonzero(logw > -np.inf)[0], np.nonzero(lwn > -np.inf)[0]
    k = _pred_key(p)
    _, _, S2, m2, pm2 = _probe(rbpf, p, **{k: p[k][:, keep_i], "logw": logw[keep_i], "xs_next": p["xs_next"][:, keep_j], "logws_next": lwn[keep_j]})
    _check_moments(S2, m2, pm2, want, f"{family}, without them")


@pytest.mark.parametrize("family", ["mag", "D", "pose3"])
def test_nothing_comes_back_from_a_step_without_smoothed_weight(rbpf, family):
    """Every c(j) = -inf (no successor carries weight, or no predecessor does: D = -inf): the mass is 0, log(mass) = -inf must not
    become a NaN, and S, m and pair_mass are exactly 0."""
    N, M = 300, 70
    p = PS.probe(family, N, M)
    n = p["S"].shape[0]
    for kw in (dict(logws_next=np.full(M, -np.inf)), dict(logw=np.full(N, -np.inf)),
               dict(logw=np.full(N, -np.inf), logws_next=np.full(M, -np.inf))):
        D, lws, S, m, pm = _probe(rbpf, p, **kw)
        assert np.all(lws == -np.inf)
        np.testing.assert_array_equal(S, np.zeros((n, n)))
        np.testing.assert_array_equal(m, np.zeros(n))
        assert pm == 0.0


@pytest.mark.parametrize("family,N,M", [("mag", 300, 70), ("D", 300, 70), ("pose3", 300, 70), ("mag", 513, 257), ("pose3", 513, 257)])
def test_a_dominant_pair_and_its_duplicate(rbpf, family, N, M):
    """A successor 600 above the rest with a bit-identical duplicate, and the same among the predecessors: the four pairs between them
    carry xi = 1/4 each and everything else falls to the skip (746 below) or vanishes through exp.  At 513 x 257 the two successors lie
    in different chunks ([0, 256), [256]) and the two predecessors in different blocks."""
    p = PS.probe(family, N, M)
    k = _pred_key(p)
    pred, logw, xs, lwn = p[k].copy(), p["logw"].copy(), p["xs_next"].copy(), p["logws_next"].copy()
    i0, i1 = 30, N - 20                                                   # both live; i1 >= 256
    j0, j1 = 5, M - 1
    pred[:, i1] = pred[:, i0]
    logw[i0] = logw[i1] = 600.0
    xs[:, j1] = xs[:, j0]
    lwn[j0] = lwn[j1] = 600.0
    S, m, pm, want = _check_step(rbpf, p, f"{family} {N} x {M}, both", **{k: pred, "logw": logw, "xs_next": xs, "logws_next": lwn})
    r = PS.r_of_probe(dict(p, **{k: pred, "xs_next": xs}))(j0)[:, i0]
    assert float(np.max(np.abs(want["S"] - np.outer(r, r)))) <= 1e-12 * float(np.max(np.abs(np.outer(r, r))))   # the inputs do what they are for: that pair's r r'
    _check_step(rbpf, p, f"{family} {N} x {M}, predecessors", **{k: pred, "logw": logw})
    _check_step(rbpf, p, f"{family} {N} x {M}, successors", xs_next=xs, logws_next=lwn)


def test_pruning_leaves_a_pair_decided_by_the_quaternion_alone(rbpf):
    """The plain rows are equal across the predecessors, log w too; the successors carry the LAST predecessor's predicted quaternion
    (phi = 0 there), cov is block diagonal: the plain rows' skip test cannot tell the pairs apart, the block alone does, and the last
    predecessor carries nearly all of xi -- with a residual whose block entries are 0."""
    N, M = 300, 70
    p = dict(PS.probe("pose3", N, M))
    mu, xs, cov = p["mu"].copy(), p["xs_next"].copy(), p["cov"].copy()
    mu[:3] = mu[:3, :1]
    xs[3:] = mu[3:, N - 1:N]
    cov[:3, 3:] = 0.0
    cov[3:, :3] = 0.0
    logw = np.zeros(N)
    q = dict(p, mu=mu, xs_next=xs, cov=cov, logw=logw)
    assert np.all(np.argmax(G.lp_of_probe(q), axis=0) == N - 1)
    _check_step(rbpf, p, "pose3, the quaternion alone", mu=mu, xs_next=xs, cov=cov, logw=logw)


# ------------------------------------------------------------------------------------------------
# 2. full runs
# ------------------------------------------------------------------------------------------------
def _runner(rbpf, kind, name):
    import test_gpu_map_trajectory as MT                                  # the sessions of the MAP tests: same cases, same handles
    return MT._runner(rbpf, kind, name)


def _forget_mean_calls(r, kind):
    if kind in ("gauss", "pose"):
        r.h.mean_calls, r.h.mus = 0, []


def _reference(r, kind, X, W):
    if kind == "mag":
        return PS.run_mag(r.c, X, W)
    if kind == "landmark":
        return PS.run_landmark(r.p, X, W)
    assert r.h.mean_calls == V.N_T - 1                                    # once per step, t = N_T-2 .. 0
    return PS.run_case(r.c, X, W, mus=list(r.h.mus)[::-1])


MARG = ("w_smooth", "mean", "cov", "ess", "mass")
STATS = ("S", "m", "pair_mass")


@pytest.mark.parametrize("kind,name", PS.FULL_RUNS)
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
            marg = s.smoothed_marginals(want=MARG)
            _forget_mean_calls(r, kind)
            out = s.transition_statistics(want=MARG + STATS)
            assert _live(rbpf) == before                                  # the workspace went back to the pool
            X = np.ascontiguousarray(np.transpose(xn_fwd, (2, 0, 1)))    # [T x n x N], the device's own forward particles
            W = np.ascontiguousarray(fwd["trace_w"].T)
            res = _reference(r, kind, X, W)                               # (with what the `mean` handle returned)
            again = s.transition_statistics(want=MARG + STATS)
            default = s.transition_statistics()
            only = s.transition_statistics(want=("S",))
    assert _live(rbpf) == base
    assert fwd["first_degenerate_step"] == -1
    n = res["S"].shape[1]
    assert out["S"].shape == (n, n, T - 1) and out["m"].shape == (n, T - 1) and out["pair_mass"].shape == (T - 1,)
    for k in MARG:                                                        # the marginal smoother's outputs: the same kernels, bit for bit
        np.testing.assert_array_equal(out[k], marg[k])
    worst = np.zeros(3)
    for t in range(T - 1):
        want = dict(S=res["S"][t], m=res["m"][t], pair_mass=res["pair_mass"][t], mass=res["mass"][t])
        e = _check_moments(np.ascontiguousarray(out["S"][:, :, t]), out["m"][:, t].copy(), out["pair_mass"][t], want, f"{kind} {name} page {t}",
                           factor=T - 1 - t)
        worst = np.maximum(worst, np.array(e) / (T - 1 - t))
    print(f"{kind} {name}: worst per backward step: S {worst[0]:.2e}, m {worst[1]:.2e}, |pair_mass - 1| {worst[2]:.2e}")
    for k in MARG + STATS:                                                # two calls in a row: bit-identical
        np.testing.assert_array_equal(again[k], out[k])
    assert set(default) == {"S", "m", "pair_mass", "w_smooth", "mean"}
    for k in default:
        np.testing.assert_array_equal(default[k], out[k])
    assert set(only) == {"S"}
    np.testing.assert_array_equal(only["S"], out["S"])
    # the statistics estimate the noise the run was made with, to the accuracy N_T - 1 = 6 pages allow: positive definite at least
    assert np.all(np.linalg.eigvalsh(rbpf.transition_noise_estimate(out["S"], np.ones(T - 1))) > 0.0)


def test_the_other_smoothers_are_left_as_they_were(rbpf):
    for kind, name in (("mag", "pages"), ("pose", "E")):
        r = _runner(rbpf, kind, name)
        with r.session() as s:
            s.advance(V.N_T)
            sm0 = s.smoothed_marginals(want=MARG)
            bs0 = s.backward_simulate(16, rng=rbpf.PhiloxRNG(5))
            mt0 = s.map_trajectory()
            s.transition_statistics()
            sm1 = s.smoothed_marginals(want=MARG)
            bs1 = s.backward_simulate(16, rng=rbpf.PhiloxRNG(5))
            mt1 = s.map_trajectory()
        for k in sm0:
            np.testing.assert_array_equal(sm1[k], sm0[k])
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
        a = s.transition_statistics(want=MARG + STATS)
    mp = rbpf.DenseMagMap(rbpf.DenseMagModel(c["NN"], c["L"]), c["mean"], c["V"], c["sigma2"])
    S, m, pm, ex = rbpf.particleTransitionStatisticsLocalization(mp.dynModel, mp.measModel, c["odometry"], c["y"], c["x0_nonLin"], c["Q"], np.eye(3),
                                                                 c["N_P"], c["dt"], rng=rbpf.ReplayRNG(c["U"], c["Z"]), extras=True)
    for got, k in ((S, "S"), (m, "m"), (pm, "pair_mass")):
        np.testing.assert_array_equal(got, a[k])
    for k in MARG:
        np.testing.assert_array_equal(ex[k], a[k])
    assert ex["traj_max"].shape == (7, V.N_T) and S.shape == (6, 6, V.N_T - 1)
    h = _runner(rbpf, "pose", "E")
    with h.session() as s:
        s.advance(V.N_T)
        b = s.transition_statistics()
    p = h.c.p
    h.h.reset()
    S, m, pm = rbpf.particleTransitionStatisticsLocalization(h.h.map(rbpf), None, p["odometry"], p["y"], p["x0_nonLin"], p["Q"], p["R"], p["N_P"],
                                                             p["dt"], rng=rbpf.ReplayRNG(p["U"], p["Z"]))
    for got, k in ((S, "S"), (m, "m"), (pm, "pair_mass")):
        np.testing.assert_array_equal(got, b[k])


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
    r = _runner(rbpf, "mag", "plain")
    T = V.N_T
    for kw in (dict(keep_history=False, trace=True), dict(keep_history=True, trace=False)):
        with r.session(**kw) as s:
            s.advance(T)
            s.sync()
            _refused(rbpf, s.transition_statistics, rbpf.RBPF_ERR_STATE, "keep_history = 1 and trace = 1")
    with r.session() as s:
        _refused(rbpf, s.transition_statistics, rbpf.RBPF_ERR_STATE, "0 of 7 steps are done")       # no history at all
        s.advance(3)
        s.sync()
        _refused(rbpf, s.transition_statistics, rbpf.RBPF_ERR_STATE, "3 of 7 steps are done")
        with pytest.raises(ValueError):
            s.transition_statistics(want=("x_map",))
        s.advance(T - 3)
        good = s.transition_statistics()
    with r.session() as s:                                                # a valid run in the same process afterwards
        s.advance(T)
        again = s.transition_statistics()
    for k in good:
        np.testing.assert_array_equal(again[k], good[k])


def test_refusals_of_the_generic_entry_points(rbpf):
    r = _runner(rbpf, "gauss", "D")
    h, lib, T = r.h, rbpf.load_library(), V.N_T
    rows = (C.c_int32 * 3)(*h.c.rows)
    mask = 4                                                              # rows[2] = state row 3 is the angle
    none8 = (None,) * 8
    base = _live(rbpf)
    with r.session(transition=False) as s:                                # a DeviceMap without a transition
        s.advance(T)
        s.sync()
        _refused(rbpf, s.transition_statistics, rbpf.RBPF_ERR_UNSUPPORTED, "transition density")
    h.reset()
    p = h.c.p
    _refused(rbpf, lambda: rbpf.particleTransitionStatisticsLocalization(h.map(rbpf, transition=False), None, p["odometry"], p["y"], p["x0_nonLin"],
                                                                          p["Q"], p["R"], p["N_P"], p["dt"], rng=rbpf.ReplayRNG(p["U"], p["Z"])),
             rbpf.RBPF_ERR_UNSUPPORTED, "transition density")
    for kw in (dict(keep_history=False, trace=True), dict(keep_history=True, trace=False)):
        with r.session(**kw) as s:
            s.advance(T)
            s.sync()
            _refused(rbpf, s.transition_statistics, rbpf.RBPF_ERR_STATE, "keep_history = 1 and trace = 1")
    with r.session() as s:
        s.advance(2)
        s.sync()
        _refused(rbpf, s.transition_statistics, rbpf.RBPF_ERR_STATE, "2 of 7 steps are done")
        s.advance(T - 2)
        s.sync()
        before = _live(rbpf)
        good = s.transition_statistics(want=MARG + STATS)
        t, xn = C.c_int32(0), C.c_void_p()
        # out of order at the C ABI
        assert lib.rbpf_loc_generic_pair_stats_step_device(s.ctx, None, None) == rbpf.RBPF_ERR_STATE and b"no statistics pass is open" in lib.rbpf_last_error()
        assert lib.rbpf_loc_generic_pair_stats_particles_device(s.ctx, C.byref(t), C.byref(xn)) == rbpf.RBPF_ERR_STATE
        assert lib.rbpf_loc_generic_pair_stats_finish(s.ctx, *none8) == rbpf.RBPF_ERR_STATE
        assert lib.rbpf_loc_generic_pair_stats_begin(s.ctx, 3, rows, mask, 0) == rbpf.RBPF_ERR_INVALID_ARG     # a block that runs past n_sel
        assert lib.rbpf_loc_generic_pair_stats_begin(s.ctx, 3, rows, 8, -1) == rbpf.RBPF_ERR_INVALID_ARG       # an angle bit above n_sel
        assert _live(rbpf) == before
        assert lib.rbpf_loc_generic_pair_stats_begin(s.ctx, 3, rows, mask, -1) == rbpf.RBPF_OK
        assert _live(rbpf) == before + rbpf.device_map_pair_stats_workspace_bytes(4, 3, V.N_P, T)
        assert lib.rbpf_loc_generic_pair_stats_begin(s.ctx, 3, rows, mask, -1) == rbpf.RBPF_ERR_STATE and b"a statistics pass is open" in lib.rbpf_last_error()
        for st in (lib.rbpf_loc_generic_backward_begin(s.ctx, 4, None, 1, 3, rows, mask),                       # nor a backward pass beside it,
                   lib.rbpf_loc_generic_map_begin(s.ctx, 3, rows, mask, -1),                                    # a MAP pass
                   lib.rbpf_loc_generic_marginal_begin(s.ctx, 3, rows, mask, -1)):                              # or a marginal pass
            assert st == rbpf.RBPF_ERR_STATE and b"a statistics pass is open" in lib.rbpf_last_error()
        assert lib.rbpf_loc_generic_marginal_step_device(s.ctx, None, None) == rbpf.RBPF_ERR_STATE            # the marginal family sees no pass of its own
        assert lib.rbpf_loc_generic_pair_stats_particles_device(s.ctx, C.byref(t), C.byref(xn)) == rbpf.RBPF_OK and t.value == T - 2 and xn.value
        assert lib.rbpf_loc_generic_pair_stats_step_device(s.ctx, None, None) == rbpf.RBPF_ERR_INVALID_ARG      # every step needs mu and cov
        bad = np.asfortranarray(np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]]))
        st = lib.rbpf_loc_generic_pair_stats_step_device(s.ctx, xn, bad.ctypes.data_as(C.POINTER(C.c_double)))  # refused before mu is read
        assert st == rbpf.RBPF_ERR_CHOL_FAILED and b"step 5" in lib.rbpf_last_error()
        pm = np.zeros(T - 1)
        assert lib.rbpf_loc_generic_pair_stats_finish(s.ctx, *((None,) * 7), pm.ctypes.data_as(C.POINTER(C.c_double))) == rbpf.RBPF_ERR_STATE
        assert b"steps 5 .. 0 of the statistics pass" in lib.rbpf_last_error()
        assert _live(rbpf) == before                                      # ... and the workspace is back all the same
        # a statistics pass cannot begin while a backward, a MAP or a marginal pass is open
        assert lib.rbpf_loc_generic_backward_begin(s.ctx, 4, None, 1, 3, rows, mask) == rbpf.RBPF_OK
        assert lib.rbpf_loc_generic_pair_stats_begin(s.ctx, 3, rows, mask, -1) == rbpf.RBPF_ERR_STATE and b"a backward pass is open" in lib.rbpf_last_error()
        assert lib.rbpf_loc_generic_backward_finish(s.ctx, None, None, None) == rbpf.RBPF_OK
        assert lib.rbpf_loc_generic_map_begin(s.ctx, 3, rows, mask, -1) == rbpf.RBPF_OK
        assert lib.rbpf_loc_generic_pair_stats_begin(s.ctx, 3, rows, mask, -1) == rbpf.RBPF_ERR_STATE and b"a MAP pass is open" in lib.rbpf_last_error()
        assert lib.rbpf_loc_generic_map_finish(s.ctx, None, None, None) == rbpf.RBPF_OK
        assert lib.rbpf_loc_generic_marginal_begin(s.ctx, 3, rows, mask, -1) == rbpf.RBPF_OK
        assert lib.rbpf_loc_generic_pair_stats_begin(s.ctx, 3, rows, mask, -1) == rbpf.RBPF_ERR_STATE and b"a marginal pass is open" in lib.rbpf_last_error()
        assert lib.rbpf_loc_generic_marginal_finish(s.ctx, *((None,) * 5)) == rbpf.RBPF_OK
        assert _live(rbpf) == before
        st = lib.rbpf_loc_pair_stats_smooth(s.ctx, *none8)                                                      # the dense-mag entry point refuses
        assert st == rbpf.RBPF_ERR_UNSUPPORTED and b"transition density" in lib.rbpf_last_error()
        # a cov that is not positive definite, through the binding: before any handle or kernel runs
        tr = s.map.transition
        s.map.transition = rbpf.DeviceTransition(h.mean, lambda dt, Q: bad, h.c.rows, h.c.angle_rows)
        calls = h.mean_calls
        _refused(rbpf, s.transition_statistics, rbpf.RBPF_ERR_CHOL_FAILED, "step 0")
        assert h.mean_calls == calls
        s.map.transition = tr
        # a `mean` handle that returns the wrong shape, and one that raises at its third call: nothing stays behind
        h.returns = "shape"
        with pytest.raises(ValueError, match="mean returned"):
            s.transition_statistics()
        assert _live(rbpf) == before
        h.returns = None
        import test_gpu_device_map_smoother as GS
        h.mean_calls, h.fail_at = 0, 3
        with pytest.raises(GS.Boom):
            s.transition_statistics()
        assert _live(rbpf) == before
        h.fail_at = None
        again = s.transition_statistics(want=MARG + STATS)                # a valid run afterwards
        for k in MARG + STATS:
            np.testing.assert_array_equal(again[k], good[k])
    with r.session() as s:                                                # rbpf_destroy releases an open pass too
        s.advance(T)
        assert lib.rbpf_loc_generic_pair_stats_begin(s.ctx, 3, rows, mask, -1) == rbpf.RBPF_OK
    assert _live(rbpf) == base
