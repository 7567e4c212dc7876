"""GPU: the fixed-lag smoother (LocalizationSession.fixed_lag_estimates, rbpf_loc_fixed_lag_*, rbpf_loc_generic_fixed_lag_*,
csrc/rbpf_loc_fixedlag.hpp) against the restatement (tests/fixed_lag_ref.py: every sum in long double; full runs against the DIRECT
definition, a backward FFBSm recursion per horizon, not against the forward recursion under test).

Tolerances (TOL = 1e-9, the project's class for this arithmetic).  Probes: tau_next within TOL of max |tau| (one step), |reach - 1|
below TOL where D is finite, everything exactly 0 where it is not; D is the marginal probe's D bit for bit.  Full runs: lag l gets
the factor l (lag 0, one reduction, the factor 1); first moments are measured against sd = max |X - c| of the step they belong to,
second moments against sd^2; |mass - 1| below (steps carried) x TOL.  Two things the bare rule leaves open, decided here:
  * a mean is an fp64 number of the size of the state, not of its spread: every comparison of means carries the format's own term
    4 eps max |X| of the step, and of covariances its square (it matters only where sd < 1e-6 max |X|);
  * a step whose particles are all bit-identical (the committed runs start from one x0 column: step 0) has no spread; its exact
    moments are x0 and 0, and what two paths differ by there is their weights' sum minus 1 (bounded by TOL in the passes' own
    tests) times |x0|: sd is taken as max |X| of the step.

The probe shapes are forward_stats_ref's: 300 x 70 (a ragged successor block; two predecessor chunks of 256, the second with a partial
last tile), 513 x 257 (two successor blocks, three chunks), 1 x 5, 1 x 1, 600 x 520 (three chunks x three blocks); the chunk counts
are asserted from the pass's own rule.  K = 1, KB, KB + 1 and 35 at 300 x 70: one column, a full column block, a block boundary,
dense-mag with covariances.

Measured on an MI355X: the probes' largest errors tau_next 3.0e-12 of the carry's scale (dense-mag, K = 1 and K = 33 at 300 x 70;
2.0e-12 at 600 x 520), the Gaussian and pose terms below 7e-14 (p4a of the sweep), |reach - 1| at most 3.1e-15.  Full runs: every
mean and covariance error, against the direct definition and against smoothed_marginals, lay within the format's term; covariances
beyond it at most 4.3e-16 of sd^2 per lag carried (gauss D); |mass - 1| at most 3.1e-15 per step (mag pages)."""
import ctypes as C
import warnings

import numpy as np
import pytest

import fixed_lag_ref as FL
import map_trajectory_ref as V
import marginal_smoother_ref as G
import transition_sweep_ref as TS

pytestmark = pytest.mark.gpu

TOL = 1e-9
EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble
KB = FL.KB
ALL = ("mean", "cov", "lag_of", "by_lag", "mass")
MOM2 = {("mag", "plain"), ("mag", "pages"), ("gauss", "D"), ("pose", "E")}
LAGS = (1, 3, 6, 9)


def _live(rbpf):
    return int(rbpf.load_library().rbpf_device_bytes_live())


# ------------------------------------------------------------------------------------------------
# 1. the probes
# ------------------------------------------------------------------------------------------------
def _probe(rbpf, p, **kw):
    a = dict(p)
    a.update(kw)
    if a["kind"] == "mag":
        return rbpf.loc_fixed_lag_step(a["X"], a["logw"], a["xs_next"], a["tau"], a["odo"], a["dt"], a["Q"], moments=a.get("moments", 1))[:-1]
    return rbpf.device_map_fixed_lag_step(a["mu"], a["logw"], a["xs_next"], a["tau"], a["cov"], rows=a["rows"], angle_rows=a["angle_rows"],
                                          quat_rows=a["quat_rows"], moments=a.get("moments", 1))[:-1]


def _marginal_D(rbpf, p, **kw):
    a = dict(p)
    a.update(kw)
    if a["kind"] == "mag":
        return rbpf.loc_marginal_step(a["X"], a["logw"], a["xs_next"], a["logws_next"], a["odo"], a["dt"], a["Q"])[0]
    return rbpf.device_map_marginal_step(a["mu"], a["logw"], a["xs_next"], a["logws_next"], a["cov"], rows=a["rows"], angle_rows=a["angle_rows"],
                                         quat_rows=a["quat_rows"])[0]


def _check_carry(got, want, scale, what):
    D, tn, reach = got
    wt, wD = np.asarray(want["tau"], dtype=LD), np.asarray(want["D"], dtype=np.float64)
    assert tn.shape == wt.shape and reach.shape == wD.shape and D.shape == wD.shape
    assert np.all(np.isfinite(tn)) and np.all(np.isfinite(reach))
    fin = wD > -np.inf
    np.testing.assert_array_equal(np.isfinite(D), fin)
    assert np.all(reach[~fin] == 0.0) and np.all(tn[:, ~fin] == 0.0)
    if not fin.any():
        print(f"{what}: every D is -inf, everything exactly 0")
        return 0.0, 0.0
    et = float(np.max(np.abs(tn.astype(LD) - wt))) / scale
    er = float(np.max(np.abs(reach[fin] - 1.0)))
    print(f"{what}: tau_next {et:.2e} of {scale:.3g}, |reach - 1| {er:.2e}")
    assert et <= TOL and er < TOL
    return et, er


def _check_step(rbpf, p, what, **kw):
    """The probe on p (with kw over its inputs) against the restatement of the same inputs; D against the marginal probe's."""
    got = _probe(rbpf, p, **kw)
    q = dict(p)
    q.update(kw)
    if kw:
        lp = G.lp_of_probe(q) if set(kw) - {"logw", "tau", "moments"} else p["lp"]
        want = FL.step(q["logw"], lp, q["tau"])
    else:
        want = p["fl"]
    np.testing.assert_array_equal(got[0], _marginal_D(rbpf, p, **{k: v for k, v in kw.items() if k not in ("tau", "moments")}))
    live = np.asarray(q["logw"]) > -np.inf
    scale = float(np.max(np.abs(np.atleast_2d(q["tau"])[:, live]))) if live.any() else 1.0
    _check_carry(got, want, scale, what)
    return got, want


@pytest.mark.parametrize("family", FL.PROBE_FAMILIES)
@pytest.mark.parametrize("N,M", FL.PROBE_SHAPES)
def test_probe(rbpf, family, N, M):
    assert FL.chunks(300, 70)[1] == 2 and FL.chunks(513, 257)[1] == 3 and FL.chunks(600, 520)[1] == 3   # the pass's own rule
    assert set(FL.PROBE_SHAPES) == {(300, 70), (513, 257), (1, 5), (1, 1), (600, 520)}
    _check_step(rbpf, FL.probe(family, N, M, 3), f"{family} {N} x {M}")


@pytest.mark.parametrize("family", ["mag", "D", "pose3"])
@pytest.mark.parametrize("K", [1, KB, KB + 1, 35])
def test_column_counts(rbpf, family, K):
    """One column, a full block, a block boundary, dense-mag with covariances (7 x 10 / 2 = 35); the enter kernel's moments do not
    show in the outputs."""
    p = FL.probe(family, 300, 70, K)
    got, _ = _check_step(rbpf, p, f"{family}, K = {K}")
    again = _probe(rbpf, p, moments=2)
    for a, b in zip(got, again):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("name", TS.NAMES)
def test_every_term_instantiation(rbpf, name):
    _check_step(rbpf, FL.sweep(name), name)


@pytest.mark.parametrize("family", ["mag", "D", "pose3", "B"])
def test_column_independence(rbpf, family):
    """A column gives the same bits alone, as column 0 of K = KB + 1 and as its last column (a block of one column)."""
    p = FL.probe(family, 300, 70, KB + 1)
    col = p["tau"][5]
    alone = _probe(rbpf, p, tau=col[None, :])
    others = p["tau"][:KB]
    first = _probe(rbpf, p, tau=np.vstack((col[None, :], others)))
    last = _probe(rbpf, p, tau=np.vstack((others, col[None, :])))
    np.testing.assert_array_equal(first[1][0], alone[1][0])
    np.testing.assert_array_equal(last[1][KB], alone[1][0])
    np.testing.assert_array_equal(first[1][1:], last[1][:KB])             # ... and so do the others, one place further on
    for g in (first, last):
        np.testing.assert_array_equal(g[0], alone[0])
        np.testing.assert_array_equal(g[2], alone[2])


def _pred_key(p):
    return "X" if p["kind"] == "mag" else "mu"


@pytest.mark.parametrize("family", ["mag", "D", "pose3", "B"])
def test_minus_infinity_predecessors(rbpf, family):
    """Predecessors with log w = -inf, next to the boundaries of every tile depth (64, 128, 256) too, carrying +-1e300: the answer of
    the inputs without them, finite (0 x inf would be NaN)."""
    N, M, K = 300, 70, KB + 1
    p = FL.probe(family, N, M, K)
    logw, tau = p["logw"].copy(), p["tau"].copy()
    dead = [40, 63, 64, 127, 128, 255, 256]
    logw[dead] = -np.inf
    tau[:, dead] = 1e300
    tau[::2, dead] = -1e300
    got, want = _check_step(rbpf, p, f"{family}, -inf predecessors", logw=logw, tau=tau)
    clean = _probe(rbpf, p, logw=logw)                                   # what they carry changes nothing: bit for bit
    for a, b in zip(got, clean):
        np.testing.assert_array_equal(a, b)
    keep = np.nonzero(logw > -np.inf)[0]
    k = _pred_key(p)
    got2 = _probe(rbpf, p, **{k: p[k][:, keep], "logw": logw[keep], "tau": p["tau"][:, keep]})
    _check_carry(got2, want, float(np.max(np.abs(p["tau"][:, keep]))), f"{family}, without them")


@pytest.mark.parametrize("family", ["mag", "D", "pose3"])
def test_no_live_predecessor(rbpf, family):
    N, M = 300, 70
    p = FL.probe(family, N, M, 3)
    D, tn, reach = _probe(rbpf, p, logw=np.full(N, -np.inf))
    assert np.all(D == -np.inf) and np.all(tn == 0.0) and np.all(reach == 0.0)


# ------------------------------------------------------------------------------------------------
# 2. full runs
# ------------------------------------------------------------------------------------------------
def _runner(rbpf, kind, name):
    import test_gpu_map_trajectory as MT                                  # the sessions of the MAP tests: same cases, same handles
    return MT._runner(rbpf, kind, name)


def _handled(kind):
    return kind in ("gauss", "pose")


def _forget_mean_calls(r, kind):
    if _handled(kind):
        r.h.mean_calls, r.h.mus = 0, []


def _scales(X, W):
    """Per step: (sd, the format's term 4 eps max |X|); sd = max |X - c|, max |X| where every particle of the step is the same."""
    T = X.shape[0]
    sd, fmt = np.zeros(T), np.zeros(T)
    for s in range(T):
        big = float(np.max(np.abs(X[s])))
        tied = bool(np.all(X[s] == X[s][:, :1]))
        sd[s] = big if tied else float(np.max(np.abs(X[s] - (X[s] @ W[s])[:, None])))
        fmt[s] = 4.0 * EPS * big
    return sd, fmt


def _reference(r, kind, X, W, lag, moments):
    c = r.p if kind == "landmark" else r.c
    mus = list(r.h.mus)[:X.shape[0] - 1] if _handled(kind) else None     # in the order it was called: t = 0 .. N_T-2
    return FL.run_full(kind, c, X, W, lag, moments, mus=mus, how=FL.direct)


@pytest.mark.parametrize("kind,name", FL.FULL_RUNS)
def test_full_run(rbpf, kind, name):
    r = _runner(rbpf, kind, name)
    N, T = V.N_P, V.N_T
    moments = 2 if (kind, name) in MOM2 else 1
    want_names = ALL if moments == 2 else tuple(k for k in ALL if k != "cov")
    base = _live(rbpf)
    outs = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        with r.session() as s:
            s.advance(T)
            fwd = s.finish(extras=True)
            xn_fwd = s.history()
            s.sync()
            sm = s.smoothed_marginals(want=("mean", "cov"))
            for lag in LAGS:
                _forget_mean_calls(r, kind)
                outs[lag] = s.fixed_lag_estimates(lag, want=want_names)
                if _handled(kind):
                    assert r.h.mean_calls == T - 1                        # once per step, ascending t (the reference takes them so)
                    if lag == LAGS[0]:
                        mus = list(r.h.mus)
                    calls = r.h.mean_calls
                again = s.fixed_lag_estimates(lag, want=want_names)       # folds nothing
                if _handled(kind):
                    assert r.h.mean_calls == calls
                for k in want_names:
                    np.testing.assert_array_equal(again[k], outs[lag][k])
                s.reset_fixed_lag()
    assert _live(rbpf) == base
    assert fwd["first_degenerate_step"] == -1
    X = np.ascontiguousarray(np.transpose(xn_fwd, (2, 0, 1)))            # [T x n x N], the device's own forward particles
    W = np.ascontiguousarray(fwd["trace_w"].T)
    n = X.shape[1]
    if _handled(kind):
        r.h.mus = mus
    ref = _reference(r, kind, X, W, T - 1, moments)
    sd, fmt = _scales(X, W)
    worst = np.zeros(4)
    for lag in LAGS:
        o = outs[lag]
        assert o["mean"].shape == (n, T) and o["by_lag"].shape == (n, lag + 1, T) and o["mass"].shape == (T,) and o["lag_of"].shape == (T,)
        np.testing.assert_array_equal(o["lag_of"], np.minimum(lag, T - 1 - np.arange(T)))
        assert o["mass"][0] == 1.0
        for t in range(T):
            assert abs(o["mass"][t] - 1.0) < max(t, 1) * TOL
            worst[2] = max(worst[2], abs(o["mass"][t] - 1.0) / max(t, 1))
            for l in range(lag + 1):
                if t - l < 0:
                    assert np.all(np.isnan(o["by_lag"][:, l, t]))
                    continue
                s_ = t - l
                mean, cov = FL.moments_of(ref, l, t)
                f = max(l, 1)
                e = float(np.max(np.abs(o["by_lag"][:, l, t].astype(LD) - mean)))
                assert e <= f * TOL * sd[s_] + fmt[s_], (lag, l, t, e)
                if sd[s_] > 0.0:
                    worst[0] = max(worst[0], e / (f * sd[s_]))
        for s_ in range(T):
            l = int(o["lag_of"][s_])
            np.testing.assert_array_equal(o["mean"][:, s_], o["by_lag"][:, l, s_ + l])
            f = max(l, 1)
            if moments == 2:
                mean, cov = FL.moments_of(ref, l, s_ + l)
                np.testing.assert_array_equal(o["cov"][:, :, s_], o["cov"][:, :, s_].T)
                e = float(np.max(np.abs(o["cov"][:, :, s_].astype(LD) - cov)))
                assert e <= f * TOL * sd[s_] ** 2 + fmt[s_] ** 2, (lag, s_, e)
                if sd[s_] > 0.0:
                    worst[1] = max(worst[1], e / (f * sd[s_] ** 2))
        # two device paths, one estimator: the horizon T - 1 is smoothed_marginals of the finished run
        for l in range(min(lag, T - 1) + 1):
            s_ = T - 1 - l
            f = max(l, 1)
            e = float(np.max(np.abs(o["by_lag"][:, l, T - 1] - sm["mean"][:, s_])))
            assert e <= f * TOL * sd[s_] + fmt[s_], (lag, l, e)
            if sd[s_] > 0.0:
                worst[3] = max(worst[3], e / (f * sd[s_]))
            if moments == 2 and int(o["lag_of"][s_]) == l:
                e = float(np.max(np.abs(o["cov"][:, :, s_] - sm["cov"][:, :, s_])))
                assert e <= f * TOL * sd[s_] ** 2 + fmt[s_] ** 2, (lag, l, e)
        # ... and lag 0 is the filter's weighted mean
        for t in range(T):
            e = float(np.max(np.abs(o["by_lag"][:, 0, t] - X[t] @ W[t])))
            assert e <= TOL * sd[t] + fmt[t]
    print(f"{kind} {name}: worst per lag carried: mean {worst[0]:.2e} of sd, cov {worst[1]:.2e} of sd^2, |mass - 1| {worst[2]:.2e} per step, "
          f"mean against smoothed_marginals {worst[3]:.2e} of sd")
    # a column does not depend on the lag of the carry: bit for bit
    np.testing.assert_array_equal(outs[6]["by_lag"][:, :4, :], outs[3]["by_lag"])
    np.testing.assert_array_equal(outs[9]["by_lag"][:, :7, :], outs[6]["by_lag"])
    np.testing.assert_array_equal(outs[3]["by_lag"][:, :2, :], outs[1]["by_lag"])
    assert np.all(np.isnan(outs[9]["by_lag"][:, 7:, :]))


def _stated_bytes(rbpf, s, lag, moments):
    if s.driver is None:
        return rbpf.loc_fixed_lag_workspace_bytes(V.N_P, V.N_T, lag, moments)
    rows, _, qpos, _ = s.map.transition.layout(s.nN)
    return rbpf.device_map_fixed_lag_workspace_bytes(s.nN, len(rows), V.N_P, V.N_T, lag, moments, quat_pos=qpos)


@pytest.mark.parametrize("kind,name,lag,moments", [("mag", "pages", 2, 2), ("gauss", "D", 3, 1), ("pose", "E", 2, 2)])
def test_incremental_equals_one_shot(rbpf, kind, name, lag, moments):
    r = _runner(rbpf, kind, name)
    T = V.N_T
    names = ALL if moments == 2 else tuple(k for k in ALL if k != "cov")
    base = _live(rbpf)
    with r.session() as s:
        s.advance(3)
        s.sync()
        before = _live(rbpf)
        _forget_mean_calls(r, kind)
        first = s.fixed_lag_estimates(lag, want=names)
        if _handled(kind):
            assert r.h.mean_calls == 2
        assert first["mean"].shape[1] == 3 and first["mass"].shape == (3,)
        with_carry = _live(rbpf)
        assert with_carry == before + _stated_bytes(rbpf, s, lag, moments)    # exactly the stated bytes while the carry lives
        s.advance(4)
        s.sync()
        grown = _live(rbpf) - with_carry                                  # (what the filter's own steps took, if anything)
        _forget_mean_calls(r, kind)
        second = s.fixed_lag_estimates(lag, want=names)
        if _handled(kind):
            assert r.h.mean_calls == 4                                    # once per newly folded step
        assert _live(rbpf) == with_carry + grown
        means_only = s.fixed_lag_estimates(lag)                           # the carry keeps its moments; the default names the mean
        assert set(means_only) == {"mean"}
        np.testing.assert_array_equal(means_only["mean"], second["mean"])
        s.reset_fixed_lag()
        assert _live(rbpf) == before + grown
        third = s.fixed_lag_estimates(lag, want=names)                    # from an empty carry again
        assert _live(rbpf) == with_carry + grown
    assert _live(rbpf) == base                                            # close hands the carry back too
    with r.session() as s:
        s.advance(T)
        fresh = s.fixed_lag_estimates(lag, want=names)
    assert _live(rbpf) == base
    final = first["lag_of"] == lag
    assert final.sum() == 3 - lag and not final[-1]
    for k in ("mean", "cov"):
        if k in names:
            np.testing.assert_array_equal(second[k][..., :3][..., final], first[k][..., final])      # final columns stay
    np.testing.assert_array_equal(second["by_lag"][:, :, :3], first["by_lag"])
    np.testing.assert_array_equal(second["mass"][:3], first["mass"])
    for k in names:
        np.testing.assert_array_equal(second[k], fresh[k])
        np.testing.assert_array_equal(third[k], fresh[k])


def test_the_other_passes_are_left_as_they_were(rbpf):
    MARG = ("w_smooth", "mean", "cov", "ess", "mass")
    RUN = ("S_run", "m_run", "mass_run", "tau_S", "tau_m")
    for kind, name in (("mag", "pages"), ("pose", "E")):
        r = _runner(rbpf, kind, name)
        with r.session() as s:
            s.advance(V.N_T)
            sm0 = s.smoothed_marginals(want=MARG)
            bs0 = s.backward_simulate(16, rng=rbpf.PhiloxRNG(5))
            mt0 = s.map_trajectory()
            rs0 = s.running_statistics(want=RUN)
            s.reset_running_statistics()
            fl0 = s.fixed_lag_estimates(3, want=ALL)
            sm1 = s.smoothed_marginals(want=MARG)                         # with the fixed-lag carry alive
            bs1 = s.backward_simulate(16, rng=rbpf.PhiloxRNG(5))
            mt1 = s.map_trajectory()
            rs1 = s.running_statistics(want=RUN)                          # ... and a ForwardCarry beside it
            fl1 = s.fixed_lag_estimates(3, want=ALL)
        for a, b in ((sm0, sm1), (bs0, bs1), (rs0, rs1), (fl0, fl1)):
            for k in a:
                np.testing.assert_array_equal(b[k], a[k])
        for k in ("x_map", "index"):
            np.testing.assert_array_equal(mt1[k], mt0[k])
        assert mt1["score"] == mt0["score"]


def test_one_shot_equals_the_session(rbpf):
    c = V.mag_case("pages")                                               # dt and Q in pages
    r = _runner(rbpf, "mag", "pages")
    with r.session() as s:
        s.advance(V.N_T)
        a = s.fixed_lag_estimates(2, want=ALL)
    mp = rbpf.DenseMagMap(rbpf.DenseMagModel(c["NN"], c["L"]), c["mean"], c["V"], c["sigma2"])
    mean, cov, lag_of, ex = rbpf.particleFixedLagSmootherLocalization(mp.dynModel, mp.measModel, c["odometry"], c["y"], c["x0_nonLin"], c["Q"],
                                                                      np.eye(3), c["N_P"], c["dt"], 2, rng=rbpf.ReplayRNG(c["U"], c["Z"]),
                                                                      every=2, extras=True)
    for got, k in ((mean, "mean"), (cov, "cov"), (lag_of, "lag_of"), (ex["by_lag"], "by_lag"), (ex["mass"], "mass")):
        np.testing.assert_array_equal(got, a[k])
    assert ex["traj_max"].shape == (7, V.N_T) and mean.shape == (7, V.N_T) and cov.shape == (7, 7, V.N_T)


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
            _refused(rbpf, lambda: s.fixed_lag_estimates(2), rbpf.RBPF_ERR_STATE, "keep_history = 1 and trace = 1")
    with r.session() as s:
        _refused(rbpf, lambda: s.fixed_lag_estimates(2), rbpf.RBPF_ERR_STATE, "0 steps are done")
        s.advance(1)
        s.sync()
        _refused(rbpf, lambda: s.fixed_lag_estimates(2), rbpf.RBPF_ERR_STATE, "1 steps are done")
        with pytest.raises(ValueError):
            s.fixed_lag_estimates(2, want=("S",))
        s.reset_fixed_lag()                                               # no carry: nothing happens
        s.advance(1)
        s.sync()
        _refused(rbpf, lambda: s.fixed_lag_estimates(0), rbpf.RBPF_ERR_INVALID_ARG, "lag must be in 1 .. 64")
        _refused(rbpf, lambda: s.fixed_lag_estimates(-1), rbpf.RBPF_ERR_INVALID_ARG, "lag must be in 1 .. 64")
        assert s.fixed_lag_estimates(2, want=("mass",))["mass"].shape == (2,)       # 2 steps are enough
        _refused(rbpf, lambda: s.fixed_lag_estimates(3), rbpf.RBPF_ERR_STATE, "built with lag = 2, moments = 1")
        _refused(rbpf, lambda: s.fixed_lag_estimates(2, want=("cov",)), rbpf.RBPF_ERR_STATE, "built with lag = 2, moments = 1")
        s.reset_fixed_lag()
        assert s.fixed_lag_estimates(3, want=("cov",))["cov"].shape == (7, 7, 2)
        lib = rbpf.load_library()
        assert lib.rbpf_loc_generic_fixed_lag_begin(s.ctx, 1, (C.c_int32 * 1)(0), 0, -1, 2, 1) == rbpf.RBPF_ERR_INVALID_ARG   # not a generic context


def test_refusals_of_the_generic_entry_points(rbpf):
    r = _runner(rbpf, "gauss", "D")
    h, lib, T = r.h, rbpf.load_library(), V.N_T
    rows = (C.c_int32 * 3)(*h.c.rows)
    mask = 4                                                              # rows[2] = state row 3 is the angle
    base = _live(rbpf)
    with r.session(transition=False) as s:                                # a DeviceMap without a transition
        s.advance(T)
        s.sync()
        _refused(rbpf, lambda: s.fixed_lag_estimates(2), rbpf.RBPF_ERR_UNSUPPORTED, "transition density")
    h.reset()
    p = h.c.p
    _refused(rbpf, lambda: rbpf.particleFixedLagSmootherLocalization(h.map(rbpf, transition=False), None, p["odometry"], p["y"], p["x0_nonLin"],
                                                                      p["Q"], p["R"], p["N_P"], p["dt"], 2, rng=rbpf.ReplayRNG(p["U"], p["Z"])),
             rbpf.RBPF_ERR_UNSUPPORTED, "transition density")
    for kw in (dict(keep_history=False, trace=True), dict(keep_history=True, trace=False)):
        with r.session(**kw) as s:
            s.advance(T)
            s.sync()
            _refused(rbpf, lambda: s.fixed_lag_estimates(2), rbpf.RBPF_ERR_STATE, "keep_history = 1 and trace = 1")
    with r.session() as s:
        _refused(rbpf, lambda: s.fixed_lag_estimates(2), rbpf.RBPF_ERR_STATE, "0 steps are done")
        s.advance(1)
        s.sync()
        _refused(rbpf, lambda: s.fixed_lag_estimates(2), rbpf.RBPF_ERR_STATE, "1 steps are done")
    with r.session() as s:                                                # the undisturbed session the disturbed one must end equal to
        s.advance(T)
        good = s.fixed_lag_estimates(2, want=("mean", "lag_of", "by_lag", "mass"))
    with r.session() as s:
        s.advance(T)
        s.sync()
        before = _live(rbpf)
        t, xn = C.c_int32(0), C.c_void_p()
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))            # noqa: E731
        eye = np.asfortranarray(np.eye(3))
        # out of order at the C ABI
        assert lib.rbpf_loc_generic_fixed_lag_step_device(s.ctx, None, None) == rbpf.RBPF_ERR_STATE
        assert b"no fixed-lag stepping is open" in lib.rbpf_last_error()
        assert lib.rbpf_loc_generic_fixed_lag_particles_device(s.ctx, C.byref(t), C.byref(xn)) == rbpf.RBPF_ERR_STATE
        assert lib.rbpf_loc_generic_fixed_lag_finish(s.ctx, None, None) == rbpf.RBPF_ERR_STATE
        assert lib.rbpf_loc_generic_fixed_lag_begin(s.ctx, 3, rows, mask, 0, 2, 1) == rbpf.RBPF_ERR_INVALID_ARG    # a block that runs past n_sel
        assert lib.rbpf_loc_generic_fixed_lag_begin(s.ctx, 3, rows, mask, -1, 0, 1) == rbpf.RBPF_ERR_INVALID_ARG   # lag < 1
        assert lib.rbpf_loc_generic_fixed_lag_begin(s.ctx, 3, rows, mask, -1, 2, 3) == rbpf.RBPF_ERR_INVALID_ARG   # moments
        assert lib.rbpf_loc_generic_fixed_lag_reset(s.ctx) == rbpf.RBPF_OK                                         # no carry: nothing happens
        assert _live(rbpf) == before
        assert lib.rbpf_loc_generic_fixed_lag_begin(s.ctx, 3, rows, mask, -1, 2, 1) == rbpf.RBPF_OK
        carry = rbpf.device_map_fixed_lag_workspace_bytes(4, 3, V.N_P, T, 2, 1)
        assert _live(rbpf) == before + carry
        assert lib.rbpf_loc_generic_fixed_lag_begin(s.ctx, 3, rows, mask, -1, 2, 1) == rbpf.RBPF_ERR_STATE         # a second begin
        assert b"a fixed-lag stepping is open" in lib.rbpf_last_error()
        for st in (lib.rbpf_loc_generic_backward_begin(s.ctx, 4, None, 1, 3, rows, mask),                          # nor one of the other five
                   lib.rbpf_loc_generic_map_begin(s.ctx, 3, rows, mask, -1),
                   lib.rbpf_loc_generic_marginal_begin(s.ctx, 3, rows, mask, -1),
                   lib.rbpf_loc_generic_pair_stats_begin(s.ctx, 3, rows, mask, -1),
                   lib.rbpf_loc_generic_forward_stats_begin(s.ctx, 3, rows, mask, -1),
                   lib.rbpf_loc_generic_fixed_lag_reset(s.ctx)):                                                   # nor a reset
            assert st == rbpf.RBPF_ERR_STATE and b"a fixed-lag stepping is open" in lib.rbpf_last_error()
        assert _live(rbpf) == before + carry
        assert lib.rbpf_loc_generic_fixed_lag_particles_device(s.ctx, C.byref(t), C.byref(xn)) == rbpf.RBPF_OK and t.value == 0 and xn.value
        assert lib.rbpf_loc_generic_fixed_lag_step_device(s.ctx, None, None) == rbpf.RBPF_ERR_INVALID_ARG          # every step needs mu and cov
        bad = np.asfortranarray(np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]]))
        st = lib.rbpf_loc_generic_fixed_lag_step_device(s.ctx, xn, dp(bad))                                        # refused before mu is read
        assert st == rbpf.RBPF_ERR_CHOL_FAILED and b"step 0" in lib.rbpf_last_error()
        pg = np.zeros((3 * 4 + 1) * T)
        assert lib.rbpf_loc_generic_fixed_lag_finish(s.ctx, dp(pg), None) == rbpf.RBPF_ERR_STATE
        assert b"from 1 on were not folded in" in lib.rbpf_last_error()
        assert lib.rbpf_loc_generic_fixed_lag_finish(s.ctx, None, None) == rbpf.RBPF_ERR_STATE                     # ... and the stepping is closed
        assert _live(rbpf) == before + carry                                                                       # the carry stays
        # with another lag, other moments or other rows than the carry was built with: reset first
        assert lib.rbpf_loc_generic_fixed_lag_begin(s.ctx, 3, rows, mask, -1, 3, 1) == rbpf.RBPF_ERR_STATE and b"built with lag = 2" in lib.rbpf_last_error()
        assert lib.rbpf_loc_generic_fixed_lag_begin(s.ctx, 3, rows, mask, -1, 2, 2) == rbpf.RBPF_ERR_STATE and b"moments = 1" in lib.rbpf_last_error()
        assert lib.rbpf_loc_generic_fixed_lag_begin(s.ctx, 2, rows, 0, -1, 2, 1) == rbpf.RBPF_ERR_STATE and b"other rows" in lib.rbpf_last_error()
        # this stepping cannot begin while one of the other five is open (the carry alive or not)
        none5 = (None,) * 5
        for begin, finish, what in ((lambda: lib.rbpf_loc_generic_backward_begin(s.ctx, 4, None, 1, 3, rows, mask),
                                     lambda: lib.rbpf_loc_generic_backward_finish(s.ctx, None, None, None), b"a backward pass is open"),
                                    (lambda: lib.rbpf_loc_generic_map_begin(s.ctx, 3, rows, mask, -1),
                                     lambda: lib.rbpf_loc_generic_map_finish(s.ctx, None, None, None), b"a MAP pass is open"),
                                    (lambda: lib.rbpf_loc_generic_marginal_begin(s.ctx, 3, rows, mask, -1),
                                     lambda: lib.rbpf_loc_generic_marginal_finish(s.ctx, *none5), b"a marginal pass is open"),
                                    (lambda: lib.rbpf_loc_generic_pair_stats_begin(s.ctx, 3, rows, mask, -1),
                                     lambda: lib.rbpf_loc_generic_pair_stats_finish(s.ctx, *((None,) * 8)), b"a statistics pass is open"),
                                    (lambda: lib.rbpf_loc_generic_forward_stats_begin(s.ctx, 3, rows, mask, -1),
                                     lambda: lib.rbpf_loc_generic_forward_stats_finish(s.ctx, *none5), b"a running-statistics stepping is open")):
            assert begin() == rbpf.RBPF_OK
            assert lib.rbpf_loc_generic_fixed_lag_begin(s.ctx, 3, rows, mask, -1, 2, 1) == rbpf.RBPF_ERR_STATE and what in lib.rbpf_last_error()
            assert finish() == rbpf.RBPF_OK
        assert lib.rbpf_loc_generic_forward_stats_reset(s.ctx) == rbpf.RBPF_OK                                     # (the running statistics' carry)
        assert _live(rbpf) == before + carry
        st = lib.rbpf_loc_fixed_lag_update(s.ctx, 2, 1, None, None)                                                # the dense-mag entry point refuses
        assert st == rbpf.RBPF_ERR_UNSUPPORTED and b"transition density" in lib.rbpf_last_error()
        assert lib.rbpf_loc_fixed_lag_reset(s.ctx) == rbpf.RBPF_ERR_INVALID_ARG
        assert lib.rbpf_loc_generic_fixed_lag_reset(s.ctx) == rbpf.RBPF_OK
        assert _live(rbpf) == before
        # a `mean` handle that returns the wrong shape: the stepping is closed, the carry (step 0 alone) stays
        h.returns = "shape"
        with pytest.raises(ValueError, match="mean returned"):
            s.fixed_lag_estimates(2)
        assert _live(rbpf) == before + carry
        h.returns = None
        s.reset_fixed_lag()
        # ... and one that raises at its third call: two steps are folded in, a valid call resumes there
        import test_gpu_device_map_smoother as GS
        h.mean_calls, h.fail_at = 0, 3
        with pytest.raises(GS.Boom):
            s.fixed_lag_estimates(2)
        assert _live(rbpf) == before + carry
        h.fail_at = None
        h.mean_calls = 0
        again = s.fixed_lag_estimates(2, want=("mean", "lag_of", "by_lag", "mass"))
        assert h.mean_calls == T - 1 - 2                                  # steps 2 .. N_T-2 only
        for k in again:
            np.testing.assert_array_equal(again[k], good[k])
    assert _live(rbpf) == base
    with r.session() as s:                                                # rbpf_destroy releases a living carry and an open stepping
        s.advance(T)
        assert lib.rbpf_loc_generic_fixed_lag_begin(s.ctx, 3, rows, mask, -1, 2, 1) == rbpf.RBPF_OK
    assert _live(rbpf) == base
