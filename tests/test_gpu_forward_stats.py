"""GPU: the running two-slice statistics (LocalizationSession.running_statistics, rbpf_loc_forward_stats_*,
rbpf_loc_generic_forward_stats_*, csrc/rbpf_loc_forwardstats.hpp) against the restatement (tests/forward_stats_ref.py: every sum in
long double, the residuals from pair_stats_ref, D from marginal_smoother_ref.step).

Tolerances (TOL = 1e-9, the project's class for this arithmetic, as tests/test_gpu_pair_stats.py): tau_S and the pages' S within TOL
of max |S_ref| of the step (over every successor for tau, of the page for a page); tau_m and m within TOL of the square root of that
scale; |reach - 1| and |mass - 1| below TOL wherever D is finite (reach exactly 0 where it is not).  In full runs page k gets the
factor k + 1: the error is carried forward one step at a time.  D of the probes is the marginal probes' D bit for bit: the same kernels
produce it.

The probe shapes are the smallest at which the pass can go wrong: 300 x 70 (a ragged successor block; two predecessor chunks of 256,
the second with a partial last tile at every tile depth), 513 x 257 (two successor blocks, three chunks), 1 x 5 and 1 x 1, 600 x 520
(three chunks x three blocks).  The chunk counts are asserted from the pass's own rule (forward_stats_ref.chunks).

Measured on an MI355X: the probes' largest errors tau_S 3.8e-12 (dense-mag, 600 x 520), tau_m 3.9e-12 (dense-mag, 300 x 70),
|reach - 1| 1.6e-13 (dense-mag, the duplicated dominant predecessor), all of their scales; the Gaussian and pose terms stay below
1.8e-13.  Full runs, per step carried: S at most 8.5e-16, m 9.5e-16 (the landmark map), |mass - 1| 3.1e-15; the last page against the
same session's transition_statistics: S at most 7.2e-16, m 3.3e-15."""
import ctypes as C
import warnings

import numpy as np
import pytest

import forward_stats_ref as FS
import map_trajectory_ref as V
import marginal_smoother_ref as G
import pair_stats_ref as PS
import transition_sweep_ref as TS

pytestmark = pytest.mark.gpu

TOL = 1e-9
LD = np.longdouble
NAMES = ("S_run", "m_run", "mass_run", "tau_S", "tau_m")


def _live(rbpf):
    return int(rbpf.load_library().rbpf_device_bytes_live())


# ------------------------------------------------------------------------------------------------
# 1. the probes
# ------------------------------------------------------------------------------------------------
def _probe(rbpf, p, **kw):
    a = dict(p)
    a.update(kw)
    if a["kind"] == "mag":
        return rbpf.loc_forward_stats_step(a["X"], a["logw"], a["xs_next"], a["tau_S"], a["tau_m"], a["odo"], a["dt"], a["Q"])[:-1]
    return rbpf.device_map_forward_stats_step(a["mu"], a["logw"], a["xs_next"], a["tau_S"], a["tau_m"], a["cov"], rows=a["rows"],
                                              angle_rows=a["angle_rows"], quat_rows=a["quat_rows"], s_scale=a["s_scale"])[:-1]


def _marginal_D(rbpf, p, **kw):
    a = dict(p)
    a.update(kw)
    if a["kind"] == "mag":
        return rbpf.loc_marginal_step(a["X"], a["logw"], a["xs_next"], a["logws_next"], a["odo"], a["dt"], a["Q"])[0]
    return rbpf.device_map_marginal_step(a["mu"], a["logw"], a["xs_next"], a["logws_next"], a["cov"], rows=a["rows"], angle_rows=a["angle_rows"],
                                         quat_rows=a["quat_rows"])[0]


def _check_carry(got, want, what, factor=1.0):
    """(D, tau_S, tau_m, reach) of a probe against the restatement's step; returns the three errors."""
    D, tS, tm, reach = got
    wS, wm, wD = np.asarray(want["tau_S"], dtype=LD), np.asarray(want["tau_m"], dtype=LD), np.asarray(want["D"], dtype=np.float64)
    assert tS.shape == wS.shape and tm.shape == wm.shape and reach.shape == wD.shape
    assert np.all(np.isfinite(tS)) and np.all(np.isfinite(tm)) and np.all(np.isfinite(reach))
    np.testing.assert_array_equal(tS, tS.transpose(1, 0, 2))              # both triangles come from one sum
    fin = wD > -np.inf
    np.testing.assert_array_equal(np.isfinite(D), fin)
    assert np.all(reach[~fin] == 0.0) and np.all(tS[:, :, ~fin] == 0.0) and np.all(tm[:, ~fin] == 0.0)
    if not fin.any():
        print(f"{what}: every D is -inf, everything exactly 0")
        return 0.0, 0.0, 0.0
    sS = float(np.max(np.abs(wS)))
    sm = float(np.sqrt(sS))
    eS = float(np.max(np.abs(tS.astype(LD) - wS))) / sS
    em = float(np.max(np.abs(tm.astype(LD) - wm))) / sm
    er = float(np.max(np.abs(reach[fin] - 1.0)))
    print(f"{what}: tau_S {eS:.2e} of {sS:.3g}, tau_m {em:.2e} of {sm:.3g}, |reach - 1| {er:.2e}")
    assert eS <= factor * TOL and em <= factor * TOL and er < factor * TOL
    return eS, em, er


def _check_step(rbpf, p, what, **kw):
    """The probe on p (with kw over its inputs) against the restatement of the same inputs; D against the marginal probe's."""
    got = _probe(rbpf, p, **kw)
    if kw:
        q = dict(p)
        q.update(kw)
        lp = G.lp_of_probe(q) if set(kw) - {"logw", "tau_S", "tau_m", "s_scale"} else p["lp"]
        want = FS.step(q["logw"], lp, (q["tau_S"], q["tau_m"]), PS.r_of_probe(q), q["s_scale"])
    else:
        want = p["fs"]
    np.testing.assert_array_equal(got[0], _marginal_D(rbpf, p, **{k: v for k, v in kw.items() if k not in ("tau_S", "tau_m", "s_scale")}))
    _check_carry(got, want, what)
    return got, want


@pytest.mark.parametrize("family", FS.PROBE_FAMILIES)
@pytest.mark.parametrize("N,M", FS.PROBE_SHAPES)
def test_probe(rbpf, family, N, M):
    assert FS.chunks(300, 70)[1] == 2 and FS.chunks(513, 257)[1] == 3 and FS.chunks(600, 520)[1] == 3   # the pass's own rule
    assert (300, 70) in FS.PROBE_SHAPES and (513, 257) in FS.PROBE_SHAPES and (1, 5) in FS.PROBE_SHAPES and (1, 1) in FS.PROBE_SHAPES
    _check_step(rbpf, FS.probe(family, N, M), f"{family} {N} x {M}")


@pytest.mark.parametrize("name", TS.NAMES)
def test_every_term_instantiation(rbpf, name):
    """tau in the CALLER's residual order on the way in and out: a wrong (un-)permutation behind a quaternion block shows here."""
    _check_step(rbpf, FS.sweep(name), name)


def _pred_key(p):
    return "X" if p["kind"] == "mag" else "mu"


@pytest.mark.parametrize("family", ["mag", "D", "pose3", "B"])
def test_minus_infinity_predecessors(rbpf, family):
    """Predecessors with log w = -inf, next to the tile boundaries of every tile depth (64, 128, 256) too, carrying garbage: the answer
    of the inputs without them."""
    N, M = 300, 70
    p = FS.probe(family, N, M)
    logw, tS, tm = p["logw"].copy(), p["tau_S"].copy(), p["tau_m"].copy()
    dead = [40, 63, 64, 127, 128, 255, 256]
    logw[dead] = -np.inf
    tS[:, :, dead], tm[:, dead] = 1e300, -1e300                          # what they carry must not matter (no 0 * inf)
    got, want = _check_step(rbpf, p, f"{family}, -inf predecessors", logw=logw, tau_S=tS, tau_m=tm)
    keep = np.nonzero(logw > -np.inf)[0]
    k = _pred_key(p)
    got2 = _probe(rbpf, p, **{k: p[k][:, keep], "logw": logw[keep], "tau_S": p["tau_S"][:, :, keep], "tau_m": p["tau_m"][:, keep]})
    _check_carry(got2, want, f"{family}, without them")


@pytest.mark.parametrize("family", ["mag", "D", "pose3"])
def test_no_live_predecessor(rbpf, family):
    N, M = 300, 70
    p = FS.probe(family, N, M)
    D, tS, tm, reach = _probe(rbpf, p, logw=np.full(N, -np.inf))
    assert np.all(D == -np.inf)
    assert np.all(tS == 0.0) and np.all(tm == 0.0) and np.all(reach == 0.0)


@pytest.mark.parametrize("family,N,M", [("mag", 300, 70), ("D", 300, 70), ("pose3", 300, 70), ("mag", 513, 257), ("B", 513, 257)])
def test_a_dominant_predecessor_and_its_duplicate(rbpf, family, N, M):
    """One predecessor 600 above the rest: tau_next(j) = tau(i0) + s(i0, j) for every j.  The same with a bit-identical duplicate at
    weight 1/2 each: in another tile at 300 (30 and 280) and in another chunk at 513 (30 and 493)."""
    p = FS.probe(family, N, M)
    k = _pred_key(p)
    i0, i1 = 30, N - 20
    logw = p["logw"].copy()
    logw[i0] = 600.0
    got, want = _check_step(rbpf, p, f"{family} {N} x {M}, one", logw=logw)
    r_of = PS.r_of_probe(p)
    wS = np.stack([p["tau_S"][:, :, i0].astype(LD) + LD(p["s_scale"]) * np.outer(r_of(j)[:, i0], r_of(j)[:, i0]) for j in range(M)], axis=2)
    wm = np.stack([p["tau_m"][:, i0].astype(LD) + r_of(j)[:, i0] for j in range(M)], axis=1)
    sS = float(np.max(np.abs(wS)))
    assert float(np.max(np.abs(got[1] - wS))) <= TOL * sS and float(np.max(np.abs(got[2] - wm))) <= TOL * np.sqrt(sS)
    pred, tS, tm = p[k].copy(), p["tau_S"].copy(), p["tau_m"].copy()
    pred[:, i1], tS[:, :, i1], tm[:, i1] = pred[:, i0], tS[:, :, i0], tm[:, i0]
    logw[i1] = 600.0
    got2, _ = _check_step(rbpf, p, f"{family} {N} x {M}, two", **{k: pred, "logw": logw, "tau_S": tS, "tau_m": tm})
    assert float(np.max(np.abs(got2[1] - wS))) <= TOL * sS and float(np.max(np.abs(got2[2] - wm))) <= TOL * np.sqrt(sS)


@pytest.mark.parametrize("family", ["D", "pose3"])
def test_s_scale_zero_carries_the_S_part_through(rbpf, family):
    """s_scale = 0: the S part of tau_next is the plain omega-average of the incoming tau_S."""
    N, M = 300, 70
    p = FS.probe(family, N, M)
    got, want = _check_step(rbpf, p, f"{family}, s_scale = 0", s_scale=0.0)
    logw, lp = np.asarray(p["logw"], dtype=LD), np.asarray(p["lp"], dtype=LD)
    live = np.nonzero(logw > -np.inf)[0]
    for j in (0, 33, M - 1):
        w = np.exp(logw[live] + lp[live, j] - want["D"][j])
        avg = np.sum(p["tau_S"][:, :, live].astype(LD) * w[None, None, :], axis=2)
        assert float(np.max(np.abs(got[1][:, :, j] - avg))) <= TOL * float(np.max(np.abs(want["tau_S"])))


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


def _reference(r, kind, X, W):
    if kind == "mag":
        return FS.run_mag(r.c, X, W)
    if kind == "landmark":
        return FS.run_landmark(r.p, X, W)
    return FS.run_case(r.c, X, W, mus=list(r.h.mus))                      # in the order it was called: t = 0 .. N_T-2


def _dts(r, kind, T):
    if kind == "mag":
        return V.pages(r.c, T)[0][:T - 1]
    return FS.steps_dt((r.p if kind == "landmark" else r.c.p)["dt"], T)


def _check_page(S, m, mass, wS, wm, what, factor):
    wS, wm = np.asarray(wS, dtype=LD), np.asarray(wm, dtype=LD)
    np.testing.assert_array_equal(S, S.T)
    sS = float(np.max(np.abs(wS)))
    sm = float(np.sqrt(sS))
    eS = float(np.max(np.abs(S.astype(LD) - wS))) / sS
    em = float(np.max(np.abs(m.astype(LD) - wm))) / sm
    ep = abs(float(mass) - 1.0)
    print(f"{what}: S {eS:.2e} of {sS:.3g}, m {em:.2e} of {sm:.3g}, |mass - 1| {ep:.2e}")
    assert eS <= factor * TOL and em <= factor * TOL and ep < factor * TOL
    return eS, em, ep


@pytest.mark.parametrize("kind,name", FS.FULL_RUNS)
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
            _forget_mean_calls(r, kind)
            out = s.running_statistics(want=NAMES)
            if _handled(kind):
                assert r.h.mean_calls == T - 1                            # once per step, ascending t (the reference takes them so)
            X = np.ascontiguousarray(np.transpose(xn_fwd, (2, 0, 1)))    # [T x n x N], the device's own forward particles
            W = np.ascontiguousarray(fwd["trace_w"].T)
            res = _reference(r, kind, X, W)
            calls = r.h.mean_calls if _handled(kind) else 0
            again = s.running_statistics(want=NAMES)                      # folds nothing
            if _handled(kind):
                assert r.h.mean_calls == calls
            default = s.running_statistics()
            off = s.transition_statistics(want=("S", "m"))
    assert _live(rbpf) == base
    assert fwd["first_degenerate_step"] == -1
    n = res["S_run"].shape[1]
    assert out["S_run"].shape == (n, n, T - 1) and out["m_run"].shape == (n, T - 1) and out["mass_run"].shape == (T - 1,)
    assert out["tau_S"].shape == (n, n, N) and out["tau_m"].shape == (n, N)
    worst = np.zeros(3)
    for k in range(T - 1):
        e = _check_page(np.ascontiguousarray(out["S_run"][:, :, k]), out["m_run"][:, k].copy(), out["mass_run"][k], res["S_run"][k], res["m_run"][k],
                        f"{kind} {name} page {k}", factor=k + 1)
        worst = np.maximum(worst, np.array(e) / (k + 1))
    print(f"{kind} {name}: worst per step carried: S {worst[0]:.2e}, m {worst[1]:.2e}, |mass - 1| {worst[2]:.2e}")
    tS, tm = res["taus"][-1]
    sS = float(np.max(np.abs(tS)))
    assert float(np.max(np.abs(out["tau_S"] - tS))) <= (T - 1) * TOL * sS and float(np.max(np.abs(out["tau_m"] - tm))) <= (T - 1) * TOL * np.sqrt(sS)
    # two device paths, one identity: the last page is the offline pass's sum_t S_t / dt_t and sum_t m_t
    dt = _dts(r, kind, T)
    wS = np.sum(off["S"].astype(LD) / dt.astype(LD)[None, None, :], axis=2)
    wm = np.sum(off["m"].astype(LD), axis=1)
    _check_page(np.ascontiguousarray(out["S_run"][:, :, -1]), out["m_run"][:, -1].copy(), out["mass_run"][-1], wS, wm,
                f"{kind} {name} last page against transition_statistics", factor=T - 1)
    for k in NAMES:                                                       # two calls in a row: bit-identical
        np.testing.assert_array_equal(again[k], out[k])
    assert set(default) == {"S_run", "m_run"}
    for k in default:
        np.testing.assert_array_equal(default[k], out[k])
    Qh, bias = rbpf.running_noise_estimate(out["S_run"], out["m_run"])
    assert Qh.shape == (n, n, T - 1) and bias.shape == (n, T - 1) and np.all(np.linalg.eigvalsh(Qh[:, :, -1]) > 0.0)


def _stated_bytes(rbpf, s):
    if s.driver is None:
        return rbpf.loc_forward_stats_workspace_bytes(V.N_P, V.N_T)
    rows, _, qpos, _ = s.map.transition.layout(s.nN)
    return rbpf.device_map_forward_stats_workspace_bytes(s.nN, len(rows), V.N_P, V.N_T, quat_pos=qpos)


@pytest.mark.parametrize("kind,name", [("mag", "pages"), ("gauss", "D"), ("pose", "E")])
def test_incremental_equals_one_shot(rbpf, kind, name):
    r = _runner(rbpf, kind, name)
    T = V.N_T
    base = _live(rbpf)
    with r.session() as s:
        s.advance(3)
        s.sync()
        before = _live(rbpf)
        first = s.running_statistics(want=NAMES)
        assert first["S_run"].shape[2] == 2 and first["mass_run"].shape == (2,)
        with_carry = _live(rbpf)
        assert with_carry == before + _stated_bytes(rbpf, s)        # exactly the stated bytes while the carry lives
        s.advance(4)
        s.sync()
        grown = _live(rbpf) - with_carry                                  # (what the filter's own steps took, if anything)
        second = s.running_statistics(want=NAMES)
        assert _live(rbpf) == with_carry + grown
        s.reset_running_statistics()
        assert _live(rbpf) == before + grown
        third = s.running_statistics(want=NAMES)                          # from an empty carry again
        assert _live(rbpf) == with_carry + grown
    assert _live(rbpf) == base                                            # close hands the carry back too
    with r.session() as s:
        s.advance(T)
        fresh = s.running_statistics(want=NAMES)
    assert _live(rbpf) == base
    for k in ("S_run", "m_run", "mass_run"):
        np.testing.assert_array_equal(second[k][..., :2], first[k])      # the first call's two pages reappear bit for bit
    for k in NAMES:
        np.testing.assert_array_equal(second[k], fresh[k])
        np.testing.assert_array_equal(third[k], fresh[k])


def test_the_other_smoothers_are_left_as_they_were(rbpf):
    MARG = ("w_smooth", "mean", "cov", "ess", "mass")
    STATS = MARG + ("S", "m", "pair_mass")
    for kind, name in (("mag", "pages"), ("pose", "E")):
        r = _runner(rbpf, kind, name)
        with r.session() as s:
            s.advance(V.N_T)
            sm0 = s.smoothed_marginals(want=MARG)
            bs0 = s.backward_simulate(16, rng=rbpf.PhiloxRNG(5))
            mt0 = s.map_trajectory()
            ts0 = s.transition_statistics(want=STATS)
            rs0 = s.running_statistics(want=NAMES)
            sm1 = s.smoothed_marginals(want=MARG)                         # with the carry alive
            bs1 = s.backward_simulate(16, rng=rbpf.PhiloxRNG(5))
            mt1 = s.map_trajectory()
            ts1 = s.transition_statistics(want=STATS)
            rs1 = s.running_statistics(want=NAMES)
        for a, b in ((sm0, sm1), (bs0, bs1), (ts0, ts1), (rs0, rs1)):
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
        a = s.running_statistics(want=NAMES)
    mp = rbpf.DenseMagMap(rbpf.DenseMagModel(c["NN"], c["L"]), c["mean"], c["V"], c["sigma2"])
    S, m, mass, ex = rbpf.particleRunningStatisticsLocalization(mp.dynModel, mp.measModel, c["odometry"], c["y"], c["x0_nonLin"], c["Q"], np.eye(3),
                                                                c["N_P"], c["dt"], rng=rbpf.ReplayRNG(c["U"], c["Z"]), every=2, extras=True)
    for got, k in ((S, "S_run"), (m, "m_run"), (mass, "mass_run"), (ex["tau_S"], "tau_S"), (ex["tau_m"], "tau_m")):
        np.testing.assert_array_equal(got, a[k])
    assert ex["traj_max"].shape == (7, V.N_T) and S.shape == (6, 6, V.N_T - 1)


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
            _refused(rbpf, s.running_statistics, rbpf.RBPF_ERR_STATE, "keep_history = 1 and trace = 1")
    with r.session() as s:
        _refused(rbpf, s.running_statistics, rbpf.RBPF_ERR_STATE, "0 steps are done")
        s.advance(1)
        s.sync()
        _refused(rbpf, s.running_statistics, rbpf.RBPF_ERR_STATE, "1 steps are done")
        with pytest.raises(ValueError):
            s.running_statistics(want=("S",))
        s.reset_running_statistics()                                      # no carry: nothing happens
        s.advance(1)
        assert s.running_statistics(want=("mass_run",))["mass_run"].shape == (1,)    # 2 steps are enough
        lib = rbpf.load_library()
        assert lib.rbpf_loc_generic_forward_stats_begin(s.ctx, 1, (C.c_int32 * 1)(0), 0, -1) == rbpf.RBPF_ERR_INVALID_ARG   # not a generic context


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
        _refused(rbpf, s.running_statistics, rbpf.RBPF_ERR_UNSUPPORTED, "transition density")
    h.reset()
    p = h.c.p
    _refused(rbpf, lambda: rbpf.particleRunningStatisticsLocalization(h.map(rbpf, transition=False), None, p["odometry"], p["y"], p["x0_nonLin"],
                                                                       p["Q"], p["R"], p["N_P"], p["dt"], rng=rbpf.ReplayRNG(p["U"], p["Z"])),
             rbpf.RBPF_ERR_UNSUPPORTED, "transition density")
    for kw in (dict(keep_history=False, trace=True), dict(keep_history=True, trace=False)):
        with r.session(**kw) as s:
            s.advance(T)
            s.sync()
            _refused(rbpf, s.running_statistics, rbpf.RBPF_ERR_STATE, "keep_history = 1 and trace = 1")
    with r.session() as s:
        _refused(rbpf, s.running_statistics, rbpf.RBPF_ERR_STATE, "0 steps are done")
        s.advance(1)
        s.sync()
        _refused(rbpf, s.running_statistics, rbpf.RBPF_ERR_STATE, "1 steps are done")
        with pytest.raises(ValueError):
            s.running_statistics(want=("pair_mass",))
    with r.session() as s:                                                # the undisturbed session the disturbed one must end equal to
        s.advance(T)
        good = s.running_statistics(want=NAMES)
    with r.session() as s:
        s.advance(T)
        s.sync()
        before = _live(rbpf)
        t, xn = C.c_int32(0), C.c_void_p()
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))            # noqa: E731
        eye = np.asfortranarray(np.eye(3))
        # out of order at the C ABI
        assert lib.rbpf_loc_generic_forward_stats_step_device(s.ctx, None, None, 1.0) == rbpf.RBPF_ERR_STATE
        assert b"no running-statistics stepping is open" in lib.rbpf_last_error()
        assert lib.rbpf_loc_generic_forward_stats_particles_device(s.ctx, C.byref(t), C.byref(xn)) == rbpf.RBPF_ERR_STATE
        assert lib.rbpf_loc_generic_forward_stats_finish(s.ctx, *none5) == rbpf.RBPF_ERR_STATE
        assert lib.rbpf_loc_generic_forward_stats_begin(s.ctx, 3, rows, mask, 0) == rbpf.RBPF_ERR_INVALID_ARG   # a block that runs past n_sel
        assert lib.rbpf_loc_generic_forward_stats_begin(s.ctx, 3, rows, 8, -1) == rbpf.RBPF_ERR_INVALID_ARG     # an angle bit above n_sel
        assert lib.rbpf_loc_generic_forward_stats_reset(s.ctx) == rbpf.RBPF_OK                                  # no carry: nothing happens
        assert _live(rbpf) == before
        assert lib.rbpf_loc_generic_forward_stats_begin(s.ctx, 3, rows, mask, -1) == rbpf.RBPF_OK
        carry = rbpf.device_map_forward_stats_workspace_bytes(4, 3, V.N_P, T)
        assert _live(rbpf) == before + carry
        assert lib.rbpf_loc_generic_forward_stats_begin(s.ctx, 3, rows, mask, -1) == rbpf.RBPF_ERR_STATE        # a second begin
        assert b"a running-statistics stepping is open" in lib.rbpf_last_error()
        for st in (lib.rbpf_loc_generic_backward_begin(s.ctx, 4, None, 1, 3, rows, mask),                       # nor one of the other four
                   lib.rbpf_loc_generic_map_begin(s.ctx, 3, rows, mask, -1),
                   lib.rbpf_loc_generic_marginal_begin(s.ctx, 3, rows, mask, -1),
                   lib.rbpf_loc_generic_pair_stats_begin(s.ctx, 3, rows, mask, -1),
                   lib.rbpf_loc_generic_forward_stats_reset(s.ctx)):                                            # nor a reset
            assert st == rbpf.RBPF_ERR_STATE and b"a running-statistics stepping is open" in lib.rbpf_last_error()
        assert _live(rbpf) == before + carry
        assert lib.rbpf_loc_generic_forward_stats_particles_device(s.ctx, C.byref(t), C.byref(xn)) == rbpf.RBPF_OK and t.value == 0 and xn.value
        assert lib.rbpf_loc_generic_forward_stats_step_device(s.ctx, None, None, 1.0) == rbpf.RBPF_ERR_INVALID_ARG   # every step needs mu and cov
        assert lib.rbpf_loc_generic_forward_stats_step_device(s.ctx, xn, dp(eye), -1.0) == rbpf.RBPF_ERR_INVALID_ARG
        bad = np.asfortranarray(np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]]))
        st = lib.rbpf_loc_generic_forward_stats_step_device(s.ctx, xn, dp(bad), 1.0)                            # refused before mu is read
        assert st == rbpf.RBPF_ERR_CHOL_FAILED and b"step 0" in lib.rbpf_last_error()
        pm = np.zeros(T - 1)
        assert lib.rbpf_loc_generic_forward_stats_finish(s.ctx, None, None, dp(pm), None, None) == rbpf.RBPF_ERR_STATE
        assert b"from 0 on were not folded in" in lib.rbpf_last_error()
        assert lib.rbpf_loc_generic_forward_stats_finish(s.ctx, *none5) == rbpf.RBPF_ERR_STATE                  # ... and the stepping is closed
        assert _live(rbpf) == before + carry                                                                    # the carry stays
        # with other rows than the carry was built with: reset first
        assert lib.rbpf_loc_generic_forward_stats_begin(s.ctx, 2, rows, 0, -1) == rbpf.RBPF_ERR_STATE and b"other rows" in lib.rbpf_last_error()
        # this stepping cannot begin while one of the other four is open (the carry alive or not)
        for begin, finish, what in ((lambda: lib.rbpf_loc_generic_backward_begin(s.ctx, 4, None, 1, 3, rows, mask),
                                     lambda: lib.rbpf_loc_generic_backward_finish(s.ctx, None, None, None), b"a backward pass is open"),
                                    (lambda: lib.rbpf_loc_generic_map_begin(s.ctx, 3, rows, mask, -1),
                                     lambda: lib.rbpf_loc_generic_map_finish(s.ctx, None, None, None), b"a MAP pass is open"),
                                    (lambda: lib.rbpf_loc_generic_marginal_begin(s.ctx, 3, rows, mask, -1),
                                     lambda: lib.rbpf_loc_generic_marginal_finish(s.ctx, *none5), b"a marginal pass is open"),
                                    (lambda: lib.rbpf_loc_generic_pair_stats_begin(s.ctx, 3, rows, mask, -1),
                                     lambda: lib.rbpf_loc_generic_pair_stats_finish(s.ctx, *((None,) * 8)), b"a statistics pass is open")):
            assert begin() == rbpf.RBPF_OK
            assert lib.rbpf_loc_generic_forward_stats_begin(s.ctx, 3, rows, mask, -1) == rbpf.RBPF_ERR_STATE and what in lib.rbpf_last_error()
            assert finish() == rbpf.RBPF_OK
        assert _live(rbpf) == before + carry
        st = lib.rbpf_loc_forward_stats_update(s.ctx, *none5)                                                   # the dense-mag entry point refuses
        assert st == rbpf.RBPF_ERR_UNSUPPORTED and b"transition density" in lib.rbpf_last_error()
        assert lib.rbpf_loc_forward_stats_reset(s.ctx) == rbpf.RBPF_ERR_INVALID_ARG
        assert lib.rbpf_loc_generic_forward_stats_reset(s.ctx) == rbpf.RBPF_OK
        assert _live(rbpf) == before
        # a cov that is not positive definite, through the binding: before any handle or kernel runs
        tr = s.map.transition
        s.map.transition = rbpf.DeviceTransition(h.mean, lambda dt, Q: bad, h.c.rows, h.c.angle_rows)
        calls = h.mean_calls
        _refused(rbpf, s.running_statistics, rbpf.RBPF_ERR_CHOL_FAILED, "step 0")
        assert h.mean_calls == calls
        s.map.transition = tr
        # a `mean` handle that returns the wrong shape: the stepping is closed, the (empty) carry stays
        h.returns = "shape"
        with pytest.raises(ValueError, match="mean returned"):
            s.running_statistics()
        assert _live(rbpf) == before + carry
        h.returns = None
        s.reset_running_statistics()
        # ... and one that raises at its third call: two steps are folded in, a valid call resumes there
        import test_gpu_device_map_smoother as GS
        h.mean_calls, h.fail_at = 0, 3
        with pytest.raises(GS.Boom):
            s.running_statistics()
        assert _live(rbpf) == before + carry
        h.fail_at = None
        h.mean_calls = 0
        again = s.running_statistics(want=NAMES)
        assert h.mean_calls == T - 1 - 2                                  # steps 2 .. N_T-2 only
        for k in NAMES:
            np.testing.assert_array_equal(again[k], good[k])
    assert _live(rbpf) == base
    with r.session() as s:                                                # rbpf_destroy releases a living carry and an open stepping
        s.advance(T)
        assert lib.rbpf_loc_generic_forward_stats_begin(s.ctx, 3, rows, mask, -1) == rbpf.RBPF_OK
    assert _live(rbpf) == base
