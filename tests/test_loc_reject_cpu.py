"""CPU: the restatement of backward simulation by rejection sampling (tests/loc_reject_ref.py) draws from the backward kernel, equals
the existing restatement at max_tries = 0, and every fixture of tests/test_gpu_loc_reject.py meets the conditions under which the GPU
tests compare every index: all margins at least 100 x their error measure, the fp64 and the long-double decisions equal."""
import numpy as np
import pytest

import localization_smoother_ref as LS
import loc_reject_ref as J
import transition_sweep_ref as TS

LD = np.longdouble


def _chi2_quantile_999(df):
    try:
        from scipy.stats import chi2
        return float(chi2.ppf(0.999, df))
    except ImportError:                                                    # Wilson-Hilferty, z(0.999) = 3.090232
        return df * (1.0 - 2.0 / (9.0 * df) + 3.090232306167813 * np.sqrt(2.0 / (9.0 * df))) ** 3


def test_the_law_of_the_indices():
    """N = 12 particles (two of weight 0), 3 successors each repeated 10 000 times, R = 4, the device generator's counters with a
    fixed seed: the counts of the drawn indices per successor against the exact backward probabilities w_i exp(logp_i) / sum."""
    N, reps, R, seed = 12, 10000, 4, 20260101
    M = 3 * reps
    p = J.mag_fixture(N=64, M=3, spread=0.5, seed=17)
    keep = np.arange(10, 10 + N)                                           # (the fixture's first and last ten weights are zeros)
    X, w = p["X"][:, keep], p["w"][keep].copy()
    w[[0, 7]] = 0.0
    lp64, lp_ld = J.lp_mag(p["xs_next"], X, p["odo"], p["dt"], p["Q"])
    cols = np.arange(M) % 3
    u = np.array([J.philox_ref.uniform2(seed, j, 0, J.philox_ref.BACKWARD_LANE, 0)[0] for j in range(M)])
    res = J.step(lp64[:, cols], lp_ld[:, cols], w, J.PhiloxTries(seed, 0, R), u)
    n_acc, n_fb = int(np.sum(res["accepted_at"] >= 0)), int(np.sum(res["accepted_at"] < 0))
    print(f"accepted {n_acc}, fallback {n_fb} of {M}")
    assert n_acc >= 0.05 * M and n_fb >= 0.05 * M                          # both kinds of draw are in the sample
    assert not np.any(w[res["index"]] == 0.0)
    live = np.nonzero(w > 0)[0]
    for s in range(3):
        pr = (w[live].astype(LD) * np.exp(lp_ld[live, s]))
        pr = (pr / np.sum(pr)).astype(np.float64)
        expected = reps * pr
        counts = np.bincount(res["index"][cols == s], minlength=N)[live]
        assert counts.sum() == reps
        assert np.all(expected >= 5.0), expected                          # Pearson's approximation stands
        stat = float(np.sum((counts - expected) ** 2 / expected))
        bound = _chi2_quantile_999(live.size - 1)
        print(f"successor {s}: chi2 = {stat:.2f}, 0.999 quantile at df = {live.size - 1}: {bound:.2f}, smallest expected count {expected.min():.1f}")
        assert stat < bound


def test_max_tries_zero_is_the_existing_restatement():
    c = J.session_case("mag")
    X, W = J.session_forward("mag")
    T, M, seed = X.shape[0], 130, J.SESSION["seed"]
    sim = J.simulate(X, W, J.session_lp("mag", X), seed, 0, M)
    old = LS.backward_simulate(X, W, c["odometry"], c["Q"], c["dt"], J.backward_uniforms(seed, T, M))
    np.testing.assert_array_equal(sim["index"], old["index"])
    np.testing.assert_array_equal(sim["index_ld"], old["index_ld"])
    assert np.all(sim["n_fallback"][:-1] == M) and sim["n_fallback"][-1] == 0 and not np.any(sim["n_tries"])


def _check(res, mixed):
    ok, worst = J.conditions(res)
    acc, fb = J.shares(res)
    print(f"smallest margin / error {worst:.3g}; accepted {acc:.3f}, fallback {fb:.3f}")
    assert ok
    if mixed:
        assert acc >= 0.2 and fb >= 0.2


def test_mag_fixture_holds():
    p = J.mag_fixture()
    assert (p["X"].shape[1], p["xs_next"].shape[1]) == J.MAG_SHAPE and p["u_try"].shape[0] == J.MIXED_R
    assert np.all(p["w"][:10] == 0) and np.all(p["w"][-10:] == 0)
    res = J.reference(p)
    _check(res, True)
    assert res["n_fallback"] > 256                                         # M' crosses a trajectory block of the all-pairs pass
    # the expectation stated for this regime (0.5 sd, R = 16): a share of about 0.53 falls back
    assert abs(J.shares(res)[1] - 0.53) < 0.1


@pytest.mark.parametrize("name", TS.NAMES)
def test_sweep_fixture_holds(name):
    p = J.sweep_fixture(name)
    assert (p["mu"].shape[1], p["xs_next"].shape[1]) == J.SWEEP_SHAPE
    _check(J.reference(p), True)


def test_nothing_falls_back_fixture_holds():
    res = J.reference(J.nothing_falls_back_fixture())
    _check(res, False)
    assert res["n_fallback"] == 0


@pytest.mark.parametrize("base", ["mag", "g3", "p3"])
def test_far_successor_fixture_holds(base):
    p = J.mag_fixture() if base == "mag" else J.sweep_fixture(base)
    j = 77
    res = J.reference(J.far_successor(p, j))
    _check(res, True)
    assert res["accepted_at"][j] == -1
    lp = J.logp_of(J.far_successor(p, j))[0][:, j]
    assert np.all(np.exp(lp) == 0)                                         # every fp64 exp is 0: no try can be accepted
    keep = np.arange(res["index"].size) != j
    np.testing.assert_array_equal(res["index"][keep], J.reference(p)["index"][keep])


@pytest.mark.parametrize("kind", J.SESSION_KINDS)
def test_session_fixture_holds(kind):
    """On the restatement's own forward pass; the GPU test asserts the same on the arrays it reads back.  n_traj = 130 is the first
    130 trajectories of n_traj = 700: the counters are keyed by the trajectory."""
    X, W = J.session_forward(kind)
    sim = J.simulate(X, W, J.session_lp(kind, X), J.SESSION["seed"], J.SESSION["R"], max(J.SESSION["n_traj"]))
    ok, worst = J.simulate_holds(sim)
    print(f"{kind}: smallest margin / error {worst:.3g}; n_fallback {sim['n_fallback'].tolist()}, n_tries {sim['n_tries'].tolist()}")
    assert ok
    T = X.shape[0]
    assert np.all(sim["n_fallback"][:T - 1] > 0) and np.all(sim["n_fallback"][:T - 1] < max(J.SESSION["n_traj"]))
