"""The sweep over every instantiation of the transition term (tests/transition_sweep_ref.py), the parts that need no device: the
conditions under which tests/test_gpu_transition_sweep.py means something, checked on the references alone.

  coverage     the table holds each of the 25 term types of gs_pick once, and the probes' argument helper takes every layout;
  margins      every draw at least 100 eps_ref from a cdf edge (the project's margin condition), every near-best set of the MAP step
               a singleton (the project's cap of 1 % with nothing on the path, tightened to 0), every wrapped angle residual at
               least 0.05 rad from +-pi, the rotation residuals below pi / 2 - 0.1: e0 > 0.09, away from the sign flip;
  power        a deliberately wrong evaluation (two plain rows of the successors swapped, an angle bit dropped, the first and last
               residual of cov swapped, the off-diagonal part of its last row and column halved) moves the long-double logp by more
               than 1e-6 of max |logp|, 1000 x the tolerance of the GPU test;
  far          in far_first the rows of W before the skip test alone put every displaced pair more than 746 below its successor's
               maximum of l = log w + logp (the running maximum minus 746 is the kernels' bound, and it never exceeds that); in
               far_last they leave it above that bound while the whole l lies more than 746 below."""
import itertools

import numpy as np
import pytest

import transition_sweep_ref as T

LD = np.longdouble
POWER = 1e-6


def _all(name):
    return [(v, T.inputs(name, v), T.reference(name, v)) for v in T.variants(name)]


# ------------------------------------------------------------------------------------------------
# 1. the table
# ------------------------------------------------------------------------------------------------
def test_the_table_holds_every_term_type_once():
    want = [("gauss", n, a) for n in range(1, 9) for a in (False, True)]
    want += [("pose", n, a) for n in range(5) for a in (False, True) if not (n == 0 and a)]
    assert len(want) == 25 and len(T.LAYOUTS) == 25 and len(set(T.NAMES)) == 25
    assert sorted(l.type for l in T.LAYOUTS) == sorted(want)
    assert len(T.FAR_CASES) == 49                                          # two per layout, less far_first of p0


def test_the_layouts_are_shuffled_as_stated():
    first = middle = last = before = after = 0
    for l in T.LAYOUTS:
        assert len(set(l.rows)) == l.n_sel and min(l.rows) >= 0 and max(l.rows) < T.N_NONLIN
        for rows in (l.plain, l.quat_rows or ()) if l.quat_rows else (l.rows,):
            rows = list(rows)
            assert len(rows) < 2 or rows != sorted(rows), (l.name, rows)
            assert len(rows) < 3 or rows != sorted(rows, reverse=True), (l.name, rows)
        assert set(l.angle_rows) <= set(l.plain)
        if l.angle_rows and len(l.plain) >= 2:
            bits = [l.plain.index(a) for a in l.angle_rows]                # kernel order
            assert len(bits) >= 2
            if len(l.plain) >= 3:
                assert not T.all_adjacent(bits), (l.name, bits)
        if l.quat_rows:
            assert l.rows[l.qpos:l.qpos + 4] == l.quat_rows
            if l.n_plain:
                first += l.qpos == 0
                last += l.qpos + 4 == l.n_sel
                middle += 0 < l.qpos < l.n_sel - 4
            before += any(l.rows.index(a) < l.qpos for a in l.angle_rows)
            after += any(l.rows.index(a) > l.qpos for a in l.angle_rows)
    assert first >= 1 and middle >= 1 and last >= 1 and before >= 2 and after >= 2
    assert any(bin(l.angle_mask()).count("1") > 1 for l in T.LAYOUTS)


@pytest.mark.parametrize("name", T.NAMES)
def test_the_probes_take_the_layout(rbpf, name):
    l, p = T.layout(name), T.inputs(name)
    mu, xs, cov, rows, mask, qpos = rbpf.host._transition_probe_args(**T.probe_args(p))
    assert mu.shape == (l.n_sel, T.N) and xs.shape == (T.N_NONLIN, T.M) and cov.shape == (l.n_res, l.n_res)
    assert tuple(rows.tolist()) == l.rows and mask == l.angle_mask() and qpos == l.qpos
    if l.quat_rows:
        assert rbpf.host._quat_position(l.rows, l.angle_rows, l.quat_rows) == l.qpos
        assert not mask & (0xF << qpos)
    # kernel order: every residual once, the plain ones in the caller's order
    order = l.kernel_order()
    assert sorted(order) == list(range(l.n_res)) and order[:max(l.n_plain, 0)] == sorted(order[:max(l.n_plain, 0)])


# ------------------------------------------------------------------------------------------------
# 2. the inputs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", T.NAMES)
def test_the_inputs_are_as_stated(name):
    l = T.layout(name)
    p = T.inputs(name)
    cov = p["cov"]
    np.testing.assert_array_equal(cov, cov.T)
    assert np.linalg.cond(cov) < 1e3 and len(set(np.diag(cov).tolist())) == l.n_res
    assert l.n_res == 1 or np.min(np.abs(cov[~np.eye(l.n_res, dtype=bool)])) > 0.0            # full
    assert np.all(p["w"][:10] == 0.0) and np.all(p["w"][-10:] == 0.0) and np.all(p["w"][10:-10] > 0.0)
    assert np.all(p["delta"][:10] == -np.inf) and np.all(np.isfinite(p["delta"][10:-10]))
    decoys = [r for r in range(T.N_NONLIN) if r not in l.rows]
    assert np.all(np.abs(p["xs_next"][decoys]) >= 1e3) and len(set(p["xs_next"][decoys].ravel().tolist())) == len(decoys) * T.M
    assert np.max(np.abs(p["xs_next"][list(l.rows)])) < 4.0
    for a in l.angle_rows:                                                 # the predecessors are spread over seven turns
        k = np.rint((p["mu"][l.rows.index(a)] - 3.1) / (2.0 * np.pi))
        assert set(k.tolist()) == set(range(-3, 4))
    if l.quat_rows:
        assert np.max(np.abs(np.sum(p["mu"][l.qpos:l.qpos + 4] ** 2, axis=0) - 1.0)) < 1e-14
        assert np.max(np.abs(np.sum(p["xs_next"][list(l.quat_rows)] ** 2, axis=0) - 1.0)) < 1e-14
    for v in T.variants(name):
        q = T.inputs(name, v)
        if v != "base":
            live = np.nonzero(p["w"] > 0)[0]
            assert q["displaced"].size == live.size // 2 and np.all(p["w"][q["displaced"]] > 0)
            same = np.setdiff1d(np.arange(T.N), q["displaced"])
            np.testing.assert_array_equal(q["mu"][:, same], p["mu"][:, same])
        dist = T.worst_wrap_distance(q)
        assert dist >= T.WRAP_MARGIN, (v, dist)
        if l.quat_rows:
            phi = T.P.max_phi(q["xs_next"], q["mu"], q["rows"], q["quat_rows"])
            assert phi < np.pi / 2 - 0.1, (v, phi)


@pytest.mark.parametrize("name", T.NAMES)
def test_margins_and_near_best_sets(name):
    for v, p, o in _all(name):
        ratio = float(np.min(o["margin"] / o["eps_ref"]))
        rel = float(np.max(np.abs(o["logp"] - o["logp_ld"])) / np.max(np.abs(o["logp_ld"])))
        sizes = [n.size for n in o["near"]]
        print(f"{name} {v}: min margin {ratio:.2e} eps_ref, logp fp64 vs long double {rel:.2e}, largest near-best set {max(sizes)}")
        assert np.all(o["margin"] >= 100.0 * o["eps_ref"])
        assert rel <= 1e-10
        np.testing.assert_array_equal(o["index"], o["index_ld"])
        assert np.all(p["w"][o["index"]] > 0)
        assert sizes == [1] * T.M
        np.testing.assert_array_equal(o["arg"], [n[0] for n in o["near"]])
        assert np.all(np.isfinite(o["best"].astype(np.float64)))
        if v != "base":                                                    # the reference never selects a displaced particle either
            assert not np.any(np.isin(o["index"], p["displaced"])) and not np.any(np.isin(o["arg"], p["displaced"]))
    assert len(np.unique(T.reference(name)["index"])) > T.M // 2           # the draws are spread, over both chunks
    assert T.reference(name)["index"].max() >= 256 and T.reference(name)["index"].min() < 256


# ------------------------------------------------------------------------------------------------
# 3. discriminating power
# ------------------------------------------------------------------------------------------------
def _mutations(p):
    """(label, keyword arguments of a wrong evaluation)."""
    l = p["layout"]
    for a, b in itertools.combinations(l.plain, 2):                        # (a)
        xs = p["xs_next"].copy()
        xs[[a, b]] = xs[[b, a]]
        yield f"successor rows {a} and {b} swapped", dict(xs_next=xs)
    for a in l.angle_rows:                                                 # (b)
        yield f"angle bit of row {a} dropped", dict(angle_rows=tuple(r for r in l.angle_rows if r != a))
    if l.n_res >= 2:
        perm = list(range(l.n_res))
        perm[0], perm[-1] = perm[-1], perm[0]
        yield "first and last residual of cov swapped", dict(cov=p["cov"][np.ix_(perm, perm)])   # (c)
        cov = p["cov"].copy()
        cov[-1, :-1] *= 0.5
        cov[:-1, -1] *= 0.5
        yield "off-diagonal part of the last row and column of cov halved", dict(cov=cov)        # (d)


@pytest.mark.parametrize("name", T.NAMES)
def test_a_wrong_evaluation_shows(name):
    p = T.inputs(name)
    l = p["layout"]
    right = T.reference(name)["logp_ld"]
    scale = np.max(np.abs(right))
    effects = []
    for label, kw in _mutations(p):
        eff = float(np.max(np.abs(T.logp_ld(p, **kw) - right)) / scale)
        effects.append(eff)
        assert eff > POWER, (label, eff)
    want = len(l.plain) * (len(l.plain) - 1) // 2 + len(l.angle_rows) + (2 if l.n_res >= 2 else 0)
    assert len(effects) == want
    if effects:
        print(f"{name}: {len(effects)} mutations, smallest effect {min(effects):.2e} of max |logp| = {float(scale):.1f}")


# ------------------------------------------------------------------------------------------------
# 4. the far variants
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,variant", T.FAR_CASES)
def test_far_variants_sit_where_the_skip_test_does(name, variant):
    p, o = T.inputs(name, variant), T.reference(name, variant)
    l = p["layout"]
    head, whole = T.kernel_sums(p)
    scale = np.max(np.abs(o["logp_ld"]))
    assert float(np.max(np.abs(whole - o["logp_ld"])) / scale) <= 1e-12    # z'z does not depend on the order of the residuals
    lw = np.log(p["w"][p["displaced"]].astype(LD))[:, None]
    with np.errstate(divide="ignore"):
        top = np.max(np.log(p["w"].astype(LD))[:, None] + o["logp_ld"], axis=0)[None, :]
    bound = top - LD(T.SKIP)
    part, full = lw + head[p["displaced"]], lw + whole[p["displaced"]]
    print(f"{name} {variant}: rows before the test {l.skip_rows}; displaced pairs: head - max in [{float(np.min(part - top)):.0f}, "
          f"{float(np.max(part - top)):.0f}], whole - max at most {float(np.max(full - top)):.0f}")
    assert np.all(full < bound)                                            # exp is exactly 0: below -745.14
    if variant == "far_first":
        if l.skip_rows >= 1:
            assert np.all(part < bound)                                    # the test fires
        else:
            assert l.type[:2] == ("gauss", 1)                              # NR = 1: no early test
    else:
        assert np.all(part > bound)                                        # the test cannot fire: exp alone
        if l.skip_rows == 0:
            assert np.all(head == 0.0)
