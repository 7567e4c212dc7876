"""Backward simulation in a DeviceMap for pose states (rbpf.DeviceTransition(..., quat_rows=...)), the parts that need no device:
the checker itself (tests/pose_transition_ref.py), the margin condition on every case the GPU tests run (every draw, none
excluded), and the prototypes, exports and refusals that come before any device is touched.

The checker-only tests pass with or without the feature: they validate the committed inputs.  Bounds: 1e-12 relative for two
evaluations of one density in the same precision (a 6 x 6 forward substitution of condition < 1e3 and a quaternion product: a few
hundred eps in fp64, far less in long double); the margin condition is that of tests/test_device_map_smoother_cpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import localization_smoother_ref as LS
import pose_transition_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rbpf_loc_generic_backward_pose_begin", "rbpf_loc_generic_backward_pose_workspace_bytes", "rbpf_loc_generic_backward_pose_step"]
LD = np.longdouble


def _never(*a):
    raise AssertionError("a handle was called")


# ------------------------------------------------------------------------------------------------
# 1. the checker
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,M", [(1, 1), (70, 5), (257, 65)])
def test_model_e_form_is_the_dense_mag_density(N, M):
    """logp of tests/localization_smoother_ref.py (the checker tied to the reference's run_localization.m) on its own probe inputs
    equals this checker's with mu = (p + dx_pos, qRight(q) dq) and the block-diagonal cov, in long double."""
    p = LS.probe_case(N, M)
    mu, cov = P.dense_mag_as_pose(p)
    if N != 70:                                                            # the examples' diagonal Q: blkdiag(dt Q(1:3,1:3), dt Q(4:6,4:6))
        np.testing.assert_array_equal(cov, p["dt"] * np.diag(np.diag(p["Q"])))
    worst = 0.0
    for j in range(M):
        want = LS.logp(p["xs_next"][:, j], p["X"], p["odo"], p["dt"], p["Q"], LD)
        got = P.logp(p["xs_next"][:, j], mu, cov, P.ROWS_E, (), P.QUAT_E, LD)
        worst = max(worst, float(np.max(np.abs(got - want)) / np.max(np.abs(want))))
    print(f"dense-mag {N} x {M}: pose checker vs localization_smoother_ref, long double: {worst:.2e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("name,N,M", P.PROBE_LOGP_CASES)
def test_atan2_form_is_the_literal_logq(name, N, M):
    p = P.probe_case(name, N, M)
    worst = 0.0
    for j in range(M):
        a = P.logp(p["xs_next"][:, j], p["mu"], p["cov"], p["rows"], p["angle_rows"], p["quat_rows"], LD)
        b = P.logp(p["xs_next"][:, j], p["mu"], p["cov"], p["rows"], p["angle_rows"], p["quat_rows"], LD, logq=P.logq_acos)
        worst = max(worst, float(np.max(np.abs(a - b)) / np.max(np.abs(b))))
    print(f"{name} {N} x {M}: atan2 form vs acos / sin form of tools/logq.m, long double: {worst:.2e}")
    assert worst <= 1e-12


def test_logp_does_not_depend_on_where_the_block_sits_in_rows():
    """Model G's rows (4, 0, 1, 2, 3, 6) against the orders (0, 1, 2, 3, 4, 6) and (4, 6, 0, 1, 2, 3), mu and cov permuted with them."""
    p = P.probe_case("G", 70, 5)
    base = np.stack([P.logp(p["xs_next"][:, j], p["mu"], p["cov"], p["rows"], p["angle_rows"], p["quat_rows"], LD) for j in range(5)])
    # residual order of (4, q, 6) is [r4, phi, r6] = 0, (1, 2, 3), 4
    for rows, mu_perm, res_perm in (((0, 1, 2, 3, 4, 6), (1, 2, 3, 4, 0, 5), (1, 2, 3, 0, 4)),
                                    ((4, 6, 0, 1, 2, 3), (0, 5, 1, 2, 3, 4), (0, 4, 1, 2, 3))):
        assert tuple(p["rows"][k] for k in mu_perm) == rows
        mu = p["mu"][list(mu_perm)]
        cov = p["cov"][np.ix_(res_perm, res_perm)]
        got = np.stack([P.logp(p["xs_next"][:, j], mu, cov, rows, p["angle_rows"], p["quat_rows"], LD) for j in range(5)])
        err = float(np.max(np.abs(got - base)) / np.max(np.abs(base)))
        print(f"rows {rows}: {err:.2e}")
        assert err <= 1e-12


@pytest.mark.parametrize("name", P.MODELS)
def test_the_density_inverts_the_sampler(name):
    """At x' = dyn(x, z), logp = -z'z / 2 (fp64, 1e-12 relative as in tests/test_device_map_smoother_cpu.py; |z| of a few units)."""
    c = P.case(name, 8, 4)
    rs = np.random.RandomState(5 + ord(name))
    worst = 0.0
    for trial in range(20):
        t = trial % 3
        x = rs.uniform(-1.0, 1.0, (c.nN, 1))
        x[list(c.quat_rows)] = P.expq(rs.standard_normal((3, 1)))
        for a in c.angle_rows:
            x[a] = 0.5
        z = rs.standard_normal((1, c.n_res))
        xp = c.dyn(x, t, z)[:, 0]
        got = P.logp(xp, c.mean(x, t), c.cov(t), c.rows, c.angle_rows, c.quat_rows)[0]
        zz = float(np.sum(z * z))
        worst = max(worst, abs(got + 0.5 * zz) / (0.5 * zz))
    print(f"model {name}: largest |logp + z'z/2| / |z'z/2| {worst:.2e}")
    assert worst < 1e-12


def _check_margins(name, margin, eps_ref, logp_rel):
    print(f"{name}: min margin {float(np.min(margin)):.3e}, eps_ref {float(np.max(eps_ref)):.3e}, logp fp64 vs long double {logp_rel:.3e}")
    assert np.all(margin >= 100.0 * eps_ref)                               # every draw: the cap on excluded draws is zero
    assert logp_rel <= 1e-10


@pytest.mark.parametrize("name,N,M", P.PROBE_LOGP_CASES + P.PROBE_INDEX_CASES)
def test_margin_condition_of_the_probe_cases(name, N, M):
    p = P.probe_case(name, N, M)
    o = P.probe_reference(name, N, M)
    rel = float(np.max(np.abs(o["logp"] - o["logp_ld"])) / np.max(np.abs(o["logp_ld"])))
    _check_margins(f"probe {name} {N} x {M}", o["margin"], o["eps_ref"], rel)
    np.testing.assert_array_equal(o["index"], o["index_ld"])
    assert np.all(p["w"][o["index"]] > 0)
    if N > 2048:
        assert o["index"].max() >= 2048                                    # beyond the largest chunk: not the first one
    phi = P.max_phi(p["xs_next"], p["mu"], p["rows"], p["quat_rows"])
    print(f"largest |phi| {phi:.3f} rad")
    assert phi < 1.0                                                       # e0 > cos(1): far from the sign flip
    assert np.max(np.abs(np.sum(p["mu"][p["case"].qpos:p["case"].qpos + 4] ** 2, axis=0) - 1.0)) < 1e-14   # mu_q is a unit quaternion
    for a in p["angle_rows"]:                                              # the angle residuals: a few sd from 0 mod 2 pi, never near +-pi
        k = p["rows"].index(a)
        r = P.wrap(p["xs_next"][a][None, :] - p["mu"][k][:, None])
        assert np.max(np.abs(r)) < 2.0
        if N >= 64:
            assert np.max(np.abs(p["xs_next"][a][None, :] - p["mu"][k][:, None])) > 1.5 * np.pi   # ... and the wrap changes some of them


@pytest.mark.parametrize("name,N_P,N_T,M", P.FULL_RUNS)
def test_margin_condition_of_the_full_runs(name, N_P, N_T, M):
    """On the restatement's own forward pass (the device's differs from it by rounding; the GPU test repeats the check on the
    device's arrays)."""
    c = P.case(name, N_P, N_T)
    X, W, AI = P.forward_arrays(c)
    _, W_ld, AI_ld = P.forward_arrays(c, np.longdouble)
    np.testing.assert_array_equal(AI, AI_ld)                               # the forward draws sit on no bin edge either
    assert len(np.unique(AI[1:])) > 1
    mus, covs = P.transition_arrays(c, X)
    u = P.full_run_uniforms(N_T, M)
    o = P.backward_simulate(X, W, mus, covs, u, c.rows, c.angle_rows, c.quat_rows)
    _check_margins(f"full run {name} {N_P} x {N_T} x {M}", o["margin"], o["eps_ref"], o["logp_rel"])
    np.testing.assert_array_equal(o["index"], o["index_ld"])
    print(f"largest |phi| {o['max_phi']:.3f} rad")
    assert o["max_phi"] < 1.0
    q = list(c.quat_rows)
    assert np.max(np.abs(np.sum(X[:, q] ** 2, axis=1) - 1.0)) < 1e-13      # the particles stay unit quaternions
    import rbpf_oracle as O
    np.testing.assert_array_equal(o["index"][N_T - 1], [O.sample(W[N_T - 1], uu) for uu in u[N_T - 1]])
    if name == "G":
        assert X[:, 6].max() > 3.0 and X[:, 6].min() < -3.0               # the heading passes +-pi during the run
        assert c.rows.index(c.quat_rows[0]) == 1 and np.count_nonzero(c.cov(0)) == 25          # block not last, cov coupled


# ------------------------------------------------------------------------------------------------
# 2. the library and the binding, before any device
# ------------------------------------------------------------------------------------------------
def test_prototypes_and_exports(rbpf):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rbpf.h")).read(), flags=re.S)
    lib = rbpf.load_library()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in rbpf.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None, name
    assert lib.rbpf_abi_version() == 9
    assert int(re.search(r"#define\s+RBPF_ABI_VERSION\s+(\d+)", src).group(1)) == 9


def test_device_transition_resolves_a_quaternion_block(rbpf):
    tr = rbpf.DeviceTransition(_never, quat_rows=(3, 4, 5, 6))
    assert tr.resolve(7) == ((0, 1, 2, 3, 4, 5, 6), 0, 3)
    assert tr.layout(7) == ((0, 1, 2, 3, 4, 5, 6), 0, 3, 6)
    tr = rbpf.DeviceTransition(_never, rows=(4, 0, 1, 2, 3, 6), angle_rows=(6,), quat_rows=(0, 1, 2, 3))
    assert tr.resolve(8) == ((4, 0, 1, 2, 3, 6), 1 << 5, 1)                # the mask's bits index positions in rows
    assert rbpf.DeviceTransition(_never, quat_rows=(0, 1, 2, 3)).layout(4) == ((0, 1, 2, 3), 0, 0, 3)
    assert rbpf.DeviceTransition(_never, rows=(0, 1, 3), angle_rows=(3,)).layout(4) == ((0, 1, 3), 4, -1, 3)   # no block: as before
    for kw, nN in ((dict(quat_rows=(3, 4, 5)), 7),                                             # not four
                   (dict(quat_rows=(3, 4, 5, 5)), 7),                                          # not distinct
                   (dict(rows=(0, 1, 2, 3, 4, 5), quat_rows=(3, 4, 5, 6)), 7),                 # not all in rows
                   (dict(rows=(3, 0, 4, 5, 6), quat_rows=(3, 4, 5, 6)), 7),                    # not adjacent
                   (dict(rows=(4, 3, 5, 6), quat_rows=(3, 4, 5, 6)), 7),                       # not in order
                   (dict(rows=(0, 3, 4, 5, 6), angle_rows=(4,), quat_rows=(3, 4, 5, 6)), 7),   # an angle row in the block
                   (dict(quat_rows=(3, 4, 5, 6)), 6)):                                         # a row the state does not have
        with pytest.raises(rbpf.RBPFError) as ei:
            rbpf.DeviceTransition(_never, **kw).resolve(nN)
        assert ei.value.status == rbpf.RBPF_ERR_INVALID_ARG, kw
    # the default cov = dt Q needs n_w == n_res = n_sel - 1
    Q = np.eye(6)
    tr = rbpf.DeviceTransition(_never, quat_rows=(3, 4, 5, 6))
    np.testing.assert_array_equal(tr.covariance(0.5, Q, tr.layout(7)[3]), 0.5 * Q)
    with pytest.raises(rbpf.RBPFError) as ei:
        tr.covariance(0.5, np.eye(7), 6)
    assert ei.value.status == rbpf.RBPF_ERR_INVALID_ARG and "n_w == n_res" in str(ei.value)


def test_workspace_bytes(rbpf):
    lib = rbpf.load_library()
    a, b = C.c_size_t(0), C.c_size_t(0)
    nN, ns, N, T, M = 7, 7, 4100, 6, 130
    assert lib.rbpf_loc_generic_backward_pose_workspace_bytes(nN, ns, 3, N, T, M, C.byref(a)) == rbpf.RBPF_OK
    assert a.value >= 8 * ((ns + 1) * N + 2 * 3 * M + T * M + nN * M * T + nN * T) + 4 * M * T   # Xhat has n_sel + 1 rows
    assert rbpf.device_map_backward_workspace_bytes(nN, ns, N, T, M, quat_pos=3) == a.value
    # with quat_pos = -1 it is the existing entry point
    assert lib.rbpf_loc_generic_backward_pose_workspace_bytes(nN, 6, -1, N, T, M, C.byref(b)) == rbpf.RBPF_OK
    assert b.value == rbpf.device_map_backward_workspace_bytes(nN, 6, N, T, M)
    assert a.value - b.value == 8 * N
    for bad in ((7, 7, 4, 8, 3, 4), (7, 3, 0, 8, 3, 4), (7, 7, -2, 8, 3, 4), (9, 7, 0, 8, 3, 4), (7, 8, 0, 8, 3, 4), (3, 3, 0, 8, 3, 4),
                (7, 7, 3, 0, 3, 4), (7, 7, 3, 8, 0, 4), (7, 7, 3, 8, 3, 0), (7, 9, -1, 8, 3, 4)):
        assert lib.rbpf_loc_generic_backward_pose_workspace_bytes(*bad, C.byref(a)) == rbpf.RBPF_ERR_INVALID_ARG, bad
    assert lib.rbpf_loc_generic_backward_pose_workspace_bytes(nN, ns, 3, N, T, M, None) == rbpf.RBPF_ERR_INVALID_ARG


def test_a_null_context_is_refused(rbpf):
    lib = rbpf.load_library()
    rows = (C.c_int32 * 7)(*range(7))
    assert lib.rbpf_loc_generic_backward_pose_begin(None, 4, None, 1, 7, rows, 0, 3) == rbpf.RBPF_ERR_INVALID_ARG
    assert b"localisation" in lib.rbpf_last_error()


def test_the_probe_refuses_bad_arguments_before_any_device(rbpf):
    lib = rbpf.load_library()
    p = P.probe_case("G", 70, 5)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))                                      # noqa: E731
    mu, w, cov, u = (np.ascontiguousarray(p[k]) for k in ("mu", "w", "cov", "u"))
    xs = np.asfortranarray(p["xs_next"])
    rows = (C.c_int32 * 10)(4, 0, 1, 2, 3, 6, 5, 7, 0, 0)
    idx = (C.c_int32 * 5)()
    call = lambda **kw: lib.rbpf_loc_generic_backward_pose_step(*[kw.get(k, v) for k, v in (                               # noqa: E731
        ("N", 70), ("M", 5), ("nN", 8), ("ns", 6), ("rows", rows), ("mask", 1 << 5), ("qpos", 1), ("mu", dp(mu)), ("w", dp(w)), ("xs", dp(xs)),
        ("cov", dp(cov)), ("u", dp(u)), ("index", idx), ("logp", None), ("reps", 1), ("ms", None))])
    for k in ("rows", "mu", "w", "xs", "cov", "u", "index"):
        assert call(**{k: None}) == rbpf.RBPF_ERR_INVALID_ARG, k
    for kw, word in ((dict(qpos=6), b"not inside rows"), (dict(qpos=-2), b"not inside rows"), (dict(qpos=17), b"not inside rows"),
                     (dict(qpos=3), b"runs past n_sel"), (dict(ns=4, mask=0, qpos=1), b"runs past n_sel"),
                     (dict(mask=1 << 2), b"quaternion block"), (dict(mask=(1 << 5) | (1 << 1)), b"quaternion block"),
                     (dict(ns=10, mask=0, qpos=0), b"n_sel - 1"),
                     (dict(mask=1 << 6), b"angle_mask"), (dict(N=0), b""), (dict(M=0), b""), (dict(nN=9), b""), (dict(nN=6), b"no row")):
        assert call(**kw) == rbpf.RBPF_ERR_INVALID_ARG, kw
        assert word in lib.rbpf_last_error(), (kw, lib.rbpf_last_error())
    dup = (C.c_int32 * 6)(4, 0, 1, 2, 0, 6)
    assert call(rows=dup) == rbpf.RBPF_ERR_INVALID_ARG and b"twice" in lib.rbpf_last_error()
    bad = np.asfortranarray(np.eye(5))
    bad[1, 0] = bad[0, 1] = 2.0
    assert call(cov=dp(bad)) == rbpf.RBPF_ERR_CHOL_FAILED and b"positive definite" in lib.rbpf_last_error()
    # the binding: mu of n_sel rows, cov of n_res = n_sel - 1
    args = dict(mu=p["mu"], w=p["w"], xs_next=p["xs_next"], cov=p["cov"], u=p["u"], rows=p["rows"], angle_rows=p["angle_rows"], quat_rows=p["quat_rows"])
    for kw in (dict(cov=np.eye(6)), dict(mu=p["mu"][:5]), dict(quat_rows=(0, 1, 2)), dict(quat_rows=(1, 2, 3, 5)), dict(angle_rows=(2,)),
               dict(rows=None)):
        with pytest.raises(rbpf.RBPFError) as ei:
            rbpf.device_map_backward_step(**dict(args, **kw))
        assert ei.value.status == rbpf.RBPF_ERR_INVALID_ARG, kw
    if rbpf.device_count() == 0:
        assert call() == rbpf.RBPF_ERR_NO_DEVICE and b"no HIP device" in lib.rbpf_last_error()
        with pytest.raises(rbpf.RBPFError) as ei:
            rbpf.device_map_backward_step(**args)
        assert ei.value.status == rbpf.RBPF_ERR_NO_DEVICE
