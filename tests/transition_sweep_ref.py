"""The case table that runs EVERY instantiation of the transition term GsTerm<NR, ANG, QP> (csrc/rbpf_loc_generic_smooth.hip) through
the one-step probes rbpf.device_map_backward_step and rbpf.device_map_map_step, and its inputs.  gs_pick selects 25 term types:

    Gaussian  n_res = 1 .. 8  x  {no angle row, at least one}                                                          16
    pose      a quaternion block behind n_plain = 0 .. 4 plain rows  x  {no angle row, one or more}, minus (0, angle)    9

LAYOUTS holds one layout per type, drawn from SEED: n_nonlin = 8 everywhere; `rows` a shuffled selection of the state rows (never
ascending; neither ascending nor descending from three rows on); the block's four rows a shuffled selection too, adjacent in `rows`
at position QPOS[name]: first, in the middle or last, with angle rows before it, after it or on both sides.  An angle layout with
two plain rows marks both (two bits are adjacent whatever one does); from three plain rows on it marks two or more, not all
adjacent.  Gaussian layouts are named g<n_res>[a], pose layouts p<n_plain>[a].

INPUTS of one step (inputs(name, variant)): N = 300 predecessors, M = 70 successors: two chunks of backward_chunk_size and a partial
tile.  cov = D C D, C = (B B' / n + I) / 2 a full correlation-like matrix, D distinct standard deviations (plain rows 0.04 .. 0.08,
angle rows 0.025 .. 0.035, the block 0.012 .. 0.018 -- so that 60 of them stay inside a half turn), redrawn until cond(cov) < 1e3.
Predecessors (mu) and successors (xs_next) lie two transition standard deviations (2 chol(cov) z) around one centre, the quaternion
as centre (x) expq(noise).  On an angle row the centre is 3.1, the successors are wrapped into [-pi, pi] as a model's post does and
predecessor i is offset by k_i 2 pi, k_i in -3 .. 3: every residual needs the wrap.  The state rows that are NOT selected are decoys
of magnitude 1e3 .. 2e3, another value for every row and successor (the probes take mu by selected rows only, so the predecessors
have none): a kernel that reads a wrong row is wrong by orders of magnitude.  The first and the last ten weights are exact zeros;
delta = log w for the MAP probe, -inf there.

VARIANTS.  "base", and two in which every second live predecessor (DISPLACED) is moved FAR_SD = 60 marginal standard deviations away
  far_first  along residual 0 IN KERNEL ORDER (kernel_order: a Gaussian layout keeps the caller's order; a pose layout has the plain
             rows first, in the caller's order, and the block last): rows[0], or the first plain row.  The rows before the terms'
             skip test (the first NR / 2, or the plain rows) then decide alone.  Not built for n_plain = 0: no plain row, no test.
  far_last   along the LAST residual in kernel order only: the last row of `rows`, or a rotation mu_q <- mu_q (x) expq(-d e_3) that
             moves the block's third residual by d = 60 of its standard deviations (|phi| stays below pi / 2, where the sign flip of
             e sits).  W is lower triangular, so the rows before the skip test do not see it: the pair must vanish through exp alone.

REFERENCES: nothing is restated here.  reference(name, variant) evaluates device_map_smoother_ref.backward_step or
pose_transition_ref.backward_step (index, index_ld, logp_ld, margin, eps_ref) and map_trajectory_ref.step on the long-double logp
(best, arg, near).  kernel_sums gives, from the same residuals, -z'z / 2 in kernel order, whole and up to the skip test.

Nothing in the package imports this file."""
import numpy as np

import device_map_ref as dm
import device_map_smoother_ref as S
import map_trajectory_ref as V
import pose_transition_ref as P

LD = np.longdouble
N_NONLIN, N, M = 8, 300, 70
SEED = 61803
FAR_SD = 60.0
SKIP = 746.0                                   # kBackwardSkip
WRAP_MARGIN = 0.05                             # every wrapped angle residual stays this far from +-pi
VARIANTS = ("base", "far_first", "far_last")
# the position of q0 in rows.  n_sel = n_plain + 4: p0 is the block alone; first: p1, p3a; last: p1a, p3; in the middle: the rest
QPOS = {"p0": 0, "p1": 0, "p1a": 1, "p2": 1, "p2a": 1, "p3": 3, "p3a": 0, "p4": 2, "p4a": 3}


class Layout:
    def __init__(self, name, rows, angle_rows, quat_rows):
        self.name, self.rows, self.angle_rows = name, tuple(rows), tuple(angle_rows)
        self.quat_rows = tuple(quat_rows) if quat_rows is not None else None
        self.n_sel = len(self.rows)
        self.n_plain = self.n_sel - 4 if self.quat_rows else -1             # -1: no block (the template's QP)
        self.n_res = self.n_sel - 1 if self.quat_rows else self.n_sel
        self.qpos = self.rows.index(self.quat_rows[0]) if self.quat_rows else -1
        # the term type gs_pick selects
        self.type = ("pose", self.n_plain, bool(self.angle_rows)) if self.quat_rows else ("gauss", self.n_res, bool(self.angle_rows))
        self.plain = tuple(r for r in self.rows if not (self.quat_rows and r in self.quat_rows))   # the caller's order
        self.skip_rows = self.n_plain if self.quat_rows else self.n_res // 2                        # rows of W before the skip test

    def residual_positions(self):
        """For every residual in the caller's order, the position in rows it comes from (the block: that of q0, three times)."""
        out = []
        for pos, r in enumerate(self.rows):
            if pos == self.qpos:
                out += [pos] * 3
            elif not (self.quat_rows and r in self.quat_rows):
                out.append(pos)
        return out

    def kernel_order(self):
        """The caller's residual indices in the order the kernels take them: plain rows first, the block last."""
        if not self.quat_rows:
            return list(range(self.n_res))
        pos = self.residual_positions()
        return [k for k in range(self.n_res) if pos[k] != self.qpos] + [k for k in range(self.n_res) if pos[k] == self.qpos]

    def angle_mask(self):
        """Bit p: position p of rows is an angle row (the probes' convention)."""
        return sum(1 << self.rows.index(a) for a in self.angle_rows)

    def args(self):
        return dict(rows=self.rows, angle_rows=self.angle_rows, quat_rows=self.quat_rows)


def _shuffled(rs, pool, n):
    while True:
        r = [int(v) for v in rs.permutation(pool)[:n]]
        if n < 2 or (r != sorted(r) and (n < 3 or r != sorted(r, reverse=True))):
            return r


def all_adjacent(positions):
    p = sorted(positions)
    return all(b - a == 1 for a, b in zip(p, p[1:]))


def _angle_positions(rs, n):
    """Which of n plain rows (by their order among the plain rows) are angles."""
    if n <= 2:
        return tuple(range(n))
    while True:
        pos = tuple(sorted(int(v) for v in rs.permutation(n)[:rs.randint(2, n)]))
        if not all_adjacent(pos):
            return pos


def _table():
    rs = np.random.RandomState(SEED)
    out = []
    for n in range(1, 9):
        for ang in (False, True):
            rows = _shuffled(rs, N_NONLIN, n)
            out.append(Layout(f"g{n}" + ("a" if ang else ""), rows, [rows[k] for k in _angle_positions(rs, n)] if ang else (), None))
    for n_plain in range(5):
        for ang in (False, True):
            if ang and n_plain == 0:
                continue
            name = f"p{n_plain}" + ("a" if ang else "")
            quat = _shuffled(rs, N_NONLIN, 4)
            plain = _shuffled(rs, [r for r in range(N_NONLIN) if r not in quat], n_plain)
            q = QPOS[name]
            out.append(Layout(name, plain[:q] + quat + plain[q:], [plain[k] for k in _angle_positions(rs, n_plain)] if ang else (), quat))
    return out


LAYOUTS = _table()
NAMES = [l.name for l in LAYOUTS]
_BY_NAME = {l.name: l for l in LAYOUTS}


def layout(name):
    return _BY_NAME[name]


def variants(name):
    return tuple(v for v in VARIANTS if not (v == "far_first" and layout(name).n_plain == 0))


FAR_CASES = [(n, v) for n in NAMES for v in variants(n) if v != "base"]

_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _base(name):
    l = layout(name)
    rs = np.random.RandomState(SEED + 1 + 101 * NAMES.index(name))
    pos = l.residual_positions()
    kind = ["quat" if p == l.qpos else "angle" if l.rows[p] in l.angle_rows else "plain" for p in pos]
    span = dict(plain=(0.04, 0.08), angle=(0.025, 0.035), quat=(0.012, 0.018))
    while True:
        cov = P._spd(rs, np.array([rs.uniform(*span[k]) for k in kind]))
        cov = 0.5 * (cov + cov.T)
        if np.linalg.cond(cov) < 1e3:
            break
    Lc = np.linalg.cholesky(cov)
    n_pred, n_succ = 2.0 * (Lc @ rs.standard_normal((l.n_res, N))), 2.0 * (Lc @ rs.standard_normal((l.n_res, M)))
    mu = np.zeros((l.n_sel, N))
    xs = rs.choice([-1.0, 1.0], (N_NONLIN, M)) * rs.uniform(1e3, 2e3, (N_NONLIN, M))           # the decoys
    k = 0
    while k < l.n_res:
        p = pos[k]
        if kind[k] == "quat":
            qc = P.expq(0.4 * rs.standard_normal(3)).reshape(4, 1)
            mu[p:p + 4] = P.qmul(qc * np.ones((1, N)), P.expq(n_pred[k:k + 3]))
            xs[list(l.quat_rows)] = P.qmul(qc * np.ones((1, M)), P.expq(n_succ[k:k + 3]))
            k += 3
            continue
        if kind[k] == "angle":
            mu[p] = 3.1 + n_pred[k] + S.TWO_PI * rs.randint(-3, 4, N)
            xs[l.rows[p]] = S.wrap(3.1 + n_succ[k])
        else:
            c = rs.uniform(-1.0, 1.0)
            mu[p], xs[l.rows[p]] = c + n_pred[k], c + n_succ[k]
        k += 1
    w = rs.random_sample(N) + 0.05
    w[:10] = 0.0
    w[-10:] = 0.0
    w /= w.sum()
    with np.errstate(divide="ignore"):
        delta = np.log(w)
    return dict(layout=l, mu=mu, xs_next=xs, cov=cov, w=w, delta=delta, u=rs.random_sample(M), displaced=np.zeros(0, dtype=np.int64), **l.args())


def inputs(name, variant="base"):
    """dict(layout, mu [n_sel x N], xs_next [8 x M], cov, w, delta, u, displaced, rows, angle_rows, quat_rows), built once."""
    def make():
        p = dict(_once(("in", name, "base"), lambda: _base(name)))
        if variant == "base":
            return p
        l = p["layout"]
        assert variant in variants(name), (name, variant)
        disp = np.nonzero(p["w"] > 0)[0][1::2]
        mu, order, pos = p["mu"].copy(), l.kernel_order(), l.residual_positions()
        k = order[0] if variant == "far_first" else order[-1]
        d = FAR_SD * np.sqrt(p["cov"][k, k])
        if pos[k] == l.qpos:                                               # far_last of a pose layout: the block's third residual
            q = slice(l.qpos, l.qpos + 4)
            mu[q, disp] = P.qmul(mu[q, disp], P.expq(np.array([[0.0], [0.0], [-d]])) * np.ones((1, disp.size)))
        else:
            mu[pos[k], disp] += d
        p.update(mu=mu, displaced=disp)
        return p
    return _once(("in", name, variant), make)


def probe_args(p):
    return dict(mu=p["mu"], xs_next=p["xs_next"], cov=p["cov"], rows=p["rows"], angle_rows=p["angle_rows"], quat_rows=p["quat_rows"])


def backward_step(p, **kw):
    """The existing checker of p's family on (possibly modified) inputs."""
    a = dict(p)
    a.update(kw)
    if a["quat_rows"] is not None:
        return P.backward_step(a["mu"], a["w"], a["xs_next"], a["cov"], a["u"], a["rows"], a["angle_rows"], a["quat_rows"])
    return S.backward_step(a["mu"], a["w"], a["xs_next"], a["cov"], a["u"], a["rows"], a["angle_rows"])


def logp_ld(p, **kw):
    """The long-double logp matrix [N x M] of (possibly modified) inputs."""
    a = dict(p)
    a.update(kw)
    if a["quat_rows"] is not None:
        return V.lp_pose(a["xs_next"], a["mu"], a["cov"], a["rows"], a["angle_rows"], a["quat_rows"])
    return V.lp_gauss(a["xs_next"], a["mu"], a["cov"], a["rows"], a["angle_rows"])


def reference(name, variant="base"):
    """backward_step of inputs(name, variant) plus best, arg, near of map_trajectory_ref.step on its long-double logp; once."""
    def make():
        p = inputs(name, variant)
        o = backward_step(p)
        o["best"], o["arg"], o["near"] = V.step(p["delta"], o["logp_ld"])
        return o
    return _once(("ref", name, variant), make)


def residuals(p, dtype=LD):
    """r [M x n_res x N] in the caller's order (pose_transition_ref.residual_vector; without a block it is the plain statement)."""
    return np.stack([P.residual_vector(p["xs_next"][:, j], p["mu"], p["rows"], p["angle_rows"], p["quat_rows"], dtype) for j in range(M)])


def kernel_sums(p):
    """(head, whole) [N x M], long double: -z'z / 2 over the rows of W before the skip test and over all rows, the residuals and cov
    taken in kernel order."""
    l = p["layout"]
    order = l.kernel_order()
    Lk = dm.chol(np.asarray(p["cov"], dtype=np.float64)[np.ix_(order, order)].astype(LD))
    r = residuals(p)
    head, whole = np.zeros((N, M), dtype=LD), np.zeros((N, M), dtype=LD)
    for j in range(M):
        z = dm.forward(Lk, r[j][order])
        head[:, j] = -LD(0.5) * np.sum(z[:l.skip_rows] ** 2, axis=0)
        whole[:, j] = -LD(0.5) * np.sum(z * z, axis=0)
    return head, whole


def worst_wrap_distance(p):
    """The smallest distance of a wrapped angle residual from +-pi over all pairs (pi if there is no angle row)."""
    worst = np.pi
    for a in p["angle_rows"]:
        r = S.wrap(p["xs_next"][a][None, :] - p["mu"][p["rows"].index(a)][:, None])
        worst = min(worst, float(np.pi - np.max(np.abs(r))))
    return worst
