#!/usr/bin/env python3
"""What backward simulation by rejection sampling (csrc/rbpf_loc_reject.hpp) costs next to the all-pairs step on the same inputs, at
N = M in {8192, 65 536}, in ONE process, every shape warmed up first -- the protocol of tools/loc_backward_bench.py and
tools/marginal_smoother_bench.py:

  all_pairs  the probes rbpf_loc_backward_step / rbpf_loc_generic_backward_(pose_)step: prologue + all-pairs pass + locate.
  rejection  the probes rbpf_loc_backward_reject_step / rbpf_loc_generic_backward_reject_step with the device generator's tries:
             prologue + cdf + tries + compaction + the read-back of M' + the all-pairs pass on M' rows + commit, between two events.
  A window is one probe call of REPS event-timed repetitions (its median); the rejection and the all-pairs windows alternate; the
  figure is the median of 5 windows, the spread (max - min) / median over the windows.
  Terms: dense-mag; the Gaussian term at n_res = 1, 3, 6; the pose form with 3 plain rows (the dense-mag inputs in that form).
  Regimes: the cloud of predecessors 0.25, 0.5, 1 and 2 transition standard deviations wide, the successors drawn from random
  predecessors with one transition's noise.  Per regime: the ratio rejection / all-pairs (also where rejection loses), the measured
  acceptance per try = accepted trajectories / tries made, and the share of trajectories that fell back.

  t_try and R*: at N = M = 65 536 in the dense-mag map with every successor out of reach (acceptance 0, everything falls back),
  t_try = (step at R = R_FAR - step at R = 0) / R_FAR, t_pass = the all-pairs step, R* = t_pass / t_try; the default max_tries is
  rbpf.reject_default_max_tries(N, M, R*): the largest power of two not above R* at that size, scaled by N M / 65 536^2 below it.
  It is what the regimes of every size run with (--max-tries overrides it).  The same two times are measured at the other sizes
  too, to show what the scaled default stands against.
  max_tries = 0: the step must take no longer than the all-pairs step plus the larger window spread (reported per term and size).
  session    one whole LocalizationSession.backward_simulate of N_T = 6 in the dense-mag map per method, host clock, after a warm-up.

  The compile report is that of tools/marginal_smoother_bench.py (every kernel of csrc/rbpf_loc_smooth.hip and
  csrc/rbpf_loc_generic_smooth.hip: registers, LDS, scratch, occupancy, instruction count), stored with --this-report / --parent-report.
  Writes profiles/loc_reject_bench.json.

Usage: loc_reject_bench.py [--out FILE] [--sizes N ...] [--reps 3] [--windows 5] [--steps 6] [--max-tries R] [--this-report FILE]
                           [--parent-report FILE]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

SPREADS = (0.25, 0.5, 1.0, 2.0)
R_FAR = 512                                  # tries of the run that measures t_try: its step is then a fifth longer than at R = 0


def _expq(v):                                                              # [3 x K] -> unit quaternions [4 x K]
    a = np.linalg.norm(v, axis=0)
    return np.vstack((np.cos(a), np.sin(a) / np.where(a > 0, a, 1.0) * v))


def _qmul(a, b):
    return np.vstack((a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                      a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]))


def dense_mag_inputs(N, M, spread, seed=1):
    """tools/device_map_backward_bench.dense_mag_inputs with the cloud `spread` standard deviations wide."""
    import cases
    import localization_ref as R
    rs = np.random.RandomState(seed + N)
    dt, Q = 0.01, cases.Q_MAG
    sd = np.sqrt(dt * np.diag(Q))
    X = np.zeros((7, N))
    X[0:3] = np.array([[1.5], [-0.7], [0.3]]) + spread * sd[0:3, None] * rs.standard_normal((3, N))
    q0 = R._expq(0.4 * rs.standard_normal(3)).reshape(4, 1)
    X[3:7] = _qmul(q0, _expq(spread * sd[3:6, None] * rs.standard_normal((3, N))))
    dx = np.concatenate((0.05 * rs.standard_normal(3), R._expq(0.02 * rs.standard_normal(3))))
    w = rs.random_sample(N) + 0.05
    w /= w.sum()
    pick = rs.randint(N, size=M)
    xs = np.zeros((7, M))
    xs[0:3] = X[0:3, pick] + dx[0:3, None] + sd[0:3, None] * rs.standard_normal((3, M))
    xs[3:7] = _qmul(_qmul(dx[3:7].reshape(4, 1) * np.ones((1, M)), X[3:7, pick]), _expq(sd[3:6, None] * rs.standard_normal((3, M))))
    return dict(X=X, w=w, xs_next=xs, odo=dx, dt=dt, Q=Q, u=rs.random_sample(M))


def generic_inputs(n_res, N, M, spread, seed=1):
    """tools/device_map_backward_bench.generic_inputs (no angle row) with the cloud `spread` standard deviations wide."""
    rs = np.random.RandomState(seed + 10 * n_res + N)
    B = rs.standard_normal((n_res, n_res))
    cov = 0.02 * (B @ B.T) / n_res + 0.01 * np.eye(n_res)
    L = np.linalg.cholesky(cov)
    mu = rs.uniform(-1, 1, (n_res, 1)) + spread * (L @ rs.standard_normal((n_res, N)))
    w = rs.random_sample(N) + 0.05
    w /= w.sum()
    xs = mu[:, rs.randint(N, size=M)] + L @ rs.standard_normal((n_res, M))
    return dict(mu=mu, w=w, xs_next=xs, cov=cov, u=rs.random_sample(M), quat_rows=None)


def pose_inputs(d):
    """The dense-mag inputs in the pose form: mu = (p + dx_pos, qRight(q) dq), cov = blkdiag(dt Q(1:3,1:3), dt Q(4:6,4:6))."""
    X, dx, dt, Q = d["X"], d["odo"], d["dt"], d["Q"]
    mu = np.vstack((X[0:3] + dx[0:3, None], _qmul(dx[3:7].reshape(4, 1) * np.ones((1, X.shape[1])), X[3:7])))
    cov = np.zeros((6, 6))
    cov[0:3, 0:3], cov[3:6, 3:6] = dt * Q[0:3, 0:3], dt * Q[3:6, 3:6]
    return dict(mu=mu, w=d["w"], xs_next=d["xs_next"], cov=cov, u=d["u"], quat_rows=(3, 4, 5, 6))


def runners(rbpf, p):
    """(all_pairs(reps) -> ms, rejection(R, reps) -> (accepted_at, ms)) of one set of inputs."""
    if "X" in p:
        a = (p["X"], p["w"], p["xs_next"], p["odo"], p["dt"], p["Q"])
        return (lambda reps: rbpf.loc_backward_step(*a, p["u"], reps=reps)[2],
                lambda R, reps: rbpf.loc_backward_reject_step(*a, int(R), p["u"], reps=reps)[1:])
    a = (p["mu"], p["w"], p["xs_next"], p["cov"])
    return (lambda reps: rbpf.device_map_backward_step(*a, p["u"], quat_rows=p["quat_rows"], reps=reps)[2],
            lambda R, reps: rbpf.device_map_backward_reject_step(*a, int(R), p["u"], quat_rows=p["quat_rows"], reps=reps)[1:])


def stats(ms):
    med = float(np.median(ms))
    return dict(ms=med, windows_ms=[float(v) for v in ms], spread=float((max(ms) - min(ms)) / med))


def compare(rbpf, p, R, a):
    """Alternated windows of the rejection step at R tries and the all-pairs step on the inputs p."""
    pairs, rej = runners(rbpf, p)
    rej(R, 1)                                                              # warm-up
    pairs(1)
    ms_rej, ms_pairs, acc = [], [], None
    for _ in range(a.windows):
        acc, ms = rej(R, a.reps)
        ms_rej.append(ms)
        ms_pairs.append(pairs(a.reps))
    M = acc.size
    tries = int(np.sum(np.where(acc >= 0, acc + 1, R)))
    rec = dict(max_tries=int(R), rejection=stats(ms_rej), all_pairs=stats(ms_pairs), accepted=int(np.sum(acc >= 0)), n_fallback=int(np.sum(acc < 0)),
               n_tries=tries, acceptance_per_try=float(np.sum(acc >= 0)) / max(tries, 1), fallback_share=float(np.sum(acc < 0)) / M)
    rec["ratio"] = rec["rejection"]["ms"] / rec["all_pairs"]["ms"]
    rec["slack_ms"] = max(rec["rejection"]["spread"] * rec["rejection"]["ms"], rec["all_pairs"]["spread"] * rec["all_pairs"]["ms"])
    return rec


def inputs_of(term, N, spread):
    if term == "dense_mag":
        return dense_mag_inputs(N, N, spread)
    if term == "pose, 3 plain rows":
        return pose_inputs(dense_mag_inputs(N, N, spread))
    return generic_inputs(int(term.split("=")[1]), N, N, spread)


TERMS = ("dense_mag", "n_res = 1", "n_res = 3", "n_res = 6", "pose, 3 plain rows")


def measure_r_star(rbpf, a, N=65536):
    p = dense_mag_inputs(N, N, 1.0)
    p["xs_next"] = p["xs_next"].copy()
    p["xs_next"][0] += 10.0                                                # every successor out of reach: every exp is 0
    zero, far = compare(rbpf, p, 0, a), compare(rbpf, p, R_FAR, a)
    assert far["accepted"] == 0 and zero["n_fallback"] == N
    t_try = (far["rejection"]["ms"] - zero["rejection"]["ms"]) / R_FAR
    t_pass = float(np.median([zero["all_pairs"]["ms"], far["all_pairs"]["ms"]]))
    r_star = t_pass / t_try
    return dict(N=N, M=N, term="dense_mag, every successor out of reach", R_far=R_FAR, step_ms_at_R_far=far["rejection"]["ms"],
                step_ms_at_R_0=zero["rejection"]["ms"], t_try_ms=t_try, t_pass_ms=t_pass, R_star=r_star,
                largest_power_of_two_not_above=int(2 ** int(np.floor(np.log2(r_star)))) if r_star >= 1 else 0,
                note="a rejected try of an out-of-reach successor ends after the position term; a try that reaches the orientation term costs more")


def session(rbpf, N, T, R):
    import localization_ref as Rf
    c = Rf.loc_case(64, T, 13)
    mp = rbpf.DenseMagMap(rbpf.DenseMagModel(c["NN"], c["L"]), c["mean"], c["V"], c["sigma2"])
    rec = dict(map="dense-mag, m = 13, tests/localization_ref.loc_case", N=N, M=N, N_T=T, max_tries=int(R))
    with rbpf.LocalizationSession(mp, c["odometry"], c["y"], c["x0_nonLin"], c["Q"], N, c["dt"], rng=rbpf.PhiloxRNG(3), keep_history=True,
                                  trace=True) as s:
        s.advance(T)
        s.finish()
        for method, kw in (("all_pairs", {}), ("rejection", dict(method="rejection", max_tries=int(R)))):
            want = ("index", "n_fallback", "n_tries") if kw else ("index",)
            s.backward_simulate(N, rng=rbpf.PhiloxRNG(4), want=want, **kw)    # warm-up
            t0 = time.perf_counter()
            out = s.backward_simulate(N, rng=rbpf.PhiloxRNG(5), want=want, **kw)
            rec[method + "_ms"] = (time.perf_counter() - t0) * 1e3
            if kw:
                rec["n_fallback"] = [int(v) for v in out["n_fallback"]]
                rec["n_tries"] = [int(v) for v in out["n_tries"]]
    rec["ratio"] = rec["rejection_ms"] / rec["all_pairs_ms"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loc_reject_bench.json"))
    ap.add_argument("--sizes", type=int, nargs="*", default=[8192, 65536])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--max-tries", type=int, default=None)
    ap.add_argument("--this-report", default=None)
    ap.add_argument("--parent-report", default=None)
    a = ap.parse_args()
    doc = dict(tool="tools/loc_reject_bench.py", device=None,
               timing=f"median of {a.windows} windows, a window = the median of {a.reps} event-timed repetitions of one step; the rejection and "
                      f"the all-pairs windows alternate in one process on the same inputs, both warmed up first; spread = (max - min) / median "
                      f"over the windows; session: host clock, synchronised",
               not_measured=["other N", "M != N", "angle rows", "n_res = 8 and the pose form with other plain-row counts", "a DeviceMap session (torch handle per step)",
                             "hardware counters: what paces the tries kernel is a supposition"], runs=[])
    if a.sizes:
        import torch
        rbpf = importlib.import_module("rao-blackwellized-slam-smoothing_amd")
        doc["device"] = torch.cuda.get_device_name(torch.device("cuda", torch.cuda.current_device()))
        doc["r_star"] = measure_r_star(rbpf, a)
        print(json.dumps(doc["r_star"]), flush=True)
        for N in a.sizes:
            R = a.max_tries if a.max_tries is not None else rbpf.reject_default_max_tries(N, N, doc["r_star"]["R_star"])
            rec = dict(N=N, M=N, max_tries_of_the_regimes=int(R), terms=[])
            if N != doc["r_star"]["N"]:
                rec["r_star_at_this_size"] = measure_r_star(rbpf, a, N)
                print(json.dumps(rec["r_star_at_this_size"]), flush=True)
            for term in TERMS:
                t = dict(term=term, regimes=[])
                for spread in SPREADS:
                    r = compare(rbpf, inputs_of(term, N, spread), R, a)
                    r["spread_sd"] = spread
                    t["regimes"].append(r)
                    print(json.dumps(dict(N=N, term=term, spread_sd=spread, ratio=r["ratio"], acceptance_per_try=r["acceptance_per_try"],
                                          fallback_share=r["fallback_share"], rejection_ms=r["rejection"]["ms"], all_pairs_ms=r["all_pairs"]["ms"])),
                          flush=True)
                if term == "dense_mag" and R >= 8:                        # the same regimes with an eighth of the tries: what the tail costs
                    t["regimes_at_an_eighth_of_the_tries"] = []
                    for spread in SPREADS:
                        r = compare(rbpf, inputs_of(term, N, spread), R // 8, a)
                        r["spread_sd"] = spread
                        t["regimes_at_an_eighth_of_the_tries"].append(r)
                        print(json.dumps(dict(N=N, term=term, max_tries=R // 8, spread_sd=spread, ratio=r["ratio"],
                                              fallback_share=r["fallback_share"], rejection_ms=r["rejection"]["ms"])), flush=True)
                z = compare(rbpf, inputs_of(term, N, 1.0), 0, a)
                t["max_tries_0"] = dict(rejection_ms=z["rejection"]["ms"], all_pairs_ms=z["all_pairs"]["ms"], slack_ms=z["slack_ms"],
                                        no_longer_than_all_pairs_plus_spread=bool(z["rejection"]["ms"] <= z["all_pairs"]["ms"] + z["slack_ms"]),
                                        windows=dict(rejection=z["rejection"]["windows_ms"], all_pairs=z["all_pairs"]["windows_ms"]))
                print(json.dumps(dict(N=N, term=term, max_tries_0=t["max_tries_0"])), flush=True)
                rec["terms"].append(t)
            rec["session"] = session(rbpf, N, a.steps, R)
            print(json.dumps(rec["session"]), flush=True)
            doc["runs"].append(rec)
    else:
        doc["not_measured"] = ["every timing: this file holds the compile report alone"]
    if a.this_report:
        with open(a.this_report) as f:
            doc["compile_report"] = dict(flags="--offload-arch=gfx950 -O3", this_tree=json.load(f))
        if a.parent_report:
            with open(a.parent_report) as f:
                old = json.load(f)
            new = doc["compile_report"]["this_tree"]
            doc["compile_report"]["existing_kernels_unchanged"] = all(new.get(k) == v for k, v in old.items())
            doc["compile_report"]["new_kernels_with_scratch"] = [k for k, v in new.items() if k not in old and v["scratch_bytes_per_lane"]]
            doc["compile_report"]["parent"] = "every kernel of the parent commit is in this_tree with the same figures" if \
                doc["compile_report"]["existing_kernels_unchanged"] else old
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
