#!/usr/bin/env python3
"""What one step of the fixed-lag smoother (csrc/rbpf_loc_fixedlag.hpp: the normaliser pass and its merge, the carry pass over
K = lag H columns, its merge, the enter kernel and the reducers) costs next to what a user had to run before it existed -- `lag`
marginal steps of the same term on the same inputs -- and next to one step of the running statistics, at N = M in {8192, 65 536},
in ONE process, every shape warmed up first: the protocol of tools/forward_stats_bench.py, whose compile report and input generators
this tool takes.

  fixed_lag   the probes rbpf_loc_fixed_lag_step / rbpf_loc_generic_fixed_lag_step between two device events, with a random incoming
              carry of K = lag H columns, lag in {4, 8, 16}, H = n (means only) and n (n + 3) / 2 (with covariances), n the state rows.
  marginal    the probes rbpf_loc_marginal_step / rbpf_loc_generic_marginal_step, log w_{t+1|T} = log w; the figure compared against
              is lag x one marginal step.
  forward     the probes rbpf_loc_forward_stats_step / rbpf_loc_generic_forward_stats_step.
  A window is one probe call of REPS event-timed repetitions (its median); the kinds of window alternate; the figure is the median
  of 5 windows, the spread (max - min) / median over the windows.  Terms: dense-mag; n_res = 1, 3, 6, 8; the pose form with 3 plain
  rows (the dense-mag inputs in model E's form).
  The expectation reported against: a step with means only at lag = 8 takes no longer than 8 marginal steps plus the larger spread.

  kb          the choice of the pass's column block KB: one dense-mag step at N = M = 65 536 with K = 56 (lag 8, means only) and
              K = 280 (with covariances), in this library and, with --kb-variant LIB, in a tuning variant built with the other KB
              (`_build.build(defines={"RBPF_FIXED_LAG_KB": 16}, out=LIB)`), timed in a child process of its own.

  session     one whole LocalizationSession.fixed_lag_estimates(8) from an empty carry and one smoothed_marginals() of N_T = 6 on
              model A of tests/device_map_smoother_ref.py with a torch `mean` handle, host clock, after a warm-up call each,
              alternated 5 times.

  The compile report (--only-compile-report, --this-report, --parent-report) is tools/marginal_smoother_bench.py's.
  Writes profiles/fixed_lag_bench.json.

Usage: fixed_lag_bench.py [--out FILE] [--sizes N ...] [--reps 3] [--windows 5] [--steps 6] [--kb-variant LIB] [--this-report FILE]
                          [--parent-report FILE]
       fixed_lag_bench.py --only-compile-report FILE [--root DIR]
       fixed_lag_bench.py --kb-probe                                       (prints the two timings of the loaded library as JSON)"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import marginal_smoother_bench as MB                                      # noqa: E402

LAGS = (4, 8, 16)


def columns(n, moments):
    return n if moments == 1 else n * (n + 3) // 2


def carry(K, N, seed=5):
    return np.random.default_rng(seed).standard_normal((K, N))


def compare(name, N, n, run_fl, run_marg, run_fwd, a):
    """run_fl(tau, moments, reps), run_marg(reps), run_fwd(reps) -> ms."""
    taus = {(lag, m): carry(lag * columns(n, m), N) for lag in LAGS for m in (1, 2)}
    for key, tau in taus.items():                                          # warm-up
        run_fl(tau, key[1], 1)
    run_marg(1)
    run_fwd(1)
    ms = {key: [] for key in taus}
    ms_marg, ms_fwd = [], []
    for _ in range(a.windows):
        for key, tau in taus.items():
            ms[key].append(run_fl(tau, key[1], a.reps))
        ms_marg.append(run_marg(a.reps))
        ms_fwd.append(run_fwd(a.reps))
    rec = dict(term=name, state_rows=n, marginal=MB.stats(ms_marg, N), forward=MB.stats(ms_fwd, N), fixed_lag=[])
    for (lag, m), v in ms.items():
        st = MB.stats(v, N)
        st.update(lag=lag, moments=m, K=lag * columns(n, m), lag_marginal_steps_ms=lag * rec["marginal"]["ms"],
                  ratio_to_lag_marginal_steps=st["ms"] / (lag * rec["marginal"]["ms"]), ratio_to_forward_step=st["ms"] / rec["forward"]["ms"])
        rec["fixed_lag"].append(st)
    e = next(r for r in rec["fixed_lag"] if r["lag"] == 8 and r["moments"] == 1)
    spread = max(e["spread"], rec["marginal"]["spread"])
    rec["verdict"] = dict(fixed_lag_ms=e["ms"], eight_marginal_steps_ms=e["lag_marginal_steps_ms"], larger_spread=spread,
                          expectation_met=bool(e["ms"] <= e["lag_marginal_steps_ms"] * (1.0 + spread)))
    print(json.dumps(rec), flush=True)
    return rec


def kb_probe(rbpf, reps, windows):
    """One dense-mag step at N = M = 65 536 with K = 56 and K = 280, medians of `windows` windows of `reps` repetitions."""
    import device_map_backward_bench as B
    N = 65536
    X, w, xs, dx, dt, Q, u = B.dense_mag_inputs(N, N)
    with np.errstate(divide="ignore"):
        lw = np.log(w)
    out = {}
    for K, m in ((56, 1), (280, 2)):
        tau = carry(K, N)
        rbpf.loc_fixed_lag_step(X, lw, xs, tau, dx, dt, Q, moments=m, reps=1)
        v = [rbpf.loc_fixed_lag_step(X, lw, xs, tau, dx, dt, Q, moments=m, reps=reps)[-1] for _ in range(windows)]
        out[f"K={K}"] = dict(ms=float(np.median(v)), windows_ms=[float(x) for x in v])
    return out


def session(rbpf, torch, dev, N, T, windows):
    import device_map_smoother_ref as S
    import generic_model_torch as gmt
    c = S.case("A", N, T)
    p = c.p
    tm = gmt.TorchGenericModel(c.m, p, dev)
    mean = lambda xn, dx, dt, Q: xn + tm.bend * torch.sin(xn) + tm.A @ dx.reshape(-1, 1)       # noqa: E731
    mp = rbpf.DeviceMap(rbpf.DeviceHandles(tm.dynModel, tm.measModel), p["mean"], p["V"], p["R"],
                        transition=rbpf.DeviceTransition(mean, c.cov_of))
    with rbpf.LocalizationSession(mp, p["odometry"], p["y"], p["x0_nonLin"], p["Q"], N, p["dt"], rng=rbpf.PhiloxRNG(3), keep_history=True,
                                  trace=True) as s:
        s.advance(T)
        s.sync()
        s.smoothed_marginals()                                             # warm-up
        s.fixed_lag_estimates(8, want=("mean", "cov"))
        ms_f, ms_s = [], []
        for _ in range(windows):
            s.reset_fixed_lag()
            t0 = time.perf_counter()
            out = s.fixed_lag_estimates(8, want=("mean", "cov", "mass"))
            ms_f.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            sm = s.smoothed_marginals(want=("mean", "cov"))
            ms_s.append((time.perf_counter() - t0) * 1e3)
    med = lambda v: float(np.median(v))                                    # noqa: E731
    return dict(model="A (n_res = 3)", N_T=T, lag=8, fixed_lag_estimates_ms=med(ms_f), smoothed_marginals_ms=med(ms_s),
                fixed_lag_estimates_windows_ms=ms_f, smoothed_marginals_windows_ms=ms_s, ratio=med(ms_f) / med(ms_s),
                worst_mass_error=float(np.max(np.abs(out["mass"] - 1.0))),
                means_against_smoothed_marginals=float(np.max(np.abs(out["mean"] - sm["mean"]))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fixed_lag_bench.json"))
    ap.add_argument("--sizes", type=int, nargs="*", default=[8192, 65536])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--kb-variant", default=None)
    ap.add_argument("--kb-probe", action="store_true")
    ap.add_argument("--this-report", default=None)
    ap.add_argument("--parent-report", default=None)
    ap.add_argument("--only-compile-report", default=None)
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    if a.only_compile_report:
        with open(a.only_compile_report, "w") as f:
            json.dump(MB.compile_report(a.root), f, indent=1)
            f.write("\n")
        return
    if a.kb_probe:
        rbpf = importlib.import_module("rao-blackwellized-slam-smoothing_amd")
        print(json.dumps(kb_probe(rbpf, a.reps, a.windows)))
        return
    doc = dict(tool="tools/fixed_lag_bench.py", device=None,
               timing=f"median of {a.windows} windows, a window = the median of {a.reps} event-timed repetitions of one step; the kinds of "
                      f"window alternate in one process, all warmed up first; spread = (max - min) / median over the windows; session: host "
                      f"clock, synchronised, median of {a.windows} alternated calls",
               expectation="a fixed-lag step with means only at lag = 8 takes no longer than 8 marginal steps plus the larger window spread",
               not_measured=["other N", "M != N", "N_T beyond the session's", "hardware counters", "what paces the carry pass"], runs=[])
    if a.sizes:                                                            # (--sizes with no value: the compile report alone, no device)
        import torch
        import device_map_backward_bench as B
        rbpf = importlib.import_module("rao-blackwellized-slam-smoothing_amd")
        dev = torch.device("cuda", torch.cuda.current_device())
        doc["device"] = torch.cuda.get_device_name(dev)
        doc["kb"] = dict(this_library=kb_probe(rbpf, a.reps, a.windows))
        if a.kb_variant:
            env = dict(os.environ, RBPF_LIB_PATH=os.path.abspath(a.kb_variant))
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--kb-probe", "--reps", str(a.reps), "--windows", str(a.windows)],
                                 env=env, stdout=subprocess.PIPE, text=True, check=True, timeout=300)
            doc["kb"]["variant"] = json.loads(res.stdout.strip().splitlines()[-1])
        print(json.dumps(doc["kb"]), flush=True)
    else:
        doc["not_measured"] = ["every timing: this file holds the compile report alone"]
    for N in a.sizes:
        rec = dict(N=N, M=N, terms=[])
        X, w, xs, dx, dt, Q, u = B.dense_mag_inputs(N, N)
        with np.errstate(divide="ignore"):
            lw = np.log(w)
        fS, fm = np.zeros((6, 6, N)), np.zeros((6, N))
        rec["terms"].append(compare("dense_mag", N, 7, lambda tau, m, r: rbpf.loc_fixed_lag_step(X, lw, xs, tau, dx, dt, Q, moments=m, reps=r)[-1],
                                    lambda r: rbpf.loc_marginal_step(X, lw, xs, lw, dx, dt, Q, reps=r)[-1],
                                    lambda r: rbpf.loc_forward_stats_step(X, lw, xs, fS, fm, dx, dt, Q, reps=r)[-1], a))
        for n_res in (1, 3, 6, 8):
            p = B.generic_inputs(n_res, N, N, False)
            lwp = np.log(p["w"])
            gS, gm = np.zeros((n_res, n_res, N)), np.zeros((n_res, N))
            rec["terms"].append(compare(
                f"n_res = {n_res}", N, p["xs_next"].shape[0],
                lambda tau, m, r: rbpf.device_map_fixed_lag_step(p["mu"], lwp, p["xs_next"], tau, p["cov"], angle_rows=p["angle_rows"], moments=m, reps=r)[-1],
                lambda r: rbpf.device_map_marginal_step(p["mu"], lwp, p["xs_next"], lwp, p["cov"], angle_rows=p["angle_rows"], reps=r)[-1],
                lambda r: rbpf.device_map_forward_stats_step(p["mu"], lwp, p["xs_next"], gS, gm, p["cov"], angle_rows=p["angle_rows"], reps=r)[-1], a))
        # the dense-mag inputs in the pose form: mu = (p + dx_pos, qRight(q) dq), cov = blkdiag(dt Q(1:3,1:3), dt Q(4:6,4:6))
        dq, q = dx[3:7], X[3:7]
        mu_q = np.vstack((dq[0] * q[0] - dq[1] * q[1] - dq[2] * q[2] - dq[3] * q[3], dq[0] * q[1] + dq[1] * q[0] + dq[2] * q[3] - dq[3] * q[2],
                          dq[0] * q[2] - dq[1] * q[3] + dq[2] * q[0] + dq[3] * q[1], dq[0] * q[3] + dq[1] * q[2] - dq[2] * q[1] + dq[3] * q[0]))
        mu = np.vstack((X[0:3] + dx[0:3, None], mu_q))
        cov = np.zeros((6, 6))
        cov[0:3, 0:3], cov[3:6, 3:6] = dt * Q[0:3, 0:3], dt * Q[3:6, 3:6]
        rec["terms"].append(compare("pose, 3 plain rows", N, 7,
                                    lambda tau, m, r: rbpf.device_map_fixed_lag_step(mu, lw, xs, tau, cov, quat_rows=(3, 4, 5, 6), moments=m, reps=r)[-1],
                                    lambda r: rbpf.device_map_marginal_step(mu, lw, xs, lw, cov, quat_rows=(3, 4, 5, 6), reps=r)[-1],
                                    lambda r: rbpf.device_map_forward_stats_step(mu, lw, xs, fS, fm, cov, quat_rows=(3, 4, 5, 6), reps=r)[-1], a))
        rec["session"] = session(rbpf, torch, dev, N, a.steps, a.windows)
        print(json.dumps(rec["session"]), flush=True)
        doc["runs"].append(rec)
    if a.this_report:
        with open(a.this_report) as f:
            doc["compile_report"] = dict(flags="--offload-arch=gfx950 -O3", this_tree=json.load(f))
        if a.parent_report:
            with open(a.parent_report) as f:
                old = json.load(f)
            new = doc["compile_report"]["this_tree"]
            changed = {k: dict(parent=v, this_tree=new.get(k)) for k, v in old.items() if new.get(k) != v}
            doc["compile_report"]["existing_kernels"] = len(old)
            doc["compile_report"]["existing_kernels_changed"] = changed
            doc["compile_report"]["new_kernels"] = [k for k in new if k not in old]
            doc["compile_report"]["new_kernels_with_scratch"] = [k for k, v in new.items() if k not in old and v["scratch_bytes_per_lane"]]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
