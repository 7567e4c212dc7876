#!/usr/bin/env python3
"""What one backward step of the backward-simulation smoother for localisation costs (rbpf_loc_backward_simulate), at
N = M (particles = trajectories) in {8192, 65 536}, on an m = 13 map with the examples' Q and dt = 0.01, next to the forward
filter's step of the same session.

Per size the tool records
  forward_ms_per_step     the localisation filter: host clock around advance(T - 1) + sync, keep_history = 1 and trace = 1
  backward_ms_per_step    the probe rbpf_loc_backward_step on the session's own arrays (X[T-2], w[T-2], xs = X[T-1] gathered by a
                          draw from w[T-1]): median over REPS repetitions of the device time of prologue + all-pairs pass +
                          merge/locate, between two events
  pairs_per_s             N M / that time
  session_ms_per_step     host clock around backward_simulate(M) / T: the same kernels plus the Philox fill, the gathers, the means
                          and the copies back
  fp64_ops_per_pair       counted from csrc/rbpf_loc_smooth.hip as written (a multiply and an add count one each, no contraction
                          assumed): 87 additions / multiplications + 1 sqrt + 1 division + 1 atan2 + 1 exp for a pair that is not
                          skipped; 26 for a pair skipped after its position term
  skipped_fraction        the share of the pairs whose position term alone puts them 746 below the row's maximum (host count on a
                          sample of the trajectories; such a pair costs the position term only)
Writes one JSON document (default profiles/loc_backward_bench.json).

Usage: loc_backward_bench.py [--out FILE] [--sizes N ...] [--steps 8] [--reps 5]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
rbpf = importlib.import_module("rao-blackwellized-slam-smoothing_amd")

OPS = dict(add_mul=87, sqrt=1, div=1, atan2=1, exp=1, skipped_pair_add_mul=26)


def skipped_fraction(X, w, xs_next, odo, dt, Q, n_sample=16):
    """Host count with the restatement's formulas: pairs whose log w + position term is 746 below the row's maximum."""
    import localization_smoother_ref as S
    Sp, _ = S.noise_inverses(dt, Q)
    with np.errstate(divide="ignore"):
        lw = np.log(w)
    js = np.linspace(0, xs_next.shape[1] - 1, n_sample).astype(int)
    frac = []
    for j in js:
        z = Sp @ (xs_next[0:3, j:j + 1] - X[0:3] - np.asarray(odo)[0:3, None])
        lpos = lw - 0.5 * np.sum(z * z, axis=0)
        l = lw + S.logp(xs_next[:, j], X, odo, dt, Q)
        frac.append(float(np.mean(lpos < np.max(l) - 746.0)))
    return float(np.mean(frac))


def run(N, T, reps):
    import localization_ref as R
    c = R.loc_case(64, T, 13)                                              # the map, the path and the odometry; N_P is set below
    mp = rbpf.DenseMagMap(rbpf.DenseMagModel(c["NN"], c["L"]), c["mean"], c["V"], c["sigma2"])
    rec = dict(N=N, M=N, N_T=T)
    with rbpf.LocalizationSession(mp, c["odometry"], c["y"], c["x0_nonLin"], c["Q"], N, c["dt"], rng=rbpf.PhiloxRNG(3),
                                  keep_history=True, trace=True) as s:
        s.advance(1)
        s.sync()
        t0 = time.perf_counter()
        s.advance(T - 1)
        s.sync()
        rec["forward_ms_per_step"] = (time.perf_counter() - t0) / (T - 1) * 1e3
        fwd = s.finish(extras=True)
        X = s.history()
        s.backward_simulate(N, rng=rbpf.PhiloxRNG(4), want=("index",))     # warm-up
        t0 = time.perf_counter()
        out = s.backward_simulate(N, rng=rbpf.PhiloxRNG(5), want=("index",))
        rec["session_ms_per_step"] = (time.perf_counter() - t0) / T * 1e3
    W = fwd["trace_w"]
    idx_last = out["index"][:, T - 1]
    xs_next = X[:, idx_last, T - 1]
    u = rbpf.PhiloxRNG(5).backward_uniforms(N, T)[T - 2]
    args = (X[:, :, T - 2], W[:, T - 2], xs_next, c["odometry"][T - 2], c["dt"], c["Q"], u)
    index, _, ms = rbpf.loc_backward_step(*args, reps=reps)
    rec["probe_equals_session"] = bool(np.array_equal(index, out["index"][:, T - 2]))
    rec["backward_ms_per_step"] = ms
    rec["pairs_per_s"] = float(N) * N / (ms * 1e-3)
    rec["skipped_fraction"] = skipped_fraction(*args[:6])
    rec["n_eff_at_that_step"] = float(1.0 / np.sum(W[:, T - 2] ** 2))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loc_backward_bench.json"))
    ap.add_argument("--sizes", type=int, nargs="+", default=[8192, 65536])
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    doc = dict(tool="tools/loc_backward_bench.py", map="m = 13, tests/localization_ref.loc_case", fp64_ops_per_pair=OPS,
               timing=f"forward / session: host clock, synchronised; backward step: median of {a.reps} event-timed repetitions",
               runs=[])
    for N in a.sizes:
        doc["runs"].append(run(N, a.steps, a.reps))
        print(json.dumps(doc["runs"][-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
