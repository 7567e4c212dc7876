#!/usr/bin/env python3
"""examples/mag-localization-mapping on the device path with synthetic data (the recorded robot data set is not part of this
repository): draw a field and a 'bean_6D' path, build the map once by batch regression (DenseMagMap.from_data, run_localization.m:
134-151) and once by running the device SLAM filter over the training path (DenseMagMap.from_posterior), then localise the path
GLOBALLY -- initial positions uniform over the path's bounding box (:156-160) -- at N_P = 1000 and 65 536.

    python tools/mag_localization_demo.py [N_T=120] [m=1000] [seed=1] [out=profiles/localization_demo.json]

Prints one JSON line per run (position error of traj_mean over time, step time); nothing is asserted on these numbers."""
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
rbpf = importlib.import_module("rao-blackwellized-slam-smoothing_amd")
dg = importlib.import_module("rao-blackwellized-slam-smoothing_amd.datagen")

Q = np.diag(np.concatenate((10 ** 2 * np.array([0.05 ** 2, 0.05 ** 2, 0.01 ** 2]), (np.array([0.01, 0.01, 0.3]) * np.pi / 180) ** 2)))
THETA = np.array([650.0, 1.2, 200.0, 10.0])


def main():
    a = sys.argv[1:]
    N_T = int(a[0]) if len(a) > 0 else 120
    m = int(a[1]) if len(a) > 1 else 1000
    seed = int(a[2]) if len(a) > 2 else 1
    out = a[3] if len(a) > 3 else os.path.join(ROOT, "profiles", "localization_demo.json")
    dt = 0.01
    d = dg.bean_6D(N_T, Q, THETA, dt, seed=seed, m_sim=2000)
    model, x0_lin, P0, R = rbpf.dense_mag_prior(m, d["LL"], THETA)
    pos = d["pos"].T
    y_nav = np.stack([dg._quat2rmat(d["quat"][t]) @ d["y"][t] for t in range(N_T)])
    maps = {"from_data": rbpf.DenseMagMap.from_data(model, pos, y_nav, THETA)}
    t0 = time.perf_counter()
    f = rbpf.particleFilter(model.dynModel, model.measModel, d["dx"], d["y"], d["initState"], x0_lin, P0, Q, R, 64, dt,
                            rng=rbpf.PhiloxRNG(seed), want_xn_traj=False)
    slam_s = time.perf_counter() - t0
    maps["from_posterior"] = rbpf.DenseMagMap.from_posterior(model, f[2], f[4], float(THETA[3]))
    rs = np.random.RandomState(seed + 1)
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    results = []
    for name, mp in maps.items():
        for N_P in (1000, 65536):
            x0 = np.repeat(d["initState"].reshape(7, 1), N_P, axis=1)
            x0[0] = lo[0] + (hi[0] - lo[0]) * rs.random_sample(N_P)
            x0[1] = lo[1] + (hi[1] - lo[1]) * rs.random_sample(N_P)
            with rbpf.LocalizationSession(mp, d["dx"], d["y"], x0, Q, N_P, dt, rng=rbpf.PhiloxRNG(seed)) as s:
                s.advance(2)
                s.sync()
                t0 = time.perf_counter()
                s.advance(N_T - 2)
                s.sync()
                step_ms = (time.perf_counter() - t0) * 1e3 / (N_T - 2)
                b = s.finish()
            err = np.linalg.norm(b["traj_mean"][0:3] - d["pos"], axis=0)
            r = dict(map=name, N_P=N_P, m=m, N_T=N_T, step_ms=step_ms, slam_filter_s=slam_s if name == "from_posterior" else None,
                     first_degenerate_step=b["first_degenerate_step"],
                     pos_err_m=[float(e) for e in err[:: max(N_T // 12, 1)]], pos_err_final_m=float(err[-1]))
            print(json.dumps(r), flush=True)
            results.append(r)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
