#!/usr/bin/env python3
"""The protocol behind the reference's only quantitative artefact, examples/slam-dense-mag/boxplot-mag.png, on the device path.

examples/slam-dense-mag/main.m:37-57: for each magnetometer disturbance o in magDist = [0; 1; 5; 10] (added to the second body
axis of every measurement, run_dense3D_magfield.m:81 `y = y + params.magDisti`) run nSim = 20 simulations of
run_dense3D_magfield(params): synthetic bean_6D data (3 laps x 64 points, T = 192), m = 512 basis functions, N_P = 100,
particleFilter, particleSmoother (covariance form) with N_K = 10, and the EKF baseline (ekf_dense.m).  Per simulation
(main.m:50-53, run_dense3D_magfield.m:155-183,216-237,252-255): the position RMSE after a Procrustes alignment, per axis, then
sqrt(mean(.^2)) over the axes, for the EKF, the filter's weighted-mean trajectory and the LAST smoother iteration -- the three
boxes per disturbance of boxplot-mag.png (main.m:70-73: columns [1,3] of rmses_ekf_pf and rmses_ps(:,end)).

Read off the PNG (y axis [0, 0.3] m, main.m:80): o = 0 medians ~ EKF 0.125 / PF 0.14 / PS 0.115 m; o = 10 ~ EKF 0.26 / PF 0.145 /
PS 0.13 m; PS below PF in all four panels; the EKF degrades with the disturbance, the particle methods hardly do.

    python tools/boxplot_mag.py [n_sim=20] [N_K=10] [N_P=100] [m=512] [ekf=host|device] [out=profiles/r03_boxplot_mag.json]

ekf=device runs the EKF on the device (ekf.ekf_dense_batch): the four disturbance levels of a simulation are one call.  The
default, ekf=host, is the numpy recursion over the device helper kernels.

MATLAB's random stream cannot be replayed here, so the simulations use numpy data seeds 1..n_sim (one data set per simulation,
shared by the four disturbance levels -- the reference draws fresh data for every run) and device Philox streams."""
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MAG_DIST = (0.0, 1.0, 5.0, 10.0)                                            # main.m:41, second column


def run_protocol(n_sim=20, N_K=10, N_P=100, m=512, N_T=192, levels=MAG_DIST, verbose=False, ekf="host"):
    if ekf not in ("host", "device"):
        raise ValueError('ekf must be "host" or "device"')
    ekf_on_device = ekf == "device"
    rbpf = importlib.import_module("rao-blackwellized-slam-smoothing_amd")
    dg = importlib.import_module("rao-blackwellized-slam-smoothing_amd.datagen")
    mt = importlib.import_module("rao-blackwellized-slam-smoothing_amd.metrics")
    ekf = importlib.import_module("rao-blackwellized-slam-smoothing_amd.ekf")
    import bench                                                             # Q and theta of main.m:22-23
    Q, theta, dt = bench.q_mag(), bench.THETA_MAG, 0.01
    total = lambda rp: float(np.sqrt(np.mean(np.asarray(rp) ** 2)))          # noqa: E731   main.m:50-53
    rows = {o: dict(ekf=[], pf=[], ps=[], ps_iter=[]) for o in levels}
    secs = dict(ekf=0.0, pf=0.0, ps=0.0)
    for sim in range(1, n_sim + 1):
        d = dg.bean_6D(N_T, Q, theta, dt, seed=sim)
        mdl, x0_lin, P0_lin, R = rbpf.dense_mag_prior(m, d["LL"], theta)
        n = mdl.nLin
        if ekf_on_device:                                                    # the levels of this simulation in one call
            t0 = time.perf_counter()
            x0 = np.concatenate((d["initState"][0:3], np.zeros(3), np.asarray(x0_lin).ravel()))
            P0 = np.zeros((6 + n, 6 + n))
            P0[6:, 6:] = P0_lin
            nl = len(levels)
            rep = lambda a: np.stack([np.asarray(a, dtype=np.float64)] * nl)                       # noqa: E731
            xf_b, qnb_b, _ = ekf.ekf_dense_batch([mdl] * nl, rep(d["LL"]), rep(d["dx"]), np.stack([d["y"] + np.array([0.0, o, 0.0]) for o in levels]),
                                                 rep(x0), rep(d["initState"][3:7]), rep(P0), Q, R, dt, keep_P=False)
            secs["ekf"] += time.perf_counter() - t0
        for io, o in enumerate(levels):
            y = d["y"] + np.array([0.0, o, 0.0])                             # run_dense3D_magfield.m:81
            t0 = time.perf_counter()
            if ekf_on_device:
                xf, qnb = xf_b[io], qnb_b[io]
            else:
                x0 = np.concatenate((d["initState"][0:3], np.zeros(3), np.asarray(x0_lin).ravel()))   # :248-250
                P0 = np.zeros((6 + n, 6 + n))
                P0[6:, 6:] = P0_lin
                xf, qnb, _ = ekf.ekf_dense(mdl, d["LL"], d["dx"], y, x0, d["initState"][3:7], P0, Q, R, dt)
            rows[o]["ekf"].append(total(mt.rmse_dense_mag(d["pos"], d["quat"], np.vstack((xf[0:3], qnb)))[0]))
            t1 = time.perf_counter()
            out = rbpf.particleFilter(mdl.dynModel, mdl.measModel, d["dx"], y, d["initState"], x0_lin, P0_lin, Q, R, N_P, dt,
                                      rng=rbpf.PhiloxRNG(1000 + sim))
            rows[o]["pf"].append(total(mt.rmse_dense_mag(d["pos"], d["quat"], out[1])[0]))          # weighted mean, :161
            t2 = time.perf_counter()
            XNK, _, _ = rbpf.particleSmoother(mdl.dynModel, mdl.measModel, mdl.dynResNorm, d["dx"], y, d["initState"], x0_lin,
                                              P0_lin, Q, R, N_P, N_K, dt, rng=rbpf.PhiloxRNG(2000 + sim))
            it = [total(mt.rmse_dense_mag(d["pos"], d["quat"], XNK[:, :, k])[0]) for k in range(N_K)]
            rows[o]["ps"].append(it[-1])                                     # rmses_ps(:,end), main.m:72
            rows[o]["ps_iter"].append(it)
            t3 = time.perf_counter()
            secs["ekf"] += t1 - t0
            secs["pf"] += t2 - t1
            secs["ps"] += t3 - t2
            if verbose:
                print(f"sim {sim:2d} o={o:4.1f}  EKF {rows[o]['ekf'][-1]:.4f}  PF {rows[o]['pf'][-1]:.4f}  PS {it[-1]:.4f}", flush=True)
    q = lambda v: [round(float(x), 4) for x in np.percentile(v, [25, 50, 75])]   # noqa: E731
    table = []
    for o in levels:
        r = rows[o]
        table.append(dict(disturbance=o, n_sim=n_sim,
                          ekf_q25_median_q75=q(r["ekf"]), pf_q25_median_q75=q(r["pf"]), ps_q25_median_q75=q(r["ps"]),
                          ps_median_by_iteration=[round(float(x), 4) for x in np.median(np.asarray(r["ps_iter"]), axis=0)],
                          ekf=[round(x, 4) for x in r["ekf"]], pf=[round(x, 4) for x in r["pf"]], ps=[round(x, 4) for x in r["ps"]]))
    return dict(protocol="examples/slam-dense-mag/main.m:37-57 (boxplot-mag.png)", ekf=("device" if ekf_on_device else "host"), N_P=N_P, N_K=N_K, N_T=N_T, m=m, n_sim=n_sim,
                smoother="particleSmoother (covariance form), last iteration", filter="particleFilter, weighted mean",
                seconds=dict((k, round(v, 2)) for k, v in secs.items()), table=table,
                reference_png_medians_read_by_eye={"0": dict(ekf=0.125, pf=0.14, ps=0.115), "10": dict(ekf=0.26, pf=0.145, ps=0.13)})


def check_ordering(res, slack=1.0):
    """What boxplot-mag.png shows: PS median < PF median at all four disturbances; the EKF median
    grows with the disturbance and exceeds the PF's at o = 10; the o = 0 medians lie in [0.08, 0.20] m.  slack < 1 lets
    neighbouring EKF medians differ by that factor the wrong way (o = 0 and o = 1 are within 2 % of each other over 20 runs)."""
    med = {r["disturbance"]: (r["ekf_q25_median_q75"][1], r["pf_q25_median_q75"][1], r["ps_q25_median_q75"][1]) for r in res["table"]}
    problems = []
    for o, (e, p, s) in med.items():
        if not s < p:
            problems.append(f"o={o}: PS median {s} is not below PF median {p}")
    lv = sorted(med)
    if not all(slack * med[a][0] <= med[b][0] for a, b in zip(lv[:-1], lv[1:])) or not med[lv[0]][0] < med[lv[-1]][0]:
        problems.append(f"EKF medians do not grow with the disturbance: {[med[o][0] for o in lv]}")
    if not med[lv[-1]][0] > med[lv[-1]][1]:
        problems.append(f"o={lv[-1]}: EKF median {med[lv[-1]][0]} does not exceed PF median {med[lv[-1]][1]}")
    for name, v in zip(("EKF", "PF", "PS"), med[lv[0]]):
        if not 0.08 <= v <= 0.20:
            problems.append(f"o={lv[0]}: {name} median {v} outside [0.08, 0.20] m")
    return problems


if __name__ == "__main__":
    kw = dict(a.split("=") for a in sys.argv[1:])
    out_path = kw.pop("out", os.path.join(ROOT, "profiles", "r03_boxplot_mag.json"))
    res = run_protocol(verbose=True, ekf=kw.pop("ekf", "host"), **{k: int(v) for k, v in kw.items()})
    res["ordering_problems"] = check_ordering(res)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("disturbance |  EKF q25/med/q75        |  PF (weighted mean)     |  PS (last iteration)")
    for r in res["table"]:
        print(f"{r['disturbance']:11.1f} | {r['ekf_q25_median_q75']} | {r['pf_q25_median_q75']} | {r['ps_q25_median_q75']}")
    print("seconds:", res["seconds"], " ordering problems:", res["ordering_problems"] or "none")
