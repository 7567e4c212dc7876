#!/usr/bin/env python3
"""The EKF baseline of examples/slam-dense-mag, host recursion against the device recursion, at the Monte-Carlo protocol's size
(main.m:37-57: m = 512, N_T = 192, Q and theta of main.m:22-23, 20 data sets x 4 magnetometer disturbances = 80 runs).

    python tools/ekf_bench.py [out=profiles/ekf_device_bench.json] [reps=5] [host_reps=3] [batches=1,4,80] [kernel_stats=DIR]
    python tools/ekf_bench.py trace_only=1 [batches=80]        # the workload alone, to run under a kernel tracer

Records, all on the same machine in the same session:
  * host seconds per run: ekf.ekf_dense (numpy recursion, two synchronous helper-kernel calls per step), median of host_reps;
  * device seconds per call of ekf.ekf_dense_batch with keep_P=False at every batch size: a host clock around the whole call
    (packing, uploads of P0, 2 N_T + 2 launches, the synchronise, downloads), median / min / max of reps after one warm-up call;
  * with kernel_stats=DIR (the output directory of `rocprofv3 --kernel-trace --stats --output-format csv -- python
    tools/ekf_bench.py trace_only=1`): the average time of ekf_update_kernel and ekf_gain_kernel per launch at the traced batch
    size, and the update kernel's rate against its bytes, one read and one write of B n^2 8 bytes per step.
The device figures need a GPU; without one the tool fails (no fallback)."""
import csv
import glob
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MAG_DIST = (0.0, 1.0, 5.0, 10.0)


def protocol_runs(B, m=512, N_T=192):
    """The first B runs of the protocol: data set sim = 1 + b // 4 with disturbance MAG_DIST[b % 4]."""
    rbpf = importlib.import_module("rao-blackwellized-slam-smoothing_amd")
    dg = importlib.import_module("rao-blackwellized-slam-smoothing_amd.datagen")
    import bench
    Q, theta, dt = bench.q_mag(), bench.THETA_MAG, 0.01
    sims, runs = {}, []
    for b in range(B):
        sim = 1 + b // len(MAG_DIST)
        if sim not in sims:
            d = dg.bean_6D(N_T, Q, theta, dt, seed=sim)
            mdl, x0_lin, P0_lin, R = rbpf.dense_mag_prior(m, d["LL"], theta)
            n = mdl.nLin
            P0 = np.zeros((6 + n, 6 + n))
            P0[6:, 6:] = P0_lin
            sims[sim] = dict(d=d, mdl=mdl, R=R, P0=P0, x0=np.concatenate((d["initState"][0:3], np.zeros(3), np.asarray(x0_lin).ravel())))
        s = sims[sim]
        runs.append(dict(mdl=s["mdl"], LL=s["d"]["LL"], odo=s["d"]["dx"], y=s["d"]["y"] + np.array([0.0, MAG_DIST[b % 4], 0.0]),
                         x0=s["x0"], q0=s["d"]["initState"][3:7], P0=s["P0"], R=s["R"]))
    return runs, Q, dt


def device_call(ekf, runs, Q, dt):
    st = lambda k: np.stack([r[k] for r in runs])                            # noqa: E731
    return ekf.ekf_dense_batch([r["mdl"] for r in runs], st("LL"), st("odo"), st("y"), st("x0"), st("q0"), st("P0"), Q, st("R"), dt,
                               keep_P=False)


def kernel_stats(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_stats.csv under {d}")
    out = {}
    for r in csv.DictReader(open(files[0])):
        for name in ("ekf_update_kernel", "ekf_gain_kernel"):
            if name in r["Name"]:
                out[name] = dict(calls=int(r["Calls"]), average_us=float(r["AverageNs"]) / 1e3, total_ms=float(r["TotalDurationNs"]) / 1e6)
    return out


def main():
    kw = dict(a.split("=") for a in sys.argv[1:])
    batches = [int(v) for v in kw.get("batches", "1,4,80").split(",")]
    reps, host_reps = int(kw.get("reps", 5)), int(kw.get("host_reps", 3))
    m, N_T = int(kw.get("m", 512)), int(kw.get("N_T", 192))
    rbpf = importlib.import_module("rao-blackwellized-slam-smoothing_amd")
    ekf = importlib.import_module("rao-blackwellized-slam-smoothing_amd.ekf")
    if rbpf.device_count() < 1:
        raise SystemExit("ekf_bench: no HIP device (a timing taken without one says nothing)")
    runs, Q, dt = protocol_runs(max(batches), m, N_T)
    if kw.get("trace_only"):
        for B in batches:
            device_call(ekf, runs[:B], Q, dt)
            device_call(ekf, runs[:B], Q, dt)
        return
    n = m + 9
    res = dict(m=m, n=n, N_T=N_T, protocol="examples/slam-dense-mag/main.m:37-57", keep_P=False,
               update_bytes_per_run_and_step=2 * n * n * 8)
    r0 = runs[0]
    host_args = (r0["mdl"], r0["LL"], r0["odo"], r0["y"], r0["x0"], r0["q0"], r0["P0"], Q, r0["R"], dt)
    ekf.ekf_dense(r0["mdl"], r0["LL"], r0["odo"][:7], r0["y"][:8], r0["x0"], r0["q0"], r0["P0"], Q, r0["R"], dt)     # warm-up
    ts = []
    for _ in range(host_reps):
        t0 = time.perf_counter()
        ref = ekf.ekf_dense(*host_args)
        ts.append(time.perf_counter() - t0)
    res["host_seconds_per_run"] = dict(median=float(np.median(ts)), min=min(ts), max=max(ts), reps=host_reps)
    res["device"] = []
    for B in batches:
        got = device_call(ekf, runs[:B], Q, dt)                              # warm-up of this shape
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            got = device_call(ekf, runs[:B], Q, dt)
            ts.append(time.perf_counter() - t0)
        med = float(np.median(ts))
        dist = [float(np.max(np.abs(g[0] - r)) / max(1.0, float(np.max(np.abs(r))))) for g, r in zip(got[:2], ref[:2])]
        dist.append(float(np.max(np.abs(got[2][0] - ref[2][:, :, -1])) / max(1.0, float(np.max(np.abs(ref[2][:, :, -1]))))))
        res["device"].append(dict(B=B, seconds_per_call=dict(median=med, min=min(ts), max=max(ts), reps=reps),
                                  seconds_per_run=med / B, host_over_device_per_run=res["host_seconds_per_run"]["median"] / (med / B),
                                  run0_distance_from_host_path_xf_q_Pfinal=dist))
        print(json.dumps(res["device"][-1]), flush=True)
    if kw.get("kernel_stats"):
        ks = kernel_stats(kw["kernel_stats"])
        Bt = int(kw.get("traced_B", max(batches)))
        res["kernels_traced_at_B"] = Bt
        res["kernels"] = ks
        if "ekf_update_kernel" in ks:
            byt = Bt * 2 * n * n * 8
            res["update_kernel"] = dict(bytes_per_step=byt, average_us=ks["ekf_update_kernel"]["average_us"],
                                        TB_per_s=byt / (ks["ekf_update_kernel"]["average_us"] * 1e-6) / 1e12)
    out_path = kw.get("out", os.path.join(ROOT, "profiles", "ekf_device_bench.json"))
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
