#!/usr/bin/env python3
"""What the sparseFeatures = true branch costs per step when the model is device code (rbpf.DeviceSparseHandles,
RBPF_MODEL_GENERIC_SPARSE) next to the built-in sparse-visual family, at N_P = 8192 and 65 536:

  (n_y, nLin) = (20, 40)   the pinhole camera of examples/slam-sparse-visual at the example's size, as torch handles
                           (tests/sparse_models_torch.py) AND as the built-in family, in the same run
  (n_y, nLin) = (32, 96)   range-only beacons in 3-D (tests/sparse_models.py), the largest admitted shape, as torch handles

Every output is observed at every step (the most a step can cost); the vehicle stands still up to its process noise, which the
handles draw with torch.randn; the resampling uniforms come from the device Philox generator.

Per run the tool records
  ms_per_step            handles + step + normalisation / resampling: a warm-up, then the median of WINDOWS windows of STEPS steps,
                         each window a host clock around work that ends in a synchronise
  kernel_ms              the step kernel's own time (sparse_ext_step_kernel / sparse_step_kernel): HIP events around every launch
                         of one more window (rbpf_timing_enable / rbpf_timing_read), mean over its launches
  kernel_bytes           what one launch has to move: covariance in and out, means in and out, for the device-code family also
                         the Jacobian and yhat in -- N_P (2 nLin^2 + n_y nLin + n_y + 2 nLin) 8 against N_P (2 nLin^2 + 2 nLin + 6) 8
  kernel_frac_hbm_peak   kernel_bytes / kernel_ms over the HBM peak of 8 TB/s
and at (20, 40) the ratio of the two kernels' times next to the ratio of their byte counts.
Writes one JSON document (default profiles/sparse_device_bench.json).

Usage: sparse_device_bench.py [--out FILE] [--particles N ...] [--windows 5] [--steps 20] [--warmup 8]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
rbpf = importlib.import_module("rao-blackwellized-slam-smoothing_amd")

HBM_PEAK_GBPS = 8000.0                          # MI355X: HBM3E 8 TB/s (as bench.py)


def pinhole_problem(oracle, nLand, T, seed=1):
    rs = np.random.RandomState(seed)
    model = oracle.SparseVisualModel(nLand=nLand)
    mp = np.vstack((rs.uniform(-3, 3, nLand), rs.uniform(2.5, 8, nLand)))
    x0 = np.zeros(3)
    xl = mp.T.reshape(-1)
    y = model.measModel(x0, xl)[0][None, :] + 0.01 * rs.standard_normal((T, nLand))
    return dict(model=model, odometry=np.zeros((T - 1, 3)), y=y, x0_nonLin=x0, x0_lin=xl + 0.1 * rs.standard_normal(2 * nLand),
                P0_lin=0.5 ** 2 * np.eye(2 * nLand), Q=np.diag([1e-3 ** 2, 1e-3 ** 2, 1e-4 ** 2]), R=0.1 ** 2 * np.eye(nLand), dt=1.0)


def range_only_problem(sm, L, T, seed=1):
    rs = np.random.RandomState(seed)
    model = sm.RangeOnly3DModel(L)
    xl = (rs.uniform(-8.0, 8.0, (L, 3)) + np.array([0.0, 0.0, 12.0])).reshape(-1)
    x0 = np.zeros(3)
    y = model.measModel(x0, xl)[0][None, :] + 0.05 * rs.standard_normal((T, L))
    return dict(model=model, odometry=np.zeros((T - 1, 3)), y=y, x0_nonLin=x0, x0_lin=xl + 0.1 * rs.standard_normal(3 * L),
                P0_lin=0.5 ** 2 * np.eye(3 * L), Q=np.diag([1e-3 ** 2] * 3), R=0.05 ** 2 * np.eye(L), dt=1.0)


def filter_args(p, N):
    return (p["odometry"], p["y"], p["x0_nonLin"], p["x0_lin"], p["P0_lin"], p["Q"], p["R"], N, p["dt"])


def device_handles(torch, smt, p):
    """The torch twin with its normals from the device generator instead of a replay buffer."""
    dev = torch.device("cuda", torch.cuda.current_device())
    tw = smt.twin_of(p["model"], dict(p, rng=types.SimpleNamespace(Z=np.zeros((1, 1, 1, 3)))), dev)

    def dyn(xn, dx, dt, Q):
        return xn + dx.reshape(-1, 1) + tw.Lq[0] @ torch.randn(xn.shape, dtype=torch.float64, device=xn.device)

    torch.cuda.synchronize()
    return rbpf.DeviceSparseHandles(dyn, tw._meas)


def measure(session, a):
    s = session
    s.advance(a.warmup)
    s.sync()
    ms = []
    for _ in range(a.windows):
        t0 = time.perf_counter()
        s.advance(a.steps)
        s.sync()
        ms.append((time.perf_counter() - t0) / a.steps * 1e3)
    s.timing(True)
    s.advance(a.steps)
    s.sync()
    tm = s.timing(reset=True)
    s.timing(False)
    k_ms = tm["ms"] / max(tm["launches"], 1)
    k_bytes = tm["scheduled_bytes_per_launch"]
    return {"ms_per_step": statistics.median(ms), "windows_ms": ms, "kernel_ms": k_ms, "kernel_launches_timed": tm["launches"],
            "kernel_bytes": k_bytes, "kernel_GBps": k_bytes / (k_ms * 1e-3) / 1e9 if k_ms > 0 else None,
            "kernel_frac_hbm_peak": k_bytes / (k_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS if k_ms > 0 else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_device_bench.json"))
    ap.add_argument("--particles", type=int, nargs="*", default=[8192, 65536])
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=8)
    a = ap.parse_args()
    if a.windows < 5 or a.steps < 20:
        ap.error("at least 5 windows of at least 20 steps")
    if rbpf.device_count() < 1:
        raise SystemExit("sparse_device_bench: no HIP device visible (nothing is measured without one)")
    import torch
    import rbpf_oracle as oracle
    import sparse_models as sm
    import sparse_models_torch as smt
    T = a.warmup + (a.windows + 1) * a.steps + 2
    doc = {"tool": "tools/sparse_device_bench.py", "device": torch.cuda.get_device_name(0),
           "timing": f"warm-up {a.warmup} steps, median of {a.windows} windows of {a.steps} steps (host clock, synchronised); kernel: HIP "
                     f"events around every launch of one more window of {a.steps} steps, mean",
           "hbm_peak_GBps": HBM_PEAK_GBPS, "runs": []}
    problems = (("pinhole", pinhole_problem(oracle, 20, T)), ("range_only_3d", range_only_problem(sm, 32, T)))
    for N in a.particles:
        for name, p in problems:
            m = p["model"]
            run = {"N_P": N, "model": name, "n_y": m.ny, "nLin": m.nLin}
            with rbpf.FilterSession(device_handles(torch, smt, p), *filter_args(p, N), rng=rbpf.PhiloxRNG(1)) as s:
                run["device_handles"] = measure(s, a)
            if name == "pinhole":
                with rbpf.FilterSession(rbpf.SparseVisualModel(m.nLand), *filter_args(p, N), rng=rbpf.PhiloxRNG(1)) as s:
                    run["builtin_sparse_visual"] = measure(s, a)
                dv, bi = run["device_handles"], run["builtin_sparse_visual"]
                run["kernel_time_ratio_device_over_builtin"] = dv["kernel_ms"] / bi["kernel_ms"]
                run["kernel_bytes_ratio_device_over_builtin"] = dv["kernel_bytes"] / bi["kernel_bytes"]
            doc["runs"].append(run)
            print(json.dumps(run), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(doc, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
