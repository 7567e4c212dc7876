#!/usr/bin/env python3
"""What localisation in the fixed landmark map of a sparseFeatures device-code model (rbpf.DeviceLandmarkMap) costs on one MI355X:
the weight kernel alone and the whole step, next to the plain torch evaluation of the same weights and to the SLAM filter step of
the same handles and shape, in one process.

The models and problems are those of tools/sparse_device_bench.py: the pinhole camera at the example's size, (n_y, nLin) =
(20, 40), and range-only beacons at the largest admitted shape, (32, 96), as torch handles (tests/sparse_models_torch.py) that draw
their normals from the device generator.  The map is mean = the problem's x0_lin, V = tril(randn) sqrt(0.02 / nLin).  Every shape
is measured with every output observed and with every second output observed (NaN in the odd columns of y).

Per shape (N_P, n_y, nLin) and mask the tool records
  kernel         rbpf_loc_landmark_weights on what measModel returns at N_P states around x0: device events around every launch,
                 ROUNDS rounds of REPS launches after a warm-up round, the median of the round medians and their spread;
                 ALTERNATING with
  torch          the observed rows of dy @ V.T, the Gram matrices, + R(ind,ind), torch.linalg.cholesky, the triangular solve and the
                 log-weight on the same device tensors, device events around every evaluation, the same rounds; and the distance
                 between the two results;
  step           LocalizationSession(DeviceLandmarkMap) driven by the handles: warm-up, then WINDOWS windows of STEPS steps, each a
                 host clock around work that ends in a synchronise (handles + weight kernel + normalisation + resampling);
  slam_step      FilterSession(DeviceSparseHandles) of the same handles, shape and y, the same windows.
From the sizes: the useful flop, N_P M nLin (nLin + 1) for Y = V H(ind,:)' on the lower triangle plus N_P nLin M (M + 1) for the Gram
matrix, the flop the issued MFMAs perform (tiles of 16, pad included), the bytes N_P (M nLin + M + 1) 8 of the observed rows, yhat
and the log-weight, each over the kernel time and against the 78.6 TF fp64 matrix peak and 8 TB/s.  No hardware counter is read.

Usage: landmark_map_bench.py [--out FILE] [--shapes N,model ...] [--rounds 3] [--reps 7] [--windows 5] [--steps 20] [--no-slam]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
rbpf = importlib.import_module("rao-blackwellized-slam-smoothing_amd")

SHAPES = [(65536, "pinhole"), (65536, "range_only_3d"), (8192, "range_only_3d")]
FP64_MATRIX_PEAK = 78.6e12
HBM_PEAK = 8.0e12


def shape_figures(N, M, n):
    nrt, nct = -(-n // 16), -(-M // 16)
    mfma = nrt * (nrt + 1) // 2 * 4 * nct + nrt * 4 * (3 if nct == 2 else 1)
    return {"useful_flop": float(N) * M * n * (n + 1) + float(N) * n * M * (M + 1), "issued_mfma_flop": float(N) * mfma * 2048.0,
            "bytes": float(N) * (M * n + M + 1) * 8.0, "mfma_per_particle": mfma}


def windows_ms(advance, sync, warmup, windows, steps):
    advance(warmup)
    sync()
    ms = []
    for _ in range(windows):
        t0 = time.perf_counter()
        advance(steps)
        sync()
        ms.append((time.perf_counter() - t0) / steps * 1e3)
    return {"ms_per_step": statistics.median(ms), "windows_ms": ms, "spread_ms": max(ms) - min(ms)}


def torch_weights(torch, yhat, dy, Vt, R, y, ind):
    N, M, n = dy.shape[0], ind.numel(), dy.shape[2]
    H = dy[:, ind, :]
    Y = (H.reshape(N * M, n) @ Vt).reshape(N, M, n)
    S = Y @ Y.transpose(1, 2) + R[ind][:, ind]
    e = y[ind] - yhat[:, ind]
    L = torch.linalg.cholesky(S)
    z = torch.linalg.solve_triangular(L, e.unsqueeze(-1), upper=False).squeeze(-1)
    return -torch.log(torch.diagonal(L, dim1=1, dim2=2)).sum(1) - 0.5 * (z * z).sum(1) - 0.5 * M * np.log(2 * np.pi)


def bench_kernel(torch, h, p, y0, N, a):
    """The kernel and the torch evaluation on the same handle outputs, in alternating rounds."""
    dev = torch.device("cuda", torch.cuda.current_device())
    f = dict(dtype=torch.float64, device=dev)
    gen = torch.Generator(device=dev).manual_seed(3)
    xn = torch.as_tensor(np.asarray(p["x0_nonLin"], dtype=np.float64), device=dev).reshape(-1, 1) + 0.01 * torch.randn((3, N), generator=gen, **f)
    xl = torch.as_tensor(p["mean"], device=dev).repeat(N, 1)
    yhat, dy = h.measModel(xn, xl)
    yhat, dy = yhat.contiguous(), dy.contiguous()
    Vt, R, y = (torch.as_tensor(np.ascontiguousarray(x), **f) for x in (np.tril(p["V"]).T, p["R"], np.nan_to_num(y0)))
    ind = torch.as_tensor(np.flatnonzero(~np.isnan(y0)), device=dev)
    yhat_host, dy_host = yhat.cpu().numpy(), dy.cpu().numpy()
    kernel, torch_ms, logw = [], [], None
    for r in range(a.rounds + 1):                                     # round 0 warms both up
        _, logw, ms = rbpf.landmark_map_weights(yhat_host, dy_host, p["V"], p["R"], y0, reps=a.reps)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
        for e0, e1 in ev:
            e0.record()
            lw = torch_weights(torch, yhat, dy, Vt, R, y, ind)
            e1.record()
        torch.cuda.synchronize()
        if r:
            kernel.append(ms)
            torch_ms.append(statistics.median(e0.elapsed_time(e1) for e0, e1 in ev))
    diff = float(np.max(np.abs(lw.cpu().numpy() - logw)) / np.max(np.abs(logw)))
    return {"kernel_ms": statistics.median(kernel), "kernel_round_medians_ms": kernel, "kernel_spread_ms": max(kernel) - min(kernel),
            "torch_ms": statistics.median(torch_ms), "torch_round_medians_ms": torch_ms, "torch_spread_ms": max(torch_ms) - min(torch_ms),
            "launches_each": a.rounds * a.reps, "logw_rel_distance_kernel_torch": diff}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "landmark_map_bench.json"))
    ap.add_argument("--shapes", nargs="*", default=None, help="N_P,model pairs (model: pinhole or range_only_3d); default: the three shapes of DESIGN.md section 4")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--no-slam", action="store_true", help="skip the SLAM filter step (recorded as not measured)")
    a = ap.parse_args()
    if a.rounds * a.reps < 20 or a.windows < 5:
        ap.error("at least 20 timed launches (rounds x reps) and 5 windows")
    if rbpf.device_count() < 1:
        raise SystemExit("landmark_map_bench: no HIP device visible (nothing is measured without one)")
    import torch
    import rbpf_oracle as oracle
    import sparse_device_bench as sdb
    import sparse_models as sm
    import sparse_models_torch as smt
    shapes = [(int(s.split(",")[0]), s.split(",")[1]) for s in a.shapes] if a.shapes else SHAPES
    T = a.warmup + a.windows * a.steps + 4
    doc = {"tool": "tools/landmark_map_bench.py", "device": torch.cuda.get_device_name(0),
           "fp64_matrix_peak_TF": FP64_MATRIX_PEAK / 1e12, "hbm_peak_TBps": HBM_PEAK / 1e12,
           "timing": f"kernel and torch: device events, a warm-up round, then {a.rounds} alternating rounds of {a.reps} launches, median of the round "
                     f"medians; steps: warm-up {a.warmup}, median of {a.windows} windows of {a.steps} steps (host clock, each window ends in a synchronise)",
           "not_measured": "hardware counters (achieved occupancy, LDS conflicts, MFMA utilisation, bytes fetched from HBM)",
           "runs": []}
    for N, name in shapes:
        p = sdb.pinhole_problem(oracle, 20, T) if name == "pinhole" else sdb.range_only_problem(sm, 32, T)
        d, n = p["model"].ny, p["model"].nLin
        p["mean"] = np.asarray(p["x0_lin"], dtype=np.float64).copy()
        p["V"] = np.tril(np.random.RandomState(7).standard_normal((n, n))) * np.sqrt(0.02 / n)
        for mask in ("all", "half"):
            q = dict(p, y=p["y"].copy())
            if mask == "half":
                q["y"][:, 1::2] = np.nan
            M = int(np.count_nonzero(~np.isnan(q["y"][0])))
            h = sdb.device_handles(torch, smt, q)
            mp = rbpf.DeviceLandmarkMap(h, q["mean"], q["V"], q["R"])
            run = dict(N_P=N, model=name, n_y=d, nLin=n, observed=M, **shape_figures(N, M, n))
            run.update(bench_kernel(torch, h, q, q["y"][0], N, a))
            t = run["kernel_ms"] * 1e-3
            run["kernel_useful_TFLOPs"] = run["useful_flop"] / t / 1e12
            run["share_of_fp64_matrix_peak_useful"] = run["useful_flop"] / t / FP64_MATRIX_PEAK
            run["share_of_fp64_matrix_peak_issued"] = run["issued_mfma_flop"] / t / FP64_MATRIX_PEAK
            run["TBps"] = run["bytes"] / t / 1e12
            run["share_of_hbm_peak"] = run["bytes"] / t / HBM_PEAK
            run["least_time_ms"] = max(run["useful_flop"] / FP64_MATRIX_PEAK, run["bytes"] / HBM_PEAK) * 1e3
            run["torch_over_kernel"] = run["torch_ms"] / run["kernel_ms"]
            with rbpf.LocalizationSession(mp, q["odometry"], q["y"], q["x0_nonLin"], q["Q"], N, q["dt"], rng=rbpf.PhiloxRNG(1)) as s:
                run["step"] = windows_ms(s.advance, s.sync, a.warmup, a.windows, a.steps)
            if a.no_slam:
                run["slam_step"] = {"ms_per_step": "not measured", "reason": "--no-slam"}
            else:
                with rbpf.FilterSession(h, *sdb.filter_args(q, N), rng=rbpf.PhiloxRNG(1)) as s:
                    run["slam_step"] = windows_ms(s.advance, s.sync, a.warmup, a.windows, a.steps)
                run["slam_step_over_step"] = run["slam_step"]["ms_per_step"] / run["step"]["ms_per_step"]
            doc["runs"].append(run)
            print(json.dumps(run), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(doc, f, indent=1)
                f.write("\n")
            del h, mp
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
